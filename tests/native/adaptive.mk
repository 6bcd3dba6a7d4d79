# Host check of the adaptive supersampling (tests/test_adaptive_host.py), TEST INFRASTRUCTURE ONLY: adaptive_host.cpp
# unity-includes rt_api.cpp and is built with host-side ASan + UBSan, as shutter_host beside it is (same flags;
# the device code is not instrumented), then linked with the product's kernel objects.  Run as a plain
# executable on the CPU; no device call is reached.
#   make -f adaptive.mk         -> build/adaptive_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HIPCC ?= /opt/rocm/bin/hipcc
FP := -ffp-contract=off -fno-fast-math
HSAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fsanitize=float-cast-overflow \
        -Xarch_host -fno-sanitize-recover=all
HFLAGS := -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 $(FP) -fhip-fp32-correctly-rounded-divide-sqrt \
          -fno-gpu-flush-denormals-to-zero -fno-omit-frame-pointer -Wall

all: $(OUT)adaptive_host

$(OUT)adaptive_host.o: $(HERE)adaptive_host.cpp $(CSRC)rt_api.cpp $(CSRC)rt_internal.h $(CSRC)rt_resolve.h $(ROOT)include/raytracer_hip.h
	@mkdir -p $(OUT)
	$(HIPCC) $(HFLAGS) $(HSAN) -x hip -c -o $@ $<

# the product's kernel objects (uninstrumented device code + launch stubs)
$(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o:
	$(MAKE) -s -C $(CSRC)

$(OUT)adaptive_host: $(OUT)adaptive_host.o $(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o $@ $^ -ldl -lm -pthread

.PHONY: all
