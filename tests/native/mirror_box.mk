# Host check of the direct kernel's mirrored screen boxes (tests/test_mirror_box_host.py), TEST INFRASTRUCTURE
# ONLY: mirror_box_host.cpp unity-includes rt_api.cpp and is built with host-side ASan + UBSan, as san_host_asan
# in the Makefile beside it is (same flags; the device code is not instrumented), then linked with the product's
# kernel objects and a sanitized oracle.c.  Run as a plain executable on the CPU; no device call is reached.
#   make -f mirror_box.mk          -> build/mirror_box_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
CC ?= gcc
HIPCC ?= /opt/rocm/bin/hipcc
FP := -ffp-contract=off -fno-fast-math
CFLAGS := -O1 -g -std=c11 $(FP) -msse2 -mfpmath=sse -fno-omit-frame-pointer -Wall -Wextra -Wno-unused-parameter -pthread
SAN := -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all
HSAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fsanitize=float-cast-overflow \
        -Xarch_host -fno-sanitize-recover=all
HFLAGS := -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 $(FP) -fhip-fp32-correctly-rounded-divide-sqrt \
          -fno-gpu-flush-denormals-to-zero -fno-omit-frame-pointer -Wall

all: $(OUT)mirror_box_host

$(OUT)mirror_box_oracle.o: $(ROOT)oracle/oracle.c $(ROOT)oracle/oracle.h
	@mkdir -p $(OUT)
	$(CC) $(CFLAGS) $(SAN) -c -o $@ $<

$(OUT)mirror_box_host.o: $(HERE)mirror_box_host.cpp $(CSRC)rt_api.cpp $(CSRC)rt_internal.h $(ROOT)include/raytracer_hip.h
	@mkdir -p $(OUT)
	$(HIPCC) $(HFLAGS) $(HSAN) -x hip -c -o $@ $<

# the product's kernel objects (uninstrumented device code + launch stubs)
$(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o:
	$(MAKE) -s -C $(CSRC)

$(OUT)mirror_box_host: $(OUT)mirror_box_host.o $(OUT)mirror_box_oracle.o $(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o $@ $^ -ldl -lm -pthread

.PHONY: all
