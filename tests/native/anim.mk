# Host check of scene tracks (tests/test_anim_host.py), TEST INFRASTRUCTURE ONLY.
#   build/anim_host   anim_host.cpp with rt_api.cpp's host code inside (a unity include, like the Makefile's `unity`
#                     programs), host-side ASan + UBSan (-Xarch_host: the gfx950 device code is not instrumented),
#                     linked with the product's kernel objects; run as a plain executable on contexts without
#                     devices: no device call is reached.
#   make -f anim.mk   -> build/anim_host
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
HDRS := $(wildcard $(CSRC)*.h) $(ROOT)include/raytracer_hip.h
KOBJ := $(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o

all: $(OUT)anim_host

$(KOBJ):
	$(MAKE) -s -C $(CSRC)

$(OUT)anim_host: $(HERE)anim_host.cpp $(CSRC)rt_api.cpp $(HDRS) $(KOBJ) $(HERE)anim.mk
	@mkdir -p $(OUT)
	$(HIPCC) $(HFLAGS) $(HSAN) -x hip -c -o $@.o $<
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o $@ $@.o $(KOBJ) -ldl -lm -pthread

.PHONY: all
