# Host check of scene-track shutters (tests/test_anim_shutter_host.py), TEST INFRASTRUCTURE ONLY.
#   build/anim_shutter_host       anim_shutter_host.cpp with rt_api.cpp's host code inside (a unity include), linked with
#                                 the product's kernel objects; contexts without devices: no device call is reached
#   build/anim_shutter_host_asan  the same program under host-side ASan + UBSan (-Xarch_host: the gfx950 device code
#                                 is not instrumented)
# Both are stand-alone executables, run directly.
#   make -f anim_shutter.mk  -> both
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HIPCC ?= /opt/rocm/bin/hipcc
FP := -ffp-contract=off -fno-fast-math
HSAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fsanitize=float-cast-overflow \
        -Xarch_host -fno-sanitize-recover=all
HFLAGS := -g -std=c++17 -fPIC --offload-arch=gfx950 $(FP) -fhip-fp32-correctly-rounded-divide-sqrt \
          -fno-gpu-flush-denormals-to-zero -fno-omit-frame-pointer -Wall
HDRS := $(wildcard $(CSRC)*.h) $(ROOT)include/raytracer_hip.h
KOBJ := $(CSRC)obj/rt_kernel.o $(CSRC)obj/rt_codec.o

all: $(OUT)anim_shutter_host $(OUT)anim_shutter_host_asan

$(KOBJ):
	$(MAKE) -s -C $(CSRC)

$(OUT)anim_shutter_host: $(HERE)anim_shutter_host.cpp $(CSRC)rt_api.cpp $(HDRS) $(KOBJ) $(HERE)anim_shutter.mk
	@mkdir -p $(OUT)
	$(HIPCC) -O2 $(HFLAGS) -x hip -c -o $@.o $<
	$(HIPCC) --offload-arch=gfx950 -o $@ $@.o $(KOBJ) -ldl -lm -pthread

$(OUT)anim_shutter_host_asan: $(HERE)anim_shutter_host.cpp $(CSRC)rt_api.cpp $(HDRS) $(KOBJ) $(HERE)anim_shutter.mk
	@mkdir -p $(OUT)
	$(HIPCC) -O1 $(HFLAGS) $(HSAN) -x hip -c -o $@.o $<
	$(HIPCC) --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o $@ $@.o $(KOBJ) -ldl -lm -pthread

.PHONY: all
