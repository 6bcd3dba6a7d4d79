# Host check of supersampled path, shutter and track launches (tests/test_path_ss_host.py), TEST INFRASTRUCTURE ONLY.
#   build/path_ss_host       path_ss_host.cpp: plain host C++ against the device-free headers rt_internal.h and
#                            rt_resolve.h (no device code is compiled or linked), optimised
#   build/path_ss_host_asan  the same program under ASan + UBSan
# Both are stand-alone executables, run directly.
#   make -f path_ss.mk  -> both
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
PFLAGS := -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS := $(CSRC)rt_internal.h $(CSRC)rt_resolve.h $(ROOT)include/raytracer_hip.h

all: $(OUT)path_ss_host $(OUT)path_ss_host_asan

$(OUT)path_ss_host: $(HERE)path_ss_host.cpp $(HDRS) $(HERE)path_ss.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) -O2 $(PFLAGS) -I$(CSRC) -o $@ $<

$(OUT)path_ss_host_asan: $(HERE)path_ss_host.cpp $(HDRS) $(HERE)path_ss.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) -O1 $(PFLAGS) $(SAN) -I$(CSRC) -o $@ $<

.PHONY: all
