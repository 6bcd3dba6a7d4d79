# Host check of adaptive path and track launches (tests/test_path_adaptive_host.py), TEST INFRASTRUCTURE ONLY.
#   build/path_adaptive_host       path_adaptive_host.cpp: plain host C++ against the device-free header rt_internal.h
#                                  (no device code is compiled or linked), optimised
#   build/path_adaptive_host_asan  the same program under ASan + UBSan
# Both are stand-alone executables, run directly.
#   make -f path_adaptive.mk  -> both
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
PFLAGS := -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS := $(CSRC)rt_internal.h $(CSRC)rt_resolve.h $(ROOT)include/raytracer_hip.h

all: $(OUT)path_adaptive_host $(OUT)path_adaptive_host_asan

$(OUT)path_adaptive_host: $(HERE)path_adaptive_host.cpp $(HDRS) $(HERE)path_adaptive.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) -O2 $(PFLAGS) -I$(CSRC) -o $@ $<

$(OUT)path_adaptive_host_asan: $(HERE)path_adaptive_host.cpp $(HDRS) $(HERE)path_adaptive.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) -O1 $(PFLAGS) $(SAN) -I$(CSRC) -o $@ $<

.PHONY: all
