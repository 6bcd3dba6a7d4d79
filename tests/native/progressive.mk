# Host check of progressive accumulation (tests/test_progressive_host.py), TEST INFRASTRUCTURE ONLY.
#   build/progressive_host   progressive_host.cpp: plain host C++ against the device-free headers of csrc
#                            (rt_resolve.h, rt_progressive.h, rt_internal.h), one compile and link under ASan + UBSan,
#                            like the Makefile's `pure` programs; no device code is compiled or linked, and the
#                            program is run as a plain executable.
#   make -f progressive.mk   -> build/progressive_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
PFLAGS := -O1 -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all

all: $(OUT)progressive_host

$(OUT)progressive_host: $(HERE)progressive_host.cpp $(CSRC)rt_internal.h $(CSRC)rt_resolve.h $(CSRC)rt_progressive.h \
                        $(ROOT)include/raytracer_hip.h $(HERE)progressive.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) $(PFLAGS) $(SAN) -I$(CSRC) -o $@ $< -lm -pthread

.PHONY: all
