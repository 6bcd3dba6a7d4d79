# Host check of the plane footprints (tests/test_foot_host.py), TEST INFRASTRUCTURE ONLY: foot_host.cpp includes
# rt_foot.h (and through it rt_internal.h) and is built as host C++ with ASan + UBSan, the sanitizers dark.mk gives
# dark_host, and without FMA contraction (the binary32 restatement of the kernel's primary direction and plane test).
# Run as a plain executable on the CPU; there is no device code in it.
#   make -f foot.mk          -> build/foot_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
SAN := -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=all

all: $(OUT)foot_host

$(OUT)foot_host: $(HERE)foot_host.cpp $(CSRC)rt_foot.h $(CSRC)rt_internal.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -O1 -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall $(SAN) -I$(CSRC) -o $@ $<

.PHONY: all
