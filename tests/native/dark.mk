# Host check of the dark-tile skip's guard (tests/test_dark_host.py), TEST INFRASTRUCTURE ONLY: dark_host.cpp
# includes rt_dark.h (and through it rt_internal.h) and is built as host C++ with ASan + UBSan, the sanitizers
# variant.mk gives variant_host, and without FMA contraction (the binary32 restatement of the reference's term).
# Run as a plain executable on the CPU; there is no device code in it.
#   make -f dark.mk          -> build/dark_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
SAN := -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=all

all: $(OUT)dark_host

$(OUT)dark_host: $(HERE)dark_host.cpp $(CSRC)rt_dark.h $(CSRC)rt_internal.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -O1 -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall $(SAN) -I$(CSRC) -o $@ $<

.PHONY: all
