# Host check of the trace kernels' variant selection (tests/test_variant_host.py), TEST INFRASTRUCTURE ONLY:
# variant_host.cpp includes rt_internal.h alone and is built as host C++ with ASan + UBSan, the sanitizers
# path.mk gives path_host.  Run as a plain executable on the CPU; there is no device code in it.
#   make -f variant.mk          -> build/variant_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
SAN := -fsanitize=address -fsanitize=undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=all

all: $(OUT)variant_host

$(OUT)variant_host: $(HERE)variant_host.cpp $(CSRC)rt_internal.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -O1 -g -std=c++17 -fno-omit-frame-pointer -Wall $(SAN) -I$(CSRC) -o $@ $<

.PHONY: all
