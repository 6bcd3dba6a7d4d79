# Host check of the shadow pre-test's group and union records (tests/test_shadow_group_host.py), TEST INFRASTRUCTURE ONLY.
#   build/shadow_group_host   shadow_group_host.cpp: plain host C++ against the device-free headers of csrc
#                             (rt_scene.h, rt_shadow_pre.h, rt_internal.h), one compile and link under ASan + UBSan with
#                             the flags of the Makefile's `pure` programs; no device code is compiled or linked, and the
#                             program is run as a plain executable.
#   make -f shadow_group.mk   -> build/shadow_group_host
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
OUT := $(HERE)build/
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
PFLAGS := -O1 -g -std=c++17 -fno-omit-frame-pointer -ffp-contract=off -Wall
SAN := -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all

all: $(OUT)shadow_group_host

$(OUT)shadow_group_host: $(HERE)shadow_group_host.cpp $(wildcard $(CSRC)*.h) $(ROOT)include/raytracer_hip.h $(HERE)shadow_group.mk
	@mkdir -p $(OUT)
	$(HOSTCXX) $(PFLAGS) $(SAN) -I$(CSRC) -o $@ $< -lm -pthread

.PHONY: all
