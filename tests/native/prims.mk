# Device harness of the arithmetic primitives (tests/test_gpu_prims.py), TEST INFRASTRUCTURE ONLY.
#   gpu/libprims_gpu.so      prims_gpu.hip: one kernel per primitive of csrc/rt_prims.h, rt_fastmath.h, rt_pow.h
#                            and rt_resolve.h, compiled with the flags of the trace kernels' translation unit --
#                            asked of csrc/Makefile (print-flags), not copied -- so it pins what the library's
#                            build makes of the same source.
#   gpu/liboracle_batch.so   oracle_batch.c + oracle/oracle.c with the oracle's flags: the per-function entry
#                            points over arrays (CPU).
#   make -f prims.mk         -> both.  PRIMS_CSRC, PRIMS_EXTRA and PRIMS_OUT build a harness from another copy of
#                            the headers, with extra flags, to another file (checks that the tests can fail).
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(HERE)../../
CSRC := $(ROOT)uu-infogr-raytracer_amd/csrc/
HIPCC ?= /opt/rocm/bin/hipcc
CC ?= gcc
PRIMS_CSRC ?= $(CSRC)
PRIMS_EXTRA ?=
PRIMS_OUT ?= $(HERE)gpu/libprims_gpu.so
LIBFLAGS := $(shell $(MAKE) -s --no-print-directory -C $(CSRC) print-flags)
ORACLE_CFLAGS := -O2 -std=c11 -fPIC -ffp-contract=off -fno-fast-math -msse2 -mfpmath=sse -fno-strict-aliasing \
                 -Wall -Wextra -Wno-unused-parameter -pthread

all: $(PRIMS_OUT) $(HERE)gpu/liboracle_batch.so

$(PRIMS_OUT): $(HERE)prims_gpu.hip $(PRIMS_CSRC)rt_prims.h $(PRIMS_CSRC)rt_fastmath.h $(PRIMS_CSRC)rt_pow.h \
              $(PRIMS_CSRC)rt_pow_tables.h $(PRIMS_CSRC)rt_resolve.h $(PRIMS_CSRC)rt_internal.h $(CSRC)Makefile \
              $(HERE)prims.mk
	@test -n "$(LIBFLAGS)" || { echo "prims.mk: csrc/Makefile print-flags gave nothing" >&2; exit 1; }
	@mkdir -p $(dir $@)
	$(HIPCC) $(LIBFLAGS) $(PRIMS_EXTRA) -I$(PRIMS_CSRC) -shared -o $@ $<

$(HERE)gpu/liboracle_batch.so: $(HERE)oracle_batch.c $(ROOT)oracle/oracle.c $(ROOT)oracle/oracle.h \
                               $(ROOT)include/raytracer_hip.h $(HERE)prims.mk
	@mkdir -p $(dir $@)
	$(CC) $(ORACLE_CFLAGS) -shared -o $@ $(HERE)oracle_batch.c $(ROOT)oracle/oracle.c -lm -pthread

.PHONY: all
