"""The device's arithmetic primitives, one by one, against exact references (GPU).

"Bit-exact with the reference" rests on a few per-lane operations of csrc/rt_prims.h, rt_fastmath.h, rt_pow.h and
rt_resolve.h having exactly the right rounding; the rest of the suite sees them only through 8-bit pixels.  Here
tests/native/prims_gpu.hip -- built by tests/native/prims.mk with the flags csrc/Makefile reports (print-flags) --
applies one primitive per kernel, element i on lane i % 64 of wave i / 64, and every result is compared bit for bit
(NaN equals NaN, payload ignored) with a plain reference of higher precision or with the CPU oracle's per-function
entry points (tests/native/oracle_batch.c loops over them).  No tolerance anywhere.

The CPU-side conditions (the inputs can tell a reciprocal-multiply division from a true one, a contracted dot from a
plain one, fmaxf from IEEE maximum, ocml's pow from glibc's) are asserted inside the tests: inputs that stop
separating the wrong forms fail the test.

RT_PRIMS_LIB names another build of the harness (a deliberately wrong one, to see the tests fail)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

# (signalling NaNs among the random bit patterns: numpy reports their conversions)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "uu-infogr-raytracer_amd", "csrc")
PRIMS_LIB = os.path.join(NATIVE, "gpu", "libprims_gpu.so")
BATCH_LIB = os.path.join(NATIVE, "gpu", "liboracle_batch.so")
SOURCES = [os.path.join(NATIVE, f) for f in ("prims_gpu.hip", "prims.mk", "oracle_batch.c")] + \
          [os.path.join(CSRC, f) for f in ("rt_prims.h", "rt_fastmath.h", "rt_pow.h", "rt_pow_tables.h", "rt_resolve.h",
                                           "rt_internal.h", "Makefile")] + \
          [os.path.join(ROOT, "oracle", f) for f in ("oracle.c", "oracle.h")]

F32 = np.float32
F64 = np.float64
INT_MIN = -2 ** 31
POW_GENERIC, POW_ONE, POW_HALF, POW_TWO = 0, 1, 2, 3  # rt_internal.h


# ----------------------------------------------------------------------------------------------------------------
# the harness
# ----------------------------------------------------------------------------------------------------------------
def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(s) for s in SOURCES)


class Prims:
    def __init__(self, lib):
        self.lib = lib

    def __call__(self, name, ins, outs, n, ints=()):
        """Run prims_<name>: `ins` numpy arrays (uploaded as they are), `ints` plain int arguments after them, then
        one output per (dtype, elements per item) in `outs`; returns the outputs as numpy arrays."""
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0") for a in ins]
        res = [torch.zeros(max(1, n * per * np.dtype(dt).itemsize), dtype=torch.uint8, device="cuda:0")
               for dt, per in outs]
        for a, t in zip(ins, dev):
            assert t.numel() == a.nbytes
        args = [C.c_void_p(t.data_ptr()) for t in dev] + [C.c_int(v) for v in ints] + \
               [C.c_void_p(t.data_ptr()) for t in res]
        fn = getattr(self.lib, "prims_" + name)
        fn.restype = C.c_int
        rc = fn(*args, C.c_longlong(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, f"prims_{name}: hipError {rc}"
        torch.cuda.synchronize()
        out = [t.cpu().numpy()[:n * per * np.dtype(dt).itemsize].view(dt) for t, (dt, per) in zip(res, outs)]
        del dev
        return out if len(out) > 1 else out[0]


@pytest.fixture(scope="module")
def prims():
    """The harness library, built like build() builds it when it is missing or older than its sources; a build that
    does not work fails the tests (never a skip)."""
    path = os.environ.get("RT_PRIMS_LIB") or PRIMS_LIB
    if (path == PRIMS_LIB and _stale(PRIMS_LIB)) or _stale(BATCH_LIB):
        r = subprocess.run(["make", "-s", "-f", "prims.mk", "-C", NATIVE], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            pytest.fail("tests/native/prims.mk failed:\n" + (r.stdout + r.stderr)[-4000:])
    if not os.path.exists(path):
        pytest.fail(f"no harness library at {path}")
    import torch
    torch.cuda.set_device(0)
    return Prims(C.CDLL(path))


@pytest.fixture(scope="module")
def batch(prims):
    return C.CDLL(BATCH_LIB)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def libm_pow(batch, x, y):
    x = np.ascontiguousarray(x, dtype=F64)
    y = np.ascontiguousarray(np.broadcast_to(np.asarray(y, dtype=F64), x.shape))
    out = np.empty_like(x)
    batch.libm_batch_pow(_ptr(x), _ptr(y), _ptr(out), C.c_long(x.size))
    # the loop really is the host libm's pow: the same bits as calling it through ctypes
    m = C.CDLL("libm.so.6")
    m.pow.restype = C.c_double
    m.pow.argtypes = [C.c_double, C.c_double]
    for i in np.linspace(0, x.size - 1, 200).astype(int):
        assert _same_bits(np.array([m.pow(x.flat[i], y.flat[i])]), out.reshape(-1)[i:i + 1]).all()
    return out


# ----------------------------------------------------------------------------------------------------------------
# comparison and input sets
# ----------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind != "f":
        return a == b
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got, want, what, *inputs):
    ok = _same_bits(got, want)
    if not ok.all():
        bad = np.flatnonzero(~ok.reshape(len(ok), -1).all(axis=1) if ok.ndim > 1 else ~ok)
        lines = []
        for i in bad[:8]:
            ins = ", ".join(_show(x[i]) for x in inputs)
            lines.append(f"  [{i}] ({ins}): got {_show(got[i])}, want {_show(want[i])}")
        pytest.fail(f"{what}: {bad.size} of {len(ok)} differ\n" + "\n".join(lines))


def _show(v):
    v = np.asarray(v)
    if v.ndim:
        return "(" + ", ".join(_show(x) for x in v) + ")"
    if v.dtype.kind == "f":
        return f"{float(v).hex()}"
    return hex(int(v))


def f32_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(F32)


def r32(x):
    """One rounding of a float64 value to binary32, kept in float64 for the next exact step."""
    return np.asarray(x, dtype=F64).astype(F32).astype(F64)


def fm_bounds():
    """FM_*_LO / HI of rt_fastmath.h, read from the header."""
    text = open(os.path.join(CSRC, "rt_fastmath.h")).read()
    vals = {k: float.fromhex(v) for k, v in re.findall(r"(FM_\w+_(?:LO|HI)) = (0x1p-?\d+)f", text)}
    assert sorted(vals) == ["FM_DIV_HI", "FM_DIV_LO", "FM_RCP_HI", "FM_RCP_LO", "FM_SQRT_HI", "FM_SQRT_LO"], vals
    return vals


MANTISSAS = (0, 1, 0x7fffff, 0x7ffffe, 0x400000, 0x3fffff, 0x555555, 0x2aaaaa)
N_RANDOM = 1 << 18


def edge_set(signed=True, seed=1):
    """The edge set, as bit patterns -> float32: every biased exponent 0..255 x 8 mantissas (2,048: holds +0, +inf,
    NaNs, the smallest and largest subnormal, FLT_MAX), +-0, +-inf, NaN, both subnormal ends and FLT_MAX by name (9),
    each FM_* domain bound of rt_fastmath.h with its two neighbours (18), and 2^18 seeded random bit patterns.  Signed:
    the named part also with the sign bit set (2 x 2,075 + 2^18 = 266,294); unsigned: random patterns with the sign
    cleared (2,075 + 2^18 = 264,219)."""
    exps = (np.arange(256, dtype=np.uint32) << 23)[:, None] | np.array(MANTISSAS, dtype=np.uint32)[None, :]
    named = np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 1, 0x007fffff, 0x7f7fffff, 0x3f800000],
                     dtype=np.uint32)
    bounds = np.array([v for x in fm_bounds().values() for v in (F32(x).view(np.uint32) + np.array([-1, 0, 1]))],
                      dtype=np.uint32)
    fixed = np.concatenate([exps.ravel(), named, bounds])
    rnd = np.random.default_rng(seed).integers(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    if signed:
        bits = np.concatenate([fixed, fixed ^ np.uint32(0x80000000), rnd])
    else:
        bits = np.concatenate([fixed & np.uint32(0x7fffffff), rnd & np.uint32(0x7fffffff)])
    return bits.view(F32).copy()


SPECIALS = f32_bits([0, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000, 1, 0x80000001,
                     0x007fffff, 0x807fffff, 0x7f7fffff, 0xff7fffff])  # +-0 +-1 +-inf NaN +-subnormals +-FLT_MAX


def test_edge_set_counts():
    """The sets named in the docstrings have the sizes they state (CPU arithmetic only)."""
    assert edge_set(True).size == 2 * 2075 + N_RANDOM == 266294
    assert edge_set(False).size == 2075 + N_RANDOM == 264219
    e = edge_set(True).view(np.uint32)
    for b in (0, 0x80000000, 0x7f800000, 0xff800000, 1, 0x007fffff, 0x7f7fffff):
        assert (e == b).any()
    assert np.isnan(edge_set(True)).any() and SPECIALS.size == 13


# ----------------------------------------------------------------------------------------------------------------
# a. correct rounding
# ----------------------------------------------------------------------------------------------------------------
def ref_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(x.astype(F64)).astype(F32)


def ref_rcp(x):
    with np.errstate(all="ignore"):
        return (1.0 / x.astype(F64)).astype(F32)


def ref_div(a, b):
    with np.errstate(all="ignore"):
        return (a.astype(F64) / b.astype(F64)).astype(F32)


def ref_inv_len(x):
    return ref_rcp(ref_sqrt(x))


def test_float64_reference_is_the_correctly_rounded_binary32_operation():
    """The reference of a: the operation in float64 rounded once to float32 (53 >= 2 * 24 + 2 bits: the double
    rounding cannot change the result).  On 2^18 inputs it equals numpy's own float32 '/' and sqrt everywhere."""
    rng = np.random.default_rng(7)
    a = rng.uniform(0.1, 10, N_RANDOM).astype(F32)
    b = rng.uniform(0.1, 10, N_RANDOM).astype(F32)
    assert _same_bits(ref_div(a, b), a / b).all() and _same_bits(ref_sqrt(a), np.sqrt(a)).all()
    e = edge_set(False)
    with np.errstate(all="ignore"):
        assert _same_bits(ref_sqrt(e), np.sqrt(e)).all() and _same_bits(ref_rcp(e), F32(1) / e).all()


@pytest.mark.parametrize("name,ref", [("cr_sqrt", ref_sqrt), ("sqrt_cr", ref_sqrt), ("cr_rcp", ref_rcp),
                                      ("rcp_cr", ref_rcp), ("cr_inv_len", ref_inv_len)])
def test_unary_correct_rounding(prims, name, ref):
    """cr_sqrt, sqrt_cr, cr_rcp, rcp_cr, cr_inv_len on the signed edge set (266,294 inputs, subnormal inputs and
    results among them: a build that flushes denormals fails).  Reference: the operation in numpy float64 rounded
    once to float32; cr_inv_len is two such steps (sqrt, then reciprocal), as Vector3.Normalize does it."""
    x = edge_set(True)
    assert_bits(prims(name, [x], [(F32, 1)], x.size), ref(x), name, x)


def division_inputs():
    e = edge_set(True)
    rng = np.random.default_rng(11)
    ua = rng.uniform(0.1, 10, N_RANDOM).astype(F32)
    ub = rng.uniform(0.1, 10, N_RANDOM).astype(F32)
    sa, sb = [g.ravel() for g in np.meshgrid(SPECIALS, SPECIALS, indexing="ij")]
    return (np.concatenate([e, ua, sa]), np.concatenate([rng.permutation(e), ub, sb])), (ua, ub)


@pytest.mark.parametrize("name", ["div", "div_cr"])
def test_division_correct_rounding(prims, name):
    """'a / b' as the library's flags compile it, and div_cr: the signed edge set against a seeded shuffle of itself
    (266,294 pairs), 2^18 pairs from uniform(0.1, 10) and every pair of 13 special values (169).  Reference: the
    float64 quotient rounded once.  Condition: on the uniform pairs at least 15 % of the correctly rounded quotients
    differ from fl(a * fl(1 / b)) (25.7 % measured), or the inputs could not tell a reciprocal multiply from a
    division."""
    (a, b), (ua, ub) = division_inputs()
    share = float(np.mean(~_same_bits(ref_div(ua, ub), ua * (F32(1) / ub))))
    print(f"quotients that differ from a * (1 / b): {share:.3%}")
    assert share >= 0.15, share
    assert_bits(prims(name, [a, b], [(F32, 1)], a.size), ref_div(a, b), name, a, b)


# ----------------------------------------------------------------------------------------------------------------
# b. no contraction
# ----------------------------------------------------------------------------------------------------------------
def ref_dot(a, b):
    """((x*x') + (y*y')) + (z*z') with a float32 rounding after every operation (float64 holds each product of two
    floats exactly, and a once-rounded float64 sum of two floats rounds to the correctly rounded float32 sum)."""
    a, b = a.astype(F64), b.astype(F64)
    with np.errstate(all="ignore"):
        return r32(r32(r32(a[:, 0] * b[:, 0]) + r32(a[:, 1] * b[:, 1])) + r32(a[:, 2] * b[:, 2])).astype(F32)


def fused_dot(a, b):
    """dot with its last two products fused into their additions: fma(z, z', fma(y, y', x*x'))."""
    a, b = a.astype(F64), b.astype(F64)
    with np.errstate(all="ignore"):
        return r32(r32(r32(a[:, 0] * b[:, 0]) + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F32)


def vector_inputs(k, seed):
    """k arrays of n x 3 floats: 2^18 seeded uniform(-1, 1) vectors, then the signed edge set under k x 3 seeded
    shuffles (266,294 vectors)."""
    rng = np.random.default_rng(seed)
    e = edge_set(True)
    out = []
    for _ in range(k):
        u = rng.uniform(-1, 1, (N_RANDOM, 3)).astype(F32)
        out.append(np.concatenate([u, np.stack([rng.permutation(e) for _ in range(3)], axis=1)]))
    return out


def test_dot_has_no_contraction(prims):
    """dot(a, b).  Reference: float64 with an explicit round to float32 after every single operation.  Inputs: 2^18
    uniform(-1, 1) vector pairs and 266,294 pairs from the edge set.  Condition: at least 20 % of the uniform pairs
    give a different float when the last two products are fused into their additions (35.4 % measured)."""
    a, b = vector_inputs(2, 21)
    share = float(np.mean(~_same_bits(ref_dot(a[:N_RANDOM], b[:N_RANDOM]), fused_dot(a[:N_RANDOM], b[:N_RANDOM]))))
    print(f"dots that differ when contracted: {share:.3%}")
    assert share >= 0.20, share
    assert_bits(prims("dot", [a, b], [(F32, 1)], len(a)), ref_dot(a, b), "dot", a, b)


def test_normalize_has_no_contraction(prims):
    """normalize(a) = a * cr_inv_len(dot(a, a)).  Reference: ref_dot, the two correctly rounded steps of
    cr_inv_len, and one rounded product per component.  Inputs as for dot (one vector each: 528,438)."""
    a, = vector_inputs(1, 22)
    s = ref_inv_len(ref_dot(a, a)).astype(F64)
    with np.errstate(all="ignore"):
        want = (a.astype(F64) * s[:, None]).astype(F32)
    got = prims("normalize", [a], [(F32, 3)], len(a)).reshape(-1, 3)
    assert_bits(got, want, "normalize", a)


def test_sub_then_dot_has_no_contraction(prims):
    """dot(sub(a, b), c), the shape of sphere_t's b and c terms.  Reference: one rounded difference per component,
    then ref_dot.  Inputs as for dot (528,438 triples)."""
    a, b, c = vector_inputs(3, 23)
    with np.errstate(all="ignore"):
        d = (a.astype(F64) - b.astype(F64)).astype(F32)
    assert_bits(prims("sub_dot", [a, b, c], [(F32, 1)], len(a)), ref_dot(d, c), "sub_dot", a, b, c)


def test_discriminant_has_no_contraction(prims):
    """b*b - a4*c in the form sphere_t writes it, compiled with the library's flags.  Reference: both products and the
    difference each rounded to float32.  Inputs: 2^18 uniform(-1, 1) triples and 266,294 from the edge set.
    Condition: the share of uniform triples whose float changes when either product is fused into the subtraction is
    at least half of the 24.4 % (fma(-a4, c, b*b)) and 25.4 % (fma(b, b, -(a4*c))) measured on the CPU."""
    rng = np.random.default_rng(24)
    e = edge_set(True)
    b, a4, c = [np.concatenate([rng.uniform(-1, 1, N_RANDOM).astype(F32), rng.permutation(e)]) for _ in range(3)]
    b6, a6, c6 = b.astype(F64), a4.astype(F64), c.astype(F64)
    with np.errstate(all="ignore"):
        want = r32(r32(b6 * b6) - r32(a6 * c6)).astype(F32)
        fused1 = r32(r32(b6 * b6) - a6 * c6).astype(F32)
        fused2 = r32(b6 * b6 - r32(a6 * c6)).astype(F32)
    s1 = float(np.mean(~_same_bits(want[:N_RANDOM], fused1[:N_RANDOM])))
    s2 = float(np.mean(~_same_bits(want[:N_RANDOM], fused2[:N_RANDOM])))
    print(f"discriminants that differ when contracted: {s1:.3%} / {s2:.3%}")
    assert s1 >= 0.244 / 2 and s2 >= 0.254 / 2, (s1, s2)
    assert_bits(prims("disc", [b, a4, c], [(F32, 1)], b.size), want, "disc", b, a4, c)


# ----------------------------------------------------------------------------------------------------------------
# c. IEEE 754-2019 maximum / minimum
# ----------------------------------------------------------------------------------------------------------------
def ieee_maximum(a, b):
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return 0.0 if math.copysign(1.0, a) > 0 or math.copysign(1.0, b) > 0 else -0.0
    return a if a > b else b


def ieee_minimum(a, b):
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return -0.0 if math.copysign(1.0, a) < 0 or math.copysign(1.0, b) < 0 else 0.0
    return a if a < b else b


def test_nmax0_nmin_are_ieee_maximum_minimum(prims):
    """nmax0(a) = maximum(a, +0) and nmin(a, b) = minimum(a, b) of IEEE 754-2019, written out in Python: NaN
    propagates from either side and -0 < +0.  Inputs: the cross product of 13 values {+-0, +-1, +-inf, NaN, both
    +-subnormal ends, +-FLT_MAX} (169 pairs; nmax0: the 13) plus 2^16 random bit patterns / pairs.  The expected
    table holds the cases where fmaxf / fminf answer differently -- NaN against a number (they return the number)
    and -0 against +0 in both orders (they may return either) -- which is asserted."""
    rng = np.random.default_rng(31)
    ra, rb = [rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(F32) for _ in range(2)]
    sa, sb = [g.ravel() for g in np.meshgrid(SPECIALS, SPECIALS, indexing="ij")]
    a, b = np.concatenate([sa, ra]), np.concatenate([sb, rb])
    want_min = np.array([ieee_minimum(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=F64).astype(F32)
    m = np.concatenate([SPECIALS, ra])
    want_max0 = np.array([ieee_maximum(x, 0.0) for x in m.tolist()], dtype=F64).astype(F32)
    # where fminf / fmaxf would differ
    nan_num = (np.isnan(a) ^ np.isnan(b))
    assert nan_num[:169].sum() == 24 and np.isnan(want_min[nan_num]).all()
    zeros = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    assert zeros[:169].sum() == 2 and np.signbit(want_min[zeros]).all()
    assert np.isnan(want_max0[np.isnan(m)]).all() and np.isnan(m[:13]).sum() == 1
    neg0 = m.view(np.uint32) == 0x80000000
    assert neg0[:13].sum() == 1 and (want_max0[neg0].view(np.uint32) == 0).all()
    assert_bits(prims("nmin", [a, b], [(F32, 1)], a.size), want_min, "nmin", a, b)
    assert_bits(prims("nmax0", [m], [(F32, 1)], m.size), want_max0, "nmax0", m)


# ----------------------------------------------------------------------------------------------------------------
# d. (int)float   e. ShiftColor   f. the checkerboard
# ----------------------------------------------------------------------------------------------------------------
def net_f2i(x):
    """.NET's (int)float in Python integers: NaN or a value outside [-2^31, 2^31) -> int.MinValue, else truncation
    toward zero."""
    return np.array([INT_MIN if (v != v or not (-2 ** 31 <= v < 2 ** 31)) else int(v)
                     for v in np.asarray(x, dtype=F64).tolist()], dtype=np.int64)


def oracle_f2i(batch, x):
    out = np.empty(x.size, dtype=np.int32)
    batch.oracle_batch_net_float_to_int(_ptr(x), _ptr(out), C.c_long(x.size))
    return out


def f2i_inputs():
    near = []
    for v in (2.0 ** 31, 2.0 ** 24, 1.0, 0.5, 0.99999994, 2.0 ** 23, 1e9):
        b = int(F32(v).view(np.uint32))
        near += [b - 2, b - 1, b, b + 1, b + 2]
    near = np.array(near, dtype=np.uint32)
    sub = np.array([1, 2, 0x7fffff, 0x400000], dtype=np.uint32)
    fixed = np.concatenate([near, sub])
    return np.concatenate([f32_bits(fixed), f32_bits(fixed | np.uint32(0x80000000)), edge_set(True)])


def test_net_f2i(prims, batch):
    """net_f2i.  Reference: Python integer arithmetic (NaN or outside [-2^31, 2^31) -> INT_MIN, else truncation),
    which must agree with oracle_net_float_to_int on the same inputs.  Inputs: +-2^31, +-2^24, +-2^23, +-1, +-0.5,
    +-0.99999994 and +-1e9 each with two float neighbours on either side, subnormals (78 values), and the signed
    edge set (266,294)."""
    x = f2i_inputs()
    assert x.size == 78 + 266294
    want = net_f2i(x).astype(np.int32)
    assert (oracle_f2i(batch, x) == want).all()
    assert (want == INT_MIN).sum() > 1000 and (want[:78] == np.int32(2 ** 31 - 128)).any()
    assert_bits(prims("net_f2i", [x], [(np.int32, 1)], x.size), want, "net_f2i", x)


def ref_shift_channel(x):
    """ShiftColor's channel, the C# line by line in numpy binary32: Math.Clamp(c, 0, 1) (NaN passes), * 255f rounded
    to float32, Math.Floor, (int) as net_f2i, (byte)."""
    with np.errstate(all="ignore"):
        cl = np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)
        m = (cl * F32(255)).astype(F32)
        fl = np.floor(m)
    return (net_f2i(fl) & 0xff).astype(np.uint32)


def shift_inputs():
    vals = []
    for k in range(256):
        o = int(F32(k / 255).view(np.uint32)) + np.arange(-64, 65, dtype=np.int64)  # ordinals around fl(k / 255)
        vals.append(np.where(o >= 0, o, 0x80000000 - o).astype(np.uint32))
    extra = f32_bits([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0x80000000, 0xbf800000, 0xbf000000, 0xc2c80000,
                      0x3f800001, 0x40000000, 0x437f0000, 0x43800000, 0x4f000000, 0x7f7fffff, 0xff7fffff, 1, 0x007fffff,
                      0x80000001, 0x807fffff])
    return np.concatenate([np.concatenate(vals).view(F32), extra])


def test_shift_channel(prims, batch):
    """shift_channel.  Reference: ref_shift_channel (numpy binary32, line by line), cross-checked against
    oracle_shift_color.  Inputs: for every k in 0..255 every float within +-64 ulp of fl(k / 255) (33,024 values:
    where the floor flips), and NaN of both signs, +-inf, -0, negatives, values above 1, FLT_MAX and subnormals
    (19)."""
    x = shift_inputs()
    assert x.size == 33024 + 19
    want = ref_shift_channel(x)
    orc = np.empty(x.size, dtype=np.int32)
    batch.oracle_batch_shift_channel(_ptr(x), _ptr(orc), C.c_long(x.size))
    assert (orc.astype(np.uint32) == want).all()
    assert len(np.unique(want)) == 256
    assert_bits(prims("shift_channel", [x], [(np.uint32, 1)], x.size), want, "shift_channel", x)


def test_checker_tile(prims):
    """checker_tile(u, v).  Reference: net_f2i twice, a wrapping 32-bit add, & 1, as a float.  Inputs: pairs around
    the integers -4..4 of both signs (+-1 ulp: 729), (2^31, 2^31), (NaN, x) and (x, NaN), where INT_MIN + INT_MIN
    and INT_MIN + x wrap, (-0.5, 0.5) and its mirror, (2^31 - 128, 1) (12 named pairs), 2^16 random pairs in
    +-1e9 (floats that large are even integers: they exercise the conversion's range, not the parity) and 2^16 in
    +-2^20, where both parities and fractions occur."""
    around = []
    for k in range(-4, 5):
        b = F32(k)
        around += [np.nextafter(b, F32(-np.inf)), b, np.nextafter(b, F32(np.inf))]
    around = np.array(around, dtype=F32)
    gu, gv = [g.ravel() for g in np.meshgrid(around, around, indexing="ij")]
    nan, big = F32(np.nan), F32(2.0 ** 31)
    named = np.array([(big, big), (nan, F32(1)), (nan, F32(2)), (F32(1), nan), (nan, nan), (-big, -big), (big, F32(1)),
                      (F32(-0.5), F32(0.5)), (F32(0.5), F32(-0.5)), (F32(2 ** 31 - 128), F32(1)), (F32(-0.0), F32(1)),
                      (F32(np.inf), F32(-np.inf))], dtype=F32)
    rng = np.random.default_rng(41)
    h = 1 << 16
    u = np.concatenate([gu, named[:, 0], rng.uniform(-1e9, 1e9, h).astype(F32), rng.uniform(-2 ** 20, 2 ** 20, h).astype(F32)])
    v = np.concatenate([gv, named[:, 1], rng.uniform(-1e9, 1e9, h).astype(F32), rng.uniform(-2 ** 20, 2 ** 20, h).astype(F32)])
    assert u.size == 729 + 12 + 2 * h
    want = (((net_f2i(u) + net_f2i(v)) & 0xffffffff) & 1).astype(F32)
    assert want[729] == 0 and want[730] == 1 and want[731] == 0  # INT_MIN + INT_MIN wraps to 0; INT_MIN + 1 is odd
    assert 0.4 < want[-h:].mean() < 0.6
    assert_bits(prims("checker_tile", [u, v], [(F32, 1)], u.size), want, "checker_tile", u, v)


# ----------------------------------------------------------------------------------------------------------------
# g. attenuation
# ----------------------------------------------------------------------------------------------------------------
def positive_inputs():
    rng = np.random.default_rng(51)
    e = edge_set(False)
    e = e[~np.isnan(e)]
    return np.concatenate([e, rng.integers(0, 0x7f800000, N_RANDOM, dtype=np.uint64).astype(np.uint32).view(F32)])


def test_plane_att(prims, batch):
    """plane_att(t).  Reference: (float)(1.0 / pow((double)t, 2.0)) with the host libm's pow, the function the oracle
    calls.  Inputs: the positive edge set without NaN (zero, subnormal t and FLT_MAX among them) and 2^18 random
    positive floats."""
    t = positive_inputs()
    with np.errstate(all="ignore"):
        want = (1.0 / libm_pow(batch, t.astype(F64), 2.0)).astype(F32)
    assert np.isinf(want).any() and (want == 0).any()
    assert_bits(prims("plane_att", [t], [(F32, 1)], t.size), want, "plane_att", t)


def test_sphere_att(prims):
    """sphere_att(t) = (1 / t) * t.  Reference: the correctly rounded reciprocal (a), then one rounded product.
    Inputs as for plane_att."""
    t = positive_inputs()
    with np.errstate(all="ignore"):
        want = (ref_rcp(t).astype(F64) * t.astype(F64)).astype(F32)
    assert np.isnan(want).any() and (want != 1).sum() > 1000
    assert_bits(prims("sphere_att", [t], [(F32, 1)], t.size), want, "sphere_att", t)


# ----------------------------------------------------------------------------------------------------------------
# h. Math.Pow
# ----------------------------------------------------------------------------------------------------------------
POW_X_MAX = 0x3f800010
# profiles/r06_pow_check.txt: the two inputs at which ocml's pow rounds to a different float than glibc's
OCML_DIFFERS = [(0x3dd7cf12, float.fromhex("0x1.946b02p+4")), (0x3ed34fde, float.fromhex("0x1.273c82p+2"))]


def pow_x():
    rng = np.random.default_rng(61)
    bits = np.concatenate([np.arange(0, POW_X_MAX + 1, 1 << 12, dtype=np.int64),
                           np.arange(POW_X_MAX - 4095, POW_X_MAX + 1, dtype=np.int64),
                           rng.integers(0, POW_X_MAX + 1, 1 << 14, dtype=np.int64),
                           np.array([b for b, _ in OCML_DIFFERS], dtype=np.int64)])
    return np.unique(bits).astype(np.uint32).view(F32)


def pow_cases():
    from test_gpu_parity import POW_EXPONENTS
    cases = [(float(F32(e)), POW_GENERIC) for e in POW_EXPONENTS]
    for e, kind in ((0.5, POW_HALF), (1.0, POW_ONE), (2.0, POW_TWO)):
        cases += [(e, kind), (e, POW_GENERIC)]
    return cases


def test_pow_inputs_hold_the_ocml_mismatches():
    """Both (x, n) of profiles/r06_pow_check.txt at which the device's own pow rounds differently are in the set."""
    x = pow_x().view(np.uint32)
    exps = [e for e, _ in pow_cases()]
    text = open(os.path.join(ROOT, "profiles", "r06_pow_check.txt")).read()
    for b, n in OCML_DIFFERS:
        assert (x == b).any() and n in exps
        assert f"({b:#010x}), n = {float(F32(n)).hex().replace('0000000p', 'p')}" in text, (hex(b), n)


@pytest.mark.parametrize("case", range(21))
def test_spec_pow_and_glibc_pow(prims, batch, case):
    """glibc_pow((double)x, (double)n) and spec_pow<true>(x, kind, n) on the device.  Reference: the host libm's pow,
    the double bit for bit and its float rounding.  Cases: the 15 POW_EXPONENTS of tests/test_gpu_parity.py as
    POW_GENERIC, and 0.5, 1 and 2 each with its fast kind and as POW_GENERIC (the fast path's float must be the
    generic one's).  x: bit patterns 0 .. 0x3f800010 in steps of 2^12, each of the last 4,096, 2^14 seeded random
    patterns in that range and the two inputs where ocml's pow differs (about 280,500 distinct values)."""
    cases = pow_cases()
    assert len(cases) == 21
    e, kind = cases[case]
    x = pow_x()
    assert 280000 < x.size < 281000 and all((x.view(np.uint32) == b).any() for b, _ in OCML_DIFFERS)
    want_d = libm_pow(batch, x.astype(F64), e)
    with np.errstate(all="ignore"):
        want_f = want_d.astype(F32)
    got_d, got_f = prims("spec_pow", [x, np.full(x.size, kind, np.uint32), np.full(x.size, e, F32)],
                         [(F64, 1), (F32, 1)], x.size)
    assert_bits(got_d, want_d, f"glibc_pow(x, {e})", x)
    assert_bits(got_f, want_f, f"spec_pow(x, kind {kind}, {e})", x)


def pow_double_inputs():
    mx, tiny = np.finfo(F64).max, 5e-324
    g = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, tiny, -tiny, 2.2250738585072009e-308,
                  -2.2250738585072009e-308, 2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 1.5, -1.5, 2.0 ** -70, -2.0 ** -70,
                  2.0 ** 64, -2.0 ** 64, 2.0 ** 53 - 1, -(2.0 ** 53 - 1), 2.0 ** 52 + 1, 1e300, 1e-300, 1024.0, -1074.0,
                  1075.0, 1 + 2.0 ** -52, 1 - 2.0 ** -53, mx, -mx, 0.9999, 1.0001, 1e5, -1e5, 709.5, -745.2], dtype=F64)
    gx, gy = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    rng = np.random.default_rng(62)
    h = 1 << 15
    rx = rng.integers(0, 1 << 64, h, dtype=np.uint64).view(F64)
    ry = rng.integers(0, 1 << 64, h, dtype=np.uint64).view(F64)
    mx_ = rng.uniform(0.05, 20, h) * np.where(rng.random(h) < 0.2, -1, 1)
    my = np.where(rng.random(h) < 0.5, rng.uniform(-1100, 1100, h), np.round(rng.uniform(-400, 400, h)))
    return np.concatenate([gx, rx, mx_]), np.concatenate([gy, ry, my]), g.size


def test_glibc_pow_whole_double_range(prims, batch):
    """glibc_pow(x, y) over the double range.  Reference: the host libm's pow, bit for bit.  Inputs: a grid of 41
    special values crossed with itself (1,681: +-0, +-1, +-inf, NaN, subnormals, negative x with odd, even and
    non-integer y, |y| below 2^-65 and above 2^63, overflow and underflow) plus 2^16 random (x, y): half random bit
    patterns, half x in +-[0.05, 20] with y in +-1100 or an integer in +-400."""
    x, y, g = pow_double_inputs()
    assert g == 41 and x.size == 41 * 41 + (1 << 16)
    want = libm_pow(batch, x, y)
    assert np.isinf(want).any() and (want == 0).any() and np.isnan(want).any() and (want < 0).any()
    sub = np.abs(want[np.isfinite(want) & (want != 0)]) < 2.2250738585072014e-308
    assert sub.any()
    assert_bits(prims("glibc_pow", [x, y], [(F64, 1)], x.size), want, "glibc_pow", x, y)


# ----------------------------------------------------------------------------------------------------------------
# i. root selection with mixed waves
# ----------------------------------------------------------------------------------------------------------------
N_RAYS = 1 << 16
N_SPHERES = 16


def f32dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def perp(v, rng):
    w = np.cross(v, rng.normal(size=v.shape))
    return unit(w)


@pytest.fixture(scope="module")
def rays():
    """2^16 rays (origin o, direction d) x 16 spheres = 2^20 (ray, sphere) elements, element = ray * 16 + sphere.
    Every ray is aimed at one target sphere by a category (and meets the 15 others as it may):
      0 hits          1 misses              2 tangent (aimed at the rim in float64, rounded: disc lands within a
      few ulp of 0 on both sides)           3 origin inside the sphere     4 origin on the sphere
      5 sphere behind the ray               6 b = +0 (oc perpendicular to d, exact zeros)
      7 unnormalised direction, length up to 30 (a light's position)
      8 distance 0.001 |d| to the surface (the shadow epsilon's edge), unnormalised
      9 zero direction (b = -0 for some)   10 direction with a2 = +inf     11 NaN direction component
    Categories 9-11 have no finite positive 2a: only the <false> forms take them."""
    rng = np.random.default_rng(71)
    centers = rng.uniform(-6, 6, (N_SPHERES, 3)).astype(F32)
    radii = np.concatenate([rng.uniform(0.3, 2.0, N_SPHERES - 3), [0.01, 5.0, 1.0]]).astype(F32)
    cat = np.concatenate([np.repeat(np.arange(9), N_RAYS // 9 - 40), np.repeat([9, 10, 11], 120)])
    cat = np.concatenate([cat, np.zeros(N_RAYS - cat.size, dtype=cat.dtype)])
    tgt = rng.integers(0, N_SPHERES, N_RAYS)
    c, r = centers[tgt].astype(F64), radii[tgt].astype(F64)[:, None]
    u = unit(rng.normal(size=(N_RAYS, 3)))  # direction of travel
    w = perp(u, rng)
    dist = rng.uniform(0.5, 12, (N_RAYS, 1))
    length = np.where(np.isin(cat, (7, 8)), rng.uniform(0.05, 30, N_RAYS), 1.0)[:, None]
    off = np.select([cat == 0, cat == 1, cat == 2], [rng.uniform(0, 0.95, N_RAYS), rng.uniform(1.05, 4, N_RAYS), 1.0],
                    default=rng.uniform(0, 1.5, N_RAYS))[:, None]
    o = c - u * (r + dist) + w * r * off
    # tangent: aim from o at the rim point, so that the exact discriminant is 0
    rim_dir = unit(np.where((cat == 2)[:, None], _tangent_dir(o, c, r, w), u))
    d = rim_dir * length
    o = np.where((cat == 3)[:, None], c + u * r * rng.uniform(0, 0.9, (N_RAYS, 1)), o)
    o = np.where((cat == 4)[:, None], c - u * r, o)
    d = np.where((cat == 5)[:, None], -d, d)
    o = np.where((cat == 8)[:, None], c - u * r - d * 0.001 * (1 + rng.uniform(-3e-5, 3e-5, (N_RAYS, 1))), o)
    o, d = o.astype(F32), d.astype(F32)
    # b = +0: oc along one axis, d along another (exact zeros in every product)
    k = np.flatnonzero(cat == 6)
    ax = rng.integers(0, 3, k.size)
    oc = np.zeros((k.size, 3), F32)
    oc[np.arange(k.size), ax] = (radii[tgt[k]] * rng.uniform(0.2, 1.8, k.size) * rng.choice([-1, 1], k.size)).astype(F32)
    o[k] = centers[tgt[k]] + oc  # (the sum is rounded: b is an exact zero only up to that, checked below)
    d[k] = 0
    d[k, (ax + 1) % 3] = rng.choice([-1, 1], k.size).astype(F32)
    d[cat == 9] = 0
    o[np.flatnonzero(cat == 9)[::2]] -= F32(20)  # oc < 0 in every component: each product is -0, so b = -0
    d[cat == 10] *= F32(1e20)
    nanrows = np.flatnonzero(cat == 11)
    d[nanrows, rng.integers(0, 3, nanrows.size)] = np.nan
    return {"o": o, "d": d, "centers": centers, "radii": radii, "cat": cat, "tgt": tgt}


def _tangent_dir(o, c, r, w):
    """From o towards the point of the sphere's rim in the plane of (c - o, w) where the ray is tangent."""
    oc = c - o
    L = np.linalg.norm(oc, axis=1, keepdims=True)
    ax = oc / L
    wp = unit(w - ax * np.sum(w * ax, axis=1, keepdims=True))
    s = np.clip(r / L, 0, 1)  # sine of the tangent's angle
    return ax * np.sqrt(1 - s * s) + wp * s


def elements(rays):
    """The 2^20 (ray, sphere) elements with the kernel-side constants in numpy binary32 as rt_set_scene / the trace
    kernels derive them (r2 = r * r; a = dot(d, d), a2 = 2a, a4 = 4a, a2_ok = 2a finite and > 0) and, for the wave
    layouts only, the candidate predicate of root_t1 / shadow_decide."""
    o = np.repeat(rays["o"], N_SPHERES, axis=0)
    d = np.repeat(rays["d"], N_SPHERES, axis=0)
    cen = np.tile(rays["centers"], (N_RAYS, 1))
    rad = np.tile(rays["radii"], N_RAYS)
    with np.errstate(all="ignore"):
        r2 = rad * rad
        a = f32dot(d, d)
        a2, a4 = F32(2) * a, F32(4) * a
        a2_ok = (a2 > 0) & (a2 < np.inf)
        oc = o - cen
        b = F32(2) * f32dot(oc, d)
        cc = f32dot(oc, oc) - r2
        disc = b * b - a4 * cc
        cand = (disc >= 0) & (b <= 0)
    return {"o": o, "d": d, "cen": cen, "rad": rad, "sph": np.column_stack([cen, r2]).astype(F32), "a": a, "a2": a2,
            "a4": a4, "a2_ok": a2_ok, "b": b, "disc": disc, "cand": cand,
            "cat": np.repeat(rays["cat"], N_SPHERES), "own": np.repeat(rays["tgt"], N_SPHERES) ==
            np.tile(np.arange(N_SPHERES), N_RAYS)}


@pytest.fixture(scope="module")
def elems(rays):
    return elements(rays)


LAYOUT_WAVES = 192


def wave_layout(cand, valid, seed):
    """Element order for one launch: every valid element in its own order (4 rays x 16 spheres per wave: interleaved
    candidates and non-candidates), then, built explicitly from the candidate (C) and non-candidate (N) pools, 192
    waves each of: 64 C; 64 N; one C at lane 0, 31, 32, 63 among 63 N; C and N alternating.  Returns the index array
    (a multiple of 64 long) and the wave kinds found in it."""
    rng = np.random.default_rng(seed)
    C_, N_ = np.flatnonzero(cand & valid), np.flatnonzero(~cand & valid)
    assert C_.size >= 64 and N_.size >= 64
    base = np.flatnonzero(valid)
    base = np.concatenate([base, N_[:(-base.size) % 64]])
    blocks = [base]
    blocks.append(rng.choice(C_, LAYOUT_WAVES * 64))
    blocks.append(rng.choice(N_, LAYOUT_WAVES * 64))
    for lane in (0, 31, 32, 63):
        wv = rng.choice(N_, (LAYOUT_WAVES, 64))
        wv[:, lane] = rng.choice(C_, LAYOUT_WAVES)
        blocks.append(wv.ravel())
    alt = rng.choice(N_, (LAYOUT_WAVES, 64))
    alt[:, ::2] = rng.choice(C_, (LAYOUT_WAVES, 32))
    blocks.append(alt.ravel())
    order = np.concatenate(blocks)
    assert order.size % 64 == 0
    cw = cand[order].reshape(-1, 64)
    count = cw.sum(axis=1)
    kinds = {"all": int((count == 64).sum()), "none": int((count == 0).sum()), "mixed": int(((count > 1) & (count < 64)).sum())}
    for lane in (0, 31, 32, 63):
        kinds[f"one@{lane}"] = int(((count == 1) & cw[:, lane]).sum())
    assert all(v >= LAYOUT_WAVES for v in kinds.values()), kinds
    return order, kinds


def oracle_sphere(batch, e, order, eps):
    o, d, cen, rad = [np.ascontiguousarray(e[k][order]) for k in ("o", "d", "cen", "rad")]
    dist = np.empty(order.size, F32)
    coll = np.empty(order.size, np.int32)
    batch.oracle_batch_intersect_sphere(_ptr(o), _ptr(d), _ptr(cen), _ptr(rad), C.c_float(eps), _ptr(dist), _ptr(coll),
                                        C.c_long(order.size))
    return dist, coll


def test_root_inputs_cover_their_categories(elems):
    """CPU only: the ray set holds what its docstring promises -- tangent rays with disc within a few ulp of 0 on
    both sides, b = +0 and b = -0, origins inside and on spheres, a2 = +inf and NaN, zero directions."""
    e = elems
    own = e["own"]
    t = own & (e["cat"] == 2)
    scale = np.abs(e["b"][t]) ** 2
    near = np.abs(e["disc"][t]) <= 16 * np.spacing(scale.astype(F32))
    assert near.mean() > 0.9, near.mean()
    assert (e["disc"][t][near] > 0).sum() > 500 and (e["disc"][t][near] < 0).sum() > 500
    bz = e["b"][own & (e["cat"] == 6)]
    assert (bz == 0).mean() > 0.9 and (~np.signbit(bz[bz == 0])).all()
    b9 = e["b"][e["cat"] == 9]
    assert (b9 == 0).all() and np.signbit(b9).any() and (~np.signbit(b9)).any()
    assert np.isinf(e["a2"][e["cat"] == 10]).all() and np.isnan(e["a2"][e["cat"] == 11]).all()
    assert (e["a2"][e["cat"] == 9] == 0).all() and e["a2_ok"][e["cat"] <= 8].all()
    assert e["a"][e["cat"] == 7].max() > 400  # light positions up to length 30
    hits = own & (e["cat"] == 0)
    assert e["cand"][hits].mean() > 0.99 and e["cand"].mean() < 0.5


@pytest.mark.parametrize("form", ["ok", "any"])
def test_sphere_t(prims, batch, elems, form):
    """sphere_t<true> ("ok": every element's 2a finite and > 0) and sphere_t<false> ("any": all 2^20 elements, the
    zero, infinite and NaN directions among them, a2_ok per lane).  Reference: oracle_intersect_sphere with epsilon 0,
    the literal formula.  Contract: where the oracle reports a selectable collision (dist > 0, a primary ray's rule)
    sphere_t returns that distance bit for bit; elsewhere a value <= 0 or NaN; and the secondary rule
    (t - 0.01f > 0) selects the same elements.  Every wave layout is built explicitly (wave_layout)."""
    e = elems
    valid = e["a2_ok"] if form == "ok" else np.ones_like(e["a2_ok"])
    order, kinds = wave_layout(e["cand"], valid, 81)
    print(f"sphere_t<{form}>: {order.size} elements, waves {kinds}")
    ins = [np.ascontiguousarray(e[k][order]) for k in ("o", "d", "a2", "a4")]
    ins += [e["a2_ok"][order].astype(np.int32), np.ascontiguousarray(e["sph"][order])]
    got = prims("sphere_t_" + form, ins, [(F32, 1)], order.size)
    dist, coll = oracle_sphere(batch, e, order, 0.0)
    sel = (coll != 0) & (dist > 0)
    assert sel.sum() > 50000 and (~sel).sum() > 50000
    bad_sel = sel & ~_same_bits(got, dist)
    with np.errstate(all="ignore"):
        bad_rej = ~sel & ~(np.isnan(got) | (got <= 0))
        sec = ((got - F32(0.01)) > 0) != ((dist - F32(0.01)) > 0)
    for what, bad in (("selectable distance differs", bad_sel), ("rejected element returns t > 0", bad_rej),
                      ("secondary selection differs", sec)):
        if bad.any():
            i = np.flatnonzero(bad)[:6]
            pytest.fail(f"sphere_t<{form}>: {what} at {bad.sum()} elements, e.g. wave {i // 64} lane {i % 64}: got "
                        f"{got[i]}, oracle {dist[i]} (collision {coll[i]}), category {e['cat'][order][i]}")


def shadow_threshold_by_bisection(a2):
    """The smallest float n with fl(fl(n / a2) - 0.001f) > 0, by bisection over bit patterns (n / a2 is monotonic in
    n for a2 > 0): DevLight::sh_t."""
    lo = np.zeros(a2.size, np.int64)           # n = +0 fails
    hi = np.full(a2.size, 0x7f800000, np.int64)  # n = +inf passes
    def passes(bits):
        n = bits.astype(np.uint32).view(F32)
        with np.errstate(all="ignore"):
            return (ref_div(n, a2) - F32(0.001)) > 0
    assert passes(hi).all() and not passes(lo).any()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        p = passes(mid)
        hi = np.where(p, mid, hi)
        lo = np.where(p, lo, mid)
    return hi.astype(np.uint32).view(F32)


@pytest.mark.parametrize("form", ["ok", "ok_thresh", "any"])
def test_shadow_blocked(prims, batch, elems, form):
    """shadow_blocked<true, false> ("ok"), <true, true> ("ok_thresh", the division-free threshold form) and
    <false, false> ("any", a2_ok per lane) with the ray's origin as the hit point and its direction as the light's
    position.  Reference: oracle_intersect_sphere with epsilon 0.001; the boolean equals its `collision`.  a, a2, a4
    as rt_set_scene derives them; sh_t is found here by bisection (shadow_threshold_by_bisection), not copied.  Every
    wave layout is built explicitly."""
    e = elems
    valid = e["a2_ok"] if form != "any" else np.ones_like(e["a2_ok"])
    order, kinds = wave_layout(e["cand"], valid, 82)
    print(f"shadow_blocked<{form}>: {order.size} elements, waves {kinds}")
    a2 = e["a2"][order]
    sh_t = np.zeros(order.size, F32)
    if form == "ok_thresh":
        ua, inv = np.unique(a2, return_inverse=True)
        sh_t = shadow_threshold_by_bisection(ua)[inv]
    light = np.column_stack([e["d"][order], e["a"][order], a2, e["a4"][order], sh_t, np.zeros(order.size, F32)])
    ins = [np.ascontiguousarray(e["o"][order]), np.ascontiguousarray(light.astype(F32)),
           e["a2_ok"][order].astype(np.int32), np.ascontiguousarray(e["sph"][order])]
    got = prims("shadow_" + form, ins, [(np.int32, 1)], order.size)
    dist, coll = oracle_sphere(batch, e, order, 0.001)
    assert (coll != 0).sum() > 50000 and (coll == 0).sum() > 50000
    # the epsilon's edge is really in the set: elements blocked without it and not with it
    _, coll0 = oracle_sphere(batch, e, order, 0.0)
    assert ((coll0 != 0) & (coll == 0)).sum() > 100
    bad = got != (coll != 0)
    if bad.any():
        i = np.flatnonzero(bad)[:6]
        pytest.fail(f"shadow_blocked<{form}>: {bad.sum()} of {order.size} differ, e.g. wave {i // 64} lane {i % 64}: "
                    f"got {got[i]}, oracle collision {coll[i]} distance {dist[i]}, category {e['cat'][order][i]}")


def test_plane_t(prims, batch, rays):
    """plane_t.  Reference: oracle_intersect_plane; plane_t > 0 iff the oracle collides, and then the values are
    equal bit for bit.  cn = dot(center, normal) in numpy binary32 as rt_set_scene derives it.  Inputs: the 2^16
    rays against 8 planes (axis-aligned and oblique normals, unnormalised too: 2^19 elements), which holds rays
    parallel to a plane (exact zero denominators: the axis-aligned directions of category 6 and the zero
    directions), origins in a plane, and NaN and huge directions."""
    rng = np.random.default_rng(91)
    normals = np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1), (0.3, 0.9, -0.2), (-2, 0.5, 1), (0, 3, 0),
                        (0.577, 0.577, 0.577)], dtype=F32)
    pc = rng.uniform(-5, 5, (8, 3)).astype(F32)
    pc[0] = (0, -1, 0)
    n_el = N_RAYS * 8
    o = np.repeat(rays["o"], 8, axis=0)
    d = np.repeat(rays["d"], 8, axis=0)
    nor, cen = np.tile(normals, (N_RAYS, 1)), np.tile(pc, (N_RAYS, 1))
    o[::1024 * 8] = cen[::1024 * 8]  # origins at the plane's centre
    with np.errstate(all="ignore"):
        cn = f32dot(cen, nor)
        den = f32dot(d, nor)
    assert (den == 0).sum() > 5000 and np.isnan(den).any()
    got = prims("plane_t", [o, d, nor, cn], [(F32, 1)], n_el)
    dist = np.empty(n_el, F32)
    coll = np.empty(n_el, np.int32)
    batch.oracle_batch_intersect_plane(_ptr(o), _ptr(d), _ptr(cen), _ptr(nor), _ptr(dist), _ptr(coll), C.c_long(n_el))
    assert (coll != 0).sum() > 100000 and (coll == 0).sum() > 100000 and np.isinf(dist[coll != 0]).any()
    with np.errstate(all="ignore"):
        pos = got > 0
    assert (pos == (coll != 0)).all(), f"{(pos != (coll != 0)).sum()} selections differ"
    assert_bits(got[pos], dist[pos], "plane_t", o[pos], d[pos])


# ----------------------------------------------------------------------------------------------------------------
# j. the supersampling resolve on the device
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
def test_resolve_on_device(prims, s):
    """resolve_unpack / resolve_add / resolve_round for k = 2^s samples a side.  Reference: the round-half-up mean
    per channel in integers, (sum + k^2/2) // k^2.  Inputs: a block of all 0x00FFFFFF (the largest sums) and one of
    zeros, 765 blocks whose channel sums sit on m k^2 + k^2/2 - 1, + 0 and + 1 for every m in 0..254 (another m
    per channel), and 2^14 random blocks."""
    k2 = 1 << (2 * s)
    rng = np.random.default_rng(100 + s)

    def spread(total):  # k2 samples in 0..255 with the given sums (total <= 255 * k2)
        q, r = np.divmod(total, k2)
        return q[:, None] + (np.arange(k2)[None, :] < r[:, None])

    m = np.repeat(np.arange(255), 3)
    dl = np.tile([-1, 0, 1], 255)
    tr, tg, tb = [mm * k2 + k2 // 2 + dl for mm in (m, (m * 7) % 255, 254 - m)]
    edge = (spread(tr) << 16) | (spread(tg) << 8) | spread(tb)
    px = np.concatenate([np.full((1, k2), 0x00ffffff), np.zeros((1, k2), np.int64), edge,
                         rng.integers(0, 1 << 24, (1 << 14, k2))]).astype(np.int64)
    assert px.max() <= 0x00ffffff and len(px) == 2 + 765 + (1 << 14)
    want = np.zeros(len(px), np.int64)
    for sh in (16, 8, 0):
        total = ((px >> sh) & 0xff).sum(axis=1)
        want |= ((total + k2 // 2) // k2) << sh
    assert want[0] == 0x00ffffff and want.max() <= 0x00ffffff
    got = prims("resolve", [px.astype(np.uint32)], [(np.uint32, 1)], len(px), ints=(s,))
    assert_bits(got, want.astype(np.uint32), f"resolve s={s}", px.astype(np.uint32))
