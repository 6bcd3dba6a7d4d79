// prims_gpu.hip -- the trace kernels' arithmetic primitives, one per kernel, TEST INFRASTRUCTURE ONLY
// (tests/test_gpu_prims.py; built by prims.mk with the flags of csrc/Makefile's print-flags).
//
// Every entry point takes device pointers, an element count and a stream, launches one kernel of 64-lane
// workgroups that applies one primitive of csrc/rt_prims.h, rt_fastmath.h, rt_pow.h or rt_resolve.h to each
// element and stores the result with a plain vector store, and returns the launch's hipError_t.  Element i runs
// on lane i % 64 of wave i / 64, so the caller decides which inputs share a wave (root_t1 and shadow_decide
// branch on a wave-wide ballot).  Nothing is restated here: each kernel only loads operands, calls the
// product's function and stores what it returns.  (The one exception is prims_disc, see there.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_fastmath.h"
#include "rt_internal.h"
#include "rt_pow.h"
#include "rt_prims.h"
#include "rt_resolve.h"

namespace {

using namespace rtk;

constexpr int WG = 64;

// one element per lane; lanes past n leave before any ballot
template <typename F>
__global__ __launch_bounds__(WG) void map_kernel(long long n, F f) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i < n) f(i);
}

template <typename F>
int run(long long n, void* stream, F f) {
    if (n <= 0) return (int)hipSuccess;
    if (n > (1LL << 24)) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + WG - 1) / WG);
    hipLaunchKernelGGL(map_kernel<F>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, n, f);
    return (int)hipGetLastError();
}

__device__ __forceinline__ f3 ld3(const float* p, long long i) { return mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

}  // namespace

#define UNARY(name, expr)                                                                      \
    extern "C" int prims_##name(const float* x, float* out, long long n, void* stream) {       \
        return run(n, stream, [=] __device__(long long i) { const float a = x[i]; out[i] = (expr); }); \
    }
#define BINARY(name, expr)                                                                             \
    extern "C" int prims_##name(const float* x, const float* y, float* out, long long n, void* stream) { \
        return run(n, stream, [=] __device__(long long i) {                                            \
            const float a = x[i], b = y[i];                                                            \
            out[i] = (expr);                                                                           \
        });                                                                                            \
    }

// a. correctly rounded operations
UNARY(cr_sqrt, cr_sqrt(a))
UNARY(cr_rcp, cr_rcp(a))
UNARY(cr_inv_len, cr_inv_len(a))
UNARY(sqrt_cr, sqrt_cr(a))
UNARY(rcp_cr, rcp_cr(a))
BINARY(div, a / b)
BINARY(div_cr, div_cr(a, b))

// b. sums and products without contraction (vectors: n x 3 floats)
extern "C" int prims_dot(const float* a, const float* b, float* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = dot(ld3(a, i), ld3(b, i)); });
}
extern "C" int prims_normalize(const float* a, float* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) {
        const f3 r = normalize(ld3(a, i));
        out[3 * i] = r.x, out[3 * i + 1] = r.y, out[3 * i + 2] = r.z;
    });
}
extern "C" int prims_sub_dot(const float* a, const float* b, const float* c, float* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = dot(sub(ld3(a, i), ld3(b, i)), ld3(c, i)); });
}
// The discriminant's shape, b*b - a4*c: sphere_t does not name it, so this line pins what the library's
// compile flags make of that expression (no fused multiply-add); the expression inside sphere_t itself is
// covered through prims_sphere_t's tangent rays.
extern "C" int prims_disc(const float* b, const float* a4, const float* c, float* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = b[i] * b[i] - a4[i] * c[i]; });
}

// c. IEEE 754-2019 maximum / minimum
UNARY(nmax0, nmax0(a))
BINARY(nmin, nmin(a, b))

// d. .NET's (int)float;  e. ShiftColor's channel;  f. the checkerboard parity
extern "C" int prims_net_f2i(const float* x, int32_t* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = net_f2i(x[i]); });
}
extern "C" int prims_shift_channel(const float* x, uint32_t* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = shift_channel(x[i]); });
}
BINARY(checker_tile, checker_tile(a, b))

// g. attenuation
UNARY(plane_att, plane_att(a))
UNARY(sphere_att, sphere_att(a))

// h. Math.Pow: the double of glibc_pow((double)x, (double)e) and the float of spec_pow<true>(x, kind, e)
extern "C" int prims_spec_pow(const float* x, const uint32_t* kind, const float* e, double* out_d, float* out_f,
                              long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) {
        out_d[i] = glibc_pow((double)x[i], (double)e[i], g_pow_log, g_pow_exp);
        out_f[i] = spec_pow<true>(x[i], kind[i], e[i]);
    });
}
extern "C" int prims_glibc_pow(const double* x, const double* y, double* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) { out[i] = glibc_pow(x[i], y[i], g_pow_log, g_pow_exp); });
}

// i. root selection.  o, d: n x 3; sph: n x 4 (cx, cy, cz, r2); a2, a4, a2_ok per element.
template <bool A2OK>
static int sphere_t_run(const float* o, const float* d, const float* a2, const float* a4, const int32_t* a2_ok,
                        const float* sph, float* out, long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) {
        const DevSphere s{sph[4 * i], sph[4 * i + 1], sph[4 * i + 2], sph[4 * i + 3]};
        out[i] = sphere_t<A2OK>(ld3(o, i), ld3(d, i), a2[i], a4[i], a2_ok[i] != 0, s);
    });
}
extern "C" int prims_sphere_t_ok(const float* o, const float* d, const float* a2, const float* a4,
                                 const int32_t* a2_ok, const float* sph, float* out, long long n, void* stream) {
    return sphere_t_run<true>(o, d, a2, a4, a2_ok, sph, out, n, stream);
}
extern "C" int prims_sphere_t_any(const float* o, const float* d, const float* a2, const float* a4,
                                  const int32_t* a2_ok, const float* sph, float* out, long long n, void* stream) {
    return sphere_t_run<false>(o, d, a2, a4, a2_ok, sph, out, n, stream);
}
// hp: n x 3; light: n x 8 (px, py, pz, a, a2, a4, sh_t, unused); sph: n x 4
template <bool A2OK, bool THRESH>
static int shadow_run(const float* hp, const float* light, const int32_t* a2_ok, const float* sph, int32_t* out,
                      long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) {
        DevLight l{};
        const float* q = light + 8 * i;
        l.px = q[0], l.py = q[1], l.pz = q[2], l.a = q[3], l.a2 = q[4], l.a4 = q[5], l.sh_t = q[6];
        const DevSphere s{sph[4 * i], sph[4 * i + 1], sph[4 * i + 2], sph[4 * i + 3]};
        out[i] = shadow_blocked<A2OK, THRESH>(ld3(hp, i), l, a2_ok[i] != 0, s) ? 1 : 0;
    });
}
extern "C" int prims_shadow_ok(const float* hp, const float* light, const int32_t* a2_ok, const float* sph,
                               int32_t* out, long long n, void* stream) {
    return shadow_run<true, false>(hp, light, a2_ok, sph, out, n, stream);
}
extern "C" int prims_shadow_ok_thresh(const float* hp, const float* light, const int32_t* a2_ok, const float* sph,
                                      int32_t* out, long long n, void* stream) {
    return shadow_run<true, true>(hp, light, a2_ok, sph, out, n, stream);
}
extern "C" int prims_shadow_any(const float* hp, const float* light, const int32_t* a2_ok, const float* sph,
                                int32_t* out, long long n, void* stream) {
    return shadow_run<false, false>(hp, light, a2_ok, sph, out, n, stream);
}
// o, d, normal: n x 3; cn per element
extern "C" int prims_plane_t(const float* o, const float* d, const float* normal, const float* cn, float* out,
                             long long n, void* stream) {
    return run(n, stream, [=] __device__(long long i) {
        DevPlane p{};
        p.nx = normal[3 * i], p.ny = normal[3 * i + 1], p.nz = normal[3 * i + 2], p.cn = cn[i];
        out[i] = plane_t(ld3(o, i), ld3(d, i), p);
    });
}

// j. the supersampling resolve: px holds n blocks of (1 << s)^2 samples
extern "C" int prims_resolve(const uint32_t* px, int s, uint32_t* out, long long n, void* stream) {
    if (s < 0 || s > 3) return (int)hipErrorInvalidValue;
    return run(n, stream, [=] __device__(long long i) {
        const int m = 1 << (2 * s);
        ResolveSum sum = resolve_unpack(px[i * m]);
        for (int k = 1; k < m; ++k) sum = resolve_add(sum, resolve_unpack(px[i * m + k]));
        out[i] = resolve_round(sum, s);
    });
}
