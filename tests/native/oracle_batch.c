/* oracle_batch.c -- the CPU oracle's per-function entry points over arrays, TEST INFRASTRUCTURE ONLY
 * (tests/test_gpu_prims.py; built by prims.mk together with oracle/oracle.c and its flags).  A loop around each
 * entry point and nothing else: a million calls through ctypes would take longer than the whole GPU test. */
#include <math.h>
#include <stdint.h>

#include "../../oracle/oracle.h"

/* the host libm's pow, the function the oracle calls for Math.Pow */
void libm_batch_pow(const double* x, const double* y, double* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = pow(x[i], y[i]);
}

static rt_vec3 v3at(const float* p, long i) {
    rt_vec3 v = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    return v;
}

/* o, d, center: n x 3 */
void oracle_batch_intersect_sphere(const float* o, const float* d, const float* center, const float* radius,
                                   float epsilon, float* distance, int32_t* collision, long n) {
    for (long i = 0; i < n; ++i) {
        int c = 0;
        distance[i] = oracle_intersect_sphere(v3at(o, i), v3at(d, i), v3at(center, i), radius[i], epsilon, &c);
        collision[i] = c;
    }
}

/* o, d, center, normal: n x 3 */
void oracle_batch_intersect_plane(const float* o, const float* d, const float* center, const float* normal,
                                  float* distance, int32_t* collision, long n) {
    for (long i = 0; i < n; ++i) {
        int c = 0;
        distance[i] = oracle_intersect_plane(v3at(o, i), v3at(d, i), v3at(center, i), v3at(normal, i), &c);
        collision[i] = c;
    }
}

void oracle_batch_net_float_to_int(const float* v, int32_t* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = oracle_net_float_to_int(v[i]);
}

/* the blue byte of oracle_shift_color((0, 0, v)) */
void oracle_batch_shift_channel(const float* v, int32_t* out, long n) {
    for (long i = 0; i < n; ++i) {
        rt_vec3 c = {0.0f, 0.0f, v[i]};
        out[i] = oracle_shift_color(c) & 0xff;
    }
}
