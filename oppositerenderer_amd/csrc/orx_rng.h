/*
 * orx_rng.h — the random numbers and the sampling routines of the device code.
 *
 * Replaces helpers/random.h (cuRAND XORWOW), helpers/samplers.h and helpers/helpers.h of the reference.
 * Float expressions keep the reference's operand order; the library is built
 * with -ffp-contract=off and correctly rounded div/sqrt so the kernels agree
 * bit for bit with the CPU oracle on every control-flow decision.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orx_detmath.h"
#include "orx_scene_types.h" /* f3 */

namespace orx {

__host__ __device__ inline bool refract(f3& r, f3 i, f3 n, float ior) {
    f3 nn = n;
    float negNdotV = dot(i, nn);
    float eta;
    if (negNdotV > 0.0f) {
        eta = ior;
        nn = -n;
        negNdotV = -negNdotV;
    } else {
        eta = 1.f / ior;
    }
    const float k = 1.f - eta * eta * (1.f - negNdotV * negNdotV);
    if (k < 0.0f) {
        r = mk1(0.f);
        return false;
    }
    r = normalize(i * eta - nn * (eta * negNdotV + sqrtf(k)));
    return true;
}

/* ------------------------------------------------------------------ */
/* cuRAND XORWOW state, kept in registers; SoA planes in HBM           */
/* ------------------------------------------------------------------ */
struct Rng {
    uint32_t v0, v1, v2, v3, v4, d;
};
struct RngPlanes {
    uint32_t* p[6]; /* v0..v4, d : [slots] each, coalesced dword access */
};
__device__ __forceinline__ Rng rng_load(const RngPlanes& P, size_t s) {
    return Rng{P.p[0][s], P.p[1][s], P.p[2][s], P.p[3][s], P.p[4][s], P.p[5][s]};
}
__device__ __forceinline__ void rng_store(const RngPlanes& P, size_t s, const Rng& r) {
    P.p[0][s] = r.v0; P.p[1][s] = r.v1; P.p[2][s] = r.v2;
    P.p[3][s] = r.v3; P.p[4][s] = r.v4; P.p[5][s] = r.d;
}
/* curand_init(seed, 0, 0) — subsequence and offset 0: no skip-ahead */
__host__ __device__ __forceinline__ Rng rng_init(uint64_t seed) {
    uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    uint32_t s1 = ((uint32_t)(seed >> 32)) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0;
    uint32_t t1 = 2591861531u * s1;
    Rng r;
    r.d = 6615241u + t1 + t0;
    r.v0 = 123456789u + t0;
    r.v1 = 362436069u ^ t0;
    r.v2 = 521288629u + t1;
    r.v3 = 88675123u ^ t1;
    r.v4 = 5783321u + t0;
    return r;
}
__host__ __device__ __forceinline__ uint32_t rng_next(Rng& s) {
    uint32_t t = s.v0 ^ (s.v0 >> 2);
    s.v0 = s.v1;
    s.v1 = s.v2;
    s.v2 = s.v3;
    s.v3 = s.v4;
    s.v4 = (s.v4 ^ (s.v4 << 4)) ^ (t ^ (t << 1));
    s.d += 362437u;
    return s.v4 + s.d;
}
/* getRandomUniformFloat (helpers/random.h:65-69): curand_uniform is
 * x*2^-32 + 2^-33 which nvcc contracts into one FMA. */
__device__ __forceinline__ float rnd(Rng& s) {
    uint32_t x = rng_next(s);
    float u = __builtin_fmaf((float)x, 2.3283064e-10f, 2.3283064e-10f / 2.0f);
    return maxf(u - ORX_FLT_EPSILON, 0.0f);
}

/* ------------------------------------------------------------------ */
/* samplers (helpers/samplers.h, helpers.h:119-134)                    */
/* ------------------------------------------------------------------ */
__device__ __forceinline__ void create_coordinate_system(f3 N, f3& U, f3& V) {
    if (fabsf(N.x) > fabsf(N.y)) {
        float invLength = 1.f / sqrtf(N.x * N.x + N.z * N.z);
        U = mk(-N.z * invLength, 0.f, N.x * invLength);
    } else {
        float invLength = 1.f / sqrtf(N.y * N.y + N.z * N.z);
        U = mk(0.f, N.z * invLength, -N.y * invLength);
    }
    V = cross(N, U);
}
/* sampleUnitHemisphereCos (samplers.h:24-43) */
__device__ __forceinline__ f3 sample_hemisphere_cos(f3 normal, float sx, float sy) {
    float theta = orx_acosf(sqrtf(sx));
    float phi = 2.0f * ORX_PI_F * sy;
    float st = orx_sinf(theta);
    float xs = st * orx_cosf(phi);
    float ys = orx_cosf(theta);
    float zs = st * orx_sinf(phi);
    f3 U, V;
    create_coordinate_system(normal, U, V);
    return normalize(U * xs + normal * ys + V * zs);
}
/* sampleUnitHemisphere (samplers.h:46-57) */
__device__ __forceinline__ f3 sample_hemisphere(f3 normal, float sx, float sy) {
    f3 U, V;
    create_coordinate_system(normal, U, V);
    float phi = 2.0f * ORX_PI_F * sx;
    float r = sqrtf(sy);
    float x = r * orx_cosf(phi);
    float y = r * orx_sinf(phi);
    float z = 1.0f - x * x - y * y;
    z = z > 0.0f ? sqrtf(z) : 0.0f;
    return normalize(U * x + V * y + normal * z);
}
/* sampleUnitSphere (samplers.h:59-72) */
__device__ __forceinline__ f3 sample_unit_sphere(float sx, float sy) {
    f3 v;
    v.z = 1.f - 2.f * sx;
    float phi = 2 * ORX_PI_F * sy;
    float r = sqrtf(1.f - v.z * v.z);
    v.x = r * orx_cosf(phi);
    v.y = r * orx_sinf(phi);
    return v;
}
/* sampleDisc (samplers.h:74-93) */
__device__ __forceinline__ f3 sample_disc(float sx, float sy, f3 center, float radius, f3 normal) {
    f3 U, V;
    create_coordinate_system(normal, U, V);
    float r = sqrtf(sx);
    float theta = 2.f * ORX_PI_F * sy;
    float x = r * orx_cosf(theta);
    float y = r * orx_sinf(theta);
    return center + (U * x + V * y) * radius;
}

}  // namespace orx
