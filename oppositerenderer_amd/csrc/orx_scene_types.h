/*
 * orx_scene_types.h — the plain scene structs and the float3 they are made of, shared by the device code
 * (the headers under orx_device.h include this) and the host-only scene preparation (orx_scene_host.cpp).  No HIP in it: under
 * hipcc the functions carry the device qualifiers they always had, elsewhere they are plain inline functions.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#include "orx_detmath.h"

#if defined(__HIPCC__)
#define ORX_HDI __host__ __device__ __forceinline__
#else
#define ORX_HDI inline
#endif

namespace orx {

/* ------------------------------------------------------------------ */
/* float3 with OptiX semantics                                          */
/* ------------------------------------------------------------------ */
struct f3 {
    float x, y, z;
};
ORX_HDI f3 mk(float x, float y, float z) { return f3{x, y, z}; }
ORX_HDI f3 mk1(float a) { return f3{a, a, a}; }
ORX_HDI f3 operator+(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
ORX_HDI f3 operator-(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
ORX_HDI f3 operator*(f3 a, f3 b) { return f3{a.x * b.x, a.y * b.y, a.z * b.z}; }
ORX_HDI f3 operator*(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
ORX_HDI f3 operator*(float s, f3 a) { return f3{s * a.x, s * a.y, s * a.z}; }
ORX_HDI f3 operator-(f3 a) { return f3{-a.x, -a.y, -a.z}; }
/* optix float3 / float = a * (1.0f / s) */
ORX_HDI f3 operator/(f3 a, float s) {
    float inv = 1.0f / s;
    return a * inv;
}
ORX_HDI float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ORX_HDI f3 cross(f3 a, f3 b) {
    return f3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
ORX_HDI float length(f3 a) { return sqrtf(dot(a, a)); }
ORX_HDI f3 normalize(f3 a) {
    float inv = 1.0f / sqrtf(dot(a, a));
    return a * inv;
}
ORX_HDI float maxf(float a, float b) { return a > b ? a : b; }
ORX_HDI float fmax3(f3 a) { return fmaxf(fmaxf(a.x, a.y), a.z); }
ORX_HDI float favgf(f3 v) { return (v.x + v.y + v.z) * 0.3333333333f; }
ORX_HDI f3 reflect(f3 i, f3 n) { return i - (n * 2.0f) * dot(n, i); }
ORX_HDI bool isnan3(f3 v) { return v.x != v.x || v.y != v.y || v.z != v.z; }

/* ------------------------------------------------------------------ */
/* scene                                                               */
/* ------------------------------------------------------------------ */
enum : int32_t { MAT_DIFFUSE = 0, MAT_EMITTER = 1, MAT_MIRROR = 2, MAT_GLASS = 3, MAT_GLOSSY = 4, MAT_TEXTURE = 5 };
enum : int32_t { LIGHT_AREA = 0, LIGHT_POINT = 1, LIGHT_SPOT = 2 };

struct DevMaterial {
    int32_t type;
    f3 Kd, Ks, Kr, Kt;
    float ior, exponent;
    f3 powerPerArea, Lemit;
    float inverseArea;
    int32_t tex; /* Texture: index into DevScene::tex */
};
/* Texture images (material/Texture.cpp:83-107): RGBA8 texels in HBM */
struct DevTexture {
    const uint8_t* rgba;
    const uint8_t* nrgba; /* normal map or NULL */
    uint32_t w, h, nw, nh;
};
struct DevLight {
    int32_t type;
    f3 power, position, v1, v2, normal, Lemit; /* Lemit doubles as intensity */
    f3 direction;
    float area, inverseArea, angle;
};
/* parallelogram: plane (n,d), anchor, v1/|v1|^2, v2/|v2|^2 (Cornell.cpp:45-56) */
struct DevQuad {
    float nx, ny, nz, d;
    float ax, ay, az, v1x;
    float v1y, v1z, v2x, v2y;
    float v2z, pad0, pad1, pad2;
};
struct DevSphere {
    float cx, cy, cz, r;
};

/* Per-ray slab-test constants.  A zero direction component is replaced by
 * +-1e-30 for the box tests only: the tilted ray leaves a conservative box
 * (>= 1e-20 margin, see the builder) only beyond t = 1e10, so no box the exact
 * ray reaches is culled; the triangle tests use the exact direction.
 * The node test multiplies coordinate differences by the reciprocal, 1e30: beyond 3.4e8 that product
 * overflows, and (origin - o) * inv = -inf culled boxes the ray was inside of.  So a mesh whose coordinates
 * pass 1.3e6 gets a larger substitute, max |coordinate| * 2^-120: the products of a ray that starts within 250
 * times that bound stay finite, and the tilt over a run as long as the bound (bound^2 * 2^-120: 1e-19 at 4e8,
 * 1e-12 at 1e12) stays inside the builder's relative 1e-6 expansion of any box further than that from a
 * coordinate plane.  Smaller meshes keep 1e-30 and every decision they had. */
ORX_HDI float orx_dir_zero(float max_abs_coordinate) {
    return fmaxf(1e-30f, max_abs_coordinate * 0x1p-120f);
}

}  // namespace orx
