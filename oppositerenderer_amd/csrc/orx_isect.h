/*
 * orx_isect.h — the scene as the kernels see it, a hit, and the primitive intersectors.
 *
 * Replaces geometry_instance/{parallelogram,Sphere,TriangleMesh}.cu (intersection) of the reference.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orx_bvh_nodes.h"
#include "orx_detmath.h"
#include "orx_scene_types.h" /* f3, the material / light / primitive structs */

namespace orx {

/* ------------------------------------------------------------------ */
/* scene                                                               */
/* ------------------------------------------------------------------ */
struct DevScene {
    uint32_t nq, ns, nt;
    const DevQuad* quads;
    const uint32_t* qmat;
    const DevSphere* spheres;
    const uint32_t* smat;
    /* triangles in BVH leaf order: tri_v[3k] = {p0.xyz, original triangle id bits},
     * tri_v[3k+1] = p1, tri_v[3k+2] = p2 (48 B per triangle, no index indirection) */
    const float4* tri_v;
    const float4* tri_n;       /* [nt][3] vertex normals in leaf order, or NULL */
    const float2* tri_uv;      /* [nt][3] texcoords in leaf order, or NULL (TriangleMesh.cu:74-84) */
    const float4* tri_t;       /* [nt][3] tangents, [nt][3] bitangents in leaf order, or NULL */
    const float4* tri_bt;
    const DevTexture* tex;
    uint32_t ntex;
    const uint32_t* tmat;      /* leaf order */
    const DevMaterial* mats;
    const DevLight* lights;
    uint32_t nl;
    /* bounding sphere (AAB::getBoundingSphere with Vector3::length bug) */
    float bs_cx, bs_cy, bs_cz, bs_r;
    /* triangle BVH4 (nt > 0); a traversal pushes at most stack_entries refs */
    const DevNode4* bvh4;
    uint32_t bvh_nodes;
    uint32_t stack_entries;
    float dir_zero; /* what a zero direction component becomes in the box tests: orx_dir_zero() of the mesh */
    unsigned long long* trav_stats; /* [16] in ORX_TRAV_STATS builds, else unused */
};

/* Traversal stack: per-lane column of a dynamic LDS array [stack_entries][64]
 * owned by a 64-thread (one-wave) block; entry k of a lane at s[k * 64].  The
 * depth bound is computed from the tree at orx_init_scene and the launch
 * passes ORX_STACK_BYTES(S) of dynamic LDS. */
#define ORX_STACK_DECL extern __shared__ uint32_t orx_stack_lds[]
#define ORX_STACK_PTR (&orx_stack_lds[threadIdx.x & 63])
#define ORX_STACK_BYTES(S) ((size_t)((S).stack_entries + 2) * 64 * 4) /* + 2: StackL::put past the bound */

struct Hit {
    float t;
    int32_t prim;  /* global id: quads, spheres, triangles (original triangle order) */
    uint32_t slot; /* triangles: index in leaf order */
    float b, g;    /* triangle barycentrics */
    f3 sn;         /* sphere normal attribute */
};

/* parallelogram.cu:49-76 */
__device__ __forceinline__ bool isect_quad(const DevQuad& q, f3 o, f3 d, float tmin, float tmax, float& tout) {
    f3 n = mk(q.nx, q.ny, q.nz);
    float dt = dot(d, n);
    float t = (q.d - dot(n, o)) / dt;
    if (t > tmin && t < tmax) {
        f3 p = o + d * t;
        f3 vi = p - mk(q.ax, q.ay, q.az);
        float a1 = dot(mk(q.v1x, q.v1y, q.v1z), vi);
        if (a1 >= 0 && a1 <= 1) {
            float a2 = dot(mk(q.v2x, q.v2y, q.v2z), vi);
            if (a2 >= 0 && a2 <= 1) {
                tout = t;
                return true;
            }
        }
    }
    return false;
}
/* Sphere.cu:32-56 */
__device__ __forceinline__ bool isect_sphere(const DevSphere& s, f3 o, f3 d, float tmin, float tmax, float& tout,
                                             f3& nout) {
    f3 O = o - mk(s.cx, s.cy, s.cz);
    float b = dot(O, d);
    float c = dot(O, O) - s.r * s.r;
    float disc = b * b - c;
    if (disc > 0.0f) {
        float sdisc = sqrtf(disc);
        float root1 = (-b - sdisc);
        if (root1 > tmin && root1 < tmax) {
            tout = root1;
            nout = (O + d * root1) / s.r;
            return true;
        }
        float root2 = (-b + sdisc);
        if (root2 > tmin && root2 < tmax) {
            tout = root2;
            nout = (O + d * root2) / s.r;
            return true;
        }
    }
    return false;
}
/* OptiX intersect_triangle_branchless (TriangleMesh.cu:46) */
__device__ __forceinline__ bool isect_tri(f3 p0, f3 p1, f3 p2, f3 o, f3 d, float tmin, float tmax, float& tout,
                                          float& bout, float& gout) {
    f3 e0 = p1 - p0;
    f3 e1 = p0 - p2;
    f3 n = cross(e1, e0);
    f3 e2 = (p0 - o) * (1.0f / dot(n, d));
    f3 i = cross(d, e2);
    float beta = dot(i, e1);
    float gamma = dot(i, e0);
    float t = dot(n, e2);
    if ((t < tmax) & (t > tmin) & (beta >= 0.0f) & (gamma >= 0.0f) & (beta + gamma <= 1)) {
        tout = t;
        bout = beta;
        gout = gamma;
        return true;
    }
    return false;
}
__device__ __forceinline__ f3 ld_f3(const float4& v) { return mk(v.x, v.y, v.z); }

}  // namespace orx
