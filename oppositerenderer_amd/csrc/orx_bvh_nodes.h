/*
 * orx_bvh_nodes.h — the BVH node layouts and build options shared by the host
 * builder (orx_bvh_host.cpp), the device builder (orx_bvh.hip) and the
 * traversal kernels (orx_traverse.h).  Plain C++: needs no HIP header.
 */
#pragma once

#include <stdint.h>

namespace orx {

/* Binary BVH node (build only): 32 B, leaves hold a primitive range */
struct DevBvhNode {
    float lo[3];
    uint32_t left_or_first; /* inner: left child index; leaf: first prim in prim_index */
    float hi[3];
    uint32_t count_or_right; /* leaf: 0x80000000 | count; inner: right child */
};

/* Four-wide BVH node, 64 B (one 64-B segment, four dwordx4 loads), collapsed
 * from the binary SAH tree.  Child boxes are quantised to 8 bits per bound
 * against the node's origin with a power-of-two scale per axis, rounded
 * outward (so every decoded box contains the child's conservative box):
 *   lo_k(child i) = origin_k + qlo_k[i] * s_k,   s_k = 2^e_k
 * The scales are stored as floats (the x scale in the first 16 B, y and z in
 * the last), so the node test reads them instead of decoding exponent bytes.
 * Child reference: inner node index, or ORX_LEAF | first << 3 | (count - 1)
 * for a triangle range in leaf order, or ORX_EMPTY. */
struct DevBvh4 {
    float ox, oy, oz;
    float sx;          /* 2^e_x */
    uint32_t qlo[3];   /* per axis: byte i = child i */
    uint32_t qhi[3];
    uint32_t child[4];
    float sy, sz;      /* 2^e_y, 2^e_z */
};
/* fp32 variant (ORX_BVH_FP32): 128 B, child bounds unquantised, SoA by
 * axis so the near/far bound quadruples are picked by address */
struct DevBvh4F {
    float b[6][4];     /* lo_x, hi_x, lo_y, hi_y, lo_z, hi_z; [child] */
    uint32_t child[4];
    uint32_t pad[4];
};
#ifdef ORX_BVH_FP32
typedef DevBvh4F DevNode4;
#else
typedef DevBvh4 DevNode4;
#endif
constexpr uint32_t ORX_LEAF = 0x80000000u;
constexpr uint32_t ORX_EMPTY = 0xffffffffu;
constexpr uint32_t ORX_DONE = 0x7fffffffu; /* traversal sentinel: no node */

#define ORX_BVH_STACK 32 /* depth cap of the binary build */

/* What both builders take; the defaults were measured on the 1080p hall
 * (tools/trav_stats.py): the SAH leaf test up to 8 triangles cuts triangle
 * tests/ray 5.9 -> 3.2 */
struct BvhBuildOptions {
    int bins = 32;          /* SAH bins per axis (ORX_BVH_BINS, 2..32) */
    uint32_t leaf_max = 8;  /* largest leaf (ORX_BVH_LEAF_MAX, 1..8) */
    float leaf_sah = 0.6f;  /* node traversal cost relative to a triangle test (ORX_BVH_LEAF_SAH); 0 = leaves of <= leaf_max, no test */
    int treelet_passes = 3; /* treelet restructuring sweeps of the binary tree (ORX_BVH_TREELET, 0..8) */
    int treelet_leaves = 9; /* ORX_BVH_TREELET_LEAVES: 9 or 7 (9: hall PPM +0.9 %, VCM +0.6 % over 7; 11 priced: no further gain) */
    bool sah_collapse = true; /* SAH-optimal four-wide collapse (ORX_BVH_COLLAPSE); false: open the largest-area child */
};

}  // namespace orx
