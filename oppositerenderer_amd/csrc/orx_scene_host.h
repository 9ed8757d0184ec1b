/*
 * orx_scene_host.h — scene preparation on the host: everything orx_init_scene does before it needs a device.
 * Validation of a caller's orx_scene, the reference's material, light and parallelogram formulas, the rewrite of
 * the triangle attributes in BVH leaf order, and the layout of the texture images.  Plain C++: no HIP, no device
 * allocation, so it can be built, tested and sanitised without a GPU (tests/scene_host_check.cpp).
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "orx.h"
#include "orx_scene_types.h"

namespace orx {

/* Every refusal orx_init_scene makes before it builds anything: ORX_OK, or a status with *err set.  `world` is the
 * renderer's shard count.  Reads nothing outside the arrays' stated sizes; an array whose count is non-zero must
 * not be NULL. */
orx_status scene_validate(const orx_scene* s, const orx_config& cfg, uint32_t world, std::string* err);

/* a validated scene, converted to what the kernels read (all but the triangles, which wait for the BVH) */
struct HostScene {
    std::vector<DevQuad> quads;
    std::vector<DevSphere> spheres;
    std::vector<DevMaterial> mats;
    std::vector<DevLight> lights;
    bool has_tex = false; /* a Texture material exists */
    bool media = false;   /* cfg.enable_media and the scene has a medium box: lo, hi, sigma_s, sigma_a */
    f3 med_lo{}, med_hi{};
    float sig_s = 0.f, sig_a = 0.f;
    float dir_zero = 0.f; /* orx_dir_zero() of the mesh's coordinates */
    f3 aabb_lo{}, aabb_hi{};
    float bs_cx = 0.f, bs_cy = 0.f, bs_cz = 0.f, bs_r = 0.f; /* AAB::getBoundingSphere, with the reference's bug */
};
HostScene scene_prepare(const orx_scene& s, const orx_config& cfg);

/* the triangle attributes in BVH leaf order: position k holds triangle leaf_order[k].  float4 per vertex
 * (v: xyz and, at a triangle's first vertex, the original id's bits; n, t, bt: xyz, 0), float2 per vertex (uv);
 * an attribute the scene lacks stays empty, tangents and bitangents unless normals and both are there */
struct LeafArrays {
    std::vector<float> v, n, uv, t, bt;
    std::vector<uint32_t> mat; /* the triangle's material, leaf order */
};
/* ORX_ERR_INVALID_ARGUMENT with *err set if leaf_order names a triangle >= nt (a builder's fault) */
orx_status scene_leaf_arrays(const orx_scene& s, const uint32_t* leaf_order, uint32_t nt, LeafArrays* out,
                             std::string* err);

/* the texture images back to back, each aligned to 256 bytes: texture i's texels at rgba[i], its normal map
 * (if it has one) at normal[i] */
struct TextureLayout {
    std::vector<size_t> rgba, normal;
    size_t total = 0;
};
TextureLayout scene_texture_layout(const orx_scene& s);

}  // namespace orx
