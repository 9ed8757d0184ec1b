/*
 * orx_scene_host.cpp — scene validation and conversion on the host (orx_scene_host.h).  Float expressions keep
 * the reference's operand order; built with -ffp-contract=off like the rest of the library.
 */
#include "orx_scene_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace orx {

static f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }

static orx_status refuse(std::string* err, orx_status st, const char* msg) {
    if (err) *err = msg;
    return st;
}
#define ORX_NEED(ptr) \
    if (!s->ptr) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "scene array " #ptr " is NULL")

orx_status scene_validate(const orx_scene* s, const orx_config& cfg, uint32_t world, std::string* err) {
    if (!s) return ORX_ERR_INVALID_ARGUMENT;
    if (s->n_lights == 0 || !s->lights) return refuse(err, ORX_ERR_NO_LIGHTS, "No lights exists in this scene.");
    if (s->n_materials == 0 || !s->materials) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "scene has no materials");
    const uint32_t nq = s->n_quads, ns = s->n_spheres, nt = s->n_triangles, nm = s->n_materials;
    /* the traversal addresses triangles (48 B) and BVH4 nodes (64 B, fewer than triangles) with
     * 32-bit byte offsets */
    if (nt >= (1u << 26)) return refuse(err, ORX_ERR_UNSUPPORTED, "more than 2^26 triangles");
    /* material indices and triangle vertex indices */
    if (nq) {
        ORX_NEED(quads);
        ORX_NEED(quad_material);
    }
    for (uint32_t i = 0; i < nq; i++)
        if (s->quad_material[i] >= nm) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "quad material out of range");
    if (ns) {
        ORX_NEED(spheres);
        ORX_NEED(sphere_material);
    }
    for (uint32_t i = 0; i < ns; i++)
        if (s->sphere_material[i] >= nm) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "sphere material out of range");
    if (s->n_textures) ORX_NEED(textures);
    for (uint32_t i = 0; i < s->n_textures; i++) {
        const orx_texture& t = s->textures[i];
        if (!t.rgba || !t.width || !t.height || (t.normal_rgba && (!t.normal_width || !t.normal_height)))
            return refuse(err, ORX_ERR_INVALID_ARGUMENT, "texture image without texels");
    }
    for (uint32_t i = 0; i < nm; i++)
        if (s->materials[i].type == ORX_MAT_TEXTURE &&
            (s->materials[i].texture < 0 || (uint32_t)s->materials[i].texture >= s->n_textures))
            return refuse(err, ORX_ERR_INVALID_ARGUMENT, "Texture material without a texture image");
    if (cfg.enable_media && s->n_media) {
        if (s->n_media != 1 || !s->media)
            return refuse(err, ORX_ERR_UNSUPPORTED, "participating media: one medium box per scene");
        const float* m = s->media;
        if (!(m[0] < m[3] && m[1] < m[4] && m[2] < m[5]) || !(m[6] >= 0 && m[7] >= 0 && m[6] + m[7] > 0))
            return refuse(err, ORX_ERR_INVALID_ARGUMENT, "medium box: min < max and sigma_s + sigma_a > 0");
        if (cfg.volumetric_photons == 0)
            return refuse(err, ORX_ERR_INVALID_ARGUMENT, "volumetric_photons must be > 0 with media");
        if (world > 1) return refuse(err, ORX_ERR_UNSUPPORTED, "participating media are single-device");
    }
    if (s->n_vertices) ORX_NEED(vertices);
    if (nt) {
        ORX_NEED(triangles);
        ORX_NEED(triangle_material);
    }
    for (uint32_t i = 0; i < nt; i++) {
        if (s->triangle_material[i] >= nm) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "triangle material out of range");
        for (int k = 0; k < 3; k++)
            if (s->triangles[3 * (size_t)i + k] >= s->n_vertices)
                return refuse(err, ORX_ERR_INVALID_ARGUMENT, "triangle vertex index out of range");
    }
    for (uint32_t i = 0; i < nm; i++)
        if (s->materials[i].type < 0 || s->materials[i].type > ORX_MAT_TEXTURE)
            return refuse(err, ORX_ERR_INVALID_ARGUMENT, "unknown material type");
    return ORX_OK;
}
#undef ORX_NEED

static DevLight make_light(const orx_light& L) {
    /* Light ctors (renderer/Light.cpp:14-49) */
    DevLight l;
    std::memset(&l, 0, sizeof l);
    l.type = L.type;
    l.power = ld3(L.power);
    l.position = ld3(L.position);
    if (L.type == ORX_LIGHT_AREA) {
        l.v1 = ld3(L.v1);
        l.v2 = ld3(L.v2);
        f3 c = cross(l.v1, l.v2);
        l.normal = normalize(c);
        l.area = length(c);
        l.inverseArea = 1.0f / l.area;
        l.Lemit = (l.power * l.inverseArea) * ORX_1_PI_F;
    } else if (L.type == ORX_LIGHT_POINT) {
        l.Lemit = (l.power * 0.25f) * ORX_1_PI_F;
    } else {
        l.direction = ld3(L.direction); /* ctor normalises its by-value parameter only (Light.cpp:41) */
        l.normal = l.direction;
        l.angle = L.angle;
        float angleFactor = 1.0f / (1.0f - cosf(l.angle * 180 * ORX_1_PI_F));
        l.Lemit = ((l.power * 0.25f) * ORX_1_PI_F) * angleFactor;
    }
    return l;
}

HostScene scene_prepare(const orx_scene& s, const orx_config& cfg) {
    HostScene h;
    const uint32_t nq = s.n_quads, ns = s.n_spheres, nm = s.n_materials;
    /* Cornell::createParallelogram (scene/Cornell.cpp:33-64) */
    h.quads.resize(nq);
    for (uint32_t i = 0; i < nq; i++) {
        const float* q = s.quads + 9 * (size_t)i;
        f3 anchor = ld3(q), o1 = ld3(q + 3), o2 = ld3(q + 6);
        f3 normal = normalize(cross(o1, o2));
        float d = dot(normal, anchor);
        f3 v1 = o1 / dot(o1, o1), v2 = o2 / dot(o2, o2);
        h.quads[i] = DevQuad{normal.x, normal.y, normal.z, d, anchor.x, anchor.y, anchor.z, v1.x,
                             v1.y, v1.z, v2.x, v2.y, v2.z, 0, 0, 0};
    }
    h.spheres.resize(ns);
    for (uint32_t i = 0; i < ns; i++) {
        const float* c = s.spheres + 4 * (size_t)i;
        h.spheres[i] = DevSphere{c[0], c[1], c[2], c[3]};
    }
    h.mats.resize(nm);
    for (uint32_t i = 0; i < nm; i++) {
        const orx_material& m = s.materials[i];
        DevMaterial d;
        std::memset(&d, 0, sizeof d);
        d.type = m.type;
        d.Kd = ld3(m.Kd);
        d.Ks = ld3(m.Ks);
        d.Kr = ld3(m.Kr);
        d.Kt = ld3(m.Kt);
        d.ior = m.ior;
        d.exponent = m.exponent;
        d.tex = m.texture;
        if (m.type == ORX_MAT_DIFFUSE_EMITTER) {
            /* DiffuseEmitter.cpp:17-25, :48-62 */
            f3 power = ld3(m.power) * d.Kd;
            d.inverseArea = m.inverse_area;
            d.powerPerArea = power * m.inverse_area;
            d.Lemit = (power * m.inverse_area) * ORX_1_PI_F;
        } else if (m.type == ORX_MAT_GLOSSY) {
            /* Glossy.cpp:16-30 */
            f3 sumK = d.Kd + d.Ks;
            float sumScale = 1.f / maxf(maxf(sumK.x, sumK.y), sumK.z);
            if (sumScale < 1.f) {
                d.Kd = d.Kd * sumScale;
                d.Ks = d.Ks * sumScale;
            }
        }
        h.mats[i] = d;
        h.has_tex |= m.type == ORX_MAT_TEXTURE;
    }
    h.lights.resize(s.n_lights);
    for (uint32_t i = 0; i < s.n_lights; i++) h.lights[i] = make_light(s.lights[i]);
    h.media = cfg.enable_media && s.n_media;
    if (h.media) {
        h.med_lo = ld3(s.media);
        h.med_hi = ld3(s.media + 3);
        h.sig_s = s.media[6];
        h.sig_a = s.media[7];
    }
    float max_abs = 0.f; /* of the mesh's coordinates: the box tests' substitute for a zero direction component */
    for (size_t i = 0; s.n_triangles && i < 3 * (size_t)s.n_vertices; i++)
        max_abs = std::max(max_abs, std::fabs(s.vertices[i]));
    h.dir_zero = orx_dir_zero(max_abs);
    /* AAB::getBoundingSphere (math/AAB.cpp:26-33) with Vector3::length's
     * dot bug a.z*b.x (math/Vector3.cpp:27-30) */
    f3 lo = ld3(s.aabb_min), hi = ld3(s.aabb_max);
    h.aabb_lo = lo;
    h.aabb_hi = hi;
    f3 center = (lo + hi) * 0.5f;
    f3 e = hi - center;
    h.bs_cx = center.x;
    h.bs_cy = center.y;
    h.bs_cz = center.z;
    h.bs_r = sqrtf(e.x * e.x + e.y * e.y + e.z * e.x);
    return h;
}

orx_status scene_leaf_arrays(const orx_scene& s, const uint32_t* leaf_order, uint32_t nt, LeafArrays* out,
                             std::string* err) {
    LeafArrays& a = *out;
    a = LeafArrays{};
    const bool has_tb = s.normals && s.tangents && s.bitangents; /* TriangleMesh.cu:56-70 */
    a.v.resize((size_t)nt * 12);
    a.mat.resize(nt);
    if (s.normals) a.n.resize((size_t)nt * 12);
    if (s.texcoords) a.uv.resize((size_t)nt * 6);
    if (has_tb) a.t.resize((size_t)nt * 12), a.bt.resize((size_t)nt * 12);
    /* the next float4 of each array, or null for an array the scene lacks */
    float *pv = a.v.data(), *pn = s.normals ? a.n.data() : nullptr, *puv = s.texcoords ? a.uv.data() : nullptr;
    float *pt = has_tb ? a.t.data() : nullptr, *pbt = has_tb ? a.bt.data() : nullptr;
    auto put4 = [](float*& d, const float* p, float w) {
        d[0] = p[0], d[1] = p[1], d[2] = p[2], d[3] = w;
        d += 4;
    };
    for (uint32_t k = 0; k < nt; k++) {
        const uint32_t i = leaf_order[k];
        if (i >= nt) return refuse(err, ORX_ERR_INVALID_ARGUMENT, "BVH leaf order names a triangle out of range");
        a.mat[k] = s.triangle_material[i];
        for (int v = 0; v < 3; v++) {
            const size_t vi = s.triangles[3 * (size_t)i + v];
            float w = 0.f;
            if (v == 0) std::memcpy(&w, &i, 4);
            put4(pv, s.vertices + 3 * vi, w);
            if (pn) put4(pn, s.normals + 3 * vi, 0.f);
            if (puv) *puv++ = s.texcoords[2 * vi], *puv++ = s.texcoords[2 * vi + 1];
            if (pt) {
                put4(pt, s.tangents + 3 * vi, 0.f);
                put4(pbt, s.bitangents + 3 * vi, 0.f);
            }
        }
    }
    return ORX_OK;
}

TextureLayout scene_texture_layout(const orx_scene& s) {
    TextureLayout L;
    L.rgba.resize(s.n_textures);
    L.normal.resize(s.n_textures);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (uint32_t i = 0; i < s.n_textures; i++) {
        const orx_texture& t = s.textures[i];
        L.rgba[i] = L.total;
        L.total += al((size_t)t.width * t.height * 4);
        L.normal[i] = L.total;
        if (t.normal_rgba) L.total += al((size_t)t.normal_width * t.normal_height * 4);
    }
    return L;
}

}  // namespace orx
