// scene_host_check.cpp — stand-alone check of scene preparation on the host (oppositerenderer_amd/csrc/orx_scene_host.cpp).
// Built by tests/test_scene_host.py together with orx_scene_host.cpp and nothing else (no HIP, no liborx.so), under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Every input array is a heap block of exactly its stated size, so a
// read past an array is a sanitizer report.  It checks:
//   1. conversions whose results are exactly representable, bit for bit against constants: the parallelogram's plane
//      and scaled edges, the area light's area, the point light's intensity, the Glossy normalisation, the emitter's
//      power per area, the bounding sphere with the reference's z*x term;
//   2. every refusal of scene_validate, by status and exact message, one broken field at a time from one valid scene,
//      and that the valid scene passes;
//   3. the triangle attributes in leaf order, with and without normals, texcoords and tangents, and a leaf order
//      that names a triangle out of range;
//   4. the 256-byte-aligned texture layout.
// Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "orx_scene_host.h"

using namespace orx;

namespace {

int failures = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                                  \
        }                                                                \
    } while (0)

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
bool same(float a, float b) { return bits(a) == bits(b); }
bool same3(f3 a, float x, float y, float z) { return same(a.x, x) && same(a.y, y) && same(a.z, z); }

/* heap blocks of exactly the bytes asked for, freed with the scene */
struct Heap {
    std::vector<void*> blocks;
    ~Heap() {
        for (void* p : blocks) std::free(p);
    }
    template <class T>
    T* dup(std::initializer_list<T> v) {
        T* p = static_cast<T*>(std::malloc(v.size() * sizeof(T)));
        std::copy(v.begin(), v.end(), p);
        blocks.push_back(p);
        return p;
    }
    template <class T>
    T* zeros(size_t n) {
        T* p = static_cast<T*>(std::calloc(n, sizeof(T)));
        blocks.push_back(p);
        return p;
    }
};

orx_material material(int32_t type, float kd, float ks) {
    orx_material m;
    std::memset(&m, 0, sizeof m);
    m.type = type;
    for (int k = 0; k < 3; k++) m.Kd[k] = kd, m.Ks[k] = ks;
    m.texture = -1;
    return m;
}

/* the valid scene: 1 quad, 1 sphere, 2 triangles over 4 vertices, 1 texture, 6 materials of the six types, an area
 * and a point light, one medium box; the mutable pointers are the scene's own arrays */
struct TestScene {
    Heap heap;
    orx_scene s;
    uint32_t *qmat, *smat, *tris, *tmat;
    orx_material* mats;
    orx_texture* tex;
    float* media;
    TestScene() {
        std::memset(&s, 0, sizeof s);
        s.n_quads = 1;
        s.quads = heap.dup<float>({1, 2, 3, 2, 0, 0, 0, 0, 4});
        s.quad_material = qmat = heap.dup<uint32_t>({0});
        s.n_spheres = 1;
        s.spheres = heap.dup<float>({1, 1, 1, 0.5f});
        s.sphere_material = smat = heap.dup<uint32_t>({2});
        s.n_vertices = 4;
        s.vertices = heap.dup<float>({0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3});
        s.n_triangles = 2;
        s.triangles = tris = heap.dup<uint32_t>({0, 1, 2, 1, 2, 3});
        s.triangle_material = tmat = heap.dup<uint32_t>({5, 4});
        s.n_materials = 6;
        mats = heap.zeros<orx_material>(6);
        for (int32_t t = 0; t < 6; t++) mats[t] = material(t, 1.f, 1.f);
        orx_material& em = mats[ORX_MAT_DIFFUSE_EMITTER];
        em.Kd[0] = em.Kd[1] = em.Kd[2] = 0.5f;
        em.power[0] = 2, em.power[1] = 4, em.power[2] = 8;
        em.inverse_area = 0.5f;
        mats[ORX_MAT_TEXTURE].texture = 0;
        s.materials = mats;
        s.n_lights = 2;
        orx_light* lights = heap.zeros<orx_light>(2);
        lights[0].type = ORX_LIGHT_AREA;
        lights[0].power[0] = lights[0].power[1] = lights[0].power[2] = 16;
        lights[0].position[0] = 1, lights[0].position[1] = 2, lights[0].position[2] = 3;
        lights[0].v1[0] = 2;
        lights[0].v2[2] = 4;
        lights[1].type = ORX_LIGHT_POINT;
        lights[1].power[0] = 4, lights[1].power[1] = 8, lights[1].power[2] = 16;
        s.lights = lights;
        s.aabb_max[0] = 4, s.aabb_max[1] = 4, s.aabb_max[2] = 8;
        s.n_textures = 1;
        tex = heap.zeros<orx_texture>(1);
        tex[0].width = 2, tex[0].height = 1;
        tex[0].rgba = heap.zeros<uint8_t>(8);
        s.textures = tex;
        s.n_media = 1;
        s.media = media = heap.dup<float>({0, 0, 0, 1, 2, 3, 0.5f, 0.25f});
    }
};

orx_config config(uint32_t enable_media) {
    orx_config c;
    std::memset(&c, 0, sizeof c);
    c.enable_media = enable_media;
    c.volumetric_photons = 1000;
    return c;
}

/* one refusal: the valid scene with `breakit` applied must give `want` and exactly `msg` */
void refused(const char* what, orx_status want, const char* msg, const std::function<void(TestScene&)>& breakit,
             orx_config cfg = config(1), uint32_t world = 1) {
    TestScene t;
    breakit(t);
    std::string err = "untouched";
    const orx_status st = scene_validate(&t.s, cfg, world, &err);
    if (st != want || err != msg) {
        std::printf("FAILED refusal '%s': status %d, message '%s' (wanted %d, '%s')\n", what, (int)st, err.c_str(),
                    (int)want, msg);
        failures++;
    }
}

void check_validate() {
    {
        TestScene t;
        std::string err = "untouched";
        CHECK(scene_validate(&t.s, config(1), 1, &err) == ORX_OK && err == "untouched");
        CHECK(scene_validate(&t.s, config(0), 4, &err) == ORX_OK); /* no media: any world */
        CHECK(scene_validate(nullptr, config(0), 1, &err) == ORX_ERR_INVALID_ARGUMENT);
    }
    const orx_status INV = ORX_ERR_INVALID_ARGUMENT, UNS = ORX_ERR_UNSUPPORTED;
    refused("no lights", ORX_ERR_NO_LIGHTS, "No lights exists in this scene.", [](TestScene& t) { t.s.n_lights = 0; });
    refused("lights NULL", ORX_ERR_NO_LIGHTS, "No lights exists in this scene.", [](TestScene& t) { t.s.lights = nullptr; });
    refused("no materials", INV, "scene has no materials", [](TestScene& t) { t.s.n_materials = 0; });
    refused("materials NULL", INV, "scene has no materials", [](TestScene& t) { t.s.materials = nullptr; });
    refused("quad material", INV, "quad material out of range", [](TestScene& t) { t.qmat[0] = 6; });
    refused("sphere material", INV, "sphere material out of range", [](TestScene& t) { t.smat[0] = 6; });
    refused("triangle material", INV, "triangle material out of range", [](TestScene& t) { t.tmat[1] = 6; });
    refused("vertex index", INV, "triangle vertex index out of range", [](TestScene& t) { t.tris[5] = 4; });
    refused("texture without texels", INV, "texture image without texels", [](TestScene& t) { t.tex[0].rgba = nullptr; });
    refused("texture of width 0", INV, "texture image without texels", [](TestScene& t) { t.tex[0].width = 0; });
    refused("normal map of width 0", INV, "texture image without texels", [](TestScene& t) {
        t.tex[0].normal_rgba = t.heap.zeros<uint8_t>(4);
        t.tex[0].normal_height = 1;
    });
    refused("normal map of height 0", INV, "texture image without texels", [](TestScene& t) {
        t.tex[0].normal_rgba = t.heap.zeros<uint8_t>(4);
        t.tex[0].normal_width = 1;
    });
    refused("Texture material, index -1", INV, "Texture material without a texture image",
            [](TestScene& t) { t.mats[5].texture = -1; });
    refused("Texture material, index n_textures", INV, "Texture material without a texture image",
            [](TestScene& t) { t.mats[5].texture = 1; });
    refused("material type -1", INV, "unknown material type", [](TestScene& t) { t.mats[0].type = -1; });
    refused("material type 6", INV, "unknown material type", [](TestScene& t) { t.mats[3].type = 6; });
    /* the count alone: no triangle array is looked at */
    refused("2^26 triangles", UNS, "more than 2^26 triangles", [](TestScene& t) {
        t.s.n_triangles = 1u << 26;
        t.s.triangles = t.s.triangle_material = nullptr;
    });
    /* media */
    const char* one_box = "participating media: one medium box per scene";
    const char* box = "medium box: min < max and sigma_s + sigma_a > 0";
    refused("two medium boxes", UNS, one_box, [](TestScene& t) { t.s.n_media = 2; });
    refused("media NULL", UNS, one_box, [](TestScene& t) { t.s.media = nullptr; });
    refused("medium box min == max", INV, box, [](TestScene& t) { t.media[4] = t.media[1]; });
    refused("medium sigma_s < 0", INV, box, [](TestScene& t) { t.media[6] = -0.5f; });
    refused("medium sigma sum 0", INV, box, [](TestScene& t) { t.media[6] = t.media[7] = 0.f; });
    {
        orx_config c = config(1);
        c.volumetric_photons = 0;
        refused("no volumetric photons", INV, "volumetric_photons must be > 0 with media", [](TestScene&) {}, c);
    }
    refused("media on a shard", UNS, "participating media are single-device", [](TestScene&) {}, config(1), 2);
    {
        TestScene t; /* enable_media off: the medium array is not looked at */
        t.s.n_media = 2;
        t.s.media = nullptr;
        std::string err;
        CHECK(scene_validate(&t.s, config(0), 1, &err) == ORX_OK);
    }
    /* arrays whose count is non-zero */
    refused("quads NULL", INV, "scene array quads is NULL", [](TestScene& t) { t.s.quads = nullptr; });
    refused("quad_material NULL", INV, "scene array quad_material is NULL", [](TestScene& t) { t.s.quad_material = nullptr; });
    refused("spheres NULL", INV, "scene array spheres is NULL", [](TestScene& t) { t.s.spheres = nullptr; });
    refused("sphere_material NULL", INV, "scene array sphere_material is NULL",
            [](TestScene& t) { t.s.sphere_material = nullptr; });
    refused("textures NULL", INV, "scene array textures is NULL", [](TestScene& t) { t.s.textures = nullptr; });
    refused("vertices NULL", INV, "scene array vertices is NULL", [](TestScene& t) { t.s.vertices = nullptr; });
    refused("triangles NULL", INV, "scene array triangles is NULL", [](TestScene& t) { t.s.triangles = nullptr; });
    refused("triangle_material NULL", INV, "scene array triangle_material is NULL",
            [](TestScene& t) { t.s.triangle_material = nullptr; });
    {
        TestScene t; /* a count of zero asks for no array */
        t.s.n_quads = t.s.n_spheres = t.s.n_triangles = t.s.n_vertices = t.s.n_textures = 0;
        t.s.quads = t.s.spheres = t.s.vertices = nullptr;
        t.s.quad_material = t.s.sphere_material = t.s.triangles = t.s.triangle_material = nullptr;
        t.s.textures = nullptr;
        t.mats[5].type = ORX_MAT_DIFFUSE;
        std::string err;
        CHECK(scene_validate(&t.s, config(1), 1, &err) == ORX_OK);
        const HostScene h = scene_prepare(t.s, config(1));
        CHECK(h.quads.empty() && h.spheres.empty() && h.mats.size() == 6 && !h.has_tex);
        CHECK(same(h.dir_zero, 1e-30f));
    }
}

void check_prepare() {
    TestScene t;
    const HostScene h = scene_prepare(t.s, config(1));
    CHECK(h.quads.size() == 1 && h.spheres.size() == 1 && h.mats.size() == 6 && h.lights.size() == 2);
    /* parallelogram: anchor (1,2,3), offsets (2,0,0) and (0,0,4) */
    const DevQuad& q = h.quads[0];
    CHECK(same(q.nx, 0.f) && same(q.ny, -1.f) && same(q.nz, 0.f) && same(q.d, -2.f));
    CHECK(same(q.ax, 1.f) && same(q.ay, 2.f) && same(q.az, 3.f));
    CHECK(same(q.v1x, 0.5f) && same(q.v1y, 0.f) && same(q.v1z, 0.f));
    CHECK(same(q.v2x, 0.f) && same(q.v2y, 0.f) && same(q.v2z, 0.25f));
    CHECK(same(q.pad0, 0.f) && same(q.pad1, 0.f) && same(q.pad2, 0.f));
    const DevSphere& sp = h.spheres[0];
    CHECK(same(sp.cx, 1.f) && same(sp.cy, 1.f) && same(sp.cz, 1.f) && same(sp.r, 0.5f));
    /* area light with the same edges */
    const DevLight& la = h.lights[0];
    CHECK(la.type == LIGHT_AREA && same(la.area, 8.f) && same(la.inverseArea, 0.125f));
    CHECK(same3(la.normal, 0.f, -1.f, 0.f) && same3(la.position, 1.f, 2.f, 3.f));
    CHECK(same3(la.v1, 2.f, 0.f, 0.f) && same3(la.v2, 0.f, 0.f, 4.f));
    CHECK(same3(la.Lemit, (16.f * 0.125f) * ORX_1_PI_F, (16.f * 0.125f) * ORX_1_PI_F, (16.f * 0.125f) * ORX_1_PI_F));
    /* point light, power (4,8,16) */
    const DevLight& lp = h.lights[1];
    CHECK(lp.type == LIGHT_POINT);
    CHECK(same3(lp.Lemit, (4.f * 0.25f) * ORX_1_PI_F, (8.f * 0.25f) * ORX_1_PI_F, (16.f * 0.25f) * ORX_1_PI_F));
    CHECK(same(lp.area, 0.f) && same(lp.inverseArea, 0.f));
    /* materials */
    for (int32_t k = 0; k < 6; k++) CHECK(h.mats[k].type == k);
    const DevMaterial& em = h.mats[MAT_EMITTER];
    CHECK(same3(em.powerPerArea, 0.5f, 1.f, 2.f) && same(em.inverseArea, 0.5f));
    CHECK(same3(em.Lemit, 0.5f * ORX_1_PI_F, 1.f * ORX_1_PI_F, 2.f * ORX_1_PI_F));
    const DevMaterial& gl = h.mats[MAT_GLOSSY]; /* Kd = Ks = 1: both halved */
    CHECK(same3(gl.Kd, 0.5f, 0.5f, 0.5f) && same3(gl.Ks, 0.5f, 0.5f, 0.5f));
    CHECK(same3(h.mats[MAT_DIFFUSE].Kd, 1.f, 1.f, 1.f)); /* only Glossy is normalised */
    CHECK(h.mats[MAT_TEXTURE].tex == 0 && h.has_tex);
    {
        TestScene u; /* Kd = Ks = 0.25: the sum is below 1, both unchanged */
        u.mats[MAT_GLOSSY] = material(ORX_MAT_GLOSSY, 0.25f, 0.25f);
        const HostScene g = scene_prepare(u.s, config(0));
        CHECK(same3(g.mats[MAT_GLOSSY].Kd, 0.25f, 0.25f, 0.25f) && same3(g.mats[MAT_GLOSSY].Ks, 0.25f, 0.25f, 0.25f));
        CHECK(!g.media);
    }
    /* AABB (0,0,0)-(4,4,8): 16 = 4 + 4 + 4*2 with the reference's e.z * e.x; e.z * e.z would give sqrt(24) */
    CHECK(same(h.bs_cx, 2.f) && same(h.bs_cy, 2.f) && same(h.bs_cz, 4.f) && same(h.bs_r, 4.f));
    CHECK(same3(h.aabb_lo, 0.f, 0.f, 0.f) && same3(h.aabb_hi, 4.f, 4.f, 8.f));
    CHECK(same(h.dir_zero, 1e-30f));
    CHECK(h.media && same3(h.med_lo, 0.f, 0.f, 0.f) && same3(h.med_hi, 1.f, 2.f, 3.f));
    CHECK(same(h.sig_s, 0.5f) && same(h.sig_a, 0.25f));
}

/* 3 triangles over 4 vertices in leaf order {2,0,1}; attribute a of vertex v, component c is 100 a + 10 v + c */
void check_leaf_arrays() {
    Heap heap;
    auto attr = [&](int a, int comps) {
        float* p = heap.zeros<float>(4 * (size_t)comps);
        for (int v = 0; v < 4; v++)
            for (int c = 0; c < comps; c++) p[comps * v + c] = (float)(100 * a + 10 * v + c);
        return p;
    };
    orx_scene s;
    std::memset(&s, 0, sizeof s);
    s.n_vertices = 4;
    s.vertices = attr(0, 3);
    s.n_triangles = 3;
    const uint32_t tri[9] = {0, 1, 2, 1, 2, 3, 3, 0, 2};
    s.triangles = heap.dup<uint32_t>({0, 1, 2, 1, 2, 3, 3, 0, 2});
    s.triangle_material = heap.dup<uint32_t>({7, 8, 9});
    const float *normals = attr(1, 3), *uv = attr(2, 2), *tan = attr(3, 3), *bitan = attr(4, 3);
    const uint32_t* order = heap.dup<uint32_t>({2, 0, 1});
    auto holds = [&](const std::vector<float>& out, int a, int comps, bool ids) {
        if (out.size() != (size_t)9 * (comps == 2 ? 2 : 4)) return false;
        const size_t stride = comps == 2 ? 2 : 4;
        for (uint32_t k = 0; k < 3; k++)
            for (int v = 0; v < 3; v++) {
                const float* o = out.data() + stride * (3 * k + v);
                const uint32_t vi = tri[3 * order[k] + v];
                for (int c = 0; c < comps; c++)
                    if (!same(o[c], (float)(100 * a + 10 * vi + c))) return false;
                if (comps == 3 && bits(o[3]) != (ids && v == 0 ? order[k] : 0u)) return false;
            }
        return true;
    };
    for (int variant = 0; variant < 4; variant++) {
        s.normals = variant & 1 ? normals : nullptr;
        s.texcoords = variant & 2 ? uv : nullptr;
        s.tangents = s.bitangents = nullptr;
        LeafArrays la;
        std::string err = "untouched";
        CHECK(scene_leaf_arrays(s, order, 3, &la, &err) == ORX_OK && err == "untouched");
        CHECK(holds(la.v, 0, 3, true));
        CHECK(la.mat.size() == 3 && la.mat[0] == 9 && la.mat[1] == 7 && la.mat[2] == 8);
        CHECK(s.normals ? holds(la.n, 1, 3, false) : la.n.empty());
        CHECK(s.texcoords ? holds(la.uv, 2, 2, false) : la.uv.empty());
        CHECK(la.t.empty() && la.bt.empty());
    }
    {
        LeafArrays la;
        std::string err;
        s.normals = normals;
        s.texcoords = uv;
        s.tangents = tan;
        s.bitangents = nullptr; /* tangents without bitangents: neither array */
        CHECK(scene_leaf_arrays(s, order, 3, &la, &err) == ORX_OK && la.t.empty() && la.bt.empty());
        s.bitangents = bitan;
        CHECK(scene_leaf_arrays(s, order, 3, &la, &err) == ORX_OK);
        CHECK(holds(la.t, 3, 3, false) && holds(la.bt, 4, 3, false) && holds(la.n, 1, 3, false));
        s.normals = nullptr; /* hasTangentsAndBitangents needs the normals too */
        CHECK(scene_leaf_arrays(s, order, 3, &la, &err) == ORX_OK && la.t.empty() && la.bt.empty() && la.n.empty());
    }
    {
        const uint32_t* bad = heap.dup<uint32_t>({0, 3, 1});
        LeafArrays la;
        std::string err;
        CHECK(scene_leaf_arrays(s, bad, 3, &la, &err) == ORX_ERR_INVALID_ARGUMENT);
        CHECK(err == "BVH leaf order names a triangle out of range");
    }
    {
        LeafArrays la; /* no triangles: nothing is read */
        std::string err;
        orx_scene e;
        std::memset(&e, 0, sizeof e);
        CHECK(scene_leaf_arrays(e, nullptr, 0, &la, &err) == ORX_OK && la.v.empty() && la.mat.empty());
    }
}

void check_texture_layout() {
    Heap heap;
    orx_texture* tex = heap.zeros<orx_texture>(2);
    tex[0].width = 3, tex[0].height = 5;
    tex[0].rgba = heap.zeros<uint8_t>(3 * 5 * 4);
    tex[1].width = 1, tex[1].height = 1;
    tex[1].rgba = heap.zeros<uint8_t>(4);
    tex[1].normal_width = 2, tex[1].normal_height = 2;
    tex[1].normal_rgba = heap.zeros<uint8_t>(2 * 2 * 4);
    orx_scene s;
    std::memset(&s, 0, sizeof s);
    s.n_textures = 2;
    s.textures = tex;
    const TextureLayout L = scene_texture_layout(s);
    CHECK(L.rgba.size() == 2 && L.normal.size() == 2);
    CHECK(L.rgba[0] == 0 && L.rgba[1] == 256 && L.normal[1] == 512 && L.total == 768);
    s.n_textures = 0;
    s.textures = nullptr;
    CHECK(scene_texture_layout(s).total == 0);
}

}  // namespace

int main() {
    check_validate();
    check_prepare();
    check_leaf_arrays();
    check_texture_layout();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
