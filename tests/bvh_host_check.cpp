// bvh_host_check.cpp — stand-alone check of the host BVH builder (oppositerenderer_amd/csrc/orx_bvh_host.cpp).
// Built by tests/test_bvh_host.py together with orx_bvh_host.cpp and nothing else (no HIP, no liborx.so), under
// AddressSanitizer + UndefinedBehaviorSanitizer.  It makes its meshes itself with a fixed LCG (bvh_check_common.h,
// shared with the device check), builds each with several option sets and checks the structure of the result: the
// leaves cover every triangle once, the stack bound is the one a walk of the tree gives, every child box (quantised
// and fp32) contains the triangles beneath it, and closest hits through either node array equal a brute-force
// search bit for bit.  The degenerate meshes (deep trees, a zero extent, far from the origin, huge, identical and
// zero-area triangles) get ray sets with zero direction components, cut windows and ties, compared in t, id, beta
// and gamma against the product's triangle formula over all triangles.  Exit status 0: all held.
#include "bvh_check_common.h"
#include "orx_bvh_host.h"

using namespace bvhcheck;

namespace {

/* the one triangle test the searches of the jittered grids use (Moeller-Trumbore, fp32): distance, or INFINITY */
float hit_triangle(const Mesh& m, uint32_t tri, const float* o, const float* d) {
    const float *a = m.vert(tri, 0), *b = m.vert(tri, 1), *c = m.vert(tri, 2);
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.f) return INFINITY;
    const float inv = 1.0f / det;
    const float s[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    const float u = (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]) * inv;
    if (!(u >= 0.f && u <= 1.f)) return INFINITY;
    const float q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
    const float v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) * inv;
    if (!(v >= 0.f && u + v <= 1.f)) return INFINITY;
    const float t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv;
    return t > 0.f ? t : INFINITY;
}

struct Closest {
    float t = INFINITY;
    uint32_t tri = 0xffffffffu;
    void offer(float tt, uint32_t id) {
        if (tt < t) t = tt, tri = id;
    }
};

template <class Node>
Closest trace(const Mesh& m, const HostBvh4& h, const std::vector<Node>& nodes, const float* o, const float* d) {
    Closest best;
    std::vector<uint32_t> stack = {0u};
    while (!stack.empty()) {
        const Node& n = nodes[stack.back()];
        stack.pop_back();
        for (int i = 0; i < 4; i++) {
            const uint32_t ref = n.child[i];
            if (ref == ORX_EMPTY || !hit_box(decode(n, i), o, d)) continue;
            if (!(ref & ORX_LEAF)) {
                stack.push_back(ref);
                continue;
            }
            const uint32_t first = (ref & ~ORX_LEAF) >> 3, count = (ref & 7u) + 1u;
            for (uint32_t k = first; k < first + count; k++) best.offer(hit_triangle(m, h.leaf_order[k], o, d), h.leaf_order[k]);
        }
    }
    return best;
}

struct Rays {
    std::vector<float> o, d;  /* float3 each */
    std::vector<Closest> brute;
};

/* seeded rays from around and above an n x n grid towards points on and a little beside it, and their closest
 * hits by brute force: computed once per mesh, shared by every option set */
Rays make_rays(const Mesh& m, float n, uint32_t count, uint32_t seed) {
    Rays r;
    Lcg g{seed};
    for (uint32_t i = 0; i < count; i++) {
        const float o[3] = {n * (2.f * g.next() - 0.5f), n * (2.f * g.next() - 0.5f), 0.5f + n * g.next()};
        const float p[3] = {n * (1.4f * g.next() - 0.2f), n * (1.4f * g.next() - 0.2f), 0.6f * (g.next() - 0.5f)};
        r.o.insert(r.o.end(), o, o + 3);
        for (int k = 0; k < 3; k++) r.d.push_back(p[k] - o[k]);
        Closest c;
        for (uint32_t t = 0; t < m.nt(); t++) c.offer(hit_triangle(m, t, &r.o[3 * i], &r.d[3 * i]), t);
        r.brute.push_back(c);
    }
    return r;
}

/* build, structure, one summary line; false: nothing to trace through */
bool build_and_walk(const std::string& name, const Mesh& m, const BvhBuildOptions& opt, HostBvh4& h) {
    current = name;
    const char* msg = build_host_bvh4(m.v.data(), m.i.data(), m.nt(), opt, &h);
    CHECK(msg == nullptr, "build failed: %s", msg);
    if (msg) return false;
    if (!check_structure(m, h.nodes, &h.nodes_f, h.leaf_order, h.depth, h.stack_bound, opt.leaf_max)) return false;
    std::printf("%-40s %6u triangles %6zu nodes depth %2u bound %2u\n", name.c_str(), m.nt(), h.nodes.size(), h.depth,
                h.stack_bound);
    return true;
}

void check_case(const std::string& name, const Mesh& m, const BvhBuildOptions& opt, const Rays* rays) {
    HostBvh4 h;
    if (!build_and_walk(name, m, opt, h) || !rays || failures) return;
    const uint32_t nt = m.nt();
    uint32_t hits = 0;
    for (size_t i = 0; i < rays->brute.size(); i++) {
        const float *o = &rays->o[3 * i], *d = &rays->d[3 * i];
        const Closest &b = rays->brute[i], q = trace(m, h, h.nodes, o, d), f = trace(m, h, h.nodes_f, o, d);
        hits += b.t != INFINITY;
        CHECK(same_bits(q.t, b.t), "ray %zu: %a through the quantised nodes, %a by brute force", i, q.t, b.t);
        CHECK(same_bits(f.t, b.t), "ray %zu: %a through the fp32 nodes, %a by brute force", i, f.t, b.t);
        for (const Closest* c : {&q, &f})
            if (c->tri != b.tri && c->tri < nt && b.tri < nt)
                CHECK(same_bits(hit_triangle(m, c->tri, o, d), hit_triangle(m, b.tri, o, d)),
                      "ray %zu: triangle %u, brute force %u, at different distances", i, c->tri, b.tri);
    }
    /* the rays must exercise both outcomes */
    CHECK(hits > rays->brute.size() / 2 && hits < rays->brute.size(), "%u of %zu rays hit", hits, rays->brute.size());
}

/* a degenerate mesh: the ray set through both node arrays against the reference, in t, id, beta and gamma */
void check_degenerate(const std::string& name, const RayCase& c, const BvhBuildOptions& opt, const RaySet* rays) {
    HostBvh4 h;
    if (!build_and_walk(name, c.mesh, opt, h) || !rays || failures) return;
    for (size_t i = 0; i < rays->size(); i++) {
        const float *o = &rays->o[3 * i], *d = &rays->d[3 * i];
        const RefHit& b = rays->closest[i];
        const RefHit q = trace_ref(c.mesh, h.nodes, h.leaf_order, o, d, rays->tmin[i], rays->tmax[i]);
        const RefHit f = trace_ref(c.mesh, h.nodes_f, h.leaf_order, o, d, rays->tmin[i], rays->tmax[i]);
        CHECK(same_hit(q, b), "ray %zu: t %a triangle %u through the quantised nodes, t %a triangle %u by brute force", i,
              q.t, q.tri, b.t, b.tri);
        CHECK(same_hit(f, b), "ray %zu: t %a triangle %u through the fp32 nodes, t %a triangle %u by brute force", i, f.t,
              f.tri, b.t, b.tri);
    }
}

}  // namespace

int main() {
    const BvhBuildOptions defaults;
    CHECK(defaults.bins == 32 && defaults.leaf_max == 8 && defaults.leaf_sah == 0.6f && defaults.treelet_passes == 3 &&
              defaults.treelet_leaves == 9 && defaults.sah_collapse,
          "BvhBuildOptions defaults changed");
    const std::vector<NamedOptions> sets = option_sets();

    struct Case {
        std::string name;
        Mesh mesh;
        float extent; /* > 0: trace rays over [0, extent]^2 */
    };
    std::vector<Case> cases;
    cases.push_back({"one triangle", repeated_triangle(1), 0.f});
    /* zero centroid extent and more than leaf_max of them: the object-median path */
    cases.push_back({"nine identical triangles", repeated_triangle(9), 0.f});
    for (uint32_t n : {1u, 3u, 12u, 48u})
        cases.push_back({"grid" + std::to_string(n), jittered_grid(n, 0x9e3779b9u + n), n >= 12 ? (float)n : 0.f});
    for (const Case& c : cases) {
        Rays rays;
        if (c.extent > 0.f) rays = make_rays(c.mesh, c.extent, 2000, 0x2545f491u);
        for (const NamedOptions& s : sets) check_case(c.name + ", " + s.name, c.mesh, s.opt, c.extent > 0.f ? &rays : nullptr);
    }
    /* at the median-split cap of the binary build, without the treelet sweeps (with them, and with every other
     * option set: among the geometric meshes below) */
    check_case("geometric 1.003, " + std::string(sets[2].name), geometric(20000, 1.003), sets[2].opt, nullptr);

    /* the degenerate meshes.  The geometric ones are the trees the treelet sweeps used to deepen past
     * ORX_BVH_STACK: every option set, the defaults included, must build them below the cap. */
    for (const RayCase& c : degenerate_cases()) {
        RaySet rays;
        current = c.name;
        if (c.rays) {
            rays = make_ray_set(c.mesh, RAYS_PER_SET, 0x2545f491u);
            check_hit_share(c, rays);
        }
        for (const NamedOptions& s : sets) check_degenerate(c.name + ", " + s.name, c, s.opt, c.rays ? &rays : nullptr);
    }

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
