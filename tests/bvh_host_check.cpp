// bvh_host_check.cpp — stand-alone check of the host BVH builder (oppositerenderer_amd/csrc/orx_bvh_host.cpp).
// Built by tests/test_bvh_host.py together with orx_bvh_host.cpp and nothing else (no HIP, no liborx.so), under
// AddressSanitizer + UndefinedBehaviorSanitizer.  It makes its meshes itself with a fixed LCG, builds each with
// several option sets and checks the structure of the result: the leaves cover every triangle once, the stack
// bound is the one a walk of the tree gives, every child box (quantised and fp32) contains the triangles beneath
// it, and closest hits through either node array equal a brute-force search bit for bit.  Exit status 0: all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "orx_bvh_host.h"

using namespace orx;

namespace {

int failures = 0;
std::string current;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (failures++ < 20) {                            \
                std::printf("FAIL [%s] ", current.c_str());   \
                std::printf(__VA_ARGS__);                     \
                std::printf(" (%s)\n", #cond);                \
            }                                                 \
        }                                                     \
    } while (0)

struct Lcg {
    uint32_t s;
    float next() { /* [0, 1) */
        s = s * 1664525u + 1013904223u;
        return (float)(s >> 8) * (1.0f / 16777216.0f);
    }
};

struct Mesh {
    std::vector<float> v;    /* float3 per vertex */
    std::vector<uint32_t> i; /* three per triangle */
    uint32_t nt() const { return (uint32_t)(i.size() / 3); }
    const float* vert(uint32_t tri, int k) const { return &v[3 * (size_t)i[3 * (size_t)tri + k]]; }
};

Mesh repeated_triangle(uint32_t copies) {
    Mesh m;
    m.v = {0.f, 0.f, 0.f, 1.f, 0.f, 0.25f, 0.f, 1.f, 0.5f};
    for (uint32_t c = 0; c < copies; c++) m.i.insert(m.i.end(), {0u, 1u, 2u});
    return m;
}

/* n x n cells on [0, n]^2, every vertex jittered in x, y and height: 2 n^2 triangles.  The columns widen with x
 * (fivefold from first to last), so that the best SAH split is not the middle one whatever the number of bins. */
Mesh jittered_grid(uint32_t n, uint32_t seed) {
    Mesh m;
    Lcg r{seed};
    for (uint32_t y = 0; y <= n; y++)
        for (uint32_t x = 0; x <= n; x++) {
            const float u = (float)x / (float)n, width = (0.5f + 2.f * u) / 1.5f;
            m.v.push_back((float)x * (0.5f + u) / 1.5f + 0.35f * width * (r.next() - 0.5f));
            m.v.push_back((float)y + 0.35f * (r.next() - 0.5f));
            m.v.push_back(0.6f * (r.next() - 0.5f));
        }
    for (uint32_t y = 0; y < n; y++)
        for (uint32_t x = 0; x < n; x++) {
            const uint32_t a = y * (n + 1) + x, b = a + 1, c = a + n + 1, d = c + 1;
            m.i.insert(m.i.end(), {a, b, d, a, d, c});
        }
    return m;
}

/* triangle k at scale s = growth^k: every SAH split peels a few triangles off one end, so the binary build runs
 * into its depth cap and finishes with object-median splits */
Mesh geometric(uint32_t nt, double growth) {
    Mesh m;
    double s = 1.0;
    for (uint32_t k = 0; k < nt; k++, s *= growth) {
        const float f = (float)s, g = (float)(1.01 * s), h = (float)(0.01 * s);
        const float p[9] = {f, 0.f, 0.f, g, 0.f, 0.f, f, h, 0.f};
        m.v.insert(m.v.end(), p, p + 9);
        m.i.insert(m.i.end(), {3 * k, 3 * k + 1, 3 * k + 2});
    }
    return m;
}

struct Box {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void add(const float* p) {
        for (int k = 0; k < 3; k++) lo[k] = std::fmin(lo[k], p[k]), hi[k] = std::fmax(hi[k], p[k]);
    }
    void add(const Box& b) { add(b.lo), add(b.hi); }
    bool inside(const Box& outer) const {
        for (int k = 0; k < 3; k++)
            if (!(outer.lo[k] <= lo[k] && hi[k] <= outer.hi[k])) return false;
        return true;
    }
};

/* child i of a quantised node: origin + q * scale, the decode of the traversal kernels (q * scale is exact) */
Box decode(const DevBvh4& n, int i) {
    const float o[3] = {n.ox, n.oy, n.oz}, s[3] = {n.sx, n.sy, n.sz};
    Box b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = o[k] + (float)((n.qlo[k] >> (8 * i)) & 0xffu) * s[k];
        b.hi[k] = o[k] + (float)((n.qhi[k] >> (8 * i)) & 0xffu) * s[k];
    }
    return b;
}
Box decode(const DevBvh4F& n, int i) {
    Box b;
    for (int k = 0; k < 3; k++) b.lo[k] = n.b[2 * k][i], b.hi[k] = n.b[2 * k + 1][i];
    return b;
}

struct Walk {
    const Mesh& m;
    const HostBvh4& h;
    uint32_t leaf_max;
    std::vector<uint32_t> covered; /* per leaf-order slot: leaves that hold it */
    std::vector<uint8_t> seen;     /* per node */

    /* the exact box of the triangles beneath `node`; bound = the stack entries a traversal of it can hold */
    Box visit(uint32_t node, uint32_t depth4, uint32_t& bound) {
        Box all;
        bound = 0;
        CHECK(node < h.nodes.size(), "node %u out of range", node);
        if (node >= h.nodes.size()) return all;
        CHECK(!seen[node], "node %u reached twice", node);
        if (seen[node]) return all;
        seen[node] = 1;
        CHECK(depth4 <= h.depth, "four-wide depth %u above the binary depth %u", depth4, h.depth);
        const DevBvh4& q = h.nodes[node];
        const DevBvh4F& f = h.nodes_f[node];
        uint32_t children = 0, sub = 0;
        for (int i = 0; i < 4; i++) {
            const uint32_t ref = q.child[i];
            CHECK(f.child[i] == ref, "node %u child %d: %08x in nodes, %08x in nodes_f", node, i, ref, f.child[i]);
            if (ref == ORX_EMPTY) {
                for (int k = 0; k < 3; k++)
                    CHECK(((q.qlo[k] >> (8 * i)) & 0xffu) == 255u && ((q.qhi[k] >> (8 * i)) & 0xffu) == 0u,
                          "node %u empty slot %d axis %d is not the empty box", node, i, k);
                continue;
            }
            children++;
            Box under;
            if (ref & ORX_LEAF) {
                const uint32_t first = (ref & ~ORX_LEAF) >> 3, count = (ref & 7u) + 1u;
                CHECK(count >= 1 && count <= leaf_max, "node %u leaf of %u triangles, leaf_max %u", node, count, leaf_max);
                CHECK((uint64_t)first + count <= m.nt(), "node %u leaf range %u + %u past %u", node, first, count, m.nt());
                for (uint32_t k = first; k < first + count && k < m.nt(); k++) {
                    covered[k]++;
                    const uint32_t tri = h.leaf_order[k];
                    if (tri < m.nt())
                        for (int v = 0; v < 3; v++) under.add(m.vert(tri, v));
                }
            } else {
                uint32_t b = 0;
                under = visit(ref, depth4 + 1, b);
                sub = b > sub ? b : sub;
            }
            CHECK(under.inside(decode(q, i)), "node %u child %d: quantised box misses a vertex beneath it", node, i);
            CHECK(under.inside(decode(f, i)), "node %u child %d: fp32 box misses a vertex beneath it", node, i);
            all.add(under);
        }
        CHECK(children >= 1, "node %u has no children", node);
        bound = (children ? children - 1u : 0u) + sub;
        return all;
    }
};

/* the one triangle test every search below uses (Moeller-Trumbore, fp32): distance, or INFINITY */
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

/* does the ray o + t d, t >= 0, meet the box?  In double, so that this test never culls by its own rounding. */
bool hit_box(const Box& b, const float* o, const float* d) {
    double t0 = 0.0, t1 = INFINITY;
    for (int k = 0; k < 3; k++) {
        if (d[k] == 0.f) {
            if (o[k] < b.lo[k] || o[k] > b.hi[k]) return false;
            continue;
        }
        double n = ((double)b.lo[k] - o[k]) / d[k], f = ((double)b.hi[k] - o[k]) / d[k];
        if (n > f) std::swap(n, f);
        t0 = n > t0 ? n : t0;
        t1 = f < t1 ? f : t1;
    }
    return t0 <= t1;
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

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

void check_case(const std::string& name, const Mesh& m, const BvhBuildOptions& opt, const Rays* rays) {
    current = name;
    HostBvh4 h;
    const char* msg = build_host_bvh4(m.v.data(), m.i.data(), m.nt(), opt, &h);
    CHECK(msg == nullptr, "build failed: %s", msg);
    if (msg) return;
    const uint32_t nt = m.nt();
    CHECK(h.leaf_order.size() == nt, "leaf_order has %zu entries for %u triangles", h.leaf_order.size(), nt);
    CHECK(!h.nodes.empty() && h.nodes.size() == h.nodes_f.size(), "%zu nodes, %zu fp32 nodes", h.nodes.size(),
          h.nodes_f.size());
    if (h.leaf_order.size() != nt || h.nodes.empty() || h.nodes.size() != h.nodes_f.size()) return;
    std::vector<uint32_t> times(nt, 0);
    for (uint32_t id : h.leaf_order) {
        CHECK(id < nt, "leaf_order holds %u", id);
        if (id < nt) times[id]++;
    }
    for (uint32_t t = 0; t < nt; t++) CHECK(times[t] == 1, "triangle %u is %u times in leaf_order", t, times[t]);
    CHECK(h.depth < ORX_BVH_STACK, "depth %u", h.depth);
    CHECK(h.stack_bound <= 96, "stack bound %u", h.stack_bound);

    Walk w{m, h, opt.leaf_max, std::vector<uint32_t>(nt, 0), std::vector<uint8_t>(h.nodes.size(), 0)};
    uint32_t bound = 0;
    w.visit(0, 0, bound);
    CHECK(bound == h.stack_bound, "stack bound %u, a walk of the tree gives %u", h.stack_bound, bound);
    for (uint32_t k = 0; k < nt; k++) CHECK(w.covered[k] == 1, "leaf-order slot %u is in %u leaves", k, w.covered[k]);
    for (size_t n = 0; n < h.nodes.size(); n++) CHECK(w.seen[n], "node %zu is unreachable", n);
    std::printf("%-40s %6u triangles %6zu nodes depth %2u bound %2u\n", name.c_str(), nt, h.nodes.size(), h.depth,
                h.stack_bound);
    if (!rays || failures) return;

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

}  // namespace

int main() {
    const BvhBuildOptions defaults;
    CHECK(defaults.bins == 32 && defaults.leaf_max == 8 && defaults.leaf_sah == 0.6f && defaults.treelet_passes == 3 &&
              defaults.treelet_leaves == 9 && defaults.sah_collapse,
          "BvhBuildOptions defaults changed");
    struct Named {
        const char* name;
        BvhBuildOptions opt;
    };
    std::vector<Named> sets(5);
    sets[0].name = "defaults";
    sets[1].name = "treelet_leaves=7";
    sets[1].opt.treelet_leaves = 7;
    sets[2].name = "no treelets, no sah collapse";
    sets[2].opt.treelet_passes = 0;
    sets[2].opt.sah_collapse = false;
    sets[3].name = "leaf_sah=0 leaf_max=4";
    sets[3].opt.leaf_sah = 0.f;
    sets[3].opt.leaf_max = 4;
    sets[4].name = "bins=8";
    sets[4].opt.bins = 8;

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
        for (const Named& s : sets) check_case(c.name + ", " + s.name, c.mesh, s.opt, c.extent > 0.f ? &rays : nullptr);
    }
    /* at the median-split cap of the binary build.  Only without the treelet sweeps: with them the tree grows
     * past ORX_BVH_STACK and the build is rejected (known issue), which is not asserted here. */
    check_case("geometric 1.003, " + std::string(sets[2].name), geometric(20000, 1.003), sets[2].opt, nullptr);

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
