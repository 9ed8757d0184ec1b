// bvh_check_common.h — what the stand-alone BVH checks share: tests/bvh_host_check.cpp (the host builder, on the
// CPU under sanitizers) and tests/bvh_device_check.hip (the device builder and the traversal loops, on the GPU).
// Meshes and ray sets from a fixed LCG, the structure walk of a four-wide tree, and the reference every closest
// hit is compared with bit for bit: a brute-force search over all triangles in original order with the product's
// own triangle formula (isect_tri, orx_isect.h) restated in plain fp32 C++.  Build with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "orx_bvh_nodes.h"

namespace bvhcheck {

using namespace orx;

inline int failures = 0;
inline std::string current;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (bvhcheck::failures++ < 20) {                  \
                std::printf("FAIL [%s] ", bvhcheck::current.c_str()); \
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
    uint32_t below(uint32_t n) { /* [0, n) */
        s = s * 1664525u + 1013904223u;
        return (uint32_t)(((uint64_t)(s >> 8) * n) >> 24);
    }
};

struct Mesh {
    std::vector<float> v;    /* float3 per vertex */
    std::vector<uint32_t> i; /* three per triangle */
    uint32_t nt() const { return (uint32_t)(i.size() / 3); }
    const float* vert(uint32_t tri, int k) const { return &v[3 * (size_t)i[3 * (size_t)tri + k]]; }
};

inline Mesh repeated_triangle(uint32_t copies) {
    Mesh m;
    m.v = {0.f, 0.f, 0.f, 1.f, 0.f, 0.25f, 0.f, 1.f, 0.5f};
    for (uint32_t c = 0; c < copies; c++) m.i.insert(m.i.end(), {0u, 1u, 2u});
    return m;
}

/* n x n cells on [0, n]^2, every vertex jittered in x, y and height: 2 n^2 triangles.  The columns widen with x
 * (fivefold from first to last), so that the best SAH split is not the middle one whatever the number of bins. */
inline Mesh jittered_grid(uint32_t n, uint32_t seed) {
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

/* n x n unit cells with z exactly 0 (a zero extent on one axis), every coordinate moved by `offset` in x and y
 * and then multiplied by `scale`: 2 n^2 triangles */
inline Mesh flat_grid(uint32_t n, float offset, float scale) {
    Mesh m;
    for (uint32_t y = 0; y <= n; y++)
        for (uint32_t x = 0; x <= n; x++) {
            m.v.push_back(((float)x + offset) * scale);
            m.v.push_back(((float)y + offset) * scale);
            m.v.push_back(0.f);
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
inline Mesh geometric(uint32_t nt, double growth) {
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

/* triangles without area: three collinear vertices each, some with two or all three vertices equal */
inline Mesh zero_area(uint32_t nt, uint32_t seed) {
    Mesh m;
    Lcg r{seed};
    for (uint32_t k = 0; k < nt; k++) {
        /* multiples of 1/64 below 8: the sums and the edge products are exact, so the normal is exactly 0 */
        auto grid = [&](float scale) { return std::floor(r.next() * scale * 64.f) / 64.f; };
        const float a[3] = {grid(4.f), grid(4.f), grid(1.f)};
        const float e[3] = {grid(1.f) - 0.5f, grid(1.f) - 0.5f, grid(1.f) - 0.5f};
        const float s1 = k % 4 == 1 ? 0.f : 1.f, s2 = k % 4 == 1 || k % 4 == 2 ? 0.f : 2.f;
        for (int j = 0; j < 3; j++) m.v.push_back(a[j]);
        for (int j = 0; j < 3; j++) m.v.push_back(a[j] + s1 * e[j]);
        for (int j = 0; j < 3; j++) m.v.push_back(a[j] + s2 * e[j]);
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
inline Box decode(const DevBvh4& n, int i) {
    const float o[3] = {n.ox, n.oy, n.oz}, s[3] = {n.sx, n.sy, n.sz};
    Box b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = o[k] + (float)((n.qlo[k] >> (8 * i)) & 0xffu) * s[k];
        b.hi[k] = o[k] + (float)((n.qhi[k] >> (8 * i)) & 0xffu) * s[k];
    }
    return b;
}
inline Box decode(const DevBvh4F& n, int i) {
    Box b;
    for (int k = 0; k < 3; k++) b.lo[k] = n.b[2 * k][i], b.hi[k] = n.b[2 * k + 1][i];
    return b;
}

/* A walk of a four-wide tree from the root: every node reached once, leaves within range and within leaf_max,
 * every child's quantised box (and fp32 box, where the builder made fp32 nodes) around the triangles beneath
 * it, empty slots holding the empty box.  The device builder makes quantised nodes only: nodes_f = nullptr. */
struct Walk {
    const Mesh& m;
    const std::vector<DevBvh4>& nodes;
    const std::vector<DevBvh4F>* nodes_f; /* same topology with fp32 boxes, or nullptr */
    const std::vector<uint32_t>& leaf_order;
    uint32_t depth; /* of the binary tree the nodes were collapsed from */
    uint32_t leaf_max;
    std::vector<uint32_t> covered; /* per leaf-order slot: leaves that hold it */
    std::vector<uint8_t> seen;     /* per node */
    uint32_t depth4 = 0;           /* deepest four-wide node met */

    Walk(const Mesh& mesh, const std::vector<DevBvh4>& q, const std::vector<DevBvh4F>* f,
         const std::vector<uint32_t>& order, uint32_t binary_depth, uint32_t lmax)
        : m(mesh), nodes(q), nodes_f(f), leaf_order(order), depth(binary_depth), leaf_max(lmax), covered(mesh.nt(), 0),
          seen(q.size(), 0) {}

    /* the exact box of the triangles beneath `node`; bound = the stack entries a traversal of it can hold */
    Box visit(uint32_t node, uint32_t d4, uint32_t& bound) {
        Box all;
        bound = 0;
        CHECK(node < nodes.size(), "node %u out of range", node);
        if (node >= nodes.size()) return all;
        CHECK(!seen[node], "node %u reached twice", node);
        if (seen[node]) return all;
        seen[node] = 1;
        CHECK(d4 <= depth, "four-wide depth %u above the binary depth %u", d4, depth);
        if (d4 > depth) return all; /* also ends a walk round a cycle of unseen nodes */
        depth4 = d4 > depth4 ? d4 : depth4;
        const DevBvh4& q = nodes[node];
        uint32_t children = 0, sub = 0;
        for (int i = 0; i < 4; i++) {
            const uint32_t ref = q.child[i];
            if (nodes_f)
                CHECK((*nodes_f)[node].child[i] == ref, "node %u child %d: %08x in nodes, %08x in nodes_f", node, i, ref,
                      (*nodes_f)[node].child[i]);
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
                    const uint32_t tri = leaf_order[k];
                    if (tri < m.nt())
                        for (int v = 0; v < 3; v++) under.add(m.vert(tri, v));
                }
            } else {
                uint32_t b = 0;
                under = visit(ref, d4 + 1, b);
                sub = b > sub ? b : sub;
            }
            CHECK(under.inside(decode(q, i)), "node %u child %d: quantised box misses a vertex beneath it", node, i);
            if (nodes_f)
                CHECK(under.inside(decode((*nodes_f)[node], i)), "node %u child %d: fp32 box misses a vertex beneath it",
                      node, i);
            all.add(under);
        }
        CHECK(children >= 1, "node %u has no children", node);
        bound = (children ? children - 1u : 0u) + sub;
        return all;
    }
};

/* the structure checks every tree gets, from either builder; false: not fit for tracing rays through */
inline bool check_structure(const Mesh& m, const std::vector<DevBvh4>& nodes, const std::vector<DevBvh4F>* nodes_f,
                            const std::vector<uint32_t>& leaf_order, uint32_t depth, uint32_t stack_bound,
                            uint32_t leaf_max) {
    const int before = failures;
    const uint32_t nt = m.nt();
    CHECK(leaf_order.size() == nt, "leaf_order has %zu entries for %u triangles", leaf_order.size(), nt);
    CHECK(!nodes.empty() && (!nodes_f || nodes.size() == nodes_f->size()), "%zu nodes, %zu fp32 nodes", nodes.size(),
          nodes_f ? nodes_f->size() : (size_t)0);
    CHECK(nodes.size() <= nt, "%zu four-wide nodes for %u triangles", nodes.size(), nt);
    if (failures != before) return false;
    std::vector<uint32_t> times(nt, 0);
    for (uint32_t id : leaf_order) {
        CHECK(id < nt, "leaf_order holds %u", id);
        if (id < nt) times[id]++;
    }
    for (uint32_t t = 0; t < nt; t++) CHECK(times[t] == 1, "triangle %u is %u times in leaf_order", t, times[t]);
    CHECK(depth < ORX_BVH_STACK, "depth %u", depth);
    CHECK(stack_bound <= 96, "stack bound %u", stack_bound);
    if (failures != before) return false;

    Walk w(m, nodes, nodes_f, leaf_order, depth, leaf_max);
    uint32_t bound = 0;
    w.visit(0, 0, bound);
    CHECK(bound == stack_bound, "stack bound %u, a walk of the tree gives %u", stack_bound, bound);
    for (uint32_t k = 0; k < nt; k++) CHECK(w.covered[k] == 1, "leaf-order slot %u is in %u leaves", k, w.covered[k]);
    for (size_t n = 0; n < nodes.size(); n++) CHECK(w.seen[n], "node %zu is unreachable", n);
    return failures == before;
}

/* does the ray o + t d, t >= 0, meet the box?  In double, so that this test never culls by its own rounding. */
inline bool hit_box(const Box& b, const float* o, const float* d) {
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

/* ---- the reference ---- */
struct V3 {
    float x, y, z;
};
inline V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

/* isect_tri of orx_isect.h (the branch-free form), operation for operation in fp32 */
inline bool isect_tri_ref(const float* a, const float* b, const float* c, const float* o, const float* d, float tmin,
                          float tmax, float& tout, float& bout, float& gout) {
    const V3 p0{a[0], a[1], a[2]}, p1{b[0], b[1], b[2]}, p2{c[0], c[1], c[2]}, ro{o[0], o[1], o[2]}, rd{d[0], d[1], d[2]};
    const V3 e0 = sub(p1, p0), e1 = sub(p0, p2), n = cross3(e1, e0);
    const float s = 1.0f / dot3(n, rd);
    const V3 q = sub(p0, ro), e2{q.x * s, q.y * s, q.z * s};
    const V3 i = cross3(rd, e2);
    const float beta = dot3(i, e1), gamma = dot3(i, e0), t = dot3(n, e2);
    if ((t < tmax) & (t > tmin) & (beta >= 0.0f) & (gamma >= 0.0f) & (beta + gamma <= 1)) {
        tout = t, bout = beta, gout = gamma;
        return true;
    }
    return false;
}

struct RefHit {
    float t = INFINITY, b = 0.f, g = 0.f;
    uint32_t tri = 0xffffffffu;
    bool hit() const { return tri != 0xffffffffu; }
};
inline bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
inline bool same_hit(const RefHit& a, const RefHit& b) {
    if (a.hit() != b.hit()) return false;
    return !a.hit() || (a.tri == b.tri && same_bits(a.t, b.t) && same_bits(a.b, b.b) && same_bits(a.g, b.g));
}

/* one triangle offered to a closest-hit search that goes through the triangles in any order: a strictly nearer
 * hit replaces, an equally near one only from a lower id (in original order: the first of a tie stays) */
inline void offer(const Mesh& m, uint32_t tri, const float* o, const float* d, float tmin, float tmax, RefHit& best) {
    float t, b, g;
    if (!isect_tri_ref(m.vert(tri, 0), m.vert(tri, 1), m.vert(tri, 2), o, d, tmin, tmax, t, b, g)) return;
    if (!best.hit() || t < best.t || (t == best.t && tri < best.tri)) best.t = t, best.b = b, best.g = g, best.tri = tri;
}
/* brute force over all triangles in original order, tmin < t < tmax, a strictly smaller t replaces */
inline RefHit ref_closest(const Mesh& m, const float* o, const float* d, float tmin, float tmax) {
    RefHit best;
    for (uint32_t tri = 0; tri < m.nt(); tri++) {
        float t, b, g;
        if (isect_tri_ref(m.vert(tri, 0), m.vert(tri, 1), m.vert(tri, 2), o, d, tmin, tmax, t, b, g) &&
            (!best.hit() || t < best.t))
            best.t = t, best.b = b, best.g = g, best.tri = tri;
    }
    return best;
}
/* any hit in the window (shadow rays) */
inline bool ref_any(const Mesh& m, const float* o, const float* d, float tmin, float tmax) {
    float t, b, g;
    for (uint32_t tri = 0; tri < m.nt(); tri++)
        if (isect_tri_ref(m.vert(tri, 0), m.vert(tri, 1), m.vert(tri, 2), o, d, tmin, tmax, t, b, g)) return true;
    return false;
}

/* closest hit through a four-wide tree on the host (boxes by hit_box, which culls nothing a ray reaches) */
template <class Node>
RefHit trace_ref(const Mesh& m, const std::vector<Node>& nodes, const std::vector<uint32_t>& leaf_order, const float* o,
                 const float* d, float tmin, float tmax) {
    RefHit best;
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
            for (uint32_t k = first; k < first + count; k++) offer(m, leaf_order[k], o, d, tmin, tmax, best);
        }
    }
    return best;
}

/* ---- ray sets ---- */
struct RaySet {
    std::vector<float> o, d, tmin, tmax; /* float3, float3, float, float per ray */
    std::vector<RefHit> closest;         /* the reference, computed once per mesh */
    std::vector<uint8_t> any;
    uint32_t hits = 0;
    size_t size() const { return tmin.size(); }
    void add(const float* oo, const float* dd, float t0, float t1) {
        o.insert(o.end(), oo, oo + 3), d.insert(d.end(), dd, dd + 3), tmin.push_back(t0), tmax.push_back(t1);
    }
};

constexpr float RAY_TMAX = 1.e27f; /* RT_DEFAULT_MAX of the kernels */

/* `count` rays for a mesh (not a multiple of 64: the last wave of a launch is partial), in blocks of 64:
 *   block 0   every ray misses: origins above the mesh, directions away from it;
 *   block 1   the same, but lane 17 is aimed at a triangle;
 *   then, ray by ray in rotation,
 *   (a) general position: from a point near a triangle (distances in units of that triangle's size, so that
 *       meshes spanning many orders of magnitude get rays at every scale) to a point inside it, or to a point
 *       beside the mesh;
 *   (b) one or two direction components exactly zero, +0.f and -0.f, through a vertex (shared, in a grid), an edge
 *       midpoint or an interior point, and along the mesh's lines of constant y and of constant x through a vertex;
 *   (c) rays in the plane z = the vertex's z (the plane of a flat mesh), through a vertex;
 *   (d) origins on a triangle and just beside its centroid (inside its leaf's box), and rays whose window is cut
 *       at the hit the full window gives: tmin = that t (excludes it), tmax = that t (excludes everything), tmax
 *       = the next float above it (keeps it), tmax half of it.
 * Then the reference results: closest[] and any[]. */
inline RaySet make_ray_set(const Mesh& m, uint32_t count, uint32_t seed) {
    RaySet r;
    Lcg g{seed};
    Box all;
    for (uint32_t t = 0; t < m.nt(); t++)
        for (int k = 0; k < 3; k++) all.add(m.vert(t, k));
    float span = 0.f;
    for (int k = 0; k < 3; k++) span = std::fmax(span, all.hi[k] - all.lo[k]);
    if (!(span > 0.f)) span = 1.f;
    struct Target {
        float p[3], size;
    };
    /* a point of a random triangle: kind 0 inside, 1 a vertex, 2 an edge midpoint; size = its longest box side */
    auto target = [&](int kind) {
        const uint32_t tri = g.below(m.nt());
        const float *a = m.vert(tri, 0), *b = m.vert(tri, 1), *c = m.vert(tri, 2);
        float u = 0.1f + 0.5f * g.next(), v = 0.1f + 0.3f * g.next();
        if (kind == 1) u = v = 0.f;
        if (kind == 2) u = 0.5f, v = 0.f;
        Target t;
        t.size = 0.f;
        for (int k = 0; k < 3; k++) {
            t.p[k] = a[k] + u * (b[k] - a[k]) + v * (c[k] - a[k]);
            t.size = std::fmax(t.size, std::fmax(std::fmax(a[k], b[k]), c[k]) - std::fmin(std::fmin(a[k], b[k]), c[k]));
        }
        if (!(t.size > 0.f)) t.size = 1.f;
        return t;
    };
    auto away = [&]() { /* above the mesh, going up and outward */
        const float o[3] = {all.lo[0] + span * g.next(), all.lo[1] + span * g.next(), all.hi[2] + span * (0.5f + g.next())};
        const float d[3] = {g.next() - 0.5f, g.next() - 0.5f, 0.25f + g.next()};
        r.add(o, d, 0.f, RAY_TMAX);
    };
    auto aimed = [&](const Target& t, float t0, float t1) { /* from above or below the target, at its own scale */
        const float side = g.next() < 0.8f ? 1.f : -1.f;
        const float o[3] = {t.p[0] + t.size * 3.f * (g.next() - 0.5f), t.p[1] + t.size * 3.f * (g.next() - 0.5f),
                            t.p[2] + side * t.size * (0.5f + 2.f * g.next())};
        const float d[3] = {t.p[0] - o[0], t.p[1] - o[1], t.p[2] - o[2]};
        r.add(o, d, t0, t1);
    };
    for (uint32_t i = 0; i < 64 && r.size() < count; i++) away();
    for (uint32_t i = 0; i < 64 && r.size() < count; i++) {
        if (i == 17) aimed(target(0), 0.f, RAY_TMAX);
        else away();
    }
    for (uint32_t n = 0; r.size() < count; n++) {
        const uint32_t kind = n % 16;
        const float zero = (n / 16) % 2 ? -0.f : 0.f;
        if (kind < 5) { /* (a) towards */
            aimed(target(0), 0.f, RAY_TMAX);
        } else if (kind == 5) { /* (a) beside: aimed at a point outside the mesh's box */
            Target t = target(0);
            t.p[0] = all.hi[0] + span * (0.05f + g.next());
            aimed(t, 0.f, RAY_TMAX);
        } else if (kind == 6) { /* (b) two zero components: straight down or up through a vertex / edge / inside */
            const Target t = target((int)((n / 16) % 3));
            const float up = (n / 48) % 2 ? -1.f : 1.f;
            const float o[3] = {t.p[0], t.p[1], t.p[2] + up * t.size * (0.5f + g.next())};
            const float d[3] = {zero, (n / 32) % 2 ? -0.f : 0.f, -up};
            r.add(o, d, 0.f, RAY_TMAX);
        } else if (kind == 7) { /* (b) one zero component, through a vertex or an edge midpoint */
            const Target t = target(1 + (int)(n / 16) % 2);
            const float h = t.size * (0.5f + g.next()), s = t.size * (g.next() - 0.5f);
            const bool xz = (n / 32) % 2;
            const float o[3] = {xz ? t.p[0] - s : t.p[0], xz ? t.p[1] : t.p[1] - s, t.p[2] + h};
            const float d[3] = {xz ? s : zero, xz ? zero : s, -h};
            r.add(o, d, 0.f, RAY_TMAX);
        } else if (kind == 8) { /* (b) + (c) along a line of constant y or x through a vertex, in its z plane */
            const Target t = target(1);
            const bool alongx = (n / 16) % 4 < 2;
            const float back = span * (0.25f + g.next()), dir = (n / 64) % 2 ? -1.f : 1.f;
            const float o[3] = {alongx ? t.p[0] - dir * back : t.p[0], alongx ? t.p[1] : t.p[1] - dir * back, t.p[2]};
            const float d[3] = {alongx ? dir : zero, alongx ? zero : dir, (n / 32) % 2 ? -0.f : 0.f};
            r.add(o, d, 0.f, RAY_TMAX);
        } else if (kind == 9) { /* (c) in the vertex's z plane, general direction within it */
            const Target t = target(1);
            const float dx = g.next() - 0.5f, dy = g.next() - 0.5f;
            const float o[3] = {t.p[0] - 2.f * dx * t.size, t.p[1] - 2.f * dy * t.size, t.p[2]};
            const float d[3] = {dx, dy, zero};
            r.add(o, d, 0.f, RAY_TMAX);
        } else if (kind == 10) { /* (d) origin on the surface */
            const Target t = target((int)(n / 16) % 3);
            const float d[3] = {g.next() - 0.5f, g.next() - 0.5f, g.next() - 0.5f};
            r.add(t.p, d, 0.f, RAY_TMAX);
        } else if (kind == 11) { /* (d) origin just beside a triangle: inside its leaf's box */
            const Target t = target(0);
            const float o[3] = {t.p[0], t.p[1], t.p[2] + t.size * 1e-3f * (g.next() - 0.5f)};
            const float d[3] = {g.next() - 0.5f, g.next() - 0.5f, g.next() - 0.5f};
            r.add(o, d, 1e-4f, RAY_TMAX);
        } else { /* (d) windows cut at the hit of the full window */
            aimed(target(0), 0.f, RAY_TMAX);
            const size_t k = r.size() - 1;
            const RefHit h = ref_closest(m, &r.o[3 * k], &r.d[3 * k], 0.f, RAY_TMAX);
            const float t = h.hit() ? h.t : 1.f;
            if (kind == 12) r.tmin[k] = t;
            if (kind == 13) r.tmax[k] = t;
            if (kind == 14) r.tmax[k] = std::nextafter(t, INFINITY);
            if (kind == 15) r.tmax[k] = 0.5f * t;
        }
    }
    for (size_t k = 0; k < r.size(); k++) {
        r.closest.push_back(ref_closest(m, &r.o[3 * k], &r.d[3 * k], r.tmin[k], r.tmax[k]));
        r.any.push_back(ref_any(m, &r.o[3 * k], &r.d[3 * k], r.tmin[k], r.tmax[k]) ? 1 : 0);
        r.hits += r.closest.back().hit();
        CHECK(r.any.back() == (r.closest.back().hit() ? 1 : 0), "ray %zu: the reference's any hit and closest hit differ", k);
    }
    return r;
}

/* ---- the cases both programs run ---- */
struct NamedOptions {
    const char* name;
    BvhBuildOptions opt;
};
inline std::vector<NamedOptions> option_sets() {
    std::vector<NamedOptions> sets(5);
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
    return sets;
}

enum Expect { HITS_AND_MISSES, NO_HIT_POSSIBLE };
struct RayCase {
    std::string name;
    Mesh mesh;
    bool rays;       /* false: structure checks only */
    bool id0_wins;   /* identical triangles: every hit is triangle 0's */
    Expect expect;
};
/* the degenerate meshes: deep trees, a zero extent, far from the origin, huge, identical and zero-area triangles */
inline std::vector<RayCase> degenerate_cases() {
    std::vector<RayCase> c;
    c.push_back({"geometric 2000 x 1.01", geometric(2000, 1.01), true, false, HITS_AND_MISSES});
    c.push_back({"geometric 4000 x 1.005", geometric(4000, 1.005), true, false, HITS_AND_MISSES});
    c.push_back({"geometric 20000 x 1.0008", geometric(20000, 1.0008), false, false, HITS_AND_MISSES});
    c.push_back({"geometric 20000 x 1.003", geometric(20000, 1.003), false, false, HITS_AND_MISSES});
    c.push_back({"flat grid16", flat_grid(16, 0.f, 1.f), true, false, HITS_AND_MISSES});
    c.push_back({"flat grid16 + 1e7", flat_grid(16, 1e7f, 1.f), true, false, HITS_AND_MISSES});
    /* the triangle formula's own normal (an edge product, 1e60) overflows here: no ray can hit, see below */
    c.push_back({"flat grid16 x 1e30", flat_grid(16, 0.f, 1e30f), true, false, NO_HIT_POSSIBLE});
    for (uint32_t n : {2u, 8u, 9u, 10u, 3000u})
        c.push_back({std::to_string(n) + " identical triangles", repeated_triangle(n), true, true, HITS_AND_MISSES});
    c.push_back({"32 zero-area triangles", zero_area(32, 0x51ed270bu), true, false, NO_HIT_POSSIBLE});
    return c;
}
/* the rays of a set must make the reference alone produce both outcomes.  Two meshes cannot be hit at all by
 * the product's triangle formula, whatever the ray: a triangle without area has the normal 0 and its t is 0 x inf
 * = NaN, and at scale 1e30 the normal is inf and t is inf x 0 = NaN.  For them the reference must say so. */
inline void check_hit_share(const RayCase& c, const RaySet& r) {
    if (c.expect == NO_HIT_POSSIBLE) CHECK(r.hits == 0, "%u of %zu rays hit a mesh that cannot be hit", r.hits, r.size());
    else CHECK(r.hits > r.size() / 4 && r.hits < r.size(), "%u of %zu rays hit", r.hits, r.size());
    if (c.id0_wins)
        for (size_t k = 0; k < r.size(); k++)
            CHECK(!r.closest[k].hit() || r.closest[k].tri == 0, "ray %zu: triangle %u wins among identical ones", k,
                  r.closest[k].tri);
}
constexpr uint32_t RAYS_PER_SET = 4093;

}  // namespace bvhcheck
