// bvh_device_check.hip — stand-alone check of the device BVH builder (oppositerenderer_amd/csrc/orx_bvh.hip) and of
// the traversal loops of orx_traverse.h, on the GPU.  Built by `make` in oppositerenderer_amd/csrc with the product's
// flags from orx_bvh.hip, orx_bvh_host.cpp and this file; run once by tests/test_gpu_bvh_device.py.
//
// Per mesh (bvh_check_common.h: the host check's meshes, among them deep, flat, far, huge, identical and
// zero-area ones) and option set: build with device_build_bvh4, copy the nodes and the leaf order back and walk
// the tree as the host check walks the host builder's; on three meshes compare the tree with the host builder's;
// then lay the triangles out as orx_init_scene does and trace the mesh's ray set with trace_closest (StackL),
// trace_closest_t over StackH<16> and StackH<4>, trace_any, trace_any_t over StackH<16> and trace_any_chain.
// Closest hits must equal a brute-force search with the same triangle formula on the host bit for bit in t, id,
// beta and gamma; any-hit results must equal its boolean.  Every HIP call is checked and the first error ends
// the program before any further GPU work.  One line per case, then `all checks passed`; exit status 0: all held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "bvh_check_common.h"
#include "orx_bvh_host.h"
#include "orx_kernels.h"
#include "orx_traverse.h"

using namespace bvhcheck;

#define HIPCK(call)                                                                                     \
    do {                                                                                                \
        const hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                         \
            std::printf("HIP error [%s] %s: %s (%s:%d)\n", current.c_str(), #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                            \
            std::fflush(stdout);                                                                        \
            std::exit(2);                                                                               \
        }                                                                                               \
    } while (0)

struct DevRay {
    float ox, oy, oz, tmin, dx, dy, dz, tmax;
};
struct DevHit {
    float t, b, g;
    uint32_t id, slot, hit;
};

enum Mode { CLOSEST_L, CLOSEST_H16, CLOSEST_H4, ANY_L, ANY_H16, MODES };
const char* const mode_name[MODES] = {"trace_closest", "trace_closest_t<StackH<16>>", "trace_closest_t<StackH<4>>",
                                      "trace_any", "trace_any_t<StackH<16>>"};

/* one ray per lane, one wave per block; the lanes past the last ray leave before the traversal */
template <int MODE>
__global__ __launch_bounds__(64) void k_trace(orx::DevScene S, const DevRay* __restrict__ rays, uint32_t n,
                                              DevHit* __restrict__ out, uint32_t* gstk, uint32_t ndeep) {
    ORX_STACK_DECL;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const DevRay r = rays[i];
    const orx::f3 o = orx::mk(r.ox, r.oy, r.oz), d = orx::mk(r.dx, r.dy, r.dz);
    orx::Hit h;
    h.t = 0.f, h.prim = -1, h.slot = 0, h.b = 0.f, h.g = 0.f;
    bool hit;
    if constexpr (MODE == CLOSEST_L) {
        hit = orx::trace_closest(S, o, d, r.tmin, r.tmax, h, ORX_STACK_PTR);
    } else if constexpr (MODE == CLOSEST_H16) {
        hit = orx::trace_closest_t(S, o, d, r.tmin, r.tmax, h,
                                   orx::StackH<16>{ORX_STACK_PTR, gstk, blockIdx.x, ndeep, threadIdx.x}, orx::NodesG{});
    } else if constexpr (MODE == CLOSEST_H4) {
        hit = orx::trace_closest_t(S, o, d, r.tmin, r.tmax, h,
                                   orx::StackH<4>{ORX_STACK_PTR, gstk, blockIdx.x, ndeep, threadIdx.x}, orx::NodesG{});
    } else if constexpr (MODE == ANY_L) {
        hit = orx::trace_any(S, o, d, r.tmin, r.tmax, ORX_STACK_PTR);
    } else {
        hit = orx::trace_any_t(S, o, d, r.tmin, r.tmax,
                               orx::StackH<16>{ORX_STACK_PTR, gstk, blockIdx.x, ndeep, threadIdx.x}, orx::NodesG{});
    }
    out[i] = DevHit{h.t, h.b, h.g, (uint32_t)h.prim, h.slot, hit ? 1u : 0u};
}

/* trace_any_chain's ray source: the lane's rays are rays[cur .. end) */
struct ChainRays {
    const DevRay* rays;
    uint32_t* occ;
    uint32_t cur, end;
    __device__ __forceinline__ bool next(orx::f3& o, orx::f3& d, float& tmin, float& tmax) {
        if (cur >= end) return false;
        const DevRay r = rays[cur++];
        o = orx::mk(r.ox, r.oy, r.oz), d = orx::mk(r.dx, r.dy, r.dz), tmin = r.tmin, tmax = r.tmax;
        return true;
    }
    __device__ __forceinline__ void result(bool occluded) { occ[cur - 1] = occluded ? 1u : 0u; }
};
/* lane l of the launch walks rays first[l] .. first[l + 1]: none to five each */
__global__ __launch_bounds__(64) void k_chain(orx::DevScene S, const DevRay* __restrict__ rays,
                                              const uint32_t* __restrict__ first, uint32_t* __restrict__ occ) {
    ORX_STACK_DECL;
    const uint32_t l = blockIdx.x * 64u + threadIdx.x;
    ChainRays R{rays, occ, first[l], first[l + 1]};
    orx::trace_any_chain(S, R, ORX_STACK_PTR);
}

template <class T>
struct DevArray {
    T* p = nullptr;
    explicit DevArray(size_t n) { HIPCK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T))); }
    DevArray(const DevArray&) = delete;
    ~DevArray() { (void)hipFree(p); }
    void upload(const std::vector<T>& h) { HIPCK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> download(size_t n) const {
        std::vector<T> h(n);
        HIPCK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

struct DeviceTree {
    std::vector<orx::DevBvh4> nodes;
    std::vector<uint32_t> leaf_order;
    uint32_t depth = 0, stack_bound = 0;
};

/* the leaves of a tree, each the sorted ids of its triangles, in sorted order */
std::vector<std::vector<uint32_t>> leaf_sets(const std::vector<orx::DevBvh4>& nodes, const std::vector<uint32_t>& order) {
    std::vector<std::vector<uint32_t>> out;
    for (const orx::DevBvh4& n : nodes)
        for (int i = 0; i < 4; i++) {
            const uint32_t ref = n.child[i];
            if (ref == orx::ORX_EMPTY || !(ref & orx::ORX_LEAF)) continue;
            const uint32_t first = (ref & ~orx::ORX_LEAF) >> 3, count = (ref & 7u) + 1u;
            std::vector<uint32_t> ids(order.begin() + first, order.begin() + first + count);
            std::sort(ids.begin(), ids.end());
            out.push_back(ids);
        }
    std::sort(out.begin(), out.end());
    return out;
}
/* the sorted ids beneath a child reference */
void ids_beneath(const std::vector<orx::DevBvh4>& nodes, const std::vector<uint32_t>& order, uint32_t ref,
                 std::vector<uint32_t>& ids) {
    if (ref == orx::ORX_EMPTY) return;
    if (ref & orx::ORX_LEAF) {
        const uint32_t first = (ref & ~orx::ORX_LEAF) >> 3, count = (ref & 7u) + 1u;
        ids.insert(ids.end(), order.begin() + first, order.begin() + first + count);
        return;
    }
    for (int i = 0; i < 4; i++) ids_beneath(nodes, order, nodes[ref].child[i], ids);
}
/* from the root down, the first node whose children hold different triangle sets in the two trees */
void print_first_difference(const DeviceTree& d, const orx::HostBvh4& h) {
    std::vector<std::pair<uint32_t, uint32_t>> todo = {{0u, 0u}};
    for (size_t k = 0; k < todo.size(); k++) {
        const orx::DevBvh4 &a = d.nodes[todo[k].first], &b = h.nodes[todo[k].second];
        std::vector<std::pair<std::vector<uint32_t>, uint32_t>> sa, sb;
        for (int i = 0; i < 4; i++) {
            std::vector<uint32_t> ia, ib;
            ids_beneath(d.nodes, d.leaf_order, a.child[i], ia);
            ids_beneath(h.nodes, h.leaf_order, b.child[i], ib);
            std::sort(ia.begin(), ia.end());
            std::sort(ib.begin(), ib.end());
            if (!ia.empty()) sa.push_back({ia, a.child[i]});
            if (!ib.empty()) sb.push_back({ib, b.child[i]});
        }
        std::sort(sa.begin(), sa.end());
        std::sort(sb.begin(), sb.end());
        bool same = sa.size() == sb.size();
        for (size_t i = 0; same && i < sa.size(); i++)
            same = sa[i].first == sb[i].first && ((sa[i].second & orx::ORX_LEAF) == (sb[i].second & orx::ORX_LEAF));
        if (!same) {
            std::printf("  first difference: device node %u, host node %u (%zu nodes down the breadth-first order)\n",
                        todo[k].first, todo[k].second, k);
            for (const auto& s : sa)
                std::printf("    device child %s of %zu triangles, ids %u..%u\n", s.second & orx::ORX_LEAF ? "leaf" : "node",
                            s.first.size(), s.first.front(), s.first.back());
            for (const auto& s : sb)
                std::printf("    host   child %s of %zu triangles, ids %u..%u\n", s.second & orx::ORX_LEAF ? "leaf" : "node",
                            s.first.size(), s.first.front(), s.first.back());
            return;
        }
        for (size_t i = 0; i < sa.size(); i++)
            if (!(sa[i].second & orx::ORX_LEAF)) todo.push_back({sa[i].second, sb[i].second});
    }
    std::printf("  the trees hold the same triangle sets node by node\n");
}

struct GpuRays {
    const RaySet& set;
    uint32_t n, blocks;
    DevArray<DevRay> rays;
    DevArray<DevHit> hits;
    DevArray<uint32_t> occ, chain_first;
    uint32_t chain_blocks = 0;
    explicit GpuRays(const RaySet& s)
        : set(s), n((uint32_t)s.size()), blocks((n + 63) / 64), rays(n), hits(n), occ(n), chain_first(2 * (size_t)n + 130) {
        std::vector<DevRay> h(n);
        for (uint32_t k = 0; k < n; k++)
            h[k] = DevRay{s.o[3 * k], s.o[3 * k + 1], s.o[3 * k + 2], s.tmin[k], s.d[3 * k], s.d[3 * k + 1], s.d[3 * k + 2],
                          s.tmax[k]};
        rays.upload(h);
        /* lane l takes (5 l + 3 (l / 64)) % 6 rays: none to five, a different number from its neighbours */
        std::vector<uint32_t> first = {0u};
        for (uint32_t l = 0; first.back() < n || first.size() % 64 != 1; l++)
            first.push_back(std::min(n, first.back() + (5u * l + 3u * (l / 64u)) % 6u));
        chain_blocks = (uint32_t)(first.size() - 1) / 64u;
        CHECK(first.size() <= 2 * (size_t)n + 130, "chain table of %zu entries", first.size());
        if (first.size() > 2 * (size_t)n + 130) std::exit(1);
        chain_first.upload(first);
    }
};

/* CHECK prints the first failures only: say per case and loop how many rays differ, and which come first */
void report(const std::vector<uint32_t>& differ, const RaySet& set) {
    if (differ.empty()) return;
    std::printf("  [%s] %zu of %zu rays differ:", current.c_str(), differ.size(), set.size());
    for (size_t i = 0; i < differ.size() && i < 12; i++) std::printf(" %u", differ[i]);
    std::printf("\n");
}

void trace_and_compare(const std::string& name, const RayCase& c, const DeviceTree& t, GpuRays& g) {
    const Mesh& m = c.mesh;
    const uint32_t nt = m.nt();
    /* the scene as orx_init_scene lays it out: triangles in leaf order, tri_v[3k].w = the original id */
    std::vector<float4> tv(3 * (size_t)nt);
    for (uint32_t k = 0; k < nt; k++) {
        const uint32_t id = t.leaf_order[k];
        for (int v = 0; v < 3; v++) {
            const float* p = m.vert(id, v);
            float w = 0.f;
            if (v == 0) std::memcpy(&w, &id, 4);
            tv[3 * (size_t)k + v] = make_float4(p[0], p[1], p[2], w);
        }
    }
    DevArray<float4> dtv(tv.size());
    dtv.upload(tv);
    DevArray<orx::DevBvh4> dnodes(t.nodes.size());
    dnodes.upload(t.nodes);
    orx::DevScene S;
    std::memset(&S, 0, sizeof S);
    S.nt = nt;
    S.tri_v = dtv.p;
    S.bvh4 = dnodes.p;
    S.bvh_nodes = (uint32_t)t.nodes.size();
    S.stack_entries = t.stack_bound + 1; /* as orx_init_scene */
    float max_abs = 0.f;
    for (float x : m.v) max_abs = std::max(max_abs, std::fabs(x));
    S.dir_zero = orx::orx_dir_zero(max_abs); /* as orx_init_scene */
    const uint32_t deep16 = orx::StackH<16>::deep(S.stack_entries), deep4 = orx::StackH<4>::deep(S.stack_entries);
    const size_t gblocks = std::max(g.blocks, g.chain_blocks);
    DevArray<uint32_t> gstk(gblocks * std::max(deep16, deep4) * 64u);

    for (int mode = 0; mode < MODES; mode++) {
        current = name + ", " + mode_name[mode];
        HIPCK(hipMemset(g.hits.p, 0xff, (size_t)g.n * sizeof(DevHit)));
        const dim3 grid(g.blocks), block(64);
        switch (mode) {
        case CLOSEST_L:
            hipLaunchKernelGGL(k_trace<CLOSEST_L>, grid, block, ORX_STACK_BYTES(S), 0, S, g.rays.p, g.n, g.hits.p, gstk.p, 1u);
            break;
        case CLOSEST_H16:
            hipLaunchKernelGGL(k_trace<CLOSEST_H16>, grid, block, orx::StackH<16>::lds_bytes(), 0, S, g.rays.p, g.n, g.hits.p,
                               gstk.p, deep16);
            break;
        case CLOSEST_H4:
            hipLaunchKernelGGL(k_trace<CLOSEST_H4>, grid, block, orx::StackH<4>::lds_bytes(), 0, S, g.rays.p, g.n, g.hits.p,
                               gstk.p, deep4);
            break;
        case ANY_L:
            hipLaunchKernelGGL(k_trace<ANY_L>, grid, block, ORX_STACK_BYTES(S), 0, S, g.rays.p, g.n, g.hits.p, gstk.p, 1u);
            break;
        default:
            hipLaunchKernelGGL(k_trace<ANY_H16>, grid, block, orx::StackH<16>::lds_bytes(), 0, S, g.rays.p, g.n, g.hits.p,
                               gstk.p, deep16);
        }
        HIPCK(hipGetLastError());
        HIPCK(hipDeviceSynchronize());
        const std::vector<DevHit> got = g.hits.download(g.n);
        std::vector<uint32_t> differ;
        for (uint32_t k = 0; k < g.n; k++) {
            const DevHit& h = got[k];
            const RefHit& r = g.set.closest[k];
            const int before = failures;
            struct Note { /* the rays that failed a check below, whichever way the loop body is left */
                std::vector<uint32_t>& v;
                uint32_t k;
                int before;
                ~Note() {
                    if (failures != before) v.push_back(k);
                }
            } note{differ, k, before};
            CHECK(h.hit <= 1u, "ray %u: no result written", k);
            if (mode == ANY_L || mode == ANY_H16) {
                CHECK(h.hit == g.set.any[k], "ray %u: any hit %u, the reference %u", k, h.hit, (unsigned)g.set.any[k]);
                continue;
            }
            CHECK((h.hit == 1u) == r.hit(), "ray %u: hit %u, the reference %d (t %a triangle %u)", k, h.hit, (int)r.hit(), r.t,
                  r.tri);
            if (h.hit != 1u || !r.hit()) continue;
            CHECK(h.id == r.tri && same_bits(h.t, r.t) && same_bits(h.b, r.b) && same_bits(h.g, r.g),
                  "ray %u: t %a triangle %u beta %a gamma %a, the reference t %a triangle %u beta %a gamma %a", k, h.t, h.id, h.b,
                  h.g, r.t, r.tri, r.b, r.g);
            CHECK(h.slot < nt && t.leaf_order[h.slot < nt ? h.slot : 0] == h.id, "ray %u: slot %u is not triangle %u's", k, h.slot,
                  h.id);
        }
        report(differ, g.set);
    }
    current = name + ", trace_any_chain";
    HIPCK(hipMemset(g.occ.p, 0xff, (size_t)g.n * 4));
    hipLaunchKernelGGL(k_chain, dim3(g.chain_blocks), dim3(64), ORX_STACK_BYTES(S), 0, S, g.rays.p, g.chain_first.p, g.occ.p);
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    const std::vector<uint32_t> occ = g.occ.download(g.n);
    std::vector<uint32_t> differ;
    for (uint32_t k = 0; k < g.n; k++) {
        CHECK(occ[k] == g.set.any[k], "ray %u: occluded %u, the reference %u", k, occ[k], (unsigned)g.set.any[k]);
        if (occ[k] != g.set.any[k]) differ.push_back(k);
    }
    report(differ, g.set);
    current = name;
}

/* build on the device, copy back, walk; false: nothing to trace through */
bool build_and_walk(const std::string& name, const Mesh& m, const orx::BvhBuildOptions& opt, DeviceTree& t) {
    current = name;
    const uint32_t nt = m.nt();
    DevArray<float> dV(m.v.size());
    DevArray<uint32_t> dI(m.i.size());
    dV.upload(m.v);
    dI.upload(m.i);
    DevArray<orx::DevBvh4> dnodes((size_t)nt + 1);
    DevArray<uint32_t> dorder(nt);
    uint32_t nodes4 = 0;
    bool ok = false;
    HIPCK(orx::device_build_bvh4(nullptr, dV.p, dI.p, nt, opt, dnodes.p, nt, dorder.p, &nodes4, &t.stack_bound, &t.depth, &ok));
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    CHECK(ok, "the device build failed (quantisation or capacity)");
    CHECK(nodes4 >= 1 && nodes4 <= nt, "%u four-wide nodes for %u triangles", nodes4, nt);
    if (!ok || nodes4 < 1 || nodes4 > nt) return false;
    t.nodes = dnodes.download(nodes4);
    t.leaf_order = dorder.download(nt);
    if (!check_structure(m, t.nodes, nullptr, t.leaf_order, t.depth, t.stack_bound, opt.leaf_max)) return false;
    return true;
}

/* the two builders on one mesh and option set: equal node count, depth, stack bound and leaves */
void compare_with_host(const Mesh& m, const orx::BvhBuildOptions& opt, const DeviceTree& d) {
    orx::HostBvh4 h;
    const char* msg = orx::build_host_bvh4(m.v.data(), m.i.data(), m.nt(), opt, &h);
    CHECK(msg == nullptr, "the host build failed: %s", msg);
    if (msg) return;
    const int before = failures;
    CHECK(d.nodes.size() == h.nodes.size(), "%zu nodes, the host builder %zu", d.nodes.size(), h.nodes.size());
    CHECK(d.depth == h.depth, "depth %u, the host builder %u", d.depth, h.depth);
    CHECK(d.stack_bound == h.stack_bound, "stack bound %u, the host builder %u", d.stack_bound, h.stack_bound);
    CHECK(leaf_sets(d.nodes, d.leaf_order) == leaf_sets(h.nodes, h.leaf_order), "the leaves differ from the host builder's");
    if (failures != before) print_first_difference(d, h);
}

int main() {
    const std::vector<NamedOptions> sets = option_sets();
    std::vector<RayCase> cases;
    cases.push_back({"one triangle", repeated_triangle(1), true, true, HITS_AND_MISSES});
    for (uint32_t n : {1u, 3u, 12u, 48u})
        cases.push_back({"grid" + std::to_string(n), jittered_grid(n, 0x9e3779b9u + n), true, false, HITS_AND_MISSES});
    for (RayCase& c : degenerate_cases()) cases.push_back(std::move(c));

    for (const RayCase& c : cases) {
        current = c.name;
        RaySet rays;
        if (c.rays) {
            rays = make_ray_set(c.mesh, RAYS_PER_SET, 0x2545f491u);
            check_hit_share(c, rays);
        }
        GpuRays* g = c.rays ? new GpuRays(rays) : nullptr;
        const bool twin = c.name == "grid12" || c.name == "grid48" || c.name == "geometric 2000 x 1.01";
        for (size_t s = 0; s < sets.size(); s++) {
            const std::string name = c.name + ", " + sets[s].name;
            DeviceTree t;
            if (!build_and_walk(name, c.mesh, sets[s].opt, t)) continue;
            if (twin && (s == 0 || s == 2)) compare_with_host(c.mesh, sets[s].opt, t);
            const int before = failures;
            if (g) trace_and_compare(name, c, t, *g);
            std::printf("%-50s %6u triangles %6zu nodes depth %2u bound %2u  %s\n", name.c_str(), c.mesh.nt(), t.nodes.size(),
                        t.depth, t.stack_bound,
                        !g ? "structure only" : failures == before ? "rays exact" : "RAYS DIFFER");
            std::fflush(stdout);
        }
        delete g;
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
