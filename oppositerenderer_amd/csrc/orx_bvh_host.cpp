/*
 * orx_bvh_host.cpp — the host BVH builder (see orx_bvh_host.h).
 */
#include "orx_bvh_host.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace orx {

namespace {

bool leaf(const DevBvhNode& n) { return (n.count_or_right & 0x80000000u) != 0; }
/* half the surface area of a box; an inverted (empty) box counts as 0 */
float area(const float* lo, const float* hi) {
    float dx = std::max(0.f, hi[0] - lo[0]), dy = std::max(0.f, hi[1] - lo[1]), dz = std::max(0.f, hi[2] - lo[2]);
    return dx * dy + dy * dz + dz * dx;
}
/* the same of a built node, whose box is never inverted: no clamp, as in the device collapse's b2area (the two
 * forms differ only where an extent is NaN, so both are kept) */
float area(const DevBvhNode& n) {
    float dx = n.hi[0] - n.lo[0], dy = n.hi[1] - n.lo[1], dz = n.hi[2] - n.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

/* host-side BVH over triangles: binned SAH, conservative boxes */
struct BuildTri {
    float lo[3], hi[3], c[3];
};

struct BvhBuilder {
    std::vector<DevBvhNode> nodes;
    std::vector<uint32_t> prims;
    const std::vector<BuildTri>* tris = nullptr;

    static void grow(float* lo, float* hi, const float* l2, const float* h2) {
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], l2[k]);
            hi[k] = std::max(hi[k], h2[k]);
        }
    }
    uint32_t max_depth = 0;
    int bins = 32; /* BvhBuildOptions */
    uint32_t leaf_max = 8;
    float leaf_sah = 0.6f;
    static uint32_t ceil_log2(uint32_t v) {
        uint32_t l = 0;
        while ((1u << l) < v) l++;
        return l;
    }
    uint32_t build(uint32_t first, uint32_t count, uint32_t depth = 0) {
        if (depth > max_depth) max_depth = depth;
        uint32_t idx = (uint32_t)nodes.size();
        nodes.push_back(DevBvhNode{});
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = first; i < first + count; i++) {
            const BuildTri& t = (*tris)[prims[i]];
            grow(lo, hi, t.lo, t.hi);
            grow(clo, chi, t.c, t.c);
        }
        /* conservative expansion so that rounding in the slab test can never
         * cull a primitive the exact test would hit */
        for (int k = 0; k < 3; k++) {
            float m = std::max(std::fabs(lo[k]), std::fabs(hi[k]));
            float e = m * 1e-6f + 1e-20f;
            nodes[idx].lo[k] = lo[k] - e;
            nodes[idx].hi[k] = hi[k] + e;
        }
        if (count <= 1 || (count <= leaf_max && leaf_sah == 0.f)) {
            nodes[idx].left_or_first = first;
            nodes[idx].count_or_right = 0x80000000u | count;
            return idx;
        }
        /* binned SAH on the centroid extent; object-median split once the
         * depth budget (ORX_BVH_STACK) would otherwise be at risk */
        const int NB = bins;
        int best_axis = -1, best_split = 0;
        float best_cost = INFINITY;
        const bool median = depth + ceil_log2((count + 3) / 4) + 2 >= ORX_BVH_STACK;
        for (int ax = 0; ax < 3 && !median; ax++) {
            float ext = chi[ax] - clo[ax];
            if (!(ext > 0)) continue;
            uint32_t cnt[64] = {0};
            float blo[64][3], bhi[64][3];
            for (int b = 0; b < NB; b++)
                for (int k = 0; k < 3; k++) blo[b][k] = INFINITY, bhi[b][k] = -INFINITY;
            for (uint32_t i = first; i < first + count; i++) {
                const BuildTri& t = (*tris)[prims[i]];
                int b = std::min(NB - 1, (int)((t.c[ax] - clo[ax]) / ext * NB));
                cnt[b]++;
                grow(blo[b], bhi[b], t.lo, t.hi);
            }
            float rl[64], rcount[64];
            float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
            uint32_t acc = 0;
            for (int b = NB - 1; b > 0; b--) {
                acc += cnt[b];
                grow(alo, ahi, blo[b], bhi[b]);
                rl[b] = area(alo, ahi);
                rcount[b] = (float)acc;
            }
            float llo[3] = {INFINITY, INFINITY, INFINITY}, lhi[3] = {-INFINITY, -INFINITY, -INFINITY};
            uint32_t lc = 0;
            for (int b = 0; b < NB - 1; b++) {
                lc += cnt[b];
                grow(llo, lhi, blo[b], bhi[b]);
                float cost = area(llo, lhi) * (float)lc + rl[b + 1] * rcount[b + 1];
                if (lc > 0 && lc < count && cost < best_cost) {
                    best_cost = cost;
                    best_axis = ax;
                    best_split = b;
                }
            }
        }
        if (count <= leaf_max) {
            /* SAH leaf test: split cost Ct + (A_L N_L + A_R N_R)/A vs leaf cost N (Ci = 1) */
            const float A = area(lo, hi);
            if (best_axis < 0 || !(A > 0) || leaf_sah + best_cost / A >= (float)count) {
                nodes[idx].left_or_first = first;
                nodes[idx].count_or_right = 0x80000000u | count;
                return idx;
            }
        }
        uint32_t mid;
        if (best_axis < 0) {
            /* object median along the widest centroid axis */
            int ax = 0;
            for (int a = 1; a < 3; a++)
                if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
            mid = first + count / 2;
            std::nth_element(prims.begin() + first, prims.begin() + mid, prims.begin() + first + count,
                             [&](uint32_t p, uint32_t q) { return (*tris)[p].c[ax] < (*tris)[q].c[ax]; });
        } else {
            float ext = chi[best_axis] - clo[best_axis];
            auto it = std::partition(prims.begin() + first, prims.begin() + first + count, [&](uint32_t p) {
                const BuildTri& t = (*tris)[p];
                int b = std::min(NB - 1, (int)((t.c[best_axis] - clo[best_axis]) / ext * NB));
                return b <= best_split;
            });
            mid = (uint32_t)(it - prims.begin());
            if (mid == first || mid == first + count) mid = first + count / 2;
        }
        uint32_t l = build(first, mid - first, depth + 1);
        uint32_t r = build(mid, first + count - mid, depth + 1);
        nodes[idx].left_or_first = l;
        nodes[idx].count_or_right = r;
        return idx;
    }
};

/* Treelet restructuring of the binary tree (Karras & Aila 2013, the refinement of OptiX's Trbvh; the host
 * counterpart of the device builder's k_bvh_treelet, priced in tools/bvh_quality.cpp): per inner node, bottom
 * up, the treelet of its 7 largest-area descendants' subtrees is rebuilt as the SAH-optimal binary tree over
 * them (dynamic programme over the 127 subsets; node cost leaf_sah x area, leaf cost area x triangles), reusing
 * the treelet's inner nodes.  Boxes are unions of the children's (already conservatively expanded) boxes. */
struct TreeletOpt {
    std::vector<DevBvhNode>& B;
    float ci;
    size_t nl = 7; /* treelet leaves */
    std::vector<double> cost;
    explicit TreeletOpt(std::vector<DevBvhNode>& b, float c) : B(b), ci(c), cost(b.size(), 0.0) {}
    void refresh(uint32_t n) {
        DevBvhNode& x = B[n];
        if (leaf(x)) {
            cost[n] = (double)area(x.lo, x.hi) * (double)(x.count_or_right & 0x7fffffffu);
            return;
        }
        const DevBvhNode &l = B[x.left_or_first], &r = B[x.count_or_right];
        for (int k = 0; k < 3; k++) x.lo[k] = std::min(l.lo[k], r.lo[k]), x.hi[k] = std::max(l.hi[k], r.hi[k]);
        cost[n] = (double)ci * area(x.lo, x.hi) + cost[x.left_or_first] + cost[x.count_or_right];
    }
    uint32_t emit(int S, uint32_t hint, const std::vector<uint32_t>& inner, size_t& next, const std::vector<int>& split,
                  const std::vector<uint32_t>& lv) {
        if ((S & (S - 1)) == 0) return lv[__builtin_ctz(S)];
        const uint32_t id = hint != 0xffffffffu ? hint : inner[next++];
        const uint32_t l = emit(split[S], 0xffffffffu, inner, next, split, lv);
        const uint32_t r = emit(S ^ split[S], 0xffffffffu, inner, next, split, lv);
        B[id].left_or_first = l;
        B[id].count_or_right = r;
        refresh(id);
        return id;
    }
    bool restructure(uint32_t n) {
        if (leaf(B[n])) return false;
        std::vector<uint32_t> lv = {B[n].left_or_first, B[n].count_or_right}, inner = {n};
        while (lv.size() < nl) {
            int bi = -1;
            float ba = -1.f;
            for (size_t i = 0; i < lv.size(); i++)
                if (!leaf(B[lv[i]]) && area(B[lv[i]].lo, B[lv[i]].hi) > ba) ba = area(B[lv[i]].lo, B[lv[i]].hi), bi = (int)i;
            if (bi < 0) break;
            const uint32_t c = lv[bi];
            inner.push_back(c);
            lv[bi] = B[c].left_or_first;
            lv.push_back(B[c].count_or_right);
        }
        const int m = (int)lv.size();
        if (m < 3) return false;
        const int full = (1 << m) - 1;
        std::vector<double> copt(1 << m, 0.0);
        std::vector<float> ar(1 << m, 0.f);
        std::vector<int> split(1 << m, 0);
        for (int S = 1; S <= full; S++) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = 0; i < m; i++)
                if (S >> i & 1)
                    for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], B[lv[i]].lo[k]), hi[k] = std::max(hi[k], B[lv[i]].hi[k]);
            ar[S] = area(lo, hi);
        }
        for (int S = 1; S <= full; S++) {
            if ((S & (S - 1)) == 0) {
                copt[S] = cost[lv[__builtin_ctz(S)]];
                continue;
            }
            double best = INFINITY;
            int bp = 0;
            const int low = S & -S;
            for (int P = (S - 1) & S; P; P = (P - 1) & S) {
                if (!(P & low)) continue;
                const double c = copt[P] + copt[S ^ P];
                if (c < best) best = c, bp = P;
            }
            copt[S] = (double)ci * ar[S] + best;
            split[S] = bp;
        }
        if (!(copt[full] < cost[n] * (1.0 - 1e-6))) return false;
        size_t next = 1;
        emit(full, n, inner, next, split, lv);
        return true;
    }
    uint32_t pass() {
        std::vector<uint32_t> order, st = {0u};
        while (!st.empty()) {
            const uint32_t n = st.back();
            st.pop_back();
            order.push_back(n);
            if (!leaf(B[n])) st.push_back(B[n].left_or_first), st.push_back(B[n].count_or_right);
        }
        uint32_t changed = 0;
        for (auto it = order.rbegin(); it != order.rend(); ++it) {
            refresh(*it);
            changed += restructure(*it);
        }
        return changed;
    }
    uint32_t depth(uint32_t n) const {
        return leaf(B[n]) ? 0u : 1u + std::max(depth(B[n].left_or_first), depth(B[n].count_or_right));
    }
};

/* Collapse the binary SAH tree into the four-wide quantised BVH the kernels
 * traverse (DevBvh4).  Each node opens its largest-area inner children until
 * it has four; child boxes are quantised outward on an 8-bit grid per axis.
 * `bound` = the most stack entries a traversal can hold: at a node with k
 * children hit, k-1 are pushed before descending. */
struct Bvh4Builder {
    const std::vector<DevBvhNode>* b2 = nullptr;
    std::vector<DevBvh4> out;
    std::vector<DevBvh4F> outf; /* same topology, fp32 child boxes */
    bool ok = true;
    /* the SAH-optimal collapse (Ylitie et al. 2017; the device builder's k_bvh_sahdp): F[n][i], the cheapest cover of n's
     * subtree by at most i roots (a four-wide node visit costing 2.5 triangle tests x area, a leaf area x
     * triangles), and K[n][i] the roots given to the left child (0: n is one root) */
    std::vector<std::array<double, 5>> F;
    std::vector<std::array<uint8_t, 5>> K;
    void dp(uint32_t n) {
        const std::vector<DevBvhNode>& B = *b2;
        if (F.empty()) F.assign(B.size(), {}), K.assign(B.size(), {});
        const float a = area(B[n]);
        if (leaf(B[n])) {
            for (int i = 1; i <= 4; i++) F[n][i] = (double)a * (double)(B[n].count_or_right & 0x7fffffffu), K[n][i] = 0;
            return;
        }
        const uint32_t l = B[n].left_or_first, r = B[n].count_or_right;
        dp(l);
        dp(r);
        auto G = [&](int i, int& kb) {
            double best = INFINITY;
            for (int k = 1; k < i; k++)
                if (F[l][k] + F[r][i - k] < best) best = F[l][k] + F[r][i - k], kb = k;
            return best;
        };
        int k = 1;
        F[n][1] = 2.5 * (double)a + G(4, k);
        K[n][1] = (uint8_t)k; /* the distribution inside n's own node */
        for (int i = 2; i <= 4; i++) {
            const double g = G(i, k);
            if (g < F[n][1]) F[n][i] = g, K[n][i] = (uint8_t)k;
            else F[n][i] = F[n][1], K[n][i] = 0;
        }
    }
    void roots(uint32_t n, int i, std::vector<uint32_t>& out_) const {
        const std::vector<DevBvhNode>& B = *b2;
        if (i == 1 || leaf(B[n]) || K[n][i] == 0) {
            out_.push_back(n);
            return;
        }
        roots(B[n].left_or_first, K[n][i], out_);
        roots(B[n].count_or_right, i - K[n][i], out_);
    }

    /* outward 8-bit quantisation of [clo, chi] on origin + q * 2^e */
    static bool quantise(float origin, int e, float clo, float chi, uint32_t& qlo, uint32_t& qhi) {
        const float sc = std::ldexp(1.0f, e);
        auto dec = [&](uint32_t q) { return origin + (float)q * sc; };
        double fl = std::floor(((double)clo - origin) / sc), ch = std::ceil(((double)chi - origin) / sc);
        qlo = (uint32_t)std::min(255.0, std::max(0.0, fl));
        qhi = (uint32_t)std::min(255.0, std::max(0.0, ch));
        while (qlo > 0 && dec(qlo) > clo) qlo--;
        if (dec(qlo) > clo) return false;
        while (qhi < 255 && dec(qhi) < chi) qhi++;
        return dec(qhi) >= chi;
    }
    uint32_t build(uint32_t n2, uint32_t& bound) {
        const std::vector<DevBvhNode>& B = *b2;
        std::vector<uint32_t> ch;
        if (leaf(B[n2])) {
            ch.push_back(n2);
        } else if (!F.empty()) {
            roots(B[n2].left_or_first, K[n2][1], ch);
            roots(B[n2].count_or_right, 4 - K[n2][1], ch);
        } else {
            ch = {B[n2].left_or_first, B[n2].count_or_right};
            while (ch.size() < 4) {
                int bi = -1;
                float ba = -1.f;
                for (size_t i = 0; i < ch.size(); i++)
                    if (!leaf(B[ch[i]]) && area(B[ch[i]]) > ba) ba = area(B[ch[i]]), bi = (int)i;
                if (bi < 0) break;
                const uint32_t c = ch[bi];
                ch[bi] = B[c].left_or_first;
                ch.push_back(B[c].count_or_right);
            }
        }
        DevBvh4 nd;
        std::memset(&nd, 0, sizeof nd);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t c : ch)
            for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], B[c].lo[k]), hi[k] = std::max(hi[k], B[c].hi[k]);
        nd.ox = lo[0];
        nd.oy = lo[1];
        nd.oz = lo[2];
        for (int k = 0; k < 3; k++) {
            const float ext = hi[k] - lo[k];
            int e = -126;
            if (ext > 0) {
                int ee;
                std::frexp(ext / 255.0f, &ee);
                e = std::max(-126, ee - 1);
            }
            for (;; e++) {
                if (e > 127) { ok = false; break; }
                bool good = true;
                uint32_t ql[4] = {0, 0, 0, 0}, qh[4] = {0, 0, 0, 0};
                for (size_t i = 0; i < ch.size() && good; i++)
                    good = quantise(lo[k], e, B[ch[i]].lo[k], B[ch[i]].hi[k], ql[i], qh[i]);
                if (!good) continue;
                uint32_t wl = 0, wh = 0;
                /* an empty slot gets the empty box lo = 255 > hi = 0: every ray misses it */
                for (int i = 0; i < 4; i++) wl |= ((size_t)i < ch.size() ? ql[i] : 255u) << (8 * i), wh |= qh[i] << (8 * i);
                nd.qlo[k] = wl;
                nd.qhi[k] = wh;
                (k == 0 ? nd.sx : k == 1 ? nd.sy : nd.sz) = ldexpf(1.0f, e); /* 2^e, exact for e in [-126, 127] */
                break;
            }
        }
        const uint32_t idx = (uint32_t)out.size();
        out.push_back(nd);
        DevBvh4F nf;
        std::memset(&nf, 0, sizeof nf);
        for (int i = 0; i < 4; i++) {
            const bool has = (size_t)i < ch.size();
            for (int k = 0; k < 3; k++) {
                nf.b[2 * k][i] = has ? B[ch[i]].lo[k] : INFINITY;
                nf.b[2 * k + 1][i] = has ? B[ch[i]].hi[k] : -INFINITY;
            }
        }
        outf.push_back(nf);
        uint32_t sub = 0;
        uint32_t refs[4] = {ORX_EMPTY, ORX_EMPTY, ORX_EMPTY, ORX_EMPTY};
        for (size_t i = 0; i < ch.size(); i++) {
            const DevBvhNode& c = B[ch[i]];
            if (leaf(c)) {
                const uint32_t cnt = c.count_or_right & 0x7fffffffu;
                if (cnt == 0 || cnt > 8 || c.left_or_first >= (1u << 28)) ok = false;
                refs[i] = ORX_LEAF | (c.left_or_first << 3) | (cnt - 1u);
            } else {
                uint32_t b = 0;
                refs[i] = build(ch[i], b);
                sub = std::max(sub, b);
            }
        }
        for (int i = 0; i < 4; i++) out[idx].child[i] = outf[idx].child[i] = refs[i];
        bound = (uint32_t)ch.size() - 1u + sub;
        return idx;
    }
};

}  // namespace

BvhBuildOptions bvh_options_from_env() {
    BvhBuildOptions o;
    if (const char* e = getenv("ORX_BVH_BINS")) o.bins = std::max(2, std::min(32, atoi(e)));
    if (const char* e = getenv("ORX_BVH_LEAF_MAX")) o.leaf_max = (uint32_t)std::max(1, std::min(8, atoi(e)));
    if (const char* e = getenv("ORX_BVH_LEAF_SAH")) o.leaf_sah = (float)atof(e);
    /* treelet restructuring sweeps of the binary tree and the SAH-optimal four-wide collapse (the refinement
     * OptiX's Trbvh does, Scene.cpp:353): hall photon-path node steps 17.71 -> 16.91 per ray, PPM frame +2.5 %,
     * VCM +2.6 % (profiles/r06j_bvh_treelet_ab.txt); ORX_BVH_TREELET=0 / ORX_BVH_COLLAPSE=0: the round-5 tree */
    if (const char* e = getenv("ORX_BVH_TREELET")) o.treelet_passes = std::max(0, std::min(8, atoi(e)));
    if (const char* e = getenv("ORX_BVH_COLLAPSE")) o.sah_collapse = atoi(e) != 0;
    if (const char* e = getenv("ORX_BVH_TREELET_LEAVES")) o.treelet_leaves = atoi(e) == 7 ? 7 : 9;
    return o;
}

const char* build_host_bvh4(const float* vertices, const uint32_t* indices, uint32_t nt, const BvhBuildOptions& opt,
                            HostBvh4* out) {
    std::vector<BuildTri> bt(nt);
    for (uint32_t i = 0; i < nt; i++) {
        BuildTri& b = bt[i];
        for (int k = 0; k < 3; k++) b.lo[k] = INFINITY, b.hi[k] = -INFINITY;
        for (int v = 0; v < 3; v++) {
            const float* p = vertices + 3 * (size_t)indices[3 * (size_t)i + v];
            for (int k = 0; k < 3; k++) {
                b.lo[k] = std::min(b.lo[k], p[k]);
                b.hi[k] = std::max(b.hi[k], p[k]);
            }
        }
        for (int k = 0; k < 3; k++) b.c[k] = 0.5f * (b.lo[k] + b.hi[k]);
    }
    BvhBuilder bb;
    bb.tris = &bt;
    bb.bins = opt.bins;
    bb.leaf_max = opt.leaf_max;
    bb.leaf_sah = opt.leaf_sah;
    bb.prims.resize(nt);
    for (uint32_t i = 0; i < nt; i++) bb.prims[i] = i;
    bb.nodes.reserve(2 * (size_t)nt / 2 + 1);
    bb.build(0, nt);
    if (opt.treelet_passes > 0) { /* the device builder's sweeps, on the host tree */
        /* The sweeps restructure by cost alone and can deepen a tree that the binned build kept below
         * ORX_BVH_STACK with its median splits (long chains of boxes that grow geometrically).  If they did,
         * the binned tree is taken as it was: the sweeps only reorder the nodes' links and boxes, never prims. */
        const std::vector<DevBvhNode> binned = bb.nodes;
        TreeletOpt to(bb.nodes, opt.leaf_sah > 0.f ? opt.leaf_sah : 0.6f);
        to.nl = (size_t)opt.treelet_leaves;
        for (int p = 0; p < opt.treelet_passes; p++) to.pass();
        const uint32_t swept = to.depth(0);
        if (swept >= ORX_BVH_STACK) bb.nodes = binned;
        else bb.max_depth = swept;
    }
    if (bb.max_depth >= ORX_BVH_STACK) return "BVH deeper than the traversal stack";
    Bvh4Builder b4;
    b4.b2 = &bb.nodes;
    b4.out.reserve(bb.nodes.size() / 2 + 1);
    if (opt.sah_collapse) b4.dp(0);
    uint32_t stack_bound = 0;
    b4.build(0, stack_bound);
    if (!b4.ok) return "BVH4 quantisation failed";
    out->nodes = std::move(b4.out);
    out->nodes_f = std::move(b4.outf);
    out->leaf_order = std::move(bb.prims);
    out->stack_bound = stack_bound;
    out->depth = bb.max_depth;
    return nullptr;
}

}  // namespace orx
