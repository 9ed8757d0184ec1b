/*
 * orx_traverse.h — BVH4 traversal: the node tests, the traversal stacks and the three loops
 * (closest hit, any hit, a chain of any-hit rays).
 *
 * Replaces the OptiX device runtime's acceleration-structure traversal.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orx_bvh_nodes.h"
#include "orx_isect.h"
#include "orx_scene_types.h" /* orx_dir_zero */

namespace orx {

/* per-ray slab-test constants (what a zero direction component becomes: orx_dir_zero, orx_scene_types.h) */
struct RayBox {
    f3 o, inv;
    bool nx, ny, nz; /* negative direction: the near slab of that axis is the box's hi bound */
    f3 oinv;         /* -o * inv (fp32 boxes: t = fma(bound, inv, oinv)) */
};
__device__ __forceinline__ RayBox ray_box(f3 o, f3 d, float zero = 1e-30f) {
    auto safe = [zero](float v) { return fabsf(v) > zero ? v : copysignf(zero, v); };
    RayBox rb;
    rb.o = o;
    /* v_rcp_f32 (1 ulp): the builder's 1e-6 relative box expansion covers it */
    rb.inv = mk(__builtin_amdgcn_rcpf(safe(d.x)), __builtin_amdgcn_rcpf(safe(d.y)), __builtin_amdgcn_rcpf(safe(d.z)));
    rb.nx = rb.inv.x < 0.f;
    rb.ny = rb.inv.y < 0.f;
    rb.nz = rb.inv.z < 0.f;
    rb.oinv = mk(-o.x * rb.inv.x, -o.y * rb.inv.y, -o.z * rb.inv.z);
    return rb;
}
/* The window the box tests get: the triangle tests' (tmin, tmax), widened by 2^-20 (8 ulp) at both ends.
 * A slab distance carries the rounding of v_rcp_f32 (1 ulp), of (origin - o) * inv and of the fma, and the
 * triangle test's t has roundings of its own, all relative to t; the builder's box expansion is relative to
 * the box's coordinates.  Where a box has no extent at coordinate 0 (an axis-aligned face in a coordinate plane:
 * expansion 1e-20), or lies much further from the ray's origin than from the coordinate origin, the expansion
 * does not cover them, and a box was culled against a window that ended within a few ulp behind its triangle's
 * hit: a tmax just past the hit, or the equally distant hit of a higher triangle id found first (tie lost). */
constexpr float ORX_BOX_TMIN = 1.f - 0x1p-20f, ORX_BOX_TMAX = 1.f + 0x1p-20f;
/* Test the four quantised child boxes of a node against (tmin, tmax):
 * t = (origin + q*s - o) * inv evaluated as fma(q, s*inv, (origin - o)*inv);
 * the rounding of that form is far below the builder's 1e-6 relative box
 * expansion, so the test stays conservative.  The near/far bound of each
 * axis is picked once per node from the ray's direction signs, so a child
 * costs 6 fma + 4 min/max (identical values to the min/max slab form).
 * Returns entry distances (+inf for misses) and child refs. */
__device__ __forceinline__ void node_test_q(const float4 A, const float4 B, const float4 C, const float4 D,
                                            const RayBox& rb, float tmin, float tmax, float t[4], uint32_t c[4]) {
    const float sx = A.w, sy = D.z, sz = D.w;
    const float ax = (A.x - rb.o.x) * rb.inv.x, bx = sx * rb.inv.x;
    const float ay = (A.y - rb.o.y) * rb.inv.y, by = sy * rb.inv.y;
    const float az = (A.z - rb.o.z) * rb.inv.z, bz = sz * rb.inv.z;
    const uint32_t lx = __float_as_uint(B.x), ly = __float_as_uint(B.y), lz = __float_as_uint(B.z);
    const uint32_t hx = __float_as_uint(B.w), hy = __float_as_uint(C.x), hz = __float_as_uint(C.y);
    const uint32_t nxq = rb.nx ? hx : lx, fxq = rb.nx ? lx : hx;
    const uint32_t nyq = rb.ny ? hy : ly, fyq = rb.ny ? ly : hy;
    const uint32_t nzq = rb.nz ? hz : lz, fzq = rb.nz ? lz : hz;
    c[0] = __float_as_uint(C.z);
    c[1] = __float_as_uint(C.w);
    c[2] = __float_as_uint(D.x);
    c[3] = __float_as_uint(D.y);
    /* two children per v_pk_fma_f32 */
    typedef float v2q __attribute__((ext_vector_type(2)));
    auto q2 = [](uint32_t w, int i) {
        return v2q{(float)((w >> (8 * i)) & 0xffu), (float)((w >> (8 * i + 8)) & 0xffu)};
    };
    const v2q ax2 = v2q{ax, ax}, bx2 = v2q{bx, bx}, ay2 = v2q{ay, ay}, by2 = v2q{by, by};
    const v2q az2 = v2q{az, az}, bz2 = v2q{bz, bz};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const v2q tnx = __builtin_elementwise_fma(q2(nxq, 2 * h), bx2, ax2);
        const v2q tfx = __builtin_elementwise_fma(q2(fxq, 2 * h), bx2, ax2);
        const v2q tny = __builtin_elementwise_fma(q2(nyq, 2 * h), by2, ay2);
        const v2q tfy = __builtin_elementwise_fma(q2(fyq, 2 * h), by2, ay2);
        const v2q tnz = __builtin_elementwise_fma(q2(nzq, 2 * h), bz2, az2);
        const v2q tfz = __builtin_elementwise_fma(q2(fzq, 2 * h), bz2, az2);
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = 2 * h + e;
            const float t0 = fmaxf(fmaxf(fmaxf(tnx[e], tny[e]), tnz[e]), tmin);
            const float t1 = fminf(fminf(fminf(tfx[e], tfy[e]), tfz[e]), tmax);
            t[i] = t0 <= t1 ? t0 : INFINITY; /* an empty slot holds an empty box (lo 255 > hi 0) */
        }
    }
}
/* Node and triangle loads are buffer loads: one 32-bit byte offset per lane (a shift, where a
 * 64-bit address costs two 64-bit VALU operations), the resource in SGPRs.  orx_init_scene keeps
 * the node and triangle arrays below 4 GiB. */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t orx_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0xffffffff, 0x00020000);
}
__device__ __forceinline__ float4 ld16(__amdgpu_buffer_rsrc_t r, uint32_t bo) {
    typedef uint32_t u4b __attribute__((ext_vector_type(4)));
    const u4b v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)bo, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void node_test(const DevBvh4* nodes, uint32_t idx, const RayBox& rb, float tmin, float tmax,
                                          float t[4], uint32_t c[4]) {
    const __amdgpu_buffer_rsrc_t r = orx_rsrc(nodes);
    const uint32_t bo = idx << 6;
    node_test_q(ld16(r, bo), ld16(r, bo + 16), ld16(r, bo + 32), ld16(r, bo + 48), rb, tmin, tmax, t, c);
}
typedef float v2t __attribute__((ext_vector_type(2)));
/* fp32-box node test: t = fma(bound, inv, -o*inv), two children per
 * v_pk_fma_f32; same conservativeness argument as the quantised form */
__device__ __forceinline__ void node_test(const DevBvh4F* nodes, uint32_t idx, const RayBox& rb, float tmin, float tmax,
                                          float t[4], uint32_t c[4]) {
    const float* base = reinterpret_cast<const float*>(nodes + idx);
    const float4 NX = *(const float4*)(base + (rb.nx ? 4 : 0)), FX = *(const float4*)(base + (rb.nx ? 0 : 4));
    const float4 NY = *(const float4*)(base + (rb.ny ? 12 : 8)), FY = *(const float4*)(base + (rb.ny ? 8 : 12));
    const float4 NZ = *(const float4*)(base + (rb.nz ? 20 : 16)), FZ = *(const float4*)(base + (rb.nz ? 16 : 20));
    const uint4 CC = *(const uint4*)(base + 24);
    c[0] = CC.x;
    c[1] = CC.y;
    c[2] = CC.z;
    c[3] = CC.w;
    const v2t ix = v2t{rb.inv.x, rb.inv.x}, iy = v2t{rb.inv.y, rb.inv.y}, iz = v2t{rb.inv.z, rb.inv.z};
    const v2t ox = v2t{rb.oinv.x, rb.oinv.x}, oy = v2t{rb.oinv.y, rb.oinv.y}, oz = v2t{rb.oinv.z, rb.oinv.z};
    const v2t tnx0 = __builtin_elementwise_fma(v2t{NX.x, NX.y}, ix, ox), tnx1 = __builtin_elementwise_fma(v2t{NX.z, NX.w}, ix, ox);
    const v2t tfx0 = __builtin_elementwise_fma(v2t{FX.x, FX.y}, ix, ox), tfx1 = __builtin_elementwise_fma(v2t{FX.z, FX.w}, ix, ox);
    const v2t tny0 = __builtin_elementwise_fma(v2t{NY.x, NY.y}, iy, oy), tny1 = __builtin_elementwise_fma(v2t{NY.z, NY.w}, iy, oy);
    const v2t tfy0 = __builtin_elementwise_fma(v2t{FY.x, FY.y}, iy, oy), tfy1 = __builtin_elementwise_fma(v2t{FY.z, FY.w}, iy, oy);
    const v2t tnz0 = __builtin_elementwise_fma(v2t{NZ.x, NZ.y}, iz, oz), tnz1 = __builtin_elementwise_fma(v2t{NZ.z, NZ.w}, iz, oz);
    const v2t tfz0 = __builtin_elementwise_fma(v2t{FZ.x, FZ.y}, iz, oz), tfz1 = __builtin_elementwise_fma(v2t{FZ.z, FZ.w}, iz, oz);
    const float tn[4][3] = {{tnx0.x, tny0.x, tnz0.x}, {tnx0.y, tny0.y, tnz0.y}, {tnx1.x, tny1.x, tnz1.x}, {tnx1.y, tny1.y, tnz1.y}};
    const float tf[4][3] = {{tfx0.x, tfy0.x, tfz0.x}, {tfx0.y, tfy0.y, tfz0.y}, {tfx1.x, tfy1.x, tfz1.x}, {tfx1.y, tfy1.y, tfz1.y}};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float t0 = fmaxf(fmaxf(fmaxf(tn[i][0], tn[i][1]), tn[i][2]), tmin);
        const float t1 = fminf(fminf(fminf(tf[i][0], tf[i][1]), tf[i][2]), tmax);
        t[i] = (t0 <= t1 && c[i] != 0xffffffffu) ? t0 : INFINITY;
    }
}
/* compare-exchange by entry distance; the distances by min/max (never NaN here: +inf or a
 * max with tmin), which leaves the compare's mask to the two reference selects */
__device__ __forceinline__ void cswap(float& ta, uint32_t& ca, float& tb, uint32_t& cb) {
    /* the distances are >= tmin >= 0 or +inf, so their bit patterns order like the values: unsigned
     * compare and min/max (fminf/fmaxf had cost two NaN-quieting v_max_f32 per exchange) */
    const uint32_t ua = __float_as_uint(ta), ub = __float_as_uint(tb);
    const bool sw = ub < ua;
    const uint32_t c = sw ? cb : ca;
    cb = sw ? ca : cb;
    ca = c;
    ta = __uint_as_float(ua < ub ? ua : ub);
    tb = __uint_as_float(ua < ub ? ub : ua);
}

/* Traversal policies (trace_closest_t / trace_any_t): the stack (StackL: the
 * lane's column of the dynamic-LDS array [stack_entries][64]; StackH below) and the
 * node source (NodesG: S.bvh4).  Measured and dropped: the top 85 / 341 nodes in LDS
 * (DESIGN.md §4). */
struct StackL {
    uint32_t* s;
    __device__ __forceinline__ void push(int& sp, uint32_t v) const { s[(sp++) * 64] = v; }
    __device__ __forceinline__ uint32_t pop(int& sp) const { return s[(--sp) * 64]; }
    /* write entry k without moving the stack pointer (k may run two past the bound) */
    __device__ __forceinline__ void put(int k, uint32_t v) const { s[k * 64] = v; }
    /* the whole stack is in LDS: every wave is shallow */
    __device__ __forceinline__ bool shallow(int, int) const { return true; }
    __device__ __forceinline__ void put_l(int k, uint32_t v) const { put(k, v); }
    __device__ __forceinline__ uint32_t pop_l(int& sp) const { return pop(sp); }
};
/* A short LDS stack continued in global memory: entries k < NL in the lane's LDS column, deeper
 * ones in the block's own global array [depth][64] at column `lane` (g_ = the block's base, so the
 * 32-bit buffer offsets stay below depth * 256 B whatever the launch size), through buffer
 * loads/stores (kept apart from the LDS accesses, which the compiler would otherwise merge with
 * them into flat loads).  The LDS column holds NL + 1 entries: a push always writes LDS, at min(k, NL) (entry
 * NL is a dump slot), and only a push or pop past NL takes the branch to global memory.  The traversal
 * loops test once per node step whether any lane of the wave could pass NL (shallow(): one ballot) and
 * otherwise push and pop through put_l / pop_l, LDS only, without the clamp and the per-entry branch
 * (hall photon pass 3.555 -> 3.494 ms serial, frame +1.1 %, profiles/r06za_stack_fast_path_ab.txt).  For kernels whose occupancy
 * the full-depth LDS stack limits (k_vcm_shadow: 61 VGPRs, 4 waves per SIMD with 35 LDS entries,
 * 8 with 16; k_ppm_photon). */
template <int NL>
struct StackH {
    uint32_t* s;
    __amdgpu_buffer_rsrc_t g;
    uint32_t lane;
    static constexpr uint32_t gstride = 64;
    static constexpr size_t lds_bytes() { return (size_t)(NL + 1) * 64 * 4; }
    /* global entries per lane for a tree whose stack bound is `entries` (the pushes run two past it) */
    __host__ __device__ static constexpr uint32_t deep(uint32_t entries) { return entries + 2 > NL ? entries + 2 - NL : 1u; }
    /* g_: the buffer of every block's [deep][64] entries, block `blk`'s part is used */
    __device__ __forceinline__ StackH(uint32_t* s_, uint32_t* g_, uint32_t blk, uint32_t ndeep, uint32_t lane_)
        : s(s_), g(__builtin_amdgcn_make_buffer_rsrc(g_ + (size_t)blk * ndeep * 64u, 0, ndeep * 256u, 0x00020000)),
          lane(lane_) {}
    __device__ __forceinline__ void push(int& sp, uint32_t v) const { put(sp++, v); }
    __device__ __forceinline__ uint32_t pop(int& sp) const {
        --sp;
        uint32_t v = s[(sp < NL ? sp : NL) * 64];
        if (sp >= NL) v = __builtin_amdgcn_raw_buffer_load_b32(g, (int)(((uint32_t)(sp - NL) * gstride + lane) * 4u), 0, 0);
        return v;
    }
    __device__ __forceinline__ void put(int k, uint32_t v) const {
        s[(k < NL ? k : NL) * 64] = v;
        if (k >= NL) __builtin_amdgcn_raw_buffer_store_b32(v, g, (int)(((uint32_t)(k - NL) * gstride + lane) * 4u), 0, 0);
    }
    /* wave-uniform: no lane's next `n` entries (from sp) reach past the LDS column, so put_l / pop_l
     * (LDS only, no clamp and no per-entry branch to global memory) serve this step */
    __device__ __forceinline__ bool shallow(int sp, int n) const { return !__ballot(sp + n > NL); }
    __device__ __forceinline__ void put_l(int k, uint32_t v) const { s[k * 64] = v; }
    __device__ __forceinline__ uint32_t pop_l(int& sp) const { return s[(--sp) * 64]; }
};
struct NodesG {
    __device__ __forceinline__ void test(const DevScene& S, uint32_t idx, const RayBox& rb, float tmin, float tmax,
                                         float t[4], uint32_t c[4]) const {
        node_test(S.bvh4, idx, rb, tmin, tmax, t, c);
    }
};

/* Optional traversal statistics (build with -DORX_TRAV_STATS): rays, inner
 * nodes visited, leaves visited, triangle tests — per ray type (closest/any). */
#ifdef ORX_TRAV_STATS
#define ORX_TS_DECL uint32_t ts_nodes = 0, ts_leaves = 0, ts_tris = 0, ts_wn = 0, ts_wl = 0
#define ORX_TS_INC(v, n) (v) += (n)
/* wave-level loop iterations: counted by the wave's first active lane */
#define ORX_TS_WAVE(v) (v) += ((uint32_t)(__ffsll((unsigned long long)__ballot(1)) - 1) == (threadIdx.x & 63u))
#define ORX_TS_DECL_TOP uint32_t ts_top[4] = {0, 0, 0, 0}
#define ORX_TS_TOP(idx)                                                     \
    do {                                                                    \
        ts_top[0] += (idx) < 21u;                                           \
        ts_top[1] += (idx) < 85u;                                           \
        ts_top[2] += (idx) < 341u;                                          \
        ts_top[3] += (idx) < 1365u;                                         \
    } while (0)
#define ORX_TS_FLUSH_TOP()                                                  \
    do {                                                                    \
        for (int q_ = 0; q_ < 4; q_++) atomicAdd(&S.trav_stats[16 + q_], (unsigned long long)ts_top[q_]); \
    } while (0)
#define ORX_TS_FLUSH(base)                                                  \
    do {                                                                    \
        atomicAdd(&S.trav_stats[(base) + 0], 1ull);                       \
        atomicAdd(&S.trav_stats[(base) + 1], (unsigned long long)ts_nodes);  \
        atomicAdd(&S.trav_stats[(base) + 2], (unsigned long long)ts_leaves); \
        atomicAdd(&S.trav_stats[(base) + 3], (unsigned long long)ts_tris);   \
        atomicAdd(&S.trav_stats[8 + (base) / 2], (unsigned long long)ts_wn);  \
        atomicAdd(&S.trav_stats[9 + (base) / 2], (unsigned long long)ts_wl);  \
    } while (0)
#else
#define ORX_TS_DECL
#define ORX_TS_DECL_TOP
#define ORX_TS_TOP(idx)
#define ORX_TS_FLUSH_TOP()
#define ORX_TS_INC(v, n)
#define ORX_TS_WAVE(v)
#define ORX_TS_FLUSH(base)
#endif

/* Closest hit over all primitives; equal t resolves to the lowest global
 * primitive id, which is OptiX NoAccel's child order (Cornell.cpp:183-189)
 * and is independent of traversal order, so BVH and brute force agree.
 * Triangles: near-first BVH4 traversal; the hit children of a node are
 * sorted by entry distance, the nearest is taken and the others are pushed
 * far-to-near on the lane's LDS stack. */
template <class STK, class NODES>
__device__ inline bool trace_closest_t(const DevScene& S, f3 o, f3 d, float tmin, float tmax, Hit& h, const STK& stk,
                                       const NODES& nodes) {
    float best = tmax;
    int32_t bp = -1;
    uint32_t bslot = 0;
    float t;
    for (uint32_t i = 0; i < S.nq; i++) {
        if (isect_quad(S.quads[i], o, d, tmin, best, t)) {
            best = t;
            bp = (int32_t)i;
        }
    }
    f3 sn = mk1(0);
    for (uint32_t i = 0; i < S.ns; i++) {
        f3 n;
        if (isect_sphere(S.spheres[i], o, d, tmin, best, t, n)) {
            best = t;
            bp = (int32_t)(S.nq + i);
            sn = n;
        }
    }
    float bb = 0, bg = 0;
    if (S.nt) {
        const uint32_t base = S.nq + S.ns;
        const RayBox rb = ray_box(o, d, S.dir_zero);
        const float tmin_box = tmin * ORX_BOX_TMIN;
        int sp = 0;
        uint32_t ref = 0; /* root */
        ORX_TS_DECL;
        ORX_TS_DECL_TOP;
        /* speculative while-while (Aila & Laine 2009): a lane that reaches a
         * leaf postpones it and keeps descending until every lane of the wave
         * holds a leaf, then all process theirs together */
        uint32_t lf = 0; /* postponed leaf, or a non-leaf value for none */
        while (ref != ORX_DONE) {
            while (!(ref & ORX_LEAF) && ref != ORX_DONE) {
                float ct[4];
                uint32_t cc[4];
                nodes.test(S, ref, rb, tmin_box, best * ORX_BOX_TMAX, ct, cc);
                ORX_TS_INC(ts_nodes, 1);
                ORX_TS_TOP(ref);
                ORX_TS_WAVE(ts_wn);
                cswap(ct[0], cc[0], ct[1], cc[1]);
                cswap(ct[2], cc[2], ct[3], cc[3]);
                cswap(ct[0], cc[0], ct[2], cc[2]);
                cswap(ct[1], cc[1], ct[3], cc[3]);
                cswap(ct[1], cc[1], ct[2], cc[2]);
                /* (dropping the last two exchanges, a near-first order only for the first
                 * child, measured 4.03 -> 4.29 ms on the hall photon pass: order matters) */
                {
                    /* branch-free pushes: the three entries are written unconditionally at
                     * their final positions (misses sort last), then the pointer moves by the
                     * hits (photon pass 4.03 -> 3.98 ms against one branch per push) */
                    const int n3 = ct[3] != INFINITY, n2 = ct[2] != INFINITY, n1 = ct[1] != INFINITY;
                    if (stk.shallow(sp, 3)) { /* the common case: the three entries in LDS */
                        stk.put_l(sp, cc[3]);
                        stk.put_l(sp + n3, cc[2]);
                        stk.put_l(sp + n3 + n2, cc[1]);
                        sp += n3 + n2 + n1;
                        ref = ct[0] != INFINITY ? cc[0] : (sp ? stk.pop_l(sp) : ORX_DONE);
                    } else {
                        stk.put(sp, cc[3]);
                        stk.put(sp + n3, cc[2]);
                        stk.put(sp + n3 + n2, cc[1]);
                        sp += n3 + n2 + n1;
                        ref = ct[0] != INFINITY ? cc[0] : (sp ? stk.pop(sp) : ORX_DONE);
                    }
                }
                if ((ref & ORX_LEAF) && !(lf & ORX_LEAF)) {
                    lf = ref;
                    ref = sp ? stk.pop(sp) : ORX_DONE;
                }
                if (!__ballot(!(lf & ORX_LEAF))) break;
            }
            while (lf & ORX_LEAF) {
                const uint32_t first = (lf & 0x7fffffffu) >> 3, cnt = (lf & 7u) + 1u;
                ORX_TS_INC(ts_leaves, 1);
                ORX_TS_INC(ts_tris, cnt);
                ORX_TS_WAVE(ts_wl);
                const __amdgpu_buffer_rsrc_t tr = orx_rsrc(S.tri_v);
                for (uint32_t k = first; k < first + cnt; k++) {
                    const uint32_t tb = k * 48u;
                    const float4 v0 = ld16(tr, tb), v1 = ld16(tr, tb + 16), v2 = ld16(tr, tb + 32);
                    const int32_t gid = (int32_t)(base + __float_as_uint(v0.w));
                    float b, g;
                    /* accept t < best, or t == best from a lower primitive id */
                    float lim = bp >= 0 ? orx_as_float(orx_as_uint(best) + 1u) : best;
                    if (isect_tri(ld_f3(v0), ld_f3(v1), ld_f3(v2), o, d, tmin, lim, t, b, g) &&
                        (t < best || gid < bp)) {
                        best = t;
                        bp = gid;
                        bslot = k;
                        bb = b;
                        bg = g;
                    }
                }
                lf = ref; /* another leaf postponed behind it: process it too */
                if (ref & ORX_LEAF) ref = sp ? stk.pop(sp) : ORX_DONE;
            }
        }
        ORX_TS_FLUSH(0);
        ORX_TS_FLUSH_TOP();
    }
    if (bp < 0) return false;
    h.t = best;
    h.prim = bp;
    h.slot = bslot;
    h.b = bb;
    h.g = bg;
    h.sn = sn;
    return true;
}
__device__ __forceinline__ bool trace_closest(const DevScene& S, f3 o, f3 d, float tmin, float tmax, Hit& h,
                                              uint32_t* stk) {
    return trace_closest_t(S, o, d, tmin, tmax, h, StackL{stk}, NodesG{});
}

/* any hit in (tmin,tmax): every material's RayType::SHADOW any-hit is
 * gatherAnyHitOnNonEmitter (Material.cpp:18-26, DirectRadianceEstimation.cu:79-83) */
template <class STK, class NODES>
__device__ inline bool trace_any_t(const DevScene& S, f3 o, f3 d, float tmin, float tmax, const STK& stk,
                                   const NODES& nodes) {
    float t;
    for (uint32_t i = 0; i < S.nq; i++)
        if (isect_quad(S.quads[i], o, d, tmin, tmax, t)) return true;
    for (uint32_t i = 0; i < S.ns; i++) {
        f3 n;
        if (isect_sphere(S.spheres[i], o, d, tmin, tmax, t, n)) return true;
    }
    if (S.nt) {
        const RayBox rb = ray_box(o, d, S.dir_zero);
        const float tmin_box = tmin * ORX_BOX_TMIN, tmax_box = tmax * ORX_BOX_TMAX;
        int sp = 0;
        uint32_t ref = 0;
        ORX_TS_DECL;
        uint32_t lf = 0; /* speculative while-while, as trace_closest */
        while (ref != ORX_DONE) {
            while (!(ref & ORX_LEAF) && ref != ORX_DONE) {
                float ct[4];
                uint32_t cc[4];
                nodes.test(S, ref, rb, tmin_box, tmax_box, ct, cc);
                ORX_TS_INC(ts_nodes, 1);
                ORX_TS_WAVE(ts_wn);
                /* branch-free: every hit child is written to the stack (the order does not
                 * matter for any hit), the last one is taken back from registers */
                const int h0 = ct[0] != INFINITY, h1 = ct[1] != INFINITY, h2 = ct[2] != INFINITY,
                          h3 = ct[3] != INFINITY;
                const uint32_t next = h3 ? cc[3] : h2 ? cc[2] : h1 ? cc[1] : h0 ? cc[0] : ORX_DONE;
                if (stk.shallow(sp, 4)) { /* the common case: the four entries in LDS */
                    stk.put_l(sp, cc[0]);
                    sp += h0;
                    stk.put_l(sp, cc[1]);
                    sp += h1;
                    stk.put_l(sp, cc[2]);
                    sp += h2;
                    stk.put_l(sp, cc[3]);
                    sp += h3;
                    sp -= next != ORX_DONE;
                    ref = next != ORX_DONE ? next : (sp ? stk.pop_l(sp) : ORX_DONE);
                } else {
                    stk.put(sp, cc[0]);
                    sp += h0;
                    stk.put(sp, cc[1]);
                    sp += h1;
                    stk.put(sp, cc[2]);
                    sp += h2;
                    stk.put(sp, cc[3]);
                    sp += h3;
                    sp -= next != ORX_DONE;
                    ref = next != ORX_DONE ? next : (sp ? stk.pop(sp) : ORX_DONE);
                }
                if ((ref & ORX_LEAF) && !(lf & ORX_LEAF)) {
                    lf = ref;
                    ref = sp ? stk.pop(sp) : ORX_DONE;
                }
                if (!__ballot(!(lf & ORX_LEAF))) break;
            }
            while (lf & ORX_LEAF) {
                const uint32_t first = (lf & 0x7fffffffu) >> 3, cnt = (lf & 7u) + 1u;
                ORX_TS_INC(ts_leaves, 1);
                ORX_TS_WAVE(ts_wl);
                const __amdgpu_buffer_rsrc_t tr = orx_rsrc(S.tri_v);
                for (uint32_t k = first; k < first + cnt; k++) {
                    float b, g;
                    ORX_TS_INC(ts_tris, 1);
                    const uint32_t tb = k * 48u;
                    if (isect_tri(ld_f3(ld16(tr, tb)), ld_f3(ld16(tr, tb + 16)), ld_f3(ld16(tr, tb + 32)), o, d,
                                  tmin, tmax, t, b, g)) {
                        ORX_TS_FLUSH(4);
                        return true;
                    }
                }
                lf = ref;
                if (ref & ORX_LEAF) ref = sp ? stk.pop(sp) : ORX_DONE;
            }
        }
        ORX_TS_FLUSH(4);
    }
    return false;
}

__device__ __forceinline__ bool trace_any(const DevScene& S, f3 o, f3 d, float tmin, float tmax, uint32_t* stk) {
    return trace_any_t(S, o, d, tmin, tmax, StackL{stk}, NodesG{});
}

/* Several shadow rays per lane in one traversal loop: a lane whose ray has ended (occluder found,
 * or stack empty) starts its next ray at once instead of waiting for the slowest lane of the wave
 * to finish the current one, so a wave runs for the maximum over its lanes of their summed walks,
 * not for the sum over the rays of the slowest walk.  Each ray's own test sequence is trace_any's
 * (the same result, occluded or not).  RAYS supplies the lane's rays in order:
 *   bool next(f3& o, f3& d, float& tmin, float& tmax)  — false when the lane has no more;
 *   void result(bool occluded)                          — the outcome of the ray `next` gave last. */
template <class RAYS, class STK>
__device__ __forceinline__ void trace_any_chain_t(const DevScene& S, RAYS& R, const STK& stk) {
    f3 o = mk1(0.f), d = mk1(0.f);
    float tmin = 0.f, tmax = 0.f, tmin_box = 0.f, tmax_box = 0.f;
    RayBox rb = ray_box(o, mk1(1.f), S.dir_zero);
    int sp = 0;
    uint32_t ref = ORX_DONE, lf = 0;
    /* the lane's next ray that needs a BVH walk (quad and sphere hits, and scenes without
     * triangles, are decided here) */
    auto fetch = [&]() -> bool {
        while (R.next(o, d, tmin, tmax)) {
            float t;
            bool hit = false;
            for (uint32_t i = 0; i < S.nq && !hit; i++) hit = isect_quad(S.quads[i], o, d, tmin, tmax, t);
            for (uint32_t i = 0; i < S.ns && !hit; i++) {
                f3 n;
                hit = isect_sphere(S.spheres[i], o, d, tmin, tmax, t, n);
            }
            if (hit || !S.nt) {
                R.result(hit);
                continue;
            }
            rb = ray_box(o, d, S.dir_zero);
            tmin_box = tmin * ORX_BOX_TMIN, tmax_box = tmax * ORX_BOX_TMAX;
            sp = 0;
            ref = 0;
            lf = 0;
            return true;
        }
        return false;
    };
    bool have = fetch();
    const __amdgpu_buffer_rsrc_t tr = orx_rsrc(S.tri_v);
    while (__ballot(have)) {
        if (!have) continue;
        /* one round of trace_any_t's speculative while-while */
        while (!(ref & ORX_LEAF) && ref != ORX_DONE) {
            float ct[4];
            uint32_t cc[4];
            node_test(S.bvh4, ref, rb, tmin_box, tmax_box, ct, cc);
            const int h0 = ct[0] != INFINITY, h1 = ct[1] != INFINITY, h2 = ct[2] != INFINITY, h3 = ct[3] != INFINITY;
            const uint32_t next = h3 ? cc[3] : h2 ? cc[2] : h1 ? cc[1] : h0 ? cc[0] : ORX_DONE;
            if (stk.shallow(sp, 4)) { /* the common case: the four entries in LDS */
                stk.put_l(sp, cc[0]);
                sp += h0;
                stk.put_l(sp, cc[1]);
                sp += h1;
                stk.put_l(sp, cc[2]);
                sp += h2;
                stk.put_l(sp, cc[3]);
                sp += h3;
                sp -= next != ORX_DONE;
                ref = next != ORX_DONE ? next : (sp ? stk.pop_l(sp) : ORX_DONE);
            } else {
                stk.put(sp, cc[0]);
                sp += h0;
                stk.put(sp, cc[1]);
                sp += h1;
                stk.put(sp, cc[2]);
                sp += h2;
                stk.put(sp, cc[3]);
                sp += h3;
                sp -= next != ORX_DONE;
                ref = next != ORX_DONE ? next : (sp ? stk.pop(sp) : ORX_DONE);
            }
            if ((ref & ORX_LEAF) && !(lf & ORX_LEAF)) {
                lf = ref;
                ref = sp ? stk.pop(sp) : ORX_DONE;
            }
            if (!__ballot(!(lf & ORX_LEAF))) break;
        }
        bool occl = false;
        while ((lf & ORX_LEAF) && !occl) {
            const uint32_t first = (lf & 0x7fffffffu) >> 3, cnt = (lf & 7u) + 1u;
            for (uint32_t k = first; k < first + cnt && !occl; k++) {
                float t, b, g;
                const uint32_t tb = k * 48u;
                occl = isect_tri(ld_f3(ld16(tr, tb)), ld_f3(ld16(tr, tb + 16)), ld_f3(ld16(tr, tb + 32)), o, d, tmin,
                                 tmax, t, b, g);
            }
            if (!occl) {
                lf = ref;
                if (ref & ORX_LEAF) ref = sp ? stk.pop(sp) : ORX_DONE;
            }
        }
        if (occl || ref == ORX_DONE) {
            R.result(occl);
            have = fetch();
        }
    }
}
template <class RAYS>
__device__ __forceinline__ void trace_any_chain(const DevScene& S, RAYS& R, uint32_t* stkp) {
    trace_any_chain_t(S, R, StackL{stkp});
}

}  // namespace orx
