/*
 * orx_kernels.hip — gfx950 kernels of the render core: the indirect radiance estimate over the
 * uniform photon grid, as the wave-union kernel k_ppm_gather_union and the per-lane kernel
 * k_ppm_gather (launch_ppm_gather chooses), the slab mode's tile list (k_gather_tiles,
 * k_tile_compact) and the sharded gather's hit-point export and attenuation (k_export_hp,
 * k_indirect_atten).  What the kernels assume of the grid (the order of the sorted planes, subofs,
 * dir_q8, the margin) is in orx_photon_grid.h; orx_grid.hip builds it.
 * The gather keeps the unit's old name and the other passes moved out of it: tests and tools
 * address the gather's source by this name (the ORX_W5_C* coefficients read from its text, the
 * inline-dot scan of tests/test_asm_hazards.py).
 *
 * One kernel per reference OptiX entry point / Thrust step, and the unit it lives in:
 *   k_rng_init          initRandomStateBuffer  (OptixRenderer_SpatialHash.cu:310-334)             orx_raypass.hip
 *   k_ppm_eye           PPM_RAYTRACE_PASS      (ppm/RayGeneratorPPM.cu:31-66)                     orx_raypass.hip
 *   k_ppm_photon        PPM_PHOTON_PASS        (ppm/PhotonGenerator.cu:81-128 + material          orx_raypass.hip
 *                       closest-hit photon programs) fused with the photon AABB
 *                       reduction of getPhotonsBoundingBox (SpatialHash.cu:123-128)
 *   k_grid_setup        cell size / grid dims  (SpatialHash.cu:229-249), on device                orx_raypass.hip
 *   k_bs_*              calculateHashCellsKernel + sort_by_key + exclusive_scan                   orx_grid.hip
 *                       (SpatialHash.cu:152-207) as an LDS bucket counting sort
 *   k_grid_permute      the sorted photon array, as SoA planes                                    orx_grid.hip
 *   k_ppm_gather_union  PPM_INDIRECT_RADIANCE_ESTIMATION_PASS (ppm/IndirectRadianceEstimation.cu:69-227),
 *                       wave-union form; k_ppm_gather the per-lane form (sharded gathers at N >= 8) here
 *   k_ppm_gather_hash   the same pass over the stochastic-hash photon map (:131-162)              orx_hash.hip
 *   k_slab_*            the sharded gather's spatial photon partition (no reference counterpart)  orx_slab.hip
 *   k_ppm_direct_output PPM_DIRECT + PPM_OUTPUT (ppm/DirectRadianceEstimation.cu:29-77, ppm/Output.cu:32-37) orx_raypass.hip
 *   k_pt                PT_RAYTRACE_PASS       (pt/RayGeneratorPT.cu:46-131)                      orx_raypass.hip
 * (the kd-tree photon map and its gather: orx_kdtree.hip; VCM: orx_vcm.hip, orx_vcm_merge.hip.)
 */
#include <cmath>
#include <cstdlib>

#include "orx_kernels_common.h"
#include "orx_photon_grid.h"

namespace orx {

/* ------------------------------------------------------------------ */
/* indirect radiance estimate: uniform-grid gather                     */
/* ------------------------------------------------------------------ */
/* XCD-aware tile order: block b runs on XCD b % 8; XCD k takes tiles [k per, (k+1) per) of the
 * image's tiles, or of the slab mode's list of tiles that gather here (a band of the image
 * would otherwise leave most XCDs idle when the rank's hit points cluster in the image).
 * gi.order = S > 0: the image's tiles taken in super-tiles of S x S tiles (super-tiles row-major,
 * tiles row-major inside), XCD k a contiguous run of that order, so the blocks an XCD runs at
 * once cover a patch S tiles tall instead of a strip one tile tall (fewer photon-plane lines
 * fetched into its L2 per tile).  false: no tile for this block. */
__host__ __device__ __forceinline__ uint32_t gather_order_count(uint32_t order, uint32_t ntx, uint32_t nty) {
    if (!order) return ntx * nty;
    return ((ntx + order - 1) / order) * ((nty + order - 1) / order) * order * order;
}
__device__ __forceinline__ bool gather_tile(const GatherIn& gi, uint32_t ntx, uint32_t ntiles, uint32_t& tile) {
    if (!gi.tile_list) {
        if (!gi.order) {
            const uint32_t per = (ntiles + 7) / 8;
            tile = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
            return true;
        }
        const uint32_t S = gi.order, nty = ntiles / ntx, nsx = (ntx + S - 1) / S;
        const uint32_t total = gather_order_count(S, ntx, nty), per = (total + 7) / 8;
        const uint32_t o = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
        if (o >= total) return false;
        const uint32_t st = o / (S * S), w = o - st * (S * S);
        const uint32_t tx = (st % nsx) * S + w % S, ty = (st / nsx) * S + w / S;
        if (tx >= ntx || ty >= nty) return false;
        tile = ty * ntx + tx;
        return true;
    }
    const uint32_t n = *gi.tile_count, per = (n + 7) / 8;
    const uint32_t i = blockIdx.x >> 3, k = (blockIdx.x & 7u) * per + i;
    if (i >= per || k >= n) return false;
    tile = gi.tile_list[k];
    return true;
}

/* Per-pixel gather, packed fp32: one lane per pixel, four 8x8 wave tiles per
 * 256-thread block (neighbouring lanes share photons in L1), tiles dealt to
 * the eight XCDs in contiguous bands (neighbouring tiles share one L2).
 *
 * The work of a lane is the list of sub-row chords of its window (see the
 * photon-grid layout in orx_photon_grid.h); the reference walks the (z,y) cell rows of the
 * window (IndirectRadianceEstimation.cu:95-129) and so would a nested loop
 * here, but then a wave runs, per row and sub-row, as long as its longest
 * lane: the sum of maxima.  Instead the chords are collected first (phase A:
 * up to GQ non-empty [first, end) photon ranges per lane, in LDS) and then
 * walked as one flat stream of batches (phase B), so the wave runs for the
 * maximum of the lanes' sums.  A batch is four consecutive photons, one
 * dwordx4 buffer load per SoA plane (one VGPR offset, plane offsets in
 * SGPRs), two photons per packed instruction:
 *   1. positions -> d^2 <= r^2 (the oracle's unfused operations);
 *   2. if any lane photon is within r: the int8 direction word -> facing
 *      test by v_dot4_i32_i8, exact fp32 directions only inside the band
 *      (DIRQ_BAND; same decisions as the exact test, by the bound at dir_q8);
 *   3. if any photon is accepted: powers, kernel weight, accumulation.
 * So the accepted photon set is bit-identical to the reference's; the kernel
 * weight (photonPower, :59-67) and the sums, which the device accumulates in
 * a different order anyway, use fused multiply-adds (within ~1e-7 per term).
 * The visit counters are the reference's whole-window counts (:113/:124). */
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4))); /* dword-aligned float4 */
__device__ __forceinline__ v2f lo2(float4 v) { return v2f{v.x, v.y}; }
__device__ __forceinline__ v2f hi2(float4 v) { return v2f{v.z, v.w}; }
__device__ __forceinline__ v2f lo2(f4u v) { return v2f{v.x, v.y}; }
__device__ __forceinline__ v2f hi2(f4u v) { return v2f{v.z, v.w}; }
/* sorted-photon plane load: one buffer resource over the planes, the plane's
 * byte offset in an SGPR (soffset) and the photon's byte offset in a VGPR, so
 * the loads of a batch share one address register */
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4u ldp(__amdgpu_buffer_rsrc_t rs, uint32_t so, uint32_t bo) {
    const u4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)bo, (int)so, 0);
    return f4u{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
}
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0; }

/* The reference's visit counters of a window (IndirectRadianceEstimation.cu:113/:124): every
 * (z,y) row from x_lo to x_hi, whole rows, two offset reads per row.  Eight rows' reads are
 * issued before any is used (one memory round trip per eight rows instead of per row). */
__device__ __forceinline__ void window_visits(const uint32_t* __restrict__ offsets, uint32_t gx, uint32_t gy,
                                              uint32_t x_lo, uint32_t x_hi, uint32_t y_lo, uint32_t ny,
                                              uint32_t z_lo, uint32_t nrows, uint32_t& dC, uint32_t& dP) {
    uint32_t z = z_lo, yy = y_lo;
    for (uint32_t t0 = 0; t0 < nrows; t0 += 8) {
        uint32_t a[8], b[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            a[k] = b[k] = 0;
            if (t0 + k < nrows) {
                const uint32_t from = x_lo + yy * gx + z * gx * gy;
                a[k] = offsets[from];
                b[k] = offsets[from + (x_hi - x_lo) + 1];
                if (++yy == y_lo + ny) yy = y_lo, z++;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) dP += b[k] - a[k];
    }
    dC += nrows;
}

/* photonPower (IndirectRadianceEstimation.cu:59-67), w = alpha*(1 - (1 - exp(-beta d^2 / 2r^2)) /
 * (1 - e^-beta)), evaluated as one degree-5 polynomial in u = d^2/r^2: the minimax fit of w(u) on
 * [0, 1] (relative error 7.7e-7; 1.2e-6 with fp32 coefficients and Horner rounding).  One v_pk_mul
 * and five v_pk_fma_f32 per pair of photons, the coefficients compile-time constants (SGPRs); the
 * accepted photons are decided by the exact distance test, so only the weights (and the sums,
 * summed in another order anyway) differ from the oracle's. */
constexpr float ORX_W5_C0 = 1.8179986476898193f, ORX_W5_C1 = -2.0686328411102295f;
constexpr float ORX_W5_C2 = 1.0091534852981567f, ORX_W5_C3 = -0.32518523931503296f;
constexpr float ORX_W5_C4 = 0.07352562248706818f, ORX_W5_C5 = -0.009477914310991764f;
__device__ __forceinline__ v2f weight2u(v2f u);
__device__ __forceinline__ v2f weight2(v2f ir2, v2f d2) { return weight2u(d2 * ir2); }
/* packed broadcasts through op_sel: `pair.lo - x`, `pair.hi - x`, `a * pair.lo`, `a * pair.hi`
 * on both halves of x / a.  The union kernel keeps its hit point, normal and 1/r^2 two to a
 * register pair (four pairs instead of seven broadcast pairs: the kernel's VGPR budget sets its
 * waves per SIMD); the arithmetic is the same IEEE operation as the broadcast form. */
__device__ __forceinline__ v2f pk_sub_blo(v2f pair, v2f x) {
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(pair), "v"(x));
    return r;
}
__device__ __forceinline__ v2f pk_sub_bhi(v2f pair, v2f x) {
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(pair), "v"(x));
    return r;
}
__device__ __forceinline__ v2f pk_mul_blo(v2f a, v2f pair) {
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(pair));
    return r;
}
__device__ __forceinline__ v2f pk_mul_bhi(v2f a, v2f pair) {
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(pair));
    return r;
}
__device__ __forceinline__ v2f weight2u(v2f u) {
    v2f p = __builtin_elementwise_fma(v2f{ORX_W5_C5, ORX_W5_C5}, u, v2f{ORX_W5_C4, ORX_W5_C4});
    p = __builtin_elementwise_fma(p, u, v2f{ORX_W5_C3, ORX_W5_C3});
    p = __builtin_elementwise_fma(p, u, v2f{ORX_W5_C2, ORX_W5_C2});
    p = __builtin_elementwise_fma(p, u, v2f{ORX_W5_C1, ORX_W5_C1});
    return __builtin_elementwise_fma(p, u, v2f{ORX_W5_C0, ORX_W5_C0});
}
/* The union gather's form: the same polynomial in d^2 with coefficients c_k / r^(2k) (one radius per
 * launch: uniform, in SGPRs), so the u = d^2 / r^2 multiply per pair leaves the batch, and divided
 * through by the d^8 coefficient c_4 / r^8 (`scale`), so the first Horner step adds the inline
 * constant 1 (a coefficient pair in the first step would need a VGPR copy per batch: the packed
 * FMA reads one SGPR operand); the lane's sums are multiplied by `scale` once at the end.  The host
 * takes it only where the coefficients and the scale keep the sums in range (launch_ppm_gather). */
struct WPoly {
    float k[6]; /* k[4] = 1 */
    float scale;
};
__device__ __forceinline__ v2f weight2d(v2f d2, const WPoly& w) {
    v2f p = __builtin_elementwise_fma(v2f{w.k[5], w.k[5]}, d2, v2f{1.f, 1.f});
    p = __builtin_elementwise_fma(p, d2, v2f{w.k[3], w.k[3]});
    p = __builtin_elementwise_fma(p, d2, v2f{w.k[2], w.k[2]});
    p = __builtin_elementwise_fma(p, d2, v2f{w.k[1], w.k[1]});
    return __builtin_elementwise_fma(p, d2, v2f{w.k[0], w.k[0]});
}
/* int8 facing prefilter dot products of four photons' direction words with the hit point's nq.
 * gfx950 runs v_dot* like its matrix-core instructions: another VALU instruction may read a dot's
 * result only three wait states after it.  The compiler pads the instructions it emits but not
 * those inside inline assembly, so the four dots and the wait states are one asm block (outputs
 * early-clobbered: no dot overwrites a word a later one reads), with the inline 0 accumulator (the
 * builtin selects v_dot4c_i32_i8, whose accumulator costs a v_mov per dot: hall 1026 -> 1020
 * Mpaths/s).  A single-dot asm statement was correct only while the scheduler happened to put
 * three instructions between each dot and its compare; the two-hit-point gather variant's schedule
 * read a result one instruction later and dropped photons (profiles/r05h_gather_two_hitpoints_ab.txt).
 * tests/test_asm_hazards.py checks every inline dot of the compiled kernels. */
__device__ __forceinline__ void sdot4x4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int32_t nq, int32_t& q0,
                                        int32_t& q1, int32_t& q2, int32_t& q3) {
    asm("v_dot4_i32_i8 %0, %4, %8, 0\n\t"
        "v_dot4_i32_i8 %1, %5, %8, 0\n\t"
        "v_dot4_i32_i8 %2, %6, %8, 0\n\t"
        "v_dot4_i32_i8 %3, %7, %8, 0\n\t"
        "s_nop 2"
        : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(nq));
}

constexpr uint32_t GQ = 8; /* chord ranges per lane per phase A (LDS: GQ * 8 B per lane) */

/* the hit point's sphere (grown by a margin far above the rounding of the distance test) misses
 * the AABB of this rank's photons */
__device__ __forceinline__ bool sphere_misses_grid(const GridParams& g, f3 pos, float r) {
    const float m = r * 1e-3f + g.cell * GRID_MARGIN, rr = r + m;
    return pos.x + rr < g.clo[0] || pos.x - rr > g.chi[0] || pos.y + rr < g.clo[1] || pos.y - rr > g.chi[1] ||
           pos.z + rr < g.clo[2] || pos.z - rr > g.chi[2];
}
/* a hit point this rank does not gather: cull 1, its sphere misses the rank's photons; cull 2
 * (slab mode), its position's bin on the slab axis is another rank's (every photon within r of
 * an owned hit point was sent here with the halo, so owners gather complete windows) */
__device__ __forceinline__ bool gather_skips(const GatherIn& gi, const GridParams& g, f3 pos, float r) {
    if (gi.cull == 2) {
        const float v = gi.own_axis == 0 ? pos.x : gi.own_axis == 1 ? pos.y : pos.z;
        const uint32_t b = slab_bin(gi.own_sb, v, gi.own_axis);
        return b < gi.own_lo || b > gi.own_hi;
    }
    return gi.cull == 1 && sphere_misses_grid(g, pos, r);
}

/* NSUB: sub-rows per cell row (SUBR^2, or 1 for the cell-order layout) */
template <uint32_t NSUB>
#ifndef ORX_GATHER_LANE_WAVES
#define ORX_GATHER_LANE_WAVES 7 /* waves per SIMD the per-lane gather is register-capped for (72 VGPRs, no spills) */
#endif
__global__ __launch_bounds__(256, ORX_GATHER_LANE_WAVES) void k_ppm_gather(GatherIn gi, PhotonBufs pb, Consts c, uint32_t ntx,
                                                    uint32_t ntiles) {
    __shared__ uint2 rq[GQ][256];
    const uint32_t tid = threadIdx.x;
    uint32_t tile;
    if (!gather_tile(gi, ntx, ntiles, tile)) return; /* block-uniform */
    const uint32_t w = tid >> 6, l = tid & 63;
    const uint32_t x = (tile % ntx) * 16 + (w & 1) * 8 + (l & 7);
    const uint32_t y = (tile / ntx) * 16 + (w >> 1) * 8 + (l >> 3);
    const uint32_t j = gather_row(gi, y);
    const GridParams g = *pb.grid;
    uint32_t dC = 0, dP = 0;
    ORX_TS_DECL;
    /* The lane's window (here) and its sub-row chord (phase A) are written out again in
     * k_ppm_gather_union, and a change to either is made in both.  As shared forceinline functions
     * (the window as a struct of the bounds, the chord as quarter indices and the cut flag) they
     * compiled to other register allocations: this kernel went from 0 to 4 spilled VGPRs with the
     * window alone and to 10-12 with the chord too, at its 72-VGPR cap; the union kernel's VGPR and
     * spill counts moved as well. */
    const bool live = tile < ntiles && x < gi.W && y < gi.segments * gi.seg_rows;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    float2 Cc = make_float2(0.f, 0.f);
    size_t i = 0;
    if (live) {
        i = (size_t)j * gi.W + x;
        hp_load(gi, j, x, A, B, Cc);
    }
    const uint32_t flags = __float_as_uint(A.w);
    const f3 pos = mk(A.x, A.y, A.z);
    const float radius2 = c.ppm_radius2;
    const float radius = c.ppm_radius;
    const float invCellSize = 1.f / g.cell;
    const f3 np = pos - mk(g.ox, g.oy, g.oz);
    uint32_t x_lo = 0, x_hi = 0, y_lo = 0, z_lo = 0, ny = 0, nrows = 0;
    if (live && (flags & PRD_HIT_NON_SPECULAR) && g.G && !gather_skips(gi, g, pos, radius)) {
        const int32_t ixl = orx_f2i_sat((np.x - radius) * invCellSize);
        const int32_t iyl = orx_f2i_sat((np.y - radius) * invCellSize);
        const int32_t izl = orx_f2i_sat((np.z - radius) * invCellSize);
        x_lo = (uint32_t)(ixl > 0 ? ixl : 0);
        y_lo = (uint32_t)(iyl > 0 ? iyl : 0);
        z_lo = (uint32_t)(izl > 0 ? izl : 0);
        const uint32_t ux = orx_f2u_sat((np.x + radius) * invCellSize);
        const uint32_t uy = orx_f2u_sat((np.y + radius) * invCellSize);
        const uint32_t uz = orx_f2u_sat((np.z + radius) * invCellSize);
        x_hi = (g.gx - 1) < ux ? (g.gx - 1) : ux;
        const uint32_t y_hi = (g.gy - 1) < uy ? (g.gy - 1) : uy;
        const uint32_t z_hi = (g.gz - 1) < uz ? (g.gz - 1) : uz;
        if (x_lo <= x_hi && y_lo <= y_hi && z_lo <= z_hi) {
            ny = y_hi - y_lo + 1;
            nrows = (z_hi - z_lo + 1) * ny;
            if (gi.visits) window_visits(pb.offsets, g.gx, g.gy, x_lo, x_hi, y_lo, ny, z_lo, nrows, dC, dP);
        }
    }
    const v2f irr = v2f{1.0f / radius2, 0.f}; /* pairs broadcast through op_sel (pk_sub_blo ...) */
    v2f accx = v2f{0.f, 0.f}, accy = accx, accz = accx;
    const v2f pxy = v2f{pos.x, pos.y}, pzn = v2f{pos.z, B.x}, nyz = v2f{B.y, B.z};
    const int32_t nq = (int32_t)dir_q8(B.x, B.y, B.z);
    /* SP_PLANES * splane * 4 < 4 GiB: checked on the host (resize) */
    const __amdgpu_buffer_rsrc_t SR = __builtin_amdgcn_make_buffer_rsrc((void*)pb.sorted, 0, 0xffffffff, 0x00020000);
    const uint32_t PB = pb.splane * 4u;
    /* a sub-row's box grown by m (covers the rounding of the cell / half-cell
     * assignment) that misses the sphere holds no photon within r; otherwise
     * only the x quarters the chord [p.x - rx, p.x + rx] (+m) touches are walked */
    const float m = g.cell * GRID_MARGIN;
    constexpr uint32_t HS = NSUB > 1 ? SUBR : 1u;
    const float hc = g.cell / (float)HS; /* exact: HS is 1 or 2 */
    uint32_t t = 0;
    while (wave_any(t < nrows)) {
        /* phase A: the next up to GQ non-empty chords of this lane's window, in LDS */
        ORX_TS_WAVE(ts_wl); /* trav stats: wave-level phase-A rounds */
        uint32_t n = 0;
        while (t < nrows && n + NSUB <= GQ) {
            const uint32_t zq = t / ny;
            const uint32_t z = z_lo + zq, yy = y_lo + (t - zq * ny);
            t++;
            uint32_t offs[NSUB], ends[NSUB];
#pragma unroll
            for (uint32_t sr = 0; sr < NSUB; sr++) {
                offs[sr] = ends[sr] = 0;
                const uint32_t hz = z * HS + sr / HS, hy = yy * HS + sr % HS;
                const float zc0 = g.oz + (float)hz * hc - m, zc1 = g.oz + (float)(hz + 1) * hc + m;
                const float dz = fmaxf(0.f, fmaxf(zc0 - pos.z, pos.z - zc1));
                const float yc0 = g.oy + (float)hy * hc - m, yc1 = g.oy + (float)(hy + 1) * hc + m;
                const float dy = fmaxf(0.f, fmaxf(yc0 - pos.y, pos.y - yc1));
                const float rem = radius2 - dy * dy - dz * dz;
                if (rem < 0.f) continue;
                const float rx = sqrtf(rem) + m;
                const int32_t cxl = orx_f2i_sat(orx_floorf((np.x - rx) * invCellSize));
                const int32_t cxh = orx_f2i_sat(orx_floorf((np.x + rx) * invCellSize));
                const uint32_t xl = cxl > (int32_t)x_lo ? (uint32_t)cxl : x_lo;
                const uint32_t xh = cxh < (int32_t)x_hi ? (uint32_t)cxh : x_hi;
                if (cxh < 0 || xl > xh) continue;
                /* x-quarter trimming of the chord's end cells */
                const float sx = invCellSize * (float)SUBX;
                const int32_t q0 = orx_f2i_sat(orx_floorf((np.x - rx) * sx));
                const int32_t q1 = orx_f2i_sat(orx_floorf((np.x + rx) * sx));
                const uint32_t a0 = q0 > (int32_t)(SUBX * xl) ? (uint32_t)q0 : SUBX * xl;
                const uint32_t a1 = q1 < (int32_t)(SUBX * xh + SUBX - 1) ? (uint32_t)q1 : SUBX * xh + SUBX - 1;
                if (q1 < 0 || a0 > a1) continue;
                const uint32_t* so = pb.subofs + ((size_t)(yy + z * g.gy) * NSUB + sr) * g.gx * SUBX;
                offs[sr] = so[a0];
                ends[sr] = so[a1 + 1];
            }
#pragma unroll
            for (uint32_t sr = 0; sr < NSUB; sr++)
                if (ends[sr] > offs[sr]) rq[n++][tid] = make_uint2(offs[sr], ends[sr]);
        }
        /* phase B: one flat stream of batches over the collected chords */
        uint32_t k = 0, kb = 0, kend = 0;
        for (;;) {
            while (kb >= kend && k < n) {
                const uint2 r = rq[k++][tid];
                kb = r.x;
                kend = r.y;
                ORX_TS_INC(ts_leaves, 1);
            }
            const bool has = kb < kend;
            if (!wave_any(has)) break;
            if (!has) continue;
            ORX_TS_INC(ts_nodes, 1);
            ORX_TS_WAVE(ts_wn);
            const uint32_t bo = kb << 2;
            const f4u X = ldp(SR, SP_X * PB, bo), Y = ldp(SR, SP_Y * PB, bo), Z = ldp(SR, SP_Z * PB, bo);
            const v2f dx0 = pk_sub_blo(pxy, lo2(X)), dx1 = pk_sub_blo(pxy, hi2(X));
            const v2f dy0 = pk_sub_bhi(pxy, lo2(Y)), dy1 = pk_sub_bhi(pxy, hi2(Y));
            const v2f dz0 = pk_sub_blo(pzn, lo2(Z)), dz1 = pk_sub_blo(pzn, hi2(Z));
            const v2f d20 = (dx0 * dx0 + dy0 * dy0) + dz0 * dz0;
            const v2f d21 = (dx1 * dx1 + dy1 * dy1) + dz1 * dz1;
            bool in0 = d20.x <= radius2;
            bool in1 = kb + 1 < kend && d20.y <= radius2;
            bool in2 = kb + 2 < kend && d21.x <= radius2;
            bool in3 = kb + 3 < kend && d21.y <= radius2;
            kb += 4;
            if (!(in0 | in1 | in2 | in3)) continue;
            /* facing: dot(-dir, n) >= 0  <=>  dot(dir, n) <= 0 (negation is exact) */
            const u4v Q = __builtin_amdgcn_raw_buffer_load_b128(SR, (int)bo, (int)(SP_DIRQ * PB), 0);
            int32_t q0, q1, q2, q3;
            sdot4x4(Q.x, Q.y, Q.z, Q.w, nq, q0, q1, q2, q3);
            in0 = in0 && q0 <= DIRQ_BAND;
            in1 = in1 && q1 <= DIRQ_BAND;
            in2 = in2 && q2 <= DIRQ_BAND;
            in3 = in3 && q3 <= DIRQ_BAND;
            const bool u0 = in0 && q0 >= -DIRQ_BAND, u1 = in1 && q1 >= -DIRQ_BAND;
            const bool u2 = in2 && q2 >= -DIRQ_BAND, u3 = in3 && q3 >= -DIRQ_BAND;
            if (u0 | u1 | u2 | u3) { /* inside the band: the exact test */
                const f4u DX = ldp(SR, SP_DX * PB, bo), DY = ldp(SR, SP_DY * PB, bo), DZ = ldp(SR, SP_DZ * PB, bo);
                const v2f nd0 = (pk_mul_bhi(lo2(DX), pzn) + pk_mul_blo(lo2(DY), nyz)) + pk_mul_bhi(lo2(DZ), nyz);
                const v2f nd1 = (pk_mul_bhi(hi2(DX), pzn) + pk_mul_blo(hi2(DY), nyz)) + pk_mul_bhi(hi2(DZ), nyz);
                in0 = in0 && (!u0 || nd0.x <= 0.f);
                in1 = in1 && (!u1 || nd0.y <= 0.f);
                in2 = in2 && (!u2 || nd1.x <= 0.f);
                in3 = in3 && (!u3 || nd1.y <= 0.f);
            }
            if (!(in0 | in1 | in2 | in3)) continue;
            const f4u WX = ldp(SR, SP_PX * PB, bo), WY = ldp(SR, SP_PY * PB, bo), WZ = ldp(SR, SP_PZ * PB, bo);
            /* the weight of every photon of the batch (rejected ones get 0 by select) */
            v2f w0 = weight2u(pk_mul_blo(d20, irr)), w1 = weight2u(pk_mul_blo(d21, irr));
            ORX_TS_INC(ts_tris, (uint32_t)in0 + (uint32_t)in1 + (uint32_t)in2 + (uint32_t)in3);
            w0.x = in0 ? w0.x : 0.f;
            w0.y = in1 ? w0.y : 0.f;
            w1.x = in2 ? w1.x : 0.f;
            w1.y = in3 ? w1.y : 0.f;
            accx = __builtin_elementwise_fma(lo2(WX), w0, accx);
            accy = __builtin_elementwise_fma(lo2(WY), w0, accy);
            accz = __builtin_elementwise_fma(lo2(WZ), w0, accz);
            accx = __builtin_elementwise_fma(hi2(WX), w1, accx);
            accy = __builtin_elementwise_fma(hi2(WY), w1, accy);
            accz = __builtin_elementwise_fma(hi2(WZ), w1, accz);
        }
    }
    /* gather_store and gather_count (orx_kernels_common.h) written out, here and in the union kernel:
     * a change to either half is made in both.  Calling them left this kernel's counts as they were
     * in the product build but took the cell-order instance of the ORX_TRAV_STATS build from 22 to
     * 34 spilled VGPRs. */
    if (live) {
        const float ax = accx.x + accx.y, ay = accy.x + accy.y, az = accz.x + accz.y;
        const f3 att = mk(B.w, Cc.x, Cc.y);
        const float s1 = 1.0f / (ORX_PI_F * c.ppm_radius2);
        const float s2 = 1.0f / c.emitted_f;
        const f3 ind = ((mk(ax, ay, az) * att) * s1) * s2;
        gi.indirect[3 * i + 0] = ind.x;
        gi.indirect[3 * i + 1] = ind.y;
        gi.indirect[3 * i + 2] = ind.z;
        if (gi.dbg) {
            gi.dbg[2 * i] = dC;
            gi.dbg[2 * i + 1] = dP;
        }
    }
#ifdef ORX_TRAV_STATS
    atomicAdd((unsigned long long*)&pb.grid->st_lane_batches, (unsigned long long)ts_nodes);
    atomicAdd((unsigned long long*)&pb.grid->st_wave_batches, (unsigned long long)ts_wn);
    atomicAdd((unsigned long long*)&pb.grid->st_lane_rows, (unsigned long long)ts_leaves);
    atomicAdd((unsigned long long*)&pb.grid->st_wave_rows, (unsigned long long)ts_wl);
    atomicAdd((unsigned long long*)&pb.grid->st_accepted, (unsigned long long)ts_tris);
#endif
    const uint64_t sp = wave_sum_u64(dP), sc = wave_sum_u64(dC);
    if ((threadIdx.x & 63) == 0 && sp) {
        atomicAdd((unsigned long long*)&pb.grid->photons_visited, (unsigned long long)sp);
        atomicAdd((unsigned long long*)&pb.grid->cells_visited, (unsigned long long)sc);
        atomicAdd((unsigned long long*)&pb.grid->photons_visited_total, (unsigned long long)sp);
        atomicAdd((unsigned long long*)&pb.grid->cells_visited_total, (unsigned long long)sc);
    }
}

/* Wave-broadcast gather over the union of a wave's chords.
 *
 * The per-lane gather above is bound by the vector-memory address path: every
 * dwordx4 photon load costs the TA ~16-20 cycles whatever the lanes share, for
 * four photons of one lane.  Here a wave walks, sub-row by sub-row, the union
 * of its 64 lanes' chords and reads each photon ONCE: 64 photons per coalesced
 * load into the wave's LDS image, then every lane reads the same batch of four
 * (ds_read_b128 broadcast), so the cost per photon is the lanes' arithmetic
 * (union_chunk_lds; only the exact directions inside the facing band are
 * scalar loads).
 * Each lane accepts exactly the photons of its own chord range (the per-lane
 * kernel's candidate set, [subofs[a0], subofs[a1 + 1]) inside its reference
 * window) that pass its distance and facing tests, so the accepted set per
 * pixel is the per-lane kernel's (= the reference's); the union only adds
 * photons a lane rejects.  Lanes are 8x8 pixel tiles (hitpoints of neighbouring
 * pixels are near each other in the scene).
 * Per batch of four photons: positions -> d^2 test and the lane's range test;
 * a batch no lane accepts ends there (one ballot); then the int8 direction
 * words -> facing, exact directions only inside the band; then powers. */
/* Wave-uniform min / max over the 64 lanes (callers run with EXEC all ones): DPP moves inside
 * each row of 16 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_ror 4, row_ror 8: VALU operands, no
 * LDS round trip), then the four row results by v_readlane and scalar min/max.  A __shfl_xor
 * butterfly is six dependent ds_bpermute_b32 round trips; the union gather reduces twice per
 * sub-row. */
template <bool MIN>
__device__ __forceinline__ uint32_t wave_minmax_u32(uint32_t v) {
    auto op = [](uint32_t a, uint32_t b) { return MIN ? min(a, b) : max(a, b); };
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false));
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    const uint32_t r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    const uint32_t r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return wave_minmax_u32<true>(v); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_minmax_u32<false>(v); }
/* uniform 16-B read of a photon plane through the scalar unit */
__device__ __forceinline__ f4u sload4(const float* __restrict__ plane, uint32_t k) {
    return *reinterpret_cast<const f4u*>(plane + k);
}
__device__ __forceinline__ u4v sload4u(const float* __restrict__ plane, uint32_t k) {
    return *reinterpret_cast<const u4v*>(plane + k);
}
struct UChunk { /* lane k: photon c + k of the chunk */
    float X, Y, Z, WX, WY, WZ;
    uint32_t Q;
};
__device__ __forceinline__ UChunk uload_chunk(const float* __restrict__ SX, const float* __restrict__ SY,
                                              const float* __restrict__ SZ, const float* __restrict__ SQ,
                                              const float* __restrict__ SPX, const float* __restrict__ SPY,
                                              const float* __restrict__ SPZ, uint32_t k) {
    UChunk b;
    b.X = SX[k];
    b.Y = SY[k];
    b.Z = SZ[k];
    b.Q = __float_as_uint(SQ[k]);
    b.WX = SPX[k];
    b.WY = SPY[k];
    b.WZ = SPZ[k];
    return b;
}
/* The union kernel's per-batch constants and accumulators (LDS-broadcast form) */
struct UAcc {
    v2f accx, accy, accz;
};
struct UConst {
    v2f pxy, pzn, nyz, irr; /* (p.x, p.y), (p.z, n.x), (n.y, n.z), (1/r^2, -) */
    int32_t nq;
    const float* SDX;
    const float* SDY;
    const float* SDZ;
};
/* One 64-photon chunk of a sub-row's union, staged in the wave's LDS image L[7][64]
 * (x y z dirq px py pz; slots past the sub-row's end hold x = +inf, so no lane can
 * accept them).  Batches of four photons are read by every lane from the same LDS
 * address (ds_read_b128 broadcast: LDS-array cycles, no VALU), then:
 *   d^2 <= r2 (r2 = -1 for a lane without a chord on this sub-row), and with RANGE the
 *   lane's chord test [lo, lo + len); the facing prefilter; the weight and sums.
 * RANGE = false when every lane's chord is its whole margin-grown extent on the
 * sub-row (not cut by its reference window): then a union photon outside the chord
 * is farther than r from the lane's hit point (the margin argument of the chord
 * trimming), so the distance test alone decides, as the per-lane kernel's chord +
 * distance tests do. */
template <bool RANGE, bool DF>
__device__ __forceinline__ void union_chunk_lds(const float* __restrict__ L, uint32_t c, uint32_t ce, uint32_t lo,
                                                uint32_t len, float r2, const UConst& k, const WPoly& wp, UAcc& a) {
    const float4* L4 = reinterpret_cast<const float4*>(L);
    /* one batch of four; two per loop step, so the second batch's LDS reads take the first's address
     * plus an offset (one address increment per two batches) */
    auto batch = [&](const uint32_t e) {
        const uint32_t kb = c + e;
        const float4 X = L4[e >> 2], Y = L4[16 + (e >> 2)], Z = L4[32 + (e >> 2)];
        const v2f dx0 = pk_sub_blo(k.pxy, lo2(X)), dx1 = pk_sub_blo(k.pxy, hi2(X));
        const v2f dy0 = pk_sub_bhi(k.pxy, lo2(Y)), dy1 = pk_sub_bhi(k.pxy, hi2(Y));
        const v2f dz0 = pk_sub_blo(k.pzn, lo2(Z)), dz1 = pk_sub_blo(k.pzn, hi2(Z));
        const v2f d20 = (dx0 * dx0 + dy0 * dy0) + dz0 * dz0;
        const v2f d21 = (dx1 * dx1 + dy1 * dy1) + dz1 * dz1;
        bool in0 = d20.x <= r2, in1 = d20.y <= r2, in2 = d21.x <= r2, in3 = d21.y <= r2;
        if (RANGE) {
            const uint32_t t = kb - lo;
            in0 = in0 && t < len;
            in1 = in1 && t + 1 < len;
            in2 = in2 && t + 2 < len;
            in3 = in3 && t + 3 < len;
        }
        if (!wave_any(in0 | in1 | in2 | in3)) return;
        const uint4 Q = reinterpret_cast<const uint4*>(L4)[48 + (e >> 2)];
        int32_t q0, q1, q2, q3;
        sdot4x4(Q.x, Q.y, Q.z, Q.w, k.nq, q0, q1, q2, q3);
        in0 = in0 && q0 <= DIRQ_BAND;
        in1 = in1 && q1 <= DIRQ_BAND;
        in2 = in2 && q2 <= DIRQ_BAND;
        in3 = in3 && q3 <= DIRQ_BAND;
        const bool u0 = in0 && q0 >= -DIRQ_BAND, u1 = in1 && q1 >= -DIRQ_BAND;
        const bool u2 = in2 && q2 >= -DIRQ_BAND, u3 = in3 && q3 >= -DIRQ_BAND;
        /* The two tests below are lane-divergent ifs, not wave_any: the exec-mask save and skip is
         * scalar, where a ballot of these combined masks compiled to a select and a compare (two
         * VALU each, of ~56 per batch).  A lane that skips the sums adds fma(w, 0, acc) = acc. */
        if (u0 | u1 | u2 | u3) { /* inside the band: the exact test (rare) */
            const uint32_t ku = (uint32_t)__builtin_amdgcn_readfirstlane((int)kb);
            const f4u DX = sload4(k.SDX, ku), DY = sload4(k.SDY, ku), DZ = sload4(k.SDZ, ku);
            const v2f nd0 = (pk_mul_bhi(lo2(DX), k.pzn) + pk_mul_blo(lo2(DY), k.nyz)) + pk_mul_bhi(lo2(DZ), k.nyz);
            const v2f nd1 = (pk_mul_bhi(hi2(DX), k.pzn) + pk_mul_blo(hi2(DY), k.nyz)) + pk_mul_bhi(hi2(DZ), k.nyz);
            in0 = in0 && (!u0 || nd0.x <= 0.f);
            in1 = in1 && (!u1 || nd0.y <= 0.f);
            in2 = in2 && (!u2 || nd1.x <= 0.f);
            in3 = in3 && (!u3 || nd1.y <= 0.f);
        }
        if (in0 | in1 | in2 | in3) {
            const float4 WX = L4[64 + (e >> 2)], WY = L4[80 + (e >> 2)], WZ = L4[96 + (e >> 2)];
            v2f w0, w1;
            if (DF) {
                w0 = weight2d(d20, wp);
                w1 = weight2d(d21, wp);
            } else {
                w0 = weight2u(pk_mul_blo(d20, k.irr));
                w1 = weight2u(pk_mul_blo(d21, k.irr));
            }
            w0.x = in0 ? w0.x : 0.f;
            w0.y = in1 ? w0.y : 0.f;
            w1.x = in2 ? w1.x : 0.f;
            w1.y = in3 ? w1.y : 0.f;
            a.accx = __builtin_elementwise_fma(lo2(WX), w0, a.accx);
            a.accy = __builtin_elementwise_fma(lo2(WY), w0, a.accy);
            a.accz = __builtin_elementwise_fma(lo2(WZ), w0, a.accz);
            a.accx = __builtin_elementwise_fma(hi2(WX), w1, a.accx);
            a.accy = __builtin_elementwise_fma(hi2(WY), w1, a.accy);
            a.accz = __builtin_elementwise_fma(hi2(WZ), w1, a.accz);
        }
    };
    for (uint32_t e = 0; e < ce; e += 8) {
        batch(e);
        if (e + 4 < ce) batch(e + 4);
    }
}


/* Photons are broadcast through the wave's LDS image (union_chunk_lds), with the chord test
 * dropped on sub-rows where no lane's chord is cut by its window.  (A v_readlane broadcast from
 * the chunk registers measured 2.81 ms against 1.91 on the serial hall gather, 16x4 and 4x16
 * wave tiles slower than 8x8.)  Block = 16x16 pixels, four 8x8 wave tiles; blocks are dealt
 * XCD-major (block b runs on XCD b % 8 and takes the tiles [k per, (k+1) per) of XCD k). */
/* 7 waves per SIMD (at most 72 VGPRs): the next chunk's loads are not issued ahead of the
 * current chunk's batches (that prefetch held 7 VGPRs and kept the kernel at 5 waves), and the
 * hit point, normal and 1/r^2 sit two to a register pair, broadcast by op_sel (pk_sub_blo ...);
 * the extra waves hide more of the load latency than the prefetch did: 4K conference serial
 * gather 26.2 -> 24.7 ms at 6 waves, 24.2 at 7; configs[4] 8-rank gather 6.39 -> 6.01 ms; hall
 * unchanged.  The cell-order instance spills 8 VGPRs outside the batch loop. */
#ifndef ORX_UNION_WAVES
#define ORX_UNION_WAVES 7 /* waves per SIMD the union gather is register-capped for (at 8 it spills 37-49 VGPRs) */
#endif
template <uint32_t NSUB, bool DF>
__global__ __launch_bounds__(256, ORX_UNION_WAVES) void k_ppm_gather_union(GatherIn gi, PhotonBufs pb, Consts c, uint32_t ntx,
                                                          uint32_t ntiles, WPoly wp) {
    __shared__ float ulds[4][7 * 64];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    uint32_t tile;
    if (!gather_tile(gi, ntx, ntiles, tile)) return; /* block-uniform */
    const uint32_t x = (tile % ntx) * 16 + (w & 1) * 8 + (l & 7);
    const uint32_t y = (tile / ntx) * 16 + (w >> 1) * 8 + (l >> 3);
    const uint32_t j = gather_row(gi, y);
    const bool live = tile < ntiles && x < gi.W && y < gi.segments * gi.seg_rows;
    const GridParams g = *pb.grid;
    uint32_t dC = 0, dP = 0;
    ORX_TS_DECL;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    float2 Cc = make_float2(0.f, 0.f);
    size_t i = 0;
    if (live) {
        i = (size_t)j * gi.W + x;
        hp_load(gi, j, x, A, B, Cc);
    }
    const uint32_t flags = __float_as_uint(A.w);
    const f3 pos = mk(A.x, A.y, A.z);
    const float radius2 = c.ppm_radius2;
    const float radius = c.ppm_radius;
    const float invCellSize = 1.f / g.cell;
    const f3 np = pos - mk(g.ox, g.oy, g.oz);
    uint32_t x_lo = 1, x_hi = 0, y_lo = 1, y_hi = 0, z_lo = 1, z_hi = 0;
    bool act = false;
    if (live && (flags & PRD_HIT_NON_SPECULAR) && g.G && !gather_skips(gi, g, pos, radius)) {
        const int32_t ixl = orx_f2i_sat((np.x - radius) * invCellSize);
        const int32_t iyl = orx_f2i_sat((np.y - radius) * invCellSize);
        const int32_t izl = orx_f2i_sat((np.z - radius) * invCellSize);
        x_lo = (uint32_t)(ixl > 0 ? ixl : 0);
        y_lo = (uint32_t)(iyl > 0 ? iyl : 0);
        z_lo = (uint32_t)(izl > 0 ? izl : 0);
        const uint32_t ux = orx_f2u_sat((np.x + radius) * invCellSize);
        const uint32_t uy = orx_f2u_sat((np.y + radius) * invCellSize);
        const uint32_t uz = orx_f2u_sat((np.z + radius) * invCellSize);
        x_hi = (g.gx - 1) < ux ? (g.gx - 1) : ux;
        y_hi = (g.gy - 1) < uy ? (g.gy - 1) : uy;
        z_hi = (g.gz - 1) < uz ? (g.gz - 1) : uz;
        act = x_lo <= x_hi && y_lo <= y_hi && z_lo <= z_hi;
        if (act && gi.visits) /* the reference's visit counters: every (z,y) row of the window, whole rows */
            window_visits(pb.offsets, g.gx, g.gy, x_lo, x_hi, y_lo, y_hi - y_lo + 1, z_lo,
                          (z_hi - z_lo + 1) * (y_hi - y_lo + 1), dC, dP);
    }
    v2f accx = v2f{0.f, 0.f}, accy = accx, accz = accx;
    const int32_t nq = (int32_t)dir_q8(B.x, B.y, B.z);
    const float* __restrict__ SX = pb.sorted + (size_t)SP_X * pb.splane;
    const float* __restrict__ SY = pb.sorted + (size_t)SP_Y * pb.splane;
    const float* __restrict__ SZ = pb.sorted + (size_t)SP_Z * pb.splane;
    const float* __restrict__ SQ = pb.sorted + (size_t)SP_DIRQ * pb.splane;
    const float* __restrict__ SDX = pb.sorted + (size_t)SP_DX * pb.splane;
    const float* __restrict__ SDY = pb.sorted + (size_t)SP_DY * pb.splane;
    const float* __restrict__ SDZ = pb.sorted + (size_t)SP_DZ * pb.splane;
    const float* __restrict__ SPX = pb.sorted + (size_t)SP_PX * pb.splane;
    const float* __restrict__ SPY = pb.sorted + (size_t)SP_PY * pb.splane;
    const float* __restrict__ SPZ = pb.sorted + (size_t)SP_PZ * pb.splane;
    const float m = g.cell * GRID_MARGIN;
    constexpr uint32_t HS = NSUB > 1 ? SUBR : 1u;
    const float hc = g.cell / (float)HS;
    const UConst UK{v2f{pos.x, pos.y}, v2f{pos.z, B.x}, v2f{B.y, B.z}, v2f{1.0f / radius2, 0.f}, nq, SDX, SDY, SDZ};
    UAcc UA{accx, accy, accz};
    /* the union of the lanes' windows (rows) */
    const uint32_t UZ0 = wave_min_u32(act ? z_lo : 0xffffffffu), UZ1 = wave_max_u32(act ? z_hi : 0u);
    const uint32_t UY0 = wave_min_u32(act ? y_lo : 0xffffffffu), UY1 = wave_max_u32(act ? y_hi : 0u);
    for (uint32_t z = UZ0; z <= UZ1 && UZ0 <= UZ1; z++) {
        for (uint32_t yy = UY0; yy <= UY1; yy++) {
            const bool inrow = act && z >= z_lo && z <= z_hi && yy >= y_lo && yy <= y_hi;
            const uint32_t rowc = yy + z * g.gy;
            for (uint32_t sr = 0; sr < NSUB; sr++) {
                /* this lane's chord on the sub-row (the per-lane kernel's), as quarter indices;
                 * cut: the chord is shorter than the margin-grown extent [q0, q1] inside the grid
                 * (its reference window ends inside it) */
                uint32_t a0 = 0xffffffffu, a1 = 0u;
                bool cut = false;
                if (inrow) {
                    const uint32_t hz = z * HS + sr / HS, hy = yy * HS + sr % HS;
                    const float zc0 = g.oz + (float)hz * hc - m, zc1 = g.oz + (float)(hz + 1) * hc + m;
                    const float dz = fmaxf(0.f, fmaxf(zc0 - pos.z, pos.z - zc1));
                    const float yc0 = g.oy + (float)hy * hc - m, yc1 = g.oy + (float)(hy + 1) * hc + m;
                    const float dy = fmaxf(0.f, fmaxf(yc0 - pos.y, pos.y - yc1));
                    const float rem = radius2 - dy * dy - dz * dz;
                    if (rem >= 0.f) {
                        const float rx = sqrtf(rem) + m;
                        const int32_t cxl = orx_f2i_sat(orx_floorf((np.x - rx) * invCellSize));
                        const int32_t cxh = orx_f2i_sat(orx_floorf((np.x + rx) * invCellSize));
                        const uint32_t xl = cxl > (int32_t)x_lo ? (uint32_t)cxl : x_lo;
                        const uint32_t xh = cxh < (int32_t)x_hi ? (uint32_t)cxh : x_hi;
                        if (cxh >= 0 && xl <= xh) {
                            const float sx = invCellSize * (float)SUBX;
                            const int32_t q0 = orx_f2i_sat(orx_floorf((np.x - rx) * sx));
                            const int32_t q1 = orx_f2i_sat(orx_floorf((np.x + rx) * sx));
                            const uint32_t b0 = q0 > (int32_t)(SUBX * xl) ? (uint32_t)q0 : SUBX * xl;
                            const uint32_t b1 =
                                q1 < (int32_t)(SUBX * xh + SUBX - 1) ? (uint32_t)q1 : SUBX * xh + SUBX - 1;
                            if (q1 >= 0 && b0 <= b1) {
                                a0 = b0;
                                a1 = b1;
                                const int32_t qmax = (int32_t)(SUBX * g.gx) - 1;
                                cut = (int32_t)b0 > (q0 > 0 ? q0 : 0) || (int32_t)b1 < (q1 < qmax ? q1 : qmax);
                            }
                        }
                    }
                }
                const uint32_t A0 = wave_min_u32(a0), A1 = wave_max_u32(a1);
                if (A0 > A1) continue;
                if (l == 0) ORX_TS_INC(ts_wl, 1); /* trav stats: sub-rows a wave walks */
                const uint32_t* so = pb.subofs + ((size_t)rowc * NSUB + sr) * g.gx * SUBX;
                const uint32_t U0 = so[A0], U1 = so[A1 + 1]; /* uniform: scalar loads */
                if (U0 >= U1) continue;
                if (l == 0) ORX_TS_INC(ts_tris, 1); /* trav stats (union kernel): sub-rows with photons */
                /* this lane's candidates [lo, lo + len): needed only on sub-rows where some lane's
                 * chord is cut (two scattered loads) */
#ifdef ORX_TRAV_STATS
                constexpr bool need_all = true;
#else
                constexpr bool need_all = false;
#endif
                const bool range = wave_any(cut);
                uint32_t lo = 0, len = 0;
                if ((need_all || range) && a0 <= a1) {
                    lo = so[a0];
                    len = so[a1 + 1] - lo;
                }
                ORX_TS_INC(ts_nodes, len);              /* trav stats: lane candidate photons */
                if (l == 0) ORX_TS_INC(ts_wn, U1 - U0); /* union photons of the wave */
                ORX_TS_INC(ts_leaves, 1);
                /* a lane without a chord here accepts nothing (its window excludes the
                 * sub-row, or its sphere misses it) */
                const float r2 = a0 <= a1 ? radius2 : -1.f;
                float* L = ulds[w];
                uint32_t cc = U0;
                while (cc < U1) {
                    const uint32_t cn = cc + 64;
                    const UChunk cur = uload_chunk(SX, SY, SZ, SQ, SPX, SPY, SPZ, cc + l);
                    const uint32_t ce = U1 - cc < 64 ? U1 - cc : 64;
                    L[l] = cc + l < U1 ? cur.X : INFINITY;
                    L[64 + l] = cur.Y;
                    L[128 + l] = cur.Z;
                    L[192 + l] = __uint_as_float(cur.Q);
                    L[256 + l] = cur.WX;
                    L[320 + l] = cur.WY;
                    L[384 + l] = cur.WZ;
                    __builtin_amdgcn_wave_barrier();
                    if (range) union_chunk_lds<true, DF>(L, cc, ce, lo, len, r2, UK, wp, UA);
                    else union_chunk_lds<false, DF>(L, cc, ce, lo, len, r2, UK, wp, UA);
                    __builtin_amdgcn_wave_barrier();
                    cc = cn;
                }
            }
        }
    }
    accx = UA.accx;
    accy = UA.accy;
    accz = UA.accz;
#ifdef ORX_TRAV_STATS
    atomicAdd((unsigned long long*)&pb.grid->st_lane_batches, (unsigned long long)ts_nodes);
    atomicAdd((unsigned long long*)&pb.grid->st_wave_batches, (unsigned long long)ts_wn);
    atomicAdd((unsigned long long*)&pb.grid->st_lane_rows, (unsigned long long)ts_leaves);
    atomicAdd((unsigned long long*)&pb.grid->st_wave_rows, (unsigned long long)ts_wl);
    atomicAdd((unsigned long long*)&pb.grid->st_accepted, (unsigned long long)ts_tris);
#endif
    /* gather_store and gather_count (orx_kernels_common.h) written out, as in the per-lane kernel:
     * calling them changes this kernel's SGPR spill count in all four instances (20 -> 18, 10 -> 8,
     * 27 -> 20, 15 -> 13), and its register allocation is not traded for tidiness. */
    if (live) {
        float ax = accx.x + accx.y, ay = accy.x + accy.y, az = accz.x + accz.y;
        if (DF) {
            ax *= wp.scale;
            ay *= wp.scale;
            az *= wp.scale;
        }
        const f3 att = mk(B.w, Cc.x, Cc.y);
        const float s1 = 1.0f / (ORX_PI_F * c.ppm_radius2);
        const float s2 = 1.0f / c.emitted_f;
        const f3 ind = ((mk(ax, ay, az) * att) * s1) * s2;
        gi.indirect[3 * i + 0] = ind.x;
        gi.indirect[3 * i + 1] = ind.y;
        gi.indirect[3 * i + 2] = ind.z;
        if (gi.dbg) {
            gi.dbg[2 * i] = dC;
            gi.dbg[2 * i + 1] = dP;
        }
    }
    const uint64_t sp = wave_sum_u64(dP), sc = wave_sum_u64(dC);
    if ((threadIdx.x & 63) == 0 && sp) {
        atomicAdd((unsigned long long*)&pb.grid->photons_visited, (unsigned long long)sp);
        atomicAdd((unsigned long long*)&pb.grid->cells_visited, (unsigned long long)sc);
        atomicAdd((unsigned long long*)&pb.grid->photons_visited_total, (unsigned long long)sp);
        atomicAdd((unsigned long long*)&pb.grid->cells_visited_total, (unsigned long long)sc);
    }
}

__global__ __launch_bounds__(256) void k_gather_tiles(GatherIn gi, PhotonBufs pb, Consts c, uint32_t ntx,
                                                      uint8_t* flags) {
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const uint32_t x = (tile % ntx) * 16 + (w & 1) * 8 + (l & 7);
    const uint32_t y = (tile / ntx) * 16 + (w >> 1) * 8 + (l >> 3);
    const uint32_t j = gather_row(gi, y);
    const bool live = x < gi.W && y < gi.segments * gi.seg_rows;
    const GridParams g = *pb.grid;
    bool act = false;
    if (live) {
        const float4 A = hp_load_a(gi, j, x);
        act = (__float_as_uint(A.w) & PRD_HIT_NON_SPECULAR) && g.G &&
              !gather_skips(gi, g, mk(A.x, A.y, A.z), c.ppm_radius);
    }
    const int any = __syncthreads_or(act);
    if (tid == 0) flags[tile] = (uint8_t)(any != 0);
    if (!any && live) {
        const size_t i = (size_t)j * gi.W + x;
        gi.indirect[3 * i + 0] = 0.f;
        gi.indirect[3 * i + 1] = 0.f;
        gi.indirect[3 * i + 2] = 0.f;
    }
}
/* one block: the flagged tiles in ascending order */
__global__ __launch_bounds__(1024) void k_tile_compact(const uint8_t* flags, uint32_t ntiles, uint32_t* list,
                                                       uint32_t* count) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t base;
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    if (tid == 0) base = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < ntiles; t0 += 1024) {
        const uint32_t t = t0 + tid;
        const bool f = t < ntiles && flags[t];
        const uint64_t m = __ballot(f);
        const uint32_t pre = (uint32_t)__popcll(m & ((1ull << l) - 1ull));
        if (l == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = base;
        for (uint32_t k = 0; k < w; k++) off += wsum[k];
        if (f) list[off + pre] = t;
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0;
            for (uint32_t k = 0; k < 16; k++) tot += wsum[k];
            base += tot;
        }
        __syncthreads();
    }
    if (tid == 0) *count = base;
}
/* orx_export_hitpoints: the own rows' gather inputs in the 28-B exchange layout (plane A
 * pos|flags float4, plane N normal float3; GatherIn.raw) — the attenuation stays with the owner */
__global__ __launch_bounds__(256) void k_export_hp(PixelBufs px, uint32_t n, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 B = px.hpB[i];
    reinterpret_cast<float4*>(dst)[i] = px.hpA[i];
    float* N = dst + 4 * hp_export_plane(n) + 3 * (size_t)i;
    N[0] = B.x;
    N[1] = B.y;
    N[2] = B.z;
}
/* orx_ppm_finish of a shard: own-row indirect = the summed unattenuated estimate times the hit
 * point's attenuation (IndirectRadianceEstimation.cu:220 multiplies before the normalisation;
 * the same value up to fp32 order) */
__global__ __launch_bounds__(256) void k_indirect_atten(PixelBufs px, uint32_t n, const float* __restrict__ in) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 B = px.hpB[i];
    const float2 Cc = px.hpC[i];
    px.indirect[3 * (size_t)i + 0] = in[3 * (size_t)i + 0] * B.w;
    px.indirect[3 * (size_t)i + 1] = in[3 * (size_t)i + 1] * Cc.x;
    px.indirect[3 * (size_t)i + 2] = in[3 * (size_t)i + 2] * Cc.y;
}
void launch_export_hp(hipStream_t s, const PixelBufs& px, uint32_t n, float* dst) {
    hipLaunchKernelGGL(k_export_hp, dim3((n + 255) / 256), dim3(256), 0, s, px, n, dst);
}
void launch_indirect_atten(hipStream_t s, const PixelBufs& px, uint32_t n, const float* in) {
    hipLaunchKernelGGL(k_indirect_atten, dim3((n + 255) / 256), dim3(256), 0, s, px, n, in);
}
void launch_gather_tiles(hipStream_t s, const GatherIn& gi, const PhotonBufs& pb, const Consts& c, uint8_t* flags,
                         uint32_t* list, uint32_t* count) {
    const uint32_t rows = gi.segments * gi.seg_rows;
    const uint32_t ntx = (gi.W + 15) / 16, nty = (rows + 15) / 16, ntiles = ntx * nty;
    hipLaunchKernelGGL(k_gather_tiles, dim3(ntiles), dim3(256), 0, s, gi, pb, c, ntx, flags);
    hipLaunchKernelGGL(k_tile_compact, dim3(1), dim3(1024), 0, s, flags, ntiles, list, count);
}

void launch_ppm_gather(hipStream_t s, const GatherIn& gi, const PhotonBufs& pb, const Consts& c) {
    const uint32_t rows = gi.segments * gi.seg_rows;
    const uint32_t ntx = (gi.W + 15) / 16, nty = (rows + 15) / 16, ntiles = ntx * nty;
    const uint32_t norder = gi.tile_list ? ntiles : gather_order_count(gi.order, ntx, nty);
    const dim3 grid(8 * ((norder + 7) / 8));
    /* The sharded gather (segments = ranks, cell-order layout, no visit counters) meets 1/N of
     * the photons.  Where a rank's photons are sparse in the grid the wave union's per-row work
     * outweighs the photons it shares and the per-lane kernel is faster: hall 1080p, 2048^2
     * launch (tools/shard_model.py, per-rank gather union / per-lane: N=2 1.29 / 1.56 ms, N=4
     * 0.73 / 0.80, N=8 0.47 / 0.43, i.e. 4.2 / 2.1 slots per grid cell at N=4 / 8); at the 4K
     * conference's 16M-photon launch the union is far ahead at N=8 too (8.4 slots per cell:
     * 6.41 / 9.34 ms).  So the per-lane kernel takes row shards of 8+ segments below 3 slots per
     * cell.  Measured on one device (serial hall gather / 4K conference frame): per-lane 2.5 ms /
     * 120 ms, union 1.91 / 53.3. */
    static const int kern = [] { /* ORX_GATHER_KERNEL: 0 auto, 1 union, 2 per-lane (A/B) */
        const char* e = getenv("ORX_GATHER_KERNEL");
        return e ? atoi(e) : 0;
    }();
    const bool lane = kern == 2 || (kern == 0 && gi.segments >= 8 && !gi.cull && pb.S < 3u * pb.gcells);
    if (lane) {
        if (pb.nsub == 1) hipLaunchKernelGGL((k_ppm_gather<1>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles);
        else hipLaunchKernelGGL((k_ppm_gather<SUBR * SUBR>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles);
        return;
    }
    /* the weight polynomial in d^2 divided through by c_4 / r^8 (weight2d) where that scale and the
     * coefficients are normal floats; else in u = d^2 / r^2 (weight2u) */
    static const int dform_env = [] {
        const char* e = getenv("ORX_GATHER_DFORM");
        return e ? atoi(e) : 1;
    }();
    WPoly wp{};
    bool df = dform_env != 0;
    {
        const double irr = (double)(1.0f / c.ppm_radius2);
        const double ck[6] = {ORX_W5_C0, ORX_W5_C1, ORX_W5_C2, ORX_W5_C3, ORX_W5_C4, ORX_W5_C5};
        const double c4 = ck[4] * irr * irr * irr * irr;
        /* a lane's sums carry a factor 1 / scale until the end: far inside fp32 for a scale in [1e-20, 1e20] */
        df = df && std::isfinite(c4) && std::fabs(c4) >= 1e-20 && std::fabs(c4) <= 1e20;
        double sc = 1.0;
        for (int k = 0; k < 6; k++, sc *= irr) {
            const double v = ck[k] * sc / c4;
            df = df && std::isfinite(v) && std::fabs(v) < 1e37 && std::fabs(v) > 1e-37;
            wp.k[k] = (float)v;
        }
        wp.k[4] = 1.f;
        wp.scale = (float)c4;
    }
    if (pb.nsub == 1) {
        if (df) hipLaunchKernelGGL((k_ppm_gather_union<1, true>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles, wp);
        else hipLaunchKernelGGL((k_ppm_gather_union<1, false>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles, wp);
    } else {
        if (df) hipLaunchKernelGGL((k_ppm_gather_union<SUBR * SUBR, true>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles, wp);
        else hipLaunchKernelGGL((k_ppm_gather_union<SUBR * SUBR, false>), grid, dim3(256), 0, s, gi, pb, c, ntx, ntiles, wp);
    }
}

}  // namespace orx
