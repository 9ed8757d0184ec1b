/*
 * orx_slab.hip — slab mode of the sharded PPM gather, gfx950: the histograms the host plans the
 * slabs from (k_slab_hist, k_slab_bbox), the photons packed per destination rank (k_slab_pack) and
 * the received ones turned into this rank's deposits (k_slab_import).  The gather's side of the
 * mode (ownership cull, tile list) is in orx_kernels.hip.
 */
#include <algorithm>

#include "orx_kernels_common.h"

namespace orx {

/* ------------------------------------------------------------------ */
/* spatial photon partition of the sharded gather (slab mode)          */
/* ------------------------------------------------------------------ */
/* Rank g of N receives every photon whose position falls in its slab of one axis of the scene
 * AABB, and gathers only the hit points whose sphere reaches its photons; the bins and the
 * bin -> rank table are the host's plan (multigpu.slab_plan) over the all-gathered histograms.
 * The bin of a position is computed by one function (slab_bin, orx_kernels.h) in the histogram,
 * in the pack and in the gather's ownership test, so the host's per-rank counts are exact. */
__device__ __forceinline__ bool slot_valid(const PhotonBufs& pb, uint32_t s) {
    const uint32_t p = s / pb.D, k = s - p * pb.D;
    return (pb.vmask[p] >> k) & 1u;
}
/* [2][3][nb] counts: the valid deposits of the own photon pass and the own rows' non-specular
 * hit points per bin of each axis; then [2][SLAB_VOX^3] counts of both over a coarse voxel grid
 * of the scene AABB (voxel x + V (y + V z)), which the plan uses to weigh each hit point by the
 * photon density around it.  LDS histograms, one global add per non-empty bin and block; the
 * voxel counters are 16-bit halves of one word (photons low, hit points high), so a block takes
 * a contiguous chunk of at most 65535 slots and 65535 pixels. */
constexpr uint32_t SLAB_MAX_BINS = 1024;
/* 24 KB of axis bins + 128 KB of voxel counts: one block per CU on gfx950's 160 KB LDS
 * (the Makefile's ARCH is gfx950 only; a smaller-LDS target fails here, not at launch) */
static_assert((6 * SLAB_MAX_BINS + SLAB_VOX * SLAB_VOX * SLAB_VOX) * 4 <= 160 * 1024,
              "k_slab_hist's LDS histograms exceed gfx950's 160 KB per workgroup");
__global__ __launch_bounds__(256) void k_slab_hist(PhotonBufs pb, PixelBufs px, SlabBins sb, SlabBins vb,
                                                   uint32_t cs, uint32_t cp, uint32_t* hist) {
    __shared__ uint32_t lh[6 * SLAB_MAX_BINS];
    __shared__ uint32_t lv[SLAB_VOX * SLAB_VOX * SLAB_VOX];
    const uint32_t n6 = 6 * sb.nb, NV = SLAB_VOX * SLAB_VOX * SLAB_VOX;
    for (uint32_t k = threadIdx.x; k < n6; k += blockDim.x) lh[k] = 0;
    for (uint32_t k = threadIdx.x; k < NV; k += blockDim.x) lv[k] = 0;
    __syncthreads();
    const uint32_t s0 = blockIdx.x * cs, s1 = s0 + cs < pb.S ? s0 + cs : pb.S;
    for (uint32_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
        if (!slot_valid(pb, s)) continue;
        const float4 q = pb.pos4[s];
        atomicAdd(&lh[0 * sb.nb + slab_bin(sb, q.x, 0)], 1u);
        atomicAdd(&lh[1 * sb.nb + slab_bin(sb, q.y, 1)], 1u);
        atomicAdd(&lh[2 * sb.nb + slab_bin(sb, q.z, 2)], 1u);
        atomicAdd(&lv[slab_bin(vb, q.x, 0) + SLAB_VOX * (slab_bin(vb, q.y, 1) + SLAB_VOX * slab_bin(vb, q.z, 2))], 1u);
    }
    const uint32_t npx = px.rows * px.W;
    const uint32_t p0 = blockIdx.x * cp, p1 = p0 + cp < npx ? p0 + cp : npx;
    for (uint32_t i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
        const float4 A = px.hpA[i];
        if (!(__float_as_uint(A.w) & PRD_HIT_NON_SPECULAR)) continue;
        atomicAdd(&lh[3 * sb.nb + slab_bin(sb, A.x, 0)], 1u);
        atomicAdd(&lh[4 * sb.nb + slab_bin(sb, A.y, 1)], 1u);
        atomicAdd(&lh[5 * sb.nb + slab_bin(sb, A.z, 2)], 1u);
        atomicAdd(&lv[slab_bin(vb, A.x, 0) + SLAB_VOX * (slab_bin(vb, A.y, 1) + SLAB_VOX * slab_bin(vb, A.z, 2))],
                  1u << 16);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n6; k += blockDim.x)
        if (lh[k]) atomicAdd(&hist[k], lh[k]);
    uint32_t* hv = hist + n6 + 6; /* past the photon AABB words (k_slab_bbox) */
    for (uint32_t k = threadIdx.x; k < NV; k += blockDim.x) {
        const uint32_t v = lv[k];
        if (v & 0xffffu) atomicAdd(&hv[k], v & 0xffffu);
        if (v >> 16) atomicAdd(&hv[NV + k], v >> 16);
    }
}
void launch_slab_hist(hipStream_t s, const PhotonBufs& pb, const PixelBufs& px, const SlabBins& sb,
                      const SlabBins& vb, uint32_t* hist) {
    const uint32_t npx = px.rows * px.W;
    uint32_t blocks = std::max((pb.S + 65534) / 65535, (npx + 65534) / 65535);
    blocks = std::max(blocks, 64u);
    const uint32_t cs = (pb.S + blocks - 1) / blocks, cp = (npx + blocks - 1) / blocks;
    hipLaunchKernelGGL(k_slab_hist, dim3(blocks), dim3(256), 0, s, pb, px, sb, vb, cs, cp, hist);
}

/* valid deposits -> the send buffer, rank-major: photon record (9 floats: position, direction,
 * power) at cursor[rank]++.  A block takes SLAB_CHUNK slots: counts per destination in LDS,
 * one device atomic per destination reserves the block's run, then every photon takes its
 * place in it (the order inside a run is not the slot order: it only changes the gather's
 * fp32 summation order on the receiving rank) */
constexpr uint32_t SLAB_CHUNK = 4096;
constexpr uint32_t SLAB_MAX_RANKS = 64;
__global__ __launch_bounds__(256) void k_slab_pack(PhotonBufs pb, SlabBins sb, uint32_t axis, uint32_t halo,
                                                   const uint8_t* __restrict__ bin_dest, uint32_t world,
                                                   uint32_t* cursor, uint32_t cap, float* __restrict__ send) {
    __shared__ uint32_t cnt[SLAB_MAX_RANKS], base[SLAB_MAX_RANKS];
    for (uint32_t c0 = blockIdx.x * SLAB_CHUNK; c0 < pb.S; c0 += gridDim.x * SLAB_CHUNK) {
        const uint32_t c1 = c0 + SLAB_CHUNK < pb.S ? c0 + SLAB_CHUNK : pb.S;
        if (threadIdx.x < SLAB_MAX_RANKS) cnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t s = c0 + threadIdx.x; s < c1; s += blockDim.x) {
            if (!slot_valid(pb, s)) continue;
            const float4 q = pb.pos4[s];
            const float v = axis == 0 ? q.x : axis == 1 ? q.y : q.z;
            const uint32_t b = slab_bin(sb, v, axis);
            const uint32_t d0 = bin_dest[b > halo ? b - halo : 0u];
            const uint32_t d1 = bin_dest[b + halo < sb.nb ? b + halo : sb.nb - 1u];
            for (uint32_t d = d0; d <= d1; d++) atomicAdd(&cnt[d], 1u);
        }
        __syncthreads();
        if (threadIdx.x < world) {
            const uint32_t n = cnt[threadIdx.x];
            base[threadIdx.x] = n ? atomicAdd(&cursor[threadIdx.x], n) : 0u;
            cnt[threadIdx.x] = 0;
        }
        __syncthreads();
        for (uint32_t s = c0 + threadIdx.x; s < c1; s += blockDim.x) {
            if (!slot_valid(pb, s)) continue;
            const float4* rec = pb.slots + 4 * (size_t)s;
            const float4 a = rec[0], b = rec[1];
            const float pz = rec[2].x;
            const float v = axis == 0 ? a.x : axis == 1 ? a.y : a.z;
            const uint32_t bn = slab_bin(sb, v, axis);
            const uint32_t d0 = bin_dest[bn > halo ? bn - halo : 0u];
            const uint32_t d1 = bin_dest[bn + halo < sb.nb ? bn + halo : sb.nb - 1u];
            for (uint32_t d = d0; d <= d1; d++) { /* the owner and the ranks within the halo */
                const uint32_t o = base[d] + atomicAdd(&cnt[d], 1u);
                if (o >= cap) continue; /* a plan whose counts disagree with the photons: never write past */
                float* w = send + 9 * (size_t)o;
                w[0] = a.x; w[1] = a.y; w[2] = a.z;
                w[3] = b.x; w[4] = b.y; w[5] = b.z;
                w[6] = a.w; w[7] = b.w; w[8] = pz;
            }
        }
        __syncthreads();
    }
}
void launch_slab_pack(hipStream_t s, const PhotonBufs& pb, const SlabBins& sb, uint32_t axis, uint32_t halo,
                      const uint8_t* bin_dest, uint32_t world, uint32_t* cursor, uint32_t cap, float* send) {
    uint32_t blocks = (pb.S + SLAB_CHUNK - 1) / SLAB_CHUNK;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(k_slab_pack, dim3(blocks), dim3(256), 0, s, pb, sb, axis, halo, bin_dest, world, cursor, cap,
                       send);
}

/* received photon records -> this rank's deposit records: record i is slot i of photon group
 * i / D (deposit mask bit i % D), with its compact position and the photon AABB of the grid
 * setup (the replicas k_grid_setup folds; reset beforehand) */
__global__ __launch_bounds__(256) void k_slab_import(PhotonBufs pb, const float* __restrict__ recv, uint32_t n) {
    float lo_x = INFINITY, lo_y = INFINITY, lo_z = INFINITY;
    float hi_x = -INFINITY, hi_y = -INFINITY, hi_z = -INFINITY;
    const uint32_t groups = (n + pb.D - 1) / pb.D;
    const uint32_t T = gridDim.x * blockDim.x;
    const uint32_t g_end = ((groups + T - 1) / T) * T; /* every lane runs the same trip count */
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < g_end; g += T) {
        if (g >= groups) continue;
        uint32_t mask = 0;
        for (uint32_t k = 0; k < pb.D; k++) {
            const uint32_t i = g * pb.D + k;
            if (i >= n) break;
            const float* w = recv + 9 * (size_t)i;
            const float x = w[0], y = w[1], z = w[2];
            float4* rec = pb.slots + 4 * (size_t)i;
            rec[0] = make_float4(x, y, z, w[6]);
            rec[1] = make_float4(w[3], w[4], w[5], w[7]);
            rec[2].x = w[8];
            pb.pos4[i] = make_float4(x, y, z, 0.f);
            mask |= 1u << k;
            lo_x = fminf(lo_x, x); lo_y = fminf(lo_y, y); lo_z = fminf(lo_z, z);
            hi_x = fmaxf(hi_x, x); hi_y = fmaxf(hi_y, y); hi_z = fmaxf(hi_z, z);
        }
        pb.vmask[g] = (uint8_t)mask;
    }
    photon_bbox_flush(pb, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, (blockIdx.x * 4 + (threadIdx.x >> 6)) & (BBOX_REPLICAS - 1),
                      threadIdx.x & 63);
}
__global__ void k_slab_bbox(PhotonBufs pb, uint32_t* out) {
    const uint32_t lane = threadIdx.x;
    for (int k = 0; k < 6; k++) {
        uint32_t v = pb.bbox[k * BBOX_REPLICAS + lane];
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
            v = k < 3 ? min(v, w) : max(v, w);
        }
        if (lane == 0) out[k] = v;
    }
}
void launch_slab_bbox(hipStream_t s, const PhotonBufs& pb, uint32_t* out) {
    hipLaunchKernelGGL(k_slab_bbox, dim3(1), dim3(64), 0, s, pb, out);
}
void launch_slab_import(hipStream_t s, const PhotonBufs& pb, const float* recv, uint32_t n) {
    const uint32_t groups = (n + pb.D - 1) / pb.D;
    uint32_t blocks = (groups + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(k_slab_import, dim3(blocks), dim3(256), 0, s, pb, recv, n);
}

}  // namespace orx
