/*
 * orx_grid.hip — the photon grid build of the uniform-grid photon map, gfx950:
 * calculateHashCellsKernel + sort_by_key + exclusive_scan (OptixRenderer_SpatialHash.cu:152-207)
 * as an LDS bucket counting sort (k_bs_*), the reference's cell offsets (k_grid_coarse_offsets)
 * and the sorted photon array as SoA planes (k_grid_permute).  The grid itself (origin, cell
 * size, dimensions) is k_grid_setup's, in orx_raypass.hip; what the gather may assume of the
 * result is in orx_photon_grid.h.
 */
#include <cstdlib>

#include "orx_kernels_common.h"
#include "orx_photon_grid.h"

namespace orx {

/* ------------------------------------------------------------------ */
/* block-wide exclusive scan (the bucket sort's table scan)             */
/* ------------------------------------------------------------------ */
constexpr int SCAN_BLOCK = 1024; /* elements per block: 256 threads x 4 */

__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* total) {
    __shared__ uint32_t ws[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) ws[w] = x;
    __syncthreads();
    uint32_t pre = 0;
    for (int q = 0; q < w; q++) pre += ws[q];
    *total = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    return pre + x - v;
}

/* one grid photon: a deposit record -> the SoA planes at grid
 * position dst (the reference's sorted photon array, SpatialHash.cu:193-196) */
__device__ __forceinline__ void grid_put(const PhotonBufs& pb, uint32_t dst, const float4 a, const float4 b, float cz) {
    const size_t P = pb.splane;
    float* o = pb.sorted + dst;
    o[SP_X * P] = a.x;
    o[SP_Y * P] = a.y;
    o[SP_Z * P] = a.z;
    o[SP_DIRQ * P] = __uint_as_float(dir_q8(b.x, b.y, b.z));
    o[SP_DX * P] = b.x;
    o[SP_DY * P] = b.y;
    o[SP_DZ * P] = b.z;
    o[SP_PX * P] = a.w;
    o[SP_PY * P] = b.w;
    o[SP_PZ * P] = cz;
}
/* grid order -> SoA planes: destination-major, so the ten plane writes are
 * coalesced and the source reads are whole float4s */
__global__ __launch_bounds__(256) void k_grid_permute(PhotonBufs pb) {
    const uint32_t valid = pb.grid->valid;
    const uint32_t T = gridDim.x * blockDim.x;
    for (uint32_t d0 = blockIdx.x * blockDim.x + threadIdx.x; d0 < valid; d0 += 4 * T) {
        uint32_t src[4];
        float4 a[4], b[4];
        float cz[4];
#pragma unroll
        for (int q = 0; q < 4; q++) src[q] = d0 + q * T < valid ? pb.perm[d0 + q * T] : 0xffffffffu;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (src[q] != 0xffffffffu) {
                const float4* rec = pb.slots + 4 * (size_t)src[q];
                a[q] = rec[0];
                b[q] = rec[1];
                cz[q] = rec[2].x;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (src[q] != 0xffffffffu) grid_put(pb, d0 + q * T, a[q], b[q], cz[q]);
    }
}
/* ------------------------------------------------------------------ */
/* photon grid without global atomics: two-level bucket counting sort  */
/* ------------------------------------------------------------------ */
/* An atomic-rank counting sort (the first version) issues one device-scope atomic per
 * photon into a 4 MB histogram; across 8 XCDs those resolve at the memory
 * side (~25 G/s measured), which makes the hash pass the slowest of the grid
 * build.  Here:
 *   A  k_bs_count    per chunk of BS_CHUNK slots: keys, LDS histogram of the
 *                    coarse bucket key >> bshift -> table[bucket][chunk]
 *   S  scan of the table (bucket-major) -> where each chunk's bucket run starts
 *   B  k_bs_place    per chunk: LDS cursors from the table, (key, slot) pairs
 *                    appended to their bucket run
 *   C  k_bs_cells    one block per bucket: LDS histogram of its cells, LDS
 *                    scan -> offsets of those cells, permutation by LDS cursors
 *   D  k_grid_coarse_offsets (nsub > 1) the reference's cell offsets
 * All counting is in LDS.  Offsets equal the reference's exclusive scan over
 * the cell histogram (keys >= G are the reference's overflow cell G and, as
 * there, fall beyond offsets[G] = valid: they are dropped).
 * The order the photons end up in (virtual cells, sub-rows, x quarters) and the
 * sub-cell key are the contract with the gather: orx_photon_grid.h. */
constexpr uint32_t BS_CHUNK = 16384;
constexpr uint32_t BS_THREADS = 512;
constexpr uint32_t BS_MAXB = 2048; /* buckets */

__global__ __launch_bounds__(BS_THREADS) void k_bs_count(PhotonBufs pb) {
    __shared__ uint32_t hist[BS_MAXB];
    const GridParams g = *pb.grid;
    const uint32_t nb = (g.G * pb.nsub + (1u << pb.bshift) - 1) >> pb.bshift;
    for (uint32_t i = threadIdx.x; i < BS_MAXB; i += BS_THREADS) hist[i] = 0;
    __syncthreads();
    const float inv = 1.f / g.cell;
    const uint32_t c0 = blockIdx.x * BS_CHUNK;
    for (uint32_t k = threadIdx.x; k < BS_CHUNK; k += BS_THREADS) {
        const uint32_t s = c0 + k;
        if (s >= pb.S) break;
        uint32_t key = 0xffffffffu;
        const uint32_t p = s / pb.D, d = s - p * pb.D;
        if (g.G && ((pb.vmask[p] >> d) & 1u)) {
            const float4 a = pb.pos4[s];
            const f3 pp = (mk(a.x, a.y, a.z) - mk(g.ox, g.oy, g.oz)) * inv;
            const uint32_t cx = orx_f2u_sat(orx_floorf(pp.x));
            const uint32_t cy = orx_f2u_sat(orx_floorf(pp.y));
            const uint32_t cz = orx_f2u_sat(orx_floorf(pp.z));
            const uint32_t kk = cx + cy * g.gx + cz * g.gx * g.gy;
            if (kk < g.G) { /* calculateHashCellsKernel clamps to G: the overflow cell, beyond valid */
                /* sub-cell key: the x quarter of the cell, so that the gather can
                 * trim a row to the chord at quarter-cell granularity */
                int32_t q = (int32_t)orx_floorf(pp.x * (float)SUBX) - (int32_t)SUBX * (int32_t)cx;
                q = q < 0 ? 0 : (q > (int32_t)SUBX - 1 ? (int32_t)SUBX - 1 : q);
                uint32_t vc = kk;
                if (pb.nsub > 1) { /* sub-row: y and z halves (x2 is exact, so the halves nest in the cells) */
                    int32_t hy = (int32_t)orx_floorf(pp.y * (float)SUBR) - (int32_t)SUBR * (int32_t)cy;
                    int32_t hz = (int32_t)orx_floorf(pp.z * (float)SUBR) - (int32_t)SUBR * (int32_t)cz;
                    hy = hy < 0 ? 0 : (hy > (int32_t)SUBR - 1 ? (int32_t)SUBR - 1 : hy);
                    hz = hz < 0 ? 0 : (hz > (int32_t)SUBR - 1 ? (int32_t)SUBR - 1 : hz);
                    const uint32_t row = cy + cz * g.gy;
                    vc = (row * pb.nsub + (uint32_t)hz * SUBR + (uint32_t)hy) * g.gx + cx;
                }
                key = vc * SUBX + (uint32_t)q;
                atomicAdd(&hist[vc >> pb.bshift], 1u);
            }
        }
        pb.keys[s] = key;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += BS_THREADS) pb.bs_table[(size_t)b * pb.bs_nchunk + blockIdx.x] = hist[b];
}

/* exclusive scan of n = nb * nchunk table entries in place (three kernels) */
__global__ __launch_bounds__(256) void k_bs_scan_reduce(PhotonBufs pb) {
    const uint32_t nb = (pb.grid->G * pb.nsub + (1u << pb.bshift) - 1) >> pb.bshift;
    const uint32_t n = nb * pb.bs_nchunk;
    const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * 4;
    uint32_t sum = 0;
    for (int k = 0; k < 4; k++)
        if (base + k < n) sum += pb.bs_table[base + k];
    uint32_t total;
    (void)block_exclusive_scan_256(sum, &total);
    if (threadIdx.x == 0) pb.bs_partials[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_bs_scan_partials(PhotonBufs pb, uint32_t nblocks) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? pb.bs_partials[i] : 0;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan_256(v, &total);
        if (i < nblocks) pb.bs_partials[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) pb.bs_partials[nblocks] = carry; /* grand total = valid photons */
}
__global__ __launch_bounds__(256) void k_bs_scan_apply(PhotonBufs pb) {
    const uint32_t nb = (pb.grid->G * pb.nsub + (1u << pb.bshift) - 1) >> pb.bshift;
    const uint32_t n = nb * pb.bs_nchunk;
    if (blockIdx.x * SCAN_BLOCK >= n) return;
    const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * 4;
    uint32_t v[4], sum = 0;
    for (int k = 0; k < 4; k++) {
        v[k] = base + k < n ? pb.bs_table[base + k] : 0;
        sum += v[k];
    }
    uint32_t total;
    uint32_t ex = block_exclusive_scan_256(sum, &total) + pb.bs_partials[blockIdx.x];
    for (int k = 0; k < 4; k++) {
        if (base + k < n) pb.bs_table[base + k] = ex;
        ex += v[k];
    }
}

__global__ __launch_bounds__(BS_THREADS) void k_bs_place(PhotonBufs pb) {
    __shared__ uint32_t cur[BS_MAXB];
    const uint32_t G = pb.grid->G * pb.nsub;
    const uint32_t nb = (G + (1u << pb.bshift) - 1) >> pb.bshift;
    for (uint32_t b = threadIdx.x; b < nb; b += BS_THREADS) cur[b] = pb.bs_table[(size_t)b * pb.bs_nchunk + blockIdx.x];
    __syncthreads();
    const uint32_t c0 = blockIdx.x * BS_CHUNK;
    constexpr uint32_t U = 4;
    for (uint32_t k0 = threadIdx.x; k0 < BS_CHUNK; k0 += U * BS_THREADS) {
        uint32_t kv[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t s = c0 + k0 + u * BS_THREADS;
            kv[u] = s < pb.S ? pb.keys[s] : 0xffffffffu;
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            if (kv[u] != 0xffffffffu) {
                const uint32_t pos = atomicAdd(&cur[(kv[u] / SUBX) >> pb.bshift], 1u);
                pb.bs_pairs[pos] = make_uint2(kv[u], c0 + k0 + u * BS_THREADS);
            }
        }
    }
}

/* one block per bucket: histogram of its sub-cells (virtual cell x quarter),
 * LDS scan -> sub-cell offsets (the gather's chord trimming) and, for nsub = 1,
 * the cell offsets (the reference's), permutation by LDS cursors */
__global__ __launch_bounds__(1024) void k_bs_cells(PhotonBufs pb, uint32_t cb, uint32_t nscan) {
    extern __shared__ uint32_t lds[]; /* [SUBX * cb] histogram / cursors */
    const uint32_t G = pb.grid->G * pb.nsub; /* virtual cells */
    const uint32_t nb = (G + cb - 1) / cb;
    const uint32_t b = blockIdx.x;
    const uint32_t total = pb.bs_partials[nscan]; /* grand total written by k_bs_scan_partials */
    if (b > nb) return;
    /* bucket nb (one past the last) only writes offsets[G] = valid when G is a multiple of cb */
    const uint32_t start = b < nb ? pb.bs_table[(size_t)b * pb.bs_nchunk] : total;
    const uint32_t end = b + 1 < nb ? pb.bs_table[(size_t)(b + 1) * pb.bs_nchunk] : total;
    const uint32_t nf = SUBX * cb, f0 = b * nf;
    for (uint32_t i = threadIdx.x; i < nf; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    for (uint32_t i0 = start + threadIdx.x; i0 < end; i0 += 4 * blockDim.x) {
        uint32_t kv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * blockDim.x;
            kv[u] = i < end ? pb.bs_pairs[i].x : 0xffffffffu;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++)
            if (kv[u] != 0xffffffffu) atomicAdd(&lds[kv[u] - f0], 1u);
    }
    __syncthreads();
    /* exclusive scan of lds[0..nf) by 1024 threads, nf/1024 entries each */
    __shared__ uint32_t wsum[16];
    const uint32_t per = nf / blockDim.x;
    const uint32_t t0 = threadIdx.x * per;
    uint32_t run = 0;
    for (uint32_t k = 0; k < per; k++) run += lds[t0 + k];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = run;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0;
    for (uint32_t q = 0; q < w; q++) pre += wsum[q];
    uint32_t ex = start + pre + x - run;
    for (uint32_t k = 0; k < per; k++) {
        const uint32_t f = f0 + t0 + k, c = f / SUBX;
        const uint32_t v = lds[t0 + k];
        if (c <= G) {
            if (f % SUBX == 0 && pb.nsub == 1) pb.offsets[c] = ex;
            if (c < G || f % SUBX == 0) pb.subofs[f] = ex;
        }
        lds[t0 + k] = ex; /* becomes the sub-cell's cursor */
        ex += v;
    }
    if (threadIdx.x == 0 && b == 0) {
        pb.grid->valid = total;
        pb.grid->valid_total += total;
    }
    __syncthreads();
    for (uint32_t i0 = start + threadIdx.x; i0 < end; i0 += 4 * blockDim.x) {
        uint2 kv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t i = i0 + u * blockDim.x;
            kv[u] = i < end ? pb.bs_pairs[i] : make_uint2(0xffffffffu, 0u);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++)
            if (kv[u].x != 0xffffffffu) {
                const uint32_t pos = atomicAdd(&lds[kv[u].x - f0], 1u);
                pb.perm[pos] = kv[u].y;
            }
    }
}

/* the reference's cell offsets from the sub-row offsets: cell (x, row) starts
 * after all photons of the earlier rows and, in each of the row's nsub
 * sub-rows, after the photons of cells x' < x */
__global__ __launch_bounds__(256) void k_grid_coarse_offsets(PhotonBufs pb) {
    const GridParams g = *pb.grid;
    const uint32_t rowlen = g.gx * SUBX;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c <= g.G; c += gridDim.x * blockDim.x) {
        const uint32_t row = c / g.gx, x = c - row * g.gx;
        const size_t r0 = (size_t)row * pb.nsub * rowlen;
        uint32_t o = pb.subofs[r0];
        if (c < g.G)
            for (uint32_t s = 0; s < pb.nsub; s++) {
                const size_t b = r0 + (size_t)s * rowlen;
                o += pb.subofs[b + x * SUBX] - pb.subofs[b];
            }
        pb.offsets[c] = o;
    }
}

static uint32_t bs_nscan(const PhotonBufs& pb) {
    const uint32_t nbmax = (pb.gmax * pb.nsub + (1u << pb.bshift) - 1) >> pb.bshift;
    return (nbmax * pb.bs_nchunk + SCAN_BLOCK - 1) / SCAN_BLOCK;
}
void launch_grid_bucket_count(hipStream_t s, const PhotonBufs& pb) {
    hipLaunchKernelGGL(k_bs_count, dim3(pb.bs_nchunk), dim3(BS_THREADS), 0, s, pb);
}
void launch_grid_bucket_scan(hipStream_t s, const PhotonBufs& pb) {
    const uint32_t nscan = bs_nscan(pb);
    hipLaunchKernelGGL(k_bs_scan_reduce, dim3(nscan), dim3(256), 0, s, pb);
    hipLaunchKernelGGL(k_bs_scan_partials, dim3(1), dim3(256), 0, s, pb, nscan);
    hipLaunchKernelGGL(k_bs_scan_apply, dim3(nscan), dim3(256), 0, s, pb);
}
void launch_grid_bucket_place(hipStream_t s, const PhotonBufs& pb) {
    /* (staging a half chunk's pairs in LDS bucket by bucket, so that the writes of a wave go out in
     * runs, measured slower on the pipelined hall frame: 1034-1035 -> 1026-1028 Mpaths/s) */
    hipLaunchKernelGGL(k_bs_place, dim3(pb.bs_nchunk), dim3(BS_THREADS), 0, s, pb);
    const uint32_t cb = 1u << pb.bshift;
    const uint32_t nbmax = (pb.gmax * pb.nsub + cb - 1) / cb;
    static const uint32_t cells_threads = [] {
        const char* e = getenv("ORX_BS_CELLS_THREADS");
        const int v = e ? atoi(e) : 512; /* 512: co-schedules better beside the pipelined gather */
        return (uint32_t)(v == 256 || v == 1024 ? v : 512);
    }();
    hipLaunchKernelGGL(k_bs_cells, dim3(nbmax + 1), dim3(cells_threads), SUBX * cb * 4, s, pb, cb, bs_nscan(pb));
    if (pb.nsub > 1) {
        unsigned cblocks = (pb.gmax + 1 + 255) / 256;
        if (cblocks > 4096) cblocks = 4096;
        hipLaunchKernelGGL(k_grid_coarse_offsets, dim3(cblocks), dim3(256), 0, s, pb);
    }
    /* applying the permutation inside k_bs_cells (one block per bucket, scattered
     * record reads at its occupancy) measured 3.5 ms against 0.5 ms for this pass */
    /* (the record reads shared by a quad of lanes through LDS, 16 record lines per load instead
     * of 64, measured slower: hall grid build 1.20 -> 1.41 ms) */
    unsigned blocks = (pb.S + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_grid_permute, dim3(blocks), dim3(256), 0, s, pb);
}

}  // namespace orx
