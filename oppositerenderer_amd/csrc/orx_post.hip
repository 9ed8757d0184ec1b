/*
 * orx_post.hip — passes over the running sum behind an iteration: the per-pixel convergence statistics
 * (orx_set_convergence), the estimate's error planes and tile reduction (orx_get_convergence) and the 8-bit
 * display resolve (orx_get_display).  No render kernel knows of them: the statistics take an iteration's
 * radiance as the difference of the running sum before and after it (include/orx.h gives the operation
 * order, which tests/convergence_ref.py restates).
 *
 * The update is bandwidth-bound elementwise work, 52 B per pixel (S and prev read, prev written, A and M2
 * read and written): a lane takes 4 consecutive pixels, so S and prev move as three 16-byte accesses each and
 * A and M2 as one each; the tail of fewer than 4 pixels is scalar; a grid-stride loop over at most 2048
 * blocks of 256; no LDS, no atomics.
 */
#include "orx_display.h"
#include "orx_host.h"

using namespace orx;

namespace {

constexpr uint32_t POST_MAX_BLOCKS = 2048;

inline uint32_t post_grid(size_t items) {
    const size_t want = (items + 255) / 256;
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(want, POST_MAX_BLOCKS));
}

/* one pixel of the update, in the order include/orx.h states */
__device__ __forceinline__ void conv_pixel(float sr, float sg, float sb, float pr, float pg, float pb, float& A, float& M2,
                                           uint32_t n) {
    const float dr = sr - pr, dg = sg - pg, db = sb - pb;
    const float y = (0.2126f * dr + 0.7152f * dg) + 0.0722f * db;
    if (n == 1u) {
        A = y;
        M2 = 0.0f;
    } else {
        const float mo = A / (float)(n - 1u);
        A = A + y;
        const float mn = A / (float)n;
        M2 = M2 + (y - mo) * (y - mn);
    }
}

__global__ void __launch_bounds__(256) k_conv_update(const float* __restrict__ S, float* __restrict__ prev,
                                                     float* __restrict__ A, float* __restrict__ M2, size_t npx, uint32_t n,
                                                     uint32_t zero) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t ng = npx / 4;
    const float4* __restrict__ S4 = reinterpret_cast<const float4*>(S);
    float4* __restrict__ P4 = reinterpret_cast<float4*>(prev);
    float4* __restrict__ A4 = reinterpret_cast<float4*>(A);
    float4* __restrict__ M4 = reinterpret_cast<float4*>(M2);
    for (size_t g = tid; g < ng; g += nt) {
        const float4 s0 = S4[3 * g], s1 = S4[3 * g + 1], s2 = S4[3 * g + 2];
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0, a = p0, m = p0;
        if (!zero) {
            p0 = P4[3 * g];
            p1 = P4[3 * g + 1];
            p2 = P4[3 * g + 2];
        }
        if (n != 1u) {
            a = A4[g];
            m = M4[g];
        }
        conv_pixel(s0.x, s0.y, s0.z, p0.x, p0.y, p0.z, a.x, m.x, n);
        conv_pixel(s0.w, s1.x, s1.y, p0.w, p1.x, p1.y, a.y, m.y, n);
        conv_pixel(s1.z, s1.w, s2.x, p1.z, p1.w, p2.x, a.z, m.z, n);
        conv_pixel(s2.y, s2.z, s2.w, p2.y, p2.z, p2.w, a.w, m.w, n);
        A4[g] = a;
        M4[g] = m;
        P4[3 * g] = s0;
        P4[3 * g + 1] = s1;
        P4[3 * g + 2] = s2;
    }
    for (size_t i = ng * 4 + tid; i < npx; i += nt) { /* the ragged tail, at most 3 pixels */
        const float sr = S[3 * i], sg = S[3 * i + 1], sb = S[3 * i + 2];
        const float pr = zero ? 0.f : prev[3 * i], pg = zero ? 0.f : prev[3 * i + 1], pb = zero ? 0.f : prev[3 * i + 2];
        float a = 0.f, m = 0.f;
        if (n != 1u) {
            a = A[i];
            m = M2[i];
        }
        conv_pixel(sr, sg, sb, pr, pg, pb, a, m, n);
        A[i] = a;
        M2[i] = m;
        prev[3 * i] = sr;
        prev[3 * i + 1] = sg;
        prev[3 * i + 2] = sb;
    }
}

/* e = sqrtf(M2 / (n (n - 1))) / fmaxf(A / n, floor) and m = A / n per pixel (n >= 2) */
__global__ void __launch_bounds__(256) k_conv_error(const float* __restrict__ A, const float* __restrict__ M2,
                                                    float* __restrict__ e, float* __restrict__ m, size_t npx, uint32_t n,
                                                    float floor) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const float fn = (float)n, d = fn * (float)(n - 1u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += nt) {
        const float se = sqrtf(M2[i] / d);
        const float mean = A[i] / fn;
        e[i] = se / fmaxf(mean, floor);
        m[i] = mean;
    }
}

/* One block per 16x16 tile of a full-frame [H][W] plane pair: sums of e and m, the count above the
 * threshold and the pixels the tile has; a wave reduction over 64 lanes, then the 4 waves' partials
 * through LDS. */
__global__ void __launch_bounds__(256) k_conv_tiles(const float* __restrict__ e, const float* __restrict__ m, uint32_t W,
                                                    uint32_t H, float threshold, ConvTile* __restrict__ tiles) {
    __shared__ float s_e[4], s_m[4];
    __shared__ uint32_t s_a[4], s_c[4];
    const uint32_t t = threadIdx.x;
    const uint32_t x = blockIdx.x * CONV_TILE + (t & 15u), y = blockIdx.y * CONV_TILE + (t >> 4);
    float ve = 0.f, vm = 0.f;
    uint32_t va = 0u, vc = 0u;
    if (x < W && y < H) {
        const size_t i = (size_t)y * W + x;
        ve = e[i];
        vm = m[i];
        va = ve > threshold ? 1u : 0u;
        vc = 1u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ve += __shfl_down(ve, off, 64);
        vm += __shfl_down(vm, off, 64);
        va += __shfl_down(va, off, 64);
        vc += __shfl_down(vc, off, 64);
    }
    if ((t & 63u) == 0u) {
        s_e[t >> 6] = ve;
        s_m[t >> 6] = vm;
        s_a[t >> 6] = va;
        s_c[t >> 6] = vc;
    }
    __syncthreads();
    if (t == 0u) {
        ConvTile q;
        q.sum_e = (s_e[0] + s_e[1]) + (s_e[2] + s_e[3]);
        q.sum_m = (s_m[0] + s_m[1]) + (s_m[2] + s_m[3]);
        q.above = s_a[0] + s_a[1] + s_a[2] + s_a[3];
        q.count = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        tiles[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = q;
    }
}

/* one pixel per lane, one dword store per pixel */
__global__ void __launch_bounds__(256) k_display(const float* __restrict__ sum, size_t npx, float inv_iterations,
                                                 float inv_gamma, int bgra, uint32_t* __restrict__ dst) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += nt)
        dst[i] = orx_display_pixel(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2], inv_iterations, inv_gamma, bgra);
}

/* the planes inside conv.stat, each padded to whole 4-pixel groups: prev [npx][3], A [npx], M2 [npx] */
inline size_t conv_pad(size_t npx) { return (npx + 3) & ~(size_t)3; }
inline float* conv_prev(orx_renderer* r) { return r->conv.stat.as<float>(); }
inline float* conv_A(orx_renderer* r) { return r->conv.stat.as<float>() + 3 * conv_pad(r->conv.npx); }
inline float* conv_M2(orx_renderer* r) { return r->conv.stat.as<float>() + 4 * conv_pad(r->conv.npx); }

/* planes for the renderer's current rows, zeroed (on its own stream, as resize clears the sum) */
orx_status conv_planes(orx_renderer* r) {
    const size_t npx = (size_t)r->rows * r->W;
    HIPCHK(r, r->conv.stat.ensure(conv_pad(npx) * 20));
    r->conv.npx = npx;
    r->conv.err_n = 0;
    HIPCHK(r, hipMemsetAsync(r->conv.stat.p, 0, conv_pad(npx) * 20, r->stream));
    return ORX_OK;
}

}  // namespace

void orx::launch_conv_tiles(hipStream_t st, const float* e, const float* m, uint32_t W, uint32_t H, float threshold,
                            ConvTile* tiles) {
    const dim3 grid((W + CONV_TILE - 1) / CONV_TILE, (H + CONV_TILE - 1) / CONV_TILE);
    hipLaunchKernelGGL(k_conv_tiles, grid, dim3(256), 0, st, e, m, W, H, threshold, tiles);
}
void orx::launch_display(hipStream_t st, const float* sum, size_t npx, float inv_iterations, float inv_gamma, int bgra,
                         uint32_t* dst) {
    if (!npx) return;
    hipLaunchKernelGGL(k_display, dim3(post_grid(npx)), dim3(256), 0, st, sum, npx, inv_iterations, inv_gamma, bgra, dst);
}

orx_status orx::conv_resized(orx_renderer* r) {
    if (!r->conv.on) return ORX_OK;
    const orx_status s = conv_planes(r);
    if (s != ORX_OK) return s;
    r->conv.count = 0;
    r->conv.zero = true;
    return ORX_OK;
}

orx_status orx::conv_rebase(orx_renderer* r) {
    if (!r->conv.on || !r->rng_ready) return ORX_OK; /* no frame yet: the first resize sizes the planes */
    const orx_status s = conv_planes(r);
    if (s != ORX_OK) return s;
    HIPCHK(r, hipMemcpyAsync(conv_prev(r), r->d_out.p, r->conv.npx * 12, hipMemcpyDeviceToDevice, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    r->conv.count = 0;
    r->conv.zero = false;
    return ORX_OK;
}

void orx::conv_begin(orx_renderer* r, uint64_t local_iteration_number) {
    if (!r->conv.on) return;
    if (local_iteration_number == 0) { /* begin_iteration clears the sum */
        r->conv.count = 0;
        r->conv.zero = true;
    }
    r->conv.last = r->conv.it;
    r->conv.it.n = ++r->conv.count;
    r->conv.it.zero = r->conv.zero ? 1u : 0u;
    r->conv.zero = false;
}

void orx::conv_update(orx_renderer* r, hipStream_t st, const ConvIt& it) {
    if (!r->conv.on || !r->conv.npx || !it.n) return;
    ev_begin(r, P_CONVERGENCE, st);
    hipLaunchKernelGGL(k_conv_update, dim3(post_grid((r->conv.npx + 3) / 4)), dim3(256), 0, st,
                       (const float*)r->d_out.as<float>(), conv_prev(r), conv_A(r), conv_M2(r), r->conv.npx, it.n, it.zero);
    ev_end(r, P_CONVERGENCE, st);
}

orx_status orx::conv_error_planes(orx_renderer* r, float floor, float* e, float* m, uint32_t* n_out) {
    if (!r->conv.on) return set_err(r, ORX_ERR_STATE, "convergence statistics are off (orx_set_convergence)");
    if (r->conv.count < 2) return set_err(r, ORX_ERR_STATE, "the statistics window holds fewer than 2 iterations");
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t st = cur_stream(r);
    if (r->pipe.gather_in_flight) HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_gdone[r->pipe.pp], 0)); /* as orx_get_output_device */
    if (r->conv.npx)
        hipLaunchKernelGGL(k_conv_error, dim3(post_grid(r->conv.npx)), dim3(256), 0, st, (const float*)conv_A(r),
                           (const float*)conv_M2(r), e, m, r->conv.npx, r->conv.count, floor);
    HIPCHK(r, hipGetLastError());
    if (n_out) *n_out = r->conv.count;
    return ORX_OK;
}

extern "C" {

orx_status orx_set_convergence(orx_renderer* r, int enable) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    HIPCHK(r, hipSetDevice(r->device));
    const orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    r->conv.on = enable != 0;
    r->conv.count = 0;
    r->conv.zero = false;
    r->conv.it = r->conv.last = r->fin.conv = ConvIt{};
    if (!r->conv.on) { /* off holds nothing */
        r->conv.stat.release();
        r->conv.err.release();
        r->conv.tiles.release();
        r->conv.npx = 0;
        r->conv.err_n = 0;
        return ORX_OK;
    }
    return conv_rebase(r);
}

orx_status orx_get_convergence(orx_renderer* r, float floor, float threshold, orx_convergence* out, float* tile_error,
                               size_t tile_bytes) {
    if (!r || !out) return ORX_ERR_INVALID_ARGUMENT;
    if (!positive_finite(floor)) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "floor must be finite and > 0");
    if (threshold != threshold) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "threshold is NaN");
    if (!r->conv.on) return set_err(r, ORX_ERR_STATE, "convergence statistics are off (orx_set_convergence)");
    if (r->world > 1) return set_err(r, ORX_ERR_STATE, "a sharded renderer holds part of a frame: ask its render group");
    if (r->conv.count < 2 || !r->conv.npx)
        return set_err(r, ORX_ERR_STATE, "the statistics window holds fewer than 2 iterations");
    const uint32_t tx = (r->W + CONV_TILE - 1) / CONV_TILE, ty = (r->H + CONV_TILE - 1) / CONV_TILE;
    const size_t nt = (size_t)tx * ty;
    if (tile_error && tile_bytes < nt * 4) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "tile_error too small");
    HIPCHK(r, hipSetDevice(r->device));
    const orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    const size_t npx = r->conv.npx;
    HIPCHK(r, r->conv.err.ensure(npx * 8));
    HIPCHK(r, r->conv.tiles.ensure(nt * sizeof(ConvTile)));
    float* e = r->conv.err.as<float>();
    float* m = e + npx;
    uint32_t n = 0;
    const orx_status s1 = conv_error_planes(r, floor, e, m, &n);
    if (s1 != ORX_OK) return s1;
    hipStream_t st = cur_stream(r);
    launch_conv_tiles(st, e, m, r->W, r->H, threshold, r->conv.tiles.as<ConvTile>());
    HIPCHK(r, hipGetLastError());
    std::vector<ConvTile> tiles(nt);
    HIPCHK(r, hipMemcpyAsync(tiles.data(), r->conv.tiles.p, nt * sizeof(ConvTile), hipMemcpyDeviceToHost, st));
    HIPCHK(r, hipStreamSynchronize(st));
    r->conv.err_n = n;
    conv_finish_tiles(tiles.data(), tx, ty, n, out, tile_error);
    return ORX_OK;
}

orx_status orx_get_display(orx_renderer* r, float inv_iterations, float inv_gamma, int32_t format, uint8_t* dst,
                           size_t dst_bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!positive_finite(inv_iterations) || !positive_finite(inv_gamma))
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "inv_iterations and inv_gamma must be finite and > 0");
    if (format != ORX_DISPLAY_RGBA8 && format != ORX_DISPLAY_BGRA8)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "unknown display format");
    if (!r->d_out.p) return set_err(r, ORX_ERR_STATE, "no frame rendered yet");
    const size_t npx = (size_t)r->rows * r->W;
    if (dst_bytes < npx * 4) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    HIPCHK(r, hipSetDevice(r->device));
    const orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    HIPCHK(r, r->d_display.ensure(npx * 4));
    hipStream_t st = cur_stream(r);
    launch_display(st, r->d_out.as<float>(), npx, inv_iterations, inv_gamma, format == ORX_DISPLAY_BGRA8,
                   r->d_display.as<uint32_t>());
    HIPCHK(r, hipGetLastError());
    HIPCHK(r, hipMemcpyAsync(dst, r->d_display.p, npx * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(r, hipStreamSynchronize(st));
    return ORX_OK;
}

}  // extern "C"
