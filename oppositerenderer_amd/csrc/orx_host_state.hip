/*
 * orx_host_state.hip — checkpoint / resume of one renderer (include/orx.h, "Checkpoint / resume"): the copy
 * kernels between the renderer's buffers and a blob's canonical arrays, orx_save_state and
 * orx_restore_state, and the per-rank halves orx_group_state.hip builds a group's save and restore from.
 * The blob's bytes are read and written by orx_state.cpp alone.
 *
 * Nothing here runs during an iteration: the scratch arrays live for one call.
 */
#include "orx_host.h"
#include "orx_state.h"

using namespace orx;

/* RNG planes [6][rows * RW] -> interleaved words [row][x][6]; local row j lands on row row0 + j * step
 * of dst (canonical: rank, world; compact: 0, 1).  One thread per slot: six coalesced plane loads, one
 * 24-byte record as three 8-byte stores (records are 8-byte aligned: the array is, and 24 = 3 * 8). */
__global__ void __launch_bounds__(256) k_state_rng_export(RngPlanes rng, uint32_t* __restrict__ dst, uint32_t RW,
                                                          uint32_t rows, uint32_t row0, uint32_t step) {
    const size_t n = (size_t)rows * RW;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += nt) {
        const size_t j = s / RW, x = s - j * RW;
        uint2* o = reinterpret_cast<uint2*>(dst + (((size_t)row0 + j * step) * RW + x) * 6);
        o[0] = make_uint2(rng.p[0][s], rng.p[1][s]);
        o[1] = make_uint2(rng.p[2][s], rng.p[3][s]);
        o[2] = make_uint2(rng.p[4][s], rng.p[5][s]);
    }
}

/* the inverse: row row0 + j * step of src -> local row j of the planes */
__global__ void __launch_bounds__(256) k_state_rng_import(RngPlanes rng, const uint32_t* __restrict__ src, uint32_t RW,
                                                          uint32_t rows, uint32_t row0, uint32_t step) {
    const size_t n = (size_t)rows * RW;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += nt) {
        const size_t j = s / RW, x = s - j * RW;
        const uint2* i = reinterpret_cast<const uint2*>(src + (((size_t)row0 + j * step) * RW + x) * 6);
        const uint2 a = i[0], b = i[1], c = i[2];
        rng.p[0][s] = a.x;
        rng.p[1][s] = a.y;
        rng.p[2][s] = b.x;
        rng.p[3][s] = b.y;
        rng.p[4][s] = c.x;
        rng.p[5][s] = c.y;
    }
}

/* rows of `len` floats: row s0 + j * sstep of src -> row d0 + j * dstep of dst, j < rows.  With (0, 1) ->
 * (rank, world) a rank's output rows go to their place in [H][W][3] (what k_group_assemble_rows does for
 * all ranks' blocks at once); with (rank, world) -> (0, 1) it is that kernel's inverse. */
__global__ void __launch_bounds__(256) k_state_rows_copy(const float* __restrict__ src, float* __restrict__ dst,
                                                         uint32_t len, uint32_t rows, uint32_t s0, uint32_t sstep,
                                                         uint32_t d0, uint32_t dstep) {
    const size_t n = (size_t)rows * len;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nt) {
        const size_t j = i / len, x = i - j * len;
        dst[((size_t)d0 + j * dstep) * len + x] = src[((size_t)s0 + j * sstep) * len + x];
    }
}

static inline uint32_t copy_grid(size_t items) { return (uint32_t)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, 4096)); }

void orx::state_describe(const orx_renderer* r, orx_state_info* info) {
    std::memset(info, 0, sizeof *info);
    info->version = STATE_VERSION;
    info->kind = STATE_KIND_FRAME;
    info->flags = r->vcm.estimated ? STATE_FLAG_VCM_ESTIMATED : 0u;
    info->width = r->W;
    info->height = r->H;
    info->rng_width = r->RW;
    info->rng_height = r->RH;
    info->photon_launch_width = r->cfg.photon_launch_width;
    info->photon_launch_height = r->cfg.photon_launch_height;
    info->method = r->note.method;
    info->ppm_radius = r->note.radius;
    info->iteration_number = r->note.iter;
    info->local_iteration_number = r->note.local;
    info->scene_key = r->note.scene_key;
    info->total_bytes = orx_state_packed_bytes(info);
}

orx_status orx::state_check(orx_renderer* r, const orx_state_info* info) {
    char msg[200];
    if (info->kind != STATE_KIND_FRAME)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "the state blob is a BATCH container, not a frame");
    if (info->scene_key != r->note.scene_key) {
        snprintf(msg, sizeof msg, "the state was saved for another scene: key %016llx, this renderer's scene has %016llx",
                 (unsigned long long)info->scene_key, (unsigned long long)r->note.scene_key);
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, msg);
    }
    const uint32_t PW = r->cfg.photon_launch_width, PH = r->cfg.photon_launch_height;
    if (info->photon_launch_width != PW || info->photon_launch_height != PH) {
        snprintf(msg, sizeof msg, "the state was saved with a photon launch of %u x %u, this renderer launches %u x %u",
                 info->photon_launch_width, info->photon_launch_height, PW, PH);
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, msg);
    }
    if (info->rng_width != std::max(PW, info->width) || info->rng_height != std::max(PH, info->height))
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "the state's RNG size is not max(photon launch, image)");
    return ORX_OK;
}

orx_status orx::state_rows_export(orx_renderer* r, uint32_t* rng_dev, float* out_dev, bool canonical) {
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t st = cur_stream(r);
    const uint32_t row0 = canonical ? r->rank : 0u, step = canonical ? r->world : 1u;
    if (r->rng_rows)
        hipLaunchKernelGGL(k_state_rng_export, dim3(copy_grid((size_t)r->rng_rows * r->RW)), dim3(256), 0, st, r->px.rng,
                           rng_dev, r->RW, r->rng_rows, row0, step);
    if (r->rows)
        hipLaunchKernelGGL(k_state_rows_copy, dim3(copy_grid((size_t)r->rows * r->W * 3)), dim3(256), 0, st,
                           (const float*)r->d_out.p, out_dev, r->W * 3, r->rows, 0u, 1u, row0, step);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx::state_rows_import(orx_renderer* r, const orx_state_info* info, const uint32_t* rng_dev, const float* out_dev,
                                  bool canonical) {
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s = sync_all(r); /* nothing in flight may touch the buffers being replaced */
    if (s != ORX_OK) return s;
    /* what begin_iteration does for a request of another size (resizeBuffers, OptixRenderer.cpp:826-848),
     * with the estimate flag of the saved render: the estimate launch advances every RNG slot */
    r->vcm.psf_x = 1.0f / (float)info->width;
    r->vcm.psf_y = 1.0f / (float)info->height;
    r->vcm.estimated = (info->flags & STATE_FLAG_VCM_ESTIMATED) != 0;
    if ((s = resize_unseeded(r, info->width, info->height)) != ORX_OK) return s;
    const uint32_t row0 = canonical ? r->rank : 0u, step = canonical ? r->world : 1u;
    if (r->rng_rows)
        hipLaunchKernelGGL(k_state_rng_import, dim3(copy_grid((size_t)r->rng_rows * r->RW)), dim3(256), 0, r->stream, r->px.rng,
                           rng_dev, r->RW, r->rng_rows, row0, step);
    if (r->rows)
        hipLaunchKernelGGL(k_state_rows_copy, dim3(copy_grid((size_t)r->rows * r->W * 3)), dim3(256), 0, r->stream, out_dev,
                           r->d_out.as<float>(), r->W * 3, r->rows, row0, step, 0u, 1u);
    HIPCHK(r, hipGetLastError());
    HIPCHK(r, hipStreamSynchronize(r->stream)); /* the caller frees the arrays; an external stream sees the frame */
    note_iteration(r, info->iteration_number, info->local_iteration_number, info->ppm_radius, info->method);
    return conv_rebase(r); /* the restored sum is the base of a new statistics window */
}

extern "C" {

size_t orx_state_bytes(const orx_renderer* r) {
    if (!r || !r->rng_ready || !r->note.have) return 0;
    orx_state_info info;
    state_describe(r, &info);
    return (size_t)info.total_bytes;
}

orx_status orx_save_state(orx_renderer* r, void* dst, size_t dst_bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (r->world > 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "a sharded renderer holds part of a frame: save through its render group");
    if (r->media.on)
        return set_err(r, ORX_ERR_UNSUPPORTED,
                       "participating media: the volumetric photon table the next eye pass gathers is not part of the state");
    if (!r->scene_ready || !r->rng_ready || !r->note.have) return set_err(r, ORX_ERR_STATE, "no frame rendered yet");
    orx_state_info info;
    state_describe(r, &info);
    size_t nr = 0, no = 0;
    if (!info.total_bytes || !state_frame_sections(&info, &nr, &no)) return set_err(r, ORX_ERR_STATE, "frame sizes overflow");
    if (dst_bytes < info.total_bytes) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s = sync_all(r); /* the pipelined gather, the overlapped resolve */
    if (s != ORX_OK) return s;
    DevBuf words, sum;
    HIPCHK(r, words.ensure(nr));
    HIPCHK(r, sum.ensure(no));
    if ((s = state_rows_export(r, words.as<uint32_t>(), sum.as<float>(), true)) != ORX_OK) return s;
    uint8_t* p = static_cast<uint8_t*>(dst) + STATE_HEADER_BYTES;
    HIPCHK(r, hipMemcpyAsync(p, words.p, nr, hipMemcpyDeviceToHost, cur_stream(r)));
    HIPCHK(r, hipMemcpyAsync(p + nr, sum.p, no, hipMemcpyDeviceToHost, cur_stream(r)));
    HIPCHK(r, hipStreamSynchronize(cur_stream(r)));
    if (!state_seal_frame(&info, dst, dst_bytes)) return set_err(r, ORX_ERR_STATE, "could not pack the state");
    return ORX_OK;
}

orx_status orx_restore_state(orx_renderer* r, const void* blob, size_t bytes) {
    if (!r || !blob) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->scene_ready) return set_err(r, ORX_ERR_STATE, "orx_restore_state before orx_init_scene");
    if (r->world > 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "a sharded renderer holds part of a frame: restore through its render group");
    if (r->media.on)
        return set_err(r, ORX_ERR_UNSUPPORTED, "participating media: a renderer with a medium box neither saves nor restores");
    orx_state_info info;
    const uint32_t* rng = nullptr;
    const float* out = nullptr;
    if (state_open(blob, bytes, &info, &rng, &out) != ORX_OK)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "not a state blob (truncated, damaged or of another format version)");
    orx_status s = state_check(r, &info);
    if (s != ORX_OK) return s;
    size_t nr = 0, no = 0;
    state_frame_sections(&info, &nr, &no); /* a valid frame: checked by the codec */
    HIPCHK(r, hipSetDevice(r->device));
    DevBuf words, sum;
    HIPCHK(r, words.ensure(nr));
    HIPCHK(r, sum.ensure(no));
    HIPCHK(r, hipMemcpy(words.p, rng, nr, hipMemcpyHostToDevice));
    HIPCHK(r, hipMemcpy(sum.p, out, no, hipMemcpyHostToDevice));
    return state_rows_import(r, &info, words.as<uint32_t>(), sum.as<float>(), true);
}

}  // extern "C"
