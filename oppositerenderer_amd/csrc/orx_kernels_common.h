/*
 * orx_kernels_common.h — device helpers that more than one kernel unit uses (private: included by
 * .hip units only).  What a single unit uses stays in that unit: wave_any and wave_min_u32 /
 * wave_max_u32 in orx_kernels.hip, block_exclusive_scan_256 in orx_grid.hip, slot_valid in orx_slab.hip.
 * Wave size is 64 on CDNA4; the reductions are written for it.
 */
#pragma once
#include "orx_kernels.h"

namespace orx {

/* float <-> uint32 whose unsigned order is the floats' order (atomicMin / atomicMax on floats; GridBox) */
__device__ __forceinline__ uint32_t f2ord(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

/* a wave's photon AABB into PhotonBufs::bbox (the photon pass and the slab import; k_grid_setup folds it) */
__device__ __forceinline__ void photon_bbox_flush(const PhotonBufs& pb, float lo_x, float lo_y, float lo_z, float hi_x,
                                                  float hi_y, float hi_z, uint32_t rep, uint32_t lane) {
    /* wave AABB -> device-wide ordered-int atomics (one lane per component) */
    lo_x = wave_min(lo_x); lo_y = wave_min(lo_y); lo_z = wave_min(lo_z);
    hi_x = wave_max(hi_x); hi_y = wave_max(hi_y); hi_z = wave_max(hi_z);
    /* 64 replicas per component keep same-address atomic contention low */
    if (lane < 6) {
        float v = lane == 0 ? lo_x : lane == 1 ? lo_y : lane == 2 ? lo_z : lane == 3 ? hi_x : lane == 4 ? hi_y : hi_z;
        if (lane < 3) {
            if (v != INFINITY) atomicMin(&pb.bbox[lane * BBOX_REPLICAS + rep], f2ord(v));
        } else {
            if (v != -INFINITY) atomicMax(&pb.bbox[lane * BBOX_REPLICAS + rep], f2ord(v));
        }
    }
}

/* The end of a gather kernel, in two halves.  The hash and kd-tree gathers call them; the two
 * uniform-grid kernels (orx_kernels.hip) carry the same statements written out, because they sit at
 * their register caps and the calls changed their spill counts: a change here is made there too.
 * gather_store, for a lane with a pixel i: the estimate of IndirectRadianceEstimation.cu:211-221,
 * the summed flux `acc` times the hit point's attenuation (B.w, Cc), over pi r^2, over the emitted
 * photons, in exactly this order of operations (the hash gather's sums are the oracle's bit for
 * bit), and the lane's visit counts dC cells / dP photons into dbg. */
__device__ __forceinline__ void gather_store(const GatherIn& gi, const Consts& c, size_t i, const f3& acc, const float4& B,
                                             const float2& Cc, uint32_t dC, uint32_t dP) {
    const f3 att = mk(B.w, Cc.x, Cc.y);
    const float s1 = 1.0f / (ORX_PI_F * c.ppm_radius2);
    const float s2 = 1.0f / c.emitted_f;
    const f3 ind = ((acc * att) * s1) * s2;
    gi.indirect[3 * i + 0] = ind.x;
    gi.indirect[3 * i + 1] = ind.y;
    gi.indirect[3 * i + 2] = ind.z;
    if (gi.dbg) {
        gi.dbg[2 * i] = dC;
        gi.dbg[2 * i + 1] = dP;
    }
}
/* gather_count, for every lane of the wave: its counts added to the grid's counters.  CELLS = false:
 * the kd-tree gather, which visits nodes and has no cell counter to add to. */
template <bool CELLS = true>
__device__ __forceinline__ void gather_count(const PhotonBufs& pb, uint32_t dC, uint32_t dP) {
    const uint64_t sp = wave_sum_u64(dP), sc = CELLS ? wave_sum_u64(dC) : 0;
    if ((threadIdx.x & 63) == 0 && sp) {
        atomicAdd((unsigned long long*)&pb.grid->photons_visited, (unsigned long long)sp);
        if (CELLS) atomicAdd((unsigned long long*)&pb.grid->cells_visited, (unsigned long long)sc);
        atomicAdd((unsigned long long*)&pb.grid->photons_visited_total, (unsigned long long)sp);
        if (CELLS) atomicAdd((unsigned long long*)&pb.grid->cells_visited_total, (unsigned long long)sc);
    }
}

}  // namespace orx
