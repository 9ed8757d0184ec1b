/*
 * orx_photon_grid.h — what the photon grid build (orx_grid.hip) and the uniform-grid gather
 * (orx_kernels.hip) must agree on (private: included by .hip units only).  The plane indices SP_*
 * and the sub-cell counts SUBX / SUBR are in orx_kernels.h: the host sizes and exports the planes
 * with them.
 *
 * Sorted planes.  PhotonBufs::sorted holds the grid's photons as SP_PLANES float planes of stride
 * splane (SoA): position x y z, the direction word dir_q8 (below), the exact direction, the power.
 * Photon k of the order below is element k of every plane (grid_put).
 *
 * Order, sub-row layout (nsub = SUBR^2 = 4).  Photons are ordered by a virtual cell
 *   vc = ((y + z gy) nsub + s) gx + x,   s = SUBR (z half) + (y half),
 * then by the x quarter: every cell row (y,z) is stored as four sub-rows, each
 * holding the photons of one (y,z) quarter of the row's cells in x order.  A
 * gather chord on a sub-row is one contiguous range of subofs, and the
 * quarter-height sub-rows hug the sphere (fewer photons tested per pixel);
 * the photons of a reference cell are the union of its four sub-row pieces,
 * so the reference offsets (the visit counters, the exported grid) come from
 * the sub-row offsets by k_grid_coarse_offsets.  With nsub = 1 (cell order) vc is the reference's
 * cell x + y gx + z gx gy.
 *
 * Sub-cell key (PhotonBufs::keys, bs_pairs) = vc * SUBX + q, q the x quarter of the photon in its
 * cell; PhotonBufs::subofs[key] is the first photon of that sub-cell, so sub-row (y, z, s) is
 * subofs[((y + z gy) nsub + s) gx SUBX + ...] and the quarters a0..a1 of it hold the photons
 * [subofs[a0], subofs[a1 + 1]).  Cell, half and quarter of a photon are floors of
 * (p - origin) / cell scaled by 1, SUBR and SUBX, each clamped into its cell (k_bs_count).
 */
#pragma once
#include "orx_kernels.h"

namespace orx {

/* The gather decides which sub-rows and quarters can hold a photon within r of a hit point from
 * their boxes grown by this fraction of a cell: far above the rounding of the build's cell, half
 * and quarter assignment (a few ulp of the coordinate), so no photon within r is missed. */
constexpr float GRID_MARGIN = 1e-3f;

/* Direction prefilter word of a grid photon (sorted plane SP_DIRQ): the
 * direction as three int8 snorm bytes q = rint(127 d).  The gather's facing
 * test dot(d, n) <= 0 is decided from v_dot4_i32_i8(q, qn) (qn the same
 * quantisation of the hit point's normal) whenever that integer dot lies
 * outside +-DIRQ_BAND; inside the band the exact fp32 direction planes decide.
 * Bound: |q/127 - d|_inf <= 0.5/127 + eps, so for |d|_1, |n|_1 <= 1.7325
 *   |qd.qn - 127^2 d.n| <= 127^2 (0.5/127 (|d|_1 + |n|_1) + 3 (0.5/127)^2) <= 221
 * and every decision taken from the integer dot equals the exact one.  A
 * direction (or normal) outside that 1-norm bound, with a component above 1 in
 * magnitude (which would wrap in the byte) or NaN quantises to 0, which always
 * lands in the band. */
constexpr int32_t DIRQ_BAND = 232;
__device__ __forceinline__ uint32_t dir_q8(float x, float y, float z) {
    /* the 1-norm bound of the error estimate, and |c| <= 1 so rint(127 c) fits an int8 */
    if (!(fabsf(x) + fabsf(y) + fabsf(z) <= 1.7325f) || !(fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))) <= 1.0f))
        return 0u;
    const int32_t qx = (int32_t)rintf(x * 127.f), qy = (int32_t)rintf(y * 127.f), qz = (int32_t)rintf(z * 127.f);
    return ((uint32_t)qx & 0xffu) | (((uint32_t)qy & 0xffu) << 8) | (((uint32_t)qz & 0xffu) << 16);
}

}  // namespace orx
