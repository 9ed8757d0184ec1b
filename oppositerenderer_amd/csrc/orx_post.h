/*
 * orx_post.h — the passes over the running sum behind an iteration (orx_post.hip: convergence statistics,
 * the tile reduction of the estimate, the 8-bit display resolve) and the host code that finishes them
 * (orx_post_host.cpp, no device).  Internal: not installed.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "orx.h"

namespace orx {

/* what k_conv_tiles leaves per 16x16 tile of global pixel coordinates */
struct ConvTile {
    float sum_e, sum_m;    /* over the tile's pixels: error, mean luminance */
    uint32_t above, count; /* pixels with error > threshold; pixels the tile has */
};
/* an iteration's place in the statistics window: its number n (from 1) and whether it is the first of a
 * window whose base is a cleared sum (prev is then taken as 0) */
struct ConvIt {
    uint32_t n = 0, zero = 0;
};
constexpr uint32_t CONV_TILE = 16;

/* what the display and convergence entry points ask of a scale or a floor (NaN and infinity fail x - x == 0) */
inline bool positive_finite(float x) { return x > 0.0f && x - x == 0.0f; }

/* orx_post_host.cpp: the frame's numbers from the tile records (tile mean = sum_e / count in fp32, the frame
 * means in double; the worst tile is the first of the largest mean, tiles without a mean, NaN, never);
 * tile_error [tiles_y][tiles_x] or NULL */
void conv_finish_tiles(const ConvTile* tiles, uint32_t tiles_x, uint32_t tiles_y, uint32_t n, orx_convergence* out,
                       float* tile_error);

}  // namespace orx

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
struct orx_renderer;
namespace orx {

/* kernels' launchers (any full-frame plane, so the render group reuses them) */
void launch_conv_tiles(hipStream_t st, const float* e, const float* m, uint32_t W, uint32_t H, float threshold,
                       ConvTile* tiles);
void launch_display(hipStream_t st, const float* sum, size_t npx, float inv_iterations, float inv_gamma, int bgra,
                    uint32_t* dst);

/* the hooks of the host units; all of them return at once while the statistics are off */
/* a frame of another size (the sum was cleared): the planes follow, a new window on a zero base */
orx_status conv_resized(orx_renderer* r);
/* a new window whose base is the current sum (switched on mid-render, a restore); the renderer is idle */
orx_status conv_rebase(orx_renderer* r);
/* an iteration starts: its place in the window into r->conv.it (the one before into r->conv.last) */
void conv_begin(orx_renderer* r, uint64_t local_iteration_number);
/* the update of iteration `it` on `st`, behind that iteration's last write to the running sum */
void conv_update(orx_renderer* r, hipStream_t st, const ConvIt& it);
/* the error and mean-luminance planes of the renderer's own rows into e and m ([rows*W] each, device) on its
 * stream, behind an outstanding finish; ORX_ERR_STATE with the statistics off or a window of n < 2 */
orx_status conv_error_planes(orx_renderer* r, float floor, float* e, float* m, uint32_t* n_out);

}  // namespace orx
#endif
