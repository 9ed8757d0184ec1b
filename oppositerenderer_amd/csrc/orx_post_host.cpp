/*
 * orx_post_host.cpp — the host halves of the post passes, no device: orx_display_convert (the display rule of
 * include/orx_display.h over a host array) and the frame numbers of the convergence estimate from the
 * device's tile records.  Plain C++, so tests/post_host_check.cpp runs it under the sanitizers.
 */
#include <cmath>
#include <cstring>

#include "orx_display.h"
#include "orx_post.h"

void orx::conv_finish_tiles(const ConvTile* tiles, uint32_t tiles_x, uint32_t tiles_y, uint32_t n, orx_convergence* out,
                            float* tile_error) {
    std::memset(out, 0, sizeof *out);
    out->iterations = n;
    out->tiles_x = tiles_x;
    out->tiles_y = tiles_y;
    double se = 0.0, sm = 0.0;
    uint64_t px = 0, above = 0;
    bool have = false;
    const size_t nt = (size_t)tiles_x * tiles_y;
    for (size_t t = 0; t < nt; t++) {
        const ConvTile& q = tiles[t];
        const float mean = q.count ? q.sum_e / (float)q.count : 0.0f;
        if (tile_error) tile_error[t] = mean;
        se += (double)q.sum_e;
        sm += (double)q.sum_m;
        px += q.count;
        above += q.above;
        if (q.count && mean == mean && (!have || mean > out->max_tile_error)) {
            have = true;
            out->max_tile_error = mean;
            out->max_tile = (uint32_t)t;
        }
    }
    out->pixels_above = (uint32_t)above;
    out->mean_error = px ? (float)(se / (double)px) : 0.0f;
    out->mean_luminance = px ? (float)(sm / (double)px) : 0.0f;
}

extern "C" orx_status orx_display_convert(const float* sum, size_t n_pixels, float inv_iterations, float inv_gamma,
                                          int32_t format, uint8_t* dst) {
    if ((!sum || !dst) && n_pixels) return ORX_ERR_INVALID_ARGUMENT;
    if (!orx::positive_finite(inv_iterations) || !orx::positive_finite(inv_gamma)) return ORX_ERR_INVALID_ARGUMENT;
    if (format != ORX_DISPLAY_RGBA8 && format != ORX_DISPLAY_BGRA8) return ORX_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_pixels; i++) {
        const uint32_t px = orx_display_pixel(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2], inv_iterations, inv_gamma,
                                              format == ORX_DISPLAY_BGRA8);
        dst[4 * i + 0] = (uint8_t)(px & 255u);
        dst[4 * i + 1] = (uint8_t)((px >> 8) & 255u);
        dst[4 * i + 2] = (uint8_t)((px >> 16) & 255u);
        dst[4 * i + 3] = (uint8_t)(px >> 24);
    }
    return ORX_OK;
}
