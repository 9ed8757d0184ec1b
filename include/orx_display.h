/*
 * orx_display.h — the 8-bit display rule, one function for the host call (orx_display_convert) and the
 * device resolve (orx_get_display): same text, same bytes (orx_powf of orx_detmath.h is bit-identical on
 * both sides; the product and the truncation are exact fp32 operations).
 *
 * The rule is the reference consumer's (Gui/gui/RenderWidget.cpp:197 divides the running sum by the
 * iteration count, :296-313 applies gamma and clamps to bytes), restated:
 *     v = c * inv_iterations
 *     !(v > 0)  (zero, negative, NaN)  ->  0
 *     else g = orx_powf(v, inv_gamma) * 255.f;  (uint8_t)fminf(255.f, g)     (truncation; inf -> 255)
 */
#ifndef ORX_DISPLAY_H
#define ORX_DISPLAY_H

#include "orx_detmath.h"

#ifdef __cplusplus
extern "C" {
#endif

static inline ORX_HD uint32_t orx_display_byte(float c, float inv_iterations, float inv_gamma) {
    const float v = c * inv_iterations;
    if (!(v > 0.0f)) return 0u;
    if (v == orx_as_float(0x7f800000u)) return 255u; /* orx_powf takes finite arguments */
    const float g = orx_powf(v, inv_gamma) * 255.0f;
    return g < 255.0f ? (uint32_t)g : 255u; /* fminf(255.f, g), g > 0 and never NaN here */
}

/* one pixel as a little-endian dword: bytes R G B A (bgra = 0) or B G R A (bgra != 0), alpha 255 */
static inline ORX_HD uint32_t orx_display_pixel(float r, float g, float b, float inv_iterations, float inv_gamma,
                                                int bgra) {
    const uint32_t br = orx_display_byte(r, inv_iterations, inv_gamma);
    const uint32_t bg = orx_display_byte(g, inv_iterations, inv_gamma);
    const uint32_t bb = orx_display_byte(b, inv_iterations, inv_gamma);
    return (bgra ? bb : br) | (bg << 8) | ((bgra ? br : bb) << 16) | 0xff000000u;
}

#ifdef __cplusplus
}
#endif

#endif /* ORX_DISPLAY_H */
