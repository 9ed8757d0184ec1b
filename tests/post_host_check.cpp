/*
 * post_host_check.cpp — the host halves of the post passes (csrc/orx_post_host.cpp: orx_display_convert and
 * the tile finishing of orx_get_convergence) as a program of its own, built with AddressSanitizer +
 * UndefinedBehaviorSanitizer by tests/test_convergence_cpu.py.  Buffers are heap blocks of exactly the
 * documented sizes, so a read or write past an odd-sized array is reported.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "orx.h"
#include "orx_display.h"
#include "orx_post.h"

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            failures++;                                           \
        }                                                         \
    } while (0)

static void display_sizes() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)37 * 21, (size_t)1025}) {
        float* sum = (float*)std::malloc(n * 12 + 1);
        uint8_t* dst = (uint8_t*)std::malloc(n * 4 + 1);
        unsigned s = 12345u + (unsigned)n;
        for (size_t i = 0; i < 3 * n; i++) {
            s = s * 1664525u + 1013904223u;
            sum[i] = (float)(s >> 8) * (4.0f / 16777216.0f);
        }
        if (n >= 3) {
            const float special[9] = {0.f, -1.f, nan, inf, 1e-30f, 1.f, 0.5f, 4.f, -inf};
            std::memcpy(sum, special, sizeof special);
        }
        for (int fmt = 0; fmt < 2; fmt++) {
            CHECK(orx_display_convert(sum, n, 0.5f, 1.0f / 2.2f, fmt, dst) == ORX_OK);
            for (size_t i = 0; i < n; i++) {
                CHECK(dst[4 * i + 3] == 255);
                for (int c = 0; c < 3; c++)
                    CHECK(dst[4 * i + (fmt ? 2 - c : c)] == orx_display_byte(sum[3 * i + c], 0.5f, 1.0f / 2.2f));
            }
        }
        if (n >= 3) {
            CHECK(orx_display_convert(sum, n, 1.0f, 1.0f, 0, dst) == ORX_OK);
            CHECK(dst[0] == 0 && dst[1] == 0 && dst[2] == 0);     /* 0, -1, NaN */
            CHECK(dst[4] == 255 && dst[5] == 0 && dst[6] == 255); /* inf, 1e-30, 1 */
            CHECK(dst[8] == 127 && dst[9] == 255 && dst[10] == 0); /* 0.5 -> 127.5 truncated, 4 clamped, -inf */
        }
        std::free(sum);
        std::free(dst);
    }
    float one[3] = {1, 1, 1};
    uint8_t px[4];
    const float bad[5] = {0.f, -1.f, nan, inf, -inf};
    for (float b : bad) {
        CHECK(orx_display_convert(one, 1, b, 1.f, 0, px) == ORX_ERR_INVALID_ARGUMENT);
        CHECK(orx_display_convert(one, 1, 1.f, b, 0, px) == ORX_ERR_INVALID_ARGUMENT);
    }
    CHECK(orx_display_convert(one, 1, 1.f, 1.f, 2, px) == ORX_ERR_INVALID_ARGUMENT);
    CHECK(orx_display_convert(one, 1, 1.f, 1.f, -1, px) == ORX_ERR_INVALID_ARGUMENT);
    CHECK(orx_display_convert(nullptr, 1, 1.f, 1.f, 0, px) == ORX_ERR_INVALID_ARGUMENT);
    CHECK(orx_display_convert(one, 1, 1.f, 1.f, 0, nullptr) == ORX_ERR_INVALID_ARGUMENT);
}

static void tile_finish() {
    /* frames of odd sizes: 37x21 (3x2 tiles, partial in both axes), 1x1, 16x16, 17x33 */
    const unsigned sizes[4][2] = {{37, 21}, {1, 1}, {16, 16}, {17, 33}};
    for (const auto& wh : sizes) {
        const unsigned W = wh[0], H = wh[1], tx = (W + 15) / 16, ty = (H + 15) / 16;
        const size_t nt = (size_t)tx * ty;
        orx::ConvTile* tiles = (orx::ConvTile*)std::malloc(nt * sizeof(orx::ConvTile));
        float* map = (float*)std::malloc(nt * 4);
        double se = 0, sm = 0;
        unsigned px = 0, above = 0, worst = 0;
        float worst_mean = -1.f;
        for (unsigned j = 0; j < ty; j++)
            for (unsigned i = 0; i < tx; i++) {
                const unsigned w = std::min(16u, W - 16 * i), h = std::min(16u, H - 16 * j), t = i + tx * j;
                tiles[t].count = w * h;
                tiles[t].sum_e = 0.01f * (float)(w * h) * (float)(1 + (t * 7) % 5);
                tiles[t].sum_m = 0.5f * (float)(w * h);
                tiles[t].above = t % 3;
                se += tiles[t].sum_e;
                sm += tiles[t].sum_m;
                px += w * h;
                above += t % 3;
                const float mean = tiles[t].sum_e / (float)(w * h);
                if (mean > worst_mean) {
                    worst_mean = mean;
                    worst = t;
                }
            }
        orx_convergence c;
        for (float* out_map : {map, (float*)nullptr}) {
            orx::conv_finish_tiles(tiles, tx, ty, 6, &c, out_map);
            CHECK(c.iterations == 6 && c.tiles_x == tx && c.tiles_y == ty);
            CHECK(px == W * H && c.pixels_above == above);
            CHECK(c.max_tile == worst && c.max_tile_error == worst_mean);
            CHECK(c.mean_error == (float)(se / px) && c.mean_luminance == (float)(sm / px));
            CHECK(c.reserved[0] == 0 && c.reserved[1] == 0 && c.reserved[2] == 0);
        }
        for (size_t t = 0; t < nt; t++) CHECK(map[t] == tiles[t].sum_e / (float)tiles[t].count);
        /* a tile whose mean is NaN is never the worst; an empty record divides nothing */
        tiles[0].sum_e = std::numeric_limits<float>::quiet_NaN();
        orx::conv_finish_tiles(tiles, tx, ty, 2, &c, map);
        CHECK(nt == 1 || c.max_tile != 0);
        tiles[0].count = 0;
        orx::conv_finish_tiles(tiles, tx, ty, 2, &c, map);
        CHECK(map[0] == 0.f);
        std::free(tiles);
        std::free(map);
    }
}

int main() {
    display_sizes();
    tile_finish();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
