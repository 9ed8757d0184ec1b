/*
 * state_codec_check.cpp — the checkpoint codec (oppositerenderer_amd/csrc/orx_state.cpp) as a program of its
 * own, built by tests/test_state_codec.py with that source alone under AddressSanitizer +
 * UndefinedBehaviorSanitizer.  Every blob handed to the codec sits in a heap allocation of exactly its
 * length, so a read past `bytes` is a sanitizer report.  It asserts:
 *   1. pack -> info_read / unpack round trips, words bit-equal, for 4x2 (rng 4x2) and 5x3 (rng 7x4);
 *   2. every prefix of a valid blob, a wrong magic, version 2, a flipped byte at every offset (header, both
 *      sections, all three checksums), a total size beyond `bytes`, and sizes whose product overflows 64 bits
 *      (with the header checksum made right again, so that the size check is what rejects) all give
 *      ORX_ERR_INVALID_ARGUMENT;
 *   3. a seeded mutation fuzz of 4000 blobs (byte flips, truncation, random header words with the header
 *      checksum repaired) never faults, and whatever it accepts has sections inside the allocation;
 *   4. orx_scene_key ignores pointer values and sees every array;
 *   5. row placement (state_rank_rows, state_place_rows: what a ROWS group's per-rank save and restore do on the
 *      host) for worlds 1, 2, 3, 5, row totals 1, 4, 5, 25 and rows of 24 and 12 bytes times a width of 7.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "orx.h"
#include "orx_state.h"

static int failures = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                               \
        }                                                             \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

/* the blob in an allocation of exactly n bytes */
static std::unique_ptr<unsigned char[]> exact(const std::vector<unsigned char>& v, size_t n) {
    std::unique_ptr<unsigned char[]> p(new unsigned char[n ? n : 1]);
    if (n) std::memcpy(p.get(), v.data(), n);
    return p;
}
static orx_status read_exact(const std::vector<unsigned char>& v, size_t n, orx_state_info* info) {
    auto p = exact(v, n);
    const uint32_t* r = nullptr;
    const float* o = nullptr;
    const orx_status a = orx_state_info_read(p.get(), n, info);
    const orx_status b = orx_state_unpack(p.get(), n, &r, &o);
    CHECK(a == b);
    if (b == ORX_OK) { /* the views lie inside the allocation */
        size_t nr = 0, no = 0;
        if (info->kind == 0) {
            CHECK(orx::state_frame_sections(info, &nr, &no));
            CHECK((const unsigned char*)r == p.get() + 128 && (const unsigned char*)o == p.get() + 128 + nr);
            CHECK(128 + nr + no <= n);
            volatile unsigned char sink = 0; /* touch both ends of both sections */
            sink ^= ((const unsigned char*)r)[0] ^ ((const unsigned char*)r)[nr - 1];
            sink ^= ((const unsigned char*)o)[0] ^ ((const unsigned char*)o)[no - 1];
        } else {
            CHECK(info->total_bytes <= n);
        }
    }
    return a;
}

static void repair_header_sum(std::vector<unsigned char>& b) {
    const uint64_t h = orx::fnv1a64(b.data(), 120);
    for (int k = 0; k < 8; k++) b[120 + k] = (unsigned char)(h >> (8 * k));
}

static std::vector<unsigned char> make_blob(uint32_t W, uint32_t H, uint32_t RW, uint32_t RH, std::vector<uint32_t>* words,
                                            std::vector<float>* sum) {
    orx_state_info info;
    std::memset(&info, 0, sizeof info);
    info.kind = 0;
    info.flags = 1;
    info.width = W;
    info.height = H;
    info.rng_width = RW;
    info.rng_height = RH;
    info.photon_launch_width = RW;
    info.photon_launch_height = RH;
    info.method = ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING;
    info.ppm_radius = 0.123f;
    info.iteration_number = 41;
    info.local_iteration_number = 40;
    info.scene_key = 0x0123456789abcdefull;
    words->resize((size_t)RW * RH * 6);
    sum->resize((size_t)W * H * 3);
    for (uint32_t& w : *words) w = rnd();
    for (float& f : *sum) f = (float)rnd() / 65536.0f;
    const size_t n = orx_state_packed_bytes(&info);
    CHECK(n == 128 + words->size() * 4 + sum->size() * 4);
    std::vector<unsigned char> blob(n);
    CHECK(orx_state_pack(&info, words->data(), sum->data(), blob.data(), n - 1) == ORX_ERR_INVALID_ARGUMENT);
    CHECK(orx_state_pack(&info, words->data(), sum->data(), blob.data(), n) == ORX_OK);
    return blob;
}

static void round_trip(uint32_t W, uint32_t H, uint32_t RW, uint32_t RH) {
    std::vector<uint32_t> words;
    std::vector<float> sum;
    const std::vector<unsigned char> blob = make_blob(W, H, RW, RH, &words, &sum);
    orx_state_info got;
    CHECK(read_exact(blob, blob.size(), &got) == ORX_OK);
    CHECK(got.version == 1 && got.kind == 0 && got.flags == 1 && got.width == W && got.height == H);
    CHECK(got.rng_width == RW && got.rng_height == RH && got.photon_launch_width == RW && got.photon_launch_height == RH);
    CHECK(got.method == ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING && got.ppm_radius == 0.123f);
    CHECK(got.iteration_number == 41 && got.local_iteration_number == 40 && got.scene_key == 0x0123456789abcdefull);
    CHECK(got.total_bytes == blob.size() && got.world == 0 && got.calls == 0);
    const uint32_t* r = nullptr;
    const float* o = nullptr;
    CHECK(orx_state_unpack(blob.data(), blob.size(), &r, &o) == ORX_OK);
    CHECK(std::memcmp(r, words.data(), words.size() * 4) == 0);
    CHECK(std::memcmp(o, sum.data(), sum.size() * 4) == 0);
    /* trailing bytes beyond the total are ignored */
    std::vector<unsigned char> longer = blob;
    longer.resize(blob.size() + 5, 0xAA);
    CHECK(read_exact(longer, longer.size(), &got) == ORX_OK);
}

static void rejections(uint32_t W, uint32_t H, uint32_t RW, uint32_t RH) {
    std::vector<uint32_t> words;
    std::vector<float> sum;
    const std::vector<unsigned char> blob = make_blob(W, H, RW, RH, &words, &sum);
    orx_state_info info;
    for (size_t n = 0; n < blob.size(); n++) CHECK(read_exact(blob, n, &info) == ORX_ERR_INVALID_ARGUMENT);
    for (size_t at = 0; at < blob.size(); at++) { /* header, both sections and the three checksums */
        std::vector<unsigned char> b = blob;
        b[at] ^= (unsigned char)(1u << (at % 8));
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
    }
    {
        std::vector<unsigned char> b = blob; /* magic, with a right header checksum */
        b[0] = 'X';
        repair_header_sum(b);
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
        b = blob; /* version 2 */
        b[8] = 2;
        repair_header_sum(b);
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
        b = blob; /* total one more than the bytes given */
        const uint64_t t = blob.size() + 1;
        for (int k = 0; k < 8; k++) b[16 + k] = (unsigned char)(t >> (8 * k));
        repair_header_sum(b);
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
        /* rng 2^32-1 squared times 24 overflows 64 bits; so does the total that would match it */
        for (uint64_t total : {(uint64_t)blob.size(), ~(uint64_t)0, (uint64_t)128}) {
            b = blob;
            for (int k = 0; k < 8; k++) b[40 + k] = 0xFF;
            for (int k = 0; k < 8; k++) b[16 + k] = (unsigned char)(total >> (8 * k));
            repair_header_sum(b);
            CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
        }
        b = blob; /* image 2^32-1 squared: the product fits, times 12 does not */
        for (int k = 0; k < 8; k++) b[32 + k] = 0xFF;
        for (int k = 0; k < 8; k++) b[40 + k] = 0xFF;
        repair_header_sum(b);
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
        b = blob; /* kind 2 */
        b[24] = 2;
        repair_header_sum(b);
        CHECK(read_exact(b, b.size(), &info) == ORX_ERR_INVALID_ARGUMENT);
    }
    CHECK(orx_state_info_read(nullptr, 128, &info) == ORX_ERR_INVALID_ARGUMENT);
    CHECK(orx_state_info_read(blob.data(), blob.size(), nullptr) == ORX_ERR_INVALID_ARGUMENT);
    orx_state_info bad;
    std::memset(&bad, 0, sizeof bad);
    bad.width = bad.height = bad.rng_width = bad.rng_height = 0xFFFFFFFFu;
    CHECK(orx_state_packed_bytes(&bad) == 0);
    CHECK(orx_state_packed_bytes(nullptr) == 0);
    bad.width = 4, bad.height = 2, bad.rng_width = 3, bad.rng_height = 2; /* rng narrower than the image */
    CHECK(orx_state_packed_bytes(&bad) == 0);
}

static void fuzz(int rounds) {
    std::vector<uint32_t> words;
    std::vector<float> sum;
    const std::vector<unsigned char> blob = make_blob(5, 3, 7, 4, &words, &sum);
    int accepted = 0;
    for (int it = 0; it < rounds; it++) {
        std::vector<unsigned char> b = blob;
        const uint32_t mode = rnd() % 4;
        if (mode == 0) { /* a few byte flips anywhere */
            for (uint32_t k = 0, n = 1 + rnd() % 4; k < n; k++) b[rnd() % b.size()] ^= (unsigned char)(1 + rnd() % 255);
        } else if (mode == 1) { /* random header words, checksum repaired: sizes reach the size checks */
            for (uint32_t k = 0, n = 1 + rnd() % 3; k < n; k++) {
                const size_t at = 16 + 4 * (rnd() % 26);
                const uint32_t v = rnd() % 3 == 0 ? 0xFFFFFFFFu : rnd() % 2 ? rnd() % 9 : (rnd() << 16) ^ rnd();
                for (int q = 0; q < 4; q++) b[at + q] = (unsigned char)(v >> (8 * q));
            }
            repair_header_sum(b);
        } else if (mode == 2) { /* truncated, header repaired to claim the new length */
            b.resize(rnd() % b.size());
            if (b.size() >= 128) {
                const uint64_t t = b.size();
                for (int k = 0; k < 8; k++) b[16 + k] = (unsigned char)(t >> (8 * k));
                repair_header_sum(b);
            }
        } else { /* a container header over a frame's payload */
            b[24] = 1;
            b[88] = (unsigned char)(rnd() % 70);
            repair_header_sum(b);
        }
        orx_state_info info;
        if (read_exact(b, b.size(), &info) == ORX_OK) accepted++;
    }
    std::printf("fuzz: %d blobs, %d accepted\n", rounds, accepted);
    CHECK(accepted < rounds / 4); /* only header fields without consequence may change */
}

static void scene_key() {
    float quads[18], quads2[18];
    uint32_t qm[2] = {0, 1}, qm2[2] = {0, 1};
    for (int i = 0; i < 18; i++) quads[i] = quads2[i] = (float)i * 0.5f;
    orx_material mats[2];
    orx_light light;
    std::memset(mats, 0, sizeof mats);
    std::memset(&light, 0, sizeof light);
    mats[1].Kd[0] = 0.5f;
    light.power[0] = 10.f;
    orx_scene a;
    std::memset(&a, 0, sizeof a);
    a.n_quads = 2;
    a.quads = quads;
    a.quad_material = qm;
    a.n_materials = 2;
    a.materials = mats;
    a.n_lights = 1;
    a.lights = &light;
    a.aabb_max[0] = 1.f;
    orx_scene b = a;
    b.quads = quads2; /* other pointers, same contents */
    b.quad_material = qm2;
    CHECK(orx_scene_key(&a) == orx_scene_key(&b));
    CHECK(orx_scene_key(&a) != 0 && orx_scene_key(nullptr) == 0);
    const uint64_t k0 = orx_scene_key(&a);
    quads2[17] += 1.f;
    CHECK(orx_scene_key(&b) != k0);
    quads2[17] -= 1.f;
    qm2[1] = 0;
    CHECK(orx_scene_key(&b) != k0);
    qm2[1] = 1;
    mats[1].Kd[0] = 0.25f;
    CHECK(orx_scene_key(&a) != k0);
    mats[1].Kd[0] = 0.5f;
    light.power[0] = 11.f;
    CHECK(orx_scene_key(&a) != k0);
    light.power[0] = 10.f;
    a.aabb_max[0] = 2.f;
    CHECK(orx_scene_key(&a) != k0);
    a.aabb_max[0] = 1.f;
    float medium[8] = {0, 0, 0, 1, 1, 1, 0.5f, 0.1f};
    a.n_media = 1;
    a.media = medium;
    CHECK(orx_scene_key(&a) != k0);
    a.n_media = 0;
    a.media = nullptr;
    CHECK(orx_scene_key(&a) == k0);
}

/* Row placement of a ROWS group's per-rank checkpoint path: rank k of n holds the rows k, k + n, ... of `total`.
 * Every rank's compact rows, filled with a pattern of (rank, local row, byte), go into one frame between guard
 * bytes; every frame byte is checked against the closed form (row y belongs to rank y % n as its local row y / n),
 * the guards must be untouched, and the reverse direction must give the compact rows back bit for bit. */
static unsigned char row_pattern(uint32_t k, size_t j, size_t b) { return (unsigned char)(k * 89u + j * 31u + b * 7u + 1u); }

static void row_placement(uint32_t n, uint32_t total, size_t row_bytes) {
    const size_t GUARD = 64, frame_bytes = (size_t)total * row_bytes;
    std::vector<unsigned char> frame(GUARD + frame_bytes + GUARD, 0xEE);
    std::vector<std::vector<unsigned char>> compact(n);
    uint32_t held = 0;
    for (uint32_t k = 0; k < n; k++) {
        uint32_t want = 0; /* len(range(k, total, n)) */
        for (uint32_t y = k; y < total; y += n) want++;
        const uint32_t rows = orx::state_rank_rows(total, k, n);
        CHECK(rows == want);
        if (rows != want) return;
        held += rows;
        /* exactly the rank's bytes (one spare byte where it has none), so that a row too many is a sanitizer report */
        compact[k].assign(rows ? rows * row_bytes : 1, 0);
        for (size_t j = 0; j < rows; j++)
            for (size_t b = 0; b < row_bytes; b++) compact[k][j * row_bytes + b] = row_pattern(k, j, b);
        orx::state_place_rows(frame.data() + GUARD, compact[k].data(), rows, k, n, row_bytes, true);
    }
    CHECK(held == total);
    for (size_t i = 0; i < GUARD; i++) CHECK(frame[i] == 0xEE && frame[GUARD + frame_bytes + i] == 0xEE);
    for (size_t y = 0; y < total; y++)
        for (size_t b = 0; b < row_bytes; b++)
            CHECK(frame[GUARD + y * row_bytes + b] == row_pattern((uint32_t)(y % n), y / n, b));
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t rows = orx::state_rank_rows(total, k, n);
        std::vector<unsigned char> back(rows ? rows * row_bytes : 1, 0);
        orx::state_place_rows(back.data(), frame.data() + GUARD, rows, k, n, row_bytes, false);
        CHECK(back == compact[k]);
    }
}

int main() {
    for (uint32_t n : {1u, 2u, 3u, 5u})
        for (uint32_t total : {1u, 4u, 5u, 25u})
            for (size_t row_bytes : {(size_t)24 * 7, (size_t)12 * 7}) row_placement(n, total, row_bytes);
    CHECK(orx::state_rank_rows(4, 4, 5) == 0); /* world 5, 4 rows: rank 4 holds none */
    round_trip(4, 2, 4, 2);
    round_trip(5, 3, 7, 4);
    rejections(4, 2, 4, 2);
    rejections(5, 3, 7, 4);
    fuzz(4000);
    scene_key();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
