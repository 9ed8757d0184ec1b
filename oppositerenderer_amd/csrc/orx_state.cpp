/*
 * orx_state.cpp — the checkpoint blob's codec: everything that parses or writes its bytes
 * (include/orx.h, "Checkpoint / resume").  Plain C++: no HIP call, no renderer, no device; built with the
 * host compiler and, alone, under the sanitizers (tests/state_codec_check.cpp).
 *
 * Every read of a blob goes through rd32 / rd64 on offsets below a size checked first; size fields are
 * multiplied with overflow checks before anything is indexed with them.
 */
#include "orx_state.h"

#include <cstring>

namespace orx {

static const char MAGIC[8] = {'O', 'R', 'X', 'S', 'T', 'A', 'T', 'E'};

/* header offsets (bytes) */
enum : size_t {
    O_MAGIC = 0, O_VERSION = 8, O_HEADER = 12, O_TOTAL = 16, O_KIND = 24, O_FLAGS = 28, O_W = 32, O_H = 36,
    O_RW = 40, O_RH = 44, O_PW = 48, O_PH = 52, O_METHOD = 56, O_RADIUS = 60, O_ITER = 64, O_LOCAL = 72,
    O_SCENE = 80, O_WORLD = 88, O_RESERVED = 92, O_CALLS = 96, O_SUM_A = 104, O_SUM_B = 112, O_SUM_HEADER = 120
};
static_assert(O_SUM_HEADER + 8 == STATE_HEADER_BYTES, "header layout");

uint64_t fnv1a64(const void* p, size_t n, uint64_t h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) {
        h ^= b[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

static void wr32(unsigned char* p, uint32_t v) {
    for (int k = 0; k < 4; k++) p[k] = (unsigned char)(v >> (8 * k));
}
static void wr64(unsigned char* p, uint64_t v) {
    for (int k = 0; k < 8; k++) p[k] = (unsigned char)(v >> (8 * k));
}
static uint32_t rd32(const unsigned char* p) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
static uint64_t rd64(const unsigned char* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

static bool mul_ok(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_mul_overflow(a, b, out); }
static bool add_ok(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_add_overflow(a, b, out); }

bool state_frame_sections(const orx_state_info* info, size_t* rng_bytes, size_t* out_bytes) {
    if (!info->width || !info->height || info->rng_width < info->width || info->rng_height < info->height) return false;
    uint64_t slots = 0, rng = 0, px = 0, out = 0, sum = 0;
    if (!mul_ok(info->rng_width, info->rng_height, &slots) || !mul_ok(slots, 24, &rng)) return false;
    if (!mul_ok(info->width, info->height, &px) || !mul_ok(px, 12, &out)) return false;
    if (!add_ok(rng, out, &sum) || !add_ok(sum, STATE_HEADER_BYTES, &sum)) return false;
    if (sum > (uint64_t)SIZE_MAX) return false;
    *rng_bytes = (size_t)rng;
    *out_bytes = (size_t)out;
    return true;
}

void state_write_header(const orx_state_info* info, uint64_t sum_a, uint64_t sum_b, void* dst) {
    unsigned char* h = static_cast<unsigned char*>(dst);
    std::memset(h, 0, STATE_HEADER_BYTES);
    std::memcpy(h + O_MAGIC, MAGIC, 8);
    wr32(h + O_VERSION, STATE_VERSION);
    wr32(h + O_HEADER, (uint32_t)STATE_HEADER_BYTES);
    wr64(h + O_TOTAL, info->total_bytes);
    wr32(h + O_KIND, info->kind);
    wr32(h + O_FLAGS, info->flags);
    wr32(h + O_W, info->width);
    wr32(h + O_H, info->height);
    wr32(h + O_RW, info->rng_width);
    wr32(h + O_RH, info->rng_height);
    wr32(h + O_PW, info->photon_launch_width);
    wr32(h + O_PH, info->photon_launch_height);
    wr32(h + O_METHOD, (uint32_t)info->method);
    uint32_t rbits;
    std::memcpy(&rbits, &info->ppm_radius, 4);
    wr32(h + O_RADIUS, rbits);
    wr64(h + O_ITER, info->iteration_number);
    wr64(h + O_LOCAL, info->local_iteration_number);
    wr64(h + O_SCENE, info->scene_key);
    wr32(h + O_WORLD, info->world);
    wr64(h + O_CALLS, info->calls);
    wr64(h + O_SUM_A, sum_a);
    wr64(h + O_SUM_B, sum_b);
    wr64(h + O_SUM_HEADER, fnv1a64(h, O_SUM_HEADER));
}

bool state_seal_frame(orx_state_info* info, void* dst, size_t dst_bytes) {
    size_t rng = 0, out = 0;
    if (!dst || info->kind != STATE_KIND_FRAME || !state_frame_sections(info, &rng, &out)) return false;
    const size_t total = STATE_HEADER_BYTES + rng + out;
    if (dst_bytes < total) return false;
    info->version = STATE_VERSION;
    info->total_bytes = total;
    const unsigned char* p = static_cast<const unsigned char*>(dst) + STATE_HEADER_BYTES;
    state_write_header(info, fnv1a64(p, rng), fnv1a64(p + rng, out), dst);
    return true;
}

/* header and payload checks shared by orx_state_info_read and orx_state_unpack; the section offsets of a
 * frame through *rng_off / *out_off (a container: its payload, and 0) */
static orx_status state_parse(const void* blob, size_t bytes, orx_state_info* out, size_t* rng_off, size_t* out_off) {
    if (!blob || !out || bytes < STATE_HEADER_BYTES) return ORX_ERR_INVALID_ARGUMENT;
    const unsigned char* h = static_cast<const unsigned char*>(blob);
    if (std::memcmp(h + O_MAGIC, MAGIC, 8) != 0) return ORX_ERR_INVALID_ARGUMENT;
    if (rd32(h + O_VERSION) != STATE_VERSION || rd32(h + O_HEADER) != STATE_HEADER_BYTES) return ORX_ERR_INVALID_ARGUMENT;
    if (rd64(h + O_SUM_HEADER) != fnv1a64(h, O_SUM_HEADER)) return ORX_ERR_INVALID_ARGUMENT;
    orx_state_info i;
    std::memset(&i, 0, sizeof i);
    i.version = STATE_VERSION;
    i.total_bytes = rd64(h + O_TOTAL);
    i.kind = rd32(h + O_KIND);
    i.flags = rd32(h + O_FLAGS);
    i.width = rd32(h + O_W);
    i.height = rd32(h + O_H);
    i.rng_width = rd32(h + O_RW);
    i.rng_height = rd32(h + O_RH);
    i.photon_launch_width = rd32(h + O_PW);
    i.photon_launch_height = rd32(h + O_PH);
    i.method = (int32_t)rd32(h + O_METHOD);
    const uint32_t rbits = rd32(h + O_RADIUS);
    std::memcpy(&i.ppm_radius, &rbits, 4);
    i.iteration_number = rd64(h + O_ITER);
    i.local_iteration_number = rd64(h + O_LOCAL);
    i.scene_key = rd64(h + O_SCENE);
    i.world = rd32(h + O_WORLD);
    i.calls = rd64(h + O_CALLS);
    if (rd32(h + O_RESERVED) != 0) return ORX_ERR_INVALID_ARGUMENT;
    if (i.total_bytes < STATE_HEADER_BYTES || i.total_bytes > (uint64_t)bytes) return ORX_ERR_INVALID_ARGUMENT;
    size_t a = 0, b = 0;
    if (i.kind == STATE_KIND_FRAME) {
        if (!state_frame_sections(&i, &a, &b)) return ORX_ERR_INVALID_ARGUMENT;
        if (i.total_bytes != (uint64_t)STATE_HEADER_BYTES + a + b) return ORX_ERR_INVALID_ARGUMENT; /* no overflow: checked */
        if (i.world != 0 || i.calls != 0) return ORX_ERR_INVALID_ARGUMENT;
    } else if (i.kind == STATE_KIND_BATCH) {
        if (i.world == 0 || i.world > 64) return ORX_ERR_INVALID_ARGUMENT;
        a = (size_t)(i.total_bytes - STATE_HEADER_BYTES);
    } else {
        return ORX_ERR_INVALID_ARGUMENT;
    }
    const unsigned char* p = h + STATE_HEADER_BYTES;
    if (rd64(h + O_SUM_A) != fnv1a64(p, a) || rd64(h + O_SUM_B) != fnv1a64(p + a, b)) return ORX_ERR_INVALID_ARGUMENT;
    *out = i;
    if (rng_off) *rng_off = STATE_HEADER_BYTES;
    if (out_off) *out_off = i.kind == STATE_KIND_FRAME ? STATE_HEADER_BYTES + a : 0;
    return ORX_OK;
}

orx_status state_open(const void* blob, size_t bytes, orx_state_info* info, const uint32_t** rng, const float** output) {
    size_t a = 0, b = 0;
    if (!rng || !output) return ORX_ERR_INVALID_ARGUMENT;
    const orx_status s = state_parse(blob, bytes, info, &a, &b);
    if (s != ORX_OK) return s;
    const unsigned char* h = static_cast<const unsigned char*>(blob);
    *rng = reinterpret_cast<const uint32_t*>(h + a);
    *output = b ? reinterpret_cast<const float*>(h + b) : nullptr;
    return ORX_OK;
}

uint32_t state_rank_rows(uint32_t total, uint32_t k, uint32_t n) { return total > k ? (total - k + n - 1) / n : 0u; }

void state_place_rows(void* dst, const void* src, size_t rows, uint32_t k, uint32_t n, size_t row_bytes, bool to_frame) {
    for (size_t j = 0; j < rows; j++) {
        const size_t frame = (k + j * n) * row_bytes, compact = j * row_bytes;
        std::memcpy(static_cast<unsigned char*>(dst) + (to_frame ? frame : compact),
                    static_cast<const unsigned char*>(src) + (to_frame ? compact : frame), row_bytes);
    }
}

/* one array of a scene into the key: its presence, then its bytes */
static uint64_t key_array(uint64_t h, const void* p, uint64_t count, size_t elem) {
    const unsigned char present = p && count ? 1 : 0;
    h = fnv1a64(&present, 1, h);
    return present ? fnv1a64(p, (size_t)count * elem, h) : h;
}
static uint64_t key_u32(uint64_t h, uint32_t v) {
    unsigned char b[4];
    wr32(b, v);
    return fnv1a64(b, 4, h);
}

}  // namespace orx

using namespace orx;

extern "C" {

orx_status orx_state_info_read(const void* blob, size_t bytes, orx_state_info* out) {
    return state_parse(blob, bytes, out, nullptr, nullptr);
}

size_t orx_state_packed_bytes(const orx_state_info* info) {
    size_t rng = 0, out = 0;
    if (!info || info->kind != STATE_KIND_FRAME || !state_frame_sections(info, &rng, &out)) return 0;
    return STATE_HEADER_BYTES + rng + out;
}

orx_status orx_state_pack(const orx_state_info* info, const uint32_t* rng, const float* output, void* dst, size_t dst_bytes) {
    size_t nr = 0, no = 0;
    if (!info || !rng || !output || !dst || info->kind != STATE_KIND_FRAME || !state_frame_sections(info, &nr, &no))
        return ORX_ERR_INVALID_ARGUMENT;
    if (dst_bytes < STATE_HEADER_BYTES + nr + no) return ORX_ERR_INVALID_ARGUMENT;
    unsigned char* p = static_cast<unsigned char*>(dst) + STATE_HEADER_BYTES;
    /* the payload is little-endian words; so is every host this builds for */
    std::memcpy(p, rng, nr);
    std::memcpy(p + nr, output, no);
    orx_state_info i = *info;
    i.world = 0;
    i.calls = 0;
    return state_seal_frame(&i, dst, dst_bytes) ? ORX_OK : ORX_ERR_INVALID_ARGUMENT;
}

orx_status orx_state_unpack(const void* blob, size_t bytes, const uint32_t** rng, const float** output) {
    orx_state_info i;
    return state_open(blob, bytes, &i, rng, output);
}

uint64_t orx_scene_key(const orx_scene* s) {
    if (!s) return 0;
    uint64_t h = FNV_BASIS;
    h = key_u32(h, s->n_quads);
    h = key_array(h, s->quads, s->n_quads, 36);
    h = key_array(h, s->quad_material, s->n_quads, 4);
    h = key_u32(h, s->n_spheres);
    h = key_array(h, s->spheres, s->n_spheres, 16);
    h = key_array(h, s->sphere_material, s->n_spheres, 4);
    h = key_u32(h, s->n_vertices);
    h = key_array(h, s->vertices, s->n_vertices, 12);
    h = key_array(h, s->normals, s->n_vertices, 12);
    h = key_u32(h, s->n_triangles);
    h = key_array(h, s->triangles, s->n_triangles, 12);
    h = key_array(h, s->triangle_material, s->n_triangles, 4);
    h = key_u32(h, s->n_materials);
    static_assert(sizeof(orx_material) == 20 * 4 && sizeof(orx_light) == 17 * 4, "4-byte fields, no padding");
    h = key_array(h, s->materials, s->n_materials, sizeof(orx_material));
    h = key_u32(h, s->n_lights);
    h = key_array(h, s->lights, s->n_lights, sizeof(orx_light));
    h = fnv1a64(s->aabb_min, 12, h);
    h = fnv1a64(s->aabb_max, 12, h);
    h = key_array(h, s->texcoords, s->n_vertices, 8);
    h = key_array(h, s->tangents, s->n_vertices, 12);
    h = key_array(h, s->bitangents, s->n_vertices, 12);
    h = key_u32(h, s->n_textures);
    for (uint32_t t = 0; s->textures && t < s->n_textures; t++) {
        const orx_texture& x = s->textures[t];
        h = key_u32(h, x.width);
        h = key_u32(h, x.height);
        h = key_array(h, x.rgba, (uint64_t)x.width * x.height, 4);
        h = key_u32(h, x.normal_width);
        h = key_u32(h, x.normal_height);
        h = key_array(h, x.normal_rgba, (uint64_t)x.normal_width * x.normal_height, 4);
    }
    h = key_u32(h, s->n_media);
    h = key_array(h, s->media, s->n_media, 32);
    return h;
}

}  // extern "C"
