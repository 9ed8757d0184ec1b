/*
 * orx_state.h — the checkpoint blob's codec (orx_state.cpp): header layout, checksums, the scene key, a rank's rows.
 * Host only: nothing here makes a HIP call.  The layout is documented in include/orx.h
 * ("Checkpoint / resume") and pinned by tests/golden/state_v1_tiny.bin.
 * Internal: not installed, nothing under include/ sees it.
 */
#pragma once
#include <cstddef>
#include <cstdint>

#include "orx.h"

namespace orx {

constexpr size_t STATE_HEADER_BYTES = 128;
constexpr uint32_t STATE_VERSION = 1;
constexpr uint32_t STATE_KIND_FRAME = 0, STATE_KIND_BATCH = 1;
constexpr uint32_t STATE_FLAG_VCM_ESTIMATED = 1u;

/* FNV-1a 64 over n bytes, continuing from h (the offset basis for a fresh sum) */
constexpr uint64_t FNV_BASIS = 0xcbf29ce484222325ull;
uint64_t fnv1a64(const void* p, size_t n, uint64_t h = FNV_BASIS);

/* bytes of a frame's two payload sections; false when a size overflows or a dimension is zero */
bool state_frame_sections(const orx_state_info* info, size_t* rng_bytes, size_t* out_bytes);

/* Writes the 128-byte header of `info` at dst with the payload checksums given and its own checksum;
 * info->total_bytes is written as it stands. */
void state_write_header(const orx_state_info* info, uint64_t sum_a, uint64_t sum_b, void* dst);

/* Finishes a frame blob whose payload sections were written in place behind the header at dst:
 * sets info->total_bytes, sums both sections and writes the header.  false: sizes overflow or dst too small. */
bool state_seal_frame(orx_state_info* info, void* dst, size_t dst_bytes);

/* orx_state_info_read and orx_state_unpack in one pass over the blob (the sections are summed once) */
orx_status state_open(const void* blob, size_t bytes, orx_state_info* info, const uint32_t** rng, const float** output);

/* the rows of `total` that rank k of n holds: k, k + n, k + 2 n, ... (orx_set_shard) */
uint32_t state_rank_rows(uint32_t total, uint32_t k, uint32_t n);

/* `rows` rows of row_bytes each between rank k's compact rows (local row j at j) and the frame's rows k + j n:
 * to_frame, dst is the frame and src the compact rows; else dst the compact rows and src the frame */
void state_place_rows(void* dst, const void* src, size_t rows, uint32_t k, uint32_t n, size_t row_bytes, bool to_frame);

}  // namespace orx
