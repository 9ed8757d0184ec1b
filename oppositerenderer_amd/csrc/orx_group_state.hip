/*
 * orx_group_state.hip — checkpoint / resume of a render group (include/orx.h, "Checkpoint / resume"): ROWS, one
 * frame of the ranks' rows; BATCH, a container of the ranks' frames.  Built from the per-rank halves of
 * orx_host_state.hip and the codec of orx_state.cpp, which also places a rank's rows in the frame on the host.
 */
#include "orx_group.h"
#include "orx_state.h"

using namespace orx;

extern "C" {

/* every rank has a frame and numbers to save */
static bool group_has_state(const orx_group* g) {
    if (!g || !g->W || !g->H) return false;
    for (const GroupRank& q : g->rk)
        if (!orx_state_bytes(q.r)) return false;
    return true;
}

size_t orx_group_state_bytes(const orx_group* g) {
    if (!group_has_state(g)) return 0;
    orx_state_info info;
    state_describe(g->rk[0].r, &info);
    if (g->gc.partition == ORX_GROUP_ROWS) return (size_t)info.total_bytes;
    return STATE_HEADER_BYTES + (size_t)g->n * (size_t)info.total_bytes;
}

/* ROWS: the ranks' rows into the frame at dst (header sealed by the caller) */
static orx_status rows_save_sections(orx_group* g, const orx_state_info& info, uint8_t* rng_host, uint8_t* out_host) {
    size_t nr = 0, no = 0;
    if (!state_frame_sections(&info, &nr, &no)) return gerr(g, ORX_ERR_STATE, "frame sizes overflow");
    const size_t rng_row = (size_t)info.rng_width * 24, out_row = (size_t)info.width * 12;
    if (g->comm->shared_device()) { /* one device: every rank's rows de-interleaved into one pair of arrays */
        GroupRank& root = g->rk[0];
        GroupBuf words, sum;
        GHIP(g, words.ensure(root.device, nr));
        GHIP(g, sum.ensure(root.device, no));
        for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, state_rows_export(g->rk[k].r, (uint32_t*)words.p, sum.f(), true));
        const orx_status s = group_sync(g);
        if (s != ORX_OK) return s;
        GHIP(g, hipSetDevice(root.device));
        GHIP(g, hipMemcpy(rng_host, words.p, nr, hipMemcpyDeviceToHost));
        GHIP(g, hipMemcpy(out_host, sum.p, no, hipMemcpyDeviceToHost));
        return ORX_OK;
    }
    /* a device per rank: its rows compact on its device, through the host, row by row into the frame */
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        const size_t jr = q.r->rng_rows, jo = q.r->rows;
        if (jr != state_rank_rows(info.rng_height, k, g->n) || jo != state_rank_rows(info.height, k, g->n))
            return gerr(g, ORX_ERR_STATE, "rank " + std::to_string(k) + " does not hold its rows of the frame");
        GroupBuf words, sum;
        std::vector<uint8_t> hw(jr * rng_row), hs(jo * out_row);
        GHIP(g, words.ensure(q.device, jr * rng_row));
        GHIP(g, sum.ensure(q.device, jo * out_row));
        GRANK(g, k, state_rows_export(q.r, (uint32_t*)words.p, sum.f(), false));
        GHIP(g, hipSetDevice(q.device));
        GHIP(g, hipStreamSynchronize(q.main));
        if (!hw.empty()) GHIP(g, hipMemcpy(hw.data(), words.p, hw.size(), hipMemcpyDeviceToHost));
        if (!hs.empty()) GHIP(g, hipMemcpy(hs.data(), sum.p, hs.size(), hipMemcpyDeviceToHost));
        state_place_rows(rng_host, hw.data(), jr, k, g->n, rng_row, true);
        state_place_rows(out_host, hs.data(), jo, k, g->n, out_row, true);
    }
    return ORX_OK;
}

orx_status orx_group_save_state(orx_group* g, void* dst, size_t dst_bytes) {
    if (!g || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!group_has_state(g)) return gerr(g, ORX_ERR_STATE, "no frame rendered yet (BATCH: on every rank)");
    const size_t need = orx_group_state_bytes(g);
    if (dst_bytes < need) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    uint8_t* p = static_cast<uint8_t*>(dst);
    if (g->gc.partition == ORX_GROUP_BATCH) {
        orx_state_info head;
        state_describe(g->rk[0].r, &head);
        const size_t each = (size_t)head.total_bytes;
        for (uint32_t k = 0; k < g->n; k++) {
            if (orx_state_bytes(g->rk[k].r) != each) return gerr(g, ORX_ERR_STATE, "the ranks' frames differ in size");
            GRANK(g, k, orx_save_state(g->rk[k].r, p + STATE_HEADER_BYTES + k * each, each));
        }
        head.kind = STATE_KIND_BATCH;
        head.flags = 0;
        head.world = g->n;
        head.calls = g->calls;
        head.total_bytes = need;
        /* the numbers of the group's last call: the rank that rendered it holds them */
        for (uint32_t k = 0; k < g->n; k++)
            if (g->rk[k].r->note.iter > head.iteration_number) {
                head.iteration_number = g->rk[k].r->note.iter;
                head.ppm_radius = g->rk[k].r->note.radius;
                head.method = g->rk[k].r->note.method;
            }
        head.local_iteration_number = g->calls ? g->calls - 1 : 0;
        state_write_header(&head, fnv1a64(p + STATE_HEADER_BYTES, need - STATE_HEADER_BYTES), FNV_BASIS, p);
        return ORX_OK;
    }
    for (uint32_t k = 0; k < g->n; k++) /* a sharded renderer with a medium box does not exist; as on one renderer */
        if (g->rk[k].r->media.on) return gerr(g, ORX_ERR_UNSUPPORTED, "participating media: the volumetric photon table is not part of the state");
    orx_state_info info;
    state_describe(g->rk[0].r, &info);
    size_t nr = 0, no = 0;
    if (!state_frame_sections(&info, &nr, &no)) return gerr(g, ORX_ERR_STATE, "frame sizes overflow");
    if ((s = rows_save_sections(g, info, p + STATE_HEADER_BYTES, p + STATE_HEADER_BYTES + nr)) != ORX_OK) return s;
    if (!state_seal_frame(&info, dst, dst_bytes)) return gerr(g, ORX_ERR_STATE, "could not pack the state");
    return ORX_OK;
}

/* ROWS: each rank loads its rows of the frame */
static orx_status rows_restore_sections(orx_group* g, const orx_state_info& info, const uint8_t* rng_host, const uint8_t* out_host) {
    size_t nr = 0, no = 0;
    state_frame_sections(&info, &nr, &no); /* a valid frame: checked by the codec */
    const size_t rng_row = (size_t)info.rng_width * 24, out_row = (size_t)info.width * 12;
    if (g->comm->shared_device()) {
        GroupRank& root = g->rk[0];
        GroupBuf words, sum;
        GHIP(g, words.ensure(root.device, nr));
        GHIP(g, sum.ensure(root.device, no));
        GHIP(g, hipSetDevice(root.device));
        GHIP(g, hipMemcpy(words.p, rng_host, nr, hipMemcpyHostToDevice));
        GHIP(g, hipMemcpy(sum.p, out_host, no, hipMemcpyHostToDevice));
        for (uint32_t k = 0; k < g->n; k++)
            GRANK(g, k, state_rows_import(g->rk[k].r, &info, (const uint32_t*)words.p, sum.f(), true));
        return ORX_OK;
    }
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        const size_t jr = state_rank_rows(info.rng_height, k, g->n), jo = state_rank_rows(info.height, k, g->n);
        std::vector<uint8_t> hw(jr * rng_row), hs(jo * out_row);
        state_place_rows(hw.data(), rng_host, jr, k, g->n, rng_row, false);
        state_place_rows(hs.data(), out_host, jo, k, g->n, out_row, false);
        GroupBuf words, sum;
        GHIP(g, words.ensure(q.device, hw.size()));
        GHIP(g, sum.ensure(q.device, hs.size()));
        GHIP(g, hipSetDevice(q.device));
        if (!hw.empty()) GHIP(g, hipMemcpy(words.p, hw.data(), hw.size(), hipMemcpyHostToDevice));
        if (!hs.empty()) GHIP(g, hipMemcpy(sum.p, hs.data(), hs.size(), hipMemcpyHostToDevice));
        GRANK(g, k, state_rows_import(q.r, &info, (const uint32_t*)words.p, sum.f(), false));
    }
    return ORX_OK;
}

orx_status orx_group_restore_state(orx_group* g, const void* blob, size_t bytes) {
    if (!g || !blob) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->scene_ready) return gerr(g, ORX_ERR_STATE, "orx_group_restore_state before orx_group_init_scene");
    orx_state_info info;
    const uint32_t* rng = nullptr;
    const float* out = nullptr;
    if (state_open(blob, bytes, &info, &rng, &out) != ORX_OK)
        return gerr(g, ORX_ERR_INVALID_ARGUMENT, "not a state blob (truncated, damaged or of another format version)");
    const bool batch = g->gc.partition == ORX_GROUP_BATCH;
    if (batch != (info.kind == STATE_KIND_BATCH))
        return gerr(g, ORX_ERR_INVALID_ARGUMENT, batch ? "a BATCH group restores a BATCH container, not a frame"
                                                        : "a ROWS group restores a frame, not a BATCH container");
    if (batch && info.world != g->n)
        return gerr(g, ORX_ERR_INVALID_ARGUMENT, "the container holds " + std::to_string(info.world) + " ranks, this group has " +
                                                     std::to_string(g->n));
    /* every frame is checked against its rank before any rank changes */
    std::vector<const uint8_t*> frames;
    std::vector<orx_state_info> fi;
    if (batch) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(rng);
        size_t left = (size_t)info.total_bytes - STATE_HEADER_BYTES;
        for (uint32_t k = 0; k < g->n; k++) {
            orx_state_info f;
            if (orx_state_info_read(p, left, &f) != ORX_OK || f.kind != STATE_KIND_FRAME)
                return gerr(g, ORX_ERR_INVALID_ARGUMENT, "the container's frame of rank " + std::to_string(k) + " is damaged");
            if (f.width != info.width || f.height != info.height)
                return gerr(g, ORX_ERR_INVALID_ARGUMENT, "the container's frames differ in size");
            GRANK(g, k, state_check(g->rk[k].r, &f));
            frames.push_back(p);
            fi.push_back(f);
            p += f.total_bytes;
            left -= (size_t)f.total_bytes;
        }
    } else {
        for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, state_check(g->rk[k].r, &info));
    }
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    /* the group's own frame size, method, exchange buffers and pipelining bookkeeping, as the first
     * request of that size sets them */
    orx_request det;
    std::memset(&det, 0, sizeof det);
    det.width = info.width;
    det.height = info.height;
    det.method = info.method;
    g->W = g->H = 0;
    g->method = -1;
    if ((s = group_prepare(g, &det)) != ORX_OK) return s;
    g->pending = -1;
    if (batch) {
        for (uint32_t k = 0; k < g->n; k++) {
            GRANK(g, k, orx_restore_state(g->rk[k].r, frames[k], (size_t)fi[k].total_bytes));
            g->rk[k].local_it = fi[k].local_iteration_number + 1;
        }
        g->calls = info.calls;
        return ORX_OK;
    }
    return rows_restore_sections(g, info, reinterpret_cast<const uint8_t*>(rng), reinterpret_cast<const uint8_t*>(out));
}

} /* extern "C" */
