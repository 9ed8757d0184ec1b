/*
 * orx_group.hip — multi-GPU render groups behind the C ABI (include/orx.h, orx_create_group).
 *
 * A group is N orx_renderer ranks behind one handle plus the collectives between them, so that a C++
 * host drives an N-GPU frame with the call sequence of one renderer.  It restates in C++ what the
 * reference does in DistributedApplication.cpp:96-122 (deal iterations and radii to the render
 * servers), RenderServerRenderer.cpp:146-165 (renderNextIteration per request) and
 * RenderResultPacketReceiver.cpp:63-190 (merge the running sums), and what
 * oppositerenderer_amd/multigpu.py does over torch.distributed:
 *
 *   ORX_GROUP_ROWS   one frame over N row shards (orx_set_shard): ShardedPPM / ShardedVCM / ShardedPT
 *   ORX_GROUP_BATCH  whole iterations dealt round-robin, running sums merged: BatchSharded
 *
 * Everything the ranks do goes through the public phase API of include/orx.h; this file adds only the
 * orchestration and the exchange buffers.  The communicator (LOCAL or RCCL) and the group's kernels are
 * orx_group_comm.hip, checkpoint / resume is orx_group_state.hip.
 *
 * photon_partition = ORX_PHOTONS_SLABS puts the spatial photon partition (orx_set_slab_partition) behind
 * the same handle: ShardedPPM._iteration_slab and slab_exchange of multigpu.py with the planner of
 * orx_slab_plan.cpp on the host and the photon records moved by GroupComm::all_to_all_v.
 */
#include <chrono>
#include <new>

#include "orx_group.h"
#include "orx_slab_plan.h"

static thread_local std::string g_create_error;

/* a rank's exported hit points (orx_export_hitpoints): seven planes of its padded rows */
static inline size_t hp_bytes(const orx_group* g) { return orx::hp_export_plane((size_t)g->max_rows * g->W) * 28; }

orx_status group_sync(orx_group* g) {
    for (GroupRank& q : g->rk) {
        GHIP(g, hipSetDevice(q.device));
        for (hipStream_t s : {q.main, q.comm, q.side, q.fin})
            if (s) GHIP(g, hipStreamSynchronize(s));
    }
    return ORX_OK;
}

template <class F>
static std::vector<hipStream_t> streams_of(orx_group* g, F pick) {
    std::vector<hipStream_t> st(g->n);
    for (uint32_t k = 0; k < g->n; k++) st[k] = pick(g->rk[k]);
    return st;
}

/* pipelined ROWS PPM: the outstanding reduce-scatter + orx_ppm_finish_on, on the finish streams */
static orx_status group_drain(orx_group* g) {
    if (g->pending < 0) return ORX_OK;
    const int s = g->pending;
    g->pending = -1;
    const size_t blk = (size_t)g->max_rows * g->W * 3;
    std::vector<const float*> send(g->n);
    std::vector<float*> recv(g->n);
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        GHIP(g, hipSetDevice(q.device));
        GHIP(g, hipStreamWaitEvent(q.fin, q.ev_partial, 0));
        send[k] = q.ind_partial[s].f();
        recv[k] = q.ind_local[s].f();
    }
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.fin; });
    GCOMM(g, g->comm->reduce_scatter(send.data(), recv.data(), blk, st.data(), e_));
    for (uint32_t k = 0; k < g->n; k++)
        GRANK(g, k, orx_ppm_finish_on(g->rk[k].r, recv[k], blk * 4, (void*)g->rk[k].fin));
    return ORX_OK;
}

orx_status group_quiesce(orx_group* g) {
    const orx_status s = group_drain(g);
    return s != ORX_OK ? s : group_sync(g);
}

orx_status group_prepare(orx_group* g, const orx_request* det) {
    if (det->width == 0 || det->height == 0) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "zero-sized request");
    const bool resized = det->width != g->W || det->height != g->H;
    if (!resized && det->method == g->method) return ORX_OK;
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    g->method = det->method;
    if (!resized) return ORX_OK;
    if ((s = group_sync(g)) != ORX_OK) return s;
    g->W = det->width;
    g->H = det->height;
    g->k = 0;
    const bool rows = g->gc.partition == ORX_GROUP_ROWS;
    g->max_rows = rows ? (g->H + g->n - 1) / g->n : g->H;
    const size_t blk = (size_t)g->max_rows * g->W * 3 * 4, hpb = hp_bytes(g);
    const bool shared = g->comm->shared_device();
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        GHIP(g, q.out_local.ensure(q.device, blk));
        q.local_it = 0;
        if (!rows) continue;
        for (int set = 0; set < (g->pipe ? 2 : 1); set++) {
            GHIP(g, q.hp_local[set].ensure(q.device, hpb));
            if (!shared || k == 0) GHIP(g, q.hp_all[set].ensure(q.device, hpb * g->n));
            GHIP(g, q.ind_partial[set].ensure(q.device, blk * g->n));
            GHIP(g, q.ind_local[set].ensure(q.device, blk));
        }
        GHIP(g, q.splat_all.ensure(q.device, blk * g->n));
        GHIP(g, q.splat_own.ensure(q.device, blk));
        if (!shared || k == 0) GHIP(g, q.out_all.ensure(q.device, blk * g->n));
    }
    g->calls = 0;
    GHIP(g, g->image.ensure(g->rk[0].device, (size_t)g->W * g->H * 12));
    return ORX_OK;
}

/* the rank whose gathered buffers rank k reads: on a shared device rank 0's serve everyone */
static inline GroupRank& gather_holder(orx_group* g, uint32_t k) { return g->rk[g->comm->shared_device() ? 0 : k]; }

static hipStream_t main_stream(GroupRank& q) { return q.main; }

/* an all-gather of `bytes` per rank on the streams `stream` picks: rank k sends own(rank k) and receives every
 * rank's block, in rank order, in gathered(its gather_holder) */
template <class S, class A, class B>
static orx_status group_all_gather(orx_group* g, S stream, A own, B gathered, size_t bytes) {
    std::vector<const void*> send(g->n);
    std::vector<void*> recv(g->n);
    for (uint32_t k = 0; k < g->n; k++) {
        send[k] = own(g->rk[k]);
        recv[k] = gathered(gather_holder(g, k));
    }
    const std::vector<hipStream_t> st = streams_of(g, stream);
    GCOMM(g, g->comm->all_gather(send.data(), recv.data(), bytes, st.data(), e_));
    return ORX_OK;
}

/* SLABS, after the photon trace: histograms -> plan (host) -> pack -> all-to-all of the photon records ->
 * import + grid (multigpu.py slab_exchange), all on the ranks' main streams.  The host waits for the copy of
 * the gathered histograms (that stream only): the one synchronisation per iteration the slab partition adds.
 * When it returns every rank's histogram of this iteration is in, so each rank's main stream is past the
 * previous iteration's import, and the previous all-to-all is done: the record buffers may be replaced. */
static orx_status slab_exchange(orx_group* g, float radius) {
    const uint32_t n = g->n, NB = ORX_GROUP_SLAB_BINS;
    const size_t words = orx_slab_histogram_words(NB);
    for (uint32_t k = 0; k < n; k++) GRANK(g, k, orx_ppm_slab_histogram(g->rk[k].r, (uint32_t*)g->rk[k].hist.p, NB));
    const orx_status s = group_all_gather(
        g, main_stream, [](GroupRank& q) { return q.hist.p; }, [](GroupRank& q) { return q.hists.p; }, words * 4);
    if (s != ORX_OK) return s;
    GroupRank& root = g->rk[0];
    GHIP(g, hipSetDevice(root.device));
    GHIP(g, hipMemcpyAsync(g->h_hists, root.hists.p, words * 4 * n, hipMemcpyDeviceToHost, root.main));
    GHIP(g, hipStreamSynchronize(root.main));
    uint32_t halo[3];
    for (uint32_t a = 0; a < 3; a++) halo[a] = orx_ppm_slab_halo(root.r, NB, a, radius);
    g->plan.have = false;
    g->plan.counts.assign((size_t)n * n, 0);
    if (orx_slab_plan(g->h_hists, n, NB, halo, &g->plan.axis, g->plan.bin_dest, g->plan.counts.data(), g->plan.box) != ORX_OK)
        return gerr(g, ORX_ERR_STATE, "orx_slab_plan rejected the group's histograms");
    const uint64_t* counts = g->plan.counts.data();
    const uint32_t axis = g->plan.axis;
    std::vector<const float*> out(n);
    std::vector<float*> in(n);
    const orx::SlabRunLayout lay = orx::slab_run_layout(counts, n);
    const std::vector<uint64_t>& n_recv = lay.recv_total;
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        const uint64_t n_send = lay.send_total[k];
        q.dest_base.assign(n, 0);
        for (uint32_t d = 0; d < n; d++) {
            const uint64_t base = lay.send_ofs[(size_t)k * n + d];
            if (base > 0xffffffffull) return gerr(g, ORX_ERR_UNSUPPORTED, "send buffer beyond 2^32 records");
            q.dest_base[d] = (uint32_t)base;
        }
        /* sized from the plan, an eighth to spare so that a slowly growing count does not reallocate */
        const size_t need = (size_t)n_send * ORX_RECORD_DWORDS * 4;
        if (q.rec_send.bytes < need || !q.rec_send.p) GHIP(g, q.rec_send.ensure(q.device, need + need / 8));
        GRANK(g, k, orx_ppm_slab_pack(q.r, g->plan.bin_dest, NB, axis, halo[axis], q.dest_base.data(), n_send, q.rec_send.p));
        out[k] = q.rec_send.f();
    }
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        const size_t need = (size_t)n_recv[k] * ORX_RECORD_DWORDS * 4;
        if (q.rec_recv.bytes < need || !q.rec_recv.p) GHIP(g, q.rec_recv.ensure(q.device, need + need / 8));
        in[k] = q.rec_recv.f();
    }
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    GCOMM(g, g->comm->all_to_all_v(out.data(), in.data(), counts, st.data(), e_));
    for (uint32_t k = 0; k < n; k++) {
        uint32_t lo, hi;
        orx::slab_owned(g->plan.bin_dest, NB, k, &lo, &hi);
        GRANK(g, k, orx_ppm_slab_import(g->rk[k].r, in[k], n_recv[k], g->plan.box, axis, NB, lo, hi));
    }
    g->plan.have = true;
    return ORX_OK;
}

static orx_status rows_ppm_pipelined(orx_group* g, uint64_t it, uint64_t local_it, float radius, const orx_request* det) {
    const int s = (int)g->k;
    g->k ^= 1u;
    const uint32_t n = g->n;
    const size_t hpb = hp_bytes(g), blk = (size_t)g->max_rows * g->W * 12;
    /* eye pass, then export; the all-gather on the communication streams behind it */
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_ppm_local_eye(q.r, it, local_it, radius, det));
        GRANK(g, k, orx_export_hitpoints(q.r, q.hp_local[s].p, hpb));
        GHIP(g, hipEventRecord(q.ev_export, q.main));
        GHIP(g, hipStreamWaitEvent(q.comm, q.ev_export, 0));
    }
    orx_status s0 = group_all_gather(
        g, [](GroupRank& q) { return q.comm; }, [s](GroupRank& q) { return q.hp_local[s].p; },
        [s](GroupRank& q) { return q.hp_all[s].p; }, hpb);
    if (s0 != ORX_OK) return s0;
    for (uint32_t k = 0; k < n; k++) {
        GHIP(g, hipSetDevice(g->rk[k].device));
        GHIP(g, hipEventRecord(g->rk[k].ev_gathered, g->rk[k].comm));
    }
    /* the previous iteration's reduce-scatter + finish, issued behind this all-gather */
    if ((s0 = group_drain(g)) != ORX_OK) return s0;
    if (g->slabs) { /* photon trace; the grid is built over the imported photons of the rank's slab */
        for (uint32_t k = 0; k < n; k++) GRANK(g, k, orx_ppm_local_photon_trace(g->rk[k].r));
        if ((s0 = slab_exchange(g, radius)) != ORX_OK) return s0;
    } else {
        for (uint32_t k = 0; k < n; k++) GRANK(g, k, orx_ppm_local_photons(g->rk[k].r));
    }
    /* the gather on the side stream once the hit points are in */
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GHIP(g, hipSetDevice(q.device));
        GHIP(g, hipStreamWaitEvent(q.side, q.ev_gathered, 0));
        GRANK(g, k, orx_ppm_gather_external(q.r, gather_holder(g, k).hp_all[s].p, n, q.ind_partial[s].p, blk * n));
        GHIP(g, hipSetDevice(q.device));
        GHIP(g, hipEventRecord(q.ev_partial, q.side));
    }
    g->pending = s;
    return ORX_OK;
}

static orx_status rows_ppm_serial(orx_group* g, uint64_t it, uint64_t local_it, float radius, const orx_request* det) {
    const uint32_t n = g->n;
    const size_t hpb = hp_bytes(g), blk = (size_t)g->max_rows * g->W * 12;
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        if (g->slabs) GRANK(g, k, orx_ppm_local_trace(q.r, it, local_it, radius, det));
        else GRANK(g, k, orx_ppm_local_passes(q.r, it, local_it, radius, det));
        GRANK(g, k, orx_export_hitpoints(q.r, q.hp_local[0].p, hpb));
    }
    orx_status s0 = group_all_gather(
        g, main_stream, [](GroupRank& q) { return q.hp_local[0].p; }, [](GroupRank& q) { return q.hp_all[0].p; }, hpb);
    if (s0 != ORX_OK) return s0;
    if (g->slabs) {
        s0 = slab_exchange(g, radius);
        if (s0 != ORX_OK) return s0;
    }
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    std::vector<const float*> part(n);
    std::vector<float*> own(n);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_ppm_gather_external(q.r, gather_holder(g, k).hp_all[0].p, n, q.ind_partial[0].p, blk * n));
        part[k] = q.ind_partial[0].f();
        own[k] = q.ind_local[0].f();
    }
    GCOMM(g, g->comm->reduce_scatter(part.data(), own.data(), blk / 4, st.data(), e_));
    for (uint32_t k = 0; k < n; k++) GRANK(g, k, orx_ppm_finish(g->rk[k].r, own[k], blk));
    return ORX_OK;
}

static orx_status rows_vcm(orx_group* g, uint64_t it, uint64_t local_it, float radius, const orx_request* det) {
    const uint32_t n = g->n;
    const size_t blk = (size_t)g->max_rows * g->W * 12;
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    std::vector<const float*> all(n);
    std::vector<float*> own(n);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_vcm_local_light(q.r, it, local_it, radius, det));
        GRANK(g, k, orx_export_vcm_splats(q.r, q.splat_all.p, blk * n));
        all[k] = q.splat_all.f();
        own[k] = q.splat_own.f();
    }
    GCOMM(g, g->comm->reduce_scatter(all.data(), own.data(), blk / 4, st.data(), e_));
    for (uint32_t k = 0; k < n; k++)
        GRANK(g, k, orx_vcm_finish(g->rk[k].r, own[k], (size_t)orx_local_rows(g->rk[k].r) * g->W * 12));
    return ORX_OK;
}

/* BATCH: the sum of the ranks' running sums into rank 0's image (a rank that has not rendered this
 * frame size yet contributes zeros).  Overwrites the image: nothing accumulates across calls. */
static orx_status batch_reduce(orx_group* g) {
    const uint32_t n = g->n;
    const size_t bytes = (size_t)g->W * g->H * 12;
    std::vector<const float*> send(n);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        if (q.local_it > 0) {
            GRANK(g, k, orx_get_output_device(q.r, q.out_local.p, bytes));
        } else {
            GHIP(g, hipSetDevice(q.device));
            GHIP(g, hipMemsetAsync(q.out_local.p, 0, bytes, q.main));
        }
        send[k] = q.out_local.f();
    }
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    GCOMM(g, g->comm->reduce(send.data(), g->image.f(), bytes / 4, st.data(), e_));
    return ORX_OK;
}

static void group_free(orx_group* g) {
    if (!g) return;
    for (GroupRank& q : g->rk) {
        if (q.r) {
            hipSetDevice(q.device);
            for (hipStream_t s : {q.comm, q.side, q.fin})
                if (s) hipStreamSynchronize(s);
        }
    }
    delete g->comm; /* before the renderers and streams its collectives ran on */
    g->comm = nullptr;
    for (GroupRank& q : g->rk) {
        if (q.r) orx_destroy(q.r); /* synchronises the renderer's own streams */
        hipSetDevice(q.device);
        for (hipStream_t s : {q.comm, q.side, q.fin})
            if (s) hipStreamDestroy(s);
        for (hipEvent_t e : {q.ev_export, q.ev_gathered, q.ev_partial})
            if (e) hipEventDestroy(e);
    }
    if (g->h_hists) hipHostFree(g->h_hists);
    delete g; /* every GroupBuf, on its device */
}

extern "C" {

void orx_default_group_config(orx_group_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->partition = ORX_GROUP_BATCH;
    c->comm = ORX_COMM_AUTO;
    c->reduce_every = 8;
    c->pipeline = 1;
}

uint32_t orx_batch_seed(uint32_t seed, uint32_t rank, uint64_t clock_ns) {
    if (rank == 0) return seed;
    if (seed == 0) seed = (uint32_t)(clock_ns ^ (clock_ns >> 32));
    const uint32_t s = seed + 0x9E3779B9u * rank;
    return s ? s : 1u;
}

orx_status orx_create_group(uint32_t n, const int* hip_devices, const orx_config* cfg, const orx_group_config* gcfg,
                            orx_group** out) {
    /* every argument check before the first HIP call */
    if (out) *out = nullptr;
    g_create_error.clear();
    if (!out || !hip_devices || n == 0 || n > ORX_GROUP_MAX) {
        g_create_error = "orx_create_group: 1 to 64 ranks, a device list and a result pointer";
        return ORX_ERR_INVALID_ARGUMENT;
    }
    orx_config c;
    if (cfg) c = *cfg;
    else orx_default_config(&c);
    orx_group_config gc;
    if (gcfg) gc = *gcfg;
    else orx_default_group_config(&gc);
    if (gc.partition > ORX_GROUP_ROWS || gc.comm > ORX_COMM_RCCL) {
        g_create_error = "orx_create_group: unknown partition or communicator";
        return ORX_ERR_INVALID_ARGUMENT;
    }
    bool one_device = true;
    for (uint32_t k = 0; k < n; k++) {
        if (hip_devices[k] < 0) {
            g_create_error = "orx_create_group: negative device index";
            return ORX_ERR_INVALID_ARGUMENT;
        }
        one_device = one_device && hip_devices[k] == hip_devices[0];
    }
    if (gc.comm == ORX_COMM_LOCAL && !one_device) {
        g_create_error = "the local communicator needs every rank on one device";
        return ORX_ERR_UNSUPPORTED;
    }
    if (gc.comm == ORX_COMM_RCCL && n > 1 && one_device) {
        g_create_error = "the RCCL communicator needs one device per rank";
        return ORX_ERR_UNSUPPORTED;
    }
    const bool rows = gc.partition == ORX_GROUP_ROWS;
    if (gc.photon_partition > ORX_PHOTONS_SLABS) {
        g_create_error = "orx_create_group: unknown photon partition";
        return ORX_ERR_INVALID_ARGUMENT;
    }
    if (gc.photon_partition == ORX_PHOTONS_SLABS && !rows) {
        g_create_error = "photon slabs partition one frame over the ranks: ORX_GROUP_ROWS only";
        return ORX_ERR_INVALID_ARGUMENT;
    }
    if (rows && n > 1 && (c.photon_map == 1 || c.enable_media)) {
        g_create_error = "the stochastic hash photon map and participating media are single-device";
        return ORX_ERR_UNSUPPORTED;
    }
    /* one slab means nothing to exchange: a one-rank group runs the rows path */
    const bool slabs = rows && n > 1 && gc.photon_partition == ORX_PHOTONS_SLABS;
    if (slabs && c.photon_map != 0) {
        g_create_error = "photon slabs need the uniform-grid photon map";
        return ORX_ERR_UNSUPPORTED;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        g_create_error = "no HIP device";
        return ORX_ERR_DEVICE;
    }
    for (uint32_t k = 0; k < n; k++)
        if (hip_devices[k] >= count) {
            g_create_error = "orx_create_group: device index past the device count";
            return ORX_ERR_INVALID_ARGUMENT;
        }
    orx_group* g = new (std::nothrow) orx_group();
    if (!g) return ORX_ERR_OUT_OF_MEMORY;
    g->n = n;
    g->cfg = c;
    g->gc = gc;
    g->slabs = slabs;
    g->rk.resize(n);
    for (uint32_t k = 0; k < n; k++) g->rk[k].device = hip_devices[k];
    const uint64_t clock_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                                  std::chrono::system_clock::now().time_since_epoch())
                                  .count();
    orx_status st = ORX_OK;
    const char* what = "";
    for (uint32_t k = 0; k < n && st == ORX_OK; k++) {
        GroupRank& q = g->rk[k];
        orx_config ck = c;
        if (!rows) ck.seed = orx_batch_seed(c.seed, k, clock_ns);
        what = "orx_create";
        if ((st = orx_create(q.device, &ck, &q.r)) != ORX_OK) break;
        q.main = (hipStream_t)orx_stream(q.r);
        what = "stream and event creation";
        if (hipSetDevice(q.device) != hipSuccess ||
            hipStreamCreateWithFlags(&q.comm, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&q.side, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&q.fin, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&q.ev_export, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&q.ev_gathered, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&q.ev_partial, hipEventDisableTiming) != hipSuccess) {
            st = ORX_ERR_DEVICE;
            break;
        }
        if (rows) {
            what = "orx_set_shard";
            if ((st = orx_set_shard(q.r, k, n)) != ORX_OK) break;
            if (slabs) {
                what = "orx_set_slab_partition";
                if ((st = orx_set_slab_partition(q.r, 1)) != ORX_OK) break;
            }
            if (gc.pipeline && c.photon_map != 1) {
                what = "orx_set_ppm_pipeline";
                if ((st = orx_set_ppm_pipeline(q.r, (void*)q.side, 1)) != ORX_OK) break;
            }
        }
    }
    g->pipe = rows && gc.pipeline && c.photon_map != 1;
    if (st == ORX_OK) {
        std::string e;
        what = "communicator";
        st = group_comm_create(gc.comm, n, hip_devices, one_device, &g->comm, e);
        if (st == ORX_OK && slabs) st = g->comm->prepare_all_to_all(e);
        if (st != ORX_OK) g_create_error = e;
    }
    if (st == ORX_OK && slabs) {
        /* the histogram buffers do not depend on the frame size; on a shared device rank 0's gathered
         * histograms serve everyone.  The record buffers are sized by each iteration's plan. */
        what = "slab histogram buffers";
        const size_t hb = orx_slab_histogram_words(ORX_GROUP_SLAB_BINS) * 4;
        hipError_t he = hipSuccess;
        for (uint32_t k = 0; k < n && he == hipSuccess; k++) {
            GroupRank& q = g->rk[k];
            he = q.hist.ensure(q.device, hb);
            if (he == hipSuccess && (!g->comm->shared_device() || k == 0)) he = q.hists.ensure(q.device, hb * n);
        }
        if (he == hipSuccess && (he = hipSetDevice(g->rk[0].device)) == hipSuccess)
            he = hipHostMalloc((void**)&g->h_hists, hb * n, hipHostMallocDefault);
        if (he != hipSuccess) {
            g->h_hists = nullptr;
            st = he == hipErrorOutOfMemory ? ORX_ERR_OUT_OF_MEMORY : ORX_ERR_DEVICE;
        }
    }
    if (st != ORX_OK) {
        if (g_create_error.empty()) g_create_error = std::string("orx_create_group: ") + what + " failed";
        group_free(g);
        return st;
    }
    *out = g;
    return ORX_OK;
}

orx_status orx_group_init_scene(orx_group* g, const orx_scene* scene) {
    if (!g || !scene) return ORX_ERR_INVALID_ARGUMENT;
    /* validated once, before any rank is touched (the ranks' configurations differ in the seed alone): a refused
     * scene leaves every rank on the scene it had */
    orx_renderer* r0 = g->rk[0].r;
    GRANK(g, 0, orx::scene_validate(scene, r0->cfg, r0->world, &r0->err));
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    g->scene_ready = false; /* a rank's failure leaves the ranks on different scenes: no scene until all hold it */
    for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, orx::init_scene_checked(g->rk[k].r, *scene));
    g->scene_ready = true;
    return ORX_OK;
}

orx_status orx_group_render_next_iteration(orx_group* g, uint64_t iteration_number, uint64_t local_iteration_number,
                                           float ppm_radius, int create_output, const orx_request* det) {
    if (!g || !det) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->scene_ready) return gerr(g, ORX_ERR_STATE, "Traced before OptixRenderer was initialized.");
    if (det->method != ORX_METHOD_PATH_TRACING && det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING &&
        det->method != ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING)
        return gerr(g, ORX_ERR_UNSUPPORTED, "render method not supported by this build");
    orx_status s = group_prepare(g, det);
    if (s != ORX_OK) return s;
    if (g->gc.partition == ORX_GROUP_BATCH) {
        /* global iteration i goes to rank i % n with the rank's own local count; local iteration 0
         * restarts the accumulation on every rank, as it does on one renderer */
        if (local_iteration_number == 0) {
            for (GroupRank& q : g->rk) q.local_it = 0;
            g->calls = 0;
        }
        const uint32_t k = (uint32_t)(iteration_number % g->n);
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_render_next_iteration(q.r, iteration_number, q.local_it, ppm_radius, create_output, det));
        q.local_it++;
        g->calls++;
        if (g->gc.reduce_every && g->calls % ((uint64_t)g->gc.reduce_every * g->n) == 0) return batch_reduce(g);
        return ORX_OK;
    }
    if (det->method == ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING)
        return g->pipe ? rows_ppm_pipelined(g, iteration_number, local_iteration_number, ppm_radius, det)
                       : rows_ppm_serial(g, iteration_number, local_iteration_number, ppm_radius, det);
    if (det->method == ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING)
        return rows_vcm(g, iteration_number, local_iteration_number, ppm_radius, det);
    for (uint32_t k = 0; k < g->n; k++) /* PT: own rows, no exchange */
        GRANK(g, k, orx_render_next_iteration(g->rk[k].r, iteration_number, local_iteration_number, ppm_radius,
                                              create_output, det));
    return ORX_OK;
}

/* the merged running sum into g->image on rank 0 (enqueued; the caller waits with group_sync) */
static orx_status group_image(orx_group* g) {
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    GroupRank& root = g->rk[0];
    if (g->gc.partition == ORX_GROUP_BATCH) return batch_reduce(g);
    const size_t blk = (size_t)g->max_rows * g->W * 12;
    for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, orx_get_output_device(g->rk[k].r, g->rk[k].out_local.p, blk));
    s = group_all_gather(
        g, main_stream, [](GroupRank& q) { return q.out_local.p; }, [](GroupRank& q) { return q.out_all.p; }, blk);
    if (s != ORX_OK) return s;
    GHIP(g, hipSetDevice(root.device));
    group_assemble_rows(root.main, root.out_all.f(), g->image.f(), g->W, g->H, g->n, g->max_rows);
    GHIP(g, hipGetLastError());
    return ORX_OK;
}

orx_status orx_group_get_output(orx_group* g, float* dst, size_t dst_bytes) {
    if (!g || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->W || !g->H) return gerr(g, ORX_ERR_STATE, "no frame rendered yet");
    const size_t need = (size_t)g->W * g->H * 12;
    if (dst_bytes < need) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    orx_status s = group_image(g);
    if (s != ORX_OK) return s;
    GroupRank& root = g->rk[0];
    if ((s = group_sync(g)) != ORX_OK) return s;
    GHIP(g, hipSetDevice(root.device));
    GHIP(g, hipMemcpy(dst, g->image.p, need, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, orx::check_grid(g->rk[k].r));
    return ORX_OK;
}

orx_status orx_group_get_display(orx_group* g, float inv_iterations, float inv_gamma, int32_t format, uint8_t* dst,
                                 size_t dst_bytes) {
    if (!g || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!orx::positive_finite(inv_iterations) || !orx::positive_finite(inv_gamma))
        return gerr(g, ORX_ERR_INVALID_ARGUMENT, "inv_iterations and inv_gamma must be finite and > 0");
    if (format != ORX_DISPLAY_RGBA8 && format != ORX_DISPLAY_BGRA8)
        return gerr(g, ORX_ERR_INVALID_ARGUMENT, "unknown display format");
    if (!g->W || !g->H) return gerr(g, ORX_ERR_STATE, "no frame rendered yet");
    const size_t npx = (size_t)g->W * g->H;
    if (dst_bytes < npx * 4) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    orx_status s = group_image(g);
    if (s != ORX_OK) return s;
    GroupRank& root = g->rk[0];
    if ((s = group_sync(g)) != ORX_OK) return s; /* BATCH reduces on every rank's stream */
    GHIP(g, g->display.ensure(root.device, npx * 4));
    GHIP(g, hipSetDevice(root.device));
    orx::launch_display(root.main, g->image.f(), npx, inv_iterations, inv_gamma, format == ORX_DISPLAY_BGRA8,
                        (uint32_t*)g->display.p);
    GHIP(g, hipGetLastError());
    GHIP(g, hipStreamSynchronize(root.main));
    GHIP(g, hipMemcpy(dst, g->display.p, npx * 4, hipMemcpyDeviceToHost));
    return ORX_OK;
}

orx_status orx_group_set_convergence(orx_group* g, int enable) {
    if (!g) return ORX_ERR_INVALID_ARGUMENT;
    if (g->gc.partition == ORX_GROUP_BATCH)
        return gerr(g, ORX_ERR_UNSUPPORTED, "convergence statistics need the ROWS partition (BATCH ranks hold windows of their own)");
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, orx_set_convergence(g->rk[k].r, enable));
    g->conv_on = enable != 0;
    if (!g->conv_on) {
        for (GroupRank& q : g->rk) {
            q.conv_local.release();
            q.conv_all.release();
        }
        g->conv_full.release();
        g->conv_tiles.release();
    }
    return ORX_OK;
}

orx_status orx_group_get_convergence(orx_group* g, float floor, float threshold, orx_convergence* out, float* tile_error,
                                     size_t tile_bytes) {
    if (!g || !out) return ORX_ERR_INVALID_ARGUMENT;
    if (!orx::positive_finite(floor)) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "floor must be finite and > 0");
    if (threshold != threshold) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "threshold is NaN");
    if (!g->conv_on) return gerr(g, ORX_ERR_STATE, "convergence statistics are off (orx_group_set_convergence)");
    if (!g->W || !g->H) return gerr(g, ORX_ERR_STATE, "no frame rendered yet");
    const uint32_t tx = (g->W + orx::CONV_TILE - 1) / orx::CONV_TILE, ty = (g->H + orx::CONV_TILE - 1) / orx::CONV_TILE;
    const size_t nt = (size_t)tx * ty;
    if (tile_error && tile_bytes < nt * 4) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "tile_error too small");
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    /* a rank's block: its error plane, then its mean-luminance plane, [max_rows][W] each */
    const size_t plane = (size_t)g->max_rows * g->W, blk = 2 * plane * 4, npx = (size_t)g->W * g->H;
    const bool shared = g->comm->shared_device();
    uint32_t n = 0;
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        GHIP(g, q.conv_local.ensure(q.device, blk));
        if (!shared || k == 0) GHIP(g, q.conv_all.ensure(q.device, blk * g->n));
    }
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        uint32_t nk = 0;
        GRANK(g, k, orx::conv_error_planes(q.r, floor, q.conv_local.f(), q.conv_local.f() + plane, &nk));
        if (k && nk != n) return gerr(g, ORX_ERR_STATE, "the ranks' statistics windows differ");
        n = nk;
    }
    s = group_all_gather(
        g, main_stream, [](GroupRank& q) { return q.conv_local.p; }, [](GroupRank& q) { return q.conv_all.p; }, blk);
    if (s != ORX_OK) return s;
    GroupRank& root = g->rk[0];
    GHIP(g, g->conv_full.ensure(root.device, 2 * npx * 4));
    GHIP(g, g->conv_tiles.ensure(root.device, nt * sizeof(orx::ConvTile)));
    GHIP(g, hipSetDevice(root.device));
    float* e = g->conv_full.f();
    float* m = e + npx;
    group_assemble_plane(root.main, root.conv_all.f(), e, g->W, g->H, g->n, g->max_rows, 2 * plane, 0);
    group_assemble_plane(root.main, root.conv_all.f(), m, g->W, g->H, g->n, g->max_rows, 2 * plane, plane);
    orx::launch_conv_tiles(root.main, e, m, g->W, g->H, threshold, (orx::ConvTile*)g->conv_tiles.p);
    GHIP(g, hipGetLastError());
    if ((s = group_sync(g)) != ORX_OK) return s;
    std::vector<orx::ConvTile> tiles(nt);
    GHIP(g, hipSetDevice(root.device));
    GHIP(g, hipMemcpy(tiles.data(), g->conv_tiles.p, nt * sizeof(orx::ConvTile), hipMemcpyDeviceToHost));
    orx::conv_finish_tiles(tiles.data(), tx, ty, n, out, tile_error);
    return ORX_OK;
}

uint32_t orx_group_world(const orx_group* g) { return g ? g->n : 0; }

orx_renderer* orx_group_renderer(orx_group* g, uint32_t rank) { return g && rank < g->n ? g->rk[rank].r : nullptr; }

int orx_group_pipelined(const orx_group* g) {
    return g && g->pipe && g->method == ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING && orx_ppm_pipelined(g->rk[0].r) ? 1 : 0;
}

const char* orx_group_comm_name(const orx_group* g) { return g && g->comm ? g->comm->name() : ""; }

/* a NULL group: the message of this thread's last failed orx_create_group */
const char* orx_group_last_error(const orx_group* g) { return g ? g->err.c_str() : g_create_error.c_str(); }

void orx_group_destroy(orx_group* g) {
    if (!g) return;
    group_drain(g);
    group_free(g);
}

/* host arrays through the communicator's sums, on the ranks' own streams; rows padded to 16 B */
static orx_status debug_collective(orx_group* g, const float* in, size_t per_rank, size_t block, float* out,
                                   bool scatter) {
    if (!g || !in || !out || per_rank == 0) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->comm->shared_device()) return gerr(g, ORX_ERR_UNSUPPORTED, "the debug collectives run on the local communicator");
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    const uint32_t n = g->n;
    const int dev = g->rk[0].device;
    const size_t in_stride = (per_rank + 3) / 4 * 4;
    const size_t out_rows = scatter ? n : 1, out_len = scatter ? block : per_rank, out_stride = (out_len + 3) / 4 * 4;
    GHIP(g, g->dbg_in.ensure(dev, in_stride * n * 4));
    GHIP(g, g->dbg_out.ensure(dev, out_stride * out_rows * 4));
    std::vector<const float*> send(n);
    std::vector<float*> recv(n);
    for (uint32_t k = 0; k < n; k++) {
        GHIP(g, hipMemcpy(g->dbg_in.f() + k * in_stride, in + k * per_rank, per_rank * 4, hipMemcpyHostToDevice));
        send[k] = g->dbg_in.f() + k * in_stride;
        recv[k] = g->dbg_out.f() + (scatter ? k * out_stride : 0);
    }
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    if (scatter) GCOMM(g, g->comm->reduce_scatter(send.data(), recv.data(), block, st.data(), e_));
    else GCOMM(g, g->comm->reduce(send.data(), recv[0], per_rank, st.data(), e_));
    if ((s = group_sync(g)) != ORX_OK) return s;
    for (size_t k = 0; k < out_rows; k++)
        GHIP(g, hipMemcpy(out + k * out_len, g->dbg_out.f() + k * out_stride, out_len * 4, hipMemcpyDeviceToHost));
    return ORX_OK;
}

orx_status orx_group_debug_reduce_scatter(orx_group* g, const float* in, size_t block_floats, float* out) {
    if (!g || block_floats == 0) return ORX_ERR_INVALID_ARGUMENT;
    return debug_collective(g, in, block_floats * g->n, block_floats, out, true);
}

orx_status orx_group_debug_reduce(orx_group* g, const float* in, size_t n_floats, float* out) {
    return debug_collective(g, in, n_floats, 0, out, false);
}

orx_status orx_group_slab_plan(const orx_group* g, uint32_t* axis, uint8_t* bin_dest, uint64_t* counts) {
    if (!g || !axis || !bin_dest || !counts) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->plan.have) return ORX_ERR_STATE; /* the group is const: no message is stored */
    *axis = g->plan.axis;
    std::memcpy(bin_dest, g->plan.bin_dest, ORX_GROUP_SLAB_BINS);
    std::memcpy(counts, g->plan.counts.data(), (size_t)g->n * g->n * sizeof(uint64_t));
    return ORX_OK;
}

/* host arrays through the communicator's all-to-all, on the ranks' own streams; each rank's buffer starts
 * on 16 B, the runs inside it wherever their 36-byte records put them */
orx_status orx_group_debug_all_to_all(orx_group* g, const float* in, const uint64_t* counts, float* out) {
    if (!g || !in || !counts || !out) return ORX_ERR_INVALID_ARGUMENT;
    if (!g->comm->shared_device()) return gerr(g, ORX_ERR_UNSUPPORTED, "the debug collectives run on the local communicator");
    orx_status s = group_quiesce(g);
    if (s != ORX_OK) return s;
    const uint32_t n = g->n;
    const int dev = g->rk[0].device;
    for (size_t i = 0; i < (size_t)n * n; i++)
        if (counts[i] > 0xffffffffull) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "run beyond 2^32 records");
    const orx::SlabRunLayout lay = orx::slab_run_layout(counts, n);
    std::vector<size_t> ns(n), nr(n), so(n + 1, 0), ro(n + 1, 0); /* floats; padded offsets */
    for (uint32_t k = 0; k < n; k++) {
        ns[k] = (size_t)lay.send_total[k] * ORX_RECORD_DWORDS;
        nr[k] = (size_t)lay.recv_total[k] * ORX_RECORD_DWORDS;
        so[k + 1] = so[k] + (ns[k] + 3) / 4 * 4;
        ro[k + 1] = ro[k] + (nr[k] + 3) / 4 * 4;
    }
    GHIP(g, g->dbg_in.ensure(dev, so[n] * 4));
    GHIP(g, g->dbg_out.ensure(dev, ro[n] * 4));
    std::vector<const float*> send(n);
    std::vector<float*> recv(n);
    size_t hi = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (ns[k]) GHIP(g, hipMemcpy(g->dbg_in.f() + so[k], in + hi, ns[k] * 4, hipMemcpyHostToDevice));
        hi += ns[k];
        send[k] = g->dbg_in.f() + so[k];
        recv[k] = g->dbg_out.f() + ro[k];
    }
    const std::vector<hipStream_t> st = streams_of(g, main_stream);
    GCOMM(g, g->comm->all_to_all_v(send.data(), recv.data(), counts, st.data(), e_));
    if ((s = group_sync(g)) != ORX_OK) return s;
    size_t ho = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (nr[k]) GHIP(g, hipMemcpy(out + ho, g->dbg_out.f() + ro[k], nr[k] * 4, hipMemcpyDeviceToHost));
        ho += nr[k];
    }
    return ORX_OK;
}

} /* extern "C" */
