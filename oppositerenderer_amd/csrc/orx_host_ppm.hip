/*
 * orx_host_ppm.hip — progressive photon mapping on the host: the pipelined buffer sets and the kernels'
 * views of them, the eye/photon/grid/gather and media helpers, the serial and the pipelined
 * single-device schedule, and the sharded phase API (orx_ppm_local_*, slabs, external gather, finish).
 */
#include "orx_host.h"

using namespace orx;

/* The kernels' views of the current buffer set (pp) and photon output set (po).  Every px / pb / kd
 * pointer into a PpmSet or PhotonOut is written here and nowhere else: after resize, after a rotation
 * (next_set) and after the output-set flip. */
void orx::bind_ppm_views(orx_renderer* r) {
    const uint32_t pm = r->cfg.photon_map;
    const PpmSet& s = r->pipe.set[r->pipe.pp];
    const PpmSet& g = r->pipe.set[pm == 0 ? r->pipe.pp : 0]; /* the uniform grid's buffers exist once under the other maps */
    const PhotonOut& o = r->gasync.out[r->gasync.po];
    const size_t nhp = (size_t)r->max_rows * r->W;
    r->px.hpA = s.hp.as<float4>();
    r->px.hpB = r->px.hpA + nhp;
    r->px.hpC = (float2*)(r->px.hpA + 2 * nhp);
    r->px.direct = s.dir.as<float>();
    PhotonBufs& pb = r->pb;
    pb.grid = s.grid.as<GridParams>();
    pb.sorted = g.sorted.as<float>();
    pb.subofs = g.subofs.as<uint32_t>(); /* null only while nothing has sized it */
    pb.offsets = g.offsets.as<uint32_t>();
    pb.slots = (pm == 1 ? s.hslots : o.slots).as<float4>(); /* the hash gather reads the deposit records */
    pb.vmask = o.vmask.as<uint8_t>();
    pb.pos4 = o.pos4.as<float4>();
    pb.bbox = o.bbox.as<uint32_t>();
    pb.hcount = s.hcount.as<uint32_t>(); /* the hash's table: null under the other maps */
    pb.hwin = s.hwin.as<uint32_t>();
    if (pm == 2) {
        r->kds.view.tree = s.kdtree.as<float4>();
        r->kds.view.tree_bc = r->kds.view.tree + r->kds.view.tree_size + 1;
    }
}

orx_status orx::size_ppm_set(orx_renderer* r, PpmSet& b, uint32_t k) {
    const FrameSizes& f = r->fs;
    const uint32_t pm = r->cfg.photon_map;
    HIPCHK(r, b.hp.ensure(f.nhp * 40));
    HIPCHK(r, hipMemsetAsync(b.hp.p, 0, f.nhp * 40, r->stream)); /* pad rows: flags 0 */
    HIPCHK(r, b.dir.ensure(f.nhp * 12));
    HIPCHK(r, b.grid.ensure(sizeof(GridParams)));
    HIPCHK(r, hipMemsetAsync(b.grid.p, 0, sizeof(GridParams), r->stream));
    if (k == 0 || pm == 0) {
        const size_t bytes = (size_t)SP_PLANES * f.splane * 4;
        HIPCHK(r, b.sorted.ensure(bytes));
        HIPCHK(r, hipMemsetAsync(b.sorted.p, 0, bytes, r->stream)); /* tail reads stay finite */
        HIPCHK(r, b.subofs.ensure(f.G2 * 4 * SUBX * f.nsub + 16));
        HIPCHK(r, b.offsets.ensure(f.G2 * 4));
        HIPCHK(r, hipMemsetAsync(b.offsets.p, 0, f.G2 * 4, r->stream));
    }
    if (pm == 1) {
        HIPCHK(r, b.hslots.ensure(f.S_cap * 64));
        HIPCHK(r, b.hcount.ensure(f.hnum * 4));
        HIPCHK(r, b.hwin.ensure(f.hnum * 4));
    } else if (pm == 2) {
        HIPCHK(r, b.kdtree.ensure(f.tree * 48 + 48));
        HIPCHK(r, hipMemsetAsync(b.kdtree.p, 0, f.tree * 48 + 48, r->stream));
    }
    return ORX_OK;
}
orx_status orx::size_photon_out(orx_renderer* r, PhotonOut& o) {
    const FrameSizes& f = r->fs;
    if (r->cfg.photon_map != 1) HIPCHK(r, o.slots.ensure(f.S_cap * 64)); /* the hash's records: PpmSet::hslots */
    HIPCHK(r, o.vmask.ensure(f.S_cap / f.D + 1));
    HIPCHK(r, hipMemsetAsync(o.vmask.p, 0, f.S_cap / f.D + 1, r->stream));
    HIPCHK(r, o.pos4.ensure(f.S_cap * 16 + 16));
    HIPCHK(r, o.bbox.ensure(6 * BBOX_REPLICAS * 4));
    HIPCHK(r, hipMemsetAsync(o.bbox.p, 0xff, 3 * BBOX_REPLICAS * 4, r->stream));
    HIPCHK(r, hipMemsetAsync(o.bbox.as<uint32_t>() + 3 * BBOX_REPLICAS, 0, 3 * BBOX_REPLICAS * 4, r->stream));
    return ORX_OK;
}
orx_status orx::kd_resize(orx_renderer* r) {
    const FrameSizes& f = r->fs;
    const size_t S = f.S, tree = f.tree, nblk = f.nblk, ntiles = f.ntiles;
    HIPCHK(r, r->kds.ids.ensure(6 * S * 4 + 64));
    HIPCHK(r, r->kds.keys.ensure(2 * S * 4 + 64));
    HIPCHK(r, r->kds.nodepos.ensure(S * 4 + 16));
    HIPCHK(r, r->kds.lst.ensure(6 * S * 16 + 64));
    HIPCHK(r, r->kds.nkey.ensure(tree * 8 + 16));
    HIPCHK(r, r->kds.seg.ensure(tree * 8 + 16));
    HIPCHK(r, r->kds.box.ensure(tree * 24 + 24));
    HIPCHK(r, r->kds.ninfo.ensure(tree * 4 + 16));
    HIPCHK(r, r->kds.P.ensure(tree * 12 + 64));
    HIPCHK(r, r->kds.ppart.ensure(6 * nblk * 4 + 64));
    HIPCHK(r, r->kds.table.ensure(256 * ntiles * 4 + 64));
    HIPCHK(r, r->kds.tpart.ensure(f.tp * 4));
    HIPCHK(r, r->kds.vpart.ensure(nblk * 4 + 64));
    HIPCHK(r, r->kds.count.ensure(64));
    KdBufs& kd = r->kds.view;
    kd.S = (uint32_t)S;
    kd.tree_size = (uint32_t)tree;
    kd.levels = f.levels;
    kd.ntiles = (uint32_t)ntiles;
    for (int q = 0; q < 2; q++)
        for (int a = 0; a < 3; a++) {
            kd.ids[q][a] = r->kds.ids.as<uint32_t>() + (size_t)(3 * q + a) * S;
            kd.lst[q][a] = r->kds.lst.as<float4>() + (size_t)(3 * q + a) * S;
        }
    kd.keys[0] = r->kds.keys.as<uint32_t>();
    kd.keys[1] = kd.keys[0] + S;
    kd.nodepos = r->kds.nodepos.as<uint32_t>();
    kd.nkey = r->kds.nkey.as<uint2>();
    kd.seg = r->kds.seg.as<uint2>();
    kd.box = r->kds.box.as<float>();
    kd.ninfo = r->kds.ninfo.as<uint32_t>();
    kd.nodeP = r->kds.P.as<uint32_t>();
    kd.ppart = r->kds.ppart.as<uint32_t>();
    kd.table = r->kds.table.as<uint32_t>();
    kd.tpart = r->kds.tpart.as<uint32_t>();
    kd.vpart = r->kds.vpart.as<uint32_t>();
    kd.count = r->kds.count.as<uint32_t>();
    HIPCHK(r, hipMemsetAsync(r->kds.count.p, 0, 64, r->stream));
    return ORX_OK;
}

/* The further buffer sets of PPM pipelining, allocated on the first pipelined iteration after a
 * resize, so PT/VCM-only renderers and the serial schedule never hold them.  One device takes three
 * sets (ORX_PIPE_SETS=2: two): with two, the eye pass of iteration i + 1 waited for the gather and
 * output of i - 1, which on the hall ran until the grid build of i had ended, and the photon pass of
 * i + 1 then waited ~1 ms per frame for that eye pass (seen in a kernel trace); the sharded
 * pipeline keeps two (its finish may be held back one iteration, orx_ppm_finish_on). */
orx_status orx::ensure_second_set(orx_renderer* r) {
    if (r->pipe.bufs) return ORX_OK;
    static const uint32_t sets_env = [] {
        const char* e = getenv("ORX_PIPE_SETS");
        return e && atoi(e) == 2 ? 2u : 3u;
    }();
    r->pipe.nsets = r->fin.shard_pipe ? 2u : sets_env;
    for (uint32_t k = 1; k < r->pipe.nsets; k++) {
        const orx_status s0 = size_ppm_set(r, r->pipe.set[k], k);
        if (s0 != ORX_OK) return s0;
    }
    /* The asynchronous grid build (ORX_GRID_ASYNC=1) pays where the chain eye -> photon -> grid -> next
     * photon sets the frame (hall: 1059 -> 1071 Mpaths/s); where the gather does it only reorders a
     * throughput-bound frame and costs 1-2 % (Cornell 2056 -> 2012, conference 4K 585 -> 578;
     * profiles/r06p_grid_async_ab.txt), so it is off by default. */
    static const int async_env = [] {
        const char* e = getenv("ORX_GRID_ASYNC");
        return e ? atoi(e) : -1;
    }();
    const bool eligible = r->pipe.nsets == 3 && r->cfg.photon_map == 0 && !r->media.on;
    r->gasync.on = eligible && async_env > 0;
    r->gasync.probe_stage = eligible && async_env < 0 ? 1u : 0u;
    r->gasync.probe_ms[0] = r->gasync.probe_ms[1] = 0.f;
    r->gasync.out_b = eligible && async_env != 0;
    if (r->gasync.out_b) { /* the photon pass's second output set (the first is resize's) */
        const orx_status s0 = size_photon_out(r, r->gasync.out[1]);
        if (s0 != ORX_OK) return s0;
        /* both sets' last-reader events exist from here on, so a wait on either is valid */
        HIPCHK(r, hipEventRecord(r->gasync.ev_gsrc[0], r->stream));
        HIPCHK(r, hipEventRecord(r->gasync.ev_gsrc[1], r->stream));
        for (hipEvent_t& e : r->gasync.ev_pm)
            if (!e) HIPCHK(r, hipEventCreate(&e));
    }
    /* the zero-fills above ran on the own stream; on a caller stream (the sharded pipeline) the
     * eye pass and grid build of this iteration write these buffers right after the rotation */
    if (r->use_ext) HIPCHK(r, hipStreamSynchronize(r->stream));
    r->pipe.bufs = true;
    return ORX_OK;
}
/* the next iteration's buffer set: with two sets the other one, with three the least recently used */
static void next_set(orx_renderer* r) {
    r->pipe.pp = (r->pipe.pp + r->pipe.nsets - 1) % r->pipe.nsets;
    bind_ppm_views(r);
}

/* The volumetric table's grid for radius R (host): the box padded by 2R, cells >= 1.01 R and at
 * least the cube root of (volume / table slots), at most 1024 per axis (orx_media_dev.h VolMap) */
static void vol_grid(orx_renderer* r, float R) {
    VolMap& vm = r->media.vm;
    vm.R = R;
    const f3 pad = mk1(2.f * R);
    vm.glo = vm.lo - pad;
    const f3 ext = (vm.hi + pad) - vm.glo;
    double cell = std::max((double)R * 1.01, std::cbrt((double)ext.x * ext.y * ext.z / (double)r->cfg.volumetric_photons));
    cell = std::max(cell, (double)std::max(ext.x, std::max(ext.y, ext.z)) / 1024.0);
    vm.cell = (float)cell * 1.0001f;
    const float e[3] = {ext.x, ext.y, ext.z};
    for (int k = 0; k < 3; k++) vm.n[k] = std::min(1024u, std::max(1u, (uint32_t)std::ceil(e[k] / vm.cell)));
    vm.G = vm.n[0] * vm.n[1] * vm.n[2];
    vm.ilo = vm.lo - mk1(R);
    vm.ihi = vm.hi + mk1(R);
}
static MediaBufs media_bufs(orx_renderer* r) {
    MediaBufs mb;
    mb.vm = r->media.vm;
    mb.vm.start = r->media.start.as<uint32_t>();
    mb.vm.rec = r->media.rec.as<float4>();
    mb.volR = r->media.volR.as<float>();
    mb.ev_a = r->media.ev_a.as<float4>();
    mb.ev_b = r->media.ev_b.as<float4>();
    return mb;
}
/* after the photon pass: this pass's volumetric table, gathered by the next eye pass with this
 * iteration's radius (volumetricRadius = PPMRadius after the eye pass, OptixRenderer.cpp:592-593) */
static orx_status vol_build(orx_renderer* r, hipStream_t st, float R) {
    vol_grid(r, R);
    HIPCHK(r, r->media.start.ensure(((size_t)r->media.vm.G + 2) * 4));
    VolBuild vb;
    vb.ev_a = r->media.ev_a.as<float4>();
    vb.ev_b = r->media.ev_b.as<float4>();
    vb.nphot = r->prows * r->cfg.photon_launch_width;
    vb.D = r->cfg.max_photon_deposits;
    vb.NV = r->cfg.volumetric_photons;
    vb.vcnt = r->media.cnt.as<uint32_t>();
    vb.vwin = r->media.win.as<uint32_t>();
    vb.vA = r->media.A.as<float4>();
    vb.vB = r->media.B.as<float4>();
    vb.keys = r->media.keys.as<uint32_t>();
    vb.vals = r->media.vals.as<uint32_t>();
    vb.keys_sorted = r->media.keys2.as<uint32_t>();
    vb.vals_sorted = r->media.vals2.as<uint32_t>();
    vb.sort_tmp = r->media.sort.p;
    vb.sort_tmp_bytes = vol_sort_tmp_bytes(vb.NV);
    vb.start = r->media.start.as<uint32_t>();
    vb.rec = r->media.rec.as<float4>();
    launch_vol_build(st, vb, r->media.vm);
    r->media.vm.valid = 1;
    return ORX_OK;
}

/* The gather's tile order (GatherIn.order) for an image of `px` pixels: super-tiles of 8 x 8 tiles
 * (128 x 128 pixels) from 4M pixels up, image bands per XCD below.  At configs[4] the super-tiles
 * halve the union gather's fetches from beyond L2 (2 x FETCH_SIZE 22.3 -> 11.8 GB per launch;
 * 16 x 16: 10.4 GB) and the frame gains 2.8 % (serial gather 24.1 -> 23.1 ms); on the 1080p hall
 * the serial gather gains too (1.37 -> 1.21 ms) but the pipelined frame, where the gather overlaps
 * the next iteration's passes, does not (977 / 971 Mpaths/s, two runs each;
 * profiles/r04b_gather_order_ab.txt).  ORX_GATHER_ORDER=S forces S (0: bands). */
static uint32_t gather_order(size_t px) {
    static const int o = [] {
        const char* e = getenv("ORX_GATHER_ORDER");
        return e ? std::max(0, std::min(64, atoi(e))) : -1;
    }();
    return o >= 0 ? (uint32_t)o : (px >= (4u << 20) ? 8u : 0u);
}

static GatherIn local_gather_in(orx_renderer* r) {
    GatherIn gi;
    gi.base = (const uint8_t*)r->px.hpA;
    gi.seg_bytes = (size_t)r->max_rows * r->W * 40;
    gi.segments = 1;
    gi.seg_rows = r->max_rows;
    gi.W = r->W;
    gi.indirect = r->d_ind.as<float>();
    gi.dbg = r->cfg.debug_counters ? r->d_dbg.as<uint32_t>() : nullptr;
    gi.cull = 0;
    gi.visits = 1;
    gi.order = gather_order((size_t)r->W * r->H);
    return gi;
}

static void ppm_eye(orx_renderer* r, const DevCamera& cam, const Consts& c) {
    ev_begin(r, P_EYE);
    if (r->media.on) {
        const MediaBufs mb = media_bufs(r);
        launch_ppm_eye(cur_stream(r), r->scene, cam, r->px, c, &mb);
    } else {
        launch_ppm_eye(cur_stream(r), r->scene, cam, r->px, c);
    }
    ev_end(r, P_EYE);
}
/* initializeStochasticHashPhotonMap (OptixRenderer_SpatialHash.cu:286-302): the scene AABB padded
 * by r + 0.0001 (AAB::addPadding, the sum in double as written), cell = r, grid = max(1, ceil(extent/r))
 * with OptiX's float3/float (multiplication by the reciprocal, calculateGridSize :42-50) */
static HashParams hash_params(const orx_renderer* r, float ppm_radius) {
    const float a = (float)((double)ppm_radius + 0.0001);
    const f3 lo = r->aabb_lo - mk1(a), hi = r->aabb_hi + mk1(a);
    const f3 f = (hi - lo) * (1.0f / ppm_radius);
    HashParams hp;
    hp.ox = lo.x;
    hp.oy = lo.y;
    hp.oz = lo.z;
    hp.cell = ppm_radius;
    hp.gx = std::max(1u, orx_f2u_sat(orx_ceilf(f.x)));
    hp.gy = std::max(1u, orx_f2u_sat(orx_ceilf(f.y)));
    hp.gz = std::max(1u, orx_f2u_sat(orx_ceilf(f.z)));
    hp.mask = r->pb.hnum - 1u;
    return hp;
}
static void ppm_grid_build(orx_renderer* r, const PhotonBufs& pb, const GridBox& gb = GridBox{}, hipStream_t on = nullptr);
/* photon pass (+ the overlapped direct pass), then the photon map (build_map: false in slab
 * mode, whose grid is built over the imported photons by orx_ppm_slab_import) */
static orx_status ppm_photons_grid(orx_renderer* r, const Consts& c, bool build_map = true) {
    hipStream_t st = cur_stream(r);
    ev_begin(r, P_PHOTON);
    r->pipe.eye_chain = false;
    MediaBufs mb{};
    if (r->media.on) mb = media_bufs(r);
    if (!launch_ppm_photon(st, r->scene, r->px, r->pb, c, r->media.on ? &mb : nullptr)) {
        ev_end(r, P_PHOTON);
        return set_err(r, ORX_ERR_STATE, "photon pass larger than its traversal-stack buffer (photon_stack_ensure)");
    }
    if (r->media.on) vol_build(r, st, c.ppm_radius);
    ev_end(r, P_PHOTON);
    if (r->pipe.overlap_direct) {
        /* the direct pass needs the hitpoints and the RNG states the photon pass
         * left (slot (x,y) is shared, Appendix A.2); nothing after it reads
         * either until the output pass, so it runs beside the grid build and
         * the gather */
        hipEventRecord(r->pipe.ev_photon_done, st);
        hipStreamWaitEvent(r->aux, r->pipe.ev_photon_done, 0);
        ev_begin(r, P_DIRECT, r->aux);
        launch_ppm_direct_output(r->aux, r->scene, r->px, c, 1);
        ev_end(r, P_DIRECT, r->aux);
        hipEventRecord(r->pipe.ev_direct_done, r->aux);
    }
    if (!build_map) return ORX_OK;
    if (r->pb.hash) {
        ev_begin(r, P_SETUP_HASH);
        launch_hash_build(st, r->pb, hash_params(r, c.ppm_radius));
        ev_end(r, P_SETUP_HASH);
        return ORX_OK;
    }
    if (r->cfg.photon_map == 2) { /* createPhotonKdTreeOnCPU, on the device */
        ev_begin(r, P_SETUP_HASH);
        launch_kd_build(st, r->pb, r->kds.view);
        ev_end(r, P_SETUP_HASH);
        return ORX_OK;
    }
    ppm_grid_build(r, r->pb);
    return ORX_OK;
}
/* grid build: the atomic-free bucket sort (an atomic-rank counting sort measured slower:
 * one device-scope atomic per photon into a 4 MB histogram); on `on`, or the
 * renderer's stream */
static void ppm_grid_build(orx_renderer* r, const PhotonBufs& pb, const GridBox& gb, hipStream_t on) {
    hipStream_t st = on ? on : cur_stream(r);
    ev_begin(r, P_SETUP_HASH, st);
    launch_grid_setup(st, pb, gb);
    launch_grid_bucket_count(st, pb);
    ev_end(r, P_SETUP_HASH, st);
    ev_begin(r, P_SCAN, st);
    launch_grid_bucket_scan(st, pb);
    ev_end(r, P_SCAN, st);
    ev_begin(r, P_SCATTER, st);
    launch_grid_bucket_place(st, pb);
    ev_end(r, P_SCATTER, st);
}
/* the gather over the renderer's photon map: kd-tree, stochastic hash or uniform grid */
static void ppm_gather(orx_renderer* r, hipStream_t st, const GatherIn& gi, const Consts& c) {
    if (r->cfg.photon_map == 2) launch_ppm_gather_kd(st, gi, r->pb, r->kds.view, c);
    else if (r->pb.hash) launch_ppm_gather_hash(st, gi, r->pb, hash_params(r, c.ppm_radius), c);
    else launch_ppm_gather(st, gi, r->pb, c);
}
static orx_status ppm_local_passes(orx_renderer* r, const DevCamera& cam, const Consts& c) {
    ppm_eye(r, cam, c);
    return ppm_photons_grid(r, c);
}

/* One PPM iteration pass after pass on the current stream (orx_render_next_iteration without
 * pipelining): the direct pass on the aux stream beside the grid build and the gather; the output
 * accumulation after both */
orx_status orx::ppm_serial_iteration(orx_renderer* r, const DevCamera& cam, const Consts& c) {
    hipStream_t st = cur_stream(r);
    r->pipe.overlap_direct = true;
    const orx_status sp = ppm_local_passes(r, cam, c);
    r->pipe.overlap_direct = false;
    if (sp != ORX_OK) return sp;
    ev_begin(r, P_GATHER);
    ppm_gather(r, st, local_gather_in(r), c);
    if (r->media.on) launch_vol_indirect(st, r->px, r->media.volR.as<float>(), c.emitted_f);
    ev_end(r, P_GATHER);
    ev_begin(r, P_DIRECT);
    HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_direct_done, 0));
    launch_ppm_direct_output(st, r->scene, r->px, c, 2);
    ev_end(r, P_DIRECT);
    return ORX_OK;
}

/* the asynchronous grid build when the measured photon pass + grid build exceed this multiple of the gather.
 * Measured on the first pipelined iteration (its radius is the largest, so its gather the dearest): hall
 * 5.59 / 3.44 ms = 1.62 (the asynchronous build gains 1.2-1.8 % there), Cornell 0.79 / 0.98 = 0.81 and
 * conference 4K 19.2 / 51.0 = 0.38 (it loses 1-2 %); the threshold sits at their geometric middle
 * (profiles/r06p_grid_async_ab.txt, r06zh_grid_schedule_choice.txt) */
constexpr float GRID_CHAIN_RATIO = 1.15f;

/* One PPM iteration whose gather and output are left running on gstream, overlapping the next
 * iteration's eye, photon and grid passes (orx_render_next_iteration, single device).  Every
 * kernel and its inputs are those of the serial schedule; only the buffer set alternates. */
orx_status orx::ppm_pipelined_iteration(orx_renderer* r, const orx_request* det, float ppm_radius,
                                        uint64_t local_iteration_number) {
    const DevCamera cam = camera_setup(det->camera);
    const Consts c = make_consts(r, ppm_radius, local_iteration_number);
    hipStream_t st = r->stream;
    next_set(r);
    const uint32_t k = r->pipe.pp;
    const bool measure = r->gasync.probe_stage == 1;
    if (r->gasync.probe_stage == 2) { /* after the measured iteration: this photon pass waits for its gather */
        HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_gdone[r->gasync.probe_k], 0));
        r->gasync.probe_stage = 3;
    } else if (r->gasync.probe_stage == 3) { /* the device still holds the previous iteration: no bubble */
        HIPCHK(r, hipEventSynchronize(r->gasync.ev_pm[3]));
        HIPCHK(r, hipEventElapsedTime(&r->gasync.probe_ms[0], r->gasync.ev_pm[0], r->gasync.ev_pm[1]));
        HIPCHK(r, hipEventElapsedTime(&r->gasync.probe_ms[1], r->gasync.ev_pm[2], r->gasync.ev_pm[3]));
        r->gasync.on = r->gasync.probe_ms[0] > GRID_CHAIN_RATIO * r->gasync.probe_ms[1];
        r->gasync.probe_stage = 0;
    }
    /* asynchronous build: the photon pass writes the other output set, whose last reader is the grid build
     * two iterations back; synchronous after asynchronous iterations: the current set, last read by the
     * previous iteration's build on gridq (else an event long complete) */
    if (r->gasync.on) {
        r->gasync.po ^= 1u;
        bind_ppm_views(r);
    }
    if (r->gasync.out_b) HIPCHK(r, hipStreamWaitEvent(st, r->gasync.ev_gsrc[r->gasync.po], 0));
    /* the set's previous gather + output (two iterations back) and, through the RNG chain
     * (slot (x,y) is advanced by eye, photon and direct in turn), the last direct pass */
    HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_gdone[k], 0));
    HIPCHK(r, hipStreamWaitEvent(r->aux, r->pipe.ev_gdone[k], 0)); /* eye and direct write this set */
    /* The eye pass needs the RNG slots after the direct pass of i (aux, stream order) and this
     * set free (above); not the grid build of i, which is still running on st.  So it runs on
     * aux beside that grid build, and the photon pass waits for it (RNG chain) and, in stream
     * order, for the grid build (the deposit records it reads).  Without an unbroken chain of
     * pipelined iterations aux first waits for everything enqueued on st. */
    if (!r->pipe.eye_chain) {
        HIPCHK(r, hipEventRecord(r->pipe.ev_main, st));
        HIPCHK(r, hipStreamWaitEvent(r->aux, r->pipe.ev_main, 0));
    }
    ev_begin(r, P_EYE, r->aux);
    launch_ppm_eye(r->aux, r->scene, cam, r->px, c);
    ev_end(r, P_EYE, r->aux);
    HIPCHK(r, hipEventRecord(r->pipe.ev_eye_done, r->aux));
    HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_eye_done, 0));
    r->pipe.overlap_direct = true;
    if (measure) HIPCHK(r, hipEventRecord(r->gasync.ev_pm[0], st));
    const orx_status sp = ppm_photons_grid(r, c, !r->gasync.on); /* photon, direct (aux), grid */
    if (measure) HIPCHK(r, hipEventRecord(r->gasync.ev_pm[1], st));
    r->pipe.overlap_direct = false;
    if (sp != ORX_OK) return sp;
    if (r->gasync.on) {
        /* the grid build on its own stream: the photon pass of i + 1 waits only for the RNG chain (eye of i + 1
         * after the direct pass of i) and for this build's end of reading the output set two iterations on */
        HIPCHK(r, hipStreamWaitEvent(r->gridq, r->pipe.ev_photon_done, 0));
        ppm_grid_build(r, r->pb, GridBox{}, r->gridq);
        HIPCHK(r, hipEventRecord(r->gasync.ev_gsrc[r->gasync.po], r->gridq));
        HIPCHK(r, hipEventRecord(r->pipe.ev_grid_done, r->gridq));
    } else {
        HIPCHK(r, hipEventRecord(r->pipe.ev_grid_done, st));
    }
    hipStream_t g = r->gstream;
    HIPCHK(r, hipStreamWaitEvent(g, r->pipe.ev_grid_done, 0));
    ev_begin(r, P_GATHER, g);
    if (measure) HIPCHK(r, hipEventRecord(r->gasync.ev_pm[2], g));
    ppm_gather(r, g, local_gather_in(r), c);
    if (measure) {
        HIPCHK(r, hipEventRecord(r->gasync.ev_pm[3], g));
        r->gasync.probe_stage = 2;
        r->gasync.probe_k = k;
    }
    ev_end(r, P_GATHER, g);
    HIPCHK(r, hipStreamWaitEvent(g, r->pipe.ev_direct_done, 0));
    ev_begin(r, P_DIRECT, g);
    launch_ppm_direct_output(g, r->scene, r->px, c, 2);
    ev_end(r, P_DIRECT, g);
    conv_update(r, g, r->conv.it);
    HIPCHK(r, hipEventRecord(r->pipe.ev_gdone[k], g));
    r->pipe.gather_in_flight = true;
    r->pipe.eye_chain = true;
    HIPCHK(r, hipGetLastError());
    r->last_method = (uint64_t)det->method;
    r->last_consts = c;
    return ORX_OK;
}

extern "C" {

orx_status orx_ppm_local_passes(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                                float ppm_radius, const orx_request* det) {
    if (!r || !det) return ORX_ERR_INVALID_ARGUMENT;
    if (r->media.on) return set_err(r, ORX_ERR_UNSUPPORTED, "participating media run through orx_render_next_iteration");
    if (det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "orx_ppm_local_passes needs a PPM request");
    r->pipe.last_pipelined = false;
    orx_status s0 = begin_iteration(r, local_iteration_number, det);
    if (s0 != ORX_OK) return s0;
    DevCamera cam = camera_setup(det->camera);
    Consts c = make_consts(r, ppm_radius, local_iteration_number);
    const orx_status sp = ppm_local_passes(r, cam, c);
    if (sp != ORX_OK) return sp;
    HIPCHK(r, hipGetLastError());
    r->last_method = (uint64_t)det->method;
    r->last_consts = c;
    note_iteration(r, iteration_number, local_iteration_number, ppm_radius, det->method);
    return ORX_OK;
}

orx_status orx_ppm_local_eye(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                             float ppm_radius, const orx_request* det) {
    if (!r || !det) return ORX_ERR_INVALID_ARGUMENT;
    if (r->media.on) return set_err(r, ORX_ERR_UNSUPPORTED, "participating media run through orx_render_next_iteration");
    if (det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "orx_ppm_local_eye needs a PPM request");
    orx_status s0 = begin_iteration(r, local_iteration_number, det, r->fin.shard_pipe);
    if (s0 != ORX_OK) return s0;
    if (r->fin.shard_pipe && (s0 = ensure_second_set(r)) != ORX_OK) return s0;
    DevCamera cam = camera_setup(det->camera);
    Consts c = make_consts(r, ppm_radius, local_iteration_number);
    r->pipe.last_pipelined = r->fin.shard_pipe && r->pipe.bufs;
    if (r->pipe.last_pipelined) {
        if (r->fin.due) { /* the previous iteration's finish comes later: hold its set */
            if (r->fin.snap) return set_err(r, ORX_ERR_STATE, "two sharded PPM finishes outstanding");
            r->fin.px = r->px;
            r->fin.consts = r->last_consts;
            r->fin.pp = r->pipe.pp;
            r->fin.conv = r->conv.last;
            r->fin.snap = true;
        }
        r->fin.due = true;
        /* the other buffer set; its last gather + finish (two iterations back) and, through the
         * RNG chain, the last direct pass precede this eye pass */
        next_set(r);
        HIPCHK(r, hipStreamWaitEvent(cur_stream(r), r->pipe.ev_gdone[r->pipe.pp], 0));
        HIPCHK(r, hipStreamWaitEvent(cur_stream(r), r->pipe.ev_direct_done, 0));
        HIPCHK(r, hipStreamWaitEvent(r->aux, r->pipe.ev_gdone[r->pipe.pp], 0));
    } else if (r->fin.shard_pipe) {
        flush_pipeline(r);
    }
    ppm_eye(r, cam, c);
    HIPCHK(r, hipGetLastError());
    r->last_method = (uint64_t)det->method;
    r->last_consts = c;
    note_iteration(r, iteration_number, local_iteration_number, ppm_radius, det->method);
    return ORX_OK;
}

orx_status orx_ppm_local_photons(orx_renderer* r) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->rng_ready) return set_err(r, ORX_ERR_STATE, "orx_ppm_local_eye first");
    HIPCHK(r, hipSetDevice(r->device));
    r->pipe.overlap_direct = r->pipe.last_pipelined; /* direct pass on the aux stream right after the photons */
    const orx_status sp = ppm_photons_grid(r, r->last_consts);
    r->pipe.overlap_direct = false;
    if (sp != ORX_OK) return sp;
    if (r->pipe.last_pipelined) HIPCHK(r, hipEventRecord(r->pipe.ev_grid_done, cur_stream(r)));
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_set_slab_partition(orx_renderer* r, int enable) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (enable && r->cfg.photon_map != 0)
        return set_err(r, ORX_ERR_UNSUPPORTED, "the slab partition needs the uniform-grid photon map");
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    r->slab.on = enable != 0;
    r->rng_ready = false; /* re-allocate the photon buffers for the imported photons */
    return ORX_OK;
}

orx_status orx_ppm_local_trace(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                               float ppm_radius, const orx_request* det) {
    if (!r || !det) return ORX_ERR_INVALID_ARGUMENT;
    if (r->media.on) return set_err(r, ORX_ERR_UNSUPPORTED, "participating media run through orx_render_next_iteration");
    if (det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "orx_ppm_local_trace needs a PPM request");
    if (!r->slab.on) return set_err(r, ORX_ERR_STATE, "orx_ppm_local_trace is the slab mode's first phase");
    r->pipe.last_pipelined = false;
    orx_status s0 = begin_iteration(r, local_iteration_number, det);
    if (s0 != ORX_OK) return s0;
    DevCamera cam = camera_setup(det->camera);
    Consts c = make_consts(r, ppm_radius, local_iteration_number);
    ppm_eye(r, cam, c);
    const orx_status sp = ppm_photons_grid(r, c, false);
    if (sp != ORX_OK) return sp;
    HIPCHK(r, hipGetLastError());
    r->last_method = (uint64_t)det->method;
    r->last_consts = c;
    note_iteration(r, iteration_number, local_iteration_number, ppm_radius, det->method);
    return ORX_OK;
}

orx_status orx_ppm_local_photon_trace(orx_renderer* r) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->rng_ready) return set_err(r, ORX_ERR_STATE, "orx_ppm_local_eye first");
    if (!r->slab.on) return set_err(r, ORX_ERR_STATE, "orx_ppm_local_photon_trace is a slab-mode phase");
    HIPCHK(r, hipSetDevice(r->device));
    r->pipe.overlap_direct = r->pipe.last_pipelined; /* direct pass on the aux stream right after the photons */
    const orx_status sp = ppm_photons_grid(r, r->last_consts, false);
    r->pipe.overlap_direct = false;
    if (sp != ORX_OK) return sp;
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

static_assert(SLAB_VOX == ORX_SLAB_VOXELS, "slab voxel grid: kernels and ABI disagree");
size_t orx_slab_histogram_words(uint32_t nb) {
    return (size_t)6 * nb + 6 + (size_t)2 * ORX_SLAB_VOXELS * ORX_SLAB_VOXELS * ORX_SLAB_VOXELS;
}
static SlabBins slab_bins(const orx_renderer* r, uint32_t nb) {
    SlabBins sb;
    const float lo[3] = {r->aabb_lo.x, r->aabb_lo.y, r->aabb_lo.z}, hi[3] = {r->aabb_hi.x, r->aabb_hi.y, r->aabb_hi.z};
    for (int a = 0; a < 3; a++) {
        const float ext = hi[a] - lo[a];
        sb.lo[a] = lo[a];
        sb.inv[a] = ext > 0.f ? (float)nb / ext : 0.f;
    }
    sb.nb = nb;
    return sb;
}

uint32_t orx_ppm_slab_halo(const orx_renderer* r, uint32_t nb, uint32_t axis, float radius) {
    if (!r || axis > 2 || nb == 0) return 2u;
    const SlabBins sb = slab_bins(r, nb);
    const float h = orx_floorf(radius * sb.inv[axis]);
    return (h >= 0.f && h < 1e6f ? (uint32_t)h : 0u) + 2u;
}
orx_status orx_ppm_slab_histogram(orx_renderer* r, uint32_t* hist, uint32_t nb) {
    if (!r || !hist || nb < ORX_SLAB_VOXELS || nb > 1024 || nb % ORX_SLAB_VOXELS) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->slab.on || !r->rng_ready) return set_err(r, ORX_ERR_STATE, "orx_ppm_slab_histogram: slab mode, after the photon pass");
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t st = cur_stream(r);
    HIPCHK(r, hipMemsetAsync(hist, 0, orx_slab_histogram_words(nb) * 4, st));
    launch_slab_hist(st, r->pb, r->px, slab_bins(r, nb), slab_bins(r, ORX_SLAB_VOXELS), hist);
    launch_slab_bbox(st, r->pb, hist + 6 * (size_t)nb);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_ppm_slab_pack(orx_renderer* r, const uint8_t* bin_dest, uint32_t nb, uint32_t axis, uint32_t halo_bins,
                             const uint32_t* dest_base, uint64_t send_records, void* send) {
    if (!r || !bin_dest || !dest_base || !send || nb == 0 || nb > 1024 || axis > 2) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->slab.on || !r->rng_ready) return set_err(r, ORX_ERR_STATE, "orx_ppm_slab_pack: slab mode, after the photon pass");
    if (r->world > 64) return set_err(r, ORX_ERR_UNSUPPORTED, "slab mode supports at most 64 ranks");
    for (uint32_t b = 0; b < nb; b++)
        if (bin_dest[b] >= r->world || (b && bin_dest[b] < bin_dest[b - 1]))
            return set_err(r, ORX_ERR_INVALID_ARGUMENT, "bin_dest must be ascending ranks < world");
    /* the run of each rank must lie inside the send buffer; the plan's counts come from the
     * histogram of the same photons, so the runs are exactly filled */
    for (uint32_t d = 0; d < r->world; d++)
        if (dest_base[d] > send_records || (d && dest_base[d] < dest_base[d - 1]))
            return set_err(r, ORX_ERR_INVALID_ARGUMENT, "dest_base must be ascending and inside the send buffer");
    if (send_records > 0xffffffffull) return set_err(r, ORX_ERR_UNSUPPORTED, "send buffer beyond 2^32 records");
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t st = cur_stream(r);
    HIPCHK(r, r->slab.tab.ensure(8192));
    HIPCHK(r, r->slab.cur.ensure(64 * 4));
    HIPCHK(r, hipMemcpyAsync(r->slab.tab.p, bin_dest, nb, hipMemcpyHostToDevice, st));
    HIPCHK(r, hipMemcpyAsync(r->slab.cur.p, dest_base, (size_t)r->world * 4, hipMemcpyHostToDevice, st));
    launch_slab_pack(st, r->pb, slab_bins(r, nb), axis, halo_bins, r->slab.tab.as<uint8_t>(), r->world,
                     r->slab.cur.as<uint32_t>(), (uint32_t)send_records, (float*)send);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_ppm_slab_import(orx_renderer* r, const void* recv, uint64_t n, const uint32_t* photon_box,
                               uint32_t axis, uint32_t nb, uint32_t own_lo, uint32_t own_hi) {
    if (!r || (!recv && n) || axis > 2 || nb == 0 || nb > 1024) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->slab.on || !r->rng_ready) return set_err(r, ORX_ERR_STATE, "orx_ppm_slab_import: slab mode, after the photon pass");
    if (n > r->fs.S_cap) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "more photons than the slab import capacity");
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t st = cur_stream(r);
    /* the photon AABB replicas hold the own photon pass's deposits: reset, then the imported ones */
    HIPCHK(r, hipMemsetAsync(r->pb.bbox, 0xff, 3 * BBOX_REPLICAS * 4, st));
    HIPCHK(r, hipMemsetAsync(r->pb.bbox + 3 * BBOX_REPLICAS, 0, 3 * BBOX_REPLICAS * 4, st));
    PhotonBufs pbi = r->pb;
    const size_t groups = n ? (n + pbi.D - 1) / pbi.D : 1; /* an empty import: one group with no deposit */
    pbi.S = (uint32_t)(groups * pbi.D);
    pbi.bs_nchunk = (pbi.S + 16383) / 16384;
    if (n == 0) HIPCHK(r, hipMemsetAsync(r->pb.vmask, 0, 1, st));
    else launch_slab_import(st, pbi, (const float*)recv, (uint32_t)n);
    GridBox gb{};
    if (photon_box) {
        gb.on = 1;
        for (int k = 0; k < 6; k++) gb.b[k] = photon_box[k];
    }
    ppm_grid_build(r, pbi, gb);
    r->slab.own_axis = axis;
    r->slab.own_nb = nb;
    r->slab.own_lo = own_lo;
    r->slab.own_hi = own_hi;
    if (r->pipe.last_pipelined) HIPCHK(r, hipEventRecord(r->pipe.ev_grid_done, st));
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_export_hitpoints(orx_renderer* r, void* dst, size_t bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    const size_t npx = (size_t)r->max_rows * r->W, need = hp_export_plane(npx) * 28;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    HIPCHK(r, hipSetDevice(r->device));
    launch_export_hp(cur_stream(r), r->px, (uint32_t)npx, (float*)dst);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_ppm_gather_external(orx_renderer* r, const void* hp, uint32_t segments, void* indirect, size_t bytes) {
    if (!r || !hp || !indirect || segments == 0) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->rng_ready) return set_err(r, ORX_ERR_STATE, "no local passes yet");
    if (r->pb.hash) return set_err(r, ORX_ERR_UNSUPPORTED, "the stochastic hash photon map is single-device");
    size_t need = (size_t)segments * r->max_rows * r->W * 12;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "indirect buffer too small");
    HIPCHK(r, hipSetDevice(r->device));
    GatherIn gi;
    gi.base = (const uint8_t*)hp;
    gi.seg_bytes = hp_export_plane((size_t)r->max_rows * r->W) * 28;
    gi.raw = 1;
    gi.segments = segments;
    gi.seg_rows = r->max_rows;
    gi.W = r->W;
    gi.indirect = (float*)indirect;
    gi.dbg = nullptr;
    gi.cull = r->slab.on ? 2u : 0u;
    gi.own_axis = r->slab.own_axis;
    gi.own_lo = r->slab.own_lo;
    gi.own_hi = r->slab.own_hi;
    if (r->slab.on) gi.own_sb = slab_bins(r, r->slab.own_nb);
    gi.visits = 0; /* rank-local counts are not the reference's; no per-pixel debug buffers here */
    gi.order = gather_order((size_t)r->W * r->H);
    hipStream_t st = cur_stream(r);
    if (r->pipe.last_pipelined) { /* on the side stream, after the grid build */
        st = gather_stream(r);
        HIPCHK(r, hipStreamWaitEvent(st, r->pipe.ev_grid_done, 0));
    }
    ev_begin(r, P_GATHER, st);
    if (r->slab.on && r->cfg.photon_map == 0) { /* the tiles with hit points that reach this rank's photons */
        const size_t ntiles = (size_t)((r->W + 15) / 16) * ((segments * r->max_rows + 15) / 16);
        HIPCHK(r, r->slab.tiles.ensure(ntiles * 5 + 64));
        uint32_t* list = r->slab.tiles.as<uint32_t>();
        uint32_t* count = list + ntiles;
        uint8_t* flags = (uint8_t*)(count + 4);
        launch_gather_tiles(st, gi, r->pb, r->last_consts, flags, list, count);
        gi.tile_list = list;
        gi.tile_count = count;
    }
    ppm_gather(r, st, gi, r->last_consts);
    ev_end(r, P_GATHER, st);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}

orx_status orx_ppm_finish_on(orx_renderer* r, const void* indirect, size_t bytes, void* stream) {
    if (!r || !indirect) return ORX_ERR_INVALID_ARGUMENT;
    size_t need = (size_t)r->max_rows * r->W * 12;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "indirect buffer too small");
    HIPCHK(r, hipSetDevice(r->device));
    if (r->pipe.last_pipelined) {
        /* output only (direct ran beside the grid build), on `stream` (NULL: the side stream): the oldest
         * outstanding iteration, i.e. the one before the last eye pass if its finish was held back */
        if (!r->fin.snap && !r->fin.due) return set_err(r, ORX_ERR_STATE, "no sharded PPM iteration to finish");
        const bool prev = r->fin.snap;
        const PixelBufs px = prev ? r->fin.px : r->px;
        const Consts c = prev ? r->fin.consts : r->last_consts;
        const uint32_t k = prev ? r->fin.pp : r->pipe.pp;
        hipStream_t g = stream ? (hipStream_t)stream : gather_stream(r);
        launch_indirect_atten(g, px, (uint32_t)(need / 12), (const float*)indirect);
        /* the direct pass of that iteration: not yet overwritten, since the next one's photon pass (which
         * records the event again) is issued after this finish */
        HIPCHK(r, hipStreamWaitEvent(g, r->pipe.ev_direct_done, 0));
        ev_begin(r, P_DIRECT, g);
        launch_ppm_direct_output(g, r->scene, px, c, 2);
        ev_end(r, P_DIRECT, g);
        conv_update(r, g, prev ? r->fin.conv : r->conv.it);
        HIPCHK(r, hipEventRecord(r->pipe.ev_gdone[k], g));
        if (prev) r->fin.snap = false;
        else r->fin.due = false;
        r->pipe.gather_in_flight = true;
        HIPCHK(r, hipGetLastError());
        return ORX_OK;
    }
    hipStream_t st = stream ? (hipStream_t)stream : cur_stream(r);
    launch_indirect_atten(st, r->px, (uint32_t)(need / 12), (const float*)indirect);
    ev_begin(r, P_DIRECT, st);
    launch_ppm_direct_output(st, r->scene, r->px, r->last_consts);
    ev_end(r, P_DIRECT, st);
    conv_update(r, st, r->conv.it);
    HIPCHK(r, hipGetLastError());
    return ORX_OK;
}
orx_status orx_ppm_finish(orx_renderer* r, const void* indirect, size_t bytes) {
    return orx_ppm_finish_on(r, indirect, bytes, nullptr);
}

orx_status orx_set_ppm_pipeline(orx_renderer* r, void* side_stream, int enable) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (enable && r->cfg.photon_map == 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "sharded PPM pipelining needs the uniform grid or kd-tree photon map");
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    r->fin.shard_pipe = enable != 0;
    r->fin.side = enable ? (hipStream_t)side_stream : nullptr;
    r->fin.due = r->fin.snap = false;
    r->rng_ready = false; /* re-allocate the frame with the second buffer set (as orx_set_shard) */
    return ORX_OK;
}


}  // extern "C"
