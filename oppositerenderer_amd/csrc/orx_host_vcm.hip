/*
 * orx_host_vcm.hip — the VCM_BIDIRECTIONAL_PATH_TRACING branch of renderNextIteration
 * (OptixRenderer.cpp:675-795) on the host: buffers and views, the light and camera passes with their
 * overlap and vertex merging, and the sharded phase API (orx_vcm_local_light / _finish).
 *
 * Row-sharded layout: rank r owns image rows y = rank + j*world (j < rows);
 * light subpath i pairs with own pixel i, so vertex counts, light vertices,
 * camera colours and the output hold own rows only.  The light pass's
 * connectCameraT1 splats land anywhere on the image: they are accumulated in
 * an owner-block buffer [world][max_rows][W][3] that a sharded run sums
 * across ranks (reduce-scatter) before the camera pass.
 */
#include "orx_host.h"

using namespace orx;

extern "C" orx_status orx_vcm_mis_factors(uint32_t width, uint32_t height, float radius, int merging, float* mis_vc, float* mis_vm,
                               float* vm_normalization) {
    if (!mis_vc || !mis_vm || !vm_normalization) return ORX_ERR_INVALID_ARGUMENT;
    /* etaVCM = (nVM / nVC) * PI * r^2 with nVC = 1, nVM = lightSubPathCount (OptixRenderer.cpp:677-696) */
    const float count = (float)(width * height);
    const float ppmRadiusSquared = radius * radius;
    const float etaVCM = (count / (float)1u) * ORX_PI_F * ppmRadiusSquared;
    *mis_vc = 1.f / etaVCM;
    *mis_vm = merging ? etaVCM : 0.f;
    *vm_normalization = 1.f / (ppmRadiusSquared * ORX_PI_F * count);
    return ORX_OK;
}

/* vertex merging: the caches and the grid of this iteration (vcm_prepare); vb.cvA stays null with
 * cfg.vcm_merging off */
static orx_status vcm_prepare_merging(orx_renderer* r, float ppm_radius, float vm_norm) {
    VcmBufs& vb = r->vcm.vb;
    vb.cvA = nullptr;
    if (!r->cfg.vcm_merging) return ORX_OK;
    const size_t lpx = (size_t)r->W * r->rows;
    const uint32_t cvmax = r->cfg.vcm_max_path_length;
    const size_t nrec = lpx * cvmax, nslots = lpx * VCM_MAX_VERTS;
    if (nrec >= (1ull << 31) || nslots >= (1ull << 31))
        return set_err(r, ORX_ERR_UNSUPPORTED, "vertex merging: more than 2^31 vertex slots");
    VcmMergeBufs& mb = r->mg.mb;
    const size_t sort_tmp = nslots ? vcm_merge_sort_tmp_bytes((uint32_t)nslots) : 0;
    const size_t G1 = (size_t)VCM_MERGE_GRID_MAX * VCM_MERGE_GRID_MAX * VCM_MERGE_GRID_MAX + 2;
    if (r->mg.mpx != lpx || !r->mg.cverts.p) {
        HIPCHK(r, r->mg.cverts.ensure(nrec * 64 + 64));
        HIPCHK(r, r->mg.cvcount.ensure(lpx * 4 + 4));
        HIPCHK(r, r->mg.keys.ensure(nslots * 16 + 64));
        HIPCHK(r, r->mg.sort.ensure(sort_tmp + 64));
        HIPCHK(r, r->mg.start.ensure(G1 * 4));
        HIPCHK(r, r->mg.lrec.ensure(nslots * 48 + 64));
        HIPCHK(r, r->mg.part.ensure(nrec * 16 + 64));
        HIPCHK(r, r->mg.merge.ensure(lpx * 12 + 12));
        if (r->cfg.debug_counters) {
            HIPCHK(r, r->mg.cand.ensure(nrec * 4 + 4));
            HIPCHK(r, r->mg.count.ensure(lpx * 8 + 8));
        }
        HIPCHK(r, hipMemsetAsync(r->mg.cvcount.p, 0, lpx * 4, cur_stream(r)));
        r->mg.mpx = lpx;
        r->mg.merged = false;
    }
    if (r->has_tex) HIPCHK(r, r->mg.cvkd.ensure(nrec * 16 + 16));
    vb.cvA = r->mg.cverts.as<float4>();
    vb.cvB = vb.cvA + nrec;
    vb.cvC = vb.cvB + nrec;
    vb.cvD = vb.cvC + nrec;
    vb.cvE = r->has_tex ? r->mg.cvkd.as<float4>() : nullptr;
    vb.cvcount = r->mg.cvcount.as<uint32_t>();
    vb.cvmax = cvmax;
    mb.nmats = r->n_mats;
    mb.nslots = (uint32_t)nslots;
    mb.keys = r->mg.keys.as<uint32_t>();
    mb.vals = mb.keys + nslots;
    mb.keys_sorted = mb.vals + nslots;
    mb.vals_sorted = mb.keys_sorted + nslots;
    mb.sort_tmp = r->mg.sort.p;
    mb.sort_tmp_bytes = sort_tmp;
    mb.start = r->mg.start.as<uint32_t>();
    mb.lr0 = r->mg.lrec.as<float4>();
    mb.lr1 = mb.lr0 + nslots;
    mb.lr2 = mb.lr1 + nslots;
    mb.part = r->mg.part.as<float4>();
    mb.merge = r->mg.merge.as<float>();
    mb.cand = r->cfg.debug_counters ? r->mg.cand.as<uint32_t>() : nullptr;
    mb.mcount = r->cfg.debug_counters ? r->mg.count.as<uint32_t>() : nullptr;
    /* the grid over the scene AABB: cells of edge max(2 rq, largest extent / 128); vertices and query
     * windows are clamped into it, so a degenerate box or radius only costs candidates */
    VcmMergeGrid& g = r->mg.grid;
    const f3 lo = r->aabb_lo, hi = r->aabb_hi;
    const float ext[3] = {hi.x - lo.x, hi.y - lo.y, hi.z - lo.z};
    const float maxext = std::max(std::max(ext[0], ext[1]), std::max(ext[2], 0.f));
    float scale = 0.f;
    for (float v : {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}) scale = std::max(scale, fabsf(v));
    g.ox = lo.x;
    g.oy = lo.y;
    g.oz = lo.z;
    g.r2 = ppm_radius * ppm_radius;
    /* the window's half-width covers every pair the fp32 test accepts: d2 <= r2 bounds each |d.x| by
     * r (1 + 2^-23), and the window's own subtractions round by at most an ulp of the coordinate */
    g.rq = fabsf(ppm_radius) * 1.0001f + 1e-5f * scale;
    g.misVc = r->vcm.c.misVc;
    g.vmNorm = vm_norm;
    const float cell = std::max(2.f * g.rq, maxext / (float)VCM_MERGE_GRID_MAX);
    uint32_t gd[3] = {1, 1, 1};
    g.inv = 0.f;
    if (cell > 0.f && std::isfinite(cell) && std::isfinite(maxext) && std::isfinite(scale)) {
        g.inv = 1.f / cell;
        if (std::isfinite(g.inv)) {
            for (int a = 0; a < 3; a++) {
                const float n = ceilf(ext[a] * g.inv);
                gd[a] = n >= (float)VCM_MERGE_GRID_MAX ? VCM_MERGE_GRID_MAX : n >= 1.f ? (uint32_t)n : 1u;
            }
        } else {
            g.inv = 0.f;
        }
    }
    g.gx = gd[0];
    g.gy = gd[1];
    g.gz = gd[2];
    g.G = gd[0] * gd[1] * gd[2];
    return ORX_OK;
}

/* The kernels' view of the current VCM set (vcm.dpar).  Every vcm.vb pointer into a VcmSet, and the
 * control words and constants copy that go with the set's parity, is written here and nowhere else.
 * lcap: room for the light pass's deferred camera connections (0: it traces them itself). */
static void bind_vcm_views(orx_renderer* r, size_t lcap = 0) {
    VcmBufs& vb = r->vcm.vb;
    const VcmSet& vs = r->vcm.set[r->vcm.dpar];
    const size_t lpx = (size_t)r->W * r->rows, plane = lpx * VCM_MAX_VERTS;
    vb.vcount = vs.count.as<uint32_t>();
    vb.vA = vs.verts.as<float4>();
    vb.vB = vb.vA + plane;
    vb.vC = vb.vB + plane;
    vb.vD = vb.vC + plane;
    vb.vE = r->has_tex ? vs.kd.as<float4>() : nullptr;
    vb.splat = vs.splat.as<float>();
    vb.splat_in = vb.splat + (size_t)r->rank * r->max_rows * r->W * 3;
    vb.consts_keep = vb.consts + 1 + r->vcm.dpar; /* vcm.consts: [0] the launches', [1 + set] the resolve's */
    vb.dq0 = vs.dq.as<float4>(); /* null with ORX_VCM_DEFER=0: the shadow rays in place */
    if (vb.dq0) {
        const size_t cap = r->vcm.dqcap, nslot = (size_t)r->rows * r->RW;
        vb.dq1 = vb.dq0 + cap;
        vb.dq2 = vb.dq1 + cap;
        vb.docc = (uint8_t*)(vb.dq2 + cap);
        vb.demis = vs.dpx.as<float4>();
        vb.dhead = (uint32_t*)(vb.demis + lpx);
        vb.dctl = vb.work + (r->vcm.dpar ? 8 : 4); /* vcm.work: [0..1] work counters, [4..7] / [8..11] the lists' control words */
        vb.dcap = (uint32_t)std::min<size_t>(cap, 0xfffffff0u);
        for (int k = 0; k < 6; k++) vb.rsave.p[k] = vs.rngsave.as<uint32_t>() + (size_t)k * nslot;
    }
    vb.lcq = lcap ? vs.lcq.as<float4>() : nullptr;
    vb.lcap = (uint32_t)lcap;
    vb.lctl = lcap ? vb.work + (r->vcm.dpar ? 14 : 12) : nullptr;
}

/* buffers, views and constants of one VCM iteration on the current set */
static orx_status vcm_prepare(orx_renderer* r, const orx_request* det, float ppm_radius) {
    VcmSet& vs = r->vcm.set[r->vcm.dpar];
    const size_t lpx = (size_t)r->W * r->rows;
    const size_t spx = (size_t)r->W * r->max_rows * r->world;
    if (r->vcm.npx != lpx || r->vcm.spx != spx) {
        HIPCHK(r, vs.count.ensure(lpx * 4 + 4));
        HIPCHK(r, vs.verts.ensure(lpx * VCM_MAX_VERTS * 64 + 64));
        HIPCHK(r, vs.splat.ensure(spx * 12 + 12));
        HIPCHK(r, r->vcm.cam.ensure(lpx * 12 + 12));
        HIPCHK(r, hipMemsetAsync(vs.count.p, 0, lpx * 4, cur_stream(r)));
        HIPCHK(r, hipMemsetAsync(r->vcm.cam.p, 0, lpx * 12, cur_stream(r)));
        r->vcm.npx = lpx;
        r->vcm.kd = false;
        r->vcm.spx = spx;
    }
    VcmBufs& vb = r->vcm.vb;
    vb.RW = r->RW;
    vb.rng = r->px.rng;
    if (r->has_tex && !r->vcm.kd) {
        HIPCHK(r, vs.kd.ensure(lpx * VCM_MAX_VERTS * 16 + 16));
        r->vcm.kd = true;
    }
    vb.splat_n = (uint32_t)std::min<size_t>(spx * 3, 0xffffffffu);
    {
        const size_t waves = std::max(vcm_camera_waves(((r->W + 7) / 8) * ((r->rows + 7) / 8)),
                                      vcm_light_waves((uint32_t)((lpx + 63) / 64)));
        /* [waves] queues for the light pass and walk, [waves] for the resolve's rerun beside them */
        HIPCHK(r, r->vcm.shq.ensure(2 * waves * VCM_SHQ_PER_WAVE * 16 + 16));
        vb.shq = r->vcm.shq.as<float4>();
        vb.shq_rerun = vb.shq + waves * VCM_SHQ_PER_WAVE;
        HIPCHK(r, r->vcm.work.ensure(64)); /* [0..1] work counters, [4..7] / [8..11] entry-list control words */
        vb.work = r->vcm.work.as<uint32_t>();
        HIPCHK(r, r->vcm.consts.ensure(3 * sizeof(VcmConsts))); /* [0] the launches', [1 + set] the resolve's */
        vb.consts = r->vcm.consts.as<VcmConsts>();
    }
    vb.cam = r->vcm.cam.as<float>();
    vb.output = r->d_out.as<float>();
    {
        /* The camera pass defers its connection shadow rays to k_vcm_shadow through an entry list of
         * ORX_VCM_DEFER = N per own pixel (default 16; the hall averages 6.5; a list that overflows makes
         * the pass rerun in place, small N exercises that, tests/test_gpu_parity.py); 0 traces them in
         * place inside the camera kernel.  Hall camera pass 6.21 -> 5.74 ms (473 -> 500 Mpaths/s): the
         * shadow kernel (61 VGPRs) runs at 8 waves per SIMD with a 16-entry LDS stack continued in
         * global memory, against the camera kernel's 3 (profiles/r04g_vcm_shadow_short_stack.txt) */
        static const uint32_t per_px = [] {
            const char* e = getenv("ORX_VCM_DEFER");
            return e ? (uint32_t)std::max(0, atoi(e)) : 16u;
        }();
        if (per_px) {
            const size_t cap = lpx * per_px;
            const size_t nslot = (size_t)r->rows * r->RW;
            HIPCHK(r, vs.dq.ensure(cap * 49 + 64));
            HIPCHK(r, vs.dpx.ensure(lpx * 20 + 64));
            HIPCHK(r, vs.rngsave.ensure(nslot * 24 + 16));
            r->vcm.dqcap = cap;
            /* the shadow kernel's deep stack entries: (stack bound + 2 - 16) per lane of the largest grid */
            int dev = 0, cus = 256;
            hipGetDevice(&dev);
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            const size_t lanes = (size_t)cus * 32 * 64;
            const uint32_t deep = vcm_shadow_stack_deep(r->scene.stack_entries);
            HIPCHK(r, r->vcm.shstk.ensure((size_t)deep * lanes * 4 + 64));
            vb.shstk = r->vcm.shstk.as<uint32_t>();
            vb.shstk_lanes = (uint32_t)lanes;
            vb.shdeep = deep;
        }
    }
    bind_vcm_views(r);
    VcmConsts& c = r->vcm.c;
    float ulen = 0.f, vlen = 0.f;
    DevCamera cam = camera_setup(det->camera, &ulen, &vlen);
    c.eye = cam.eye;
    c.lookdir = cam.lookdir;
    c.u = cam.u;
    c.v = cam.v;
    c.unitU = normalize(cam.u);
    c.unitV = normalize(cam.v);
    c.lookdirN = normalize(cam.lookdir);
    c.lookdirLen = length(cam.lookdir);
    c.ipsx = 2.0f * ulen;
    c.ipsy = 2.0f * vlen;
    c.psfx = r->vcm.psf_x;
    c.psfy = r->vcm.psf_y;
    c.W = r->W;
    c.H = r->H;
    c.count = r->W * r->H;
    c.rank = r->rank;
    c.world = r->world;
    c.rows = r->rows;
    c.max_rows = r->max_rows;
    c.lcount = r->W * r->rows;
    c.maxPathLen = r->cfg.vcm_max_path_length;
    /* misVc = 1 / etaVCM; misVm = etaVCM with vertex merging, 0 without (vcmUseVM = false) */
    float vm_norm = 0.f;
    orx_vcm_mis_factors(r->W, r->H, ppm_radius, r->cfg.vcm_merging != 0, &c.misVc, &c.misVm, &vm_norm);
    return vcm_prepare_merging(r, ppm_radius, vm_norm);
}

static orx_status vcm_light(orx_renderer* r) {
    hipStream_t st = cur_stream(r);
    ev_begin(r, P_VCM_LIGHT);
    if (!r->vcm.estimated) { /* subpath length estimate launch: advances the RNG, stores nothing */
        launch_vcm_light(st, r->scene, r->vcm.vb, r->vcm.c, true);
        r->vcm.estimated = true;
    }
    HIPCHK(r, hipMemsetAsync(r->vcm.vb.splat, 0, r->vcm.spx * 12, st));
    launch_vcm_light(st, r->scene, r->vcm.vb, r->vcm.c, false);
    ev_end(r, P_VCM_LIGHT);
    if (r->vcm.vb.cvA) { /* vertex merging: this iteration's light vertices into their grid */
        ev_begin(r, P_VCM_GRID);
        launch_vcm_merge_grid(st, r->scene, r->vcm.vb, r->mg.mb, r->mg.grid, r->vcm.c.lcount);
        ev_end(r, P_VCM_GRID);
    }
    return ORX_OK;
}

static orx_status vcm_camera(orx_renderer* r, bool overlap = false) {
    if (!overlap) {
        hipStream_t st = cur_stream(r);
        ev_begin(r, P_VCM_CAMERA);
        launch_vcm_camera_walk(st, r->scene, r->vcm.vb, r->vcm.c);
        ev_end(r, P_VCM_CAMERA);
        ev_begin(r, P_VCM_SHADOW);
        launch_vcm_camera_resolve(st, r->scene, r->vcm.vb, r->vcm.c);
        ev_end(r, P_VCM_SHADOW);
        if (r->vcm.vb.cvA) { /* vertex merging, after whichever of k_vcm_accum and the rerun wrote the colours */
            ev_begin(r, P_VCM_MERGE);
            launch_vcm_merge(st, r->scene, r->vcm.vb, r->mg.mb, r->mg.grid, r->vcm.c.lcount);
            ev_end(r, P_VCM_MERGE);
            r->mg.merged = true;
        }
        return ORX_OK;
    }
    /* the walk on the renderer's stream, the resolve (with the rerun an overflow needs) on aux beside the
     * next iteration's light pass and walk (the pass interval ends with the resolve); the stream then
     * waits for the previous iteration's resolve, since the next light pass and walk write the set it
     * reads (light image, light vertices, entry list, RNG start words, constants copy) */
    hipStream_t st = cur_stream(r);
    ev_begin(r, P_VCM_CAMERA);
    launch_vcm_camera_walk(st, r->scene, r->vcm.vb, r->vcm.c);
    ev_end(r, P_VCM_CAMERA);
    HIPCHK(r, hipEventRecord(r->vcm.ev_cam, st));
    if (r->vcm.resolve_in_flight) HIPCHK(r, hipStreamWaitEvent(st, r->vcm.ev_acc, 0));
    HIPCHK(r, hipStreamWaitEvent(r->aux, r->vcm.ev_cam, 0));
    ev_begin(r, P_VCM_SHADOW, r->aux);
    launch_vcm_camera_resolve(r->aux, r->scene, r->vcm.vb, r->vcm.c);
    ev_end(r, P_VCM_SHADOW, r->aux);
    conv_update(r, r->aux, r->conv.it); /* behind k_vcm_accum and the rerun an overflow needs */
    HIPCHK(r, hipEventRecord(r->vcm.ev_acc, r->aux));
    r->vcm.resolve_in_flight = true;
    return ORX_OK;
}

orx_status orx::vcm_check_lights(orx_renderer* r) {
    for (const DevLight& l : r->host_lights)
        if (l.type == LIGHT_SPOT)
            return set_err(r, ORX_ERR_UNSUPPORTED, "VCM: spot lights are not emitted by lightEmit (helpers/light.h:130)");
    return ORX_OK;
}

/* One VCM iteration on one device.  overlap: on the set the last resolve does not read (light image,
 * entry lists, and what the resolve's in-place rerun after an overflow reads: light vertices with
 * counts and texel colours, the walk's RNG start words), the resolve left running on aux. */
orx_status orx::vcm_iteration(orx_renderer* r, const orx_request* det, float ppm_radius, bool overlap) {
    orx_status s = vcm_prepare(r, det, ppm_radius);
    if (s != ORX_OK) return s;
    /* vertex merging runs its passes serially (the merge reads what the next light pass would rewrite) */
    overlap = overlap && r->vcm.vb.dq0 && !r->cfg.vcm_merging;
    if (overlap) {
        const VcmSet& cur = r->vcm.set[r->vcm.dpar];
        VcmSet& next = r->vcm.set[r->vcm.dpar ^ 1u];
        HIPCHK(r, next.splat.ensure(cur.splat.bytes));
        HIPCHK(r, next.dq.ensure(cur.dq.bytes));
        HIPCHK(r, next.dpx.ensure(cur.dpx.bytes));
        HIPCHK(r, next.verts.ensure(cur.verts.bytes));
        HIPCHK(r, next.count.ensure(cur.count.bytes));
        HIPCHK(r, next.rngsave.ensure(cur.rngsave.bytes));
        if (r->has_tex) HIPCHK(r, next.kd.ensure(cur.kd.bytes));
        /* the light pass's camera connections go with the resolve too (hall 536 -> 568 Mpaths/s,
         * profiles/r05r_vcm_light_defer_ab.txt): room for 4 per own subpath, against the hall's ~3 stored
         * light vertices per subpath with at most one connection each (a wave whose queue does not fit
         * traces it in place; ORX_VCM_LIGHT_DEFER=0: all in place) */
        static const uint32_t lper = [] {
            const char* e = getenv("ORX_VCM_LIGHT_DEFER");
            return e ? (uint32_t)std::max(0, atoi(e)) : 4u;
        }();
        const size_t lcap = std::min<size_t>((size_t)r->W * r->rows * lper, 0x0ffffff0u);
        if (lcap) {
            HIPCHK(r, r->vcm.set[0].lcq.ensure(lcap * 48 + 64));
            HIPCHK(r, r->vcm.set[1].lcq.ensure(lcap * 48 + 64));
        }
        r->vcm.dpar ^= 1u;
        bind_vcm_views(r, lcap);
    }
    if ((s = vcm_light(r)) != ORX_OK) return s;
    r->vcm.last_overlap = overlap;
    return vcm_camera(r, overlap);
}

extern "C" {

/* test hook: drive the last VCM iteration's resolve again with stale list state -- the entry count
 * past the capacity, every odd own pixel's list head past the entries, and 64 light-connection entries
 * appended whose pixel offsets lie past the light image -- as a walk or light pass that did not write
 * this set's control words would leave them (vcm.h:315-400 / :43-58 have no such state: the device-side
 * bounds in k_vcm_accum and k_vcm_light_shadow are ours).  Synchronous; the colours land in
 * ORX_BUF_VCM_CAMERA (the output is accumulated once more: not a render) */
orx_status orx_debug_vcm_stale_resolve(orx_renderer* r) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    const VcmBufs& vb = r->vcm.vb;
    if (!vb.dq0 || !r->vcm.npx) return set_err(r, ORX_ERR_STATE, "no VCM iteration with deferred lists");
    HIPCHK(r, hipSetDevice(r->device));
    flush_pipeline(r);
    HIPCHK(r, hipStreamSynchronize(cur_stream(r)));
    HIPCHK(r, hipDeviceSynchronize());
    const size_t lpx = r->vcm.npx;
    std::vector<uint32_t> head(lpx);
    HIPCHK(r, hipMemcpy(head.data(), vb.dhead, lpx * 4, hipMemcpyDeviceToHost));
    for (size_t p = 1; p < lpx; p += 2) head[p] = vb.dcap + (uint32_t)p;
    HIPCHK(r, hipMemcpy(vb.dhead, head.data(), lpx * 4, hipMemcpyHostToDevice));
    const uint32_t stale = 0xfffffff0u;
    HIPCHK(r, hipMemcpy(vb.dctl, &stale, 4, hipMemcpyHostToDevice));
    if (vb.lcq && vb.lcap >= 64) {
        uint32_t lc[2] = {0, 0};
        HIPCHK(r, hipMemcpy(lc, vb.lctl, 8, hipMemcpyDeviceToHost));
        const uint32_t base = std::min(lc[0], vb.lcap - 64);
        std::vector<float4> e(3 * 64);
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t at = vb.splat_n + 3 * k; /* past the light image */
            float w;
            memcpy(&w, &at, 4);
            e[3 * k + 0] = make_float4(0.f, 0.f, 0.f, 0.f); /* distance 0: unoccluded without a walk */
            e[3 * k + 1] = make_float4(0.f, 0.f, 1.f, w);
            e[3 * k + 2] = make_float4(1.f, 1.f, 1.f, 0.f);
        }
        HIPCHK(r, hipMemcpy(vb.lcq + 3 * (size_t)base, e.data(), e.size() * 16, hipMemcpyHostToDevice));
        lc[0] = base + 64;
        HIPCHK(r, hipMemcpy(vb.lctl, lc, 4, hipMemcpyHostToDevice));
    }
    launch_vcm_camera_resolve(cur_stream(r), r->scene, vb, r->vcm.c);
    HIPCHK(r, hipGetLastError());
    HIPCHK(r, hipStreamSynchronize(cur_stream(r)));
    return ORX_OK;
}

size_t orx_vcm_splat_bytes(const orx_renderer* r) { return r ? (size_t)r->W * r->max_rows * r->world * 12 : 0; }

orx_status orx_vcm_local_light(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                               float ppm_radius, const orx_request* det) {
    if (!r || !det) return ORX_ERR_INVALID_ARGUMENT;
    if (det->method != ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING)
        return set_err(r, ORX_ERR_INVALID_ARGUMENT, "orx_vcm_local_light needs a VCM request");
    if (vcm_check_lights(r) != ORX_OK) return ORX_ERR_UNSUPPORTED;
    if (r->cfg.vcm_merging && r->world > 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "vertex merging is single-device (a rank would need every rank's light vertices)");
    orx_status s = begin_iteration(r, local_iteration_number, det);
    if (s != ORX_OK) return s;
    if ((s = vcm_prepare(r, det, ppm_radius)) != ORX_OK) return s;
    if ((s = vcm_light(r)) != ORX_OK) return s;
    HIPCHK(r, hipGetLastError());
    r->vcm.finish_due = true;
    r->last_method = (uint64_t)det->method;
    r->last_consts = make_consts(r, ppm_radius, local_iteration_number);
    note_iteration(r, iteration_number, local_iteration_number, ppm_radius, det->method);
    return ORX_OK;
}

orx_status orx_export_vcm_splats(orx_renderer* r, void* dst, size_t bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->vcm.finish_due) return set_err(r, ORX_ERR_STATE, "no VCM light pass to export");
    const size_t need = orx_vcm_splat_bytes(r);
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    HIPCHK(r, hipSetDevice(r->device));
    HIPCHK(r, hipMemcpyAsync(dst, r->vcm.vb.splat, need, hipMemcpyDeviceToDevice, cur_stream(r)));
    return ORX_OK;
}

orx_status orx_vcm_finish(orx_renderer* r, const void* splat_own_rows, size_t bytes) {
    if (!r || !splat_own_rows) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->vcm.finish_due) return set_err(r, ORX_ERR_STATE, "orx_vcm_finish without a light pass");
    const size_t need = (size_t)r->W * r->rows * 12;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "splat buffer too small");
    HIPCHK(r, hipSetDevice(r->device));
    /* the summed own-row splats replace the local ones (readable as ORX_BUF_VCM_SPLAT) */
    float* own = r->vcm.vb.splat + (size_t)r->rank * r->max_rows * r->W * 3;
    if ((const void*)own != splat_own_rows)
        HIPCHK(r, hipMemcpyAsync(own, splat_own_rows, need, hipMemcpyDeviceToDevice, cur_stream(r)));
    orx_status s = vcm_camera(r);
    if (s != ORX_OK) return s;
    conv_update(r, cur_stream(r), r->conv.it);
    HIPCHK(r, hipGetLastError());
    r->vcm.finish_due = false;
    return ORX_OK;
}


}  // extern "C"
