/*
 * orx_host_read.hip — reading the renderer's device buffers back in the reference's layouts
 * (orx_read_buffer), and the debug entry points that only read or poke buffers.
 */
#include "orx_host.h"

using namespace orx;

extern "C" {

#ifdef ORX_TRAV_STATS
/* stats build only: [closest: rays, nodes, leaves, tris, any: rays, nodes, leaves, tris]; reset = 1 zeroes */
int orx_trav_stats_read(orx_renderer* r, unsigned long long* out, int reset) {
    if (!r || !r->scene.trav_stats || hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpy(out, r->scene.trav_stats, 96, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    /* [16]: gather photons accepted (out must hold 21 values) */
    if (r->pb.grid && hipMemcpy(out + 16, &r->pb.grid->st_accepted, 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    /* [17..20]: closest-hit node visits to BVH4 nodes with index < 21, 85, 341, 1365 (the top 2..5 levels) */
    if (hipMemcpy(out + 17, r->scene.trav_stats + 16, 32, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (reset && hipMemset(r->scene.trav_stats, 0, 256) != hipSuccess) return 1;
    /* [12..15]: gather lane batches, wave batches, lane rows, wave rows */
    if (r->pb.grid) {
        if (hipMemcpy(out + 12, &r->pb.grid->st_lane_batches, 32, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (reset && hipMemset(&r->pb.grid->st_lane_batches, 0, 40) != hipSuccess) return 1;
    } else {
        for (int k = 12; k < 16; k++) out[k] = 0;
    }
    return 0;
}
#endif

orx_status orx_debug_limit_photon_stack(orx_renderer* r, uint32_t lanes) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (lanes < r->pb.tlanes) r->pb.tlanes = lanes;
    return ORX_OK;
}

orx_status orx_read_buffer(orx_renderer* r, int32_t id, void* dst, size_t bytes, size_t* out_bytes) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    if (!r->rng_ready) return set_err(r, ORX_ERR_STATE, "no frame rendered yet");
    HIPCHK(r, hipSetDevice(r->device));
    {
        orx_status s0 = sync_all(r);
        if (s0 != ORX_OK) return s0;
    }
    GridParams g{};
    HIPCHK(r, hipMemcpy(&g, r->pb.grid, sizeof g, hipMemcpyDeviceToHost));
    const size_t npx = (size_t)r->rows * r->W;
    const size_t nslot = (size_t)r->rng_rows * r->RW;
    size_t need = 0;
    switch (id) {
    case ORX_BUF_RNG: need = nslot * 24; break;
    case ORX_BUF_HITPOINTS: need = npx * 13 * 4; break;
    case ORX_BUF_PHOTONS: need = (r->pb.hash ? (size_t)r->pb.hnum : (size_t)g.valid) * 36; break;
    case ORX_BUF_GRID_OFFSETS: need = (r->pb.hash ? (size_t)r->pb.hnum : (size_t)g.G + 1) * 4; break;
    case ORX_BUF_INDIRECT: case ORX_BUF_DIRECT: case ORX_BUF_OUTPUT: need = npx * 12; break;
    case ORX_BUF_PHOTON_SLOTS: need = (size_t)r->pb.S * 36; break;
    case ORX_BUF_KD_TREE: need = r->cfg.photon_map == 2 ? (size_t)r->kds.view.tree_size * 40 : 0; break;
    case ORX_BUF_DEBUG_VISITED: need = npx * 8; break;
    case ORX_BUF_VCM_VERTEX_COUNT: need = r->vcm.npx * 4; break;
    case ORX_BUF_VCM_VERTICES: need = r->vcm.npx * VCM_MAX_VERTS * 64; break;
    case ORX_BUF_VCM_SPLAT: case ORX_BUF_VCM_CAMERA: need = r->vcm.npx * 12; break;
    case ORX_BUF_VOLUMETRIC: need = r->media.on ? npx * 12 : 0; break;
    case ORX_BUF_VOLUMETRIC_PHOTONS: need = r->media.on ? (size_t)r->cfg.volumetric_photons * 28 : 0; break;
    case ORX_BUF_VCM_CAMERA_VERTEX_COUNT: case ORX_BUF_VCM_CAMERA_VERTICES: case ORX_BUF_VCM_MERGE:
    case ORX_BUF_VCM_MERGE_COUNT: case ORX_BUF_VCM_MERGE_CANDIDATES:
        if (!r->cfg.vcm_merging) return set_err(r, ORX_ERR_STATE, "vertex merging is off (orx_config.vcm_merging)");
        if (!r->mg.merged || r->mg.mpx != npx) return set_err(r, ORX_ERR_STATE, "no VCM iteration with vertex merging yet");
        if ((id == ORX_BUF_VCM_MERGE_COUNT || id == ORX_BUF_VCM_MERGE_CANDIDATES) && !r->cfg.debug_counters)
            return set_err(r, ORX_ERR_STATE, "the merge pair counts are kept with debug_counters = 1");
        need = id == ORX_BUF_VCM_CAMERA_VERTICES ? r->mg.mpx * r->vcm.vb.cvmax * 64
               : id == ORX_BUF_VCM_MERGE         ? r->mg.mpx * 12
                                                 : r->mg.mpx * 4;
        break;
    case ORX_BUF_CONV_PREV: case ORX_BUF_CONV_SUM: case ORX_BUF_CONV_M2: case ORX_BUF_CONV_ERROR:
        if (!r->conv.on) return set_err(r, ORX_ERR_STATE, "convergence statistics are off (orx_set_convergence)");
        if (id == ORX_BUF_CONV_ERROR && !r->conv.err_n) return set_err(r, ORX_ERR_STATE, "no orx_get_convergence query yet");
        need = r->conv.npx * (id == ORX_BUF_CONV_PREV ? 12 : 4);
        break;
    default: return set_err(r, ORX_ERR_INVALID_ARGUMENT, "unknown buffer id");
    }
    if (out_bytes) *out_bytes = need;
    if (!dst) return ORX_OK;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    auto d2h = [&](void* h, const void* d, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost); };
    switch (id) {
    case ORX_BUF_RNG: {
        std::vector<uint32_t> planes(nslot * 6);
        HIPCHK(r, d2h(planes.data(), r->d_rng.p, nslot * 24));
        uint32_t* o = (uint32_t*)dst;
        for (size_t i = 0; i < nslot; i++)
            for (int k = 0; k < 6; k++) o[6 * i + k] = planes[k * nslot + i];
        break;
    }
    case ORX_BUF_HITPOINTS: {
        std::vector<float4> A(npx), B(npx);
        std::vector<float2> Cc(npx);
        HIPCHK(r, d2h(A.data(), r->px.hpA, npx * 16));
        HIPCHK(r, d2h(B.data(), r->px.hpB, npx * 16));
        HIPCHK(r, d2h(Cc.data(), r->px.hpC, npx * 8));
        float* o = (float*)dst;
        for (size_t i = 0; i < npx; i++) {
            uint32_t flags;
            std::memcpy(&flags, &A[i].w, 4);
            bool ns = (flags & PRD_HIT_NON_SPECULAR) != 0;
            float v[13] = {A[i].x, A[i].y, A[i].z,
                           ns ? B[i].x : 0.f, ns ? B[i].y : 0.f, ns ? B[i].z : 0.f,
                           B[i].w, Cc[i].x, Cc[i].y,
                           ns ? 0.f : B[i].x, ns ? 0.f : B[i].y, ns ? 0.f : B[i].z, A[i].w};
            std::memcpy(o + 13 * i, v, sizeof v);
        }
        break;
    }
    case ORX_BUF_PHOTONS: {
        if (r->pb.hash) { /* the table: each entry's photon (its winning slot), zeros when empty */
            const size_t hn = r->pb.hnum, ns = (size_t)r->pb.S;
            std::vector<uint32_t> cnt(hn), win(hn);
            std::vector<float4> R(4 * ns);
            HIPCHK(r, d2h(cnt.data(), r->pb.hcount, hn * 4));
            HIPCHK(r, d2h(win.data(), r->pb.hwin, hn * 4));
            if (ns) HIPCHK(r, d2h(R.data(), r->pb.slots, ns * 64));
            float* o = (float*)dst;
            for (size_t h = 0; h < hn; h++) {
                float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (cnt[h] && win[h] && win[h] <= ns) {
                    const float4 a = R[4 * (win[h] - 1)], b = R[4 * (win[h] - 1) + 1], c = R[4 * (win[h] - 1) + 2];
                    const float t[9] = {a.w, b.w, c.x, a.x, a.y, a.z, b.x, b.y, b.z};
                    std::memcpy(v, t, sizeof v);
                }
                std::memcpy(o + 9 * h, v, sizeof v);
            }
            break;
        }
        /* nine SoA planes -> [n][power3 position3 direction3] (Photon.h:10-33 order) */
        const size_t n = g.valid, P = r->pb.splane;
        std::vector<float> pl(9 * n);
        static const uint32_t order[9] = {SP_PX, SP_PY, SP_PZ, SP_X, SP_Y, SP_Z, SP_DX, SP_DY, SP_DZ};
        for (int q = 0; q < 9 && n; q++)
            HIPCHK(r, d2h(pl.data() + q * n, r->pb.sorted + order[q] * P, n * 4));
        /* sub-row layout: present the reference's cell order (each cell = its
         * nsub sub-row pieces, k_bs_count); within a cell the order is free */
        std::vector<uint32_t> idx;
        if (r->pb.subofs && r->pb.nsub > 1 && n) {
            const size_t rowlen = (size_t)g.gx * SUBX, nso = (size_t)g.G * r->pb.nsub * SUBX + 1;
            std::vector<uint32_t> so(nso);
            HIPCHK(r, d2h(so.data(), r->pb.subofs, nso * 4));
            idx.reserve(n);
            for (size_t c = 0; c < g.G; c++) {
                const size_t row = c / g.gx, x = c % g.gx;
                for (uint32_t sr = 0; sr < r->pb.nsub; sr++) {
                    const size_t b = (row * r->pb.nsub + sr) * rowlen + x * SUBX;
                    for (uint32_t k = so[b]; k < so[b + SUBX]; k++) idx.push_back(k);
                }
            }
            if (idx.size() != n) return set_err(r, ORX_ERR_STATE, "sub-row offsets do not cover the valid photons");
        }
        float* o = (float*)dst;
        for (size_t i = 0; i < n; i++) {
            const size_t src = idx.empty() ? i : idx[i];
            for (int k = 0; k < 9; k++) o[9 * i + k] = pl[k * n + src];
        }
        break;
    }
    case ORX_BUF_PHOTON_SLOTS: {
        const size_t n = (size_t)r->pb.S;
        std::vector<float4> R(4 * n);
        std::vector<uint8_t> vm((size_t)r->prows * r->cfg.photon_launch_width);
        if (n) HIPCHK(r, d2h(R.data(), r->pb.slots, n * 64));
        if (!vm.empty()) HIPCHK(r, d2h(vm.data(), r->pb.vmask, vm.size()));
        float* o = (float*)dst;
        const uint32_t D = r->pb.D; /* slots per emitted photon */
        for (size_t i = 0; i < n; i++) {
            const bool valid = (vm[i / D] >> (i % D)) & 1u;
            const float4 a = R[4 * i], b = R[4 * i + 1], c = R[4 * i + 2];
            float v[9] = {a.w, b.w, c.x, a.x, a.y, a.z, b.x, b.y, b.z};
            if (!valid) std::memset(v, 0, sizeof v);
            std::memcpy(o + 9 * i, v, sizeof v);
        }
        break;
    }
    case ORX_BUF_KD_TREE: { /* [tree_size][power3 position3 direction3 axis] */
        const size_t n = r->kds.view.tree_size;
        std::vector<float4> T(3 * n);
        if (n) HIPCHK(r, d2h(T.data(), r->kds.view.tree, n * 16));
        if (n) HIPCHK(r, d2h(T.data() + n, r->kds.view.tree_bc, n * 32));
        float* o = (float*)dst;
        for (size_t i = 0; i < n; i++) {
            const float4 a = T[i], b = T[n + 2 * i], c = T[n + 2 * i + 1];
            const float v[10] = {b.x, b.y, b.z, a.x, a.y, a.z, b.w, c.x, c.y, a.w};
            std::memcpy(o + 10 * i, v, sizeof v);
        }
        break;
    }
    case ORX_BUF_GRID_OFFSETS: HIPCHK(r, d2h(dst, r->pb.hash ? r->pb.hcount : r->pb.offsets, need)); break;
    case ORX_BUF_INDIRECT: HIPCHK(r, d2h(dst, r->d_ind.p, need)); break;
    case ORX_BUF_VOLUMETRIC: if (need) HIPCHK(r, d2h(dst, r->media.volR.p, need)); break;
    case ORX_BUF_VOLUMETRIC_PHOTONS: {
        if (!need) break;
        const size_t NV = r->cfg.volumetric_photons;
        std::vector<uint32_t> cnt(NV);
        std::vector<float4> A(NV), B(NV);
        HIPCHK(r, d2h(cnt.data(), r->media.cnt.p, NV * 4));
        HIPCHK(r, d2h(A.data(), r->media.A.p, NV * 16));
        HIPCHK(r, d2h(B.data(), r->media.B.p, NV * 16));
        float* o = (float*)dst;
        for (size_t i = 0; i < NV; i++) {
            const bool on = r->media.vm.valid && cnt[i];
            float v[7] = {on ? B[i].x : 0.f, on ? B[i].y : 0.f, on ? B[i].z : 0.f,
                          on ? A[i].x : 0.f, on ? A[i].y : 0.f, on ? A[i].z : 0.f, 0.f};
            const uint32_t c = on ? cnt[i] : 0u;
            std::memcpy(&v[6], &c, 4);
            std::memcpy(o + 7 * i, v, sizeof v);
        }
        break;
    }
    case ORX_BUF_DIRECT: HIPCHK(r, d2h(dst, r->px.direct, need)); break;
    case ORX_BUF_OUTPUT: HIPCHK(r, d2h(dst, r->d_out.p, need)); break;
    case ORX_BUF_DEBUG_VISITED: HIPCHK(r, d2h(dst, r->d_dbg.p, need)); break;
    case ORX_BUF_VCM_VERTEX_COUNT: HIPCHK(r, d2h(dst, r->vcm.vb.vcount, need)); break;
    case ORX_BUF_VCM_SPLAT: /* own rows of the owner-block buffer */
        HIPCHK(r, d2h(dst, r->vcm.vb.splat_in, need));
        break;
    case ORX_BUF_VCM_CAMERA: HIPCHK(r, d2h(dst, r->vcm.cam.p, need)); break;
    case ORX_BUF_VCM_VERTICES: { /* four float4 planes [9][npx] -> [9][npx][16] */
        const size_t plane = r->vcm.npx * VCM_MAX_VERTS;
        std::vector<float4> P(4 * plane);
        HIPCHK(r, d2h(P.data(), r->vcm.vb.vA, 4 * plane * 16));
        float* o = (float*)dst;
        for (size_t i = 0; i < plane; i++)
            for (int k = 0; k < 4; k++) std::memcpy(o + 16 * i + 4 * k, &P[k * plane + i], 16);
        break;
    }
    case ORX_BUF_VCM_CAMERA_VERTEX_COUNT: HIPCHK(r, d2h(dst, r->mg.cvcount.p, need)); break;
    case ORX_BUF_VCM_CAMERA_VERTICES: { /* four float4 planes [cvmax][npx] -> [cvmax][npx][16] */
        const size_t plane = r->mg.mpx * r->vcm.vb.cvmax;
        std::vector<float4> P(4 * plane);
        HIPCHK(r, d2h(P.data(), r->mg.cverts.p, 4 * plane * 16));
        float* o = (float*)dst;
        for (size_t i = 0; i < plane; i++)
            for (int k = 0; k < 4; k++) std::memcpy(o + 16 * i + 4 * k, &P[k * plane + i], 16);
        break;
    }
    case ORX_BUF_VCM_MERGE: HIPCHK(r, d2h(dst, r->mg.merge.p, need)); break;
    case ORX_BUF_CONV_PREV: case ORX_BUF_CONV_SUM: case ORX_BUF_CONV_M2: { /* conv.stat: prev, A, M2 on padded planes */
        const size_t pad = (r->conv.npx + 3) & ~(size_t)3;
        const size_t at = id == ORX_BUF_CONV_PREV ? 0 : id == ORX_BUF_CONV_SUM ? 3 * pad : 4 * pad;
        if (need) HIPCHK(r, d2h(dst, r->conv.stat.as<float>() + at, need));
        break;
    }
    case ORX_BUF_CONV_ERROR: if (need) HIPCHK(r, d2h(dst, r->conv.err.p, need)); break;
    case ORX_BUF_VCM_MERGE_COUNT: case ORX_BUF_VCM_MERGE_CANDIDATES: { /* [npx][2]: accepted, candidates */
        std::vector<uint32_t> both(2 * r->mg.mpx);
        HIPCHK(r, d2h(both.data(), r->mg.count.p, both.size() * 4));
        uint32_t* o = (uint32_t*)dst;
        for (size_t i = 0; i < r->mg.mpx; i++) o[i] = both[2 * i + (id == ORX_BUF_VCM_MERGE_CANDIDATES ? 1 : 0)];
        break;
    }
    }
    return ORX_OK;
}


}  // extern "C"
