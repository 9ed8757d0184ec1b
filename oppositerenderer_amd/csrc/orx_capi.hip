/*
 * orx_capi.hip — host side of liborx.so: the OptixRenderer replacement.
 *
 * Owns the device buffers and sequences the passes of one progressive
 * iteration exactly as OptixRenderer::renderNextIteration does
 * (RenderEngine/renderer/OptixRenderer.cpp:507-821), but as plain HIP
 * launches on one stream: no OptiX context, no per-launch validation, no
 * debug-buffer maps (the reference maps ~36 MB of debug counters to the
 * host every PPM iteration, OptixRenderer.cpp:620/:872-953; here they stay
 * on the device and are summed in-kernel).
 *
 * This unit: configuration and lifecycle, orx_init_scene (BVH build, upload and binding of a scene that
 * orx_scene_host.cpp has validated and converted on the host), resize (the frame's counts and single buffers; the
 * buffer sets are sized in orx_host_ppm.hip), pass timing, stream flushes, the orx_render_next_iteration dispatch,
 * output getters and stats.  The PPM schedules are in orx_host_ppm.hip, VCM in orx_host_vcm.hip, orx_read_buffer in
 * orx_host_read.hip, checkpoints in orx_host_state.hip (a rank's share of a frame's rows: state_rank_rows, orx_state.cpp).
 */
#include <ctime>
#include <new>

#include "orx_bvh_host.h"
#include "orx_host.h"
#include "orx_state.h"

using namespace orx;

/* host float3 with the same OptiX semantics as the device (f3 is __host__) */
static f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }

static float dtor(float d) { return d * ((float)M_PI / 180.f); } /* Camera.cpp:87-90 */

DevCamera orx::camera_setup(const orx_camera& c, float* ulen_out, float* vlen_out) {
    /* Camera::setup (renderer/Camera.cpp:333-345) */
    DevCamera k;
    f3 eye = ld3(c.eye), lookat = ld3(c.lookat), up = ld3(c.up);
    k.eye = eye;
    k.lookdir = lookat - eye;
    float lookdir_len = length(k.lookdir);
    up = normalize(up);
    f3 cu = normalize(cross(k.lookdir, up));
    f3 cv = normalize(cross(cu, k.lookdir));
    float ulen = lookdir_len * tanf(dtor(c.hfov * 0.5f));
    k.u = cu * ulen;
    float vlen = lookdir_len * tanf(dtor(c.vfov * 0.5f));
    k.v = cv * vlen;
    k.aperture = c.aperture;
    if (ulen_out) *ulen_out = ulen;
    if (vlen_out) *vlen_out = vlen;
    return k;
}

static orx_status photon_stack_ensure(orx_renderer* r);

extern "C" {

void orx_default_config(orx_config* c) {
    std::memset(c, 0, sizeof *c);
    c->photon_launch_width = 1024;
    c->photon_launch_height = 1024;
    c->max_photon_deposits = 4;
    c->photon_grid_max_size = 100 * 100 * 100;
    c->max_photon_trace_depth = 7;
    c->max_radiance_trace_depth = 9;
    c->vcm_max_path_length = 10;
    c->seed = 0;
    c->debug_counters = 1;
    c->volumetric_photons = 200000; /* NUM_VOLUMETRIC_PHOTONS (config.h:35) */
}

/* stochastic hash: photonsSize = NUM_PHOTONS must be a power of two (getHashValue masks with
 * photonsSize - 1; OptixRenderer.cpp:46 "Ensure that NUM PHOTONS are a power of 2"), and a path's
 * deposits (one per non-specular hit at depth >= 1, never capped) fit the 8-bit deposit mask */
static bool hash_config_ok(const orx_config& c) {
    const uint64_t n = (uint64_t)c.photon_launch_width * c.photon_launch_height * c.max_photon_deposits;
    return n && n <= (1ull << 31) && (n & (n - 1)) == 0 && c.max_photon_trace_depth <= 9;
}

/* The deferred gather's stream at the highest priority (ORX_GATHER_PRIO=0: the lowest): at configs[4] (4K) the
 * gather stream is the frame's long pole (gather 23.7 ms serial, ~42 ms beside the next iteration's eye, photon
 * and grid passes, which need ~20 ms), and dispatching its workgroups first gains 1.8 % (552 -> 562 Mpaths/s,
 * 45.4 -> 44.6 ms); on the 1080p hall the frame is unchanged (1014 / 1014 Mpaths/s)
 * (profiles/r06i_gather_priority_ab.txt) */
static int gather_stream_priority() {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
    static const bool high = [] {
        const char* e = getenv("ORX_GATHER_PRIO");
        return !(e && atoi(e) == 0);
    }();
    return high ? greatest : least;
}

/* the asynchronous grid build's stream: the gather's priority, or the least (ORX_GRIDQ_PRIO=0) */
static int grid_stream_priority() {
    static const bool low = [] {
        const char* e = getenv("ORX_GRIDQ_PRIO");
        return e && atoi(e) == 0;
    }();
    int least = 0, greatest = 0;
    if (low && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) return least;
    return gather_stream_priority();
}

/* the events that order the renderer's streams (no timing): created and destroyed with it */
static std::vector<hipEvent_t*> order_events(orx_renderer* r) {
    orx::PpmPipe& p = r->pipe;
    return {&r->gasync.ev_gsrc[0], &r->gasync.ev_gsrc[1], &p.ev_grid_done, &p.ev_gdone[0], &p.ev_gdone[1], &p.ev_gdone[2],
            &p.ev_photon_done, &p.ev_direct_done, &p.ev_eye_done, &r->vcm.ev_cam, &r->vcm.ev_acc, &p.ev_main};
}

orx_status orx_create(int hip_device, const orx_config* cfg, orx_renderer** out) {
    if (!out) return ORX_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    orx_config c;
    if (cfg) c = *cfg;
    else orx_default_config(&c);
    if (c.max_photon_deposits == 0 || c.max_photon_deposits > 8 || c.photon_launch_width == 0 ||
        c.photon_launch_height == 0 || c.photon_grid_max_size == 0 || c.photon_grid_max_size > (1u << 26) ||
        c.gather_variant > 2 || c.photon_map > 2 || c.vcm_merging > 1 || (c.photon_map == 1 && !hash_config_ok(c)) ||
        (c.photon_map == 2 && (uint64_t)c.photon_launch_width * c.photon_launch_height * c.max_photon_deposits >
                                  (1ull << 28)))
        return ORX_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ORX_ERR_DEVICE;
    if (hip_device < 0 || hip_device >= n) return ORX_ERR_INVALID_ARGUMENT;
    orx_renderer* r = new (std::nothrow) orx_renderer();
    if (!r) return ORX_ERR_OUT_OF_MEMORY;
    r->device = hip_device;
    r->cfg = c;
    if (hipSetDevice(hip_device) != hipSuccess ||
        hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&r->aux, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&r->gstream, hipStreamNonBlocking, gather_stream_priority()) != hipSuccess ||
        hipStreamCreateWithPriority(&r->gridq, hipStreamNonBlocking, grid_stream_priority()) != hipSuccess) {
        orx_destroy(r);
        return ORX_ERR_DEVICE;
    }
    for (hipEvent_t* e : order_events(r))
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
            orx_destroy(r);
            return ORX_ERR_DEVICE;
        }
    *out = r;
    return ORX_OK;
}

void orx_destroy(orx_renderer* r) {
    if (!r) return;
    hipSetDevice(r->device);
    /* every stream first: the pass timing events are recorded on all of them */
    for (hipStream_t s : {r->stream, r->aux, r->gstream, r->gridq})
        if (s) hipStreamSynchronize(s);
    for (int p = 0; p < P_COUNT; p++)
        for (hipEvent_t e : r->timing.ev[p]) hipEventDestroy(e);
    for (hipEvent_t* e : order_events(r))
        if (*e) hipEventDestroy(*e);
    for (hipEvent_t e : r->gasync.ev_pm) /* the schedule probe's, created with the second output set */
        if (e) hipEventDestroy(e);
    for (hipStream_t s : {r->gstream, r->gridq, r->aux, r->stream})
        if (s) hipStreamDestroy(s);
    delete r;
}

const char* orx_last_error(const orx_renderer* r) { return r ? r->err.c_str() : "null renderer"; }
void* orx_stream(orx_renderer* r) { return r ? (void*)r->stream : nullptr; }

orx_status orx_set_shard(orx_renderer* r, uint32_t rank, uint32_t world) {
    if (!r || world == 0 || rank >= world) return ORX_ERR_INVALID_ARGUMENT;
    if (world > 1 && r->cfg.enable_media)
        return set_err(r, ORX_ERR_UNSUPPORTED, "participating media are single-device");
    if (world > 1 && r->cfg.photon_map == 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "the stochastic hash photon map is single-device (one table per iteration)");
    r->rank = rank;
    r->world = world;
    r->rng_ready = false; /* force re-allocation of the local rows */
    return ORX_OK;
}

orx_status orx_init_scene(orx_renderer* r, const orx_scene* s) {
    if (!r || !s) return ORX_ERR_INVALID_ARGUMENT;
    const orx_status st = scene_validate(s, r->cfg, r->world, &r->err);
    return st == ORX_OK ? init_scene_checked(r, *s) : st;
}

}  // extern "C"

static hipError_t up(DevBuf& b, const void* src, size_t bytes) {
    hipError_t e = b.ensure(bytes);
    if (e != hipSuccess) return e;
    if (bytes) return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    return hipSuccess;
}
template <class T>
static hipError_t up(DevBuf& b, const std::vector<T>& v) {
    return up(b, v.data(), v.size() * sizeof(T));
}

/* everything of the scene but the BVH nodes: primitives, materials, lights, the triangle attributes in leaf
 * order, and the texture images back to back with their descriptors */
hipError_t SceneBufs::upload(const orx_scene& s, const HostScene& h, const LeafArrays& la, const TextureLayout& tl) {
    hipError_t e;
#define UP(...)                                     \
    if ((e = up(__VA_ARGS__)) != hipSuccess) return e
    UP(quads, h.quads);
    UP(qmat, s.quad_material, (size_t)s.n_quads * 4);
    UP(spheres, h.spheres);
    UP(smat, s.sphere_material, (size_t)s.n_spheres * 4);
    UP(triv, la.v);
    UP(trin, la.n);
    UP(tmat, la.mat);
    UP(mats, h.mats);
    UP(triuv, la.uv);
    UP(trit, la.t);
    UP(tribt, la.bt);
    if ((e = texels.ensure(tl.total)) != hipSuccess) return e;
    std::vector<DevTexture> texd(s.n_textures);
    uint8_t* base = texels.as<uint8_t>();
    for (uint32_t i = 0; i < s.n_textures; i++) {
        const orx_texture& t = s.textures[i];
        DevTexture& d = texd[i];
        std::memset(&d, 0, sizeof d);
        d.w = t.width;
        d.h = t.height;
        d.rgba = base + tl.rgba[i];
        e = hipMemcpy(base + tl.rgba[i], t.rgba, (size_t)t.width * t.height * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        if (t.normal_rgba) {
            d.nw = t.normal_width;
            d.nh = t.normal_height;
            d.nrgba = base + tl.normal[i];
            e = hipMemcpy(base + tl.normal[i], t.normal_rgba, (size_t)t.normal_width * t.normal_height * 4,
                          hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
        }
    }
    UP(texdesc, texd);
    UP(lights, h.lights);
#undef UP
    return hipSuccess;
}

/* orx_init_scene behind scene_validate: prepare, BVH build, leaf arrays, upload, bind.  Nothing of the renderer
 * is written before the scene is prepared, and scene_ready is false from the first device write to the end: a
 * failure in between leaves no scene (the next iteration is refused), never the old scene's numbers over the
 * new scene's buffers. */
orx_status orx::init_scene_checked(orx_renderer* r, const orx_scene& s) {
    const uint32_t nt = s.n_triangles;
    const HostScene h = scene_prepare(s, r->cfg);
    const TextureLayout tl = scene_texture_layout(s);
    HIPCHK(r, hipSetDevice(r->device));
    {
        orx_status s0 = sync_all(r); /* in-flight passes read the scene being replaced */
        if (s0 != ORX_OK) return s0;
    }
    r->scene_ready = false;
    SceneBufs& sb = r->sb;
    /* triangles: BVH over triangle boxes, then vertex / normal / material
     * arrays rewritten in leaf order (tri_v[3k].w carries the original id) */
    /* BVH: built on the device (orx_bvh.hip) by default; the host builder
     * (orx_bvh_host.cpp) is the reference implementation (ORX_BVH_HOST=1) and
     * the only one for the fp32-box variant */
    const BvhBuildOptions bvh_opt = bvh_options_from_env();
#ifdef ORX_BVH_FP32
    const bool device_bvh = false;
#else
    const char* host_env = getenv("ORX_BVH_HOST");
    const bool device_bvh = !(host_env && atoi(host_env));
#endif
    std::vector<uint32_t> leaf_order;
    uint32_t stack_bound = 0, nodes4 = 0;
    HostBvh4 hb;
    if (nt && device_bvh) {
        DevBuf dV, dI;
        HIPCHK(r, dV.ensure((size_t)s.n_vertices * 12));
        HIPCHK(r, dI.ensure((size_t)nt * 12));
        HIPCHK(r, hipMemcpy(dV.p, s.vertices, (size_t)s.n_vertices * 12, hipMemcpyHostToDevice));
        HIPCHK(r, hipMemcpy(dI.p, s.triangles, (size_t)nt * 12, hipMemcpyHostToDevice));
        HIPCHK(r, sb.bvh.ensure((size_t)nt * sizeof(DevBvh4) + 64));
        HIPCHK(r, sb.bvhprims.ensure((size_t)nt * 4));
        uint32_t depth = 0;
        bool ok = false;
        HIPCHK(r, device_build_bvh4(r->stream, dV.as<float>(), dI.as<uint32_t>(), nt, bvh_opt, sb.bvh.as<DevBvh4>(), nt,
                                    sb.bvhprims.as<uint32_t>(), &nodes4, &stack_bound, &depth, &ok));
        if (!ok) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "device BVH build failed (quantisation or capacity)");
        if (depth >= ORX_BVH_STACK) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "BVH deeper than the traversal stack");
        leaf_order.resize(nt);
        HIPCHK(r, hipMemcpy(leaf_order.data(), sb.bvhprims.p, (size_t)nt * 4, hipMemcpyDeviceToHost));
    } else if (nt) {
        if (const char* msg = build_host_bvh4(s.vertices, s.triangles, nt, bvh_opt, &hb))
            return set_err(r, ORX_ERR_INVALID_ARGUMENT, msg);
        leaf_order.swap(hb.leaf_order);
        stack_bound = hb.stack_bound;
        nodes4 = (uint32_t)hb.nodes.size();
    }
    if (stack_bound > 96) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "BVH4 traversal stack bound above 96");
    LeafArrays la;
    {
        const orx_status st = scene_leaf_arrays(s, leaf_order.data(), nt, &la, &r->err);
        if (st != ORX_OK) return st;
    }
    HIPCHK(r, sb.upload(s, h, la, tl));
#ifdef ORX_BVH_FP32
    HIPCHK(r, up(sb.bvh, hb.nodes_f));
#else
    if (!device_bvh) HIPCHK(r, up(sb.bvh, hb.nodes));
#endif
    r->media.on = h.media;
    r->media.vm = VolMap{};
    if (h.media) {
        r->media.vm.on = 1;
        r->media.vm.lo = h.med_lo;
        r->media.vm.hi = h.med_hi;
        r->media.vm.sig_s = h.sig_s;
        r->media.vm.sig_a = h.sig_a;
        const uint32_t NV = r->cfg.volumetric_photons;
        HIPCHK(r, r->media.cnt.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.win.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.A.ensure((size_t)NV * 16));
        HIPCHK(r, r->media.B.ensure((size_t)NV * 16));
        HIPCHK(r, r->media.keys.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.vals.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.keys2.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.vals2.ensure((size_t)NV * 4));
        HIPCHK(r, r->media.sort.ensure(vol_sort_tmp_bytes(NV) + 256));
        HIPCHK(r, r->media.rec.ensure((size_t)NV * 32 + 32));
    }
    const bool has_tb = !la.t.empty();
    DevScene& S = r->scene;
    S.nq = s.n_quads;
    S.ns = s.n_spheres;
    S.nt = nt;
    S.quads = sb.quads.as<DevQuad>();
    S.qmat = sb.qmat.as<uint32_t>();
    S.spheres = sb.spheres.as<DevSphere>();
    S.smat = sb.smat.as<uint32_t>();
    S.tri_v = sb.triv.as<float4>();
    S.tri_n = s.normals ? sb.trin.as<float4>() : nullptr;
    S.tmat = sb.tmat.as<uint32_t>();
    S.tri_uv = s.texcoords && nt ? sb.triuv.as<float2>() : nullptr;
    S.tri_t = has_tb ? sb.trit.as<float4>() : nullptr;
    S.tri_bt = has_tb ? sb.tribt.as<float4>() : nullptr;
    S.tex = sb.texdesc.as<DevTexture>();
    S.ntex = s.n_textures;
    S.mats = sb.mats.as<DevMaterial>();
    r->n_mats = s.n_materials;
    r->has_tex = h.has_tex;
    S.lights = sb.lights.as<DevLight>();
    S.nl = s.n_lights;
    r->host_lights = h.lights;
    S.bvh4 = sb.bvh.as<DevNode4>();
    S.bvh_nodes = nodes4;
    S.stack_entries = nt ? stack_bound + 1 : 0;
    S.dir_zero = h.dir_zero;
#ifdef ORX_TRAV_STATS
    HIPCHK(r, r->vcm.tstats.ensure(256));
    HIPCHK(r, hipMemset(r->vcm.tstats.p, 0, 256));
    S.trav_stats = r->vcm.tstats.as<unsigned long long>();
#else
    S.trav_stats = nullptr;
#endif
    r->aabb_lo = h.aabb_lo;
    r->aabb_hi = h.aabb_hi;
    S.bs_cx = h.bs_cx;
    S.bs_cy = h.bs_cy;
    S.bs_cz = h.bs_cz;
    S.bs_r = h.bs_r;
    r->vcm.estimated = false;
    r->note.scene_key = orx_scene_key(&s);
    r->note.have = false;
    r->scene_ready = true;
    return photon_stack_ensure(r);
}

extern "C" {

/* the photon pass's deep traversal-stack entries: (stack bound + 2 - its LDS entries) per photon of
 * the device (1.4 GB for 4096^2 photons on the conference room; touched only by paths whose stack
 * outgrows LDS); sized again whenever a scene or a resize comes in */
static orx_status photon_stack_ensure(orx_renderer* r) {
    const size_t lanes = ((size_t)r->pb.prows * r->pb.PW + 63) / 64 * 64;
    const uint32_t deep = photon_stack_deep(r->scene.stack_entries);
    HIPCHK(r, r->gs.ptrav.ensure(256 + (size_t)deep * lanes * 4));
    r->pb.tstk = r->gs.ptrav.as<uint32_t>();
    r->pb.tlanes = (uint32_t)lanes;
    r->pb.tdeep = deep;
    return ORX_OK;
}

/* every count the frame's buffers are sized by, from the configuration and the rows resize has just set */
static FrameSizes frame_sizes(const orx_renderer* r) {
    const orx_config& c = r->cfg;
    const uint32_t PW = c.photon_launch_width, PH = c.photon_launch_height;
    FrameSizes f;
    /* slots per emitted photon: the deposit limit (uniform grid), or room for every non-specular
     * hit at depth 1..max depth - 1 (stochastic hash: store_photon.h never counts deposits) */
    f.D = c.photon_map == 1 ? std::min(c.max_photon_trace_depth, 8u) : c.max_photon_deposits;
    f.nhp = (size_t)r->max_rows * r->W; /* hitpoint planes padded to max_rows */
    f.nslot_rng = (size_t)r->rng_rows * r->RW;
    f.nphot = (size_t)r->prows * PW;
    f.S = f.nphot * f.D;
    /* slab mode: room for every deposit slot of the global launch (the photons this rank imports) */
    f.S_cap = r->slab.on ? std::max(f.S, (size_t)PW * PH * f.D) : f.S;
    f.G2 = (size_t)c.photon_grid_max_size + 2;
    /* 64 photons of tail padding per plane: the union gather loads whole 64-photon chunks, up to
     * index U1 + 63 of the last plane */
    f.splane = ((f.S_cap + 64) + 3) & ~(size_t)3;
    /* bucket-sort grid build: at most 2048 buckets of 2^bshift virtual cells
     * (nsub sub-rows per cell row, k_bs_count) */
    /* sub-row layout on one device; a row-partition shard of world >= 2 gathers all W*H hit points
     * against 1/N of the photons and runs faster on whole cell rows (tools/shard_model.py, hall
     * 1080p: per-rank gather N=2 1.40 -> 1.32 ms, N=8 0.96 -> 0.90 ms, grid build shorter too);
     * a slab shard holds the single-device photon density in its cells: sub-rows (configs[4]
     * N=2 rank 0: 47 ms gather in cell order) */
    const bool cell_order = c.gather_variant == 1 || (c.gather_variant == 0 && r->world >= 2 && !r->slab.on);
    f.nsub = cell_order ? 1u : SUBR * SUBR;
    const size_t vmax = (size_t)c.photon_grid_max_size * f.nsub;
    f.bshift = 10;
    while (((vmax + (1u << f.bshift) - 1) >> f.bshift) > 2048) f.bshift++;
    f.bs_nchunk = (f.S + 16383) / 16384;
    f.bs_nchunk_cap = (f.S_cap + 16383) / 16384;
    f.bs_nbmax = (vmax + (1u << f.bshift) - 1) >> f.bshift;
    f.bs_nscan = (f.bs_nbmax * f.bs_nchunk_cap + 1023) / 1024;
    if (c.photon_map == 1) f.hnum = (size_t)PW * PH * c.max_photon_deposits; /* NUM_PHOTONS */
    if (c.photon_map == 2) {
        /* m_photonKdTreeSize = pow2roundup(NUM_PHOTONS + 1) - 1 (OptixRenderer.cpp:65-74, :207) */
        uint32_t t = (uint32_t)f.S;
        t |= t >> 1;
        t |= t >> 2;
        t |= t >> 4;
        t |= t >> 8;
        t |= t >> 16;
        f.tree = (size_t)t; /* pow2roundup(S + 1) - 1 */
        while (((size_t)1 << f.levels) - 1 < f.tree) f.levels++;
        f.nblk = (f.S + 1023) / 1024;
        f.ntiles = (f.S + 4095) / 4096;
        f.tp = std::max((256 * f.ntiles + 1023) / 1024, (6 * f.nblk + 1023) / 1024) + 16;
    }
    return f;
}

/* The frame's buffers for a W x H image: everything single, and the first buffer set and photon
 * output set, which become the current ones (the further sets: ensure_second_set) */
static orx_status resize(orx_renderer* r, uint32_t W, uint32_t H, bool seed_rng = true) {
    r->pipe.pp = r->gasync.po = 0;
    const uint32_t PW = r->cfg.photon_launch_width, PH = r->cfg.photon_launch_height;
    const bool hash = r->cfg.photon_map == 1;
    r->fin.due = r->fin.snap = false; /* a finish held back across a resize is dropped with its buffers */
    r->W = W;
    r->H = H;
    r->RW = std::max(PW, W);
    r->RH = std::max(PH, H);
    r->rows = state_rank_rows(H, r->rank, r->world);
    r->rng_rows = state_rank_rows(r->RH, r->rank, r->world);
    r->prows = state_rank_rows(PH, r->rank, r->world);
    r->max_rows = (H + r->world - 1) / r->world;
    const FrameSizes& f = r->fs = frame_sizes(r);
    if ((size_t)SP_PLANES * f.splane * 4 > 0xffffff00ull) /* the gather addresses the planes with 32-bit buffer offsets */
        return set_err(r, ORX_ERR_UNSUPPORTED, "photon slots per device exceed the 4 GiB sorted-photon window");
    HIPCHK(r, r->d_rng.ensure(f.nslot_rng * 24));
    HIPCHK(r, r->d_ind.ensure(f.nhp * 12));
    HIPCHK(r, r->d_out.ensure(f.nhp * 12));
    HIPCHK(r, r->d_dbg.ensure(f.nhp * 8));
    if (r->media.on) { /* volumetricRadiance per pixel, last volumetric event per photon */
        HIPCHK(r, r->media.volR.ensure(f.nhp * 12));
        HIPCHK(r, r->media.ev_a.ensure(f.nphot * 16 + 16));
        HIPCHK(r, r->media.ev_b.ensure(f.nphot * 16 + 16));
        HIPCHK(r, hipMemsetAsync(r->media.volR.p, 0, f.nhp * 12, r->stream));
        r->media.vm.valid = 0;
    }
    HIPCHK(r, r->gs.perm.ensure(f.S_cap * 4 + 16));
    HIPCHK(r, r->gs.keys.ensure(f.S_cap * 4));
    HIPCHK(r, r->gs.bstable.ensure(f.bs_nbmax * f.bs_nchunk_cap * 4 + 16));
    HIPCHK(r, r->gs.bspartials.ensure((f.bs_nscan + 2) * 4));
    HIPCHK(r, r->gs.bspairs.ensure(f.S_cap * 8 + 16));
    HIPCHK(r, hipMemsetAsync(r->d_out.p, 0, f.nhp * 12, r->stream));
    {
        orx_status st = size_ppm_set(r, r->pipe.set[0], 0);
        if (st == ORX_OK) st = size_photon_out(r, r->gasync.out[0]);
        if (st != ORX_OK) return st;
    }
    /* the second buffer set of PPM pipelining is allocated on the first pipelined iteration
     * (ensure_second_set); the sharded pipeline (orx_set_ppm_pipeline) wants it at once */
    r->pipe.bufs = r->pipe.gather_in_flight = false;

    PixelBufs& px = r->px;
    px.W = W;
    px.H = H;
    px.rank = r->rank;
    px.world = r->world;
    px.rows = r->rows;
    px.RW = r->RW;
    for (int k = 0; k < 6; k++) px.rng.p[k] = r->d_rng.as<uint32_t>() + k * f.nslot_rng;
    px.seg_rows = r->max_rows;
    px.indirect = r->d_ind.as<float>();
    px.output = r->d_out.as<float>();
    px.dbg = r->cfg.debug_counters ? r->d_dbg.as<uint32_t>() : nullptr;
    PhotonBufs& pb = r->pb;
    pb.PW = PW;
    pb.PH = PH;
    pb.prows = r->prows;
    pb.D = f.D;
    pb.S = (uint32_t)f.S;
    pb.hash = hash ? 1u : 0u;
    pb.Dlim = hash ? 0xffffffffu : f.D;
    pb.hnum = (uint32_t)f.hnum;
    {
        orx_status st = photon_stack_ensure(r);
        if (st == ORX_OK && r->cfg.photon_map == 2) st = kd_resize(r);
        if (st != ORX_OK) return st;
    }
    pb.gmax = r->cfg.photon_grid_max_size;
    /* ORX_SHARD_CELLS=2: a row shard of world N sizes its cells for gmax / N cells (N times the
     * single-device volume, the single-device photons per cell; the accepted set does not depend on
     * the cell size).  Measured slower (tools/shard_model.py, N = 8: configs[4] per-rank gather
     * 5.96 -> 8.43 ms in cell order, 5.82 -> 6.24 ms on sub-rows; hall 0.42 ms either way): a
     * window of radius r ~ one single-device cell then walks 2^3 cells of twice the edge, about 2.4x
     * the volume of the 3^3 it walks otherwise, so the default keeps single-device cells */
    {
        static const int scaled = [] {
            const char* e = getenv("ORX_SHARD_CELLS");
            return e && atoi(e) == 2 ? 1 : 0;
        }();
        pb.gcells = (r->world >= 2 && !r->slab.on && scaled) ? std::max(1u, pb.gmax / r->world) : pb.gmax;
    }
    pb.splane = (uint32_t)f.splane;
    pb.perm = r->gs.perm.as<uint32_t>();
    pb.keys = r->gs.keys.as<uint32_t>();
    pb.bshift = f.bshift;
    pb.nsub = f.nsub;
    pb.bs_nchunk = (uint32_t)f.bs_nchunk;
    pb.bs_table = r->gs.bstable.as<uint32_t>();
    pb.bs_partials = r->gs.bspartials.as<uint32_t>();
    pb.bs_pairs = r->gs.bspairs.as<uint2>();
    bind_ppm_views(r);

    /* initializeRandomStates (OptixRenderer_SpatialHash.cu:310-347) */
    if (seed_rng) {
        uint32_t seed = r->cfg.seed;
        if (seed == 0) seed = 574133u * (uint32_t)clock() + (uint32_t)(47844152748ull * (uint32_t)time(NULL));
        launch_rng_init(r->stream, px.rng, r->RW, r->rng_rows, r->rank, r->world, seed);
    }
    HIPCHK(r, hipGetLastError());
    r->rng_ready = true;
    return conv_resized(r); /* the sum was cleared above: a new statistics window */
}

}  // extern "C"

orx_status orx::resize_unseeded(orx_renderer* r, uint32_t W, uint32_t H) { return resize(r, W, H, false); }

/* roctx ranges around every pass (the role of the reference's NVTX ranges,
 * renderer/helpers/nsight.h:17-199): visible in `rocprofv3 --marker-trace`;
 * they span the host-side enqueue, the HIP events above time the device work */
static const char* const PASS_NAME[P_COUNT] = {
    "OptixEntryPoint::RAYTRACE_PASS (ppm_eye)",   "OptixEntryPoint::PHOTON_PASS (ppm_photon)",
    "Creating photon map (grid_hash)",            "Creating photon map (grid_scan)",
    "Creating photon map (grid_scatter)",         "OptixEntryPoint::INDIRECT_RADIANCE_ESTIMATION (ppm_gather)",
    "OptixEntryPoint::PPM_DIRECT_RADIANCE_ESTIMATION_PASS (ppm_direct_output)",
    "OptixEntryPoint::PT_RAYTRACE_PASS (pt)",     "OptixEntryPoint::VCM_LIGHT_PASS (vcm_light)",
    "OptixEntryPoint::VCM_CAMERA_PASS (vcm_camera)", "OptixEntryPoint::VCM_CAMERA_PASS (vcm_shadow)",
    "VCM vertex merging (vcm_grid)",              "VCM vertex merging (vcm_merge)",
    "Convergence statistics (convergence)"};
void orx::ev_begin(orx_renderer* r, int p, hipStream_t st) {
    roctxRangePushA(PASS_NAME[p]);
    if (!r->timing.on || r->timing.ev_n[p] >= EV_POOL) return;
    auto& v = r->timing.ev[p];
    while (v.size() < 2 * (size_t)r->timing.ev_n[p] + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        v.push_back(e);
    }
    hipEventRecord(v[2 * r->timing.ev_n[p]], st);
}
void orx::ev_end(orx_renderer* r, int p, hipStream_t st) {
    roctxRangePop();
    if (!r->timing.on || r->timing.ev_n[p] >= EV_POOL || r->timing.ev[p].size() < 2 * (size_t)r->timing.ev_n[p] + 2) return;
    hipEventRecord(r->timing.ev[p][2 * r->timing.ev_n[p] + 1], st);
    r->timing.ev_n[p]++;
}

/* order everything later on the renderer's stream (and the gather stream) after a VCM camera
 * pass's resolve half still running on aux */
void orx::flush_vcm(orx_renderer* r) {
    if (!r->vcm.resolve_in_flight) return;
    hipStreamWaitEvent(cur_stream(r), r->vcm.ev_acc, 0);
    if (r->gstream) hipStreamWaitEvent(r->gstream, r->vcm.ev_acc, 0);
    r->vcm.resolve_in_flight = false;
}
/* order everything later on the renderer's stream after a deferred gather + output */
void orx::flush_pipeline(orx_renderer* r) {
    flush_vcm(r);
    r->pipe.eye_chain = false;
    if (!r->pipe.gather_in_flight) return;
    hipStreamWaitEvent(cur_stream(r), r->pipe.ev_gdone[r->pipe.pp], 0);
    r->pipe.gather_in_flight = false;
}

orx_status orx::sync_all(orx_renderer* r) {
    flush_pipeline(r);
    HIPCHK(r, hipStreamSynchronize(r->stream));
    HIPCHK(r, hipStreamSynchronize(r->aux));
    if (r->use_ext) HIPCHK(r, hipStreamSynchronize(r->ext_stream));
    if (r->gstream) HIPCHK(r, hipStreamSynchronize(r->gstream));
    if (r->gridq) HIPCHK(r, hipStreamSynchronize(r->gridq));
    if (r->fin.shard_pipe) HIPCHK(r, hipStreamSynchronize(r->fin.side));
    return ORX_OK;
}

Consts orx::make_consts(orx_renderer* r, float ppm_radius, uint64_t local_iteration_number) {
    Consts c;
    c.max_photon_depth = r->cfg.max_photon_trace_depth;
    c.max_radiance_depth = r->cfg.max_radiance_trace_depth;
    c.ppm_radius = ppm_radius;
    c.ppm_radius2 = ppm_radius * ppm_radius;
    /* emittedPhotonsPerIterationFloat: global launch (all ranks) */
    c.emitted_f = (float)(r->cfg.photon_launch_width * r->cfg.photon_launch_height);
    c.local_iteration = (uint32_t)(local_iteration_number != 0);
    c.media = r->media.on ? 1u : 0u;
    return c;
}

/* resize / RNG init / output clear common to every method (OptixRenderer.cpp:531-557) */
orx_status orx::begin_iteration(orx_renderer* r, uint64_t local_iteration_number, const orx_request* det, bool pipelined,
                                bool vcm_overlap) {
    if (!r->scene_ready) return set_err(r, ORX_ERR_STATE, "Traced before OptixRenderer was initialized.");
    if (det->width == 0 || det->height == 0) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "zero-sized request");
    HIPCHK(r, hipSetDevice(r->device));
    if (det->width != r->W || det->height != r->H) { /* resizeBuffers (OptixRenderer.cpp:826-848) */
        r->vcm.psf_x = 1.0f / (float)det->width;
        r->vcm.psf_y = 1.0f / (float)det->height;
        r->vcm.estimated = false;
    }
    if (det->width != r->W || det->height != r->H || !r->rng_ready) {
        orx_status s0 = sync_all(r); /* nothing in flight may touch the buffers being replaced */
        if (s0 != ORX_OK) return s0;
        orx_status st = resize(r, det->width, det->height);
        if (st != ORX_OK) return st;
        if (r->use_ext) HIPCHK(r, hipStreamSynchronize(r->stream)); /* resize work ran on the own stream */
    }
    /* an overlapped VCM iteration leaves the last resolve running: its light pass may start beside it */
    if (!(vcm_overlap && local_iteration_number != 0)) flush_vcm(r);
    if (!pipelined) {
        if (vcm_overlap) {
            r->pipe.eye_chain = false;
            if (r->pipe.gather_in_flight) HIPCHK(r, hipStreamWaitEvent(cur_stream(r), r->pipe.ev_gdone[r->pipe.pp], 0));
            r->pipe.gather_in_flight = false;
        } else {
            flush_pipeline(r);
        }
    }
    r->timing.iterations++;
    conv_begin(r, local_iteration_number);
    /* the output accumulates on the gather stream when pipelined (after the previous output) */
    if (local_iteration_number == 0)
        HIPCHK(r, hipMemsetAsync(r->d_out.p, 0, (size_t)r->max_rows * r->W * 12, pipelined ? gather_stream(r) : cur_stream(r)));
    return ORX_OK;
}

extern "C" {

static orx_status render_next_iteration(orx_renderer* r, uint64_t local_iteration_number, float ppm_radius,
                                        const orx_request* det);
orx_status orx_render_next_iteration(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                                     float ppm_radius, int create_output, const orx_request* det) {
    (void)create_output; /* ignored by the reference engine too */
    if (!r || !det) return ORX_ERR_INVALID_ARGUMENT;
    char range[48]; /* OptixRenderer.cpp:518-520 */
    snprintf(range, sizeof range, "OptixRenderer::Trace Iteration %llu", (unsigned long long)iteration_number);
    roctxRangePushA(range);
    const orx_status st = render_next_iteration(r, local_iteration_number, ppm_radius, det);
    if (st == ORX_OK) note_iteration(r, iteration_number, local_iteration_number, ppm_radius, det->method);
    roctxRangePop();
    return st;
}
static orx_status render_next_iteration(orx_renderer* r, uint64_t local_iteration_number, float ppm_radius,
                                        const orx_request* det) {
    if (det->method != ORX_METHOD_PATH_TRACING && det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING &&
        det->method != ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING)
        return set_err(r, ORX_ERR_UNSUPPORTED, "render method not supported by this build");
    if (det->method == ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING && r->world > 1)
        return set_err(r, ORX_ERR_STATE, "sharded VCM runs through orx_vcm_local_light/orx_export_vcm_splats/orx_vcm_finish");
    if (det->method == ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING && vcm_check_lights(r) != ORX_OK)
        return ORX_ERR_UNSUPPORTED;
    if (det->method == ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING && r->world > 1)
        return set_err(r, ORX_ERR_STATE, "sharded PPM runs through orx_ppm_local_passes/_gather_external/_finish");
    if (r->media.on && det->method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING)
        return set_err(r, ORX_ERR_UNSUPPORTED, "participating media: progressive photon mapping only");
    if (r->media.on && r->cfg.photon_map == 1)
        return set_err(r, ORX_ERR_UNSUPPORTED, "participating media: uniform grid or kd-tree photon map");
    static const int pipeline_env = [] {
        const char* e = getenv("ORX_PIPELINE");
        return e ? atoi(e) : 1;
    }();
    const int pipe_on = r->pipe.mode >= 0 ? r->pipe.mode : pipeline_env;
    const bool pipelined = pipe_on && det->method == ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING && r->world == 1 &&
                           !r->use_ext && !r->media.on;
    /* VCM: the camera pass's resolve half beside the next light pass (ORX_VCM_OVERLAP=0: serial) */
    static const int vcm_overlap_env = [] {
        const char* e = getenv("ORX_VCM_OVERLAP");
        return e ? atoi(e) : 1;
    }();
    const bool vcm_overlap = pipe_on && vcm_overlap_env && det->method == ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING &&
                             r->world == 1 && !r->use_ext && !r->cfg.vcm_merging;
    orx_status s0 = begin_iteration(r, local_iteration_number, det, pipelined, vcm_overlap);
    r->vcm.last_overlap = false;
    if (s0 != ORX_OK) return s0;
    if (pipelined && (s0 = ensure_second_set(r)) != ORX_OK) return s0;
    r->pipe.last_pipelined = pipelined && r->pipe.bufs;
    if (r->pipe.last_pipelined) return ppm_pipelined_iteration(r, det, ppm_radius, local_iteration_number);
    if (pipelined) flush_pipeline(r);
    DevCamera cam = camera_setup(det->camera);
    Consts c = make_consts(r, ppm_radius, local_iteration_number);
    orx_status s = ORX_OK;
    if (det->method == ORX_METHOD_PATH_TRACING) {
        ev_begin(r, P_PT);
        launch_pt(cur_stream(r), r->scene, cam, r->px, c);
        ev_end(r, P_PT);
    } else if (det->method == ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING) {
        s = vcm_iteration(r, det, ppm_radius, vcm_overlap);
    } else {
        s = ppm_serial_iteration(r, cam, c);
    }
    if (s != ORX_OK) return s;
    /* the statistics behind the iteration's last write to the sum (an overlapped VCM resolve has its own) */
    if (!r->vcm.last_overlap) conv_update(r, cur_stream(r), r->conv.it);
    HIPCHK(r, hipGetLastError());
    r->last_method = (uint64_t)det->method;
    r->last_consts = c;
    return ORX_OK;
}

orx_status orx_set_stream(orx_renderer* r, void* stream, int use_external) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    r->use_ext = use_external != 0;
    r->ext_stream = (hipStream_t)stream;
    return ORX_OK;
}
uint32_t orx_local_rows(const orx_renderer* r) { return r ? r->rows : 0; }
uint32_t orx_max_local_rows(const orx_renderer* r) { return r ? (r->H + r->world - 1) / r->world : 0; }
size_t orx_hitpoint_export_bytes(const orx_renderer* r) {
    return r ? hp_export_plane((size_t)((r->H + r->world - 1) / r->world) * r->W) * 28 : 0;
}

static orx_status check_grid_error(orx_renderer* r) {
    const DevBuf& grid = r->pipe.set[r->pipe.pp].grid;
    if (r->last_method != ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING || !grid.p) return ORX_OK;
    GridParams g;
    orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    HIPCHK(r, hipMemcpy(&g, grid.p, sizeof g, hipMemcpyDeviceToHost));
    if (g.error)
        return set_err(r, ORX_ERR_GRID_TOO_LARGE, "Too many cells in SpatialHash.cu, over defined PHOTON_GRID_MAX_SIZE.");
    return ORX_OK;
}

orx_status orx_get_output(orx_renderer* r, float* dst, size_t bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    size_t need = (size_t)r->rows * r->W * 12;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    if (!r->d_out.p) return set_err(r, ORX_ERR_STATE, "no frame rendered yet");
    HIPCHK(r, hipSetDevice(r->device));
    orx_status s0 = sync_all(r);
    if (s0 != ORX_OK) return s0;
    HIPCHK(r, hipMemcpy(dst, r->d_out.p, need, hipMemcpyDeviceToHost));
    return check_grid_error(r);
}

orx_status orx_get_output_device(orx_renderer* r, void* dst, size_t bytes) {
    if (!r || !dst) return ORX_ERR_INVALID_ARGUMENT;
    size_t need = (size_t)r->rows * r->W * 12;
    if (bytes < need) return set_err(r, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    if (!r->d_out.p) return set_err(r, ORX_ERR_STATE, "no frame rendered yet");
    HIPCHK(r, hipSetDevice(r->device));
    /* after the last pipelined output pass; the pipeline itself stays unbroken (the copy only
     * reads the running sum, which the next output pass, on the gather stream after the grid
     * build that follows this copy on the main stream, writes) */
    if (r->pipe.gather_in_flight) HIPCHK(r, hipStreamWaitEvent(cur_stream(r), r->pipe.ev_gdone[r->pipe.pp], 0));
    HIPCHK(r, hipMemcpyAsync(dst, r->d_out.p, need, hipMemcpyDeviceToDevice, cur_stream(r)));
    return ORX_OK;
}

uint32_t orx_width(const orx_renderer* r) { return r ? r->W : 0; }
uint32_t orx_height(const orx_renderer* r) { return r ? r->H : 0; }
size_t orx_output_bytes(const orx_renderer* r) { return r ? (size_t)r->W * r->H * 12 : 0; }
uint32_t orx_emitted_photons_per_iteration(const orx_renderer* r) {
    return r ? r->cfg.photon_launch_width * r->cfg.photon_launch_height : 0;
}

orx_status orx_get_stats(orx_renderer* r, orx_stats* out) {
    if (!r || !out) return ORX_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof *out);
    HIPCHK(r, hipSetDevice(r->device));
    {
        orx_status s0 = sync_all(r);
        if (s0 != ORX_OK) return s0;
    }
    if (r->pipe.set[r->pipe.pp].grid.p) {
        GridParams g;
        HIPCHK(r, hipMemcpy(&g, r->pipe.set[r->pipe.pp].grid.p, sizeof g, hipMemcpyDeviceToHost));
        out->grid_size[0] = g.gx;
        out->grid_size[1] = g.gy;
        out->grid_size[2] = g.gz;
        out->cell_size = g.cell;
        out->world_origin[0] = g.ox;
        out->world_origin[1] = g.oy;
        out->world_origin[2] = g.oz;
        out->valid_photons = g.valid;
        out->num_cells = g.G;
        out->photons_visited = g.photons_visited;
        out->cells_visited = g.cells_visited;
        out->photons_visited_total = g.photons_visited_total;
        out->cells_visited_total = g.cells_visited_total;
        out->valid_photons_total = g.valid_total;
        for (uint32_t k = 0; k < (r->pipe.bufs ? r->pipe.nsets : 1u); k++) { /* the other buffer sets' share of the totals */
            if (k == r->pipe.pp) continue;
            GridParams g2;
            HIPCHK(r, hipMemcpy(&g2, r->pipe.set[k].grid.p, sizeof g2, hipMemcpyDeviceToHost));
            out->photons_visited_total += g2.photons_visited_total;
            out->cells_visited_total += g2.cells_visited_total;
            out->valid_photons_total += g2.valid_total;
        }
    }
    if (r->vcm.vb.dq0 && r->vcm.npx) { /* the last VCM camera pass's deferred connection shadow rays */
        uint32_t ctl[2] = {0, 0};
        HIPCHK(r, hipMemcpy(ctl, r->vcm.vb.dctl, 8, hipMemcpyDeviceToHost));
        out->vcm_shadow_rays = ctl[0];
        out->vcm_shadow_overflow = ctl[1];
    }
    if (r->vcm.vb.lcq && r->vcm.vb.lctl) { /* the last light pass's deferred camera connections */
        uint32_t ctl[2] = {0, 0};
        HIPCHK(r, hipMemcpy(ctl, r->vcm.vb.lctl, 8, hipMemcpyDeviceToHost));
        /* entries reserved minus those a wave could not fit and traced in place (their reserved range
         * below lcap holds inert placeholders): the connections the resolve traced */
        out->vcm_light_connections = ctl[0] - std::min(ctl[0], ctl[1]);
        out->vcm_light_inplace = ctl[1];
    }
    for (int p = 0; p < P_COUNT; p++) {
        double tot = 0.0;
        for (int k = 0; k < r->timing.ev_n[p]; k++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r->timing.ev[p][2 * k], r->timing.ev[p][2 * k + 1]) == hipSuccess) tot += ms;
        }
        out->pass_ms[p] = (float)tot;
    }
    out->timed_iterations = r->timing.iterations;
    out->bvh_stack_entries = r->scene.stack_entries;
    return check_grid_error(r);
}

int orx_ppm_pipelined(const orx_renderer* r) { return r && (r->pipe.last_pipelined || r->vcm.last_overlap) ? 1 : 0; }
int orx_ppm_grid_schedule(const orx_renderer* r, float* probe_ms) {
    if (!r) return -2;
    if (probe_ms) {
        probe_ms[0] = r->gasync.probe_ms[0];
        probe_ms[1] = r->gasync.probe_ms[1];
    }
    return r->gasync.probe_stage ? -1 : r->gasync.on ? 1 : 0;
}
orx_status orx_set_iteration_pipelining(orx_renderer* r, int mode) {
    if (!r || mode < -1 || mode > 1) return ORX_ERR_INVALID_ARGUMENT;
    r->pipe.mode = mode;
    return ORX_OK;
}

orx_status orx_reset_timing(orx_renderer* r) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    HIPCHK(r, hipSetDevice(r->device));
    {
        orx_status s0 = sync_all(r);
        if (s0 != ORX_OK) return s0;
    }
    for (int p = 0; p < P_COUNT; p++) r->timing.ev_n[p] = 0;
    r->timing.iterations = 0;
    for (uint32_t k = 0; k < (r->pipe.bufs ? r->pipe.nsets : 1u); k++) { /* every set holds its iterations' share */
        void* grid = r->pipe.set[k].grid.p;
        if (!grid) continue;
        GridParams g;
        HIPCHK(r, hipMemcpy(&g, grid, sizeof g, hipMemcpyDeviceToHost));
        g.photons_visited_total = 0;
        g.cells_visited_total = 0;
        g.valid_total = 0;
        g.union_photons_total = 0;
        HIPCHK(r, hipMemcpy(grid, &g, sizeof g, hipMemcpyHostToDevice));
    }
    return ORX_OK;
}

}  // extern "C"

/* for orx_group.hip (orx_group_get_output): the grid error orx_get_output reports */
orx_status orx::check_grid(orx_renderer* r) {
    if (!r) return ORX_ERR_INVALID_ARGUMENT;
    HIPCHK(r, hipSetDevice(r->device));
    return check_grid_error(r);
}
