/*
 * orx_host.h — the renderer's host-side state and the functions its host units share
 * (orx_capi.hip, orx_host_ppm.hip, orx_host_vcm.hip, orx_host_read.hip, orx_host_state.hip, orx_post.hip, orx_group*.hip).
 * Scene validation and conversion are a host-only unit of their own (orx_scene_host.cpp), as are the BVH builder
 * (orx_bvh_host.cpp), the slab planner, the checkpoint codec and the display resolve's host half.
 * Internal: not installed, nothing under include/ sees it.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "orx.h"
#include "orx_kernels.h"
#include "orx_post.h"
#include "orx_scene_host.h"

namespace orx {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

enum PassId { P_EYE = 0, P_PHOTON, P_SETUP_HASH, P_SCAN, P_SCATTER, P_GATHER, P_DIRECT, P_PT, P_VCM_LIGHT, P_VCM_CAMERA,
              P_VCM_SHADOW, P_VCM_GRID, P_VCM_MERGE, P_CONVERGENCE, P_COUNT };
static_assert((int)P_COUNT == (int)ORX_PASS_COUNT && P_COUNT <= 16, "orx_pass / orx_stats.pass_ms");
constexpr int EV_POOL = 1024; /* timed launches kept per pass between resets */

/* One buffer set of PPM pipelining: what the deferred gather + output of iteration i read while the
 * next iterations write their own.  Hit points, direct light and grid parameters always; then the
 * uniform grid's sorted photons and offsets (photon_map 0), or the hash's deposit records and table
 * (1), or the kd-tree (2).  Under photon maps 1 and 2 the uniform grid's three exist in set[0] only. */
struct PpmSet {
    DevBuf hp, dir, grid, sorted, subofs, offsets, hslots, hcount, hwin, kdtree;
};
/* what the photon pass writes and the grid build reads: deposit records (uniform grid and kd-tree; the
 * hash's live in PpmSet::hslots), validity bits, positions, AABB replicas */
struct PhotonOut {
    DevBuf slots, vmask, pos4, bbox;
};
/* One set of what an overlapped VCM resolve (and its in-place rerun) reads while the next iteration's
 * light pass and walk write the other: light image, entry lists and per-pixel list heads, light
 * vertices with their counts and texel colours, the walk's RNG start words, the light pass's deferred
 * camera connections */
struct VcmSet {
    DevBuf splat, dq, dpx, verts, count, kd, rngsave, lcq;
};
/* the scene on the device, written by orx_init_scene alone (orx_capi.hip); triuv, trit, tribt, texels and texdesc:
 * the Texture material's attributes and images */
struct SceneBufs {
    DevBuf quads, qmat, spheres, smat, triv, trin, tmat, mats, lights, bvh, bvhprims;
    DevBuf triuv, trit, tribt, texels, texdesc;
    hipError_t upload(const orx_scene& s, const HostScene& h, const LeafArrays& la, const TextureLayout& tl);
};
/* What a frame's buffers are sized by, computed once at the top of resize: the first buffer set and photon
 * output set and every further one (size_ppm_set, size_photon_out) take their byte counts from here. */
struct FrameSizes {
    size_t nhp = 0;       /* hit points: max_rows * W (planes padded to max_rows) */
    size_t nslot_rng = 0; /* RNG slots of the own rows */
    size_t nphot = 0;     /* photons this rank emits */
    uint32_t D = 0;       /* deposit slots per emitted photon */
    size_t S = 0;         /* nphot * D */
    size_t S_cap = 0;     /* slab mode: room for every deposit slot of the global launch; else S */
    size_t splane = 0;    /* floats per sorted-photon plane */
    size_t G2 = 0;        /* grid cells + 2 */
    uint32_t nsub = 0, bshift = 0; /* sub-rows per cell row; the bucket sort's 2^bshift virtual cells per bucket */
    size_t bs_nchunk = 0, bs_nchunk_cap = 0, bs_nbmax = 0, bs_nscan = 0;
    size_t hnum = 0; /* the stochastic hash's table entries (photon_map 1) */
    /* kd-tree (photon_map 2): nodes, levels, 1024-photon blocks, 4096-photon tiles, scan partials */
    size_t tree = 0, nblk = 0, ntiles = 0, tp = 0;
    uint32_t levels = 0;
};

/* The renderer's state by owner: each struct below names at its head the unit that runs its schedule and does
 * most of its writes; orx_renderer holds one of each next to what every unit shares.  The writes from elsewhere:
 * orx_capi.hip sizes gs.*, media.volR / ev_a / ev_b and the first buffer sets in resize; drops stale state there and
 * in the flush functions (pipe.pp / bufs / gather_in_flight / eye_chain, gasync.po, fin.due / snap, media.vm.valid,
 * vcm.resolve_in_flight), member by member, around calls that can fail; sets pipe.mode from its entry point, media.*,
 * vcm.tstats and note.* in init_scene, and vcm.psf_*, vcm.estimated, vcm.last_overlap, pipe.last_pipelined and
 * note.* when an iteration begins.  orx_host_state.hip sets vcm.psf_* and vcm.estimated on a restore; orx_post.hip
 * files fin.conv. */

/* orx_host_ppm.hip.  PPM iteration pipelining (world 1, own stream): the gather and output of iteration i run on
 * gstream beside the eye/photon/grid passes of iteration i+1, each iteration on the next of nsets
 * buffer sets: 3 on one device (the eye pass of i + 1 then waits for the gather of i - 2, not of
 * i - 1), 2 for the sharded pipeline.  pp: the current set; ev_gdone[k] marks the end of the last
 * gather+output on set[k]; bufs: set[1..nsets) are allocated */
struct PpmPipe {
    uint32_t nsets = 2, pp = 0;
    bool bufs = false, last_pipelined = false;
    bool gather_in_flight = false; /* a gather is in flight */
    PpmSet set[3];
    hipEvent_t ev_grid_done = nullptr, ev_gdone[3] = {nullptr, nullptr, nullptr};
    int mode = -1; /* orx_set_iteration_pipelining: -1 = ORX_PIPELINE env */
    /* the PPM direct pass on aux, overlapped with the grid build and gather */
    hipEvent_t ev_photon_done = nullptr, ev_direct_done = nullptr;
    bool overlap_direct = false;
    /* pipelined PPM: the eye pass of iteration i+1 runs on aux right behind the direct pass of i
     * (the RNG chain), beside the grid build of i; ev_eye_done orders the photon pass after it.
     * eye_chain: aux is already ordered after every earlier renderer-stream write the eye pass
     * reads (the previous call was a pipelined iteration, nothing else enqueued since) */
    hipEvent_t ev_eye_done = nullptr, ev_main = nullptr;
    bool eye_chain = false;
};
/* orx_host_ppm.hip.  One device, three buffer sets, uniform grid: the grid build of iteration i on a stream of
 * its own (gridq) beside the photon pass of i + 1, the photon pass's outputs alternating between out[0] and
 * out[1] (po: the one the last photon pass wrote; out_b: out[1] is allocated, the asynchronous build may run);
 * ev_gsrc[o]: the last grid build that read out[o] */
struct GridAsync {
    bool on = false;
    uint32_t po = 0;
    hipEvent_t ev_gsrc[2] = {nullptr, nullptr};
    PhotonOut out[2];
    bool out_b = false;
    /* the schedule chosen from the workload (ORX_GRID_ASYNC unset): the first pipelined iteration after a
     * resize times its photon pass + grid build on the renderer's stream and its gather, the next one's
     * photon pass waits for that gather (so nothing overlaps it), and the iteration after that picks the
     * asynchronous build if photon + grid take more than GRID_CHAIN_RATIO x the gather (the chain, not the
     * gather, then sets the frame).  probe_stage: 0 decided, 1 measure, 2 isolate, 3 decide */
    uint32_t probe_stage = 0, probe_k = 0;
    float probe_ms[2] = {0.f, 0.f}; /* photon + grid, gather of the measured iteration */
    hipEvent_t ev_pm[4] = {};
};
/* orx_host_ppm.hip.  Sharded PPM pipelining (orx_set_ppm_pipeline): gather + finish on the caller's side stream */
struct ShardFinish {
    bool shard_pipe = false;
    hipStream_t side = nullptr;
    /* its finishes (orx_ppm_finish / _on): due, the current iteration's is outstanding; snap, the
     * previous iteration's is, its pixel buffers, constants and buffer set held here (the caller may issue
     * it after the next iteration's eye pass, behind that iteration's hit-point all-gather) */
    bool due = false, snap = false;
    PixelBufs px{};
    Consts consts{};
    uint32_t pp = 0;
    ConvIt conv{}; /* and its place in the statistics window */
};
/* orx_host_ppm.hip.  Slab mode (orx_set_slab_partition): photon buffers sized for the imported slab photons */
struct SlabState {
    bool on = false;
    DevBuf tab, cur;
    DevBuf tiles; /* slab gather: tile list, count, flags */
    uint32_t own_axis = 0, own_nb = 0, own_lo = 1, own_hi = 0; /* slab gather: the bins this rank owns */
};
/* orx_host_ppm.hip.  The grid build's and the photon pass's scratch, sized by resize */
struct GridScratch {
    DevBuf perm, keys;
    DevBuf bstable, bspartials, bspairs; /* bucket-sort grid build */
    DevBuf ptrav;                        /* photon pass: the deep traversal-stack entries */
};
/* orx_host_ppm.hip.  kd-tree photon map (photon_map = 2, orx_kdtree.hip): the build's scratch (the trees are
 * PpmSet::kdtree) and the kernels' view of it */
struct KdScratch {
    DevBuf ids, lst, nkey, keys, nodepos, seg, box, ninfo, P, ppart, table, tpart, vpart, count;
    KdBufs view{};
};
/* orx_host_ppm.hip.  Participating medium (cfg.enable_media with a medium box): the box, this frame's per-pixel
 * volumetricRadiance and per-photon last events, the volumetric table of the last photon pass and its build's
 * buffers */
struct MediaState {
    bool on = false;
    VolMap vm{};
    DevBuf volR, ev_a, ev_b;
    DevBuf cnt, win, A, B, keys, vals, keys2, vals2, sort, start, rec;
};
/* orx_host_vcm.hip */
struct VcmState {
    /* pixelSizeFactor (OptixRenderer.cpp:306, :846), LVC estimate flag (:83, :461, :847) */
    float psf_x = 1.0f, psf_y = 1.0f;
    bool estimated = false;
    size_t npx = 0;  /* own-row subpaths W*rows the VCM buffers are sized for */
    size_t spx = 0;  /* owner-block splat pixels W*max_rows*world */
    bool finish_due = false; /* light pass done, camera pass (orx_vcm_finish) outstanding */
    bool kd = false;         /* set[dpar].kd sized for the current npx */
    VcmBufs vb{};            /* the kernels' view; its per-set pointers are written by bind_vcm_views alone */
    VcmConsts c{};
    DevBuf cam, shq, work, consts;
    DevBuf tstats; /* ORX_TRAV_STATS builds: the traversal counters of every method, bound by init_scene */
    DevBuf shstk; /* VCM camera pass: the shadow kernel's deep stack */
    /* VCM overlap (single device, deferred shadow rays): the camera pass's resolve (shadow rays,
     * colours) of iteration i runs on aux beside the light pass and walk of i+1, each iteration on
     * set[dpar] (the serial schedule stays on one); ev_cam ends the walk, ev_acc the resolve */
    VcmSet set[2];
    uint32_t dpar = 0;
    bool last_overlap = false;
    size_t dqcap = 0; /* entries per list (ORX_VCM_DEFER per own pixel) */
    hipEvent_t ev_cam = nullptr, ev_acc = nullptr;
    bool resolve_in_flight = false; /* a resolve is in flight on aux */
};
/* orx_host_vcm.hip.  VCM vertex merging (cfg.vcm_merging, orx_vcm_merge.hip): the camera-vertex cache with its
 * texel colours and counts, the light-vertex grid (sort keys and values, sort scratch, cell starts,
 * cell-ordered records), the per-record colours, the per-pixel merging colour and debug counts;
 * allocated by the first VCM iteration with merging on, sized for mpx own pixels */
struct VcmMergeState {
    DevBuf cverts, cvkd, cvcount, keys, sort, start, lrec, part, cand, merge, count;
    size_t mpx = 0;
    bool merged = false; /* the merge buffers hold an iteration's results */
    VcmMergeBufs mb{};
    VcmMergeGrid grid{};
};
/* orx_post.hip.  Convergence statistics (orx_set_convergence), nothing of it allocated while off: stat holds
 * prev[3], A and M2 over npx = rows * W own pixels; count iterations of the window have begun,
 * zero: the next one is the first on a cleared sum; it / last: the place in the window of the
 * iteration begun last and of the one before (whose sharded finish may still be held back);
 * err: the e and m planes of the last query (err_n: its n, 0 none) */
struct ConvState {
    bool on = false, zero = false;
    uint32_t count = 0, err_n = 0;
    size_t npx = 0;
    ConvIt it{}, last{};
    DevBuf stat, err, tiles;
};
/* orx_capi.hip.  Timing: event pairs per pass since the last orx_reset_timing */
struct PassTiming {
    std::vector<hipEvent_t> ev[P_COUNT];
    int ev_n[P_COUNT]{};
    uint32_t iterations = 0;
    bool on = true;
};
/* orx_host_state.hip.  Checkpoints: the scene's key, and the numbers of the last iteration as the caller
 * passed them (have: there was one, or a restore) */
struct CheckpointNote {
    uint64_t scene_key = 0;
    bool have = false;
    uint64_t iter = 0, local = 0;
    float radius = 0.f;
    int32_t method = -1;
};

}  // namespace orx

struct orx_renderer {
    int device = 0;
    orx_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;     /* PPM direct pass, overlapped with the grid build and gather; VCM resolve */
    hipStream_t gstream = nullptr; /* the deferred gather + output of PPM pipelining */
    hipStream_t gridq = nullptr;   /* the asynchronous grid build */
    hipStream_t ext_stream = nullptr; /* caller-provided stream (orx_set_stream) */
    bool use_ext = false;
    /* scene */
    bool scene_ready = false;
    orx::SceneBufs sb;
    bool has_tex = false;
    orx::DevScene scene{};
    uint32_t n_mats = 0;
    std::vector<orx::DevLight> host_lights;
    orx::f3 aabb_lo{}, aabb_hi{};  /* IScene::getSceneAABB (the stochastic hash grid's bounds) */
    /* frame */
    uint32_t W = 10, H = 10, RW = 0, RH = 0;
    uint32_t rank = 0, world = 1;
    uint32_t rows = 0, max_rows = 0, rng_rows = 0, prows = 0;
    bool rng_ready = false;
    orx::FrameSizes fs{};
    orx::DevBuf d_rng, d_ind, d_out, d_dbg;
    orx::DevBuf d_display; /* orx_get_display: the rows' RGBA8 / BGRA8 image */
    /* the kernels' views; their per-set pointers are written by bind_ppm_views alone */
    orx::PixelBufs px{};
    orx::PhotonBufs pb{};
    uint64_t last_method = 0;
    orx::Consts last_consts{};
    /* by owner */
    orx::PpmPipe pipe;
    orx::GridAsync gasync;
    orx::ShardFinish fin;
    orx::SlabState slab;
    orx::GridScratch gs;
    orx::KdScratch kds;
    orx::MediaState media;
    orx::VcmState vcm;
    orx::VcmMergeState mg;
    orx::ConvState conv;
    orx::PassTiming timing;
    orx::CheckpointNote note;
};

namespace orx {

inline orx_status set_err(orx_renderer* r, orx_status s, const std::string& m) {
    if (r) r->err = m;
    return s;
}
#define HIPCHK(r, x)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess)                                                                             \
            return set_err(r, e_ == hipErrorOutOfMemory ? ORX_ERR_OUT_OF_MEMORY : ORX_ERR_DEVICE,          \
                           std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_));           \
    } while (0)

inline hipStream_t cur_stream(orx_renderer* r) { return r->use_ext ? r->ext_stream : r->stream; }
/* the stream the deferred gather + output run on */
inline hipStream_t gather_stream(orx_renderer* r) { return r->fin.shard_pipe ? r->fin.side : r->gstream; }

/* orx_capi.hip */
/* a timed interval and roctx range around pass p's launches on `st` (default: the current stream) */
void ev_begin(orx_renderer* r, int p, hipStream_t st);
void ev_end(orx_renderer* r, int p, hipStream_t st);
inline void ev_begin(orx_renderer* r, int p) { ev_begin(r, p, cur_stream(r)); }
inline void ev_end(orx_renderer* r, int p) { ev_end(r, p, cur_stream(r)); }
void flush_vcm(orx_renderer* r);
void flush_pipeline(orx_renderer* r);
orx_status sync_all(orx_renderer* r);
orx_status begin_iteration(orx_renderer* r, uint64_t local_iteration_number, const orx_request* det, bool pipelined = false,
                           bool vcm_overlap = false);
/* orx_init_scene for a scene that scene_validate has passed (orx_group.hip validates once for all ranks) */
orx_status init_scene_checked(orx_renderer* r, const orx_scene& s);
DevCamera camera_setup(const orx_camera& c, float* ulen_out = nullptr, float* vlen_out = nullptr);
Consts make_consts(orx_renderer* r, float ppm_radius, uint64_t local_iteration_number);
/* ORX_ERR_GRID_TOO_LARGE of the renderer's last PPM iteration (synchronises it; for orx_group.hip) */
orx_status check_grid(orx_renderer* r);

/* resize without the RNG seeding launch (orx_restore_state loads the words instead) */
orx_status resize_unseeded(orx_renderer* r, uint32_t W, uint32_t H);
/* what a checkpoint's header carries: every entry point that starts an iteration leaves them here */
inline void note_iteration(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number, float ppm_radius,
                           int32_t method) {
    r->note.have = true;
    r->note.iter = iteration_number;
    r->note.local = local_iteration_number;
    r->note.radius = ppm_radius;
    r->note.method = method;
}

/* orx_host_state.hip: a renderer's share of a checkpoint; orx_group_state.hip moves its ranks' rows with these */
/* the frame header of the renderer's state (sizes, last iteration, flags, scene key) */
void state_describe(const orx_renderer* r, orx_state_info* info);
/* ORX_ERR_INVALID_ARGUMENT unless `info` is a frame of this renderer's scene and photon launch size */
orx_status state_check(orx_renderer* r, const orx_state_info* info);
/* The rank's RNG rows and output rows into device arrays on its device, on its stream (the caller has
 * synchronised the renderer and waits for the stream): canonical, the whole frame's arrays [RH][RW][6] and
 * [H][W][3], local row j at global row rank + j world; else compact ones of the own rows, local row j at j */
orx_status state_rows_export(orx_renderer* r, uint32_t* rng_dev, float* out_dev, bool canonical);
/* The inverse, as a restore: sizes the frame for info's W x H without seeding, loads the rows, sets the
 * pixel size factor, the estimate flag and the last iteration's numbers; synchronous */
orx_status state_rows_import(orx_renderer* r, const orx_state_info* info, const uint32_t* rng_dev, const float* out_dev,
                             bool canonical);

/* orx_host_ppm.hip */
void bind_ppm_views(orx_renderer* r);
/* allocate and zero-fill buffer set k (the uniform grid's three buffers: set 0, or every set under photon_map 0)
 * and a photon output set, by r->fs; resize sizes index 0 with them, ensure_second_set the others */
orx_status size_ppm_set(orx_renderer* r, PpmSet& set, uint32_t k);
orx_status size_photon_out(orx_renderer* r, PhotonOut& out);
/* the kd-tree build's scratch and the kernels' view of it (photon_map 2), by r->fs */
orx_status kd_resize(orx_renderer* r);
orx_status ensure_second_set(orx_renderer* r);
orx_status ppm_serial_iteration(orx_renderer* r, const DevCamera& cam, const Consts& c);
orx_status ppm_pipelined_iteration(orx_renderer* r, const orx_request* det, float ppm_radius,
                                   uint64_t local_iteration_number);

/* orx_host_vcm.hip */
orx_status vcm_check_lights(orx_renderer* r);
orx_status vcm_iteration(orx_renderer* r, const orx_request* det, float ppm_radius, bool overlap);

}  // namespace orx
