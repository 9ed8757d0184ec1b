/*
 * orx_group.h — the render group's state and what its two host units share: orx_group.hip (creation, the
 * schedules, output, display, convergence, debug collectives) and orx_group_state.hip (checkpoint / resume).
 * The communicator and the group's kernels are behind orx_group_comm.h.
 * Internal: not installed, nothing under include/ sees it.
 */
#pragma once
#include "orx_group_comm.h"
#include "orx_host.h"

/* a device allocation that remembers its device: freed there by release() and by the destructor */
struct GroupBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
    GroupBuf() = default;
    GroupBuf(GroupBuf&& o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr; } /* and so not copyable */
    ~GroupBuf() { release(); }
    hipError_t ensure(int dev, size_t need) {
        if (p && bytes >= need && dev == device) return hipSuccess;
        release();
        device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e != hipSuccess) return e;
        e = hipMalloc(&p, std::max<size_t>(need, 16));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = need;
        return hipSuccess;
    }
    void release() {
        if (p) {
            hipSetDevice(device);
            hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
    float* f() const { return (float*)p; }
};

/* per rank: the streams the schedule supplies to the renderer and the communicator, and its buffers */
struct GroupRank {
    orx_renderer* r = nullptr;
    int device = 0;
    hipStream_t main = nullptr;                            /* the renderer's own stream (borrowed) */
    hipStream_t comm = nullptr, side = nullptr, fin = nullptr; /* hit-point all-gather; gather; reduce-scatter + finish */
    hipEvent_t ev_export = nullptr, ev_gathered = nullptr, ev_partial = nullptr;
    /* two sets (pipelined PPM alternates): own hit points, all hit points, partial indirect of all
     * pixels, summed indirect of the own rows */
    GroupBuf hp_local[2], hp_all[2], ind_partial[2], ind_local[2];
    GroupBuf splat_all, splat_own; /* VCM */
    GroupBuf out_local, out_all;   /* own rows / whole frame; every rank's blocks (ROWS output) */
    GroupBuf conv_local, conv_all; /* orx_group_get_convergence: own error + luminance planes; every rank's */
    /* SLABS: own histogram, every rank's histograms, packed photon records out and in */
    GroupBuf hist, hists, rec_send, rec_recv;
    std::vector<uint32_t> dest_base; /* SLABS: where the records for rank d start in rec_send */
    uint64_t local_it = 0;         /* BATCH: the rank's own iteration count */
};

struct orx_group {
    uint32_t n = 0;
    orx_config cfg{};
    orx_group_config gc{};
    std::vector<GroupRank> rk;
    GroupComm* comm = nullptr;
    bool scene_ready = false;
    bool pipe = false; /* ROWS: orx_set_ppm_pipeline is on */
    std::string err;
    uint32_t W = 0, H = 0, max_rows = 0;
    int32_t method = -1;
    uint32_t k = 0;      /* pipelined PPM: the buffer set of the next iteration */
    int pending = -1;    /* pipelined PPM: the set whose reduce-scatter + finish are outstanding */
    uint64_t calls = 0;  /* BATCH: iterations since the last restart */
    GroupBuf image;      /* rank 0: [H][W][3], ROWS de-interleaved / BATCH merged sum */
    GroupBuf dbg_in, dbg_out;
    GroupBuf conv_full, conv_tiles, display; /* rank 0: the frame's error + luminance planes, tile records; BGRA8 / RGBA8 */
    bool conv_on = false;
    /* ROWS + ORX_PHOTONS_SLABS with n > 1: the spatial photon partition for PPM frames */
    bool slabs = false;
    uint32_t* h_hists = nullptr; /* pinned: the all-gathered histograms of one iteration */
    struct {
        bool have = false;
        uint32_t axis = 0;
        uint8_t bin_dest[ORX_GROUP_SLAB_BINS];
        std::vector<uint64_t> counts; /* [n][n] */
        uint32_t box[6];
    } plan;
    __attribute__((visibility("hidden"))) ~orx_group() = default; /* frees the GroupBufs; not one of the library's symbols */
};

static inline orx_status gerr(orx_group* g, orx_status s, const std::string& m) {
    if (g) g->err = m;
    return s;
}
/* a rank's failure, copied with its rank number in front */
static inline orx_status rank_err(orx_group* g, uint32_t k, orx_status s) {
    g->err = "rank " + std::to_string(k) + ": " + orx_last_error(g->rk[k].r);
    return s;
}
#define GHIP(g, x)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            return gerr(g, e_ == hipErrorOutOfMemory ? ORX_ERR_OUT_OF_MEMORY : ORX_ERR_DEVICE,      \
                        std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_));        \
    } while (0)
#define GRANK(g, k, x)                                   \
    do {                                                 \
        const orx_status s_ = (x);                       \
        if (s_ != ORX_OK) return rank_err(g, (k), s_);   \
    } while (0)
#define GCOMM(g, x)                                                      \
    do {                                                                 \
        std::string e_;                                                  \
        const orx_status s_ = (x);                                       \
        if (s_ != ORX_OK) return gerr(g, s_, std::string(g->comm->name()) + " communicator: " + e_); \
    } while (0)

#pragma GCC visibility push(hidden)
/* orx_group.hip */
/* every stream of the group idle: before exchange buffers are replaced or read on the host */
orx_status group_sync(orx_group* g);
/* the outstanding pipelined finish issued (group_drain), then group_sync: before the ranks' state is replaced or read */
orx_status group_quiesce(orx_group* g);
/* the exchange buffers follow the frame size (and the method) of the request */
orx_status group_prepare(orx_group* g, const orx_request* det);
#pragma GCC visibility pop
