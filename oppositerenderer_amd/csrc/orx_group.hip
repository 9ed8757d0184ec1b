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
 * orchestration, the exchange buffers and the communicator:
 *
 *   LOCAL  every rank on one device in one process: the all-gather is device-to-device copies, the two
 *          sums are the kernels below (rank order 0..n-1 in fp32, no atomics: equal to a sequential
 *          float32 sum on the host)
 *   RCCL   librccl opened with dlopen when selected (liborx.so has no link dependency on it), one
 *          communicator per rank (ncclCommInitAll), group calls around the collectives
 *
 * photon_partition = ORX_PHOTONS_SLABS puts the spatial photon partition (orx_set_slab_partition) behind
 * the same handle: ShardedPPM._iteration_slab and slab_exchange of multigpu.py with the planner of
 * orx_slab_plan.cpp on the host and the photon records moved by GroupComm::all_to_all_v (LOCAL: one launch
 * of k_group_all_to_all; RCCL: ncclSend / ncclRecv in one group, unmeasured on hardware like every N > 1
 * collective over RCCL: one GPU per box, and RCCL refuses two ranks on one GPU).
 */
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "orx.h"
#include "orx_host.h"
#include "orx_slab_plan.h"
#include "orx_state.h"

#define ORX_GROUP_MAX 64u
#define ORX_GROUP_SLAB_BINS 1024u /* multigpu.SLAB_BINS */
#define ORX_RECORD_DWORDS 9u      /* a photon record: position, direction, power */

/* ------------------------------------------------------------------ kernels ---- */

struct GroupPtrs {
    const float* in[ORX_GROUP_MAX];
    float* out[ORX_GROUP_MAX];
};

/* out[i] = in[0][ofs + i] + in[1][ofs + i] + ... + in[n-1][ofs + i], i < B, strictly in rank order.
 * vec: every in[r] is 16-B aligned, so in[r] + ofs share one misalignment; a scalar head brings them to
 * 16 B, float4 loads cover the body (float4 stores too when `out` lands on 16 B there, scalar stores
 * otherwise: the loads are n times the stores), a scalar tail the rest. */
__device__ __forceinline__ float group_sum_at(const GroupPtrs& p, uint32_t n, size_t i) {
    float a = p.in[0][i];
    for (uint32_t r = 1; r < n; r++) a += p.in[r][i];
    return a;
}

__device__ __forceinline__ void group_sum_block(const GroupPtrs& p, uint32_t n, size_t ofs, float* __restrict__ out,
                                                size_t B, bool vec) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    size_t head = vec ? (size_t)((4u - (uint32_t)(ofs & 3u)) & 3u) : B;
    if (head > B) head = B;
    const size_t nv = (B - head) / 4;
    const size_t tail = head + nv * 4;
    for (size_t i = tid; i < head; i += nt) out[i] = group_sum_at(p, n, ofs + i);
    const bool ovec = (((uintptr_t)(out + head)) & 15u) == 0;
    for (size_t v = tid; v < nv; v += nt) {
        const size_t i = ofs + head + v * 4;
        float4 a = *reinterpret_cast<const float4*>(p.in[0] + i);
        for (uint32_t r = 1; r < n; r++) {
            const float4 b = *reinterpret_cast<const float4*>(p.in[r] + i);
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        float* o = out + head + v * 4;
        if (ovec) {
            *reinterpret_cast<float4*>(o) = a;
        } else {
            o[0] = a.x;
            o[1] = a.y;
            o[2] = a.z;
            o[3] = a.w;
        }
    }
    for (size_t i = tail + tid; i < B; i += nt) out[i] = group_sum_at(p, n, ofs + i);
}

/* out[k][j] = in[0][k B + j] + in[1][k B + j] + ...: blockIdx.y is the receiving rank k */
__global__ void __launch_bounds__(256) k_group_reduce_scatter(GroupPtrs p, uint32_t n, size_t B, int vec) {
    const uint32_t k = blockIdx.y;
    group_sum_block(p, n, (size_t)k * B, p.out[k], B, vec != 0);
}

/* out[0][j] = in[0][j] + in[1][j] + ... */
__global__ void __launch_bounds__(256) k_group_reduce(GroupPtrs p, uint32_t n, size_t N, int vec) {
    group_sum_block(p, n, 0, p.out[0], N, vec != 0);
}

/* rank blocks [n][max_rows][W][3] (local row j of rank g = global row g + j n) -> [H][W][3] */
__global__ void __launch_bounds__(256) k_group_assemble_rows(const float* __restrict__ blocks, float* __restrict__ out,
                                                             uint32_t W, uint32_t H, uint32_t n, uint32_t max_rows) {
    const size_t row = (size_t)W * 3, total = row * H;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nt) {
        const size_t y = i / row, x = i - y * row;
        const size_t g = y % n, j = y / n;
        out[i] = blocks[(g * max_rows + j) * row + x];
    }
}

/* the one-channel sibling: rank blocks of `block` floats each, whose plane at `off` is [max_rows][W] -> [H][W] */
__global__ void __launch_bounds__(256) k_group_assemble_plane(const float* __restrict__ blocks, float* __restrict__ out,
                                                              uint32_t W, uint32_t H, uint32_t n, uint32_t max_rows,
                                                              size_t block, size_t off) {
    const size_t total = (size_t)W * H;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += nt) {
        const size_t y = i / W, x = i - y * W;
        const size_t g = y % n, j = y / n;
        out[i] = blocks[g * block + off + j * W + x];
    }
}

/* one (s, d) run of the photon all-to-all: dword offsets into rank s's send and rank d's receive buffer */
struct GroupRun {
    uint64_t src, dst, n;
};

/* every run of an all-to-all in one launch: blockIdx.y is the pair s * n + d, its blocks stride over the
 * run.  Records are 9 dwords, so a run starts on any 4-byte boundary: dwords are copied, and 16 bytes at a
 * time only over the part where source and destination are both 16-byte aligned (they are when the two
 * starts share their misalignment: a dword head brings both there).  Plain vector loads and stores. */
__global__ void __launch_bounds__(256) k_group_all_to_all(GroupPtrs p, uint32_t n, const GroupRun* __restrict__ runs) {
    const uint32_t pair = blockIdx.y, s = pair / n, d = pair - s * n;
    const GroupRun r = runs[pair];
    if (r.n == 0) return;
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(p.in[s]) + r.src;
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(p.out[d]) + r.dst;
    const size_t N = r.n;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    size_t head = N;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) == 0) head = (size_t)(((16u - ((uintptr_t)src & 15u)) & 15u) / 4u);
    if (head > N) head = N;
    const size_t nv = (N - head) / 4;
    const size_t tail = head + nv * 4;
    for (size_t i = tid; i < head; i += nt) dst[i] = src[i];
    for (size_t v = tid; v < nv; v += nt)
        *reinterpret_cast<uint4*>(dst + head + v * 4) = *reinterpret_cast<const uint4*>(src + head + v * 4);
    for (size_t i = tail + tid; i < N; i += nt) dst[i] = src[i];
}

static inline uint32_t stream_grid(size_t items, uint32_t rows = 1) {
    const size_t want = (items + 255) / 256;
    const size_t cap = std::max<size_t>(1, 2048 / std::max(1u, rows));
    return (uint32_t)std::max<size_t>(1, std::min(want, cap));
}

/* ------------------------------------------------------------- communicator ---- */

/* One call serves all ranks: per-rank send and receive buffers and per-rank streams; the ordering
 * between the ranks' streams is the communicator's business.  On return, work issued later on streams[k]
 * sees rank k's result, and may overwrite rank k's send buffer. */
struct GroupComm {
    virtual ~GroupComm() {}
    virtual const char* name() const = 0;
    /* all ranks share one device: receive buffers of an all-gather may be one and the same */
    virtual bool shared_device() const = 0;
    virtual orx_status all_gather(const void* const* send, void* const* recv, size_t bytes, const hipStream_t* st,
                                  std::string& err) = 0;
    /* recv[k][j] = sum_r send[r][k block + j] */
    virtual orx_status reduce_scatter(const float* const* send, float* const* recv, size_t block, const hipStream_t* st,
                                      std::string& err) = 0;
    /* recv_root[j] = sum_r send[r][j], on rank 0 */
    virtual orx_status reduce(const float* const* send, float* recv_root, size_t n_floats, const hipStream_t* st,
                              std::string& err) = 0;
    /* what all_to_all_v needs beyond the other collectives, once, at group creation */
    virtual orx_status prepare_all_to_all(std::string&) { return ORX_OK; }
    /* photon records (36 bytes): rank s sends counts[s * n + d] records to rank d.  send[s] holds s's runs for
     * d = 0..n-1 back to back, recv[d] receives the runs of s = 0..n-1 back to back; the caller sizes both. */
    virtual orx_status all_to_all_v(const float* const* send, float* const* recv, const uint64_t* counts,
                                    const hipStream_t* st, std::string& err) = 0;
};

#define COMM_HIP(x)                                                                   \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            err = std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_); \
            return e_ == hipErrorOutOfMemory ? ORX_ERR_OUT_OF_MEMORY : ORX_ERR_DEVICE; \
        }                                                                             \
    } while (0)

struct LocalComm final : GroupComm {
    uint32_t n = 0;
    int device = 0;
    std::vector<hipEvent_t> ev_in;
    hipEvent_t ev_done = nullptr;
    /* all_to_all_v: the runs of one call on the device, and the last launch that read them */
    GroupRun* d_runs = nullptr;
    hipEvent_t ev_runs = nullptr;
    std::vector<GroupRun> h_runs;

    ~LocalComm() override {
        hipSetDevice(device);
        for (hipEvent_t e : ev_in)
            if (e) hipEventDestroy(e);
        if (ev_done) hipEventDestroy(ev_done);
        if (ev_runs) hipEventDestroy(ev_runs);
        if (d_runs) hipFree(d_runs);
    }
    orx_status init(uint32_t world, int dev, std::string& err) {
        n = world;
        device = dev;
        COMM_HIP(hipSetDevice(device));
        ev_in.assign(n, nullptr);
        for (hipEvent_t& e : ev_in) COMM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        COMM_HIP(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
        return ORX_OK;
    }
    const char* name() const override { return "local"; }
    bool shared_device() const override { return true; }

    /* the collective runs on rank 0's stream once every rank's stream has reached the call ... */
    orx_status begin(const hipStream_t* st, std::string& err) {
        COMM_HIP(hipSetDevice(device));
        for (uint32_t k = 1; k < n; k++) {
            COMM_HIP(hipEventRecord(ev_in[k], st[k]));
            COMM_HIP(hipStreamWaitEvent(st[0], ev_in[k], 0));
        }
        return ORX_OK;
    }
    /* ... and every rank's stream goes on after it */
    orx_status end(const hipStream_t* st, std::string& err) {
        COMM_HIP(hipGetLastError());
        if (n > 1) COMM_HIP(hipEventRecord(ev_done, st[0]));
        for (uint32_t k = 1; k < n; k++) COMM_HIP(hipStreamWaitEvent(st[k], ev_done, 0));
        return ORX_OK;
    }
    orx_status all_gather(const void* const* send, void* const* recv, size_t bytes, const hipStream_t* st,
                          std::string& err) override {
        orx_status s = begin(st, err);
        if (s != ORX_OK) return s;
        for (uint32_t d = 0; d < n; d++) {
            bool seen = false; /* ranks that share a receive buffer get one copy */
            for (uint32_t e = 0; e < d; e++) seen = seen || recv[e] == recv[d];
            if (seen) continue;
            for (uint32_t k = 0; k < n; k++)
                COMM_HIP(hipMemcpyAsync((uint8_t*)recv[d] + (size_t)k * bytes, send[k], bytes, hipMemcpyDeviceToDevice,
                                        st[0]));
        }
        return end(st, err);
    }
    static bool aligned16(const float* const* send, uint32_t n) {
        for (uint32_t r = 0; r < n; r++)
            if ((uintptr_t)send[r] & 15u) return false;
        return true;
    }
    orx_status reduce_scatter(const float* const* send, float* const* recv, size_t block, const hipStream_t* st,
                              std::string& err) override {
        orx_status s = begin(st, err);
        if (s != ORX_OK) return s;
        if (block) {
            GroupPtrs p{};
            for (uint32_t r = 0; r < n; r++) {
                p.in[r] = send[r];
                p.out[r] = recv[r];
            }
            hipLaunchKernelGGL(k_group_reduce_scatter, dim3(stream_grid(block / 4 + 3, n), n), dim3(256), 0, st[0], p, n,
                               block, aligned16(send, n) ? 1 : 0);
        }
        return end(st, err);
    }
    orx_status reduce(const float* const* send, float* recv_root, size_t n_floats, const hipStream_t* st,
                      std::string& err) override {
        orx_status s = begin(st, err);
        if (s != ORX_OK) return s;
        if (n_floats) {
            GroupPtrs p{};
            for (uint32_t r = 0; r < n; r++) p.in[r] = send[r];
            p.out[0] = recv_root;
            hipLaunchKernelGGL(k_group_reduce, dim3(stream_grid(n_floats / 4 + 3)), dim3(256), 0, st[0], p, n, n_floats,
                               aligned16(send, n) ? 1 : 0);
        }
        return end(st, err);
    }
    orx_status all_to_all_v(const float* const* send, float* const* recv, const uint64_t* counts, const hipStream_t* st,
                            std::string& err) override {
        orx_status s0 = begin(st, err);
        if (s0 != ORX_OK) return s0;
        if (!d_runs) {
            COMM_HIP(hipMalloc((void**)&d_runs, (size_t)n * n * sizeof(GroupRun)));
            COMM_HIP(hipEventCreateWithFlags(&ev_runs, hipEventDisableTiming));
            COMM_HIP(hipEventRecord(ev_runs, st[0]));
        }
        h_runs.assign((size_t)n * n, GroupRun{0, 0, 0});
        std::vector<uint64_t> recv_ofs(n, 0);
        uint64_t longest = 0;
        GroupPtrs p{};
        for (uint32_t s = 0; s < n; s++) {
            p.in[s] = send[s];
            p.out[s] = recv[s];
            uint64_t send_ofs = 0;
            for (uint32_t d = 0; d < n; d++) {
                const uint64_t c = counts[(size_t)s * n + d] * ORX_RECORD_DWORDS;
                h_runs[(size_t)s * n + d] = GroupRun{send_ofs, recv_ofs[d], c};
                send_ofs += c;
                recv_ofs[d] += c;
                longest = std::max(longest, c);
            }
        }
        if (longest) {
            /* the table may still be read by the previous call's launch on another stream */
            COMM_HIP(hipStreamWaitEvent(st[0], ev_runs, 0));
            COMM_HIP(hipMemcpyAsync(d_runs, h_runs.data(), h_runs.size() * sizeof(GroupRun), hipMemcpyHostToDevice, st[0]));
            hipLaunchKernelGGL(k_group_all_to_all, dim3(stream_grid((size_t)(longest / 4 + 3), n * n), n * n), dim3(256), 0,
                               st[0], p, n, d_runs);
            COMM_HIP(hipEventRecord(ev_runs, st[0]));
        }
        return end(st, err);
    }
};

/* librccl through dlopen: the handful of entry points and constants of nccl.h this file needs */
struct RcclComm final : GroupComm {
    typedef void* comm_t;
    typedef int (*init_all_t)(comm_t*, int, const int*);
    typedef int (*destroy_t)(comm_t);
    typedef int (*group_t)(void);
    typedef int (*all_gather_t)(const void*, void*, size_t, int, comm_t, hipStream_t);
    typedef int (*reduce_scatter_t)(const void*, void*, size_t, int, int, comm_t, hipStream_t);
    typedef int (*reduce_t)(const void*, void*, size_t, int, int, int, comm_t, hipStream_t);
    typedef int (*send_t)(const void*, size_t, int, int, comm_t, hipStream_t);
    typedef int (*recv_t)(void*, size_t, int, int, comm_t, hipStream_t);
    typedef const char* (*error_string_t)(int);
    enum { NCCL_INT8 = 0, NCCL_FLOAT32 = 7, NCCL_SUM = 0 }; /* ncclDataType_t, ncclRedOp_t */

    void* lib = nullptr;
    init_all_t p_init_all = nullptr;
    destroy_t p_destroy = nullptr;
    group_t p_group_start = nullptr, p_group_end = nullptr;
    all_gather_t p_all_gather = nullptr;
    reduce_scatter_t p_reduce_scatter = nullptr;
    reduce_t p_reduce = nullptr;
    error_string_t p_error_string = nullptr;
    send_t p_send = nullptr; /* resolved by prepare_all_to_all only: older libraries keep working without */
    recv_t p_recv = nullptr;
    uint32_t n = 0;
    std::vector<int> dev;
    std::vector<comm_t> comms;

    ~RcclComm() override {
        for (uint32_t k = 0; k < comms.size(); k++)
            if (comms[k] && p_destroy) {
                hipSetDevice(dev[k]);
                p_destroy(comms[k]);
            }
        /* the library stays loaded: it owns threads and device state beyond its communicators */
    }
    std::string nccl_err(const char* what, int rc) const {
        return std::string("RCCL error in ") + what + ": " + (p_error_string ? p_error_string(rc) : "?");
    }
    /* ORX_ERR_UNSUPPORTED with the dlopen message when the library or one of its symbols is missing */
    orx_status load(std::string& err) {
        const char* names[] = {getenv("ORX_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        std::string msg;
        for (const char* nm : names) {
            if (!nm || !*nm) continue;
            lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
            const char* e = dlerror();
            if (msg.empty()) msg = e ? e : "dlopen failed";
        }
        if (!lib) {
            err = "RCCL communicator unavailable: " + msg;
            return ORX_ERR_UNSUPPORTED;
        }
        struct {
            const char* name;
            void** fn;
        } syms[] = {{"ncclCommInitAll", (void**)&p_init_all},     {"ncclCommDestroy", (void**)&p_destroy},
                    {"ncclGroupStart", (void**)&p_group_start},   {"ncclGroupEnd", (void**)&p_group_end},
                    {"ncclAllGather", (void**)&p_all_gather},     {"ncclReduceScatter", (void**)&p_reduce_scatter},
                    {"ncclReduce", (void**)&p_reduce},            {"ncclGetErrorString", (void**)&p_error_string}};
        for (auto& s : syms) {
            *s.fn = dlsym(lib, s.name);
            if (!*s.fn) {
                const char* e = dlerror();
                err = std::string("RCCL communicator unavailable: ") + (e ? e : s.name);
                return ORX_ERR_UNSUPPORTED;
            }
        }
        return ORX_OK;
    }
    orx_status init(uint32_t world, const int* devices, std::string& err) {
        n = world;
        dev.assign(devices, devices + world);
        orx_status s = load(err);
        if (s != ORX_OK) return s;
        comms.assign(n, nullptr);
        const int rc = p_init_all(comms.data(), (int)n, dev.data());
        if (rc != 0) {
            err = nccl_err("ncclCommInitAll", rc);
            comms.assign(n, nullptr);
            return ORX_ERR_DEVICE;
        }
        return ORX_OK;
    }
    const char* name() const override { return "rccl"; }
    bool shared_device() const override { return false; }

#define COMM_NCCL(x)                  \
    do {                              \
        const int rc_ = (x);          \
        if (rc_ != 0) {               \
            err = nccl_err(#x, rc_);  \
            if (n > 1) p_group_end(); \
            return ORX_ERR_DEVICE;    \
        }                             \
    } while (0)

    orx_status all_gather(const void* const* send, void* const* recv, size_t bytes, const hipStream_t* st,
                          std::string& err) override {
        if (n > 1) COMM_NCCL(p_group_start());
        for (uint32_t k = 0; k < n; k++) {
            COMM_HIP(hipSetDevice(dev[k]));
            COMM_NCCL(p_all_gather(send[k], recv[k], bytes, NCCL_INT8, comms[k], st[k]));
        }
        if (n > 1) {
            const int rc = p_group_end();
            if (rc != 0) {
                err = nccl_err("ncclGroupEnd", rc);
                return ORX_ERR_DEVICE;
            }
        }
        return ORX_OK;
    }
    orx_status reduce_scatter(const float* const* send, float* const* recv, size_t block, const hipStream_t* st,
                              std::string& err) override {
        if (n > 1) COMM_NCCL(p_group_start());
        for (uint32_t k = 0; k < n; k++) {
            COMM_HIP(hipSetDevice(dev[k]));
            COMM_NCCL(p_reduce_scatter(send[k], recv[k], block, NCCL_FLOAT32, NCCL_SUM, comms[k], st[k]));
        }
        if (n > 1) {
            const int rc = p_group_end();
            if (rc != 0) {
                err = nccl_err("ncclGroupEnd", rc);
                return ORX_ERR_DEVICE;
            }
        }
        return ORX_OK;
    }
    orx_status reduce(const float* const* send, float* recv_root, size_t n_floats, const hipStream_t* st,
                      std::string& err) override {
        if (n > 1) COMM_NCCL(p_group_start());
        for (uint32_t k = 0; k < n; k++) {
            COMM_HIP(hipSetDevice(dev[k]));
            /* the receive buffer is used on the root only; the others pass a valid pointer of their own */
            void* recv = k == 0 ? (void*)recv_root : (void*)send[k];
            COMM_NCCL(p_reduce(send[k], recv, n_floats, NCCL_FLOAT32, NCCL_SUM, 0, comms[k], st[k]));
        }
        if (n > 1) {
            const int rc = p_group_end();
            if (rc != 0) {
                err = nccl_err("ncclGroupEnd", rc);
                return ORX_ERR_DEVICE;
            }
        }
        return ORX_OK;
    }
    orx_status prepare_all_to_all(std::string& err) override {
        struct {
            const char* name;
            void** fn;
        } syms[] = {{"ncclSend", (void**)&p_send}, {"ncclRecv", (void**)&p_recv}};
        for (auto& s : syms) {
            *s.fn = lib ? dlsym(lib, s.name) : nullptr;
            if (!*s.fn) {
                const char* e = dlerror();
                err = std::string("RCCL point-to-point unavailable (the photon all-to-all of ORX_PHOTONS_SLABS): ") +
                      (e ? e : s.name);
                return ORX_ERR_UNSUPPORTED;
            }
        }
        return ORX_OK;
    }
    /* one group around every rank's sends and receives of 9 count floats; zero counts are skipped */
    orx_status all_to_all_v(const float* const* send, float* const* recv, const uint64_t* counts, const hipStream_t* st,
                            std::string& err) override {
        if (!p_send || !p_recv) {
            err = "ncclSend / ncclRecv not resolved";
            return ORX_ERR_STATE;
        }
        if (n == 1) { /* nothing to send: the own run, in stream order */
            COMM_HIP(hipSetDevice(dev[0]));
            if (counts[0])
                COMM_HIP(hipMemcpyAsync(recv[0], send[0], (size_t)counts[0] * ORX_RECORD_DWORDS * 4,
                                        hipMemcpyDeviceToDevice, st[0]));
            return ORX_OK;
        }
        COMM_NCCL(p_group_start());
        for (uint32_t k = 0; k < n; k++) {
            COMM_HIP(hipSetDevice(dev[k]));
            uint64_t so = 0, ro = 0;
            for (uint32_t d = 0; d < n; d++) {
                const uint64_t c = counts[(size_t)k * n + d] * ORX_RECORD_DWORDS;
                if (c) COMM_NCCL(p_send(send[k] + so, (size_t)c, NCCL_FLOAT32, (int)d, comms[k], st[k]));
                so += c;
            }
            for (uint32_t s = 0; s < n; s++) {
                const uint64_t c = counts[(size_t)s * n + k] * ORX_RECORD_DWORDS;
                if (c) COMM_NCCL(p_recv(recv[k] + ro, (size_t)c, NCCL_FLOAT32, (int)s, comms[k], st[k]));
                ro += c;
            }
        }
        const int rc = p_group_end();
        if (rc != 0) {
            err = nccl_err("ncclGroupEnd", rc);
            return ORX_ERR_DEVICE;
        }
        return ORX_OK;
    }
};

/* -------------------------------------------------------------------- group ---- */

struct GroupBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
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
};

static thread_local std::string g_create_error;

static orx_status gerr(orx_group* g, orx_status s, const std::string& m) {
    if (g) g->err = m;
    return s;
}
/* a rank's failure, copied with its rank number in front */
static orx_status rank_err(orx_group* g, uint32_t k, orx_status s) {
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

static inline size_t hp_floats(uint32_t max_rows, uint32_t W) { return 7 * (((size_t)max_rows * W + 3) / 4 * 4); }

/* every stream of the group idle: before exchange buffers are replaced or read on the host */
static orx_status group_sync(orx_group* g) {
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

/* the exchange buffers follow the frame size (and the method) of the request */
static orx_status group_prepare(orx_group* g, const orx_request* det) {
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
    const size_t blk = (size_t)g->max_rows * g->W * 3 * 4, hpb = hp_floats(g->max_rows, g->W) * 4;
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

/* SLABS, after the photon trace: histograms -> plan (host) -> pack -> all-to-all of the photon records ->
 * import + grid (multigpu.py slab_exchange), all on the ranks' main streams.  The host waits for the copy of
 * the gathered histograms (that stream only): the one synchronisation per iteration the slab partition adds.
 * When it returns every rank's histogram of this iteration is in, so each rank's main stream is past the
 * previous iteration's import, and the previous all-to-all is done: the record buffers may be replaced. */
static orx_status slab_exchange(orx_group* g, float radius) {
    const uint32_t n = g->n, NB = ORX_GROUP_SLAB_BINS;
    const size_t words = orx_slab_histogram_words(NB);
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
    {
        std::vector<const void*> send(n);
        std::vector<void*> recv(n);
        for (uint32_t k = 0; k < n; k++) {
            GroupRank& q = g->rk[k];
            GRANK(g, k, orx_ppm_slab_histogram(q.r, (uint32_t*)q.hist.p, NB));
            send[k] = q.hist.p;
            recv[k] = gather_holder(g, k).hists.p;
        }
        GCOMM(g, g->comm->all_gather(send.data(), recv.data(), words * 4, st.data(), e_));
    }
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
    std::vector<uint64_t> n_recv(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        uint64_t n_send = 0;
        q.dest_base.assign(n, 0);
        for (uint32_t d = 0; d < n; d++) {
            if (n_send > 0xffffffffull) return gerr(g, ORX_ERR_UNSUPPORTED, "send buffer beyond 2^32 records");
            q.dest_base[d] = (uint32_t)n_send;
            n_send += counts[(size_t)k * n + d];
            n_recv[d] += counts[(size_t)k * n + d];
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
    const size_t hpb = hp_floats(g->max_rows, g->W) * 4, blk = (size_t)g->max_rows * g->W * 12;
    std::vector<const void*> send(n);
    std::vector<void*> recv(n);
    /* eye pass, then export; the all-gather on the communication streams behind it */
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_ppm_local_eye(q.r, it, local_it, radius, det));
        GRANK(g, k, orx_export_hitpoints(q.r, q.hp_local[s].p, hpb));
        GHIP(g, hipEventRecord(q.ev_export, q.main));
        GHIP(g, hipStreamWaitEvent(q.comm, q.ev_export, 0));
        send[k] = q.hp_local[s].p;
        recv[k] = gather_holder(g, k).hp_all[s].p;
    }
    {
        const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.comm; });
        GCOMM(g, g->comm->all_gather(send.data(), recv.data(), hpb, st.data(), e_));
    }
    for (uint32_t k = 0; k < n; k++) {
        GHIP(g, hipSetDevice(g->rk[k].device));
        GHIP(g, hipEventRecord(g->rk[k].ev_gathered, g->rk[k].comm));
    }
    /* the previous iteration's reduce-scatter + finish, issued behind this all-gather */
    orx_status s0 = group_drain(g);
    if (s0 != ORX_OK) return s0;
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
        GRANK(g, k, orx_ppm_gather_external(q.r, recv[k], n, q.ind_partial[s].p, blk * n));
        GHIP(g, hipSetDevice(q.device));
        GHIP(g, hipEventRecord(q.ev_partial, q.side));
    }
    g->pending = s;
    return ORX_OK;
}

static orx_status rows_ppm_serial(orx_group* g, uint64_t it, uint64_t local_it, float radius, const orx_request* det) {
    const uint32_t n = g->n;
    const size_t hpb = hp_floats(g->max_rows, g->W) * 4, blk = (size_t)g->max_rows * g->W * 12;
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
    std::vector<const void*> send(n);
    std::vector<void*> recv(n);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        if (g->slabs) GRANK(g, k, orx_ppm_local_trace(q.r, it, local_it, radius, det));
        else GRANK(g, k, orx_ppm_local_passes(q.r, it, local_it, radius, det));
        GRANK(g, k, orx_export_hitpoints(q.r, q.hp_local[0].p, hpb));
        send[k] = q.hp_local[0].p;
        recv[k] = gather_holder(g, k).hp_all[0].p;
    }
    GCOMM(g, g->comm->all_gather(send.data(), recv.data(), hpb, st.data(), e_));
    if (g->slabs) {
        const orx_status s0 = slab_exchange(g, radius);
        if (s0 != ORX_OK) return s0;
    }
    std::vector<const float*> part(n);
    std::vector<float*> own(n);
    for (uint32_t k = 0; k < n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_ppm_gather_external(q.r, recv[k], n, q.ind_partial[0].p, blk * n));
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
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
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
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
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
        for (int s = 0; s < 2; s++) {
            q.hp_local[s].release();
            q.hp_all[s].release();
            q.ind_partial[s].release();
            q.ind_local[s].release();
        }
        q.splat_all.release();
        q.splat_own.release();
        q.out_local.release();
        q.out_all.release();
        q.conv_local.release();
        q.conv_all.release();
        q.hist.release();
        q.hists.release();
        q.rec_send.release();
        q.rec_recv.release();
    }
    if (g->h_hists) hipHostFree(g->h_hists);
    g->image.release();
    g->dbg_in.release();
    g->dbg_out.release();
    g->conv_full.release();
    g->conv_tiles.release();
    g->display.release();
    delete g;
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
        if (gc.comm == ORX_COMM_RCCL || (gc.comm == ORX_COMM_AUTO && !one_device)) {
            RcclComm* rc = new (std::nothrow) RcclComm();
            g->comm = rc;
            st = rc ? rc->init(n, hip_devices, e) : ORX_ERR_OUT_OF_MEMORY;
        } else {
            LocalComm* lc = new (std::nothrow) LocalComm();
            g->comm = lc;
            st = lc ? lc->init(n, hip_devices[0], e) : ORX_ERR_OUT_OF_MEMORY;
        }
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
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
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
    const size_t need = (size_t)g->W * g->H * 12;
    const size_t blk = (size_t)g->max_rows * g->W * 12;
    std::vector<const void*> send(g->n);
    std::vector<void*> recv(g->n);
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        GRANK(g, k, orx_get_output_device(q.r, q.out_local.p, blk));
        send[k] = q.out_local.p;
        recv[k] = gather_holder(g, k).out_all.p;
    }
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
    GCOMM(g, g->comm->all_gather(send.data(), recv.data(), blk, st.data(), e_));
    GHIP(g, hipSetDevice(root.device));
    hipLaunchKernelGGL(k_group_assemble_rows, dim3(stream_grid(need / 4)), dim3(256), 0, root.main,
                       (const float*)recv[0], g->image.f(), g->W, g->H, g->n, g->max_rows);
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

static bool positive_finite(float x) { return x > 0.0f && x - x == 0.0f; }

orx_status orx_group_get_display(orx_group* g, float inv_iterations, float inv_gamma, int32_t format, uint8_t* dst,
                                 size_t dst_bytes) {
    if (!g || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!positive_finite(inv_iterations) || !positive_finite(inv_gamma))
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
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
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
    if (!positive_finite(floor)) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "floor must be finite and > 0");
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
    std::vector<const void*> send(g->n);
    std::vector<void*> recv(g->n);
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
        send[k] = q.conv_local.p;
        recv[k] = gather_holder(g, k).conv_all.p;
    }
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
    GCOMM(g, g->comm->all_gather(send.data(), recv.data(), blk, st.data(), e_));
    GroupRank& root = g->rk[0];
    GHIP(g, g->conv_full.ensure(root.device, 2 * npx * 4));
    GHIP(g, g->conv_tiles.ensure(root.device, nt * sizeof(orx::ConvTile)));
    GHIP(g, hipSetDevice(root.device));
    float* e = g->conv_full.f();
    float* m = e + npx;
    hipLaunchKernelGGL(k_group_assemble_plane, dim3(stream_grid(npx)), dim3(256), 0, root.main, (const float*)recv[0], e,
                       g->W, g->H, g->n, g->max_rows, 2 * plane, (size_t)0);
    hipLaunchKernelGGL(k_group_assemble_plane, dim3(stream_grid(npx)), dim3(256), 0, root.main, (const float*)recv[0], m,
                       g->W, g->H, g->n, g->max_rows, 2 * plane, plane);
    orx::launch_conv_tiles(root.main, e, m, g->W, g->H, threshold, (orx::ConvTile*)g->conv_tiles.p);
    GHIP(g, hipGetLastError());
    if ((s = group_sync(g)) != ORX_OK) return s;
    std::vector<orx::ConvTile> tiles(nt);
    GHIP(g, hipSetDevice(root.device));
    GHIP(g, hipMemcpy(tiles.data(), g->conv_tiles.p, nt * sizeof(orx::ConvTile), hipMemcpyDeviceToHost));
    orx::conv_finish_tiles(tiles.data(), tx, ty, n, out, tile_error);
    return ORX_OK;
}

/* ---- checkpoint / resume (include/orx.h): ROWS, one frame of the ranks' rows; BATCH, the ranks' frames ---- */

using orx::FNV_BASIS;
using orx::fnv1a64;
using orx::STATE_HEADER_BYTES;
using orx::STATE_KIND_BATCH;
using orx::STATE_KIND_FRAME;
using orx::state_check;
using orx::state_describe;
using orx::state_frame_sections;
using orx::state_open;
using orx::state_rows_export;
using orx::state_rows_import;
using orx::state_seal_frame;
using orx::state_write_header;

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
        auto body = [&]() -> orx_status {
            GHIP(g, words.ensure(root.device, nr));
            GHIP(g, sum.ensure(root.device, no));
            for (uint32_t k = 0; k < g->n; k++) GRANK(g, k, state_rows_export(g->rk[k].r, (uint32_t*)words.p, sum.f(), true));
            const orx_status s = group_sync(g);
            if (s != ORX_OK) return s;
            GHIP(g, hipSetDevice(root.device));
            GHIP(g, hipMemcpy(rng_host, words.p, nr, hipMemcpyDeviceToHost));
            GHIP(g, hipMemcpy(out_host, sum.p, no, hipMemcpyDeviceToHost));
            return ORX_OK;
        };
        const orx_status s = body();
        words.release();
        sum.release();
        return s;
    }
    /* a device per rank: its rows compact on its device, through the host, row by row into the frame */
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        const size_t jr = q.r->rng_rows, jo = q.r->rows;
        GroupBuf words, sum;
        std::vector<uint8_t> hw(jr * rng_row), hs(jo * out_row);
        auto body = [&]() -> orx_status {
            GHIP(g, words.ensure(q.device, jr * rng_row));
            GHIP(g, sum.ensure(q.device, jo * out_row));
            GRANK(g, k, state_rows_export(q.r, (uint32_t*)words.p, sum.f(), false));
            GHIP(g, hipSetDevice(q.device));
            GHIP(g, hipStreamSynchronize(q.main));
            if (!hw.empty()) GHIP(g, hipMemcpy(hw.data(), words.p, hw.size(), hipMemcpyDeviceToHost));
            if (!hs.empty()) GHIP(g, hipMemcpy(hs.data(), sum.p, hs.size(), hipMemcpyDeviceToHost));
            return ORX_OK;
        };
        const orx_status s = body();
        words.release();
        sum.release();
        if (s != ORX_OK) return s;
        for (size_t j = 0; j < jr; j++) std::memcpy(rng_host + (k + j * g->n) * rng_row, hw.data() + j * rng_row, rng_row);
        for (size_t j = 0; j < jo; j++) std::memcpy(out_host + (k + j * g->n) * out_row, hs.data() + j * out_row, out_row);
    }
    return ORX_OK;
}

orx_status orx_group_save_state(orx_group* g, void* dst, size_t dst_bytes) {
    if (!g || !dst) return ORX_ERR_INVALID_ARGUMENT;
    if (!group_has_state(g)) return gerr(g, ORX_ERR_STATE, "no frame rendered yet (BATCH: on every rank)");
    const size_t need = orx_group_state_bytes(g);
    if (dst_bytes < need) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "destination too small");
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
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
            if (g->rk[k].r->st_iter > head.iteration_number) {
                head.iteration_number = g->rk[k].r->st_iter;
                head.ppm_radius = g->rk[k].r->st_radius;
                head.method = g->rk[k].r->st_method;
            }
        head.local_iteration_number = g->calls ? g->calls - 1 : 0;
        state_write_header(&head, fnv1a64(p + STATE_HEADER_BYTES, need - STATE_HEADER_BYTES), FNV_BASIS, p);
        return ORX_OK;
    }
    for (uint32_t k = 0; k < g->n; k++) /* a sharded renderer with a medium box does not exist; as on one renderer */
        if (g->rk[k].r->media) return gerr(g, ORX_ERR_UNSUPPORTED, "participating media: the volumetric photon table is not part of the state");
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
        auto body = [&]() -> orx_status {
            GHIP(g, words.ensure(root.device, nr));
            GHIP(g, sum.ensure(root.device, no));
            GHIP(g, hipSetDevice(root.device));
            GHIP(g, hipMemcpy(words.p, rng_host, nr, hipMemcpyHostToDevice));
            GHIP(g, hipMemcpy(sum.p, out_host, no, hipMemcpyHostToDevice));
            for (uint32_t k = 0; k < g->n; k++)
                GRANK(g, k, state_rows_import(g->rk[k].r, &info, (const uint32_t*)words.p, sum.f(), true));
            return ORX_OK;
        };
        const orx_status s = body();
        words.release();
        sum.release();
        return s;
    }
    auto local_rows = [&](uint32_t total, uint32_t k) { return total > k ? (size_t)(total - k + g->n - 1) / g->n : (size_t)0; };
    for (uint32_t k = 0; k < g->n; k++) {
        GroupRank& q = g->rk[k];
        const size_t jr = local_rows(info.rng_height, k), jo = local_rows(info.height, k);
        std::vector<uint8_t> hw(jr * rng_row), hs(jo * out_row);
        for (size_t j = 0; j < jr; j++) std::memcpy(hw.data() + j * rng_row, rng_host + (k + j * g->n) * rng_row, rng_row);
        for (size_t j = 0; j < jo; j++) std::memcpy(hs.data() + j * out_row, out_host + (k + j * g->n) * out_row, out_row);
        GroupBuf words, sum;
        auto body = [&]() -> orx_status {
            GHIP(g, words.ensure(q.device, hw.size()));
            GHIP(g, sum.ensure(q.device, hs.size()));
            GHIP(g, hipSetDevice(q.device));
            if (!hw.empty()) GHIP(g, hipMemcpy(words.p, hw.data(), hw.size(), hipMemcpyHostToDevice));
            if (!hs.empty()) GHIP(g, hipMemcpy(sum.p, hs.data(), hs.size(), hipMemcpyHostToDevice));
            GRANK(g, k, state_rows_import(q.r, &info, (const uint32_t*)words.p, sum.f(), false));
            return ORX_OK;
        };
        const orx_status s = body();
        words.release();
        sum.release();
        if (s != ORX_OK) return s;
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
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
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
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
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
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
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
    orx_status s = group_drain(g);
    if (s != ORX_OK) return s;
    if ((s = group_sync(g)) != ORX_OK) return s;
    const uint32_t n = g->n;
    const int dev = g->rk[0].device;
    std::vector<size_t> ns(n, 0), nr(n, 0), so(n + 1, 0), ro(n + 1, 0); /* floats; padded offsets */
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = 0; b < n; b++) {
            if (counts[(size_t)a * n + b] > 0xffffffffull) return gerr(g, ORX_ERR_INVALID_ARGUMENT, "run beyond 2^32 records");
            ns[a] += (size_t)counts[(size_t)a * n + b] * ORX_RECORD_DWORDS;
            nr[b] += (size_t)counts[(size_t)a * n + b] * ORX_RECORD_DWORDS;
        }
    for (uint32_t k = 0; k < n; k++) {
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
    const std::vector<hipStream_t> st = streams_of(g, [](GroupRank& q) { return q.main; });
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
