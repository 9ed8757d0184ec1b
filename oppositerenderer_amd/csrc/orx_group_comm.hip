/*
 * orx_group_comm.hip — the communicators of a render group (orx_group.hip) and the group's kernels.
 *
 *   LOCAL  every rank on one device in one process: the all-gather is device-to-device copies, the two
 *          sums are the kernels below (rank order 0..n-1 in fp32, no atomics: equal to a sequential
 *          float32 sum on the host)
 *   RCCL   librccl opened with dlopen when selected (liborx.so has no link dependency on it), one
 *          communicator per rank (ncclCommInitAll), group calls around the collectives
 *
 * The photon records of ORX_PHOTONS_SLABS are moved by GroupComm::all_to_all_v (LOCAL: one launch
 * of k_group_all_to_all; RCCL: ncclSend / ncclRecv in one group, unmeasured on hardware like every N > 1
 * collective over RCCL: one GPU per box, and RCCL refuses two ranks on one GPU).
 */
#include "orx_group_comm.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "orx_slab_plan.h"

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

void group_assemble_rows(hipStream_t st, const float* blocks, float* out, uint32_t W, uint32_t H, uint32_t n,
                         uint32_t max_rows) {
    hipLaunchKernelGGL(k_group_assemble_rows, dim3(stream_grid((size_t)W * H * 3)), dim3(256), 0, st, blocks, out, W, H, n,
                       max_rows);
}

void group_assemble_plane(hipStream_t st, const float* blocks, float* out, uint32_t W, uint32_t H, uint32_t n,
                          uint32_t max_rows, size_t block, size_t off) {
    hipLaunchKernelGGL(k_group_assemble_plane, dim3(stream_grid((size_t)W * H)), dim3(256), 0, st, blocks, out, W, H, n,
                       max_rows, block, off);
}

/* ------------------------------------------------------------- communicator ---- */

#define COMM_HIP(x)                                                                   \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            err = std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_); \
            return e_ == hipErrorOutOfMemory ? ORX_ERR_OUT_OF_MEMORY : ORX_ERR_DEVICE; \
        }                                                                             \
    } while (0)

namespace {

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
        const orx::SlabRunLayout lay = orx::slab_run_layout(counts, n);
        h_runs.resize((size_t)n * n);
        uint64_t longest = 0;
        GroupPtrs p{};
        for (uint32_t s = 0; s < n; s++) {
            p.in[s] = send[s];
            p.out[s] = recv[s];
        }
        for (size_t i = 0; i < h_runs.size(); i++) {
            h_runs[i] = GroupRun{lay.send_ofs[i] * ORX_RECORD_DWORDS, lay.recv_ofs[i] * ORX_RECORD_DWORDS,
                                 counts[i] * ORX_RECORD_DWORDS};
            longest = std::max(longest, h_runs[i].n);
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
    struct Sym {
        const char* name;
        void** fn;
    };
    /* every symbol from the library, or ORX_ERR_UNSUPPORTED and `what` with the dlsym message (the name without one) */
    orx_status resolve(std::initializer_list<Sym> syms, const char* what, std::string& err) {
        for (const Sym& s : syms) {
            *s.fn = lib ? dlsym(lib, s.name) : nullptr;
            if (!*s.fn) {
                const char* e = dlerror();
                err = std::string(what) + (e ? e : s.name);
                return ORX_ERR_UNSUPPORTED;
            }
        }
        return ORX_OK;
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
        return resolve({{"ncclCommInitAll", (void**)&p_init_all},   {"ncclCommDestroy", (void**)&p_destroy},
                        {"ncclGroupStart", (void**)&p_group_start}, {"ncclGroupEnd", (void**)&p_group_end},
                        {"ncclAllGather", (void**)&p_all_gather},   {"ncclReduceScatter", (void**)&p_reduce_scatter},
                        {"ncclReduce", (void**)&p_reduce},          {"ncclGetErrorString", (void**)&p_error_string}},
                       "RCCL communicator unavailable: ", err);
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

    /* `call(k)` for every rank on its device, in one group when there is more than one rank */
    template <class F>
    orx_status grouped(std::string& err, F call) {
        if (n > 1) COMM_NCCL(p_group_start());
        for (uint32_t k = 0; k < n; k++) {
            COMM_HIP(hipSetDevice(dev[k]));
            const orx_status s = call(k);
            if (s != ORX_OK) return s;
        }
        const int rc = n > 1 ? p_group_end() : 0;
        if (rc != 0) {
            err = nccl_err("ncclGroupEnd", rc);
            return ORX_ERR_DEVICE;
        }
        return ORX_OK;
    }
    orx_status all_gather(const void* const* send, void* const* recv, size_t bytes, const hipStream_t* st,
                          std::string& err) override {
        return grouped(err, [&](uint32_t k) -> orx_status {
            COMM_NCCL(p_all_gather(send[k], recv[k], bytes, NCCL_INT8, comms[k], st[k]));
            return ORX_OK;
        });
    }
    orx_status reduce_scatter(const float* const* send, float* const* recv, size_t block, const hipStream_t* st,
                              std::string& err) override {
        return grouped(err, [&](uint32_t k) -> orx_status {
            COMM_NCCL(p_reduce_scatter(send[k], recv[k], block, NCCL_FLOAT32, NCCL_SUM, comms[k], st[k]));
            return ORX_OK;
        });
    }
    orx_status reduce(const float* const* send, float* recv_root, size_t n_floats, const hipStream_t* st,
                      std::string& err) override {
        return grouped(err, [&](uint32_t k) -> orx_status {
            /* the receive buffer is used on the root only; the others pass a valid pointer of their own */
            void* recv = k == 0 ? (void*)recv_root : (void*)send[k];
            COMM_NCCL(p_reduce(send[k], recv, n_floats, NCCL_FLOAT32, NCCL_SUM, 0, comms[k], st[k]));
            return ORX_OK;
        });
    }
    orx_status prepare_all_to_all(std::string& err) override {
        return resolve({{"ncclSend", (void**)&p_send}, {"ncclRecv", (void**)&p_recv}},
                       "RCCL point-to-point unavailable (the photon all-to-all of ORX_PHOTONS_SLABS): ", err);
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
        const orx::SlabRunLayout lay = orx::slab_run_layout(counts, n);
        return grouped(err, [&](uint32_t k) -> orx_status {
            for (uint32_t d = 0; d < n; d++) {
                const size_t i = (size_t)k * n + d;
                const uint64_t c = counts[i] * ORX_RECORD_DWORDS, so = lay.send_ofs[i] * ORX_RECORD_DWORDS;
                if (c) COMM_NCCL(p_send(send[k] + so, (size_t)c, NCCL_FLOAT32, (int)d, comms[k], st[k]));
            }
            for (uint32_t s = 0; s < n; s++) {
                const size_t i = (size_t)s * n + k;
                const uint64_t c = counts[i] * ORX_RECORD_DWORDS, ro = lay.recv_ofs[i] * ORX_RECORD_DWORDS;
                if (c) COMM_NCCL(p_recv(recv[k] + ro, (size_t)c, NCCL_FLOAT32, (int)s, comms[k], st[k]));
            }
            return ORX_OK;
        });
    }
};

}  // namespace

orx_status group_comm_create(uint32_t comm, uint32_t n, const int* devices, bool one_device, GroupComm** out,
                             std::string& err) {
    if (comm == ORX_COMM_RCCL || (comm == ORX_COMM_AUTO && !one_device)) {
        RcclComm* rc = new (std::nothrow) RcclComm();
        *out = rc;
        return rc ? rc->init(n, devices, err) : ORX_ERR_OUT_OF_MEMORY;
    }
    LocalComm* lc = new (std::nothrow) LocalComm();
    *out = lc;
    return lc ? lc->init(n, devices[0], err) : ORX_ERR_OUT_OF_MEMORY;
}
