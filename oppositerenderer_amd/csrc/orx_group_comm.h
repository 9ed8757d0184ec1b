/*
 * orx_group_comm.h — what a render group (orx_group.hip) asks of its communicator (orx_group_comm.hip): the
 * collectives between the ranks' buffers and the kernels that put gathered rank blocks back into a frame.
 * Internal: not installed, nothing under include/ sees it.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "orx.h"

#define ORX_GROUP_MAX 64u
#define ORX_GROUP_SLAB_BINS 1024u /* multigpu.SLAB_BINS */
#define ORX_RECORD_DWORDS 9u      /* a photon record: position, direction, power */

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
     * d = 0..n-1 back to back, recv[d] receives the runs of s = 0..n-1 back to back (orx::slab_run_layout); the
     * caller sizes both. */
    virtual orx_status all_to_all_v(const float* const* send, float* const* recv, const uint64_t* counts,
                                    const hipStream_t* st, std::string& err) = 0;
};

/* The communicator of n ranks on `devices` (one_device: all the same): RCCL when `comm` (orx_group_config.comm)
 * asks for it or ORX_COMM_AUTO meets more than one device, else LOCAL.  On failure *out is still the caller's to
 * delete (or nullptr) and `err` says why. */
orx_status group_comm_create(uint32_t comm, uint32_t n, const int* devices, bool one_device, GroupComm** out,
                             std::string& err);

/* rank blocks [n][max_rows][W][3] (local row j of rank g = global row g + j n) -> out [H][W][3], on st */
void group_assemble_rows(hipStream_t st, const float* blocks, float* out, uint32_t W, uint32_t H, uint32_t n,
                         uint32_t max_rows);
/* the one-channel sibling: rank blocks of `block` floats each, whose plane at `off` is [max_rows][W] -> out [H][W] */
void group_assemble_plane(hipStream_t st, const float* blocks, float* out, uint32_t W, uint32_t H, uint32_t n,
                          uint32_t max_rows, size_t block, size_t off);
