/*
 * orx_slab_plan.h — the host planner of the spatial photon partition ("slab mode", include/orx.h
 * orx_set_slab_partition): from the all-gathered histograms of one iteration to one axis, the
 * bin -> rank table, the photon all-to-all's counts and the union photon AABB.  It restates
 * multigpu.split_slab_hists, slab_plan (the voxel form), slab_counts and slab_owned in double
 * precision.  Plain C++: no HIP, so it can be built, tested and sanitised without a GPU.  The C entry
 * point orx_slab_plan (include/orx.h) is defined in the same unit.
 */
#pragma once

#include <stdint.h>

#include <vector>

namespace orx {

#define ORX_SLAB_PLAN_MAX_WORLD 64u
#define ORX_SLAB_PLAN_MAX_BINS 1024u

/* the relative weights of a bin's cost: the gather (hit points x photons of their voxel), the import
 * and grid build (photons), the per-pixel work (hit points); each term normalised to sum 1 */
struct SlabWeights {
    double gather = 0.8, photon = 0.15, pixel = 0.05;
};

/* hists: [world][6 nbins + 6 + 2 V^3] words as orx_ppm_slab_histogram writes them; halo_bins: one per
 * axis (NULL: 0).  Writes the axis, bin_dest[nbins] (ascending ranks), counts[world][world] (records
 * rank s sends to rank d, halo copies included) and photon_box[6] (NULL: not wanted).  Returns nullptr
 * on success, else a static message (an argument out of range; nothing is written then). */
const char* slab_plan(const uint32_t* hists, uint32_t world, uint32_t nbins, const uint32_t* halo_bins,
                      const SlabWeights& w, uint32_t* axis, uint8_t* bin_dest, uint64_t* counts, uint32_t* photon_box);

/* the bins `rank` owns, [*lo, *hi]; *lo > *hi (1, 0) when it owns none */
void slab_owned(const uint8_t* bin_dest, uint32_t nbins, uint32_t rank, uint32_t* lo, uint32_t* hi);

/* Where the runs of the photon all-to-all lie, in records, from counts[n][n]: rank s's send buffer holds its
 * runs for d = 0..n-1 back to back, rank d's receive buffer the runs of s = 0..n-1 back to back.
 * send_ofs / recv_ofs [n][n]: the start of run (s, d) in s's send and in d's receive buffer;
 * send_total / recv_total [n]: the records a rank sends and receives. */
struct SlabRunLayout {
    std::vector<uint64_t> send_ofs, recv_ofs, send_total, recv_total;
};
SlabRunLayout slab_run_layout(const uint64_t* counts, uint32_t n);

}  // namespace orx
