/*
 * orx_bvh_host.h — the host BVH builder: binned-SAH binary build, treelet
 * restructuring and the collapse to four-wide quantised nodes.  It is the
 * reference the device builder (orx_bvh.hip) is compared against, the builder
 * behind ORX_BVH_HOST=1 and the only one for the fp32-box variant.  Plain C++:
 * no HIP, so it can be built, tested and sanitised without a GPU.
 */
#pragma once

#include <stdint.h>

#include <vector>

#include "orx_bvh_nodes.h"

namespace orx {

struct HostBvh4 {
    std::vector<DevBvh4> nodes;    /* quantised four-wide nodes, root at 0 */
    std::vector<DevBvh4F> nodes_f; /* same topology, fp32 child boxes */
    std::vector<uint32_t> leaf_order; /* position k holds the original id of the k-th triangle in leaf order */
    uint32_t stack_bound = 0;      /* the most stack entries a traversal can hold */
    uint32_t depth = 0;            /* depth of the binary tree the nodes were collapsed from */
};

/* the defaults overridden by ORX_BVH_BINS, ORX_BVH_LEAF_MAX, ORX_BVH_LEAF_SAH, ORX_BVH_TREELET,
 * ORX_BVH_TREELET_LEAVES and ORX_BVH_COLLAPSE, each clamped to its range */
BvhBuildOptions bvh_options_from_env();

/* vertices: float3 per vertex; indices: three per triangle, nt > 0 triangles.
 * Returns nullptr on success, else a static message; *out is then unspecified. */
const char* build_host_bvh4(const float* vertices, const uint32_t* indices, uint32_t nt, const BvhBuildOptions& opt,
                            HostBvh4* out);

}  // namespace orx
