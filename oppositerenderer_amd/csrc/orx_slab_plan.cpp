/*
 * orx_slab_plan.cpp — see orx_slab_plan.h.  Integer counts are summed exactly (uint64, or doubles
 * below 2^53); only the normalised weights are inexact.  One plan serves every rank of a group, so a
 * last-bit difference from the NumPy planner (its pairwise sums) changes no result: both are valid
 * partitions.
 */
#include "orx_slab_plan.h"

#include <cmath>
#include <cstddef>
#include <vector>

#include "orx.h"

namespace orx {

static inline size_t hist_words(uint32_t nb) {
    return (size_t)6 * nb + 6 + (size_t)2 * ORX_SLAB_VOXELS * ORX_SLAB_VOXELS * ORX_SLAB_VOXELS;
}

const char* slab_plan(const uint32_t* hists, uint32_t world, uint32_t nb, const uint32_t* halo_bins, const SlabWeights& wt,
                      uint32_t* axis_out, uint8_t* bin_dest, uint64_t* counts, uint32_t* photon_box) {
    if (!hists || !axis_out || !bin_dest || !counts) return "orx_slab_plan: NULL argument";
    if (world == 0 || world > ORX_SLAB_PLAN_MAX_WORLD) return "orx_slab_plan: 1 to 64 ranks";
    if (nb < ORX_SLAB_VOXELS || nb > ORX_SLAB_PLAN_MAX_BINS || nb % ORX_SLAB_VOXELS)
        return "orx_slab_plan: nbins must be a multiple of ORX_SLAB_VOXELS, at most 1024";
    const uint32_t V = ORX_SLAB_VOXELS, V3 = V * V * V, layer = nb / V;
    const size_t words = hist_words(nb);

    /* voxel counts over the ranks, then hit points x photons per voxel */
    std::vector<double> vph(V3, 0.0), vhp(V3, 0.0);
    for (uint32_t s = 0; s < world; s++) {
        const uint32_t* v = hists + s * words + (size_t)6 * nb + 6;
        for (uint32_t i = 0; i < V3; i++) {
            vph[i] += (double)v[i];
            vhp[i] += (double)v[V3 + i];
        }
    }

    std::vector<double> ph(nb), hp(nb), w(nb), slab(world);
    std::vector<uint8_t> dest(nb);
    double best_cost = 0.0;
    int best = -1;
    for (uint32_t a = 0; a < 3; a++) {
        for (uint32_t b = 0; b < nb; b++) {
            uint64_t p = 0, h = 0;
            for (uint32_t s = 0; s < world; s++) {
                p += hists[s * words + (size_t)a * nb + b];
                h += hists[s * words + (size_t)(3 + a) * nb + b];
            }
            ph[b] = (double)p;
            hp[b] = (double)h;
        }
        /* per voxel layer of this axis: the gather cost of one hit point */
        double lc[ORX_SLAB_VOXELS] = {}, lh[ORX_SLAB_VOXELS] = {};
        for (uint32_t z = 0; z < V; z++)
            for (uint32_t y = 0; y < V; y++)
                for (uint32_t x = 0; x < V; x++) {
                    const uint32_t i = x + V * (y + V * z), l = a == 0 ? x : a == 1 ? y : z;
                    lc[l] += vph[i] * vhp[i];
                    lh[l] += vhp[i];
                }
        for (uint32_t b = 0; b < nb; b++) w[b] = 0.0;
        for (int term = 0; term < 3; term++) {
            const double weight = term == 0 ? wt.gather : term == 1 ? wt.photon : wt.pixel;
            double tot = 0.0;
            auto part = [&](uint32_t b) {
                if (term == 1) return ph[b];
                if (term == 2) return hp[b];
                const uint32_t l = b / layer;
                return hp[b] * (lh[l] > 0.0 ? lc[l] / lh[l] : 0.0);
            };
            for (uint32_t b = 0; b < nb; b++) tot += part(b);
            if (tot > 0.0)
                for (uint32_t b = 0; b < nb; b++) w[b] += weight * part(b) / tot;
        }
        double total = 0.0;
        for (uint32_t b = 0; b < nb; b++) total += w[b];
        std::vector<uint8_t> d(nb);
        double cost = 0.0;
        if (total > 0.0) {
            /* the rank whose share of the cumulative cost holds the bin's midpoint */
            double cum = 0.0;
            for (uint32_t r = 0; r < world; r++) slab[r] = 0.0;
            for (uint32_t b = 0; b < nb; b++) {
                cum += w[b];
                const double mid = cum - 0.5 * w[b];
                double f = std::floor(mid * (double)world / total);
                if (!(f >= 0.0)) f = 0.0;
                if (f > (double)(world - 1)) f = (double)(world - 1);
                d[b] = (uint8_t)f;
                /* cumulative midpoints ascend; keep the table ascending against rounding too */
                if (b && d[b] < d[b - 1]) d[b] = d[b - 1];
                slab[d[b]] += w[b];
            }
            for (uint32_t r = 0; r < world; r++)
                if (slab[r] > cost) cost = slab[r];
        } else {
            for (uint32_t b = 0; b < nb; b++) {
                const uint32_t r = (uint32_t)((uint64_t)b * world / nb);
                d[b] = (uint8_t)(r < world - 1 ? r : world - 1);
            }
        }
        if (best < 0 || cost < best_cost) { /* ties: the lower axis */
            best = (int)a;
            best_cost = cost;
            dest = d;
        }
    }

    const uint32_t axis = (uint32_t)best;
    const uint64_t halo = halo_bins ? halo_bins[axis] : 0;
    for (size_t i = 0; i < (size_t)world * world; i++) counts[i] = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t d0 = dest[b > halo ? b - halo : 0];
        const uint32_t d1 = dest[b + halo < nb ? b + halo : nb - 1];
        for (uint32_t s = 0; s < world; s++) {
            const uint64_t p = hists[s * words + (size_t)axis * nb + b];
            if (!p) continue;
            for (uint32_t d = d0; d <= d1; d++) counts[(size_t)s * world + d] += p;
        }
    }
    if (photon_box) {
        for (int k = 0; k < 6; k++) photon_box[k] = k < 3 ? 0xffffffffu : 0u;
        for (uint32_t s = 0; s < world; s++) {
            const uint32_t* box = hists + s * words + (size_t)6 * nb;
            for (int k = 0; k < 3; k++) {
                if (box[k] < photon_box[k]) photon_box[k] = box[k];
                if (box[3 + k] > photon_box[3 + k]) photon_box[3 + k] = box[3 + k];
            }
        }
    }
    *axis_out = axis;
    for (uint32_t b = 0; b < nb; b++) bin_dest[b] = dest[b];
    return nullptr;
}

void slab_owned(const uint8_t* bin_dest, uint32_t nb, uint32_t rank, uint32_t* lo, uint32_t* hi) {
    *lo = 1;
    *hi = 0;
    bool any = false;
    for (uint32_t b = 0; b < nb; b++) {
        if (bin_dest[b] != rank) continue;
        if (!any) *lo = b;
        *hi = b;
        any = true;
    }
}

SlabRunLayout slab_run_layout(const uint64_t* counts, uint32_t n) {
    const std::vector<uint64_t> runs((size_t)n * n), ranks(n, 0);
    SlabRunLayout l{runs, runs, ranks, ranks};
    for (uint32_t s = 0; s < n; s++)
        for (uint32_t d = 0; d < n; d++) {
            const size_t i = (size_t)s * n + d;
            l.send_ofs[i] = l.send_total[s];
            l.recv_ofs[i] = l.recv_total[d];
            l.send_total[s] += counts[i];
            l.recv_total[d] += counts[i];
        }
    return l;
}

}  // namespace orx

extern "C" orx_status orx_slab_plan(const uint32_t* hists, uint32_t world, uint32_t nbins, const uint32_t halo_bins[3],
                                    uint32_t* axis, uint8_t* bin_dest, uint64_t* counts, uint32_t photon_box[6]) {
    return orx::slab_plan(hists, world, nbins, halo_bins, orx::SlabWeights(), axis, bin_dest, counts, photon_box)
               ? ORX_ERR_INVALID_ARGUMENT
               : ORX_OK;
}
