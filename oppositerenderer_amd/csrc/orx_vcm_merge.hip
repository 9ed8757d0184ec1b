/*
 * orx_vcm_merge.hip — the vertex-merging half of VCM for gfx950 (orx_config.vcm_merging).
 *
 * The reference ships vertex connection only (m_vcmUseVM = false, OptixRenderer.cpp:301) and has no
 * merging program, so the definition is the published algorithm (Georgiev et al., "Light Transport
 * Simulation with Vertex Connection and Merging", tech. rep. eqs. 37-41; SmallVCM
 * RangeQuery::Process) in this renderer's own quantities:
 *
 *   at every camera vertex at which connections are made (non-specular, any depth up to
 *   vcm_max_path_length), for every stored light vertex of ANY subpath with
 *       d = lightPos - camPos,  dot(d, d) <= r^2            (fp32, x*x + y*y + z*z)
 *   lightDir = the light vertex's world dirFix
 *   f = cameraBsdf.vcm_f(lightDir, cos, dirPdfW, revPdfW)   (pair skipped when f is zero)
 *   dirPdfW *= cameraBsdf.cont;  revPdfW *= lightBsdf.cont
 *   wLight  = L.dVCM * misVc + L.dVM * dirPdfW
 *   wCamera = C.dVCM * misVc + C.dVM * revPdfW
 *   contrib += f * L.throughput / (wLight + 1 + wCamera)
 *   colour  += C.throughput * vm_normalization * contrib
 *
 * There is no combined path-length cap: connectVertices has none either (vcm.h:315-400), so
 * connection and merging weight the same path set.
 *
 * Passes (all on the renderer's stream, serial):
 *   grid   after the light pass: every slot (k, p) of the light-vertex cache gets its cell (G for an
 *          empty slot), a stable radix sort orders them (cell order, slot order inside a cell:
 *          deterministic), and the valid ones are rewritten as three cell-ordered float4 planes
 *          pos|dVCM, throughput|dVM, worldDir|cont, so the merge never touches the four cache planes
 *   merge  after the camera pass's resolve: one lane per camera-vertex record (k, p), k-major (a wave
 *          holds 64 neighbouring pixels of one depth); the lane walks the cell rows its sphere
 *          overlaps, tests the distance on the first plane and loads the other two only for accepted
 *          pairs; its colour goes to part[k][p] with a plain store
 *   sum    per pixel, part[0..n-1][p] in order -> merge, and added to the camera colour and the output
 * No float atomics anywhere: two runs give the same bits.  Every index read from a count, offset or
 * record is bounded before it is used.
 */
#include <hipcub/hipcub.hpp>

#include "orx_kernels.h"
#include "orx_vcm_bsdf.h"

namespace orx {

/* cell coordinate of v on one axis, clamped into the grid (NaN: cell 0) */
__device__ __forceinline__ uint32_t mg_cell1(float v, float o, float inv, uint32_t g) {
    const float f = orx_floorf((v - o) * inv);
    if (!(f > 0.f)) return 0u;
    return f >= (float)g ? g - 1u : (uint32_t)f;
}

__global__ __launch_bounds__(256) void k_vcm_merge_keys(VcmBufs vb, VcmMergeBufs mb, VcmMergeGrid g, uint32_t lcount) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mb.nslots) return;
    const uint32_t k = i / lcount, p = i - k * lcount;
    uint32_t key = g.G;
    const uint32_t n = min(vb.vcount[p], VCM_MAX_VERTS);
    if (k < n) {
        const float4 A = vb.vA[i];
        key = mg_cell1(A.x, g.ox, g.inv, g.gx) +
              g.gx * (mg_cell1(A.y, g.oy, g.inv, g.gy) + g.gy * mg_cell1(A.z, g.oz, g.inv, g.gz));
    }
    mb.keys[i] = key;
    mb.vals[i] = i;
}
/* start[c] = first sorted slot of cell c (lower bound), c in [0, G + 1]; start[G] = valid vertices */
__global__ __launch_bounds__(256) void k_vcm_merge_starts(VcmMergeBufs mb, uint32_t G) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > G + 1u) return;
    uint32_t lo = 0, hi = mb.nslots;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mb.keys_sorted[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    mb.start[c] = lo;
}
/* the valid light vertices in cell order, as the merge reads them.  The continuation probability is
 * that of the BSDF connect_vertex rebuilds at the vertex: Lambert from Kd (the texel colour for Texture),
 * plus Phong for Glossy */
__global__ __launch_bounds__(256) void k_vcm_merge_records(DevScene S, VcmBufs vb, VcmMergeBufs mb, uint32_t G) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= min(mb.start[G], mb.nslots)) return;
    const uint32_t s = mb.vals_sorted[j];
    if (s >= mb.nslots) { /* not a slot: an inert record (no sort output is) */
        mb.lr0[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        mb.lr1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        mb.lr2[j] = make_float4(0.f, 0.f, 1.f, 0.f);
        return;
    }
    const float4 A = vb.vA[s], B = vb.vB[s], Cn = vb.vC[s], D = vb.vD[s];
    const uint32_t mi = __float_as_uint(A.w);
    f3 thr = mk(B.x, B.y, B.z);
    float cont = 0.f;
    if (mi < mb.nmats) {
        const DevMaterial& m = S.mats[mi];
        f3 kd = m.Kd;
        if (vb.vE && m.type == MAT_TEXTURE) {
            const float4 E = vb.vE[s];
            kd = mk(E.x, E.y, E.z);
        }
        const f3 fix = mk(D.x, D.y, D.z);
        cont = fminf(1.f, cont + bx_cont(mk_bx(T_LAMBERT, kd), fix));
        if (m.type == MAT_GLOSSY) cont = fminf(1.f, cont + bx_cont(mk_bx(T_PHONG, m.Ks, m.exponent), fix));
    } else {
        thr = mk1(0.f);
    }
    const f3 wdir = frame_from_normal(mk(Cn.x, Cn.y, Cn.z)).to_world(mk(D.x, D.y, D.z));
    mb.lr0[j] = make_float4(A.x, A.y, A.z, B.w);
    mb.lr1[j] = make_float4(thr.x, thr.y, thr.z, D.w);
    mb.lr2[j] = make_float4(wdir.x, wdir.y, wdir.z, cont);
}

/* one lane per camera-vertex record i = k * lcount + p */
__global__ __launch_bounds__(256) void k_vcm_merge(DevScene S, VcmBufs vb, VcmMergeBufs mb, VcmMergeGrid g,
                                                   uint32_t lcount) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= vb.cvmax * lcount) return;
    const uint32_t k = i / lcount, p = i - k * lcount;
    if (k >= min(vb.cvcount[p], vb.cvmax)) return;
    const float4 A = vb.cvA[i], B = vb.cvB[i], Cn = vb.cvC[i], D = vb.cvD[i];
    const uint32_t mi = __float_as_uint(A.w);
    const f3 hit = mk(A.x, A.y, A.z);
    f3 contrib = mk1(0.f);
    uint32_t accepted = 0, cand = 0;
    if (mi < mb.nmats) {
        /* the camera BSDF as material_bsdf builds it at a non-specular vertex (Diffuse, Texture, Glossy) */
        const DevMaterial& m = S.mats[mi];
        f3 kd = m.Kd;
        if (vb.cvE && m.type == MAT_TEXTURE) {
            const float4 E = vb.cvE[i];
            kd = mk(E.x, E.y, E.z);
        }
        VBsdf cb;
        cb.init(mk(Cn.x, Cn.y, Cn.z), -mk(D.x, D.y, D.z), false);
        cb.add(mk_bx(T_LAMBERT, kd));
        if (m.type == MAT_GLOSSY) cb.add(mk_bx(T_PHONG, m.Ks, m.exponent));
        const float cdVCM = B.w * g.misVc, cdVM = Cn.w;
        const uint32_t x0 = mg_cell1(hit.x - g.rq, g.ox, g.inv, g.gx), x1 = mg_cell1(hit.x + g.rq, g.ox, g.inv, g.gx);
        const uint32_t y0 = mg_cell1(hit.y - g.rq, g.oy, g.inv, g.gy), y1 = mg_cell1(hit.y + g.rq, g.oy, g.inv, g.gy);
        const uint32_t z0 = mg_cell1(hit.z - g.rq, g.oz, g.inv, g.gz), z1 = mg_cell1(hit.z + g.rq, g.oz, g.inv, g.gz);
        const uint32_t nvalid = min(mb.start[g.G], mb.nslots);
        for (uint32_t z = z0; z <= z1; ++z)
            for (uint32_t y = y0; y <= y1; ++y) {
                /* the cells x0..x1 of a row are contiguous in the sorted order */
                const uint32_t row = g.gx * (y + g.gy * z);
                const uint32_t jb = min(mb.start[row + x0], nvalid), je = min(mb.start[row + x1 + 1u], nvalid);
                for (uint32_t j = jb; j < je; ++j) {
                    const float4 R0 = mb.lr0[j];
                    const f3 d = mk(R0.x, R0.y, R0.z) - hit;
                    const float d2 = dot(d, d);
                    cand++;
                    if (!(d2 <= g.r2)) continue;
                    accepted++;
                    const float4 R1 = mb.lr1[j], R2 = mb.lr2[j];
                    float cosv = 0.f, dirPdfW, revPdfW;
                    const f3 f = cb.vcm_f(mk(R2.x, R2.y, R2.z), cosv, dirPdfW, revPdfW);
                    if (iszero(f)) continue;
                    dirPdfW *= cb.cont;
                    revPdfW *= R2.w;
                    const float wLight = R0.w * g.misVc + R1.w * dirPdfW;
                    const float wCamera = cdVCM + cdVM * revPdfW;
                    const float misWeight = 1.f / (wLight + 1.f + wCamera);
                    contrib = contrib + (f * misWeight) * mk(R1.x, R1.y, R1.z);
                }
            }
    }
    const f3 col = (mk(B.x, B.y, B.z) * g.vmNorm) * contrib;
    mb.part[i] = make_float4(col.x, col.y, col.z, __uint_as_float(accepted));
    if (mb.cand) mb.cand[i] = cand;
}

/* the pixel's merging colour, its records' parts added in order, then what camera_finish / k_vcm_accum
 * did with the connections' colour: into the camera colour and the running sum */
__global__ __launch_bounds__(256) void k_vcm_merge_sum(VcmBufs vb, VcmMergeBufs mb, uint32_t lcount) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= lcount) return;
    const uint32_t n = min(vb.cvcount[p], vb.cvmax);
    f3 color = mk1(0.f);
    uint32_t acc = 0, cand = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const size_t i = (size_t)k * lcount + p;
        const float4 a = mb.part[i];
        color = color + mk(a.x, a.y, a.z);
        acc += __float_as_uint(a.w);
        if (mb.cand) cand += mb.cand[i];
    }
    const size_t o3 = 3 * (size_t)p;
    mb.merge[o3 + 0] = color.x;
    mb.merge[o3 + 1] = color.y;
    mb.merge[o3 + 2] = color.z;
    vb.cam[o3 + 0] = vb.cam[o3 + 0] + color.x;
    vb.cam[o3 + 1] = vb.cam[o3 + 1] + color.y;
    vb.cam[o3 + 2] = vb.cam[o3 + 2] + color.z;
    vb.output[o3 + 0] = vb.output[o3 + 0] + color.x;
    vb.output[o3 + 1] = vb.output[o3 + 1] + color.y;
    vb.output[o3 + 2] = vb.output[o3 + 2] + color.z;
    if (mb.mcount) {
        mb.mcount[2 * (size_t)p] = acc;
        mb.mcount[2 * (size_t)p + 1] = cand;
    }
}

size_t vcm_merge_sort_tmp_bytes(uint32_t nslots) {
    size_t bytes = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nslots);
    return bytes;
}

void launch_vcm_merge_grid(hipStream_t s, const DevScene& S, const VcmBufs& vb, const VcmMergeBufs& mb,
                           const VcmMergeGrid& g, uint32_t lcount) {
    if (!mb.nslots || !lcount) return;
    const uint32_t bN = (mb.nslots + 255) / 256;
    hipLaunchKernelGGL(k_vcm_merge_keys, dim3(bN), dim3(256), 0, s, vb, mb, g, lcount);
    int end_bit = 1; /* keys 0..G */
    while (end_bit < 32 && ((uint64_t)g.G >> end_bit)) end_bit++;
    size_t bytes = mb.sort_tmp_bytes;
    hipcub::DeviceRadixSort::SortPairs(mb.sort_tmp, bytes, (const uint32_t*)mb.keys, mb.keys_sorted,
                                       (const uint32_t*)mb.vals, mb.vals_sorted, (int)mb.nslots, 0, end_bit, s);
    hipLaunchKernelGGL(k_vcm_merge_starts, dim3((g.G + 2u + 255) / 256), dim3(256), 0, s, mb, g.G);
    hipLaunchKernelGGL(k_vcm_merge_records, dim3(bN), dim3(256), 0, s, S, vb, mb, g.G);
}

void launch_vcm_merge(hipStream_t s, const DevScene& S, const VcmBufs& vb, const VcmMergeBufs& mb,
                      const VcmMergeGrid& g, uint32_t lcount) {
    if (!lcount) return;
    const uint32_t n = vb.cvmax * lcount;
    if (n) hipLaunchKernelGGL(k_vcm_merge, dim3((n + 255) / 256), dim3(256), 0, s, S, vb, mb, g, lcount);
    hipLaunchKernelGGL(k_vcm_merge_sum, dim3((lcount + 255) / 256), dim3(256), 0, s, vb, mb, lcount);
}

}  // namespace orx
