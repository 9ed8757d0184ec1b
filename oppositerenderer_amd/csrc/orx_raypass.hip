/*
 * orx_raypass.hip — the ray passes of the render core, gfx950: k_rng_init, k_ppm_eye, k_ppm_photon,
 * k_ppm_direct_output, k_pt, and k_grid_setup (the table of kernels and reference entry points is
 * in orx_kernels.hip).
 * k_grid_setup is here, after the photon pass whose AABB replicas it folds and resets: its machine
 * code depends on the unit it is compiled in (orx_detmath.h's helpers are `static inline`, inlined by
 * the compiler's cost model, which counts their other callers in the shading code), and the grid it
 * computes is an input of every later kernel.
 * Wave size is 64 on CDNA4; block reductions are written for it.
 */
#include "orx_kernels_common.h"

namespace orx {

__device__ __forceinline__ void store_hitpoint(const PixelBufs& px, size_t i, const RadiancePRD& prd) {
    /* Union: non-specular hits carry normal, others carry radiance (the
     * unused one is identically zero in RayGeneratorPPM's PRD). */
    bool ns = (prd.flags & PRD_HIT_NON_SPECULAR) != 0;
    f3 nr = ns ? prd.normal : prd.radiance;
    px.hpA[i] = make_float4(prd.position.x, prd.position.y, prd.position.z, __uint_as_float(prd.flags));
    px.hpB[i] = make_float4(nr.x, nr.y, nr.z, prd.attenuation.x);
    px.hpC[i] = make_float2(prd.attenuation.y, prd.attenuation.z);
}

/* ------------------------------------------------------------------ */
/* RNG init: curand_init(seed + slot, 0, 0)                            */
/* ------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void k_rng_init(RngPlanes rng, uint32_t RW, uint32_t rows, uint32_t rank,
                                                  uint32_t world, uint32_t seed) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)rows * RW;
    if (i >= n) return;
    uint32_t j = (uint32_t)(i / RW), x = (uint32_t)(i % RW);
    uint32_t y = rank + world * j;
    uint32_t gslot = y * RW + x;
    rng_store(rng, i, rng_init((uint64_t)(uint32_t)(seed + gslot)));
}
void launch_rng_init(hipStream_t s, RngPlanes rng, uint32_t RW, uint32_t rows, uint32_t rank, uint32_t world,
                     uint32_t seed) {
    size_t n = (size_t)rows * RW;
    hipLaunchKernelGGL(k_rng_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rng, RW, rows, rank, world,
                       seed);
}

/* Pixel tile of a 64-lane wave for the per-pixel passes (eye, direct, PT): 8x8 local pixels
 * on one device; a shard owns image rows rank + world*j, so 8 local rows would span 8*world
 * image rows (incoherent primary and shadow rays): 16x4 local pixels for 2-4 ranks, 32x2 for 8+ */
__host__ __device__ __forceinline__ uint32_t pix_tile_shift(uint32_t world) { return world >= 8 ? 2u : world >= 2 ? 1u : 0u; }
__device__ __forceinline__ void pix_tile(const PixelBufs& px, uint32_t& x, uint32_t& j) {
    const uint32_t sh = pix_tile_shift(px.world), tw = 8u << sh;
    x = blockIdx.x * tw + (threadIdx.x & (tw - 1));
    j = blockIdx.y * (8u >> sh) + (threadIdx.x >> (3 + sh));
}
static dim3 pix_grid(const PixelBufs& px) {
    const uint32_t sh = pix_tile_shift(px.world), tw = 8u << sh, th = 8u >> sh;
    return dim3((px.W + tw - 1) / tw, (px.rows + th - 1) / th);
}

/* ------------------------------------------------------------------ */
/* PPM eye pass                                                        */
/* ------------------------------------------------------------------ */
template <bool MEDIA>
__global__ __launch_bounds__(64) void k_ppm_eye(DevScene S, DevCamera cam, PixelBufs px, Consts c, VolMap vm,
                                                float* volR) {
    ORX_STACK_DECL;
    uint32_t x, j;
    pix_tile(px, x, j);
    if (x >= px.W || j >= px.rows) return;
    uint32_t y = px.rank + px.world * j;
    size_t slot = (size_t)j * px.RW + x;
    Rng rs = rng_load(px.rng, slot);
    RadiancePRD prd;
    prd.attenuation = mk1(1.0f);
    prd.radiance = mk1(0.f);
    prd.depth = 0;
    prd.flags = 0;
    prd.position = mk1(0.f);
    prd.normal = mk1(0.f);
    prd.newdir = mk1(0.f);
    f3 o, d;
    primary_ray(cam, x, y, px.W, px.H, rs, o, d);
    if (MEDIA) {
        f3 vr;
        trace_radiance_vol(S, vm, c.max_radiance_depth, o, d, 0.001f, prd, rs, ORX_STACK_PTR, vr);
        const size_t i = (size_t)j * px.W + x;
        volR[3 * i + 0] = vr.x;
        volR[3 * i + 1] = vr.y;
        volR[3 * i + 2] = vr.z;
    } else {
        trace_radiance(S, c.max_radiance_depth, o, d, 0.001f, prd, rs, ORX_STACK_PTR);
    }
    store_hitpoint(px, (size_t)j * px.W + x, prd);
    rng_store(px.rng, slot, rs);
}
void launch_ppm_eye(hipStream_t s, const DevScene& S, const DevCamera& cam, const PixelBufs& px, const Consts& c,
                    const MediaBufs* mb) {
    const dim3 grid = pix_grid(px);
    if (mb) hipLaunchKernelGGL((k_ppm_eye<true>), grid, dim3(64), ORX_STACK_BYTES(S), s, S, cam, px, c, mb->vm, mb->volR);
    else hipLaunchKernelGGL((k_ppm_eye<false>), grid, dim3(64), ORX_STACK_BYTES(S), s, S, cam, px, c, VolMap{}, nullptr);
}

/* ------------------------------------------------------------------ */
/* PPM photon pass (+ AABB of the valid deposits)                      */
/* ------------------------------------------------------------------ */
/* Photon pass (PhotonGenerator.cu:83-128 + the photon closest-hit programs).  Each lane carries
 * one photon path.  Photon p = j*PW + x always uses RNG slot (j, x) and deposit slots
 * [p*D, p*D + D), so the result does not depend on which lane traced it. */
struct PhotonPath {
    f3 o, d, power;
    float weight, tmin;
    uint32_t p_local, depth, numStored, mask;
    size_t slot;
};
/* the medium's extra photon state (ParticipatingMedium.cu:110-201): ray type and tmax, the open
 * scatter probe (depth at its start, scatter position) and the volumetric events so far */
struct PhotonMedia {
    float tmax;
    bool inmed, probe;
    uint32_t pdepth, nev;
    f3 spos, ev_pos, ev_pow;
};
__device__ __forceinline__ void photon_emit(const DevScene& S, const PixelBufs& px, const PhotonBufs& pb, uint32_t p,
                                            PhotonPath& P, Rng& rs) {
    const uint32_t j = p / pb.PW, x = p - j * pb.PW;
    P.p_local = p;
    P.slot = (size_t)j * px.RW + x;
    rs = rng_load(px.rng, P.slot);
    /* PhotonGenerator.cu:91-107 */
    int lightIndex = 0;
    if (S.nl > 1) {
        float sample = rnd(rs);
        int li = (int)(sample * (float)S.nl);
        lightIndex = li < (int)(S.nl - 1) ? li : (int)(S.nl - 1);
    }
    const DevLight& L = S.lights[lightIndex];
    float powerScale = (float)S.nl;
    f3 power = L.power * powerScale;
    f3 origin = L.position, dir = mk1(0.f);
    float photonPowerFactor = 1.f;
    float s1x = rnd(rs), s1y = rnd(rs);
    /* generatePhotonOriginAndDirection (PhotonGenerator.cu:40-79) */
    if (L.type == LIGHT_AREA) {
        float s2x = rnd(rs), s2y = rnd(rs);
        origin = origin + (L.v1 * s1x + L.v2 * s1y);
        dir = sample_hemisphere(L.normal, s2x, s2y);
    } else if (L.type == LIGHT_POINT) {
        f3 bc = mk(S.bs_cx, S.bs_cy, S.bs_cz);
        f3 sceneCenterToLight = L.position - bc;
        float lightDistance = length(sceneCenterToLight);
        sceneCenterToLight = sceneCenterToLight / lightDistance;
        bool wellOutside = (double)lightDistance > 1.5 * (double)S.bs_r;
        if (wellOutside) {
            f3 pointOnDisc = sample_disc(s1x, s1y, bc, S.bs_r, sceneCenterToLight);
            dir = normalize(pointOnDisc - origin);
            float rr = S.bs_r * S.bs_r + lightDistance * lightDistance;
            photonPowerFactor = (1 - lightDistance * (1.0f / sqrtf(rr))) / 2.f;
        } else {
            dir = sample_unit_sphere(s1x, s1y);
        }
    } else {
        f3 pointOnDisc = sample_disc(s1x, s1y, origin + L.direction, orx_sinf(L.angle / 2), L.direction);
        dir = normalize(pointOnDisc - origin);
    }
    P.power = power * photonPowerFactor;
    P.o = origin;
    P.d = dir;
    P.weight = 1.0f;
    P.tmin = 0.0001f;
    P.depth = 0;
    P.numStored = 0;
    P.mask = 0;
}

/* What a photon does at the end of its ray (Diffuse.cu:92-135, Glossy.cu:94-137, Mirror.cu:65-77,
 * Glass.cu:164-205, DiffuseEmitter.cu:56-59, ParticipatingMedium.cu:110-201): deposit,
 * Russian roulette and the next ray in P; false once the path has ended (its deposit mask and
 * RNG state are then stored). */
template <bool MEDIA>
__device__ __forceinline__ bool photon_after_hit(const DevScene& S, const PixelBufs& px, const PhotonBufs& pb,
                                                 const Consts& c, PhotonPath& P, Rng& rs, bool hit, const Hit& h,
                                                 bool had_probe, float& lo_x, float& lo_y, float& lo_z, float& hi_x,
                                                 float& hi_y, float& hi_z, const VolMap& vm, PhotonMedia& M,
                                                 const MediaBufs& mb) {
    bool done = false;
    if (!hit) {
        done = true;
    } else if (MEDIA && h.prim == MED_PRIM) {
        P.depth++;
        const f3 N = normalize(h.sn);
        const f3 hitPoint = P.o + P.d * h.t;
        if (dot(N, P.d) > 0 && M.inmed) { /* leaving the box */
            P.o = hitPoint + P.d * 0.0001f;
            P.tmin = 0.001f;
            M.tmax = RT_DEFAULT_MAX;
            M.inmed = false;
        } else { /* sample the scatter distance, probe [0.001, scatterT] */
            const float sig_t = vm.sig_a + vm.sig_s;
            const float sample = rnd(rs);
            const float st = -orx_logf(1 - sample) / sig_t;
            M.spos = hitPoint + P.d * st;
            M.probe = true;
            M.pdepth = P.depth;
            P.o = hitPoint;
            P.tmin = 0.001f;
            M.tmax = st;
            M.inmed = true;
        }
    } else {
        if (MEDIA) M.tmax = RT_DEFAULT_MAX;
        const DevMaterial& m = S.mats[prim_material(S, h)];
        const f3 hitPoint = P.o + P.d * h.t;
        if (m.type == MAT_DIFFUSE || m.type == MAT_GLOSSY || m.type == MAT_TEXTURE) {
            /* Texture.cu:116-175 differs only in Kd = texel colour,
             * the weight cutoff (0.01) and the new ray's tmin (0.01) */
            const bool tex = m.type == MAT_TEXTURE;
            const f3 N = shading_normal(S, h);
            if (P.depth >= 1 && P.numStored < pb.D) {
                const uint32_t si = P.p_local * pb.D + P.numStored;
                float4* rec = pb.slots + 4 * (size_t)si;
                rec[0] = make_float4(hitPoint.x, hitPoint.y, hitPoint.z, P.power.x);
                pb.pos4[si] = make_float4(hitPoint.x, hitPoint.y, hitPoint.z, 0.f);
                rec[1] = make_float4(P.d.x, P.d.y, P.d.z, P.power.y);
                rec[2].x = P.power.z;
                /* the hash's STORE_PHOTON (store_photon.h:19-25) counts every deposit */
                if (fmax3(P.power) > 0 || pb.hash) {
                    P.mask |= 1u << P.numStored;
                    lo_x = fminf(lo_x, hitPoint.x); lo_y = fminf(lo_y, hitPoint.y); lo_z = fminf(lo_z, hitPoint.z);
                    hi_x = fmaxf(hi_x, hitPoint.x); hi_y = fmaxf(hi_y, hitPoint.y); hi_z = fmaxf(hi_z, hitPoint.z);
                }
                P.numStored++;
            }
            const f3 Kd = tex ? tex_color(S, m, h) : m.Kd;
            P.power = P.power * Kd;
            P.weight *= fmax3(Kd);
            if (P.depth >= 3) {
                float probContinue = favgf(Kd);
                float probSample = rnd(rs);
                if (probSample >= probContinue) done = true;
                else P.power = P.power / probContinue;
            }
            if (!done) {
                P.depth++;
                if (P.depth >= c.max_photon_depth || (double)P.weight < (tex ? 0.01 : 0.001) ||
                    P.numStored >= pb.Dlim) {
                    done = true;
                } else {
                    float s0 = rnd(rs);
                    float s1 = rnd(rs);
                    P.d = sample_hemisphere_cos(N, s0, s1);
                    P.o = hitPoint;
                    P.tmin = tex ? 0.01f : 0.0001f;
                    if (MEDIA) M.inmed = false;
                }
            }
        } else if (m.type == MAT_EMITTER) {
            if (MEDIA && !M.inmed) P.depth++; /* closestHitPhoton is the PHOTON program only */
            done = true;
        } else if (m.type == MAT_MIRROR) {
            const f3 N = shading_normal(S, h);
            P.depth++;
            if (P.depth <= c.max_photon_depth) {
                P.power = P.power * m.Kr;
                P.d = reflect(P.d, N);
                P.o = hitPoint;
                P.tmin = 0.0001f;
                if (MEDIA) M.inmed = false;
            } else {
                done = true;
            }
        } else {
            const f3 wsn = shading_normal(S, h);
            const bool outside = dot(wsn, P.d) < 0;
            const f3 N = outside ? wsn : -wsn;
            const float n1 = outside ? 1.0f : m.ior, n2 = outside ? m.ior : 1.0f;
            f3 refr;
            bool valid;
            const float refl = glass_reflect_factor(P.d, N, n1, n2, refr, valid);
            const float sample = rnd(rs);
            const bool reflected = sample <= refl;
            const f3 nd = reflected ? reflect(P.d, N) : refr;
            P.depth++;
            if (P.depth <= c.max_photon_depth) {
                P.o = hitPoint;
                P.d = nd;
                P.tmin = 0.0001f;
                if (MEDIA) M.inmed = (outside && !reflected) || (!outside && reflected);
            } else {
                done = true;
            }
        }
    }
    if (MEDIA && had_probe && P.depth == M.pdepth) { /* the probe met nothing that took the path over */
        done = true;
        if (rnd(rs) < vm.sig_s / (vm.sig_a + vm.sig_s)) {
            M.nev++;
            M.ev_pos = M.spos;
            M.ev_pow = P.power;
            if (P.depth < c.max_photon_depth) {
                const float s0 = rnd(rs), s1 = rnd(rs);
                P.d = sample_unit_sphere(s0, s1);
                P.o = M.spos;
                P.tmin = 0.001f;
                M.tmax = RT_DEFAULT_MAX;
                M.inmed = false;
                done = false;
            }
        }
    }
    if (done) {
        pb.vmask[P.p_local] = (uint8_t)P.mask;
        rng_store(px.rng, P.slot, rs);
        if (MEDIA) {
            mb.ev_a[P.p_local] = make_float4(M.ev_pos.x, M.ev_pos.y, M.ev_pos.z, __uint_as_float(M.nev));
            mb.ev_b[P.p_local] = make_float4(M.ev_pow.x, M.ev_pow.y, M.ev_pow.z, 0.f);
        }
        return false;
    }
    return true;
}

/* One bounce of a photon path: its ray, then photon_after_hit. */
template <bool MEDIA, class STK, class NODES>
__device__ __forceinline__ bool photon_bounce(const DevScene& S, const PixelBufs& px, const PhotonBufs& pb,
                                              const Consts& c, PhotonPath& P, Rng& rs, const STK& stk,
                                              const NODES& nodes, float& lo_x, float& lo_y, float& lo_z,
                                              float& hi_x, float& hi_y, float& hi_z, const VolMap& vm,
                                              PhotonMedia& M, const MediaBufs& mb) {
    Hit h;
    bool had_probe = false;
    bool hit;
    if (MEDIA) {
        had_probe = M.probe;
        M.probe = false;
        hit = trace_closest_m(S, vm, P.o, P.d, P.tmin, M.tmax, M.inmed, h, stk, nodes);
    } else {
        hit = trace_closest_t(S, P.o, P.d, P.tmin, RT_DEFAULT_MAX, h, stk, nodes);
    }
    return photon_after_hit<MEDIA>(S, px, pb, c, P, rs, hit, h, had_probe, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, vm, M, mb);
}


/* One photon per lane: block b traces photons [64b, 64b + 64).  The kernel is register-capped at
 * ORX_PHOTON_WAVES waves per SIMD (6: 80 VGPRs and 13 spilled; uncapped it took 121 and ran at 4;
 * hall frame 6.43 ms at 4 waves, 6.33 at 5, 6.19 at 6, 7 no better) and its traversal stack is PHOTON_LDS_STACK entries per lane in LDS continued in global memory
 * (StackH, one column per photon): the whole stack in LDS (35 entries on the hall, 9.5 KB per wave)
 * would hold a CU to 16 waves.  (Persistent waves on a work counter spilled at 5 waves and ran
 * slower; per-lane refill from a device counter, a wavefront pass with
 * per-bounce queues and a direction-binned photon order were measured slower on the hall: DESIGN.md
 * section 4.) */
#ifndef ORX_PHOTON_WAVES
#define ORX_PHOTON_WAVES 6
#endif
constexpr int PHOTON_LDS_STACK = 16;
template <bool MEDIA>
__global__ __launch_bounds__(64, ORX_PHOTON_WAVES) void k_ppm_photon(DevScene S, PixelBufs px, PhotonBufs pb, Consts c,
                                                                     MediaBufs mb) {
    ORX_STACK_DECL;
    const uint32_t lane = threadIdx.x;
    const uint32_t total = pb.prows * pb.PW;
    const uint32_t p = blockIdx.x * 64u + lane;
    const StackH<PHOTON_LDS_STACK> stk{ORX_STACK_PTR, pb.tstk, blockIdx.x, pb.tdeep, lane};
    float lo_x = INFINITY, lo_y = INFINITY, lo_z = INFINITY;
    float hi_x = -INFINITY, hi_y = -INFINITY, hi_z = -INFINITY;
    PhotonPath P;
    PhotonMedia M;
    M.tmax = RT_DEFAULT_MAX;
    M.inmed = M.probe = false;
    M.pdepth = M.nev = 0;
    M.spos = M.ev_pos = M.ev_pow = mk1(0.f);
    Rng rs;
    bool alive = p < total;
    if (alive) photon_emit(S, px, pb, p, P, rs);
    while (__ballot(alive)) {
        if (alive)
            alive = photon_bounce<MEDIA>(S, px, pb, c, P, rs, stk, NodesG{}, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, mb.vm,
                                         M, mb);
    }
    photon_bbox_flush(pb, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, blockIdx.x & (BBOX_REPLICAS - 1), lane);
}

uint32_t photon_stack_deep(uint32_t entries) { return StackH<PHOTON_LDS_STACK>::deep(entries); }
/* false (nothing launched): the deep-stack buffer does not cover the launch (the caller reports
 * ORX_ERR_STATE; photon_stack_ensure sizes it at every scene and resize) */
bool launch_ppm_photon(hipStream_t s, const DevScene& S, const PixelBufs& px, const PhotonBufs& pb, const Consts& c,
                       const MediaBufs* mb) {
    const uint32_t total = pb.prows * pb.PW;
    if (total == 0) return true;
    const uint32_t blocks = (total + 63) / 64;
    if ((size_t)blocks * 64 > pb.tlanes || pb.tdeep < StackH<PHOTON_LDS_STACK>::deep(S.stack_entries)) return false;
    const size_t lds = StackH<PHOTON_LDS_STACK>::lds_bytes();
    if (mb)
        hipLaunchKernelGGL((k_ppm_photon<true>), dim3(blocks), dim3(64), lds, s, S, px, pb, c, *mb);
    else
        hipLaunchKernelGGL((k_ppm_photon<false>), dim3(blocks), dim3(64), lds, s, S, px, pb, c, MediaBufs{});
    return true;
}

/* ------------------------------------------------------------------ */
/* grid setup: createUniformGridPhotonMap host math, on one thread     */
/* ------------------------------------------------------------------ */
__global__ void k_grid_setup(PhotonBufs pb, GridBox gb) {
    /* lanes k*64..: fold the replicas, then reset them for the next photon pass */
    __shared__ uint32_t red[6];
    const uint32_t lane = threadIdx.x;
    for (int k = 0; k < 6; k++) {
        uint32_t v = pb.bbox[k * BBOX_REPLICAS + lane];
        for (int o = 32; o > 0; o >>= 1) {
            uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
            v = k < 3 ? min(v, w) : max(v, w);
        }
        if (lane == 0) red[k] = v;
        pb.bbox[k * BBOX_REPLICAS + lane] = k < 3 ? 0xffffffffu : 0u;
    }
    __syncthreads();
    if (lane != 0) return;
    uint32_t b[6];
    GridParams* g = pb.grid;
    /* the photons' own AABB: the slab gather's cull box */
    const bool own = red[0] != 0xffffffffu;
    for (int k = 0; k < 3; k++) {
        g->clo[k] = own ? ord2f(red[k]) : INFINITY;
        g->chi[k] = own ? ord2f(red[k + 3]) : -INFINITY;
    }
    for (int k = 0; k < 6; k++) b[k] = gb.on ? gb.b[k] : red[k];
    bool any = b[0] != 0xffffffffu; /* min initialised to ord(+max) */
    f3 lo, hi;
    if (any) {
        lo = mk(ord2f(b[0]), ord2f(b[1]), ord2f(b[2]));
        hi = mk(ord2f(b[3]), ord2f(b[4]), ord2f(b[5]));
    } else {
        lo = mk1(0.f);
        hi = mk1(0.f);
    }
    /* padAABB (SpatialHash.cu:135-141) */
    lo = mk(lo.x - 0.0000001f, lo.y - 0.0000001f, lo.z - 0.0000001f);
    hi = mk(hi.x + 0.0000001f, hi.y + 0.0000001f, hi.z + 0.0000001f);
    f3 ext = hi - lo;
    /* getSmallestPossibleCellSize (SpatialHash.cu:62-71) */
    float sceneVolume = ext.x * ext.y * ext.z;
    float minVolumePerCell = sceneVolume / (float)pb.gcells;
    float radiusC = orx_powf(minVolumePerCell, 1.0f / 3.0f);
    f3 ncf = ext / radiusC;
    uint32_t nx = orx_f2u_sat(orx_floorf(ncf.x)), ny = orx_f2u_sat(orx_floorf(ncf.y)),
             nz = orx_f2u_sat(orx_floorf(ncf.z));
    f3 each = mk(ext.x / (float)nx, ext.y / (float)ny, ext.z / (float)nz);
    float smallest = fmax3(each);
    float cellSize = (float)((double)smallest + 0.001);
    /* calculateGridSize (SpatialHash.cu:42-50) */
    f3 f = ext / cellSize;
    uint32_t gx = orx_f2u_sat(orx_ceilf(f.x)), gy = orx_f2u_sat(orx_ceilf(f.y)), gz = orx_f2u_sat(orx_ceilf(f.z));
    gx = gx < 1 ? 1 : gx;
    gy = gy < 1 ? 1 : gy;
    gz = gz < 1 ? 1 : gz;
    uint64_t G = (uint64_t)gx * gy * gz;
    g->ox = lo.x; g->oy = lo.y; g->oz = lo.z;
    g->cell = cellSize;
    g->gx = gx; g->gy = gy; g->gz = gz;
    g->any_valid = any;
    g->photons_visited = 0;
    g->cells_visited = 0;
    if (G > pb.gmax) {
        g->error = 1;
        g->G = 0;
    } else {
        g->error = 0;
        g->G = (uint32_t)G;
    }
}
void launch_grid_setup(hipStream_t s, const PhotonBufs& pb, const GridBox& gb) {
    hipLaunchKernelGGL(k_grid_setup, dim3(1), dim3(64), 0, s, pb, gb);
}

/* ------------------------------------------------------------------ */
/* direct radiance (4 shadow samples) + output accumulation            */
/* ------------------------------------------------------------------ */
/* MODE 0: direct + output fused; 1: direct only (overlapping the grid build
 * and gather on a second stream); 2: output only (out = [out +] direct + indirect) */
template <int MODE>
__global__ __launch_bounds__(64) void k_ppm_direct_output(DevScene S, PixelBufs px, Consts c) {
    ORX_STACK_DECL;
    uint32_t x, j;
    pix_tile(px, x, j);
    if (x >= px.W || j >= px.rows) return;
    const size_t i = (size_t)j * px.W + x;
    if (MODE == 2) {
        const f3 d = mk(px.direct[3 * i], px.direct[3 * i + 1], px.direct[3 * i + 2]);
        const f3 ind = mk(px.indirect[3 * i], px.indirect[3 * i + 1], px.indirect[3 * i + 2]);
        const f3 fin = d + ind;
        f3 out = fin;
        if (c.local_iteration != 0) out = mk(px.output[3 * i], px.output[3 * i + 1], px.output[3 * i + 2]) + fin;
        px.output[3 * i + 0] = out.x;
        px.output[3 * i + 1] = out.y;
        px.output[3 * i + 2] = out.z;
        return;
    }
    const float4 A = px.hpA[i];
    const float4 B = px.hpB[i];
    const float2 Cc = px.hpC[i];
    const uint32_t flags = __float_as_uint(A.w);
    f3 direct;
    if (!(flags & PRD_HIT_NON_SPECULAR)) {
        f3 rad = mk(B.x, B.y, B.z);
        if ((flags & PRD_HIT_EMITTER) && !(flags & PRD_HIT_SPECULAR))
            direct = mk(fminf(rad.x, 1.f), fminf(rad.y, 1.f), fminf(rad.z, 1.f));
        else
            direct = rad;
    } else if (c.media) { /* numShadowSamples = ENABLE_PARTICIPATING_MEDIA ? 0 : 4 (DirectRadianceEstimation.cu:54) */
        direct = mk1(0.f);
    } else {
        const size_t slot = (size_t)j * px.RW + x;
        Rng rs = rng_load(px.rng, slot);
        const int numLights = (int)S.nl;
        const f3 pos = mk(A.x, A.y, A.z), nrm = mk(B.x, B.y, B.z);
        f3 avg = mk1(0.f);
        for (int s = 0; s < 4; s++) {
            float sample = rnd(rs);
            int li = (int)(sample * (float)numLights);
            int randomLightIndex = li < numLights - 1 ? li : numLights - 1;
            float scale = (float)numLights;
            f3 lc = light_contribution(S, S.lights[randomLightIndex], pos, nrm, rs, ORX_STACK_PTR);
            avg = avg + lc * scale;
        }
        direct = (mk(B.w, Cc.x, Cc.y) * avg) / (float)4;
        rng_store(px.rng, slot, rs);
    }
    px.direct[3 * i + 0] = direct.x;
    px.direct[3 * i + 1] = direct.y;
    px.direct[3 * i + 2] = direct.z;
    if (MODE == 1) return;
    f3 ind = mk(px.indirect[3 * i], px.indirect[3 * i + 1], px.indirect[3 * i + 2]);
    f3 fin = direct + ind;
    f3 out = fin;
    if (c.local_iteration != 0) out = mk(px.output[3 * i], px.output[3 * i + 1], px.output[3 * i + 2]) + fin;
    px.output[3 * i + 0] = out.x;
    px.output[3 * i + 1] = out.y;
    px.output[3 * i + 2] = out.z;
}
void launch_ppm_direct_output(hipStream_t s, const DevScene& S, const PixelBufs& px, const Consts& c, int mode) {
    const dim3 grid = pix_grid(px);
    if (mode == 1) hipLaunchKernelGGL(k_ppm_direct_output<1>, grid, dim3(64), ORX_STACK_BYTES(S), s, S, px, c);
    else if (mode == 2) hipLaunchKernelGGL(k_ppm_direct_output<2>, grid, dim3(64), 0, s, S, px, c);
    else hipLaunchKernelGGL(k_ppm_direct_output<0>, grid, dim3(64), ORX_STACK_BYTES(S), s, S, px, c);
}

/* ------------------------------------------------------------------ */
/* path tracing                                                        */
/* ------------------------------------------------------------------ */
__global__ __launch_bounds__(64) void k_pt(DevScene S, DevCamera cam, PixelBufs px, Consts c) {
    ORX_STACK_DECL;
    uint32_t x, j;
    pix_tile(px, x, j);
    if (x >= px.W || j >= px.rows) return;
    const uint32_t y = px.rank + px.world * j;
    const size_t i = (size_t)j * px.W + x;
    const size_t slot = (size_t)j * px.RW + x;
    /* the PRD copy and the global slot start from the same state and are
     * advanced independently (RayGeneratorPT.cu:52, :89, :111, :130) */
    Rng G = rng_load(px.rng, slot);
    Rng rs = G;
    const int numLights = (int)S.nl;
    RadiancePRD prd;
    prd.attenuation = mk1(1.0f);
    prd.radiance = mk1(0.f);
    prd.depth = 0;
    prd.flags = 0;
    prd.position = mk1(0.f);
    prd.normal = mk1(0.f);
    prd.newdir = mk1(0.f);
    f3 o, d;
    primary_ray(cam, x, y, px.W, px.H, rs, o, d);
    f3 fin = mk1(0);
    for (int it = 0; it < 5; it++) {
        prd.flags = PRD_PATH_TRACING;
        trace_radiance(S, c.max_radiance_depth, o, d, 0.001f, prd, rs, ORX_STACK_PTR);
        if (prd.flags & PRD_HIT_EMITTER) {
            if ((prd.flags & PRD_HIT_SPECULAR) || it == 0) fin = prd.radiance;
            break;
        } else if (prd.flags & PRD_HIT_NON_SPECULAR) {
            f3 accum = mk1(0);
            int li = (int)(rnd(G) * (float)numLights);
            float scale = (float)numLights;
            f3 lc = light_contribution(S, S.lights[li], prd.position, prd.normal, rs, ORX_STACK_PTR) * scale;
            accum = accum + lc;
            f3 direct = (prd.attenuation * accum) / (float)1;
            fin = fin + direct;
            o = prd.position;
            d = prd.newdir;
        } else {
            break;
        }
        if (it >= 3) {
            float sample = rnd(G);
            float p = fmax3(prd.attenuation);
            if (sample > p) break;
            prd.attenuation = prd.attenuation / p;
        }
    }
    if (!isnan3(fin)) {
        f3 out = fin;
        if (c.local_iteration != 0) out = mk(px.output[3 * i], px.output[3 * i + 1], px.output[3 * i + 2]) + fin;
        px.output[3 * i + 0] = out.x;
        px.output[3 * i + 1] = out.y;
        px.output[3 * i + 2] = out.z;
    }
    rng_store(px.rng, slot, rs);
}
void launch_pt(hipStream_t s, const DevScene& S, const DevCamera& cam, const PixelBufs& px, const Consts& c) {
    const dim3 grid = pix_grid(px);
    hipLaunchKernelGGL(k_pt, grid, dim3(64), ORX_STACK_BYTES(S), s, S, cam, px, c);
}

}  // namespace orx
