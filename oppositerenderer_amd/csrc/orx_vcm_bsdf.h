/*
 * orx_vcm_bsdf.h — the VCM integrator's BSDF restatement (renderer/BSDF.h VcmBSDF, BxDF.h,
 * reflection.h, math/DifferentialGeometry.h), shared by the walk kernels (orx_vcm.hip) and the
 * vertex-merging pass (orx_vcm_merge.hip).  Device code only; every function is inline.
 */
#pragma once
#include "orx_kernels.h"

namespace orx {

constexpr float VCM_EPS_COSINE = 1e-6f;  /* config.h:42 */
constexpr float VCM_EPS_RAY = 1e-3f;     /* config.h:43 */
constexpr float VCM_RAY_LEN_MIN = 0.0001f;
constexpr float VCM_EPS_PHONG = 1e-3f;   /* BxDF.h:253 */

/* BxDF::Type (BxDF.h:47-67) */
enum : uint32_t {
    BX_REFLECTION = 1, BX_TRANSMISSION = 2, BX_DIFFUSE = 4, BX_GLOSSY = 8, BX_SPECULAR = 16, BX_ALL = 31,
    BX_LAMBERTIAN = 32, BX_SPEC_REFLECTION = 64, BX_SPEC_TRANSMISSION = 128, BX_PHONG = 256
};

__device__ __forceinline__ bool iszero(f3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }
__device__ __forceinline__ float luminance_cie(f3 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }
__device__ __forceinline__ f3 local_reflect(f3 w) { return mk(-w.x, -w.y, w.z); }

/* DifferentialGeometry (math/DifferentialGeometry.h) */
struct Frame {
    f3 b, t, n;
    __device__ __forceinline__ f3 to_world(f3 a) const { return b * a.x + t * a.y + n * a.z; }
    __device__ __forceinline__ f3 to_local(f3 a) const { return mk(dot(b, a), dot(t, a), dot(n, a)); }
};
__device__ __forceinline__ Frame frame_from_normal(f3 nrm) {
    Frame f;
    f.n = normalize(nrm);
    f3 tmp = fabsf(f.n.x) > 0.99f ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
    f.t = normalize(cross(f.n, tmp));
    f.b = cross(f.t, f.n);
    return f;
}

/* FresnelDielectric::evaluate (reflection.h:106-133) */
__device__ inline float fresnel_dielectric(float cosi, float eta_i, float eta_t) {
    cosi = fmaxf(-1.0f, fminf(cosi, 1.0f));
    const bool entering = cosi > 0.0f;
    float ei = entering ? eta_i : eta_t, et = entering ? eta_t : eta_i;
    float sint = ei / et * sqrtf(fmaxf(0.0f, 1.0f - cosi * cosi));
    if (sint >= 1.0f) return 1.0f;
    cosi = fabsf(cosi);
    float cost = sqrtf(fmaxf(0.0f, 1.0f - sint * sint));
    float Rparl = ((et * cosi) - (ei * cost)) / ((et * cosi) + (ei * cost));
    float Rperp = ((ei * cosi) - (et * cost)) / ((ei * cosi) + (et * cost));
    return (Rparl * Rparl + Rperp * Rperp) * 0.5f;
}

struct Bxdf {
    uint32_t type;
    f3 R;
    float exponent;
    float ei, et;
    bool dielectric;
};
__device__ __forceinline__ bool bx_match(uint32_t type, uint32_t mask) {
    return (type & BX_ALL & mask) == (type & BX_ALL);
}
__device__ __forceinline__ float bx_fresnel(const Bxdf& b, float c) {
    return b.dielectric ? fresnel_dielectric(c, b.ei, b.et) : 1.0f;
}
__device__ __forceinline__ float bx_cont(const Bxdf& b, f3 wo) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN || k == BX_PHONG) return fmaxf(b.R.x, maxf(b.R.y, b.R.z));
    if (k == BX_SPEC_REFLECTION) return bx_fresnel(b, wo.z) * fmaxf(b.R.x, maxf(b.R.y, b.R.z));
    return 1.f - bx_fresnel(b, wo.z);
}
__device__ __forceinline__ float bx_albedo(const Bxdf& b, f3 wo) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN || k == BX_PHONG) return luminance_cie(b.R);
    if (k == BX_SPEC_REFLECTION) return bx_fresnel(b, wo.z) * luminance_cie(b.R);
    return (1.f - bx_fresnel(b, wo.z)) * luminance_cie(b.R);
}
__device__ __forceinline__ Bxdf mk_bx(uint32_t type, f3 R, float e = 0.f, float ei = 1.f, float et = 1.f,
                                      bool diel = false) {
    Bxdf b;
    b.type = type; b.R = R; b.exponent = e; b.ei = ei; b.et = et; b.dielectric = diel;
    return b;
}
constexpr uint32_t T_LAMBERT = BX_LAMBERTIAN | BX_REFLECTION | BX_DIFFUSE;
constexpr uint32_t T_PHONG = BX_PHONG | BX_REFLECTION | BX_GLOSSY;
constexpr uint32_t T_SREFL = BX_SPEC_REFLECTION | BX_REFLECTION | BX_SPECULAR;
constexpr uint32_t T_STRANS = BX_SPEC_TRANSMISSION | BX_TRANSMISSION | BX_SPECULAR;

__device__ __forceinline__ float pow_cos_pdf(f3 n, f3 d, float power) {
    const float cosTheta = fmaxf(0.f, dot(n, d));
    return (power + 1.f) * orx_powf(cosTheta, power) * (ORX_1_PI_F * 0.5f);
}
__device__ inline float bx_pdf(const Bxdf& b, f3 wo, f3 wi, bool rev) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN) {
        if (wo.z * wi.z > 0.0f) return rev ? fabsf(wo.z) * ORX_1_PI_F : fabsf(wi.z) * ORX_1_PI_F;
        return 0.f;
    }
    if (k == BX_PHONG) {
        f3 r = local_reflect(wo);
        if (dot(r, wi) <= VCM_EPS_PHONG) return 0.f;
        return pow_cos_pdf(r, wi, b.exponent);
    }
    return 0.f;
}
__device__ inline f3 phong_f(const Bxdf& b, f3 wo, f3 wi, float* pdf) {
    if (wo.z < VCM_EPS_COSINE || wi.z < VCM_EPS_COSINE) {
        if (pdf) *pdf = 0.f;
        return mk1(0.f);
    }
    f3 r = local_reflect(wo);
    float d = dot(r, wi);
    if (d <= VCM_EPS_PHONG) {
        if (pdf) *pdf = 0.f;
        return mk1(0.f);
    }
    if (pdf) *pdf = pow_cos_pdf(r, wi, b.exponent);
    f3 rho = ((b.R * (b.exponent + 2.f)) * 0.5f) * ORX_1_PI_F;
    return rho * orx_powf(d, b.exponent);
}
__device__ inline f3 bx_f(const Bxdf& b, f3 wo, f3 wi) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN) return b.R * ORX_1_PI_F;
    if (k == BX_PHONG) return phong_f(b, wo, wi, nullptr);
    return mk1(0.f);
}
__device__ inline f3 bx_vcm_f(const Bxdf& b, f3 wo, f3 wi, float& dpdf, float& rpdf) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN) {
        if (wo.z < VCM_EPS_COSINE || wi.z < VCM_EPS_COSINE) return mk1(0.f);
        dpdf = fmaxf(0.f, wi.z * ORX_1_PI_F);
        rpdf = fmaxf(0.f, wo.z * ORX_1_PI_F);
        return b.R * ORX_1_PI_F;
    }
    if (k == BX_PHONG) {
        float pdf = 0.f;
        f3 f = phong_f(b, wo, wi, &pdf);
        dpdf = pdf;
        rpdf = pdf;
        return f;
    }
    dpdf = 0.f;
    rpdf = 0.f;
    return mk1(0.f);
}
__device__ inline f3 bx_sample_f(const Bxdf& b, f3 wo, f3& wi, float s0, float s1, float& pdf, bool adjoint) {
    const uint32_t k = b.type & ~BX_ALL;
    if (k == BX_LAMBERTIAN) {
        if (wo.z < VCM_EPS_COSINE) { pdf = 0.f; return mk1(0.f); }
        /* optixu cosine_sample_hemisphere */
        const float r = sqrtf(s0);
        const float phi = 2.0f * ORX_PI_F * s1;
        wi.x = r * orx_cosf(phi);
        wi.y = r * orx_sinf(phi);
        wi.z = sqrtf(fmaxf(0.0f, 1.0f - wi.x * wi.x - wi.y * wi.y));
        pdf = bx_pdf(b, wo, wi, false);
        return b.R * ORX_1_PI_F;
    }
    if (k == BX_PHONG) {
        const float phi = 2.f * ORX_PI_F * s0;
        const float z = orx_powf(s1, 1.f / (b.exponent + 1.f));
        const float r = sqrtf(1.f - z * z);
        wi = mk(orx_cosf(phi) * r, orx_sinf(phi) * r, z);
        if (wo.z < VCM_EPS_COSINE || wi.z < VCM_EPS_COSINE) { pdf = 0.f; return mk1(0.f); }
        const f3 refl = local_reflect(wo);
        const Frame dg = frame_from_normal(refl);
        wi = dg.to_world(wi);
        const float d = dot(refl, wi);
        if (d <= VCM_EPS_PHONG) { pdf = 0.f; return mk1(0.f); }
        pdf = bx_pdf(b, wo, wi, false);
        f3 rho = ((b.R * (b.exponent + 2.f)) * 0.5f) * ORX_1_PI_F;
        return rho * orx_powf(d, b.exponent);
    }
    if (k == BX_SPEC_REFLECTION) {
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1.0f;
        const float R = bx_fresnel(b, wo.z);
        return (b.R * R) / fabsf(wi.z);
    }
    const bool entering = wo.z > 0.0f;
    const float ei = entering ? b.ei : b.et, et = entering ? b.et : b.ei;
    const float sini2 = 1.0f - wo.z * wo.z;
    const float eta = ei / et;
    const float sint2 = eta * eta * sini2;
    if (sint2 >= 1.f) return mk1(0.f); /* pdf left untouched (BxDF.h:496) */
    float cost = sqrtf(fmaxf(0.f, 1.f - sint2));
    if (entering) cost = -cost;
    wi = mk(eta * -wo.x, eta * -wo.y, cost);
    pdf = 1.f;
    const float T = 1.f - bx_fresnel(b, wo.z);
    if (adjoint) return (b.R * T) / fabsf(wi.z);
    return ((b.R * T) * (eta * eta)) / fabsf(wi.z);
}

struct VBsdf {
    Frame dg;
    f3 gn;
    f3 fix;
    Bxdf bx[2];
    float pick[2];
    float cont;
    int n;
    bool fix_is_light;

    __device__ __forceinline__ void init(f3 world_normal, f3 incident, bool is_light) {
        dg = frame_from_normal(world_normal);
        gn = world_normal;
        fix_is_light = is_light;
        fix = dg.to_local(incident);
        n = 0;
        cont = 0.f;
        pick[0] = pick[1] = 0.f;
    }
    /* (all BxDF slots are addressed with compile-time indices so the BSDF
     * stays in registers: no scratch) */
    __device__ __forceinline__ void add(const Bxdf& b) {
        float rr = 0.f;
        rr += bx_cont(b, fix);
        cont = fminf(1.f, cont + rr);
        float albedo = 0.f;
        albedo += bx_albedo(b, fix);
        if (n == 0) {
            bx[0] = b;
            pick[0] = albedo;
        } else {
            bx[1] = b;
            pick[1] = albedo;
        }
        n++;
    }
    __device__ __forceinline__ int count(uint32_t mask) const {
        int c = 0;
#pragma unroll
        for (int i = 0; i < 2; i++) c += (i < n && bx_match(bx[i].type, mask)) ? 1 : 0;
        return c;
    }
    __device__ __forceinline__ bool is_specular() const { return count(BX_ALL & ~BX_SPECULAR) == 0; }
    __device__ __forceinline__ float sum_pick(uint32_t mask) const {
        float c = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++)
            if (i < n && bx_match(bx[i].type, mask)) c += pick[i];
        return c;
    }
    /* VcmBSDF::sampleF via vcmSampleF (BSDF.h:411-485) */
    __device__ f3 sample_f(float sx, float sy, float sz, f3& world_wi, float& pdf, float& cos_out,
                           uint32_t& sampled) const {
        int index = 0;
        float sum = 0.f;
        const int nMatched = count(BX_ALL);
        if (nMatched) {
            sum = sum_pick(BX_ALL);
            float prev = 0.f;
            bool found = false;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                if (!found && i < n && bx_match(bx[i].type, BX_ALL)) {
                    const float cp = pick[i] / sum;
                    if (sx < prev + cp) { index = i; found = true; }
                    else prev += cp;
                }
            }
        }
        if (sum == 0.f) { pdf = 0.0f; return mk1(0.f); }
        const Bxdf b = index ? bx[1] : bx[0];
        const float pick_index = index ? pick[1] : pick[0];
        const f3 world_wo = dg.to_world(fix);
        const f3 wo = dg.to_local(world_wo);
        f3 wi = mk1(0.f);
        f3 f = bx_sample_f(b, wo, wi, sy, sz, pdf, fix_is_light);
        const float q = pick_index / sum;
        pdf *= q;
        if (pdf == 0.0f) { sampled = 0; return mk1(0.f); }
        sampled = b.type;
        world_wi = dg.to_world(wi);
        cos_out = fabsf(wi.z);
        if (!(b.type & BX_SPECULAR)) {
            if (nMatched > 1) {
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    if (i >= n || i == index || !bx_match(bx[i].type, BX_ALL)) continue;
                    float comp = 0.f;
                    comp += bx_pdf(bx[i], wo, wi, false);
                    pdf += comp * q;
                }
            }
            uint32_t m2 = BX_ALL;
            if (dot(gn, world_wi) * dot(gn, world_wo) >= 0.0f) m2 &= ~BX_TRANSMISSION;
            else m2 &= ~BX_REFLECTION;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                if (i >= n || i == index || !bx_match(bx[i].type, m2)) continue;
                f = f + bx_f(bx[i], wo, wi);
            }
        }
        return f;
    }
    /* VcmBSDF::pdf(dir, All & ~Specular, aEvalRevPdf = true) (BSDF.h:391-407) */
    __device__ float pdf_rev(f3 world_gen) const {
        const uint32_t mask = BX_ALL & ~BX_SPECULAR;
        const f3 wi = dg.to_local(world_gen);
        const float sum = sum_pick(mask);
        if (sum == 0.f) return 0.f;
        float pdf = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (i < n && bx_match(bx[i].type, mask)) {
                float comp = 0.f;
                comp += bx_pdf(bx[i], fix, wi, true);
                pdf += comp * pick[i] / sum;
            }
        }
        return pdf;
    }
    /* VcmBSDF::vcmF (BSDF.h:488-541) */
    __device__ f3 vcm_f(f3 world_gen, float& cos_gen, float& dpdf, float& rpdf) const {
        const f3 gen = dg.to_local(world_gen);
        const f3 world_fix = dg.to_world(fix);
        dpdf = 0.f;
        rpdf = 0.f;
        if (fix.z < VCM_EPS_COSINE || gen.z < VCM_EPS_COSINE) return mk1(0.f);
        cos_gen = gen.z;
        uint32_t mask = BX_ALL;
        if (dot(gn, world_gen) * dot(gn, world_fix) >= 0.0f) mask &= ~BX_TRANSMISSION;
        else mask &= ~BX_REFLECTION;
        const float sum = sum_pick(mask);
        if (sum == 0.f) return mk1(0.f);
        f3 f = mk1(0.f);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (i < n && bx_match(bx[i].type, mask)) {
                float dp = 0.f, rp = 0.f;
                f = f + bx_vcm_f(bx[i], fix, gen, dp, rp);
                const float q = pick[i] / sum;
                dp *= q;
                rp *= q;
                dpdf += dp;
                rpdf += rp;
            }
        }
        return f;
    }
};

}  // namespace orx
