/*
 * orx_shade.h — what a hit means: material, normals, textures; the camera, the radiance walk
 * and the light sampling.
 *
 * Replaces helpers/camera.h, helpers/light.h (getLightContribution) and the OptiX closest-hit /
 * any-hit dispatch (flattened into switch-on-material) of the reference.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orx_detmath.h"
#include "orx_isect.h"
#include "orx_rng.h"
#include "orx_scene_types.h"
#include "orx_traverse.h"

namespace orx {

/* ------------------------------------------------------------------ */
/* RadiancePRD flags (renderer/RadiancePRD.h:30-35)                    */
/* ------------------------------------------------------------------ */
constexpr uint32_t PRD_HIT_EMITTER = 1u << 31;
constexpr uint32_t PRD_ERROR = 1u << 30;
constexpr uint32_t PRD_MISS = 1u << 29;
constexpr uint32_t PRD_HIT_SPECULAR = 1u << 28;
constexpr uint32_t PRD_HIT_NON_SPECULAR = 1u << 27;
constexpr uint32_t PRD_PATH_TRACING = 1u << 26;
constexpr float RT_DEFAULT_MAX = 1.e27f;

__device__ __forceinline__ uint32_t prim_material(const DevScene& S, const Hit& h) {
    if ((uint32_t)h.prim < S.nq) return S.qmat[h.prim];
    if ((uint32_t)h.prim < S.nq + S.ns) return S.smat[h.prim - S.nq];
    return S.tmat[h.slot];
}
/* world shading normal as the closest-hit programs see it:
 * normalize(rtTransformNormal(shadingNormal)) with identity transforms. */
__device__ __forceinline__ f3 shading_normal(const DevScene& S, const Hit& h) {
    if ((uint32_t)h.prim < S.nq) {
        const DevQuad& q = S.quads[h.prim];
        return normalize(mk(q.nx, q.ny, q.nz));
    }
    if ((uint32_t)h.prim < S.nq + S.ns) return normalize(h.sn);
    const uint32_t ti = h.slot;
    if (S.tri_n) {
        f3 n0 = ld_f3(S.tri_n[3 * ti]), n1 = ld_f3(S.tri_n[3 * ti + 1]), n2 = ld_f3(S.tri_n[3 * ti + 2]);
        return normalize(normalize(n1 * h.b + n2 * h.g + n0 * (1.0f - h.b - h.g)));
    }
    f3 p0 = ld_f3(S.tri_v[3 * ti]), p1 = ld_f3(S.tri_v[3 * ti + 1]), p2 = ld_f3(S.tri_v[3 * ti + 2]);
    return normalize(normalize(cross(p0 - p2, p1 - p0)));
}
/* geometric normal as the VCM closest-hit programs see it */
__device__ __forceinline__ f3 geometric_normal(const DevScene& S, const Hit& h) {
    if ((uint32_t)h.prim < S.nq) {
        const DevQuad& q = S.quads[h.prim];
        return normalize(mk(q.nx, q.ny, q.nz));
    }
    if ((uint32_t)h.prim < S.nq + S.ns) return normalize(h.sn);
    const uint32_t ti = h.slot;
    f3 p0 = ld_f3(S.tri_v[3 * ti]), p1 = ld_f3(S.tri_v[3 * ti + 1]), p2 = ld_f3(S.tri_v[3 * ti + 2]);
    return normalize(normalize(cross(p0 - p2, p1 - p0)));
}

/* Texture attributes (TriangleMesh.cu:61-84); parallelograms and spheres
 * write no textureCoordinate / tangent attributes: (0,0), no normal map. */
__device__ __forceinline__ void hit_texcoord(const DevScene& S, const Hit& h, float& u, float& v) {
    u = 0.f;
    v = 0.f;
    if ((uint32_t)h.prim < S.nq + S.ns || !S.tri_uv) return;
    const float2 t0 = S.tri_uv[3 * h.slot], t1 = S.tri_uv[3 * h.slot + 1], t2 = S.tri_uv[3 * h.slot + 2];
    const float w0 = 1.0f - h.b - h.g;
    u = (t1.x * h.b + t2.x * h.g) + t0.x * w0;
    v = (t1.y * h.b + t2.y * h.g) + t0.y * w0;
}
/* tex2D(diffuseSampler, textureCoordinate).xyz (Texture.cu:107-109) */
__device__ inline f3 tex_color(const DevScene& S, const DevMaterial& m, const Hit& h) {
    const DevTexture& t = S.tex[m.tex];
    float u, v, c[4];
    hit_texcoord(S, h, u, v);
    orx_tex2d_linear(t.rgba, t.w, t.h, u, v, c);
    return mk(c[0], c[1], c[2]);
}
/* getNormalMappedNormal when hasNormals (Texture.cu:69-77, :88-95) */
__device__ inline f3 tex_normal(const DevScene& S, const DevMaterial& m, const Hit& h, f3 wsn) {
    const DevTexture& t = S.tex[m.tex];
    if (!t.nrgba || !S.tri_n || !S.tri_t || (uint32_t)h.prim < S.nq + S.ns) return wsn;
    const uint32_t k = 3 * h.slot;
    const float w0 = 1.0f - h.b - h.g;
    f3 T = normalize(ld_f3(S.tri_t[k + 1]) * h.b + ld_f3(S.tri_t[k + 2]) * h.g + ld_f3(S.tri_t[k]) * w0);
    f3 B = normalize(ld_f3(S.tri_bt[k + 1]) * h.b + ld_f3(S.tri_bt[k + 2]) * h.g + ld_f3(S.tri_bt[k]) * w0);
    T = normalize(T);
    B = normalize(B);
    float u, v, c[4];
    hit_texcoord(S, h, u, v);
    orx_tex2d_linear(t.nrgba, t.nw, t.nh, u, v, c);
    const float nx = 2.f * c[0] - 1.f, ny = 2.f * c[1] - 1.f, nz = 2.f * c[2] - 1.f;
    return normalize(mk(nx * T.x + ny * B.x + nz * wsn.x, nx * T.y + ny * B.y + nz * wsn.y,
                        nx * T.z + ny * B.z + nz * wsn.z));
}

/* ------------------------------------------------------------------ */
/* camera (Camera.cpp:333-345 derived on the host; helpers/camera.h)   */
/* ------------------------------------------------------------------ */
struct DevCamera {
    f3 eye, lookdir, u, v;
    float aperture;
};
/* RayGeneratorPPM.cu:40-48 / RayGeneratorPT.cu:53-61 + modifyRayForDepthOfField */
__device__ __forceinline__ void primary_ray(const DevCamera& cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H,
                                            Rng& rs, f3& o, f3& d) {
    float sx = rnd(rs);
    float sy = rnd(rs);
    float dx = ((float)x + sx) / (float)W * 2.0f - 1.0f;
    float dy = ((float)y + sy) / (float)H * 2.0f - 1.0f;
    f3 origin = cam.eye;
    f3 dir = normalize(cam.u * dx + cam.v * dy + cam.lookdir);
    if (cam.aperture > 0) {
        f3 focal = cam.eye + cam.lookdir;
        f3 camLookDir = normalize(cam.lookdir);
        float focalPlaneT = (dot(camLookDir, focal) - dot(camLookDir, cam.eye)) / dot(camLookDir, dir);
        f3 lookAt = origin + dir * focalPlaneT;
        float ux = rnd(rs);
        float uy = rnd(rs);
        float rr = sqrtf(ux);
        float th = 2.f * ORX_PI_F * uy;
        float discx = rr * orx_cosf(th);
        float discy = rr * orx_sinf(th);
        origin = origin + ((cam.u * discx) * cam.aperture + (cam.v * discy) * cam.aperture);
        dir = normalize(lookAt - origin);
    }
    o = origin;
    d = dir;
}

/* ------------------------------------------------------------------ */
/* radiance ray: RadiancePRD through the closest-hit programs          */
/* ------------------------------------------------------------------ */
struct RadiancePRD {
    f3 attenuation, radiance;
    uint32_t depth;
    f3 position, normal;
    uint32_t flags;
    f3 newdir;
};

__device__ __forceinline__ float glass_reflect_factor(f3 d, f3 N, float n1, float n2, f3& refr, bool& valid) {
    valid = refract(refr, d, N, n2 / n1);
    float cosI = -dot(d, N);
    float cosT = -dot(refr, N);
    float refl = 1.f;
    if (valid) {
        float rp = (n2 * cosI - n1 * cosT) / (n2 * cosI + n1 * cosT);
        float rs = (n1 * cosI - n2 * cosT) / (n1 * cosI + n2 * cosT);
        refl = (rp * rp + rs * rs) / 2.f;
    }
    return refl;
}

/* Iterative form of the rtTrace(RADIANCE) recursion: Diffuse.cu:71-87,
 * Glossy.cu:74-90, DiffuseEmitter.cu:40-51, Mirror.cu:50-63, Glass.cu:90-143,
 * miss RayGeneratorPPM.cu:72-77. */
__device__ inline void trace_radiance(const DevScene& S, uint32_t maxd, f3 o, f3 d, float tmin, RadiancePRD& prd,
                                      Rng& rs, uint32_t* stk) {
    for (;;) {
        Hit h;
        if (!trace_closest(S, o, d, tmin, RT_DEFAULT_MAX, h, stk)) {
            prd.flags = PRD_MISS;
            prd.attenuation = mk1(0.f);
            prd.radiance = mk1(0.f);
            return;
        }
        const DevMaterial& m = S.mats[prim_material(S, h)];
        f3 hitPoint = o + d * h.t;
        f3 N = shading_normal(S, h);
        if (m.type == MAT_DIFFUSE || m.type == MAT_GLOSSY) {
            prd.flags |= PRD_HIT_NON_SPECULAR;
            prd.attenuation = prd.attenuation * m.Kd;
            prd.normal = N;
            prd.position = hitPoint;
            prd.depth++;
            if (prd.flags & PRD_PATH_TRACING) {
                float s0 = rnd(rs);
                float s1 = rnd(rs);
                prd.newdir = sample_hemisphere_cos(N, s0, s1);
            }
            return;
        } else if (m.type == MAT_TEXTURE) { /* Texture.cu:83-110: mapped normal, no depth++ */
            prd.flags |= PRD_HIT_NON_SPECULAR;
            prd.normal = tex_normal(S, m, h, N);
            prd.position = hitPoint;
            if (prd.flags & PRD_PATH_TRACING) {
                float s0 = rnd(rs);
                float s1 = rnd(rs);
                prd.newdir = sample_hemisphere_cos(N, s0, s1);
            }
            prd.attenuation = prd.attenuation * tex_color(S, m, h);
            return;
        } else if (m.type == MAT_EMITTER) {
            prd.flags |= PRD_HIT_EMITTER;
            if (dot(N, -d) < 0.f) return;
            f3 Le = m.powerPerArea / ORX_PI_F;
            prd.radiance = prd.radiance + prd.attenuation * Le;
            return;
        } else if (m.type == MAT_MIRROR) {
            prd.depth++;
            if (prd.depth <= maxd) {
                prd.attenuation = prd.attenuation * m.Kr;
                d = reflect(d, N);
                o = hitPoint;
                tmin = 0.0001f;
                continue;
            }
            return;
        } else { /* glass */
            bool outside = dot(N, d) < 0;
            f3 Nn = outside ? N : -N;
            float n1 = outside ? 1.0f : m.ior, n2 = outside ? m.ior : 1.0f;
            f3 refr;
            bool valid;
            float refl = glass_reflect_factor(d, Nn, n1, n2, refr, valid);
            float sample = rnd(rs);
            f3 nd;
            if (sample <= refl) {
                nd = reflect(d, Nn);
            } else {
                nd = refr;
                prd.attenuation = prd.attenuation * ((n2 * n2) / (n1 * n1));
            }
            prd.flags |= PRD_HIT_SPECULAR;
            prd.flags &= ~PRD_HIT_NON_SPECULAR;
            prd.depth++;
            if (prd.depth <= maxd) {
                o = hitPoint;
                d = nd;
                tmin = 0.0001f;
                continue;
            }
            prd.attenuation = prd.attenuation * 0.f;
            return;
        }
    }
}

/* getLightContribution (helpers/light.h:29-87) */
/* The sample half of light_contribution: the point on the light, the unshadowed contribution
 * power * lightFactor and the shadow ray; false (contribution 0, no ray) when lightFactor <= 0 */
__device__ inline bool light_sample(const DevLight& light, f3 pos, f3 normal, Rng& rs, f3& lc, f3& dir, float& tmax) {
    float lightFactor = 1;
    f3 pointOnLight;
    if (light.type == LIGHT_AREA) {
        float sx = rnd(rs);
        float sy = rnd(rs);
        pointOnLight = light.position + light.v1 * sx + light.v2 * sy;
    } else if (light.type == LIGHT_POINT) {
        pointOnLight = light.position;
        lightFactor *= 1.f / 4.f;
    } else {
        return false;
    }
    f3 towardsLight = pointOnLight - pos;
    float lightDistance = length(towardsLight);
    towardsLight = towardsLight / lightDistance;
    float n_dot_l = maxf(0, dot(normal, towardsLight));
    lightFactor *= n_dot_l / (ORX_PI_F * lightDistance * lightDistance);
    if (light.type == LIGHT_AREA) lightFactor *= maxf(0, dot(-towardsLight, light.normal));
    if (!(lightFactor > 0.0f)) return false;
    tmax = (float)((double)lightDistance - 0.0001);
    dir = towardsLight;
    lc = light.power * lightFactor; /* = power * (lightFactor * att) for att = 1; occluded: 0 */
    return true;
}
/* helpers/light.h:29-87 (shadow ray from pos + 0.0001 towards the light sample) */
__device__ inline f3 light_contribution(const DevScene& S, const DevLight& light, f3 pos, f3 normal, Rng& rs,
                                        uint32_t* stk) {
    f3 lc, dir;
    float tmax;
    if (!light_sample(light, pos, normal, rs, lc, dir, tmax)) return mk1(0);
    return trace_any(S, pos, dir, 0.0001f, tmax, stk) ? mk1(0.f) : lc;
}

}  // namespace orx
