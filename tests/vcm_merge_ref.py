"""Brute-force vertex merging in NumPy: the checker of orx_config.vcm_merging.

The reference renderer has no merging code (m_vcmUseVM = false), so this restates the published
algorithm (Georgiev et al., VCM tech. rep. eqs. 37-41; SmallVCM RangeQuery::Process) in the
renderer's own quantities, from the device's own vertex buffers:

    light vertices   ORX_BUF_VCM_VERTICES       [9][npx][16]  pos3 mat thr3 dVCM normal3 dVC dirFix3 dVM
    camera vertices  ORX_BUF_VCM_CAMERA_VERTICES [K][npx][16]  pos3 mat thr3 dVCM normal3 dVM dir3 0

Every (camera vertex, light vertex) pair of the image is tested: the accept test in float32 exactly as
the device states it (d = lightPos - camPos, d2 = x*x + y*y + z*z, d2 <= r*r), everything after it in
float64.  VcmBSDF::vcmF is restated for the two non-specular BSDFs a merging vertex can have: Lambert
(Diffuse) and Lambert + Phong (Glossy).  Texture materials are not covered: their texel colours are
not part of the vertex buffers.
"""
import numpy as np

from oppositerenderer_amd import _abi

EPS_COSINE = 1e-6   # config.h:42
EPS_PHONG = 1e-3    # BxDF.h:253
PI_F = np.float32(3.14159265358979323846)
LUM = np.array([0.2126, 0.7152, 0.0722])


def mis_factors(width, height, radius, merging=True):
    """orx_vcm_mis_factors in float32, in its operation order: (misVc, misVm, vmNormalization)."""
    count = np.float32(np.uint32(width) * np.uint32(height))
    r2 = np.float32(radius) * np.float32(radius)
    eta = np.float32(np.float32(np.float32(count / np.float32(1)) * PI_F) * r2)
    mis_vc = np.float32(1) / eta
    mis_vm = eta if merging else np.float32(0)
    vm_norm = np.float32(1) / np.float32(np.float32(r2 * PI_F) * count)
    return np.float32(mis_vc), np.float32(mis_vm), np.float32(vm_norm)


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _frames(normals):
    """frame_from_normal (DifferentialGeometry): rows b, t, n for every normal."""
    n = _normalize(normals)
    tmp = np.where((np.abs(n[:, 0]) > 0.99)[:, None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    t = _normalize(np.cross(n, tmp))
    b = np.cross(t, n)
    return b, t, n


def _material_table(materials):
    """Per material id: Kd, Ks, exponent, glossy flag, merging-capable flag."""
    kd = np.array([m.Kd for m in materials], np.float64).reshape(-1, 3)
    ks = np.array([m.Ks for m in materials], np.float64).reshape(-1, 3)
    ex = np.array([m.exponent for m in materials], np.float64)
    ty = np.array([m.type for m in materials], np.int64)
    return kd, ks, ex, ty


def _flatten(verts, counts):
    """[K][npx][16] with per-pixel counts -> the valid records [n][16] and their pixel index [n]."""
    K, npx, _ = verts.shape
    k = np.arange(K)[:, None]
    valid = k < np.minimum(counts.astype(np.int64), K)[None, :]
    pix = np.broadcast_to(np.arange(npx)[None, :], (K, npx))[valid]
    return verts[valid], pix


def accepted_pairs(light_verts, light_counts, cam_verts, cam_counts, radius, chunk=256):
    """The accepted-pair count [npx] alone (any material: the accept test reads positions only)."""
    L, _ = _flatten(np.asarray(light_verts, np.float32), np.asarray(light_counts))
    Cv, cpix = _flatten(np.asarray(cam_verts, np.float32), np.asarray(cam_counts))
    count = np.zeros(np.asarray(cam_verts).shape[1], np.int64)
    r2 = np.float32(radius) * np.float32(radius)
    for s in range(0, len(Cv), chunk):
        d = L[None, :, 0:3] - Cv[s:s + chunk, None, 0:3]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        np.add.at(count, cpix[s:s + chunk], (d2 <= r2).sum(1))
    return count


def merge_reference(light_verts, light_counts, cam_verts, cam_counts, materials, width, height, radius, chunk=256):
    """The merging colour [npx][3] (float64) and the accepted-pair count [npx] of one iteration."""
    light_verts = np.asarray(light_verts, np.float32)
    cam_verts = np.asarray(cam_verts, np.float32)
    npx = cam_verts.shape[1]
    L, _ = _flatten(light_verts, np.asarray(light_counts))
    Cv, cpix = _flatten(cam_verts, np.asarray(cam_counts))
    color = np.zeros((npx, 3), np.float64)
    count = np.zeros(npx, np.int64)
    if len(L) == 0 or len(Cv) == 0:
        return color, count
    kd_t, ks_t, ex_t, ty_t = _material_table(materials)
    for mats in (L[:, 3].copy().view(np.uint32), Cv[:, 3].copy().view(np.uint32)):
        assert (mats < len(materials)).all()
        ty = ty_t[mats]
        assert np.isin(ty, (_abi.MAT_DIFFUSE, _abi.MAT_GLOSSY)).all(), "merge_reference: Diffuse and Glossy vertices only"
    mis_vc, _, vm_norm = (float(v) for v in mis_factors(width, height, radius))
    r2 = np.float32(radius) * np.float32(radius)

    # light side: position (float32 for the test), throughput, dVCM, dVM, world dirFix, continuation probability
    lpos32 = L[:, 0:3]
    lmat = L[:, 3].copy().view(np.uint32)
    lthr = L[:, 4:7].astype(np.float64)
    ldvcm = L[:, 7].astype(np.float64)
    ldvm = L[:, 15].astype(np.float64)
    lb, lt, ln = _frames(L[:, 8:11].astype(np.float64))
    lfix = L[:, 12:15].astype(np.float64)
    ldir = lb * lfix[:, 0:1] + lt * lfix[:, 1:2] + ln * lfix[:, 2:3]
    lcont = np.minimum(1.0, kd_t[lmat].max(1))
    lgl = ty_t[lmat] == _abi.MAT_GLOSSY
    lcont = np.where(lgl, np.minimum(1.0, lcont + ks_t[lmat].max(1)), lcont)

    for s in range(0, len(Cv), chunk):
        C = Cv[s:s + chunk]
        pix = cpix[s:s + chunk]
        # accept test, float32, association (x*x + y*y) + z*z
        d = lpos32[None, :, :] - C[:, None, 0:3]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        acc = d2 <= r2
        np.add.at(count, pix, acc.sum(1))
        ci, li = np.nonzero(acc)
        if len(ci) == 0:
            continue
        cmat = C[:, 3].copy().view(np.uint32)
        kd = kd_t[cmat]
        ks = ks_t[cmat]
        ex = ex_t[cmat]
        gl = ty_t[cmat] == _abi.MAT_GLOSSY
        gn = C[:, 8:11].astype(np.float64)
        b, t, n = _frames(gn)
        inc = -C[:, 12:15].astype(np.float64)
        fix = np.stack([(b * inc).sum(1), (t * inc).sum(1), (n * inc).sum(1)], 1)
        wfix = b * fix[:, 0:1] + t * fix[:, 1:2] + n * fix[:, 2:3]
        ccont = np.minimum(1.0, kd.max(1))
        ccont = np.where(gl, np.minimum(1.0, ccont + ks.max(1)), ccont)
        pick_l = kd @ LUM
        pick_p = np.where(gl, ks @ LUM, 0.0)

        # per accepted pair: VcmBSDF::vcmF of the camera BSDF towards the light vertex's dirFix
        wgen = ldir[li]
        gen = np.stack([(b[ci] * wgen).sum(1), (t[ci] * wgen).sum(1), (n[ci] * wgen).sum(1)], 1)
        fx = fix[ci]
        ok = ~((fx[:, 2] < EPS_COSINE) | (gen[:, 2] < EPS_COSINE))
        ok &= (gn[ci] * wgen).sum(1) * (gn[ci] * wfix[ci]).sum(1) >= 0.0   # reflection lobes only
        psum = pick_l[ci] + pick_p[ci]
        ok &= psum != 0.0
        psafe = np.where(psum != 0.0, psum, 1.0)
        f = kd[ci] / np.pi
        dp = np.maximum(0.0, gen[:, 2] / np.pi) * pick_l[ci] / psafe
        rp = np.maximum(0.0, fx[:, 2] / np.pi) * pick_l[ci] / psafe
        g = gl[ci]
        if g.any():
            refl = fx * np.array([-1.0, -1.0, 1.0])
            dd = (refl * gen).sum(1)
            lobe = g & (dd > EPS_PHONG)
            dsafe = np.where(lobe, dd, 1.0)
            e = ex[ci]
            pdf = np.where(lobe, (e + 1.0) * dsafe ** e * (0.5 / np.pi), 0.0)
            f = f + np.where(lobe[:, None], ks[ci] * ((e + 2.0) * 0.5 / np.pi * dsafe ** e)[:, None], 0.0)
            dp = dp + pdf * pick_p[ci] / psafe
            rp = rp + pdf * pick_p[ci] / psafe
        ok &= (f != 0.0).any(1)
        dir_pdf = dp * ccont[ci]
        rev_pdf = rp * lcont[li]
        w_light = ldvcm[li] * mis_vc + ldvm[li] * dir_pdf
        w_cam = C[ci, 7].astype(np.float64) * mis_vc + C[ci, 11].astype(np.float64) * rev_pdf
        contrib = np.where(ok[:, None], f * lthr[li] / (w_light + 1.0 + w_cam)[:, None], 0.0)
        per_vertex = np.zeros((len(C), 3), np.float64)
        np.add.at(per_vertex, ci, contrib)
        np.add.at(color, pix, C[:, 4:7].astype(np.float64) * vm_norm * per_vertex)
    return color, count
