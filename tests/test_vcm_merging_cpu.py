"""Vertex merging (orx_config.vcm_merging), the parts that need no GPU: the MIS constants
(orx_vcm_mis_factors), the config field and its ctypes mirror, and the NumPy brute-force checker
(tests/vcm_merge_ref.py) on hand-built vertices whose expected value is worked out here."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import vcm_merge_ref
from oppositerenderer_amd import _abi, renderer, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _factors(lib, w, h, r, merging):
    vc, vm, nrm = C.c_float(), C.c_float(), C.c_float()
    st = lib.orx_vcm_mis_factors(w, h, r, merging, C.byref(vc), C.byref(vm), C.byref(nrm))
    assert st == _abi.ORX_OK
    return np.float32(vc.value), np.float32(vm.value), np.float32(nrm.value)


@pytest.mark.parametrize("w,h,r", [(32, 32, 7.5), (1920, 1080, 0.02), (1, 1, 1.0)])
def test_mis_factors_match_float32_formulas(w, h, r):
    lib = renderer.load_library()
    f32 = np.float32
    pi = f32(3.14159265358979323846)
    count = f32(w * h)
    r2 = f32(r) * f32(r)
    eta = f32(f32(f32(count / f32(1)) * pi) * r2)        # (float)(W H) * pi * r^2, left to right
    want_vc = f32(1) / eta
    want_norm = f32(1) / f32(f32(r2 * pi) * count)        # 1 / (r^2 * pi * (float)(W H))
    vc, vm, nrm = _factors(lib, w, h, r, 1)
    assert vc.tobytes() == f32(want_vc).tobytes()
    assert vm.tobytes() == eta.tobytes()
    assert nrm.tobytes() == f32(want_norm).tobytes()
    vc0, vm0, nrm0 = _factors(lib, w, h, r, 0)
    assert vm0 == 0.0 and vc0.tobytes() == vc.tobytes() and nrm0.tobytes() == nrm.tobytes()
    # the checker's own restatement is the same arithmetic
    ref = vcm_merge_ref.mis_factors(w, h, r)
    assert [v.tobytes() for v in ref] == [vc.tobytes(), vm.tobytes(), nrm.tobytes()]


def test_mis_factors_null_outputs():
    lib = renderer.load_library()
    v = C.c_float()
    p = C.byref(v)
    null = C.POINTER(C.c_float)()
    for args in ((null, p, p), (p, null, p), (p, p, null)):
        assert lib.orx_vcm_mis_factors(4, 4, 1.0, 1, *args) == _abi.ORX_ERR_INVALID_ARGUMENT


def test_default_config_leaves_merging_off():
    lib = renderer.load_library()
    cfg = _abi.OrxConfig()
    cfg.vcm_merging = 7
    lib.orx_default_config(C.byref(cfg))
    assert cfg.vcm_merging == 0
    assert list(cfg.reserved) == [0, 0]
    assert _abi.default_config().vcm_merging == 0


def test_config_size_and_field_offset_match_c():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "orx.h"
int main(void){
 printf("%zu %zu %zu %u %d %d %d %d %d %d %d\n", sizeof(orx_config), offsetof(orx_config, vcm_merging),
        offsetof(orx_config, reserved), (unsigned)ORX_ABI_VERSION, (int)ORX_BUF_VCM_CAMERA_VERTEX_COUNT,
        (int)ORX_BUF_VCM_CAMERA_VERTICES, (int)ORX_BUF_VCM_MERGE, (int)ORX_BUF_VCM_MERGE_COUNT,
        (int)ORX_PASS_VCM_GRID, (int)ORX_PASS_VCM_MERGE, (int)sizeof(orx_stats));
 return 0;}
"""
    d = tempfile.mkdtemp()
    src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
    open(src, "w").write(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals[0] == 64 and C.sizeof(_abi.OrxConfig) == 64
    assert vals[1] == _abi.OrxConfig.vcm_merging.offset == 52
    assert vals[2] == _abi.OrxConfig.reserved.offset == 56
    assert vals[3] == 1
    assert vals[4:8] == [_abi.BUF_VCM_CAMERA_VERTEX_COUNT, _abi.BUF_VCM_CAMERA_VERTICES, _abi.BUF_VCM_MERGE,
                         _abi.BUF_VCM_MERGE_COUNT] == [16, 17, 18, 19]
    assert vals[8:10] == [_abi.PASS_VCM_GRID, _abi.PASS_VCM_MERGE] == [11, 12]
    assert vals[10] == C.sizeof(_abi.OrxStats)
    assert len(_abi.PASS_NAMES) == 11   # tools enumerate it: the merging passes are separate constants


# ---- the checker on hand-built vertices ----
W = H = 4
R = 2.0
KD = 0.8
C_THR, L_THR = (0.5, 0.25, 1.0), (3.0, 2.0, 1.0)
C_DVCM, C_DVM, L_DVCM, L_DVM = 0.7, 0.3, 1.9, 0.6


def _one_pair(light_pos, light_fix=(0.0, 0.0, 1.0)):
    """One Lambert camera vertex at the origin of the plane z = 0 (ray arriving straight down) in pixel 5,
    one Lambert light vertex of subpath 9 on the same plane."""
    sc = scenes.Scene("pair")
    mat = sc.add_material(scenes.Diffuse(KD))
    npx = W * H
    cam = np.zeros((3, npx, 16), np.float32)
    lig = np.zeros((9, npx, 16), np.float32)
    ccount = np.zeros(npx, np.uint32)
    lcount = np.zeros(npx, np.uint32)
    matbits = np.array([mat], np.uint32).view(np.float32)[0]
    cam[0, 5] = [0, 0, 0, matbits, *C_THR, C_DVCM, 0, 0, 1, C_DVM, 0, 0, -1, 0]
    ccount[5] = 1
    lig[0, 9] = [*light_pos, matbits, *L_THR, L_DVCM, 0, 0, 1, 123.0, *light_fix, L_DVM]
    lcount[9] = 1
    # stale slots beyond the counts must be ignored
    cam[1, 5] = cam[0, 5]
    lig[1, 9] = lig[0, 9]
    return vcm_merge_ref.merge_reference(lig, lcount, cam, ccount, sc.materials, W, H, R)


def test_reference_one_lambert_pair_inside_the_radius():
    color, count = _one_pair((R / 2, 0.0, 0.0))
    kd = float(np.float32(KD))
    mis_vc, _, vm_norm = (float(v) for v in vcm_merge_ref.mis_factors(W, H, R))
    # both directions are the plane's normal: cos = 1 on either side, Lambert only (pick ratio 1)
    f = kd / math.pi
    dir_pdf = (1.0 / math.pi) * kd        # camera BSDF pdf of the light direction x its continuation probability
    rev_pdf = (1.0 / math.pi) * kd        # reverse pdf x the light BSDF's continuation probability
    w_light = L_DVCM * mis_vc + L_DVM * dir_pdf
    w_camera = C_DVCM * mis_vc + C_DVM * rev_pdf
    # float32 record fields: compare at float32 input precision
    want = [c * vm_norm * f * l / (w_light + 1.0 + w_camera) for c, l in zip(C_THR, L_THR)]
    assert count.sum() == 1 and count[5] == 1
    np.testing.assert_allclose(color[5], want, rtol=1e-6)
    assert (np.delete(color, 5, axis=0) == 0).all()
    assert (color[5] > 0).all()


def test_reference_pair_just_outside_the_radius():
    color, count = _one_pair((float(np.nextafter(np.float32(R), np.float32(10))), 0.0, 0.0))
    assert count.sum() == 0 and (color == 0).all()
    # and exactly at the radius the float32 test d2 <= r2 accepts
    color, count = _one_pair((R, 0.0, 0.0))
    assert count.sum() == 1 and (color[5] > 0).all()


def test_reference_light_vertex_on_the_back_side():
    """The light vertex's dirFix points below the camera vertex's surface (gen.z < EPS_COSINE): inside the
    radius, so the pair is counted, but vcmF is zero."""
    color, count = _one_pair((R / 2, 0.0, 0.0), light_fix=(0.0, 0.0, -1.0))
    assert count[5] == 1 and count.sum() == 1
    assert (color == 0).all()
