"""Injected photon-grid and gather cases with a float64 brute-force reference (TEST INFRASTRUCTURE).

The uniform-grid photon map and its gather are driven through the slab-mode seam with inputs no
rendered frame produces: orx_ppm_local_trace fixes W, H, the radius and the emitted count,
orx_ppm_slab_import builds the grid over ANY photon records and orx_ppm_gather_external gathers
ANY hit points in the 28-byte export layout.  tests/test_gather_cases_cpu.py runs the cases on the
CPU oracle, tests/test_gpu_gather_injected.py on the device; both use this module's generators,
packer, reference, grid structure check and assertion.

Reference (IndirectRadianceEstimation.cu:59-67 as tests/test_detmath.py restates it), for a hit
point with the non-specular flag whose slab bin is owned:
    S = sum over photons with d^2 <= r2 and n.dir <= 0 of  w(d^2 / r2) * power
    w(u) = alpha (1 - (1 - exp(-beta u / 2)) / (1 - 0.141847)),  alpha = 1.818, beta = 1.953
    indirect = S / (pi r2) / (P P),   r2 = float(float32(r) * float32(r))
and exactly 0 for every other hit point.  All inputs are float32 values converted exactly.

Margins.  fp32 d^2 from correctly rounded differences carries at most about 4 * 2^-24 = 2.4e-7
relative error and a three-term dot about 3 * 2^-24 of |n|_1 |d|_1; MARGIN = 1e-6 is four times
that.  A pair is *certain* when d^2 <= r2 (1 - MARGIN) and n.d <= -MARGIN |n|_1 |d|_1, *ambiguous*
when it is not certain but d^2 <= r2 (1 + MARGIN) and n.d <= +MARGIN |n|_1 |d|_1.  The reference
returns lo (certain pairs), amb (ambiguous pairs), n_acc and an a-priori bound; an estimate passes
when  lo - bound <= got <= lo + amb + bound  per pixel and channel.  Cases with margin 0 test the
boundaries themselves (d^2 == r2 and n.d == 0 are accepted): there every pair within MARGIN of a
boundary must be exact in fp32 (each difference, product and partial sum representable), which the
reference asserts, so fp32 and float64 take the same decision and amb is empty by construction.

Bound (derived, not fitted; EPS = 2^-24).  Per accepted pair  b(u) = 2e-6 + 8 EPS + 12 EPS A(u) / w(u):
  2e-6          the project's bar for the weight polynomial (test_gather_weight_polynomial);
  8 EPS         the d^2 error (<= 4 EPS relative, above) through |u w'(u) / w(u)| <= 1.6 on [0, 1],
                rounded up;
  12 EPS A / w  Horner's five fused steps and the six rounded coefficients, each at most EPS of
                the magnitude sum A(u) = sum |c_k| u^k of the ORX_W5_C* constants (read from the
                source as test_detmath.py reads them); the d^2 form's rescaled coefficients
                c_k / r^(2k) / c_4' add one rounding each and are covered by the same 12.
Per pixel and channel  bound = sum b w power + n EPS sum w power + 4 EPS sum w power  (n accepted
pairs summed in any order; four roundings in the 1 / (pi r2) and 1 / emitted scale).
"""
import functools
import os
import re

import numpy as np

from oppositerenderer_amd import _abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
MARGIN = 1e-6
ALPHA, BETA, EXP_NEG_BETA = 1.818, 1.953, 0.141847
MAX_PAIRS = 3 * 10 ** 7
SEED = 1645301512
f32 = np.float32


@functools.lru_cache(None)
def w5_abs_coefficients():
    src = open(os.path.join(ROOT, "oppositerenderer_amd", "csrc", "orx_kernels.hip")).read()
    coef = {int(k): float(v) for k, v in re.findall(r"ORX_W5_C(\d) = ([-0-9.e]+)f", src)}
    assert sorted(coef) == list(range(6))
    return tuple(abs(float(f32(coef[k]))) for k in range(6))


def weight(u):
    """photonPower's weight in float64"""
    return ALPHA * (1.0 - (1.0 - np.exp(-BETA * u / 2.0)) / (1.0 - EXP_NEG_BETA))


def pair_bound(u, w):
    c = w5_abs_coefficients()
    A = np.zeros_like(u)
    for k in (5, 4, 3, 2, 1, 0):
        A = A * u + c[k]
    return 2e-6 + 8 * EPS + 12 * EPS * A / w


def radius2(radius):
    return float(f32(radius) * f32(radius))


def _exact32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64) == x


class Reference:
    """lo, amb, bound: float64 [m][3]; n_acc, n_amb: int64 [m]"""

    def __init__(self, m):
        self.lo = np.zeros((m, 3))
        self.amb = np.zeros((m, 3))
        self.bound = np.zeros((m, 3))
        self.n_acc = np.zeros(m, np.int64)
        self.n_amb = np.zeros(m, np.int64)

    def take(self, idx):
        r = Reference(len(idx))
        for k in ("lo", "amb", "bound", "n_acc", "n_amb"):
            setattr(r, k, getattr(self, k)[idx])
        return r


def reference(photons, pos, nrm, flagged, radius, P, margin=MARGIN):
    """The float64 brute force over every (hit point, photon) pair, chunked over hit points."""
    photons = np.asarray(photons, np.float32).reshape(-1, 9)
    n, m = len(photons), len(pos)
    assert n * m <= MAX_PAIRS, f"{n} photons x {m} hit points: over {MAX_PAIRS} pairs"
    ph = photons.astype(np.float64)
    px, py, pz = ph[:, 0], ph[:, 1], ph[:, 2]
    dx_, dy_, dz_ = ph[:, 3], ph[:, 4], ph[:, 5]
    pw = ph[:, 6:9]
    d1 = np.abs(ph[:, 3:6]).sum(1)
    r2 = radius2(radius)
    scale = 1.0 / (np.pi * r2) / float(P * P)
    ref = Reference(m)
    if n == 0:
        return ref
    q = np.asarray(pos, np.float32).astype(np.float64)
    nn = np.asarray(nrm, np.float32).astype(np.float64)
    n1 = np.abs(nn).sum(1)
    chunk = max(1, 2_000_000 // n)
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        ex, ey, ez = (q[s:e, 0, None] - px[None]), (q[s:e, 1, None] - py[None]), (q[s:e, 2, None] - pz[None])
        d2 = (ex * ex + ey * ey) + ez * ez
        a, b, c = nn[s:e, 0, None] * dx_[None], nn[s:e, 1, None] * dy_[None], nn[s:e, 2, None] * dz_[None]
        nd = (a + b) + c
        dm = margin * n1[s:e, None] * d1[None]
        fl = np.asarray(flagged[s:e], bool)[:, None]
        sure = (d2 <= r2 * (1.0 - margin)) & (nd <= -dm) & fl
        poss = (d2 <= r2 * (1.0 + margin)) & (nd <= dm) & fl
        if margin == 0.0:
            # boundary cases: whatever lies within MARGIN of a boundary must be exact in fp32
            near = (np.abs(d2 - r2) <= MARGIN * r2) & fl
            for t in (ex, ey, ez, ex * ex, ey * ey, ez * ez, ex * ex + ey * ey, d2):
                assert _exact32(t[near]).all(), "a pair near d^2 == r2 is not exact in fp32"
            near = (d2 <= r2 * (1.0 + MARGIN)) & (np.abs(nd) <= MARGIN * n1[s:e, None] * d1[None]) & fl
            for t in (a, b, c, a + b, nd):
                assert _exact32(t[near]).all(), "a pair near n.d == 0 is not exact in fp32"
        i, j = np.nonzero(poss)
        if len(i) == 0:
            continue
        u = d2[i, j] / r2
        w = weight(u)
        sure_ij = sure[i, j]
        contrib = w[:, None] * pw[j]
        berr = pair_bound(u, w)[:, None] * contrib
        k = e - s
        for ch in range(3):
            ref.lo[s:e, ch] = np.bincount(i[sure_ij], contrib[sure_ij, ch], k)
            ref.amb[s:e, ch] = np.bincount(i[~sure_ij], contrib[~sure_ij, ch], k)
            S = np.bincount(i, contrib[:, ch], k)
            nall = np.bincount(i, minlength=k)
            ref.bound[s:e, ch] = np.bincount(i, berr[:, ch], k) + nall * EPS * S + 4 * EPS * S
        ref.n_acc[s:e] = np.bincount(i[sure_ij], minlength=k)
        ref.n_amb[s:e] = np.bincount(i[~sure_ij], minlength=k)
    ref.lo *= scale
    ref.amb *= scale
    ref.bound *= scale
    return ref


def largest_contribution(photons, pos, nrm, radius, margin):
    """(index, d^2 / r2, n.d) of the accepted photon with the largest weight * power at one hit point"""
    ph = np.asarray(photons, np.float32).reshape(-1, 9).astype(np.float64)
    if len(ph) == 0:
        return None
    e = np.asarray(pos, np.float32).astype(np.float64)[None] - ph[:, 0:3]
    d2 = (e[:, 0] ** 2 + e[:, 1] ** 2) + e[:, 2] ** 2
    nv = np.asarray(nrm, np.float32).astype(np.float64)
    nd = ph[:, 3:6] @ nv
    r2 = radius2(radius)
    ok = (d2 <= r2 * (1 + margin)) & (nd <= margin * np.abs(nv).sum() * np.abs(ph[:, 3:6]).sum(1))
    if not ok.any():
        return None
    c = np.where(ok, weight(np.minimum(d2 / r2, 2.0)) * ph[:, 6:9].sum(1), -1.0)
    k = int(np.argmax(c))
    return k, float(d2[k] / r2), float(nd[k])


# ------------------------------------------------------------------ cases

class Case:
    """photons [n][9] float32 (position, direction, power); base hit points pos / nrm [W*H][3] and
    flagged [W*H]; segment k holds the base hit points permuted by seg_perm[k].  ref_key: cases
    with the same key share one brute-force reference (same photons, base hit points, radius, P,
    margin)."""

    def __init__(self, name, photons, pos, nrm, flagged, radius, W, H, P, **kw):
        self.name = name
        self.photons = np.ascontiguousarray(photons, np.float32).reshape(-1, 9)
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(W * H, 3)
        self.nrm = np.ascontiguousarray(nrm, np.float32).reshape(W * H, 3)
        self.flagged = np.asarray(flagged, bool).reshape(W * H)
        self.radius, self.W, self.H, self.P = float(f32(radius)), W, H, P
        self.seg_perm = kw.pop("seg_perm", [np.arange(W * H)])
        self.margin = kw.pop("margin", MARGIN)
        self.ref_key = kw.pop("ref_key", name)
        self.box = kw.pop("box", None)            # caller's photon box (ordered words) or None
        self.axis = kw.pop("axis", 0)
        self.nbins = kw.pop("nbins", 32)
        self.own = kw.pop("own", (0, 31))
        self.min_hit_frac = kw.pop("min_hit_frac", 0.5)  # flagged pixels with n_acc > 0 (cap)
        self.amb_frac = kw.pop("amb_frac", 0.0)          # flagged pixels that may have amb != 0 (cap)
        self.dense = kw.pop("dense", 0)                  # one cell must hold at least this many photons
        self.too_large = kw.pop("too_large", False)
        self.expect_cell = kw.pop("expect_cell", None)   # the cell size the case is built around (origin 100)
        assert not kw, kw
        assert len(self.photons) <= P * P * 4, "more photons than the import capacity"
        assert (self.photons[:, 6:9].max(1) > 0).all(), "the oracle takes a photon with power <= 0 as invalid"

    @property
    def segments(self):
        return len(self.seg_perm)

    @property
    def n(self):
        return len(self.photons)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _records(pos, dirs, power):
    return np.concatenate([np.asarray(pos, np.float32), np.asarray(dirs, np.float32),
                           np.asarray(power, np.float32)], axis=1)


def f2ord(v):
    """order-preserving float32 -> uint32 (include/orx.h orx_ppm_slab_import's photon_box)"""
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(w):
    w = np.asarray(w, np.uint32)
    return np.where(w & np.uint32(0x80000000), w & np.uint32(0x7fffffff), ~w).astype(np.uint32).view(np.float32)


def _random_photons(seed, n):
    rng = np.random.default_rng(seed)
    return _records(rng.uniform(100, 400, (n, 3)), _unit(rng, n), rng.uniform(0.2, 1.0, (n, 3)))


def _random_hitpoints(seed, m, lo=100.0, hi=400.0, unflagged=0.1):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (m, 3)).astype(np.float32), _unit(rng, m), rng.uniform(size=m) >= unflagged


def _corners(lo=100.0, hi=400.0):
    """two far photons that span the grid; they face +y, power 1/4"""
    return _records([[lo] * 3, [hi] * 3], [[0, 1, 0]] * 2, [[0.25] * 3] * 2)


def random_cases():
    W, H, P = 50, 37, 64
    ph = _random_photons(11, 16000)
    pos, nrm, fl = _random_hitpoints(12, W * H)
    idx = np.arange(W * H)
    kw = dict(ref_key="random", amb_frac=0.01)
    ext = ph[:, 0:3].max(0) - ph[:, 0:3].min(0)
    box = np.concatenate([f2ord(ph[:, 0:3].min(0) - f32(0.05) * ext), f2ord(ph[:, 0:3].max(0) + f32(0.05) * ext)])
    return [Case("random_s1", ph, pos, nrm, fl, 30.0, W, H, P, **kw),
            # three row-interleaved segments: the same hit points, rolled and reversed
            Case("random_s3", ph, pos, nrm, fl, 30.0, W, H, P, seg_perm=[idx, np.roll(idx, 777), idx[::-1].copy()], **kw),
            Case("photon_box", ph, pos, nrm, fl, 30.0, W, H, P, box=box, **kw)]


def multichunk_cases():
    W, H, P = 32, 24, 96
    ph = _random_photons(21, 36000)
    pos, nrm, fl = _random_hitpoints(22, W * H)
    n1 = 4 * 4097 + 1  # a partial last deposit group, and a second BS_CHUNK block of 8 slots
    return [Case("multichunk", ph, pos, nrm, fl, 20.0, W, H, P, amb_frac=0.01),
            Case("multichunk_partial", ph[:n1], pos, nrm, fl, 20.0, W, H, P, amb_frac=0.01, min_hit_frac=0.4)]


DENSE_CUBE = 251.0  # [251, 252]^3 straddles the half-cell face of its ~3.001-unit cell over [100, 400]^3


def dense_cell_cases():
    W, H, P = 32, 16, 64
    rng = np.random.default_rng(31)
    n = 6000
    ph = np.concatenate([_records(rng.uniform(DENSE_CUBE, DENSE_CUBE + 1, (n, 3)), _unit(rng, n),
                                  rng.uniform(0.2, 1.0, (n, 3))), _corners()])
    m = W * H
    pos = rng.uniform(DENSE_CUBE, DENSE_CUBE + 1, (m, 3))
    pos[m * 3 // 4:] = rng.uniform(DENSE_CUBE - 1, DENSE_CUBE + 2, (m - m * 3 // 4, 3))  # around the cube
    pos[:8] = DENSE_CUBE + np.array([[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)])  # on its corners
    nrm = _unit(rng, m)
    fl = np.ones(m, bool)
    return [Case(f"dense_cell_r{r}", ph, pos, nrm, fl, r, W, H, P, amb_frac=0.01, dense=n)
            for r in (2.0, 0.3, 40.0)]


LATTICE_BASE, LATTICE_N = 200.0, 12
# Far corner of the lattice case's photons: over [100, 299.9]^3 the reference's cell-size arithmetic gives a cell of
# exactly 2 with the origin at 100 (found by running the oracle; check_grid asserts it), so the integer lattice
# lies on cell faces and half-cell faces (y, z: SUBR) and on quarter-cell faces (x: SUBX), and a hit point on the
# lattice with r = 5 has its chord ends there too.
LATTICE_HI = float(np.float32(299.9))


def lattice_boundary_case():
    """photons on the integer lattice 200 + [0, 12)^3, r = 5: the photons at (3,4,0), (5,0,0), (0,3,4) and
    their permutations from a lattice hit point have d^2 == 25 == r2 exactly; a hit point moved one ulp
    (2^-15 at 270) along an axis puts the photon 5 units away on that axis outside, in float64 too
    (d^2 = 25 + 10 * 2^-15 + 2^-30).  Everything is an integer or a dyadic number: exact in fp32."""
    W, H, P = 16, 8, 64
    g = np.arange(LATTICE_N, dtype=np.float64) + LATTICE_BASE
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(41)
    # axis-aligned and diagonal dyadic directions; power dyadic
    dirs = np.array([[0, -1, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0.5, -0.5, 0.5],
                     [-0.5, 0.5, 0.25]])[rng.integers(0, 8, len(lat))]
    power = rng.integers(1, 9, (len(lat), 3)) / 8.0
    # The one-ulp twins sit on three lines of photons along the axes, away from the lattice: a twin moved
    # along x would see the lattice photons at (0,5,0) or (0,3,4) at d^2 = 25 + ulp^2, which fp32 rounds to 25
    # (accepted) and float64 does not: the perpendicular ulp vanishes.  On a line the only photons on the
    # sphere are the two at distance 5 along the line's own axis.
    lines, pts = [], []
    for a in range(3):
        p = np.full(3, 130.0)
        p[a] = 270.0
        for k in range(-6, 7):
            t = p.copy()
            t[a] += k
            lines.append(t)
        ulp = float(np.spacing(f32(p[a])))
        for s in (0.0, -ulp, ulp):
            t = p.copy()
            t[a] += s
            pts.append(t)
    ntwin = len(pts)
    ph = np.concatenate([_records(lat, dirs, power),
                         _records(lines, [[0, -1, 0]] * len(lines), [[0.5, 0.25, 1.0]] * len(lines)),
                         _corners(100.0, LATTICE_HI)])
    # lattice hit points; the last six have chord ends on the lattice's own faces
    for c in ((5, 5, 5), (6, 6, 6), (5, 6, 7), (6, 5, 4), (0, 0, 0), (11, 11, 11), (0, 6, 11), (7, 5, 6),
              (3, 4, 0), (5, 0, 0), (0, 3, 4), (4, 0, 3), (0, 5, 0), (0, 0, 5)):
        pts.append(np.array(c, np.float64) + LATTICE_BASE)
    while len(pts) < W * H:  # lattice and half-lattice points (dyadic; the latter have no photon on the sphere)
        pts.append(LATTICE_BASE + rng.integers(0, 23, 3) / 2.0)
    pos = np.array(pts[:W * H])
    assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
    nrm = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1]])[rng.integers(0, 4, W * H)]
    nrm[:ntwin] = [0, 1, 0]
    return Case("lattice_boundary", ph, pos, nrm, np.ones(W * H, bool), 5.0, W, H, P, margin=0.0, expect_cell=2.0)


FACING_POS = 250.0
BAND = 232.0 / 127.0 ** 2  # DIRQ_BAND over 127^2: where the int8 prefilter hands over to the exact test


def _sweep(half_steps):
    k = np.arange(-128, 129 - int(half_steps), dtype=np.float64) + (0.5 if half_steps else 0.0)
    s = [k * (0.03 / 128)]
    for v in (BAND, 0.5 / 127, 1.5 / 127, 2.5 / 127):
        for sg in (-1.0, 1.0):
            c = np.float32(sg * v)
            s.append(np.array([c, np.nextafter(c, f32(1)), np.nextafter(c, f32(-1))], np.float64))
    return np.concatenate(s)


def _facing_positions(n):
    """small integer offsets around the hit point, all within r = 5"""
    o = np.array([[i, j, k] for i in (-2, -1, 0, 1, 2) for j in (-2, -1, 0, 1, 2) for k in (-2, -1, 0, 1, 2)], np.float64)
    return FACING_POS + o[np.arange(n) % len(o)]


def facing_band_cases():
    W, H, P = 16, 8, 64
    m = W * H
    rng = np.random.default_rng(51)
    pos = np.full((m, 3), FACING_POS)
    idx = np.arange(m)
    # axis normal: n.d is the direction's y exactly (0 * x and 1 * y are exact), including y == 0
    s = _sweep(False).astype(np.float32).astype(np.float64)
    one = np.sqrt(np.maximum(0.0, 1.0 - s * s))
    dirs = np.concatenate([
        np.stack([one, s, 0 * s], 1),                      # unit directions
        np.stack([0 * s + 0.9, s, 0 * s + 0.9], 1),        # 1-norm > 1.7325: the direction word is 0
        np.stack([0 * s + 1.5, s, 0 * s + 0.25], 1),       # a component above 1: the direction word is 0
        np.stack([0 * s + 0.6, 0.6 + s, 0 * s + 0.6], 1),  # (0.6, 0.6, 0.6): word 0, faces away
        np.stack([0.25 * one, 0.25 * s, 0 * s], 1),        # short directions
        np.zeros((4, 3))])                                 # zero directions: n.d == 0, accepted
    n = len(dirs)
    ph = np.concatenate([_records(_facing_positions(n), dirs, rng.integers(1, 9, (n, 3)) / 8.0), _corners()])
    axis_n = np.tile([0.0, 1.0, 0.0], (m, 1))
    cases = [Case(f"facing_axis_x{scale}", ph, pos, axis_n * scale, np.ones(m, bool), 5.0, W, H, P, margin=0.0)
             for scale in (1.0, 0.5, 2.0)]  # 2: the normal's 1-norm is over the bound, its word is 0
    # generic unit normal: n.d = s |n|^2 up to rounding; |s| >= 1e-5 keeps every pair outside the margin
    nv = np.array([0.36, 0.48, 0.8]).astype(np.float32).astype(np.float64)
    tv = np.array([0.8, 0.0, -0.36])
    tv /= np.linalg.norm(tv)
    s = _sweep(True)
    assert np.abs(s).min() > 1e-5
    dirs = s[:, None] * nv[None] + np.sqrt(1.0 - s * s)[:, None] * tv[None]
    ph2 = np.concatenate([_records(_facing_positions(len(dirs)), dirs, rng.integers(1, 9, (len(dirs), 3)) / 8.0),
                          _corners()])
    for scale in (1.0, 0.5):
        cases.append(Case(f"facing_generic_x{scale}", ph2, pos, np.tile(nv * scale, (m, 1)), np.ones(m, bool), 5.0,
                          W, H, P, min_hit_frac=0.5))
    return cases


def dir_q8(v):
    """orx_kernels.hip dir_q8 restated: int8 snorm words q = rint(127 c), or 0 outside its bounds"""
    v = np.asarray(v, np.float32)
    q = np.rint(v * f32(127)).astype(np.int64)
    bad = ~(np.abs(v).sum(-1) <= f32(1.7325)) | ~(np.abs(v).max(-1) <= f32(1.0))
    q[bad] = 0
    return q


def facing_band_edge_case():
    """Directions whose int8 dot with the normal's word lies in (200, 232], at the far edge of the band, while
    the exact n.d is negative (accepted), and their negations (int8 dot in [-232, -200), n.d positive,
    rejected): all six quantisation errors are near half a step and pull the same way, so the integer dot is off
    by more than 200 of the 221 the bound at dir_q8 allows.  Found by enumerating the directions
    ((k1 + .504) / 127, (k2 + .504) / 127, -(k3 + .496) / 127) against one such normal; |n.d| >= 2 / 127^2 keeps
    every pair far outside the margin.  A band narrower than the error would take these decisions from the
    integer dot, wrongly."""
    W, H, P = 16, 8, 64
    m = W * H
    nv = np.array([(71 + 0.504) / 127, (72 + 0.504) / 127, (73 + 0.496) / 127]).astype(np.float32)
    k1, k2, k3 = np.meshgrid(np.arange(1, 110), np.arange(1, 110), np.arange(1, 125), indexing="ij")
    d = np.stack([(k1 + 0.504) / 127, (k2 + 0.504) / 127, -(k3 + 0.496) / 127], -1).astype(np.float32).reshape(-1, 3)
    qq = (dir_q8(d) * dir_q8(nv)[None]).sum(1)
    ex = (d.astype(np.float64) * nv.astype(np.float64)[None]).sum(1) * 127.0 ** 2
    sel = np.nonzero((qq > 200) & (qq <= 232) & (ex <= -2.0) & (np.abs(d).sum(1) <= 1.73))[0]
    assert len(sel) >= 64, len(sel)
    sel = sel[np.argsort(-qq[sel], kind="stable")][:64]
    assert qq[sel].min() > 205
    dirs = np.concatenate([d[sel], -d[sel]])
    rng = np.random.default_rng(52)
    ph = np.concatenate([_records(_facing_positions(len(dirs)), dirs, rng.integers(1, 9, (len(dirs), 3)) / 8.0),
                         _corners()])
    return Case("facing_band_edge", ph, np.full((m, 3), FACING_POS), np.tile(nv, (m, 1)), np.ones(m, bool), 5.0, W, H, P)


def degenerate_grid_cases():
    W, H, P = 16, 8, 64
    m = W * H
    rng = np.random.default_rng(61)
    nrm = np.tile([0.0, 1.0, 0.0], (m, 1))
    fl = np.ones(m, bool)
    down = [0.0, -1.0, 0.0]
    p0 = np.array([200.0, 300.0, 100.0])
    near = p0 + rng.uniform(-3, 3, (m, 3))  # r = 6: most hit points reach p0
    one = Case("degenerate_one_photon", _records([p0], [down], [[0.5, 0.25, 1.0]]), near, nrm, fl, 6.0, W, H, P)
    same = Case("degenerate_one_point", _records([p0] * 500, [down] * 500, rng.uniform(0.2, 1.0, (500, 3))), near, nrm,
                fl, 6.0, W, H, P)
    x = np.linspace(100.0, 400.0, 301)
    line_ph = _records(np.stack([x, 0 * x, 0 * x], 1), [down] * len(x), rng.uniform(0.2, 1.0, (len(x), 3)))
    line_hp = np.stack([rng.uniform(100, 400, m), rng.uniform(0, 2, m), rng.uniform(0, 2, m)], 1)
    line = Case("degenerate_line", line_ph, line_hp, nrm, fl, 6.0, W, H, P)
    # the same line lifted to y = z = 2^-11 in a caller box 2^-10 thick: the cell budget gives an [n,1,1] grid
    t = 2.0 ** -11
    thin_ph = line_ph.copy()
    thin_ph[:, 1:3] = t
    box = np.concatenate([f2ord([100.0, 0.0, 0.0]), f2ord([400.5, 2 * t, 2 * t])])
    thin = Case("degenerate_thin_box", thin_ph, line_hp, nrm, fl, 6.0, W, H, P, box=box)
    empty = Case("degenerate_empty", np.zeros((0, 9), np.float32), near, nrm, fl, 6.0, W, H, P, min_hit_frac=0.0)
    return [one, same, line, thin, empty]


def cornell_bins(nbins=32):
    sc = scenes.cornell()
    lo = np.asarray(sc.aabb_min, np.float64)
    ext = np.asarray(sc.aabb_max, np.float64) - lo
    return lo, ext / nbins


def ownership_cases():
    """hit points at slab-bin centres +- 0.4 bin on each axis in turn (nbins = 32 over the Cornell AABB)"""
    W, H, P, nb = 16, 12, 64, 32
    ph = _random_photons(11, 16000)
    rng = np.random.default_rng(71)
    lo, step = cornell_bins(nb)
    pos = rng.uniform(120, 380, (W * H, 3))
    k = 0
    for a in range(3):
        for b in range(nb):
            for off in (-0.4, 0.4):
                pos[k, a] = lo[a] + (b + 0.5 + off) * step[a]
                k += 1
    assert k == W * H
    nrm = _unit(rng, W * H)
    fl = np.ones(W * H, bool)
    return [Case(f"ownership_axis{a}_{own[0]}_{own[1]}", ph, pos, nrm, fl, 30.0, W, H, P, ref_key="ownership",
                 axis=a, nbins=nb, own=own, amb_frac=0.01)
            for a in range(3) for own in ((8, 15), (0, 31), (5, 4))]


def grid_too_large_case():
    W, H, P = 16, 8, 64
    rng = np.random.default_rng(81)
    n = 500
    xy = rng.uniform(100, 400, (n, 2))
    ph = _records(np.concatenate([xy, np.full((n, 1), 100.0)], 1), [[0, -1, 0]] * n, rng.uniform(0.2, 1.0, (n, 3)))
    pos = np.concatenate([rng.uniform(100, 400, (W * H, 2)), np.full((W * H, 1), 100.0)], 1)
    return Case("grid_too_large", ph, pos, np.tile([0.0, 1.0, 0.0], (W * H, 1)), np.ones(W * H, bool), 30.0, W, H, P,
                too_large=True, min_hit_frac=0.0)


@functools.lru_cache(None)
def all_cases():
    cs = (random_cases() + multichunk_cases() + dense_cell_cases() + [lattice_boundary_case()] + facing_band_cases()
          + [facing_band_edge_case()] + degenerate_grid_cases() + ownership_cases() + [grid_too_large_case()])
    return {c.name: c for c in cs}


# the cases the other kernel instantiations run as well (ORX_GATHER_DFORM=0, ORX_GATHER_KERNEL=2)
SETTING_CASES = ("random_s1", "random_s3", "dense_cell_r2.0", "dense_cell_r0.3", "dense_cell_r40.0", "lattice_boundary",
                 "facing_axis_x1.0", "facing_axis_x0.5", "facing_axis_x2.0", "facing_generic_x1.0", "facing_generic_x0.5",
                 "facing_band_edge")


# ------------------------------------------------------------------ packing and expectations

def export_plane(W, H):
    return (W * H + 3) & ~3


def pack_hitpoints(case):
    """`segments` segments of the 28-byte export layout, back to back: plane A [plane][4] position and
    flag bits, plane N [plane][3] the normal; plane = (H W + 3) & ~3"""
    plane = export_plane(case.W, case.H)
    m = case.W * case.H
    out = np.zeros((case.segments, plane * 7), np.float32)
    bits = np.where(case.flagged, np.uint32(_abi.PRD_HIT_NON_SPECULAR), np.uint32(0)).astype(np.uint32)
    for k, perm in enumerate(case.seg_perm):
        A = out[k, :plane * 4].reshape(plane, 4)
        N = out[k, plane * 4:].reshape(plane, 3)
        A[:m, 0:3] = case.pos[perm]
        A[:m, 3] = bits[perm].view(np.float32)
        N[:m] = case.nrm[perm]
    return out.reshape(-1)


def owned(case):
    """whether each base hit point's slab bin is owned, in float64; the bin coordinate must be far from a
    bin edge (a condition on the inputs), so fp32 and float64 agree"""
    lo, step = cornell_bins(case.nbins)
    t = (case.pos[:, case.axis].astype(np.float64) - lo[case.axis]) / step[case.axis]
    b = np.clip(np.floor(t), 0, case.nbins - 1)
    if case.own != (0, case.nbins - 1):
        frac = t - np.floor(t)
        assert ((frac > 1e-4) & (frac < 1 - 1e-4)).all(), f"{case.name}: a hit point on a slab-bin edge"
    return (b >= case.own[0]) & (b <= case.own[1])


_REF = {}


def case_reference(case):
    """the geometric reference of the base hit points (shared by ref_key), with the caps asserted"""
    if case.ref_key not in _REF:
        ref = reference(case.photons, case.pos, case.nrm, case.flagged, case.radius, case.P, case.margin)
        _REF[case.ref_key] = ref
    ref = _REF[case.ref_key]
    nfl = int(case.flagged.sum())
    hit = int((ref.n_acc[case.flagged] > 0).sum())
    namb = int((ref.amb[case.flagged] != 0).any(1).sum())
    assert hit >= case.min_hit_frac * nfl, f"{case.name}: only {hit} of {nfl} flagged hit points accept a photon"
    assert namb <= case.amb_frac * nfl, f"{case.name}: {namb} of {nfl} flagged hit points have ambiguous pairs"
    assert (ref.lo[~case.flagged] == 0).all() and (ref.bound[~case.flagged] == 0).all()
    return ref


def expected(case):
    """Reference per output pixel [segments][W*H]: not-owned hit points (and everything of a grid that is too
    large) expect exactly 0"""
    ref = case_reference(case)
    keep = owned(case) & (not case.too_large)
    refs = []
    for perm in case.seg_perm:
        r = ref.take(perm)
        z = ~keep[perm]
        r.lo[z] = r.amb[z] = r.bound[z] = 0.0
        r.n_acc[z] = 0
        refs.append(r)
    return refs


def check_estimate(case, got, label):
    """lo - bound <= got <= lo + amb + bound per pixel and channel; returns the worst |got - lo| / bound over
    the pixels without ambiguous pairs (an observation, never a threshold)"""
    got = np.asarray(got, np.float32).reshape(case.segments, case.W * case.H, 3).astype(np.float64)
    worst = 0.0
    for k, r in enumerate(expected(case)):
        g = got[k]
        bad = ~((g >= r.lo - r.bound) & (g <= r.lo + r.amb + r.bound))
        if bad.any():
            excess = np.where(bad, np.maximum(r.lo - r.bound - g, g - r.lo - r.amb - r.bound), -1.0)
            excess[np.isnan(g)] = np.inf
            px, ch = np.unravel_index(int(np.argmax(excess)), excess.shape)
            b = int(case.seg_perm[k][px])
            top = largest_contribution(case.photons, case.pos[b], case.nrm[b], case.radius, case.margin)
            msg = (f"{label} {case.name}: {int(bad.any(1).sum())} pixels outside the bound; worst: segment {k} pixel {px} "
                   f"(hit point {case.pos[b].tolist()}, normal {case.nrm[b].tolist()}) channel {ch}: n_acc {int(r.n_acc[px])}, "
                   f"got {g[px, ch]!r}, lo {r.lo[px, ch]!r}, amb {r.amb[px, ch]!r}, bound {r.bound[px, ch]!r}")
            if top is not None:
                msg += (f"; largest contribution: photon {top[0]} {case.photons[top[0]].tolist()} at d^2/r2 {top[1]!r}, "
                        f"n.d {top[2]!r}")
            raise AssertionError(msg)
        sel = (r.bound > 0) & (r.amb == 0)
        if sel.any():
            worst = max(worst, float((np.abs(g - r.lo)[sel] / r.bound[sel]).max()))
    return worst


# ------------------------------------------------------------------ grid structure

def readback_records(photon_buffer):
    """ORX_BUF_PHOTONS rows [power, position, direction] -> import records [position, direction, power]"""
    b = np.asarray(photon_buffer, np.float32).reshape(-1, 9)
    return np.concatenate([b[:, 3:6], b[:, 6:9], b[:, 0:3]], axis=1)


def _sorted_rows(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 9)
    return u[np.lexsort(u.T[::-1])]


def check_grid(case, stats, photon_buffer, offsets, label):
    """The grid over the imported photons, independent of the gather: every photon kept (as bit patterns),
    offsets a non-decreasing cover of them, every photon inside its cell's box grown by the kernels' own
    margin of 1e-3 cells.  Returns a description of the grid."""
    n = case.n
    g = [int(v) for v in stats.grid_size]
    cell = float(stats.cell_size)
    org = np.array([float(v) for v in stats.world_origin])
    desc = f"grid {g} cell {cell!r} origin {org.tolist()}"
    where = f"{label} {case.name} ({desc})"
    assert int(stats.valid_photons) == n, f"{where}: valid_photons {stats.valid_photons} of {n}"
    rec = readback_records(photon_buffer)
    assert rec.shape == (n, 9), f"{where}: {rec.shape[0]} photons read back"
    assert np.array_equal(_sorted_rows(rec), _sorted_rows(case.photons)), f"{where}: photons changed by the grid build"
    G = g[0] * g[1] * g[2]
    off = np.asarray(offsets, np.uint32).astype(np.int64)
    assert int(stats.num_cells) == G and len(off) == G + 1, f"{where}: {len(off)} offsets for {G} cells"
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all(), f"{where}: offsets do not cover the photons"
    if case.expect_cell is not None:
        assert cell == case.expect_cell and (org == 100.0).all() and g == [100, 100, 100], where
    if case.dense:
        assert np.diff(off).max() >= case.dense, f"{where}: the densest cell holds {np.diff(off).max()} photons"
    if n == 0:
        return desc
    if not np.isfinite(cell) or cell <= 0:
        assert g == [1, 1, 1], f"{where}: a grid of several cells without a finite cell size"
        return desc
    c = np.repeat(np.arange(G), np.diff(off))
    cxyz = np.stack([c % g[0], (c // g[0]) % g[1], c // (g[0] * g[1])], 1)
    t = (rec[:, 0:3].astype(np.float64) - org[None]) / cell
    # 1e-3 cells is the kernels' own margin m; the fp32 cell coordinate (pos - origin) * (1 / cell) carries three
    # roundings, at most 4 EPS of its value: 2.4e-5 cells on a 100-cell axis, but 0.04 on the 152 017-cell axis of
    # degenerate_thin_box
    tol = 1e-3 + 4 * EPS * np.abs(t)
    ok = (t >= cxyz - tol) & (t <= cxyz + 1 + tol)
    assert ok.all(), f"{where}: photon {rec[np.nonzero(~ok.all(1))[0][0]].tolist()} lies outside its cell"
    return desc


# ------------------------------------------------------------------ running a case on a shard backend

def request(W, H):
    from oppositerenderer_amd.renderer import RenderRequestDetails

    scene = scenes.cornell()
    cam = scene.default_camera.set_aspect_ratio(float(np.float32(W) / np.float32(H)))
    return RenderRequestDetails(cam, scene.name, _abi.PROGRESSIVE_PHOTON_MAPPING, W, H).to_abi()


def import_case(b, case, to_backend):
    """local_trace -> slab_import: the grid over the case's photons"""
    b.local_trace(0, 0, case.radius, request(case.W, case.H))
    rec = to_backend(case.photons.reshape(-1) if case.n else np.zeros(9, np.float32))
    b.slab_import(rec, case.n, case.box, case.axis, case.nbins, case.own)


def run_case(b, case, to_backend):
    """local_trace -> slab_import -> gather_external on a shard backend (multigpu.DeviceShard or
    oracle_lib.OracleShard, slab mode enabled); to_backend: numpy float32 -> the backend's tensor.
    Returns the gather output [segments][W*H][3]."""
    import_case(b, case, to_backend)
    hp = to_backend(pack_hitpoints(case))
    out = b.alloc(case.segments * case.W * case.H * 3)
    out.fill_(float("nan"))  # every pixel must be written
    b.gather_external(hp, case.segments, out)
    return out.cpu().numpy().reshape(case.segments, case.W * case.H, 3).copy()


# ------------------------------------------------------------------ a chord start within rounding of a quarter-cell face

CHORD_BOX = (100.3, 400.1)  # caller's photon box: a non-dyadic origin, so the cell coordinates round


def chord_probe_case():
    """any photons in CHORD_BOX: the grid follows the box alone, so its origin and cell can be read back and
    chord_edge_case built for them"""
    W, H, P = 16, 8, 64
    box = np.concatenate([f2ord([CHORD_BOX[0]] * 3), f2ord([CHORD_BOX[1]] * 3)])
    m = W * H
    return Case("chord_probe", _corners(150.0, 350.0), np.full((m, 3), 150.0), np.tile([0.0, 1.0, 0.0], (m, 1)),
                np.ones(m, bool), 5.0, W, H, P, box=box, margin=0.0)


def chord_edge_case(origin_x, cell):
    """A photon exactly on the sphere (r = 5, straight along -x from the hit point) that is the last one of its
    x quarter, while the hit point's chord start, computed as the kernels compute it but without their margin,
    fl(fl(x - o) - r), lands in the NEXT quarter: x - o lies just above a power of two and rounds up on a coarser
    grid than the photon's X - o = x - r - o below it.  The quarter is not the first of its cell, so the
    oracle's whole-cell window holds the photon.  Found by a search in numpy float32 for the grid the box gives
    (origin_x, cell as float32 from the stats); every pixel is the same hit point, so no other lane's chord
    covers the photon in the wave-union gather."""
    o, c = f32(origin_x), f32(cell)
    inv = f32(1) / c
    r = f32(5)
    mrg = f32(c * f32(1e-3))

    def quarter(v):
        return np.floor((v.astype(np.float32) * inv).astype(np.float32) * f32(4)).astype(np.int64)

    found = []
    for top, step in ((128.0, 2.0 ** -17), (256.0, 2.0 ** -16)):
        kk = np.arange(int(np.ceil((top - 5) * 4 / float(c))), int(np.floor(top * 4 / float(c))) + 1)
        for k in kk[kk % 4 != 0]:
            vk = np.floor(k * float(c) / 4 / step) * step
            A = (vk - step * np.arange(-64, 192)).astype(np.float32)  # candidates for X - o
            X = (A.astype(np.float64) + float(o))
            x = X + 5.0
            ok = _exact32(X) & _exact32(x) & (A.astype(np.float64) < top) & (x - float(o) >= top)
            x32, X32 = x.astype(np.float32), X.astype(np.float32)
            ok &= ((X32 - o).astype(np.float32) == A)
            npx = (x32 - o).astype(np.float32)
            bare = (npx - r).astype(np.float32)                      # chord start without the margin
            kept = (npx - (r + mrg).astype(np.float32)).astype(np.float32)  # and with it
            ok &= (quarter(A) == k - 1) & (quarter(bare) >= k) & (quarter(kept) <= k - 1)
            for i in np.nonzero(ok)[0]:
                found.append((float(x32[i]), float(X32[i])))
    assert found, f"no chord start rounds across a quarter face for origin {origin_x!r}, cell {cell!r}"
    W, H, P = 16, 8, 64
    m = W * H
    hx, px = found[0]
    yz = 250.0
    box = np.concatenate([f2ord([CHORD_BOX[0]] * 3), f2ord([CHORD_BOX[1]] * 3)])
    # the photon on the sphere, one a unit further in, one a unit outside, and every other found photon
    ph = _records([[px, yz, yz], [px + 1, yz, yz], [px - 1, yz, yz]] + [[b, yz + 20, yz] for _, b in found[1:8]],
                  [[0, -1, 0]] * (3 + len(found[1:8])), [[0.5, 0.25, 1.0]] * (3 + len(found[1:8])))
    case = Case("chord_edge", ph, np.tile([hx, yz, yz], (m, 1)), np.tile([0.0, 1.0, 0.0], (m, 1)), np.ones(m, bool),
                5.0, W, H, P, box=box, margin=0.0)
    case.found = found
    return case
