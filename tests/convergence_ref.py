"""NumPy float32 restatement of the convergence statistics (include/orx.h, orx_set_convergence and
orx_get_convergence): every intermediate is a float32, in the order the header states, so the device's planes
can be compared bit for bit.

    window(sums, base)    S_1..S_n (and the window's base: None = a cleared sum) -> prev, A, M2
    error_plane(A, M2, n, floor) -> e, m
    tile_stats(e, m, W, H, threshold) -> the tile map and the frame's numbers in float64
"""
import numpy as np

f32 = np.float32
TILE = 16
KR, KG, KB = f32(0.2126), f32(0.7152), f32(0.0722)


def luminance(d):
    """y = (0.2126f d.r + 0.7152f d.g) + 0.0722f d.b on [...][3] float32"""
    d = np.asarray(d, f32)
    return ((KR * d[..., 0] + KG * d[..., 1]).astype(f32) + (KB * d[..., 2]).astype(f32)).astype(f32)


def window(sums, base=None):
    """sums: the running sums after each iteration of the window, [n][npx][3]; base: the sum the window
    started on ([npx][3]), None for a cleared one.  Returns (prev, A, M2) after the last iteration."""
    sums = [np.asarray(s, f32).reshape(-1, 3) for s in sums]
    prev = np.zeros_like(sums[0]) if base is None else np.asarray(base, f32).reshape(-1, 3).copy()
    A = np.zeros(sums[0].shape[0], f32)
    M2 = np.zeros(sums[0].shape[0], f32)
    for n, S in enumerate(sums, start=1):
        y = luminance((S - prev).astype(f32))
        if n == 1:
            A = y.copy()
            M2 = np.zeros_like(y)
        else:
            mo = (A / f32(n - 1)).astype(f32)
            A = (A + y).astype(f32)
            mn = (A / f32(n)).astype(f32)
            M2 = (M2 + ((y - mo).astype(f32) * (y - mn).astype(f32)).astype(f32)).astype(f32)
        prev = S.copy()
    return prev, A, M2


def error_plane(A, M2, n, floor):
    """se = sqrtf(M2 / ((float)n (float)(n-1))); m = A / (float)n; e = se / fmaxf(m, floor)"""
    A, M2 = np.asarray(A, f32), np.asarray(M2, f32)
    d = f32(f32(n) * f32(n - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt((M2 / d).astype(f32)).astype(f32)
        m = (A / f32(n)).astype(f32)
        e = (se / np.maximum(m, f32(floor))).astype(f32)
    return e, m


def tile_stats(e, m, W, H, threshold):
    """float64 tile means [tiles_y][tiles_x] of e over the pixels each 16x16 tile has, the frame's mean
    error and mean luminance, the pixels with e > threshold and the worst tile's index tx + tiles_x ty"""
    e = np.asarray(e, f32).reshape(H, W).astype(np.float64)
    m = np.asarray(m, f32).reshape(H, W).astype(np.float64)
    tx, ty = -(-W // TILE), -(-H // TILE)
    tiles = np.zeros((ty, tx))
    for j in range(ty):
        for i in range(tx):
            tiles[j, i] = e[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE].mean()
    above = int((np.asarray(e) > np.float64(f32(threshold))).sum())
    return {"tiles": tiles, "mean_error": e.mean(), "mean_luminance": m.mean(), "pixels_above": above,
            "max_tile": int(np.argmax(tiles)), "max_tile_error": tiles.max(), "tiles_x": tx, "tiles_y": ty}


def display_bytes64(sum_rgb, inv_iterations, inv_gamma):
    """the display rule with numpy.power in float64 (bytes may differ from the fp32 rule by 1): [...][3] uint8"""
    v = np.asarray(sum_rgb, f32).astype(np.float64) * np.float64(f32(inv_iterations))
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.power(np.where(v > 0, v, 0.0), np.float64(f32(inv_gamma))) * 255.0
    out = np.where(v > 0, np.minimum(255.0, g), 0.0)
    return np.floor(out).astype(np.uint8)
