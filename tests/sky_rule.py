"""The sky-map rule of include/bhrt_api.h ("Sky maps") in numpy: the map's texels from either
input format, the bilinear lookup of a vector, and which vector a ray of each class looks up.
Float64 throughout, one operation per rounding, in the header's order."""
import numpy as np

from bhrt import abi

RGB32F, RGBA8 = abi.BHRT_SKY_RGB32F, abi.BHRT_SKY_RGBA8


def texels(data):
    """The map's float32 texels [H, W, 3] from an input array of either format."""
    t = np.asarray(data)
    if t.dtype == np.uint8:
        assert t.ndim == 3 and t.shape[2] == 4
        return t[:, :, :3].astype(np.float32) / np.float32(255.0)
    assert t.dtype == np.float32 and t.ndim == 3 and t.shape[2] == 3
    return t


def lookup(data, d):
    """The lookup of vectors d [n, 3] in the map `data` (either format): float64 [n, 3]."""
    T = texels(data).astype(np.float64)
    H, W = T.shape[:2]
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        L = np.sqrt((dx * dx + dy * dy) + dz * dz)
        ok = (L > 0.0) & np.isfinite(L)
        Ls = np.where(ok, L, 1.0)
        c = np.minimum(np.maximum(dz / Ls, -1.0), 1.0)
        theta = np.arccos(np.where(ok, c, 0.0))
        phi = np.arctan2(np.where(ok, dy, 0.0), np.where(ok, dx, 1.0))
    fx = (phi + np.pi) * (W / (2.0 * np.pi)) - 0.5
    fy = theta * (H / np.pi) - 0.5
    fi, fj = np.floor(fx), np.floor(fy)
    wx, wy = (fx - fi)[:, None], (fy - fj)[:, None]
    i0 = np.mod(fi.astype(np.int64), W)
    i1 = np.mod(fi.astype(np.int64) + 1, W)
    j0 = np.clip(fj.astype(np.int64), 0, H - 1)
    j1 = np.clip(fj.astype(np.int64) + 1, 0, H - 1)
    ux, uy = 1.0 - wx, 1.0 - wy
    out = (T[j0, i0] * ux + T[j0, i1] * wx) * uy + (T[j1, i0] * ux + T[j1, i1] * wx) * wy
    out[~ok] = 0.0
    return out


def chord_counts(chord):
    """Whether an exit chord [n, 3] counts: every component finite, squared length > 0."""
    c = np.asarray(chord, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    return np.isfinite(c).all(axis=1) & (l2 > 0.0)


def vectors(result, chord, direction):
    """The vector each ray looks up: the exit chord of a RAY_MAX_DISTANCE ray whose chord counts,
    else the ray's own direction. (Disk and horizon rays look nothing up: see uses_sky.)"""
    result = np.asarray(result)
    take = (result == abi.RAY_MAX_DISTANCE) & chord_counts(chord)
    return np.where(take[:, None], np.asarray(chord, dtype=np.float64).reshape(-1, 3),
                    np.asarray(direction, dtype=np.float64).reshape(-1, 3)), take


def uses_sky(result):
    result = np.asarray(result)
    return (result != abi.RAY_DISK) & (result != abi.RAY_HORIZON)


def smooth_map(W=64, H=32):
    """The tests' smooth map: texel (i, j) channel c = 0.5 + 0.25 (a_c . dir) at the texel's
    centre, for three fixed unit vectors a_c: it changes by <= 0.25 per radian everywhere."""
    a = np.array([[1.0, 2.0, 2.0], [-2.0, 1.0, 2.0], [2.0, -2.0, 1.0]]) / 3.0
    th = (np.arange(H) + 0.5) * (np.pi / H)
    ph = (np.arange(W) + 0.5) * (2.0 * np.pi / W) - np.pi
    dirs = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :],
                     np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.cos(th)[:, None] * np.ones(W)[None, :]], axis=2)
    return (0.5 + 0.25 * dirs @ a.T).astype(np.float32)
