"""numpy / pure-Python restatement of include/fdf.h's BRIEF semantics, shared by
tests/test_describe.py (CPU) and tests/test_gpu_describe.py: the default pattern, the steering
table, the bin of an angle, 5 x 5 box smoothing and the descriptor itself."""
import functools
import math

import numpy as np


def default_pattern():
    """((256, 4) int8, draws): xorshift32 from 0x9E3779B9, six 3-bit draws per coordinate."""
    s = 0x9E3779B9

    def coord():
        nonlocal s
        v = -21
        for _ in range(6):
            s ^= (s << 13) & 0xFFFFFFFF
            s ^= s >> 17
            s ^= (s << 5) & 0xFFFFFFFF
            v += s >> 29
        return v

    tests, seen, draws = [], set(), 0
    while len(tests) < 256:
        t = tuple(coord() for _ in range(4))
        draws += 1
        if t[0] ** 2 + t[1] ** 2 > 169 or t[2] ** 2 + t[3] ** 2 > 169:
            continue
        if t[:2] == t[2:] or t in seen:
            continue
        seen.add(t)
        tests.append(t)
    return np.array(tests, dtype=np.int8), draws


def steer(pattern, n_bins):
    """(n_bins, 256, 4) int8: double rotation with y down, one rounding to float32, then
    half away from zero, saturated."""
    p = np.asarray(pattern).reshape(256, 4).astype(np.float64)
    out = np.empty((n_bins, 256, 4), np.int8)
    for b in range(n_bins):
        theta = 2 * math.pi * b / n_bins
        c, s = math.cos(theta), math.sin(theta)
        for k in (0, 2):
            x, y = p[:, k], p[:, k + 1]
            for j, v in ((k, x * c - y * s), (k + 1, x * s + y * c)):
                f = v.astype(np.float32).astype(np.float64)
                r = np.sign(f) * np.floor(np.abs(f) + 0.5)
                out[b, :, j] = np.clip(r, -128, 127).astype(np.int8)
    return out


def bin_scale(n_bins):
    return np.float32(n_bins / (2 * math.pi))


def bins_of(angles, n_bins):
    """The bin of every float32 angle: the float32 product rounded half to even, modulo
    n_bins; 0 unless |angle| <= 7."""
    a = np.asarray(angles, dtype=np.float32)
    ok = np.abs(a) <= np.float32(7)                       # False for NaN
    t = (np.where(ok, a, np.float32(0)) * bin_scale(n_bins)).astype(np.float32)
    return np.where(ok, np.rint(t).astype(np.int64) % n_bins, 0)


def smooth(img):
    h, w = img.shape
    p = np.pad(img.astype(np.int64), 2, mode="edge")
    s = np.zeros((h, w), np.int64)
    for dy in range(5):
        for dx in range(5):
            s += p[dy:dy + h, dx:dx + w]
    return ((s + 12) // 25).astype(np.uint8)


def describe(img, pts, table, bins=None):
    """(K, 32) uint8 descriptors of the points of one frame; `bins` (K,) or None for bin 0."""
    h, w = img.shape
    pts = np.asarray(pts).reshape(-1, 2)
    if bins is None:
        bins = np.zeros(len(pts), np.int64)
    x = pts[:, 0].astype(np.int64)[:, None]
    y = pts[:, 1].astype(np.int64)[:, None]
    t = np.asarray(table).reshape(-1, 256, 4)[np.asarray(bins)].astype(np.int64)
    a = img[np.clip(y + t[:, :, 1], 0, h - 1), np.clip(x + t[:, :, 0], 0, w - 1)]
    b = img[np.clip(y + t[:, :, 3], 0, h - 1), np.clip(x + t[:, :, 2], 0, w - 1)]
    return np.packbits(a < b, axis=1, bitorder="little").reshape(len(pts), 32)


@functools.lru_cache(maxsize=None)
def default_table(n_bins):
    """The default pattern's steering table (computed once per n_bins; do not modify)."""
    t = steer(default_pattern()[0], n_bins)
    t.setflags(write=False)
    return t
