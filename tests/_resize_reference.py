"""Numpy restatement of include/fdf.h's resize and pyramid rules: the taps of an axis in Python
integers, the pixel formula in int64 and the size rule of the levels.  The tests compare the
library with this, bit for bit."""
import numpy as np

ONE = 2048


def tap(src_len, dst_len, i):
    """(i0, i1, q) of destination index ``i``."""
    s, d = int(src_len), int(dst_len)
    n = (2 * i + 1) * s - d
    i0, q = 0, 0
    if n >= 0:
        i0 = n // (2 * d)
        q = (4096 * (n % (2 * d)) + 2 * d) // (4 * d)
    if i0 >= s - 1:
        i0, q = (s - 2, ONE) if s > 1 else (0, 0)
    return i0, min(i0 + 1, s - 1), q


def taps(src_len, dst_len):
    """The table of an axis: (dst_len,) uint32, i0 << 12 | q."""
    return np.array([t[0] << 12 | t[2] for t in (tap(src_len, dst_len, i) for i in range(dst_len))],
                    dtype=np.uint32)


def resize(img, dst_w, dst_h):
    """``img`` (H, W) uint8 resized to (dst_h, dst_w): one rounding per pixel."""
    img = np.asarray(img)
    h, w = img.shape
    tx = np.array([tap(w, dst_w, i) for i in range(dst_w)], dtype=np.int64)
    ty = np.array([tap(h, dst_h, i) for i in range(dst_h)], dtype=np.int64)
    src = img.astype(np.int64)
    x0, x1, qx = tx[:, 0], tx[:, 1], tx[:, 2]
    y0, y1, qy = ty[:, 0][:, None], ty[:, 1][:, None], ty[:, 2][:, None]
    h0 = src[y0, x0] * (ONE - qx) + src[y0, x1] * qx
    h1 = src[y1, x0] * (ONE - qx) + src[y1, x1] * qx
    total = h0 * (ONE - qy) + h1 * qy
    assert total.max(initial=0) <= 255 << 22
    return ((total + (1 << 21)) >> 22).astype(np.uint8)


def level_sizes(width, height, n_levels, num=6, den=5):
    """[(w_l, h_l)] of the levels: each from the one before, rounded to nearest."""
    sizes = [(int(width), int(height))]
    for _ in range(1, n_levels):
        w, h = sizes[-1]
        sizes.append(((w * den + num // 2) // num, (h * den + num // 2) // num))
    return sizes


def pyramid(img, n_levels, num=6, den=5):
    """The levels of ``img``: level 0 is ``img`` itself, level l is level l - 1 resized."""
    h, w = np.asarray(img).shape
    levels = [np.asarray(img)]
    for lw, lh in level_sizes(w, h, n_levels, num, den)[1:]:
        levels.append(resize(levels[-1], lw, lh))
    return levels


def to_level0(points, size0, size_l):
    """Level coordinates (K, 2) mapped to level 0: (x_l + 0.5) * w_0 / w_l - 0.5 per axis, in
    float64, rounded to float32."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    size0 = np.array(size0, dtype=np.float64)
    size_l = np.array(size_l, dtype=np.float64)
    return ((pts + 0.5) * size0 / size_l - 0.5).astype(np.float32)
