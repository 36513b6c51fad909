"""Numpy restatement of include/fdf.h's warp rules: the position of a destination pixel in
float64 ufuncs, one operation at a time (numpy never fuses a multiply with an add), the pixel sum
in int64, and fdf_model_invert's fixed sequence.  Nothing here calls the library; the tests
compare the library with this, bit for bit."""
import numpy as np

ONE = 2048
LIMIT = float(1 << 30)
REPLICATE, CONSTANT = 0, 1


def positions(h, dst_w, dst_h):
    """(valid, X, Y) of every destination pixel: (dst_h, dst_w) bool, int64, int64 (X and Y are 0
    where the pixel is not valid)."""
    h = np.asarray(h, dtype=np.float64).reshape(9)
    x = np.arange(dst_w, dtype=np.float64)[None, :]
    y = np.arange(dst_h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        p = np.add(np.add(np.multiply(h[0], x), np.multiply(h[1], y)), h[2])
        q = np.add(np.add(np.multiply(h[3], x), np.multiply(h[4], y)), h[5])
        w = np.add(np.add(np.multiply(h[6], x), np.multiply(h[7], y)), h[8])
        sx = np.divide(p, w)
        sy = np.divide(q, w)
        fx = np.floor(np.add(np.multiply(sx, 2048.0), 0.5))
        fy = np.floor(np.add(np.multiply(sy, 2048.0), 0.5))
        # every comparison is false for a NaN
        valid = (w > 0) & (fx >= -LIMIT) & (fx <= LIMIT) & (fy >= -LIMIT) & (fy <= LIMIT)
    valid = np.broadcast_to(valid, (dst_h, dst_w))
    X = np.where(valid, fx, 0.0).astype(np.int64)
    Y = np.where(valid, fy, 0.0).astype(np.int64)
    return valid, X, Y


def warp(img, h, dst_w, dst_h, border=REPLICATE, fill=0):
    """``img`` (H, W) uint8 warped by ``h`` into (dst_h, dst_w): (pixels uint8, mask uint8)."""
    img = np.asarray(img)
    sh, sw = img.shape
    src = img.astype(np.int64)
    valid, X, Y = positions(h, dst_w, dst_h)
    ix, qx = X >> 11, X & 2047
    iy, qy = Y >> 11, Y & 2047

    def tap(cx, cy):
        v = src[np.clip(cy, 0, sh - 1), np.clip(cx, 0, sw - 1)]
        if border == CONSTANT:
            v = np.where((cx >= 0) & (cx < sw) & (cy >= 0) & (cy < sh), v, fill)
        return v

    total = np.zeros((dst_h, dst_w), dtype=np.int64)
    for b, wy in ((0, ONE - qy), (1, qy)):
        for a, wx in ((0, ONE - qx), (1, qx)):
            total += wy * wx * tap(ix + a, iy + b)
    assert total.max(initial=0) <= 255 << 22
    out = np.where(valid, (total + (1 << 21)) >> 22, fill).astype(np.uint8)
    mask = valid & (X >= 0) & (X <= (sw - 1) * ONE) & (Y >= 0) & (Y <= (sh - 1) * ONE)
    return out, mask.astype(np.uint8)


def model_invert(h):
    """The adjugate of ``h`` normalised to out[8] = 1, in fdf_model_invert's order, or None unless
    every entry is finite."""
    h = np.asarray(h, dtype=np.float64).reshape(9)
    m, s, d = np.multiply, np.subtract, np.divide
    with np.errstate(all="ignore"):
        c = [s(m(h[4], h[8]), m(h[5], h[7])), s(m(h[2], h[7]), m(h[1], h[8])),
             s(m(h[1], h[5]), m(h[2], h[4])), s(m(h[5], h[6]), m(h[3], h[8])),
             s(m(h[0], h[8]), m(h[2], h[6])), s(m(h[2], h[3]), m(h[0], h[5])),
             s(m(h[3], h[7]), m(h[4], h[6])), s(m(h[1], h[6]), m(h[0], h[7])),
             s(m(h[0], h[4]), m(h[1], h[3]))]
        out = np.array([d(c[k], c[8]) for k in range(8)] + [1.0], dtype=np.float64)
    return out if np.isfinite(out).all() else None
