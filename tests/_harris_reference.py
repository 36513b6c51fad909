"""The Harris response of include/fdf.h restated in numpy: clamped reads, 3 x 3 Sobel
gradients, a direct double loop over the block, everything in int64, and the rank score in
Python integers.  tests/test_harris.py pins this module to the worked values of the header's
semantics, so that the GPU tests compare the kernel with something that cannot drift."""
import numpy as np

A_MAX = 49 * 1020 ** 2            # the largest block sum (block 7)


def code(r):
    """The u16 rank score of one response (a Python integer)."""
    r = int(r)
    if r <= 0:
        return 0
    e = r.bit_length() - 1
    if e < 10:
        return r
    return ((e - 9) << 10) | ((r >> (e - 10)) & 1023)


def codes(responses):
    return np.array([code(r) for r in np.asarray(responses).reshape(-1)], dtype=np.uint16)


def sums(img, pts, block=7):
    """(a, b, c) int64 arrays of the points (K, 2) of one frame."""
    assert block in (3, 5, 7)
    h, w = img.shape
    px = np.ascontiguousarray(img).astype(np.int64)
    pts = np.asarray(pts).reshape(-1, 2)
    x = pts[:, 0].astype(np.int64)
    y = pts[:, 1].astype(np.int64)

    def I(cx, cy):
        return px[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]

    a = np.zeros(len(pts), np.int64)
    b = np.zeros(len(pts), np.int64)
    c = np.zeros(len(pts), np.int64)
    hb = block // 2
    for v in range(-hb, hb + 1):
        for d in range(-hb, hb + 1):
            X, Y = x + d, y + v
            ix = 2 * (I(X + 1, Y) - I(X - 1, Y)) + (I(X + 1, Y - 1) - I(X - 1, Y - 1)) + \
                (I(X + 1, Y + 1) - I(X - 1, Y + 1))
            iy = 2 * (I(X, Y + 1) - I(X, Y - 1)) + (I(X - 1, Y + 1) - I(X - 1, Y - 1)) + \
                (I(X + 1, Y + 1) - I(X + 1, Y - 1))
            a += ix * ix
            b += iy * iy
            c += ix * iy
    return a, b, c


def responses(img, pts, block=7, k=(1, 25)):
    """The int64 responses R = k_den (a b - c^2) - k_num (a + b)^2 of the points."""
    k_num, k_den = k
    assert 0 <= k_num <= 255 and 1 <= k_den <= 255
    a, b, c = sums(img, pts, block)
    assert a.max(initial=0) <= A_MAX and b.max(initial=0) <= A_MAX
    # both terms stay below 255 * (2 * A_MAX)^2 < 2^63: int64 holds every step
    return k_den * (a * b - c * c) - k_num * (a + b) * (a + b)


def reference(img, pts, block=7, k=(1, 25)):
    """(responses (K,) int64, rank scores (K,) uint16)."""
    r = responses(img, pts, block, k)
    return r, codes(r)


def checker3(n=24):
    """I = 255 where (x // 3 + y // 3) is odd, else 0."""
    ys, xs = np.mgrid[0:n, 0:n]
    return (((xs // 3 + ys // 3) & 1) * 255).astype(np.uint8)


def corner_frame():
    img = np.zeros((32, 32), np.uint8)
    img[16:, 16:] = 255
    return img


def edge_frame():
    img = np.zeros((32, 32), np.uint8)
    img[:, 16:] = 255
    return img


def select_reference(pts, scores, shape, cell, k):
    """Best k per cell of one frame by u16 score, ties to the earlier point, in input order
    (the rule of fdf_select_device); returns the keep mask."""
    h, w = shape
    cells_x = -(-w // cell[0])
    p = pts.astype(np.int64)
    cid = (p[:, 1] // cell[1]) * cells_x + p[:, 0] // cell[0]
    idx = np.arange(len(pts))
    order = np.lexsort((idx, -scores.astype(np.int64), cid))
    sc = cid[order]
    rank = idx - np.searchsorted(sc, sc, side="left")
    keep = np.zeros(len(pts), bool)
    keep[order[rank < k]] = True
    return keep
