"""A numpy restatement of include/fdf.h's RANSAC fundamental-matrix estimation
(fdf_fundamental_device, fdf_fundamental_check_device), independent of the kernels: the sampling in
Python integers, the fit of a sample in plain Python doubles with one operation per statement
(a Python float operation is one IEEE binary64 operation, never fused), the score as elementwise
float64 array operations in the stated order, the tie rules by explicit first-maximum scans."""
import math

import numpy as np

from _ransac_reference import (COORDS_F32, COORDS_U32, MODEL_DTYPE, NONE, correspondences,
                               frame_range, identity_matches, models_equal, start_state)

__all__ = ["COORDS_F32", "COORDS_U32", "MODEL_DTYPE", "NONE", "identity_matches", "models_equal"]

S = 8
MAX_DRAWS = 32
MIN_PIVOT = 2.0 ** -20
_U32 = 0xFFFFFFFF
_INF = float("inf")


def sample(seed, frame, hyp, m):
    """(the 8 correspondence numbers or None, the draws made) of one hypothesis."""
    st = start_state(seed, frame, hyp)
    got = []
    for draw in range(1, MAX_DRAWS + 1):
        st ^= (st << 13) & _U32
        st ^= st >> 17
        st ^= (st << 5) & _U32
        j = (st * m) >> 32
        if j not in got:
            got.append(j)
            if len(got) == S:
                return got, draw
    return None, MAX_DRAWS


def _div(a, b):
    """a / b as IEEE binary64 divides (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(_INF, a) * math.copysign(1.0, b)


def _normalise(px, py):
    """(cx, cy, d, scale) of 8 points: sequential sums in sample order from +0.0."""
    sx = 0.0
    sy = 0.0
    for k in range(S):
        sx = sx + px[k]
        sy = sy + py[k]
    cx = sx / 8.0
    cy = sy / 8.0
    d = 0.0
    for k in range(S):
        ax = abs(px[k] - cx)
        ay = abs(py[k] - cy)
        a = ax + ay
        d = d + a
    scale = _div(16.0, d)
    return cx, cy, d, scale


def fit(x, y, u, v):
    """The fundamental matrix of one sample of 8 pairs (sequences of Python floats):
    (9 floats, valid)."""
    x, y, u, v = ([float(c) for c in a] for a in (x, y, u, v))
    cx, cy, d, s = _normalise(x, y)
    cu, cv, e, t = _normalise(u, v)
    valid = 0.0 < d < _INF and 0.0 < e < _INF
    A = []
    for k in range(S):
        X = (x[k] - cx) * s
        Y = (y[k] - cy) * s
        U = (u[k] - cu) * t
        V = (v[k] - cv) * t
        A.append([U * X, U * Y, U, V * X, V * Y, V, X, Y, 1.0])

    row_used = [False] * 8
    col_used = [False] * 9
    pivot_col = [0] * 8
    for _ in range(8):
        best, pr, pc = -1.0, 0, 0
        for r in range(8):
            for c in range(9):
                if row_used[r] or col_used[c]:
                    continue
                mag = abs(A[r][c])
                if mag > best:                            # a NaN never wins; ties: lowest r, c
                    best, pr, pc = mag, r, c
        if not best >= MIN_PIVOT:
            valid = False
        row_used[pr] = True
        col_used[pc] = True
        pivot_col[pr] = pc
        piv = A[pr][pc]
        for r in range(8):
            if r == pr:
                continue
            m = _div(A[r][pc], piv)
            for j in range(9):
                if col_used[j]:
                    continue
                p = m * A[pr][j]
                A[r][j] = A[r][j] - p
    free = col_used.index(False)
    fn = [0.0] * 9
    fn[free] = 1.0
    for r in range(8):
        q = _div(A[r][free], A[r][pivot_col[r]])
        fn[pivot_col[r]] = -q

    B = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        a0 = fn[3 * r] * s
        a1 = fn[3 * r + 1] * s
        p0 = a0 * cx
        p1 = a1 * cy
        a2 = fn[3 * r + 2] - p0
        a2 = a2 - p1
        B[r] = [a0, a1, a2]
    F = [0.0] * 9
    for c in range(3):
        g0 = t * B[0][c]
        g1 = t * B[1][c]
        p0 = g0 * cu
        p1 = g1 * cv
        g2 = B[2][c] - p0
        g2 = g2 - p1
        F[c], F[3 + c], F[6 + c] = g0, g1, g2

    best, kb = -1.0, 0
    for k in range(9):
        mag = abs(F[k])
        if mag > best:
            best, kb = mag, k
    if not (0.0 < best < _INF):
        valid = False
    div = F[kb]
    out = [0.0] * 9
    for k in range(9):
        out[k] = _div(F[k], div)
        if not math.isfinite(out[k]):
            valid = False
    return out, valid


def inliers(f, x, y, u, v, threshold):
    """(H, M) bool: correspondence m is an inlier of model f[k] ((H, 9))."""
    T = np.float64(np.float32(threshold))
    f = np.asarray(f, dtype=np.float64).reshape(-1, 9)[:, :, None]
    with np.errstate(all="ignore"):
        l0 = (f[:, 0] * x + f[:, 1] * y) + f[:, 2]
        l1 = (f[:, 3] * x + f[:, 4] * y) + f[:, 5]
        l2 = (f[:, 6] * x + f[:, 7] * y) + f[:, 8]
        m0 = (f[:, 0] * u + f[:, 3] * v) + f[:, 6]
        m1 = (f[:, 1] * u + f[:, 4] * v) + f[:, 7]
        r = (u * l0 + v * l1) + l2
        g = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        return (g > 0) & (r * r <= (T * T) * g)


def hypotheses(x, y, u, v, frame, n_hyp, seed):
    """((n_hyp, 9) models, (n_hyp,) valid) of a frame's correspondences."""
    M = len(x)
    f = np.zeros((n_hyp, 9))
    valid = np.zeros(n_hyp, dtype=bool)
    xs, ys, us, vs = (np.asarray(a, dtype=np.float64).tolist() for a in (x, y, u, v))
    for k in range(n_hyp):
        got, _ = sample(seed, frame, k, M)
        if got is not None:
            f[k], valid[k] = fit([xs[j] for j in got], [ys[j] for j in got],
                                 [us[j] for j in got], [vs[j] for j in got])
    return f, valid


def estimate(x, y, u, v, frame, n_hyp, threshold, seed):
    """(model record, (M,) inlier flags, (n_hyp,) counts with -1 for an invalid hypothesis)."""
    rec = np.zeros((), dtype=MODEL_DTYPE)
    rec["n_corr"], rec["hypothesis"] = len(x), NONE
    f, valid = hypotheses(x, y, u, v, frame, n_hyp, seed)
    counts = np.full(n_hyp, -1, dtype=np.int64)
    flags = np.zeros(len(x), dtype=bool)
    if valid.any():
        inl = inliers(f, x, y, u, v, threshold)
        counts = np.where(valid, inl.sum(axis=1), -1)
        best = int(counts.argmax())                       # the first maximum: the lowest h
        rec["h"], rec["n_inliers"], rec["hypothesis"] = f[best], counts[best], best
        rec["n_valid"] = valid.sum()
        flags = inl[best]
    return rec, flags, counts


def fundamental(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, n_hyp, threshold,
                seed, inliers_out=None):
    """fdf_fundamental_device: ((F,) model records, the inlier bytes: `inliers_out`'s fill outside
    [qo[0], min(qo[F], q_cap)))."""
    n_frames = len(q_offs) - 1
    models = np.zeros(n_frames, dtype=MODEL_DTYPE)
    out = np.zeros(q_cap, dtype=np.uint8) if inliers_out is None else inliers_out.copy()
    for f in range(n_frames):
        qb, qe = frame_range(q_offs, q_cap, f)
        i, x, y, u, v = correspondences(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap,
                                        t_offs, f)
        models[f], flags, _ = estimate(x, y, u, v, f, n_hyp, threshold, seed)
        out[qb:qe] = 0
        out[i[flags]] = 1
    return models, out


def check(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, models_in, threshold,
          inliers_out=None):
    """fdf_fundamental_check_device: the caller's matrices recounted under `threshold`."""
    n_frames = len(q_offs) - 1
    models = np.array(models_in[:n_frames], dtype=MODEL_DTYPE)
    out = np.zeros(q_cap, dtype=np.uint8) if inliers_out is None else inliers_out.copy()
    for f in range(n_frames):
        qb, qe = frame_range(q_offs, q_cap, f)
        out[qb:qe] = 0
        if models[f]["hypothesis"] == NONE:
            continue
        i, x, y, u, v = correspondences(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap,
                                        t_offs, f)
        flags = inliers(models[f]["h"], x, y, u, v, threshold)[0] if len(x) else \
            np.zeros(0, dtype=bool)
        models[f]["n_corr"], models[f]["n_inliers"] = len(x), flags.sum()
        out[i[flags]] = 1
    return models, out


def models_bits_equal(a, b):
    """Field-by-field ==, the nine doubles by their bits."""
    ha = np.ascontiguousarray(a["h"]).view(np.uint64)
    hb = np.ascontiguousarray(b["h"]).view(np.uint64)
    return bool(np.array_equal(ha, hb) and
                all(np.array_equal(a[k], b[k]) for k in ("n_corr", "n_inliers", "hypothesis",
                                                         "n_valid")))


# ---- the scenes of the ground-truth tests ---------------------------------------------------

def scene_a(seed, noise=0.0):
    """200 points before two pinhole cameras (f = 500, principal point (320, 240), rotation
    0.1 rad about y, translation (0.5, 0.05, 0.1)); 60 train points replaced by uniform random
    positions.  (q float32 (200, 2), t float32 (200, 2), (200,) bool: a true pair)."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(4, 8, 200)], 1)
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    a = 0.1
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    tr = np.array([0.5, 0.05, 0.1])
    p1 = (K @ P.T).T
    p2 = (K @ (R @ P.T + tr[:, None])).T
    q = p1[:, :2] / p1[:, 2:]
    t = p2[:, :2] / p2[:, 2:]
    if noise:
        q = q + rng.normal(0, noise, q.shape)
        t = t + rng.normal(0, noise, t.shape)
    true = np.ones(200, dtype=bool)
    bad = rng.permutation(200)[:60]
    true[bad] = False
    t[bad] = np.stack([rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)], 1)
    return q.astype(np.float32), t.astype(np.float32), true


def scene_b(seed):
    """A rectified pair in integer coordinates: u = x + disparity, v = y; 20 of 100 pairs moved
    vertically by at least 5 px.  (q uint32, t uint32, (100,) bool: a true pair)."""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.integers(40, 600, 100), rng.integers(40, 440, 100)], 1)
    t = q.copy()
    t[:, 0] += rng.integers(1, 40, 100)
    true = np.ones(100, dtype=bool)
    bad = rng.permutation(100)[:20]
    true[bad] = False
    t[bad, 1] += rng.integers(5, 30, 20) * rng.choice([-1, 1], 20)
    return q.astype(np.uint32), t.astype(np.uint32), true


def scene_c(seed):
    """All points on one plane, exact coordinates: the train points are the query points under
    an integer affine map.  (q uint32, t uint32)."""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.integers(0, 200, 60), rng.integers(0, 200, 60)], 1)
    t = np.stack([2 * q[:, 0] + q[:, 1] + 7, q[:, 0] + 3 * q[:, 1] + 11], 1)
    return q.astype(np.uint32), t.astype(np.uint32)


def worked_example():
    """include/fdf.h's example: a rectified pair with two bad matches, (q_coords, t_coords) as
    uint32; seed 3, 8 hypotheses, T = 0.5."""
    q = 10 * np.array([(0, 0), (8, 0), (0, 8), (8, 8), (4, 2), (2, 6), (6, 4), (3, 3), (5, 7),
                       (7, 1), (1, 5), (6, 6)], dtype=np.uint32)
    d = np.array([(10, 0), (25, 0), (31, 0), (12, 0), (23, 0), (37, 0), (14, 0), (29, 0), (3, 0),
                  (20, 30), (18, 0), (40, 20)], dtype=np.uint32)
    return q, q + d
