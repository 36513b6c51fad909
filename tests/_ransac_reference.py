"""A numpy restatement of include/fdf.h's RANSAC model estimation (fdf_ransac_device),
independent of the kernels: the sampling in Python integers, the fit and the score as elementwise
float64 array operations vectorised over the hypotheses (numpy rounds every operation once and
never fuses two), the pivot and best-hypothesis tie rules by first-maximum argmax."""
import numpy as np

NONE = 0xFFFFFFFF
AFFINE, HOMOGRAPHY = 0, 1
COORDS_U32, COORDS_F32 = 0, 1
MAX_DRAWS = 16
MIN_PIVOT = 2.0 ** -20
MODEL_DTYPE = np.dtype([("h", "<f8", (9,)), ("n_corr", "<u4"), ("n_inliers", "<u4"),
                        ("hypothesis", "<u4"), ("n_valid", "<u4")])
_U32 = 0xFFFFFFFF


def sample_size(model):
    return {AFFINE: 3, HOMOGRAPHY: 4}[model]


def start_state(seed, frame, hyp):
    st = (seed + 0x9E3779B9 * (frame + 1) + 0x85EBCA6B * (hyp + 1)) & _U32
    st ^= st >> 16
    st = (st * 0x85EBCA6B) & _U32
    st ^= st >> 13
    st = (st * 0xC2B2AE35) & _U32
    st ^= st >> 16
    return st if st else 0x9E3779B9


def sample(seed, frame, hyp, m, s):
    """(the s correspondence numbers or None, the draws made) of one hypothesis."""
    st = start_state(seed, frame, hyp)
    got = []
    for draw in range(1, MAX_DRAWS + 1):
        st ^= (st << 13) & _U32
        st ^= st >> 17
        st ^= (st << 5) & _U32
        j = (st * m) >> 32
        if j not in got:
            got.append(j)
            if len(got) == s:
                return got, draw
    return None, MAX_DRAWS


def frame_range(offs, cap, f):
    b = min(int(offs[f]), int(cap))
    e = max(min(int(offs[f + 1]), int(cap)), b)
    return b, e


def correspondences(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, f):
    """(query indices, x, y, u, v) of frame f, the coordinates as float64."""
    qb, qe = frame_range(q_offs, q_cap, f)
    tb, te = frame_range(t_offs, t_cap, f)
    index = matches["index"][qb:qe].astype(np.int64)
    ok = (index != NONE) & (index >= tb) & (index < te)
    if keep is not None:
        ok &= np.asarray(keep)[qb:qe] != 0
    i = np.arange(qb, qe)[ok]
    q = np.asarray(q_coords)[i].astype(np.float64).reshape(-1, 2)
    t = np.asarray(t_coords)[index[ok]].astype(np.float64).reshape(-1, 2)
    return i, q[:, 0], q[:, 1], t[:, 0], t[:, 1]


def fit(x, y, u, v, model):
    """The models of H samples: x, y, u, v are (H, s); returns ((H, 9) float64, (H,) valid)."""
    H, s = x.shape
    N = 2 * s
    A = np.zeros((H, N, 8))
    b = np.zeros((H, N))
    one, rows = np.ones(H), np.arange(H)
    for k in range(s):
        xk, yk, uk, vk = x[:, k], y[:, k], u[:, k], v[:, k]
        A[:, 2 * k, 0], A[:, 2 * k, 1], A[:, 2 * k, 2] = xk, yk, one
        A[:, 2 * k, 6], A[:, 2 * k, 7] = -(uk * xk), -(uk * yk)
        A[:, 2 * k + 1, 3], A[:, 2 * k + 1, 4], A[:, 2 * k + 1, 5] = xk, yk, one
        A[:, 2 * k + 1, 6], A[:, 2 * k + 1, 7] = -(vk * xk), -(vk * yk)
        b[:, 2 * k], b[:, 2 * k + 1] = uk, vk
    A = np.ascontiguousarray(A[:, :, :N])
    valid = np.ones(H, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(N):
            mag = np.abs(A[:, c:, c])
            mag = np.where(np.isnan(mag), -1.0, mag)      # a NaN never wins
            p = mag.argmax(axis=1)                        # the first maximum: the lowest row
            valid &= mag[rows, p] >= MIN_PIVOT
            p += c
            A[rows, c], A[rows, p] = A[rows, p].copy(), A[rows, c].copy()
            b[rows, c], b[rows, p] = b[rows, p].copy(), b[rows, c].copy()
            for r in range(c + 1, N):
                m = A[:, r, c] / A[:, c, c]
                for j in range(c + 1, N):
                    A[:, r, j] = A[:, r, j] - m * A[:, c, j]
                b[:, r] = b[:, r] - m * b[:, c]
        h = np.zeros((H, 9))
        h[:, 8] = 1.0
        for i in range(N - 1, -1, -1):
            t = b[:, i].copy()
            for j in range(i + 1, N):
                t = t - A[:, i, j] * h[:, j]
            h[:, i] = t / A[:, i, i]
    return h, valid


def inliers(h, x, y, u, v, threshold):
    """(H, M) bool: correspondence m is an inlier of model h[k]."""
    T = np.float64(np.float32(threshold))
    h = h[:, :, None]
    with np.errstate(all="ignore"):
        P = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
        Q = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
        w = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
        rx = P - u * w
        ry = Q - v * w
        e = rx * rx + ry * ry
        lim = (T * T) * (w * w)
        return (w > 0) & (e <= lim)


def hypotheses(x, y, u, v, frame, model, n_hyp, seed):
    """((n_hyp, 9) models, (n_hyp,) valid) of a frame's correspondences."""
    s, M = sample_size(model), len(x)
    idx = np.zeros((n_hyp, s), dtype=np.int64)
    drawn = np.zeros(n_hyp, dtype=bool)
    for k in range(n_hyp):
        got, _ = sample(seed, frame, k, M, s)
        if got is not None:
            idx[k], drawn[k] = got, True
    if M == 0:
        return np.zeros((n_hyp, 9)), drawn
    h, valid = fit(x[idx], y[idx], u[idx], v[idx], model)
    return h, valid & drawn


def estimate(x, y, u, v, frame, model, n_hyp, threshold, seed):
    """(model record, (M,) inlier flags, (n_hyp,) counts with -1 for an invalid hypothesis)."""
    rec = np.zeros((), dtype=MODEL_DTYPE)
    rec["n_corr"], rec["hypothesis"] = len(x), NONE
    h, valid = hypotheses(x, y, u, v, frame, model, n_hyp, seed)
    counts = np.full(n_hyp, -1, dtype=np.int64)
    flags = np.zeros(len(x), dtype=bool)
    if valid.any():
        inl = inliers(h, x, y, u, v, threshold)
        counts = np.where(valid, inl.sum(axis=1), -1)
        best = int(counts.argmax())                       # the first maximum: the lowest h
        rec["h"], rec["n_inliers"], rec["hypothesis"] = h[best], counts[best], best
        rec["n_valid"] = valid.sum()
        flags = inl[best]
    return rec, flags, counts


def ransac(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, model, n_hyp,
           threshold, seed, inliers_out=None):
    """fdf_ransac_device: ((F,) model records, the inlier bytes: `inliers_out`'s fill outside
    [qo[0], min(qo[F], q_cap)))."""
    n_frames = len(q_offs) - 1
    models = np.zeros(n_frames, dtype=MODEL_DTYPE)
    out = np.zeros(q_cap, dtype=np.uint8) if inliers_out is None else inliers_out.copy()
    for f in range(n_frames):
        qb, qe = frame_range(q_offs, q_cap, f)
        i, x, y, u, v = correspondences(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap,
                                        t_offs, f)
        models[f], flags, _ = estimate(x, y, u, v, f, model, n_hyp, threshold, seed)
        out[qb:qe] = 0
        out[i[flags]] = 1
    return models, out


def models_equal(a, b):
    """Field-by-field ==, NaN equal to NaN, the sign of a zero free."""
    return bool(np.array_equal(a["h"], b["h"], equal_nan=True) and
                all(np.array_equal(a[k], b[k]) for k in ("n_corr", "n_inliers", "hypothesis",
                                                         "n_valid")))


def identity_matches(n):
    m = np.zeros(n, dtype=np.dtype([("index", "<u4"), ("distance", "<u2"), ("second", "<u2")]))
    m["index"] = np.arange(n)
    return m


def worked_example():
    """include/fdf.h's example: (q_coords, t_coords) as uint32."""
    q = np.array([(0, 0), (10, 0), (0, 10), (10, 10), (4, 7), (20, 3)], dtype=np.uint32)
    t = q + np.array([3, 5], dtype=np.uint32)
    t[4] = (50, 50)
    return q, t
