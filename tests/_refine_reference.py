"""A numpy restatement of include/fdf.h's least-squares refinement (fdf_refine_device),
independent of the kernel: the correspondences and the score are tests/_ransac_reference.py's, the
elimination is its `fit` loop restated for a given matrix (tests/test_refine.py holds the two
together bit for bit), every sum goes through ordered_sum and the denormalisation is written out
operation by operation on float64 scalars (numpy rounds every operation once and never fuses
two)."""
import numpy as np

import _ransac_reference as rr

LANES = 256
MAX_ROUNDS = 8
MIN_SCALE = 2.0 ** -20


def ordered_sum(terms):
    """The column sums of `terms` ((M,) or (M, K)) in the contract's order: term j goes to lane
    j mod 256, a lane adds its terms in increasing j from +0.0, and the lanes fold by halves."""
    a = np.asarray(terms, dtype=np.float64)
    cols = a.reshape(len(a), int(np.prod(a.shape[1:])))
    rows = -(-len(cols) // LANES)
    padded = np.zeros((rows * LANES, cols.shape[1]))
    padded[:len(cols)] = cols
    lane = np.zeros((LANES, cols.shape[1]))
    with np.errstate(all="ignore"):
        for r in range(rows):
            lane = lane + padded[r * LANES:(r + 1) * LANES]
        step = LANES // 2
        while step:
            lane = lane[:step] + lane[step:2 * step]
            step //= 2
    return lane[0].reshape(a.shape[1:])


def member_sum(flags, columns):
    """ordered_sum over the members of `flags`: the others add nothing (a +0.0)."""
    return ordered_sum(np.where(flags[:, None], np.stack(columns, axis=1), 0.0))


def solve(A, b):
    """_ransac_reference.fit's elimination and back substitution for given systems: A is
    (H, N, N), b is (H, N); returns ((H, 9) float64 with h8 = 1, (H,) valid)."""
    A, b = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64)
    H, N = b.shape
    rows = np.arange(H)
    valid = np.ones(H, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(N):
            mag = np.abs(A[:, c:, c])
            mag = np.where(np.isnan(mag), -1.0, mag)      # a NaN never wins
            p = mag.argmax(axis=1)                        # the first maximum: the lowest row
            valid &= mag[rows, p] >= rr.MIN_PIVOT
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


def normalisation(x, y, u, v, flags, model):
    """(cx, cy, s, cu, cv, t) of the members, or None when the round fails here."""
    one = np.ones(len(x))
    with np.errstate(all="ignore"):
        n, sx, sy, su, sv = member_sum(flags, [one, x, y, u, v])
        cx, cy, cu, cv = sx / n, sy / n, su / n, sv / n
        d, e = member_sum(flags, [np.abs(x - cx) + np.abs(y - cy), np.abs(u - cu) + np.abs(v - cv)])
        if not (n >= rr.sample_size(model) and 0 < d < np.inf and 0 < e < np.inf):
            return None
        return cx, cy, (n + n) / d, cu, cv, (n + n) / e


def normal_equations(x, y, u, v, flags, model, norm):
    """(G (N, N), g (N,)) of the members in normalised coordinates."""
    cx, cy, s, cu, cv, t = norm
    N = 2 * rr.sample_size(model)
    with np.errstate(all="ignore"):
        X, Y, U, V = (x - cx) * s, (y - cy) * s, (u - cu) * t, (v - cv) * t
        one = np.ones(len(x))
        r0 = [X, Y, one, None, None, None, -(U * X), -(U * Y)]       # None: a structural zero
        r1 = [None, None, None, X, Y, one, -(V * X), -(V * Y)]
        where, columns = [], []
        for i in range(N):
            for j in list(range(i, N)) + [N]:                        # column N: the right side
                other = (U, V) if j == N else (r0[j], r1[j])
                parts = [r[i] * o for r, o in zip((r0, r1), other) if r[i] is not None and o is not None]
                if parts:
                    where.append((i, j))
                    columns.append(parts[0] if len(parts) == 1 else parts[0] + parts[1])
        sums = member_sum(flags, columns)
    G, g = np.zeros((N, N)), np.zeros(N)
    for (i, j), value in zip(where, sums):
        if j == N:
            g[i] = value
        else:
            G[i, j] = G[j, i] = value
    return G, g


def denormalise(hn, norm, model):
    """The model of the normalised solution `hn` (9,), or None when the round fails here."""
    cx, cy, s, cu, cv, t = norm
    with np.errstate(all="ignore"):
        A = np.zeros((3, 3))
        for r in range(3):
            a0 = hn[3 * r] * s
            a1 = hn[3 * r + 1] * s
            A[r] = a0, a1, (hn[3 * r + 2] - a0 * cx) - a1 * cy
        h = np.zeros(9)
        h[8] = 1.0
        if model == rr.AFFINE:
            h[0], h[1], h[2] = A[0, 0] / t, A[0, 1] / t, A[0, 2] / t + cu
            h[3], h[4], h[5] = A[1, 0] / t, A[1, 1] / t, A[1, 2] / t + cv
        else:
            H = np.zeros(9)
            for c in range(3):
                H[c] = A[0, c] / t + cu * A[2, c]
                H[3 + c] = A[1, c] / t + cv * A[2, c]
                H[6 + c] = A[2, c]
            if not MIN_SCALE <= abs(H[8]) < np.inf:
                return None
            h[:8] = H[:8] / H[8]
    return h if np.isfinite(h).all() else None


def refit(x, y, u, v, flags, model):
    """One round's model over the members `flags`, or None: the round failed."""
    norm = normalisation(x, y, u, v, flags, model)
    if norm is None:
        return None
    G, g = normal_equations(x, y, u, v, flags, model, norm)
    hn, valid = solve(G[None], g[None])
    return denormalise(hn[0], norm, model) if valid[0] else None


def refine_frame(x, y, u, v, rec_in, model, threshold, n_rounds):
    """(the refined record, the (M,) member flags, the rounds accepted) of one frame."""
    rec = rec_in.copy()
    if rec["hypothesis"] == rr.NONE:
        return rec, np.zeros(len(x), dtype=bool), 0
    h = np.array(rec["h"], dtype=np.float64)
    flags = rr.inliers(h[None], x, y, u, v, threshold)[0] if len(x) else np.zeros(0, dtype=bool)
    rounds = 0
    for _ in range(n_rounds):
        h2 = refit(x, y, u, v, flags, model)
        if h2 is None:
            break
        flags2 = rr.inliers(h2[None], x, y, u, v, threshold)[0]
        if flags2.sum() < flags.sum():
            break
        h, flags, rounds = h2, flags2, rounds + 1
    rec["h"], rec["n_corr"], rec["n_inliers"] = h, len(x), flags.sum()
    return rec, flags, rounds


def refine(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, model, models_in,
           threshold, n_rounds, inliers_out=None):
    """fdf_refine_device: ((F,) model records, the inlier bytes: `inliers_out`'s fill outside
    [qo[0], min(qo[F], q_cap)), the (F,) accepted rounds)."""
    n_frames = len(q_offs) - 1
    models = np.zeros(n_frames, dtype=rr.MODEL_DTYPE)
    rounds = np.zeros(n_frames, dtype=np.uint32)
    out = np.zeros(q_cap, dtype=np.uint8) if inliers_out is None else inliers_out.copy()
    for f in range(n_frames):
        qb, qe = rr.frame_range(q_offs, q_cap, f)
        i, x, y, u, v = rr.correspondences(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap,
                                           t_offs, f)
        models[f], flags, rounds[f] = refine_frame(x, y, u, v, models_in[f], model, threshold,
                                                   n_rounds)
        out[qb:qe] = 0
        out[i[flags]] = 1
    return models, out, rounds


def model_record(h, n_corr=0, n_inliers=0, hypothesis=0, n_valid=1):
    """A model record to refine."""
    rec = np.zeros((), dtype=rr.MODEL_DTYPE)
    rec["h"] = np.asarray(h, dtype=np.float64).reshape(9)
    rec["n_corr"], rec["n_inliers"], rec["hypothesis"], rec["n_valid"] = (n_corr, n_inliers,
                                                                         hypothesis, n_valid)
    return rec
