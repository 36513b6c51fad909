"""A numpy restatement of include/fdf.h's descriptor matching (fdf_match_device,
fdf_match_filter_device), independent of the kernels: byte-wise XOR, a 256-entry popcount
table, a per-frame loop, the window, the (distance, index) tie rule, `second`, and the filter."""
import numpy as np

NONE = 0xFFFFFFFF
NO_DISTANCE = 0xFFFF
MATCH_DTYPE = np.dtype([("index", "<u4"), ("distance", "<u2"), ("second", "<u2")])
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)
_FAR = 1 << 20                                    # above any distance: not a candidate


def distances(q, t):
    """(n_q, n_t) Hamming distances of (n_q, 32) and (n_t, 32) uint8 descriptors."""
    q = np.asarray(q, dtype=np.uint8).reshape(-1, 32)
    t = np.asarray(t, dtype=np.uint8).reshape(-1, 32)
    return POPCOUNT[q[:, None, :] ^ t[None, :, :]].sum(axis=2)


def frame_range(offs, cap, f):
    b = min(int(offs[f]), int(cap))
    e = max(min(int(offs[f + 1]), int(cap)), b)
    return b, e


def match_pair(q, t, q_pts=None, t_pts=None, window=None, base=0):
    """The (n_q,) match records of one frame pair; indices are `base` + the train row."""
    out = np.zeros(len(q), dtype=MATCH_DTYPE)
    out["index"], out["distance"], out["second"] = NONE, NO_DISTANCE, NO_DISTANCE
    if len(q) == 0 or len(t) == 0:
        return out
    d = distances(q, t)
    if q_pts is not None:
        qp, tp = np.asarray(q_pts, dtype=np.int64), np.asarray(t_pts, dtype=np.int64)
        near = (np.abs(qp[:, None, 0] - tp[None, :, 0]) <= int(window[0])) & \
               (np.abs(qp[:, None, 1] - tp[None, :, 1]) <= int(window[1]))
        d = np.where(near, d, _FAR)
    rows = np.arange(len(q))
    first = d.argmin(axis=1)                      # the first minimum: the lowest index
    best = d[rows, first]
    d[rows, first] = _FAR
    second = d.min(axis=1)
    hit = best < _FAR
    out["index"][hit] = (first + base)[hit]
    out["distance"][hit] = best[hit]
    out["second"][hit & (second < _FAR)] = second[hit & (second < _FAR)]
    return out


def match(q_desc, q_offs, q_cap, t_desc, t_offs, t_cap, q_pts=None, t_pts=None, window=None,
          out=None):
    """fdf_match_device: `out` ((>= q_cap,) records, the caller's fill elsewhere) with the
    frames' entries written."""
    out = np.zeros(q_cap, dtype=MATCH_DTYPE) if out is None else out.copy()
    for f in range(len(q_offs) - 1):
        qb, qe = frame_range(q_offs, q_cap, f)
        tb, te = frame_range(t_offs, t_cap, f)
        out[qb:qe] = match_pair(q_desc[qb:qe], t_desc[tb:te],
                                None if q_pts is None else q_pts[qb:qe],
                                None if t_pts is None else t_pts[tb:te], window, base=tb)
    return out


def match_filter(matches, q_offs, q_cap, reverse=None, t_cap=0, max_distance=256, ratio=None,
                 out=None):
    """fdf_match_filter_device: the keep flags of [qo[0], min(qo[F], q_cap)), the caller's
    fill elsewhere."""
    out = np.zeros(q_cap, dtype=np.uint8) if out is None else out.copy()
    lo, hi = min(int(q_offs[0]), q_cap), min(int(q_offs[-1]), q_cap)
    for i in range(lo, hi):
        index, dist, second = (int(matches[i][k]) for k in ("index", "distance", "second"))
        keep = index != NONE
        if max_distance < 256:
            keep = keep and dist <= max_distance
        if ratio is not None and ratio[1] != 0 and second != NO_DISTANCE:
            keep = keep and dist * ratio[1] < second * ratio[0]
        if reverse is not None:
            keep = keep and index < t_cap and int(reverse[index]["index"]) == i
        out[i] = 1 if keep else 0
    return out


def as_records(array):
    """An (n, 2) 32-bit integer array (the device layout) as (n,) records."""
    return np.ascontiguousarray(array).view(MATCH_DTYPE).reshape(-1)
