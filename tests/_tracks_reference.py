"""Numpy restatement of include/fdf.h's track-set maintenance (fdf_tracks_update_device), rule by
rule over brute-force pair matrices, and a sequential greedy selection that is used only to check
that the passes converge to it."""
import numpy as np

import _brief_reference as br
import _resize_reference as rs

ONE = 2048
UNDECIDED, ADMITTED, REJECTED = 0, 1, 2
NEW = 0x80000000


def texture(seed, w, h):
    """A smooth random frame: a coarse random grid resized and box-smoothed (the library's rules)."""
    small = np.random.default_rng(seed).integers(0, 256, (max(h // 8, 2), max(w // 8, 2)))
    return br.smooth(rs.resize(small.astype(np.uint8), w, h))


def moved(big, w, h, shifts, margin=16):
    """Crops of `big` whose content moves by each of `shifts` = [(sx, sy)] from the first crop."""
    return np.stack([big[margin - sy:margin - sy + h, margin - sx:margin - sx + w]
                     for sx, sy in [(0, 0)] + list(shifts)])


def frame_range(offs, cap, f):
    b = min(int(offs[f]), cap)
    return b, max(min(int(offs[f + 1]), cap), b)


def alive_tracks(q11, status, width, height, margin):
    """Rule 1 for tracks -> a boolean mask."""
    q = np.asarray(q11, dtype=np.int64).reshape(-1, 2)
    ok = np.ones(len(q), bool) if status is None else np.asarray(status) != 0
    return (ok & (q[:, 0] >= margin * ONE) & (q[:, 0] <= (width - 1 - margin) * ONE) &
            (q[:, 1] >= margin * ONE) & (q[:, 1] <= (height - 1 - margin) * ONE))


def eligible_candidates(pts, width, height, margin):
    """Rule 1 for candidates -> a boolean mask."""
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    return ((p[:, 0] >= margin) & (p[:, 0] <= width - 1 - margin) &
            (p[:, 1] >= margin) & (p[:, 1] <= height - 1 - margin))


def track_pixels(q11):
    """Rule 2: the pixel of a Q11 position."""
    return (np.asarray(q11, dtype=np.int64).reshape(-1, 2) + 1024) >> 11


def near_matrix(a, b, min_dist):
    """near[i, j]: point i of `a` and point j of `b` are closer than min_dist (strict)."""
    a = np.asarray(a, dtype=np.int32).reshape(-1, 2)
    b = np.asarray(b, dtype=np.int32).reshape(-1, 2)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    return dx * dx + dy * dy < min_dist * min_dist


def dominators(xy, key, min_dist):
    """dom[i, j]: j dominates i (near, larger key or the same key and a lower index)."""
    key = np.asarray(key, dtype=np.int64)
    idx = np.arange(len(key))
    higher = (key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) &
                                              (idx[None, :] < idx[:, None]))
    return near_matrix(xy, xy, min_dist) & higher


def suppress(xy, key, state, min_dist, passes):
    """Rule 3: `passes` passes from the initial `state`; every pass reads the one before only."""
    state = np.array(state, dtype=np.uint8)
    dom = dominators(xy, key, min_dist)
    for _ in range(passes):
        any_adm = (dom & (state == ADMITTED)[None, :]).any(axis=1)
        any_und = (dom & (state == UNDECIDED)[None, :]).any(axis=1)
        fresh = np.where(any_adm, REJECTED, np.where(any_und, UNDECIDED, ADMITTED)).astype(np.uint8)
        state = np.where(state == UNDECIDED, fresh, state)
    return state


def greedy(xy, key, state, min_dist):
    """The sequential selection the passes converge to: the initially undecided points in
    priority order, each admitted unless an admitted point is near -> the final states."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    key = np.asarray(key, dtype=np.int64)
    out = np.array(state, dtype=np.uint8)
    todo = np.flatnonzero(out == UNDECIDED)
    order = todo[np.lexsort((todo, -key[todo]))]
    kept = []
    d2 = min_dist * min_dist
    for i in order:
        hit = any((xy[i, 0] - xy[j, 0]) ** 2 + (xy[i, 1] - xy[j, 1]) ** 2 < d2 for j in kept)
        out[i] = REJECTED if hit else ADMITTED
        if not hit:
            kept.append(i)
    return out


def update_stream(q11, status, ids, ages, cand, scores, next_id, width, height, min_dist, margin,
                  max_tracks, passes):
    """Rules 1-6 for one stream.  Returns (q11, ids, ages, kept, new, next_id): `kept` and `new` are
    the survivors' track indices and the new tracks' candidate indices, local to the stream."""
    q11 = np.asarray(q11, dtype=np.int64).reshape(-1, 2)
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    ids = np.asarray(ids, dtype=np.uint32)
    ages = np.asarray(ages, dtype=np.uint32)
    scores = np.asarray(scores, dtype=np.uint16)
    # rule 4
    pix = track_pixels(q11)
    state = np.where(alive_tracks(q11, status, width, height, margin), UNDECIDED, REJECTED)
    kept = np.flatnonzero(suppress(pix, ages, state, min_dist, passes) == ADMITTED)
    # rule 5
    blocked = near_matrix(cand, pix[kept], min_dist).any(axis=1)
    state = np.where(eligible_candidates(cand, width, height, margin) & ~blocked, UNDECIDED, REJECTED)
    adm = np.flatnonzero(suppress(cand, scores, state, min_dist, passes) == ADMITTED)
    room = max(0, max_tracks - len(kept))
    ranked = adm[np.lexsort((adm, -scores[adm].astype(np.int64)))]
    new = np.sort(ranked[:room])
    # rule 6
    out_q = np.concatenate([q11[kept], cand[new] * ONE]).astype(np.int32).reshape(-1, 2)
    out_ids = np.concatenate([ids[kept].astype(np.int64),
                              (int(next_id) + np.arange(len(new), dtype=np.int64)) & 0xFFFFFFFF])
    out_ages = np.concatenate([np.minimum(ages[kept].astype(np.int64) + 1, 0xFFFFFFFF),
                               np.zeros(len(new), np.int64)])
    return (out_q, out_ids.astype(np.uint32), out_ages.astype(np.uint32), kept, new,
            (int(next_id) + len(new)) & 0xFFFFFFFF)


def update(q11, status, ids, ages, t_offs, t_cap, cand, scores, c_offs, c_cap, next_id, width,
           height, min_dist, margin, max_tracks, passes):
    """The whole call over every stream.  Returns a dict: q11 (N, 2) int32, ids, ages, src (N,)
    uint32 of all N output entries (the caller cuts at out_cap), offsets (F + 1,) uint64 and the
    advanced next_id (F,) uint32."""
    n_frames = len(t_offs) - 1
    q11 = np.asarray(q11).reshape(-1, 2)
    cand = np.asarray(cand).reshape(-1, 2)
    parts = {"q11": [], "ids": [], "ages": [], "src": []}
    offsets = [0]
    nid = np.array(next_id, dtype=np.uint32).reshape(-1).copy()
    for f in range(n_frames):
        tb, te = frame_range(t_offs, t_cap, f)
        cb, ce = frame_range(c_offs, c_cap, f)
        st = None if status is None else np.asarray(status)[tb:te]
        q, i, a, kept, new, nxt = update_stream(
            q11[tb:te], st, np.asarray(ids)[tb:te], np.asarray(ages)[tb:te], cand[cb:ce],
            np.asarray(scores)[cb:ce], nid[f], width, height, min_dist, margin, max_tracks, passes)
        parts["q11"].append(q)
        parts["ids"].append(i)
        parts["ages"].append(a)
        parts["src"].append(np.concatenate([kept + tb, (new + cb) | NEW]).astype(np.uint32))
        offsets.append(offsets[-1] + len(i))
        nid[f] = nxt
    out = {k: (np.concatenate(v) if v else np.zeros((0, 2) if k == "q11" else 0)) for k, v in parts.items()}
    out["q11"] = out["q11"].astype(np.int32).reshape(-1, 2)
    for k in ("ids", "ages", "src"):
        out[k] = out[k].astype(np.uint32)
    out["offsets"] = np.array(offsets, dtype=np.uint64)
    out["next_id"] = nid
    return out


def header_example():
    """The worked example of include/fdf.h -> (arguments of update_stream, the expected output)."""
    args = dict(q11=[[20480, 20480], [15359, 28672], [22528, 20480], [-1, -1]], status=[1, 1, 1, 0],
                ids=[3, 4, 5, 6], ages=[5, 2, 9, 1],
                cand=[[12, 10], [20, 10], [23, 14], [21, 11], [1, 12], [28, 20]],
                scores=[90, 50, 50, 40, 99, 10], next_id=7, width=32, height=24, min_dist=5,
                margin=2, max_tracks=4, passes=8)
    want = dict(q11=[[15359, 28672], [22528, 20480], [40960, 20480], [47104, 28672]],
                ids=[4, 5, 7, 8], ages=[3, 10, 0, 0], src=[1, 2, NEW | 1, NEW | 2], next_id=9)
    return args, want
