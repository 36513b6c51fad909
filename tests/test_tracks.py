"""Track-set maintenance on the CPU: the numpy restatement of include/fdf.h's rules
(tests/_tracks_reference.py) against the sequential greedy selection it must converge to, the
invariants of a call's output, the header's worked example, the host-only scratch size export and
the export list.  The device is compared with the restatement in tests/test_gpu_tracks.py."""
import ctypes

import numpy as np
import pytest

import _tracks_reference as ts
from feature_detector_fast_amd import _native, fast_hip
from oracle import oracle

NAMES = ("fdf_tracks_scratch_bytes", "fdf_tracks_update_device", "fdf_tracks_update_points")


def texture_corners(t):
    """FAST-9 corners (no NMS) of the 208 x 144 texture crop at threshold t with their scores."""
    img = np.ascontiguousarray(ts.moved(ts.texture(5, 256, 192), 208, 144, [])[0])
    pts = oracle.detect(img, t, 9, 0)
    return pts.astype(np.int64), oracle.score_points(img, pts, 1, t, 9)


def random_points(seed=3, n=600, w=64, h=48, top=4):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
    return pts, rng.integers(0, top, n).astype(np.uint16)


def undecided(n):
    return np.zeros(n, np.uint8)


@pytest.mark.parametrize("t", [4, 12])
@pytest.mark.parametrize("min_dist", [4, 8, 16])
def test_passes_converge_to_greedy_on_a_texture(t, min_dist):
    pts, scores = texture_corners(t)
    assert len(pts) > 100
    got = ts.suppress(pts, scores, undecided(len(pts)), min_dist, 32)
    assert np.array_equal(got, ts.greedy(pts, scores, undecided(len(pts)), min_dist))
    assert (got != ts.UNDECIDED).all() and (got == ts.ADMITTED).any() and (got == ts.REJECTED).any()


@pytest.mark.parametrize("min_dist", [2, 3, 5, 9])
def test_passes_converge_to_greedy_on_random_points(min_dist):
    pts, scores = random_points()
    got = ts.suppress(pts, scores, undecided(len(pts)), min_dist, 32)
    assert np.array_equal(got, ts.greedy(pts, scores, undecided(len(pts)), min_dist))


def test_initially_rejected_points_take_no_part():
    pts, scores = random_points(seed=5)
    start = (np.arange(len(pts)) % 3 == 0).astype(np.uint8) * ts.REJECTED
    got = ts.suppress(pts, scores, start, 5, 32)
    assert np.array_equal(got, ts.greedy(pts, scores, start, 5))
    live = start == ts.UNDECIDED
    alone = ts.suppress(pts[live], scores[live], undecided(live.sum()), 5, 32)
    assert np.array_equal(got[live], alone) and (got[~live] == ts.REJECTED).all()


def test_pass_one_admits_the_local_maxima_and_sets_grow():
    pts, scores = random_points(seed=7)
    dom = ts.dominators(pts, scores, 5)
    first = ts.suppress(pts, scores, undecided(len(pts)), 5, 1)
    assert np.array_equal(first == ts.ADMITTED, ~dom.any(axis=1))
    assert not (first == ts.REJECTED).any()
    before = first
    for passes in range(2, 12):
        after = ts.suppress(pts, scores, undecided(len(pts)), 5, passes)
        decided = before != ts.UNDECIDED
        assert np.array_equal(after[decided], before[decided])      # decisions are final
        before = after
    assert (before != ts.UNDECIDED).all()


def test_strict_distance():
    pts = np.array([[10, 10], [13, 14]])
    for min_dist, near in ((5, False), (6, True)):
        assert ts.near_matrix(pts, pts, min_dist)[0, 1] == near


def test_the_headers_worked_example():
    args, want = ts.header_example()
    q, ids, ages, kept, new, nxt = ts.update_stream(**args)
    assert q.tolist() == want["q11"] and ids.tolist() == want["ids"]
    assert ages.tolist() == want["ages"] and nxt == want["next_id"]
    assert np.concatenate([kept, new | ts.NEW]).tolist() == want["src"]
    assert ts.track_pixels([[15359, 28672], [15360, 28672]])[:, 0].tolist() == [7, 8]
    one_pass = ts.update_stream(**dict(args, passes=1))
    assert one_pass[0].tolist() == want["q11"]                     # the dropped are the rejected here


def scene(seed, w=64, h=48, n_t=80, n_c=600, margin=3):
    rng = np.random.default_rng(seed)
    q11 = np.stack([rng.integers(0, w * ts.ONE, n_t), rng.integers(0, h * ts.ONE, n_t)], axis=1)
    lost = rng.random(n_t) < 0.1
    q11[lost] = -1
    status = (~lost & (rng.random(n_t) < 0.9)).astype(np.uint8)
    ids = rng.permutation(1000)[:n_t].astype(np.uint32)
    ages = rng.integers(0, 4, n_t).astype(np.uint32)
    cand, scores = random_points(seed + 100, n_c, w, h)
    return dict(q11=q11, status=status, ids=ids, ages=ages, cand=cand, scores=scores, next_id=1000,
                width=w, height=h, margin=margin)


@pytest.mark.parametrize("min_dist,max_tracks,passes", [(3, 1000, 32), (5, 60, 32), (9, 1000, 2),
                                                        (5, 10, 8)])
def test_output_invariants(min_dist, max_tracks, passes):
    s = scene(11)
    q, ids, ages, kept, new, nxt = ts.update_stream(**s, min_dist=min_dist, max_tracks=max_tracks,
                                                    passes=passes)
    pix = ts.track_pixels(q)
    near = ts.near_matrix(pix, pix, min_dist)
    np.fill_diagonal(near, False)
    assert not near.any()                       # survivors and new tracks alike keep their distance
    assert len(set(ids.tolist())) == len(ids)
    assert len(new) == max(0, min(len(new), max_tracks - len(kept))) and nxt == 1000 + len(new)
    assert np.array_equal(ages[:len(kept)], s["ages"][kept] + 1) and (ages[len(kept):] == 0).all()
    assert np.array_equal(ids[:len(kept)], s["ids"][kept])
    assert ids[len(kept):].tolist() == list(range(1000, 1000 + len(new)))
    assert np.array_equal(q[:len(kept)], s["q11"][kept])
    assert np.array_equal(q[len(kept):], s["cand"][new] * ts.ONE)
    assert (np.diff(kept) > 0).all() and (np.diff(new) > 0).all()
    assert ts.alive_tracks(s["q11"], s["status"], 64, 48, 3)[kept].all()
    assert ts.eligible_candidates(s["cand"], 64, 48, 3)[new].all()
    if max_tracks >= len(kept) + 1000:          # no budget cut: survivors first, then the greedy set
        assert len(kept) > 10 and len(new) > 10


def test_the_budget_takes_the_strongest_and_never_drops_a_survivor():
    s = scene(13)
    full = ts.update_stream(**s, min_dist=5, max_tracks=10000, passes=32)
    kept, new = full[3], full[4]
    cut = ts.update_stream(**s, min_dist=5, max_tracks=len(kept) + 7, passes=32)
    assert np.array_equal(cut[3], kept) and len(cut[4]) == 7
    order = new[np.lexsort((new, -s["scores"][new].astype(np.int64)))]
    assert np.array_equal(cut[4], np.sort(order[:7]))
    none = ts.update_stream(**s, min_dist=5, max_tracks=max(len(kept) - 3, 1), passes=32)
    assert np.array_equal(none[3], kept) and len(none[4]) == 0 and none[5] == 1000


def scratch_bytes(*args):
    v = ctypes.c_uint64(0xABCD)
    return _native.load().fdf_tracks_scratch_bytes(*args, ctypes.byref(v)), v.value


def test_scratch_bytes_export():
    rc, small = scratch_bytes(1, 64, 48, 5, 80, 600)
    assert rc == _native.FDF_OK and small > 0 and small % 256 == 0
    rc, more = scratch_bytes(4, 64, 48, 5, 80, 600)
    assert rc == _native.FDF_OK and more > small
    assert scratch_bytes(1, 64, 48, 5, 80, 6000)[1] > small
    assert scratch_bytes(0, 64, 48, 5, 80, 600) == (_native.FDF_OK, 0)
    assert fast_hip.tracks_scratch_bytes(1, (48, 64), 5, 80, 600) == small
    for bad in ((1, 0, 48, 5, 80, 600), (1, 64, 0, 5, 80, 600), (1, 65536, 48, 5, 80, 600),
                (1, 64, 65536, 5, 80, 600), (1, 64, 48, 0, 80, 600), (1, 64, 48, 256, 80, 600),
                (65536, 64, 48, 5, 80, 600), (1, 64, 48, 5, 1 << 32, 600),
                (1, 64, 48, 5, 80, 1 << 32)):
        assert scratch_bytes(*bad) == (_native.FDF_ERR_ARG, 0xABCD), bad
    assert _native.load().fdf_tracks_scratch_bytes(1, 64, 48, 5, 80, 600, None) == _native.FDF_ERR_ARG


def test_names_are_exported():
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(_native.load(), name)
    for name in ("TRACKS_NEW", "tracks_scratch_bytes", "tracks_update_device", "update_tracks",
                 "track_sequence_array"):
        assert name in fast_hip.__all__ and hasattr(fast_hip, name)
    assert fast_hip.TRACKS_NEW == ts.NEW
    assert ctypes.sizeof(_native.FdfTracksParams) == 24


def test_python_argument_checks_need_no_device():
    for kw in (dict(min_dist=0), dict(min_dist=256), dict(margin=24), dict(max_tracks=0),
               dict(passes=0), dict(passes=33)):
        with pytest.raises(ValueError):
            fast_hip.update_tracks((48, 64), np.zeros((0, 2)), [], [], np.zeros((0, 2), np.uint32),
                                   [], **kw)
