"""Track-set maintenance on the device (fdf_tracks_update_device, fdf_tracks_update_points,
track_sequence_array) against the numpy restatement of include/fdf.h's rules in
tests/_tracks_reference.py.  Every comparison is bit for bit; every run also proves that the
inputs are intact, that output entries at or past min(total, out_cap) keep their fill and that a
second identical call gives identical bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _resize_reference as rs
import _track_reference as tr
import _tracks_reference as ts
from feature_detector_fast_amd import Config, FdfError, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 0xEE
TAIL = 3                                        # rows past out_cap in every output
OUTPUTS = ("q11", "ids", "ages", "src")


def gap_tensor(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(GAP)
    return t


def dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def run_update(q11, ids, ages, t_offs, cand, scores, c_offs, next_id, shape, status=None,
               t_cap=None, c_cap=None, out_cap=None, src=True, **values):
    """fdf_tracks_update_device on uploaded arrays against the restatement, bit for bit, with the
    checks of the module's docstring.  Returns the reference's dict."""
    import torch

    q11 = np.asarray(q11, dtype=np.int64).reshape(-1, 2)
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    t_cap = len(q11) if t_cap is None else t_cap
    c_cap = len(cand) if c_cap is None else c_cap
    h, w = shape
    want = ts.update(q11, status, ids, ages, t_offs, t_cap, cand, scores, c_offs, c_cap, next_id,
                     w, h, values["min_dist"], values["margin"], values["max_tracks"],
                     values["passes"])
    total = int(want["offsets"][-1])
    out_cap = total if out_cap is None else out_cap
    n = len(t_offs) - 1

    d = {"q11": dev(torch, q11, np.int32), "ids": dev(torch, ids, np.uint32).view(torch.int32),
         "ages": dev(torch, ages, np.uint32).view(torch.int32),
         "t_offs": dev(torch, t_offs, np.int64), "cand": dev(torch, cand, np.uint32).view(torch.int32),
         "scores": dev(torch, scores, np.uint16).view(torch.int16),
         "c_offs": dev(torch, c_offs, np.int64)}
    if status is not None:
        d["status"] = dev(torch, status, np.uint8)
    kept = {k: v.clone() for k, v in d.items()}
    first_id = dev(torch, np.asarray(next_id, dtype=np.uint32).reshape(-1), np.uint32).view(torch.int32)
    rows = out_cap + TAIL
    runs = []
    for _ in range(2):
        out = {"q11": gap_tensor(torch, (rows, 2), torch.int32),
               "ids": gap_tensor(torch, (rows,), torch.int32),
               "ages": gap_tensor(torch, (rows,), torch.int32),
               "src": gap_tensor(torch, (rows,), torch.int32),
               "offsets": gap_tensor(torch, (n + 1 + TAIL,), torch.int64)}
        nid = first_id.clone()
        # the tensors hold `rows` rows, the call is told of out_cap: slices share the memory
        fast_hip.tracks_update_device(
            d["q11"][:t_cap], d["ids"][:t_cap], d["ages"][:t_cap], d["t_offs"], d["cand"][:c_cap],
            d["scores"][:c_cap], d["c_offs"], nid, out["q11"][:out_cap], out["ids"][:out_cap],
            out["ages"][:out_cap], out["offsets"][:n + 1], shape,
            track_status=None if status is None else d["status"][:t_cap],
            out_src=out["src"][:out_cap] if src else None, **values)
        torch.cuda.synchronize()
        out["next_id"] = nid
        runs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k, v in d.items():
        assert torch.equal(v, kept[k]), k
    got, again = runs
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k

    assert np.array_equal(got["offsets"][:n + 1].view(np.uint64), want["offsets"])
    assert (got["offsets"][n + 1:].view(np.uint8) == GAP).all()
    assert np.array_equal(got["next_id"].view(np.uint32), want["next_id"])
    cut = min(total, out_cap)
    for name in OUTPUTS:
        raw = got[name].view(np.uint8).reshape(rows, -1)
        if name == "src" and not src:
            assert (raw == GAP).all()
            continue
        assert (raw[cut:] == GAP).all(), name
        exp = want[name][:cut]
        assert got[name][:cut].view(exp.dtype).tobytes() == exp.tobytes(), name
    return want


def random_scene(seed, w, h, n_t, n_c, top=4, margin=3):
    rng = np.random.default_rng(seed)
    q11 = np.stack([rng.integers(0, w * ts.ONE, n_t), rng.integers(0, h * ts.ONE, n_t)], axis=1)
    lost = rng.random(n_t) < 0.1
    q11[lost] = -1
    status = (~lost & (rng.random(n_t) < 0.9)).astype(np.uint8)
    return dict(q11=q11, status=status, ids=rng.permutation(1 << 20)[:n_t],
                ages=rng.integers(0, top, n_t),
                cand=np.stack([rng.integers(0, w, n_c), rng.integers(0, h, n_c)], axis=1),
                scores=rng.integers(0, top, n_c))


def one_stream(s, next_id=1000):
    return dict(q11=s["q11"], ids=s["ids"], ages=s["ages"], t_offs=[0, len(s["q11"])],
                cand=s["cand"], scores=s["scores"], c_offs=[0, len(s["cand"])], next_id=[next_id],
                status=s["status"])


# ---- 1: random points: cell sizes, one cell, truncated passes -----------------------------------

@pytest.fixture(scope="module")
def random_64x48():
    return random_scene(21, 64, 48, 80, 600)


@pytest.mark.parametrize("min_dist", [1, 2, 3, 5, 9, 64])
@pytest.mark.parametrize("passes", [1, 2, 7, 32])
def test_random(random_64x48, min_dist, passes):
    """min_dist 64 puts the whole 64 x 48 frame into one cell; below 8 the cell stays 8 wide."""
    want = run_update(**one_stream(random_64x48), shape=(48, 64), min_dist=min_dist, margin=3,
                      max_tracks=10000, passes=passes)
    assert int(want["offsets"][-1]) > 0
    if min_dist in (3, 5) and passes == 32:
        assert ((want["src"] & ts.NEW) != 0).sum() > 10 and ((want["src"] & ts.NEW) == 0).sum() > 10


@pytest.mark.parametrize("passes", [3, 32])
def test_dense_chain(passes):
    """Every pixel a candidate with one score: priority is the raster index, the dependency chain
    runs along the rows and the undecided points of a truncated run are dropped."""
    w, h = 40, 30
    ys, xs = np.mgrid[0:h, 0:w]
    cand = np.stack([xs.ravel(), ys.ravel()], axis=1)
    scores = np.full(len(cand), 7)
    full = ts.suppress(cand, scores, np.zeros(len(cand), np.uint8), 3, passes)
    assert (full == ts.UNDECIDED).any()              # the chain is longer than 32 passes
    assert (full == ts.ADMITTED).sum() == {3: 3, 32: 112}[passes]
    want = run_update(np.zeros((0, 2)), [], [], [0, 0], cand, scores, [0, len(cand)], [5], (h, w),
                      min_dist=3, margin=0, max_tracks=10000, passes=passes)
    assert int(want["offsets"][-1]) == (full == ts.ADMITTED).sum()


# ---- 2: several streams, offsets past the capacities, a short output ----------------------------

def test_multi_stream():
    """Five streams of unequal counts: stream 1 has no tracks, stream 2 no candidates, stream 3
    neither; the last stream's offsets run past t_cap and c_cap; out_cap is below the total and the
    totals are still reported in full."""
    s = random_scene(22, 64, 48, 200, 900)
    t_offs = [0, 70, 70, 110, 110, 230]
    c_offs = [0, 300, 520, 520, 520, 1000]
    want = run_update(s["q11"], s["ids"], s["ages"], t_offs, s["cand"], s["scores"], c_offs,
                      [10, 20, 30, 40, 0xFFFFFF00], (48, 64), status=s["status"], t_cap=190,
                      c_cap=880, out_cap=150, min_dist=5, margin=3, max_tracks=10000, passes=32)
    per = np.diff(want["offsets"].astype(np.int64))
    assert per[3] == 0 and (per[[0, 1, 2, 4]] > 0).all() and per.sum() > 150
    assert want["next_id"][3] == 40 and want["next_id"][2] == 30 and want["next_id"][1] > 20
    full = run_update(s["q11"], s["ids"], s["ages"], t_offs, s["cand"], s["scores"], c_offs,
                      [10, 20, 30, 40, 0xFFFFFF00], (48, 64), status=s["status"], t_cap=190,
                      c_cap=880, min_dist=5, margin=3, max_tracks=12, passes=8, src=False)
    assert int(full["offsets"][-1]) < per.sum()


def test_out_cap_zero_and_empty_lists():
    s = random_scene(23, 64, 48, 30, 100)
    run_update(**one_stream(s), shape=(48, 64), out_cap=0, min_dist=5, margin=3, max_tracks=100,
               passes=8)
    run_update(np.zeros((0, 2)), [], [], [0, 0], np.zeros((0, 2)), [], [0, 0], [9], (48, 64),
               min_dist=5, margin=3, max_tracks=100, passes=8)


# ---- 3: boundaries ------------------------------------------------------------------------------

def test_distance_boundaries_across_cells():
    """Pairs at distance^2 exactly min_dist^2 (not near) and a little less (near), across a cell
    edge in x, in y and across the corner of the 3 x 3 neighbourhood both ways; cells are 10 pixels
    wide and the pairs lie 24 pixels or more from each other."""
    pairs = [((19, 15), (29, 15), False),       # (10, 0): 100
             ((59, 15), (68, 15), True),        # (9, 0): 81
             ((95, 19), (95, 29), False),       # (0, 10)
             ((135, 19), (135, 28), True),      # (0, 9)
             ((19, 59), (25, 67), False),       # (6, 8): 100, cells (1, 5) and (2, 6)
             ((59, 59), (66, 66), True),        # (7, 7): 98, cells (5, 5) and (6, 6)
             ((99, 59), (107, 65), False),      # (8, 6): 100
             ((140, 59), (133, 65), True)]      # (-7, 6): 85, cells (14, 5) and (13, 6)
    n = len(pairs)
    cand = np.array([p[0] for p in pairs] + [p[1] for p in pairs])
    scores = np.concatenate([np.full(n, 9), np.full(n, 5)])
    want = run_update(np.zeros((0, 2)), [], [], [0, 0], cand, scores, [0, 2 * n], [0], (120, 200),
                      min_dist=10, margin=0, max_tracks=100, passes=4)
    new = set((want["src"] & 0x7FFFFFFF).tolist())
    assert new == set(range(n)) | {n + k for k in range(n) if not pairs[k][2]}
    # the same points as tracks (ages as priorities), and as survivors against candidates
    old = run_update(cand * ts.ONE, np.arange(2 * n), scores, [0, 2 * n], np.zeros((0, 2)), [],
                     [0, 0], [0], (120, 200), min_dist=10, margin=0, max_tracks=100, passes=4)
    assert set(old["src"].tolist()) == new
    both = run_update(cand[:n] * ts.ONE, np.arange(n), np.zeros(n), [0, n], cand[n:], scores[n:],
                      [0, n], [0], (120, 200), min_dist=10, margin=0, max_tracks=100, passes=4)
    assert set(both["src"].tolist()) == set(range(n)) | {ts.NEW | k for k in range(n) if not pairs[k][2]}


def test_rounding_and_margin_boundaries():
    """X = 2048 x + 1023 rounds to pixel x, + 1024 to x + 1: near or not near a candidate; tracks
    and candidates at margin and margin - 1; X = (w - 1 - margin) * 2048 and one unit more."""
    w, h, m = 64, 48, 4
    q11 = np.array([[2048 * 20 + 1023, 2048 * 20], [2048 * 40 + 1024, 2048 * 20],
                    [m * 2048, m * 2048], [m * 2048 - 1, 2048 * 30], [2048 * 30, m * 2048 - 1],
                    [(w - 1 - m) * 2048, (h - 1 - m) * 2048], [(w - 1 - m) * 2048 + 1, 2048 * 10],
                    [2048 * 10, (h - 1 - m) * 2048 + 1]])
    cand = np.array([[25, 20], [46, 20], [m, 30], [m - 1, 35], [30, m], [35, m - 1],
                     [w - 1 - m, 30], [w - m, 36], [30, h - 1 - m], [36, h - m], [15, 20], [35, 20]])
    # min_dist 5: (25, 20) is 5 from pixel 20 (not near), (46, 20) is 5 from pixel 41 (not near);
    # (15, 20) is 5 from 20 (not near), (35, 20) is 6 from 41
    want = run_update(q11, np.arange(8) + 100, np.zeros(8), [0, 8], cand, np.arange(len(cand)) + 1,
                      [0, len(cand)], [0], (h, w), min_dist=5, margin=m, max_tracks=100, passes=4)
    old = want["src"][(want["src"] & ts.NEW) == 0].tolist()
    new = (want["src"][(want["src"] & ts.NEW) != 0] & 0x7FFFFFFF).tolist()
    assert old == [0, 1, 2, 5] and new == [0, 1, 2, 4, 6, 8, 10, 11]
    near = run_update(q11, np.arange(8) + 100, np.zeros(8), [0, 8], cand, np.arange(len(cand)) + 1,
                      [0, len(cand)], [0], (h, w), min_dist=6, margin=m, max_tracks=100, passes=4)
    new = (near["src"][(near["src"] & ts.NEW) != 0] & 0x7FFFFFFF).tolist()
    assert 0 not in new and 1 not in new and 10 not in new and 11 in new


# ---- 4: the budget ------------------------------------------------------------------------------

def test_budget():
    s = random_scene(24, 64, 48, 80, 600, top=3)
    free = run_update(**one_stream(s), shape=(48, 64), min_dist=5, margin=3, max_tracks=10000,
                      passes=32)
    kept = int(((free["src"] & ts.NEW) == 0).sum())
    fresh = int(free["offsets"][-1]) - kept
    assert kept > 8 and fresh > 20
    for max_tracks in (kept, kept - 5, 1, kept + 1, kept + fresh // 2, kept + fresh - 1,
                       kept + fresh, kept + fresh + 1):
        want = run_update(**one_stream(s), shape=(48, 64), min_dist=5, margin=3,
                          max_tracks=max_tracks, passes=32)
        n_new = int(want["offsets"][-1]) - kept
        assert n_new == max(0, min(fresh, max_tracks - kept))
        assert want["next_id"][0] == 1000 + n_new
    # scores 0..2 over some 30 admitted candidates: the cuts above fall inside runs of equal scores


def test_budget_with_sixteen_bit_scores():
    s = random_scene(25, 64, 48, 10, 600)
    s["scores"] = np.random.default_rng(2).choice([0, 255, 256, 257, 0x1234, 0x12FF, 0xFFFF], 600)
    for max_tracks in (12, 25, 40):
        run_update(**one_stream(s), shape=(48, 64), min_dist=3, margin=3, max_tracks=max_tracks,
                   passes=32)


# ---- 5: ids, ages, status, src ------------------------------------------------------------------

def test_ids_wrap_ages_saturate_and_equal_ages_go_by_index():
    q11 = np.array([[20, 20], [21, 20], [40, 20], [41, 21], [50, 40]]) * ts.ONE
    ages = [7, 7, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]
    cand = np.array([[10, 10], [30, 30], [10, 40], [55, 10]])
    want = run_update(q11, [11, 12, 13, 14, 0xFFFFFFFF], ages, [0, 5], cand, [5, 5, 5, 5], [0, 4],
                      [0xFFFFFFFE], (48, 64), min_dist=4, margin=2, max_tracks=100, passes=4)
    assert want["src"].tolist() == [0, 2, 4] + [ts.NEW | k for k in range(4)]
    assert want["ages"].tolist() == [8, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0, 0]
    assert want["ids"].tolist() == [11, 13, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    assert want["next_id"].tolist() == [2]


def test_status_null_equals_all_ones_and_src_is_optional():
    s = random_scene(26, 64, 48, 60, 200)
    args = one_stream(s)
    args["status"] = None
    a = run_update(**args, shape=(48, 64), min_dist=5, margin=3, max_tracks=100, passes=8)
    args["status"] = np.ones(60, np.uint8)
    b = run_update(**args, shape=(48, 64), min_dist=5, margin=3, max_tracks=100, passes=8, src=False)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert (s["q11"] == -1).all(axis=1).any()              # lost markers drop out by themselves
    args["status"] = np.full(60, 0x80, np.uint8)           # any non-zero byte
    c = run_update(**args, shape=(48, 64), min_dist=5, margin=3, max_tracks=100, passes=8)
    assert np.array_equal(a["src"], c["src"])


# ---- 6: many workgroups -------------------------------------------------------------------------

def test_many_workgroups():
    s = random_scene(27, 640, 480, 1500, 6000, top=1 << 16, margin=11)
    want = run_update(**one_stream(s), shape=(480, 640), min_dist=12, margin=11, max_tracks=900,
                      passes=8)
    kept = int(((want["src"] & ts.NEW) == 0).sum())
    assert 300 < kept < 900 and int(want["offsets"][-1]) == 900        # the budget cuts the refill


# ---- 7: rejected calls --------------------------------------------------------------------------

def test_rejected_calls():
    """Every FDF_ERR_ARG of the header, synchronously and with nothing written."""
    import torch

    lib = _native.load()
    ctx = fast_hip.context(0).handle
    s = random_scene(28, 64, 48, 20, 50)
    t = {"q11": dev(torch, s["q11"], np.int32), "status": dev(torch, s["status"], np.uint8),
         "ids": dev(torch, s["ids"], np.uint32).view(torch.int32),
         "ages": dev(torch, s["ages"], np.uint32).view(torch.int32),
         "t_offs": dev(torch, [0, 20], np.int64),
         "cand": dev(torch, s["cand"], np.uint32).view(torch.int32),
         "scores": dev(torch, s["scores"], np.uint16).view(torch.int16),
         "c_offs": dev(torch, [0, 50], np.int64),
         "next_id": dev(torch, [77], np.uint32).view(torch.int32)}
    out = {"q11": gap_tensor(torch, (80, 2), torch.int32), "ids": gap_tensor(torch, (80,), torch.int32),
           "ages": gap_tensor(torch, (80,), torch.int32), "src": gap_tensor(torch, (80,), torch.int32),
           "offs": gap_tensor(torch, (2,), torch.int64)}
    need = fast_hip.tracks_scratch_bytes(1, (48, 64), 5, 20, 50)
    scratch = gap_tensor(torch, (need + 256,), torch.uint8)
    base = dict(n_frames=1, width=64, height=48, min_dist=5, margin=3, max_tracks=70, passes=8,
                q11=t["q11"].data_ptr(), status=t["status"].data_ptr(), ids=t["ids"].data_ptr(),
                ages=t["ages"].data_ptr(), t_offs=t["t_offs"].data_ptr(), t_cap=20,
                cand=t["cand"].data_ptr(), scores=t["scores"].data_ptr(),
                c_offs=t["c_offs"].data_ptr(), c_cap=50, next_id=t["next_id"].data_ptr(),
                o_q11=out["q11"].data_ptr(), o_ids=out["ids"].data_ptr(),
                o_ages=out["ages"].data_ptr(), o_src=out["src"].data_ptr(), out_cap=70,
                o_offs=out["offs"].data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need,
                ctx=ctx, params=True)

    def call(**change):
        a = dict(base, **change)
        p = _native.FdfTracksParams(a["width"], a["height"], a["min_dist"], a["margin"],
                                    a["max_tracks"], a["passes"])
        rc = lib.fdf_tracks_update_device(
            a["ctx"], a["n_frames"], ctypes.byref(p) if a["params"] else None, a["q11"], a["status"],
            a["ids"], a["ages"], a["t_offs"], a["t_cap"], a["cand"], a["scores"], a["c_offs"],
            a["c_cap"], a["next_id"], a["o_q11"], a["o_ids"], a["o_ages"], a["o_src"], a["out_cap"],
            a["o_offs"], a["scratch"], a["scratch_bytes"], None)
        torch.cuda.synchronize()
        return rc

    bad = [dict(ctx=None), dict(params=False), dict(min_dist=0), dict(min_dist=256), dict(margin=24),
           dict(margin=0x80000000), dict(max_tracks=0), dict(passes=0), dict(passes=33),
           dict(width=0), dict(height=0), dict(width=65536), dict(height=65536),
           dict(n_frames=65536), dict(t_cap=1 << 32), dict(c_cap=1 << 32), dict(t_cap=1 << 31),
           dict(c_cap=1 << 31), dict(q11=None), dict(ids=None), dict(ages=None), dict(t_offs=None),
           dict(cand=None), dict(scores=None), dict(c_offs=None), dict(next_id=None),
           dict(o_q11=None), dict(o_ids=None), dict(o_ages=None), dict(o_offs=None),
           dict(scratch=None), dict(scratch_bytes=need - 1), dict(scratch=base["scratch"] + 128)]
    for key, step in (("q11", 4), ("cand", 4), ("o_q11", 4), ("t_offs", 4), ("c_offs", 4),
                      ("o_offs", 4), ("ids", 2), ("ages", 2), ("next_id", 2), ("o_ids", 2),
                      ("o_ages", 2), ("o_src", 2), ("scores", 1)):
        bad.append({key: base[key] + step})
    for change in bad:
        assert call(**change) == _native.FDF_ERR_ARG, change
    assert call(n_frames=0) == _native.FDF_OK
    for k, v in out.items():
        assert (v.view(torch.uint8) == GAP).all(), k
    assert (scratch == GAP).all() and int(t["next_id"][0]) == 77
    with pytest.raises(FdfError):
        fast_hip.tracks_update_device(t["q11"], t["ids"], t["ages"], t["t_offs"], t["cand"],
                                      t["scores"], t["c_offs"], t["next_id"], out["q11"], out["ids"],
                                      out["ages"], out["offs"], (48, 64), min_dist=5, margin=3,
                                      scratch=scratch[:need - 256])
    # the same call goes through once nothing is wrong, the 2^31 caps without d_out_src too
    assert call() == _native.FDF_OK
    assert int(out["offs"][1]) > 0 and int(t["next_id"][0]) > 77


# ---- 8: host entries ----------------------------------------------------------------------------

def test_update_tracks_host_entry():
    args, want = ts.header_example()
    got = fast_hip.update_tracks((24, 32), args["q11"], args["ids"], args["ages"], args["cand"],
                                 args["scores"], next_id=7, min_dist=5, margin=2, max_tracks=4,
                                 passes=8, status=args["status"])
    assert got.q11.tolist() == want["q11"] and got.ids.tolist() == want["ids"]
    assert got.ages.tolist() == want["ages"] and got.src.tolist() == want["src"]
    assert got.next_id == want["next_id"]
    s = random_scene(29, 64, 48, 80, 600)
    got = fast_hip.update_tracks((48, 64), s["q11"], s["ids"], s["ages"], s["cand"], s["scores"],
                                 next_id=5, min_dist=5, margin=3, max_tracks=90, passes=8,
                                 status=s["status"])
    ref = ts.update(s["q11"], s["status"], s["ids"], s["ages"], [0, 80], 80, s["cand"], s["scores"],
                    [0, 600], 600, [5], 64, 48, 5, 3, 90, 8)
    for k in OUTPUTS:
        assert np.array_equal(getattr(got, k), ref[k]), k
    assert got.next_id == ref["next_id"][0]
    empty = fast_hip.update_tracks((48, 64), np.zeros((0, 2), np.int32), [], [],
                                   np.zeros((0, 2), np.uint32), [])
    assert len(empty.ids) == 0 and empty.next_id == 0


def test_cpp_smoke_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_tracks")
    assert os.path.exists(exe), "run `make` first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout


# ---- 9: chained with the tracker ----------------------------------------------------------------

TRACK = dict(radius=4, max_iters=10, eps=20, min_eig=0.5)


def corners(img, t=12):
    return oracle.detect(np.ascontiguousarray(img), t, 9, 1, with_scores=True)


def test_track_update_track_chain():
    """track_device -> tracks_update_device -> track_device (FDF_COORDS_Q11) on three frames, every
    step against the chained restatements; the survivors keep their ids."""
    import torch

    frames = ts.moved(ts.texture(9, 112, 96), 72, 56, [(2, 1), (3, 3)])
    h, w = frames.shape[1:]
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    pyr = fast_hip.Pyramid(d_frames, 2, (2, 1))
    levels = [rs.pyramid(fr, 2, 2, 1) for fr in frames]
    xs, ys = np.meshgrid(np.linspace(6, w - 7, 5).astype(np.int64), np.linspace(6, h - 7, 4).astype(np.int64))
    pts = np.concatenate([np.stack([xs.ravel(), ys.ravel()], axis=1), [[0, 0], [70, 2], [31, 30]]])
    n = len(pts)
    ids0 = np.arange(n) + 500

    d_offs = dev(torch, [0, n], np.int64)
    q1 = gap_tensor(torch, (n, 2), torch.int32)
    st1 = gap_tensor(torch, (n,), torch.uint8)
    fast_hip.track_device(pyr, pyr, dev(torch, pts, np.int32), d_offs, q1, st1, prev_first=0,
                          next_first=1, n_frames=1, **TRACK)
    first = tr.track(levels[0:1], levels[1:2], pts, [0, n], n, **TRACK)
    assert np.array_equal(q1.cpu().numpy(), first["q11"])
    assert np.array_equal(st1.cpu().numpy(), first["status"])
    assert (first["status"] == 0).any() and (first["status"] == 1).any()

    cand, scores = corners(frames[1])
    assert len(cand) > 5
    want = run_update(first["q11"], ids0, np.zeros(n), [0, n], cand, scores, [0, len(cand)], [900],
                      (h, w), status=first["status"], min_dist=8, margin=5, max_tracks=40, passes=8)
    total = int(want["offsets"][-1])
    old = (want["src"] & ts.NEW) == 0
    assert old.any() and (~old).any()
    assert np.array_equal(want["ids"][old], ids0[want["src"][old]])
    assert want["ids"][~old].tolist() == list(range(900, 900 + int((~old).sum())))

    # the device's own output (run_update proved it equal to `want`) into the tracker as it is
    q2 = gap_tensor(torch, (total, 2), torch.int32)
    st2 = gap_tensor(torch, (total,), torch.uint8)
    fast_hip.track_device(pyr, pyr, dev(torch, want["q11"], np.int32),
                          dev(torch, want["offsets"], np.int64), q2, st2, prev_first=1, next_first=2,
                          n_frames=1, coords="q11", **TRACK)
    second = tr.track(levels[1:2], levels[2:3], want["q11"], [0, total], total,
                      coords=tr.COORDS_Q11, **TRACK)
    assert np.array_equal(q2.cpu().numpy(), second["q11"])
    assert np.array_equal(st2.cpu().numpy(), second["status"])
    assert second["status"].any()


def test_track_sequence_array():
    """Five frames through the whole loop on the device against the same chain built from the
    oracle's detections and the two restatements."""
    frames = np.ascontiguousarray(ts.moved(ts.texture(5, 256, 192), 208, 144,
                                           [(4, 1), (8, 3), (12, 5), (15, 8)]))
    h, w = frames.shape[1:]
    cfg = Config(12, 9, NonMaximalSuppression.MaxThreshold)
    opts = dict(min_dist=24, max_tracks=30, passes=8)
    got = fast_hip.track_sequence_array(frames, cfg, n_levels=2, scale=(2, 1), **opts, **TRACK)
    assert len(got) == 5

    levels = [rs.pyramid(fr, 2, 2, 1) for fr in frames]
    q11, ids, ages, nid = np.zeros((0, 2), np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
    seen, refills, drops = set(), 0, 0
    for k in range(5):
        cand, scores = corners(frames[k])
        status = None
        if k:
            moved = tr.track(levels[k - 1:k], levels[k:k + 1], q11, [0, len(q11)], len(q11),
                             coords=tr.COORDS_Q11, **TRACK)
            q11, status = moved["q11"], moved["status"]
        before = dict(zip(ids.tolist(), ages.tolist()))
        q11, ids, ages, kept, new, nid = ts.update_stream(
            q11, status, ids, ages, cand, scores, nid, w, h, margin=TRACK["radius"] + 1, **opts)
        refills += k > 0 and len(new) > 0
        drops += len(kept) < len(before)
        assert np.array_equal(got[k][0], ids) and got[k][0].dtype == np.uint32
        assert np.array_equal(got[k][1], q11) and got[k][1].dtype == np.int32
        assert np.array_equal(got[k][2], ages)
        for i, a in zip(ids.tolist(), ages.tolist()):       # ids persist and age by one per frame
            assert a == before[i] + 1 if i in before else (a == 0 and i not in seen)
        seen |= set(ids.tolist())
    assert len(ids) > 5 and ages.max() >= 3 and refills >= 2 and drops >= 2
