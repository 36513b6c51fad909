"""Least-squares refinement on the device (fdf_refine_device, fdf_refine_points) against the numpy
restatement of include/fdf.h's contract in tests/_refine_reference.py.  Every comparison is exact
(the model's doubles with ==, NaN equal to NaN, the sign of a zero free; the bytes and the rounds
equal); models, bytes and rounds are pre-filled and over-allocated so that what no frame owns can
be checked as untouched, the scratch holds garbage, and the inputs are checked unmodified."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _ransac_reference as rr
import _refine_reference as ref
import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A                                        # of the inlier bytes
MODEL_FILL = -7.25                                 # of the output models' 11 doubles
ROUNDS_FILL = -3                                   # of the rounds
EXTRA = 16                                         # bytes past the capacity
MODELS = {"affine": rr.AFFINE, "homography": rr.HOMOGRAPHY}
PLANTED = {"affine": np.array([[1.03, 0.04, 12.0], [0.02, 0.97, 25.0], [0.0, 0.0, 1.0]]),
           "homography": np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, 40.0], [1e-5, -2e-5, 1.0]])}
SIZES = (0, 3, 4, 5, 255, 256, 257, 513)           # the lane wrap and the tree's edges


@functools.lru_cache(maxsize=None)
def planted(model, m, outliers, seed, dtype=np.uint32):
    """(queries, trains) as `dtype`: `m` random integer points below 1800, their rounded
    projections under PLANTED[model] and `outliers` of the trains re-drawn; float32 sets are
    moved off the grid by a half and a quarter pixel.  Read-only."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1800, (m, 2)).astype(np.float64)
    p = np.c_[q, np.ones(m)] @ PLANTED[model].T
    t = np.rint(p[:, :2] / p[:, 2:])
    bad = rng.permutation(m)[:outliers]
    t[bad] = rng.integers(0, 2048, (len(bad), 2))
    assert t.min(initial=0) >= 0 and t.max(initial=0) < 2048
    if dtype == np.float32:
        q, t = q + 0.5, t + 0.25
    q, t = q.astype(dtype), t.astype(dtype)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def start_models(model, n, shift=0.4):
    """`n` records holding PLANTED[model] moved by `shift` pixels: what a minimal sample gives."""
    h = PLANTED[model].copy()
    h[0, 2] += shift
    h[1, 2] -= shift
    out = np.zeros(n, dtype=rr.MODEL_DTYPE)
    for f in range(n):
        out[f] = ref.model_record(h, 1000 + f, 2000 + f, 7 + f, 40 + f)
    return out


def device_coords(torch, coords):
    a = np.ascontiguousarray(coords)
    if a.dtype == np.float32:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()


def device_models(torch, records, rows=None):
    a = np.ascontiguousarray(records).view(np.float64).reshape(-1, 11)
    if rows is not None and rows > len(a):
        a = np.concatenate([a, np.full((rows - len(a), 11), MODEL_FILL)])
    return torch.from_numpy(a.copy()).cuda()


def device_scratch(torch, n_frames, q_cap, fill=0xA5):
    """A 256-byte aligned scratch tensor holding garbage: the call must not need it zeroed."""
    need = fast_hip.refine_scratch_bytes(n_frames, q_cap)
    raw = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 256
    return raw[lead:lead + need]


def run_refine(matches, q_offs, q_coords, t_coords, t_offs, model, models_in, threshold, n_rounds,
               keep=None, q_cap=None, t_cap=None, scratch=None, stream=None, in_place=False):
    """fdf_refine_device on uploaded arrays -> ((F,) model records, the (q_cap + EXTRA,) inlier
    bytes, the (F,) rounds); checks that the row past the frames' and the inputs are untouched."""
    import torch

    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    n = len(q_offs) - 1
    d_m = torch.from_numpy(np.ascontiguousarray(matches).view(np.int32).reshape(-1, 2).copy()).cuda()
    d_q, d_t = device_coords(torch, q_coords), device_coords(torch, t_coords)
    d_qo = torch.from_numpy(np.asarray(q_offs).astype(np.int64)).cuda()
    d_to = torch.from_numpy(np.asarray(t_offs).astype(np.int64)).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.uint8).copy()).cuda()
    d_in = device_models(torch, models_in, n + 1)
    d_out = d_in if in_place else torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64,
                                             device="cuda")
    inliers = torch.full((q_cap + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    rounds = torch.full((n + 1,), ROUNDS_FILL, dtype=torch.int32, device="cuda")
    if scratch is None:
        scratch = device_scratch(torch, n, q_cap)
    fast_hip.refine_device(d_m[:q_cap], d_qo, d_q, d_t[:t_cap], d_to, d_in[:n], d_out[:n], scratch,
                           keep=d_keep, inliers=inliers[:q_cap], rounds=rounds[:n], model=model,
                           threshold=threshold, n_rounds=n_rounds, stream=stream)
    torch.cuda.synchronize()
    assert (d_out[n] == MODEL_FILL).all() and rounds[n] == ROUNDS_FILL
    assert np.array_equal(d_m.cpu().numpy().view(np.uint32).reshape(-1),
                          np.ascontiguousarray(matches).view(np.uint32).reshape(-1))
    assert d_q.cpu().numpy().tobytes() == device_coords(torch, q_coords).cpu().numpy().tobytes()
    assert d_t.cpu().numpy().tobytes() == device_coords(torch, t_coords).cpu().numpy().tobytes()
    if not in_place:
        assert d_in[:n].cpu().numpy().tobytes() == np.ascontiguousarray(models_in).tobytes()
    return (fast_hip.unpack_models(d_out[:n].cpu().numpy()), inliers.cpu().numpy(),
            rounds[:n].cpu().numpy().astype(np.uint32))


def reference(matches, q_offs, q_coords, t_coords, t_offs, model, models_in, threshold, n_rounds,
              keep=None, q_cap=None, t_cap=None):
    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    return ref.refine(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, MODELS[model],
                      models_in, threshold, n_rounds,
                      inliers_out=np.full(q_cap + EXTRA, FILL, np.uint8))


def assert_same(got, want):
    for f in range(len(want[0])):
        assert rr.models_equal(got[0][f], want[0][f]), (f, got[0][f], want[0][f])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])


def both(*args, **kw):
    """(device result, reference result), asserted equal."""
    dev = {k: kw.pop(k) for k in ("scratch", "stream", "in_place") if k in kw}
    got = run_refine(*args, **kw, **dev)
    want = reference(*args, **kw)
    assert_same(got, want)
    return got, want


# ---- 1: the worked example of include/fdf.h ----------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
def test_worked_example(model, dtype):
    q, t = rr.worked_example()
    start = np.zeros(1, dtype=rr.MODEL_DTYPE)
    start[0] = ref.model_record([1, 0, 3, 0, 1, 5, 0, 0, 1], 6, 5, 3, 8)
    (got, mask, rounds), _ = both(rr.identity_matches(6), [0, 6], q.astype(dtype), t.astype(dtype),
                                  [0, 6], model, start, 1.0, 1)
    m = got[0]
    assert (m["hypothesis"], m["n_inliers"], m["n_valid"], m["n_corr"]) == (3, 5, 8, 6)
    assert rounds.tolist() == [1] and mask[:6].tolist() == [1, 1, 1, 1, 0, 1]
    assert (mask[6:] == FILL).all()
    if model == "affine":
        assert m["h"].tolist() == [1, 0, 3, 0, 1, 5, 0, 0, 1]
    else:
        assert m["h"][0] == float.fromhex("0x1.0000000000001p+0")
        assert m["h"][7] == float.fromhex("-0x1.a85e37930f5e6p-57")


# ---- 2: planted sets across the lane wrap and the tree's edges ------------------------------------

@functools.lru_cache(maxsize=None)
def size_batch(model, dtype, outlier_percent):
    """Frames of SIZES correspondences over shared arrays."""
    parts = [planted(model, m, m * outlier_percent // 100, 100 + m, dtype) for m in SIZES]
    offs = np.cumsum([0] + list(SIZES))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), offs


@pytest.mark.parametrize("model", ["affine", "homography"])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
@pytest.mark.parametrize("outlier_percent", [0, 40])
def test_planted_sizes(model, dtype, outlier_percent):
    q, t, offs = size_batch(model, dtype, outlier_percent)
    start = start_models(model, len(SIZES))
    (got, _, rounds), _ = both(rr.identity_matches(len(q)), offs, q, t, offs, model, start, 2.0, 3)
    assert got["n_corr"].tolist() == list(SIZES)
    assert np.array_equal(got["hypothesis"], start["hypothesis"])
    assert np.array_equal(got["n_valid"], start["n_valid"])
    s = rr.sample_size(MODELS[model])
    assert rounds[0] == 0 and (rounds[np.array(SIZES) < s] == 0).all()
    assert (rounds[4:] >= 1).all()                       # hundreds of inliers: a round is accepted
    # the refit is closer to the planted map than the start, which is 0.4 px off (the float
    # sets are moved off the grid: another map)
    for f in range(4, len(SIZES) if dtype == np.uint32 else 0):
        assert np.abs(got[f]["h"][[2, 5]] - PLANTED[model][:2, 2]).max() < 0.2


@pytest.mark.parametrize("n_rounds", [0, 1, 8])
def test_round_counts(n_rounds):
    q, t, offs = size_batch("homography", np.uint32, 40)
    start = start_models("homography", len(SIZES))
    (got, _, rounds), _ = both(rr.identity_matches(len(q)), offs, q, t, offs, "homography", start,
                               2.0, n_rounds)
    assert rounds.max() <= n_rounds
    if n_rounds == 0:
        assert np.array_equal(got["h"], start["h"]) and got["n_inliers"][7] > 250


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_exactly_a_sample_of_inliers(model):
    """s pairs under the model among far outliers: n = s is the smallest set that is refitted."""
    s = rr.sample_size(MODELS[model])
    q, t = planted(model, 40, 0, 77)
    t = t.copy()
    t[s:] = (t[s:] + 700) % 2048
    start = start_models(model, 1)
    (got, mask, rounds), _ = both(rr.identity_matches(40), [0, 40], q, t, [0, 40], model, start, 2.0,
                                  2)
    assert got[0]["n_inliers"] == s and mask[:40].sum() == s and mask[:s].all()
    assert rounds[0] >= 1


# ---- 3: a batch with every way a frame can be special ----------------------------------------------

def batch():
    """Six frames over shared arrays: an empty one, one whose record holds no model, one whose
    matches hold FDF_MATCH_NONE, indices outside the train range and keep = 0, two plain ones
    (one of them with a NaN in its model), and one cut by q_cap."""
    n = (0, 60, 120, 300, 40, 90)
    parts = [planted("homography", m, m // 4, 30 + k) for k, m in enumerate(n)]
    q = np.concatenate([p[0] for p in parts])
    t = np.concatenate([p[1] for p in parts])
    q_offs = np.cumsum([0] + list(n))
    matches = rr.identity_matches(len(q))
    lo = q_offs[2]
    matches["index"][lo + 5] = rr.NONE
    matches["index"][lo + 6] = 1                               # frame 1's train point
    matches["index"][lo + 7] = q_offs[3] + 2                   # frame 3's
    matches["index"][lo + 8] = len(q) + 1000                   # beyond the array
    keep = np.ones(len(q), np.uint8)
    keep[lo + 20:lo + 25] = 0
    keep[q_offs[5] + 4] = 0
    start = start_models("homography", 6)
    start[1]["hypothesis"] = rr.NONE
    start[1]["h"] = np.arange(9.0)                             # passes through whatever it holds
    start[4]["h"][4] = np.nan                                  # no inliers: nothing to refit
    return matches, q_offs, q, t, keep, start, len(q) - 10


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_batch_of_frames(model):
    matches, q_offs, q, t, keep, start, q_cap = batch()
    args = (matches, q_offs, q, t, q_offs, model, start, 3.0, 3)
    (got, mask, rounds), _ = both(*args, keep=keep, q_cap=q_cap)
    assert got["n_corr"].tolist() == [0, 1001, 120 - 4 - 5, 300, 40, 90 - 10 - 1]
    assert rounds[0] == rounds[1] == rounds[4] == 0 and got[4]["n_inliers"] == 0
    assert got[1]["h"].tolist() == list(range(9)) and got[1]["n_inliers"] == 2001
    assert not mask[q_offs[1]:q_offs[2]].any() and not mask[q_offs[4]:q_offs[5]].any()
    assert (mask[q_cap:] == FILL).all() and mask[:q_cap].sum() == got["n_inliers"][[0, 2, 3, 4, 5]].sum()
    if model == "homography":
        assert rounds[3] >= 1 and rounds[5] >= 1
    # in place: models_out is models_in
    again = run_refine(*args, keep=keep, q_cap=q_cap, in_place=True)
    assert again[0].tobytes() == got.tobytes() and np.array_equal(again[1], mask)
    assert np.array_equal(again[2], rounds)
    # a train capacity that cuts the last train range, and train offsets of their own
    t_offs = q_offs + np.array([0, 0, 0, 0, 0, 0, 50])
    both(matches, q_offs, q, t, t_offs, model, start, 3.0, 2, t_cap=len(t) - 30)
    # no keep bytes, queries that start past index 0: only the frames' bytes are written
    (_, mask, _), _ = both(matches, q_offs[2:], q, t, q_offs[2:], model, start[2:], 3.0, 1)
    assert (mask[:q_offs[2]] == FILL).all()


# ---- 4: degenerate data -----------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_degenerate_frames_keep_their_model(model):
    """Frames of: one point twenty times (d = 0), collinear points, s - 1 inliers among outliers,
    and s - 1 inliers beside a pair with a NaN and one with an infinity (float coordinates)."""
    s = rr.sample_size(MODELS[model])
    rng = np.random.default_rng(8)
    one = np.tile([[7, 9]], (20, 1))
    line = np.stack([np.arange(20) * 7, np.arange(20) * 14 + 3], axis=1)
    few = rng.integers(0, 100, (12, 2))
    few_t = few + [40, 70]
    few_t[:s - 1] = few[:s - 1] + [3, 5]
    nan = rng.integers(0, 100, (s + 1, 2))
    q = np.concatenate([one, line, few, nan]).astype(np.float32)
    t = np.concatenate([one + [3, 5], line + [3, 5], few_t, nan + [3, 5]]).astype(np.float32)
    offs = np.cumsum([0, 20, 20, 12, s + 1])
    q[offs[3], 0] = np.nan
    t[offs[3] + 1, 1] = np.inf
    start = np.zeros(4, dtype=rr.MODEL_DTYPE)
    for f in range(4):
        start[f] = ref.model_record([1, 0, 3, 0, 1, 5, 0, 0, 1], 0, 0, f, 9)
    (got, mask, rounds), _ = both(rr.identity_matches(len(q)), offs, q, t, offs, model, start, 1.0, 3)
    assert rounds.tolist() == [0, 0, 0, 0]
    assert np.array_equal(got["h"], start["h"])
    assert got["n_inliers"].tolist() == [20, 20, s - 1, s - 1]
    assert mask[offs[3]:offs[3] + 2].tolist() == [0, 0]
    # the same as integers (no NaN frame)
    both(rr.identity_matches(offs[3]), offs[:4], q[:offs[3]].astype(np.uint32),
         t[:offs[3]].astype(np.uint32), offs[:4], model, start[:3], 1.0, 3)


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_nan_pair_among_many_inliers(model):
    """A NaN and an infinity among 300 float pairs never enter a sum: the refit is the
    reference's, finite, and those two are no inliers."""
    q, t = planted(model, 300, 60, 91, np.float32)
    q, t = q.copy(), t.copy()
    q[7, 0] = np.nan
    t[9, 1] = np.nan
    q[20, 1] = np.inf
    t[33, 0] = -np.inf
    (got, mask, rounds), _ = both(rr.identity_matches(300), [0, 300], q, t, [0, 300], model,
                                  start_models(model, 1), 2.0, 2)
    assert mask[[7, 9, 20, 33]].tolist() == [0, 0, 0, 0] and rounds[0] >= 1
    assert np.isfinite(got[0]["h"]).all() and got[0]["n_inliers"] >= 230


def test_a_refit_that_loses_inliers_is_not_accepted():
    """tests/test_refine.py's construction: twenty pairs on the edge of T = 2."""
    rng = np.random.default_rng(6)
    q = np.stack([rng.integers(0, 200, 20), rng.integers(0, 200, 20)], axis=1).astype(np.uint32)
    q[:, 0] += 2
    t = q.copy()
    t[:12, 0] += 2
    t[19, 0] -= 2
    start = np.zeros(1, dtype=rr.MODEL_DTYPE)
    start[0] = ref.model_record([1, 0, 0, 0, 1, 0, 0, 0, 1])
    for model in ("affine", "homography"):
        (got, mask, rounds), _ = both(rr.identity_matches(20), [0, 20], q, t, [0, 20], model, start,
                                      2.0, 3)
        assert rounds[0] == 0 and got[0]["n_inliers"] == 20 and mask[:20].all()
        assert got[0]["h"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
        (got, _, rounds), _ = both(rr.identity_matches(20), [0, 20], q, t, [0, 20], model, start,
                                   4.0, 1)
        assert rounds[0] == 1 and got[0]["n_inliers"] == 20
        assert got[0]["h"].tolist() != [1, 0, 0, 0, 1, 0, 0, 0, 1]


# ---- 5: determinism, streams, scratch reuse --------------------------------------------------------

def test_same_call_twice_and_on_another_stream():
    import torch

    q, t, offs = size_batch("homography", np.uint32, 40)
    m = rr.identity_matches(len(q))
    start = start_models("homography", len(SIZES))
    args = (m, offs, q, t, offs, "homography", start, 2.0, 2)
    first = run_refine(*args)
    scratch = device_scratch(torch, len(offs) - 1, len(q), fill=0x3C)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        second = run_refine(*args, scratch=scratch, stream=stream)
        other = run_refine(m, offs, q, t, offs, "affine", start, 2.0, 2, scratch=scratch,
                           stream=stream)
        third = run_refine(*args, scratch=scratch, stream=stream)
    for again in (second, third):
        assert first[0].tobytes() == again[0].tobytes() and np.array_equal(first[1], again[1])
        assert np.array_equal(first[2], again[2])
    assert first[0].tobytes() != other[0].tobytes()


# ---- 6: argument errors from the C ABI -------------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    n = 32
    pts = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, n], dtype=torch.int64, device="cuda")
    matches = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    start = np.zeros(2, dtype=rr.MODEL_DTYPE)
    start["h"][:, [0, 4, 8]] = 1.0
    models_in = device_models(torch, start, 3)
    models = torch.full((3, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    rounds = torch.full((3,), ROUNDS_FILL, dtype=torch.int32, device="cuda")
    scratch = device_scratch(torch, 2, n)
    lib = _native.load()
    good = dict(ctx=fast_hip.context(0).handle, n=2, m=matches.data_ptr(), keep=None, qcap=n,
                qo=offs.data_ptr(), q=pts.data_ptr(), t=pts.data_ptr(), tcap=n, to=offs.data_ptr(),
                coords=0, model=1, min=models_in.data_ptr(), thr=3.0, nr=2, out=models.data_ptr(),
                inl=inliers.data_ptr(), r=rounds.data_ptr(), s=scratch.data_ptr(),
                sb=scratch.numel())

    def call(**kw):
        a = {**good, **kw}
        return lib.fdf_refine_device(a["ctx"], a["n"], a["m"], a["keep"], a["qcap"], a["qo"], a["q"],
                                     a["t"], a["tcap"], a["to"], a["coords"], a["model"], a["min"],
                                     a["thr"], a["nr"], a["out"], a["inl"], a["r"], a["s"], a["sb"],
                                     None)

    for bad in (dict(ctx=None), dict(m=None), dict(qo=None), dict(q=None), dict(t=None),
                dict(to=None), dict(min=None), dict(out=None), dict(s=None), dict(n=65536),
                dict(qcap=0xFFFFFFFF), dict(tcap=0xFFFFFFFF), dict(qcap=1 << 40), dict(coords=2),
                dict(model=2), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")),
                dict(nr=9), dict(nr=0xFFFFFFFF), dict(m=matches.data_ptr() + 4),
                dict(q=pts.data_ptr() + 4), dict(t=pts.data_ptr() + 4),
                dict(min=models_in.data_ptr() + 4), dict(out=models.data_ptr() + 4),
                dict(r=rounds.data_ptr() + 2), dict(s=scratch.data_ptr() + 128),
                dict(sb=scratch.numel() - 1)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(n=0, m=None, out=None, s=None, min=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (models == MODEL_FILL).all() and (inliers == FILL).all() and (rounds == ROUNDS_FILL).all()
    # the good call works, on the null stream and without the optional outputs: under the
    # identity every all-zero pair of frame 0 is an inlier (d = 0: no round), and frame 1's
    # matches (index 0) lie outside its train range
    assert call(inl=None, r=None) == _native.FDF_OK
    assert call() == _native.FDF_OK
    torch.cuda.synchronize()
    got = fast_hip.unpack_models(models[:2].cpu().numpy())
    assert got["n_corr"].tolist() == [16, 0] and got["n_inliers"].tolist() == [16, 0]
    assert np.array_equal(got["h"], start["h"]) and rounds.tolist() == [0, 0, ROUNDS_FILL]
    assert (models[2] == MODEL_FILL).all() and inliers.tolist() == [1] * 16 + [0] * 16


# ---- 7: the chain on the device -----------------------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_ransac_then_refine_on_the_device(model):
    """fdf_ransac_device's models go straight into fdf_refine_device on the same stream, in
    place, with no host copy in between; the host only checks afterwards."""
    import torch

    parts = [planted(model, m, m * 2 // 5, 50 + m) for m in (300, 0, 257)]
    q = np.concatenate([p[0] for p in parts])
    t = np.concatenate([p[1] for p in parts])
    offs = np.array([0, 300, 300, 557])
    matches = rr.identity_matches(len(q))
    n_hyp, n = 128, 3
    d_m = torch.from_numpy(matches.view(np.int32).reshape(-1, 2).copy()).cuda()
    d_q, d_t = device_coords(torch, q), device_coords(torch, t)
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    models = torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    refined = torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((len(q) + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    rounds = torch.full((n,), ROUNDS_FILL, dtype=torch.int32, device="cuda")
    need = fast_hip.ransac_scratch_bytes(n, len(q), n_hyp)
    raw = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 256
    scratch = raw[lead:lead + need]                           # one scratch serves both stages
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.ransac_device(d_m, d_o, d_q, d_t, d_o, models[:n], scratch, model=model,
                               n_hyp=n_hyp, threshold=1.5, seed=3)
        fast_hip.refine_device(d_m, d_o, d_q, d_t, d_o, models[:n], refined[:n], scratch,
                               inliers=inliers[:len(q)], rounds=rounds, model=model, threshold=1.5,
                               n_rounds=2)
        fast_hip.refine_device(d_m, d_o, d_q, d_t, d_o, models[:n], models[:n], scratch,
                               model=model, threshold=1.5, n_rounds=2)
    stream.synchronize()
    first, _ = rr.ransac(matches, None, len(q), offs, q, t, len(t), offs, MODELS[model], n_hyp, 1.5, 3)
    want = ref.refine(matches, None, len(q), offs, q, t, len(t), offs, MODELS[model], first, 1.5, 2,
                      inliers_out=np.full(len(q) + EXTRA, FILL, np.uint8))
    got = fast_hip.unpack_models(refined[:n].cpu().numpy())
    assert_same((got, inliers.cpu().numpy(), rounds.cpu().numpy().astype(np.uint32)), want)
    assert fast_hip.unpack_models(models[:n].cpu().numpy()).tobytes() == got.tobytes()
    assert (refined[n] == MODEL_FILL).all() and (models[n] == MODEL_FILL).all()
    assert got[1]["hypothesis"] == rr.NONE and got[0]["hypothesis"] != rr.NONE
    assert (got["n_inliers"] >= first["n_inliers"]).all()


# ---- 8: the host entries ---------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_host_entries_agree_with_the_device_entry(model):
    q, t = planted(model, 300, 120, 7)
    matches = rr.identity_matches(300)
    matches["index"][11] = rr.NONE
    keep = np.ones(300, np.uint8)
    keep[[2, 3]] = 0
    first, _ = rr.ransac(matches, keep, 300, [0, 300], q, t, 300, [0, 300], MODELS[model], 200, 3.0, 6)
    dev = run_refine(matches, [0, 300], q, t, [0, 300], model, first, 3.0, 2, keep=keep)
    H, mask, rec, rounds = fast_hip.refine_model(q, t, matches, first[0], keep=keep, model=model,
                                                 threshold=3.0, n_rounds=2)
    assert rr.models_equal(rec, dev[0][0]) and np.array_equal(mask, dev[1][:300].astype(bool))
    assert rounds == dev[2][0] >= 1 and rec["n_corr"] == 297 and mask.dtype == np.bool_
    assert H.shape == (3, 3) and np.array_equal(H.reshape(-1), rec["h"])
    # estimate_model with refine_rounds is the two calls; without it, today's result
    H2, mask2, rec2 = fast_hip.estimate_model(q, t, matches, keep=keep, model=model, n_hyp=200,
                                              threshold=3.0, seed=6, refine_rounds=2)
    assert rr.models_equal(rec2, rec) and np.array_equal(mask2, mask) and np.array_equal(H2, H)
    _, _, plain = fast_hip.estimate_model(q, t, matches, keep=keep, model=model, n_hyp=200,
                                          threshold=3.0, seed=6)
    assert rr.models_equal(plain, first[0])
    # float points, a (3, 3) start, train indices instead of records
    index = matches["index"].astype(np.int64)
    index[11] = -1
    Hf, maskf, recf, roundsf = fast_hip.refine_model(
        q.astype(np.float32), t.astype(np.float32), index, first[0]["h"].reshape(3, 3), keep=keep,
        model=model, threshold=3.0, n_rounds=2)
    assert np.array_equal(recf["h"], rec["h"]) and np.array_equal(maskf, mask) and roundsf == rounds
    assert (recf["hypothesis"], recf["n_valid"]) == (0, 0)
    # no model: H is None, the record passes through
    none = np.zeros((), dtype=rr.MODEL_DTYPE)
    none["hypothesis"], none["n_corr"] = rr.NONE, 5
    H, mask, rec, rounds = fast_hip.refine_model(q, t, matches, none, model=model)
    assert H is None and not mask.any() and rounds == 0 and rec.tobytes() == none.tobytes()
    H, mask, rec, rounds = fast_hip.refine_model(q[:0], t, matches[:0], first[0], model=model)
    assert H is not None and len(mask) == 0 and rounds == 0 and rec["n_corr"] == 0


def test_host_entry_rejects_bad_arguments_and_keeps_fetch_last():
    lib = _native.load()
    img = workloads.golden_image()
    pts, scores = fast_hip.detect_scored_array(img, Config(16, 9, NonMaximalSuppression.MaxThreshold))
    ctx = fast_hip.context(0).handle
    q, t = rr.worked_example()
    m = rr.identity_matches(6)
    start = np.zeros(1, dtype=rr.MODEL_DTYPE)
    start[0] = ref.model_record([1, 0, 3, 0, 1, 5, 0, 0, 1], 6, 5, 3, 8)
    out = np.zeros(1, dtype=rr.MODEL_DTYPE)
    mask = np.full(6, FILL, np.uint8)
    rounds = ctypes.c_uint32(77)

    def call(c=ctx, qc=q.ctypes.data, tc=t.ctypes.data, nq=6, nt=6, mm=m.ctypes.data, coords=0,
             model=0, mi=start.ctypes.data, thr=1.0, nr=1, o=out.ctypes.data, inl=mask.ctypes.data,
             r=ctypes.addressof(rounds)):
        return lib.fdf_refine_points(c, qc, tc, nq, nt, mm, None, coords, model, mi, thr, nr, o, inl,
                                     r)

    for bad in (dict(c=None), dict(qc=None), dict(tc=None), dict(mm=None), dict(mi=None),
                dict(o=None), dict(coords=2), dict(model=2), dict(nr=9), dict(thr=-1.0),
                dict(thr=float("nan")), dict(nq=0xFFFFFFFF), dict(nt=0xFFFFFFFF)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert not out["h"].any() and (mask == FILL).all() and rounds.value == 77
    assert call(inl=None, r=None) == _native.FDF_OK and (mask == FILL).all() and rounds.value == 77
    assert call() == _native.FDF_OK
    assert out[0]["h"].tolist() == [1, 0, 3, 0, 1, 5, 0, 0, 1] and rounds.value == 1
    assert (out[0]["n_inliers"], out[0]["hypothesis"]) == (5, 3) and mask.tolist() == [1, 1, 1, 1, 0, 1]
    assert call(o=start.ctypes.data) == _native.FDF_OK and start[0] == out[0]     # in place
    # the retained detection is still there
    got = np.zeros((len(pts), 2), dtype=np.uint32)
    got_sc = np.zeros(len(pts), dtype=np.uint16)
    n = ctypes.c_size_t(0)
    rc = lib.fdf_fetch_last(ctx, got.ctypes.data, got_sc.ctypes.data, len(pts), ctypes.byref(n))
    assert rc == _native.FDF_OK and n.value == len(pts)
    assert np.array_equal(got, pts) and np.array_equal(got_sc, scores)


def test_cpp_refine_binary():
    """tests/cpp/test_cpp_refine.cpp's data through the device entry: the binary's printed models
    (17 digits) are the same doubles."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_refine")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
    k = np.arange(40)
    q = np.stack([7 * (k % 8) + k // 8, 11 * (k // 8) + k % 3], axis=1).astype(np.uint32)
    t = q + np.array([3, 5], dtype=np.uint32)
    t[0] = (500, 400)
    start = np.zeros(1, dtype=rr.MODEL_DTYPE)
    start[0] = ref.model_record([1, 0, 3.25, 0, 1, 4.75, 0, 0, 1], 0, 0, 12, 34)
    lines = re.findall(r"^model=(\d) rounds=1 inliers=39/40 hypothesis=12 valid=34 h=(.*)$",
                       res.stdout, re.M)
    assert [int(a) for a, _ in lines] == [rr.AFFINE, rr.HOMOGRAPHY]
    for (_, text), model in zip(lines, ("affine", "homography")):
        (got, _, _), _ = both(rr.identity_matches(40), [0, 40], q, t, [0, 40], model, start, 1.0, 1)
        assert np.array_equal(np.array([float(a) for a in text.split()]), got[0]["h"])
