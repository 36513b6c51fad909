"""RANSAC fundamental-matrix estimation on the device (fdf_fundamental_device,
fdf_fundamental_check_device, fdf_fundamental_points) against the restatement of include/fdf.h's
contract in tests/_fundamental_reference.py.  Every comparison is bit for bit (the model's nine
doubles by their bits); the inlier bytes and the models are pre-filled and over-allocated so that
what no frame owns can be checked as untouched.  The scenes' ground-truth conditions are those
that tests/test_fundamental.py proves of the restatement alone."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _fundamental_reference as ref
import _resize_reference as rs
import _track_reference as tr
import _tracks_reference as ts
from feature_detector_fast_amd import _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A                                        # of the inlier bytes
MODEL_FILL = -7.25                                 # of the models' 11 doubles
EXTRA = 16                                         # rows past the capacity
TILE = 256                                         # correspondences of the kernel's LDS tile


@functools.lru_cache(maxsize=None)
def two_views(m, outliers, seed, as_float=False):
    """(queries, trains, true-pair flags): `m` points before two cameras (the second turned and
    moved), projected and rounded to pixels (or to float32), `outliers` trains re-drawn uniformly.
    Read-only."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-3, 3, m), rng.uniform(-2, 2, m), rng.uniform(4, 10, m)], 1)
    a = 0.08
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    P2 = P @ R.T + np.array([0.6, 0.1, 0.2])
    q = 700 * P[:, :2] / P[:, 2:] + (900, 700)
    t = 700 * P2[:, :2] / P2[:, 2:] + (900, 700)
    good = np.ones(m, dtype=bool)
    bad = rng.permutation(m)[:outliers]
    t[bad] = rng.uniform(0, 1800, (len(bad), 2))
    good[bad] = False
    if as_float:
        q, t = q.astype(np.float32), t.astype(np.float32)
    else:
        assert min(q.min(initial=0), t.min(initial=0)) >= 0
        q, t = np.rint(q).astype(np.uint32), np.rint(t).astype(np.uint32)
    for arr in (q, t, good):
        arr.setflags(write=False)
    return q, t, good


def device_coords(torch, coords):
    a = np.ascontiguousarray(coords)
    if a.dtype == np.float32:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()


def device_scratch(torch, n_frames, q_cap, n_hyp, fill=0xA5):
    """A 256-byte aligned scratch tensor holding garbage: the call must not need it zeroed."""
    need = fast_hip.fundamental_scratch_bytes(n_frames, q_cap, n_hyp)
    raw = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 256
    return raw[lead:lead + need]


def upload(torch, matches, q_offs, q_coords, t_coords, t_offs, keep):
    d_m = torch.from_numpy(np.ascontiguousarray(matches).view(np.int32).reshape(-1, 2).copy()).cuda()
    d_q, d_t = device_coords(torch, q_coords), device_coords(torch, t_coords)
    d_qo = torch.from_numpy(np.asarray(q_offs).astype(np.int64)).cuda()
    d_to = torch.from_numpy(np.asarray(t_offs).astype(np.int64)).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.uint8).copy()).cuda()
    return d_m, d_qo, d_q, d_t, d_to, d_keep


def run_device(matches, q_offs, q_coords, t_coords, t_offs, n_hyp, threshold, seed, keep=None,
               q_cap=None, t_cap=None, scratch=None, stream=None):
    """fdf_fundamental_device on uploaded arrays -> ((F,) model records, the (q_cap + EXTRA,)
    inlier bytes); checks that the rows past the frames' models and the inputs are untouched."""
    import torch

    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    n = len(q_offs) - 1
    d_m, d_qo, d_q, d_t, d_to, d_keep = upload(torch, matches, q_offs, q_coords, t_coords, t_offs, keep)
    models = torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((q_cap + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    if scratch is None:
        scratch = device_scratch(torch, n, q_cap, n_hyp)
    fast_hip.fundamental_device(d_m[:q_cap], d_qo, d_q, d_t[:t_cap], d_to, models[:n], scratch,
                                keep=d_keep, inliers=inliers[:q_cap], n_hyp=n_hyp,
                                threshold=threshold, seed=seed, stream=stream)
    torch.cuda.synchronize()
    assert (models[n] == MODEL_FILL).all()
    assert np.array_equal(d_m.cpu().numpy().view(np.uint32).reshape(-1),
                          np.ascontiguousarray(matches).view(np.uint32).reshape(-1))
    return fast_hip.unpack_models(models[:n].cpu().numpy()), inliers.cpu().numpy()


def run_check(matches, q_offs, q_coords, t_coords, t_offs, models_in, threshold, keep=None,
              q_cap=None, t_cap=None, in_place=False):
    """fdf_fundamental_check_device on uploaded arrays, as run_device."""
    import torch

    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    n = len(q_offs) - 1
    d_m, d_qo, d_q, d_t, d_to, d_keep = upload(torch, matches, q_offs, q_coords, t_coords, t_offs, keep)
    given = np.ascontiguousarray(models_in[:n]).view(np.float64).reshape(n, 11)
    d_in = torch.from_numpy(given.copy()).cuda()
    out = torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    if in_place:
        out[:n] = d_in
    inliers = torch.full((q_cap + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    fast_hip.fundamental_check_device(d_m[:q_cap], d_qo, d_q, d_t[:t_cap], d_to,
                                      out[:n] if in_place else d_in, out[:n], keep=d_keep,
                                      inliers=inliers[:q_cap], threshold=threshold)
    torch.cuda.synchronize()
    assert (out[n] == MODEL_FILL).all()
    assert in_place or np.array_equal(d_in.cpu().numpy().view(np.uint64), given.view(np.uint64))
    return fast_hip.unpack_models(out[:n].cpu().numpy()), inliers.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(key):
    """The restatement's result of a registered case, computed once and shared."""
    matches, q_offs, q_coords, t_coords, t_offs, n_hyp, threshold, seed, keep, q_cap, t_cap = _CASES[key]
    return ref.fundamental(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs, n_hyp,
                           threshold, seed, inliers_out=np.full(q_cap + EXTRA, FILL, np.uint8))


_CASES = {}


def both(key, matches, q_offs, q_coords, t_coords, t_offs, n_hyp, threshold, seed, keep=None,
         q_cap=None, t_cap=None, **dev):
    """(device models, device bytes, reference models), device and restatement asserted equal bit
    for bit.  `key` names the case: its reference is computed once."""
    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    _CASES.setdefault(key, (matches, q_offs, q_coords, t_coords, t_offs, n_hyp, threshold, seed,
                            keep, q_cap, t_cap))
    got, got_in = run_device(matches, q_offs, q_coords, t_coords, t_offs, n_hyp, threshold, seed,
                             keep=keep, q_cap=q_cap, t_cap=t_cap, **dev)
    want, want_in = _reference(key)
    for f in range(len(want)):
        assert ref.models_bits_equal(got[f], want[f]), (f, got[f], want[f])
    assert np.array_equal(got_in, want_in)
    return got, got_in, want


# ---- 1: the worked example of include/fdf.h ----------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
def test_worked_example(dtype):
    q, t = ref.worked_example()
    got, mask, _ = both(("worked", dtype), ref.identity_matches(12), [0, 12], q.astype(dtype),
                        t.astype(dtype), [0, 12], 8, 0.5, 3)
    m = got[0]
    assert (m["hypothesis"], m["n_inliers"], m["n_valid"], m["n_corr"]) == (2, 10, 8, 12)
    assert m["h"][5] == 1.0 and float(m["h"][7]).hex() == "-0x1.ffffffffffffep-1"
    assert mask[:12].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0] and (mask[12:] == FILL).all()


# ---- 2: two-view scenes across the kernels' size boundaries -------------------------------------

SIZES = (0, 7, 8, 9, 64, TILE - 1, TILE, TILE + 1, 600)


@functools.lru_cache(maxsize=None)
def size_batch(as_float=False):
    """Frames of SIZES correspondences, a quarter of each re-drawn, over shared arrays."""
    parts = [two_views(m, m // 4, 100 + m, as_float) for m in SIZES]
    offs = np.cumsum([0] + list(SIZES))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), offs)


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 200])
def test_sizes(n_hyp):
    """Every M around the sample size and the LDS tile, every n_hyp around the block of 64: at
    most 9 x 4 = 36 blocks, the eight-wave kernel."""
    q, t, offs = size_batch()
    got, mask, _ = both(("sizes", n_hyp), ref.identity_matches(len(q)), offs, q, t, offs, n_hyp, 1.0,
                        11)
    assert got["n_corr"].tolist() == list(SIZES)
    assert (got["hypothesis"][:2] == ref.NONE).all() and not got["h"][:2].any()
    if n_hyp >= 63:
        assert (got["n_valid"][2:] > 0).all()
        assert (got["n_inliers"][4:] * 2 >= got["n_corr"][4:]).all()     # most of the true 3/4


def test_sizes_float_coordinates():
    q, t, offs = size_batch(True)
    got, _, _ = both("sizes-float", ref.identity_matches(len(q)), offs, q, t, offs, 64, 0.75, 5)
    assert (got["n_inliers"][4:] * 2 >= got["n_corr"][4:]).all()


def test_one_wave_kernel():
    """3 frames x 2752 hypotheses = 129 blocks, above the 128 up to which eight waves share a
    block's scoring: the one-wave kernel runs (every other test runs the eight-wave one)."""
    sizes = (9, 12, 3)
    parts = [two_views(m, 0, 300 + m) for m in sizes]
    q, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    offs = np.cumsum([0] + list(sizes))
    got, _, _ = both("one-wave", ref.identity_matches(len(q)), offs, q, t, offs, 2752, 1.0, 2)
    assert got["n_valid"][0] > 2000 and got["n_valid"][1] > 2000 and got["n_valid"][2] == 0
    assert got["n_inliers"][:2].tolist() == [9, 12]


# ---- 3: a batch with every way a query is not a correspondence -----------------------------------

def test_batch_of_frames():
    """Four frames over shared arrays: an empty one, one with M = 7 (no model), one whose matches
    hold FDF_MATCH_NONE, indices outside the train range and keep = 0, and one cut by q_cap.  The
    train array has one more leading point, so every train offset is the query's plus one."""
    n = (0, 7, 120, 90)
    parts = [two_views(n[1], 0, 31), two_views(n[2], 30, 32), two_views(n[3], 20, 33)]
    q = np.concatenate([p[0] for p in parts])
    t = np.concatenate([[(5, 5)]] + [p[1] for p in parts]).astype(np.uint32)
    q_offs = np.cumsum([0] + list(n))
    t_offs = q_offs + 1
    matches = ref.identity_matches(len(q))
    matches["index"] += 1
    lo = q_offs[2]
    matches["index"][lo + 5] = ref.NONE
    matches["index"][lo + 6] = 2                               # frame 1's train point
    matches["index"][lo + 7] = t_offs[3] + 2                   # frame 3's
    matches["index"][lo + 8] = len(t) + 1000                   # beyond the array
    matches["index"][lo + 9] = lo + 9 + 2                      # a wrong but legal train point
    keep = np.ones(len(q), np.uint8)
    keep[lo + 20:lo + 25] = 0
    keep[q_offs[3] + 4] = 0
    q_cap = len(q) - 10                                        # cuts the last frame
    got, mask, _ = both("batch", matches, q_offs, q, t, t_offs, 128, 1.0, 5, keep=keep, q_cap=q_cap)
    assert got["n_corr"].tolist() == [0, 7, 120 - 4 - 5, 90 - 10 - 1]
    assert (got["hypothesis"][:2] == ref.NONE).all() and not got["h"][:2].any()
    assert mask[lo + 5:lo + 9].tolist() == [0] * 4 and not mask[lo + 20:lo + 25].any()
    assert got[2]["n_inliers"] >= 60 and got[3]["n_inliers"] >= 44
    # a train capacity that cuts frame 3's train range
    both("batch-tcap", matches, q_offs, q, t, t_offs, 64, 1.0, 5, keep=keep, t_cap=len(t) - 30)


# ---- 4: ground truth, not only self-agreement ------------------------------------------------------

def test_scene_a_exact():
    q, t, true = ref.scene_a(0)
    got, mask, _ = both("scene-a", ref.identity_matches(200), [0, 200], q, t, [0, 200], 256,
                        2.0 ** -7, 0)
    mask = mask[:200].astype(bool)
    assert mask[true].all() and not mask[~true].any() and got[0]["n_inliers"] == 140


def test_scene_a_noisy():
    q, t, true = ref.scene_a(0, noise=0.3)
    _, mask, _ = both("scene-a-noisy", ref.identity_matches(200), [0, 200], q, t, [0, 200], 256,
                      1.0, 3)
    mask = mask[:200].astype(bool)
    assert mask[true].all() and mask[~true].sum() <= 3


def test_scene_b_rectified_pair_and_the_rig_matrix():
    q, t, true = ref.scene_b(0)
    m = ref.identity_matches(100)
    got, mask, _ = both("scene-b", m, [0, 100], q, t, [0, 100], 64, 0.5, 0)
    mask = mask[:100].astype(bool)
    assert mask[true].all() and not mask[~true].any() and got[0]["n_inliers"] == 80
    f = got[0]["h"] * np.sign(got[0]["h"][5])
    assert np.allclose(f, [0, 0, 0, 0, 0, 1, 0, -1, 0], rtol=0, atol=2.0 ** -30)
    # fdf_fundamental_check_device with the rig's own matrix: exactly the pairs on one row
    rig = np.zeros(1, dtype=ref.MODEL_DTYPE)
    rig["h"][0] = [0, 0, 0, 0, 0, 1, 0, -1, 0]
    rig["hypothesis"], rig["n_valid"], rig["n_corr"] = 7, 3, 999
    out, bytes_ = run_check(m, [0, 100], q, t, [0, 100], rig, 0.5)
    want, want_bytes = ref.check(m, None, 100, [0, 100], q, t, 100, [0, 100], rig, 0.5,
                                 inliers_out=np.full(100 + EXTRA, FILL, np.uint8))
    assert ref.models_bits_equal(out[0], want[0]) and np.array_equal(bytes_, want_bytes)
    dy = np.abs(t[:, 1].astype(np.int64) - q[:, 1].astype(np.int64))
    assert np.array_equal(bytes_[:100].astype(bool), dy <= 0.5)
    assert (out[0]["n_corr"], out[0]["n_inliers"], out[0]["hypothesis"], out[0]["n_valid"]) == \
        (100, 80, 7, 3)


def test_scene_c_plane_has_no_model():
    q, t = ref.scene_c(0)
    got, mask, _ = both("scene-c", ref.identity_matches(60), [0, 60], q, t, [0, 60], 64, 0.5, 0)
    assert got[0]["n_valid"] == 0 and got[0]["hypothesis"] == ref.NONE
    assert got[0]["n_corr"] == 60 and not got[0]["h"].any() and not mask[:60].any()


# ---- 5: fdf_fundamental_check_device ---------------------------------------------------------------

@pytest.mark.parametrize("in_place", [False, True])
def test_check_reproduces_the_estimate(in_place):
    """The estimator's own models and threshold: its counts and bytes again, over the batch with
    every kind of non-correspondence; then another threshold against the restatement."""
    q, t, offs = size_batch()
    m = ref.identity_matches(len(q))
    keep = np.ones(len(q), np.uint8)
    keep[::7] = 0
    got, mask, _ = both("check-src", m, offs, q, t, offs, 64, 1.0, 4, keep=keep)
    again, mask2 = run_check(m, offs, q, t, offs, got, 1.0, keep=keep, in_place=in_place)
    assert again.tobytes() == got.tobytes() and np.array_equal(mask, mask2)
    wide, wide_mask = run_check(m, offs, q, t, offs, got, 2.5, keep=keep, in_place=in_place)
    want, want_mask = ref.check(m, keep, len(q), offs, q, t, len(q), offs, got, 2.5,
                                inliers_out=np.full(len(q) + EXTRA, FILL, np.uint8))
    assert wide.tobytes() == want.tobytes() and np.array_equal(wide_mask, want_mask)
    assert (wide["n_inliers"] >= got["n_inliers"]).all() and wide["n_inliers"].sum() > got["n_inliers"].sum()


# ---- 6: degenerate data ------------------------------------------------------------------------------

def test_identical_and_collinear_points_have_no_model():
    same = np.full((20, 2), 33, dtype=np.uint32)
    line = np.stack([np.arange(20) * 7, np.arange(20) * 14 + 3], axis=1).astype(np.uint32)
    for name, q in (("same", same), ("line", line)):
        got, mask, _ = both(("degenerate", name), ref.identity_matches(20), [0, 20], q, q, [0, 20],
                            64, 1.0, 0)
        assert got[0]["n_valid"] == 0 and got[0]["hypothesis"] == ref.NONE
        assert got[0]["n_corr"] == 20 and not got[0]["h"].any() and not mask[:20].any()


def test_nan_and_infinity():
    """NaNs and infinities among float coordinates: a NaN is never an inlier (an infinity can be:
    the rule's inf <= inf), the model is finite, and nothing is written outside the ranges
    (run_device's checks)."""
    q, t, _ = two_views(64, 0, 51, True)
    qf, tf = q.copy(), t.copy()
    qf[7, 0] = np.nan
    tf[9, 1] = np.nan
    qf[20, 1] = np.inf
    tf[33, 0] = -np.inf
    got, mask, _ = both("nan", ref.identity_matches(64), [0, 64], qf, tf, [0, 64], 128, 1.0, 3)
    assert mask[[7, 9]].tolist() == [0, 0] and mask[:64].sum() == got[0]["n_inliers"]
    assert 0 < got[0]["n_valid"] < 128 and 60 <= got[0]["n_inliers"] <= 62
    assert np.isfinite(got[0]["h"]).all()
    # every coordinate a NaN: no model
    bad = np.full((16, 2), np.nan, dtype=np.float32)
    got, mask, _ = both("all-nan", ref.identity_matches(16), [0, 16], bad, bad, [0, 16], 64, 1.0, 0)
    assert got[0]["hypothesis"] == ref.NONE and not got[0]["h"].any() and not mask[:16].any()


# ---- 7: determinism, streams, scratch reuse --------------------------------------------------------

def test_same_call_twice_and_on_another_stream():
    import torch

    q, t, offs = size_batch()
    m = ref.identity_matches(len(q))
    args = (m, offs, q, t, offs, 65, 1.0, 9)
    first = run_device(*args)
    scratch = device_scratch(torch, len(offs) - 1, len(q), 65, fill=0x3C)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        second = run_device(*args, scratch=scratch, stream=stream)
        other = run_device(m, offs, q, t, offs, 65, 1.0, 10, scratch=scratch, stream=stream)
        third = run_device(*args, scratch=scratch, stream=stream)
    for again in (second, third):
        assert first[0].tobytes() == again[0].tobytes() and np.array_equal(first[1], again[1])
    assert first[0].tobytes() != other[0].tobytes()


# ---- 8: argument errors from the C ABI -------------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    n = 32
    pts = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, n], dtype=torch.int64, device="cuda")
    matches = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    models = torch.full((3, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    given = torch.zeros((3, 11), dtype=torch.float64, device="cuda")
    inliers = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    scratch = device_scratch(torch, 2, n, 16)
    lib = _native.load()
    good = dict(ctx=fast_hip.context(0).handle, n=2, m=matches.data_ptr(), keep=None, qcap=n,
                qo=offs.data_ptr(), q=pts.data_ptr(), t=pts.data_ptr(), tcap=n, to=offs.data_ptr(),
                coords=0, n_hyp=16, thr=1.0, out=models.data_ptr(), inl=inliers.data_ptr(),
                s=scratch.data_ptr(), sb=scratch.numel(), given=given.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return lib.fdf_fundamental_device(a["ctx"], a["n"], a["m"], a["keep"], a["qcap"], a["qo"],
                                          a["q"], a["t"], a["tcap"], a["to"], a["coords"],
                                          a["n_hyp"], a["thr"], 0, a["out"], a["inl"], a["s"],
                                          a["sb"], None)

    def check(**kw):
        a = {**good, **kw}
        return lib.fdf_fundamental_check_device(a["ctx"], a["n"], a["m"], a["keep"], a["qcap"],
                                                a["qo"], a["q"], a["t"], a["tcap"], a["to"],
                                                a["coords"], a["given"], a["thr"], a["out"],
                                                a["inl"], None)

    shared = (dict(ctx=None), dict(m=None), dict(qo=None), dict(q=None), dict(t=None),
              dict(to=None), dict(out=None), dict(n=65536), dict(qcap=0xFFFFFFFF),
              dict(tcap=0xFFFFFFFF), dict(qcap=1 << 40), dict(coords=2), dict(thr=-1.0),
              dict(thr=float("nan")), dict(thr=float("inf")), dict(m=matches.data_ptr() + 4),
              dict(q=pts.data_ptr() + 4), dict(t=pts.data_ptr() + 4),
              dict(out=models.data_ptr() + 4))
    for bad in shared + (dict(s=None), dict(n_hyp=0), dict(n_hyp=65537),
                         dict(s=scratch.data_ptr() + 128), dict(sb=scratch.numel() - 1),
                         dict(n_hyp=200)):                      # the scratch is one for 16
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    for bad in shared + (dict(given=None), dict(given=given.data_ptr() + 4)):
        assert check(**bad) == _native.FDF_ERR_ARG, bad
    assert call(n=0, m=None, out=None, s=None) == _native.FDF_OK
    assert check(n=0, m=None, out=None, given=None) == _native.FDF_OK
    # fdf_ransac_device knows no third model
    assert lib.fdf_ransac_device(good["ctx"], 2, good["m"], None, n, good["qo"], good["q"], good["t"],
                                 n, good["to"], 0, 2, 16, 1.0, 0, good["out"], good["inl"], good["s"],
                                 good["sb"], None) == _native.FDF_ERR_ARG
    torch.cuda.synchronize()
    assert (models == MODEL_FILL).all() and (inliers == FILL).all()
    # the good call works, on the null stream: all-zero points are no model, and frame 1's
    # matches (index 0) lie outside its train range
    assert call() == _native.FDF_OK
    torch.cuda.synchronize()
    got = fast_hip.unpack_models(models[:2].cpu().numpy())
    assert got["n_corr"].tolist() == [16, 0] and (got["hypothesis"] == ref.NONE).all()
    assert (models[2] == MODEL_FILL).all() and (inliers == 0).all()
    # and so does the check, whose all-zero records count as models: g = 0, no inlier
    inliers.fill_(FILL)
    assert check() == _native.FDF_OK
    torch.cuda.synchronize()
    got = fast_hip.unpack_models(models[:2].cpu().numpy())
    assert got["n_corr"].tolist() == [16, 0] and got["n_inliers"].tolist() == [0, 0]
    assert (models[2] == MODEL_FILL).all() and (inliers == 0).all()


# ---- 9: chained with the tracker and the track set ---------------------------------------------------

TRACK = dict(radius=4, max_iters=10, eps=20, min_eig=0.5)


def test_track_fundamental_update_chain():
    """track_device -> fundamental_device -> tracks_update_device on one stream with nothing in
    between, the tracker's matches, status and float positions going in as they are and the
    inlier bytes as the track status; every step against the chained restatements."""
    import torch

    frames = np.ascontiguousarray(ts.moved(ts.texture(9, 104, 88), 64, 48, [(2, 1)]))
    h, w = frames.shape[1:]
    levels = [rs.pyramid(fr, 2, 2, 1) for fr in frames]
    xs, ys = np.meshgrid(np.linspace(6, w - 7, 6).astype(np.int64), np.linspace(6, h - 7, 4).astype(np.int64))
    pts = np.concatenate([np.stack([xs.ravel(), ys.ravel()], axis=1), [[0, 0], [62, 2]]])
    n, n_hyp, out_cap = len(pts), 64, 64
    cand = np.array([(10, 10), (30, 20), (50, 40), (20, 35)])
    scores = np.array([9, 8, 7, 6])

    def i32(a, dtype=np.int32):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()

    d_frames = torch.from_numpy(frames).cuda()
    pyr = fast_hip.Pyramid(d_frames, 2, (2, 1))
    d_pts, d_ptsf = i32(pts), i32(pts, np.float32)
    d_offs = i32([0, n], np.int64)
    q11 = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    xy = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    models = torch.full((2, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((n + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    scratch = device_scratch(torch, 1, n, n_hyp)
    ids, ages = i32(np.arange(n) + 500), i32(np.zeros(n))
    d_cand, d_scores, d_coffs = i32(cand), i32(scores, np.int16), i32([0, len(cand)], np.int64)
    next_id = i32([900])
    out = {k: torch.zeros((out_cap,) + s, dtype=torch.int32, device="cuda")
           for k, s in (("q11", (2,)), ("ids", ()), ("ages", ()), ("src", ()))}
    out_offs = torch.zeros(2, dtype=torch.int64, device="cuda")
    update = dict(min_dist=6, margin=3, max_tracks=40, passes=8)
    tracks_scratch = torch.zeros(fast_hip.tracks_scratch_bytes(1, (h, w), 6, n, len(cand)) + 1,
                                 dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.track_device(pyr, pyr, d_pts, d_offs, q11, status, prev_first=0, next_first=1,
                              n_frames=1, next_xy=xy, matches=matches, **TRACK)
        fast_hip.fundamental_device(matches, d_offs, d_ptsf, xy, d_offs, models[:1], scratch,
                                    keep=status, inliers=inliers[:n], n_hyp=n_hyp, threshold=1.0,
                                    seed=6)
        fast_hip.tracks_update_device(q11, ids, ages, d_offs, d_cand, d_scores, d_coffs, next_id,
                                      out["q11"], out["ids"], out["ages"], out_offs, (h, w),
                                      track_status=inliers[:n], out_src=out["src"],
                                      scratch=tracks_scratch, **update)
    stream.synchronize()

    tracked = tr.track(levels[0:1], levels[1:2], pts, [0, n], n, **TRACK)
    assert np.array_equal(q11.cpu().numpy(), tracked["q11"])
    assert np.array_equal(status.cpu().numpy(), tracked["status"]) and tracked["status"].sum() >= 8
    assert np.array_equal(xy.cpu().numpy(), tracked["f32"])
    rec = tracked["matches"].view(ref.identity_matches(1).dtype).reshape(-1)
    want, want_in = ref.fundamental(rec, tracked["status"], n, [0, n], pts.astype(np.float32),
                                    tracked["f32"], n, [0, n], n_hyp, 1.0, 6,
                                    inliers_out=np.full(n + EXTRA, FILL, np.uint8))
    got = fast_hip.unpack_models(models.cpu().numpy()[:1])
    assert ref.models_bits_equal(got[0], want[0]) and (models[1] == MODEL_FILL).all()
    assert got[0]["n_corr"] == tracked["status"].sum()
    assert np.array_equal(inliers.cpu().numpy(), want_in)
    upd = ts.update(tracked["q11"], want_in[:n], np.arange(n) + 500, np.zeros(n), [0, n], n, cand,
                    scores, [0, len(cand)], len(cand), [900], w, h, 6, 3, 40, 8)
    total = int(upd["offsets"][-1])
    assert np.array_equal(out_offs.cpu().numpy().view(np.uint64), upd["offsets"]) and total <= out_cap
    for k in ("q11", "ids", "ages", "src"):
        assert out[k][:total].cpu().numpy().tobytes() == upd[k].tobytes(), k


# ---- 10: the host entries ----------------------------------------------------------------------------

def test_host_entry_agrees_with_the_device_entry():
    q, t, true = ref.scene_a(0)
    matches = ref.identity_matches(200)
    matches["index"][11] = ref.NONE
    keep = np.ones(200, np.uint8)
    keep[[2, 3]] = 0
    dev, dev_in = run_device(matches, [0, 200], q, t, [0, 200], 100, 0.25, 6, keep=keep)
    F, mask, rec = fast_hip.estimate_fundamental(q, t, matches, keep=keep, n_hyp=100,
                                                 threshold=0.25, seed=6)
    assert ref.models_bits_equal(rec, dev[0]) and np.array_equal(mask, dev_in[:200].astype(bool))
    assert F.shape == (3, 3) and np.array_equal(F.reshape(-1), rec["h"])
    assert rec["n_corr"] == 197 and mask.dtype == np.bool_ and rec["n_inliers"] >= 100
    # integer points, train indices instead of records, no keep
    qi, ti, _ = ref.scene_b(0)
    Fi, maski, reci = fast_hip.estimate_fundamental(qi, ti, np.arange(100), n_hyp=64,
                                                    threshold=0.5, seed=0)
    want, want_in = _reference("scene-b") if "scene-b" in _CASES else ref.fundamental(
        ref.identity_matches(100), None, 100, [0, 100], qi, ti, 100, [0, 100], 64, 0.5, 0)
    assert ref.models_bits_equal(reci, want[0]) and np.array_equal(maski, want_in[:100].astype(bool))
    # no model: F is None
    F, mask, rec = fast_hip.estimate_fundamental(q[:7], t, matches[:7])
    assert F is None and not mask.any() and rec["n_corr"] == 7 and rec["hypothesis"] == ref.NONE
    F, mask, rec = fast_hip.estimate_fundamental(q[:0], t, matches[:0])
    assert F is None and len(mask) == 0 and rec["n_corr"] == 0 and rec["hypothesis"] == ref.NONE


def test_cpp_fundamental_binary():
    """The C++ binary prints the worked example's result as hexadecimal doubles: the device
    entry's bits."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_fundamental")
    assert os.path.exists(exe), "run `make` first"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
    q, t = ref.worked_example()
    got, _ = run_device(ref.identity_matches(12), [0, 12], q, t, [0, 12], 8, 0.5, 3)
    line = next(l for l in res.stdout.splitlines() if l.startswith("hypothesis="))
    assert line.startswith("hypothesis=2 inliers=10/12 valid=8 f=")
    printed = [float.fromhex(v) for v in line.split("f=")[1].split()]
    assert np.array_equal(np.array(printed).view(np.uint64),
                          np.ascontiguousarray(got[0]["h"]).view(np.uint64))
