"""RANSAC model estimation on the device (fdf_ransac_device, fdf_ransac_points) against the numpy
restatement of include/fdf.h's contract in tests/_ransac_reference.py.  Every comparison is exact
(the model's doubles with ==, NaN equal to NaN, the sign of a zero free); the inlier bytes and the
models are pre-filled and over-allocated so that what no frame owns can be checked as untouched."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import _match_reference as mref
import _ransac_reference as ref
import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A                                        # of the inlier bytes
MODEL_FILL = -7.25                                 # of the models' 11 doubles
EXTRA = 16                                         # rows past the capacity
TILE = 256                                         # correspondences of the kernel's LDS tile
MODELS = {"affine": ref.AFFINE, "homography": ref.HOMOGRAPHY}

# three mild planted transforms; every projected coordinate of a query below 1800 stays below 2048
PLANTED = (np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, 40.0], [1e-5, -2e-5, 1.0]]),
           np.array([[0.95, -0.05, 90.0], [0.04, 1.01, 3.0], [-1e-5, 1e-5, 1.0]]),
           np.array([[1.0, 0.0, 17.0], [0.0, 1.0, 9.0], [0.0, 0.0, 1.0]]))


@functools.lru_cache(maxsize=None)
def planted(m, outliers, seed, which=0):
    """(queries, trains, planted inlier flags): `m` random integer points, their rounded
    projections, and `outliers` of the trains re-drawn uniformly.  Read-only."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1800, (m, 2)).astype(np.uint32)
    p = np.c_[q.astype(np.float64), np.ones(m)] @ PLANTED[which].T
    t = np.rint(p[:, :2] / p[:, 2:]).astype(np.int64)
    assert t.min(initial=0) >= 0 and t.max(initial=0) < 2048
    t = t.astype(np.uint32)
    good = np.ones(m, dtype=bool)
    bad = rng.permutation(m)[:outliers]
    t[bad] = rng.integers(0, 2048, (len(bad), 2))
    good[bad] = False
    for a in (q, t, good):
        a.setflags(write=False)
    return q, t, good


def device_coords(torch, coords):
    a = np.ascontiguousarray(coords)
    if a.dtype == np.float32:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()


def device_scratch(torch, n_frames, q_cap, n_hyp, fill=0xA5):
    """A 256-byte aligned scratch tensor holding garbage: the call must not need it zeroed."""
    need = fast_hip.ransac_scratch_bytes(n_frames, q_cap, n_hyp)
    raw = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 256
    return raw[lead:lead + need]


def run_ransac(matches, q_offs, q_coords, t_coords, t_offs, model, n_hyp, threshold, seed,
               keep=None, q_cap=None, t_cap=None, scratch=None, stream=None):
    """fdf_ransac_device on uploaded arrays -> ((F,) model records, the (q_cap + EXTRA,) inlier
    bytes); checks that the rows past the frames' models and the inputs are untouched."""
    import torch

    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    n = len(q_offs) - 1
    d_m = torch.from_numpy(np.ascontiguousarray(matches).view(np.int32).reshape(-1, 2).copy()).cuda()
    d_q, d_t = device_coords(torch, q_coords), device_coords(torch, t_coords)
    d_qo = torch.from_numpy(np.asarray(q_offs).astype(np.int64)).cuda()
    d_to = torch.from_numpy(np.asarray(t_offs).astype(np.int64)).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.uint8).copy()).cuda()
    models = torch.full((n + 1, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((q_cap + EXTRA,), FILL, dtype=torch.uint8, device="cuda")
    if scratch is None:
        scratch = device_scratch(torch, n, q_cap, n_hyp)
    fast_hip.ransac_device(d_m[:q_cap], d_qo, d_q, d_t[:t_cap], d_to, models[:n], scratch,
                           keep=d_keep, inliers=inliers[:q_cap], model=model, n_hyp=n_hyp,
                           threshold=threshold, seed=seed, stream=stream)
    torch.cuda.synchronize()
    assert (models[n] == MODEL_FILL).all()
    assert np.array_equal(d_m.cpu().numpy().view(np.uint32).reshape(-1),
                          np.ascontiguousarray(matches).view(np.uint32).reshape(-1))
    return fast_hip.unpack_models(models[:n].cpu().numpy()), inliers.cpu().numpy()


def reference(matches, q_offs, q_coords, t_coords, t_offs, model, n_hyp, threshold, seed,
              keep=None, q_cap=None, t_cap=None):
    q_cap = len(matches) if q_cap is None else q_cap
    t_cap = len(t_coords) if t_cap is None else t_cap
    return ref.ransac(matches, keep, q_cap, q_offs, q_coords, t_coords, t_cap, t_offs,
                      MODELS[model], n_hyp, threshold, seed,
                      inliers_out=np.full(q_cap + EXTRA, FILL, np.uint8))


def both(*args, **kw):
    """(device models, device bytes, reference models, reference bytes), asserted equal."""
    dev = {k: kw.pop(k) for k in ("scratch", "stream") if k in kw}
    got, got_in = run_ransac(*args, **kw, **dev)
    want, want_in = reference(*args, **kw)
    for f in range(len(want)):
        assert ref.models_equal(got[f], want[f]), (f, got[f], want[f])
    assert np.array_equal(got_in, want_in)
    return got, got_in, want, want_in


# ---- 1: the worked example of include/fdf.h ----------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
def test_worked_example(model, dtype):
    q, t = ref.worked_example()
    got, mask, _, _ = both(ref.identity_matches(6), [0, 6], q.astype(dtype), t.astype(dtype), [0, 6],
                           model, 8, 1.0, 0)
    m = got[0]
    assert (m["hypothesis"], m["n_inliers"], m["n_valid"], m["n_corr"]) == (3, 5, 8, 6)
    assert m["h"].tolist() == [1, 0, 3, 0, 1, 5, 0, 0, 1]
    assert mask[:6].tolist() == [1, 1, 1, 1, 0, 1] and (mask[6:] == FILL).all()


# ---- 2: planted homographies across the kernels' size boundaries --------------------------------

SIZES = (4, 5, 63, 64, 65, TILE + 1, 300)


@functools.lru_cache(maxsize=None)
def size_batch():
    """Frames of SIZES correspondences, a third of each re-drawn, over shared arrays."""
    parts = [planted(m, m // 3, 100 + m) for m in SIZES]
    offs = np.cumsum([0] + list(SIZES))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), offs,
            np.concatenate([p[2] for p in parts]))


@pytest.mark.parametrize("model", ["affine", "homography"])
@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 257, 1217])
def test_planted_sizes(model, n_hyp):
    """n_hyp = 1217 is 7 frames x 20 hypothesis blocks: above the 128 blocks up to which eight waves
    share a block's scoring, so the one-wave kernel runs; the smaller ones run the shared one."""
    q, t, offs, _ = size_batch()
    got, _, _, _ = both(ref.identity_matches(len(q)), offs, q, t, offs, model, n_hyp, 3.0, 11)
    assert got["n_corr"].tolist() == list(SIZES)
    if n_hyp >= 63 and model == "homography":
        assert (got["n_inliers"][2:] * 2 >= got["n_corr"][2:]).all()     # the planted two thirds


@pytest.mark.parametrize("n_hyp", [8192, 8193])
def test_grid_width_threshold(n_hyp):
    """One frame with 128 and with 129 hypothesis blocks: the last grid of the eight-wave kernel
    and the first of the one-wave kernel."""
    q, t, _ = planted(65, 20, 61)
    got = both(ref.identity_matches(65), [0, 65], q, t, [0, 65], "homography", n_hyp, 3.0, 2)[0]
    assert got[0]["n_inliers"] >= 45 and got[0]["n_valid"] > n_hyp // 2


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_planted_inliers_are_all_found(model):
    """300 matches, half of them outliers, 256 hypotheses: the reference alone finds every planted
    inlier, so the device must too (agreeing garbage cannot pass)."""
    q, t, good = planted(300, 150, 7, which=2 if model == "affine" else 0)
    got, mask, _, _ = both(ref.identity_matches(300), [0, 300], q, t, [0, 300], model, 256, 3.0, 0)
    assert good.sum() == 150 and got[0]["n_inliers"] >= 150
    assert mask[:300][good].all()


def test_float_coordinates_and_seeds():
    """The same planted data as floats with half-pixel offsets; another seed is another result."""
    q, t, _ = planted(300, 100, 8)
    qf, tf = q.astype(np.float32) + np.float32(0.5), t.astype(np.float32) + np.float32(0.25)
    m = ref.identity_matches(300)
    a = both(m, [0, 300], qf, tf, [0, 300], "homography", 128, 2.5, 1)[0]
    b = both(m, [0, 300], qf, tf, [0, 300], "homography", 128, 2.5, 2)[0]
    assert a[0]["n_inliers"] >= 150 and b[0]["n_inliers"] >= 150
    assert not np.array_equal(a[0]["h"], b[0]["h"])


# ---- 3: a batch with every way a query is not a correspondence -----------------------------------

def test_batch_of_frames():
    """Four frames over shared arrays: an empty one, one with M = 3 (an affine, no homography),
    one whose matches hold FDF_MATCH_NONE, indices outside the train range and keep = 0, and one
    cut by q_cap; each with its own planted transform."""
    n = (0, 3, 120, 90)
    parts = [planted(n[1], 0, 31, 2), planted(n[2], 30, 32, 0), planted(n[3], 20, 33, 1)]
    q = np.concatenate([p[0] for p in parts])
    t = np.concatenate([p[1] for p in parts])
    q_offs = np.cumsum([0] + list(n))
    matches = ref.identity_matches(len(q))
    lo = q_offs[2]
    matches["index"][lo + 5] = ref.NONE
    matches["index"][lo + 6] = 1                               # frame 1's train point
    matches["index"][lo + 7] = q_offs[3] + 2                   # frame 3's
    matches["index"][lo + 8] = len(q) + 1000                   # beyond the array
    matches["index"][lo + 9] = lo + 9 + 1                      # a wrong but legal train point
    keep = np.ones(len(q), np.uint8)
    keep[lo + 20:lo + 25] = 0
    keep[q_offs[3] + 4] = 0
    q_cap = len(q) - 10                                        # cuts the last frame
    for model in ("affine", "homography"):
        got, mask, _, _ = both(matches, q_offs, q, t, q_offs, model, 128, 3.0, 5, keep=keep,
                               q_cap=q_cap)
        assert got["n_corr"].tolist() == [0, 3, 120 - 4 - 5, 90 - 10 - 1]
        assert got[0]["hypothesis"] == ref.NONE and not got[0]["h"].any()
        assert (got[1]["hypothesis"] != ref.NONE) == (model == "affine")
        assert mask[lo + 5:lo + 9].tolist() == [0] * 4 and not mask[lo + 20:lo + 25].any()
        # the frames' models are their own: frame 1's is the translation (17, 9)
        if model == "affine":              # exact data, coordinates below 2^11: far inside 2^-30
            assert np.allclose(got[1]["h"], [1, 0, 17, 0, 1, 9, 0, 0, 1], rtol=0, atol=2.0 ** -30)
        # at least 81 and 59 planted inliers are left in frames 2 and 3: most of them are found,
        # which a model of the neighbouring frame (another transform) would not do
        # (the planted transforms are no affine maps)
        if model == "homography":
            assert got[2]["n_inliers"] >= 60 and got[3]["n_inliers"] >= 44
    # a train capacity that cuts frame 3's train range, and separate train offsets
    t_offs = q_offs + np.array([0, 0, 0, 0, 50])
    both(matches, q_offs, q, t, t_offs, "homography", 64, 3.0, 5, t_cap=len(t) - 30)


# ---- 4: degenerate data --------------------------------------------------------------------------

def test_collinear_points_have_no_model():
    q = np.stack([np.arange(20) * 7, np.arange(20) * 14 + 3], axis=1).astype(np.uint32)
    for model in ("affine", "homography"):
        got, mask, _, _ = both(ref.identity_matches(20), [0, 20], q, q, [0, 20], model, 64, 3.0, 0)
        assert got[0]["n_valid"] == 0 and got[0]["hypothesis"] == ref.NONE
        assert got[0]["n_corr"] == 20 and not got[0]["h"].any() and not mask[:20].any()


def test_repeated_points():
    """The same four points three times: only samples of four different points are valid."""
    q = np.array([(0, 0), (100, 0), (0, 100), (100, 120)] * 3, dtype=np.uint32)
    got, mask, _, _ = both(ref.identity_matches(12), [0, 12], q, q, [0, 12], "homography", 64, 3.0, 0)
    assert (got[0]["n_valid"], got[0]["n_inliers"]) == (12, 12) and mask[:12].all()


def test_two_queries_on_one_train_point():
    q, t, _ = planted(40, 0, 41, 2)
    matches = ref.identity_matches(40)
    matches["index"][[3, 4, 5]] = 3
    got, mask, _, _ = both(matches, [0, 40], q, t, [0, 40], "homography", 64, 1.0, 0)
    assert got[0]["n_inliers"] == 38 and mask[:6].tolist() == [1, 1, 1, 1, 0, 0]


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_nan_and_infinity(model):
    """A NaN and an infinity among float coordinates: never inliers, and nothing faults."""
    q, t, _ = planted(64, 0, 51, 2)
    qf, tf = q.astype(np.float32), t.astype(np.float32)
    qf[7, 0] = np.nan
    tf[9, 1] = np.nan
    qf[20, 1] = np.inf
    tf[33, 0] = -np.inf
    got, mask, _, _ = both(ref.identity_matches(64), [0, 64], qf, tf, [0, 64], model, 128, 2.0, 3)
    assert mask[[7, 9, 20, 33]].tolist() == [0, 0, 0, 0]
    assert got[0]["n_inliers"] == 60 and 0 < got[0]["n_valid"] < 128
    assert np.isfinite(got[0]["h"]).all()


# ---- 5: determinism, streams, scratch reuse --------------------------------------------------------

def test_same_call_twice_and_on_another_stream():
    import torch

    q, t, offs, _ = size_batch()
    m = ref.identity_matches(len(q))
    args = (m, offs, q, t, offs, "homography", 65, 3.0, 9)
    first = run_ransac(*args)
    scratch = device_scratch(torch, len(offs) - 1, len(q), 65, fill=0x3C)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        second = run_ransac(*args, scratch=scratch, stream=stream)
        other = run_ransac(m, offs, q, t, offs, "affine", 65, 3.0, 9, scratch=scratch,
                           stream=stream)
        third = run_ransac(*args, scratch=scratch, stream=stream)
    for again in (second, third):
        assert first[0].tobytes() == again[0].tobytes() and np.array_equal(first[1], again[1])
    assert first[0].tobytes() != other[0].tobytes()


# ---- 6: argument errors from the C ABI -------------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    n = 32
    pts = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, n], dtype=torch.int64, device="cuda")
    matches = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    models = torch.full((3, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    scratch = device_scratch(torch, 2, n, 16)
    lib = _native.load()
    good = dict(ctx=fast_hip.context(0).handle, n=2, m=matches.data_ptr(), keep=None, qcap=n,
                qo=offs.data_ptr(), q=pts.data_ptr(), t=pts.data_ptr(), tcap=n, to=offs.data_ptr(),
                coords=0, model=1, n_hyp=16, thr=3.0, out=models.data_ptr(),
                inl=inliers.data_ptr(), s=scratch.data_ptr(), sb=scratch.numel())

    def call(**kw):
        a = {**good, **kw}
        return lib.fdf_ransac_device(a["ctx"], a["n"], a["m"], a["keep"], a["qcap"], a["qo"], a["q"],
                                     a["t"], a["tcap"], a["to"], a["coords"], a["model"],
                                     a["n_hyp"], a["thr"], 0, a["out"], a["inl"], a["s"], a["sb"],
                                     None)

    for bad in (dict(ctx=None), dict(m=None), dict(qo=None), dict(q=None), dict(t=None),
                dict(to=None), dict(out=None), dict(s=None), dict(n=65536), dict(qcap=0xFFFFFFFF),
                dict(tcap=0xFFFFFFFF), dict(qcap=1 << 40), dict(n_hyp=0), dict(n_hyp=65537),
                dict(coords=2), dict(model=2), dict(thr=-1.0), dict(thr=float("nan")),
                dict(thr=float("inf")), dict(m=matches.data_ptr() + 4), dict(q=pts.data_ptr() + 4),
                dict(t=pts.data_ptr() + 4), dict(out=models.data_ptr() + 4),
                dict(s=scratch.data_ptr() + 128), dict(sb=scratch.numel() - 1),
                dict(n_hyp=200)):                               # the scratch is one for 16
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(n=0, m=None, out=None, s=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (models == MODEL_FILL).all() and (inliers == FILL).all()
    # the good call works, on the null stream: all-zero points are no model, and frame 1's
    # matches (index 0) lie outside its train range
    assert call() == _native.FDF_OK
    torch.cuda.synchronize()
    got = fast_hip.unpack_models(models[:2].cpu().numpy())
    assert got["n_corr"].tolist() == [16, 0] and (got["hypothesis"] == ref.NONE).all()
    assert (models[2] == MODEL_FILL).all() and (inliers == 0).all()


# ---- 7: end to end ---------------------------------------------------------------------------------

def test_device_chain():
    """detect -> orient -> smooth -> describe -> match both ways -> filter (ratio and cross-check)
    -> RANSAC on one stream with nothing in between: the second frame is the first moved by
    (3, 2), and that is the translation the model holds."""
    import torch

    img = workloads.golden_image()
    h, w = img.shape
    shifted = np.pad(img, ((2, 0), (3, 0)), mode="edge")[:h, :w]
    frames = torch.from_numpy(np.stack([img, shifted])).cuda()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap, n_bins, window, n_hyp = 1024, 30, (12, 10), 128
    pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(3, dtype=torch.int64, device="cuda")
    ang = torch.zeros(cap, dtype=torch.float32, device="cuda")
    smoothed = torch.zeros_like(frames)
    desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)).cuda()
    fwd = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    rev = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    keep = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    models = torch.full((2, 11), MODEL_FILL, dtype=torch.float64, device="cuda")
    inliers = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    scratch = device_scratch(torch, 1, cap, n_hyp)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.detect_device(frames, cfg, pts, offs)
        fast_hip.orient_device(frames, pts, offs, ang)
        fast_hip.smooth_device(frames, smoothed)
        fast_hip.describe_device(smoothed, pts, offs, desc, table, n_bins, angles=ang)
        fast_hip.match_device(desc, offs[:-1], desc, offs[1:], fwd, q_points=pts, t_points=pts,
                              window=window)
        fast_hip.match_device(desc, offs[1:], desc, offs[:-1], rev, q_points=pts, t_points=pts,
                              window=window)
        fast_hip.match_filter_device(fwd, offs[:-1], keep, reverse=rev, max_distance=80,
                                     ratio=(4, 5))
        for k, model in enumerate(("affine", "homography")):
            fast_hip.ransac_device(fwd, offs[:-1], pts, pts, offs[1:], models[k:k + 1], scratch,
                                   keep=keep, inliers=inliers if k else None, model=model,
                                   n_hyp=n_hyp, threshold=1.5, seed=4)
    stream.synchronize()
    o = offs.cpu().numpy()
    n0 = int(o[1])
    h_pts = pts.cpu().numpy().view(np.uint32)
    h_fwd, h_keep = mref.as_records(fwd.cpu().numpy()), keep.cpu().numpy()
    got = fast_hip.unpack_models(models.cpu().numpy())
    for k, model in enumerate(("affine", "homography")):
        want, want_in = ref.ransac(h_fwd, h_keep, cap, o[:-1], h_pts, h_pts, cap, o[1:], MODELS[model],
                                   n_hyp, 1.5, 4, inliers_out=np.full(cap, FILL, np.uint8))
        assert ref.models_equal(got[k], want[0])
        assert got[k]["n_inliers"] >= want[0]["n_inliers"] > 20
        assert got[k]["n_corr"] == h_keep[:n0].sum()
        # the shift, up to the rounding of a fit over coordinates below 2^9 (a relative 2^-40)
        assert np.allclose(got[k]["h"], [1, 0, 3, 0, 1, 2, 0, 0, 1], rtol=0, atol=2.0 ** -30)
    assert np.array_equal(inliers.cpu().numpy(), want_in)
    assert (inliers[n0:] == FILL).all()


# ---- 8: the host entries ---------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_host_entry_agrees_with_the_device_entry(model):
    q, t, good = planted(300, 150, 7, which=2 if model == "affine" else 0)
    matches = ref.identity_matches(300)
    matches["index"][11] = ref.NONE
    keep = np.ones(300, np.uint8)
    keep[[2, 3]] = 0
    dev, dev_in = run_ransac(matches, [0, 300], q, t, [0, 300], model, 200, 3.0, 6, keep=keep)
    H, mask, rec = fast_hip.estimate_model(q, t, matches, keep=keep, model=model, n_hyp=200,
                                           threshold=3.0, seed=6)
    assert ref.models_equal(rec, dev[0]) and np.array_equal(mask, dev_in[:300].astype(bool))
    assert H.shape == (3, 3) and np.array_equal(H.reshape(-1), rec["h"])
    assert rec["n_corr"] == 297 and mask.dtype == np.bool_
    # float points, train indices instead of records, no keep
    index = matches["index"].astype(np.int64)
    index[11] = -1
    Hf, maskf, recf = fast_hip.estimate_model(q.astype(np.float32), t.astype(np.float32), index,
                                              model=model, n_hyp=200, threshold=3.0, seed=6)
    want, want_in = ref.ransac(matches, None, 300, [0, 300], q, t, 300, [0, 300], MODELS[model], 200,
                               3.0, 6)
    assert ref.models_equal(recf, want[0]) and np.array_equal(maskf, want_in.astype(bool))
    # no model: H is None
    H, mask, rec = fast_hip.estimate_model(q[:2], t, matches[:2], model=model)
    assert H is None and not mask.any() and rec["n_corr"] == 2 and rec["hypothesis"] == ref.NONE
    H, mask, rec = fast_hip.estimate_model(q[:0], t, matches[:0], model=model)
    assert H is None and len(mask) == 0 and rec["n_corr"] == 0 and rec["hypothesis"] == ref.NONE


def test_host_entry_rejects_bad_arguments_and_keeps_fetch_last():
    lib = _native.load()
    img = workloads.golden_image()
    pts, scores = fast_hip.detect_scored_array(img, Config(16, 9, NonMaximalSuppression.MaxThreshold))
    ctx = fast_hip.context(0).handle
    q, t = ref.worked_example()
    m = ref.identity_matches(6)
    out = np.zeros(1, dtype=ref.MODEL_DTYPE)
    mask = np.full(6, FILL, np.uint8)

    def call(c=ctx, qc=q.ctypes.data, tc=t.ctypes.data, nq=6, nt=6, mm=m.ctypes.data, coords=0,
             model=1, n_hyp=8, thr=1.0, o=out.ctypes.data, inl=mask.ctypes.data):
        return lib.fdf_ransac_points(c, qc, tc, nq, nt, mm, None, coords, model, n_hyp, thr, 0, o,
                                     inl)

    for bad in (dict(c=None), dict(qc=None), dict(tc=None), dict(mm=None), dict(o=None),
                dict(coords=2), dict(model=2), dict(n_hyp=0), dict(n_hyp=65537), dict(thr=-1.0),
                dict(thr=float("nan")), dict(nq=0xFFFFFFFF), dict(nt=0xFFFFFFFF)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert not out["h"].any() and (mask == FILL).all()
    assert call(inl=None) == _native.FDF_OK and (mask == FILL).all()
    assert call() == _native.FDF_OK
    assert (out[0]["hypothesis"], out[0]["n_inliers"]) == (3, 5) and mask.tolist() == [1, 1, 1, 1, 0, 1]
    # the retained detection is still there
    got = np.zeros((len(pts), 2), dtype=np.uint32)
    got_sc = np.zeros(len(pts), dtype=np.uint16)
    n = ctypes.c_size_t(0)
    rc = lib.fdf_fetch_last(ctx, got.ctypes.data, got_sc.ctypes.data, len(pts), ctypes.byref(n))
    assert rc == _native.FDF_OK and n.value == len(pts)
    assert np.array_equal(got, pts) and np.array_equal(got_sc, scores)


def test_cpp_ransac_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_ransac")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
    assert res.stdout.count("hypothesis=3 inliers=5/6 valid=8 h=1 0 3 0 1 5 0 0 1") == 2
