"""Best-K keypoint selection per grid cell (fdf_select_device, fdf_select_points) against a
numpy restatement of its semantics: per frame, a stable sort of the points by (cell,
descending score, index) and the first k of each cell.  Everything is compared bit for bit:
points, scores, offsets and keep flags."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_SCORES = np.array([0, 1, 255, 256, 257, 511, 512, 65535], dtype=np.uint16)


def reference(pts, scores, offs, shape, cell, k, cap=None):
    """(sel_pts, sel_scores, sel_offsets, keep, stats) of the selection.  stats: the largest
    cell population, and the number of cells whose k-th and (k+1)-th scores are equal."""
    h, w = shape
    cw = cell[0] or w
    ch = cell[1] or h
    cells_x = -(-w // cw)
    cap = len(pts) if cap is None else cap
    keep = np.zeros(cap, dtype=np.uint8)
    sel_offs = np.zeros(len(offs), dtype=np.uint64)
    largest, tie_cuts = 0, 0
    for f in range(len(offs) - 1):
        b, e = min(int(offs[f]), cap), min(int(offs[f + 1]), cap)
        p = pts[b:e].astype(np.int64)
        s = scores[b:e].astype(np.int64)
        cid = (p[:, 1] // ch) * cells_x + p[:, 0] // cw
        idx = np.arange(e - b)
        order = np.lexsort((idx, -s, cid))
        sc = cid[order]
        rank = idx - np.searchsorted(sc, sc, side="left")
        keep[b + order[rank < k]] = 1
        sel_offs[f + 1] = sel_offs[f] + np.uint64(np.count_nonzero(rank < k))
        if e > b:
            largest = max(largest, int(rank.max()) + 1)
            ss = s[order]
            at_cut = np.nonzero(rank == k)[0]           # the (k+1)-th of a cell
            tie_cuts += int(np.count_nonzero(ss[at_cut] == ss[at_cut - 1]))
    m = keep.astype(bool)
    return pts[:cap][m], scores[:cap][m], sel_offs, keep, (largest, tie_cuts)


def run_device(pts, scores, offs, shape, cell, k, cap=None, sel_cap=None):
    """fdf_select_device on uploaded arrays -> (sel_pts, sel_scores, sel_offsets, keep)."""
    import torch

    cap = len(pts) if cap is None else cap
    d_pts = torch.from_numpy(np.ascontiguousarray(pts[:cap]).view(np.int32)).cuda()
    d_sc = torch.from_numpy(np.ascontiguousarray(scores[:cap]).view(np.int16)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()
    sel_cap = cap if sel_cap is None else sel_cap
    sel = torch.full((sel_cap, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((sel_cap,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((len(offs),), -1, dtype=torch.int64, device="cuda")
    keep = torch.full((cap,), 7, dtype=torch.uint8, device="cuda")
    fast_hip.select_device(d_pts, d_sc, d_offs, shape, cell, k, sel, sel_sc, sel_offs, keep=keep)
    torch.cuda.synchronize()
    so = sel_offs.cpu().numpy().astype(np.uint64)
    n = min(int(so[-1]), sel_cap)
    return (sel[:n].cpu().numpy().view(np.uint32), sel_sc[:n].cpu().numpy().view(np.uint16), so,
            keep.cpu().numpy())


def check_device(pts, scores, offs, shape, cell, k):
    want = reference(pts, scores, offs, shape, cell, k)
    got = run_device(pts, scores, offs, shape, cell, k)
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    return want, got


@functools.lru_cache(maxsize=None)
def detected(which, nms):
    img = workloads.golden_image() if which == "golden" else workloads.s3_frame(1, 128, 96)
    pts, scores = fast_hip.detect_scored_array(img, Config(16, 9, NonMaximalSuppression(nms)))
    return img.shape, pts, scores


CELLS = [(32, 32, 1), (32, 32, 3), (16, 8, 2), (64, 48, 5), (7, 5, 1), (300, 1, 2), (0, 0, 50)]


@pytest.mark.parametrize("cw,ch,k", CELLS)
@pytest.mark.parametrize("nms", [0, 1, 2])
@pytest.mark.parametrize("which", ["golden", "s3"])
def test_detector_output(which, nms, cw, ch, k):
    shape, pts, scores = detected(which, nms)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    want = reference(pts, scores, offs, shape, (cw, ch), k)
    largest, tie_cuts = want[4]
    assert largest > k, "the case must drop points"
    if nms in (0, 1) and (cw, ch, k) in ((16, 8, 2), (7, 5, 1)):
        assert tie_cuts >= 1, "the case must cut through a tie"
    check_device(pts, scores, offs, shape, (cw, ch), k)


@functools.lru_cache(maxsize=None)
def tie_frame():
    w, h = 67, 41
    ys, xs = np.mgrid[0:h, 0:w]
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    scores = TIE_SCORES[np.random.default_rng(5).integers(0, len(TIE_SCORES), len(pts))]
    return (h, w), pts, scores


@pytest.mark.parametrize("cw,ch,k", [(16, 8, 3), (0, 0, 100), (67, 1, 1), (1, 1, 1)])
def test_synthetic_ties(cw, ch, k):
    shape, pts, scores = tie_frame()
    offs = np.array([0, len(pts)], dtype=np.uint64)
    want, _ = check_device(pts, scores, offs, shape, (cw, ch), k)
    if (cw, ch) == (1, 1):
        assert want[3].all()                       # one point per cell: everything is kept
    else:
        assert want[4][1] >= 1                     # the cut goes through a tie


@pytest.mark.parametrize("cw,ch,k", [(1, 16, 1), (3, 4, 2)])
def test_column_groups(cw, ch, k):
    """More cells in a row than the kernel holds histograms for at once."""
    w, h = 2048, 16
    rng = np.random.default_rng(9)
    flat = np.sort(rng.choice(w * h, 6000, replace=False))
    pts = np.stack([flat % w, flat // w], axis=1).astype(np.uint32)
    scores = rng.integers(0, 65536, len(pts)).astype(np.uint16)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    want, _ = check_device(pts, scores, offs, (h, w), (cw, ch), k)
    assert want[4][0] > k


@pytest.mark.parametrize("variant", ["large", "cap40", "sel_cap"])
def test_device_chain(variant):
    """detect_device -> score_device -> select_device on one stream, nothing in between; a
    frame with no keypoints sits in mid-batch."""
    import torch

    frames = workloads.s1_frames_torch(4, 5, 256, 160)
    frames[2].zero_()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap = 40 if variant == "cap40" else 100_000
    cell, k = (32, 32), 2
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(6, dtype=torch.int64, device="cuda")
    scores = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    sel_cap = 25 if variant == "sel_cap" else cap
    sel = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    keep = torch.full((cap,), 7, dtype=torch.uint8, device="cuda")
    fast_hip.detect_device(frames, cfg, out, offs)
    fast_hip.score_device(frames, cfg, out, offs, scores)
    fast_hip.select_device(out, scores, offs, (160, 256), cell, k, sel[:sel_cap],
                           sel_sc[:sel_cap], sel_offs, keep=keep)
    torch.cuda.synchronize()
    h_offs = offs.cpu().numpy().astype(np.uint64)
    assert h_offs[2] == h_offs[3] and h_offs[-1] > 40      # the empty frame; cap40 truncates
    n_in = min(int(h_offs[-1]), cap)
    h_pts = out.cpu().numpy().view(np.uint32)
    h_sc = scores.cpu().numpy().view(np.uint16)
    want = reference(h_pts, h_sc, h_offs, (160, 256), cell, k, cap=cap)
    assert want[4][0] > k
    total = int(want[2][-1])
    assert np.array_equal(sel_offs.cpu().numpy().astype(np.uint64), want[2])
    assert np.array_equal(keep.cpu().numpy()[:n_in], want[3][:n_in])
    assert not keep.cpu().numpy()[n_in:].any()
    n = min(total, sel_cap)
    if variant == "sel_cap":
        assert total > sel_cap
    assert np.array_equal(sel[:n].cpu().numpy().view(np.uint32), want[0][:n])
    assert np.array_equal(sel_sc[:n].cpu().numpy().view(np.uint16), want[1][:n])
    assert (sel[n:] == -1).all() and (sel_sc[n:] == -1).all()   # nothing past the end


def test_k_covers_every_cell():
    shape, pts, scores = detected("golden", 0)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    for cell, k in (((32, 32), 100_000), ((0, 0), len(pts)), ((16, 8), 0xffffffff)):
        got = run_device(pts, scores, offs, shape, cell, k)
        assert np.array_equal(got[0], pts) and np.array_equal(got[1], scores)
        assert got[3].all() and int(got[2][-1]) == len(pts)


def test_deterministic():
    shape, pts, scores = tie_frame()
    offs = np.array([0, len(pts)], dtype=np.uint64)
    a = run_device(pts, scores, offs, shape, (16, 8), 3)
    b = run_device(pts, scores, offs, shape, (16, 8), 3)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_empty_inputs():
    """No frames' worth of points, frames the reference answers with an empty list, and a
    batch whose frames are all empty."""
    pts = np.zeros((0, 2), np.uint32)
    scores = np.zeros(0, np.uint16)
    got = fast_hip.select_best(pts, scores, (200, 300), (32, 32), 3)
    assert got[0].shape == (0, 2) and got[1].shape == (0,)
    shape, p, s = tie_frame()
    got = fast_hip.select_best(p[:10], s[:10], (5, 67), (8, 8), 1)      # height 5: empty shape
    assert got[0].shape == (0, 2)
    offs = np.array([0, 0, 0, 0], dtype=np.uint64)
    got = run_device(p[:16], s[:16], offs, shape, (8, 8), 1)
    assert not got[2].any() and not got[3].any() and len(got[0]) == 0
    # points only in the last frame, the first two empty
    offs = np.array([0, 0, 0, 16], dtype=np.uint64)
    check_device(p[:16], s[:16], offs, shape, (8, 8), 1)


def test_host_path():
    shape, pts, scores = detected("golden", 1)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    for cell, k in (((32, 32), 2), ((0, 0), 20), ((7, 5), 1)):
        want = reference(pts, scores, offs, shape, cell, k)
        got = fast_hip.select_best(pts, scores, shape, cell, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got = fast_hip.select_best(pts, scores, shape, cell, k, offsets=offs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    # several frames through the host path
    _, tp, ts = tie_frame()
    tshape = (41, 67)
    toffs = np.array([0, 67 * 10, 67 * 10, 67 * 41], dtype=np.uint64)   # rows 0-9 | none | rest
    want = reference(tp, ts, toffs, tshape, (16, 8), 3)
    got = fast_hip.select_best(tp, ts, tshape, (16, 8), 3, offsets=toffs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])


def test_host_capacity_two_call():
    shape, pts, scores = detected("golden", 0)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    want = reference(pts, scores, offs, shape, (32, 32), 3)
    total = len(want[0])
    lib = _native.load()
    ctx = fast_hip.context(0)
    cap = 10
    assert total > cap
    out = np.full((total, 2), 0xffffffff, dtype=np.uint32)
    out_sc = np.full(total, 0xffff, dtype=np.uint16)
    n = ctypes.c_size_t(0)

    def call(cap):
        return lib.fdf_select_points(ctx.handle, pts.ctypes.data, scores.ctypes.data, None, 1,
                                     len(pts), shape[1], shape[0], 32, 32, 3, out.ctypes.data,
                                     out_sc.ctypes.data, cap, None, ctypes.byref(n))

    assert call(cap) == _native.FDF_ERR_CAPACITY
    assert n.value == total
    assert np.array_equal(out[:cap], want[0][:cap]) and (out[cap:] == 0xffffffff).all()
    assert call(n.value) == _native.FDF_OK
    assert n.value == total
    assert np.array_equal(out, want[0]) and np.array_equal(out_sc, want[1])


def test_host_path_keeps_fetch_last():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    fast_hip.select_best(pts, scores, img.shape, (32, 32), 2)
    lib = _native.load()
    ctx = fast_hip.context(0)
    out = np.zeros((len(pts), 2), dtype=np.uint32)
    out_sc = np.zeros(len(pts), dtype=np.uint16)
    n = ctypes.c_size_t(0)
    rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data, out_sc.ctypes.data, len(pts),
                            ctypes.byref(n))
    assert rc == _native.FDF_OK and n.value == len(pts)
    assert np.array_equal(out, pts) and np.array_equal(out_sc, scores)


def test_detect_best_array():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.SumAbsolute)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    want = fast_hip.select_best(pts, scores, img.shape, (64, 48), 5)
    got = fast_hip.detect_best_array(img, cfg, (64, 48), 5)
    assert 0 < len(got[0]) < len(pts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_select_device_argument_errors():
    """k = 0, a short scratch and a misaligned scratch: FDF_ERR_ARG, and nothing is launched
    (the outputs keep their fill)."""
    import torch

    shape, pts, scores = tie_frame()
    n = len(pts)
    d_pts = torch.from_numpy(pts.view(np.int32)).cuda()
    d_sc = torch.from_numpy(scores.view(np.int16)).cuda()
    d_offs = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    sel = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    need = fast_hip.select_scratch_bytes(1, shape, (16, 8), n)
    scratch = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0
    lib = _native.load()
    ctx = fast_hip.context(0)

    def call(k, scratch_ptr, scratch_bytes, offsets_ptr=sel_offs.data_ptr()):
        return lib.fdf_select_device(ctx.handle, 1, shape[1], shape[0], d_pts.data_ptr(),
                                     d_sc.data_ptr(), n, d_offs.data_ptr(), 16, 8, k,
                                     sel.data_ptr(), sel_sc.data_ptr(), n, offsets_ptr, None,
                                     scratch_ptr, scratch_bytes, None)

    assert call(0, scratch.data_ptr(), need) == _native.FDF_ERR_ARG
    assert call(3, scratch.data_ptr(), need - 1) == _native.FDF_ERR_ARG
    assert call(3, scratch.data_ptr() + 64, need) == _native.FDF_ERR_ARG
    assert call(3, None, need) == _native.FDF_ERR_ARG
    assert call(3, scratch.data_ptr(), need, offsets_ptr=None) == _native.FDF_ERR_ARG
    torch.cuda.synchronize()
    assert (sel == -1).all() and (sel_sc == -1).all() and (sel_offs == -1).all()
    # the same call with a good scratch works (NULL stream = the HIP null stream)
    assert call(3, scratch.data_ptr(), need) == _native.FDF_OK
    torch.cuda.synchronize()
    want = reference(pts, scores, np.array([0, n], dtype=np.uint64), shape, (16, 8), 3)
    assert np.array_equal(sel_offs.cpu().numpy().astype(np.uint64), want[2])
    m = int(want[2][-1])
    assert np.array_equal(sel[:m].cpu().numpy().view(np.uint32), want[0])


def test_cpp_select_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_select")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
