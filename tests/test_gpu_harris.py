"""Harris corner response (fdf_harris_device, fdf_harris_points) against the numpy restatement
of include/fdf.h's semantics in tests/_harris_reference.py (pinned to the worked values by
tests/test_harris.py).  Every comparison is bit for bit, on the int64 responses and on the
u16 rank scores."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import workloads
from _harris_reference import (checker3, corner_frame, edge_frame, reference, select_reference)
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_FILL = 0x5A5A
RESP_FILL = 0x5A5A5A5A5A5A5A5A
ORB_K = (1, 25)


def run_device(frames, pts, offs, block, k=ORB_K, cap=None, responses=True, frame_stride=None,
               lead=0, extra=0):
    """fdf_harris_device on uploaded arrays -> (scores (cap + extra,) uint16, responses
    (cap + extra,) int64 or None), both pre-filled.  Frames are laid out `frame_stride` bytes
    apart, `lead` bytes into their allocation, with guard bytes around them."""
    import torch

    frames = np.asarray(frames)
    f, h, w = frames.shape
    stride = h * w if frame_stride is None else frame_stride
    flat = torch.full((lead + f * stride + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_frames = torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)
    d_frames.copy_(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    want_flat = flat.clone()
    cap = len(pts) if cap is None else cap
    d_pts = torch.from_numpy(np.ascontiguousarray(pts[:cap]).view(np.int32)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()
    sc = torch.full((cap + extra,), SCORE_FILL, dtype=torch.int16, device="cuda")
    resp = torch.full((cap + extra,), RESP_FILL, dtype=torch.int64, device="cuda") \
        if responses else None
    fast_hip.harris_device(d_frames, d_pts, d_offs, sc, block=block, k=k, responses=resp)
    torch.cuda.synchronize()
    assert torch.equal(flat, want_flat)               # frames and guard bytes untouched
    return sc.cpu().numpy().view(np.uint16), resp.cpu().numpy() if responses else None


def check_frame(img, pts, block, k=ORB_K, host=True, device=True):
    """One frame through the device entry and the host entry; returns the exact responses."""
    pts = np.ascontiguousarray(pts, dtype=np.uint32)
    want, want_sc = reference(img, pts, block, k)
    if device:
        offs = np.array([0, len(pts)], dtype=np.uint64)
        sc, resp = run_device(img[None], pts, offs, block, k)
        assert np.array_equal(resp, want)
        assert np.array_equal(sc, want_sc)
    if host:
        h_sc, h_resp = fast_hip.keypoint_harris(img, pts, block, k, responses=True)
        assert np.array_equal(h_resp, want)
        assert np.array_equal(h_sc, want_sc)
        assert np.array_equal(fast_hip.keypoint_harris(img, pts, block, k), want_sc)
    return want, want_sc


def near_border(pts, shape, block):
    """Points whose (block + 2)^2 window leaves the frame (hb + 1 from a border)."""
    h, w = shape
    m = block // 2 + 1
    x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    return int(np.count_nonzero((x < m) | (y < m) | (x + m >= w) | (y + m >= h)))


def every_pixel(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def golden_points(which):
    return workloads.read_points(os.path.join(workloads.GOLDEN, f"kp_t16_n9_{which}.txt"))


# ---- 1: the golden frame ---------------------------------------------------------------------

@pytest.mark.parametrize("block", [3, 5, 7])
@pytest.mark.parametrize("which,count,nonpos3", [("off", 309, 17), ("maxt", 131, 7)])
def test_golden_frame(which, count, nonpos3, block):
    img = workloads.golden_image()
    pts = golden_points(which)
    assert img.shape == (200, 300) and len(pts) == count
    # the detector's points lie 3 pixels inside: the clamped path needs window points too
    border = np.array([(0, 0), (299, 199), (1, 100), (150, 1), (298, 50), (100, 198), (2, 2),
                       (3, 3), (4, 4), (296, 196), (295, 195)], dtype=np.uint32)
    both = np.concatenate([pts, border])
    assert near_border(both, img.shape, block) >= 1      # the clamped path is in the case set
    assert near_border(both, img.shape, block) < len(both)   # and so is the fast one
    want, _ = check_frame(img, both, block)
    if block == 7:
        assert (want[:count] > 0).all()
    if block == 3:
        assert int(np.count_nonzero(want[:count] <= 0)) == nonpos3


# ---- 2: exact synthetic frames ---------------------------------------------------------------

def test_worked_frames():
    pts = every_pixel(32, 32)
    want, sc = check_frame(corner_frame(), pts, 7)
    at = lambda x, y: y * 32 + x
    assert want[at(16, 16)] == 1167741344610000 and sc[at(16, 16)] == 42022
    assert want[at(15, 15)] == 599464460610000 and sc[at(15, 15)] == 41026
    assert want[at(0, 0)] == 0 and sc[at(0, 0)] == 0
    want, sc = check_frame(edge_frame(), pts, 7)
    assert want[at(16, 16)] == -212156703360000 and sc[at(16, 16)] == 0
    assert (want <= 0).all() and not sc.any()             # a straight edge is no corner
    want, sc = check_frame(np.full((32, 32), 93, np.uint8), pts, 7)
    assert not want.any() and not sc.any()


@pytest.mark.parametrize("k,bits", [((1, 25), 53), ((0, 255), 57), ((255, 1), 58),
                                    ((255, 255), 58)])
def test_checker3_wide_arithmetic(k, bits):
    """Responses that neither a double nor an int32 holds."""
    img = checker3()
    pts = np.array([(x, y) for y in range(8, 16) for x in range(8, 16)], dtype=np.uint32)
    want, _ = reference(img, pts, 7, k)
    assert max(abs(int(v)) for v in want).bit_length() >= bits
    check_frame(img, pts, 7, k)
    check_frame(img, every_pixel(24, 24), 7, k, host=False)


# ---- 3: frames smaller than the window -------------------------------------------------------

@pytest.mark.parametrize("block", [3, 7])
def test_frames_smaller_than_the_window(block):
    """1 x 9 and 9 x 1 are shape errors of the device entry (as for fdf_orient_device: the
    detector's shape rules) and run through the host entry, which has none."""
    for seed, (w, h) in enumerate(((7, 7), (1, 9), (9, 1), (20, 64), (64, 20))):
        img = workloads.s3_frame(20 + seed, w, h)
        pts = every_pixel(w, h)
        if min(w, h) <= block + 2:
            assert near_border(pts, img.shape, block) == len(pts)
        check_frame(img, pts, block, device=(w >= 7 and h >= 7))


def test_every_pixel_odd_width():
    """67 x 41, every pixel, block 7: the last rows' dword reads end at the frame's end."""
    img = workloads.s3_frame(2, 67, 41)
    pts = every_pixel(67, 41)
    assert 0 < near_border(pts, img.shape, 7) < len(pts)
    check_frame(img, pts, 7)
    check_frame(img, pts, 5, host=False)
    check_frame(img, pts, 3, host=False)


# ---- 4: the batch contract -------------------------------------------------------------------

@pytest.mark.parametrize("responses", [True, False])
def test_batch_contract(responses):
    w, h, block = 96, 64, 7
    frames = np.stack([workloads.s3_frame(10, w, h), np.zeros((h, w), np.uint8),
                       workloads.s3_frame(11, w, h)])
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    per = [fast_hip.detect_array(f, cfg) for f in frames]
    assert len(per[0]) > 20 and len(per[1]) == 0 and len(per[2]) > 20
    pts = np.concatenate(per).astype(np.uint32)
    offs = np.cumsum([0] + [len(p) for p in per]).astype(np.uint64)
    total = int(offs[-1])
    cap = total - 9                                  # the last frame is cut
    assert cap > int(offs[1])
    sc, resp = run_device(frames, pts, offs, block, cap=cap, responses=responses,
                          frame_stride=w * h + 37, lead=1, extra=16)
    w0, s0 = reference(frames[0], per[0], block)
    w2, s2 = reference(frames[2], pts[int(offs[1]):cap], block)
    assert np.array_equal(sc[:cap], np.concatenate([s0, s2]))
    assert (sc[cap:] == SCORE_FILL).all()
    if responses:
        assert np.array_equal(resp[:cap], np.concatenate([w0, w2]))
        assert (resp[cap:] == RESP_FILL).all()


def test_batch_contract_tail_untouched():
    """The offsets end below the capacity: the entries after them keep their fill, whatever
    the points there hold."""
    w, h, block = 96, 64, 5
    frames = np.stack([workloads.s3_frame(12, w, h)] * 2)
    pts = every_pixel(w, h)[::7]
    k = len(pts)
    both = np.concatenate([pts, pts, np.full((40, 2), 0xFFFFFFFF, np.uint32)])
    offs = np.array([0, k, 2 * k], dtype=np.uint64)
    sc, resp = run_device(frames, both, offs, block, frame_stride=w * h + 1)
    want, want_sc = reference(frames[0], pts, block)
    assert np.array_equal(resp[:k], want) and np.array_equal(resp[k:2 * k], want)
    assert np.array_equal(sc[:k], want_sc) and np.array_equal(sc[k:2 * k], want_sc)
    assert (sc[2 * k:] == SCORE_FILL).all() and (resp[2 * k:] == RESP_FILL).all()


# ---- 5: the device chain ---------------------------------------------------------------------

def moments_reference(img, pts, r):
    """The exact (m10, m01) of fdf_orient_device (include/fdf.h) for one frame."""
    u = fast_hip.orient_disc(r)
    h, w = img.shape
    px = img.astype(np.int64)
    x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    m10 = np.zeros(len(pts), np.int64)
    m01 = np.zeros(len(pts), np.int64)
    for v in range(-r, r + 1):
        row = np.clip(y + v, 0, h - 1)
        for d in range(-int(u[abs(v)]), int(u[abs(v)]) + 1):
            val = px[row, np.clip(x + d, 0, w - 1)]
            m10 += d * val
            m01 += v * val
    return np.stack([m10, m01], axis=1)


def test_device_chain():
    """detect_device -> harris_device -> select_device -> orient_device on one side stream
    with nothing in between, against oracle detection + numpy Harris + numpy selection + numpy
    moments."""
    import torch

    w, h, f, r = 256, 160, 3, 15
    frames = workloads.s1_frames_torch(4, f, w, h)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap = 20_000
    cell, k = (32, 32), 2
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(f + 1, dtype=torch.int64, device="cuda")
    scores = torch.full((cap,), SCORE_FILL, dtype=torch.int16, device="cuda")
    sel = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((f + 1,), -1, dtype=torch.int64, device="cuda")
    ang = torch.full((cap,), -77.0, dtype=torch.float32, device="cuda")
    mom = torch.full((cap, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.detect_device(frames, cfg, out, offs)
        fast_hip.harris_device(frames, out, offs, scores)
        fast_hip.select_device(out, scores, offs, (h, w), cell, k, sel, sel_sc, sel_offs)
        fast_hip.orient_device(frames, sel, sel_offs, ang, radius=r, moments=mom)
    stream.synchronize()
    h_frames = frames.cpu().numpy()
    want_pts, want_sc, want_mom, want_offs, all_sc = [], [], [], [0], []
    for i in range(f):
        p = np.asarray(oracle.detect(h_frames[i], 16, 9, 1), dtype=np.uint32).reshape(-1, 2)
        _, s = reference(h_frames[i], p)
        keep = select_reference(p, s, (h, w), cell, k)
        all_sc.append(s)
        want_pts.append(p[keep])
        want_sc.append(s[keep])
        want_mom.append(moments_reference(h_frames[i], p[keep], r))
        want_offs.append(want_offs[-1] + int(keep.sum()))
    n = want_offs[-1]
    total = int(offs[-1])
    assert n > 50 and total > n
    assert np.array_equal(scores[:total].cpu().numpy().view(np.uint16), np.concatenate(all_sc))
    assert (scores[total:] == SCORE_FILL).all()
    assert sel_offs.cpu().numpy().tolist() == want_offs
    assert np.array_equal(sel[:n].cpu().numpy().view(np.uint32), np.concatenate(want_pts))
    assert np.array_equal(sel_sc[:n].cpu().numpy().view(np.uint16), np.concatenate(want_sc))
    assert np.array_equal(mom[:n].cpu().numpy(), np.concatenate(want_mom))
    assert (mom[n:] == 0x5A5A5A5A).all()


# ---- 6: argument errors ----------------------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    w, h = 96, 64
    frames = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    pts = torch.full((32, 2), 20, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, 32], dtype=torch.int64, device="cuda")
    sc = torch.full((32,), SCORE_FILL, dtype=torch.int16, device="cuda")
    resp = torch.full((33,), RESP_FILL, dtype=torch.int64, device="cuda")
    lib = _native.load()
    ctx = fast_hip.context(0)
    good = dict(ctx=ctx.handle, frames=frames.data_ptr(), n=2, w=w, h=h, stride=w * h,
                pts=pts.data_ptr(), cap=32, offs=offs.data_ptr(), block=7, k_num=1, k_den=25,
                sc=sc.data_ptr(), resp=resp.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.fdf_harris_device(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["stride"],
                                     a["pts"], a["cap"], a["offs"], a["block"], a["k_num"],
                                     a["k_den"], a["sc"], a["resp"], None)

    for bad in (dict(block=0), dict(block=4), dict(block=9), dict(k_den=0), dict(k_den=256),
                dict(k_num=256), dict(ctx=None), dict(frames=None), dict(pts=None),
                dict(offs=None), dict(sc=None), dict(n=65536), dict(stride=w * h - 1),
                dict(resp=resp.data_ptr() + 4), dict(resp=resp.data_ptr() + 1)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(h=2) == _native.FDF_ERR_SIZE
    assert call(h=6) == _native.FDF_OK               # a shape with no keypoints: nothing to do
    assert call(n=0) == _native.FDF_OK
    assert call(cap=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (sc == SCORE_FILL).all() and (resp == RESP_FILL).all()
    # the good call works, on the null stream and without responses
    assert call(resp=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (sc == 0).all() and (resp == RESP_FILL).all()
    assert call(k_num=0, k_den=255, block=3) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (resp[:32] == 0).all() and resp[32] == RESP_FILL


# ---- 7: the host entry -----------------------------------------------------------------------

def test_host_entry_rejects_points_outside():
    img = workloads.golden_image()
    h, w = img.shape
    for bad in ((w, 5), (5, h), (0xFFFFFFFF, 0)):
        with pytest.raises(_native.FdfError) as info:
            fast_hip.keypoint_harris(img, np.array([(10, 10), bad], dtype=np.uint32))
        assert info.value.status == _native.FDF_ERR_ARG
    lib = _native.load()
    pts = np.array([(w, 5)], dtype=np.uint32)
    sc = np.full(1, SCORE_FILL, np.uint16)
    rc = lib.fdf_harris_points(fast_hip.context(0).handle, img.ctypes.data, w, h, w,
                               pts.ctypes.data, 1, 7, 1, 25, sc.ctypes.data, None)
    assert rc == _native.FDF_ERR_ARG and sc[0] == SCORE_FILL
    pts[0] = (5, 5)
    for block, k_num, k_den in ((4, 1, 25), (7, 256, 25), (7, 1, 0)):
        rc = lib.fdf_harris_points(fast_hip.context(0).handle, img.ctypes.data, w, h, w,
                                   pts.ctypes.data, 1, block, k_num, k_den, sc.ctypes.data, None)
        assert rc == _native.FDF_ERR_ARG and sc[0] == SCORE_FILL
    assert fast_hip.keypoint_harris(img, np.zeros((0, 2), np.uint32)).shape == (0,)


def test_host_entry_keeps_fetch_last():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    fast_hip.keypoint_harris(img, pts)
    lib = _native.load()
    ctx = fast_hip.context(0)
    out = np.zeros((len(pts), 2), dtype=np.uint32)
    out_sc = np.zeros(len(pts), dtype=np.uint16)
    n = ctypes.c_size_t(0)
    rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data, out_sc.ctypes.data, len(pts),
                            ctypes.byref(n))
    assert rc == _native.FDF_OK and n.value == len(pts)
    assert np.array_equal(out, pts) and np.array_equal(out_sc, scores)


def test_host_entry_row_stride():
    """A view with rows further apart than its width."""
    big = workloads.s3_frame(6, 80, 50)
    view = big[:, 3:67]
    assert view.strides[0] == 80
    pts = every_pixel(64, 50)[::5]
    want, want_sc = reference(np.ascontiguousarray(view), pts)
    sc, resp = fast_hip.keypoint_harris(view, pts, responses=True)
    assert np.array_equal(resp, want) and np.array_equal(sc, want_sc)


def test_detect_harris_array():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, sc = fast_hip.detect_harris_array(img, cfg)
    assert np.array_equal(pts, golden_points("maxt"))
    assert np.array_equal(sc, reference(img, pts)[1])
    pts3, sc3 = fast_hip.detect_harris_array(img, cfg, block=3, k=(0, 255))
    assert np.array_equal(pts3, pts)
    assert np.array_equal(sc3, reference(img, pts, 3, (0, 255))[1])


# ---- 8: the scale pyramid --------------------------------------------------------------------

def test_multiscale_ranked_by_harris():
    import torch

    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cell, k, block, hk = (64, 64), 2, 5, (1, 20)
    got = fast_hip.detect_multiscale_array(img, cfg, n_levels=3, cell=cell, k=k, rank="harris",
                                           block=block, harris_k=hk)
    pyr = fast_hip.Pyramid(torch.from_numpy(img[None].copy()).cuda(), 3)
    torch.cuda.synchronize()
    differs = 0
    for l in range(3):
        level = pyr.level(l)[0].cpu().numpy()
        part = got.level == l
        pts = fast_hip.detect_array(level, cfg)
        _, sc = reference(level, pts, block, hk)
        keep = select_reference(pts, sc, level.shape, cell, k)
        assert 0 < keep.sum() < len(pts)
        assert np.array_equal(got.points[part], pts[keep])
        assert np.array_equal(got.scores[part], sc[keep])
        angles = fast_hip.keypoint_angles(level, pts[keep])
        assert np.array_equal(got.angles[part], angles)
        fast_sel, _ = fast_hip.select_best(pts, fast_hip.detect_scored_array(level, cfg)[1],
                                           level.shape, cell, k)
        differs += int(not np.array_equal(fast_sel, pts[keep]))
    assert differs > 0                                # the ranking is not the detector's
    # without selection: every detection with its Harris rank score
    everything = fast_hip.detect_multiscale_array(img, cfg, n_levels=2, rank="harris")
    part = everything.level == 0
    assert np.array_equal(everything.points[part], golden_points("maxt"))
    assert np.array_equal(everything.scores[part], reference(img, golden_points("maxt"))[1])


def test_multiscale_default_is_rank_fast():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    a = fast_hip.detect_multiscale_array(img, cfg, n_levels=3, cell=(64, 64), k=2)
    b = fast_hip.detect_multiscale_array(img, cfg, n_levels=3, cell=(64, 64), k=2, rank="fast")
    assert a.sizes == b.sizes
    for name in ("level", "points", "points0", "scores", "angles", "descriptors"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


# ---- 9: the C++ wrapper ----------------------------------------------------------------------

def test_cpp_harris_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_harris")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
