"""Keypoint orientation by intensity centroid (fdf_orient_device, fdf_orient_points) against a
numpy restatement of include/fdf.h's semantics: the umax disc table, clamped reads, int64
sums, np.arctan2 in float64.  Moments are compared bit for bit.  Angles are compared by
circular difference with arctan2 of the exact moments; the bound of 1e-5 rad separates
"atan2f of the right arguments" (float32 rounding of these angles is 2.9e-7) from a wrong
formula (swapped arguments, a flipped sign, degrees)."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_TOL = 1e-5
ANGLE_FILL = -77.0
MOMENT_FILL = 0x5A5A5A5A


def disc(r):
    """OpenCV's umax rule."""
    vmax = int(math.floor(r * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(r * math.sqrt(2.0) / 2))
    u = [0] * (r + 2)
    for v in range(vmax + 1):
        u[v] = int(math.floor(math.sqrt(r * r - v * v) + 0.5))
    v0 = 0
    for v in range(r, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:r + 1]


def reference(img, pts, r):
    """(moments (K, 2) int64, angles (K,) float64) of the points of one frame."""
    h, w = img.shape
    px = img.astype(np.int64)
    x = pts[:, 0].astype(np.int64)
    y = pts[:, 1].astype(np.int64)
    m10 = np.zeros(len(pts), np.int64)
    m01 = np.zeros(len(pts), np.int64)
    u = disc(r)
    for v in range(-r, r + 1):
        row = np.clip(y + v, 0, h - 1)
        for d in range(-u[abs(v)], u[abs(v)] + 1):
            val = px[row, np.clip(x + d, 0, w - 1)]
            m10 += d * val
            m01 += v * val
    return np.stack([m10, m01], axis=1), np.arctan2(m01.astype(np.float64), m10.astype(np.float64))


def check_angles(got, moments):
    """`got` float32 against arctan2 of the exact moments; returns the largest difference."""
    want = np.arctan2(moments[:, 1].astype(np.float64), moments[:, 0].astype(np.float64))
    diff = np.abs(got.astype(np.float64) - want)
    diff = np.minimum(diff, 2 * np.pi - diff)
    worst = float(diff.max()) if len(diff) else 0.0
    print(f"largest angle difference {worst:.3g} rad over {len(diff)} points")
    assert worst <= ANGLE_TOL
    assert np.all(got > -np.pi - ANGLE_TOL) and np.all(got <= np.float32(np.pi))
    zero = (moments == 0).all(axis=1)
    assert np.all(got[zero] == 0.0)
    return worst


def run_device(frames, pts, offs, r, cap=None, moments=True, frame_stride=None, lead=0,
               extra=0):
    """fdf_orient_device on uploaded arrays -> (angles (cap + extra,), moments (cap + extra, 2)
    or None), both pre-filled.  Frames are laid out `frame_stride` bytes apart, `lead` bytes
    into their allocation."""
    import torch

    frames = np.asarray(frames)
    f, h, w = frames.shape
    stride = h * w if frame_stride is None else frame_stride
    flat = torch.full((lead + f * stride + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_frames = torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)
    d_frames.copy_(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    cap = len(pts) if cap is None else cap
    d_pts = torch.from_numpy(np.ascontiguousarray(pts[:cap]).view(np.int32)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()
    ang = torch.full((cap + extra,), ANGLE_FILL, dtype=torch.float32, device="cuda")
    mom = torch.full((cap + extra, 2), MOMENT_FILL, dtype=torch.int32, device="cuda") \
        if moments else None
    fast_hip.orient_device(d_frames, d_pts, d_offs, ang, radius=r, moments=mom)
    torch.cuda.synchronize()
    assert (flat[:lead] == 0xEE).all() and (flat[lead + f * stride:] == 0xEE).all()
    return ang.cpu().numpy(), mom.cpu().numpy() if moments else None


def check_frame(img, pts, r, host=True):
    """One frame through the device entry (and the host entry); returns the exact moments."""
    pts = np.ascontiguousarray(pts, dtype=np.uint32)
    want, _ = reference(img, pts, r)
    assert np.abs(want).max(initial=0) < 1 << 24
    offs = np.array([0, len(pts)], dtype=np.uint64)
    ang, mom = run_device(img[None], pts, offs, r)
    assert np.array_equal(mom, want)
    check_angles(ang, want)
    if host:
        h_ang, h_mom = fast_hip.keypoint_angles(img, pts, radius=r, moments=True)
        assert np.array_equal(h_mom, want)
        assert h_ang.tobytes() == ang.tobytes()
        assert fast_hip.keypoint_angles(img, pts, radius=r).tobytes() == ang.tobytes()
    return want, ang


def near_border(pts, shape, r):
    h, w = shape
    x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    return int(np.count_nonzero((x < r) | (y < r) | (x + r >= w) | (y + r >= h)))


@functools.lru_cache(maxsize=None)
def golden_points(which):
    return workloads.read_points(os.path.join(workloads.GOLDEN, f"kp_t16_n9_{which}.txt"))


# ---- 1: the golden frame ---------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2, 7, 15, 16, 31])
@pytest.mark.parametrize("which,count,border15", [("off", 309, 8), ("maxt", 131, 7)])
def test_golden_frame(which, count, border15, r):
    img = workloads.golden_image()
    pts = golden_points(which)
    assert img.shape == (200, 300) and len(pts) == count
    if r == 15:
        assert near_border(pts, img.shape, r) == border15
    if r >= 15:
        assert near_border(pts, img.shape, r) >= 1      # the clamped path is in the case set
        assert near_border(pts, img.shape, r) < count   # and so is the fast one
    want, ang = check_frame(img, pts, r)
    if r == 15:
        q = (ang >= 0).astype(int) * 2 + (np.abs(ang) > np.pi / 2).astype(int)
        assert all(np.count_nonzero(q == k) > 0 for k in range(4)), np.bincount(q, minlength=4)


# ---- 2: exact synthetic frames ---------------------------------------------------------------

def grid_points(w, h, step=5):
    xs = sorted(set(list(range(0, w, step)) + [w - 1]))
    ys = sorted(set(list(range(0, h, step)) + [h - 1]))
    return np.array([(x, y) for y in ys for x in xs], dtype=np.uint32)


@pytest.mark.parametrize("r", [3, 15])
def test_synthetic_gradients(r):
    w, h = 64, 48
    xs = np.broadcast_to(np.arange(w, dtype=np.uint8)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=np.uint8)[:, None], (h, w))
    pts = grid_points(w, h)
    mom, ang = check_frame(np.full((h, w), 93, np.uint8), pts, r)
    assert not mom.any() and np.all(ang == 0.0) and not np.signbit(ang).any()
    mom, ang = check_frame(np.ascontiguousarray(xs), pts, r)
    assert not mom[:, 1].any() and np.all(mom[:, 0] > 0) and np.all(ang == 0.0)
    mom, ang = check_frame(np.ascontiguousarray(63 - xs), pts, r)
    assert not mom[:, 1].any() and np.all(mom[:, 0] < 0) and np.all(ang == np.float32(np.pi))
    mom, ang = check_frame(np.ascontiguousarray(ys), pts, r)
    assert not mom[:, 0].any() and np.all(mom[:, 1] > 0)
    assert np.all(np.abs(ang.astype(np.float64) - np.pi / 2) <= ANGLE_TOL)
    mom, ang = check_frame(np.ascontiguousarray(47 - ys), pts, r)
    assert not mom[:, 0].any() and np.all(mom[:, 1] < 0)
    assert np.all(np.abs(ang.astype(np.float64) + np.pi / 2) <= ANGLE_TOL)


def test_largest_moment():
    """Left half 0, right half 255, r = 31, centred on the edge: every tap with d > 0 reads
    255 and every other tap 0 (or has weight 0), the largest m10 there is."""
    w, h, r = 64, 48, 31
    img = np.zeros((h, w), np.uint8)
    img[:, 32:] = 255
    pts = np.array([(32, 24), (31, 24)], dtype=np.uint32)
    mom, ang = check_frame(img, pts, r)
    u = disc(r)
    largest = 255 * sum(u[abs(v)] * (u[abs(v)] + 1) // 2 for v in range(-r, r + 1))
    assert largest < 1 << 24
    assert mom[0].tolist() == [largest, 0] and ang[0] == 0.0
    # the mirrored frame: the most negative m10
    mom, ang = check_frame(np.ascontiguousarray(img[:, ::-1]), pts, r)
    assert mom[1].tolist() == [-largest, 0] and ang[1] == np.float32(np.pi)


# ---- 3: frames smaller than the disc ---------------------------------------------------------

@pytest.mark.parametrize("r", [15, 31])
def test_frames_smaller_than_the_disc(r):
    img = workloads.s3_frame(3, 7, 7)
    check_frame(img, np.array([(3, 3)], dtype=np.uint32), r)
    for w, h in ((20, 64), (64, 20)):
        img = workloads.s3_frame(4, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
        assert near_border(pts, img.shape, r) == len(pts)
        check_frame(img, pts, r, host=(r == 15))


# ---- 4: dense input --------------------------------------------------------------------------

def test_dense_detections():
    img = workloads.s3_frame(1, 128, 96)
    pts = fast_hip.detect_array(img, Config(16, 9, NonMaximalSuppression.Off))
    assert len(pts) > 2000
    assert 0 < near_border(pts, img.shape, 15) < len(pts)
    check_frame(img, pts, 15)


def test_every_pixel():
    img = workloads.s3_frame(2, 67, 41)
    ys, xs = np.mgrid[0:41, 0:67]
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    check_frame(img, pts, 3)


# ---- 5: the batch contract -------------------------------------------------------------------

@pytest.mark.parametrize("moments", [True, False])
def test_batch_contract(moments):
    w, h, r = 96, 64, 15
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
    ang, mom = run_device(frames, pts, offs, r, cap=cap, moments=moments,
                          frame_stride=w * h + 37, lead=1, extra=16)
    want = np.concatenate([reference(frames[0], per[0], r)[0],
                           reference(frames[2], pts[int(offs[1]):cap], r)[0]])
    if moments:
        assert np.array_equal(mom[:cap], want)
        assert (mom[cap:] == MOMENT_FILL).all()
    check_angles(ang[:cap], want)
    assert (ang[cap:] == ANGLE_FILL).all()


def test_batch_contract_tail_untouched():
    """The offsets end below the capacity: the entries after them keep their fill."""
    w, h, r = 96, 64, 7
    frames = np.stack([workloads.s3_frame(12, w, h)] * 2)
    pts = grid_points(w, h, 7)
    k = len(pts)
    both = np.concatenate([pts, pts, np.full((40, 2), 0xFFFFFFFF, np.uint32)])
    offs = np.array([0, k, 2 * k], dtype=np.uint64)
    ang, mom = run_device(frames, both, offs, r, frame_stride=w * h + 1)
    want = reference(frames[0], pts, r)[0]
    assert np.array_equal(mom[:k], want) and np.array_equal(mom[k:2 * k], want)
    check_angles(ang[:2 * k], np.concatenate([want, want]))
    assert (ang[2 * k:] == ANGLE_FILL).all() and (mom[2 * k:] == MOMENT_FILL).all()


# ---- 6: the device chain ---------------------------------------------------------------------

def select_reference(pts, scores, shape, cell, k):
    """Best k per cell of one frame, ties to the earlier point, in input order."""
    h, w = shape
    cells_x = -(-w // cell[0])
    p = pts.astype(np.int64)
    cid = (p[:, 1] // cell[1]) * cells_x + p[:, 0] // cell[0]
    idx = np.arange(len(pts))
    order = np.lexsort((idx, -scores.astype(np.int64), cid))
    sc = cid[order]
    rank = idx - np.searchsorted(sc, sc, side="left")
    keep = np.zeros(len(pts), bool)
    keep[order[rank < k]] = True
    return pts[keep]


def test_device_chain():
    """detect_device -> score_device -> select_device -> orient_device on one stream with
    nothing in between, against oracle detection + numpy selection + numpy orientation."""
    import torch

    w, h, f, r = 256, 160, 3, 15
    frames = workloads.s1_frames_torch(4, f, w, h)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap = 20_000
    cell, k = (32, 32), 2
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(f + 1, dtype=torch.int64, device="cuda")
    scores = torch.zeros((cap,), dtype=torch.int16, device="cuda")
    sel = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((f + 1,), -1, dtype=torch.int64, device="cuda")
    ang = torch.full((cap,), ANGLE_FILL, dtype=torch.float32, device="cuda")
    mom = torch.full((cap, 2), MOMENT_FILL, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.detect_device(frames, cfg, out, offs)
        fast_hip.score_device(frames, cfg, out, offs, scores)
        fast_hip.select_device(out, scores, offs, (h, w), cell, k, sel, sel_sc, sel_offs)
        fast_hip.orient_device(frames, sel, sel_offs, ang, radius=r, moments=mom)
    stream.synchronize()
    h_frames = frames.cpu().numpy()
    want_pts, want_mom, want_offs = [], [], [0]
    for i in range(f):
        p, s = oracle.detect(h_frames[i], 16, 9, 1, with_scores=True)
        kept = select_reference(np.asarray(p, dtype=np.uint32).reshape(-1, 2),
                                np.asarray(s), (h, w), cell, k)
        want_pts.append(kept)
        want_mom.append(reference(h_frames[i], kept, r)[0])
        want_offs.append(want_offs[-1] + len(kept))
    want_pts = np.concatenate(want_pts)
    want_mom = np.concatenate(want_mom)
    n = want_offs[-1]
    assert n > 50
    assert sel_offs.cpu().numpy().tolist() == want_offs
    assert np.array_equal(sel[:n].cpu().numpy().view(np.uint32), want_pts)
    assert np.array_equal(mom[:n].cpu().numpy(), want_mom)
    check_angles(ang[:n].cpu().numpy(), want_mom)
    assert (ang[n:] == ANGLE_FILL).all() and (mom[n:] == MOMENT_FILL).all()


# ---- 7: argument errors ----------------------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    w, h = 96, 64
    frames = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    pts = torch.full((32, 2), 20, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, 32], dtype=torch.int64, device="cuda")
    ang = torch.full((32,), ANGLE_FILL, dtype=torch.float32, device="cuda")
    mom = torch.full((32, 2), MOMENT_FILL, dtype=torch.int32, device="cuda")
    lib = _native.load()
    ctx = fast_hip.context(0)
    good = dict(ctx=ctx.handle, frames=frames.data_ptr(), n=2, w=w, h=h, stride=w * h,
                pts=pts.data_ptr(), cap=32, offs=offs.data_ptr(), r=15, ang=ang.data_ptr(),
                mom=mom.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.fdf_orient_device(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["stride"],
                                     a["pts"], a["cap"], a["offs"], a["r"], a["ang"], a["mom"],
                                     None)

    for bad in (dict(r=0), dict(r=32), dict(ctx=None), dict(frames=None), dict(pts=None),
                dict(offs=None), dict(ang=None), dict(n=65536), dict(stride=w * h - 1)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(h=2) == _native.FDF_ERR_SIZE
    assert call(h=6) == _native.FDF_OK               # a shape with no keypoints: nothing to do
    assert call(n=0) == _native.FDF_OK
    assert call(cap=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (ang == ANGLE_FILL).all() and (mom == MOMENT_FILL).all()
    # the good call works, on the null stream and without moments
    assert call(mom=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (ang == 0.0).all() and (mom == MOMENT_FILL).all()


def test_host_entry_rejects_points_outside():
    img = workloads.golden_image()
    h, w = img.shape
    for bad in ((w, 5), (5, h), (0xFFFFFFFF, 0)):
        with pytest.raises(_native.FdfError) as info:
            fast_hip.keypoint_angles(img, np.array([(10, 10), bad], dtype=np.uint32))
        assert info.value.status == _native.FDF_ERR_ARG
    lib = _native.load()
    pts = np.array([(w, 5)], dtype=np.uint32)
    ang = np.zeros(1, np.float32)
    rc = lib.fdf_orient_points(fast_hip.context(0).handle, img.ctypes.data, w, h, w,
                               pts.ctypes.data, 1, 15, ang.ctypes.data, None)
    assert rc == _native.FDF_ERR_ARG
    assert fast_hip.keypoint_angles(img, np.zeros((0, 2), np.uint32)).shape == (0,)


def test_host_entry_keeps_fetch_last():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    fast_hip.keypoint_angles(img, pts)
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
    pts = grid_points(64, 50)
    want = reference(np.ascontiguousarray(view), pts, 15)[0]
    ang, mom = fast_hip.keypoint_angles(view, pts, moments=True)
    assert np.array_equal(mom, want)
    check_angles(ang, want)


def test_detect_oriented_array():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores, ang = fast_hip.detect_oriented_array(img, cfg)
    assert np.array_equal(pts, golden_points("maxt"))
    assert np.array_equal(scores, fast_hip.detect_scored_array(img, cfg)[1])
    assert ang.tobytes() == fast_hip.keypoint_angles(img, pts).tobytes()
    check_angles(ang, reference(img, pts, 15)[0])


# ---- 8: the C++ wrapper ----------------------------------------------------------------------

def test_cpp_orient_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_orient")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
