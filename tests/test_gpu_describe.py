"""Steered BRIEF descriptors and 5 x 5 box smoothing on the device (fdf_smooth_device,
fdf_describe_device, fdf_describe_points) against the numpy restatement of include/fdf.h's
semantics in tests/_brief_reference.py.  Everything is compared bit for bit."""
import ctypes
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import workloads
from _brief_reference import bin_scale, bins_of, default_table, describe, smooth, steer
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 0xEE
DESC_FILL = 0xA5


@functools.lru_cache(maxsize=None)
def golden_points(which):
    return workloads.read_points(os.path.join(workloads.GOLDEN, f"kp_t16_n9_{which}.txt"))


@functools.lru_cache(maxsize=None)
def golden_frame(smoothed):
    img = workloads.golden_image()
    img = smooth(img) if smoothed else img
    img.setflags(write=False)
    return img


def strided(torch, frames, stride, lead):
    """The frames on the device `stride` bytes apart, `lead` bytes into an allocation filled
    with GAP -> (the whole allocation, the (F, H, W) view)."""
    f, h, w = frames.shape
    flat = torch.full((lead + f * stride + 64,), GAP, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)
    return flat, view


def run_smooth(frames, in_stride=None, out_stride=None, lead_in=0, lead_out=0):
    """fdf_smooth_device on uploaded frames; checks that no byte outside the output frames
    changed and returns the smoothed frames."""
    import torch

    frames = np.array(frames)                            # a writable copy for torch
    f, h, w = frames.shape
    in_stride = h * w if in_stride is None else in_stride
    out_stride = h * w if out_stride is None else out_stride
    _, d_in = strided(torch, frames, in_stride, lead_in)
    d_in.copy_(torch.from_numpy(frames).cuda())
    flat_out, d_out = strided(torch, frames, out_stride, lead_out)
    fast_hip.smooth_device(d_in, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    d_out.fill_(GAP)                       # what is left must be the untouched fill
    assert (flat_out == GAP).all()
    assert np.array_equal(d_in.cpu().numpy(), frames)
    return got


def run_describe(frames, pts, offs, table, angles=None, cap=None, frame_stride=None, lead=0,
                 extra=0):
    """fdf_describe_device on uploaded arrays -> (cap + extra, 32) uint8, pre-filled."""
    import torch

    frames = np.array(frames)                            # a writable copy for torch
    f, h, w = frames.shape
    stride = h * w if frame_stride is None else frame_stride
    flat, d_frames = strided(torch, frames, stride, lead)
    d_frames.copy_(torch.from_numpy(frames).cuda())
    before = flat.clone()
    cap = len(pts) if cap is None else cap
    d_pts = torch.from_numpy(np.ascontiguousarray(pts[:cap]).view(np.int32)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()
    d_table = torch.from_numpy(np.array(table)).cuda()
    d_ang = None if angles is None else \
        torch.from_numpy(np.ascontiguousarray(angles[:cap], dtype=np.float32)).cuda()
    desc = torch.full((cap + extra, 32), DESC_FILL, dtype=torch.uint8, device="cuda")
    fast_hip.describe_device(d_frames, d_pts, d_offs, desc, d_table, table.shape[0],
                             angles=d_ang)
    torch.cuda.synchronize()
    assert torch.equal(flat, before)
    return desc.cpu().numpy()


def describe_frame(img, pts, table, angles=None):
    pts = np.ascontiguousarray(pts, dtype=np.uint32)
    offs = np.array([0, len(pts)], dtype=np.uint64)
    return run_describe(img[None], pts, offs, table, angles=angles)


def every_pixel(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)


def random_frame(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- 1: smoothing ----------------------------------------------------------------------------

def test_smooth_golden_frame():
    img = workloads.golden_image()
    got = run_smooth(img[None])[0]
    assert np.array_equal(got, golden_frame(True))
    assert zlib.crc32(got.tobytes()) == 485772551 and int(got.sum()) == 1481930


# widths below 8 run the thread-per-pixel kernel, 8 and above the strip kernel; 9, 11 and 67
# end in a partial column group; 70 and 200 rows are more than one strip
@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (5, 4), (7, 7), (67, 9), (8, 5), (9, 6), (11, 3),
                                 (12, 1), (13, 70), (1, 40), (1030, 17)])
def test_smooth_shapes(w, h):
    img = random_frame(100 + w, w, h)
    assert np.array_equal(run_smooth(img[None])[0], smooth(img))


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_smooth_unaligned_base(lead):
    for w, h in ((64, 24), (67, 9), (5, 4)):
        img = random_frame(lead, w, h)
        assert np.array_equal(run_smooth(img[None], lead_in=lead, lead_out=4 - lead)[0],
                              smooth(img))


def test_smooth_extreme_values():
    w, h = 67, 23
    full = np.full((h, w), 255, np.uint8)
    assert np.array_equal(run_smooth(full[None])[0], full)
    ys, xs = np.mgrid[0:h, 0:w]
    board = (((xs + ys) & 1) * 255).astype(np.uint8)
    got = run_smooth(board[None])[0]
    assert np.array_equal(got, smooth(board))
    assert set(np.unique(got[2:-2, 2:-2]).tolist()) == {122, 133}     # 12 or 13 of 25 set
    zero = np.zeros((h, w), np.uint8)
    assert np.array_equal(run_smooth(zero[None])[0], zero)


def test_smooth_batch_strides():
    w, h = 75, 31
    frames = np.stack([random_frame(7 + k, w, h) for k in range(3)])
    got = run_smooth(frames, in_stride=w * h + 13, out_stride=w * h + 50, lead_in=3, lead_out=1)
    for k in range(3):
        assert np.array_equal(got[k], smooth(frames[k])), k


# ---- 2: descriptors of the golden frame --------------------------------------------------------

def test_golden_pinned_values():
    pts = golden_points("off")
    assert len(pts) == 309
    pinned = {True: (1486779190, [155, 24, 224, 234, 2, 4, 200, 233], 37587),
              False: (2716640503, [15, 24, 177, 40, 2, 8, 116, 232], 37830)}
    for smoothed, (crc, first, bits) in pinned.items():
        img = golden_frame(smoothed)
        want = describe(img, pts, default_table(1))
        assert zlib.crc32(want.tobytes()) == crc                 # the reference itself
        for n_bins in (1, 30):                                   # no angles: bin 0 either way
            got = describe_frame(img, pts, default_table(n_bins))
            assert np.array_equal(got, want)
            assert zlib.crc32(got.tobytes()) == crc
            assert got[0, :8].tolist() == first
            assert int(np.unpackbits(got).sum()) == bits
        host = fast_hip.keypoint_descriptors(workloads.golden_image(), pts, n_bins=1,
                                             smooth=smoothed)
        assert zlib.crc32(host.tobytes()) == crc


@pytest.mark.parametrize("n_bins", [1, 30])
@pytest.mark.parametrize("which,count", [("off", 309), ("maxt", 131)])
def test_golden_frame_steered(which, count, n_bins):
    import torch

    raw = workloads.golden_image()
    pts = golden_points(which)
    assert len(pts) == count
    # the angles orient_device gives these points on the raw frame
    d_ang = torch.zeros(count, dtype=torch.float32, device="cuda")
    fast_hip.orient_device(torch.from_numpy(raw[None]).cuda(),
                           torch.from_numpy(pts.view(np.int32)).cuda(),
                           torch.tensor([0, count], dtype=torch.int64, device="cuda"), d_ang)
    angles = d_ang.cpu().numpy()
    assert np.array_equal(angles, fast_hip.keypoint_angles(raw, pts))
    bins = bins_of(angles, n_bins)
    if n_bins == 30:
        assert len(np.unique(bins)) > 10
    table = default_table(n_bins)
    for smoothed in (False, True):
        img = golden_frame(smoothed)
        want = describe(img, pts, table, bins)
        assert np.array_equal(describe_frame(img, pts, table, angles), want)
        assert np.array_equal(describe_frame(img, pts, table), describe(img, pts, table))
        host = fast_hip.keypoint_descriptors(raw, pts, angles, n_bins=n_bins, smooth=smoothed)
        assert np.array_equal(host, want)


# ---- 3: borders --------------------------------------------------------------------------------

def test_every_pixel_of_a_small_frame():
    w, h = 24, 20
    img = random_frame(31, w, h)
    pts = every_pixel(w, h)
    angles = np.random.default_rng(32).uniform(-np.pi, np.pi, len(pts)).astype(np.float32)
    table = default_table(30)
    want = describe(img, pts, table, bins_of(angles, 30))
    assert np.array_equal(describe_frame(img, pts, table, angles), want)
    assert np.array_equal(fast_hip.keypoint_descriptors(img, pts, angles, smooth=False), want)
    want = describe(smooth(img), pts, table, bins_of(angles, 30))
    assert np.array_equal(fast_hip.keypoint_descriptors(img, pts, angles), want)


def test_frame_of_3_by_3():
    """Every tap of every point is clamped.  The host entry takes any shape; the device entry
    treats the shapes the detector answers with an empty list as fdf_orient_device does:
    FDF_OK, nothing written."""
    img = random_frame(33, 3, 3)
    pts = every_pixel(3, 3)
    angles = np.linspace(-3, 3, 9).astype(np.float32)
    table = default_table(12)
    for smoothed in (False, True):
        want = describe(smooth(img) if smoothed else img, pts, table, bins_of(angles, 12))
        got = fast_hip.keypoint_descriptors(img, pts, angles, n_bins=12, smooth=smoothed)
        assert np.array_equal(got, want)
    assert (describe_frame(img, pts, table, angles) == DESC_FILL).all()
    img7 = random_frame(34, 7, 7)                    # the smallest shape with keypoints
    pts7 = every_pixel(7, 7)
    assert np.array_equal(describe_frame(img7, pts7, table), describe(img7, pts7, table))


# ---- 4: a custom pattern -----------------------------------------------------------------------

def test_custom_pattern_with_extreme_offsets():
    rng = np.random.default_rng(41)
    pat = rng.integers(-128, 128, size=(256, 4), dtype=np.int64).astype(np.int8)
    pat[0] = (-128, -128, 127, 127)
    pat[1] = (127, -128, -128, 127)
    pat[2] = (-128, 0, 127, 0)
    pat[3] = (0, 127, 0, -128)
    n_bins = 12
    table = steer(pat, n_bins)
    assert np.array_equal(table, fast_hip.brief_steer(pat, n_bins))
    assert table.min() == -128 and table.max() == 127
    for img in (workloads.golden_image(), random_frame(42, 24, 20)):
        h, w = img.shape
        pts = every_pixel(w, h)[::7]
        angles = rng.uniform(-np.pi, np.pi, len(pts)).astype(np.float32)
        want = describe(img, pts, table, bins_of(angles, n_bins))
        assert np.array_equal(describe_frame(img, pts, table, angles), want)
        host = fast_hip.keypoint_descriptors(img, pts, angles, pattern=pat, n_bins=n_bins,
                                             smooth=False)
        assert np.array_equal(host, want)


# ---- 5: bin boundaries -------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins", [1, 7, 30, 360])
def test_bin_boundaries(n_bins):
    """The angles at which the product lands on k + 0.5, their float32 neighbours, and the
    values the bin rule names."""
    scale = float(bin_scale(n_bins))
    ks = np.arange(-n_bins, n_bins, dtype=np.float64)
    mid = ((ks + 0.5) / scale).astype(np.float32)
    special = np.array([np.pi, -np.pi, 0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0, 7.0,
                        -7.0, np.nextafter(np.float32(7), np.float32(8))], dtype=np.float32)
    angles = np.concatenate([mid, np.nextafter(mid, np.float32(-10)),
                             np.nextafter(mid, np.float32(10)), special]).astype(np.float32)
    assert np.all(np.abs(angles[:-len(special)]) < 7)
    bins = bins_of(angles, n_bins)
    assert bins.min() == 0 and bins.max() == n_bins - 1
    if n_bins > 1:
        assert len(np.unique(bins)) == n_bins
    assert bins[-8:-3].tolist() == [0] * 5 and bins[-1] == 0   # NaN, +-inf, +-100, above 7
    img = random_frame(51, 40, 36)
    pts = np.tile(np.array([[19, 17]], dtype=np.uint32), (len(angles), 1))
    table = default_table(n_bins)
    per_bin = describe(img, np.tile(pts[:1], (n_bins, 1)), table, np.arange(n_bins))
    assert len({d.tobytes() for d in per_bin}) > 0.9 * n_bins  # a wrong bin shows
    got = describe_frame(img, pts, table, angles)
    assert np.array_equal(got, per_bin[bins])


# ---- 6: the batch contract ---------------------------------------------------------------------

@pytest.mark.parametrize("with_angles", [True, False])
def test_batch_contract(with_angles):
    w, h, n_bins = 96, 64, 30
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
    angles = np.random.default_rng(61).uniform(-np.pi, np.pi, total).astype(np.float32) \
        if with_angles else None
    table = default_table(n_bins)
    got = run_describe(frames, pts, offs, table, angles=angles, cap=cap,
                       frame_stride=w * h + 37, lead=1, extra=16)
    bins = bins_of(angles, n_bins) if with_angles else np.zeros(total, np.int64)
    k = int(offs[1])
    want = np.concatenate([describe(frames[0], pts[:k], table, bins[:k]),
                           describe(frames[2], pts[k:cap], table, bins[k:cap])])
    assert np.array_equal(got[:cap], want)
    assert (got[cap:] == DESC_FILL).all()


def test_batch_contract_tail_untouched():
    """The offsets end below the capacity: the entries after them keep their fill."""
    w, h = 96, 64
    frames = np.stack([workloads.s3_frame(12, w, h)] * 2)
    pts = every_pixel(w, h)[::41]
    k = len(pts)
    both = np.concatenate([pts, pts, np.full((40, 2), 0xFFFFFFFF, np.uint32)])
    offs = np.array([0, k, 2 * k], dtype=np.uint64)
    table = default_table(4)
    got = run_describe(frames, both, offs, table, frame_stride=w * h + 1)
    want = describe(frames[0], pts, table)
    assert np.array_equal(got[:k], want) and np.array_equal(got[k:2 * k], want)
    assert (got[2 * k:] == DESC_FILL).all()


def test_points_outside_the_frame_are_safe():
    """Unspecified descriptors, but nothing outside the buffers is touched and the points
    inside are right."""
    w, h = 40, 30
    img = random_frame(62, w, h)
    pts = np.array([(5, 5), (w, 5), (5, h), (0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 3), (39, 29)],
                   dtype=np.uint32)
    angles = np.array([0.5, np.nan, 1e30, -1e30, 6.9, -2.0], dtype=np.float32)
    table = default_table(30)
    got = describe_frame(img, pts, table, angles)
    want = describe(img, pts[[0, 5]], table, bins_of(angles[[0, 5]], 30))
    assert np.array_equal(got[[0, 5]], want)


# ---- 7: the rotation property ------------------------------------------------------------------

def test_quarter_turn_of_the_frame():
    """At 4 bins a bin step is an exact quarter turn of the pattern, so the descriptor of
    (x, y) at angle a in a frame equals that of the turned point at angle a + pi / 2 in the
    frame turned the same way (y pointing down: (x, y) -> (h - 1 - y, x), np.rot90(k=-1))."""
    w, h, margin = 61, 47, 13
    a_img = random_frame(71, w, h)
    b_img = np.ascontiguousarray(np.rot90(a_img, k=-1))
    assert b_img.shape == (w, h) and b_img[5, h - 1 - 3] == a_img[3, 5]
    ys, xs = np.mgrid[margin:h - margin:3, margin:w - margin:3]
    a_pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    b_pts = np.stack([h - 1 - a_pts[:, 1], a_pts[:, 0]], axis=1).astype(np.uint32)
    rng = np.random.default_rng(72)
    a_ang = (rng.integers(0, 4, len(a_pts)) * (np.pi / 2) +
             rng.uniform(-0.5, 0.5, len(a_pts))).astype(np.float32)
    b_ang = (a_ang.astype(np.float64) + np.pi / 2).astype(np.float32)
    assert np.array_equal((bins_of(a_ang, 4) + 1) % 4, bins_of(b_ang, 4))
    table = default_table(4)
    a_desc = describe_frame(a_img, a_pts, table, a_ang)
    assert np.array_equal(a_desc, describe(a_img, a_pts, table, bins_of(a_ang, 4)))
    assert np.array_equal(describe_frame(b_img, b_pts, table, b_ang), a_desc)
    # the other sense of rotation does not: the sign of the angle is pinned
    wrong = (a_ang.astype(np.float64) - np.pi / 2).astype(np.float32)
    assert not np.array_equal(describe_frame(b_img, b_pts, table, wrong), a_desc)


# ---- 8: the device chain -----------------------------------------------------------------------

def test_device_chain():
    """detect -> score -> select -> orient -> smooth -> describe on one stream with nothing in
    between, against the host entries and the numpy reference."""
    import torch

    w, h, r, n_bins = 300, 200, 15, 30
    img = workloads.golden_image()
    frames = torch.from_numpy(np.stack([img, np.ascontiguousarray(img[::-1])])).cuda()
    f = frames.shape[0]
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap = 4096
    cell, k = (32, 32), 2
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(f + 1, dtype=torch.int64, device="cuda")
    scores = torch.zeros((cap,), dtype=torch.int16, device="cuda")
    sel = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    sel_sc = torch.full((cap,), -1, dtype=torch.int16, device="cuda")
    sel_offs = torch.full((f + 1,), -1, dtype=torch.int64, device="cuda")
    ang = torch.full((cap,), -77.0, dtype=torch.float32, device="cuda")
    smoothed = torch.full((f, h, w), GAP, dtype=torch.uint8, device="cuda")
    desc = torch.full((cap, 32), DESC_FILL, dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.detect_device(frames, cfg, out, offs)
        fast_hip.score_device(frames, cfg, out, offs, scores)
        fast_hip.select_device(out, scores, offs, (h, w), cell, k, sel, sel_sc, sel_offs)
        fast_hip.orient_device(frames, sel, sel_offs, ang, radius=r)
        fast_hip.smooth_device(frames, smoothed)
        fast_hip.describe_device(smoothed, sel, sel_offs, desc, table, n_bins, angles=ang)
    stream.synchronize()
    so = sel_offs.cpu().numpy()
    n = int(so[-1])
    assert 20 < n < cap and int(offs[-1]) > n            # the selection dropped points
    h_frames = frames.cpu().numpy()
    got_pts = sel[:n].cpu().numpy().view(np.uint32)
    got_ang = ang[:n].cpu().numpy()
    got_desc = desc.cpu().numpy()
    assert (got_desc[n:] == DESC_FILL).all()
    assert np.array_equal(smoothed.cpu().numpy(), np.stack([smooth(x) for x in h_frames]))
    for i in range(f):
        lo, hi = int(so[i]), int(so[i + 1])
        p, a, d = got_pts[lo:hi], got_ang[lo:hi], got_desc[lo:hi]
        # the host entries on the same points
        assert np.array_equal(fast_hip.keypoint_angles(h_frames[i], p, r), a)
        assert np.array_equal(fast_hip.keypoint_descriptors(h_frames[i], p, a, n_bins=n_bins), d)
        assert np.array_equal(describe(smooth(h_frames[i]), p, default_table(n_bins),
                                       bins_of(a, n_bins)), d)
        # detect_described_array on the frame: the selected points are a subset of its points
        all_pts, all_ang, all_desc = fast_hip.detect_described_array(h_frames[i], cfg, r, n_bins)
        index = {tuple(q): j for j, q in enumerate(all_pts.tolist())}
        rows = [index[tuple(q)] for q in p.tolist()]
        assert np.array_equal(all_ang[rows], a) and np.array_equal(all_desc[rows], d)


def test_detect_described_array():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, ang, desc = fast_hip.detect_described_array(img, cfg)
    assert np.array_equal(pts, golden_points("maxt"))
    assert np.array_equal(ang, fast_hip.keypoint_angles(img, pts))
    assert desc.shape == (131, 32) and desc.dtype == np.uint8
    assert np.array_equal(desc, describe(smooth(img), pts, default_table(30), bins_of(ang, 30)))


# ---- 9: argument errors and the host entry -----------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    w, h = 96, 64
    frames = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    pts = torch.full((32, 2), 20, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 16, 32], dtype=torch.int64, device="cuda")
    ang = torch.zeros((32,), dtype=torch.float32, device="cuda")
    table = torch.from_numpy(np.array(default_table(4))).cuda()
    desc = torch.full((32, 32), DESC_FILL, dtype=torch.uint8, device="cuda")
    smoothed = torch.full((2, h, w), GAP, dtype=torch.uint8, device="cuda")
    lib = _native.load()
    ctx = fast_hip.context(0)
    good = dict(ctx=ctx.handle, frames=frames.data_ptr(), n=2, w=w, h=h, stride=w * h,
                pts=pts.data_ptr(), cap=32, offs=offs.data_ptr(), ang=ang.data_ptr(),
                table=table.data_ptr(), bins=4, desc=desc.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.fdf_describe_device(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["stride"],
                                       a["pts"], a["cap"], a["offs"], a["ang"], a["table"],
                                       a["bins"], a["desc"], None)

    for bad in (dict(bins=0), dict(bins=361), dict(ctx=None), dict(frames=None), dict(pts=None),
                dict(offs=None), dict(table=None), dict(desc=None), dict(n=65536),
                dict(stride=w * h - 1)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(h=2) == _native.FDF_ERR_SIZE
    assert call(h=6) == _native.FDF_OK               # a shape with no keypoints: nothing to do
    assert call(n=0) == _native.FDF_OK
    assert call(cap=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (desc == DESC_FILL).all()
    # the good call works, on the null stream and without angles
    assert call(ang=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (desc == 0).all()                         # a constant frame: no test is true

    sgood = dict(ctx=ctx.handle, frames=frames.data_ptr(), n=2, w=w, h=h, stride=w * h,
                 out=smoothed.data_ptr(), ostride=w * h)

    def scall(**kw):
        a = dict(sgood)
        a.update(kw)
        return lib.fdf_smooth_device(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["stride"],
                                     a["out"], a["ostride"], None)

    for bad in (dict(ctx=None), dict(frames=None), dict(out=None), dict(n=65536),
                dict(stride=w * h - 1), dict(ostride=w * h - 1)):
        assert scall(**bad) == _native.FDF_ERR_ARG, bad
    for bad in (dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 15)):
        assert scall(**bad) == _native.FDF_ERR_SIZE, bad
    assert scall(n=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (smoothed == GAP).all()
    assert scall() == _native.FDF_OK
    torch.cuda.synchronize()
    assert (smoothed == 0).all()


def test_host_entry_rejects_bad_arguments():
    img = workloads.golden_image()
    h, w = img.shape
    for bad in ((w, 5), (5, h), (0xFFFFFFFF, 0)):
        with pytest.raises(_native.FdfError) as info:
            fast_hip.keypoint_descriptors(img, np.array([(10, 10), bad], dtype=np.uint32))
        assert info.value.status == _native.FDF_ERR_ARG
    lib = _native.load()
    ctx = fast_hip.context(0).handle
    pts = np.array([(10, 10)], dtype=np.uint32)
    desc = np.full(32, DESC_FILL, np.uint8)

    def call(width=w, stride=w, p=pts.ctypes.data, bins=30, sm=1, out=desc.ctypes.data, c=ctx):
        return lib.fdf_describe_points(c, img.ctypes.data, width, h, stride, p, 1, None, None,
                                       bins, sm, out)

    assert call(bins=0) == _native.FDF_ERR_ARG
    assert call(bins=361) == _native.FDF_ERR_ARG
    assert call(sm=2) == _native.FDF_ERR_ARG
    assert call(stride=w - 1) == _native.FDF_ERR_ARG
    assert call(p=None) == _native.FDF_ERR_ARG
    assert call(out=None) == _native.FDF_ERR_ARG
    assert call(c=None) == _native.FDF_ERR_ARG
    assert call(width=10) == _native.FDF_ERR_ARG       # the point is outside 10 columns
    assert (desc == DESC_FILL).all()
    assert call() == _native.FDF_OK
    assert np.array_equal(desc[None], describe(golden_frame(True), pts, default_table(1)))
    assert fast_hip.keypoint_descriptors(img, np.zeros((0, 2), np.uint32)).shape == (0, 32)


def test_host_entry_keeps_fetch_last():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    fast_hip.keypoint_descriptors(img, pts)
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
    pts = every_pixel(64, 50)[::13]
    angles = np.random.default_rng(91).uniform(-np.pi, np.pi, len(pts)).astype(np.float32)
    img = np.ascontiguousarray(view)
    for smoothed in (False, True):
        want = describe(smooth(img) if smoothed else img, pts, default_table(30),
                        bins_of(angles, 30))
        assert np.array_equal(fast_hip.keypoint_descriptors(view, pts, angles, smooth=smoothed),
                              want)


# ---- 10: the C++ wrapper -----------------------------------------------------------------------

def test_cpp_describe_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_describe")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
