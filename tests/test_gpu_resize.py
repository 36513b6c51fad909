"""Exact bilinear resize, the scale pyramid and multi-scale detection on the device
(fdf_resize_device, fdf_pyramid_device, fdf_resize_frame) against the numpy restatement of
include/fdf.h's rules in tests/_resize_reference.py.  Everything is compared bit for bit."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import workloads
from _resize_reference import level_sizes, pyramid, resize, taps, to_level0
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 0xEE


def random_frame(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def strided(torch, f, h, w, stride, lead):
    """f frames of h x w on the device `stride` bytes apart, `lead` bytes into an allocation
    filled with GAP -> (the whole allocation, the (F, H, W) view)."""
    flat = torch.full((lead + f * stride + 64,), GAP, dtype=torch.uint8, device="cuda")
    return flat, torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)


def device_taps(torch, table):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint32).view(np.int32)).cuda()


def run_resize(frames, dw, dh, in_stride=None, out_stride=None, lead_in=0, lead_out=0,
               xtaps=None, ytaps=None):
    """fdf_resize_device on uploaded frames; checks that no byte outside the output frames
    changed and that the input is intact, and returns the resized frames."""
    import torch

    frames = np.array(frames)                            # a writable copy for torch
    f, h, w = frames.shape
    in_stride = h * w if in_stride is None else in_stride
    out_stride = dh * dw if out_stride is None else out_stride
    _, d_in = strided(torch, f, h, w, in_stride, lead_in)
    d_in.copy_(torch.from_numpy(frames).cuda())
    flat_out, d_out = strided(torch, f, dh, dw, out_stride, lead_out)
    fast_hip.resize_device(d_in, d_out,
                           xtaps=None if xtaps is None else device_taps(torch, xtaps),
                           ytaps=None if ytaps is None else device_taps(torch, ytaps))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    d_out.fill_(GAP)                       # what is left must be the untouched fill
    assert (flat_out == GAP).all()
    assert np.array_equal(d_in.cpu().numpy(), frames)
    return got


# ---- 1: shapes -------------------------------------------------------------------------------

# a source narrower than 8, a destination narrower than 4 or a ratio above 2 run the
# thread-per-pixel kernel, the others the strip kernel; 31, 53, 33 and 858 end in a partial
# column group; 858 rows are more than one strip
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((2, 2), (1, 1)), ((5, 3), (4, 2)),
          ((37, 23), (31, 19)), ((64, 48), (53, 40)), ((41, 41), (20, 20)), ((40, 40), (20, 20)),
          ((100, 60), (33, 20)), ((20, 20), (47, 31)), ((1030, 9), (858, 8)),
          ((9, 1030), (8, 858))] + [((9, 9), (w, 5)) for w in (1, 2, 3, 5, 6, 7)]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_shapes(src, dst):
    img = random_frame(src[0] + 7 * dst[0], *src)
    assert np.array_equal(run_resize(img[None], *dst)[0], resize(img, *dst))


def test_paths_cover_both_kernels():
    """The shapes above reach both kernels: the host picks by the horizontal ratio."""
    fast = lambda sw, dw: sw >= 8 and dw >= 4 and sw <= 2 * dw
    picks = {fast(s[0], d[0]) for s, d in SHAPES}
    assert picks == {True, False}
    assert fast(40, 20) and not fast(41, 20) and not fast(100, 33) and fast(20, 47)


def test_same_size_is_the_identity():
    img = random_frame(3, 7, 7)
    assert np.array_equal(run_resize(img[None], 7, 7)[0], img)
    img = random_frame(4, 67, 9)
    assert np.array_equal(run_resize(img[None], 67, 9)[0], img)


def test_halving_is_the_rounded_block_mean():
    img = random_frame(5, 16, 16)
    mean = (img.reshape(8, 2, 8, 2).astype(np.int64).sum((1, 3)) + 2) // 4
    assert np.array_equal(run_resize(img[None], 8, 8)[0], mean)


def test_golden_frame_at_6_over_5():
    img = workloads.golden_image()
    h, w = img.shape
    (dw, dh) = level_sizes(w, h, 2)[1]
    assert (dw, dh) == (250, 167)
    want = resize(img, dw, dh)
    assert np.array_equal(run_resize(img[None], dw, dh)[0], want)
    assert np.array_equal(fast_hip.resize_array(img, (dh, dw)), want)


@pytest.mark.parametrize("dst", [(31, 19), (75, 50), (10, 7)])
def test_constant_255_stays_255(dst):
    full = np.full((23, 37), 255, np.uint8)
    assert (run_resize(full[None], *dst) == 255).all()
    assert not run_resize(np.zeros((1, 23, 37), np.uint8), *dst).any()


# ---- 2: strides, alignment, tables -----------------------------------------------------------

@pytest.mark.parametrize("dst", [(62, 26), (20, 9)])
def test_batch_with_gaps_on_both_sides(dst):
    w, h = 75, 31
    frames = np.stack([random_frame(7 + k, w, h) for k in range(3)])
    got = run_resize(frames, *dst, in_stride=w * h + 13, out_stride=dst[0] * dst[1] + 50,
                     lead_in=3, lead_out=1)
    for k in range(3):
        assert np.array_equal(got[k], resize(frames[k], *dst)), k


@pytest.mark.parametrize("lead", [1, 3])
def test_unaligned_bases(lead):
    for src, dst in (((64, 24), (53, 20)), ((67, 9), (56, 8)), ((5, 4), (3, 3))):
        img = random_frame(lead, *src)
        got = run_resize(img[None], *dst, lead_in=lead, lead_out=4 - lead)[0]
        assert np.array_equal(got, resize(img, *dst))


@pytest.mark.parametrize("src,dst", [((64, 48), (53, 40)), ((41, 41), (20, 20))])
def test_out_of_range_tables_stay_inside(src, dst):
    """Entries no table of fdf_resize_taps holds (i0 = 0xFFFFF, q = 4095): both kernels clamp
    every entry before use (decode_tap: i0 <= S - 1, q <= 2048; the strip kernel also clamps its
    byte selectors into the 8 loaded bytes) and address through buffer resources of exactly the
    frames' bytes, so the call completes inside the frames; the values are unspecified."""
    img = random_frame(11, *src)
    bad = np.uint32(0xFFFFF << 12 | 4095)
    xt, yt = taps(src[0], dst[0]), taps(src[1], dst[1])
    xt[::3] = bad
    yt[1::4] = bad
    got = run_resize(np.stack([img, img]), *dst, in_stride=src[0] * src[1] + 5,
                     out_stride=dst[0] * dst[1] + 9, lead_in=1, lead_out=2, xtaps=xt, ytaps=yt)
    assert got.shape == (2, dst[1], dst[0])
    assert np.array_equal(got[0], got[1])
    all_bad = np.full(max(dst), bad, dtype=np.uint32)
    got = run_resize(img[None], *dst, xtaps=all_bad[:dst[0]], ytaps=all_bad[:dst[1]])
    assert got.shape == (1, dst[1], dst[0])


def test_rejected_calls():
    """What fdf_resize_device must reject, synchronously and with nothing launched."""
    import torch

    lib = _native.load()
    ctx = fast_hip.context(0).handle
    src = torch.full((3 * 64,), 1, dtype=torch.uint8, device="cuda")
    dst = torch.full((3 * 16,), GAP, dtype=torch.uint8, device="cuda")
    xt = device_taps(torch, taps(8, 4))
    s, d, t = src.data_ptr(), dst.data_ptr(), xt.data_ptr()

    def call(d_src=s, n=3, sw=8, sh=8, ss=64, d_dst=d, dw=4, dh=4, ds=16, x=t, y=t, c=ctx):
        return lib.fdf_resize_device(c, d_src, n, sw, sh, ss, d_dst, dw, dh, ds, x, y, None)

    A, S = _native.FDF_ERR_ARG, _native.FDF_ERR_SIZE
    assert call(c=None) == A
    assert call(d_src=None) == A and call(d_dst=None) == A and call(x=None) == A and \
        call(y=None) == A
    assert call(n=65536) == A
    assert call(ss=63) == A and call(ds=15) == A              # frames closer than their size
    assert call(sw=0) == S and call(sh=0) == S and call(dw=0) == S and call(dh=0) == S
    assert call(sw=65535, sh=65535) == S                      # above 2^31 - 256 pixels
    assert call(dw=65536, dh=65536) == S
    assert call(sw=65536, sh=1) == S                          # a side no tap word can index
    assert call(n=0) == _native.FDF_OK
    assert call(n=1, ss=0, ds=0) == _native.FDF_OK            # one frame: the strides are not read
    torch.cuda.synchronize()
    assert (dst[16:] == GAP).all() and (dst[:16] == 1).all()
    plan = fast_hip.pyramid_plan((8, 8), 2, (2, 1), n_frames=3)
    assert lib.fdf_pyramid_device(ctx, s, 3, 63, plan._c, 2, d, t, None) == A
    assert lib.fdf_pyramid_device(ctx, None, 3, 64, plan._c, 2, d, t, None) == A
    assert lib.fdf_pyramid_device(ctx, s, 3, 64, plan._c, 0, d, t, None) == A
    assert lib.fdf_pyramid_device(ctx, None, 3, 64, plan._c, 1, None, None, None) == _native.FDF_OK


# ---- 3: the pyramid --------------------------------------------------------------------------

def test_pyramid_device_three_frames():
    import torch

    w, h, n = 97, 61, 4
    frames = np.stack([random_frame(20 + k, w, h) for k in range(3)])
    _, d_frames = strided(torch, 3, h, w, w * h + 11, 1)
    d_frames.copy_(torch.from_numpy(frames).cuda())
    pyr = fast_hip.Pyramid(d_frames, n, (6, 5), build=False)
    pyr.buffer.fill_(GAP)
    pyr.build()
    torch.cuda.synchronize()
    assert pyr.level(0) is d_frames
    want = [pyramid(f, n) for f in frames]
    used = torch.zeros_like(pyr.buffer, dtype=torch.bool)
    for l in range(1, n):
        level = pyr.level(l)
        assert level.is_contiguous() and level.shape == (3, *want[0][l].shape)
        for k in range(3):
            assert np.array_equal(level[k].cpu().numpy(), want[k][l]), (l, k)
        L = pyr.plan.levels[l]
        used[L.offset_bytes:L.offset_bytes + 3 * L.frame_stride_bytes] = True
    assert (pyr.buffer[~used] == GAP).all()              # the alignment gaps are not written
    assert np.array_equal(d_frames.cpu().numpy(), frames)


def test_pyramid_level_feeds_detect_device():
    import torch

    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pyr = fast_hip.Pyramid(torch.from_numpy(np.array(img)[None]).cuda(), 3)
    want_levels = pyramid(img, 3)
    for l in range(3):
        level = pyr.level(l)
        pts = torch.zeros((4096, 2), dtype=torch.int32, device="cuda")
        offs = torch.zeros(2, dtype=torch.int64, device="cuda")
        fast_hip.detect_device(level, cfg, pts, offs)
        n = int(offs[1])
        want = fast_hip.detect_array(want_levels[l], cfg)
        assert n == len(want) and n > 0
        assert np.array_equal(pts[:n].cpu().numpy().view(np.uint32), want)


def test_resize_array_and_strided_host_rows():
    img = random_frame(31, 97, 61)
    for dst in ((81, 51), (97, 61), (40, 25), (131, 80)):
        assert np.array_equal(fast_hip.resize_array(img, (dst[1], dst[0])), resize(img, *dst))
    wide = random_frame(32, 120, 61)
    assert np.array_equal(fast_hip.resize_array(wide[:, 5:102], (51, 81)),
                          resize(wide[:, 5:102], 81, 51))


def test_resize_frame_keeps_the_retained_result(golden):
    """fdf_resize_frame leaves the context's retained detection alone: fdf_fetch_last still
    returns it."""
    img, _, maxt = golden
    lib = _native.load()
    ctx = fast_hip.context(0)
    cfg = _native.FdfConfig(16, 9, 1)
    few = np.zeros((4, 2), dtype=np.uint32)
    n = ctypes.c_size_t(0)
    with ctx.lock:
        rc = lib.fdf_detect(ctx.handle, img.ctypes.data, img.shape[1], img.shape[0],
                            img.strides[0], ctypes.byref(cfg), few.ctypes.data, 4,
                            ctypes.byref(n))
        assert rc == _native.FDF_ERR_CAPACITY and n.value == len(maxt)
        assert np.array_equal(fast_hip.resize_array(img, (167, 250)), resize(img, 250, 167))
        out = np.zeros((n.value, 2), dtype=np.uint32)
        rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data, None, n.value, ctypes.byref(n))
    assert rc == _native.FDF_OK and np.array_equal(out, maxt)


def test_cpp_smoke_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_pyramid")
    assert os.path.exists(exe), "run `make` first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout


# ---- 4: multi-scale detection ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_levels():
    levels = pyramid(workloads.golden_image(), 3)
    for level in levels:
        level.setflags(write=False)
    return levels


@pytest.mark.parametrize("nms", [NonMaximalSuppression.MaxThreshold, NonMaximalSuppression.Off])
def test_detect_multiscale_equals_the_chain_per_level(nms):
    img = workloads.golden_image()
    cfg = Config(16, 9, nms)
    got = fast_hip.detect_multiscale_array(img, cfg, n_levels=3)
    h, w = img.shape
    assert got.sizes == tuple(level_sizes(w, h, 3))
    assert np.all(np.diff(got.level) >= 0) and set(got.level.tolist()) == {0, 1, 2}
    for l, level in enumerate(golden_levels()):
        part = got.level == l
        pts, angles, desc = fast_hip.detect_described_array(level, cfg)
        _, scores = fast_hip.detect_scored_array(level, cfg)
        assert len(pts) > 0
        assert np.array_equal(got.points[part], pts)
        assert np.array_equal(got.scores[part], scores)
        assert got.angles.dtype == np.float32 and np.array_equal(got.angles[part], angles)
        assert np.array_equal(got.descriptors[part], desc)
        want0 = to_level0(pts, got.sizes[0], got.sizes[l])
        assert got.points0.dtype == np.float32 and np.array_equal(got.points0[part], want0)
        if l == 0:
            assert np.array_equal(got.points0[part], pts.astype(np.float32))


def test_detect_multiscale_with_selection():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    got = fast_hip.detect_multiscale_array(img, cfg, n_levels=3, cell=(64, 64), k=2)
    everything = fast_hip.detect_multiscale_array(img, cfg, n_levels=3)
    assert 0 < len(got.points) < len(everything.points)
    for l, level in enumerate(golden_levels()):
        part = got.level == l
        pts, scores = fast_hip.detect_scored_array(level, cfg)
        sel, sel_scores = fast_hip.select_best(pts, scores, level.shape, (64, 64), 2)
        assert np.array_equal(got.points[part], sel)
        assert np.array_equal(got.scores[part], sel_scores)
        angles = fast_hip.keypoint_angles(level, sel)
        assert np.array_equal(got.angles[part], angles)
        assert np.array_equal(got.descriptors[part],
                              fast_hip.keypoint_descriptors(level, sel, angles))


def test_detect_multiscale_small_levels_and_empty_frames():
    """Levels with a side below 7 hold no keypoint and are skipped; a flat frame has none."""
    cfg = Config(16, 9)
    flat = fast_hip.detect_multiscale_array(np.zeros((40, 40), np.uint8), cfg, n_levels=4)
    assert len(flat.points) == 0 and flat.descriptors.shape == (0, 32)
    img = workloads.s3_frame(10, 24, 20)
    got = fast_hip.detect_multiscale_array(img, cfg, n_levels=4, scale=(2, 1))
    assert got.sizes == ((24, 20), (12, 10), (6, 5), (3, 3))
    assert set(got.level.tolist()) <= {0, 1}
    assert np.array_equal(got.points[got.level == 0], fast_hip.detect_array(img, cfg))
