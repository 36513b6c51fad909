"""CPU tests of the resize and pyramid host functions (fdf_resize_taps, fdf_pyramid_plan,
fdf_pyramid_taps) against tests/_resize_reference.py, and of the wrappers' argument checks, which
run before any device call."""
import ctypes
import zlib

import numpy as np
import pytest

from _resize_reference import level_sizes, resize, tap, taps, to_level0
from feature_detector_fast_amd import Config, FdfError, _native, fast_hip

SENTINEL = 0xDEADBEEF


def c_taps(src_len, dst_len):
    """fdf_resize_taps into a buffer with a sentinel word behind it."""
    buf = np.full(dst_len + 1, SENTINEL, dtype=np.uint32)
    rc = _native.load().fdf_resize_taps(src_len, dst_len, buf.ctypes.data)
    assert rc == _native.FDF_OK
    assert buf[dst_len] == SENTINEL                  # dst_len words and no more
    return buf[:dst_len]


SHAPES = [(1, 1), (1, 5), (2, 1), (5, 4), (1920, 1600), (1080, 900), (41, 20), (20, 47),
          (65535, 3)]


@pytest.mark.parametrize("s,d", SHAPES)
def test_taps_equal_the_reference(s, d):
    got = c_taps(s, d)
    assert np.array_equal(got, taps(s, d))
    assert np.array_equal(fast_hip.resize_taps(s, d), got)
    i0, q = (got >> 12).astype(np.int64), (got & 0xfff).astype(np.int64)
    assert q.max() <= 2048 and i0.min() >= 0
    # a second tap inside the axis, or the edge value that gives the first tap no weight
    edge = 2048 if s > 1 else 0
    assert np.all((i0 + 1 <= s - 1) | (q == edge))
    assert np.all(i0 <= max(s - 2, 0))


def test_worked_entries_and_crc():
    t = c_taps(1920, 1600)
    assert (int(t[0]) >> 12, int(t[0]) & 0xfff) == (0, 205)
    assert (int(t[1]) >> 12, int(t[1]) & 0xfff) == (1, 614)
    assert tap(1920, 1600, 0) == (0, 1, 205) and tap(1920, 1600, 1) == (1, 2, 614)
    assert zlib.crc32(taps(1920, 1600).tobytes()) == 2800302969      # the reference itself
    assert zlib.crc32(t.tobytes()) == 2800302969


@pytest.mark.parametrize("s", [1, 2, 7, 300, 1920])
def test_same_length_is_the_identity_table(s):
    """D = S: q = 0 and i0 = i -- but for the last index, where the rule for i0 >= S - 1 names
    the same pixel as the second tap with all the weight (i0 = S - 2, q = 2048)."""
    t = c_taps(s, s)
    i0, q = (t >> 12).astype(np.int64), (t & 0xfff).astype(np.int64)
    assert np.array_equal(i0[:-1], np.arange(s - 1)) and not q[:-1].any()
    assert (i0[-1], q[-1]) == ((s - 2, 2048) if s > 1 else (0, 0))
    assert set(np.unique(q).tolist()) <= {0, 2048}
    assert np.array_equal(np.where(q == 0, i0, np.minimum(i0 + 1, s - 1)), np.arange(s))


def test_reference_consequences():
    """The reference itself: D = S is the identity, S = 2 D the rounded 2 x 2 mean, a constant
    frame stays constant."""
    img = np.random.default_rng(1).integers(0, 256, (16, 16), dtype=np.uint8)
    assert np.array_equal(resize(img, 16, 16), img)
    mean = (img.reshape(8, 2, 8, 2).astype(np.int64).sum((1, 3)) + 2) // 4
    assert np.array_equal(resize(img, 8, 8), mean)
    assert (resize(np.full((9, 13), 255, np.uint8), 31, 4) == 255).all()


def test_taps_errors():
    lib = _native.load()
    buf = np.zeros(4, dtype=np.uint32)
    assert lib.fdf_resize_taps(4, 4, None) == _native.FDF_ERR_ARG
    assert lib.fdf_resize_taps(0, 4, buf.ctypes.data) == _native.FDF_ERR_SIZE
    assert lib.fdf_resize_taps(4, 0, buf.ctypes.data) == _native.FDF_ERR_SIZE
    assert lib.fdf_resize_taps(65536, 4, buf.ctypes.data) == _native.FDF_ERR_SIZE
    assert not buf.any()
    for bad in ((0, 4), (4, 0), (65536, 4), (-1, 4)):
        with pytest.raises(ValueError):
            fast_hip.resize_taps(*bad)


def test_plan_1080p():
    plan = fast_hip.pyramid_plan((1080, 1920), 8, (6, 5), n_frames=3)
    sizes = level_sizes(1920, 1080, 8)
    assert sizes[:4] == [(1920, 1080), (1600, 900), (1333, 750), (1111, 625)]
    assert [(L.width, L.height) for L in plan.levels] == sizes
    assert len(plan) == 8 and plan.n_frames == 3
    base = plan.levels[0]
    assert base[2:] == (0, 0, 0, 0)                  # the caller's frames: nothing of the buffer
    end, taps_end = 0, 0
    for L in plan.levels[1:]:
        assert L.frame_stride_bytes == L.width * L.height
        assert L.offset_bytes % 256 == 0 and L.offset_bytes >= end
        end = L.offset_bytes + 3 * L.frame_stride_bytes
        assert L.xtaps_offset == taps_end and L.ytaps_offset == taps_end + L.width
        taps_end = L.ytaps_offset + L.height
    assert end <= plan.total_bytes < end + 256
    assert plan.total_taps == taps_end == sum(w + h for w, h in sizes[1:])
    # n_frames scales the buffer, not the taps
    one = fast_hip.pyramid_plan((1080, 1920), 8, (6, 5))
    assert one.total_taps == plan.total_taps and one.total_bytes < plan.total_bytes
    assert sum(w * h for w, h in sizes[1:]) <= one.total_bytes


def test_plan_taps():
    plan = fast_hip.pyramid_plan((61, 97), 4)
    sizes = level_sizes(97, 61, 4)
    assert sizes == [(97, 61), (81, 51), (68, 43), (57, 36)]
    t = plan.taps()
    assert t.dtype == np.uint32 and t.shape == (plan.total_taps,)
    for l in range(1, 4):
        L = plan.levels[l]
        assert np.array_equal(t[L.xtaps_offset:L.xtaps_offset + L.width],
                              taps(sizes[l - 1][0], L.width))
        assert np.array_equal(t[L.ytaps_offset:L.ytaps_offset + L.height],
                              taps(sizes[l - 1][1], L.height))
    single = fast_hip.pyramid_plan((61, 97), 1)
    assert single.total_bytes == 0 and single.total_taps == 0 and single.taps().size == 0
    lib = _native.load()
    assert lib.fdf_pyramid_taps(plan._c, 4, 96, 61, t.ctypes.data) == _native.FDF_ERR_ARG


def test_plan_errors():
    def status(shape, n_levels, scale, n_frames=1):
        with pytest.raises(FdfError) as e:
            fast_hip.pyramid_plan(shape, n_levels, scale, n_frames)
        return e.value.status

    assert status((1080, 1920), 8, (5, 5)) == _native.FDF_ERR_ARG        # num <= den
    assert status((1080, 1920), 8, (5, 6)) == _native.FDF_ERR_ARG
    assert status((1080, 1920), 8, (6, 0)) == _native.FDF_ERR_ARG
    assert status((1080, 1920), 0, (6, 5)) == _native.FDF_ERR_ARG
    assert status((1080, 1920), 33, (6, 5)) == _native.FDF_ERR_ARG
    assert status((1080, 1920), 8, (6, 5), 65536) == _native.FDF_ERR_ARG
    assert status((0, 1920), 2, (6, 5)) == _native.FDF_ERR_SIZE
    assert status((1080, 65536), 2, (6, 5)) == _native.FDF_ERR_SIZE
    # a level reaching zero: 7 -> 2 -> 1 -> 0 at 3 / 1
    assert status((7, 7), 4, (3, 1)) == _native.FDF_ERR_SIZE
    assert len(fast_hip.pyramid_plan((7, 7), 3, (3, 1))) == 3
    assert len(fast_hip.pyramid_plan((1080, 1920), 32, (6, 5))) == 32
    with pytest.raises(TypeError):
        fast_hip.pyramid_plan((1080, 1920), 8, 1.2)
    with pytest.raises(ValueError):
        fast_hip.pyramid_plan((1080, 1920), 8, (-6, 5))


def test_plan_7x7_at_2_over_1():
    """7 x 7 at 2 / 1 with 4 levels: the size rule rounds to nearest, (1 * 1 + 1) / 2 = 1, so
    at a factor of 2 a side never reaches zero and the levels are 7, 4, 2, 1."""
    assert level_sizes(7, 7, 4, 2, 1) == [(7, 7), (4, 4), (2, 2), (1, 1)]
    plan = fast_hip.pyramid_plan((7, 7), 4, (2, 1))
    assert [(L.width, L.height) for L in plan.levels] == level_sizes(7, 7, 4, 2, 1)


def test_level0_mapping():
    pts = np.array([[0, 0], [1599, 899], [7, 3]], dtype=np.uint32)
    got = to_level0(pts, (1920, 1080), (1600, 900))
    assert got.dtype == np.float32
    assert np.array_equal(got[0], np.float32([0.1, 0.1]))
    assert np.array_equal(got[1], np.float32([1918.9, 1078.9]))
    assert np.array_equal(to_level0(pts, (97, 61), (97, 61)), pts.astype(np.float32))


def test_wrapper_argument_checks():
    import torch

    f = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((3, 4, 4), dtype=torch.uint8))     # frame counts
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((2, 4, 4), dtype=torch.int32))     # not uint8
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((2, 4, 0), dtype=torch.uint8))     # a zero side
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((2, 4, 4), dtype=torch.uint8),
                               xtaps=torch.zeros(3, dtype=torch.int32))          # too few taps
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((2, 4, 4), dtype=torch.uint8),
                               ytaps=torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, torch.zeros((2, 4, 4), dtype=torch.uint8))     # host tensors
    with pytest.raises(ValueError):
        fast_hip.resize_device(f, f[:, :4, :4])                                  # not contiguous
    plan = fast_hip.pyramid_plan((8, 8), 2, (2, 1), n_frames=2)
    buf = torch.zeros(plan.total_bytes, dtype=torch.uint8)
    taps_t = torch.zeros(plan.total_taps, dtype=torch.int32)
    with pytest.raises(TypeError):
        fast_hip.pyramid_device(f, plan.levels, buf, taps_t)
    with pytest.raises(ValueError):
        fast_hip.pyramid_device(torch.zeros((2, 8, 9), dtype=torch.uint8), plan, buf, taps_t)
    with pytest.raises(ValueError):
        fast_hip.pyramid_device(torch.zeros((3, 8, 8), dtype=torch.uint8), plan, buf, taps_t)
    with pytest.raises(ValueError):
        fast_hip.pyramid_device(f, plan, buf[:-1], taps_t)
    with pytest.raises(ValueError):
        fast_hip.pyramid_device(f, plan, buf, taps_t[:-1])
    with pytest.raises(ValueError):
        fast_hip.pyramid_device(f, plan, buf, taps_t)                            # host tensors
    with pytest.raises(ValueError):
        fast_hip.Pyramid(f)                                                      # a host tensor
    img = np.zeros((20, 30), dtype=np.uint8)
    for bad in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 16)):
        with pytest.raises(ValueError):
            fast_hip.resize_array(img, bad)
    with pytest.raises(TypeError):
        fast_hip.resize_array(img, 5)
    with pytest.raises(TypeError):
        fast_hip.resize_array(img.astype(np.float32), (5, 5))
    cfg = Config(16, 9)
    with pytest.raises(ValueError):
        fast_hip.detect_multiscale_array(img, cfg, cell=(8, 8))                  # cell without k
    with pytest.raises(ValueError):
        fast_hip.detect_multiscale_array(img, cfg, k=4)
    with pytest.raises(ValueError):
        fast_hip.detect_multiscale_array(img, cfg, radius=0)
    with pytest.raises(ValueError):
        fast_hip.detect_multiscale_array(img, cfg, n_bins=0)
    with pytest.raises(FdfError) as e:
        fast_hip.detect_multiscale_array(img, cfg, scale=(5, 6))
    assert e.value.status == _native.FDF_ERR_ARG
    with pytest.raises(FdfError) as e:
        fast_hip.detect_multiscale_array(img, cfg, n_levels=33)
    assert e.value.status == _native.FDF_ERR_ARG
    with pytest.raises(TypeError):
        fast_hip.detect_multiscale_array(img, (16, 9))


def test_resize_frame_rejects_before_the_device():
    """Shape and pointer errors of fdf_resize_frame are answered without touching a device
    (a NULL context included)."""
    lib = _native.load()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.fdf_resize_frame(None, p, 8, 8, 8, p, 4, 4, 4) == _native.FDF_ERR_ARG
    assert lib.fdf_resize_device(None, p, 1, 8, 8, 64, p, 4, 4, 16, p, p, None) == \
        _native.FDF_ERR_ARG
    assert lib.fdf_pyramid_device(None, p, 1, 64, None, 1, p, p, None) == _native.FDF_ERR_ARG
    assert ctypes.sizeof(_native.FdfPyramidLevel) == 40
