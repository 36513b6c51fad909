"""Steered BRIEF, the parts that need no GPU: the default pattern (fdf_brief_pattern) and the
steering table (fdf_brief_steer), both host only, against the pinned values of the contract in
include/fdf.h and a Python restatement of it (tests/_brief_reference.py), and the argument
checks of the Python wrappers, which run before any device call."""
import ctypes
import zlib

import numpy as np
import pytest

from _brief_reference import bins_of, default_pattern, steer
from feature_detector_fast_amd import _native, fast_hip

PATTERN_CRC = 1958958545
TABLE_CRC = {1: 1958958545, 4: 201103782, 12: 1623296657, 30: 1342541820}


def test_default_pattern_pinned_values():
    ref, draws = default_pattern()
    assert draws == 278
    got = fast_hip.brief_pattern()
    assert got.dtype == np.int8 and got.shape == (256, 4)
    assert np.array_equal(got, ref)
    assert got[0].tolist() == [5, 8, -11, -2]
    assert got[1].tolist() == [7, 9, -7, 9]
    assert got[2].tolist() == [-4, 2, 1, 7]
    assert got[3].tolist() == [4, -2, -1, -5]
    assert got[255].tolist() == [0, -1, 1, -4]
    assert zlib.crc32(got.tobytes()) == PATTERN_CRC
    assert int(np.abs(got.astype(int)).max()) == 13
    p = got.astype(int)
    assert np.all(p[:, 0] ** 2 + p[:, 1] ** 2 <= 169) and np.all(p[:, 2] ** 2 + p[:, 3] ** 2 <= 169)
    assert np.all((p[:, 0] != p[:, 2]) | (p[:, 1] != p[:, 3]))
    assert len({tuple(t) for t in p.tolist()}) == 256


def test_default_pattern_writes_1024_bytes_only():
    buf = (ctypes.c_int8 * 1040)(*([0x55] * 1040))
    assert _native.load().fdf_brief_pattern(buf) == _native.FDF_OK
    assert list(buf[1024:]) == [0x55] * 16
    assert zlib.crc32(bytes(bytearray(np.frombuffer(buf, np.uint8)[:1024]))) == PATTERN_CRC


@pytest.mark.parametrize("n_bins", [1, 4, 12, 30])
def test_steering_table_pinned_crc(n_bins):
    table = fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)
    assert table.dtype == np.int8 and table.shape == (n_bins, 256, 4)
    assert zlib.crc32(table.tobytes()) == TABLE_CRC[n_bins]
    assert np.array_equal(table[0], fast_hip.brief_pattern())
    assert np.array_equal(table, steer(default_pattern()[0], n_bins))


def test_steering_quarter_turns_are_exact():
    """Bin 1 of 4 is a turn by +90 degrees with y down: (x, y) -> (-y, x)."""
    pat = fast_hip.brief_pattern()
    t = fast_hip.brief_steer(pat, 4).astype(int)
    p = pat.astype(int)
    for k in (0, 2):
        assert np.array_equal(t[1][:, k], -p[:, k + 1]) and np.array_equal(t[1][:, k + 1], p[:, k])
        assert np.array_equal(t[2][:, k], -p[:, k]) and np.array_equal(t[2][:, k + 1], -p[:, k + 1])
        assert np.array_equal(t[3][:, k], p[:, k + 1]) and np.array_equal(t[3][:, k + 1], -p[:, k])


@pytest.mark.parametrize("n_bins", [7, 360])
def test_steering_rule_on_a_random_pattern(n_bins):
    """Every int8 value, the extremes included: rotation in double, one rounding to float32,
    half away from zero, saturation."""
    rng = np.random.default_rng(20 + n_bins)
    pat = rng.integers(-128, 128, size=(256, 4), dtype=np.int64).astype(np.int8)
    pat[0] = (127, 127, -128, -128)
    pat[1] = (-128, 127, 127, -128)
    pat[2] = (127, 0, 0, -128)
    got = fast_hip.brief_steer(pat, n_bins)
    want = steer(pat, n_bins)
    assert np.array_equal(got, want)
    assert got.min() == -128 and got.max() == 127          # saturation happens
    assert np.array_equal(fast_hip.brief_steer(pat.reshape(-1), n_bins), want)


def test_host_function_errors():
    lib = _native.load()
    pat = fast_hip.brief_pattern()
    table = np.full(2 * 1024, 0x33, np.int8)
    assert lib.fdf_brief_pattern(None) == _native.FDF_ERR_ARG
    for bad in (0, 361, 0xFFFFFFFF):
        assert lib.fdf_brief_steer(pat.ctypes.data, bad, table.ctypes.data) == _native.FDF_ERR_ARG
    assert lib.fdf_brief_steer(None, 1, table.ctypes.data) == _native.FDF_ERR_ARG
    assert lib.fdf_brief_steer(pat.ctypes.data, 1, None) == _native.FDF_ERR_ARG
    assert (table == 0x33).all()
    assert lib.fdf_brief_steer(pat.ctypes.data, 1, table.ctypes.data) == _native.FDF_OK
    assert (table[1024:] == 0x33).all() and np.array_equal(table[:1024].reshape(256, 4), pat)
    for bad in (0, 361, -1):
        with pytest.raises(ValueError):
            fast_hip.brief_steer(pat, bad)
    for bad in (pat.astype(np.int16), pat[:255], pat.reshape(4, 256)):
        with pytest.raises(TypeError):
            fast_hip.brief_steer(bad, 4)


def test_reference_bins():
    """The reference's own bin rule at the values the contract names."""
    a = np.array([0.0, -0.0, np.pi, -np.pi, np.nan, np.inf, -np.inf, 100.0, 7.0, -7.0],
                 dtype=np.float32)
    assert bins_of(a, 4).tolist() == [0, 0, 2, 2, 0, 0, 0, 0, 0, 0]
    assert bins_of(a, 1).tolist() == [0] * 10
    # 7 rad at 30 bins: 33.42 -> 33 -> 3; -7: -33 -> 27
    assert bins_of(a, 30).tolist()[-2:] == [3, 27]


def test_symbols_exported():
    for name in ("fdf_brief_pattern", "fdf_brief_steer", "fdf_smooth_device",
                 "fdf_describe_device", "fdf_describe_points"):
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(_native.load(), name)
    for name in ("brief_pattern", "brief_steer", "smooth_device", "describe_device",
                 "keypoint_descriptors", "detect_described_array"):
        assert name in fast_hip.__all__ and callable(getattr(fast_hip, name))


def test_keypoint_descriptors_rejects_bad_arguments():
    img = np.zeros((20, 20), np.uint8)
    pts = np.array([[5, 5]], np.uint32)
    for bad in (0, 361):
        with pytest.raises(ValueError):
            fast_hip.keypoint_descriptors(img, pts, n_bins=bad)
        with pytest.raises(ValueError):
            fast_hip.detect_described_array(img, None, n_bins=bad)
    for bad in (0, 32):
        with pytest.raises(ValueError):
            fast_hip.detect_described_array(img, None, radius=bad)
    with pytest.raises(TypeError):
        fast_hip.keypoint_descriptors(img, pts.astype(np.float32))
    with pytest.raises(TypeError):
        fast_hip.keypoint_descriptors(img, np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError):
        fast_hip.keypoint_descriptors(img, np.array([[-1, 5]], np.int64))
    with pytest.raises(TypeError):
        fast_hip.keypoint_descriptors(img.astype(np.float32), pts)
    with pytest.raises(ValueError):
        fast_hip.keypoint_descriptors(img[0], pts)
    for bad in (np.zeros(1, np.float64), np.zeros(2, np.float32), np.zeros((1, 1), np.float32)):
        with pytest.raises(TypeError):
            fast_hip.keypoint_descriptors(img, pts, angles=bad)
    for bad in (np.zeros((256, 4), np.uint8), np.zeros((255, 4), np.int8)):
        with pytest.raises(TypeError):
            fast_hip.keypoint_descriptors(img, pts, pattern=bad)


def test_smooth_device_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    frames = torch.zeros((2, 20, 24), dtype=torch.uint8)
    out = torch.zeros((2, 20, 24), dtype=torch.uint8)
    for bad in (dict(frames=frames.float()), dict(frames=frames[0]), dict(out=out[0]),
                dict(frames=frames[:, :, ::2], out=out[:, :, :12]),
                dict(frames=frames[:, ::2], out=out[:, :10]),
                dict(out=out.short()), dict(out=out[:1]), dict(out=out[:, :19]),
                dict(out=out[:, :, :23]),
                dict(frames=torch.zeros((1, 0, 24), dtype=torch.uint8),
                     out=torch.zeros((1, 0, 24), dtype=torch.uint8)),
                dict()):                          # well-formed but not on a GPU
        a = dict(frames=frames, out=out)
        a.update(bad)
        with pytest.raises(ValueError):
            fast_hip.smooth_device(**a)


def test_describe_device_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    frames = torch.zeros((2, 20, 24), dtype=torch.uint8)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    offs = torch.zeros(3, dtype=torch.int64)
    desc = torch.zeros((8, 32), dtype=torch.uint8)
    table = torch.zeros((4, 256, 4), dtype=torch.int8)
    ang = torch.zeros(8, dtype=torch.float32)

    def call(**kw):
        a = dict(frames=frames, points=pts, offsets=offs, desc=desc, table=table, n_bins=4)
        a.update(kw)
        fast_hip.describe_device(**a)

    for bad in (dict(n_bins=0), dict(n_bins=361), dict(n_bins=5), dict(n_bins=3),
                dict(frames=frames.float()), dict(frames=frames[0]),
                dict(frames=frames[:, :, ::2]), dict(frames=frames[:, ::2]),
                dict(points=pts.float()), dict(points=pts.long()), dict(points=pts.reshape(4, 4)),
                dict(desc=desc.char()), dict(desc=desc[:7]), dict(desc=desc.reshape(-1)),
                dict(desc=desc[:, :31]), dict(desc=torch.zeros((8, 64), dtype=torch.uint8)[:, ::2]),
                dict(table=table.byte()), dict(table=table[:, ::2]),
                dict(offsets=offs.int()), dict(offsets=offs[:2]),
                dict(angles=ang.double()), dict(angles=ang[:7]), dict(angles=ang.reshape(4, 2)),
                dict(angles=ang),                 # well-formed but not on a GPU
                dict()):                          # the same without angles
        with pytest.raises(ValueError):
            call(**bad)
