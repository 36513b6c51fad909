"""Harris corner response, the parts that need no GPU: fdf_harris_codes (host only) against
the rank-score rule in Python integers, the numpy reference (tests/_harris_reference.py)
against the worked values of the semantics in include/fdf.h, the exports, and the argument
checks of the Python wrappers (which run before any device call)."""
import os
import random
import zlib

import numpy as np
import pytest

import workloads
from _harris_reference import (checker3, code, codes, corner_frame, edge_frame, reference,
                               responses, sums)
from feature_detector_fast_amd import _native, fast_hip

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1


def c_codes(values):
    arr = np.array(values, dtype=np.int64)
    out = np.full(len(arr) + 2, 0xABCD, dtype=np.uint16)
    rc = _native.load().fdf_harris_codes(arr.ctypes.data, len(arr), out.ctypes.data)
    assert rc == _native.FDF_OK
    assert (out[len(arr):] == 0xABCD).all()           # n entries, nothing after them
    return out[:len(arr)]


def code_cases():
    vals = [0, -1, INT64_MIN, INT64_MAX]
    vals += list(range(1, 1026)) + [2047, 2048, 2049, 4095, 4096]
    for k in range(0, 63):
        vals += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    rng = random.Random(20240607)
    for _ in range(4000):
        bits = rng.randint(1, 63)
        vals.append(rng.getrandbits(bits))
        vals.append(-rng.getrandbits(bits))
    # neighbours of a mantissa step at every exponent
    for e in range(10, 63):
        step = 1 << (e - 10)
        m = rng.randint(0, 1023)
        base = (1 << e) + m * step
        vals += [base - 1, base, base + step - 1, min(base + step, INT64_MAX)]
    return vals


def test_codes_against_the_python_rule():
    vals = code_cases()
    got = c_codes(vals)
    want = np.array([code(v) for v in vals], dtype=np.uint16)
    assert np.array_equal(got, want)
    assert np.array_equal(fast_hip.harris_codes(np.array(vals, dtype=np.int64)), want)
    assert code(0) == code(-1) == code(INT64_MIN) == 0
    assert [code(v) for v in (1, 1023, 1024, 1025, 2047, 2048)] == [1, 1023, 1024, 1025, 2047, 2048]
    assert code(INT64_MAX) == 55295 and int(got[3]) == 55295
    order = np.argsort(np.array(vals, dtype=np.int64), kind="stable")
    assert np.all(np.diff(got[order].astype(np.int64)) >= 0)      # monotone non-decreasing
    assert c_codes([1167741344610000, 599464460610000]).tolist() == [42022, 41026]


def test_codes_wrapper_and_errors():
    lib = _native.load()
    one = np.zeros(1, np.int64)
    out = np.zeros(1, np.uint16)
    assert lib.fdf_harris_codes(None, 1, out.ctypes.data) == _native.FDF_ERR_ARG
    assert lib.fdf_harris_codes(one.ctypes.data, 1, None) == _native.FDF_ERR_ARG
    assert lib.fdf_harris_codes(None, 0, None) == _native.FDF_OK
    assert fast_hip.harris_codes(np.zeros(0, np.int64)).shape == (0,)
    grid = np.array([[5, 1 << 40], [-3, 1024]], dtype=np.int64)
    got = fast_hip.harris_codes(grid)
    assert got.shape == (2, 2) and got.dtype == np.uint16
    assert got.tolist() == [[5, code(1 << 40)], [0, 1024]]
    with pytest.raises(TypeError):
        fast_hip.harris_codes(np.zeros(3, np.int32))
    with pytest.raises(TypeError):
        fast_hip.harris_codes(np.zeros(3, np.float64))


def test_reference_worked_values():
    img = corner_frame()
    pts = np.array([(16, 16), (15, 15), (0, 0)], dtype=np.uint32)
    a, b, c = sums(img, pts)
    assert a.tolist() == [7542900, 5462100, 0]
    assert b.tolist() == [7542900, 5462100, 0]
    assert c.tolist() == [1040400, 1040400, 0]
    r, sc = reference(img, pts)
    assert r.tolist() == [1167741344610000, 599464460610000, 0]
    assert sc.tolist() == [42022, 41026, 0]
    a, b, c = sums(edge_frame(), np.array([(16, 16)], dtype=np.uint32))
    assert (a.tolist(), b.tolist(), c.tolist()) == ([14565600], [0], [0])
    r, sc = reference(edge_frame(), np.array([(16, 16)], dtype=np.uint32))
    assert r.tolist() == [-212156703360000] and sc.tolist() == [0]


@pytest.mark.parametrize("which,count,crcs,nonpos3", [
    ("off", 309, {7: 610568635, 5: 1037635382, 3: 2417599212}, 17),
    ("maxt", 131, {7: 956545480, 5: 3654811535, 3: 2810275981}, 7)])
def test_reference_on_the_golden_frame(which, count, crcs, nonpos3):
    img = workloads.golden_image()
    pts = workloads.read_points(os.path.join(workloads.GOLDEN, f"kp_t16_n9_{which}.txt"))
    assert img.shape == (200, 300) and len(pts) == count
    for block, crc in crcs.items():
        r = responses(img, pts, block)
        assert zlib.crc32(r.astype("<i8").tobytes()) == crc, block
        if block == 7:
            assert (r > 0).all()
        if block == 3:
            assert int(np.count_nonzero(r <= 0)) == nonpos3
        assert np.array_equal(codes(r), fast_hip.harris_codes(r))


def test_reference_checker3_needs_wide_arithmetic():
    img = checker3()
    assert img.shape == (24, 24) and img[0, 3] == 255 and img[0, 0] == 0 and img[3, 3] == 0
    pts = np.array([(x, y) for y in range(8, 16) for x in range(8, 16)], dtype=np.uint32)
    a, b, _ = sums(img, pts)
    assert max(int(a.max()), int(b.max())) == 20808000
    for k, bits in (((1, 25), 53), ((0, 255), 57), ((255, 1), 59)):
        r = responses(img, pts, 7, k)
        assert max(abs(int(v)) for v in r).bit_length() == bits, k


def test_symbols_exported():
    for name in ("fdf_harris_codes", "fdf_harris_device", "fdf_harris_points"):
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(_native.load(), name)
    for name in ("harris_codes", "harris_device", "keypoint_harris", "detect_harris_array"):
        assert name in fast_hip.__all__


BAD_BLOCK_K = (dict(block=0), dict(block=4), dict(block=9), dict(block=-3),
               dict(k=(1, 0)), dict(k=(256, 25)), dict(k=(-1, 25)), dict(k=(1, 256)),
               dict(k=1), dict(k=(1, 2, 3)))


def test_keypoint_harris_rejects_bad_arguments():
    img = np.zeros((20, 20), np.uint8)
    pts = np.array([[5, 5]], np.uint32)
    for bad in BAD_BLOCK_K:
        with pytest.raises(ValueError):
            fast_hip.keypoint_harris(img, pts, **bad)
        with pytest.raises(ValueError):
            fast_hip.detect_harris_array(img, None, **bad)
    with pytest.raises(TypeError):
        fast_hip.keypoint_harris(img, pts.astype(np.float32))
    with pytest.raises(TypeError):
        fast_hip.keypoint_harris(img, np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError):
        fast_hip.keypoint_harris(img, np.array([[-1, 5]], np.int64))
    with pytest.raises(TypeError):
        fast_hip.keypoint_harris(img.astype(np.float32), pts)


def test_harris_device_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    frames = torch.zeros((2, 20, 24), dtype=torch.uint8)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    offs = torch.zeros(3, dtype=torch.int64)
    sc = torch.zeros(8, dtype=torch.int16)
    resp = torch.zeros(8, dtype=torch.int64)

    def call(**kw):
        a = dict(frames=frames, points=pts, offsets=offs, scores=sc)
        a.update(kw)
        fast_hip.harris_device(**a)

    for bad in BAD_BLOCK_K + (
            dict(frames=frames.float()), dict(frames=frames[0]),
            dict(frames=frames[:, :, ::2]), dict(frames=frames[:, ::2]),
            dict(points=pts.float()), dict(points=pts.long()), dict(points=pts.reshape(4, 4)),
            dict(scores=sc.int()), dict(scores=sc.half()), dict(scores=sc[:7]),
            dict(scores=sc.reshape(4, 2)), dict(scores=torch.zeros(16, dtype=torch.int16)[::2]),
            dict(offsets=offs.int()), dict(offsets=offs[:2]),
            dict(responses=resp.int()), dict(responses=resp.double()), dict(responses=resp[:7]),
            dict(responses=resp.reshape(4, 2)),
            dict(responses=resp),             # well-formed but not on a GPU
            dict()):                          # the same without responses
        with pytest.raises(ValueError):
            call(**bad)


def test_multiscale_rejects_bad_rank():
    img = np.zeros((40, 40), np.uint8)
    with pytest.raises(ValueError):
        fast_hip.detect_multiscale_array(img, None, rank="bogus")
    for bad in (dict(block=4), dict(harris_k=(1, 0))):
        with pytest.raises(ValueError):
            fast_hip.detect_multiscale_array(img, None, rank="harris", **bad)
