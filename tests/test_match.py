"""CPU tests of descriptor matching: the numpy reference of tests/_match_reference.py against a
literal bit-by-bit brute force, the Python wrappers' argument checks (raised before any device
call), unpack_matches and the layout of fdf_match."""
import ctypes

import numpy as np
import pytest

import _match_reference as ref
from feature_detector_fast_amd import _native, fast_hip


def brute_force(q, t, q_pts=None, t_pts=None, window=None):
    """The contract spelled out: unpacked bits, every pair, (distance, index) order."""
    out = []
    for i in range(len(q)):
        cands = []
        for j in range(len(t)):
            if q_pts is not None and (abs(int(q_pts[i][0]) - int(t_pts[j][0])) > window[0] or
                                      abs(int(q_pts[i][1]) - int(t_pts[j][1])) > window[1]):
                continue
            d = int((np.unpackbits(q[i]) != np.unpackbits(t[j])).sum())
            cands.append((d, j))
        cands.sort()
        if not cands:
            out.append((ref.NONE, ref.NO_DISTANCE, ref.NO_DISTANCE))
        else:
            out.append((cands[0][1], cands[0][0],
                        cands[1][0] if len(cands) > 1 else ref.NO_DISTANCE))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def fields(rec):
    return np.stack([rec["index"], rec["distance"], rec["second"]], axis=1).astype(np.int64)


def tied_descriptors(rng, n):
    """Few base descriptors with 0..2 flipped bits: equal descriptors and distances abound."""
    pool = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    d = pool[rng.integers(0, 3, n)].copy()
    for row in d:
        for bit in rng.integers(0, 256, rng.integers(0, 3)):
            row[bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


@pytest.mark.parametrize("n_q,n_t", [(0, 3), (3, 0), (1, 1), (2, 1), (5, 2), (9, 17)])
def test_reference_against_brute_force(n_q, n_t):
    rng = np.random.default_rng(n_q * 31 + n_t)
    for draw in (lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8),
                 lambda n: tied_descriptors(rng, n)):
        q, t = draw(n_q), draw(n_t)
        assert np.array_equal(fields(ref.match_pair(q, t)), brute_force(q, t))
        qp = rng.integers(0, 12, (n_q, 2)).astype(np.uint32)
        tp = rng.integers(0, 12, (n_t, 2)).astype(np.uint32)
        for window in ((0, 0), (2, 1), (3, 11), (11, 11)):
            got = ref.match_pair(q, t, qp, tp, window)
            assert np.array_equal(fields(got), brute_force(q, t, qp, tp, window)), window


def test_reference_distance_extremes():
    t = np.random.default_rng(5).integers(0, 256, (1, 32), dtype=np.uint8)
    got = ref.match_pair(~t, t)
    assert fields(got).tolist() == [[0, 256, ref.NO_DISTANCE]]
    got = ref.match_pair(t, np.concatenate([~t, t, t]), base=7)
    assert fields(got).tolist() == [[8, 0, 0]]


def test_reference_frames_caps_and_filter():
    rng = np.random.default_rng(6)
    desc = tied_descriptors(rng, 40)
    offs = np.array([2, 10, 10, 25, 40], dtype=np.uint64)
    fill = np.zeros(44, dtype=ref.MATCH_DTYPE)
    fill["index"], fill["distance"] = 77, 5
    got = ref.match(desc, offs[:-1], 20, desc, offs[1:], 30, out=fill)
    assert np.array_equal(got[:2], fill[:2]) and np.array_equal(got[20:], fill[20:])
    assert (got["index"][2:10] == ref.NONE).all()                  # train frame 1 is empty
    assert np.array_equal(fields(got[10:20]), fields(ref.match_pair(desc[10:20], desc[25:30],
                                                                    base=25)))
    # the filter, each rule on its own
    m = np.zeros(6, dtype=ref.MATCH_DTYPE)
    m["index"] = [0, 1, ref.NONE, 2, 9, 1]
    m["distance"] = [10, 30, ref.NO_DISTANCE, 30, 0, 0]
    m["second"] = [20, 40, ref.NO_DISTANCE, ref.NO_DISTANCE, 0, 5]
    rev = np.zeros(3, dtype=ref.MATCH_DTYPE)
    rev["index"] = [0, 5, 1]
    o = np.array([0, 6], dtype=np.uint64)
    assert ref.match_filter(m, o, 6).tolist() == [1, 1, 0, 1, 1, 1]
    assert ref.match_filter(m, o, 6, max_distance=10).tolist() == [1, 0, 0, 0, 1, 1]
    assert ref.match_filter(m, o, 6, max_distance=300).tolist() == [1, 1, 0, 1, 1, 1]
    assert ref.match_filter(m, o, 6, ratio=(3, 4)).tolist() == [1, 0, 0, 1, 0, 1]
    assert ref.match_filter(m, o, 6, ratio=(1, 1)).tolist() == [1, 1, 0, 1, 0, 1]
    assert ref.match_filter(m, o, 6, ratio=(3, 0)).tolist() == [1, 1, 0, 1, 1, 1]
    assert ref.match_filter(m, o, 6, reverse=rev, t_cap=3).tolist() == [1, 0, 0, 0, 0, 1]
    keep = ref.match_filter(m, np.array([1, 4], dtype=np.uint64), 3, out=np.full(8, 9, np.uint8))
    assert keep.tolist() == [9, 1, 0, 9, 9, 9, 9, 9]


def test_match_layout():
    assert ctypes.sizeof(_native.FdfMatch) == 8
    assert _native.FdfMatch.index.offset == 0 and _native.FdfMatch.distance.offset == 4
    assert _native.FdfMatch.second.offset == 6
    assert fast_hip.MATCH_DTYPE.itemsize == 8 and fast_hip.MATCH_DTYPE == ref.MATCH_DTYPE
    assert fast_hip.MATCH_NONE == ref.NONE == 0xFFFFFFFF
    assert fast_hip.MATCH_NO_DISTANCE == ref.NO_DISTANCE == 0xFFFF


def test_unpack_matches_round_trip():
    rec = np.zeros(4, dtype=fast_hip.MATCH_DTYPE)
    rec["index"] = [0, 7, 0xFFFFFFFF, 0xFFFFFFFE]
    rec["distance"] = [0, 256, 0xFFFF, 3]
    rec["second"] = [0, 0xFFFF, 0xFFFF, 200]
    want = ([0, 7, -1, 0xFFFFFFFE], [0, 256, 0xFFFF, 3], [0, 0xFFFF, 0xFFFF, 200])
    packed = np.stack([rec["index"], rec["distance"].astype(np.uint32) |
                       (rec["second"].astype(np.uint32) << 16)], axis=1)
    for array in (rec, packed, packed.view(np.int32)):
        index, distance, second = fast_hip.unpack_matches(array)
        assert index.dtype == np.int64
        assert (index.tolist(), distance.tolist(), second.tolist()) == want
    assert np.array_equal(ref.as_records(packed), rec)
    assert all(len(v) == 0 for v in fast_hip.unpack_matches(np.zeros((0, 2), np.int32)))
    for bad in (np.zeros((3, 3), np.int32), np.zeros((3, 2), np.int64), np.zeros(3, np.uint32),
                np.zeros((3, 2), np.float32)):
        with pytest.raises(TypeError):
            fast_hip.unpack_matches(bad)


def test_match_device_argument_checks():
    torch = pytest.importorskip("torch")
    desc = torch.zeros((8, 32), dtype=torch.uint8)
    offs = torch.zeros(3, dtype=torch.int64)
    matches = torch.zeros((8, 2), dtype=torch.int32)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    good = dict(q_desc=desc, q_offsets=offs, t_desc=desc, t_offsets=offs, matches=matches)
    for bad in (dict(q_desc=desc.to(torch.int8)), dict(t_desc=desc[:, :31]),
                dict(q_desc=torch.zeros((8, 64), dtype=torch.uint8)[:, ::2]),
                dict(t_desc=desc.reshape(-1)), dict(matches=matches[:7]),
                dict(matches=torch.zeros((8, 2), dtype=torch.int64)),
                dict(matches=torch.zeros((8, 2), dtype=torch.float32)),
                dict(matches=torch.zeros((8, 3), dtype=torch.int32)),
                dict(q_offsets=offs.to(torch.int32)), dict(t_offsets=offs[:2]),
                dict(q_offsets=torch.zeros(4, dtype=torch.int64)),
                dict(q_offsets=torch.zeros(6, dtype=torch.int64)[::2]),
                dict(q_points=pts), dict(t_points=pts),
                dict(q_points=pts, t_points=pts),                       # no window
                dict(window=(1, 1)),                                    # no points
                dict(q_points=pts, t_points=pts[:7], window=(1, 1)),
                dict(q_points=pts.to(torch.int64), t_points=pts, window=(1, 1)),
                dict(q_points=pts, t_points=pts, window=(-1, 1)),
                dict(q_points=pts, t_points=pts, window=(1, 1 << 32))):
        with pytest.raises(ValueError):
            fast_hip.match_device(**{**good, **bad})
    with pytest.raises(TypeError):
        fast_hip.match_device(**good, q_points=pts, t_points=pts, window=3)
    # a slice of the offsets is a contiguous int64 tensor: accepted up to the device check
    with pytest.raises(ValueError, match="CUDA"):
        fast_hip.match_device(desc, offs[:-1], desc, offs[1:], matches)


def test_match_filter_device_argument_checks():
    torch = pytest.importorskip("torch")
    offs = torch.zeros(3, dtype=torch.int64)
    matches = torch.zeros((8, 2), dtype=torch.int32)
    keep = torch.zeros(8, dtype=torch.uint8)
    good = dict(matches=matches, q_offsets=offs, keep=keep)
    for bad in (dict(matches=matches.to(torch.int64)), dict(matches=matches.reshape(-1)),
                dict(keep=keep[:7]), dict(keep=keep.to(torch.int32)),
                dict(keep=torch.zeros((8, 1), dtype=torch.uint8)),
                dict(reverse=torch.zeros((5, 3), dtype=torch.int32)),
                dict(q_offsets=offs.to(torch.float64)), dict(q_offsets=offs[:0]),
                dict(ratio=(65536, 4)), dict(ratio=(3, 65536)), dict(ratio=(-1, 4)),
                dict(max_distance=-1)):
        with pytest.raises(ValueError):
            fast_hip.match_filter_device(**{**good, **bad})
    for bad in (dict(ratio=0.75), dict(ratio=(3,)), dict(ratio=(3, 4, 5))):
        with pytest.raises(TypeError):
            fast_hip.match_filter_device(**{**good, **bad})
    with pytest.raises(ValueError, match="CUDA"):
        fast_hip.match_filter_device(**good, ratio=(65535, 65535), max_distance=0)


def test_match_descriptors_argument_checks():
    q = np.zeros((4, 32), np.uint8)
    t = np.zeros((5, 32), np.uint8)
    qp, tp = np.zeros((4, 2), np.uint32), np.zeros((5, 2), np.uint32)
    for bad in (dict(q_desc=q.astype(np.int8)), dict(t_desc=t[:, :31]), dict(q_desc=q.reshape(-1)),
                dict(q_points=qp.astype(np.float32), t_points=tp, window=(1, 1)),
                dict(ratio=0.75), dict(window=5, q_points=qp, t_points=tp)):
        with pytest.raises(TypeError):
            fast_hip.match_descriptors(**{**dict(q_desc=q, t_desc=t), **bad})
    for bad in (dict(q_points=qp), dict(t_points=tp), dict(q_points=qp, t_points=tp),
                dict(window=(1, 1)), dict(q_points=qp[:3], t_points=tp, window=(1, 1)),
                dict(q_points=qp, t_points=tp[:4], window=(1, 1)), dict(ratio=(70000, 4)),
                dict(ratio=(3, 70000)), dict(max_distance=-3)):
        with pytest.raises(ValueError):
            fast_hip.match_descriptors(**{**dict(q_desc=q, t_desc=t), **bad})
