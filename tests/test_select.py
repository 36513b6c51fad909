"""Best-K selection per grid cell, the parts that need no GPU: fdf_select_scratch_bytes (host
only) and the argument checks of the Python wrappers (which run before any device call)."""
import ctypes

import numpy as np
import pytest

from feature_detector_fast_amd import _native, fast_hip


def scratch(n_frames, width, height, cw, ch, cap):
    v = ctypes.c_uint64(0xdead)
    rc = _native.load().fdf_select_scratch_bytes(n_frames, width, height, cw, ch, cap,
                                                 ctypes.byref(v))
    return rc, v.value


def test_scratch_bytes_nonzero_without_device():
    # no context is created and no device is opened: the call is plain host arithmetic
    rc, b = scratch(1, 300, 200, 32, 32, 309)
    assert rc == _native.FDF_OK and b > 0 and b % 256 == 0
    assert fast_hip.select_scratch_bytes(1, (200, 300), (32, 32), 309) == b
    rc, b = scratch(512, 1920, 1080, 0, 0, 4_000_000)
    assert rc == _native.FDF_OK and b >= 4_000_000


def test_scratch_bytes_monotonic():
    base = scratch(4, 640, 480, 32, 32, 10_000)[1]
    for cap in (10_001, 20_000, 1 << 24, 1 << 33):
        b = scratch(4, 640, 480, 32, 32, cap)[1]
        assert b >= base
        base = b
    base = 0
    for f in (1, 2, 3, 64, 512, 65535):
        b = scratch(f, 640, 480, 32, 32, 10_000)[1]
        assert b >= base
        base = b
    base = 0
    for cell in (0, 480, 240, 100, 33, 32, 8, 3, 1):   # more and more cells
        b = scratch(4, 640, 480, cell, cell, 10_000)[1]
        assert b >= base
        base = b


def test_scratch_bytes_shapes_and_errors():
    # shapes the reference answers with an empty list, and no frames: nothing is needed
    assert scratch(1, 40, 5, 8, 8, 100) == (_native.FDF_OK, 0)
    assert scratch(1, 6, 40, 8, 8, 100) == (_native.FDF_OK, 0)
    assert scratch(0, 300, 200, 8, 8, 100) == (_native.FDF_OK, 0)
    assert scratch(1, 300, 2, 8, 8, 100)[0] == _native.FDF_ERR_SIZE
    assert scratch(65536, 300, 200, 8, 8, 100)[0] == _native.FDF_ERR_ARG
    assert _native.load().fdf_select_scratch_bytes(1, 300, 200, 8, 8, 100, None) == \
        _native.FDF_ERR_ARG


def test_select_best_rejects_bad_arguments():
    pts = np.zeros((4, 2), np.uint32)
    sc = np.zeros(4, np.uint16)
    with pytest.raises(ValueError):
        fast_hip.select_best(pts, sc, (200, 300), (32, 32), 0)
    with pytest.raises(TypeError):
        fast_hip.select_best(pts.astype(np.int64), sc, (200, 300), (32, 32), 1)
    with pytest.raises(TypeError):
        fast_hip.select_best(pts, sc.astype(np.float32), (200, 300), (32, 32), 1)
    with pytest.raises(TypeError):
        fast_hip.select_best(pts.reshape(2, 4), sc, (200, 300), (32, 32), 1)
    with pytest.raises(TypeError):
        fast_hip.select_best(pts, sc[:3], (200, 300), (32, 32), 1)
    with pytest.raises(TypeError):
        fast_hip.select_best(pts, sc, (200, 300), (32, 32), 1, offsets=np.array([0, 4]))
    with pytest.raises(ValueError):
        fast_hip.detect_best_array(np.zeros((20, 20), np.uint8), None, (8, 8), 0)


def test_select_device_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    pts = torch.zeros((8, 2), dtype=torch.int32)
    sc = torch.zeros(8, dtype=torch.int16)
    offs = torch.zeros(2, dtype=torch.int64)
    sel = torch.zeros((8, 2), dtype=torch.int32)
    ssc = torch.zeros(8, dtype=torch.int16)
    soffs = torch.zeros(2, dtype=torch.int64)

    def call(**kw):
        a = dict(points=pts, scores=sc, offsets=offs, shape=(200, 300), cell=(32, 32), k=1,
                 sel=sel, sel_scores=ssc, sel_offsets=soffs)
        a.update(kw)
        fast_hip.select_device(**a)

    for bad in (dict(k=0), dict(points=pts.float()), dict(points=pts.reshape(4, 4)),
                dict(scores=sc.half()), dict(scores=sc.int()), dict(scores=sc[:4]),
                dict(offsets=offs.int()), dict(sel=sel.reshape(-1)), dict(sel_scores=ssc[:2]),
                dict(sel_offsets=soffs[:1]), dict(keep=torch.zeros(8, dtype=torch.int32)),
                dict(keep=torch.zeros(4, dtype=torch.uint8)),
                dict()):                          # the last: well-formed but not on a GPU
        with pytest.raises(ValueError):
            call(**bad)
