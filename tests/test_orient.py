"""Keypoint orientation by intensity centroid, the parts that need no GPU: fdf_orient_disc
(host only) and the argument checks of the Python wrappers (which run before any device
call)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from feature_detector_fast_amd import _native, fast_hip

ORB_DISC = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def disc(radius):
    u = (ctypes.c_uint8 * 34)(*([0xAA] * 34))
    rc = _native.load().fdf_orient_disc(radius, u)
    return rc, list(u)


def test_disc_of_orb_patch():
    rc, u = disc(15)
    assert rc == _native.FDF_OK
    assert u[:16] == ORB_DISC
    assert u[16:] == [0xAA] * 18                  # radius + 1 entries, nothing after them
    assert sum(2 * u[abs(v)] + 1 for v in range(-15, 16)) == 749
    assert list(fast_hip.orient_disc(15)) == ORB_DISC


@pytest.mark.parametrize("radius", range(1, 32))
def test_disc_every_radius(radius):
    rc, u = disc(radius)
    assert rc == _native.FDF_OK
    u, rest = u[:radius + 1], u[radius + 1:]
    assert u[0] == radius
    assert all(a >= b for a, b in zip(u, u[1:]))
    assert rest == [0xAA] * len(rest)
    # the disc is symmetric about its diagonal: (d, v) is in it iff (v, d) is
    inside = {(d, v) for v in range(radius + 1) for d in range(u[v] + 1)}
    assert inside == {(v, d) for d, v in inside}
    assert list(fast_hip.orient_disc(radius)) == u


def test_disc_errors():
    assert disc(0)[0] == _native.FDF_ERR_ARG
    assert disc(32)[0] == _native.FDF_ERR_ARG
    assert _native.load().fdf_orient_disc(15, None) == _native.FDF_ERR_ARG
    for bad in (0, 32, -1):
        with pytest.raises(ValueError):
            fast_hip.orient_disc(bad)


def test_symbols_exported():
    for name in ("fdf_orient_disc", "fdf_orient_device", "fdf_orient_points"):
        assert name in _native.EXPORTED_SYMBOLS
    for name in ("orient_disc", "orient_device", "keypoint_angles", "detect_oriented_array"):
        assert name in fast_hip.__all__


def test_keypoint_angles_rejects_bad_arguments():
    img = np.zeros((20, 20), np.uint8)
    pts = np.array([[5, 5]], np.uint32)
    for bad in (0, 32):
        with pytest.raises(ValueError):
            fast_hip.keypoint_angles(img, pts, radius=bad)
        with pytest.raises(ValueError):
            fast_hip.detect_oriented_array(img, None, radius=bad)
    with pytest.raises(TypeError):
        fast_hip.keypoint_angles(img, pts.astype(np.float32))
    with pytest.raises(TypeError):
        fast_hip.keypoint_angles(img, np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError):
        fast_hip.keypoint_angles(img, np.array([[-1, 5]], np.int64))
    with pytest.raises(TypeError):
        fast_hip.keypoint_angles(img.astype(np.float32), pts)


def test_orient_device_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    frames = torch.zeros((2, 20, 24), dtype=torch.uint8)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    offs = torch.zeros(3, dtype=torch.int64)
    ang = torch.zeros(8, dtype=torch.float32)
    mom = torch.zeros((8, 2), dtype=torch.int32)

    def call(**kw):
        a = dict(frames=frames, points=pts, offsets=offs, angles=ang)
        a.update(kw)
        fast_hip.orient_device(**a)

    for bad in (dict(radius=0), dict(radius=32),
                dict(frames=frames.float()), dict(frames=frames[0]),
                dict(frames=frames[:, :, ::2]), dict(frames=frames[:, ::2]),
                dict(points=pts.float()), dict(points=pts.long()), dict(points=pts.reshape(4, 4)),
                dict(angles=ang.double()), dict(angles=ang[:7]), dict(angles=ang.reshape(4, 2)),
                dict(offsets=offs.int()), dict(offsets=offs[:2]),
                dict(moments=mom.float()), dict(moments=mom[:7]), dict(moments=mom.reshape(-1)),
                dict(moments=mom),                # well-formed but not on a GPU
                dict()):                          # the same without moments
        with pytest.raises(ValueError):
            call(**bad)


def test_wg_share_binary():
    """The kernels' split of a frame's points over workgroups (fdfk::wg_share), checked on
    the host by tests/cpp/test_wg_share: contiguous, disjoint, covering, on pass boundaries,
    and equal to the arithmetic written out."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_wg_share")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "630 cases, 0 failures" in res.stdout
