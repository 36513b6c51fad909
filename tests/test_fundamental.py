"""CPU tests of the fundamental-matrix stage: the restatement of tests/_fundamental_reference.py and
the host sampler fdf_fundamental_sample pinned to include/fdf.h's worked values and compared over
a grid, fdf_ransac_sample unchanged, the scratch size, the argument checks that are made before
any device call, the worked example through the restatement, and the ground-truth conditions of
the scenes that tests/test_gpu_fundamental.py runs on the device."""
import ctypes
import itertools

import numpy as np
import pytest

import _fundamental_reference as ref
import _ransac_reference as rref
from feature_detector_fast_amd import _native, fast_hip

A = _native.FDF_ERR_ARG


def c_sample(seed, frame, hyp, m):
    idx = (ctypes.c_uint32 * 8)(*([7] * 8))
    draws = ctypes.c_uint32(99)
    rc = _native.load().fdf_fundamental_sample(seed, frame, hyp, m, idx, ctypes.byref(draws))
    assert rc == _native.FDF_OK
    return list(idx), draws.value


def test_worked_sampling_values():
    for args, want in (((1, 0, 0, 100), ([54, 11, 77, 18, 0, 8, 14, 35], 8)),
                       ((1, 2, 7, 9), ([1, 0, 8, 4, 2, 7, 6, 3], 16)),
                       ((0, 0, 0, 8), ([5, 2, 4, 6, 7, 1, 0, 3], 18)),
                       ((0, 0, 0, 7), (None, 32))):
        assert ref.sample(*args) == want
        assert fast_hip.fundamental_sample(*args) == want
        got = c_sample(*args)
        assert got == (want if want[0] is not None else ([ref.NONE] * 8, 32))


def test_sampler_against_reference_grid():
    invalid = valid = 0
    for seed, f, h, m in itertools.product((0, 1, 0xFFFFFFFF, 123456789), (0, 1, 65534),
                                           (0, 1, 63, 64, 65535),
                                           (0, 7, 8, 9, 10, 64, 100, 2 ** 32 - 2)):
        want, draws = ref.sample(seed, f, h, m)
        got, got_draws = c_sample(seed, f, h, m)
        assert got_draws == draws, (seed, f, h, m)
        if want is None:
            invalid += 1
            assert got == [ref.NONE] * 8 and draws == 32
        else:
            valid += 1
            assert got == want and len(set(want)) == 8 and max(want) < m
        assert m >= 8 or want is None
    assert invalid > 0 and valid > 0


def test_thirty_two_draws_make_small_sets_usable():
    """The reason for 32 draws: with 16, most hypotheses of M = 8 have no sample."""
    for m, least in ((8, 0.75), (9, 0.95)):
        ok = sum(ref.sample(3, 0, h, m)[0] is not None for h in range(400))
        assert ok >= least * 400, (m, ok)


def test_ransac_sampler_is_unchanged():
    """The draw limit of the samples of 3 and 4 is still 16, with the documented values."""
    for args, want in (((1, 0, 0, 100, 4), ([54, 11, 77, 18], 4)), ((1, 2, 7, 5, 4), ([1, 0, 4, 2], 5)),
                       ((0, 0, 0, 4, 4), ([2, 1, 3, 0], 7))):
        assert fast_hip.ransac_sample(*args) == want
    for h in range(20):
        assert fast_hip.ransac_sample(5, 1, h, 3, 4) == (None, 16)
        assert fast_hip.ransac_sample(5, 1, h, 2, 3) == (None, 16)
    for seed, h, m, s in itertools.product((0, 9), range(40), (3, 4, 5, 6), (3, 4)):
        assert fast_hip.ransac_sample(seed, 0, h, m, s) == rref.sample(seed, 0, h, m, s)


def test_sample_argument_errors():
    lib = _native.load()
    idx = (ctypes.c_uint32 * 8)()
    assert lib.fdf_fundamental_sample(0, 0, 0, 10, None, None) == A
    assert lib.fdf_fundamental_sample(0, 0, 0, 10, idx, None) == _native.FDF_OK   # draws may be NULL
    with pytest.raises(ValueError):
        fast_hip.fundamental_sample(-1, 0, 0, 10)
    with pytest.raises(ValueError):
        fast_hip.fundamental_sample(0, 0, 0, 1 << 32)


def test_scratch_bytes():
    lib = _native.load()
    assert lib.fdf_fundamental_scratch_bytes(1, 10, 10, None) == A
    for bad in ((65536, 10, 10), (1, 2 ** 32 - 1, 10), (1, 10, 0), (1, 10, 65537)):
        v = ctypes.c_uint64(0)
        assert lib.fdf_fundamental_scratch_bytes(*bad, ctypes.byref(v)) == A, bad
        with pytest.raises(ValueError):
            fast_hip.fundamental_scratch_bytes(*bad)
    for f, q, n in itertools.product((0, 1, 4, 65535), (0, 1, 300, 2 ** 32 - 2), (1, 64, 65536)):
        got = fast_hip.fundamental_scratch_bytes(f, q, n)
        assert got % 256 == 0 and got >= 32 * q + 4 * f + 4 * f * n
        assert got == fast_hip.ransac_scratch_bytes(f, q, n)


def test_entries_reject_bad_values_before_any_device_call():
    """A NULL context and bad values are refused synchronously: no device is needed."""
    lib = _native.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert lib.fdf_fundamental_device(None, 1, p, None, 4, p, p, p, 4, p, 0, 8, 1.0, 0, p, None, p,
                                      1 << 20, None) == A
    assert lib.fdf_fundamental_check_device(None, 1, p, None, 4, p, p, p, 4, p, 0, p, 1.0, p, None,
                                            None) == A
    assert lib.fdf_fundamental_points(None, p, p, 4, 4, p, None, 0, 8, 1.0, 0, p, None) == A
    q = np.zeros((4, 2), np.uint32)
    for kw in (dict(n_hyp=0), dict(n_hyp=65537), dict(threshold=-1.0), dict(threshold=float("nan")),
               dict(threshold=float("inf")), dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError):
            fast_hip.estimate_fundamental(q, q, np.arange(4), **kw)
    with pytest.raises(TypeError):
        fast_hip.estimate_fundamental(q, q.astype(np.float32), np.arange(4))
    with pytest.raises(ValueError):
        fast_hip.estimate_fundamental(q, q, np.arange(3))


def estimate(q, t, n_hyp, threshold, seed):
    n = len(q)
    models, mask = ref.fundamental(ref.identity_matches(n), None, n, [0, n], q, t, n, [0, n], n_hyp,
                                   threshold, seed)
    return models[0], mask.astype(bool)


def test_worked_example_through_the_restatement():
    q, t = ref.worked_example()
    m, mask = estimate(q, t, 8, 0.5, 3)
    assert (m["hypothesis"], m["n_inliers"], m["n_valid"], m["n_corr"]) == (2, 10, 8, 12)
    assert mask.astype(int).tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0]
    want = ["0x1.2680dad725570p-59", "0x1.4cc344e4093b5p-57", "-0x1.338fe32749f1dp-52",
            "-0x1.ff7ec58462d65p-58", "-0x1.768667157b6c1p-59", "0x1.0000000000000p+0",
            "0x1.2359a7b2aed39p-53", "-0x1.ffffffffffffep-1", "-0x1.b7ffffffffffcp-48"]
    assert [float(v).hex() for v in m["h"]] == want
    assert np.allclose(m["h"], [0, 0, 0, 0, 0, 1, 0, -1, 0], rtol=0, atol=2.0 ** -40)
    _, x, y, u, v = rref.correspondences(ref.identity_matches(12), None, 12, [0, 12], q, t, 12,
                                         [0, 12], 0)
    assert ref.estimate(x, y, u, v, 0, 8, 0.5, 3)[2].tolist() == [8, 8, 10, 9, 8, 8, 8, 8]
    # the same from float coordinates
    again, mask2 = estimate(q.astype(np.float32), t.astype(np.float32), 8, 0.5, 3)
    assert ref.models_bits_equal(again, m) and np.array_equal(mask, mask2)


def test_fit_is_exact_on_eight_exact_pairs():
    """Eight pairs of a rectified rig: the largest entry is exactly +1, f8 is (nearly) 0 and
    every pair has a residual at rounding level."""
    q, t, true = ref.scene_b(0)
    i = np.flatnonzero(true)[:8]
    f, valid = ref.fit(q[i, 0], q[i, 1], t[i, 0], t[i, 1])
    assert valid and max(abs(v) for v in f) == 1.0 and 1.0 in f
    assert ref.inliers(f, q[i, 0].astype(float), q[i, 1].astype(float), t[i, 0].astype(float),
                       t[i, 1].astype(float), 2.0 ** -20).all()


def test_fit_of_degenerate_samples_is_invalid():
    same = [5.0] * 8
    assert not ref.fit(same, same, same, same)[1]                      # d = 0
    line = [float(k) for k in range(8)]
    assert not ref.fit(line, line, line, line)[1]                      # a pivot below 2^-20
    bad = list(line)
    bad[3] = float("nan")
    assert not ref.fit(bad, line[::-1], line, same)[1]
    bad[3] = float("inf")
    assert not ref.fit(bad, line[::-1], line, same)[1]


# ---- the ground-truth conditions of the device test's scenes ------------------------------------

def test_scene_a_exact():
    q, t, true = ref.scene_a(0)
    m, mask = estimate(q, t, 256, 2.0 ** -7, 0)
    assert true.sum() == 140 and mask[true].all() and not mask[~true].any()
    assert m["n_inliers"] == 140


def test_scene_a_noisy():
    q, t, true = ref.scene_a(0, noise=0.3)
    m, mask = estimate(q, t, 256, 1.0, 3)
    assert mask[true].all() and mask[~true].sum() <= 3


def test_scene_b_rectified_pair():
    q, t, true = ref.scene_b(0)
    m, mask = estimate(q, t, 64, 0.5, 0)
    assert true.sum() == 80 and mask[true].all() and not mask[~true].any()
    f = m["h"] * np.sign(m["h"][5])
    assert np.allclose(f, [0, 0, 0, 0, 0, 1, 0, -1, 0], rtol=0, atol=2.0 ** -30)
    # the rig's own matrix flags exactly the pairs on one row
    rig = np.zeros(1, dtype=ref.MODEL_DTYPE)
    rig["h"][0] = [0, 0, 0, 0, 0, 1, 0, -1, 0]
    n = len(q)
    out, bytes_ = ref.check(ref.identity_matches(n), None, n, [0, n], q, t, n, [0, n], rig, 0.5)
    dy = np.abs(t[:, 1].astype(np.int64) - q[:, 1].astype(np.int64))
    assert np.array_equal(bytes_.astype(bool), dy <= 0.5) and out[0]["n_inliers"] == 80


def test_scene_c_plane_has_no_model():
    q, t = ref.scene_c(0)
    m, mask = estimate(q, t, 64, 0.5, 0)
    assert m["n_valid"] == 0 and m["hypothesis"] == ref.NONE and not m["h"].any()
    assert m["n_corr"] == 60 and not mask.any()


def test_check_follows_the_estimate():
    """check() with the estimator's own model and threshold gives its counts and bytes; a record
    without a model is copied."""
    q, t, _ = ref.scene_a(0)
    n = len(q)
    args = (ref.identity_matches(n), None, n, [0, n], q, t, n, [0, n])
    models, mask = ref.fundamental(*args, 64, 0.25, 1)
    again, mask2 = ref.check(*args, models, 0.25)
    assert ref.models_bits_equal(again, models) and np.array_equal(mask, mask2)
    none = np.zeros(1, dtype=ref.MODEL_DTYPE)
    none["hypothesis"], none["n_corr"] = ref.NONE, 77
    out, bytes_ = ref.check(*args, none, 0.25, inliers_out=np.full(n + 4, 9, np.uint8))
    assert out.tobytes() == none.tobytes() and not bytes_[:n].any() and (bytes_[n:] == 9).all()
