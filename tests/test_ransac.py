"""CPU tests of the RANSAC stage: the numpy reference of tests/_ransac_reference.py and the host
sampler fdf_ransac_sample pinned to include/fdf.h's worked values and compared over a grid, the
scratch size, the worked example through the reference, the layout of fdf_model and the argument
checks that are made before any device call."""
import ctypes
import itertools

import numpy as np
import pytest

import _ransac_reference as ref
from feature_detector_fast_amd import _native, fast_hip

A = _native.FDF_ERR_ARG


def c_sample(seed, frame, hyp, m, s):
    idx = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    draws = ctypes.c_uint32(99)
    rc = _native.load().fdf_ransac_sample(seed, frame, hyp, m, s, idx, ctypes.byref(draws))
    assert rc == _native.FDF_OK
    return list(idx), draws.value


def test_worked_sampling_values():
    assert ref.start_state(1, 0, 0) == 0xB0198235
    for args, want in (((1, 0, 0, 100, 4), ([54, 11, 77, 18], 4)),
                       ((1, 2, 7, 5, 4), ([1, 0, 4, 2], 5)),
                       ((0, 0, 0, 4, 4), ([2, 1, 3, 0], 7))):
        assert ref.sample(*args) == want
        assert c_sample(*args) == want
        assert fast_hip.ransac_sample(*args) == want


def test_sampler_against_reference_grid():
    invalid = 0
    for seed, f, h, m, s in itertools.product((0, 1, 0xFFFFFFFF, 123456789), (0, 1, 65534),
                                              (0, 1, 63, 64, 65535),
                                              (3, 4, 5, 64, 100, 2 ** 32 - 2), (3, 4)):
        want, draws = ref.sample(seed, f, h, m, s)
        got, got_draws = c_sample(seed, f, h, m, s)
        assert got_draws == draws, (seed, f, h, m, s)
        if want is None:
            invalid += 1
            assert got == [ref.NONE] * 4
        else:
            assert got[:s] == want and len(set(want)) == s and max(want) < m
            assert s == 4 or got[3] == ref.NONE
    assert invalid > 0                                   # m = 3 with s = 4 at the least


@pytest.mark.parametrize("m,s", [(0, 3), (1, 3), (2, 3), (0, 4), (3, 4)])
def test_too_few_correspondences_give_no_sample(m, s):
    for h in range(20):
        assert ref.sample(5, 1, h, m, s) == (None, 16)
        assert c_sample(5, 1, h, m, s) == ([ref.NONE] * 4, 16)
        assert fast_hip.ransac_sample(5, 1, h, m, s) == (None, 16)


def test_sample_argument_errors():
    lib = _native.load()
    idx = (ctypes.c_uint32 * 4)()
    for s in (0, 2, 5):
        assert lib.fdf_ransac_sample(0, 0, 0, 10, s, idx, None) == A
        with pytest.raises(ValueError):
            fast_hip.ransac_sample(0, 0, 0, 10, s)
    assert lib.fdf_ransac_sample(0, 0, 0, 10, 4, None, None) == A
    assert lib.fdf_ransac_sample(0, 0, 0, 10, 4, idx, None) == _native.FDF_OK     # draws may be NULL
    with pytest.raises(ValueError):
        fast_hip.ransac_sample(-1, 0, 0, 10, 4)
    with pytest.raises(ValueError):
        fast_hip.ransac_sample(0, 0, 0, 1 << 32, 4)


def scratch(n_frames, q_cap, n_hyp):
    v = ctypes.c_uint64(0)
    rc = _native.load().fdf_ransac_scratch_bytes(n_frames, q_cap, n_hyp, ctypes.byref(v))
    return rc, v.value


def test_scratch_bytes():
    lib = _native.load()
    assert lib.fdf_ransac_scratch_bytes(1, 10, 10, None) == A
    for bad in ((65536, 10, 10), (1, 2 ** 32 - 1, 10), (1, 10, 0), (1, 10, 65537)):
        assert scratch(*bad)[0] == A, bad
    for bad in ((65536, 10, 10), (1, 2 ** 32 - 1, 10), (1, 10, 0), (1, 10, 65537), (-1, 1, 1)):
        with pytest.raises(ValueError):
            fast_hip.ransac_scratch_bytes(*bad)
    # enough for the documented parts, a multiple of 256, and monotone in every argument
    for f, q, n in itertools.product((0, 1, 4, 65535), (0, 1, 300, 2 ** 32 - 2), (1, 64, 65536)):
        rc, got = scratch(f, q, n)
        assert rc == _native.FDF_OK and got % 256 == 0
        assert got >= 32 * q + 4 * f + 4 * f * n
        assert got == fast_hip.ransac_scratch_bytes(f, q, n)
        for f2, q2, n2 in ((f + 1, q, n), (f, q + 100, n), (f, q, n + 100)):
            if f2 <= 65535 and q2 <= 2 ** 32 - 2 and n2 <= 65536:
                assert scratch(f2, q2, n2)[1] >= got


def test_worked_example_through_the_reference():
    q, t = ref.worked_example()
    matches = ref.identity_matches(6)
    for model in (ref.AFFINE, ref.HOMOGRAPHY):
        models, mask = ref.ransac(matches, None, 6, [0, 6], q, t, 6, [0, 6], model, 8, 1.0, 0)
        m = models[0]
        assert (m["hypothesis"], m["n_inliers"], m["n_valid"], m["n_corr"]) == (3, 5, 8, 6)
        assert mask.tolist() == [1, 1, 1, 1, 0, 1]
        assert m["h"].tolist() == [1, 0, 3, 0, 1, 5, 0, 0, 1]           # -0.0 == 0.0
        # the same from float coordinates
        again, mask2 = ref.ransac(matches, None, 6, [0, 6], q.astype(np.float32),
                                  t.astype(np.float32), 6, [0, 6], model, 8, 1.0, 0)
        assert ref.models_equal(again, models) and np.array_equal(mask, mask2)
    _, x, y, u, v = ref.correspondences(matches, None, 6, [0, 6], q, t, 6, [0, 6], 0)
    counts = ref.estimate(x, y, u, v, 0, ref.HOMOGRAPHY, 8, 1.0, 0)[2]
    assert counts.tolist() == [1, 2, 1, 5, 2, 1, 2, 2]


def test_reference_correspondence_rules():
    """keep, FDF_MATCH_NONE, the train range and q_cap each remove a query; the inlier bytes
    outside the frames' range keep the caller's fill."""
    q, t = ref.worked_example()
    q = np.concatenate([q, q])
    t = np.concatenate([t, t])
    matches = ref.identity_matches(12)
    matches["index"][7] = ref.NONE
    matches["index"][8] = 2                              # frame 1's train range is [6, 12)
    keep = np.ones(12, np.uint8)
    keep[9] = 0
    fill = np.full(14, 0x77, np.uint8)
    models, mask = ref.ransac(matches, keep, 11, [1, 6, 12], q, t, 12, [0, 6, 12],
                              ref.AFFINE, 32, 1.0, 3, inliers_out=fill)
    assert models["n_corr"].tolist() == [5, 2]           # 1..5, and 6 and 10 (11 is past q_cap)
    assert mask[0] == 0x77 and (mask[11:] == 0x77).all()
    assert mask[1:6].tolist() == [1, 1, 1, 0, 1]
    assert models[1]["hypothesis"] == ref.NONE and not mask[6:11].any()
    assert not models[1]["h"].any() and models[1]["n_valid"] == 0


def test_model_layout():
    assert ctypes.sizeof(_native.FdfModel) == 88 and ctypes.alignment(_native.FdfModel) == 8
    assert _native.FdfModel.n_corr.offset == 72 and _native.FdfModel.n_valid.offset == 84
    assert fast_hip.MODEL_DTYPE == ref.MODEL_DTYPE and fast_hip.MODEL_DTYPE.itemsize == 88
    assert fast_hip.RANSAC_NONE == ref.NONE
    rec = np.zeros(2, dtype=fast_hip.MODEL_DTYPE)
    rec["h"][1], rec["n_corr"][1], rec["n_valid"][1] = np.arange(9), 5, 7
    got = fast_hip.unpack_models(rec.view(np.float64).reshape(2, 11))
    assert np.array_equal(got, rec)
    with pytest.raises(TypeError):
        fast_hip.unpack_models(np.zeros((2, 9)))


def test_c_entries_reject_bad_arguments_before_any_device_call():
    lib = _native.load()
    p = ctypes.c_void_p(4096)                            # never dereferenced: no context
    assert lib.fdf_ransac_device(None, 1, p, None, 8, p, p, p, 8, p, 0, 1, 16, 3.0, 0, p, None, p,
                                 1 << 20, None) == A
    model = _native.FdfModel()
    assert lib.fdf_ransac_points(None, p, p, 8, 8, p, None, 0, 1, 16, 3.0, 0,
                                 ctypes.byref(model), None) == A


def test_ransac_device_argument_checks():
    torch = pytest.importorskip("torch")
    matches = torch.zeros((8, 2), dtype=torch.int32)
    offs = torch.zeros(3, dtype=torch.int64)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    fpts = torch.zeros((8, 2), dtype=torch.float32)
    models = torch.zeros((2, 11), dtype=torch.float64)
    need = fast_hip.ransac_scratch_bytes(2, 8, 256)
    raw = torch.zeros(need + 512, dtype=torch.uint8)
    lead = (-raw.data_ptr()) % 256
    scratch = raw[lead:lead + need]
    flags = torch.zeros(8, dtype=torch.uint8)
    good = dict(matches=matches, q_offsets=offs, q_coords=pts, t_coords=pts, t_offsets=offs,
                models=models, scratch=scratch)
    for bad in (dict(matches=matches.to(torch.int64)), dict(matches=matches.reshape(-1)),
                dict(q_offsets=offs.to(torch.int32)), dict(t_offsets=offs[:2]),
                dict(q_coords=pts[:7]), dict(q_coords=fpts),            # mixed types
                dict(t_coords=fpts), dict(q_coords=pts.to(torch.int64)),
                dict(t_coords=torch.zeros((8, 3), dtype=torch.int32)),
                dict(q_coords=fpts.to(torch.float64), t_coords=fpts.to(torch.float64)),
                dict(models=models.to(torch.float32)), dict(models=models[:1]),
                dict(models=torch.zeros((2, 9), dtype=torch.float64)),
                dict(scratch=scratch[:-1]), dict(scratch=scratch.to(torch.int8)),
                dict(scratch=raw[lead + 1:lead + 1 + need]),            # misaligned
                dict(keep=flags[:7]), dict(keep=flags.to(torch.int32)),
                dict(inliers=flags[:7]), dict(inliers=flags.to(torch.bool)),
                dict(model="similarity"), dict(model=2), dict(n_hyp=0), dict(n_hyp=65537),
                dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(threshold=1e39),                                   # not finite as a float
                dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError):
            fast_hip.ransac_device(**{**good, **bad})
    # every check passed: the call gets as far as the device check
    for ok in (dict(), dict(q_coords=fpts, t_coords=fpts), dict(keep=flags, inliers=flags),
               dict(model="affine", threshold=0.0, seed=0xFFFFFFFF),
               dict(n_hyp=1, scratch=scratch[:fast_hip.ransac_scratch_bytes(2, 8, 1)])):
        with pytest.raises(ValueError, match="CUDA"):
            fast_hip.ransac_device(**{**good, **ok})


def test_estimate_model_argument_checks():
    q = np.zeros((4, 2), np.uint32)
    t = np.zeros((5, 2), np.uint32)
    m = np.zeros(4, dtype=fast_hip.MATCH_DTYPE)
    for bad in (dict(q_points=q.astype(np.float64)), dict(q_points=q.reshape(-1)),
                dict(t_points=t.astype(np.float32)),                   # mixed types
                dict(matches=np.zeros((4, 3), np.int32)), dict(matches=np.zeros(4, np.float32))):
        with pytest.raises(TypeError):
            fast_hip.estimate_model(**{**dict(q_points=q, t_points=t, matches=m), **bad})
    for bad in (dict(matches=m[:3]), dict(keep=np.ones(3)), dict(model="rigid"), dict(n_hyp=0),
                dict(threshold=-0.5), dict(seed=-1), dict(matches=np.array([0, 1, 2, 1 << 32]))):
        with pytest.raises(ValueError):
            fast_hip.estimate_model(**{**dict(q_points=q, t_points=t, matches=m), **bad})
    rec = fast_hip._host_matches(np.array([3, -1, 0, 2]), 4)
    assert rec["index"].tolist() == [3, fast_hip.MATCH_NONE, 0, 2]
