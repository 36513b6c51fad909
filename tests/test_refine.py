"""CPU tests of the refinement stage: the numpy restatement of tests/_refine_reference.py (the
order of its sums against a plain loop, its elimination against _ransac_reference.fit bit for
bit, its solution against numpy.linalg.lstsq, include/fdf.h's worked example, what it gains on
planted data, the degenerate cases and the acceptance rule), the scratch size and the argument
checks that are made before any device call."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import _ransac_reference as rr
import _refine_reference as ref
from feature_detector_fast_amd import _native, fast_hip

A = _native.FDF_ERR_ARG
MODELS = {"affine": rr.AFFINE, "homography": rr.HOMOGRAPHY}
PLANTED = {"affine": np.array([[1.03, 0.04, 12.0], [-0.03, 0.97, 25.0], [0.0, 0.0, 1.0]]),
           "homography": np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, 40.0], [1e-5, -2e-5, 1.0]])}


# ---- the order of the sums ---------------------------------------------------------------------

def plain_ordered_sum(values):
    lanes = [0.0] * 256
    for j, value in enumerate(values):
        lanes[j % 256] = lanes[j % 256] + value
    step = 128
    while step:
        for t in range(step):
            lanes[t] = lanes[t] + lanes[t + step]
        step //= 2
    return lanes[0]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700])
def test_ordered_sum_against_a_plain_loop(n):
    rng = np.random.default_rng(n)
    values = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)     # rounding matters
    assert ref.ordered_sum(values) == plain_ordered_sum(values.tolist())
    two = np.stack([values, values[::-1]], axis=1)
    got = ref.ordered_sum(two)
    assert got.shape == (2,) and got[0] == plain_ordered_sum(values.tolist())
    assert got[1] == plain_ordered_sum(values[::-1].tolist())


def test_member_sum_skips_what_is_no_member():
    values = np.array([1.0, np.nan, 2.0, np.inf, 4.0])
    flags = np.array([True, False, True, False, True])
    assert ref.member_sum(flags, [values, np.ones(5)]).tolist() == [7.0, 3.0]


# ---- the elimination is _ransac_reference.fit's --------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_solve_is_the_ransac_elimination(model):
    """The systems of 200 samples (some of them degenerate), built as fit builds them, through
    solve: the same bits and the same validity as fit."""
    s = rr.sample_size(MODELS[model])
    rng = np.random.default_rng(5)
    x, y, u, v = (rng.integers(0, 50, (200, s)).astype(np.float64) for _ in range(4))
    x[:20, 1], y[:20, 1] = x[:20, 0], y[:20, 0]           # a repeated point: no pivot
    want, want_valid = rr.fit(x, y, u, v, MODELS[model])
    N = 2 * s
    sys_a, sys_b = np.zeros((200, N, 8)), np.zeros((200, N))
    for k in range(s):
        xk, yk, uk, vk = x[:, k], y[:, k], u[:, k], v[:, k]
        sys_a[:, 2 * k, :3] = np.stack([xk, yk, np.ones(200)], axis=1)
        sys_a[:, 2 * k, 6:] = np.stack([-(uk * xk), -(uk * yk)], axis=1)
        sys_a[:, 2 * k + 1, 3:6] = np.stack([xk, yk, np.ones(200)], axis=1)
        sys_a[:, 2 * k + 1, 6:] = np.stack([-(vk * xk), -(vk * yk)], axis=1)
        sys_b[:, 2 * k], sys_b[:, 2 * k + 1] = uk, vk
    got, got_valid = ref.solve(sys_a[:, :, :N], sys_b)
    assert np.array_equal(got_valid, want_valid) and 0 < want_valid.sum() < 200
    assert np.array_equal(got, want, equal_nan=True)


# ---- planted data ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted(model, m, outliers, seed, width=640, height=480):
    """(x, y, u, v) float64: `m` integer points in width x height, their rounded projections under
    PLANTED[model], and `outliers` of the trains re-drawn uniformly.  Read-only."""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.integers(0, width, m), rng.integers(0, height, m)], axis=1).astype(np.float64)
    p = np.c_[q, np.ones(m)] @ PLANTED[model].T
    t = np.rint(p[:, :2] / p[:, 2:])
    bad = rng.permutation(m)[:outliers]
    t[bad] = np.stack([rng.integers(0, width, len(bad)), rng.integers(0, height, len(bad))], axis=1)
    out = tuple(np.ascontiguousarray(a) for a in (q[:, 0], q[:, 1], t[:, 0], t[:, 1]))
    for a in out:
        a.setflags(write=False)
    return out


def corner_error(h, truth, width=640, height=480):
    """The largest displacement of an image corner between the maps `h` and `truth`."""
    corners = np.array([[0, 0, 1], [width, 0, 1], [0, height, 1], [width, height, 1]], np.float64)
    a, b = corners @ np.reshape(h, (3, 3)).T, corners @ truth.T
    return np.abs(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).max()


# The largest relative difference between the restatement and lstsq over LSTSQ_CASES, measured on
# the CPU with the function below (2-norms over the nine entries): 8.1e-16 in the normalised
# solution, 1.46e-14 in the denormalised model (the translation entries are a few tens, the
# perspective ones 1e-5).  Each bound is 16 x its measured value, for other libm / LAPACK builds.
LSTSQ_MEASURED_NORMALISED, LSTSQ_MEASURED_MODEL = 8.1e-16, 1.46e-14
LSTSQ_BOUND_NORMALISED, LSTSQ_BOUND_MODEL = 16 * LSTSQ_MEASURED_NORMALISED, 16 * LSTSQ_MEASURED_MODEL
LSTSQ_CASES = [(model, m, outliers, seed) for model in ("affine", "homography")
               for m, outliers, seed in ((12, 0, 1), (300, 0, 2), (300, 120, 3), (700, 250, 4))]


def lstsq_differences(model, m, outliers, seed):
    """(relative difference of the normalised solution, of the denormalised model) between the
    restatement's round and numpy.linalg.lstsq on the same normalised stacked rows, from the
    planted map's own inliers."""
    code = MODELS[model]
    x, y, u, v = planted(model, m, outliers, seed)
    flags = rr.inliers(PLANTED[model].reshape(1, 9), x, y, u, v, 1.5)[0]
    assert flags.sum() >= m - outliers - 2
    norm = ref.normalisation(x, y, u, v, flags, code)
    G, g = ref.normal_equations(x, y, u, v, flags, code, norm)
    hn, valid = ref.solve(G[None], g[None])
    assert valid[0]
    h = ref.denormalise(hn[0], norm, code)
    # the independent route: the stacked rows, an SVD solve, 3 x 3 matrix products
    cx, cy, s, cu, cv, t = norm
    X, Y, U, V = ((a[flags] - c) * k for a, c, k in ((x, cx, s), (y, cy, s), (u, cu, t), (v, cv, t)))
    n, N = len(X), 2 * rr.sample_size(code)
    rows, rhs = np.zeros((2 * n, 8)), np.zeros(2 * n)
    rows[0::2, 0], rows[0::2, 1], rows[0::2, 2] = X, Y, 1.0
    rows[0::2, 6], rows[0::2, 7] = -(U * X), -(U * Y)
    rows[1::2, 3], rows[1::2, 4], rows[1::2, 5] = X, Y, 1.0
    rows[1::2, 6], rows[1::2, 7] = -(V * X), -(V * Y)
    rhs[0::2], rhs[1::2] = U, V
    sol = np.linalg.lstsq(rows[:, :N], rhs, rcond=None)[0]
    hn_l = np.r_[sol, np.zeros(8 - N), 1.0]
    T1 = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    T2i = np.array([[1 / t, 0, cu], [0, 1 / t, cv], [0, 0, 1]])
    H = T2i @ hn_l.reshape(3, 3) @ T1
    h_l = (H / H[2, 2]).reshape(9)
    return (np.linalg.norm(hn[0] - hn_l) / np.linalg.norm(hn_l),
            np.linalg.norm(h - h_l) / np.linalg.norm(h_l))


@pytest.mark.parametrize("case", LSTSQ_CASES)
def test_restatement_against_lstsq(case):
    normalised, model = lstsq_differences(*case)
    print(f"lstsq {case}: normalised {normalised:.3g}, model {model:.3g}")
    assert normalised <= LSTSQ_BOUND_NORMALISED and model <= LSTSQ_BOUND_MODEL


def test_normal_matrix_is_well_conditioned():
    """The reason the plain elimination is enough: after the normalisation the normal matrix of
    the quality setup has a condition number of a few tens."""
    x, y, u, v = planted("homography", 300, 120, 3)
    flags = rr.inliers(PLANTED["homography"].reshape(1, 9), x, y, u, v, 1.5)[0]
    norm = ref.normalisation(x, y, u, v, flags, rr.HOMOGRAPHY)
    G, _ = ref.normal_equations(x, y, u, v, flags, rr.HOMOGRAPHY, norm)
    assert np.array_equal(G, G.T) and G[2, 2] == flags.sum() and G[0, 3] == 0
    assert np.array_equal(G[:3, :3], G[3:6, 3:6])
    assert np.linalg.cond(G) < 100


# ---- the worked example of include/fdf.h -------------------------------------------------------

def test_worked_example():
    q, t = rr.worked_example()
    matches = rr.identity_matches(6)
    start = np.zeros(1, dtype=rr.MODEL_DTYPE)
    start[0] = ref.model_record([1, 0, 3, 0, 1, 5, 0, 0, 1], 6, 5, 3, 8)
    _, x, y, u, v = rr.correspondences(matches, None, 6, [0, 6], q, t, 6, [0, 6], 0)
    flags = np.array([1, 1, 1, 1, 0, 1], dtype=bool)
    norm = ref.normalisation(x, y, u, v, flags, rr.HOMOGRAPHY)
    assert norm == (8.0, 4.6, 10 / 53.6, 11.0, 9.6, 10 / 53.6) and norm[2] == 0.18656716417910446
    want = {"affine": [1.0, 0.0, 3.0, 0.0, 1.0, 5.0, 0.0, 0.0, 1.0],
            "homography": [float.fromhex(a) for a in (
                "0x1.0000000000001p+0", "-0x1.dc507e631a7ddp-54", "0x1.7fffffffffffdp+1",
                "0x1.886f0037424e0p-54", "0x1.0000000000000p+0", "0x1.3ffffffffffffp+2",
                "0x1.302010db87537p-57", "-0x1.a85e37930f5e6p-57", "0x1.0p+0")]}
    for model, code in MODELS.items():
        models, mask, rounds = ref.refine(matches, None, 6, [0, 6], q, t, 6, [0, 6], code, start,
                                          1.0, 1)
        assert rounds.tolist() == [1] and mask.tolist() == [1, 1, 1, 1, 0, 1]
        m = models[0]
        assert (m["n_corr"], m["n_inliers"], m["hypothesis"], m["n_valid"]) == (6, 5, 3, 8)
        assert m["h"].tolist() == want[model]
        # float coordinates are the same numbers
        again = ref.refine(matches, None, 6, [0, 6], q.astype(np.float32), t.astype(np.float32), 6,
                           [0, 6], code, start, 1.0, 1)
        assert rr.models_equal(again[0], models) and np.array_equal(again[1], mask)


# ---- what the refinement gains -----------------------------------------------------------------

def test_refinement_improves_planted_homographies():
    """32 seeded pairs of 300 points in 640 x 480, 40 % of the trains re-drawn, 256 hypotheses,
    T = 1.5, two rounds: the median over the pairs of the worst corner displacement against the
    planted map is smaller after the refinement than before."""
    truth = PLANTED["homography"]
    before, after, rounds = [], [], []
    for seed in range(32):
        x, y, u, v = planted("homography", 300, 120, 1000 + seed)
        rec, _, _ = rr.estimate(x, y, u, v, 0, rr.HOMOGRAPHY, 256, 1.5, seed)
        assert rec["hypothesis"] != rr.NONE
        refined, flags, n = ref.refine_frame(x, y, u, v, rec, rr.HOMOGRAPHY, 1.5, 2)
        assert refined["n_inliers"] == flags.sum() >= rec["n_inliers"]
        before.append(corner_error(rec["h"], truth))
        after.append(corner_error(refined["h"], truth))
        rounds.append(n)
    print(f"median worst corner error: {np.median(before):.3f} px before, "
          f"{np.median(after):.3f} px after; better in "
          f"{int(np.sum(np.array(after) < np.array(before)))} of 32; rounds {sorted(set(rounds))}")
    assert np.median(after) < np.median(before)


# ---- degenerate input keeps the model ----------------------------------------------------------

TRANSLATION = [1, 0, 3, 0, 1, 5, 0, 0, 1]


def kept(x, y, u, v, model, rec=None, threshold=1.0, n_rounds=3):
    """Refines `rec` (default: the translation (3, 5)) and checks that nothing was accepted;
    returns the record and the flags."""
    rec = ref.model_record(TRANSLATION, 99, 99, 4, 7) if rec is None else rec
    x, y, u, v = (np.asarray(a, dtype=np.float64) for a in (x, y, u, v))
    out, flags, rounds = ref.refine_frame(x, y, u, v, rec, MODELS[model], threshold, n_rounds)
    assert rounds == 0 and np.array_equal(out["h"], rec["h"], equal_nan=True)
    assert (out["hypothesis"], out["n_valid"]) == (rec["hypothesis"], rec["n_valid"])
    return out, flags


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_degenerate_sets_keep_the_model(model):
    s = rr.sample_size(MODELS[model])
    # all inliers on one point: d = 0
    x, y = np.full(10, 7.0), np.full(10, 9.0)
    out, flags = kept(x, y, x + 3, y + 5, model)
    assert flags.all() and (out["n_corr"], out["n_inliers"]) == (10, 10)
    assert ref.normalisation(x, y, x + 3, y + 5, flags, MODELS[model]) is None
    # collinear inliers: the normalisation passes, a pivot does not
    x = np.arange(20.0) * 7
    y = 2 * x + 3
    out, flags = kept(x, y, x + 3, y + 5, model)
    assert flags.all() and out["n_inliers"] == 20
    assert ref.normalisation(x, y, x + 3, y + 5, flags, MODELS[model]) is not None
    assert ref.refit(x, y, x + 3, y + 5, flags, MODELS[model]) is None
    # one inlier fewer than a sample among outliers
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, 100, 12).astype(np.float64), rng.integers(0, 100, 12).astype(np.float64)
    u, v = x + 40, y + 70
    u[:s - 1], v[:s - 1] = x[:s - 1] + 3, y[:s - 1] + 5
    out, flags = kept(x, y, u, v, model)
    assert flags.sum() == s - 1 == out["n_inliers"] and flags[:s - 1].all()
    # no model: the record passes through as it is, whatever it holds
    rec = ref.model_record(np.arange(9.0), 5, 4, rr.NONE, 0)
    out, flags = kept(x, y, x + 3, y + 5, model, rec=rec)
    assert not flags.any() and (out["n_corr"], out["n_inliers"]) == (5, 4)
    # no correspondences at all
    out, flags = kept([], [], [], [], model)
    assert (out["n_corr"], out["n_inliers"]) == (0, 0)


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_nan_coordinates(model):
    """The score is false for any NaN, so a correspondence with a NaN coordinate is never in the
    set and never enters a sum.  With s - 1 proper inliers beside it the model is kept; with
    enough of them the result is the one without that correspondence."""
    s = rr.sample_size(MODELS[model])
    rng = np.random.default_rng(4)
    x, y = rng.integers(0, 100, 30).astype(np.float64), rng.integers(0, 100, 30).astype(np.float64)
    u, v = x + 3, y + 5
    for bad in (x, v):
        few = [a[:s].copy() for a in (x, y, u, v)]
        few[0 if bad is x else 3][0] = np.nan
        out, flags = kept(*few, model)
        assert flags.tolist() == [False] + [True] * (s - 1) and out["n_inliers"] == s - 1
    rec = ref.model_record([1, 0, 3.25, 0, 1, 4.75, 0, 0, 1])
    xn = x.copy()
    xn[4] = np.nan
    with_nan = ref.refine_frame(xn, y, u, v, rec, MODELS[model], 1.0, 2)
    uo = u.copy()
    uo[4] = 1e6                                           # an outlier in the same lane instead
    without = ref.refine_frame(x, y, uo, v, rec, MODELS[model], 1.0, 2)
    assert np.array_equal(with_nan[0]["h"], without[0]["h"]) and with_nan[2] == without[2] >= 1
    assert with_nan[0]["n_inliers"] == 29 and not with_nan[1][4] and with_nan[0]["n_corr"] == 30
    assert np.allclose(with_nan[0]["h"], TRANSLATION, rtol=0, atol=1e-9)


def test_no_rounds_recount_under_the_threshold():
    x, y, u, v = planted("homography", 300, 120, 3)
    rec, flags3, _ = rr.estimate(x, y, u, v, 0, rr.HOMOGRAPHY, 64, 3.0, 1)
    out, flags, rounds = ref.refine_frame(x, y, u, v, rec, rr.HOMOGRAPHY, 0.75, 0)
    assert rounds == 0 and np.array_equal(out["h"], rec["h"])
    assert np.array_equal(flags, rr.inliers(rec["h"][None], x, y, u, v, 0.75)[0])
    assert 0 < out["n_inliers"] == flags.sum() < rec["n_inliers"] and not (flags & ~flags3).any()
    assert (out["n_corr"], out["hypothesis"], out["n_valid"]) == (300, rec["hypothesis"],
                                                                 rec["n_valid"])


@pytest.mark.parametrize("model", ["affine", "homography"])
def test_a_refit_that_loses_inliers_is_not_accepted(model):
    """20 points under the identity, T = 2: twelve trains moved by (+2, 0), one by (-2, 0), all
    on the edge of the threshold.  The least-squares fit moves towards the twelve and leaves the
    one behind: 19 < 20, so the round is not accepted."""
    rng = np.random.default_rng(6)
    x, y = rng.integers(0, 200, 20).astype(np.float64), rng.integers(0, 200, 20).astype(np.float64)
    u, v = x.copy(), y.copy()
    u[:12] += 2
    u[19] -= 2
    rec = ref.model_record([1, 0, 0, 0, 1, 0, 0, 0, 1])
    out, flags = kept(x, y, u, v, model, rec=rec, threshold=2.0)
    assert flags.all() and out["n_inliers"] == 20
    h2 = ref.refit(x, y, u, v, flags, MODELS[model])
    flags2 = rr.inliers(h2[None], x, y, u, v, 2.0)[0]
    assert flags2.sum() == 19 and not flags2[19]
    # with a threshold that keeps all twenty the same refit is accepted
    out, _, rounds = ref.refine_frame(x, y, u, v, rec, MODELS[model], 4.0, 1)
    assert rounds == 1 and np.array_equal(out["h"], h2) and out["n_inliers"] == 20


# ---- the C and Python entries before any device call ---------------------------------------------

def scratch(n_frames, q_cap):
    v = ctypes.c_uint64(0)
    rc = _native.load().fdf_refine_scratch_bytes(n_frames, q_cap, ctypes.byref(v))
    return rc, v.value


def test_scratch_bytes():
    lib = _native.load()
    assert lib.fdf_refine_scratch_bytes(1, 10, None) == A
    for bad in ((65536, 10), (1, 2 ** 32 - 1)):
        assert scratch(*bad)[0] == A, bad
    for bad in ((65536, 10), (1, 2 ** 32 - 1), (-1, 1), (1, -1)):
        with pytest.raises(ValueError):
            fast_hip.refine_scratch_bytes(*bad)
    assert scratch(1, 1) == (_native.FDF_OK, 512) and scratch(0, 0) == (_native.FDF_OK, 0)
    assert scratch(64, 8) == (_native.FDF_OK, 512) and scratch(65, 9) == (_native.FDF_OK, 1024)
    for f, q in itertools.product((0, 1, 4, 65535), (0, 1, 300, 2 ** 32 - 2)):
        rc, got = scratch(f, q)
        assert rc == _native.FDF_OK and got % 256 == 0 and got >= 32 * q + 4 * f
        assert got == fast_hip.refine_scratch_bytes(f, q)
        assert got < 32 * q + 4 * f + 512                  # two parts, each rounded up to 256
        assert got <= fast_hip.ransac_scratch_bytes(f, q, 1)


def test_c_entries_reject_bad_arguments_before_any_device_call():
    lib = _native.load()
    p = ctypes.c_void_p(4096)                            # never dereferenced: no context
    assert lib.fdf_refine_device(None, 1, p, None, 8, p, p, p, 8, p, 0, 1, p, 3.0, 2, p, None, None,
                                 p, 1 << 20, None) == A
    model = _native.FdfModel()
    assert lib.fdf_refine_points(None, p, p, 8, 8, p, None, 0, 1, ctypes.byref(model), 3.0, 2,
                                 ctypes.byref(model), None, None) == A


def test_refine_device_argument_checks():
    torch = pytest.importorskip("torch")
    matches = torch.zeros((8, 2), dtype=torch.int32)
    offs = torch.zeros(3, dtype=torch.int64)
    pts = torch.zeros((8, 2), dtype=torch.int32)
    fpts = torch.zeros((8, 2), dtype=torch.float32)
    models = torch.zeros((2, 11), dtype=torch.float64)
    need = fast_hip.refine_scratch_bytes(2, 8)
    raw = torch.zeros(need + 512, dtype=torch.uint8)
    lead = (-raw.data_ptr()) % 256
    scratch_t = raw[lead:lead + need]
    flags = torch.zeros(8, dtype=torch.uint8)
    rounds = torch.zeros(2, dtype=torch.int32)
    good = dict(matches=matches, q_offsets=offs, q_coords=pts, t_coords=pts, t_offsets=offs,
                models_in=models, models_out=models, scratch=scratch_t)
    for bad in (dict(matches=matches.to(torch.int64)), dict(q_offsets=offs.to(torch.int32)),
                dict(t_offsets=offs[:2]), dict(q_coords=pts[:7]), dict(q_coords=fpts),
                dict(t_coords=torch.zeros((8, 3), dtype=torch.int32)),
                dict(models_in=models.to(torch.float32)), dict(models_in=models[:1]),
                dict(models_out=models[:1]), dict(models_out=torch.zeros((2, 9), dtype=torch.float64)),
                dict(scratch=scratch_t[:-1]), dict(scratch=scratch_t.to(torch.int8)),
                dict(scratch=raw[lead + 1:lead + 1 + need]),            # misaligned
                dict(keep=flags[:7]), dict(inliers=flags[:7]), dict(inliers=flags.to(torch.bool)),
                dict(rounds=rounds[:1]), dict(rounds=rounds.to(torch.int64)),
                dict(model="similarity"), dict(n_rounds=-1), dict(n_rounds=9),
                dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=1e39)):
        with pytest.raises(ValueError):
            fast_hip.refine_device(**{**good, **bad})
    # every check passed: the call gets as far as the device check
    for ok in (dict(), dict(q_coords=fpts, t_coords=fpts), dict(keep=flags, inliers=flags),
               dict(rounds=rounds, n_rounds=8), dict(model="affine", threshold=0.0, n_rounds=0),
               dict(models_out=torch.zeros((3, 11), dtype=torch.float64))):
        with pytest.raises(ValueError, match="CUDA"):
            fast_hip.refine_device(**{**good, **ok})


def test_host_entry_argument_checks():
    q = np.zeros((4, 2), np.uint32)
    t = np.zeros((5, 2), np.uint32)
    m = np.zeros(4, dtype=fast_hip.MATCH_DTYPE)
    rec = np.zeros((), dtype=fast_hip.MODEL_DTYPE)
    base = dict(q_points=q, t_points=t, matches=m, estimate=rec)
    for bad in (dict(q_points=q.astype(np.float64)), dict(t_points=t.astype(np.float32)),
                dict(estimate=np.zeros(8)), dict(estimate="none"),
                dict(estimate=np.zeros(2, dtype=fast_hip.MODEL_DTYPE))):
        with pytest.raises(TypeError):
            fast_hip.refine_model(**{**base, **bad})
    for bad in (dict(matches=m[:3]), dict(keep=np.ones(3)), dict(model="rigid"), dict(n_rounds=9),
                dict(n_rounds=-1), dict(threshold=-0.5)):
        with pytest.raises(ValueError):
            fast_hip.refine_model(**{**base, **bad})
    for bad in (9, -1):
        with pytest.raises(ValueError):
            fast_hip.estimate_model(q, t, m, refine_rounds=bad)
    assert {"refine_scratch_bytes", "refine_device", "refine_model"} <= set(fast_hip.__all__)
