"""CPU tests of the tracker's host side: the level maps of libfdf.so against the numpy
restatement of include/fdf.h's rules (tests/_track_reference.py), the restatement against the
header's worked example and against an independent float64 Lucas-Kanade, its accuracy on a scene
built from the library's own exact rules, and the argument checks that run before any device
call."""
import ctypes
import functools

import numpy as np
import pytest

import _brief_reference as br
import _resize_reference as rs
import _track_reference as tr
import _warp_reference as wr
from feature_detector_fast_amd import FdfError, _native, fast_hip

A = _native.FDF_ERR_ARG
EPS = 20                                     # 1/2048 pixel: the stopping rule of every run here


# ---- the level maps of the library against the restatement -------------------------------------

def lib_map_pos(x, len0, lenl):
    return fast_hip.track_map_position(x, len0, lenl)


def lib_map_disp(d, a, b):
    return fast_hip.track_map_displacement(d, a, b)


def test_map_worked_values():
    for fn_pos, fn_disp in ((tr.map_pos, tr.map_disp), (lib_map_pos, lib_map_disp)):
        assert fn_pos(29372, 32, 16) == 14174
        assert fn_disp(-3001, 16, 32) == -6002
        assert fn_disp(-3001, 32, 16) == -1500
        assert fn_disp(5, 6, 5) == 4


def test_map_range_ends():
    top = 1 << 28
    for v in (-top, -top + 1, -1, 0, 1, top - 1, top):
        for a in (1, 2, 65535):
            for b in (1, 2, 65535):
                assert lib_map_pos(v, a, b) == tr.map_pos(v, a, b)
                assert lib_map_disp(v, a, b) == tr.map_disp(v, a, b)
    # a position is clamped into its level; equal lengths change nothing inside the frame
    assert lib_map_pos(-5, 32, 16) == 0 and lib_map_pos(top, 32, 16) == 15 * 2048
    for x in (0, 1, 1023, 1024, 31 * 2048):
        assert lib_map_pos(x, 32, 32) == x
    for d in (-4097, -1, 0, 1, 4097):
        assert lib_map_disp(d, 77, 77) == d


def test_map_random_sweep():
    rng = np.random.default_rng(11)
    n = 4000
    v = rng.integers(-(1 << 28), (1 << 28) + 1, n)
    a = rng.integers(1, 65536, n)
    b = rng.integers(1, 65536, n)
    v[: n // 2] = rng.integers(-70000, 70000, n // 2)          # and the small, signed ones
    a[: n // 4] = rng.integers(1, 40, n // 4)
    b[n // 8: n // 2] = rng.integers(1, 40, n // 2 - n // 8)
    for x, p, q in zip(v.tolist(), a.tolist(), b.tolist()):
        assert lib_map_pos(x, p, q) == tr.map_pos(x, p, q), (x, p, q)
        assert lib_map_disp(x, p, q) == tr.map_disp(x, p, q), (x, p, q)


def test_map_rejected_arguments():
    lib = _native.load()
    out = ctypes.c_int64(77)
    for fn in (lib.fdf_track_map_position, lib.fdf_track_map_displacement):
        for v, a, b in ((0, 0, 5), (0, 5, 0), (0, 65536, 5), (0, 5, 65536), ((1 << 28) + 1, 5, 5),
                        (-(1 << 28) - 1, 5, 5), (1 << 62, 5, 5)):
            assert fn(v, a, b, ctypes.byref(out)) == A
        assert fn(0, 5, 5, None) == A
    assert out.value == 77
    with pytest.raises(FdfError):
        fast_hip.track_map_position(0, 0, 5)


# ---- the restatement against the header's worked example -----------------------------------------

def worked(levels=1, start=(14 * 2048, 10 * 2048), frames=None, **kw):
    a, b = frames or tr.worked_frames()
    args = dict(radius=3, max_iters=30, eps=EPS, min_eig=0.25)
    args.update(kw)
    trace = []
    res = tr.track_point(rs.pyramid(a, levels, 2, 1), rs.pyramid(b, levels, 2, 1), start[0], start[1],
                         trace=trace, **args)
    return res, trace


def test_worked_example():
    res, trace = worked()
    assert trace[0]["A"] == (184786944, 270729216, 533045248)
    assert trace[0]["b"][0] == (-24637440, -41500672)
    assert trace[0]["pos"][0] == (33605, 23077)
    assert res == (tr.TRACKED, 32773, 22529, 0, 4)
    assert worked(max_iters=1)[0] == (tr.TRACKED, 33605, 23077, 1789, 1)
    assert worked(min_eig=1.0)[0] == (tr.LOST_EIGEN, -1, -1, tr.NO_ERR, 0)
    assert rs.pyramid(tr.worked_frames()[0], 2, 2, 1)[1].shape == (12, 16)
    assert worked(levels=2)[0] == (tr.TRACKED, 32773, 22530, 0, 5)
    assert worked(start=(29372, 21780))[0][:4] == (tr.TRACKED, 33469, 23826, 0)
    assert worked(levels=2, start=(29372, 21780))[0][:4] == (tr.TRACKED, 33468, 23826, 2)
    flat = np.full((24, 32), 7, np.uint8)
    assert worked(frames=(flat, flat), min_eig=0.0)[0] == (tr.LOST_EIGEN, -1, -1, tr.NO_ERR, 0)


def test_skips_and_losses_of_the_restatement():
    a, b = tr.worked_frames()
    lost = lambda reason, it=0: (reason, -1, -1, tr.NO_ERR, it)
    for X, Y in ((-1, 0), (0, -1), (31 * 2048 + 1, 0), (0, 23 * 2048 + 1)):
        assert tr.track_point([a], [b], X, Y, None, 3, 30, EPS, 0.25) == lost(tr.SKIPPED)
        assert tr.track_point([a], [b], 2048, 2048, (X, Y), 3, 30, EPS, 0.25) == lost(tr.SKIPPED)
    # the frame's corners are valid positions
    assert tr.track_point([a], [b], 31 * 2048, 23 * 2048, None, 3, 30, EPS, 0.0)[0] != tr.SKIPPED
    # a guess is the start: the true position as the guess converges at once
    res = tr.track_point([a], [b], 14 * 2048, 10 * 2048, (16 * 2048, 11 * 2048), 3, 30, EPS, 0.25)
    assert res[0] == tr.TRACKED and res[4] == 1 and res[3] == 0
    out = tr.track([[a]], [[b]], np.array([[14, 10], [40, 3], [5, 5]]), [0, 3], 2, radius=3,
                   min_eig=0.25)
    assert out["written"].tolist() == [True, True]               # cap cuts the third point
    assert out["status"].tolist() == [1, 0] and out["info"].tolist() == [1 | 4 << 8, 0]
    assert out["matches"].tolist() == [[0, 0xFFFF0000], [tr.MATCH_NONE, 0xFFFFFFFF]]
    assert out["f32"].tolist() == [[32773 / 2048, 22529 / 2048], [-1.0, -1.0]]


# ---- an independent float64 Lucas-Kanade ---------------------------------------------------------

def float_sample(img, x, y):
    """Continuous bilinear samples of a float image at clamped taps."""
    h, w = img.shape
    x0 = np.floor(x).astype(np.int64)
    y0 = np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    cx = lambda v: np.clip(v, 0, w - 1)
    cy = lambda v: np.clip(v, 0, h - 1)
    top = img[cy(y0), cx(x0)] * (1 - fx) + img[cy(y0), cx(x0 + 1)] * fx
    bot = img[cy(y0 + 1), cx(x0)] * (1 - fx) + img[cy(y0 + 1), cx(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def float_lk(prev, nxt, x, y, radius, max_iters, eps, min_eig):
    """Pyramidal Lucas-Kanade in float64 pixels with no quantisation anywhere: the same window,
    Scharr weights, level geometry and stopping rule, written without the restatement.  Returns
    (x, y, iterations) or None for a lost point."""
    r = radius
    n = (2 * r + 1) ** 2
    h0, w0 = prev[0].shape
    d = np.zeros(2)
    grid = np.arange(-r - 1, r + 2, dtype=np.float64)
    iters = 0
    pos = None
    for l in range(len(prev) - 1, -1, -1):
        a, b = prev[l].astype(np.float64), nxt[l].astype(np.float64)
        h, w = a.shape
        if l < len(prev) - 1:
            hu, wu = prev[l + 1].shape
            d = d * np.array([w / wu, h / hu])
        c = np.array([np.clip((x + 0.5) * w / w0 - 0.5, 0, w - 1),
                      np.clip((y + 0.5) * h / h0 - 0.5, 0, h - 1)])
        patch = float_sample(a, c[0] + grid[None, :], c[1] + grid[:, None])
        kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], dtype=np.float64)
        gx = np.zeros((2 * r + 1, 2 * r + 1))
        gy = np.zeros((2 * r + 1, 2 * r + 1))
        for v in range(3):
            for u in range(3):
                part = patch[v:v + 2 * r + 1, u:u + 2 * r + 1]
                gx += kx[v, u] * part
                gy += kx.T[v, u] * part
        tmpl = patch[1:-1, 1:-1]
        g = np.array([[np.sum(gx * gx), np.sum(gx * gy)], [np.sum(gx * gy), np.sum(gy * gy)]])
        # the mean gradient matrix in grey levels^2 per pixel^2: the Scharr gain is 32
        if np.linalg.eigvalsh(g / (1024.0 * n))[0] <= min_eig:
            if l == 0:
                return None
            continue
        pos = c + d
        if not (0 <= pos[0] <= w - 1 and 0 <= pos[1] <= h - 1):
            return None
        inner = grid[1:-1]
        for _ in range(max_iters):
            e = float_sample(b, pos[0] + inner[None, :], pos[1] + inner[:, None]) - tmpl
            iters += 1
            step = -32.0 * np.linalg.solve(g, np.array([np.sum(e * gx), np.sum(e * gy)]))
            pos = pos + step
            if not (0 <= pos[0] <= w - 1 and 0 <= pos[1] <= h - 1):
                return None
            if np.abs(step).sum() * 2048 <= eps:
                break
        d = pos - c
    return pos[0], pos[1], iters


def test_float_lk_agrees_on_the_worked_example():
    a, b = tr.worked_frames()
    x, y, iters = float_lk([a], [b], 14, 10, 3, 30, EPS, 0.25)
    assert abs(iters - 4) <= 1 and abs(x - 16) * 2048 <= EPS and abs(y - 11) * 2048 <= EPS
    assert float_lk([a], [b], 14, 10, 3, 30, EPS, 1.0) is None
    flat = np.full((24, 32), 7, np.uint8)
    assert float_lk([flat], [flat], 14, 10, 3, 30, EPS, 0.0) is None


# ---- accuracy on a scene built from the library's own exact rules -----------------------------------

POINTS = [(x, y) for y in range(40, 130, 18) for x in range(40, 200, 23)]


@functools.lru_cache(maxsize=None)
def big_scene():
    small = np.random.default_rng(7).integers(0, 256, (24, 32)).astype(np.uint8)
    big = br.smooth(rs.resize(small, 256, 192))
    big.setflags(write=False)
    return big


def shifted_pair(sx, sy):
    big = big_scene()
    return big[24:168, 24:232], big[24 - sy:168 - sy, 24 - sx:232 - sx]


@functools.lru_cache(maxsize=None)
def scene_run(sx, sy, n_levels, radius):
    """Both formulations on every point of a shifted pair: [(restatement result, float result)]."""
    a, b = shifted_pair(sx, sy)
    pa, pb = rs.pyramid(a, n_levels, 2, 1), rs.pyramid(b, n_levels, 2, 1)
    return [(tr.track_point(pa, pb, x * 2048, y * 2048, None, radius, 30, EPS, 1.0),
             float_lk(pa, pb, x, y, radius, 30, EPS, 1.0)) for x, y in POINTS]


CASES = [(1, 0, 3, 5), (3, 2, 3, 5), (7, -5, 3, 5), (12, 9, 4, 7), (-10, 11, 4, 7)]


@pytest.mark.parametrize("sx,sy,n_levels,radius", CASES)
def test_accuracy_at_integer_shifts(sx, sy, n_levels, radius):
    """No point lost and every point within eps = 20/2048 pixel of the true shift on both axes:
    at an integer shift the true position is an exact fixed point (E = 0 there) and the loop
    stops one step of at most eps short of where it is heading.  Measured over the five cases:
    4/2048 pixel at worst on an axis (5/2048 as |ex| + |ey|), 29 iterations at most in total."""
    assert len(POINTS) == 35
    worst = its = 0
    for (x, y), (res, _) in zip(POINTS, scene_run(sx, sy, n_levels, radius)):
        assert res[0] == tr.TRACKED, (x, y, res)
        worst = max(worst, abs(res[1] - (x + sx) * 2048), abs(res[2] - (y + sy) * 2048))
        its = max(its, res[4])
    print(f"shift ({sx}, {sy}): worst {worst}/2048 px, {its} iterations at most")
    assert worst <= EPS


@pytest.mark.parametrize("sx,sy,n_levels,radius", CASES)
def test_restatement_against_float_lk(sx, sy, n_levels, radius):
    """The restatement and the float64 formulation follow every point to the same place.  Both
    stop within one step of at most eps of the common fixed point, on either side of it: 2 eps
    between them.  The quantisation (positions to 1/2048 pixel, samples to 1/32 grey level) moved
    the restatement's fixed point by 4/2048 pixel at most in the accuracy runs; it is covered by
    the half eps added here.  Measured: 3.4/2048 pixel at worst."""
    worst = 0
    for (x, y), (res, flt) in zip(POINTS, scene_run(sx, sy, n_levels, radius)):
        assert res[0] == tr.TRACKED and flt is not None
        worst = max(worst, abs(res[1] - flt[0] * 2048), abs(res[2] - flt[1] * 2048))
        # and they take about as long: the stopping rules are the same
        assert abs(res[4] - flt[2]) <= 2 * n_levels
    print(f"shift ({sx}, {sy}): restatement against float64 {worst:.2f}/2048 px")
    assert worst <= 2.5 * EPS


@functools.lru_cache(maxsize=None)
def subpixel_run():
    big = big_scene()
    # content moves by (2.5, -1.25): a pixel of the moved frame shows the scene at (x - 2.5, y + 1.25)
    moved, _ = wr.warp(big, [1, 0, -2.5, 0, 1, 1.25, 0, 0, 1], 256, 192)
    a, b = big[24:168, 24:232], moved[24:168, 24:232]
    pa, pb = rs.pyramid(a, 3, 2, 1), rs.pyramid(b, 3, 2, 1)
    return [(tr.track_point(pa, pb, x * 2048, y * 2048, None, 5, 30, EPS, 1.0),
             float_lk(pa, pb, x, y, 5, 30, EPS, 1.0)) for x, y in POINTS]


def test_subpixel_shift():
    """A shift of (2.5, -1.25) pixels: the moved frame is interpolated and rounded to 8 bits, so
    the truth is no exact fixed point of either formulation.  The restatement stays within the
    float64 formulation's own worst error on the same case plus eps."""
    worst_q = worst_f = 0.0
    for (x, y), (res, flt) in zip(POINTS, subpixel_run()):
        assert res[0] == tr.TRACKED and flt is not None
        tx, ty = (x + 2.5) * 2048, (y - 1.25) * 2048
        worst_q = max(worst_q, abs(res[1] - tx), abs(res[2] - ty))
        worst_f = max(worst_f, abs(flt[0] * 2048 - tx), abs(flt[1] * 2048 - ty))
    print(f"sub-pixel shift: restatement {worst_q:.1f}/2048 px, float64 {worst_f:.1f}/2048 px")
    assert worst_q <= worst_f + EPS


# ---- inputs that take the five sums near their ceilings -------------------------------------------
#
# The device tests of tests/test_gpu_track_instances.py run these inputs through the kernel, whose
# wave reduction splits an int64 partial sum into two ints and relies on |sum| < 2^44.  What is
# asserted here are conditions on the inputs (through the restatement's trace), so that those
# device runs keep reaching the magnitudes they are there for; they are no tolerance on anything.

CEILING_RADII = (8, 13, 15)
CEILING_VALUES = dict(max_iters=30, eps=EPS, min_eig=1.0)
SUM_LIMIT = 1 << 44                      # the kernel's bound; analytically 961 * 130560^2 = 2^43.9


@functools.lru_cache(maxsize=None)
def ceiling_frames(kind):
    """(prev, next), 64 x 80, of 2 x 2 blocks of 0 and 255: "shifted" moves the content by (1, 0),
    "inverted" is 255 - prev."""
    cells = np.random.default_rng(3).integers(0, 2, (60, 60)) * 255
    big = np.repeat(np.repeat(cells, 2, 0), 2, 1)[:112, :112].astype(np.uint8)
    prev = big[16:80, 16:96]
    nxt = {"shifted": big[16:80, 15:95], "inverted": 255 - prev}[kind]
    frames = np.stack([prev, nxt])
    frames.setflags(write=False)
    return frames


def ceiling_points(start):
    """The 3 x 3 grid of the 80 x 64 frame, 10 pixels inside: pixels ("pixel") or Q11 positions
    (777, 1234) / 2048 pixel further ("q11")."""
    pts = np.array([(x, y) for y in (10, 31, 53) for x in (10, 39, 69)], dtype=np.int64)
    return pts if start == "pixel" else pts * 2048 + (777, 1234)


@functools.lru_cache(maxsize=None)
def ceiling_run(kind, start, radius):
    """The restatement on every point: [(result, trace)] (one level, CEILING_VALUES)."""
    prev, nxt = ceiling_frames(kind)
    out = []
    for x, y in ceiling_points(start) * (2048 if start == "pixel" else 1):
        trace = []
        res = tr.track_point([prev], [nxt], x, y, None, radius, trace=trace, **CEILING_VALUES)
        out.append((res, trace))
    return out


def ceiling_sums(kind, start, radius):
    """(every A, every b) over the points, as flat lists of Python integers."""
    runs = ceiling_run(kind, start, radius)
    return ([a for _, trace in runs for lv in trace for a in lv["A"]],
            [b for _, trace in runs for lv in trace for pair in lv["b"] for b in pair])


@pytest.mark.parametrize("radius", CEILING_RADII)
@pytest.mark.parametrize("start", ["pixel", "q11"])
@pytest.mark.parametrize("kind", ["shifted", "inverted"])
def test_ceiling_inputs_stay_tracked_and_below_the_bound(kind, start, radius):
    """Every point runs through all its iterations to TRACKED (no early loss that would cut the
    sums short), and every sum, the residual included, is below the kernel's 2^44."""
    runs = ceiling_run(kind, start, radius)
    assert len(runs) == 9 and all(res[0] == tr.TRACKED for res, _ in runs)
    A, b = ceiling_sums(kind, start, radius)
    assert max(map(abs, A + b + [res[3] for res, _ in runs])) < SUM_LIMIT
    if kind == "inverted":               # no fixed point: the iteration limit ends the level
        assert max(res[4] for res, _ in runs) == 30


def test_ceiling_inputs_reach_the_magnitudes():
    A, _ = ceiling_sums("shifted", "pixel", 15)
    print(f"shifted, pixel starts, r = 15: max |A| = 2^{np.log2(max(map(abs, A))):.2f}")
    assert max(map(abs, A)) >= 1 << 42
    _, b = ceiling_sums("shifted", "q11", 15)
    print(f"shifted, Q11 starts, r = 15: b from -2^{np.log2(-min(b)):.2f} to 2^{np.log2(max(b)):.2f}")
    assert min(b) <= -(1 << 34) and max(b) >= 1 << 34             # both signs through the split
    _, b = ceiling_sums("inverted", "pixel", 15)
    print(f"inverted, pixel starts, r = 15: max |b| = 2^{np.log2(max(map(abs, b))):.2f}")
    assert max(map(abs, b)) >= 1 << 37


# ---- argument checks before any device call --------------------------------------------------

def test_exports_and_constants():
    names = {"fdf_track_device", "fdf_track_frames", "fdf_track_map_position",
             "fdf_track_map_displacement"}
    assert names <= set(_native.EXPORTED_SYMBOLS)
    assert {"track_device", "track_array", "track_map_position", "track_map_displacement",
            "TrackResult", "TRACK_REASONS"} <= set(fast_hip.__all__)
    lib = _native.load()
    for name in names:
        assert hasattr(lib, name)
    assert (_native.FDF_COORDS_U32, _native.FDF_COORDS_F32, _native.FDF_COORDS_Q11) == (0, 1, 2)
    assert (tr.COORDS_U32, tr.COORDS_Q11) == (_native.FDF_COORDS_U32, _native.FDF_COORDS_Q11)
    assert lib.fdf_abi_version() == 6
    assert len(fast_hip.TRACK_REASONS) == 5


def test_c_entries_reject_a_null_context_before_any_device_call():
    lib = _native.load()
    p = ctypes.c_void_p(4096)                            # never dereferenced: no context
    levels = (_native.FdfPyramidLevel * 1)()
    levels[0].width, levels[0].height = 8, 8
    assert lib.fdf_track_device(None, p, None, 0, p, None, 0, 1, 64, levels, 1, p, 0, 4, p, None,
                                None, 3, 10, 20, 1.0, p, None, p, None, None, None, None) == A
    assert lib.fdf_track_frames(None, p, p, 8, 8, 8, p, 0, 1, None, 1, 2, 1, 3, 10, 20, 1.0, p, None,
                                p, None, None) == A


def test_wrapper_argument_checks():
    import torch

    frames = torch.zeros((3, 24, 32), dtype=torch.uint8)
    plan = fast_hip.pyramid_plan((24, 32), 1, (2, 1), 3)
    side = (frames, None, plan)
    pts = torch.zeros((5, 2), dtype=torch.int32)
    offs = torch.tensor([0, 2, 5], dtype=torch.int64)
    q11 = torch.zeros((5, 2), dtype=torch.int32)
    status = torch.zeros(5, dtype=torch.uint8)
    good = dict(prev=side, next=side, points=pts, offsets=offs, next_q11=q11, status=status,
                prev_first=0, next_first=1)
    plan2 = fast_hip.pyramid_plan((24, 32), 2, (2, 1), 3)
    for bad in (dict(radius=0), dict(radius=16), dict(max_iters=0), dict(max_iters=65),
                dict(eps=-1), dict(min_eig=-0.5), dict(min_eig=float("nan")),
                dict(min_eig=float("inf")), dict(coords="f32"), dict(coords=2),
                dict(next_first=2), dict(n_frames=3), dict(prev_first=-1),
                dict(offsets=offs[:2]), dict(offsets=offs.to(torch.int32)),
                dict(points=pts.to(torch.float32)), dict(points=pts[:, :1]),
                dict(next_q11=q11[:4]), dict(status=status[:4]), dict(status=status.to(torch.int32)),
                dict(keep=torch.zeros(4, dtype=torch.uint8)),
                dict(guess=torch.zeros((4, 2), dtype=torch.int32)),
                dict(next_xy=torch.zeros((5, 2), dtype=torch.float64)),
                dict(err=torch.zeros(5, dtype=torch.float32)),
                dict(info=torch.zeros(5, dtype=torch.int64)),
                dict(matches=torch.zeros((5, 3), dtype=torch.int32)),
                dict(next=(torch.zeros((3, 24, 30), dtype=torch.uint8), None, plan)),
                dict(next=(frames, None, plan2)),                  # two levels need a buffer
                dict(next=(torch.zeros((3, 25, 32), dtype=torch.uint8)[:, :24], None, plan))):
        with pytest.raises(ValueError):
            fast_hip.track_device(**{**good, **bad})
    with pytest.raises(TypeError):
        fast_hip.track_device(**{**good, "prev": frames})
    # every check passed: the call gets as far as the device check
    for ok in (dict(), dict(coords="q11"), dict(n_frames=1), dict(eps=0, max_iters=64, radius=15),
               dict(keep=torch.ones(5, dtype=torch.uint8), guess=torch.zeros((5, 2), dtype=torch.int32),
                    next_xy=torch.zeros((5, 2)), err=torch.zeros(5, dtype=torch.int32),
                    info=torch.zeros(5, dtype=torch.int32),
                    matches=torch.zeros((5, 2), dtype=torch.int32))):
        with pytest.raises(ValueError, match="CUDA"):
            fast_hip.track_device(**{**good, **ok})

    img = np.zeros((24, 32), dtype=np.uint8)
    pts = np.array([[3, 4]])
    for bad in (dict(radius=0), dict(max_iters=100), dict(min_eig=-1), dict(coords="pixels"),
                dict(guess=np.zeros((2, 2), np.int32))):
        with pytest.raises(ValueError):
            fast_hip.track_array(img, img, pts, **bad)
    with pytest.raises(ValueError):
        fast_hip.track_array(img, img[:20], pts)
    with pytest.raises(TypeError):
        fast_hip.track_array(img, img, np.zeros((1, 2), np.float32))
    with pytest.raises(TypeError):
        fast_hip.track_array(img.astype(np.float32), img, pts)
