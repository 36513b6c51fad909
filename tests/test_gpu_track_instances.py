"""The tracker's kernel where tests/test_gpu_track.py does not take it: every one of the twelve
window-size instances (radius 1..15), sums next to the bound the wave reduction relies on, levels
of one or two pixels a side, and coordinates whose 32-bit product with 2048 wraps.  Every call goes
through test_gpu_track.run_track: all six outputs bit for bit against tests/_track_reference.py,
no gap byte changed, rows at or past `cap` untouched, inputs intact."""
import functools

import numpy as np
import pytest

import _track_reference as tr
from test_gpu_track import grid_points, moved, reasons, run_track, texture
from test_track import CEILING_RADII, CEILING_VALUES, ceiling_frames, ceiling_points
from feature_detector_fast_amd import fast_hip

pytestmark = pytest.mark.gpu


def reason_counts(want):
    return np.bincount(want["info"][want["written"]] & 0xff, minlength=5)


# ---- 1: every instance ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def instance_scene():
    """The scene of test_radii with 18 Q11 points: 12 of the grid at random sub-pixel offsets
    (every bilinear weight non-trivial) and 6 pixel-aligned ones on the corners and borders."""
    frames = moved(texture(1, 112, 96), 80, 64, [(2, -1)])
    frames.setflags(write=False)
    inner = grid_points(80, 64, 4, 3, 6) * 2048 + np.random.default_rng(9).integers(0, 2048, (12, 2))
    border = np.array([(0, 0), (79, 63), (79, 0), (0, 63), (40, 0), (0, 30)]) * 2048
    return frames, np.concatenate([inner, border])


@pytest.mark.parametrize("radius", range(1, 16))
def test_every_instance(radius):
    """r = 1..15 are 9..961 window pixels and the slot counts 1, 1, 1, 2, 2, 3, 4, 5, 6, 7, 9,
    10, 12, 14, 16: all twelve instances, each with its own idle lanes in the last slot and 1 to 5
    passes of the template fill.  18 points are several passes of every wave; lost and tracked
    points share a workgroup."""
    frames, pts = instance_scene()
    n = len(pts)
    one = dict(next_first=1, n_levels=2, radius=radius, min_eig=0.5, coords="q11")
    want = run_track(frames, None, pts, [0, n], **one)
    counts = reason_counts(want)
    assert counts[tr.TRACKED] >= 11 and counts[tr.LOST_FRAME] >= 4, counts
    # a guess per point: the truth and up to a pixel and a half of noise
    guess = pts + np.array((2, -1)) * 2048 + np.random.default_rng(5).integers(-3000, 3000, (n, 2))
    want = run_track(frames, None, pts, [0, n], guess=guess, **one)
    assert {tr.TRACKED, tr.SKIPPED} <= reasons(want)
    # two frames of the call (the second one backwards) with 1 and 5 points
    some = np.concatenate([pts[:1], pts[9:14]])
    want = run_track(frames, frames[::-1], some, [0, 1, 6], **{**one, "next_first": 0})
    assert (want["status"][:1] == 1).all() and (want["status"][1:] == 1).any()


# ---- 2: sums near their ceilings -------------------------------------------------------------------

@pytest.mark.parametrize("radius", CEILING_RADII)
@pytest.mark.parametrize("kind", ["shifted", "inverted"])
def test_sums_near_their_ceilings(kind, radius):
    """Frames of 2 x 2 blocks of 0 and 255.  tests/test_track.py asserts on the restatement what
    these inputs reach: A above 2^42, b of both signs above 2^34 ("shifted"), |b| above 2^37 and
    the largest residuals ("inverted", where every level runs to the iteration limit), all below
    the 2^44 that the kernel's split wave sum is exact for."""
    frames = ceiling_frames(kind)
    if kind == "shifted":
        big = np.repeat(np.repeat(np.random.default_rng(3).integers(0, 2, (60, 60)) * 255, 2, 0),
                        2, 1)[:112, :112].astype(np.uint8)
        assert np.array_equal(frames, moved(big, 80, 64, [(1, 0)]))
    assert np.array_equal(ceiling_points("pixel"), grid_points(80, 64, 3, 3, 10))
    for start, coords in (("pixel", "u32"), ("q11", "q11")):
        want = run_track(frames, None, ceiling_points(start), [0, 9], next_first=1, n_levels=1,
                         radius=radius, coords=coords, **CEILING_VALUES)
        assert want["status"].all()
        if kind == "inverted":                          # no fixed point: the iteration limit
            assert (want["info"] >> 8).max() == 30


# ---- 3: levels down to one pixel -------------------------------------------------------------------

T, E, F = tr.TRACKED, tr.LOST_EIGEN, tr.LOST_FRAME
# (w, h), levels, every k-th pixel is a point, the last level, the reasons at r = 1, 6, 15
SMALL = [((9, 5), 5, 3, (1, 1), ({T, F}, {F}, {F})),
         ((33, 2), 3, 5, (9, 1), ({T, F}, {T, F}, {T, F})),
         ((2, 40), 4, 6, (1, 5), ({T, F}, {T, F}, {F})),
         ((64, 1), 2, 5, (32, 1), ({E}, {E}, {E})),
         ((1, 1), 1, 1, (1, 1), ({E}, {E}, {E})),
         ((9, 5), 8, 3, (1, 1), ({T, F}, {F}, {F}))]          # the 1 x 1 level four times
SMALL_RADII = (1, 6, 15)


@pytest.mark.parametrize("radius", SMALL_RADII)
@pytest.mark.parametrize("size,n_levels,k,last,expect", SMALL,
                         ids=[f"{w}x{h}-{n}" for (w, h), n, *_ in SMALL])
def test_levels_down_to_one_pixel(size, n_levels, k, last, expect, radius):
    """2:1 pyramids of frames a few pixels a side: both taps of a sample clamp onto one pixel, only
    position 0 is inside an axis of length 1 and the level's buffer resource is as small as one
    byte.  The reason sets are the restatement's, written down so that the cases keep their
    meaning."""
    w, h = size
    plan = fast_hip.pyramid_plan((h, w), n_levels, (2, 1), 2)
    assert (plan.levels[-1].width, plan.levels[-1].height) == last
    frames = moved(texture(5, w + 32, h + 32), w, h, [(1, 0)])
    at = np.arange(0, w * h, k)
    pts = np.stack([at % w, at // w], axis=1)
    assert len(pts) == 1 or 13 <= len(pts) <= 15
    want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=n_levels, scale=(2, 1),
                     radius=radius, min_eig=0.0)
    assert want["written"].all() and reasons(want) == expect[SMALL_RADII.index(radius)]


# ---- 4: coordinates that would wrap -----------------------------------------------------------------

def wrap_scene():
    frames = moved(texture(21, 100, 84), 64, 48, [(1, 1)])
    return frames, grid_points(64, 48, 4, 3, 8)


def test_u32_coordinates_that_wrap():
    """Pixel coordinates whose product with 2048 is small modulo 2^32 (2^21 * 2048 = 2^32,
    (2^21 + 5) * 2048 = 10240 mod 2^32) or negative as an int: all outside the frame, so skipped
    before any frame byte is read.  x = 63 is the last column."""
    frames, ordinary = wrap_scene()
    values = [2 ** 20, 2 ** 21, 2 ** 21 + 5, 2 ** 31, 2 ** 32 - 1, 63, 64]
    odd = np.array([(v, 20) for v in values] + [(20, v) for v in values] + [(v, v) for v in values])
    pts = np.empty((2 * len(odd), 2), np.int64)         # skipped and tracked waves side by side
    pts[0::2] = odd
    pts[1::2] = ordinary[np.arange(len(odd)) % len(ordinary)]
    want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=2, radius=4,
                     min_eig=0.5)
    info = (want["info"] & 0xff)[0::2]
    inside = (odd[:, 0] <= 63) & (odd[:, 1] <= 47)
    assert inside.tolist() == [v == 63 for v in values] + [False] * (2 * len(values))
    assert (info[~inside] == tr.SKIPPED).all() and (info[inside] != tr.SKIPPED).all()
    skipped = want["info"] == tr.SKIPPED                # no iteration either
    assert skipped.sum() == len(odd) - 1
    assert (want["q11"][skipped] == -1).all() and (want["err"][skipped] == tr.NO_ERR).all()
    assert (want["status"][1::2] == 1).all()


def test_q11_coordinates_at_the_ends_of_int32():
    frames, ordinary = wrap_scene()
    values = [-2 ** 31, 2 ** 31 - 1, -1, 63 * 2048, 63 * 2048 + 1]
    at = 20 * 2048 + 300
    odd = np.array([(v, at) for v in values] + [(at, v) for v in values + [47 * 2048, 47 * 2048 + 1]] +
                   [(v, v) for v in values])
    inside = (odd[:, 0] >= 0) & (odd[:, 0] <= 63 * 2048) & (odd[:, 1] >= 0) & (odd[:, 1] <= 47 * 2048)
    assert inside.sum() == 2                            # (63 * 2048, at) and (at, 47 * 2048)
    good = ordinary[np.arange(len(odd)) % len(ordinary)] * 2048 + 100
    pts = np.empty((2 * len(odd), 2), np.int64)
    pts[0::2] = odd
    pts[1::2] = good
    one = dict(next_first=1, n_levels=2, radius=4, min_eig=0.5, coords="q11")
    want = run_track(frames, None, pts, [0, len(pts)], **one)
    info = (want["info"] & 0xff)[0::2]
    assert (info[~inside] == tr.SKIPPED).all() and (info[inside] != tr.SKIPPED).all()
    assert (want["q11"][0::2][~inside] == -1).all() and (want["err"][0::2][~inside] == tr.NO_ERR).all()
    assert (want["status"][1::2] == 1).all()
    # the same values as guesses of points that are inside
    start = np.concatenate([good, good])
    guess = start + np.array((1, 1)) * 2048
    guess[0::2] = odd
    want = run_track(frames, None, start, [0, len(start)], guess=guess, **one)
    info = (want["info"] & 0xff)[0::2]
    assert (info[~inside] == tr.SKIPPED).all() and (info[inside] != tr.SKIPPED).all()
    assert (want["status"][1::2] == 1).all()
