"""Pyramidal Lucas-Kanade tracking on the device (fdf_track_device, fdf_track_frames) against the
numpy restatement of include/fdf.h's rules in tests/_track_reference.py.  Every comparison is bit
for bit; every run also proves that no gap byte between frames or levels changed, that output
entries at or past min(offs[n], cap) keep their fill and that every input is intact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _brief_reference as br
import _ransac_reference as rr
import _resize_reference as rs
import _track_reference as tr
from feature_detector_fast_amd import FdfError, _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 0xEE
TAIL = 3                                        # rows past `cap` in every output
OUTPUTS = ("q11", "f32", "status", "err", "info", "matches")


def texture(seed, w, h):
    """A smooth random frame: a coarse random grid resized and box-smoothed (the library's rules)."""
    small = np.random.default_rng(seed).integers(0, 256, (max(h // 8, 2), max(w // 8, 2)))
    return br.smooth(rs.resize(small.astype(np.uint8), w, h))


def moved(big, w, h, shifts, margin=16):
    """Crops of `big` whose content moves by each of `shifts` = [(sx, sy)] from the first crop."""
    return np.stack([big[margin - sy:margin - sy + h, margin - sx:margin - sx + w]
                     for sx, sy in [(0, 0)] + list(shifts)])


def strided(torch, f, h, w, stride, lead):
    """f frames of h x w on the device `stride` bytes apart, `lead` bytes into an allocation
    filled with GAP -> (the whole allocation, the (F, H, W) view)."""
    flat = torch.full((lead + f * stride + 64,), GAP, dtype=torch.uint8, device="cuda")
    return flat, torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)


class Side:
    """One set of frames on the device with its pyramid, and what it must still hold afterwards."""

    def __init__(self, torch, frames, n_levels, scale, stride, lead):
        f, h, w = frames.shape
        self.flat, self.view = strided(torch, f, h, w, h * w if stride is None else stride, lead)
        self.view.copy_(torch.from_numpy(np.array(frames)).cuda())
        self.pyramid = fast_hip.Pyramid(self.view, n_levels, scale)
        torch.cuda.synchronize()
        self.kept = (self.flat.clone(), self.pyramid.buffer.clone())

    def intact(self):
        return bool((self.flat == self.kept[0]).all() and (self.pyramid.buffer == self.kept[1]).all())


def gap_tensor(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(GAP)
    return t


def run_track(prev, nxt, points, offs, cap=None, prev_first=0, next_first=0, n_frames=None,
              n_levels=1, scale=(2, 1), coords="u32", keep=None, guess=None, stride=None, lead=0,
              outputs=OUTPUTS, **values):
    """fdf_track_device on uploaded frames (`nxt` None: one batch on both sides) against the
    restatement, bit for bit, with the checks of the module's docstring.  Returns the reference's
    arrays."""
    import torch

    points = np.asarray(points).reshape(-1, 2)
    cap = len(points) if cap is None else cap
    a = Side(torch, prev, n_levels, scale, stride, lead)
    b = a if nxt is None else Side(torch, nxt, n_levels, scale, stride, lead)
    n = min(len(a.view) - prev_first, len(b.view) - next_first) if n_frames is None else n_frames
    d_pts = torch.from_numpy(points.astype(np.int32 if coords == "q11" else np.uint32)
                             .view(np.int32)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.uint8)).cuda()
    d_guess = None if guess is None else torch.from_numpy(np.asarray(guess, dtype=np.int32)).cuda()
    inputs = [t for t in (d_pts, d_offs, d_keep, d_guess) if t is not None]
    kept = [t.clone() for t in inputs]
    rows = cap + TAIL
    out = {"q11": gap_tensor(torch, (rows, 2), torch.int32),
           "f32": gap_tensor(torch, (rows, 2), torch.float32),
           "status": gap_tensor(torch, (rows,), torch.uint8),
           "err": gap_tensor(torch, (rows,), torch.int32),
           "info": gap_tensor(torch, (rows,), torch.int32),
           "matches": gap_tensor(torch, (rows, 2), torch.int32)}
    given = {k: (v if k in outputs or k in ("q11", "status") else None) for k, v in out.items()}
    # the tensors hold `rows` rows, the call is told of `cap`: slices share the memory
    fast_hip.track_device(a.pyramid, b.pyramid, d_pts[:cap], d_offs, given["q11"][:cap],
                          given["status"][:cap], prev_first=prev_first, next_first=next_first,
                          n_frames=n_frames, coords=coords,
                          keep=None if d_keep is None else d_keep[:cap],
                          guess=None if d_guess is None else d_guess[:cap],
                          next_xy=None if given["f32"] is None else given["f32"][:cap],
                          err=None if given["err"] is None else given["err"][:cap],
                          info=None if given["info"] is None else given["info"][:cap],
                          matches=None if given["matches"] is None else given["matches"][:cap],
                          **values)
    torch.cuda.synchronize()
    assert a.intact() and b.intact()
    for t, k in zip(inputs, kept):
        assert torch.equal(t, k)

    levels = lambda frames: [rs.pyramid(fr, n_levels, *scale) for fr in frames]
    pa = levels(prev)
    pb = pa if nxt is None else levels(nxt)
    want = tr.track(pa[prev_first:prev_first + n], pb[next_first:next_first + n], points, offs, cap,
                    coords=tr.COORDS_Q11 if coords == "q11" else tr.COORDS_U32, keep=keep,
                    guess=guess, **values)
    written = np.concatenate([want["written"], np.zeros(TAIL, bool)])
    for name in OUTPUTS:
        got = out[name].cpu().numpy()
        raw = got.view(np.uint8).reshape(rows, -1)
        if given[name] is None:
            assert (raw == GAP).all(), name
            continue
        assert (raw[~written] == GAP).all(), name
        exp = want[name].view(got.dtype) if name != "f32" else want[name]
        assert got[:cap][written[:cap]].tobytes() == exp[written[:cap]].tobytes(), name
    return want


def grid_points(w, h, nx, ny, margin):
    xs = np.linspace(margin, w - 1 - margin, nx).astype(np.int64)
    ys = np.linspace(margin, h - 1 - margin, ny).astype(np.int64)
    return np.array([(x, y) for y in ys for x in xs])


def reasons(want):
    return set((want["info"][want["written"]] & 0xff).tolist())


# ---- 1: window sizes, levels and ratios ----------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 4, 7, 15])
def test_radii(radius):
    """9, 81, 225 and 961 window pixels: below a wave, no multiple of 64, the register maximum."""
    frames = moved(texture(1, 112, 96), 80, 64, [(2, -1)])
    pts = grid_points(80, 64, 4, 3, 6)
    want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=2, radius=radius,
                     min_eig=0.5)
    assert tr.TRACKED in reasons(want)


@pytest.mark.parametrize("scale", [(2, 1), (6, 5)])
@pytest.mark.parametrize("n_levels", [1, 2, 4])
def test_levels_and_ratios(n_levels, scale):
    frames = moved(texture(2, 104, 88), 73, 57, [(3, 2)])           # odd sizes
    pts = grid_points(73, 57, 4, 4, 5)
    want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=n_levels, scale=scale,
                     radius=5, min_eig=0.5)
    assert want["status"].sum() >= len(pts) // 2


def test_big_scene_four_levels():
    """The 208 x 144 scene of the CPU accuracy test, shift (12, 9), 4 levels, r = 7: every point
    follows the shift."""
    small = np.random.default_rng(7).integers(0, 256, (24, 32)).astype(np.uint8)
    big = br.smooth(rs.resize(small, 256, 192))
    frames = np.stack([big[24:168, 24:232], big[15:159, 12:220]])
    pts = np.array([(x, y) for y in range(40, 130, 18) for x in range(40, 200, 23)])
    want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=4, radius=7,
                     min_eig=1.0)
    assert want["status"].all()
    assert np.abs(want["q11"] - (pts + (12, 9)) * 2048).max() <= 20


# ---- 2: frames: first indices, strides, offsets, separate buffers -----------------------------------

def test_one_batch_frame_to_frame_with_gaps():
    frames = moved(texture(3, 104, 88), 70, 50, [(1, 1), (3, 0), (2, -2)])
    pts = grid_points(70, 50, 3, 3, 8)
    all_pts = np.concatenate([pts, pts + 1, pts + 2])
    offs = [0, 9, 18, 27]
    run_track(frames, None, all_pts, offs, prev_first=0, next_first=1, n_levels=3, radius=4,
              min_eig=0.5, stride=70 * 50 + 37, lead=3)
    # backwards, and a sub-range of the batch
    run_track(frames, None, all_pts[:18], offs[:3], prev_first=2, next_first=1, n_frames=2,
              n_levels=2, radius=4, min_eig=0.5, stride=70 * 50 + 1, lead=1)


def test_two_separate_buffers():
    frames = moved(texture(4, 104, 88), 64, 48, [(2, 1), (-1, 2), (0, -3)])
    pts = grid_points(64, 48, 3, 3, 8)
    all_pts = np.concatenate([pts, pts + 1])
    run_track(frames[:2], frames[2:], all_pts, [0, 9, 18], n_levels=2, radius=4, min_eig=0.5,
              stride=64 * 48 + 5, lead=7)
    run_track(frames[:1], frames[1:2], pts, [0, 9], n_levels=1, radius=4, min_eig=0.5)


# ---- 3: point lists ------------------------------------------------------------------------------------

def test_borders_and_corners():
    """Points on every border and corner: the window and the template's rim replicate the border."""
    w, h = 64, 48
    frames = moved(texture(5, 100, 84), w, h, [(1, -1)])
    xs, ys = (0, 1, 31, w - 2, w - 1), (0, 1, 23, h - 2, h - 1)
    pts = np.array([(x, y) for y in ys for x in xs])
    for radius in (2, 7):
        want = run_track(frames, None, pts, [0, len(pts)], next_first=1, n_levels=2, radius=radius,
                         min_eig=0.0)
        assert tr.TRACKED in reasons(want)


def test_point_counts_and_an_empty_frame():
    """0, 1, 3, 5 and 257 points per frame (257: more than one workgroup pass and, with the
    chunks, more than one workgroup), the empty frame in the middle."""
    frames = moved(texture(6, 104, 88), 64, 48, [(1, 0), (1, 1), (0, 1), (2, 1), (2, 2)])
    counts = [1, 3, 0, 5, 257]
    rng = np.random.default_rng(60)
    pts = np.stack([rng.integers(0, 64, sum(counts)), rng.integers(0, 48, sum(counts))], axis=1)
    offs = np.concatenate([[0], np.cumsum(counts)])
    want = run_track(frames, None, pts, offs, next_first=1, n_levels=2, radius=3, min_eig=0.5,
                     max_iters=10)
    assert want["written"].all()
    # no points at all, and offsets that say so with a capacity of rows nobody owns
    run_track(frames[:3], None, pts[:4], [0, 0, 0], next_first=1, radius=3)
    run_track(frames[:3], None, np.zeros((0, 2), np.int64), [0, 0, 0], next_first=1, radius=3)


def test_offsets_past_the_capacity():
    frames = moved(texture(7, 104, 88), 64, 48, [(1, 0), (1, 1)])
    pts = grid_points(64, 48, 4, 3, 8)
    all_pts = np.concatenate([pts, pts])
    want = run_track(frames, None, all_pts, [0, 12, 24], cap=17, next_first=1, n_levels=2, radius=3,
                     min_eig=0.5)
    assert want["written"].sum() == 17
    want = run_track(frames, None, all_pts, [0, 20, 40], cap=17, next_first=1, radius=3, min_eig=0.5)
    assert want["written"].sum() == 17                 # the second frame owns nothing


def test_keep_bytes():
    frames = moved(texture(8, 104, 88), 64, 48, [(2, 1)])
    pts = grid_points(64, 48, 4, 4, 8)
    keep = (np.arange(16) % 3 != 1).astype(np.uint8) * np.array([1, 7, 255] * 5 + [1], np.uint8)
    want = run_track(frames, None, pts, [0, 16], next_first=1, n_levels=2, radius=4, min_eig=0.5,
                     keep=keep)
    info = want["info"] & 0xff
    assert (info[keep == 0] == tr.SKIPPED).all() and (info[keep != 0] != tr.SKIPPED).all()


def test_q11_chained_over_three_frames():
    """f -> f + 1 -> f + 2 at sub-pixel positions: the second call reads the first one's next_q11,
    lost points ((-1, -1)) included, and equals the restatement chained the same way."""
    big = texture(9, 112, 96)
    frames = moved(big, 72, 56, [(2, 1), (3, 3)])
    pts = np.concatenate([grid_points(72, 56, 4, 3, 6), [[0, 0], [71, 55], [70, 2]]])
    n = len(pts)
    first = run_track(frames, None, pts, [0, n], prev_first=0, next_first=1, n_frames=1, n_levels=2,
                      radius=4, min_eig=0.5)
    assert (first["status"] == 0).any() and (first["status"] == 1).any()
    second = run_track(frames, None, first["q11"], [0, n], prev_first=1, next_first=2, n_frames=1,
                       n_levels=2, radius=4, min_eig=0.5, coords="q11")
    lost = first["status"] == 0
    assert ((second["info"] & 0xff)[lost] == tr.SKIPPED).all()
    assert (second["q11"][lost] == -1).all() and second["status"][~lost].any()
    assert (second["q11"][second["status"] == 1] & 2047).any()          # sub-pixel positions


def test_guesses():
    frames = moved(texture(10, 112, 96), 72, 56, [(9, -7)])
    pts = grid_points(72, 56, 4, 3, 14)
    n = len(pts)
    guess = (pts + (9, -7)) * 2048 + np.random.default_rng(5).integers(-3000, 3000, (n, 2))
    guess[1] = (-1, 5 * 2048)                       # outside the frame: skipped
    guess[2] = (71 * 2048 + 1, 5 * 2048)
    guess[3] = (71 * 2048, 55 * 2048)               # the far corner is inside
    for n_levels in (1, 3):
        want = run_track(frames, None, pts, [0, n], next_first=1, n_levels=n_levels, radius=5,
                         min_eig=0.5, guess=guess)
        info = want["info"] & 0xff
        assert info[1] == tr.SKIPPED and info[2] == tr.SKIPPED and info[3] != tr.SKIPPED
        assert (want["status"][4:] == 1).all()


# ---- 4: every reason, the iteration limits, optional outputs -------------------------------------------

def test_every_reason():
    w, h = 64, 48
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    tex = moved(texture(11, 100, 84), w, h, [(3, 1)])
    # reason 2: a constant patch inside a textured frame
    a, b = tex[0].copy(), tex[1].copy()
    a[10:30, 10:30] = 99
    # reason 3: content that moves off the edge (a guess next to it, the shift goes further)
    pts = np.array([(20, 20), (50, 38), (w - 2, 24), (70, 3)])
    guess = pts * 2048
    guess[2] = ((w - 1) * 2048, 24 * 2048)
    want = run_track(np.stack([a, b]), None, pts, [0, 4], next_first=1, radius=4, min_eig=0.5,
                     guess=guess)
    assert (want["info"] & 0xff).tolist() == [tr.LOST_EIGEN, tr.TRACKED, tr.LOST_FRAME, tr.SKIPPED]
    # reason 4: a near-singular window (one grey level of vertical structure) with min_eig = 0
    # against a frame with a strong vertical step; the restatement confirms it on the CPU first
    ramp = np.broadcast_to((4 * x).clip(0, 255), (h, w)).astype(np.uint8).copy()
    ramp[24, 30] += 1
    step = (np.where(y <= 24, 0, 255) * np.ones((1, w))).astype(np.uint8)
    for radius in (2, 4):
        res = tr.track_point([ramp], [step], 30 * 2048, 24 * 2048, None, radius, 30, 20, 0.0)
        assert res == (tr.LOST_STEP, -1, -1, tr.NO_ERR, 1)
        want = run_track(np.stack([ramp, step]), None, [(30, 24), (20, 10)], [0, 2], next_first=1,
                         radius=radius, min_eig=0.0)
        assert (want["info"] & 0xff)[0] == tr.LOST_STEP
    # a constant frame is lost with reason 2 even at min_eig = 0
    flat = np.full((2, h, w), 7, np.uint8)
    want = run_track(flat, None, [(30, 24)], [0, 1], next_first=1, n_levels=2, radius=4, min_eig=0.0)
    assert want["info"].tolist() == [tr.LOST_EIGEN]


@pytest.mark.parametrize("values", [dict(max_iters=1), dict(eps=0), dict(eps=0, max_iters=64),
                                    dict(eps=1 << 22), dict(max_iters=1, eps=0)])
def test_iteration_limits(values):
    frames = moved(texture(12, 104, 88), 64, 48, [(2, 2)])
    pts = grid_points(64, 48, 3, 3, 9)
    want = run_track(frames, None, pts, [0, 9], next_first=1, n_levels=2, radius=4, min_eig=0.5,
                     **values)
    iters = (want["info"] >> 8)[want["status"] == 1]
    if values.get("max_iters") == 1:
        assert (iters <= 2).all()
    if values == dict(eps=0, max_iters=64):
        assert iters.max() > 8


def test_optional_outputs_null():
    frames = moved(texture(13, 104, 88), 64, 48, [(1, 2)])
    pts = grid_points(64, 48, 3, 3, 9)
    run_track(frames, None, pts, [0, 9], next_first=1, n_levels=2, radius=4, min_eig=0.5, outputs=())
    run_track(frames, None, pts, [0, 9], next_first=1, n_levels=2, radius=4, min_eig=0.5,
              outputs=("err", "matches"))


# ---- 5: into the estimator ---------------------------------------------------------------------------

def test_tracks_feed_ransac():
    """matches, status and the float32 positions go into ransac_device as they are (the query side
    as a float32 copy of the points): the affine model of a shifted scene is the translation."""
    import torch

    sx, sy = 5, -3
    frames = moved(texture(14, 168, 136), 128, 96, [(sx, sy)])
    pts = grid_points(128, 96, 6, 5, 12)
    n = len(pts)
    d = torch.from_numpy(frames.copy()).cuda()
    pyr = fast_hip.Pyramid(d, 3, (2, 1))
    d_pts = torch.from_numpy(pts.astype(np.int32)).cuda()
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    q11 = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    xy = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    fast_hip.track_device(pyr, pyr, d_pts, offs, q11, status, prev_first=0, next_first=1, radius=6,
                          min_eig=0.5, next_xy=xy, matches=matches)
    models = torch.zeros((1, 11), dtype=torch.float64, device="cuda")
    scratch = torch.empty(fast_hip.ransac_scratch_bytes(1, n, 64), dtype=torch.uint8, device="cuda")
    inliers = torch.zeros(n, dtype=torch.uint8, device="cuda")
    fast_hip.ransac_device(matches, offs, d_pts.to(torch.float32), xy, offs, models, scratch,
                           keep=status, inliers=inliers, model="affine", n_hyp=64, threshold=0.5,
                           seed=1)
    torch.cuda.synchronize()
    assert status.cpu().numpy().all()
    rec = fast_hip.unpack_models(models.cpu().numpy())[0]
    want = np.array([1, 0, sx, 0, 1, sy, 0, 0, 1], dtype=np.float64)
    assert np.abs(rec["h"] - want).max() < 0.02 and rec["n_inliers"] == n
    # and bit for bit what the restatement of the estimator makes of the restated tracks
    ref = tr.track([rs.pyramid(frames[0], 3, 2, 1)], [rs.pyramid(frames[1], 3, 2, 1)], pts, [0, n], n,
                   radius=6, min_eig=0.5)
    assert np.array_equal(xy.cpu().numpy(), ref["f32"])
    assert np.array_equal(matches.cpu().numpy().view(np.uint32), ref["matches"])


# ---- 6: the host entry, the C++ API, rejected calls ------------------------------------------------

def test_worked_example_through_track_frames():
    a, b = tr.worked_frames()
    pts = np.array([[14, 10]])
    one = dict(radius=3, max_iters=30, eps=20, min_eig=0.25)
    r = fast_hip.track_array(a, b, pts, n_levels=1, **one)
    assert r.q11.tolist() == [[32773, 22529]] and r.err.tolist() == [0]
    assert r.status.tolist() == [True] and r.reason.tolist() == [1] and r.iterations.tolist() == [4]
    assert r.xy.tolist() == [[np.float32(32773 / 2048), np.float32(22529 / 2048)]]
    r = fast_hip.track_array(a, b, pts, n_levels=1, **{**one, "max_iters": 1})
    assert r.q11.tolist() == [[33605, 23077]] and r.err.tolist() == [1789]
    r = fast_hip.track_array(a, b, pts, n_levels=1, **{**one, "min_eig": 1.0})
    assert r.reason.tolist() == [2] and r.q11.tolist() == [[-1, -1]] and r.err.tolist() == [tr.NO_ERR]
    assert r.xy.tolist() == [[-1.0, -1.0]] and r.status.tolist() == [False]
    r = fast_hip.track_array(a, b, pts, n_levels=2, **one)
    assert r.q11.tolist() == [[32773, 22530]] and r.err.tolist() == [0] and r.iterations.tolist() == [5]
    start = np.array([[29372, 21780]])
    r = fast_hip.track_array(a, b, start, n_levels=1, coords="q11", **one)
    assert r.q11.tolist() == [[33469, 23826]] and r.err.tolist() == [0]
    r = fast_hip.track_array(a, b, start, n_levels=2, coords="q11", **one)
    assert r.q11.tolist() == [[33468, 23826]] and r.err.tolist() == [2]
    flat = np.full((24, 32), 7, np.uint8)
    r = fast_hip.track_array(flat, flat, pts, n_levels=1, **{**one, "min_eig": 0.0})
    assert r.reason.tolist() == [2]


def test_track_array_against_the_restatement():
    frames = moved(texture(15, 120, 100), 83, 61, [(4, -3)])
    padded = np.full((2, 61, 90), GAP, np.uint8)
    padded[:, :, :83] = frames
    pts = np.concatenate([grid_points(83, 61, 5, 4, 4), [[90, 3], [3, 61]]])
    guess = pts * 2048 + 700
    for n_levels, scale, g in ((3, (2, 1), None), (2, (6, 5), guess), (1, (2, 1), None)):
        r = fast_hip.track_array(padded[0, :, :83], padded[1, :, :83], pts, n_levels=n_levels,
                                 scale=scale, radius=6, min_eig=0.5, guess=g)
        want = tr.track([rs.pyramid(frames[0], n_levels, *scale)],
                        [rs.pyramid(frames[1], n_levels, *scale)], pts, [0, len(pts)], len(pts),
                        guess=g, radius=6, min_eig=0.5)
        assert np.array_equal(r.q11, want["q11"]) and np.array_equal(r.xy, want["f32"])
        assert np.array_equal(r.status, want["status"] == 1) and np.array_equal(r.err, want["err"])
        assert np.array_equal(r.reason | r.iterations << 8, want["info"])
        assert r.reason[-2:].tolist() == [0, 0]
    empty = fast_hip.track_array(frames[0], frames[1], np.zeros((0, 2), np.int64))
    assert empty.q11.shape == (0, 2) and empty.status.shape == (0,)


def test_cpp_smoke_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_track")
    assert os.path.exists(exe), "run `make` first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout


def test_rejected_calls():
    """What fdf_track_device must reject, synchronously and with nothing launched: the outputs
    keep their fill."""
    import torch

    lib = _native.load()
    ctx = fast_hip.context(0).handle
    frames = torch.zeros((3, 24, 32), dtype=torch.uint8, device="cuda")
    pyr = fast_hip.Pyramid(frames, 2, (2, 1))
    plan = pyr.plan
    pts = torch.zeros((6, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda")
    q11 = gap_tensor(torch, (6, 2), torch.int32)
    status = gap_tensor(torch, (6,), torch.uint8)
    extra = gap_tensor(torch, (8, 2), torch.int32)
    fp, bp = frames.data_ptr(), pyr.buffer.data_ptr()

    def call(**kw):
        a = dict(prev=fp, prev_pyr=bp, prev_first=0, next=fp, next_pyr=bp, next_first=1, n_frames=2,
                 stride=24 * 32, levels=plan._c, n_levels=2, points=pts.data_ptr(), coords=0, cap=6,
                 offs=offs.data_ptr(), keep=None, guess=None, radius=4, max_iters=10, eps=20,
                 min_eig=1.0, q11=q11.data_ptr(), f32=None, status=status.data_ptr(), err=None,
                 info=None, matches=None)
        a.update(kw)
        return lib.fdf_track_device(ctx, *a.values(), None)

    A, S = _native.FDF_ERR_ARG, _native.FDF_ERR_SIZE
    odd = extra.data_ptr() + 4
    for kw in (dict(radius=0), dict(radius=16), dict(max_iters=0), dict(max_iters=65),
               dict(min_eig=-1.0), dict(min_eig=float("nan")), dict(min_eig=float("inf")),
               dict(coords=1), dict(coords=3), dict(n_frames=65536), dict(n_levels=0),
               dict(n_levels=33), dict(levels=None), dict(prev=None), dict(next=None),
               dict(prev_pyr=None), dict(next_pyr=None), dict(points=None), dict(offs=None),
               dict(q11=None), dict(status=None), dict(points=odd), dict(q11=odd), dict(guess=odd),
               dict(f32=odd), dict(matches=odd), dict(err=odd + 2), dict(info=odd + 1),
               dict(stride=24 * 32 - 1)):
        assert call(**kw) == A, kw
    bad = (_native.FdfPyramidLevel * 2)()
    for k in range(2):
        for name in ("width", "height", "frame_stride_bytes", "offset_bytes"):
            setattr(bad[k], name, getattr(plan._c[k], name))
    bad[1].frame_stride_bytes = 16 * 12 - 1
    assert call(levels=bad) == A
    bad[1].frame_stride_bytes = 16 * 12
    bad[1].width = 0
    assert call(levels=bad) == S
    bad[1].width = 65536
    assert call(levels=bad) == S
    bad[1].width, bad[1].height = 65535, 65535
    assert call(levels=bad) == S
    assert call(n_frames=0) == _native.FDF_OK
    assert call(n_frames=0, points=None, q11=None) == _native.FDF_OK
    torch.cuda.synchronize()
    for t in (q11, status, extra):
        assert (t.view(torch.uint8) == GAP).all()
    # a single addressed frame's stride is not looked at; one level needs no pyramid
    assert call(next_first=0, n_frames=1, stride=0, n_levels=1, prev_pyr=None, next_pyr=None) == 0
    torch.cuda.synchronize()
    # only the tracker takes Q11 coordinates: the estimator still rejects them
    scratch = torch.empty(fast_hip.ransac_scratch_bytes(2, 6, 16), dtype=torch.uint8, device="cuda")
    models = torch.zeros((2, 11), dtype=torch.float64, device="cuda")
    rc = lib.fdf_ransac_device(ctx, 2, extra.data_ptr(), None, 6, offs.data_ptr(), pts.data_ptr(),
                               pts.data_ptr(), 6, offs.data_ptr(), _native.FDF_COORDS_Q11, 0, 16, 3.0,
                               0, models.data_ptr(), None, scratch.data_ptr(), scratch.numel(), None)
    assert rc == A
    with pytest.raises(FdfError):
        fast_hip.track_array(np.zeros((24, 32), np.uint8), np.zeros((24, 32), np.uint8),
                             np.array([[1, 1]]), n_levels=40)
