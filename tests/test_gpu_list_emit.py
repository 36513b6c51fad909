"""The band end of the LDS-list tier: every listed keypoint gets its raster rank, a suppressed
one sets a kill bit at its rank (64 words of 32 ranks), and the band's points are written
straight from the list at rank minus the kills below it (fdf_sweep_impl.h, band_nms_lds and
sweep_band).

Every expectation is the CPU oracle's (oracle.detect), never the detector's own output.  The
frames are built as in test_gpu_band_end.py: on a black frame a pixel of value > t is exactly
one keypoint as long as no other bright pixel lies on its ring, which holds for bright pixels
that are adjacent (distance 1) or at least 4 apart; adjacent bright pixels are neighbouring
keypoints whose scores order as their values, equal values tying (both suppressed).  The CPU
tests of this file assert on the oracle alone that each construction is what it claims: the
count per band, the tier (`_band_tiers`, the layout arithmetic restated as in the band-end test),
the ranks of the suppressed keypoints, and the fallback's point count against its slot."""
import functools

import numpy as np
import pytest

import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

T = 16
N = 9
NMS_MODES = [1, 2]               # max-t, SAD
W_STRIPS = 1100                  # two column strips: centres 3 .. 991 and 992 .. 1096
LIST_CAP = 2048


# ---- the geometry the detector derives from a pinned band height (restated) ------------------

def _align16(v):
    return (v + 15) & ~15


def _words_per_row(w):
    return ((w + 31) // 32 + 3) & ~3


def _layout_total(R, nw, nms):
    rows = R + (2 if nms else 0)
    nb = (nw + 3) // 4
    pq = _align16(rows * nw * 4 + 4)
    slist = pq + 4 * 256 * 4 + 4 * 64 * 4
    bprefix = slist + (LIST_CAP * 4 if nms else 0)
    rprefix = bprefix + (_align16(rows * nb * 2) if nms else 0)
    prefix_end = rprefix + (_align16(rows * 4) if nms else 0)
    return max(prefix_end, bprefix + 1024) + 64, (bprefix - pq) // 2


def _band_height(w, nms, rows):
    nstrips = (w - 3 + 991) // 992
    nsub = (4 + nstrips - 1) // nstrips
    R = (rows + nsub - 1) // nsub * nsub
    nw = _words_per_row(w)
    while R > nsub and _layout_total(R, nw, nms)[0] > 160 * 1024:
        R -= nsub
    return R


def _pos_fits(w, bitmap_rows):
    xbits = (w - 1).bit_length()
    return xbits <= 20 and bitmap_rows <= 1 << (20 - xbits)


def _slot_points(w, R):
    """Points a band's slot lists in a grid that fills the chip (slots are 4x that in a
    smaller grid)."""
    return max(256, _align16(R * _words_per_row(w) * 4)) // 8


def _band_lists(img, t, n, rows):
    """Per band: (y0, r, the band's list in raster order: its own rows' keypoints and those of
    the row above and below it, before NMS)."""
    h, w = img.shape
    R = _band_height(w, 1, rows)
    off = oracle.detect(img, t, n, 0).astype(np.int64)
    bands = []
    for y0 in range(3, h - 3, R):
        r = min(R, h - 3 - y0)
        sel = (off[:, 1] >= y0 - 1) & (off[:, 1] <= y0 + r)
        bands.append((y0, r, off[sel]))
    return bands


def _band_tiers(img, t, n, nms, rows):
    """The NMS tier of every band of `img` with the band height pinned to `rows`."""
    h, w = img.shape
    R = _band_height(w, nms, rows)
    nw = _words_per_row(w)
    slot_words = max(256, _align16(R * nw * 4)) // 4
    area = _layout_total(R, nw, nms)[1]
    tiers = []
    for y0, r, kps in _band_lists(img, t, n, rows):
        kp = len(kps)
        cap = LIST_CAP if _pos_fits(w, r + 2) else 0
        spill_cap = slot_words if cap else 0
        if kp <= cap:
            tiers.append("list")
        elif kp - cap <= spill_cap and kp <= area:
            tiers.append("spill")
        else:
            tiers.append("dense")
    return tiers


def _killed_ranks(img, t, n, nms, rows):
    """Per band: the ranks of its list that are not output (suppressed, or in a halo row)."""
    kept = {tuple(p) for p in oracle.detect(img, t, n, nms).astype(np.int64)}
    out = []
    for y0, r, kps in _band_lists(img, t, n, rows):
        out.append([i for i, (x, y) in enumerate(kps)
                    if not (y0 <= y < y0 + r and (x, y) in kept)])
    return out


# ---- frames ----------------------------------------------------------------------------------

KS = [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049]
K_ROWS = 32                      # 8 rows of 274 cells at 4-pixel spacing: 2 192 >= 2 049


@functools.lru_cache(maxsize=None)
def _count_frames():
    """Three bands of K_ROWS rows; the middle band holds exactly k isolated keypoints (4 apart,
    seeded cell order and values) and the other two none, so the middle band's list is exactly
    those k (the first band sees the ones of the middle band's first row in its halo row)."""
    frames = []
    y0 = 3 + K_ROWS
    cells = [(x, y) for y in range(y0, y0 + K_ROWS - 3, 4) for x in range(3, W_STRIPS - 3, 4)]
    assert len(cells) >= max(KS)
    for k in KS:
        img = np.zeros((3 + 3 * K_ROWS + 3, W_STRIPS), dtype=np.uint8)
        rng = np.random.Generator(np.random.PCG64(4000 + k))
        for i in rng.permutation(len(cells))[:k]:
            x, y = cells[i]
            img[y, x] = rng.integers(T + 1, 256)
        frames.append(img)
    return np.stack(frames)


KILL_ROWS = 14
KILL_WANT = [0, 31, 32, 63, 64]


@functools.lru_cache(maxsize=None)
def _kill_frame():
    """Band 1 (of three, KILL_ROWS rows each): one row of isolated keypoints and runs of
    adjacent ones with rising values (all but the last of a run suppressed), placed so that
    the suppressed ones hold ranks 0, 31, 32, 63 and 64; four equal neighbours across the
    strip boundary (x = 990 .. 993); equal neighbours across the boundary of bands 1 and 2,
    vertical and diagonal (the diagonal also across the strip boundary) -- band 2's rank 0 is
    that halo-row keypoint, band 1's last ranks are halo-row keypoints; band 2 ends with a
    suppressed keypoint at its last rank."""
    R = KILL_ROWS
    img = np.zeros((3 + 3 * R + 3, W_STRIPS), dtype=np.uint8)
    y0 = 3 + R
    ya = y0 + 2
    x = 8
    runs = [[100, 200]] + [[180]] * 29 + [[100, 150, 200]] + [[180]] * 29 + [[100, 150, 200]] + \
           [[180]] * 5
    for run in runs:
        for v in run:
            img[ya, x] = v
            x += 1
        x += 3
    assert x < 980
    img[ya, 990:994] = 200
    img[y0 + R - 1, 500] = img[y0 + R, 500] = 200
    img[y0 + R - 1, 991] = img[y0 + R, 992] = 200
    yl = 3 + 2 * R + R - 3
    img[yl, 600] = 200
    img[yl, 601] = 100
    return img


@functools.lru_cache(maxsize=None)
def _edge_rows_frame():
    """Rows 3 and h-4 are never output and still suppress: a stronger, a weaker and an equal
    keypoint in each next to one in rows 4 / h-5, and an isolated one in each.  A halo-row
    keypoint at rank 0 of band 1 (the last row of band 0) suppresses a weaker neighbour in
    band 1's first row.  Returns (frame, the keypoints NMS keeps)."""
    R = KILL_ROWS
    h = 3 + 3 * R + 3
    img = np.zeros((h, W_STRIPS), dtype=np.uint8)
    for edge, inner in ((3, 4), (h - 4, h - 5)):
        img[edge, 40], img[inner, 41] = 200, 100
        img[edge, 60], img[inner, 60] = 100, 200
        img[edge, 80], img[inner, 80] = 200, 200
        img[edge, 100] = 200
    y0 = 3 + R
    img[y0 - 1, 10], img[y0, 11] = 200, 100
    return img, [(60, 4), (10, y0 - 1), (60, h - 5)]


FB_W, FB_ROWS, FB_T = 64, 64, 1
FB_COPIES = 1040                 # one band per frame: more than 1 024 bands, so no direct route


@functools.lru_cache(maxsize=None)
def _fallback_frames():
    """Four 64-wide frames of uniform noise, one 64-row band each (t = 1: dense)."""
    return tuple(np.random.Generator(np.random.PCG64(77 + s)).integers(
        0, 256, (FB_ROWS + 6, FB_W), dtype=np.uint8) for s in range(4))


ROUTE_W, ROUTE_H, ROUTE_ROWS = 128, 38, 8      # four 8-row bands per frame
ROUTE_COPIES = 50                               # x 6 frames x 4 bands = 1 200 bands


@functools.lru_cache(maxsize=None)
def _route_frames():
    rng = np.random.Generator(np.random.PCG64(5))
    dense = rng.integers(0, 256, (ROUTE_H, ROUTE_W), dtype=np.uint8)
    sparse = np.where(rng.integers(0, 16, (ROUTE_H, ROUTE_W)) == 0, dense, np.uint8(128))
    pairs = np.zeros((ROUTE_H, ROUTE_W), dtype=np.uint8)
    for i, y in enumerate(range(3, ROUTE_H - 4)):
        pairs[y, 8 + 3 * i] = 200
        pairs[y + 1, 9 + 3 * i] = 200 + i % 3 - 1     # weaker, equal, stronger
    return tuple([workloads.s1_frame(k, ROUTE_W, ROUTE_H) for k in range(3)] +
                 [dense, sparse.astype(np.uint8), pairs])


@functools.lru_cache(maxsize=None)
def _want(kind, t, nms):
    frames = {"count": _count_frames, "fallback": _fallback_frames, "route": _route_frames}[kind]()
    return tuple(oracle.detect(f, t, N, nms) for f in frames)


# ---- CPU checks of the constructions ---------------------------------------------------------

def test_counts_and_tiers_by_construction():
    """The middle band's list is exactly k keypoints, all kept by NMS (none are neighbours);
    k <= 2 048 is the list tier in every band and 2 049 the spill tier in the middle band."""
    for k, img in zip(KS, _count_frames()):
        lists = _band_lists(img, T, N, K_ROWS)
        assert len(lists) == 3 and len(lists[1][2]) == k
        tiers = _band_tiers(img, T, N, 1, K_ROWS)
        assert tiers == ["list", "spill" if k > LIST_CAP else "list", "list"], (k, tiers)
        for nms in NMS_MODES:
            assert len(oracle.detect(img, T, N, nms)) == k


def test_kill_ranks_by_construction():
    for nms in NMS_MODES:
        killed = _killed_ranks(_kill_frame(), T, N, nms, KILL_ROWS)
        lists = _band_lists(_kill_frame(), T, N, KILL_ROWS)
        assert len(lists) == 3
        n1, n2 = len(lists[1][2]), len(lists[2][2])
        assert n1 > 65 and set(KILL_WANT) <= set(killed[1]) and n1 - 1 in killed[1]
        # the singles between the runs are kept: the kills are not everything
        assert not {1, 2, 30, 33, 34, 62, 65, 66} & set(killed[1])
        # the equal run across the strip boundary: all four suppressed
        xs = lists[1][2][killed[1]][:, 0]
        assert {990, 991, 992, 993} <= set(xs.tolist())
        assert 0 in killed[2] and n2 - 1 in killed[2] and n2 - 2 not in killed[2]
    assert _band_tiers(_kill_frame(), T, N, 1, KILL_ROWS) == ["list"] * 3


def test_edge_rows_by_construction():
    img, keep = _edge_rows_frame()
    assert len(oracle.detect(img, T, N, 0)) == 16
    for nms in NMS_MODES:
        assert [tuple(p) for p in oracle.detect(img, T, N, nms).tolist()] == keep
    assert _killed_ranks(img, T, N, 1, KILL_ROWS)[1][0] == 0       # the halo-row keypoint


def test_fallback_by_construction():
    """Every fallback frame is one list-tier band whose kept points do not fit its slot in a
    grid that fills the chip."""
    assert _band_height(FB_W, 1, FB_ROWS) == FB_ROWS
    for nms in NMS_MODES:
        for img, want in zip(_fallback_frames(), _want("fallback", FB_T, nms)):
            assert _band_tiers(img, FB_T, N, nms, FB_ROWS) == ["list"]
            assert len(want) > _slot_points(FB_W, FB_ROWS)


def test_route_frames_by_construction():
    for img in _route_frames():
        assert _band_tiers(img, T, N, 1, ROUTE_ROWS) == ["list"] * 4
    assert len(_route_frames()) * ROUTE_COPIES * 4 > 1024 < FB_COPIES


# ---- GPU -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.lock = __import__("threading").Lock()
    yield c
    c.close()


def _detect(ctx, frames, t, nms, rows, total):
    """The device path on `ctx` with the band height pinned; returns (points, offsets)."""
    import torch

    ctx.set_band_rows(rows)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = torch.full((total + 64, 2), -1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(dev.shape[0] + 1, dtype=torch.int64, device="cuda")
    fast_hip.detect_device(dev, Config(t, N, NonMaximalSuppression(nms)), out, offs, ctx=ctx)
    torch.cuda.synchronize()
    o = offs.cpu().numpy()
    assert o[-1] <= total + 64, (o[-1], total)
    return out[: o[-1]].cpu().numpy().astype(np.uint32), o.astype(np.int64)


def _check(ctx, frames, want, t, nms, rows):
    pts, offs = _detect(ctx, np.stack(frames), t, nms, rows, sum(len(x) for x in want))
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist()
    for f, x in enumerate(want):
        assert np.array_equal(pts[offs[f]:offs[f + 1]], x), f


@pytest.mark.gpu
@pytest.mark.parametrize("nms", NMS_MODES)
def test_list_tier_boundaries(ctx, nms):
    """k = 0 .. 2 048 keypoints in a band's list (the kill words' and the list's edges), and
    2 049, which spills; one frame per launch (direct route) and all as one batch."""
    frames, want = _count_frames(), _want("count", T, nms)
    _check(ctx, frames, want, T, nms, K_ROWS)
    for img, x in zip(frames, want):
        _check(ctx, [img], [x], T, nms, K_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", NMS_MODES)
def test_kill_word_boundaries(ctx, nms):
    img = _kill_frame()
    _check(ctx, [img], [oracle.detect(img, T, N, nms)], T, nms, KILL_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", NMS_MODES)
def test_always_suppressed_rows(ctx, nms):
    img, _ = _edge_rows_frame()
    _check(ctx, [img], [oracle.detect(img, T, N, nms)], T, nms, KILL_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", NMS_MODES)
def test_fallback_to_the_bitmap(ctx, nms):
    """More kept points than the slot lists: on the compaction route the band clears its
    bitmap and hands that over; alone (direct route) the same frames come from the list."""
    frames, want = _fallback_frames(), _want("fallback", FB_T, nms)
    reps = FB_COPIES // len(frames)
    _check(ctx, list(frames) * reps, list(want) * reps, FB_T, nms, FB_ROWS)
    for img, x in zip(frames, want):
        _check(ctx, [img], [x], FB_T, nms, FB_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", NMS_MODES)
def test_both_output_routes(ctx, nms):
    """One small frame (direct look-back) and 1 200 eight-row bands (compaction launch)."""
    frames, want = _route_frames(), _want("route", T, nms)
    for img, x in zip(frames, want):
        _check(ctx, [img], [x], T, nms, ROUTE_ROWS)
    _check(ctx, list(frames) * ROUTE_COPIES, list(want) * ROUTE_COPIES, T, nms, ROUTE_ROWS)
