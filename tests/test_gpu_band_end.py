"""Band-end paths of the sweep kernel: unit / band leftovers, NMS ties across band and strip
boundaries, the shift-encoded score-list positions and the last frame of a batch.

Every expectation is the CPU oracle's (oracle.detect, or oracle.avx2_detect_batch for the large
batches; both are pinned to the reference's goldens in tests/test_oracle.py), never the
detector's own output.

Constructive frames: on a black frame one pixel of value >= t + 1 is exactly one keypoint (its
whole ring is darker by more than t; every other pixel sees at most two brighter ring pixels),
so k such pixels >= 8 apart are k keypoints, and a band, a strip or a wave can be given an
exact number of them: 0, one short of a 64-lane vector, exactly one, one over, and several
(the sizes at which the partial candidate batches and max-t queues at a unit's and a band's end
change shape; the kernel tests each wave's leftovers alone, there is no pool across waves).

NMS tiers: the detector has no hook that reports which tier (LDS list, slot spill, dense) a
band took, so `_band_tiers` restates the layout arithmetic of fdf_kernels.h / fdf_api.cpp /
fdf_sweep_impl.h on the oracle's NMS-off keypoints, and test_tiers_by_construction (no GPU)
asserts that the position-encoding cases put bands in every tier.  The restatement is
conservative, not exact: the host layer makes the slots of a small grid four times larger, so a
band classed "dense" for its count may really spill; what it classes "list" or "spill" is
that, and the dense tier is also reached by construction where positions do not fit 20 bits
(4097 columns, more than 128 bitmap rows: test_position_bits_boundary)."""
import functools

import numpy as np
import pytest

import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

T = 16
KS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
W_STRIPS = 1100                  # two column strips: centres 3 .. 991 and 992 .. 1096
BAND_ROWS = [14, 46]


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
    bprefix = slist + (2048 * 4 if nms else 0)
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


def _band_tiers(img, t, n, nms, rows):
    """The NMS tier of every band of `img` with the band height pinned to `rows`."""
    h, w = img.shape
    R = _band_height(w, nms, rows)
    nw = _words_per_row(w)
    slot_words = max(256, _align16(R * nw * 4)) // 4
    area = _layout_total(R, nw, nms)[1]
    ys = oracle.detect(img, t, n, 0)[:, 1].astype(np.int64)
    tiers = []
    for y0 in range(3, h - 3, R):
        r = min(R, h - 3 - y0)
        kp = int(np.count_nonzero((ys >= y0 - 1) & (ys <= y0 + r)))
        cap = 2048 if _pos_fits(w, r + 2) else 0
        spill_cap = slot_words if cap else 0
        if kp <= cap:
            tiers.append("list")
        elif kp - cap <= spill_cap and kp <= area:
            tiers.append("spill")
        else:
            tiers.append("dense")
    return tiers


# ---- frames ----------------------------------------------------------------------------------

def _height(R):
    return 3 + 3 * R + 3         # three bands: the middle one has both NMS halo rows in-frame


def _isolated_frame(R, k, x0, x1, bands, seed):
    """A black frame (W_STRIPS wide, three bands of R rows) with k pixels of value T + 1 .. 255,
    >= 8 apart, in columns [x0, x1) of each band in `bands`; the 8 x 8 cells are taken in a
    seeded order, so the pixels spread over the band's units."""
    img = np.zeros((_height(R), W_STRIPS), dtype=np.uint8)
    rng = np.random.Generator(np.random.PCG64(seed))
    for band in bands:
        y0 = 3 + band * R
        cells = [(x, y) for y in range(y0, y0 + R, 8) for x in range(x0, x1, 8)]
        assert k <= len(cells)
        for i in rng.permutation(len(cells))[:k]:
            x, y = cells[i]
            img[y, x] = rng.integers(T + 1, 256)
    return img


def _isolated_cases(R):
    """(k per band, bands, frame) for one strip and both strips, one band and two adjacent
    bands; k is capped by what fits the region at 8-pixel spacing (one strip of a 14-row band
    holds 2 x 124 cells, so its largest counts are 129 there)."""
    cases = []
    for x0, x1 in ((3, 992), (3, W_STRIPS - 3)):
        room = len(range(3, 3 + R, 8)) * len(range(x0, x1, 8))
        for bands in ((1,), (1, 2)):
            for k in KS:
                if k <= room:
                    cases.append((k, bands, _isolated_frame(R, k, x0, x1, bands,
                                                            1000 * R + 10 * k + len(bands) + x1)))
    return cases


PAIR_DIRS = [(1, 0), (0, 1), (1, 1), (-1, 1)]


def _pair_sites(R):
    """First pixels and directions of the adjacent pairs: rows 3, 4, h-5, h-4 (rows 3 and h-4
    are never output under NMS), both sides of the band boundaries, the strip boundary
    (columns 991 / 992), and both boundaries at once."""
    h = _pair_height(R)
    sites = []
    rows = [3, 4, h - 6, h - 5, h - 4, 3 + R - 2, 3 + R - 1, 3 + R, 3 + 2 * R - 1]
    i = 0
    for dx, dy in PAIR_DIRS:
        for y in rows:
            if y + dy <= h - 4:
                sites.append((40 + 24 * i, y, dx, dy))
                i += 1
    assert 40 + 24 * i < 960
    sites.append((991, 3 + R - 1, 1, 1))                  # strip and band boundary
    sites.append((992, 3 + 2 * R - 1, -1, 1))
    strip_only = [(991, 1, 0), (991, 0, 1), (992, 0, 1), (991, 1, 1), (992, -1, 1)]
    for band, (x, dx, dy) in enumerate(strip_only, start=3):
        sites.append((x, 3 + band * R + R // 2, dx, dy))
    return sites


def _pair_height(R):
    return 3 + 8 * R + 3


def _pair_frames(R):
    """Three frames: equal values, first pixel stronger, second pixel stronger."""
    frames = []
    for va, vb in ((200, 200), (205, 200), (200, 205)):
        img = np.zeros((_pair_height(R), W_STRIPS), dtype=np.uint8)
        for x, y, dx, dy in _pair_sites(R):
            img[y, x] = va
            img[y + dy, x + dx] = vb
        frames.append(img)
    return frames


def _noise(w, h, seed, sparse):
    """Uniform noise (dense: ~a quarter of the pixels are keypoints at t = 8), or the same
    noise on one pixel in 16 of a flat frame (a few per cent)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if sparse:
        img = np.where(rng.integers(0, 16, (h, w)) == 0, img, np.uint8(128)).astype(np.uint8)
    return img


POS_WIDTHS = [7, 33, 1024, 1025, 2049, 4097]     # ceil(log2 W) = 3, 6, 10, 11, 12, 13
POS_HEIGHTS = [7, 8, 12, 25, 40]
POS_ROWS = [1, 2, 256]                            # 256: cut to the largest the layout allows


@functools.lru_cache(maxsize=None)
def _pos_frames(w):
    return tuple(_noise(w, h, 7 * w + h + s, bool(s)) for h in POS_HEIGHTS for s in (0, 1))


@functools.lru_cache(maxsize=None)
def _want(key, t, n, nms):
    kind, arg = key
    frames = _pos_frames(arg) if kind == "pos" else _wide_frames()
    return tuple(oracle.detect(f, t, n, nms) for f in frames)


@functools.lru_cache(maxsize=None)
def _wide_frames():
    # 4097 wide (13 x bits: at most 128 bitmap rows keep 20-bit positions), 140 rows
    return (workloads.s1_frame(3, 4097, 140), _noise(4097, 140, 99, True))


# ---- CPU checks of the constructions ---------------------------------------------------------

@pytest.mark.parametrize("n", [9, 12])
def test_isolated_pixels_are_single_keypoints(n):
    """The oracle on the constructive frames: k isolated pixels are exactly k keypoints, in
    every NMS mode (no two are neighbours)."""
    for k, bands, img in _isolated_cases(14)[::5]:
        for nms in (0, 1, 2):
            assert len(oracle.detect(img, T, n, nms)) == k * len(bands), (k, bands, nms)


def test_adjacent_pairs_in_the_oracle():
    """Equal neighbours are both dropped under NMS, of unequal ones the stronger stays;
    without NMS both are keypoints.  (Rows 3 and h-4 are not output under NMS, so only the
    pair sites clear of them are counted.)"""
    R = 14
    h = _pair_height(R)
    inner = [s for s in _pair_sites(R) if s[1] > 3 and s[1] + s[3] < h - 4]
    for f, keep in zip(range(3), (0, 1, 1)):
        img = np.zeros((h, W_STRIPS), dtype=np.uint8)
        va, vb = ((200, 200), (205, 200), (200, 205))[f]
        for x, y, dx, dy in inner:
            img[y, x] = va
            img[y + dy, x + dx] = vb
        assert len(oracle.detect(img, T, 9, 0)) == 2 * len(inner)
        for nms in (1, 2):
            assert len(oracle.detect(img, T, 9, nms)) == keep * len(inner), (f, nms)


def test_tiers_by_construction():
    """The position-encoding cases reach every NMS tier (restated layout arithmetic), and the
    wide frames straddle the height at which 20-bit positions stop fitting."""
    seen = set()
    for w in POS_WIDTHS:
        for rows in POS_ROWS:
            for img in _pos_frames(w):
                seen.update(_band_tiers(img, 8, 12, 2, rows))
    assert seen == {"list", "spill", "dense"}
    assert _band_height(4097, 2, 126) == 126 and _band_height(4097, 2, 127) == 127
    assert _pos_fits(4097, 126 + 2) and not _pos_fits(4097, 127 + 2)
    assert _pos_fits(4096, 256) and not _pos_fits(2049, 257) and _pos_fits(2048, 258)


# ---- GPU -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.lock = __import__("threading").Lock()
    yield c
    c.close()


def _detect(ctx, frames, t, n, nms, rows, total):
    """The device path on `ctx` with the band height pinned; returns (points, offsets)."""
    import torch

    ctx.set_band_rows(rows)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = torch.full((total + 64, 2), -1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(dev.shape[0] + 1, dtype=torch.int64, device="cuda")
    fast_hip.detect_device(dev, Config(t, n, NonMaximalSuppression(nms)), out, offs, ctx=ctx)
    torch.cuda.synchronize()
    o = offs.cpu().numpy()
    assert o[-1] <= total + 64, (o[-1], total)
    return out[: o[-1]].cpu().numpy().astype(np.uint32), o.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _isolated_batch(R):
    cases = _isolated_cases(R)
    return cases, np.stack([c[2] for c in cases])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("nms", [0, 1, 2])
@pytest.mark.parametrize("R", BAND_ROWS)
def test_isolated_keypoint_counts(ctx, R, nms, n):
    """k = 0 .. 257 isolated keypoints in one band and in two adjacent bands, over one strip
    and both, as one batch per band height (its last frame takes the exact-resource path)."""
    cases, frames = _isolated_batch(R)
    want_pts, want_offs = oracle.avx2_detect_batch(frames, T, n, nms)
    counts = np.diff(want_offs.astype(np.int64))
    assert counts.tolist() == [k * len(bands) for k, bands, _ in cases]
    pts, offs = _detect(ctx, frames, T, n, nms, R, len(want_pts))
    assert np.array_equal(offs, want_offs)
    assert np.array_equal(pts, want_pts)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("nms", [0, 1, 2])
@pytest.mark.parametrize("R", BAND_ROWS)
def test_adjacent_pairs(ctx, R, nms, n):
    """Equal and unequal neighbours, horizontal, vertical and on both diagonals, across band
    boundaries, across the strip boundary and on the first and last two centre rows."""
    frames = _pair_frames(R)
    want = [oracle.detect(f, T, n, nms) for f in frames]
    pts, offs = _detect(ctx, np.stack(frames), T, n, nms, R, sum(len(x) for x in want))
    for f, x in enumerate(want):
        assert np.array_equal(pts[offs[f]:offs[f + 1]], x), f


@pytest.mark.gpu
@pytest.mark.parametrize("rows", POS_ROWS)
@pytest.mark.parametrize("w", POS_WIDTHS)
def test_position_encoding(ctx, w, rows):
    """Widths whose x field takes 3 .. 13 bits, heights 7 .. 40, dense and sparse noise at
    t = 8 (list, spill and dense tiers: test_tiers_by_construction), every NMS mode."""
    frames = _pos_frames(w)
    for n, nms in ((12, 2), (12, 1), (9, 1), (9, 0)):
        want = _want(("pos", w), 8, n, nms)
        for img, x in zip(frames, want):
            pts, _ = _detect(ctx, img[None], 8, n, nms, rows, len(x))
            assert np.array_equal(pts, x), (img.shape, n, nms)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [126, 127])
@pytest.mark.parametrize("nms", [1, 2])
def test_position_bits_boundary(ctx, rows, nms):
    """4097 columns: 128 bitmap rows (126-row bands) are the most whose positions fit 20 bits;
    a 127-row band takes the score-free dense tier.  Same keypoints either way."""
    want = _want(("wide", 0), T, 9, nms)
    for img, x in zip(_wide_frames(), want):
        pts, _ = _detect(ctx, img[None], T, 9, nms, rows, len(x))
        assert np.array_equal(pts, x)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", [0, 1, 2])
def test_small_batch_ends_with_its_buffer(ctx, nms):
    """3 frames of 64 x 48 in a device tensor of exactly 3 * 64 * 48 bytes, the frames packed
    and the last one ending with the tensor: it is read through the exact resource.  (The
    tensor comes from a caching allocator, so the bytes after it are mapped: a read past the
    frame shows as a wrong list where it changes one, not as a fault.)"""
    w, h = 64, 48
    frames = np.stack([workloads.s1_frame(5, w, h), workloads.s3_frame(2, w, h),
                       workloads.s3_frame(3, w, h)])
    want = [oracle.detect(f, T, 9, nms) for f in frames]
    pts, offs = _detect(ctx, frames, T, 9, nms, 0, sum(len(x) for x in want))
    for f, x in enumerate(want):
        assert np.array_equal(pts[offs[f]:offs[f + 1]], x), f
