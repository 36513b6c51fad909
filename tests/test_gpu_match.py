"""Brute-force Hamming matching on the device (fdf_match_device, fdf_match_filter_device,
fdf_match_points) against the numpy restatement of include/fdf.h's semantics in
tests/_match_reference.py.  Every comparison is exact; every output buffer is pre-filled and
over-allocated so that the entries no frame owns can be checked as untouched."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import _match_reference as ref
import workloads
from feature_detector_fast_amd import Config, NonMaximalSuppression, _native, fast_hip
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A                                  # of matches: index, distance and second
KEEP_FILL = 0x77
EXTRA = 16                                         # rows past the capacity


def fill_records(n):
    return np.full((n, 2), FILL, dtype=np.uint32).view(ref.MATCH_DTYPE).reshape(-1)


def random_desc(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def tied_desc(rng, n, pool):
    """Rows of `pool` with 0..2 random bits flipped: equal descriptors and distances abound."""
    d = pool[rng.integers(0, len(pool), n)].copy()
    for row in d:
        for bit in rng.integers(0, 256, rng.integers(0, 3)):
            row[bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def device_desc(torch, desc, misalign=0):
    """The descriptors on the device; with `misalign` the tensor starts that many bytes into
    its allocation."""
    desc = np.ascontiguousarray(desc)
    raw = torch.zeros(misalign + desc.size + 64, dtype=torch.uint8, device="cuda")
    view = raw[misalign:misalign + desc.size].view(-1, 32)
    view.copy_(torch.from_numpy(desc.copy()).cuda())
    assert view.data_ptr() % 16 == misalign % 16
    return view


def device_points(torch, pts):
    return torch.from_numpy(np.ascontiguousarray(pts, dtype=np.uint32).view(np.int32).copy()).cuda()


def device_offsets(torch, offs):
    return torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()


def run_match(q_desc, q_offs, t_desc, t_offs, q_pts=None, t_pts=None, window=None):
    """fdf_match_device on uploaded sets -> (len(q_desc) + EXTRA,) records, pre-filled; the
    inputs are checked as untouched."""
    import torch

    dq, dt = device_desc(torch, q_desc), device_desc(torch, t_desc)
    dqo, dto = device_offsets(torch, q_offs), device_offsets(torch, t_offs)
    dqp = None if q_pts is None else device_points(torch, q_pts)
    dtp = None if t_pts is None else device_points(torch, t_pts)
    matches = torch.full((len(q_desc) + EXTRA, 2), FILL, dtype=torch.int32, device="cuda")
    fast_hip.match_device(dq, dqo, dt, dto, matches, q_points=dqp, t_points=dtp, window=window)
    torch.cuda.synchronize()
    assert np.array_equal(dq.cpu().numpy(), q_desc) and np.array_equal(dt.cpu().numpy(), t_desc)
    assert np.array_equal(dqo.cpu().numpy(), np.asarray(q_offs).astype(np.int64))
    assert np.array_equal(dto.cpu().numpy(), np.asarray(t_offs).astype(np.int64))
    if dqp is not None:
        assert np.array_equal(dqp.cpu().numpy().view(np.uint32), q_pts)
        assert np.array_equal(dtp.cpu().numpy().view(np.uint32), t_pts)
    return ref.as_records(matches.cpu().numpy())


def reference(q_desc, q_offs, t_desc, t_offs, q_pts=None, t_pts=None, window=None):
    return ref.match(q_desc, q_offs, len(q_desc), t_desc, t_offs, len(t_desc), q_pts, t_pts,
                     window, out=fill_records(len(q_desc) + EXTRA))


def match_one_pair(q, t, q_pts=None, t_pts=None, window=None):
    """(device result, reference) of one frame pair."""
    args = (q, [0, len(q)], t, [0, len(t)], q_pts, t_pts, window)
    return run_match(*args), reference(*args)


# ---- 1: every tile and pass edge, in one call --------------------------------------------------

def test_size_grid():
    sizes = (0, 1, 2, 63, 64, 65, 255, 256, 257, 600)
    pairs = list(itertools.product(sizes, sizes))
    q_offs = np.cumsum([0] + [a for a, _ in pairs])
    t_offs = np.cumsum([0] + [b for _, b in pairs])
    q, t = random_desc(11, q_offs[-1]), random_desc(12, t_offs[-1])
    got = run_match(q, q_offs, t, t_offs)
    want = reference(q, q_offs, t, t_offs)
    for name in ("index", "distance", "second"):
        assert np.array_equal(got[name], want[name]), name
    assert (got["index"][:q_offs[-1]] == ref.NONE).sum() == sum(a for a, b in pairs if b == 0)


# ---- 2: ties and extremes ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tied_sets(which):
    """(query, train) descriptors from a pool of 6: 300 x 300 and 257 x 1."""
    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    if which == "300x300":
        q, t = tied_desc(rng, 300, pool), tied_desc(rng, 300, pool)
        t[5] = pool[0]
        t[5, 9] ^= 0x81                            # a descriptor no other row equals
        t[5, 20] ^= 0x42
        t[17] = t[5]                               # ... but its duplicate
        q[0] = t[5]
    else:
        t = tied_desc(rng, 1, pool)
        q = tied_desc(rng, 257, pool)
        q[3] = ~t[0]
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@pytest.mark.parametrize("which", ["300x300", "257x1"])
def test_ties_and_extremes(which):
    q, t = tied_sets(which)
    got, want = match_one_pair(q, t)
    assert np.array_equal(got, want)
    if which == "300x300":
        assert tuple(got[0]) == (5, 0, 0)          # the duplicate: the lower index, second 0
        d = ref.distances(q, t)
        ties = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
        assert (ties > 1).sum() > 100              # the tie rule was exercised
    else:
        assert tuple(got[3]) == (0, 256, ref.NO_DISTANCE)
        assert (got["second"][:257] == ref.NO_DISTANCE).all() and (got["index"][:257] == 0).all()


# ---- 3: the window -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_points():
    pts = oracle.detect(workloads.golden_image(), 16, 9, 0)
    assert len(pts) == 309 and (np.diff(pts[:, 1].astype(np.int64)) >= 0).all()
    pts.setflags(write=False)
    return pts


def test_window():
    pts = golden_points()
    q, t = random_desc(31, len(pts)), random_desc(32, len(pts))
    plain, want_plain = match_one_pair(q, t)
    assert np.array_equal(plain, want_plain)
    for window in ((0, 0), (5, 3), (40, 0), (0, 40), (10 ** 6, 10 ** 6)):
        got, want = match_one_pair(q, t, pts, pts, window)
        assert np.array_equal(got, want), window
        assert (got["index"][:len(pts)] != ref.NONE).all()       # a point is in its own window
    assert np.array_equal(got, plain)                            # the last window holds all
    only_self, _ = match_one_pair(q, t, pts, pts, (0, 0))
    assert np.array_equal(only_self["index"][:len(pts)], np.arange(len(pts)))
    assert (only_self["second"][:len(pts)] == ref.NO_DISTANCE).all()


def test_window_shuffled_queries():
    pts = golden_points()
    order = np.random.default_rng(33).permutation(len(pts))
    q, t = random_desc(34, len(pts)), random_desc(35, len(pts))
    for window in ((5, 3), (40, 0), (0, 40), (25, 25)):
        got, want = match_one_pair(q, t, pts[order], pts, window)
        assert np.array_equal(got, want), window


def test_window_without_candidates():
    pts = golden_points()
    moved = pts.copy()
    moved[:, 0] += 37                              # the queries: the same points 37 columns on
    moved[::7, 1] += 500                           # ... and some far below every train point
    q, t = random_desc(36, len(pts)), random_desc(37, len(pts))
    got, want = match_one_pair(q, t, moved, pts, (5, 3))
    assert np.array_equal(got, want)
    none = got["index"][:len(pts)] == ref.NONE
    assert none[::7].all() and 50 < none.sum() < len(pts)
    assert (got["distance"][:len(pts)][none] == ref.NO_DISTANCE).all()
    assert (got["second"][:len(pts)][none] == ref.NO_DISTANCE).all()


# ---- 4: caps and shifted offsets ---------------------------------------------------------------

@pytest.mark.parametrize("with_window", [False, True])
@pytest.mark.parametrize("q_cap,t_cap", [(200, 760), (760, 420), (200, 420), (760, 760)])
def test_caps_and_shifted_offsets(q_cap, t_cap, with_window):
    """Four frames matched f -> f + 1 over one descriptor tensor that is 4-byte but not 16-byte
    aligned; the caps cut a frame in the middle and the frames past it away."""
    import torch

    offs = np.array([5, 75, 365, 495, 755])
    rows = 760
    rng = np.random.default_rng(41)
    desc = tied_desc(rng, rows, rng.integers(0, 256, (40, 32), dtype=np.uint8))
    pts = np.zeros((rows, 2), dtype=np.uint32)
    for f in range(4):
        n = offs[f + 1] - offs[f]
        pts[offs[f]:offs[f + 1], 0] = rng.integers(0, 200, n)
        pts[offs[f]:offs[f + 1], 1] = np.sort(rng.integers(0, 120, n))
    window = (60, 25) if with_window else None
    d_desc = device_desc(torch, desc, misalign=4)
    assert d_desc.data_ptr() % 16 == 4
    d_pts = device_points(torch, pts) if with_window else None
    d_offs = device_offsets(torch, offs)
    matches = torch.full((rows + EXTRA, 2), FILL, dtype=torch.int32, device="cuda")
    fast_hip.match_device(d_desc[:q_cap], d_offs[:-1], d_desc[:t_cap], d_offs[1:],
                          matches[:q_cap + EXTRA],
                          q_points=d_pts[:q_cap] if with_window else None,
                          t_points=d_pts[:t_cap] if with_window else None, window=window)
    torch.cuda.synchronize()
    got = ref.as_records(matches.cpu().numpy())
    want = ref.match(desc, offs[:-1], q_cap, desc, offs[1:], t_cap,
                     pts if with_window else None, pts if with_window else None, window,
                     out=fill_records(rows + EXTRA))
    assert np.array_equal(got, want)
    end = min(int(offs[3]), q_cap)
    assert np.array_equal(got[:5], fill_records(5)) and np.array_equal(got[end:],
                                                                       fill_records(rows + EXTRA - end))
    hit = got["index"][5:end] != ref.NONE
    assert hit.any() and (got["index"][5:end][hit] < t_cap).all()
    assert np.array_equal(d_desc.cpu().numpy(), desc)


# ---- 5: the filter -----------------------------------------------------------------------------

def run_filter(fwd, q_offs, rev=None, max_distance=256, ratio=None):
    """fdf_match_filter_device on uploaded records -> (len(fwd) + EXTRA,) uint8, pre-filled."""
    import torch

    as_tensor = lambda rec: torch.from_numpy(rec.copy().view(np.int32).reshape(-1, 2)).cuda()
    d_fwd = as_tensor(fwd)
    d_rev = None if rev is None else as_tensor(rev)
    keep = torch.full((len(fwd) + EXTRA,), KEEP_FILL, dtype=torch.uint8, device="cuda")
    fast_hip.match_filter_device(d_fwd, device_offsets(torch, q_offs), keep, reverse=d_rev,
                                 max_distance=max_distance, ratio=ratio)
    torch.cuda.synchronize()
    assert np.array_equal(ref.as_records(d_fwd.cpu().numpy()), fwd)
    return keep.cpu().numpy()


@pytest.mark.parametrize("which", ["300x300", "257x1"])
def test_filter(which):
    q, t = tied_sets(which)
    fwd = run_match(q, [0, len(q)], t, [0, len(t)])[:len(q)]
    rev = run_match(t, [0, len(t)], q, [0, len(q)])[:len(t)]
    assert np.array_equal(fwd, ref.match_pair(q, t)) and np.array_equal(rev, ref.match_pair(t, q))
    seen = set()
    for max_distance, ratio, cross in itertools.product((0, 40, 256), ((3, 4), (1, 1), None),
                                                        (False, True)):
        for offs in ([0, len(q)], [3, 100, len(q) - 4]):
            got = run_filter(fwd, offs, rev if cross else None, max_distance, ratio)
            want = ref.match_filter(fwd, offs, len(fwd), rev if cross else None, len(rev),
                                    max_distance, ratio,
                                    out=np.full(len(fwd) + EXTRA, KEEP_FILL, np.uint8))
            assert np.array_equal(got, want), (max_distance, ratio, cross, offs)
        seen.add(got[3:len(q) - 4].tobytes())
    if which == "300x300":
        assert len(seen) >= 4                      # the rules cut differently


def test_filter_forged_index():
    q, t = tied_sets("300x300")
    fwd = ref.match_pair(q, t)
    rev = ref.match_pair(t, q)
    forged = fwd.copy()
    forged["index"][[1, 50, 299]] = [len(t), len(t) + 5, 0xFFFFFFFE]
    got = run_filter(forged, [0, len(q)], rev)
    want = ref.match_filter(forged, [0, len(q)], len(q), rev, len(t),
                            out=np.full(len(q) + EXTRA, KEEP_FILL, np.uint8))
    assert np.array_equal(got, want)
    assert got[[1, 50, 299]].tolist() == [0, 0, 0] and got[:len(q)].sum() > 0
    assert run_filter(forged, [0, len(q)])[[1, 50, 299]].tolist() == [1, 1, 1]   # no cross-check


# ---- 6: stream order ---------------------------------------------------------------------------

def test_stream_order():
    """Fill, match and read back on a side stream with no host synchronisation in between."""
    import torch

    n_q, n_t = 700, 900
    q, t = random_desc(61, n_q), random_desc(62, n_t)
    h_q, h_t = torch.from_numpy(q.copy()).pin_memory(), torch.from_numpy(t.copy()).pin_memory()
    d_q = torch.zeros((n_q, 32), dtype=torch.uint8, device="cuda")
    d_t = torch.zeros((n_t, 32), dtype=torch.uint8, device="cuda")
    q_offs = device_offsets(torch, [0, 300, n_q])
    t_offs = device_offsets(torch, [0, 500, n_t])
    matches = torch.full((n_q, 2), FILL, dtype=torch.int32, device="cuda")
    keep = torch.full((n_q,), KEEP_FILL, dtype=torch.uint8, device="cuda")
    h_out = torch.zeros((n_q, 2), dtype=torch.int32).pin_memory()
    h_keep = torch.zeros((n_q,), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        d_q.copy_(h_q, non_blocking=True)
        d_t.copy_(h_t, non_blocking=True)
        fast_hip.match_device(d_q, q_offs, d_t, t_offs, matches)
        fast_hip.match_filter_device(matches, q_offs, keep, ratio=(3, 4))
        h_out.copy_(matches, non_blocking=True)
        h_keep.copy_(keep, non_blocking=True)
    stream.synchronize()
    want = ref.match(q, [0, 300, n_q], n_q, t, [0, 500, n_t], n_t)
    assert np.array_equal(ref.as_records(h_out.numpy()), want)
    assert np.array_equal(h_keep.numpy(), ref.match_filter(want, [0, 300, n_q], n_q, ratio=(3, 4)))


# ---- 7: argument errors from the C ABI ---------------------------------------------------------

def test_c_entry_argument_errors():
    """FDF_ERR_ARG synchronously and nothing launched (the outputs keep their fill)."""
    import torch

    n = 64
    raw = torch.zeros(n * 32 + 64, dtype=torch.uint8, device="cuda")
    desc = raw[:n * 32].view(n, 32)
    pts = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 32, n], dtype=torch.int64, device="cuda")
    raw_matches = torch.full((2 * n + 2,), FILL, dtype=torch.int32, device="cuda")
    matches = raw_matches[:2 * n].view(n, 2)
    keep = torch.full((n,), KEEP_FILL, dtype=torch.uint8, device="cuda")
    lib = _native.load()
    ctx = fast_hip.context(0).handle
    good = dict(ctx=ctx, n=2, qd=desc.data_ptr(), qp=None, qcap=n, qo=offs.data_ptr(),
                td=desc.data_ptr(), tp=None, tcap=n, to=offs.data_ptr(), dx=0, dy=0,
                out=matches.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return lib.fdf_match_device(a["ctx"], a["n"], a["qd"], a["qp"], a["qcap"], a["qo"], a["td"],
                                    a["tp"], a["tcap"], a["to"], a["dx"], a["dy"], a["out"], None)

    for bad in (dict(ctx=None), dict(qd=None), dict(qo=None), dict(td=None), dict(to=None),
                dict(out=None), dict(qp=pts.data_ptr()), dict(tp=pts.data_ptr()),
                dict(qd=desc.data_ptr() + 2), dict(td=desc.data_ptr() + 1),
                dict(out=raw_matches.data_ptr() + 4), dict(n=65536),
                dict(qcap=0xFFFFFFFF), dict(tcap=0xFFFFFFFF), dict(qcap=1 << 40)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert call(n=0) == _native.FDF_OK
    assert call(qcap=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (raw_matches == FILL).all()

    fgood = dict(ctx=ctx, n=2, m=matches.data_ptr(), qcap=n, qo=offs.data_ptr(), rev=None, tcap=0,
                 dist=256, num=3, den=4, keep=keep.data_ptr())

    def fcall(**kw):
        a = {**fgood, **kw}
        return lib.fdf_match_filter_device(a["ctx"], a["n"], a["m"], a["qcap"], a["qo"], a["rev"],
                                           a["tcap"], a["dist"], a["num"], a["den"], a["keep"],
                                           None)

    for bad in (dict(ctx=None), dict(m=None), dict(qo=None), dict(keep=None), dict(n=65536),
                dict(num=65536), dict(den=65536), dict(qcap=0xFFFFFFFF), dict(tcap=0xFFFFFFFF),
                dict(m=raw_matches.data_ptr() + 4),
                dict(rev=raw_matches.data_ptr() + 4, tcap=n)):
        assert fcall(**bad) == _native.FDF_ERR_ARG, bad
    assert fcall(n=0) == _native.FDF_OK
    assert fcall(qcap=0) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (keep == KEEP_FILL).all()
    # the good calls work, on the null stream: equal descriptors match index 0 of their frame
    assert call() == _native.FDF_OK
    assert call(qp=pts.data_ptr(), tp=pts.data_ptr(), out=matches.data_ptr()) == _native.FDF_OK
    assert fcall() == _native.FDF_OK
    torch.cuda.synchronize()
    got = ref.as_records(matches.cpu().numpy())
    assert (got["index"] == np.repeat([0, 32], 32)).all() and (got["distance"] == 0).all()
    assert (got["second"] == 0).all() and (raw_matches[2 * n:] == FILL).all()
    assert (keep == 0).all()                                     # 0 * 4 < 0 * 3 is false


# ---- 8: end to end -----------------------------------------------------------------------------

def test_device_chain():
    """detect -> orient -> smooth -> describe -> match both ways -> filter on one stream with
    nothing in between, against the reference run on the downloaded descriptors."""
    import torch

    img = workloads.golden_image()
    h, w = img.shape
    shifted = np.pad(img, ((2, 0), (3, 0)), mode="edge")[:h, :w]  # moved by (3, 2)
    frames = torch.from_numpy(np.stack([img, shifted])).cuda()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    cap, n_bins, window = 1024, 30, (12, 10)
    pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    offs = torch.zeros(3, dtype=torch.int64, device="cuda")
    ang = torch.zeros(cap, dtype=torch.float32, device="cuda")
    smoothed = torch.zeros_like(frames)
    desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)).cuda()
    fwd = torch.full((cap + EXTRA, 2), FILL, dtype=torch.int32, device="cuda")
    rev = torch.full((cap + EXTRA, 2), FILL, dtype=torch.int32, device="cuda")
    itself = torch.full((cap, 2), FILL, dtype=torch.int32, device="cuda")
    keep = torch.full((cap + EXTRA,), KEEP_FILL, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fast_hip.detect_device(frames, cfg, pts, offs)
        fast_hip.orient_device(frames, pts, offs, ang)
        fast_hip.smooth_device(frames, smoothed)
        fast_hip.describe_device(smoothed, pts, offs, desc, table, n_bins, angles=ang)
        fast_hip.match_device(desc, offs[:-1], desc, offs[1:], fwd, q_points=pts, t_points=pts,
                              window=window)
        fast_hip.match_device(desc, offs[1:], desc, offs[:-1], rev, q_points=pts, t_points=pts,
                              window=window)
        fast_hip.match_filter_device(fwd[:cap], offs[:-1], keep, reverse=rev[:cap],
                                     max_distance=80, ratio=(4, 5))
        fast_hip.match_device(desc, offs, desc, offs, itself)
    stream.synchronize()
    o = offs.cpu().numpy()
    n0, n = int(o[1]), int(o[2])
    assert n0 == 131 and n0 < n < cap
    h_desc, h_pts = desc.cpu().numpy(), pts.cpu().numpy().view(np.uint32)
    want_fwd = ref.match(h_desc, o[:-1], cap, h_desc, o[1:], cap, h_pts, h_pts, window,
                         out=fill_records(cap + EXTRA))
    want_rev = ref.match(h_desc, o[1:], cap, h_desc, o[:-1], cap, h_pts, h_pts, window,
                         out=fill_records(cap + EXTRA))
    got_fwd, got_rev = ref.as_records(fwd.cpu().numpy()), ref.as_records(rev.cpu().numpy())
    assert np.array_equal(got_fwd, want_fwd) and np.array_equal(got_rev, want_rev)
    want_keep = ref.match_filter(want_fwd, o[:-1], cap, want_rev, cap, 80, (4, 5),
                                 out=np.full(cap + EXTRA, KEEP_FILL, np.uint8))
    assert np.array_equal(keep.cpu().numpy(), want_keep)
    # a set against itself: every descriptor finds itself or an equal one before it
    index, distance, _ = fast_hip.unpack_matches(itself[:n].cpu().numpy())
    assert (distance == 0).all() and (index <= np.arange(n)).all() and (index >= 0).all()
    assert np.array_equal(h_desc[index], h_desc[:n])
    assert (itself[n:] == FILL).all()


# ---- 9: the host entries -----------------------------------------------------------------------

def test_host_entry():
    q_pts = workloads.read_points(os.path.join(workloads.GOLDEN, "kp_t16_n9_maxt.txt"))
    t_pts = golden_points()
    assert (len(q_pts), len(t_pts)) == (131, 309)
    rng = np.random.default_rng(91)
    pool = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    q, t = tied_desc(rng, 131, pool), tied_desc(rng, 309, pool)
    want = ref.match_pair(q, t)
    got = fast_hip.match_descriptors(q, t)
    assert got.dtype == fast_hip.MATCH_DTYPE and np.array_equal(got, want)
    window = (30, 20)
    want_w = ref.match_pair(q, t, q_pts, t_pts, window)
    assert np.array_equal(fast_hip.match_descriptors(q, t, q_pts, t_pts, window), want_w)
    assert not np.array_equal(want_w, want)                      # the window changes matches
    for kw in (dict(cross_check=True), dict(ratio=(3, 4)), dict(max_distance=3),
               dict(cross_check=True, ratio=(1, 1), max_distance=40)):
        got, keep = fast_hip.match_descriptors(q, t, **kw)
        assert np.array_equal(got, want)
        want_keep = ref.match_filter(want, [0, 131], 131,
                                     ref.match_pair(t, q) if kw.get("cross_check") else None, 309,
                                     kw.get("max_distance", 256), kw.get("ratio"))
        assert keep.dtype == np.bool_ and np.array_equal(keep, want_keep.astype(bool)), kw
    got, keep = fast_hip.match_descriptors(q, t, q_pts, t_pts, window, cross_check=True)
    want_keep = ref.match_filter(want_w, [0, 131], 131,
                                 ref.match_pair(t, q, t_pts, q_pts, window), 309)
    assert np.array_equal(got, want_w) and np.array_equal(keep, want_keep.astype(bool))
    # empty sets
    none = fast_hip.match_descriptors(q, t[:0])
    assert (none["index"] == ref.NONE).all() and (none["second"] == ref.NO_DISTANCE).all()
    assert len(fast_hip.match_descriptors(q[:0], t)) == 0
    empty, keep = fast_hip.match_descriptors(q, t[:0], cross_check=True)
    assert np.array_equal(empty, none) and not keep.any()


def test_host_entry_rejects_bad_arguments():
    lib = _native.load()
    ctx = fast_hip.context(0).handle
    q, t = random_desc(92, 4), random_desc(93, 6)
    pts = np.zeros((6, 2), np.uint32)
    out = fill_records(4)

    def call(c=ctx, qd=q.ctypes.data, qp=None, nq=4, td=t.ctypes.data, tp=None, nt=6,
             o=out.ctypes.data):
        return lib.fdf_match_points(c, qd, qp, nq, td, tp, nt, 0, 0, o)

    for bad in (dict(c=None), dict(qd=None), dict(td=None), dict(o=None),
                dict(qp=pts.ctypes.data), dict(tp=pts.ctypes.data)):
        assert call(**bad) == _native.FDF_ERR_ARG, bad
    assert np.array_equal(out, fill_records(4))
    assert call(nq=0, qd=None, o=None) == _native.FDF_OK
    assert call() == _native.FDF_OK
    assert np.array_equal(out, ref.match_pair(q, t))


def test_host_entry_keeps_fetch_last():
    img = workloads.golden_image()
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    pts, scores = fast_hip.detect_scored_array(img, cfg)
    fast_hip.match_descriptors(random_desc(94, 50), random_desc(95, 70))
    lib = _native.load()
    ctx = fast_hip.context(0)
    out = np.zeros((len(pts), 2), dtype=np.uint32)
    out_sc = np.zeros(len(pts), dtype=np.uint16)
    n = ctypes.c_size_t(0)
    rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data, out_sc.ctypes.data, len(pts),
                            ctypes.byref(n))
    assert rc == _native.FDF_OK and n.value == len(pts)
    assert np.array_equal(out, pts) and np.array_equal(out_sc, scores)


def test_cpp_match_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_match")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout
