"""Exact bilinear warp by a model per frame on the device (fdf_warp_device, fdf_warp_frame)
against the numpy restatement of include/fdf.h's rules in tests/_warp_reference.py.  Every
comparison is bit for bit; every run also proves that no byte outside the output frames or the
mask frames changed and that the input is intact."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from _warp_reference import CONSTANT, REPLICATE, model_invert, positions, warp
from feature_detector_fast_amd import _native, fast_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 0xEE
BORDERS = {REPLICATE: "replicate", CONSTANT: "constant"}
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def random_frame(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def strided(torch, f, h, w, stride, lead):
    """f frames of h x w on the device `stride` bytes apart, `lead` bytes into an allocation
    filled with GAP -> (the whole allocation, the (F, H, W) view)."""
    flat = torch.full((lead + f * stride + 64,), GAP, dtype=torch.uint8, device="cuda")
    return flat, torch.as_strided(flat, (f, h, w), (stride, w, 1), storage_offset=lead)


def device_models(torch, models, cols):
    """(F, 9) matrices as an (F, cols) float64 device tensor; columns past the ninth hold what an
    fdf_model holds there (counts: not doubles anyone reads)."""
    m = np.asarray(models, dtype=np.float64).reshape(-1, 9)
    a = np.full((len(m), cols), np.nan)
    a[:, :9] = m
    return torch.from_numpy(a).cuda()


def run_warp(frames, models, dw, dh, border=REPLICATE, fill=0, mask=True, in_stride=None,
             out_stride=None, lead_in=0, lead_out=0, cols=9):
    """fdf_warp_device on uploaded frames; checks that no byte outside the output and mask frames
    changed and that the input is intact, and returns (the warped frames, the masks or None)."""
    import torch

    frames = np.array(frames)                            # a writable copy for torch
    f, h, w = frames.shape
    in_stride = h * w if in_stride is None else in_stride
    out_stride = dh * dw if out_stride is None else out_stride
    _, d_in = strided(torch, f, h, w, in_stride, lead_in)
    d_in.copy_(torch.from_numpy(frames).cuda())
    d_models = device_models(torch, models, cols)
    kept = d_models.clone()
    flat_out, d_out = strided(torch, f, dh, dw, out_stride, lead_out)
    flat_mask, d_mask = strided(torch, f, dh, dw, out_stride, lead_out) if mask else (None, None)
    fast_hip.warp_device(d_in, d_models, d_out, border=BORDERS[border], fill=fill, mask=d_mask)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    d_out.fill_(GAP)                       # what is left must be the untouched fill
    assert (flat_out == GAP).all()
    got_mask = None
    if mask:
        got_mask = d_mask.cpu().numpy()
        d_mask.fill_(GAP)
        assert (flat_mask == GAP).all()
    assert np.array_equal(d_in.cpu().numpy(), frames)
    assert d_models.cpu().numpy().tobytes() == kept.cpu().numpy().tobytes()
    return got, got_mask


def check(frames, models, dw, dh, border=REPLICATE, fill=0, **kw):
    """run_warp against the restatement, frame by frame."""
    frames = np.asarray(frames)
    models = np.asarray(models, dtype=np.float64).reshape(-1, 9)
    got, got_mask = run_warp(frames, models, dw, dh, border, fill, **kw)
    for k in range(len(frames)):
        want, want_mask = warp(frames[k], models[k], dw, dh, border, fill)
        assert np.array_equal(got[k], want), (k, border, fill)
        if got_mask is not None:
            assert np.array_equal(got_mask[k], want_mask), (k, border, fill)
    return got, got_mask


# ---- models of a (source, destination) pair -----------------------------------------------------

def _scale(src, dst):
    return np.diag([src[0] / dst[0], src[1] / dst[1], 1.0])


def _shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float64)


def _centre(size):
    return (size[0] - 1) / 2, (size[1] - 1) / 2


def mild_homography(src, dst):
    m = np.array([[1.03, 0.05, -1.5], [-0.04, 0.98, 2.25], [0.11 / dst[0], -0.07 / dst[1], 1.0]])
    return (_scale(src, dst) @ m).reshape(9)


def rotation(src, dst, degrees=30.0):
    a = math.radians(degrees)
    r = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    cs, cd = _centre(src), _centre(dst)
    return (_shift(*cs) @ r @ _scale(src, dst) @ _shift(-cd[0], -cd[1])).reshape(9)


def zoom_out(src, dst, factor=2.5):
    cs, cd = _centre(src), _centre(dst)
    z = np.diag([factor, factor, 1.0])
    return (_shift(*cs) @ z @ _scale(src, dst) @ _shift(-cd[0], -cd[1])).reshape(9)


MODELS = {"homography": mild_homography, "rotation": rotation, "zoom_out": zoom_out}

# ---- 1: shapes -------------------------------------------------------------------------------

# destination widths below 4 run the thread-per-pixel kernel, the others the 4-column kernel;
# 5, 6, 7, 31, 53, 33 and 858 end in a partial column group; 858 x 8 and 9 x 858 are more than one
# workgroup; the 1 x 1 source has one tap for everything
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((1, 1), (9, 5)), ((2, 2), (1, 1)), ((5, 3), (4, 2)),
          ((37, 23), (31, 19)), ((64, 48), (53, 40)), ((41, 41), (20, 20)),
          ((100, 60), (33, 20)), ((20, 20), (47, 31)), ((1030, 9), (858, 8)),
          ((9, 1030), (9, 858))] + [((9, 9), (w, 5)) for w in (1, 2, 3, 5, 6, 7)]


@pytest.mark.parametrize("kind", sorted(MODELS))
@pytest.mark.parametrize("src,dst", SHAPES)
def test_warp_shapes(src, dst, kind):
    img = random_frame(src[0] + 7 * dst[0], *src)
    h = MODELS[kind](src, dst)
    check(img[None], [h], *dst, border=REPLICATE)
    check(img[None], [h], *dst, border=CONSTANT, fill=7)


def test_shapes_cover_both_kernels_and_partial_groups():
    widths = {d[0] for _, d in SHAPES}
    assert {1, 2, 3, 5, 6, 7, 31, 53, 858} <= widths
    assert any(w < 4 for w in widths) and any(w >= 4 and w % 4 for w in widths) and \
        any(w % 4 == 0 for w in widths)
    assert any(((d[0] + 3) // 4) * d[1] > 256 for _, d in SHAPES)        # more than one workgroup


def test_without_a_mask_the_pixels_are_the_same():
    img = random_frame(5, 37, 23)
    h = rotation((37, 23), (31, 19))
    with_mask, _ = check(img[None], [h], 31, 19)
    without, none = run_warp(img[None], [h], 31, 19, mask=False)
    assert none is None and np.array_equal(with_mask, without)
    narrow, none = run_warp(img[None], [h], 3, 19, mask=False)
    assert np.array_equal(narrow[0], warp(img, h, 3, 19)[0])


# ---- 2: borders, the mask, invalid pixels -------------------------------------------------------

@pytest.mark.parametrize("fill", [0, 7, 255])
@pytest.mark.parametrize("border", [REPLICATE, CONSTANT])
def test_borders_and_mask_with_every_side_outside(border, fill):
    img = random_frame(9, 37, 23)
    for dst in ((31, 19), (3, 19)):
        for h in (zoom_out((37, 23), dst), rotation((37, 23), dst, 45.0),
                  _shift(-3.25, -2.5).reshape(9), _shift(30.75, 20.5).reshape(9)):
            _, mask = check(img[None], [h], *dst, border=border, fill=fill)
            assert not mask.all()
    _, mask = check(img[None], [zoom_out((37, 23), (31, 19))], 31, 19, border=border, fill=fill)
    assert mask.any() and not mask[0, 0].any() and not mask[0, -1].any() and \
        not mask[0, :, 0].any() and not mask[0, :, -1].any()


@pytest.mark.parametrize("border", [REPLICATE, CONSTANT])
def test_the_line_w_equal_zero_inside_the_destination(border):
    """h6 = -0.125 on a 13-wide frame: w = 1 - x / 8, columns 8 and up are invalid; the columns
    before them have a small positive w: valid, far away, clamped or filled."""
    img = random_frame(10, 13, 5)
    h = [1, 0, 0, 0, 1, 0, -0.125, 0, 1]
    got, mask = check(img[None], [h], 13, 5, border=border, fill=200)
    assert (got[0][:, 8:] == 200).all() and not mask[0][:, 5:].any() and mask[0][0, :5].all()
    # tiny positive w right beside the line
    h = [1, 0, 1, 0, 1, 1, -0.125, 0, 1 + 2.0 ** -40]
    check(img[None], [h], 13, 5, border=border, fill=200)
    check(img[None], [h], 3, 5, border=border, fill=200)
    # ... and one whose position is still within 2^19 pixels: column 8 lands at x = 2^18
    h = [0.125, 0, 0, 0, 0.125, 0, -0.125, 0, 1 + 2.0 ** -18]
    valid, X, _ = positions(h, 13, 5)
    assert valid[:, :9].all() and not valid[:, 9:].any() and X[0, 8] == 1 << 29
    _, mask = check(img[None], [h], 13, 5, border=border, fill=200)
    assert not mask[0][:, 8:].any()


DEGENERATE = {
    "zero": np.zeros(9),
    "nan": np.full(9, np.nan),
    "one_nan": [1, 0, 0, 0, 1, 0, 0, 0, np.nan],
    "inf_translation": [1, 0, np.inf, 0, 1, -np.inf, 0, 0, 1],
    "inf_scale": [np.inf, 0, 0, 0, -np.inf, 0, 0, 0, 1],
    "inf_w": [1, 0, 0, 0, 1, 0, 0, 0, np.inf],
    "minus_inf_w": [1, 0, 0, 0, 1, 0, -np.inf, 0, 1],
    "huge": [1e300, 1e300, 0, -1e300, 1e300, 0, 0, 0, 1],
    "huge_over_tiny": [1e300, 0, 1e300, 0, 1e300, 1e300, 0, 0, 1e-300],
    "huge_w": [1, 0, 0, 0, 1, 0, 1e300, 1e300, 1e300],
    "negative_h8": [1, 0, 0, 0, 1, 0, 0, 0, -1],
    "negative_h8_positive_later": [1, 0, 0, 0, 1, 0, 0.25, 0, -1],
    "h8_of_4": [4, 0, 0, 0, 4, 0, 0, 0, 4],
    # FX lands on 2^30 at x = 0 and on 2^30 + 1 at x = 1; FY the same down the rows
    "limit_plus": [1 / 2048, 0, 524288, 0, 1 / 2048, 524288, 0, 0, 1],
    "limit_minus": [-1 / 2048, 0, -524288, 0, -1 / 2048, -524288, 0, 0, 1],
    "beyond_plus": [1, 0, 524288 + 1 / 2048, 0, 1, 0, 0, 0, 1],
    "beyond_minus": [1, 0, 0, 0, -1, -524288 - 1 / 2048, 0, 0, 1],
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_models(name):
    img = random_frame(11, 13, 7)
    h = DEGENERATE[name]
    for dst in ((13, 7), (2, 7)):
        for border in (REPLICATE, CONSTANT):
            got, mask = check(img[None], [h], *dst, border=border, fill=99)
            if name in ("zero", "nan", "one_nan", "negative_h8", "minus_inf_w", "beyond_plus",
                        "beyond_minus", "inf_translation"):
                assert (got == 99).all() and not mask.any()
    if name.startswith("limit"):
        valid, X, _ = positions(h, 13, 7)
        assert valid[0, 0] and abs(int(X[0, 0])) == 1 << 30 and not valid[0, 1:].any() and \
            not valid[1:].any()
    if name == "h8_of_4":
        assert np.array_equal(run_warp(img[None], [h], 13, 7)[0][0], img)


# ---- 3: exact identities -------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(7, 7), (67, 9), (3, 11)])
def test_identity_is_a_copy(size):
    img = random_frame(3, *size)
    for border in (REPLICATE, CONSTANT):
        got, mask = run_warp(img[None], [IDENTITY], *size, border=border, fill=9)
        assert np.array_equal(got[0], img) and mask.all()


def test_integer_shift_is_exact():
    img = random_frame(2, 40, 30)
    got, mask = run_warp(img[None], [[1, 0, 3, 0, 1, 5, 0, 0, 1]], 40, 30, border=CONSTANT, fill=7)
    want = np.full((30, 40), 7, np.uint8)
    want[:25, :37] = img[5:, 3:]
    assert np.array_equal(got[0], want)
    assert mask[0][:25, :37].all() and not mask[0][25:].any() and not mask[0][:, 37:].any()


def test_half_pixel_shift_is_the_rounded_mean():
    img = random_frame(3, 33, 9)
    got, _ = run_warp(img[None], [[1, 0, 0.5, 0, 1, 0, 0, 0, 1]], 33, 9)
    wide = img.astype(np.int64)
    assert np.array_equal(got[0], (wide + wide[:, np.minimum(np.arange(33) + 1, 32)] + 1) >> 1)


@pytest.mark.parametrize("dst", [(31, 19), (75, 50), (2, 7)])
def test_constant_frame_stays_constant_under_replicate(dst):
    for value in (0, 255):
        full = np.full((23, 37), value, np.uint8)
        for h in (rotation((37, 23), dst), zoom_out((37, 23), dst), mild_homography((37, 23), dst)):
            assert (run_warp(full[None], [h], *dst, fill=value)[0] == value).all()


# ---- 4: batches ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [9, 11])
@pytest.mark.parametrize("dst", [(62, 26), (3, 9)])
def test_batch_with_gaps_on_both_sides(dst, cols):
    w, h = 75, 31
    frames = np.stack([random_frame(7 + k, w, h) for k in range(3)])
    models = [rotation((w, h), dst), mild_homography((w, h), dst), np.zeros(9)]
    for border in (REPLICATE, CONSTANT):
        got, _ = check(frames, models, *dst, border=border, fill=33, in_stride=w * h + 13,
                       out_stride=dst[0] * dst[1] + 50, lead_in=3, lead_out=1, cols=cols)
        assert (got[2] == 33).all()                      # no model: a constant fill frame


@pytest.mark.parametrize("lead", [1, 3])
def test_unaligned_bases(lead):
    for src, dst in (((64, 24), (53, 20)), ((67, 9), (56, 8)), ((5, 4), (3, 3))):
        img = random_frame(lead, *src)
        check(img[None], [mild_homography(src, dst)], *dst, lead_in=lead, lead_out=4 - lead)


def grid_pair(shifts):
    """One 6 x 6 grid of query points per shift; trains = queries + shift; identity matches."""
    gx, gy = np.meshgrid(np.arange(6) * 6 + 2, np.arange(6) * 4 + 1)
    q1 = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.uint32)
    q = np.concatenate([q1 for _ in shifts])
    t = np.concatenate([q1 + np.uint32(s) for s in shifts])
    matches = np.zeros(len(q), dtype=fast_hip.MATCH_DTYPE)
    matches["index"] = np.arange(len(q))
    offs = np.arange(len(shifts) + 1) * 36
    return q, t, matches, offs


def test_models_straight_from_refine_device():
    """fdf_ransac_device -> fdf_refine_device -> fdf_warp_device on one stream; the record tensor
    goes in as it is (88 bytes apart).  The last frame has no correspondences: no model, fill."""
    import torch

    shifts = [(3, 5), (1, 0), (0, 2)]
    q, t, matches, offs = grid_pair(shifts)
    offs = np.append(offs, offs[-1])                     # a fourth frame without points
    n = 4
    d_m = torch.from_numpy(matches.view(np.int32).reshape(-1, 2).copy()).cuda()
    d_q = torch.from_numpy(q.view(np.int32).copy()).cuda()
    d_t = torch.from_numpy(t.view(np.int32).copy()).cuda()
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    models = torch.zeros((n, 11), dtype=torch.float64, device="cuda")
    need = max(fast_hip.ransac_scratch_bytes(n, len(q), 64), fast_hip.refine_scratch_bytes(n, len(q)))
    raw = torch.zeros((need + 256,), dtype=torch.uint8, device="cuda")
    lead = (-raw.data_ptr()) % 256
    scratch = raw[lead:lead + need]
    frames = np.stack([random_frame(40 + k, 40, 30) for k in range(n)])
    _, d_in = strided(torch, n, 30, 40, 1200 + 8, 2)
    d_in.copy_(torch.from_numpy(frames).cuda())
    flat_out, d_out = strided(torch, n, 30, 40, 1200 + 24, 5)
    flat_mask, d_mask = strided(torch, n, 30, 40, 1200 + 24, 5)
    fast_hip.ransac_device(d_m, d_o, d_q, d_t, d_o, models, scratch, model="affine", n_hyp=64,
                           threshold=1.0, seed=0)
    fast_hip.refine_device(d_m, d_o, d_q, d_t, d_o, models, models, scratch, model="affine",
                           threshold=1.0, n_rounds=1)
    fast_hip.warp_device(d_in, models, d_out, border="constant", fill=77, mask=d_mask)
    torch.cuda.synchronize()
    rec = fast_hip.unpack_models(models.cpu().numpy())
    assert rec["hypothesis"][3] == fast_hip.RANSAC_NONE and (rec["hypothesis"][:3] != fast_hip.RANSAC_NONE).all()
    got, got_mask = d_out.cpu().numpy(), d_mask.cpu().numpy()
    for k in range(n):
        want, want_mask = warp(frames[k], rec["h"][k], 40, 30, CONSTANT, 77)
        assert np.array_equal(got[k], want) and np.array_equal(got_mask[k], want_mask), k
    assert (got[3] == 77).all() and not got_mask[3].any()
    for k, (sx, sy) in enumerate(shifts):                # the planted shifts come out exactly
        assert np.array_equal(rec["h"][k], [1, 0, sx, 0, 1, sy, 0, 0, 1])
        assert np.array_equal(got[k][:30 - sy, :40 - sx], frames[k][sy:, sx:])
    d_out.fill_(GAP)
    d_mask.fill_(GAP)
    assert (flat_out == GAP).all() and (flat_mask == GAP).all()
    assert np.array_equal(d_in.cpu().numpy(), frames)


# ---- 5: the chain, exact --------------------------------------------------------------------------

def test_estimate_then_warp_then_warp_back():
    q, t, matches, _ = grid_pair([(3, 5)])
    H, inliers, rec = fast_hip.estimate_model(q, t, matches, model="affine", refine_rounds=1)
    assert inliers.all() and np.array_equal(H.reshape(9), [1, 0, 3, 0, 1, 5, 0, 0, 1])
    b = random_frame(50, 40, 30)
    onto_a, mask = fast_hip.warp_array(b, (H, inliers, rec), mask=True)
    assert onto_a.shape == (30, 40) and np.array_equal(onto_a[:25, :37], b[5:, 3:])
    assert mask[:25, :37].all() and not mask[25:].any() and not mask[:, 37:].any()
    assert np.array_equal(onto_a, warp(b, H, 40, 30)[0])
    inv = fast_hip.model_invert(H)
    assert np.array_equal(inv.reshape(9), [1, 0, -3, 0, 1, -5, 0, 0, 1])
    assert inv.tobytes() == model_invert(H).tobytes()
    back = fast_hip.warp_array(onto_a, inv)
    assert np.array_equal(back[5:, 3:], b[5:, 3:])                        # the overlap


# ---- 6: the host entry ----------------------------------------------------------------------------

def test_warp_array_and_strided_host_rows():
    img = random_frame(31, 97, 61)
    for dst in ((81, 51), (97, 61), (3, 25)):
        for kind in sorted(MODELS):
            h = MODELS[kind]((97, 61), dst)
            want, want_mask = warp(img, h, *dst, CONSTANT, 5)
            got, mask = fast_hip.warp_array(img, h.reshape(3, 3), (dst[1], dst[0]), border="constant",
                                            fill=5, mask=True)
            assert np.array_equal(got, want) and mask.dtype == np.bool_
            assert np.array_equal(mask, want_mask.astype(bool))
            assert np.array_equal(fast_hip.warp_array(img, h, (dst[1], dst[0])),
                                  warp(img, h, *dst)[0])
    wide = random_frame(32, 120, 61)
    h = rotation((97, 61), (97, 61))
    assert np.array_equal(fast_hip.warp_array(wide[:, 5:102], h), warp(wide[:, 5:102], h, 97, 61)[0])
    # host rows further apart on the output side, pixels and mask alike
    lib = _native.load()
    out = np.full((51, 90), GAP, np.uint8)
    mask = np.full((51, 90), GAP, np.uint8)
    src = np.ascontiguousarray(wide[:, 5:102])
    h = np.ascontiguousarray(mild_homography((97, 61), (81, 51)))
    rc = lib.fdf_warp_frame(fast_hip.context(0).handle, wide[:, 5:].ctypes.data, 97, 61, 120,
                            h.ctypes.data, out.ctypes.data, 81, 51, 90, REPLICATE, 0,
                            mask.ctypes.data)
    assert rc == _native.FDF_OK
    want, want_mask = warp(src, h, 81, 51)
    assert np.array_equal(out[:, :81], want) and np.array_equal(mask[:, :81], want_mask)
    assert (out[:, 81:] == GAP).all() and (mask[:, 81:] == GAP).all()


def test_warp_frame_keeps_the_retained_result(golden):
    """fdf_warp_frame leaves the context's retained detection alone: fdf_fetch_last still
    returns it."""
    img, _, maxt = golden
    lib = _native.load()
    ctx = fast_hip.context(0)
    cfg = _native.FdfConfig(16, 9, 1)
    few = np.zeros((4, 2), dtype=np.uint32)
    n = ctypes.c_size_t(0)
    h = rotation((300, 200), (300, 200), 5.0)
    with ctx.lock:
        rc = lib.fdf_detect(ctx.handle, img.ctypes.data, img.shape[1], img.shape[0],
                            img.strides[0], ctypes.byref(cfg), few.ctypes.data, 4,
                            ctypes.byref(n))
        assert rc == _native.FDF_ERR_CAPACITY and n.value == len(maxt)
        assert np.array_equal(fast_hip.warp_array(img, h), warp(img, h, 300, 200)[0])
        out = np.zeros((n.value, 2), dtype=np.uint32)
        rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data, None, n.value, ctypes.byref(n))
    assert rc == _native.FDF_OK and np.array_equal(out, maxt)


def test_cpp_smoke_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "test_cpp_warp")
    assert os.path.exists(exe), "run `make` first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout


# ---- 7: rejected calls ----------------------------------------------------------------------------

def test_rejected_calls():
    """What fdf_warp_device must reject, synchronously and with nothing launched: the output and
    the mask keep their fill."""
    import torch

    lib = _native.load()
    ctx = fast_hip.context(0).handle
    src = torch.full((3 * 64,), 1, dtype=torch.uint8, device="cuda")
    dst = torch.full((3 * 16,), GAP, dtype=torch.uint8, device="cuda")
    msk = torch.full((3 * 16,), GAP, dtype=torch.uint8, device="cuda")
    mod = device_models(torch, [IDENTITY] * 3, 11)
    packed = device_models(torch, [IDENTITY] * 3, 9)
    s, d, k, m = src.data_ptr(), dst.data_ptr(), msk.data_ptr(), mod.data_ptr()

    def call(d_src=s, n=3, sw=8, sh=8, ss=64, models=m, ms=88, d_dst=d, dw=4, dh=4, ds=16,
             border=0, fill=0, mask=k, c=ctx):
        return lib.fdf_warp_device(c, d_src, n, sw, sh, ss, models, ms, d_dst, dw, dh, ds, border,
                                   fill, mask, None)

    A, S = _native.FDF_ERR_ARG, _native.FDF_ERR_SIZE
    assert call(c=None) == A
    assert call(d_src=None) == A and call(d_dst=None) == A and call(models=None) == A
    assert call(n=65536) == A
    assert call(ss=63) == A and call(ds=15) == A              # frames closer than their size
    assert call(ms=64) == A and call(ms=76) == A and call(ms=0) == A      # short, misaligned
    assert call(models=m + 4) == A                            # not 8-byte aligned
    assert call(border=2) == A and call(fill=256) == A
    assert call(n=0, border=2) == A and call(n=0, ms=71) == A
    assert call(sw=0) == S and call(sh=0) == S and call(dw=0) == S and call(dh=0) == S
    assert call(sw=65535, sh=65535) == S                      # above 2^31 - 256 pixels
    assert call(dw=65536, dh=65536) == S
    assert call(sw=65536, sh=1) == S                          # a source side above 65535
    assert call(n=0) == _native.FDF_OK
    assert call(n=0, d_src=None, d_dst=None, models=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (dst == GAP).all() and (msk == GAP).all()
    assert call(n=1, ss=0, ds=0, mask=None) == _native.FDF_OK # one frame: the strides are not read
    torch.cuda.synchronize()
    assert (dst[:16] == 1).all() and (dst[16:] == GAP).all() and (msk == GAP).all()
    assert call(models=packed.data_ptr(), ms=72, mask=None) == _native.FDF_OK
    torch.cuda.synchronize()
    assert (dst == 1).all() and (msk == GAP).all()

    # fdf_warp_frame: the shape and pointer errors leave the host output alone
    img = np.ones((8, 8), np.uint8)
    out = np.full((4, 4), GAP, np.uint8)
    h = np.float64(IDENTITY)

    def frame(data=img.ctypes.data, w=8, hh=8, stride=8, model=h.ctypes.data, o=out.ctypes.data,
              dw=4, dh=4, os_=4, border=0, fill=0, c=ctx):
        return lib.fdf_warp_frame(c, data, w, hh, stride, model, o, dw, dh, os_, border, fill, None)

    for bad in (dict(c=None), dict(data=None), dict(model=None), dict(o=None), dict(stride=7),
                dict(os_=3), dict(border=2), dict(fill=256)):
        assert frame(**bad) == A, bad
    for bad in (dict(w=0), dict(hh=0), dict(dw=0), dict(dh=0), dict(w=65536, hh=1)):
        assert frame(**bad) == S, bad
    assert (out == GAP).all()
    assert frame() == _native.FDF_OK and (out == 1).all()
