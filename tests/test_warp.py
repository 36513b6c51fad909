"""CPU tests of the warp's host side: the numpy restatement of include/fdf.h's rules
(tests/_warp_reference.py) against independent formulations, fdf_model_invert against the
restatement bit for bit, and the argument checks that run before any device call."""
import ctypes

import numpy as np
import pytest

from _warp_reference import CONSTANT, REPLICATE, model_invert, positions, warp
from feature_detector_fast_amd import FdfError, _native, fast_hip

A = _native.FDF_ERR_ARG
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]
EXAMPLE = [0.75, 0.25, 0.5, -0.25, 0.75, 1, 0.0625, 0, 1]          # include/fdf.h's example
AFFINE = [0.8, -0.6, 12.25, 0.6, 0.8, -3.5, 0, 0, 1]


def random_frame(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- the restatement against independent formulations -------------------------------------------

@pytest.mark.parametrize("border", [REPLICATE, CONSTANT])
def test_identity_is_a_copy(border):
    img = random_frame(1, 37, 23)
    out, mask = warp(img, IDENTITY, 37, 23, border, 9)
    assert np.array_equal(out, img) and mask.all()
    # h8 is used as given: a model scaled by 4 is the same map
    out, mask = warp(img, [4 * v for v in IDENTITY], 37, 23, border, 9)
    assert np.array_equal(out, img) and mask.all()


def test_integer_shift_is_array_slicing():
    img = random_frame(2, 40, 30)
    out, mask = warp(img, [1, 0, 3, 0, 1, 5, 0, 0, 1], 40, 30, CONSTANT, 7)
    want = np.full((30, 40), 7, np.uint8)
    want[:25, :37] = img[5:, 3:]
    assert np.array_equal(out, want)
    inside = np.zeros((30, 40), np.uint8)
    inside[:25, :37] = 1
    assert np.array_equal(mask, inside)
    # replicate: the last row and column repeat; a negative shift repeats the first ones
    out, _ = warp(img, [1, 0, 3, 0, 1, 5, 0, 0, 1], 40, 30)
    assert np.array_equal(out, img[np.minimum(np.arange(30) + 5, 29)][:, np.minimum(np.arange(40) + 3, 39)])
    out, mask = warp(img, [1, 0, -2, 0, 1, -4, 0, 0, 1], 40, 30)
    assert np.array_equal(out, img[np.maximum(np.arange(30) - 4, 0)][:, np.maximum(np.arange(40) - 2, 0)])
    assert mask[4:, 2:].all() and not mask[:4].any() and not mask[:, :2].any()


def test_half_pixel_shift_is_the_rounded_mean():
    img = random_frame(3, 33, 9).astype(np.int64)
    out, mask = warp(img.astype(np.uint8), [1, 0, 0.5, 0, 1, 0, 0, 0, 1], 33, 9)
    right = img[:, np.minimum(np.arange(33) + 1, 32)]
    assert np.array_equal(out, (img + right + 1) >> 1)
    assert mask[:, :32].all() and not mask[:, 32].any()


@pytest.mark.parametrize("s,d", [(37, 31), (20, 47), (64, 25)])
def test_pure_scale_of_a_constant_frame(s, d):
    """h = S/D 0 0 0 S/D 0 0 0 1 of a constant frame: constant under replicate; under constant the
    pixels whose four taps lie inside the frame keep the value."""
    for value in (0, 255, 77):
        img = np.full((s, s), value, np.uint8)
        h = [s / d, 0, 0, 0, s / d, 0, 0, 0, 1]
        out, _ = warp(img, h, d, d)
        assert (out == value).all()
        out, _ = warp(img, h, d, d, CONSTANT, 3)
        valid, X, Y = positions(h, d, d)
        inner = valid & ((X >> 11) + 1 <= s - 1) & ((Y >> 11) + 1 <= s - 1)
        assert inner.any() and (out[inner] == value).all()


def test_header_example():
    img = (16 * (4 * np.arange(4)[:, None] + np.arange(4)[None, :])).astype(np.uint8)
    out, mask = warp(img, EXAMPLE, 4, 4, CONSTANT, 255)
    assert out.tolist() == [[72, 64, 57, 51], [124, 113, 103, 94], [176, 162, 149, 138],
                            [223, 211, 196, 182]]
    assert mask.tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1]]


def test_invalid_pixels_get_the_fill():
    img = random_frame(4, 13, 5)
    for h in (np.zeros(9), np.full(9, np.nan), [1, 0, 0, 0, 1, 0, 0, 0, -1],
              [1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e-300]):
        for border in (REPLICATE, CONSTANT):
            out, mask = warp(img, h, 13, 5, border, 200)
            if np.asarray(h, dtype=np.float64)[0] == 1e300:        # pixel (0, 0) maps to (0, 0)
                assert out[0, 0] == img[0, 0] and (out.ravel()[1:] == 200).all()
            else:
                assert (out == 200).all() and not mask.any()
    # the line w = 0 inside the destination: columns 8 and up are invalid; columns 5 to 7 are
    # valid and lie right of the frame (x / (1 - x / 8) > 12), where replicate repeats the edge
    out, mask = warp(img, [1, 0, 0, 0, 1, 0, -0.125, 0, 1], 13, 5, REPLICATE, 200)
    assert (out[:, 8:] == 200).all() and not mask[:, 5:].any() and mask[0, :5].all()
    assert (out[0, 5:8] == img[0, 12]).all()


# ---- fdf_model_invert --------------------------------------------------------------------------

def c_invert(h, in_place=False):
    src = np.array(h, dtype=np.float64).reshape(9)
    out = src if in_place else np.full(9, -7.0)
    rc = _native.load().fdf_model_invert(src.ctypes.data, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("h", [IDENTITY, EXAMPLE, AFFINE, [2, 0, 0, 0, 4, 0, 0, 0, 8],
                               [1.02, 0.03, -4.5, -0.02, 0.97, 3.25, 0.0004, -0.0003, 1]])
def test_model_invert_equals_the_restatement(h):
    want = model_invert(h)
    for in_place in (False, True):
        rc, got = c_invert(h, in_place)
        assert rc == _native.FDF_OK
        assert got.tobytes() == want.tobytes()
    assert fast_hip.model_invert(h).tobytes() == want.tobytes()
    assert fast_hip.model_invert(np.array(h).reshape(3, 3)).shape == (3, 3)
    assert want[8] == 1.0


def test_model_invert_worked_values():
    assert np.array_equal(model_invert(IDENTITY), np.float64(IDENTITY))
    assert np.array_equal(model_invert([1, 0, 3, 0, 1, 5, 0, 0, 1]), [1, 0, -3, 0, 1, -5, 0, 0, 1])
    # the example's determinant c8 is 0.625
    assert np.allclose(model_invert(EXAMPLE), [1.2, -0.4, -0.2, 0.5, 1.15, -1.4, -0.075, 0.025, 1],
                       rtol=1e-15, atol=0)


@pytest.mark.parametrize("h", [np.zeros(9), [1, 2, 3, 2, 4, 6, 0, 0, 1], [0, 1, 0, 0, 0, 1, 1, 0, 0],
                               np.full(9, np.nan), [np.inf, 0, 0, 0, 1, 0, 0, 0, 1]])
def test_model_invert_rejects_a_singular_matrix(h):
    """Every case has c8 = h0 h4 - h1 h3 = 0 or not finite: no inverse with out[8] = 1 (the third
    one is a permutation, whose inverse has a zero there)."""
    assert model_invert(h) is None
    rc, out = c_invert(h)
    assert rc == A and (out == -7.0).all()               # out untouched
    src = np.array(h, dtype=np.float64)
    rc, out = c_invert(src, in_place=True)
    assert rc == A and out.tobytes() == src.tobytes()
    with pytest.raises(FdfError) as e:
        fast_hip.model_invert(h)
    assert e.value.status == A


def test_model_invert_null_pointers():
    lib = _native.load()
    buf = np.float64(IDENTITY)
    assert lib.fdf_model_invert(None, buf.ctypes.data) == A
    assert lib.fdf_model_invert(buf.ctypes.data, None) == A


@pytest.mark.parametrize("h", [EXAMPLE, AFFINE, [1.02, 0.03, -4.5, -0.02, 0.97, 3.25, 0.0004, -0.0003, 1]])
def test_inverting_twice_comes_back_within_rounding(h):
    """Not a bit claim.  An entry of the adjugate is a difference of two rounded products and a
    quotient: a few eps relative to the products, which the division by the determinant scales by
    at most the condition number k relative to the largest entry.  Two inversions: an error of
    at most some tens of eps k^2 max|h| per entry; 256 eps k^2 max|h| is the bound, and the
    library's second inverse is the restatement's bit for bit."""
    h = np.float64(h)
    back = model_invert(model_invert(h))
    rc, once = c_invert(h)
    rc2, twice = c_invert(once)
    assert rc == rc2 == _native.FDF_OK and twice.tobytes() == back.tobytes()
    k = np.linalg.cond(h.reshape(3, 3))
    tol = 256 * np.finfo(np.float64).eps * k * k * np.abs(h).max()
    err = np.abs(back - h).max()
    print(f"cond {k:.3g} error {err:.3g} bound {tol:.3g}")
    assert err <= tol


# ---- argument checks before any device call --------------------------------------------------

def test_exports_and_constants():
    assert {"fdf_warp_device", "fdf_warp_frame", "fdf_model_invert"} <= set(_native.EXPORTED_SYMBOLS)
    assert {"warp_device", "warp_array", "model_invert"} <= set(fast_hip.__all__)
    lib = _native.load()
    for name in ("fdf_warp_device", "fdf_warp_frame", "fdf_model_invert"):
        assert hasattr(lib, name)
    assert (_native.FDF_BORDER_REPLICATE, _native.FDF_BORDER_CONSTANT) == (REPLICATE, CONSTANT)
    assert ctypes.sizeof(_native.FdfModel) == 88 and _native.FdfModel.h.offset == 0


def test_c_entries_reject_a_null_context_before_any_device_call():
    lib = _native.load()
    p = ctypes.c_void_p(4096)                            # never dereferenced: no context
    assert lib.fdf_warp_device(None, p, 1, 8, 8, 64, p, 72, p, 4, 4, 16, 0, 0, None, None) == A
    assert lib.fdf_warp_device(None, p, 0, 8, 8, 64, p, 72, p, 4, 4, 16, 0, 0, None, None) == A
    h = np.float64(IDENTITY)
    assert lib.fdf_warp_frame(None, p, 8, 8, 8, h.ctypes.data, p, 4, 4, 4, 0, 0, None) == A


def test_wrapper_argument_checks():
    import torch

    f = torch.zeros((2, 8, 8), dtype=torch.uint8)
    out = torch.zeros((2, 4, 6), dtype=torch.uint8)
    m9 = torch.zeros((2, 9), dtype=torch.float64)
    m11 = torch.zeros((2, 11), dtype=torch.float64)
    good = dict(frames=f, models=m9, out=out)
    for bad in (dict(out=torch.zeros((3, 4, 6), dtype=torch.uint8)),             # frame counts
                dict(out=out.to(torch.int32)), dict(out=torch.zeros((2, 4, 0), dtype=torch.uint8)),
                dict(out=f[:, :4, :6]),                                          # not contiguous
                dict(models=m9.to(torch.float32)), dict(models=m9[:1]),
                dict(models=torch.zeros((2, 10), dtype=torch.float64)),
                dict(models=m11[:, :9]), dict(models=m9.reshape(-1)),
                dict(border="reflect"), dict(border=1), dict(fill=256), dict(fill=-1),
                dict(mask=torch.zeros((2, 4, 5), dtype=torch.uint8)),
                dict(mask=torch.zeros((2, 4, 6), dtype=torch.bool)),
                dict(mask=torch.zeros((2, 5, 6), dtype=torch.uint8)[:, :4])):    # another stride
        with pytest.raises(ValueError):
            fast_hip.warp_device(**{**good, **bad})
    # every check passed: the call gets as far as the device check
    for ok in (dict(), dict(models=m11), dict(border="constant", fill=255),
               dict(mask=torch.zeros_like(out))):
        with pytest.raises(ValueError, match="CUDA"):
            fast_hip.warp_device(**{**good, **ok})

    img = np.zeros((20, 30), dtype=np.uint8)
    for bad in (dict(shape=(0, 5)), dict(shape=(1 << 16, 1 << 16)), dict(border="wrap"),
                dict(fill=300)):
        with pytest.raises(ValueError):
            fast_hip.warp_array(img, IDENTITY, **bad)
    for bad_h in (np.zeros(8), np.zeros((3, 4)), "model", [object()] * 9):
        with pytest.raises(TypeError):
            fast_hip.warp_array(img, bad_h)
    with pytest.raises(TypeError):
        fast_hip.warp_array(img, IDENTITY, shape=5)
    with pytest.raises(TypeError):
        fast_hip.warp_array(img.astype(np.float32), IDENTITY)
    with pytest.raises(TypeError):
        fast_hip.model_invert(np.zeros(4))


def test_host_model_forms():
    """Nine numbers, a 3 x 3 array, a record and estimate_model's triple all name one model."""
    rec = np.zeros(1, dtype=fast_hip.MODEL_DTYPE)
    rec["h"][0] = EXAMPLE
    want = np.float64(EXAMPLE)
    for form in (EXAMPLE, tuple(EXAMPLE), np.float64(EXAMPLE).reshape(3, 3), rec, rec[0],
                 (np.float64(EXAMPLE).reshape(3, 3), np.zeros(4, bool), rec[0]),
                 (None, np.zeros(4, bool), rec[0], 2), np.float32(IDENTITY), np.int64(IDENTITY)):
        got = fast_hip._host_model(form)
        assert got.dtype == np.float64 and got.shape == (9,) and got.flags.c_contiguous
        assert np.array_equal(got, want) or np.array_equal(got, np.float64(IDENTITY))
