"""The HIP detector: drop-in for the reference's ``fast_simd`` module (src/fast_simd.rs).

``detector(img, config)`` replaces ``fast_simd::detector`` (src/fast_simd.rs:847-859) and
returns ``list[Point]`` in raster order.  Array and batched variants return numpy arrays;
``detect_device`` keeps everything in HBM (torch CUDA tensors) for throughput.
"""
import collections
import ctypes
import threading

import numpy as np

from . import _native
from ._native import FdfConfig, FdfError, check
from .types import Config, GrayImage, NonMaximalSuppression, Point

# src/fast_simd.rs:69-72
NORTH = 0
EAST = 4
SOUTH = 8
WEST = 12

_CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
           (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))


def circle():
    """The 16-pixel Bresenham circle, index 0 north then clockwise (src/fast_simd.rs:79-98)."""
    return list(_CIRCLE)


def calculate_offsets(width):
    """Row-major memory offsets of the circle points (src/fast_simd.rs:104-110)."""
    return [dy * int(width) + dx for dx, dy in _CIRCLE]


_ctx_lock = threading.Lock()
_contexts = {}
_shard_contexts = {}


def context(device=0):
    """The process-wide :class:`_native.Context` for ``device`` (created on first use)."""
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = _native.Context(device)
            ctx.lock = threading.Lock()     # holds a two-call pattern together
            _contexts[device] = ctx
        return ctx


def shard_contexts(devices):
    """One distinct context per entry of ``devices`` (a device listed twice gets two
    contexts), for :func:`detector_batch` over several devices."""
    out, seen = [], {}
    with _ctx_lock:
        for dev in devices:
            k = seen.get(dev, 0)
            seen[dev] = k + 1
            ctx = _shard_contexts.get((dev, k))
            if ctx is None:
                ctx = _native.Context(dev)
                ctx.lock = threading.Lock()
                _shard_contexts[(dev, k)] = ctx
            out.append(ctx)
    return out


def _to_c_config(config):
    if not isinstance(config, Config):
        raise TypeError("config must be a feature_detector_fast_amd.Config")
    for name, v in (("threshold", config.threshold), ("count", config.count)):
        if not 0 <= int(v) <= 255:
            raise ValueError(f"{name} must fit in u8")
    nms = int(config.non_maximal_supression)
    if not 0 <= nms <= 255:
        raise FdfError(_native.FDF_ERR_NMS, "config")
    return FdfConfig(int(config.threshold), int(config.count), nms)


def _as_pixels(img):
    if isinstance(img, GrayImage):
        arr = img.array()
    else:
        arr = np.asarray(img)
    if arr.ndim != 2:
        raise ValueError("expected a 2-D grayscale image (H, W)")
    if arr.dtype != np.uint8:
        raise TypeError("expected uint8 pixels")
    if arr.strides[1] != 1:
        arr = np.ascontiguousarray(arr)
    return arr


def _host_points(points):
    """``points`` as a contiguous (K, 2) uint32 array."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "ui":
        raise TypeError("points must be a (K, 2) integer array")
    if pts.size and (pts.min() < 0 or pts.max() > 0xffffffff):
        raise ValueError("points must fit u32")
    return np.ascontiguousarray(pts, dtype=np.uint32)


# Argument checks of the device entries (torch tensors).

def _check_points(t, name="points", rows="cap"):
    if t.dim() != 2 or t.shape[1] != 2 or t.element_size() != 4 or not t.is_contiguous() \
            or t.is_floating_point():
        raise ValueError(f"{name} must be a contiguous ({rows}, 2) 32-bit integer tensor")


def _check_offsets(torch, t, n, name="offsets", one_dim=True):
    if t.dtype != torch.int64 or (one_dim and t.dim() != 1) or not t.is_contiguous() or \
            t.numel() < n:
        raise ValueError(f"{name} must be a contiguous int64 tensor with F+1 entries")


def _check_angles(torch, t, cap):
    if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < cap or not t.is_contiguous():
        raise ValueError("angles must be a contiguous float32 tensor with cap entries")


def _check_frames(torch, t, name="frames"):
    """(F, H, W) uint8 with contiguous frames any number of bytes apart."""
    if t.dim() != 3 or t.dtype != torch.uint8 or (
            t.numel() and (t.stride(2) != 1 or t.stride(1) != t.shape[2] or
                           (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.shape[2]))):
        raise ValueError(f"{name} must be a (F, H, W) uint8 tensor of contiguous frames")


def _frame_args(t):
    """(pointer, F, width, height, frame stride in bytes) of a _check_frames tensor."""
    f, h, w = t.shape
    return t.data_ptr(), f, w, h, t.stride(0) if f > 1 else h * w


def _check_one_device(where, tensors):
    if not all(t.is_cuda for t in tensors) or len({t.device for t in tensors}) != 1:
        raise ValueError(f"{where} needs CUDA (HIP) tensors on one device")


def _device_stream(torch, t, device, stream):
    """(device index, stream) of a call: ``t``'s device and torch's current stream by default."""
    return (t.device.index if device is None else device,
            torch.cuda.current_stream(t.device) if stream is None else stream)


def capacity_guess(pixels):
    """First output capacity of the two-call pattern: 1 keypoint per 64 pixels (real images
    have 0.5-1.5 per 100; denser results are fetched with fdf_fetch_last, not recomputed)."""
    return max(4096, int(pixels) // 64)


def _two_call(ctx, pixels, call, where, scored=False):
    """Run ``call(out_ptr, scores_ptr, cap, n_ref)`` with a guessed capacity; on
    FDF_ERR_CAPACITY copy the retained device result out with fdf_fetch_last (the detection
    runs once either way)."""
    lib = _native.load()
    cap = capacity_guess(pixels)
    out = np.empty((cap, 2), dtype=np.uint32)
    scores = np.empty(cap, dtype=np.uint16) if scored else None
    n = ctypes.c_size_t(0)
    with ctx.lock:
        rc = call(out.ctypes.data, scores.ctypes.data if scored else None, cap, n)
        if rc == _native.FDF_ERR_CAPACITY:
            out = np.empty((n.value, 2), dtype=np.uint32)
            scores = np.empty(n.value, dtype=np.uint16) if scored else None
            rc = lib.fdf_fetch_last(ctx.handle, out.ctypes.data,
                                    scores.ctypes.data if scored else None, n.value,
                                    ctypes.byref(n))
            where = "fdf_fetch_last"
    check(rc, where)
    k = n.value
    return (out[:k], scores[:k]) if scored else out[:k]


def detect_array(img, config, device=0):
    """Keypoints as a (K, 2) uint32 array of (x, y) rows in raster order."""
    arr = _as_pixels(img)
    cfg = _to_c_config(config)
    h, w = arr.shape
    ctx = context(device)
    lib = _native.load()
    stride = arr.strides[0] if arr.size else w
    ptr = arr.ctypes.data if arr.size else None
    return _two_call(ctx, w * h, lambda o, _s, cap, n: lib.fdf_detect(
        ctx.handle, ptr, w, h, stride, ctypes.byref(cfg), o, cap, ctypes.byref(n)), "fdf_detect")


def detector(img, config):
    """Drop-in for fast_simd::detector: ``list[Point]`` in raster order."""
    return [Point(int(x), int(y)) for x, y in detect_array(img, config)]


def detect_rgb_array(rgb, config, device=0):
    """Keypoints of an RGB8 (H, W, 3) image: converted on the device as image 0.24.6's
    to_luma8 (what the reference's callers do, src/main.rs:58), then detected."""
    arr = np.asarray(rgb)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError("expected an (H, W, 3) uint8 RGB image")
    if arr.strides[1] != 3 or arr.strides[2] != 1:
        arr = np.ascontiguousarray(arr)
    cfg = _to_c_config(config)
    h, w = arr.shape[:2]
    ctx = context(device)
    lib = _native.load()
    stride = arr.strides[0] if arr.size else 3 * w
    ptr = arr.ctypes.data if arr.size else None
    return _two_call(ctx, w * h, lambda o, _s, cap, n: lib.fdf_detect_rgb(
        ctx.handle, ptr, w, h, stride, ctypes.byref(cfg), o, cap, ctypes.byref(n)),
        "fdf_detect_rgb")


def detector_rgb(rgb, config):
    """``list[Point]`` for an RGB8 image (luma conversion on the device)."""
    return [Point(int(x), int(y)) for x, y in detect_rgb_array(rgb, config)]


def rgb_to_luma(frames, out, stream=None, device=None):
    """Device-side RGB8 -> grey of torch uint8 CUDA tensors: ``frames`` (F, H, W, 3)
    contiguous, ``out`` (F, H, W).  Asynchronous on ``stream`` (default: torch's current)."""
    import torch

    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or \
            not frames.is_contiguous():
        raise ValueError("frames must be a contiguous (F, H, W, 3) uint8 tensor")
    if out.shape != frames.shape[:3] or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (F, H, W) uint8 tensor")
    if not frames.is_cuda or not out.is_cuda:
        raise ValueError("rgb_to_luma needs CUDA (HIP) tensors")
    dev, stream = _device_stream(torch, frames, device, stream)
    ctx = context(dev)
    f, h, w = frames.shape[:3]
    lib = _native.load()
    check(lib.fdf_rgb_to_luma_device(ctx.handle, frames.data_ptr(), f, w, h, 3 * w * h,
                                     out.data_ptr(), ctypes.c_void_p(stream.cuda_stream)),
          "fdf_rgb_to_luma_device")


def detector_batch(frames, config, device=0, devices=None):
    """Detect on a (F, H, W) uint8 stack.  Returns (points (K, 2) uint32, offsets (F+1,))
    where frame f's keypoints are points[offsets[f]:offsets[f+1]].

    ``devices``: a list of HIP device ids to shard the frames over (contiguous shards, one
    host thread and context per entry, results in frame order: fdf_detect_batch_multi).  A
    device may be listed more than once (several contexts on one GPU)."""
    frames = np.ascontiguousarray(np.asarray(frames), dtype=np.uint8)
    if frames.ndim != 3:
        raise ValueError("expected a (F, H, W) uint8 stack")
    f, h, w = frames.shape
    cfg = _to_c_config(config)
    lib = _native.load()
    offsets = np.zeros(f + 1, dtype=np.uint64)
    ptr = frames.ctypes.data if frames.size else None
    if devices is None:
        ctx = context(device)
        pts = _two_call(ctx, f * h * w, lambda o, _s, cap, n: lib.fdf_detect_batch(
            ctx.handle, ptr, f, w, h, h * w, ctypes.byref(cfg), o, cap, offsets.ctypes.data,
            ctypes.byref(n)), "fdf_detect_batch")
        return pts, offsets
    ctxs = shard_contexts(list(devices))
    handles = (ctypes.c_void_p * len(ctxs))(*[c.handle.value for c in ctxs])
    cap = capacity_guess(f * h * w)
    out = np.empty((cap, 2), dtype=np.uint32)
    n = ctypes.c_size_t(0)
    # one global lock order (by handle), whatever order the caller lists the devices in:
    # detector_batch(devices=[0, 1]) and devices=[1, 0] from two threads cannot deadlock
    locked = sorted(ctxs, key=lambda c: c.handle.value)
    for c in locked:
        c.lock.acquire()
    try:
        rc = lib.fdf_detect_batch_multi(handles, len(ctxs), ptr, f, w, h, h * w,
                                        ctypes.byref(cfg), out.ctypes.data, cap,
                                        offsets.ctypes.data, ctypes.byref(n))
        where = "fdf_detect_batch_multi"
        if rc == _native.FDF_ERR_CAPACITY:
            out = np.empty((n.value, 2), dtype=np.uint32)
            rc = lib.fdf_fetch_last_multi(handles, len(ctxs), out.ctypes.data, n.value,
                                          ctypes.byref(n))
            where = "fdf_fetch_last_multi"
    finally:
        for c in reversed(locked):
            c.lock.release()
    check(rc, where)
    return out[: n.value], offsets


def detect_device(frames, config, out, offsets, stream=None, device=None, ctx=None):
    """Enqueue detection on device-resident frames; nothing crosses PCIe.

    ``frames``: torch uint8 CUDA tensor (F, H, W), contiguous.  ``out``: int32/uint32 CUDA
    tensor (cap, 2).  ``offsets``: int64 CUDA tensor (F+1,).  Asynchronous on ``stream``
    (a torch.cuda.Stream; default: torch's current stream).  On completion
    offsets[F] holds the total (even when it exceeds ``cap``).  ``ctx``: the context whose
    workspace the call uses (default: the device's process-wide one; see :class:`Lanes`)."""
    import torch

    if frames.dim() != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous (F, H, W) uint8 tensor")
    if not frames.is_cuda or not out.is_cuda or not offsets.is_cuda:
        raise ValueError("detect_device needs CUDA (HIP) tensors")
    if offsets.dtype != torch.int64 or offsets.numel() < frames.shape[0] + 1:
        raise ValueError("offsets must be int64 with F+1 entries")
    if out.dim() != 2 or out.shape[1] != 2 or out.element_size() != 4 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (cap, 2) 32-bit tensor")
    dev, stream = _device_stream(torch, frames, device, stream)
    cfg = _to_c_config(config)
    if ctx is None:
        ctx = context(dev)
    f, h, w = frames.shape
    rc = _native.load().fdf_detect_device(
        ctx.handle, frames.data_ptr(), f, w, h, h * w, ctypes.byref(cfg), out.data_ptr(),
        out.shape[0], offsets.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_detect_device")


class Lanes:
    """``n`` launch lanes on one device for back-to-back device-resident batches: lane i is a
    context of its own (workspace: band slots, counts, sums) and the HIP stream that context
    created.  Call k goes to lane k % n with no dependency on the other lanes, so one call's
    detector runs beside the previous calls' last workgroups and compaction: with n = 3, 512
    1080p frames take 0.391 ms per call against 0.442 ms on one stream.

    Ordering: with ``after_current=True`` (default) each call first makes its lane wait for
    the work already enqueued on torch's current stream (the producer of ``frames``), and
    :meth:`wait` makes the current stream wait for a lane's last call (before reading its
    ``out`` / ``offsets``).  Each lane needs its own ``out`` / ``offsets`` buffers while its
    call may still run."""

    def __init__(self, n=3, device=0):
        if n < 1:
            raise ValueError("at least one lane")
        self.device = int(device)
        # every lane a context of its own, the process-wide context(device) included: no
        # state of other callers' calls (workspace sizes, ticket counters, completion stream)
        # reaches a lane, and close() destroys them all
        self.ctxs = []
        for _ in range(n):
            ctx = _native.Context(self.device)
            ctx.lock = threading.Lock()
            self.ctxs.append(ctx)
        self._ext = [None] * n
        # per lane: (event recorded after a call, the tensors that call borrows), oldest first
        self._held = [collections.deque() for _ in range(n)]

    def __len__(self):
        return len(self.ctxs)

    def stream(self, lane):
        """Lane ``lane``'s HIP stream as a torch.cuda.ExternalStream (events, waits)."""
        import torch

        if self._ext[lane] is None:
            self._ext[lane] = torch.cuda.ExternalStream(self.ctxs[lane].stream,
                                                        device=torch.device("cuda", self.device))
        return self._ext[lane]

    def _hold(self, lane, tensors):
        """Keep `tensors` referenced until the lane's stream has passed the call just enqueued
        (an event recorded after it), and drop the references of earlier calls it has passed.
        (Not Tensor.record_stream: the caching allocator would then record events on the lane's
        stream when the tensor is freed, which may be after the context -- and its stream --
        is gone.)"""
        import torch

        q = self._held[lane]
        while q and q[0][0].query():
            q.popleft()
        ev = torch.cuda.Event()
        ev.record(self.stream(lane))
        q.append((ev, tensors))

    def detect_device(self, k, frames, config, out, offsets, after_current=True):
        """detect_device on lane k % n (asynchronous on that lane's stream).

        The call borrows ``frames``, ``out`` and ``offsets`` until the lane's work is done,
        as the reference's detector borrows its image for the call (src/fast_simd.rs:847):
        the lane keeps a reference to each until its stream has passed the call, so torch's
        caching allocator cannot hand their memory to another tensor while the lane still
        reads or writes it, even when the caller drops its last reference right after this
        call."""
        import torch

        lane = k % len(self.ctxs)
        s = self.stream(lane)
        if after_current:
            s.wait_stream(torch.cuda.current_stream(frames.device))
        detect_device(frames, config, out, offsets, stream=s, device=self.device,
                      ctx=self.ctxs[lane])
        self._hold(lane, (frames, out, offsets))
        return lane

    def wait(self, lane=None):
        """Make torch's current stream wait for lane ``lane`` (every lane when None)."""
        import torch

        cur = torch.cuda.current_stream(torch.device("cuda", self.device))
        for i in (range(len(self.ctxs)) if lane is None else [lane]):
            cur.wait_stream(self.stream(i))

    def close(self):
        """Wait for every lane, release the borrowed tensors, destroy the lanes' contexts."""
        try:
            for q in self._held:
                if q:
                    q[-1][0].synchronize()
        finally:
            # also after a device error: drop the borrows and the lanes' contexts (each
            # context's destroy drains its own stream first)
            for ctx in self.ctxs:
                ctx.close()
            for q in self._held:
                q.clear()
            self.ctxs = []
            self._ext = []
            self._held = []


def detect_device_rgb(frames, config, out, offsets, stream=None, device=None):
    """detect_device for RGB8 frames: ``frames`` a contiguous (F, H, W, 3) uint8 CUDA tensor;
    the detector converts pixels to luma (image 0.24.6 to_luma8) as it loads them
    (fdf_detect_device_rgb), so no grey copy is written."""
    import torch

    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or \
            not frames.is_contiguous():
        raise ValueError("frames must be a contiguous (F, H, W, 3) uint8 tensor")
    if not frames.is_cuda or not out.is_cuda or not offsets.is_cuda:
        raise ValueError("detect_device_rgb needs CUDA (HIP) tensors")
    if offsets.dtype != torch.int64 or offsets.numel() < frames.shape[0] + 1:
        raise ValueError("offsets must be int64 with F+1 entries")
    if out.dim() != 2 or out.shape[1] != 2 or out.element_size() != 4 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (cap, 2) 32-bit tensor")
    dev, stream = _device_stream(torch, frames, device, stream)
    cfg = _to_c_config(config)
    ctx = context(dev)
    f, h, w = frames.shape[:3]
    rc = _native.load().fdf_detect_device_rgb(
        ctx.handle, frames.data_ptr(), f, w, h, 3 * h * w, ctypes.byref(cfg), out.data_ptr(),
        out.shape[0], offsets.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_detect_device_rgb")


def keypoint_scores(img, points, config, device=0):
    """u16 NMS scores of the given centres (extension: the reference's Point has no score).
    ``config.non_maximal_supression`` picks MaxThreshold (src/fast_simd.rs:623-718, window =
    count) or SumAbsolute (:722-749, uses threshold)."""
    arr = _as_pixels(img)
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint32).reshape(-1, 2))
    cfg = _to_c_config(config)
    h, w = arr.shape
    scores = np.zeros(pts.shape[0], dtype=np.uint16)
    ctx = context(device)
    # fdf_score_points reuses the context's retained result buffers: hold the lock that keeps
    # a two-call pattern (detect, then fdf_fetch_last) of another thread together
    with ctx.lock:
        rc = _native.load().fdf_score_points(
            ctx.handle, arr.ctypes.data, w, h, arr.strides[0], ctypes.byref(cfg),
            pts.ctypes.data, pts.shape[0], scores.ctypes.data)
    check(rc, "fdf_score_points")
    return scores


def _ring_config(score, t, n):
    return _native.FdfConfig(t, n, int(score))


def score_rings(centers, rings, score, threshold=0, consecutive=9, device=0):
    """u16 scores of (centre, 16 circle pixels) rings on the GPU (fdf_score_rings).
    ``score`` is NonMaximalSuppression.MaxThreshold (src/fast_simd.rs:623, window
    ``consecutive``) or SumAbsolute (:722, ``threshold``); ``rings`` is (K, 16) uint8 in
    circle() order, ``centers`` (K,) uint8."""
    c = np.ascontiguousarray(np.asarray(centers, dtype=np.uint8).reshape(-1))
    r = np.ascontiguousarray(np.asarray(rings, dtype=np.uint8).reshape(-1, 16))
    if r.shape[0] != c.shape[0]:
        raise ValueError("centers and rings differ in length")
    if not 0 <= int(threshold) <= 255:
        raise ValueError("threshold must fit u8")
    cfg = _ring_config(score, threshold, consecutive)
    out = np.zeros(c.shape[0], dtype=np.uint16)
    ctx = context(device)
    with ctx.lock:   # reuses the retained result buffers, see keypoint_scores
        rc = _native.load().fdf_score_rings(ctx.handle, c.ctypes.data, r.ctypes.data,
                                            c.shape[0], ctypes.byref(cfg), out.ctypes.data)
    check(rc, "fdf_score_rings")
    return out


def keypoint_score_max_threshold(base_v, pixels, consecutive):
    """src/fast_simd.rs:623 on one ring (16 circle pixels), computed on the GPU."""
    return int(score_rings([base_v], [pixels], NonMaximalSuppression.MaxThreshold,
                           consecutive=consecutive)[0])


def keypoint_score_sum_abs_difference(pixels, center, threshold):
    """src/fast_simd.rs:722 on one ring with the masks its callers build from ``threshold``
    (:1213-1222), computed on the GPU."""
    return int(score_rings([center], [pixels], NonMaximalSuppression.SumAbsolute,
                           threshold=threshold)[0])


def score_rings_device(centers, rings, scores, score, threshold=0, consecutive=9,
                       stream=None, device=None):
    """Device-resident fdf_score_rings_device: torch uint8 (K,) centres and (K, 16) rings,
    int16/uint16-sized (K,) scores tensor, all on one GPU; asynchronous on ``stream``."""
    import torch
    if rings.dim() != 2 or rings.shape[1] != 16 or centers.numel() != rings.shape[0] \
            or scores.numel() < rings.shape[0]:
        raise ValueError("rings must be (K, 16) with K centres and K scores")
    if centers.dtype != torch.uint8 or rings.dtype != torch.uint8:
        raise ValueError("centers and rings must be uint8 tensors")
    if not (centers.is_cuda and rings.is_cuda and scores.is_cuda):
        raise ValueError("score_rings_device needs CUDA (HIP) tensors")
    if not (centers.device == rings.device == scores.device):
        raise ValueError("centers, rings and scores must be on the same device")
    if not (centers.is_contiguous() and rings.is_contiguous() and scores.is_contiguous()):
        raise ValueError("tensors must be contiguous")
    if scores.element_size() != 2:
        raise ValueError("scores must be a 16-bit tensor")
    if rings.numel() and rings.data_ptr() % 16 != 0:
        raise ValueError("rings must start on a 16-byte boundary (one 16-byte load per ring)")
    dev, stream = _device_stream(torch, rings, device, stream)
    cfg = _ring_config(score, threshold, consecutive)
    rc =_native.load().fdf_score_rings_device(
        context(dev).handle, centers.data_ptr(), rings.data_ptr(), rings.shape[0],
        ctypes.byref(cfg), scores.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_score_rings_device")


def detect_scored_array(img, config, device=0):
    """Keypoints with scores: ((K, 2) uint32 (x, y) in raster order, (K,) uint16 scores).
    The score is the one the configured NMS suppresses with, max-threshold when NMS is off
    (fdf_detect_scored)."""
    arr = _as_pixels(img)
    cfg = _to_c_config(config)
    h, w = arr.shape
    ctx = context(device)
    lib = _native.load()
    stride = arr.strides[0] if arr.size else w
    ptr = arr.ctypes.data if arr.size else None
    return _two_call(ctx, w * h, lambda o, sc, cap, n: lib.fdf_detect_scored(
        ctx.handle, ptr, w, h, stride, ctypes.byref(cfg), o, sc, cap, ctypes.byref(n)),
        "fdf_detect_scored", scored=True)


def detector_scored(img, config):
    """``list[(Point, score)]`` in raster order (the (x, y, score) output)."""
    pts, scores = detect_scored_array(img, config)
    return [(Point(int(x), int(y)), int(s)) for (x, y), s in zip(pts, scores)]


def detector_batch_scored(frames, config, device=0):
    """detector_batch with scores: (points (K, 2), scores (K,) uint16, offsets (F+1,))."""
    frames = np.ascontiguousarray(np.asarray(frames), dtype=np.uint8)
    if frames.ndim != 3:
        raise ValueError("expected a (F, H, W) uint8 stack")
    f, h, w = frames.shape
    cfg = _to_c_config(config)
    ctx = context(device)
    lib = _native.load()
    offsets = np.zeros(f + 1, dtype=np.uint64)
    ptr = frames.ctypes.data if frames.size else None
    pts, scores = _two_call(ctx, f * h * w, lambda o, sc, cap, n: lib.fdf_detect_batch_scored(
        ctx.handle, ptr, f, w, h, h * w, ctypes.byref(cfg), o, sc, cap, offsets.ctypes.data,
        ctypes.byref(n)), "fdf_detect_batch_scored", scored=True)
    return pts, scores, offsets


def score_device(frames, config, points, offsets, scores, stream=None, device=None):
    """Scores of detect_device's output, on the device: ``points`` (cap, 2) and ``offsets``
    as detect_device filled them, ``scores`` a (cap,) int16/uint16 CUDA tensor.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    if frames.dim() != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous (F, H, W) uint8 tensor")
    if not (frames.is_cuda and points.is_cuda and offsets.is_cuda and scores.is_cuda):
        raise ValueError("score_device needs CUDA (HIP) tensors")
    if scores.element_size() != 2 or not scores.is_contiguous() or \
            scores.numel() < points.shape[0]:
        raise ValueError("scores must be a contiguous 16-bit tensor with cap entries")
    if offsets.dtype != torch.int64 or offsets.numel() < frames.shape[0] + 1:
        raise ValueError("offsets must be int64 with F+1 entries")
    dev, stream = _device_stream(torch, frames, device, stream)
    cfg = _to_c_config(config)
    ctx = context(dev)
    f, h, w = frames.shape
    rc = _native.load().fdf_score_device(
        ctx.handle, frames.data_ptr(), f, w, h, h * w, ctypes.byref(cfg), points.data_ptr(),
        points.shape[0], offsets.data_ptr(), scores.data_ptr(),
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_score_device")

def _cell_k(cell, k):
    """(cell_w, cell_h, k) of a selection: ``cell`` is (cell_w, cell_h), 0 meaning the whole
    image dimension; k >= 1."""
    cw, ch = (int(v) for v in cell)
    k = int(k)
    if cw < 0 or ch < 0 or cw > 0xffffffff or ch > 0xffffffff:
        raise ValueError("cell sizes must fit in u32")
    if not 1 <= k <= 0xffffffff:
        raise ValueError("k must be at least 1")
    return cw, ch, k


def select_scratch_bytes(n_frames, shape, cell, cap):
    """Scratch bytes select_device needs (fdf_select_scratch_bytes; host only, no device):
    ``shape`` is (height, width), ``cell`` (cell_w, cell_h), ``cap`` the points' capacity."""
    h, w = (int(v) for v in shape)
    cw, ch = (int(v) for v in cell)
    v = ctypes.c_uint64()
    check(_native.load().fdf_select_scratch_bytes(int(n_frames), w, h, cw, ch, int(cap),
                                                  ctypes.byref(v)), "fdf_select_scratch_bytes")
    return v.value


def select_device(points, scores, offsets, shape, cell, k, sel, sel_scores, sel_offsets,
                  keep=None, scratch=None, stream=None):
    """Best ``k`` points per ``cell`` = (cell_w, cell_h) grid cell of every frame, on the
    device (fdf_select_device): ``points`` (cap, 2), ``scores`` (cap,) 16-bit and ``offsets``
    (F+1,) int64 (exactly F+1 entries: F is taken from it) as detect_device and score_device
    filled them, ``shape`` = (height, width).
    The kept points go to ``sel`` (sel_cap, 2) and ``sel_scores`` (sel_cap,) in input order,
    ``sel_offsets`` (F+1,) int64 gets the per-frame prefix and the full total; ``keep``
    (optional, (cap,) uint8) gets a 1 / 0 flag per input point.  Ties at the cut go to the
    earlier point.  ``scratch``: a uint8 CUDA tensor of at least select_scratch_bytes(...)
    bytes (None: allocated through torch).  Asynchronous on ``stream`` (default: torch's
    current stream)."""
    import torch

    cw, ch, k = _cell_k(cell, k)
    h, w = (int(v) for v in shape)
    _check_points(points, "points", "n")
    _check_points(sel, "sel", "n")
    for name, t, n in (("scores", scores, points.shape[0]), ("sel_scores", sel_scores, sel.shape[0])):
        if t.dim() != 1 or t.element_size() != 2 or not t.is_contiguous() or \
                t.is_floating_point() or t.numel() < n:
            raise ValueError(f"{name} must be a contiguous 16-bit integer tensor, one entry per point")
    _check_offsets(torch, offsets, 2)
    f = offsets.numel() - 1
    _check_offsets(torch, sel_offsets, f + 1, "sel_offsets", one_dim=False)
    cap = points.shape[0]
    if keep is not None and (keep.dtype != torch.uint8 or keep.numel() < cap or
                             not keep.is_contiguous()):
        raise ValueError("keep must be a contiguous uint8 tensor with cap entries")
    _check_one_device("select_device", [t for t in (points, scores, offsets, sel, sel_scores,
                                                    sel_offsets, keep, scratch) if t is not None])
    need = select_scratch_bytes(f, (h, w), (cw, ch), cap)
    if scratch is not None and (scratch.dtype != torch.uint8 or not scratch.is_contiguous()):
        raise ValueError("scratch must be a contiguous uint8 tensor")
    current = torch.cuda.current_stream(points.device)
    if stream is None:
        stream = current
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=points.device)
        if stream != current:
            # the caching allocator hands a freed block to the next request of the current
            # stream; this one is in use on `stream` until the call's kernels are done
            scratch.record_stream(stream)
    rc = _native.load().fdf_select_device(
        context(points.device.index).handle, f, w, h, points.data_ptr(), scores.data_ptr(), cap,
        offsets.data_ptr(), cw, ch, k, sel.data_ptr(), sel_scores.data_ptr(), sel.shape[0],
        sel_offsets.data_ptr(), keep.data_ptr() if keep is not None else None,
        scratch.data_ptr(), scratch.numel(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_select_device")


def select_best(points, scores, shape, cell, k, offsets=None, device=0):
    """Best ``k`` points per ``cell`` = (cell_w, cell_h) grid cell (0 = the whole image
    dimension) of raster-ordered ``points`` (K, 2) uint32 with ``scores`` (K,) uint16, for an
    image of ``shape`` = (height, width), over fdf_select_points.  Returns (points, scores)
    of the kept points in input order; with ``offsets`` ((F+1,) uint64, frames concatenated)
    also the kept points' offsets."""
    cw, ch, k = _cell_k(cell, k)
    h, w = (int(v) for v in shape)
    pts = np.asarray(points)
    sc = np.asarray(scores)
    if pts.dtype != np.uint32 or pts.ndim != 2 or pts.shape[1] != 2:
        raise TypeError("points must be a (K, 2) uint32 array")
    if sc.dtype != np.uint16 or sc.ndim != 1 or sc.shape[0] != pts.shape[0]:
        raise TypeError("scores must be a (K,) uint16 array, one per point")
    pts = np.ascontiguousarray(pts)
    sc = np.ascontiguousarray(sc)
    n = pts.shape[0]
    if offsets is not None:
        offs = np.asarray(offsets)
        if offs.dtype != np.uint64 or offs.ndim != 1 or offs.shape[0] < 2:
            raise TypeError("offsets must be a (F+1,) uint64 array")
        offs = np.ascontiguousarray(offs)
        f = offs.shape[0] - 1
    else:
        offs, f = None, 1
    ctx = context(device)
    lib = _native.load()
    out_offs = np.zeros(f + 1, dtype=np.uint64)
    cap = n                                   # a selection never exceeds its input
    out = np.empty((cap, 2), dtype=np.uint32)
    out_scores = np.empty(cap, dtype=np.uint16)
    got = ctypes.c_size_t(0)
    rc = lib.fdf_select_points(ctx.handle, pts.ctypes.data if n else None,
                               sc.ctypes.data if n else None,
                               offs.ctypes.data if offs is not None else None, f, n, w, h, cw, ch,
                               k, out.ctypes.data if cap else None,
                               out_scores.ctypes.data if cap else None, cap,
                               out_offs.ctypes.data, ctypes.byref(got))
    check(rc, "fdf_select_points")
    m = got.value
    if offsets is not None:
        return out[:m], out_scores[:m], out_offs
    return out[:m], out_scores[:m]


def detect_best_array(img, config, cell, k, device=0):
    """detect_scored_array followed by select_best: the ``k`` strongest keypoints of every
    ``cell`` = (cell_w, cell_h) grid cell, as ((K, 2) uint32 in raster order, (K,) uint16)."""
    cw, ch, k = _cell_k(cell, k)
    arr = _as_pixels(img)
    pts, scores = detect_scored_array(arr, config, device=device)
    return select_best(pts, scores, arr.shape, (cw, ch), k, device=device)


def _radius(radius):
    r = int(radius)
    if not 1 <= r <= 31:
        raise ValueError("radius must be in 1..31")
    return r


def orient_disc(radius):
    """Half-widths u[0..radius] of the orientation disc (fdf_orient_disc; host only, no
    device): row v spans the columns |d| <= u[|v|].  OpenCV's umax table."""
    r = _radius(radius)
    u = np.zeros(r + 1, dtype=np.uint8)
    check(_native.load().fdf_orient_disc(r, u.ctypes.data), "fdf_orient_disc")
    return u


def orient_device(frames, points, offsets, angles, radius=15, moments=None, stream=None,
                  device=None):
    """Intensity-centroid angles of detect_device's (or select_device's) output, on the
    device (fdf_orient_device): ``frames`` (F, H, W) uint8 with contiguous frames any number
    of bytes apart, ``points`` (cap, 2) and ``offsets`` (F+1,) int64 as detect_device filled
    them.  ``angles`` (cap,) float32 gets atan2(m01, m10) of the disc of ``radius`` around
    every point, ``moments`` (optional, (cap, 2) int32) the exact (m10, m01).  Asynchronous on
    ``stream`` (default: torch's current stream)."""
    import torch

    r = _radius(radius)
    _check_frames(torch, frames)
    _check_points(points)
    cap = points.shape[0]
    _check_angles(torch, angles, cap)
    if moments is not None and (moments.dtype != torch.int32 or moments.dim() != 2 or
                                moments.shape[1] != 2 or moments.shape[0] < cap or
                                not moments.is_contiguous()):
        raise ValueError("moments must be a contiguous (cap, 2) int32 tensor")
    _check_offsets(torch, offsets, frames.shape[0] + 1)
    _check_one_device("orient_device",
                      [frames, points, offsets, angles] + ([moments] if moments is not None else []))
    dev, stream = _device_stream(torch, frames, device, stream)
    rc = _native.load().fdf_orient_device(
        context(dev).handle, *_frame_args(frames),
        points.data_ptr(), cap, offsets.data_ptr(), r, angles.data_ptr(),
        moments.data_ptr() if moments is not None else None,
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_orient_device")


def keypoint_angles(img, points, radius=15, device=0, moments=False):
    """Intensity-centroid angles ((K,) float32, radians in (-pi, pi], y down) of the given
    ``points`` (K, 2) of one image (fdf_orient_points); with ``moments`` also the exact
    (K, 2) int32 (m10, m01).  Points outside the image are an error."""
    r = _radius(radius)
    arr = _as_pixels(img)
    pts = _host_points(points)
    h, w = arr.shape
    n = pts.shape[0]
    angles = np.zeros(n, dtype=np.float32)
    mom = np.zeros((n, 2), dtype=np.int32) if moments else None
    rc = _native.load().fdf_orient_points(
        context(device).handle, arr.ctypes.data if arr.size else None, w, h,
        arr.strides[0] if arr.size else w, pts.ctypes.data if n else None, n, r,
        angles.ctypes.data if n else None, mom.ctypes.data if moments and n else None)
    check(rc, "fdf_orient_points")
    return (angles, mom) if moments else angles


def detect_oriented_array(img, config, radius=15, device=0):
    """detect_scored_array followed by keypoint_angles: ((K, 2) uint32 points in raster
    order, (K,) uint16 scores, (K,) float32 angles)."""
    r = _radius(radius)
    arr = _as_pixels(img)
    pts, scores = detect_scored_array(arr, config, device=device)
    return pts, scores, keypoint_angles(arr, pts, r, device=device)


def _harris_args(block, k):
    """(block, k_num, k_den) of a Harris response: block 3, 5 or 7, k = (k_num, k_den) the
    rational Harris constant with 0 <= k_num <= 255 and 1 <= k_den <= 255."""
    b = int(block)
    if b not in (3, 5, 7):
        raise ValueError("block must be 3, 5 or 7")
    try:
        num, den = (int(v) for v in k)
    except (TypeError, ValueError):
        raise ValueError("k must be a pair of integers (k_num, k_den)") from None
    if not (0 <= num <= 255 and 1 <= den <= 255):
        raise ValueError("k = (k_num, k_den) needs 0 <= k_num <= 255 and 1 <= k_den <= 255")
    return b, num, den


def harris_codes(responses):
    """The u16 rank scores of int64 Harris responses (fdf_harris_codes; host only, no device):
    0 for R <= 0, R below 1024, else (e - 9) << 10 | the 10 bits below the leading one, with
    e = floor(log2 R): monotone in R, the key select_device ranks by."""
    r = np.asarray(responses)
    if r.dtype != np.int64:
        raise TypeError("responses must be an int64 array")
    flat = np.ascontiguousarray(r).reshape(-1)
    codes = np.zeros(flat.shape[0], dtype=np.uint16)
    n = flat.shape[0]
    check(_native.load().fdf_harris_codes(flat.ctypes.data if n else None, n,
                                          codes.ctypes.data if n else None), "fdf_harris_codes")
    return codes.reshape(r.shape)


def harris_device(frames, points, offsets, scores, block=7, k=(1, 25), responses=None,
                  stream=None, device=None):
    """Harris corner responses of detect_device's (or select_device's) output, on the device
    (fdf_harris_device): ``frames`` (F, H, W) uint8 with contiguous frames any number of bytes
    apart, ``points`` (cap, 2) and ``offsets`` (F+1,) int64 as detect_device filled them.
    ``scores`` (cap,) int16/uint16 gets the u16 rank score of every point's response over the
    ``block`` x ``block`` (3, 5 or 7) Sobel gradients around it with the Harris constant
    ``k`` = (k_num, k_den), ready for select_device; ``responses`` (optional, (cap,) int64) the
    exact responses.  Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    b, num, den = _harris_args(block, k)
    _check_frames(torch, frames)
    _check_points(points)
    cap = points.shape[0]
    if scores.dim() != 1 or scores.element_size() != 2 or scores.is_floating_point() or \
            not scores.is_contiguous() or scores.numel() < cap:
        raise ValueError("scores must be a contiguous 16-bit integer tensor with cap entries")
    if responses is not None and (responses.dtype != torch.int64 or responses.dim() != 1 or
                                  responses.numel() < cap or not responses.is_contiguous()):
        raise ValueError("responses must be a contiguous int64 tensor with cap entries")
    _check_offsets(torch, offsets, frames.shape[0] + 1)
    _check_one_device("harris_device", [frames, points, offsets, scores] +
                      ([responses] if responses is not None else []))
    dev, stream = _device_stream(torch, frames, device, stream)
    rc = _native.load().fdf_harris_device(
        context(dev).handle, *_frame_args(frames),
        points.data_ptr(), cap, offsets.data_ptr(), b, num, den, scores.data_ptr(),
        responses.data_ptr() if responses is not None else None,
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_harris_device")


def keypoint_harris(img, points, block=7, k=(1, 25), device=0, responses=False):
    """Harris rank scores ((K,) uint16) of the given ``points`` (K, 2) of one image
    (fdf_harris_points); with ``responses`` also the exact (K,) int64 responses.  Points
    outside the image are an error."""
    b, num, den = _harris_args(block, k)
    arr = _as_pixels(img)
    pts = _host_points(points)
    h, w = arr.shape
    n = pts.shape[0]
    scores = np.zeros(n, dtype=np.uint16)
    resp = np.zeros(n, dtype=np.int64) if responses else None
    rc = _native.load().fdf_harris_points(
        context(device).handle, arr.ctypes.data if arr.size else None, w, h,
        arr.strides[0] if arr.size else w, pts.ctypes.data if n else None, n, b, num, den,
        scores.ctypes.data if n else None, resp.ctypes.data if responses and n else None)
    check(rc, "fdf_harris_points")
    return (scores, resp) if responses else scores


def detect_harris_array(img, config, block=7, k=(1, 25), device=0):
    """detect_array followed by keypoint_harris: ((K, 2) uint32 points in raster order,
    (K,) uint16 Harris rank scores), the pair select_best takes."""
    b, num, den = _harris_args(block, k)
    arr = _as_pixels(img)
    pts = detect_array(arr, config, device=device)
    return pts, keypoint_harris(arr, pts, b, (num, den), device=device)


def _n_bins(n_bins):
    n = int(n_bins)
    if not 1 <= n <= 360:
        raise ValueError("n_bins must be in 1..360")
    return n


def _pattern(pattern):
    p = np.asarray(pattern)
    if p.dtype != np.int8 or p.size != 1024 or p.shape not in ((256, 4), (1024,)):
        raise TypeError("pattern must be a (256, 4) int8 array")
    return np.ascontiguousarray(p).reshape(256, 4)


def brief_pattern():
    """The default BRIEF pattern (fdf_brief_pattern; host only, no device): (256, 4) int8,
    test i = (x0, y0, x1, y1)."""
    p = np.zeros((256, 4), dtype=np.int8)
    check(_native.load().fdf_brief_pattern(p.ctypes.data), "fdf_brief_pattern")
    return p


def brief_steer(pattern, n_bins):
    """The steering table of ``pattern`` ((256, 4) int8) for ``n_bins`` orientation bins
    (fdf_brief_steer; host only, no device): (n_bins, 256, 4) int8, bin b = the pattern rotated
    by 2 pi b / n_bins with y pointing down."""
    n = _n_bins(n_bins)
    p = _pattern(pattern)
    table = np.zeros((n, 256, 4), dtype=np.int8)
    check(_native.load().fdf_brief_steer(p.ctypes.data, n, table.ctypes.data), "fdf_brief_steer")
    return table


def smooth_device(frames, out, stream=None, device=None):
    """5 x 5 box smoothing on the device (fdf_smooth_device): ``out`` = (sum of the 5 x 5
    neighbourhood at clamped coordinates + 12) // 25.  ``frames`` and ``out`` are (F, H, W)
    uint8 tensors of the same shape with contiguous frames any number of bytes apart (each its
    own); the bytes between output frames are not written.  They must not overlap.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    _check_frames(torch, frames)
    _check_frames(torch, out, "out")
    if frames.shape != out.shape:
        raise ValueError("frames and out must have the same shape")
    f, h, w = frames.shape
    if f > 65535 or h < 1 or w < 1 or h * w > 0x7fffff00:
        raise ValueError("at most 65535 frames of 1 <= width * height <= 2^31 - 256 pixels")
    _check_one_device("smooth_device", [frames, out])
    if f:
        span = lambda t: (t.data_ptr(), t.data_ptr() + (f - 1) * t.stride(0) + h * w)
        (a0, a1), (b0, b1) = span(frames), span(out)
        if a0 < b1 and b0 < a1:
            raise ValueError("frames and out must not overlap")
    dev, stream = _device_stream(torch, frames, device, stream)
    out_ptr, _, _, _, out_stride = _frame_args(out)
    rc = _native.load().fdf_smooth_device(
        context(dev).handle, *_frame_args(frames), out_ptr, out_stride,
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_smooth_device")


def describe_device(frames, points, offsets, desc, table, n_bins, angles=None, stream=None,
                    device=None):
    """Steered BRIEF descriptors of detect_device's (or select_device's) output, on the
    device (fdf_describe_device): ``frames`` (F, H, W) uint8 with contiguous frames any number
    of bytes apart (smoothed by smooth_device, or not: the caller's choice), ``points``
    (cap, 2) and ``offsets`` (F+1,) int64 as detect_device filled them, ``angles`` (optional,
    (cap,) float32) as orient_device filled them, ``table`` the int8 CUDA tensor of
    brief_steer(pattern, n_bins).  ``desc`` (cap, 32) uint8 gets the 256 bits of every point,
    test i in bit i % 8 of byte i // 8.  Without ``angles`` every point uses bin 0.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    n = _n_bins(n_bins)
    _check_frames(torch, frames)
    _check_points(points)
    cap = points.shape[0]
    if desc.dtype != torch.uint8 or desc.dim() != 2 or desc.shape[1] != 32 or \
            desc.shape[0] < cap or not desc.is_contiguous():
        raise ValueError("desc must be a contiguous (cap, 32) uint8 tensor")
    if table.dtype != torch.int8 or not table.is_contiguous() or table.numel() != n * 1024:
        raise ValueError("table must be a contiguous int8 tensor of n_bins * 256 * 4 entries")
    if angles is not None:
        _check_angles(torch, angles, cap)
    _check_offsets(torch, offsets, frames.shape[0] + 1)
    _check_one_device("describe_device", [frames, points, offsets, desc, table] +
                      ([angles] if angles is not None else []))
    dev, stream = _device_stream(torch, frames, device, stream)
    rc = _native.load().fdf_describe_device(
        context(dev).handle, *_frame_args(frames),
        points.data_ptr(), cap, offsets.data_ptr(),
        angles.data_ptr() if angles is not None else None, table.data_ptr(), n,
        desc.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_describe_device")


def keypoint_descriptors(img, points, angles=None, pattern=None, n_bins=30, smooth=True,
                         device=0):
    """Steered BRIEF descriptors ((K, 32) uint8) of the given ``points`` (K, 2) of one image
    (fdf_describe_points): ``angles`` (optional, (K,) float32 radians, as keypoint_angles
    returns them) pick one of ``n_bins`` rotations of ``pattern`` ((256, 4) int8; None: the
    default of brief_pattern); with ``smooth`` the tests read the 5 x 5 box-smoothed image.
    Points outside the image are an error."""
    n = _n_bins(n_bins)
    arr = _as_pixels(img)
    pts = _host_points(points)
    k = pts.shape[0]
    if angles is not None:
        ang = np.asarray(angles)
        if ang.dtype != np.float32 or ang.shape != (k,):
            raise TypeError("angles must be a (K,) float32 array, one per point")
        ang = np.ascontiguousarray(ang)
    pat = _pattern(pattern) if pattern is not None else None
    h, w = arr.shape
    desc = np.zeros((k, 32), dtype=np.uint8)
    rc = _native.load().fdf_describe_points(
        context(device).handle, arr.ctypes.data if arr.size else None, w, h,
        arr.strides[0] if arr.size else w, pts.ctypes.data if k else None, k,
        ang.ctypes.data if angles is not None and k else None,
        pat.ctypes.data if pat is not None else None, n, 1 if smooth else 0,
        desc.ctypes.data if k else None)
    check(rc, "fdf_describe_points")
    return desc


def detect_described_array(img, config, radius=15, n_bins=30, device=0):
    """detect_array, keypoint_angles on the image and keypoint_descriptors (default pattern)
    on its smoothed copy: ((K, 2) uint32 points in raster order, (K,) float32 angles,
    (K, 32) uint8 descriptors)."""
    r = _radius(radius)
    n = _n_bins(n_bins)
    arr = _as_pixels(img)
    pts = detect_array(arr, config, device=device)
    angles = keypoint_angles(arr, pts, r, device=device)
    return pts, angles, keypoint_descriptors(arr, pts, angles, n_bins=n, device=device)


# ---- exact bilinear resize and the scale pyramid ---------------------------------------------

_MAX_SIDE = 65535                 # a tap word holds i0 << 12 | q
_MAX_PIXELS = 0x7fffff00          # byte offsets of a frame fit an int


def _side(v, name, top=0xffffffff):
    n = int(v)
    if not 1 <= n <= top:
        raise ValueError(f"{name} must be in 1..{top}")
    return n


def _dst_shape(shape):
    """(dst_h, dst_w) of a resize."""
    try:
        h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise TypeError("shape must be a pair (height, width) of integers") from None
    if h < 1 or w < 1 or h * w > _MAX_PIXELS:
        raise ValueError("the destination must have 1 <= width * height <= 2^31 - 256 pixels")
    return h, w


def _scale(scale):
    try:
        num, den = (int(v) for v in scale)
    except (TypeError, ValueError):
        raise TypeError("scale must be a pair (num, den) of integers") from None
    if not (0 <= num <= 0xffffffff and 0 <= den <= 0xffffffff):
        raise ValueError("scale terms must fit u32")
    return num, den


def resize_taps(src_len, dst_len):
    """The taps of one axis of a resize from ``src_len`` to ``dst_len`` pixels
    (fdf_resize_taps; host only, no device): (dst_len,) uint32, entry i = i0 << 12 | q with the
    first source index i0 and the second tap's weight q of 2048."""
    s = _side(src_len, "src_len", _MAX_SIDE)
    d = _side(dst_len, "dst_len", _MAX_PIXELS)
    taps = np.zeros(d, dtype=np.uint32)
    check(_native.load().fdf_resize_taps(s, d, taps.ctypes.data), "fdf_resize_taps")
    return taps


def _check_taps(t, n, name):
    if t.dim() != 1 or t.element_size() != 4 or t.is_floating_point() or \
            not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{name} must be a contiguous 32-bit integer tensor, one entry per "
                         "destination index")


def _device_taps(torch, taps, device):
    return torch.from_numpy(np.ascontiguousarray(taps).view(np.int32)).to(device)


def resize_device(frames, out, xtaps=None, ytaps=None, stream=None, device=None):
    """Exact bilinear resize on the device (fdf_resize_device): ``frames`` (F, H, W) and ``out``
    (F, h, w) uint8 tensors with contiguous frames any number of bytes apart (each its own);
    the bytes between output frames are not written.  They must not overlap.  ``xtaps`` (w,)
    and ``ytaps`` (h,) are 32-bit integer tensors holding resize_taps(W, w) and
    resize_taps(H, h) (None: computed and uploaded by the call); entries are clamped on the
    device.  Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    _check_frames(torch, frames)
    _check_frames(torch, out, "out")
    f, sh, sw = frames.shape
    of, dh, dw = out.shape
    if of != f:
        raise ValueError("frames and out must hold the same number of frames")
    if f > 65535:
        raise ValueError("at most 65535 frames")
    for h, w, name in ((sh, sw, "frames"), (dh, dw, "out")):
        if h < 1 or w < 1 or h * w > _MAX_PIXELS:
            raise ValueError(f"{name}: 1 <= width * height <= 2^31 - 256 pixels")
    if sh > _MAX_SIDE or sw > _MAX_SIDE:
        raise ValueError("a source side is at most 65535 pixels")
    tensors = [frames, out]
    for t, n, name in ((xtaps, dw, "xtaps"), (ytaps, dh, "ytaps")):
        if t is not None:
            _check_taps(t, n, name)
            tensors.append(t)
    _check_one_device("resize_device", tensors)
    if f:
        (a0, a1), (b0, b1) = ((t.data_ptr(), t.data_ptr() + (f - 1) * t.stride(0) +
                               t.shape[1] * t.shape[2]) for t in (frames, out))
        if a0 < b1 and b0 < a1:
            raise ValueError("frames and out must not overlap")
    dev, stream = _device_stream(torch, frames, device, stream)
    if xtaps is None:
        xtaps = _device_taps(torch, resize_taps(sw, dw), frames.device)
    if ytaps is None:
        ytaps = _device_taps(torch, resize_taps(sh, dh), frames.device)
    out_ptr, _, _, _, out_stride = _frame_args(out)
    rc = _native.load().fdf_resize_device(
        context(dev).handle, *_frame_args(frames), out_ptr, dw, dh, out_stride,
        xtaps.data_ptr(), ytaps.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_resize_device")


def resize_array(img, shape, device=0):
    """One host image resized to ``shape`` = (height, width) (fdf_resize_frame): a (height,
    width) uint8 array, every pixel rounded once."""
    arr = _as_pixels(img)
    dh, dw = _dst_shape(shape)
    h, w = arr.shape
    if h < 1 or w < 1 or h > _MAX_SIDE or w > _MAX_SIDE or h * w > _MAX_PIXELS:
        raise ValueError("the image must have sides in 1..65535 and at most 2^31 - 256 pixels")
    out = np.zeros((dh, dw), dtype=np.uint8)
    rc = _native.load().fdf_resize_frame(context(device).handle, arr.ctypes.data, w, h,
                                         arr.strides[0], out.ctypes.data, dw, dh, dw)
    check(rc, "fdf_resize_frame")
    return out


_BORDERS = {"replicate": _native.FDF_BORDER_REPLICATE, "constant": _native.FDF_BORDER_CONSTANT}


def _border_fill(border, fill):
    """(FDF_BORDER_*, fill) of a warp."""
    if border not in _BORDERS:
        raise ValueError('border must be "replicate" or "constant"')
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("fill must be in 0..255")
    return _BORDERS[border], fill


def _host_model(h):
    """Nine float64 numbers from nine numbers, a 3 x 3 array, a MODEL_DTYPE record or what
    estimate_model / refine_model return (their record is used)."""
    if isinstance(h, tuple) and len(h) in (3, 4) and isinstance(h[2], np.void):
        h = h[2]
    a = np.asarray(h)
    if a.dtype == MODEL_DTYPE and a.size == 1:
        return np.array(a.reshape(-1)[0]["h"], dtype=np.float64)
    if a.dtype.kind in "fiu" and a.size == 9:
        return np.ascontiguousarray(a, dtype=np.float64).reshape(9).copy()
    raise TypeError("a model is nine numbers, a (3, 3) array, a MODEL_DTYPE record or "
                    "estimate_model's result")


def model_invert(h):
    """The model that warps the other way (fdf_model_invert; host only, no device): the adjugate
    of ``h`` normalised to [2, 2] = 1 as a (3, 3) float64 array.  FdfError(FDF_ERR_ARG) for a
    singular model."""
    m = _host_model(h)
    out = np.zeros(9, dtype=np.float64)
    check(_native.load().fdf_model_invert(m.ctypes.data, out.ctypes.data), "fdf_model_invert")
    return out.reshape(3, 3)


def warp_device(frames, models, out, border="replicate", fill=0, mask=None, stream=None,
                device=None):
    """Exact bilinear warp on the device (fdf_warp_device): frame f of ``frames`` (F, H, W) is
    resampled into frame f of ``out`` (F, h, w) by model f, which maps a pixel of ``out`` to a
    position in ``frames`` -- ransac_device's / refine_device's models of (query, train) warp
    the train frames onto the query frames as they are.  ``models`` is their (F, 11) float64
    record tensor or an (F, 9) float64 tensor of row-major matrices, contiguous.  Both frame
    tensors are uint8 with contiguous frames any number of bytes apart (each its own); the bytes
    between output frames are not written; they must not overlap.  ``border``: "replicate", or
    "constant" with the value ``fill``; pixels without a position (w <= 0, NaN, beyond 2^19
    pixels) get ``fill`` in both.  ``mask`` (optional, uint8, the shape and strides of ``out``)
    gets 1 where the position lies inside the source frame.  Asynchronous on ``stream``
    (default: torch's current stream)."""
    import torch

    _check_frames(torch, frames)
    _check_frames(torch, out, "out")
    f, sh, sw = frames.shape
    of, dh, dw = out.shape
    if of != f:
        raise ValueError("frames and out must hold the same number of frames")
    if f > 65535:
        raise ValueError("at most 65535 frames")
    for h, w, name in ((sh, sw, "frames"), (dh, dw, "out")):
        if h < 1 or w < 1 or h * w > _MAX_PIXELS:
            raise ValueError(f"{name}: 1 <= width * height <= 2^31 - 256 pixels")
    if sh > _MAX_SIDE or sw > _MAX_SIDE:
        raise ValueError("a source side is at most 65535 pixels")
    if models.dtype != torch.float64 or models.dim() != 2 or models.shape[1] not in (9, 11) or \
            models.shape[0] < f or not models.is_contiguous():
        raise ValueError("models must be a contiguous (F, 11) or (F, 9) float64 tensor")
    border, fill = _border_fill(border, fill)
    tensors = [frames, models, out]
    if mask is not None:
        _check_frames(torch, mask, "mask")
        if mask.shape != out.shape or (f > 1 and mask.stride(0) != out.stride(0)):
            raise ValueError("mask must have the shape and frame stride of out")
        tensors.append(mask)
    _check_one_device("warp_device", tensors)
    if f:
        spans = [(t.data_ptr(), t.data_ptr() + (f - 1) * t.stride(0) + t.shape[1] * t.shape[2])
                 for t in tensors if t is not models]
        for i, (a0, a1) in enumerate(spans):
            for b0, b1 in spans[i + 1:]:
                if a0 < b1 and b0 < a1:
                    raise ValueError("frames, out and mask must not overlap")
    dev, stream = _device_stream(torch, frames, device, stream)
    out_ptr, _, _, _, out_stride = _frame_args(out)
    rc = _native.load().fdf_warp_device(
        context(dev).handle, *_frame_args(frames), models.data_ptr(), 8 * models.shape[1],
        out_ptr, dw, dh, out_stride, border, fill,
        mask.data_ptr() if mask is not None else None, ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_warp_device")


def warp_array(img, h, shape=None, border="replicate", fill=0, mask=False, device=0):
    """One host image warped by the model ``h`` into ``shape`` = (height, width) (default: the
    image's) (fdf_warp_frame): a (height, width) uint8 array, and with ``mask`` the pair (array,
    bool mask of the pixels whose position lies inside the image).  ``h`` maps a pixel of the
    result to a position in ``img``: nine numbers, a (3, 3) array, or what estimate_model /
    refine_model return."""
    arr = _as_pixels(img)
    m = _host_model(h)
    sh, sw = arr.shape
    dh, dw = _dst_shape(arr.shape if shape is None else shape)
    if sh < 1 or sw < 1 or sh > _MAX_SIDE or sw > _MAX_SIDE or sh * sw > _MAX_PIXELS:
        raise ValueError("the image must have sides in 1..65535 and at most 2^31 - 256 pixels")
    border, fill = _border_fill(border, fill)
    out = np.zeros((dh, dw), dtype=np.uint8)
    inside = np.zeros((dh, dw), dtype=np.uint8) if mask else None
    rc = _native.load().fdf_warp_frame(
        context(device).handle, arr.ctypes.data, sw, sh, arr.strides[0], m.ctypes.data,
        out.ctypes.data, dw, dh, dw, border, fill, inside.ctypes.data if mask else None)
    check(rc, "fdf_warp_frame")
    return (out, inside.astype(bool)) if mask else out


PyramidLevel =collections.namedtuple(
    "PyramidLevel", "width height frame_stride_bytes offset_bytes xtaps_offset ytaps_offset")


class PyramidPlan:
    """The levels of a scale pyramid (fdf_pyramid_plan): ``levels`` is a tuple of
    :class:`PyramidLevel`, level 0 the caller's frames; ``total_bytes`` is the size of the
    buffer that holds the levels >= 1 of ``n_frames`` frames, ``total_taps`` the entries of the
    taps array :meth:`taps` returns."""

    def __init__(self, c_levels, n_frames, scale, total_bytes, total_taps):
        self._c = c_levels
        self.n_frames = n_frames
        self.scale = scale
        self.total_bytes = total_bytes
        self.total_taps = total_taps
        self.levels = tuple(PyramidLevel(*(getattr(L, name) for name in PyramidLevel._fields))
                            for L in c_levels)

    def __len__(self):
        return len(self.levels)

    def taps(self):
        """The x and y taps of every level >= 1 (fdf_pyramid_taps): (total_taps,) uint32."""
        taps = np.zeros(self.total_taps, dtype=np.uint32)
        base = self.levels[0]
        check(_native.load().fdf_pyramid_taps(self._c, len(self.levels), base.width, base.height,
                                              taps.ctypes.data if taps.size else None),
              "fdf_pyramid_taps")
        return taps


def pyramid_plan(shape, n_levels=8, scale=(6, 5), n_frames=1):
    """The plan of an ``n_levels`` pyramid over ``n_frames`` frames of ``shape`` = (height,
    width) at the factor ``scale`` = (num, den) > 1 between levels (fdf_pyramid_plan; host only,
    no device): w_l = (w_(l-1) * den + num // 2) // num.  A factor that is not above 1 or a
    level count outside 1..32 raises FdfError(FDF_ERR_ARG), a level with a zero dimension
    FdfError(FDF_ERR_SIZE)."""
    try:
        h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise TypeError("shape must be a pair (height, width) of integers") from None
    num, den = _scale(scale)
    n, f = int(n_levels), int(n_frames)
    if not (0 <= h <= 0xffffffff and 0 <= w <= 0xffffffff and 0 <= n <= 0xffffffff and
            0 <= f <= 0xffffffff):
        raise ValueError("sizes and counts must fit u32")
    c_levels = (_native.FdfPyramidLevel * max(1, min(n, 32)))()
    total_bytes, total_taps = ctypes.c_uint64(), ctypes.c_uint64()
    check(_native.load().fdf_pyramid_plan(w, h, num, den, n, f, c_levels,
                                          ctypes.byref(total_bytes), ctypes.byref(total_taps)),
          "fdf_pyramid_plan")
    return PyramidPlan(c_levels, f, (num, den), total_bytes.value, total_taps.value)


def pyramid_device(frames, plan, buffer, taps, stream=None, device=None):
    """Every level >= 1 of ``plan`` for the (F, H, W) uint8 ``frames`` (contiguous frames any
    number of bytes apart, F <= plan.n_frames), on the device (fdf_pyramid_device): one resize
    per level in stream order, each from the level before.  ``buffer``: a contiguous uint8
    tensor of at least plan.total_bytes bytes; ``taps``: a 32-bit integer tensor holding
    plan.taps().  Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    if not isinstance(plan, PyramidPlan):
        raise TypeError("plan must be a PyramidPlan (pyramid_plan)")
    _check_frames(torch, frames)
    f, h, w = frames.shape
    if (w, h) != (plan.levels[0].width, plan.levels[0].height):
        raise ValueError("frames do not have the plan's level-0 size")
    if f > plan.n_frames:
        raise ValueError("more frames than the plan was made for")
    if buffer.dtype != torch.uint8 or not buffer.is_contiguous() or \
            buffer.numel() < plan.total_bytes:
        raise ValueError("buffer must be a contiguous uint8 tensor of plan.total_bytes bytes")
    _check_taps(taps, plan.total_taps, "taps")
    _check_one_device("pyramid_device", [frames, buffer, taps])
    dev, stream = _device_stream(torch, frames, device, stream)
    ptr, _, _, _, stride = _frame_args(frames)
    rc = _native.load().fdf_pyramid_device(
        context(dev).handle, ptr, f, stride, plan._c, len(plan), buffer.data_ptr(),
        taps.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_pyramid_device")


class Pyramid:
    """The scale pyramid of device-resident ``frames`` ((F, H, W) uint8): the plan, its taps on
    the device and one buffer for the levels >= 1.  ``level(l)`` is a contiguous (F, h_l, w_l)
    uint8 view usable by detect_device, smooth_device, orient_device and describe_device;
    ``level(0)`` is ``frames`` itself.  ``build()`` (run by the constructor unless
    ``build=False``) enqueues the resizes; call it again after the frames change."""

    def __init__(self, frames, n_levels=8, scale=(6, 5), stream=None, build=True):
        import torch

        _check_frames(torch, frames)
        if not frames.is_cuda:
            raise ValueError("Pyramid needs a CUDA (HIP) tensor")
        f, h, w = frames.shape
        self.frames = frames
        self.plan = pyramid_plan((h, w), n_levels, scale, f)
        self.taps = _device_taps(torch, self.plan.taps(), frames.device)
        self.buffer = torch.empty(max(self.plan.total_bytes, 1), dtype=torch.uint8,
                                  device=frames.device)
        if build:
            self.build(stream)

    def __len__(self):
        return len(self.plan)

    def build(self, stream=None):
        pyramid_device(self.frames, self.plan, self.buffer, self.taps, stream=stream)

    def level(self, l):
        if not 0 <= l < len(self.plan):
            raise IndexError("no such level")
        if l == 0:
            return self.frames
        L = self.plan.levels[l]
        f = self.frames.shape[0]
        n = f * L.frame_stride_bytes
        return self.buffer[L.offset_bytes:L.offset_bytes + n].view(f, L.height, L.width)


MultiscaleKeypoints = collections.namedtuple(
    "MultiscaleKeypoints", "level points points0 scores angles descriptors sizes")


def detect_multiscale_array(img, config, n_levels=8, scale=(6, 5), cell=None, k=None, radius=15,
                            n_bins=30, device=0, rank="fast", block=7, harris_k=(1, 25)):
    """The keypoints of one host image over its scale pyramid: the image goes to the device
    once, the pyramid is built there (:class:`Pyramid`) and every level runs the device chain
    detect, score, (with ``cell`` = (cell_w, cell_h) and ``k``: best-k selection per cell,)
    orient on the level, describe on its 5 x 5 smoothed copy (default pattern, ``n_bins``
    rotations).  ``rank`` = "fast" scores with the detector's score (score_device),
    "harris" with the Harris rank score of the level (harris_device with ``block`` and the
    Harris constant ``harris_k`` = (k_num, k_den); ``k`` is taken by the selection), ORB's
    ranking: those scores feed the selection and are returned.  Returns :class:`MultiscaleKeypoints`, ordered by level, then raster:
    ``level`` (K,) int32, ``points`` (K, 2) uint32 level coordinates, ``points0`` (K, 2) float32
    level-0 coordinates ((x_l + 0.5) * w_0 / w_l - 0.5 per axis, in float64, rounded once),
    ``scores`` (K,) uint16, ``angles`` (K,) float32, ``descriptors`` (K, 32) uint8 and ``sizes``,
    the (width, height) of every level.  Levels too small to hold a keypoint (a side below 7)
    contribute none."""
    import torch

    if (cell is None) != (k is None):
        raise ValueError("cell and k go together")
    if cell is not None:
        cw, ch, k = _cell_k(cell, k)
        cell = (cw, ch)
    if rank not in ("fast", "harris"):
        raise ValueError('rank must be "fast" or "harris"')
    hb, hnum, hden = _harris_args(block, harris_k)
    r = _radius(radius)
    bins = _n_bins(n_bins)
    arr = _as_pixels(img)
    h0, w0 = arr.shape
    plan = pyramid_plan((h0, w0), n_levels, scale, 1)   # the plan's errors before any device call
    _to_c_config(config)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        frames = torch.from_numpy(np.ascontiguousarray(arr)[None].copy()).to(dev)
        pyr = Pyramid(frames, n_levels, scale)
        table = torch.from_numpy(brief_steer(brief_pattern(), bins)).to(dev)
        out = {name: [] for name in ("level", "points", "points0", "scores", "angles",
                                     "descriptors")}
        for l, L in enumerate(plan.levels):
            w, h = L.width, L.height
            if w < 7 or h < 7:
                continue
            level = pyr.level(l)
            cap = capacity_guess(w * h)
            offs = torch.zeros(2, dtype=torch.int64, device=dev)
            while True:
                pts = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
                detect_device(level, config, pts, offs)
                total = int(offs[1])
                if total <= cap:
                    break
                cap = total
            if total == 0:
                continue
            pts = pts[:total]
            scores = torch.zeros(total, dtype=torch.int16, device=dev)
            if rank == "harris":
                harris_device(level, pts, offs, scores, hb, (hnum, hden))
            else:
                score_device(level, config, pts, offs, scores)
            if cell is not None:
                sel = torch.zeros((total, 2), dtype=torch.int32, device=dev)
                sel_scores = torch.zeros(total, dtype=torch.int16, device=dev)
                sel_offs = torch.zeros(2, dtype=torch.int64, device=dev)
                select_device(pts, scores, offs, (h, w), cell, k, sel, sel_scores, sel_offs)
                total = int(sel_offs[1])
                pts, scores, offs = sel[:total], sel_scores[:total], sel_offs
            angles = torch.zeros(total, dtype=torch.float32, device=dev)
            orient_device(level, pts, offs, angles, radius=r)
            smoothed = torch.empty_like(level)
            smooth_device(level, smoothed)
            desc = torch.zeros((total, 32), dtype=torch.uint8, device=dev)
            describe_device(smoothed, pts, offs, desc, table, bins, angles=angles)
            p = pts.cpu().numpy().view(np.uint32)
            out["level"].append(np.full(total, l, dtype=np.int32))
            out["points"].append(p)
            out["points0"].append(((p.astype(np.float64) + 0.5) *
                                   np.array([w0, h0], dtype=np.float64) /
                                   np.array([w, h], dtype=np.float64) - 0.5).astype(np.float32))
            out["scores"].append(scores.cpu().numpy().view(np.uint16))
            out["angles"].append(angles.cpu().numpy())
            out["descriptors"].append(desc.cpu().numpy())
    empty = {"level": np.zeros(0, np.int32), "points": np.zeros((0, 2), np.uint32),
             "points0": np.zeros((0, 2), np.float32), "scores": np.zeros(0, np.uint16),
             "angles": np.zeros(0, np.float32), "descriptors": np.zeros((0, 32), np.uint8)}
    merged = {name: np.concatenate(v) if v else empty[name] for name, v in out.items()}
    return MultiscaleKeypoints(sizes=tuple((L.width, L.height) for L in plan.levels), **merged)


# include/fdf.h fdf_match as a numpy record; the (n, 2) 32-bit layout of the device wrappers
# holds the same 8 bytes: column 0 the index, column 1 distance | second << 16.
MATCH_DTYPE = np.dtype([("index", "<u4"), ("distance", "<u2"), ("second", "<u2")])
MATCH_NONE = _native.FDF_MATCH_NONE
MATCH_NO_DISTANCE = _native.FDF_MATCH_NO_DISTANCE
_MATCH_MAX_CAP = 0xFFFFFFFE


def _check_desc(torch, t, name):
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous (cap, 32) uint8 tensor")
    if t.shape[0] > _MATCH_MAX_CAP:
        raise ValueError(f"{name} must have fewer than 2^32 - 1 rows")
    if t.data_ptr() % 4:
        raise ValueError(f"{name} must be 4-byte aligned")


def _check_matches(t, name, rows, cap=0):
    _check_points(t, name, rows)
    if t.shape[0] < cap or t.shape[0] > _MATCH_MAX_CAP:
        raise ValueError(f"{name} must have at least {rows} and fewer than 2^32 - 1 rows")
    if t.data_ptr() % 8:
        raise ValueError(f"{name} must be 8-byte aligned")


def _match_frames(torch, q_offsets, t_offsets=None):
    """n_frames of a match call: the offsets' length less one."""
    _check_offsets(torch, q_offsets, 1, "q_offsets")
    n = q_offsets.numel() - 1
    if t_offsets is not None:
        _check_offsets(torch, t_offsets, 1, "t_offsets")
        if t_offsets.numel() != q_offsets.numel():
            raise ValueError("q_offsets and t_offsets must have the same length")
    if n > 65535:
        raise ValueError("at most 65535 frames")
    return n


def _window(window, have_points):
    """(max_dx, max_dy) of a match call; (0, 0) without points."""
    if not have_points:
        if window is not None:
            raise ValueError("a window needs q_points and t_points")
        return 0, 0
    if window is None:
        raise ValueError("q_points and t_points need a window (max_dx, max_dy)")
    try:
        dx, dy = (int(v) for v in window)
    except (TypeError, ValueError):
        raise TypeError("window must be a pair (max_dx, max_dy) of integers") from None
    if not (0 <= dx <= 0xffffffff and 0 <= dy <= 0xffffffff):
        raise ValueError("window terms must fit u32")
    return dx, dy


def _ratio(ratio):
    """(num, den) of the ratio test; (0, 0) when it is off."""
    if ratio is None:
        return 0, 0
    try:
        num, den = (int(v) for v in ratio)
    except (TypeError, ValueError):
        raise TypeError("ratio must be a pair (num, den) of integers") from None
    if not (0 <= num <= 65535 and 0 <= den <= 65535):
        raise ValueError("ratio terms must be in 0..65535")
    return num, den


def _max_distance(max_distance):
    d = int(max_distance)
    if not 0 <= d <= 0xffffffff:
        raise ValueError("max_distance must fit u32")
    return d


def match_device(q_desc, q_offsets, t_desc, t_offsets, matches, q_points=None, t_points=None,
                 window=None, stream=None, device=None):
    """Brute-force Hamming matching of describe_device's output, on the device
    (fdf_match_device): frame f of the query set (``q_desc`` (q_cap, 32) uint8, ``q_offsets``
    (F+1,) int64) against frame f of the train set (``t_desc``, ``t_offsets``, the same
    length).  The two sets may be one tensor: ``offs[:-1]`` / ``offs[1:]`` over the same
    ``desc`` match every frame against the next.  ``matches`` (q_cap, 2) 32-bit integers gets
    per query the global train index of the nearest descriptor (ties: the lowest index; -1 =
    none) in column 0 and distance | second << 16 in column 1 (unpack_matches).  With
    ``q_points`` / ``t_points`` ((cap, 2), as detect_device filled them; each train frame's y
    non-decreasing) and ``window`` = (max_dx, max_dy) only train points within the window
    are candidates.  Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    _check_desc(torch, q_desc, "q_desc")
    _check_desc(torch, t_desc, "t_desc")
    q_cap, t_cap = q_desc.shape[0], t_desc.shape[0]
    _check_matches(matches, "matches", "q_cap", q_cap)
    n = _match_frames(torch, q_offsets, t_offsets)
    if (q_points is None) != (t_points is None):
        raise ValueError("q_points and t_points go together")
    have_points = q_points is not None
    if have_points:
        _check_points(q_points, "q_points", "q_cap")
        _check_points(t_points, "t_points", "t_cap")
        if q_points.shape[0] < q_cap or t_points.shape[0] < t_cap:
            raise ValueError("q_points / t_points must have a row per descriptor")
    dx, dy = _window(window, have_points)
    _check_one_device("match_device", [q_desc, q_offsets, t_desc, t_offsets, matches] +
                      ([q_points, t_points] if have_points else []))
    dev, stream = _device_stream(torch, q_desc, device, stream)
    rc = _native.load().fdf_match_device(
        context(dev).handle, n, q_desc.data_ptr(),
        q_points.data_ptr() if have_points else None, q_cap, q_offsets.data_ptr(),
        t_desc.data_ptr(), t_points.data_ptr() if have_points else None, t_cap,
        t_offsets.data_ptr(), dx, dy, matches.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_match_device")


def match_filter_device(matches, q_offsets, keep, reverse=None, max_distance=256, ratio=None,
                        stream=None, device=None):
    """The usual tests on match_device's output, on the device (fdf_match_filter_device):
    ``keep`` (q_cap,) uint8 gets 1 for every query of ``q_offsets``' frames whose match exists,
    has distance <= ``max_distance`` (256 and above: off), passes the ratio test distance * den
    < second * num for ``ratio`` = (num, den) (None: off; Lowe's 0.75 is (3, 4)) and, with
    ``reverse`` (the (t_cap, 2) matches of the swapped sets), is its match's match; 0 for the
    others.  Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    _check_matches(matches, "matches", "q_cap")
    q_cap = matches.shape[0]
    if keep.dtype != torch.uint8 or keep.dim() != 1 or keep.numel() < q_cap or \
            not keep.is_contiguous():
        raise ValueError("keep must be a contiguous uint8 tensor with q_cap entries")
    if reverse is not None:
        _check_matches(reverse, "reverse", "t_cap")
    n = _match_frames(torch, q_offsets)
    num, den = _ratio(ratio)
    dist = _max_distance(max_distance)
    _check_one_device("match_filter_device",
                      [matches, q_offsets, keep] + ([reverse] if reverse is not None else []))
    dev, stream = _device_stream(torch, matches, device, stream)
    rc = _native.load().fdf_match_filter_device(
        context(dev).handle, n, matches.data_ptr(), q_cap, q_offsets.data_ptr(),
        reverse.data_ptr() if reverse is not None else None,
        reverse.shape[0] if reverse is not None else 0, dist, num, den, keep.data_ptr(),
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_match_filter_device")


def unpack_matches(array):
    """(index, distance, second) of a matches array in either layout, the (n,) records of
    MATCH_DTYPE or the (n, 2) 32-bit integers of match_device: index as int64 with -1 for no
    match, distance and second as uint16 (0xFFFF: none)."""
    a = np.asarray(array)
    if a.dtype == MATCH_DTYPE and a.ndim == 1:
        rec = a
    elif a.ndim == 2 and a.shape[1] == 2 and a.dtype.kind in "ui" and a.dtype.itemsize == 4:
        rec = np.ascontiguousarray(a).view(MATCH_DTYPE).reshape(-1)
    else:
        raise TypeError("expected (n,) match records or an (n, 2) 32-bit integer array")
    index = rec["index"].astype(np.int64)
    index[rec["index"] == MATCH_NONE] = -1
    return index, rec["distance"].copy(), rec["second"].copy()


def _host_desc(desc, name):
    d = np.asarray(desc)
    if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 32:
        raise TypeError(f"{name} must be a (K, 32) uint8 array")
    return np.ascontiguousarray(d)


def _match_points(q, t, qp, tp, dx, dy, device):
    out = np.zeros(len(q), dtype=MATCH_DTYPE)
    rc = _native.load().fdf_match_points(
        context(device).handle, q.ctypes.data if len(q) else None,
        qp.ctypes.data if qp is not None else None, len(q), t.ctypes.data if len(t) else None,
        tp.ctypes.data if tp is not None else None, len(t), dx, dy,
        out.ctypes.data if len(q) else None)
    check(rc, "fdf_match_points")
    return out


def match_descriptors(q_desc, t_desc, q_points=None, t_points=None, window=None,
                      cross_check=False, ratio=None, max_distance=256, device=0):
    """Nearest and second nearest train descriptor of every query descriptor
    (fdf_match_points): (n_q,) records of MATCH_DTYPE (index = MATCH_NONE: no candidate).
    ``q_desc`` (n_q, 32) and ``t_desc`` (n_t, 32) uint8; with ``q_points`` / ``t_points``
    ((n, 2), the train points' y non-decreasing) and ``window`` = (max_dx, max_dy) only train
    points within the window are candidates.  When a filter is asked for -- ``cross_check``,
    ``ratio`` = (num, den) or ``max_distance`` below 256 -- also returns the (n_q,) bool mask
    of the matches that pass (the rule of match_filter_device, applied on the host)."""
    q = _host_desc(q_desc, "q_desc")
    t = _host_desc(t_desc, "t_desc")
    if (q_points is None) != (t_points is None):
        raise ValueError("q_points and t_points go together")
    have_points = q_points is not None
    qp = tp = None
    if have_points:
        qp, tp = _host_points(q_points), _host_points(t_points)
        if len(qp) != len(q) or len(tp) != len(t):
            raise ValueError("one point per descriptor")
    dx, dy = _window(window, have_points)
    num, den = _ratio(ratio)
    dist = _max_distance(max_distance)
    fwd = _match_points(q, t, qp, tp, dx, dy, device)
    if not (cross_check or ratio is not None or dist < 256):
        return fwd
    d, s = fwd["distance"].astype(np.uint32), fwd["second"].astype(np.uint32)
    keep = fwd["index"] != MATCH_NONE
    if dist < 256:
        keep &= d <= dist
    if den:
        keep &= (s == MATCH_NO_DISTANCE) | (d * np.uint32(den) < s * np.uint32(num))
    if cross_check:
        rev = _match_points(t, q, tp, qp, dx, dy, device)
        at = np.minimum(fwd["index"], max(len(t) - 1, 0))
        back = rev["index"][at] if len(t) else np.full(len(q), MATCH_NONE, np.uint32)
        keep &= (fwd["index"] < len(t)) & (back == np.arange(len(q), dtype=np.uint32))
    return fwd, keep


# include/fdf.h fdf_model as a numpy record; the (F, 11) float64 layout of ransac_device holds the
# same 88 bytes per frame (unpack_models).
MODEL_DTYPE = np.dtype([("h", "<f8", (9,)), ("n_corr", "<u4"), ("n_inliers", "<u4"),
                        ("hypothesis", "<u4"), ("n_valid", "<u4")])
RANSAC_NONE = _native.FDF_RANSAC_NONE
_MODELS = {"affine": _native.FDF_MODEL_AFFINE, "homography": _native.FDF_MODEL_HOMOGRAPHY}
_RANSAC_MAX_HYP = 65536
_REFINE_MAX_ROUNDS = 8


def _ransac_model(model):
    try:
        return _MODELS[model]
    except (KeyError, TypeError):
        raise ValueError('model must be "affine" or "homography"') from None


def _ransac_values(n_hyp, threshold, seed):
    n_hyp, seed, threshold = int(n_hyp), int(seed), float(threshold)
    if not 1 <= n_hyp <= _RANSAC_MAX_HYP:
        raise ValueError("n_hyp must be in 1..65536")
    if not (np.isfinite(ctypes.c_float(threshold).value) and threshold >= 0):   # as the C float
        raise ValueError("threshold must be finite and not negative")
    if not 0 <= seed <= 0xffffffff:
        raise ValueError("seed must fit u32")
    return n_hyp, threshold, seed


def ransac_sample(seed, frame, hypothesis, m, s):
    """The sample of one RANSAC hypothesis (fdf_ransac_sample): (the ``s`` correspondence numbers
    below ``m`` or None when 16 draws do not give ``s`` distinct ones, the draws made)."""
    idx = (ctypes.c_uint32 * 4)()
    draws = ctypes.c_uint32()
    for name, v in (("seed", seed), ("frame", frame), ("hypothesis", hypothesis), ("m", m)):
        if not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must fit u32")
    if int(s) not in (3, 4):
        raise ValueError("s must be 3 or 4")
    check(_native.load().fdf_ransac_sample(int(seed), int(frame), int(hypothesis), int(m), int(s),
                                           idx, ctypes.byref(draws)), "fdf_ransac_sample")
    got = list(idx)[:int(s)]
    return (None if got[0] == RANSAC_NONE else got), draws.value


def ransac_scratch_bytes(n_frames, q_cap, n_hyp):
    """Bytes of ransac_device's scratch tensor (fdf_ransac_scratch_bytes)."""
    n_frames, q_cap, n_hyp = int(n_frames), int(q_cap), int(n_hyp)
    if not (0 <= n_frames <= 65535 and 0 <= q_cap <= _MATCH_MAX_CAP):
        raise ValueError("at most 65535 frames and fewer than 2^32 - 1 queries")
    if not 1 <= n_hyp <= _RANSAC_MAX_HYP:
        raise ValueError("n_hyp must be in 1..65536")
    v = ctypes.c_uint64()
    check(_native.load().fdf_ransac_scratch_bytes(n_frames, q_cap, n_hyp, ctypes.byref(v)),
          "fdf_ransac_scratch_bytes")
    return v.value


def _check_coords(torch, t, name, rows, cap=0):
    """FDF_COORDS_* of a (cap, 2) tensor of 32-bit integers or float32."""
    if t.dim() != 2 or t.shape[1] != 2 or t.element_size() != 4 or not t.is_contiguous() or \
            t.is_complex() or t.shape[0] < cap or t.shape[0] > _MATCH_MAX_CAP:
        raise ValueError(f"{name} must be a contiguous ({rows}, 2) tensor of 32-bit integers or "
                         "float32")
    if t.data_ptr() % 8:
        raise ValueError(f"{name} must be 8-byte aligned")
    return _native.FDF_COORDS_F32 if t.is_floating_point() else _native.FDF_COORDS_U32


def ransac_device(matches, q_offsets, q_coords, t_coords, t_offsets, models, scratch, keep=None,
                  inliers=None, model="homography", n_hyp=256, threshold=3.0, seed=0,
                  stream=None, device=None):
    """RANSAC estimation of one affine map or homography per frame from match_device's output,
    on the device (fdf_ransac_device).  ``matches`` (q_cap, 2) and ``q_offsets`` / ``t_offsets``
    are match_device's, ``keep`` (optional) match_filter_device's; ``q_coords`` (q_cap, 2) and
    ``t_coords`` (t_cap, 2) are both 32-bit integers (as detect_device fills them) or both
    float32 (x, y).  ``models`` (F, 11) float64 gets one fdf_model per frame (unpack_models),
    ``inliers`` (optional, (q_cap,) uint8) 1 for the inliers of each frame's best model.
    ``scratch``: a uint8 tensor of ransac_scratch_bytes(F, q_cap, n_hyp), 256-byte aligned, no
    initialisation needed.  The result is a pure function of the inputs and ``seed``.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    _check_matches(matches, "matches", "q_cap")
    q_cap = matches.shape[0]
    n = _match_frames(torch, q_offsets, t_offsets)
    kind = _check_coords(torch, q_coords, "q_coords", "q_cap", q_cap)
    if _check_coords(torch, t_coords, "t_coords", "t_cap") != kind:
        raise ValueError("q_coords and t_coords must have the same type")
    t_cap = t_coords.shape[0]
    if models.dtype != torch.float64 or models.dim() != 2 or models.shape[1] != 11 or \
            models.shape[0] < n or not models.is_contiguous():
        raise ValueError("models must be a contiguous (F, 11) float64 tensor")
    for t, name in ((keep, "keep"), (inliers, "inliers")):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < q_cap or
                              not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor with q_cap entries")
    code = _ransac_model(model)
    n_hyp, threshold, seed = _ransac_values(n_hyp, threshold, seed)
    if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous() or \
            scratch.numel() < ransac_scratch_bytes(n, q_cap, n_hyp):
        raise ValueError("scratch must be a uint8 tensor of ransac_scratch_bytes(F, q_cap, n_hyp)")
    if scratch.data_ptr() % 256:
        raise ValueError("scratch must be 256-byte aligned")
    _check_one_device("ransac_device",
                      [matches, q_offsets, q_coords, t_coords, t_offsets, models, scratch] +
                      [t for t in (keep, inliers) if t is not None])
    dev, stream = _device_stream(torch, matches, device, stream)
    rc = _native.load().fdf_ransac_device(
        context(dev).handle, n, matches.data_ptr(), keep.data_ptr() if keep is not None else None,
        q_cap, q_offsets.data_ptr(), q_coords.data_ptr(), t_coords.data_ptr(), t_cap,
        t_offsets.data_ptr(), kind, code, n_hyp, threshold, seed, models.data_ptr(),
        inliers.data_ptr() if inliers is not None else None, scratch.data_ptr(),
        scratch.numel(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_ransac_device")


def unpack_models(array):
    """(F,) records of MODEL_DTYPE from ransac_device's (F, 11) float64 array (a copy)."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 11:
        raise TypeError("expected an (F, 11) float64 array")
    return a.view(MODEL_DTYPE).reshape(-1).copy()


def _host_coords(points, name):
    """(contiguous (K, 2) uint32 or float32 array, FDF_COORDS_*)."""
    pts = np.asarray(points)
    if pts.ndim == 2 and pts.shape[1] == 2 and pts.dtype == np.float32:
        return np.ascontiguousarray(pts), _native.FDF_COORDS_F32
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "ui":
        raise TypeError(f"{name} must be a (K, 2) integer or float32 array")
    return _host_points(pts), _native.FDF_COORDS_U32


def _host_matches(matches, n):
    """(n,) MATCH_DTYPE records from records, the (n, 2) device layout, or (n,) train indices
    (a negative one: no match)."""
    a = np.asarray(matches)
    if a.dtype == MATCH_DTYPE and a.ndim == 1:
        rec = np.ascontiguousarray(a)
    elif a.ndim == 2 and a.shape[1] == 2 and a.dtype.kind in "ui" and a.dtype.itemsize == 4:
        rec = np.ascontiguousarray(a).view(MATCH_DTYPE).reshape(-1)
    elif a.ndim == 1 and a.dtype.kind in "ui":
        rec = np.zeros(len(a), dtype=MATCH_DTYPE)
        index = a.astype(np.int64)
        if index.size and index.max() > MATCH_NONE:
            raise ValueError("match indices must fit u32")
        rec["index"] = np.where(index < 0, MATCH_NONE, index)
    else:
        raise TypeError("matches must be match records, an (n, 2) 32-bit integer array or (n,) "
                        "train indices")
    if len(rec) != n:
        raise ValueError("one match per query point")
    return rec


def _host_pair(q_points, t_points, matches, keep):
    """The host sets of estimate_model and refine_model: (q, t, FDF_COORDS_*, records, keep)."""
    q, kind = _host_coords(q_points, "q_points")
    t, t_kind = _host_coords(t_points, "t_points")
    if kind != t_kind:
        raise TypeError("q_points and t_points must have the same type")
    rec = _host_matches(matches, len(q))
    if keep is not None:
        keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if keep.shape != (len(q),):
            raise ValueError("keep must have one entry per query point")
    return q, t, kind, rec, keep


def _refine_rounds(n_rounds):
    n_rounds = int(n_rounds)
    if not 0 <= n_rounds <= _REFINE_MAX_ROUNDS:
        raise ValueError("n_rounds must be in 0..8")
    return n_rounds


def _refine_points(q, t, kind, rec, keep, code, start, threshold, n_rounds, device):
    """fdf_refine_points on _host_pair's arrays: (the refined (1,) record, the uint8 mask, the
    accepted rounds)."""
    out = np.zeros(1, dtype=MODEL_DTYPE)
    mask = np.zeros(len(q), dtype=np.uint8)
    rounds = ctypes.c_uint32()
    rc = _native.load().fdf_refine_points(
        context(device).handle, q.ctypes.data if len(q) else None,
        t.ctypes.data if len(t) else None, len(q), len(t), rec.ctypes.data if len(q) else None,
        keep.ctypes.data if keep is not None and len(q) else None, kind, code, start.ctypes.data,
        threshold, n_rounds, out.ctypes.data, mask.ctypes.data if len(q) else None,
        ctypes.addressof(rounds))
    check(rc, "fdf_refine_points")
    return out, mask, rounds.value


def estimate_model(q_points, t_points, matches, keep=None, model="homography", n_hyp=256,
                   threshold=3.0, seed=0, device=0, refine_rounds=0):
    """RANSAC estimation of the affine map or homography that takes the query points to their
    matches (fdf_ransac_points): (H as a (3, 3) float64 array or None when there is no model, the
    (n_q,) bool inlier mask, the MODEL_DTYPE record).  ``q_points`` (n_q, 2) and ``t_points``
    (n_t, 2) are both integer or both float32 arrays of (x, y); ``matches`` is match_descriptors'
    result (or (n_q,) train indices, negative = none), ``keep`` an optional (n_q,) mask.
    ``refine_rounds`` > 0 refits the model over its inliers that many times at most
    (fdf_refine_points, the same threshold); 0 leaves the minimal sample's model."""
    q, t, kind, rec, keep = _host_pair(q_points, t_points, matches, keep)
    code = _ransac_model(model)
    n_hyp, threshold, seed = _ransac_values(n_hyp, threshold, seed)
    refine_rounds = _refine_rounds(refine_rounds)
    out = np.zeros(1, dtype=MODEL_DTYPE)
    mask = np.zeros(len(q), dtype=np.uint8)
    rc = _native.load().fdf_ransac_points(
        context(device).handle, q.ctypes.data if len(q) else None,
        t.ctypes.data if len(t) else None, len(q), len(t), rec.ctypes.data if len(q) else None,
        keep.ctypes.data if keep is not None and len(q) else None, kind, code, n_hyp, threshold,
        seed, out.ctypes.data, mask.ctypes.data if len(q) else None)
    check(rc, "fdf_ransac_points")
    if refine_rounds:
        out, mask, _ = _refine_points(q, t, kind, rec, keep, code, out, threshold, refine_rounds,
                                      device)
    found = out["hypothesis"][0] != RANSAC_NONE
    return (out["h"][0].reshape(3, 3).copy() if found else None), mask.astype(bool), out[0]


def refine_scratch_bytes(n_frames, q_cap):
    """Bytes of refine_device's scratch tensor (fdf_refine_scratch_bytes)."""
    n_frames, q_cap = int(n_frames), int(q_cap)
    if not (0 <= n_frames <= 65535 and 0 <= q_cap <= _MATCH_MAX_CAP):
        raise ValueError("at most 65535 frames and fewer than 2^32 - 1 queries")
    v = ctypes.c_uint64()
    check(_native.load().fdf_refine_scratch_bytes(n_frames, q_cap, ctypes.byref(v)),
          "fdf_refine_scratch_bytes")
    return v.value


def refine_device(matches, q_offsets, q_coords, t_coords, t_offsets, models_in, models_out,
                  scratch, keep=None, inliers=None, rounds=None, model="homography",
                  threshold=3.0, n_rounds=2, stream=None, device=None):
    """Least-squares refinement of ransac_device's models over their inliers, on the device
    (fdf_refine_device).  The correspondences are ransac_device's (``matches``, ``q_offsets``,
    ``q_coords``, ``t_coords``, ``t_offsets``, ``keep``); ``models_in`` (F, 11) float64 holds the
    models to refine and ``models_out`` (which may be ``models_in``) gets the refined ones;
    ``inliers`` (optional, (q_cap,) uint8) gets their inliers under ``threshold`` and ``rounds``
    (optional, (F,) int32) the rounds each frame accepted, at most ``n_rounds`` (0..8).
    ``scratch``: a uint8 tensor of refine_scratch_bytes(F, q_cap), 256-byte aligned, no
    initialisation needed.  The result is a pure function of the inputs.  Asynchronous on
    ``stream`` (default: torch's current stream)."""
    import torch

    _check_matches(matches, "matches", "q_cap")
    q_cap = matches.shape[0]
    n = _match_frames(torch, q_offsets, t_offsets)
    kind = _check_coords(torch, q_coords, "q_coords", "q_cap", q_cap)
    if _check_coords(torch, t_coords, "t_coords", "t_cap") != kind:
        raise ValueError("q_coords and t_coords must have the same type")
    t_cap = t_coords.shape[0]
    for t, name in ((models_in, "models_in"), (models_out, "models_out")):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 11 or t.shape[0] < n or \
                not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous (F, 11) float64 tensor")
    for t, name in ((keep, "keep"), (inliers, "inliers")):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < q_cap or
                              not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor with q_cap entries")
    if rounds is not None and (rounds.dtype != torch.int32 or rounds.dim() != 1 or
                               rounds.numel() < n or not rounds.is_contiguous()):
        raise ValueError("rounds must be a contiguous int32 tensor with F entries")
    code = _ransac_model(model)
    _, threshold, _ = _ransac_values(1, threshold, 0)
    n_rounds = _refine_rounds(n_rounds)
    if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous() or \
            scratch.numel() < refine_scratch_bytes(n, q_cap):
        raise ValueError("scratch must be a uint8 tensor of refine_scratch_bytes(F, q_cap)")
    if scratch.data_ptr() % 256:
        raise ValueError("scratch must be 256-byte aligned")
    _check_one_device("refine_device",
                      [matches, q_offsets, q_coords, t_coords, t_offsets, models_in, models_out,
                       scratch] + [t for t in (keep, inliers, rounds) if t is not None])
    dev, stream = _device_stream(torch, matches, device, stream)
    rc = _native.load().fdf_refine_device(
        context(dev).handle, n, matches.data_ptr(), keep.data_ptr() if keep is not None else None,
        q_cap, q_offsets.data_ptr(), q_coords.data_ptr(), t_coords.data_ptr(), t_cap,
        t_offsets.data_ptr(), kind, code, models_in.data_ptr(), threshold, n_rounds,
        models_out.data_ptr(), inliers.data_ptr() if inliers is not None else None,
        rounds.data_ptr() if rounds is not None else None, scratch.data_ptr(), scratch.numel(),
        ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_refine_device")


def refine_model(q_points, t_points, matches, estimate, keep=None, model="homography",
                 threshold=3.0, n_rounds=2, device=0):
    """Least-squares refinement of one model over its inliers (fdf_refine_points): (H as a (3, 3)
    float64 array or None when ``estimate`` holds no model, the (n_q,) bool inlier mask, the
    MODEL_DTYPE record, the rounds accepted).  The point sets, ``matches`` and ``keep`` are
    estimate_model's; ``estimate`` is its record, or a (3, 3) array to start from."""
    q, t, kind, rec, keep = _host_pair(q_points, t_points, matches, keep)
    code = _ransac_model(model)
    _, threshold, _ = _ransac_values(1, threshold, 0)
    n_rounds = _refine_rounds(n_rounds)
    start = np.zeros(1, dtype=MODEL_DTYPE)
    given = np.asarray(estimate)
    if given.dtype == MODEL_DTYPE and given.size == 1:
        start[0] = given.reshape(-1)[0]
    elif given.dtype.kind in "fiu" and given.size == 9:
        start["h"][0] = given.astype(np.float64).reshape(-1)
    else:
        raise TypeError("estimate must be a MODEL_DTYPE record or a (3, 3) array")
    out, mask, rounds = _refine_points(q, t, kind, rec, keep, code, start, threshold, n_rounds,
                                       device)
    found = out["hypothesis"][0] != RANSAC_NONE
    return (out["h"][0].reshape(3, 3).copy() if found else None), mask.astype(bool), out[0], rounds


# RANSAC fundamental-matrix estimation (fdf_fundamental.hip; include/fdf.h has the rule).

def fundamental_sample(seed, frame, hypothesis, m):
    """The sample of one fundamental-matrix hypothesis (fdf_fundamental_sample): (the 8
    correspondence numbers below ``m`` or None when 32 draws do not give 8 distinct ones, the
    draws made)."""
    idx = (ctypes.c_uint32 * 8)()
    draws = ctypes.c_uint32()
    for name, v in (("seed", seed), ("frame", frame), ("hypothesis", hypothesis), ("m", m)):
        if not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must fit u32")
    check(_native.load().fdf_fundamental_sample(int(seed), int(frame), int(hypothesis), int(m),
                                                idx, ctypes.byref(draws)),
          "fdf_fundamental_sample")
    got = list(idx)
    return (None if got[0] == RANSAC_NONE else got), draws.value


def fundamental_scratch_bytes(n_frames, q_cap, n_hyp):
    """Bytes of fundamental_device's scratch tensor (fdf_fundamental_scratch_bytes)."""
    n_frames, q_cap, n_hyp = int(n_frames), int(q_cap), int(n_hyp)
    if not (0 <= n_frames <= 65535 and 0 <= q_cap <= _MATCH_MAX_CAP):
        raise ValueError("at most 65535 frames and fewer than 2^32 - 1 queries")
    if not 1 <= n_hyp <= _RANSAC_MAX_HYP:
        raise ValueError("n_hyp must be in 1..65536")
    v = ctypes.c_uint64()
    check(_native.load().fdf_fundamental_scratch_bytes(n_frames, q_cap, n_hyp, ctypes.byref(v)),
          "fdf_fundamental_scratch_bytes")
    return v.value


def _fundamental_sets(torch, matches, q_offsets, q_coords, t_coords, t_offsets, models,
                      keep, inliers):
    """The checks that fundamental_device and fundamental_check_device share: (F, q_cap, t_cap,
    FDF_COORDS_*).  ``models``: (name, tensor) pairs."""
    _check_matches(matches, "matches", "q_cap")
    q_cap = matches.shape[0]
    n = _match_frames(torch, q_offsets, t_offsets)
    kind = _check_coords(torch, q_coords, "q_coords", "q_cap", q_cap)
    if _check_coords(torch, t_coords, "t_coords", "t_cap") != kind:
        raise ValueError("q_coords and t_coords must have the same type")
    for name, t in models:
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 11 or t.shape[0] < n or \
                not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous (F, 11) float64 tensor")
    for t, name in ((keep, "keep"), (inliers, "inliers")):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < q_cap or
                              not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor with q_cap entries")
    return n, q_cap, t_coords.shape[0], kind


def fundamental_device(matches, q_offsets, q_coords, t_coords, t_offsets, models, scratch,
                       keep=None, inliers=None, n_hyp=256, threshold=1.0, seed=0, stream=None,
                       device=None):
    """RANSAC estimation of one fundamental matrix per frame on the device
    (fdf_fundamental_device): the epipolar outlier test of a moving camera or a stereo pair.  The
    arguments are ransac_device's without ``model`` (track_device's ``matches``, ``status`` as
    ``keep`` and float positions go in as they are); ``threshold`` is a Sampson distance in
    pixels.  ``models`` (F, 11) float64 gets one fdf_model per frame (unpack_models) whose h is
    F with [u v 1] F [x y 1]^T = 0, ``inliers`` (optional, (q_cap,) uint8) 1 for the inliers of
    each frame's best F.  ``scratch``: a uint8 tensor of fundamental_scratch_bytes(F, q_cap,
    n_hyp), 256-byte aligned.  The result is a pure function of the inputs and ``seed``.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    n, q_cap, t_cap, kind = _fundamental_sets(torch, matches, q_offsets, q_coords, t_coords,
                                              t_offsets, (("models", models),), keep, inliers)
    n_hyp, threshold, seed = _ransac_values(n_hyp, threshold, seed)
    if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous() or \
            scratch.numel() < fundamental_scratch_bytes(n, q_cap, n_hyp):
        raise ValueError("scratch must be a uint8 tensor of fundamental_scratch_bytes(F, q_cap, "
                         "n_hyp)")
    if scratch.data_ptr() % 256:
        raise ValueError("scratch must be 256-byte aligned")
    _check_one_device("fundamental_device",
                      [matches, q_offsets, q_coords, t_coords, t_offsets, models, scratch] +
                      [t for t in (keep, inliers) if t is not None])
    dev, stream = _device_stream(torch, matches, device, stream)
    rc = _native.load().fdf_fundamental_device(
        context(dev).handle, n, matches.data_ptr(), keep.data_ptr() if keep is not None else None,
        q_cap, q_offsets.data_ptr(), q_coords.data_ptr(), t_coords.data_ptr(), t_cap,
        t_offsets.data_ptr(), kind, n_hyp, threshold, seed, models.data_ptr(),
        inliers.data_ptr() if inliers is not None else None, scratch.data_ptr(),
        scratch.numel(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_fundamental_device")


def fundamental_check_device(matches, q_offsets, q_coords, t_coords, t_offsets, models_in,
                             models_out, keep=None, inliers=None, threshold=1.0, stream=None,
                             device=None):
    """The caller's fundamental matrices recounted on the device (fdf_fundamental_check_device):
    no sampling.  ``models_in`` (F, 11) float64 holds one fdf_model per frame (a stereo rig's F,
    or fundamental_device's result to recount under another ``threshold``); ``models_out`` (may
    be ``models_in``) gets them with n_corr and n_inliers recounted, ``inliers`` (optional) the
    inlier bytes.  A record whose hypothesis is RANSAC_NONE holds no model and is copied.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    n, q_cap, t_cap, kind = _fundamental_sets(torch, matches, q_offsets, q_coords, t_coords,
                                              t_offsets, (("models_in", models_in),
                                                          ("models_out", models_out)), keep,
                                              inliers)
    _, threshold, _ = _ransac_values(1, threshold, 0)
    _check_one_device("fundamental_check_device",
                      [matches, q_offsets, q_coords, t_coords, t_offsets, models_in, models_out] +
                      [t for t in (keep, inliers) if t is not None])
    dev, stream = _device_stream(torch, matches, device, stream)
    rc = _native.load().fdf_fundamental_check_device(
        context(dev).handle, n, matches.data_ptr(), keep.data_ptr() if keep is not None else None,
        q_cap, q_offsets.data_ptr(), q_coords.data_ptr(), t_coords.data_ptr(), t_cap,
        t_offsets.data_ptr(), kind, models_in.data_ptr(), threshold, models_out.data_ptr(),
        inliers.data_ptr() if inliers is not None else None, ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_fundamental_check_device")


def estimate_fundamental(q_points, t_points, matches, keep=None, n_hyp=256, threshold=1.0, seed=0,
                         device=0):
    """RANSAC estimation of the fundamental matrix of the matches (fdf_fundamental_points): (F
    as a (3, 3) float64 array with [u v 1] F [x y 1]^T = 0, or None when there is no model, the
    (n_q,) bool inlier mask, the MODEL_DTYPE record).  The point sets, ``matches`` and ``keep``
    are estimate_model's; ``threshold`` is a Sampson distance in pixels."""
    q, t, kind, rec, keep = _host_pair(q_points, t_points, matches, keep)
    n_hyp, threshold, seed = _ransac_values(n_hyp, threshold, seed)
    out = np.zeros(1, dtype=MODEL_DTYPE)
    mask = np.zeros(len(q), dtype=np.uint8)
    rc = _native.load().fdf_fundamental_points(
        context(device).handle, q.ctypes.data if len(q) else None,
        t.ctypes.data if len(t) else None, len(q), len(t), rec.ctypes.data if len(q) else None,
        keep.ctypes.data if keep is not None and len(q) else None, kind, n_hyp, threshold, seed,
        out.ctypes.data, mask.ctypes.data if len(q) else None)
    check(rc, "fdf_fundamental_points")
    found = out["hypothesis"][0] != RANSAC_NONE
    return (out["h"][0].reshape(3, 3).copy() if found else None), mask.astype(bool), out[0]


# Pyramidal Lucas-Kanade tracking (fdf_track.hip; include/fdf.h has the rule).

TRACK_REASONS = ("skipped", "tracked", "eigenvalue", "left the frame", "step too large")
TrackResult = collections.namedtuple("TrackResult", "q11 xy status err reason iterations")


def _track_map(fn, name, v, a, b):
    v, a, b = int(v), int(a), int(b)
    if not (-(1 << 63) <= v < (1 << 63) and 0 <= a <= 0xffffffff and 0 <= b <= 0xffffffff):
        raise ValueError("arguments must fit int64 and u32")
    out = ctypes.c_int64()
    check(fn(v, a, b, ctypes.byref(out)), name)
    return out.value


def track_map_position(x, len0, len_l):
    """A level-0 position ``x`` in 1/2048 pixel on an axis of ``len0`` pixels at a level of
    ``len_l`` pixels (fdf_track_map_position; host only, no device)."""
    return _track_map(_native.load().fdf_track_map_position, "fdf_track_map_position", x, len0,
                      len_l)


def track_map_displacement(d, len_from, len_to):
    """A displacement ``d`` in 1/2048 pixel carried from a level of ``len_from`` pixels to one of
    ``len_to`` (fdf_track_map_displacement; host only, no device)."""
    return _track_map(_native.load().fdf_track_map_displacement, "fdf_track_map_displacement", d,
                      len_from, len_to)


def _track_coords(coords):
    try:
        return {"u32": _native.FDF_COORDS_U32, "q11": _native.FDF_COORDS_Q11}[coords]
    except (KeyError, TypeError):
        raise ValueError('coords must be "u32" or "q11"') from None


def _track_values(radius, max_iters, eps, min_eig):
    radius, max_iters, eps, min_eig = int(radius), int(max_iters), int(eps), float(min_eig)
    if not 1 <= radius <= 15:
        raise ValueError("radius must be in 1..15")
    if not 1 <= max_iters <= 64:
        raise ValueError("max_iters must be in 1..64")
    if not 0 <= eps <= 0xffffffff:
        raise ValueError("eps must fit u32")
    if not (min_eig >= 0.0 and np.isfinite(np.float32(min_eig))):
        raise ValueError("min_eig must be finite and not negative")
    return radius, max_iters, eps, min_eig


def _track_set(torch, side, name):
    """(frames, buffer or None, plan) of a Pyramid or of such a triple."""
    if isinstance(side, Pyramid):
        side = (side.frames, side.buffer, side.plan)
    try:
        frames, buffer, plan = side
    except (TypeError, ValueError):
        raise TypeError(f"{name} must be a Pyramid or (frames, buffer, plan)") from None
    if not isinstance(plan, PyramidPlan):
        raise TypeError(f"{name}: plan must be a PyramidPlan (pyramid_plan)")
    _check_frames(torch, frames, name)
    f, h, w = frames.shape
    if (w, h) != (plan.levels[0].width, plan.levels[0].height):
        raise ValueError(f"{name}: the frames do not have the plan's level-0 size")
    if len(plan) > 1:
        if f > plan.n_frames:
            raise ValueError(f"{name}: more frames than the plan was made for")
        if buffer is None or buffer.dtype != torch.uint8 or not buffer.is_contiguous() or \
                buffer.numel() < plan.total_bytes:
            raise ValueError(f"{name}: buffer must be a contiguous uint8 tensor of "
                             "plan.total_bytes bytes")
    else:
        buffer = None
    return frames, buffer, plan


def track_device(prev, next, points, offsets, next_q11, status, prev_first=0, next_first=0,
                 n_frames=None, coords="u32", keep=None, guess=None, radius=10, max_iters=30,
                 eps=20, min_eig=1.0, next_xy=None, err=None, info=None, matches=None,
                 stream=None, device=None):
    """Pyramidal Lucas-Kanade tracking on the device (fdf_track_device): frame f of the call
    follows its points from frame ``prev_first + f`` of ``prev`` into frame ``next_first + f`` of
    ``next``.  ``prev`` and ``next`` are :class:`Pyramid` objects (built) or triples (frames,
    buffer, plan) with equal plans and equal frame strides; they may be the same object: a batch
    of F frames tracked frame to frame is ``track_device(p, p, ..., prev_first=0, next_first=1)``.
    ``n_frames`` defaults to the frames both sides have from their first index on.

    ``points`` (cap, 2) 32-bit integers: pixels (``coords="u32"``, as detect_device and
    select_device fill them) or 1/2048 pixel (``coords="q11"``, as this call writes ``next_q11``);
    ``offsets`` int64 with n_frames + 1 entries; ``keep`` (optional, (cap,) uint8) 0 skips a point;
    ``guess`` (optional, (cap, 2) int32, 1/2048 pixel) is the starting position in the next frame.
    ``radius`` 1..15 is the window's half side, ``max_iters`` 1..64 per level, ``eps`` the step in
    1/2048 pixel at which a level stops, ``min_eig`` the smallest eigenvalue of the window's mean
    gradient matrix a level must have.

    Outputs, all (cap, ...) and contiguous: ``next_q11`` (cap, 2) int32 and ``status`` (cap,) uint8
    always; ``next_xy`` (cap, 2) float32, ``err`` and ``info`` (cap,) 32-bit integers and
    ``matches`` (cap, 2) 32-bit integers (match_device's records, for ransac_device) if given.
    Asynchronous on ``stream`` (default: torch's current stream)."""
    import torch

    pf, pb, plan = _track_set(torch, prev, "prev")
    nf, nb, nplan = _track_set(torch, next, "next")
    if plan.levels != nplan.levels:
        raise ValueError("prev and next must have the same levels (sizes, strides and offsets)")
    prev_first, next_first = int(prev_first), int(next_first)
    if prev_first < 0 or next_first < 0:
        raise ValueError("first-frame indices must not be negative")
    room = min(pf.shape[0] - prev_first, nf.shape[0] - next_first)
    n = room if n_frames is None else int(n_frames)
    if n < 0 or n > room:
        raise ValueError("prev and next do not hold frames up to first + n_frames")
    if n > 65535 or prev_first > 65535 or next_first > 65535:
        raise ValueError("at most 65535 frames")
    stride = max(pf.stride(0), nf.stride(0)) if max(pf.shape[0], nf.shape[0]) > 1 else \
        pf.shape[1] * pf.shape[2]
    for t in (pf, nf):
        if t.shape[0] > 1 and t.stride(0) != stride:
            raise ValueError("prev and next must have the same frame stride")
    code = _track_coords(coords)
    radius, max_iters, eps, min_eig = _track_values(radius, max_iters, eps, min_eig)
    _check_points(points)
    cap = points.shape[0]
    _check_offsets(torch, offsets, n + 1)
    tensors = [pf, nf, points, offsets, next_q11, status]
    tensors += [t for t in (pb, nb, keep, guess, next_xy, err, info, matches) if t is not None]
    for t, name in ((next_q11, "next_q11"), (guess, "guess"), (matches, "matches")):
        if t is not None:
            _check_points(t, name)
    for t, name in ((next_q11, "next_q11"), (guess, "guess"), (matches, "matches"), (points, "points")):
        if t is not None and (t.shape[0] < cap or t.data_ptr() % 8):
            raise ValueError(f"{name} must hold cap rows and be 8-byte aligned")
    if next_xy is not None and (next_xy.dtype != torch.float32 or next_xy.dim() != 2 or
                                next_xy.shape[1] != 2 or next_xy.shape[0] < cap or
                                not next_xy.is_contiguous() or next_xy.data_ptr() % 8):
        raise ValueError("next_xy must be a contiguous, 8-byte aligned (cap, 2) float32 tensor")
    for t, name in ((status, "status"), (keep, "keep")):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < cap or
                              not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor with cap entries")
    for t, name in ((err, "err"), (info, "info")):
        if t is not None and (t.dim() != 1 or t.element_size() != 4 or t.is_floating_point() or
                              t.numel() < cap or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous 32-bit integer tensor with cap entries")
    if matches is not None and cap > _MATCH_MAX_CAP:
        raise ValueError("matches: cap is at most 2^32 - 2")
    _check_one_device("track_device", tensors)
    dev, stream = _device_stream(torch, pf, device, stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = _native.load().fdf_track_device(
        context(dev).handle, ptr(pf), ptr(pb), prev_first, ptr(nf), ptr(nb), next_first, n, stride,
        plan._c, len(plan), ptr(points), code, cap, ptr(offsets), ptr(keep), ptr(guess), radius,
        max_iters, eps, min_eig, ptr(next_q11), ptr(next_xy), ptr(status), ptr(err), ptr(info),
        ptr(matches), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_track_device")


def track_array(img0, img1, points, n_levels=3, scale=(2, 1), radius=10, max_iters=30, eps=20,
                min_eig=1.0, guess=None, coords="u32", device=0):
    """The ``points`` of host image ``img0`` followed into ``img1`` (same size) by pyramidal
    Lucas-Kanade over ``n_levels`` levels at the factor ``scale`` (fdf_track_frames).  ``points``
    is (K, 2) integers: pixels, or 1/2048 pixel with ``coords="q11"``; ``guess`` (optional, (K, 2),
    1/2048 pixel) the starting positions in ``img1``.  Returns a :class:`TrackResult`: ``q11``
    (K, 2) int32 positions in 1/2048 pixel ((-1, -1) for a lost point), ``xy`` (K, 2) float32
    pixels, ``status`` (K,) bool, ``err`` (K,) uint32 (the window's sum of absolute differences in
    1/32 grey level), ``reason`` (K,) uint8 (an index into TRACK_REASONS) and ``iterations``."""
    a, b = _as_pixels(img0), _as_pixels(img1)
    if a.shape != b.shape:
        raise ValueError("img0 and img1 must have the same shape")
    if a.strides[0] != b.strides[0]:
        b = np.ascontiguousarray(b)
        a = np.ascontiguousarray(a)
    code = _track_coords(coords)
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "ui":
        raise TypeError("points must be a (K, 2) integer array")
    pts = _host_points(pts) if code == _native.FDF_COORDS_U32 else \
        np.ascontiguousarray(pts, dtype=np.int32)
    k = len(pts)
    g = None
    if guess is not None:
        g = np.ascontiguousarray(np.asarray(guess), dtype=np.int32)
        if g.shape != (k, 2):
            raise ValueError("guess must be (K, 2)")
    num, den = _scale(scale)
    radius, max_iters, eps, min_eig = _track_values(radius, max_iters, eps, min_eig)
    h, w = a.shape
    q11 = np.full((k, 2), -1, dtype=np.int32)
    xy = np.full((k, 2), -1.0, dtype=np.float32)
    status = np.zeros(k, dtype=np.uint8)
    err = np.full(k, 0xffffffff, dtype=np.uint32)
    info = np.zeros(k, dtype=np.uint32)
    ptr = lambda t: t.ctypes.data if t is not None and t.size else None
    rc = _native.load().fdf_track_frames(
        context(device).handle, a.ctypes.data, b.ctypes.data, w, h, a.strides[0], ptr(pts), code, k,
        ptr(g), int(n_levels), num, den, radius, max_iters, eps, min_eig, ptr(q11), ptr(xy),
        ptr(status), ptr(err), ptr(info))
    check(rc, "fdf_track_frames")
    return TrackResult(q11, xy, status.astype(bool), err, (info & 0xff).astype(np.uint8),
                       info >> 8)


# Track-set maintenance between two tracking calls (fdf_tracks.hip; include/fdf.h has the rule).

TRACKS_NEW = _native.FDF_TRACKS_NEW
TrackSetResult = collections.namedtuple("TrackSetResult", "q11 ids ages src next_id")


def _tracks_params(shape, min_dist, margin, max_tracks, passes):
    h, w = (int(v) for v in shape)
    min_dist, margin, max_tracks, passes = int(min_dist), int(margin), int(max_tracks), int(passes)
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError("shape must be (height, width) with sides in 1..65535")
    if not 1 <= min_dist <= 255:
        raise ValueError("min_dist must be in 1..255")
    if margin < 0 or 2 * margin >= min(w, h):
        raise ValueError("margin must satisfy 0 <= 2 * margin < min(width, height)")
    if not 1 <= max_tracks <= 0xffffffff:
        raise ValueError("max_tracks must be at least 1")
    if not 1 <= passes <= 32:
        raise ValueError("passes must be in 1..32")
    return _native.FdfTracksParams(w, h, min_dist, margin, max_tracks, passes)


def tracks_scratch_bytes(n_frames, shape, min_dist, t_cap, c_cap):
    """Scratch bytes tracks_update_device needs (fdf_tracks_scratch_bytes; host only, no
    device): ``shape`` is (height, width), ``t_cap`` and ``c_cap`` the capacities of the track
    and the candidate arrays."""
    h, w = (int(v) for v in shape)
    v = ctypes.c_uint64()
    check(_native.load().fdf_tracks_scratch_bytes(int(n_frames), w, h, int(min_dist), int(t_cap),
                                                  int(c_cap), ctypes.byref(v)),
          "fdf_tracks_scratch_bytes")
    return v.value


def _check_words(t, name, rows):
    if t.dim() != 1 or t.element_size() != 4 or t.is_floating_point() or not t.is_contiguous() or \
            t.numel() < rows:
        raise ValueError(f"{name} must be a contiguous 32-bit integer tensor with {rows} entries")


def tracks_update_device(track_q11, track_ids, track_ages, track_offsets, cand_points, cand_scores,
                         cand_offsets, next_id, out_q11, out_ids, out_ages, out_offsets, shape,
                         min_dist=16, margin=11, max_tracks=1024, passes=8, track_status=None,
                         out_src=None, scratch=None, stream=None):
    """The step between two track_device calls, on the device (fdf_tracks_update_device), for the
    F streams ``track_offsets`` and ``cand_offsets`` (int64, F+1 entries each) describe: lost
    tracks (``track_status`` 0, optional) and tracks within ``margin`` pixels of the border are
    dropped, of two tracks within ``min_dist`` pixels the older stays, and the strongest
    candidates that no survivor and no stronger admitted candidate is within ``min_dist`` of refill
    each stream up to ``max_tracks``; ``passes`` bounds the suppression passes (8 converges on
    real frames).  ``track_q11`` (t_cap, 2) int32 as track_device wrote next_q11, ``track_ids``
    and ``track_ages`` (t_cap,) 32-bit, ``cand_points`` (c_cap, 2) and ``cand_scores`` (c_cap,)
    16-bit as detect_device and score_device filled them, ``next_id`` (F,) 32-bit (read and
    advanced), ``shape`` = (height, width).

    Outputs: ``out_q11`` (out_cap, 2) int32, ``out_ids``, ``out_ages`` and the optional ``out_src``
    (out_cap,) 32-bit (a survivor's track index, TRACKS_NEW | candidate index for a new track),
    ``out_offsets`` (F+1,) int64 with the full totals.  ``out_q11`` and ``out_offsets`` are
    ``coords="q11"`` points of the next track_device call.  ``scratch``: a uint8 CUDA tensor of
    tracks_scratch_bytes(...) bytes (None: allocated through torch).  Asynchronous on ``stream``
    (default: torch's current stream)."""
    import torch

    params = _tracks_params(shape, min_dist, margin, max_tracks, passes)
    _check_offsets(torch, track_offsets, 1, "track_offsets")
    f = track_offsets.numel() - 1
    _check_offsets(torch, cand_offsets, f + 1, "cand_offsets")
    _check_offsets(torch, out_offsets, f + 1, "out_offsets")
    _check_points(track_q11, "track_q11", "t_cap")
    _check_points(cand_points, "cand_points", "c_cap")
    _check_points(out_q11, "out_q11", "out_cap")
    t_cap, c_cap, out_cap = track_q11.shape[0], cand_points.shape[0], out_q11.shape[0]
    for t, name, rows in ((track_ids, "track_ids", t_cap), (track_ages, "track_ages", t_cap),
                          (next_id, "next_id", f), (out_ids, "out_ids", out_cap),
                          (out_ages, "out_ages", out_cap), (out_src, "out_src", out_cap)):
        if t is not None:
            _check_words(t, name, rows)
    if cand_scores.dim() != 1 or cand_scores.element_size() != 2 or \
            cand_scores.is_floating_point() or not cand_scores.is_contiguous() or \
            cand_scores.numel() < c_cap:
        raise ValueError("cand_scores must be a contiguous 16-bit integer tensor with c_cap entries")
    if track_status is not None and (track_status.dtype != torch.uint8 or track_status.dim() != 1 or
                                     track_status.numel() < t_cap or
                                     not track_status.is_contiguous()):
        raise ValueError("track_status must be a contiguous uint8 tensor with t_cap entries")
    if scratch is not None and (scratch.dtype != torch.uint8 or not scratch.is_contiguous()):
        raise ValueError("scratch must be a contiguous uint8 tensor")
    tensors = [track_q11, track_ids, track_ages, track_offsets, cand_points, cand_scores,
               cand_offsets, next_id, out_q11, out_ids, out_ages, out_offsets]
    tensors += [t for t in (track_status, out_src, scratch) if t is not None]
    _check_one_device("tracks_update_device", tensors)
    need = tracks_scratch_bytes(f, shape, min_dist, t_cap, c_cap)
    current = torch.cuda.current_stream(track_offsets.device)
    if stream is None:
        stream = current
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=track_offsets.device)
        if stream != current:
            scratch.record_stream(stream)    # in use on `stream` until the call's kernels are done
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    rc = _native.load().fdf_tracks_update_device(
        context(track_offsets.device.index).handle, f, ctypes.byref(params), ptr(track_q11),
        ptr(track_status), ptr(track_ids), ptr(track_ages), ptr(track_offsets), t_cap,
        ptr(cand_points), ptr(cand_scores), ptr(cand_offsets), c_cap, ptr(next_id), ptr(out_q11),
        ptr(out_ids), ptr(out_ages), ptr(out_src), out_cap, ptr(out_offsets), scratch.data_ptr(),
        scratch.numel(), ctypes.c_void_p(stream.cuda_stream))
    check(rc, "fdf_tracks_update_device")


def update_tracks(shape, track_q11, track_ids, track_ages, cand_points, cand_scores, next_id=0,
                  min_dist=16, margin=11, max_tracks=1024, passes=8, status=None, device=0):
    """One stream's track set updated from host arrays (fdf_tracks_update_points): ``track_q11``
    (T, 2) positions in 1/2048 pixel, ``track_ids`` and ``track_ages`` (T,), ``status`` (T,)
    optional, ``cand_points`` (C, 2) pixels and ``cand_scores`` (C,).  Returns a
    :class:`TrackSetResult`: ``q11`` (K, 2) int32, ``ids``, ``ages`` and ``src`` (K,) uint32 (a
    survivor's index, TRACKS_NEW | candidate index for a new track) and the advanced ``next_id``."""
    params = _tracks_params(shape, min_dist, margin, max_tracks, passes)
    q = np.ascontiguousarray(np.asarray(track_q11).reshape(-1, 2), dtype=np.int32)
    ids = np.ascontiguousarray(track_ids, dtype=np.uint32).reshape(-1)
    ages = np.ascontiguousarray(track_ages, dtype=np.uint32).reshape(-1)
    cand = _host_points(np.asarray(cand_points).reshape(-1, 2))
    scores = np.ascontiguousarray(cand_scores, dtype=np.uint16).reshape(-1)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    nt, nc = len(q), len(cand)
    if len(ids) != nt or len(ages) != nt or len(scores) != nc or (st is not None and len(st) != nt):
        raise ValueError("the arrays of a list must have one entry per point")
    cap = nt + min(nc, params.max_tracks)
    out_q = np.empty((cap, 2), dtype=np.int32)
    out_ids, out_ages, out_src = (np.empty(cap, dtype=np.uint32) for _ in range(3))
    nid = ctypes.c_uint32(int(next_id) & 0xffffffff)
    n = ctypes.c_size_t(0)
    ptr = lambda t: t.ctypes.data if t is not None and t.size else None
    rc = _native.load().fdf_tracks_update_points(
        context(device).handle, ctypes.byref(params), ptr(q), ptr(st), ptr(ids), ptr(ages), nt,
        ptr(cand), ptr(scores), nc, ctypes.byref(nid), ptr(out_q), ptr(out_ids), ptr(out_ages),
        ptr(out_src), cap, ctypes.byref(n))
    check(rc, "fdf_tracks_update_points")
    k = n.value
    return TrackSetResult(out_q[:k], out_ids[:k], out_ages[:k], out_src[:k], nid.value)


def track_sequence_array(frames, config, min_dist=16, margin=None, max_tracks=1024, passes=8,
                         n_levels=3, scale=(2, 1), radius=10, max_iters=30, eps=20, min_eig=1.0,
                         device=0):
    """A whole detect + track loop over the host video ``frames`` ((F, H, W) uint8) on the device.
    Frame 0: detect_device + score_device, then tracks_update_device on an empty set.  Every later
    frame k: track_device from frame k - 1 (over a pyramid of ``n_levels`` levels at ``scale``),
    then tracks_update_device with frame k's detections as candidates.  ``margin`` defaults to
    ``radius + 1``.  Ids start at 0.  Only the detection counts are read back before the loop;
    the loop itself never leaves the device.  Returns one (ids (K,) uint32, q11 (K, 2) int32, ages
    (K,) uint32) triple per frame: the track set after that frame's update."""
    import torch

    arr = np.ascontiguousarray(frames)
    if arr.ndim != 3 or arr.dtype != np.uint8:
        raise ValueError("frames must be a (F, H, W) uint8 array")
    f, h, w = arr.shape
    margin = int(radius) + 1 if margin is None else margin
    params = _tracks_params((h, w), min_dist, margin, max_tracks, passes)
    radius, max_iters, eps, min_eig = _track_values(radius, max_iters, eps, min_eig)
    if f == 0:
        return []
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_frames = torch.from_numpy(arr).to(dev)
        pyr = Pyramid(d_frames, n_levels, scale)
        cap = capacity_guess(h * w) * f
        while True:
            pts = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            offs = torch.zeros(f + 1, dtype=torch.int64, device=dev)
            detect_device(d_frames, config, pts, offs)
            total = int(offs[f])
            if total <= cap:
                break
            cap = total
        scores = torch.empty(max(cap, 1), dtype=torch.int16, device=dev)
        score_device(d_frames, config, pts, offs, scores)
        bounds = offs.cpu().tolist()
        # frame k's candidates as one stream of their own: offsets {0, n_k}
        c_offs = torch.tensor([[0, bounds[k + 1] - bounds[k]] for k in range(f)],
                              dtype=torch.int64, device=dev)
        m = params.max_tracks = min(params.max_tracks, 1 << 24)
        q11 = torch.empty((f, m, 2), dtype=torch.int32, device=dev)
        ids = torch.empty((f, m), dtype=torch.int32, device=dev)
        ages = torch.empty((f, m), dtype=torch.int32, device=dev)
        t_offs = torch.zeros((f + 1, 2), dtype=torch.int64, device=dev)   # row 0: the empty set
        moved_q11 = torch.empty((m, 2), dtype=torch.int32, device=dev)
        status = torch.empty(m, dtype=torch.uint8, device=dev)
        next_id = torch.zeros(1, dtype=torch.int32, device=dev)
        n_c = max(bounds[k + 1] - bounds[k] for k in range(f))
        scratch = torch.empty(max(tracks_scratch_bytes(1, (h, w), min_dist, m, n_c), 1),
                              dtype=torch.uint8, device=dev)
        for k in range(f):
            cand = pts[bounds[k]:bounds[k + 1]]
            cand_scores = scores[bounds[k]:bounds[k + 1]]
            if k == 0:
                prev = (q11[0, :0], ids[0, :0], ages[0, :0])
                st = None
            else:
                track_device(pyr, pyr, q11[k - 1], t_offs[k], moved_q11, status, prev_first=k - 1,
                             next_first=k, n_frames=1, coords="q11", radius=radius,
                             max_iters=max_iters, eps=eps, min_eig=min_eig)
                prev = (moved_q11, ids[k - 1], ages[k - 1])
                st = status
            tracks_update_device(prev[0], prev[1], prev[2], t_offs[k], cand, cand_scores, c_offs[k],
                                 next_id, q11[k], ids[k], ages[k], t_offs[k + 1], (h, w),
                                 min_dist=min_dist, margin=margin, max_tracks=m, passes=passes,
                                 track_status=None if st is None else st[:prev[0].shape[0]],
                                 scratch=scratch)
        counts = t_offs[:, 1].cpu().tolist()
        h_q11, h_ids, h_ages = q11.cpu().numpy(), ids.cpu().numpy(), ages.cpu().numpy()
    return [(h_ids[k, :counts[k + 1]].view(np.uint32).copy(), h_q11[k, :counts[k + 1]].copy(),
             h_ages[k, :counts[k + 1]].view(np.uint32).copy()) for k in range(f)]


__all__ = ["NORTH", "EAST", "SOUTH", "WEST", "circle", "calculate_offsets", "context",
           "shard_contexts", "capacity_guess", "Lanes",
           "detect_array", "detector", "detector_batch", "detect_device", "keypoint_scores",
           "detect_scored_array", "detector_scored", "detector_batch_scored", "score_device",
           "select_scratch_bytes", "select_device", "select_best", "detect_best_array",
           "orient_disc", "orient_device", "keypoint_angles", "detect_oriented_array",
           "harris_codes", "harris_device", "keypoint_harris", "detect_harris_array",
           "brief_pattern", "brief_steer", "smooth_device", "describe_device",
           "keypoint_descriptors", "detect_described_array",
           "resize_taps", "resize_device", "resize_array", "PyramidLevel", "PyramidPlan",
           "pyramid_plan", "pyramid_device", "Pyramid", "MultiscaleKeypoints",
           "detect_multiscale_array",
           "MATCH_DTYPE", "MATCH_NONE", "MATCH_NO_DISTANCE", "match_device",
           "match_filter_device", "unpack_matches", "match_descriptors",
           "MODEL_DTYPE", "RANSAC_NONE", "ransac_sample", "ransac_scratch_bytes", "ransac_device",
           "unpack_models", "estimate_model",
           "refine_scratch_bytes", "refine_device", "refine_model",
           "fundamental_sample", "fundamental_scratch_bytes", "fundamental_device",
           "fundamental_check_device", "estimate_fundamental",
           "warp_device", "warp_array", "model_invert",
           "TRACK_REASONS", "TrackResult", "track_device", "track_array", "track_map_position",
           "track_map_displacement",
           "TRACKS_NEW", "TrackSetResult", "tracks_scratch_bytes", "tracks_update_device",
           "update_tracks", "track_sequence_array",
           "detect_rgb_array", "detector_rgb", "rgb_to_luma", "detect_device_rgb",
           "score_rings", "score_rings_device", "keypoint_score_max_threshold",
           "keypoint_score_sum_abs_difference", "NonMaximalSuppression"]
