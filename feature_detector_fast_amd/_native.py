"""ctypes binding of the C ABI in include/fdf.h (libfdf.so, built in-tree by ``make``).

There is no fallback: if the shared library is missing or no HIP device is visible the
calls raise :class:`FdfError` -- the HIP kernels are the only implementation.
"""
import ctypes
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDF_LIB_PATH: another build of the same library (A/B timing of two kernel versions,
# tools/build_rev.sh); the default is the in-tree build.
LIB_PATH = os.environ.get("FDF_LIB_PATH") or os.path.join(_HERE, "libfdf.so")

# include/fdf.h enum fdf_status
FDF_OK = 0
FDF_ERR_COUNT = 1
FDF_ERR_SIZE = 2
FDF_ERR_CAPACITY = 3
FDF_ERR_NMS = 4
FDF_ERR_DEVICE = 5
FDF_ERR_ARG = 6
FDF_ERR_ALLOC = 7
FDF_ERR_BUSY = 8
FDF_ERR_DROPPED = 9
# enum fdf_pipe_flags
FDF_PIPE_RGB = 1
FDF_PIPE_SCORES = 2

# Every symbol include/fdf.h declares (tests/test_abi.py checks the .so exports them all).
EXPORTED_SYMBOLS = (
    "fdf_abi_version", "fdf_status_string", "fdf_device_count", "fdf_validate",
    "fdf_ctx_create", "fdf_ctx_destroy", "fdf_ctx_stream", "fdf_ctx_set_timing",
    "fdf_ctx_timing", "fdf_detect", "fdf_detect_rgb", "fdf_rgb_to_luma_device",
    "fdf_detect_batch", "fdf_detect_device", "fdf_score_points", "fdf_detect_scored",
    "fdf_detect_batch_scored", "fdf_score_device", "fdf_pipeline_create",
    "fdf_pipeline_destroy", "fdf_pipeline_acquire", "fdf_pipeline_submit", "fdf_pipeline_push",
    "fdf_pipeline_collect", "fdf_ctx_set_geometry", "fdf_ctx_timing_samples", "fdf_fetch_last",
    "fdf_detect_batch_multi", "fdf_fetch_last_multi", "fdf_ctx_workspace_bytes",
    "fdf_detect_device_rgb", "fdf_circle", "fdf_calculate_offsets", "fdf_score_rings",
    "fdf_score_rings_device", "fdf_ctx_set_band_rows", "fdf_ctx_set_upload_chunks",
    "fdf_ctx_recoveries", "fdf_ctx_test_skew_tickets", "fdf_select_scratch_bytes",
    "fdf_select_device", "fdf_select_points", "fdf_orient_disc", "fdf_orient_device",
    "fdf_orient_points", "fdf_brief_pattern", "fdf_brief_steer", "fdf_smooth_device",
    "fdf_describe_device", "fdf_describe_points", "fdf_match_device",
    "fdf_match_filter_device", "fdf_match_points", "fdf_resize_taps", "fdf_resize_device",
    "fdf_resize_frame", "fdf_pyramid_plan", "fdf_pyramid_taps", "fdf_pyramid_device",
    "fdf_harris_codes", "fdf_harris_device", "fdf_harris_points", "fdf_ransac_sample",
    "fdf_ransac_scratch_bytes", "fdf_ransac_device", "fdf_ransac_points",
    "fdf_refine_scratch_bytes", "fdf_refine_device", "fdf_refine_points", "fdf_warp_device",
    "fdf_warp_frame", "fdf_model_invert", "fdf_track_device", "fdf_track_frames",
    "fdf_track_map_position", "fdf_track_map_displacement", "fdf_tracks_scratch_bytes",
    "fdf_tracks_update_device", "fdf_tracks_update_points", "fdf_fundamental_sample",
    "fdf_fundamental_scratch_bytes", "fdf_fundamental_device", "fdf_fundamental_check_device",
    "fdf_fundamental_points",
)


class FdfConfig(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_uint8), ("count", ctypes.c_uint8), ("nms", ctypes.c_uint8)]


class FdfPoint(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32)]


class FdfMatch(ctypes.Structure):
    """include/fdf.h fdf_match: 8 bytes."""
    _fields_ = [("index", ctypes.c_uint32), ("distance", ctypes.c_uint16),
                ("second", ctypes.c_uint16)]


class FdfPyramidLevel(ctypes.Structure):
    """include/fdf.h fdf_pyramid_level: 40 bytes."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("frame_stride_bytes", ctypes.c_uint64), ("offset_bytes", ctypes.c_uint64),
                ("xtaps_offset", ctypes.c_uint64), ("ytaps_offset", ctypes.c_uint64)]


class FdfModel(ctypes.Structure):
    """include/fdf.h fdf_model: 88 bytes."""
    _fields_ = [("h", ctypes.c_double * 9), ("n_corr", ctypes.c_uint32),
                ("n_inliers", ctypes.c_uint32), ("hypothesis", ctypes.c_uint32),
                ("n_valid", ctypes.c_uint32)]


class FdfTracksParams(ctypes.Structure):
    """include/fdf.h fdf_tracks_params: 24 bytes."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("min_dist", ctypes.c_uint32), ("margin", ctypes.c_uint32),
                ("max_tracks", ctypes.c_uint32), ("passes", ctypes.c_uint32)]


FDF_MATCH_NONE = 0xFFFFFFFF
FDF_MATCH_NO_DISTANCE = 0xFFFF
FDF_COORDS_U32 = 0
FDF_COORDS_F32 = 1
FDF_COORDS_Q11 = 2
FDF_TRACKS_NEW = 0x80000000
FDF_MODEL_AFFINE = 0
FDF_MODEL_HOMOGRAPHY = 1
FDF_RANSAC_NONE = 0xFFFFFFFF
FDF_BORDER_REPLICATE = 0
FDF_BORDER_CONSTANT = 1


class FdfError(RuntimeError):
    """A non-OK fdf_status; ``.status`` holds the code."""

    def __init__(self, status, where=""):
        self.status = status
        msg = status_string(status) if _lib is not None else f"status {status}"
        super().__init__(f"{where}: {msg}" if where else msg)


_lib = None


def _share_torch_runtime():
    """Map PyTorch's bundled HIP runtime before libfdf.so when torch is installed.

    torch ships its own libamdhip64.so (SONAME libamdhip64.so.7).  If libfdf.so were loaded
    first it would map /opt/rocm's copy, and a later ``import torch`` would map a second HIP
    runtime into the process, which then fails to initialise.  With torch's copy mapped
    first, libfdf.so's NEEDED libamdhip64.so.7 binds to it, so device pointers and streams
    are shared with torch.  Without torch, /opt/rocm's runtime is used."""
    if "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or spec.origin is None:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load libfdf.so once and declare the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FdfError(FDF_ERR_DEVICE, f"{LIB_PATH} is not built (run `make` or __graft_entry__.build())")
    _share_torch_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    vp = ctypes.c_void_p
    sz = ctypes.c_size_t
    u32 = ctypes.c_uint32
    u64 = ctypes.c_uint64
    cfgp = ctypes.POINTER(FdfConfig)
    lib.fdf_abi_version.restype = ctypes.c_int
    lib.fdf_status_string.restype = ctypes.c_char_p
    lib.fdf_status_string.argtypes = [ctypes.c_int]
    lib.fdf_device_count.restype = ctypes.c_int
    lib.fdf_validate.restype = ctypes.c_int
    lib.fdf_validate.argtypes = [u32, u32, cfgp, ctypes.POINTER(ctypes.c_int)]
    lib.fdf_ctx_create.restype = ctypes.c_int
    lib.fdf_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    lib.fdf_ctx_destroy.restype = None
    lib.fdf_ctx_destroy.argtypes = [vp]
    lib.fdf_ctx_stream.restype = vp
    lib.fdf_ctx_stream.argtypes = [vp]
    lib.fdf_ctx_set_timing.restype = ctypes.c_int
    lib.fdf_ctx_set_timing.argtypes = [vp, ctypes.c_int]
    lib.fdf_ctx_timing.restype = ctypes.c_int
    lib.fdf_ctx_timing.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_float),
                                   ctypes.POINTER(ctypes.c_float)]
    lib.fdf_detect.restype = ctypes.c_int
    lib.fdf_detect.argtypes = [vp, vp, u32, u32, sz, cfgp, vp, sz, ctypes.POINTER(sz)]
    lib.fdf_detect_rgb.restype = ctypes.c_int
    lib.fdf_detect_rgb.argtypes = [vp, vp, u32, u32, sz, cfgp, vp, sz, ctypes.POINTER(sz)]
    lib.fdf_rgb_to_luma_device.restype = ctypes.c_int
    lib.fdf_rgb_to_luma_device.argtypes = [vp, vp, u32, u32, u32, ctypes.c_uint64, vp, vp]
    lib.fdf_detect_batch.restype = ctypes.c_int
    lib.fdf_detect_batch.argtypes = [vp, vp, u32, u32, u32, sz, cfgp, vp, sz, vp,
                                     ctypes.POINTER(sz)]
    lib.fdf_detect_device.restype = ctypes.c_int
    lib.fdf_detect_device.argtypes = [vp, vp, u32, u32, u32, u64, cfgp, vp, u64, vp, vp]
    lib.fdf_detect_device_rgb.restype = ctypes.c_int
    lib.fdf_detect_device_rgb.argtypes = [vp, vp, u32, u32, u32, u64, cfgp, vp, u64, vp, vp]
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.fdf_circle.restype = None
    lib.fdf_circle.argtypes = [i32p, i32p]
    lib.fdf_calculate_offsets.restype = None
    lib.fdf_calculate_offsets.argtypes = [u32, i32p]
    lib.fdf_score_rings.restype = ctypes.c_int
    lib.fdf_score_rings.argtypes = [vp, vp, vp, sz, cfgp, vp]
    lib.fdf_score_rings_device.restype = ctypes.c_int
    lib.fdf_score_rings_device.argtypes = [vp, vp, vp, u64, cfgp, vp, vp]
    lib.fdf_score_points.restype = ctypes.c_int
    lib.fdf_score_points.argtypes = [vp, vp, u32, u32, sz, cfgp, vp, sz, vp]
    lib.fdf_detect_scored.restype = ctypes.c_int
    lib.fdf_detect_scored.argtypes = [vp, vp, u32, u32, sz, cfgp, vp, vp, sz, ctypes.POINTER(sz)]
    lib.fdf_detect_batch_scored.restype = ctypes.c_int
    lib.fdf_detect_batch_scored.argtypes = [vp, vp, u32, u32, u32, sz, cfgp, vp, vp, sz, vp,
                                            ctypes.POINTER(sz)]
    lib.fdf_score_device.restype = ctypes.c_int
    lib.fdf_score_device.argtypes = [vp, vp, u32, u32, u32, u64, cfgp, vp, u64, vp, vp, vp]
    lib.fdf_pipeline_create.restype = ctypes.c_int
    lib.fdf_pipeline_create.argtypes = [ctypes.c_int, u32, u32, u32, u32, u64, u32, cfgp,
                                        ctypes.POINTER(vp)]
    lib.fdf_pipeline_destroy.restype = None
    lib.fdf_pipeline_destroy.argtypes = [vp]
    lib.fdf_pipeline_acquire.restype = ctypes.c_int
    lib.fdf_pipeline_acquire.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64)]
    lib.fdf_pipeline_submit.restype = ctypes.c_int
    lib.fdf_pipeline_submit.argtypes = [vp, u64, u32]
    lib.fdf_pipeline_push.restype = ctypes.c_int
    lib.fdf_pipeline_push.argtypes = [vp, vp, u32, sz, ctypes.POINTER(u64)]
    lib.fdf_pipeline_collect.restype = ctypes.c_int
    lib.fdf_pipeline_collect.argtypes = [vp, u64, vp, vp, sz, vp, ctypes.POINTER(sz)]
    lib.fdf_ctx_workspace_bytes.restype = ctypes.c_int
    lib.fdf_ctx_workspace_bytes.argtypes = [vp, ctypes.POINTER(u64)]
    lib.fdf_ctx_test_skew_tickets.restype = ctypes.c_int
    lib.fdf_ctx_test_skew_tickets.argtypes = [vp, u32]
    lib.fdf_ctx_set_geometry.restype = ctypes.c_int
    lib.fdf_ctx_set_geometry.argtypes = [vp, u32]
    lib.fdf_ctx_set_band_rows.restype = ctypes.c_int
    lib.fdf_ctx_set_band_rows.argtypes = [vp, u32]
    lib.fdf_ctx_set_upload_chunks.restype = ctypes.c_int
    lib.fdf_ctx_set_upload_chunks.argtypes = [vp, u32]
    lib.fdf_ctx_recoveries.restype = ctypes.c_int
    lib.fdf_ctx_recoveries.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.fdf_ctx_timing_samples.restype = ctypes.c_int
    lib.fdf_ctx_timing_samples.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u32)]
    lib.fdf_fetch_last.restype = ctypes.c_int
    lib.fdf_fetch_last.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    lib.fdf_detect_batch_multi.restype = ctypes.c_int
    lib.fdf_detect_batch_multi.argtypes = [vp, u32, vp, u32, u32, u32, sz, cfgp, vp, sz, vp,
                                           ctypes.POINTER(sz)]
    lib.fdf_fetch_last_multi.restype = ctypes.c_int
    lib.fdf_fetch_last_multi.argtypes = [vp, u32, vp, sz, ctypes.POINTER(sz)]
    lib.fdf_select_scratch_bytes.restype = ctypes.c_int
    lib.fdf_select_scratch_bytes.argtypes = [u32, u32, u32, u32, u32, u64, ctypes.POINTER(u64)]
    lib.fdf_select_device.restype = ctypes.c_int
    lib.fdf_select_device.argtypes = [vp, u32, u32, u32, vp, vp, u64, vp, u32, u32, u32, vp, vp,
                                      u64, vp, vp, vp, u64, vp]
    lib.fdf_select_points.restype = ctypes.c_int
    lib.fdf_select_points.argtypes = [vp, vp, vp, vp, u32, sz, u32, u32, u32, u32, u32, vp, vp,
                                      sz, vp, ctypes.POINTER(sz)]
    lib.fdf_orient_disc.restype = ctypes.c_int
    lib.fdf_orient_disc.argtypes = [u32, vp]
    lib.fdf_orient_device.restype = ctypes.c_int
    lib.fdf_orient_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u64, vp, u32, vp, vp, vp]
    lib.fdf_orient_points.restype = ctypes.c_int
    lib.fdf_orient_points.argtypes = [vp, vp, u32, u32, sz, vp, sz, u32, vp, vp]
    lib.fdf_harris_codes.restype = ctypes.c_int
    lib.fdf_harris_codes.argtypes = [vp, sz, vp]
    lib.fdf_harris_device.restype = ctypes.c_int
    lib.fdf_harris_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u64, vp, u32, u32, u32, vp,
                                      vp, vp]
    lib.fdf_harris_points.restype = ctypes.c_int
    lib.fdf_harris_points.argtypes = [vp, vp, u32, u32, sz, vp, sz, u32, u32, u32, vp, vp]
    lib.fdf_brief_pattern.restype = ctypes.c_int
    lib.fdf_brief_pattern.argtypes = [vp]
    lib.fdf_brief_steer.restype = ctypes.c_int
    lib.fdf_brief_steer.argtypes = [vp, u32, vp]
    lib.fdf_smooth_device.restype = ctypes.c_int
    lib.fdf_smooth_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u64, vp]
    lib.fdf_describe_device.restype = ctypes.c_int
    lib.fdf_describe_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u64, vp, vp, vp, u32, vp,
                                        vp]
    lib.fdf_describe_points.restype = ctypes.c_int
    lib.fdf_describe_points.argtypes = [vp, vp, u32, u32, sz, vp, sz, vp, vp, u32, ctypes.c_int,
                                        vp]
    lib.fdf_match_device.restype = ctypes.c_int
    lib.fdf_match_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32, vp, vp]
    lib.fdf_match_filter_device.restype = ctypes.c_int
    lib.fdf_match_filter_device.argtypes = [vp, u32, vp, u64, vp, vp, u64, u32, u32, u32, vp, vp]
    lib.fdf_match_points.restype = ctypes.c_int
    lib.fdf_match_points.argtypes = [vp, vp, vp, sz, vp, vp, sz, u32, u32, vp]
    lib.fdf_resize_taps.restype = ctypes.c_int
    lib.fdf_resize_taps.argtypes = [u32, u32, vp]
    lib.fdf_resize_device.restype = ctypes.c_int
    lib.fdf_resize_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u32, u32, u64, vp, vp, vp]
    lib.fdf_resize_frame.restype = ctypes.c_int
    lib.fdf_resize_frame.argtypes = [vp, vp, u32, u32, sz, vp, u32, u32, sz]
    levelp = ctypes.POINTER(FdfPyramidLevel)
    lib.fdf_pyramid_plan.restype = ctypes.c_int
    lib.fdf_pyramid_plan.argtypes = [u32, u32, u32, u32, u32, u32, levelp, ctypes.POINTER(u64),
                                     ctypes.POINTER(u64)]
    lib.fdf_pyramid_taps.restype = ctypes.c_int
    lib.fdf_pyramid_taps.argtypes = [levelp, u32, u32, u32, vp]
    lib.fdf_pyramid_device.restype = ctypes.c_int
    lib.fdf_pyramid_device.argtypes = [vp, vp, u32, u64, levelp, u32, vp, vp, vp]
    lib.fdf_ransac_sample.restype = ctypes.c_int
    lib.fdf_ransac_sample.argtypes = [u32, u32, u32, u32, u32, vp, ctypes.POINTER(u32)]
    lib.fdf_ransac_scratch_bytes.restype = ctypes.c_int
    lib.fdf_ransac_scratch_bytes.argtypes = [u32, u64, u32, ctypes.POINTER(u64)]
    lib.fdf_ransac_device.restype = ctypes.c_int
    lib.fdf_ransac_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32, u32,
                                      ctypes.c_float, u32, vp, vp, vp, u64, vp]
    lib.fdf_ransac_points.restype = ctypes.c_int
    lib.fdf_ransac_points.argtypes = [vp, vp, vp, sz, sz, vp, vp, u32, u32, u32, ctypes.c_float,
                                      u32, vp, vp]
    lib.fdf_refine_scratch_bytes.restype = ctypes.c_int
    lib.fdf_refine_scratch_bytes.argtypes = [u32, u64, ctypes.POINTER(u64)]
    lib.fdf_refine_device.restype = ctypes.c_int
    lib.fdf_refine_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32, vp,
                                      ctypes.c_float, u32, vp, vp, vp, vp, u64, vp]
    lib.fdf_refine_points.restype = ctypes.c_int
    lib.fdf_refine_points.argtypes = [vp, vp, vp, sz, sz, vp, vp, u32, u32, vp, ctypes.c_float,
                                      u32, vp, vp, vp]
    lib.fdf_warp_device.restype = ctypes.c_int
    lib.fdf_warp_device.argtypes = [vp, vp, u32, u32, u32, u64, vp, u64, vp, u32, u32, u64, u32,
                                    u32, vp, vp]
    lib.fdf_warp_frame.restype = ctypes.c_int
    lib.fdf_warp_frame.argtypes = [vp, vp, u32, u32, sz, vp, vp, u32, u32, sz, u32, u32, vp]
    lib.fdf_model_invert.restype = ctypes.c_int
    lib.fdf_model_invert.argtypes = [vp, vp]
    i64 = ctypes.c_int64
    lib.fdf_track_map_position.restype = ctypes.c_int
    lib.fdf_track_map_position.argtypes = [i64, u32, u32, ctypes.POINTER(i64)]
    lib.fdf_track_map_displacement.restype = ctypes.c_int
    lib.fdf_track_map_displacement.argtypes = [i64, u32, u32, ctypes.POINTER(i64)]
    lib.fdf_track_device.restype = ctypes.c_int
    lib.fdf_track_device.argtypes = [vp, vp, vp, u32, vp, vp, u32, u32, u64, vp, u32, vp, u32, u64,
                                     vp, vp, vp, u32, u32, u32, ctypes.c_float, vp, vp, vp, vp, vp,
                                     vp, vp]
    lib.fdf_track_frames.restype = ctypes.c_int
    lib.fdf_track_frames.argtypes = [vp, vp, vp, u32, u32, sz, vp, u32, sz, vp, u32, u32, u32, u32,
                                     u32, u32, ctypes.c_float, vp, vp, vp, vp, vp]
    lib.fdf_tracks_scratch_bytes.restype = ctypes.c_int
    lib.fdf_tracks_scratch_bytes.argtypes = [u32, u32, u32, u32, u64, u64, ctypes.POINTER(u64)]
    lib.fdf_tracks_update_device.restype = ctypes.c_int
    lib.fdf_tracks_update_device.argtypes = [vp, u32, ctypes.POINTER(FdfTracksParams), vp, vp, vp, vp,
                                             vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp,
                                             vp, u64, vp]
    lib.fdf_tracks_update_points.restype = ctypes.c_int
    lib.fdf_tracks_update_points.argtypes = [vp, ctypes.POINTER(FdfTracksParams), vp, vp, vp, vp, sz,
                                             vp, vp, sz, ctypes.POINTER(u32), vp, vp, vp, vp, sz,
                                             ctypes.POINTER(sz)]
    lib.fdf_fundamental_sample.restype = ctypes.c_int
    lib.fdf_fundamental_sample.argtypes = [u32, u32, u32, u32, vp, ctypes.POINTER(u32)]
    lib.fdf_fundamental_scratch_bytes.restype = ctypes.c_int
    lib.fdf_fundamental_scratch_bytes.argtypes = [u32, u64, u32, ctypes.POINTER(u64)]
    lib.fdf_fundamental_device.restype = ctypes.c_int
    lib.fdf_fundamental_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32,
                                           ctypes.c_float, u32, vp, vp, vp, u64, vp]
    lib.fdf_fundamental_check_device.restype = ctypes.c_int
    lib.fdf_fundamental_check_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, vp,
                                                 ctypes.c_float, vp, vp, vp]
    lib.fdf_fundamental_points.restype = ctypes.c_int
    lib.fdf_fundamental_points.argtypes = [vp, vp, vp, sz, sz, vp, vp, u32, u32, ctypes.c_float,
                                           u32, vp, vp]
    del u8p
    _lib = lib
    return lib


def status_string(status):
    return load().fdf_status_string(int(status)).decode()


def check(status, where=""):
    if status != FDF_OK:
        raise FdfError(status, where)


class Context:
    """One device + one HIP stream (fdf_ctx_create / fdf_ctx_destroy)."""

    def __init__(self, device=0):
        lib = load()
        handle = ctypes.c_void_p()
        check(lib.fdf_ctx_create(int(device), ctypes.byref(handle)), "fdf_ctx_create")
        self._lib = lib
        self.handle = handle
        self.device = int(device)

    @property
    def stream(self):
        return self._lib.fdf_ctx_stream(self.handle)

    def set_timing(self, enable=True, every=1):
        """Record the detector and compaction kernel durations of every `every`-th call
        (dispatch-timestamped HIP events; fdf_ctx_set_timing)."""
        check(self._lib.fdf_ctx_set_timing(self.handle, max(1, int(every)) if enable else 0))

    def timing(self):
        """(calls, detector_ms_total, compaction_ms_total) since timing was enabled."""
        n, a, b = ctypes.c_uint32(), ctypes.c_float(), ctypes.c_float()
        check(self._lib.fdf_ctx_timing(self.handle, ctypes.byref(n), ctypes.byref(a),
                                       ctypes.byref(b)))
        return n.value, a.value, b.value

    def timing_samples(self):
        """Per-call (detector_ms, compaction_ms) arrays since timing was enabled."""
        import numpy as np

        n = ctypes.c_uint32()
        check(self._lib.fdf_ctx_timing_samples(self.handle, None, None, 0, ctypes.byref(n)))
        det = np.zeros(n.value, dtype=np.float32)
        com = np.zeros(n.value, dtype=np.float32)
        if n.value:
            check(self._lib.fdf_ctx_timing_samples(self.handle, det.ctypes.data, com.ctypes.data,
                                                   n.value, ctypes.byref(n)))
        return det, com

    def workspace_bytes(self):
        """Device bytes held by the context's workspace (fdf_ctx_workspace_bytes)."""
        v = ctypes.c_uint64()
        check(self._lib.fdf_ctx_workspace_bytes(self.handle, ctypes.byref(v)))
        return v.value

    def set_geometry(self, min_tasks=0):
        """Band geometry override (fdf_ctx_set_geometry): min_tasks=1 gives small jobs the
        tall bands of large batches (tests); 0 restores the default."""
        check(self._lib.fdf_ctx_set_geometry(self.handle, int(min_tasks)))

    def set_band_rows(self, rows=0):
        """Band height override (fdf_ctx_set_band_rows): bands of ``rows`` centre rows for
        every later detection (same keypoints, other NMS tiers); 0 = automatic."""
        check(self._lib.fdf_ctx_set_band_rows(self.handle, int(rows)))

    def set_upload_chunks(self, chunks=0):
        """fdf_detect's overlapped upload (fdf_ctx_set_upload_chunks): the frame in
        ``chunks`` row chunks while the detector runs; 1 = one copy first; 0 = default."""
        check(self._lib.fdf_ctx_set_upload_chunks(self.handle, int(chunks)))

    def recoveries(self):
        """(upload_fallbacks, lookback_recoveries) the host calls made on their own
        (fdf_ctx_recoveries): both 0 in a healthy run."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.fdf_ctx_recoveries(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def close(self):
        if self.handle:
            self._lib.fdf_ctx_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
