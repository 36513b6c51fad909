/*
 * fdf.h -- C ABI of the MI355X (gfx950) FAST-9..16 corner detector.
 *
 * Drop-in boundary for the reference's hot path `fast_simd::detector`
 * (iwanders/feature_detector_fast src/fast_simd.rs:847-859), which the crate API calls from
 * `Config::detect` (src/lib.rs:56-58) and `detect` (src/lib.rs:62-64).  Every entry point
 * below names the reference interface it replaces.  A Rust shim that binds these symbols
 * is shown in INTEGRATION.md; the C++ mirror of the crate API is include/fdf.hpp.
 *
 * Semantics are the reference's, bit for bit (SURVEY.md §7 "semantic contract"):
 *   - centres x in [3, w-3), y in [3, h-3); circle order of src/fast_simd.rs:79-98;
 *   - bright <=> p > c + t, dark <=> p < c - t (strict, integer);
 *   - keypoint <=> a cyclic run of >= n bright or >= n dark circle pixels (9 <= n <= 16);
 *   - NMS (MaxThreshold / SumAbsolute): keep iff y not in {3, h-4} and the score is strictly
 *     greater than every 8-neighbour that is itself a keypoint (src/fast_simd.rs:589-616);
 *   - output: points in raster order (y ascending, then x).
 * Where the reference panics, these functions return an error code and never abort.
 *
 * Ownership: the caller owns every input and output buffer.  The library owns device
 * workspace inside an opaque context, reused across calls.  No global mutable state.
 * Threading: a context serialises its own host calls; distinct contexts may be used
 * concurrently from different threads.  One context = one device + one HIP stream.
 */
#ifndef FDF_H
#define FDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 still: fdf_select_scratch_bytes, fdf_select_device and fdf_select_points were added
 * without changing any existing function, which is backward compatible; so were
 * fdf_orient_disc, fdf_orient_device and fdf_orient_points, and fdf_brief_pattern,
 * fdf_brief_steer, fdf_smooth_device, fdf_describe_device and fdf_describe_points, and
 * fdf_match_device, fdf_match_filter_device and fdf_match_points, and fdf_resize_taps,
 * fdf_resize_device, fdf_resize_frame, fdf_pyramid_plan, fdf_pyramid_taps and
 * fdf_pyramid_device, and fdf_harris_codes, fdf_harris_device and fdf_harris_points, and
 * fdf_ransac_sample, fdf_ransac_scratch_bytes, fdf_ransac_device and fdf_ransac_points, and
 * fdf_refine_scratch_bytes, fdf_refine_device and fdf_refine_points, and fdf_warp_device,
 * fdf_warp_frame and fdf_model_invert, and fdf_track_device, fdf_track_frames,
 * fdf_track_map_position and fdf_track_map_displacement (with FDF_COORDS_Q11, which only the
 * tracker accepts), and fdf_fundamental_sample, fdf_fundamental_scratch_bytes,
 * fdf_fundamental_device, fdf_fundamental_check_device and fdf_fundamental_points. */
#define FDF_ABI_VERSION 6

/* Status codes.  Shapes the reference maps to an empty Vec return FDF_OK with 0 points. */
enum fdf_status {
    FDF_OK = 0,
    FDF_ERR_COUNT = 1,     /* count n outside [9, 16]: src/fast_simd.rs:302-305 (n<9), :800 (n>16) */
    FDF_ERR_SIZE = 2,      /* h < 3, or h >= 7 with w < 6: the u32 underflows at :342 / :369 */
    FDF_ERR_CAPACITY = 3,  /* output buffer too small; *n_out holds the required point count */
    FDF_ERR_NMS = 4,       /* non_maximal_supression value not 0, 1 or 2 */
    FDF_ERR_DEVICE = 5,    /* HIP runtime failure (no device, launch or copy error) */
    FDF_ERR_ARG = 6,       /* NULL pointer, stride < width, or a size that overflows */
    FDF_ERR_ALLOC = 7,     /* device or pinned host allocation failed */
    FDF_ERR_BUSY = 8,      /* pipeline: the ticket's slot still holds uncollected results */
    FDF_ERR_DROPPED = 9    /* pipeline: a batch found more keypoints than its device capacity */
};

/* src/lib.rs:26-36 NonMaximalSuppression {Off, MaxThreshold, SumAbsolute}. */
enum fdf_nms {
    FDF_NMS_OFF = 0,
    FDF_NMS_MAX_THRESHOLD = 1,
    FDF_NMS_SUM_ABSOLUTE = 2
};

/* src/lib.rs:40-52 Config {threshold: u8, count: u8, non_maximal_supression}. */
typedef struct fdf_config {
    uint8_t threshold;
    uint8_t count;
    uint8_t nms; /* enum fdf_nms */
} fdf_config;

/* src/lib.rs:17-20 Point {x: u32, y: u32}, laid out as #[repr(C)]. */
typedef struct fdf_point {
    uint32_t x;
    uint32_t y;
} fdf_point;

typedef struct fdf_ctx fdf_ctx;

/* Library/ABI identification. */
int fdf_abi_version(void);
const char* fdf_status_string(int status);
/* Number of visible HIP devices (0 when none); never fails. */
int fdf_device_count(void);

/* Validate a configuration and image shape without touching a device.  Returns FDF_OK and
 * sets *empty = 1 for the shapes the reference answers with an empty Vec (3 <= h <= 6, or
 * h >= 7 with w == 6); otherwise the error the reference would panic with. */
int fdf_validate(uint32_t width, uint32_t height, const fdf_config* cfg, int* empty);

/* Context: binds a device and creates a non-blocking HIP stream owned by the context. */
int fdf_ctx_create(int device, fdf_ctx** out_ctx);
void fdf_ctx_destroy(fdf_ctx* ctx);
/* The context's hipStream_t (as void*), for callers that enqueue their own work beside it. */
void* fdf_ctx_stream(fdf_ctx* ctx);

/* Profiling (extension, no reference counterpart): while enabled, each detect call on the
 * context (up to 4096 of them) records the durations of its two kernel launches -- the
 * detector (pre-filter, segment test, NMS, per-band slots) and the raster-order compaction
 * -- with HIP events the dispatches themselves timestamp (no packets between the kernels).
 * A call whose grid writes its points directly has no compaction launch: 0 ms.
 * enable = k > 1 records every k-th call only (the timestamped dispatches cost ~10 us each
 * on the queue, so a timed run samples).  fdf_ctx_timing waits for the recorded calls and
 * returns their number and the summed durations of both launches in ms.  Enabling resets the
 * record. */
int fdf_ctx_set_timing(fdf_ctx* ctx, int enable);
int fdf_ctx_timing(fdf_ctx* ctx, uint32_t* calls, float* detect_ms, float* compact_ms);
/* The same record per call: *n = calls recorded; the first `cap` calls' detector and
 * compaction durations (ms) go to detect_ms[k] / compact_ms[k] (for percentiles). */
int fdf_ctx_timing_samples(fdf_ctx* ctx, float* detect_ms, float* compact_ms, uint32_t cap,
                           uint32_t* n);

/* Geometry (extension; results never depend on it): the band height is chosen so that a
 * launch has at least `min_tasks` workgroups when it can (default 0 = 1024, enough for 4
 * per CU).  min_tasks = 1 makes a small job use the tall bands and long sweep units of
 * large batches -- the parity tests reach those code paths with small inputs this way. */
int fdf_ctx_set_geometry(fdf_ctx* ctx, uint32_t min_tasks);

/* Band height override: every later detection on the context sweeps bands of `rows` centre
 * rows (rounded up to the geometry's sub-band multiple, capped by what the workgroup's LDS
 * holds, 160 KB); 0 restores the automatic choice (LDS budget, grid size, and for NMS the
 * keypoint density of the previous launch).  The keypoints are the same at every height;
 * tests use it to cross the band NMS pass's LDS / spill / dense tiers.  rows > 256 (outside
 * the automatic choice's range): FDF_ERR_ARG. */
int fdf_ctx_set_band_rows(fdf_ctx* ctx, uint32_t rows);

/* How fdf_detect gets a host frame to the device (extension).  chunks = 0 (default): a
 * packed frame (stride = width) in pinned, non-coherent host memory (hipHostMalloc /
 * hipHostRegister without the coherent flag) is read in place by the detector over PCIe, no
 * copy first; any other frame is copied before the launch.  chunks = 1: always one copy.
 * chunks = k in 2..16: a frame of >= 256 KB goes up in k row chunks on a copy stream while
 * the detector already runs, each band waiting (on the device) for the chunk holding the last
 * row it reads -- on ROCm 7 each chunk's ready flag costs a small blit launch, so this
 * measured slower.  The keypoints are the same either way. */
int fdf_ctx_set_upload_chunks(fdf_ctx* ctx, uint32_t chunks);

/* Device bytes the context's workspace holds now (host-API staging and output, per-band
 * slots and counts, compaction sums).  Slots take 1/8 byte per pixel of the largest batch
 * seen; nothing in the workspace scales with more than that. */
int fdf_ctx_workspace_bytes(fdf_ctx* ctx, uint64_t* bytes);

/* Recoveries the host entry points made on their own since the context was created (ABI 6;
 * either pointer may be NULL): `upload_fallbacks` counts fdf_detect calls whose overlapped
 * upload (fdf_ctx_set_upload_chunks k > 1) had a band's chunk wait run out, so the frame was
 * detected again from one copy; `lookback_recoveries` counts host calls whose direct-output
 * look-back ran out and whose output the compaction rebuilt from the band slots.  Both stay
 * 0 in a healthy run -- tests assert it, so a handshake that never works cannot pass by its
 * fallback. */
int fdf_ctx_recoveries(fdf_ctx* ctx, uint64_t* upload_fallbacks, uint64_t* lookback_recoveries);

/* Test hook (no effect on results otherwise): moves the context's host-side count of the
 * direct-output start tickets by `delta`, as if the device counter and the host had fallen
 * out of step (after the context's first launch, which zeroes both).  The next direct-output
 * launch then hands `delta` workgroups tickets past its
 * grid; each one touches no band's memory and sets the context's device error, so that launch
 * is reported: a host call returns FDF_ERR_DEVICE, an asynchronous fdf_detect_device reports
 * it at the context's next device call, once, and the counter is re-zeroed (later calls are
 * correct).  tests/test_gpu_api.py drives it. */
int fdf_ctx_test_skew_tickets(fdf_ctx* ctx, uint32_t delta);

/*
 * Replaces fast_simd::detector(img, config) -> Vec<Point> (src/fast_simd.rs:847).
 * Host image (row-major u8, `stride_bytes` >= width; GrayImage always has stride == width),
 * host output.  Synchronous.  Two-call pattern: if `cap` is too small, returns
 * FDF_ERR_CAPACITY with *n_out = the required count and writes the first `cap` points; the
 * whole result stays on the device, and fdf_fetch_last copies it out without detecting
 * again.
 */
int fdf_detect(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
               size_t stride_bytes, const fdf_config* cfg, fdf_point* out, size_t cap,
               size_t* n_out);

/*
 * Second half of the two-call pattern: the points (frames concatenated, raster order) of
 * the last host-API detection on this context (fdf_detect, fdf_detect_rgb, fdf_detect_batch
 * and the scored variants), and their scores when `out_scores` is not NULL (the score kind
 * of that call's config, as fdf_detect_scored).  Only copies: no detection runs.
 * FDF_ERR_CAPACITY again if `cap` < *n_out; FDF_ERR_ARG if the context holds no result
 * (no host detection yet, or fdf_score_points ran since), or if scores are asked of an
 * unscored fdf_detect that fit its `cap` and read its pinned frame in place (the frame is not
 * kept; fdf_ctx_set_upload_chunks) -- a call that returned FDF_ERR_CAPACITY keeps it.
 */
int fdf_fetch_last(fdf_ctx* ctx, fdf_point* out, uint16_t* out_scores, size_t cap,
                   size_t* n_out);

/*
 * RGB variant of fdf_detect: `data` holds RGB8 pixels (rows of 3 * width bytes at
 * `stride_bytes`), converted on the device exactly as image 0.24.6's to_luma8 -- the
 * reference's callers run `DynamicImage::ImageRgb8(img).to_luma8()` before detect
 * (src/main.rs:58, tests/compare.rs:33) -- then detected as fdf_detect does.
 */
int fdf_detect_rgb(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                   size_t stride_bytes, const fdf_config* cfg, fdf_point* out, size_t cap,
                   size_t* n_out);

/*
 * Device-side RGB8 -> grey (image 0.24.6 to_luma8: (2126 r + 7152 g + 722 b) / 10000).
 * `n_frames` frames of width x height RGB pixels (rows packed, 3 * width bytes) at
 * d_rgb + f * rgb_frame_stride_bytes; grey frames packed (width * height bytes each) at
 * d_grey.  Asynchronous on `stream` (NULL = the HIP null stream).  n_frames <= 65535.
 */
int fdf_rgb_to_luma_device(fdf_ctx* ctx, const uint8_t* d_rgb, uint32_t n_frames,
                           uint32_t width, uint32_t height, uint64_t rgb_frame_stride_bytes,
                           uint8_t* d_grey, void* stream);

/*
 * Batched host variant: `n_frames` frames of width x height, frame f at
 * data + f * frame_stride_bytes (rows packed, stride == width).  Output is every frame's
 * list concatenated in frame order; frame f's points are out[frame_offsets[f] ..
 * frame_offsets[f+1]) (frame_offsets has n_frames + 1 entries; may be NULL).
 * Capacity semantics as fdf_detect.
 */
int fdf_detect_batch(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames, uint32_t width,
                     uint32_t height, size_t frame_stride_bytes, const fdf_config* cfg,
                     fdf_point* out, size_t cap, uint64_t* frame_offsets, size_t* n_out);

/*
 * Multi-device batched variant (frames shard across GPUs with no collective).
 * The batch is cut into n_ctx contiguous shards of (nearly) equal frame counts, shard k is
 * detected on ctxs[k] by its own host thread (contexts may be on different devices, or
 * several on one), and the lists are concatenated in frame order -- the same result as
 * fdf_detect_batch on one context.  The contexts must be distinct.  Capacity semantics as
 * fdf_detect_batch; each context keeps its shard for fdf_fetch_last_multi.  The contexts are
 * locked in one global order, so concurrent calls over the same contexts listed in different
 * orders do not deadlock.
 */
int fdf_detect_batch_multi(fdf_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* data,
                           uint32_t n_frames, uint32_t width, uint32_t height,
                           size_t frame_stride_bytes, const fdf_config* cfg, fdf_point* out,
                           size_t cap, uint64_t* frame_offsets, size_t* n_out);
/* fdf_fetch_last over the contexts of the last fdf_detect_batch_multi, concatenated.  The
 * contexts must hold the shards of ONE such call, passed in that call's order; otherwise (a
 * host call on one of them since, another multi call, a reordered array) FDF_ERR_ARG. */
int fdf_fetch_last_multi(fdf_ctx* const* ctxs, uint32_t n_ctx, fdf_point* out, size_t cap,
                         size_t* n_out);

/*
 * Device-resident batched variant (the throughput path; nothing crosses PCIe).
 * `d_frames`, `d_out` and `d_frame_offsets` are device pointers on the context's device.
 * Asynchronous: enqueued on `stream` (a hipStream_t; NULL = the HIP null stream; pass
 * fdf_ctx_stream(ctx) for the context's own stream).  On
 * completion d_frame_offsets[0..n_frames] holds the exclusive prefix of per-frame counts
 * and d_frame_offsets[n_frames] the total, even when the total exceeds `cap` (points with
 * index >= cap are not written).  Argument and shape errors are returned synchronously.
 * The context's workspace is reused by each call: a call on another stream than the
 * context's previous call first waits (on the device) for that call's work.  Frames may be
 * spaced by any frame_stride_bytes >= width * height (the gap bytes are never centres or
 * circle pixels); frames before the last may be read up to 15 bytes past their end (inside
 * the batch allocation), the last frame is read exactly.  FDF_ERR_DEVICE is also returned,
 * once, by the call after an asynchronous launch whose output could not be completed (a
 * grid small enough to write its points directly, whose look-back wait ran out: the
 * bounded wait that keeps a faulty device from hanging; the host entry points recover such
 * a launch by themselves).
 */
int fdf_detect_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                      uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                      const fdf_config* cfg, fdf_point* d_out, uint64_t cap,
                      uint64_t* d_frame_offsets, void* stream);

/*
 * fdf_detect_device for RGB8 frames (rows of 3 * width bytes, frame f at
 * d_frames + f * frame_stride_bytes): the detector converts each loaded pixel with image
 * 0.24.6's to_luma8 -- (2126 r + 7152 g + 722 b) / 10000 -- so the keypoints are those of
 * fdf_rgb_to_luma_device followed by fdf_detect_device, with no grey frames written
 * (src/main.rs:58, tests/compare.rs:33).  3 * width * height < 2^31.  It needs no grey
 * buffer but is slower than the two passes, which the host RGB entry
 * points use.
 */
int fdf_detect_device_rgb(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                          uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                          const fdf_config* cfg, fdf_point* d_out, uint64_t cap,
                          uint64_t* d_frame_offsets, void* stream);

/*
 * Ring-level helpers, the reference's pub items of src/fast_simd.rs:
 *   FDF_NORTH..FDF_WEST   :69-72   circle indices of the four cardinal pixels
 *   fdf_circle            :79-98   (dx, dy) of the 16 circle pixels, index 0 north, clockwise
 *   fdf_calculate_offsets :104-110 dy * width + dx (i32, as the reference computes it)
 * Either output pointer of fdf_circle may be NULL.  Host-only, no context needed.
 */
#define FDF_NORTH 0
#define FDF_EAST 4
#define FDF_SOUTH 8
#define FDF_WEST 12
void fdf_circle(int32_t dx[16], int32_t dy[16]);
void fdf_calculate_offsets(uint32_t width, int32_t offsets[16]);

/*
 * Ring scores, the reference's keypoint_score_max_threshold(base_v, pixels, consecutive)
 * (src/fast_simd.rs:623) and keypoint_score_sum_abs_difference(pixels, centers, is_above,
 * is_below, threshold) (:722) with the masks its callers build (:282, test :1213-1222:
 * is_above = p > sat(c + t), is_below = p < sat(c - t)).  Ring k is centers[k] and the 16
 * circle pixels rings[16 k .. 16 k + 16) in fdf_circle order.  cfg->nms picks the function:
 * MaxThreshold (consecutive = cfg->count, 9..16) or SumAbsolute (threshold = cfg->threshold).
 * Runs on the GPU through the detector's own score functions (see fdf_kernels.hip), for any
 * ring.  fdf_score_rings: host in/out, synchronous; invalidates fdf_fetch_last's result.
 * fdf_score_rings_device: device pointers, d_rings 16-byte aligned, asynchronous on
 * `stream` (NULL = the HIP null stream, as for fdf_detect_device; round 6 -- NULL meant the
 * context's stream before, which is not ordered with work on the null stream).
 */
int fdf_score_rings(fdf_ctx* ctx, const uint8_t* centers, const uint8_t* rings, size_t n_rings,
                    const fdf_config* cfg, uint16_t* out_scores);
int fdf_score_rings_device(fdf_ctx* ctx, const uint8_t* d_centers, const uint8_t* d_rings,
                           uint64_t n_rings, const fdf_config* cfg, uint16_t* d_scores,
                           void* stream);

/*
 * Scores for given points (extension: the reference's Point carries no score; these are the
 * u16 values its NMS compares, src/fast_simd.rs:623-718 and :722-749).  Host in/out,
 * synchronous.  `nms` selects the score: MaxThreshold (window = cfg->count) or SumAbsolute
 * (uses cfg->threshold).  Points must be centres (3 <= x < w-3, 3 <= y < h-3).
 */
int fdf_score_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                     size_t stride_bytes, const fdf_config* cfg, const fdf_point* points,
                     size_t n_points, uint16_t* out_scores);

/*
 * Detection with scores: (x, y, score) per keypoint.  As fdf_detect / fdf_detect_batch,
 * and out_scores[k] (`cap` entries) is point k's u16 score -- the one cfg->nms suppresses
 * with (MaxThreshold: src/fast_simd.rs:623-718; SumAbsolute: :722-749), or the
 * max-threshold score when NMS is off.  Scores are computed on the device from the frame
 * already resident there; capacity semantics as fdf_detect.
 */
int fdf_detect_scored(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_config* cfg, fdf_point* out,
                      uint16_t* out_scores, size_t cap, size_t* n_out);
int fdf_detect_batch_scored(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames,
                            uint32_t width, uint32_t height, size_t frame_stride_bytes,
                            const fdf_config* cfg, fdf_point* out, uint16_t* out_scores,
                            size_t cap, uint64_t* frame_offsets, size_t* n_out);

/*
 * Device-resident scoring of fdf_detect_device's output: d_points / d_frame_offsets as that
 * call filled them (same frames, shape, config and `cap`), d_scores with `cap` entries.
 * Asynchronous on `stream`; points with index >= cap are skipped.  n_frames <= 65535.
 */
int fdf_score_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                     uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                     const fdf_config* cfg, const fdf_point* d_points, uint64_t cap,
                     const uint64_t* d_frame_offsets, uint16_t* d_scores, void* stream);

/*
 * Grid-bucketed best-K keypoint selection (extension: the reference returns every keypoint;
 * its callers keep "the strongest K" or "the strongest K per grid cell").
 *
 * Input is what fdf_detect_device followed by fdf_score_device leave on the device: frame f
 * owns the indices [offs[f], min(offs[f+1], cap)), in raster order, with x < width and
 * y < height, and one u16 score per point (any u16 value).  Cells are cell_w x cell_h pixels
 * (0 = the whole image dimension; cell_w = cell_h = 0 is "best K of the frame"):
 * cells_x = ceil(width / cell_w), the cell of (x, y) is (y / cell_h) * cells_x + x / cell_w,
 * and cells never span frames.  The rank of point i is the number of points j of its frame
 * and cell with score[j] > score[i], or score[j] == score[i] and j < i; a point is kept iff
 * its rank is below k (a stable sort by descending score; ties at the cut go to the earlier
 * point).  The kept points of each frame are written in input order with their scores;
 * d_sel_offsets[0..n_frames] is the exclusive prefix of the per-frame kept counts and
 * d_sel_offsets[n_frames] the full total even when it exceeds sel_cap (entries at index
 * >= sel_cap are not written), as fdf_detect_device does.  d_keep (optional, `cap` bytes)
 * gets 1 for a kept point and 0 otherwise.  The result is a pure function of the inputs.
 * Input that is not in raster order or lies outside the image gives an unspecified selection
 * for its frame; no access leaves the caller's buffers.
 *
 * fdf_select_scratch_bytes: host only, no context or device needed; the scratch size
 * fdf_select_device needs for these arguments (0 for the shapes the reference answers with an
 * empty list and for n_frames == 0).  width * height < 2^32.
 *
 * fdf_select_device: asynchronous on `stream` (NULL = the HIP null stream, as for
 * fdf_score_device); like that function it takes no context lock and uses no context
 * workspace, it only binds the context's device.  Nothing is allocated and nothing returns
 * to the host.  d_scratch (256-byte aligned, at least the queried size) needs no
 * initialisation and may be reused by the next call in stream order.  FDF_ERR_ARG,
 * synchronously and with nothing launched: k == 0, a NULL required pointer, a scratch that is
 * too small or misaligned, n_frames > 65535.  Empty shapes and n_frames == 0 zero
 * d_sel_offsets and return FDF_OK.
 *
 * fdf_select_points: host arrays in and out, synchronous.  frame_offsets (n_frames + 1
 * entries) may be NULL for one frame of n_points points.  Two-call pattern as fdf_detect:
 * FDF_ERR_CAPACITY with *n_out = the required count (the first `cap` are written).  Copies
 * through device buffers allocated and freed by the call and runs the same kernels; the
 * context's workspace and retained result are untouched, so fdf_fetch_last stays valid.
 * out_offsets (n_frames + 1 entries) may be NULL.
 */
int fdf_select_scratch_bytes(uint32_t n_frames, uint32_t width, uint32_t height,
                             uint32_t cell_w, uint32_t cell_h, uint64_t cap, uint64_t* bytes);
int fdf_select_device(fdf_ctx* ctx, uint32_t n_frames, uint32_t width, uint32_t height,
                      const fdf_point* d_points, const uint16_t* d_scores, uint64_t cap,
                      const uint64_t* d_frame_offsets, uint32_t cell_w, uint32_t cell_h,
                      uint32_t k, fdf_point* d_sel, uint16_t* d_sel_scores, uint64_t sel_cap,
                      uint64_t* d_sel_offsets, uint8_t* d_keep, void* d_scratch,
                      uint64_t scratch_bytes, void* stream);
int fdf_select_points(fdf_ctx* ctx, const fdf_point* points, const uint16_t* scores,
                      const uint64_t* frame_offsets, uint32_t n_frames, size_t n_points,
                      uint32_t width, uint32_t height, uint32_t cell_w, uint32_t cell_h,
                      uint32_t k, fdf_point* out, uint16_t* out_scores, size_t cap,
                      uint64_t* out_offsets, size_t* n_out);

/*
 * Keypoint orientation by intensity centroid (extension: the reference returns points only;
 * this is the angle of oFAST / ORB, OpenCV's IC_Angle).
 *
 * Disc.  radius r, 1 <= r <= 31 (ORB's patch of 31 is r = 15).  Row v of the disc, |v| <= r,
 * spans the columns |d| <= u[|v|], with the half-widths u[0..r] of OpenCV's umax rule:
 * vmax = floor(r * sqrt(2) / 2 + 1), vmin = ceil(r * sqrt(2) / 2); u[v] =
 * floor(sqrt(r^2 - v^2) + 0.5) for v in 0..vmax; then with v0 = 0, for v from r down to vmin:
 * advance v0 while u[v0] == u[v0 + 1], set u[v] = v0, then v0++.  r = 15 gives
 * 15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3 (749 pixels).
 *
 * Moments, exact in int32: for the keypoint (x, y) of a frame
 *   m10 = sum over v, |d| <= u[|v|] of d * I(x + d, y + v)
 *   m01 = sum over v, |d| <= u[|v|] of v * I(x + d, y + v)
 * where I(cx, cy) is the pixel at (clamp(cx, 0, width - 1), clamp(cy, 0, height - 1)): a
 * replicated border; the weights d and v are not clamped.  |m| < 2^24 for every r <= 31, so
 * the conversion to float is exact.  For keypoints at least r pixels inside the frame these
 * are OpenCV's moments; a caller who wants its edgeThreshold filters the others.
 *
 * Angle = atan2f((float)m01, (float)m10), radians in (-pi, pi], y pointing down;
 * m10 = m01 = 0 gives exactly 0.0f.
 *
 * fdf_orient_disc: host only, no context; writes u[0..radius] (radius + 1 entries).
 * FDF_ERR_ARG for radius 0, radius > 31 or a NULL pointer.
 *
 * fdf_orient_device: the inputs are what fdf_detect_device (or fdf_select_device) leaves on
 * the device: frame f owns the indices [offs[f], min(offs[f+1], cap)) and its pixels start at
 * d_frames + f * frame_stride_bytes (any alignment).  d_angles gets `cap` floats, d_moments
 * (optional) 2 int32 per point, m10 then m01; entries at index >= min(offs[n_frames], cap)
 * are not written.  Asynchronous on `stream` (NULL = the HIP null stream); like
 * fdf_score_device it takes no context lock and uses no context workspace, it only binds the
 * context's device; nothing is allocated and nothing returns to the host.  FDF_ERR_ARG,
 * synchronously and with nothing launched: a bad radius, a NULL required pointer,
 * n_frames > 65535, a frame stride below width * height when n_frames > 1.  Shape errors and
 * empty shapes as for fdf_score_device (FDF_OK, nothing written); width * height above
 * 2^31 - 256 is FDF_ERR_SIZE.  A point with x >= width or y >= height gives an unspecified
 * value for that point.  Whatever the points hold, no access leaves
 * [d_frames, d_frames + (n_frames - 1) * stride + width * height) or the other buffers.
 *
 * fdf_orient_points: one host frame (rows stride_bytes apart) and host points, synchronous.
 * Points outside the image are rejected with FDF_ERR_ARG.  Copies through device buffers
 * allocated and freed by the call and runs the same kernel; the context's workspace and
 * retained result are untouched, so fdf_fetch_last stays valid.  out_moments may be NULL.
 */
int fdf_orient_disc(uint32_t radius, uint8_t* half_widths);
int fdf_orient_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                      uint64_t cap, const uint64_t* d_frame_offsets, uint32_t radius,
                      float* d_angles, int32_t* d_moments, void* stream);
int fdf_orient_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_point* points, size_t n_points,
                      uint32_t radius, float* out_angles, int32_t* out_moments);

/*
 * Harris corner response of keypoints (extension: the reference returns points only; this is
 * the score ORB ranks its FAST keypoints by, OpenCV's HarrisResponses / HARRIS_SCORE).
 * Everything is exact integer arithmetic and a pure function of the inputs.
 *
 * Pixel reads.  I(cx, cy) is the pixel at (clamp(cx, 0, width - 1), clamp(cy, 0, height - 1)):
 * the replicated border of fdf_orient_device.
 *
 * Gradients (3 x 3 Sobel), at any position (X, Y):
 *   Ix = 2 (I(X+1,Y) - I(X-1,Y)) + (I(X+1,Y-1) - I(X-1,Y-1)) + (I(X+1,Y+1) - I(X-1,Y+1))
 *   Iy = 2 (I(X,Y+1) - I(X,Y-1)) + (I(X-1,Y+1) - I(X-1,Y-1)) + (I(X+1,Y+1) - I(X+1,Y-1))
 * so |Ix|, |Iy| <= 4 * 255 = 1020.
 *
 * Block sums.  block is 3, 5 or 7 (ORB's is 7), hb = block / 2.  For the keypoint (x, y), over
 * |d| <= hb, |v| <= hb and (X, Y) = (x + d, y + v):
 *   a = sum Ix^2,   b = sum Iy^2,   c = sum Ix Iy.
 * a, b <= 49 * 1020^2 = 50 979 600 and |c| <= the same: all three fit int32.  The pixels read
 * are the (block + 2)^2 window around the keypoint.
 *
 * Response.  R = k_den (a b - c^2) - k_num (a + b)^2 in int64; the Harris constant is the
 * rational k = k_num / k_den, 0 <= k_num <= 255, 1 <= k_den <= 255 (ORB's 0.04 is 1 / 25).
 * 0 <= a b - c^2 <= 50 979 600^2 and (a + b)^2 <= (2 * 50 979 600)^2 < 2^54, so both terms
 * stay below 255 * (2 * 50 979 600)^2 < 2^62 < 2^63 and no step overflows.  For keypoints at
 * least hb + 1 pixels inside the frame R / k_den * (1 / (4 * block * 255))^4 is OpenCV's float
 * response up to its float rounding; no bit parity with OpenCV is claimed.
 *
 * Rank score (u16), the key fdf_select_device ranks by.  code(R) = 0 for R <= 0; otherwise with
 * e = floor(log2 R): code = R for e < 10, and (e - 9) << 10 | ((R >> (e - 10)) & 1023) for
 * e >= 10: a monotone non-decreasing "6.10 minifloat" of R (implicit leading bit, 10 mantissa
 * bits), continuous at 1023 -> 1024, 55295 at R = 2^63 - 1.  Two responses get different
 * codes whenever they differ in their top 11 significant bits; equal codes are broken by
 * fdf_select_device's stable rule, and a caller who needs the exact order uses the int64 output.
 *
 * fdf_harris_codes: host only, no context; codes[i] = code(responses[i]).  FDF_ERR_ARG for a
 * NULL pointer with n > 0.
 *
 * fdf_harris_device: the inputs are what fdf_detect_device (or fdf_select_device) leaves on
 * the device: frame f owns the indices [offs[f], min(offs[f+1], cap)) and its pixels start at
 * d_frames + f * frame_stride_bytes (any alignment).  d_scores gets `cap` rank scores,
 * d_responses (optional, 8-byte aligned) `cap` int64 responses; entries at index
 * >= min(offs[n_frames], cap) are not written.  Asynchronous on `stream` (NULL = the HIP null
 * stream); like fdf_score_device it takes no context lock and uses no context workspace, it
 * only binds the context's device; nothing is allocated and nothing returns to the host.
 * FDF_ERR_ARG, synchronously and with nothing launched: a block other than 3, 5, 7, a k
 * outside the ranges above, a NULL required pointer, n_frames > 65535, a frame stride below
 * width * height when n_frames > 1, a d_responses that is not 8-byte aligned.  Shape errors
 * and empty shapes as for fdf_score_device (FDF_OK, nothing written); width * height above
 * 2^31 - 256 is FDF_ERR_SIZE.  A point with x >= width or y >= height gives an unspecified
 * value for that point.  Whatever the points hold, no access leaves
 * [d_frames, d_frames + (n_frames - 1) * stride + width * height) or the other buffers.
 *
 * fdf_harris_points: one host frame (rows stride_bytes apart) and host points, synchronous.
 * Points outside the image are rejected with FDF_ERR_ARG.  Copies through device buffers
 * allocated and freed by the call and runs the same kernel; the context's workspace and
 * retained result are untouched, so fdf_fetch_last stays valid.  out_responses may be NULL.
 */
int fdf_harris_codes(const int64_t* responses, size_t n, uint16_t* codes);
int fdf_harris_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                      uint64_t cap, const uint64_t* d_frame_offsets, uint32_t block,
                      uint32_t k_num, uint32_t k_den, uint16_t* d_scores, int64_t* d_responses,
                      void* stream);
int fdf_harris_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_point* points, size_t n_points,
                      uint32_t block, uint32_t k_num, uint32_t k_den, uint16_t* out_scores,
                      int64_t* out_responses);

/*
 * Steered BRIEF descriptors (extension: the reference returns points only; this is the rBRIEF
 * of ORB, the step after fdf_orient_device) and the 5 x 5 box smoothing BRIEF is usually run
 * on.  Everything is integer-exact.
 *
 * Pattern.  256 tests; test i is four int8 (x0, y0, x1, y1), 1024 bytes in all.  A caller who
 * owns OpenCV's learned ORB table passes that.  fdf_brief_pattern writes a deterministic
 * default: xorshift32 with state s = 0x9E3779B9, next() = { s ^= s << 13; s ^= s >> 17;
 * s ^= s << 5; return s; } in uint32, coord() = the sum of six successive next() >> 29, minus
 * 21 (bell-shaped in -21..21).  A draw is x0, y0, x1, y1 from four coord() calls in that
 * order; it is rejected if either point has x^2 + y^2 > 13^2, if the two points are equal or
 * if the same 4-tuple was accepted before; 256 tests are accepted (after 278 draws; test 0 is
 * 5, 8, -11, -2; crc32 of the bytes 1958958545).  Host only, no context.
 *
 * Steering table.  fdf_brief_steer writes n_bins x 256 x 4 int8, 1 <= n_bins <= 360: bin b
 * holds every pattern point rotated by theta = 2 pi b / n_bins with y pointing down (the
 * angle of fdf_orient_device): x' = x cos theta - y sin theta, y' = x sin theta + y cos theta,
 * computed in double, rounded to float, that float rounded half away from zero to an integer
 * and saturated to int8.  Bin 0 is the pattern itself.  Host only; FDF_ERR_ARG for a NULL
 * pointer or n_bins outside 1..360.
 *
 * Bin of an angle.  With scale = (float)(n_bins / (2 pi)) (computed in double), t = the float
 * product angle * scale (rounded once, not fused), the bin is t rounded to the nearest integer,
 * ties to even, taken modulo n_bins into [0, n_bins).  An angle for which |angle| <= 7 is false
 * (NaN and the infinities included) has bin 0.  d_angles == NULL means bin 0 for every point:
 * unsteered BRIEF.
 *
 * Descriptor.  For the keypoint (x, y) in bin b, bit i is 1 iff I(x + x0, y + y0) <
 * I(x + x1, y + y1) with (x0, y0, x1, y1) = table[b][i] and I read at coordinates clamped to
 * the frame (the replicated border of fdf_orient_device).  Bit i is bit i % 8 of byte i / 8
 * (test 0 is the least significant bit of byte 0, OpenCV's packing); 32 bytes per keypoint.
 *
 * Smoothing.  out(x, y) = (sum over |dx| <= 2, |dy| <= 2 of I(clamp(x + dx), clamp(y + dy))
 * + 12) / 25 in integers, for any width, height >= 1 with width * height <= 2^31 - 256
 * (FDF_ERR_SIZE otherwise).  Frames may be any number of bytes apart on either side; the gap
 * bytes of the output are not written; input and output must not overlap.  The descriptor
 * step reads whatever frames it is given: smoothing is the caller's choice.
 *
 * fdf_smooth_device, fdf_describe_device: asynchronous on `stream` (NULL = the HIP null
 * stream); like fdf_orient_device they take no context lock and use no context workspace, they
 * only bind the context's device; nothing is allocated and nothing returns to the host.
 * fdf_describe_device's indexing is fdf_orient_device's: frame f owns the indices [offs[f],
 * min(offs[f+1], cap)), d_desc gets 32 bytes per point and entries at index >=
 * min(offs[n_frames], cap) are not written.  FDF_ERR_ARG, synchronously and with nothing
 * launched: a NULL required pointer, n_frames > 65535, a frame stride below width * height when
 * n_frames > 1, n_bins outside 1..360.  For fdf_describe_device shape errors and empty shapes
 * are as for fdf_orient_device (FDF_OK, nothing written).  A point with x >= width or
 * y >= height gives an unspecified descriptor.  Whatever the points, angles and table hold, no
 * access leaves the frames' bytes or the other buffers.  Frames, table and descriptors may have any alignment.
 *
 * fdf_describe_points: one host frame (rows stride_bytes apart, any width, height >= 1) and
 * host points, synchronous; angles may be NULL, pattern NULL is the default pattern, smooth is
 * 0 or 1 (1: the descriptors are taken from the smoothed frame).  Points outside the image are
 * rejected with FDF_ERR_ARG.  Copies through device buffers allocated and freed by the call
 * and runs the same kernels; the context's workspace and retained result are untouched, so
 * fdf_fetch_last stays valid.
 */
int fdf_brief_pattern(int8_t pattern[1024]);
int fdf_brief_steer(const int8_t* pattern, uint32_t n_bins, int8_t* table);
int fdf_smooth_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, uint8_t* d_out,
                      uint64_t out_frame_stride_bytes, void* stream);
int fdf_describe_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                        uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                        uint64_t cap, const uint64_t* d_frame_offsets, const float* d_angles,
                        const int8_t* d_table, uint32_t n_bins, uint8_t* d_desc, void* stream);
int fdf_describe_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                        size_t stride_bytes, const fdf_point* points, size_t n_points,
                        const float* angles, const int8_t* pattern, uint32_t n_bins, int smooth,
                        uint8_t* out_desc);

/*
 * Brute-force Hamming matching of the descriptors (extension: the reference returns points
 * only; the step after fdf_describe_device).  Everything is exact integer arithmetic and the
 * result is a pure function of the inputs.
 *
 * Sets.  A set is what fdf_describe_device leaves on the device: 32 bytes per point and an
 * offsets array.  Frame f of the query set owns the indices [qo[f], min(qo[f+1], q_cap)), frame
 * f of the train set [to[f], min(to[f+1], t_cap)); frame f of the one is matched against frame
 * f of the other and against nothing else.  The two sets may share one descriptor array:
 * matching every frame of a batch of F against the next one is d_q_offsets = offs,
 * d_t_offsets = offs + 1, n_frames = F - 1 over the same d_desc.  Indices in the result are
 * global indices into the train arrays, not frame-relative; q_cap and t_cap must be below
 * 2^32 - 1 (FDF_ERR_ARG).
 *
 * Distance.  d(i, j) = the number of set bits of the XOR of the two descriptors, 0..256.
 *
 * Candidates of query i: every train index of its frame; with both point arrays given, only
 * those with |x_q - x_t| <= max_dx and |y_q - y_t| <= max_dy (unsigned absolute differences,
 * no wrap).  Both point arrays NULL: no window, max_dx and max_dy are ignored; one NULL and
 * one not: FDF_ERR_ARG.  With a window the train points of a frame must have non-decreasing
 * y, which the raster order of the detector and of fdf_select_device guarantees; queries may
 * come in any order.  A train frame that breaks the order gets unspecified matches, but even
 * then every reported index lies in that frame's train range or is FDF_MATCH_NONE, and no
 * access leaves the buffers.
 *
 * Result for query i.  index = the candidate with the smallest (d, j) in lexicographic order
 * (ties go to the lowest index), distance = its d, second = the smallest d over the candidates
 * other than index (it may equal distance).  No candidate: {FDF_MATCH_NONE, 0xFFFF, 0xFFFF};
 * one candidate: second = 0xFFFF.  Entries outside [qo[0], min(qo[n_frames], q_cap)) are not
 * written.
 *
 * Filter.  fdf_match_filter_device writes, for every i in [qo[0], min(qo[n_frames], q_cap)) and
 * for no other byte, d_keep[i] = 1 if all of these hold and 0 otherwise:
 *   index != FDF_MATCH_NONE;
 *   distance <= max_distance (any max_distance >= 256 disables this test);
 *   the ratio test: ratio_den == 0 (off), or second == 0xFFFF, or distance * ratio_den <
 *   second * ratio_num in uint32 (Lowe's 0.75 is 3 / 4; both terms <= 65535, FDF_ERR_ARG
 *   otherwise);
 *   the cross-check: d_reverse == NULL (off), or index < t_cap and d_reverse[index].index == i,
 *   where d_reverse (t_cap entries) is the result of the same match with the sets swapped.
 * An index a match holds is compared with t_cap before d_reverse is read at it.
 *
 * fdf_match_device, fdf_match_filter_device: asynchronous on `stream` (NULL = the HIP null
 * stream); they take no context lock and use no context workspace, they only bind the
 * context's device; nothing is allocated and nothing returns to the host.  FDF_ERR_ARG,
 * synchronously and with nothing launched: a NULL required pointer, n_frames > 65535, a cap of
 * 2^32 - 1 or more, a descriptor pointer that is not 4-byte aligned, a match array that is not
 * 8-byte aligned.  n_frames == 0 or q_cap == 0: FDF_OK, nothing written.  d_t_desc may be NULL
 * when t_cap == 0.
 *
 * fdf_match_points: one pair of host sets, synchronous; nothing about the points is rejected
 * except one array without the other; n_q == 0 is FDF_OK.  Copies through device buffers
 * allocated and freed by the call and runs the same kernel; the context's workspace and
 * retained result are untouched, so fdf_fetch_last stays valid.
 */
#define FDF_MATCH_NONE 0xFFFFFFFFu      /* index of a query with no candidate */
#define FDF_MATCH_NO_DISTANCE 0xFFFFu   /* distance / second when there is none */
typedef struct fdf_match {
    uint32_t index;
    uint16_t distance;
    uint16_t second;
} fdf_match;
int fdf_match_device(fdf_ctx* ctx, uint32_t n_frames, const uint8_t* d_q_desc,
                     const fdf_point* d_q_points, uint64_t q_cap, const uint64_t* d_q_offsets,
                     const uint8_t* d_t_desc, const fdf_point* d_t_points, uint64_t t_cap,
                     const uint64_t* d_t_offsets, uint32_t max_dx, uint32_t max_dy,
                     fdf_match* d_matches, void* stream);
int fdf_match_filter_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                            uint64_t q_cap, const uint64_t* d_q_offsets,
                            const fdf_match* d_reverse, uint64_t t_cap, uint32_t max_distance,
                            uint32_t ratio_num, uint32_t ratio_den, uint8_t* d_keep,
                            void* stream);
int fdf_match_points(fdf_ctx* ctx, const uint8_t* q_desc, const fdf_point* q_points, size_t n_q,
                     const uint8_t* t_desc, const fdf_point* t_points, size_t n_t,
                     uint32_t max_dx, uint32_t max_dy, fdf_match* out);

/*
 * RANSAC estimation of an affine map or a homography from the matches (extension: the reference
 * returns points only; the step after fdf_match_device / fdf_match_filter_device, OpenCV's
 * estimateAffine2D / findHomography with RANSAC).  The result is a pure function of the inputs:
 * the sampling is an integer generator, every floating-point step below is one IEEE binary64
 * operation rounded once (never fused into a multiply-add), and ties are broken by index.
 *
 * Correspondences of frame f.  d_matches (q_cap entries), d_q_offsets and d_t_offsets are what
 * fdf_match_device takes and leaves; d_keep (optional, q_cap bytes, NULL = all ones) is
 * fdf_match_filter_device's; d_q_coords (q_cap) and d_t_coords (t_cap) hold 8 bytes per point:
 * with coords = FDF_COORDS_U32 an fdf_point, as the detector and fdf_select_device write them,
 * with FDF_COORDS_F32 two floats x, y (the level-0 coordinates of a multi-scale caller).  Both
 * convert to double exactly.  Query i in [qo[f], min(qo[f+1], q_cap)) is a correspondence of
 * frame f iff keep[i] != 0, matches[i].index != FDF_MATCH_NONE and matches[i].index lies in
 * [to[f], min(to[f+1], t_cap)).  A frame's correspondences are numbered j = 0..M-1 in increasing
 * i; correspondence j is (x, y) = the query coordinates of i and (u, v) = the train coordinates
 * of matches[i].index.
 *
 * Model.  FDF_MODEL_AFFINE: sample size s = 3, N = 6 unknowns; FDF_MODEL_HOMOGRAPHY: s = 4,
 * N = 8.  The result is nine doubles h0..h8, row-major, h8 = 1; affine: h6 = h7 = 0.
 *
 * Sampling of hypothesis h of frame f with the caller's seed, in uint32 with wrap:
 *   st = seed + 0x9E3779B9 * (f + 1) + 0x85EBCA6B * (h + 1);
 *   st ^= st >> 16; st *= 0x85EBCA6B; st ^= st >> 13; st *= 0xC2B2AE35; st ^= st >> 16;
 *   if (st == 0) st = 0x9E3779B9;
 * next() is fdf_brief_pattern's xorshift32 { st ^= st << 13; st ^= st >> 17; st ^= st << 5;
 * return st; }.  A draw is j = ((uint64_t)next() * M) >> 32; it is accepted if it differs from
 * the draws accepted before; the sample is the first s accepted draws in that order.  16 draws
 * without s distinct values: the hypothesis is invalid (so is every hypothesis when M < s: the
 * frame has no model).  The start state of seed 1, f 0, h 0 is 0xB0198235; (seed 1, f 0, h 0,
 * M 100, s 4) gives 54, 11, 77, 18 after 4 draws, (1, 2, 7, 5, 4) gives 1, 0, 4, 2 after 5 and
 * (0, 0, 0, 4, 4) gives 2, 1, 3, 0 after 7.
 *
 * Fit.  Sample point k = 0..s-1 gives two rows of the N x N system A h = b:
 *   row 2k     = [x, y, 1, 0, 0, 0, -(u x), -(u y)],  b = u
 *   row 2k + 1 = [0, 0, 0, x, y, 1, -(v x), -(v y)],  b = v
 * (affine: the first six columns).  Gaussian elimination with partial pivoting, for column
 * c = 0..N-1: the pivot row p is the lowest r >= c with the largest |A[r][c]| (a NaN magnitude
 * never wins); the hypothesis is invalid unless |A[p][c]| >= 2^-20; rows c and p are swapped;
 * for each r > c: m = A[r][c] / A[c][c], A[r][j] = A[r][j] - m * A[c][j] for j = c+1..N-1 and
 * b[r] = b[r] - m * b[c].  Back substitution for i = N-1 down to 0: t = b[i]; for j = i+1..N-1
 * ascending t = t - A[i][j] * h[j]; h[i] = t / A[i][i].
 *
 * Score.  For every correspondence of the frame, with T = (double)threshold:
 *   P = (h0 x + h1 y) + h2,  Q = (h3 x + h4 y) + h5,  w = (h6 x + h7 y) + h8,
 *   rx = P - u w,  ry = Q - v w,  e = rx rx + ry ry,  lim = (T T) (w w);
 * an inlier iff w > 0 and e <= lim (both false for a NaN): a forward transfer error of at most
 * T pixels, without a division.  A valid hypothesis' count is its number of inliers; the best
 * hypothesis has the largest count, ties go to the lowest h.
 *
 * Output.  d_models[f] gets the best hypothesis' model bit for bit as fitted (no refit over the
 * inliers), n_corr = M, n_inliers, hypothesis and n_valid = the number of valid hypotheses.  No
 * valid hypothesis (or M < s): h all zero, n_inliers 0, hypothesis 0xFFFFFFFF.  d_inliers
 * (optional, q_cap bytes) gets, for every i in [qo[0], min(qo[n_frames], q_cap)) and for no other
 * byte, 1 if i is a correspondence and an inlier of its frame's best model and 0 otherwise.
 *
 * Example.  Queries (0,0), (10,0), (0,10), (10,10), (4,7), (20,3); trains = query + (3,5) except
 * the fifth, (50,50); matches[i].index = i, seed 0, one frame, 8 hypotheses, T = 1.  Both models:
 * hypothesis 3, 5 inliers, n_valid 8, inlier bytes 1 1 1 1 0 1, h = 1 0 3 0 1 5 0 0 1 (a zero
 * may carry either sign).  The homography's counts per hypothesis are 1 2 1 5 2 1 2 2.
 *
 * fdf_ransac_sample: host only, no context; the sample of one hypothesis in idx[0..s) and the
 * draws made in *draws (may be NULL).  An invalid hypothesis (m < s included) fills idx with
 * 0xFFFFFFFF after its 16 draws.  FDF_ERR_ARG: s not 3 or 4, a NULL idx.
 *
 * fdf_ransac_scratch_bytes: host only; the size of fdf_ransac_device's d_scratch (256-byte
 * aligned; needs no initialisation and may be reused in stream order): 32 bytes per query index,
 * 4 per frame and 4 per (frame, hypothesis).  FDF_ERR_ARG: NULL bytes, n_frames > 65535,
 * q_cap of 2^32 - 1 or more, n_hyp outside 1..65536.
 *
 * fdf_ransac_device: three kernels, asynchronous on `stream` (NULL = the HIP null stream); it
 * takes no context lock and uses no context workspace, it only binds the context's device;
 * nothing is allocated and nothing returns to the host.  FDF_ERR_ARG, synchronously and with
 * nothing launched: n_frames > 65535, a cap of 2^32 - 1 or more, n_hyp outside 1..65536, a coords
 * or model value that is none of the above, a threshold that is negative or not finite; and,
 * unless n_frames == 0 (FDF_OK, nothing written): a NULL required pointer (all but d_keep and
 * d_inliers), matches, coordinates or models that are not 8-byte aligned, a scratch that is not
 * 256-byte aligned or too small.  Whatever the offsets, matches, keep bytes and coordinates hold,
 * no access leaves the buffers; a match's index is checked against the frame's train range
 * before the train coordinates are read.  Offsets that do not ascend give unspecified results.
 *
 * fdf_ransac_points: one pair of host sets (n_q queries with their matches and optional keep
 * bytes, n_t train points), synchronous; inliers_out (n_q bytes) may be NULL.  Copies through
 * device buffers allocated and freed by the call and runs the same kernels; the context's
 * workspace and retained result are untouched, so fdf_fetch_last stays valid.
 */
#define FDF_COORDS_U32 0u   /* fdf_point */
#define FDF_COORDS_F32 1u   /* float x, y */
#define FDF_COORDS_Q11 2u   /* int32 x, y in 1/2048 pixel: fdf_track_device only (rejected here) */
#define FDF_MODEL_AFFINE 0u
#define FDF_MODEL_HOMOGRAPHY 1u
#define FDF_RANSAC_NONE 0xFFFFFFFFu   /* hypothesis of a frame without a model; an idx of no sample */
typedef struct fdf_model {
    double h[9];           /* row-major 3 x 3, h[8] = 1; all zero without a model */
    uint32_t n_corr;       /* M */
    uint32_t n_inliers;
    uint32_t hypothesis;   /* the best hypothesis, or FDF_RANSAC_NONE */
    uint32_t n_valid;      /* valid hypotheses */
} fdf_model;
int fdf_ransac_sample(uint32_t seed, uint32_t frame, uint32_t hypothesis, uint32_t m, uint32_t s,
                      uint32_t idx[4], uint32_t* draws);
int fdf_ransac_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint32_t n_hyp, uint64_t* bytes);
int fdf_ransac_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                      const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                      const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                      const uint64_t* d_t_offsets, uint32_t coords, uint32_t model,
                      uint32_t n_hyp, float threshold, uint32_t seed, fdf_model* d_models,
                      uint8_t* d_inliers, void* d_scratch, uint64_t scratch_bytes, void* stream);
int fdf_ransac_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                      size_t n_t, const fdf_match* matches, const uint8_t* keep, uint32_t coords,
                      uint32_t model, uint32_t n_hyp, float threshold, uint32_t seed,
                      fdf_model* model_out, uint8_t* inliers_out);

/*
 * Least-squares refinement of the models over their inliers (extension: the step after
 * fdf_ransac_device, the refit that estimateAffine2D / findHomography apply to their winner).
 * Like the estimation it is a pure function of its inputs: every floating-point step below is
 * one IEEE binary64 operation rounded once, only + - * / and the absolute value are used, and
 * every sum has one fixed order.
 *
 * Inputs.  The correspondences of frame f, numbered j = 0..M-1, are the RANSAC block's, from the
 * same arrays (matches, keep, capacities, offsets, coordinates, `coords`).  d_models_in[f] is the
 * frame's model, `model` says which kind (s and N as above), `threshold` need not be the one the
 * model was estimated with, n_rounds is 0..8.
 *
 * Per frame.  hypothesis == FDF_RANSAC_NONE: the record is copied unchanged, every inlier byte of
 * the frame is 0 and rounds is 0.  Otherwise the current model is d_models_in[f].h, the current
 * set is the correspondences that the Score rule above makes inliers of it under `threshold`
 * (computed, not read from any bytes) and the current count n is the set's size.  Then n_rounds
 * times:
 *
 *  1. Normalise.  Over the current set: cx = Sx / n and cy = Sy / n with Sx, Sy the sums of x and
 *     of y and n as a double; d = the sum of (|x - cx| + |y - cy|); s = (n + n) / d.  The same
 *     for (u, v) gives cu, cv, e and t = (n + n) / e.  The round fails if n is below the model's
 *     sample size or unless 0 < d < infinity and 0 < e < infinity.  X = (x - cx) * s, Y = (y - cy) * s,
 *     U = (u - cu) * t, V = (v - cv) * t.
 *  2. Normal equations.  A member gives the Fit rule's two rows in normalised coordinates,
 *       r0 = [X, Y, 1, 0, 0, 0, -(U X), -(U Y)],  r1 = [0, 0, 0, X, Y, 1, -(V X), -(V Y)]
 *     (affine: the first six columns).  For i <= j < N, G[i][j] = the sum of
 *     r0[i] * r0[j] + r1[i] * r1[j] and G[j][i] = G[i][j]; g[i] = the sum of
 *     r0[i] * U + r1[i] * V.  A product with a factor that is one of the zeros written above is
 *     not formed and not added (so G[0][0] sums X * X alone, G[0][3] is 0 and g[0] sums X * U); a
 *     factor 1 is exact.  The sign of a zero is free here as everywhere.
 *  3. Order.  Every sum of 1 and 2 is formed like this: correspondence j belongs to lane
 *     j mod 256; a lane starts from +0.0 and adds the terms of its members in increasing j
 *     (sum = sum + term); then the 256 lane sums fold as sum[t] = sum[t] + sum[t + step] for
 *     every t < step, with step = 128, 64, .., 1, and sum[0] is the result.  n is the same sum
 *     of ones (exact).
 *  4. Solve G hn = g by the Fit rule's elimination and back substitution, unchanged: the lowest
 *     row among the largest magnitudes, a NaN never wins, a pivot below 2^-20 fails the round.
 *     hn8 = 1; affine: hn6 = hn7 = 0.
 *  5. Denormalise, H = T2^-1 Hn T1 with T1 = [s 0 -s cx; 0 s -s cy; 0 0 1] and
 *     T2^-1 = [1/t 0 cu; 0 1/t cv; 0 0 1], as this sequence: for each row r = 0, 1, 2 of Hn
 *       a0 = hn[3r] * s,  a1 = hn[3r+1] * s,  a2 = (hn[3r+2] - a0 * cx) - a1 * cy;
 *     with A the three rows (a0, a1, a2), for each column c
 *       H[c] = A[0][c] / t + cu * A[2][c],  H[3+c] = A[1][c] / t + cv * A[2][c],  H[6+c] = A[2][c];
 *     h_k = H[k] / H[8] for k < 8 and h8 = 1.  The round fails unless 2^-20 <= |H[8]| < infinity.
 *     Affine: A's last row is 0 0 1, so h0 = A[0][0] / t, h1 = A[0][1] / t, h2 = A[0][2] / t + cu,
 *     h3 = A[1][0] / t, h4 = A[1][1] / t, h5 = A[1][2] / t + cv, h6 = h7 = 0, h8 = 1, without the
 *     products by zero and without a division by H[8].  Either kind: the round fails if any h_k
 *     is not finite.
 *  6. Re-score all M correspondences under h.  The round is accepted iff it did not fail and the
 *     new count is at least the current one; then h, its set and its count become current.
 *     Otherwise the frame stops and keeps what was current.
 *
 * Output.  d_models_out[f] (d_models_out may be d_models_in) gets the current h, n_corr = M,
 * n_inliers = the current count, and hypothesis and n_valid as they came.  d_inliers (optional,
 * q_cap bytes) follows the RANSAC rule: for every i in [qo[0], min(qo[n_frames], q_cap)) and for
 * no other byte, 1 if i is a correspondence in its frame's current set and 0 otherwise.  d_rounds
 * (optional, n_frames uint32_t) gets the number of accepted rounds.  n_rounds == 0 recounts and
 * rewrites the bytes under `threshold` and leaves h as it came.
 *
 * Example.  The RANSAC example's six pairs and its model 1 0 3 0 1 5 0 0 1, T = 1, one round.
 * The set is pairs 0 1 2 3 5: n = 5, cx = 8, cy = 4.6, d = 53.6, s = 10 / 53.6 =
 * 0.18656716417910446; cu = 11, cv = 9.6, e = 53.6, t = s.  Both kinds of model accept the round
 * (rounds 1) with 5 inliers and the bytes 1 1 1 1 0 1.  Affine: h = 1 0 3 0 1 5 0 0 1 again,
 * exactly.  Homography, the rounding of eight unknowns over five exact pairs:
 *   h0 = 0x1.0000000000001p+0    h1 = -0x1.dc507e631a7ddp-54   h2 = 0x1.7fffffffffffdp+1
 *   h3 = 0x1.886f0037424e0p-54   h4 = 0x1.0000000000000p+0     h5 = 0x1.3ffffffffffffp+2
 *   h6 = 0x1.302010db87537p-57   h7 = -0x1.a85e37930f5e6p-57   h8 = 1
 *
 * fdf_refine_scratch_bytes: host only; the size of fdf_refine_device's d_scratch (256-byte
 * aligned; needs no initialisation and may be reused in stream order): 32 bytes per query index
 * and 4 per frame.  FDF_ERR_ARG: NULL bytes, n_frames > 65535, q_cap of 2^32 - 1 or more.
 *
 * fdf_refine_device: two kernels, asynchronous on `stream` (NULL = the HIP null stream); it takes
 * no context lock and uses no context workspace, it only binds the context's device; nothing is
 * allocated and nothing returns to the host.  FDF_ERR_ARG, synchronously and with nothing
 * launched: n_frames > 65535, a cap of 2^32 - 1 or more, a coords or model value that is none of
 * the above, a threshold that is negative or not finite, n_rounds > 8; and, unless n_frames == 0
 * (FDF_OK, nothing written): a NULL required pointer (all but d_keep, d_inliers and d_rounds),
 * matches, coordinates or models that are not 8-byte aligned, rounds that are not 4-byte aligned,
 * a scratch that is not 256-byte aligned or too small.  The bounds guarantee of
 * fdf_ransac_device holds: whatever the inputs hold, the models included, no access leaves the
 * buffers.
 *
 * fdf_refine_points: one pair of host sets as fdf_ransac_points takes them and the model to
 * refine, synchronous; inliers_out (n_q bytes) and rounds_out may be NULL, model_out may be
 * model_in.  Copies through device buffers allocated and freed by the call and runs the same
 * kernels; the context's workspace and retained result are untouched, so fdf_fetch_last stays
 * valid.
 */
int fdf_refine_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint64_t* bytes);
int fdf_refine_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                      const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                      const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                      const uint64_t* d_t_offsets, uint32_t coords, uint32_t model,
                      const fdf_model* d_models_in, float threshold, uint32_t n_rounds,
                      fdf_model* d_models_out, uint8_t* d_inliers, uint32_t* d_rounds,
                      void* d_scratch, uint64_t scratch_bytes, void* stream);
int fdf_refine_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                      size_t n_t, const fdf_match* matches, const uint8_t* keep, uint32_t coords,
                      uint32_t model, const fdf_model* model_in, float threshold,
                      uint32_t n_rounds, fdf_model* model_out, uint8_t* inliers_out,
                      uint32_t* rounds_out);

/*
 * RANSAC estimation of a fundamental matrix from the matches or tracks (extension: the epipolar
 * outlier test of a camera that moves through a 3-D scene, or of a stereo pair, where no single
 * homography fits; OpenCV's findFundamentalMat with FM_RANSAC, the rejectWithF step of visual-
 * inertial front ends).  The result is F with [u v 1] F [x y 1]^T = 0 for a query (x, y) and its
 * train point (u, v).  Like the block above it is a pure function of its inputs: integer
 * sampling, every floating-point step one IEEE binary64 operation rounded once out of + - * / and
 * the absolute value (never fused), ties by index.
 *
 * Correspondences.  Exactly the RANSAC block's rule on the same arrays (matches, keep,
 * capacities, offsets, coordinates, `coords`), numbered j = 0..M-1; fdf_track_device's d_matches
 * and d_status (as keep) with its float positions go in as they are.
 *
 * Sampling.  The RANSAC block's start state and next(), sample size s = 8, up to 32 draws (16
 * leave most hypotheses of M = 8 or 9 without eight distinct values).  M < 8: no model.
 * (seed 1, f 0, h 0, M 100) gives 54, 11, 77, 18, 0, 8, 14, 35 after 8 draws, (1, 2, 7, 9) gives
 * 1, 0, 8, 4, 2, 7, 6, 3 after 16, (0, 0, 0, 8) gives 5, 2, 4, 6, 7, 1, 0, 3 after 18 and
 * (0, 0, 0, 7) nothing after 32.
 *
 * Fit of a sample, points k = 0..7 in sample order.
 *  1. Normalise.  Sx = the sum of x, from +0.0 in sample order (Sx = Sx + x), Sy likewise;
 *     cx = Sx / 8, cy = Sy / 8; d = the sum, in the same way, of (|x - cx| + |y - cy|);
 *     s = 16 / d.  The same over (u, v) gives cu, cv, e and t = 16 / e.  The hypothesis is
 *     invalid unless 0 < d < infinity and 0 < e < infinity.  X = (x - cx) * s, Y = (y - cy) * s,
 *     U = (u - cu) * t, V = (v - cv) * t.
 *  2. Rows of the 8 x 9 system A fn = 0 for Fn row-major as fn0..fn8:
 *       A[k] = [U X, U Y, U, V X, V Y, V, X, Y, 1]   (each product U * X etc. one operation).
 *  3. Null vector by Gauss-Jordan elimination with full pivoting (no entry is fixed at 1 in
 *     advance: a sideways-moving camera or a rectified pair has f8 = 0 exactly).  8 steps.  A
 *     step's pivot (r, c) is the largest |A[r][c]| over the rows and columns no earlier step
 *     used; ties go to the lowest r, then the lowest c; a NaN magnitude never wins.  The
 *     hypothesis is invalid if that magnitude is below 2^-20 (or none is a number).  Row r and
 *     column c are now used.  For every other row q (the used ones too): m = A[q][c] / A[r][c]
 *     and A[q][j] = A[q][j] - m * A[r][j] for every column j still unused.  After the 8 steps,
 *     with c* the column left unused: fn[c*] = 1, and for each row r with its pivot column c,
 *     fn[c] = -(A[r][c*] / A[r][c]).
 *  4. Denormalise, F = T2^T Fn T1 with T1 = [s 0 -s cx; 0 s -s cy; 0 0 1] and T2 the same of
 *     t, cu, cv, as this sequence.  For each row r = 0, 1, 2 of Fn
 *       a0 = fn[3r] * s,  a1 = fn[3r+1] * s,  a2 = (fn[3r+2] - a0 * cx) - a1 * cy;
 *     with B the three rows (a0, a1, a2), for each column c = 0, 1, 2
 *       g0 = t * B[0][c],  g1 = t * B[1][c],  G[c] = g0,  G[3+c] = g1,
 *       G[6+c] = (B[2][c] - g0 * cu) - g1 * cv.
 *  5. Scale.  With k* the lowest k of the largest |G[k]| (a NaN never wins), f_k = G[k] / G[k*]
 *     for all nine k: the division is by the signed value, so f_k* is exactly +1 and the sign of
 *     F is canonical.  The hypothesis is invalid unless 0 < |G[k*]| < infinity and every f_k is
 *     finite.
 * No rank-2 projection is applied: F is the exact solution of its eight equations, the score
 * below does not need a singular F, and callers that reject outliers do not rely on one.
 *
 * Score.  The Sampson distance without a division, with T = (double)threshold in pixels:
 *   l0 = (f0 x + f1 y) + f2,  l1 = (f3 x + f4 y) + f5,  l2 = (f6 x + f7 y) + f8,
 *   m0 = (f0 u + f3 v) + f6,  m1 = (f1 u + f4 v) + f7,
 *   r = (u l0 + v l1) + l2,  g = ((l0 l0 + l1 l1) + m0 m0) + m1 m1;
 * an inlier iff g > 0 and r r <= (T T) g (both false for a NaN; an infinite coordinate can make
 * both sides infinite, which holds: clear the keep byte of such a point).  A valid hypothesis'
 * count is its number of inliers; the best hypothesis has the largest count, ties go to the
 * lowest h.
 *
 * Output.  As in the RANSAC block, in the same fdf_model record: h = the winner's f0..f8 bit for
 * bit as fitted, n_corr = M, n_inliers, hypothesis, n_valid.  No valid hypothesis (or M < 8): h
 * all zero, n_inliers 0, hypothesis 0xFFFFFFFF.  d_inliers (optional, q_cap bytes) gets, for every
 * i in [qo[0], min(qo[n_frames], q_cap)) and for no other byte, 1 if i is a correspondence and an
 * inlier of its frame's best model and 0 otherwise.
 *
 * Example.  A rectified pair with two bad matches.  Queries (0,0), (80,0), (0,80), (80,80),
 * (40,20), (20,60), (60,40), (30,30), (50,70), (70,10), (10,50), (60,60); train = query +
 * (10,0), (25,0), (31,0), (12,0), (23,0), (37,0), (14,0), (29,0), (3,0), (20,30), (18,0),
 * (40,20); matches[i].index = i, seed 3, one frame, 8 hypotheses, T = 0.5.  Hypothesis 2 wins:
 * 10 inliers, n_valid 8, inlier bytes 1 1 1 1 1 1 1 1 1 0 1 0, counts per hypothesis
 * 8 8 10 9 8 8 8 8, and F is [0 0 0; 0 0 1; 0 -1 0] up to rounding:
 *   f0 = 0x1.2680dad725570p-59    f1 = 0x1.4cc344e4093b5p-57   f2 = -0x1.338fe32749f1dp-52
 *   f3 = -0x1.ff7ec58462d65p-58   f4 = -0x1.768667157b6c1p-59  f5 = 1
 *   f6 = 0x1.2359a7b2aed39p-53    f7 = -0x1.ffffffffffffep-1   f8 = -0x1.b7ffffffffffcp-48
 *
 * fdf_fundamental_sample: host only, no context; the sample of one hypothesis in idx[0..8) and
 * the draws made in *draws (may be NULL).  An invalid hypothesis (m < 8 included) fills idx with
 * 0xFFFFFFFF after its 32 draws.  FDF_ERR_ARG: a NULL idx.  fdf_ransac_sample is unchanged.
 *
 * fdf_fundamental_scratch_bytes: host only; the size of fdf_fundamental_device's d_scratch, which
 * is fdf_ransac_scratch_bytes' with the same errors.
 *
 * fdf_fundamental_device: fdf_ransac_device's arguments without `model`; three kernels,
 * asynchronous on `stream` (NULL = the HIP null stream), no context lock, no context workspace,
 * nothing allocated and nothing returned to the host.  The FDF_ERR_ARG list, the n_frames == 0
 * behaviour and the bounds guarantee are fdf_ransac_device's (FDF_COORDS_Q11 is rejected).
 *
 * fdf_fundamental_check_device: no sampling; d_models_in[f] holds the caller's matrix (a
 * calibrated stereo rig's, or an earlier result to recount under another threshold).  One
 * kernel, no scratch.  Per frame: hypothesis == FDF_RANSAC_NONE: the record is copied unchanged
 * and every inlier byte of the frame is 0.  Otherwise d_models_out[f] (d_models_out may be
 * d_models_in) gets h, hypothesis and n_valid as they came, n_corr = M and n_inliers = the
 * number of correspondences that the Score rule makes inliers of h under `threshold`, and
 * d_inliers (optional) the bytes by the Output rule.  It is the counterpart of
 * fdf_refine_device with n_rounds = 0.  FDF_ERR_ARG: n_frames > 65535, a cap of 2^32 - 1 or more,
 * a coords value that is none of the two, a threshold that is negative or not finite; and,
 * unless n_frames == 0 (FDF_OK, nothing written): a NULL required pointer (all but d_keep and
 * d_inliers), matches, coordinates or models that are not 8-byte aligned.  Whatever the inputs
 * hold, the models included, no access leaves the buffers.
 *
 * fdf_fundamental_points: one pair of host sets as fdf_ransac_points takes them, synchronous;
 * inliers_out (n_q bytes) may be NULL.  Copies through device buffers allocated and freed by the
 * call and runs the same kernels; the context's workspace and retained result are untouched.
 */
int fdf_fundamental_sample(uint32_t seed, uint32_t frame, uint32_t hypothesis, uint32_t m,
                           uint32_t idx[8], uint32_t* draws);
int fdf_fundamental_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint32_t n_hyp,
                                  uint64_t* bytes);
int fdf_fundamental_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                           const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                           const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                           const uint64_t* d_t_offsets, uint32_t coords, uint32_t n_hyp,
                           float threshold, uint32_t seed, fdf_model* d_models,
                           uint8_t* d_inliers, void* d_scratch, uint64_t scratch_bytes,
                           void* stream);
int fdf_fundamental_check_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                                 const uint8_t* d_keep, uint64_t q_cap,
                                 const uint64_t* d_q_offsets, const void* d_q_coords,
                                 const void* d_t_coords, uint64_t t_cap,
                                 const uint64_t* d_t_offsets, uint32_t coords,
                                 const fdf_model* d_models_in, float threshold,
                                 fdf_model* d_models_out, uint8_t* d_inliers, void* stream);
int fdf_fundamental_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                           size_t n_t, const fdf_match* matches, const uint8_t* keep,
                           uint32_t coords, uint32_t n_hyp, float threshold, uint32_t seed,
                           fdf_model* model_out, uint8_t* inliers_out);

/*
 * Exact bilinear resize and the scale pyramid (extension: the reference detects at one scale;
 * ORB-style callers run the chain above over a pyramid, 8 levels at 1.2 by default, each level
 * resized from the one before).  Everything is integer-exact.  These are not OpenCV's bits: its
 * 8-bit path truncates between the two passes; no parity with it is claimed.
 *
 * Taps of one axis.  For a source length S >= 1, a destination length D >= 1 and the destination
 * index i, the centre-aligned source position is N / (2 D) with N = (2 i + 1) S - D, in 64-bit
 * integers (no libm).  N < 0: i0 = 0, q = 0.  Otherwise i0 = N / (2 D), r = N % (2 D) and
 * q = (4096 r + 2 D) / (4 D): the fraction times 2048 rounded half up, 0..2048.  i0 >= S - 1:
 * i0 = S - 2 and q = 2048 (S = 1: i0 = 0, q = 0).  The second tap is i1 = min(i0 + 1, S - 1).
 * One uint32_t per destination index, i0 << 12 | q; S <= 65535.  S = 1920, D = 1600: index 0 is
 * i0 = 0, q = 205 and index 1 is i0 = 1, q = 614.
 *
 * Pixel.  out(x, y) = (sum over a, b in {0, 1} of wy_b * wx_a * I(ix_a, iy_b) + 2^21) >> 22 with
 * w_0 = 2048 - q and w_1 = q of each axis.  The sum is at most 255 * 2^22 < 2^30: one rounding,
 * no intermediate truncation.  So D = S is the identity, S = 2 D is (a + b + c + d + 2) / 4 of
 * each 2 x 2 block and a constant frame stays constant.  Any ratio is legal, upscaling too.
 *
 * Pyramid.  Level 0 is the caller's frames (never copied); for the rational factor num / den > 1
 * (ORB's 1.2 is 6 / 5) w_l = (w_(l-1) * den + num / 2) / num and the same for h: 1920 x 1080 at
 * 6 / 5 gives 1600 x 900, 1333 x 750, 1111 x 625, ...  Level l is resized from level l - 1.  A
 * plan is n_levels (1..32) fdf_pyramid_level entries: the level's size, and for l >= 1 the bytes
 * between its frames (width * height: packed), its 256-byte aligned offset into one pyramid
 * buffer that holds the levels >= 1 of all n_frames frames, and the offsets (in entries) of its
 * x and y taps in one taps array.  Level 0's other fields are 0.  A point of level l maps back
 * per axis by w_0 / w_l: x_0 = (x_l + 0.5) * w_0 / w_l - 0.5.
 *
 * fdf_resize_taps: host only, no context; writes dst_len words.  FDF_ERR_ARG for a NULL
 * pointer, FDF_ERR_SIZE for a zero length or src_len > 65535.
 *
 * fdf_resize_device: asynchronous on `stream` (NULL = the HIP null stream); like
 * fdf_smooth_device it takes no context lock and uses no context workspace, it only binds the
 * context's device; nothing is allocated and nothing returns to the host.  Frames may be any
 * number of bytes apart on either side and have any alignment; the gap bytes of the output are
 * not written; input and output must not overlap.  d_xtaps (dst_w words) and d_ytaps (dst_h
 * words) are device copies of fdf_resize_taps' tables; every entry is clamped on the device
 * before use (i0 <= S - 1, q <= 2048), so whatever the tables hold no access leaves the frames
 * (the values are then unspecified).  FDF_ERR_ARG, synchronously and with nothing launched: a
 * NULL pointer, n_frames > 65535, a frame stride below width * height when n_frames > 1.
 * FDF_ERR_SIZE: a zero dimension, width * height above 2^31 - 256 on either side, a source
 * side above 65535.  n_frames == 0: FDF_OK, nothing written.
 *
 * fdf_pyramid_plan: host only.  Fills levels[0..n_levels); *total_bytes (optional) gets the
 * pyramid buffer's size for n_frames frames, *total_taps (optional) the taps array's entries.
 * FDF_ERR_ARG: num <= den, den == 0, n_levels outside 1..32, n_frames > 65535, a NULL levels.
 * FDF_ERR_SIZE: a zero base dimension or one above 65535, a level with a zero dimension.
 * fdf_pyramid_taps: host only; writes the taps of every level >= 1 of a plan whose level 0 is
 * base_w x base_h (FDF_ERR_ARG if it is not).
 *
 * fdf_pyramid_device: n_levels - 1 launches of the resize kernel in stream order, level 1 from
 * d_frames (frames frame_stride_bytes apart), level l from level l - 1 inside d_pyramid; d_taps
 * holds fdf_pyramid_taps' array.  Asynchronous, as fdf_resize_device; every level is checked
 * before the first launch.  n_levels == 1: FDF_OK, nothing to do.
 *
 * fdf_resize_frame: one host frame (rows stride_bytes apart) to one host frame (rows
 * out_stride_bytes apart), synchronous.  Copies through device buffers allocated and freed by
 * the call and runs the same kernel; the context's workspace and retained result are untouched,
 * so fdf_fetch_last stays valid.
 */
typedef struct fdf_pyramid_level {
    uint32_t width;
    uint32_t height;
    uint64_t frame_stride_bytes;   /* width * height */
    uint64_t offset_bytes;         /* of the level's first frame in the pyramid buffer */
    uint64_t xtaps_offset;         /* entries into the taps array: `width` words */
    uint64_t ytaps_offset;         /* `height` words */
} fdf_pyramid_level;
int fdf_resize_taps(uint32_t src_len, uint32_t dst_len, uint32_t* taps);
int fdf_resize_device(fdf_ctx* ctx, const uint8_t* d_src, uint32_t n_frames, uint32_t src_w,
                      uint32_t src_h, uint64_t src_frame_stride_bytes, uint8_t* d_dst,
                      uint32_t dst_w, uint32_t dst_h, uint64_t dst_frame_stride_bytes,
                      const uint32_t* d_xtaps, const uint32_t* d_ytaps, void* stream);
int fdf_resize_frame(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                     size_t stride_bytes, uint8_t* out, uint32_t dst_w, uint32_t dst_h,
                     size_t out_stride_bytes);
int fdf_pyramid_plan(uint32_t base_w, uint32_t base_h, uint32_t num, uint32_t den,
                     uint32_t n_levels, uint32_t n_frames, fdf_pyramid_level* levels,
                     uint64_t* total_bytes, uint64_t* total_taps);
int fdf_pyramid_taps(const fdf_pyramid_level* levels, uint32_t n_levels, uint32_t base_w,
                     uint32_t base_h, uint32_t* taps);
int fdf_pyramid_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                       uint64_t frame_stride_bytes, const fdf_pyramid_level* levels,
                       uint32_t n_levels, uint8_t* d_pyramid, const uint32_t* d_taps,
                       void* stream);

/*
 * Exact bilinear warp of frames by a 3 x 3 model per frame (extension: what callers estimate a
 * model for -- warpAffine / warpPerspective for stabilisation, registration before differencing,
 * mosaicking).  Like the resize it is integer-exact after one fixed sequence of binary64 steps,
 * so a numpy restatement reproduces it bit for bit.  These are not OpenCV's bits.
 *
 * Direction.  The model maps a destination pixel to a source position (inverse mapping).  That
 * is what fdf_ransac_device / fdf_refine_device produce for query frame A and train frame B:
 * warping B with the model as estimated gives B registered onto A, nothing is inverted.  "Frame
 * f against frame f + 1 of one batch" is d_src = frames + stride, n_frames = F - 1.
 *
 * Models.  Frame f's nine doubles h0..h8 (row-major) are the first 72 bytes at d_models + f *
 * model_stride_bytes; the array is 8-byte aligned and the stride a multiple of 8 and at least 72:
 * 88 is an fdf_model array as the estimator leaves it, 72 is packed matrices.  h8 is used as
 * given, not assumed to be 1; an affine model needs no special path (h6 = h7 = 0).
 *
 * Position of destination pixel (x, y), x in [0, dst_w), y in [0, dst_h), both converted to
 * double; each step is one IEEE binary64 operation, never fused:
 *   P = (h0 x + h1 y) + h2,  Q = (h3 x + h4 y) + h5,  w = (h6 x + h7 y) + h8,
 *   sx = P / w,  sy = Q / w,
 *   FX = floor(sx * 2048.0 + 0.5),  FY = floor(sy * 2048.0 + 0.5).
 * The pixel is valid iff w > 0 and -2^30 <= FX <= 2^30 and -2^30 <= FY <= 2^30 (every comparison
 * is false for a NaN).  For a valid pixel X = (int32)FX, ix = X >> 11 (arithmetic shift) and
 * qx = X & 2047, the same for y; the four taps are (ix + a, iy + b) with a, b in {0, 1} and the
 * weights w_0 = 2048 - q, w_1 = q of each axis.
 *
 * Pixel.  A valid pixel is out = (sum over a, b of wy_b * wx_a * T(ix + a, iy + b) + 2^21) >> 22,
 * the resize rule's sum (below 2^30, one rounding).  T is set by `border`:
 *   FDF_BORDER_REPLICATE: T(cx, cy) = I(clamp(cx, 0, W - 1), clamp(cy, 0, H - 1)), the border of
 *     every other stage;
 *   FDF_BORDER_CONSTANT: a tap outside the frame has the value `fill` (0..255).
 * An invalid pixel is `fill` in both modes: a frame whose model is all zero (no model,
 * hypothesis == FDF_RANSAC_NONE) or holds NaNs comes out as a constant `fill` frame.
 *
 * Mask (optional d_mask, laid out like d_dst).  The byte is 1 iff the pixel is valid and
 * 0 <= X <= (W - 1) * 2048 and 0 <= Y <= (H - 1) * 2048 (the position lies inside the source
 * frame), and 0 otherwise.
 *
 * So the identity model is a copy, an integer translation is an exact shift,
 * h = 1 0 0.5 0 1 0 0 0 1 gives (I(x) + I(x + 1) + 1) >> 1 and a constant frame stays constant
 * under replicate.
 *
 * Example.  The 4 x 4 source I(x, y) = 16 (4 y + x), h = 0.75 0.25 0.5 -0.25 0.75 1 0.0625 0 1,
 * a 4 x 4 destination, constant border, fill 255: the rows are 72 64 57 51 / 124 113 103 94 /
 * 176 162 149 138 / 223 211 196 182 and the mask is all ones except the first byte of the last
 * row.
 *
 * fdf_warp_device: asynchronous on `stream` (NULL = the HIP null stream); like fdf_resize_device
 * it takes no context lock and uses no context workspace, it only binds the context's device;
 * nothing is allocated and nothing returns to the host.  Frames may be any number of bytes apart
 * on either side and have any alignment; the mask's frames lie dst_frame_stride_bytes apart too;
 * gap bytes are never written; source and destination must not overlap.  Whatever the models
 * hold (NaN, infinities, 1e300) no access leaves the frames: tap indices are clamped before use
 * and pixel accesses go through buffer resources of exactly a frame's bytes.  FDF_ERR_ARG,
 * synchronously and with nothing launched: n_frames > 65535, a frame stride below width * height
 * when n_frames > 1, a model stride below 72 or no multiple of 8, border > 1, fill > 255; and,
 * unless n_frames == 0 (FDF_OK, nothing written): a NULL pointer (all but d_mask), models that
 * are not 8-byte aligned.  FDF_ERR_SIZE: a zero dimension, width * height above 2^31 - 256 on
 * either side, a source side above 65535.
 *
 * fdf_warp_frame: one host frame (rows stride_bytes apart) to one host frame and an optional
 * mask (rows out_stride_bytes apart, both), synchronous.  Copies through device buffers allocated
 * and freed by the call and runs the same kernel; the context's workspace and retained result
 * are untouched, so fdf_fetch_last stays valid.
 *
 * fdf_model_invert: host only, no context; the model that warps the other way (A onto B): the
 * adjugate normalised to out[8] = 1, one fixed sequence with each step rounded once:
 *   c0 = h4 h8 - h5 h7,  c1 = h2 h7 - h1 h8,  c2 = h1 h5 - h2 h4,
 *   c3 = h5 h6 - h3 h8,  c4 = h0 h8 - h2 h6,  c5 = h2 h3 - h0 h5,
 *   c6 = h3 h7 - h4 h6,  c7 = h1 h6 - h0 h7,  c8 = h0 h4 - h1 h3,
 *   out_k = c_k / c8 for k < 8,  out_8 = 1.
 * FDF_ERR_ARG, with `out` untouched: a NULL pointer, or an out_k that is not finite (a singular
 * matrix).  `out` may be `h`.
 */
#define FDF_BORDER_REPLICATE 0u
#define FDF_BORDER_CONSTANT 1u
int fdf_warp_device(fdf_ctx* ctx, const uint8_t* d_src, uint32_t n_frames, uint32_t src_w,
                    uint32_t src_h, uint64_t src_frame_stride_bytes, const void* d_models,
                    uint64_t model_stride_bytes, uint8_t* d_dst, uint32_t dst_w, uint32_t dst_h,
                    uint64_t dst_frame_stride_bytes, uint32_t border, uint32_t fill,
                    uint8_t* d_mask, void* stream);
int fdf_warp_frame(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                   size_t stride_bytes, const double h[9], uint8_t* out, uint32_t dst_w,
                   uint32_t dst_h, size_t out_stride_bytes, uint32_t border, uint32_t fill,
                   uint8_t* out_mask);
int fdf_model_invert(const double h[9], double out[9]);

/*
 * Pyramidal Lucas-Kanade tracking of keypoints from one frame into another (extension: the
 * FAST + KLT front end, OpenCV's calcOpticalFlowPyrLK, with an integer contract).  Corners are
 * detected once and then followed from frame to frame at sub-pixel precision, without
 * descriptors.  Positions are held in 1/2048 pixel -- "Q11" below is an int32 in that unit -- so
 * every sum of an iteration is an integer sum, exact in any order, and only a 2 x 2 solve is
 * floating point: a short fixed sequence of unfused binary64 operations.  A numpy restatement
 * reproduces every output bit for bit.  These are not OpenCV's bits.
 *
 * Frames and levels.  `levels` is a host array of n_levels (1..32) fdf_pyramid_level entries, as
 * fdf_pyramid_device takes them.  Level 0 is the caller's frames, frame_stride_bytes apart;
 * levels >= 1 live in a pyramid buffer.  The previous and the next set each have a frames
 * pointer, a pyramid pointer and a first-frame index: frame f of the call (f < n_frames) reads
 * previous frame prev_first + f and next frame next_first + f, where
 *   level 0 of frame k is at d_frames + k * frame_stride_bytes,
 *   level l >= 1 of frame k at d_pyramid + levels[l].offset_bytes + k * levels[l].frame_stride_bytes.
 * Tracking every frame of a batch of F into the next one passes the same frames and pyramid
 * twice with prev_first = 0, next_first = 1, n_frames = F - 1 (a pointer shift cannot say this:
 * the levels have different strides).  The caller guarantees that both sets hold frames up to
 * first + n_frames.  With n_levels == 1 the pyramid pointers may be NULL.  Any ratio between the
 * levels is legal; 2 : 1 is the usual choice for tracking.
 *
 * Points.  Indexing as in fdf_orient_device: frame f owns [offs[f], min(offs[f+1], cap)).
 * `coords` is FDF_COORDS_U32 (an fdf_point, X0 = 2048 x) or FDF_COORDS_Q11 (two int32, x then y,
 * as this stage writes them, so that a caller chains f -> f+1 -> f+2 at sub-pixel positions).
 * Optional d_keep (cap bytes): 0 skips the point.  Optional d_guess (cap x two int32, Q11): the
 * starting position in the next frame at level 0; NULL means the point's own position.  A point
 * is skipped if its keep byte is 0 or if its position or its guess lies outside
 * [0, (w0 - 1) * 2048] x [0, (h0 - 1) * 2048]; it gets reason 0 and the lost outputs below, and no
 * frame byte is read for it.
 *
 * Sample.  For a frame of W x H and a Q11 position (X, Y): ix = X >> 11, qx = X & 2047 (the same
 * for y), w_0 = 2048 - q, w_1 = q, and
 *   S(X, Y) = (sum over a, b in {0, 1} of wy_b * wx_a *
 *              I(clamp(ix + a, 0, W - 1), clamp(iy + b, 0, H - 1)) + 2^16) >> 17,
 * the resize's sum rounded once to 5 fractional bits: 0..8160.
 *
 * Level maps (int64, `/` is floor division), also exported as host-only functions:
 *   map_pos(X, len0, lenl)  = clamp(((X + 1024) * lenl * 2 + len0) / (2 * len0) - 1024,
 *                                   0, (lenl - 1) * 2048)       level 0 directly to level l
 *   map_disp(D, from, to)   = (2 * D * to + from) / (2 * from)  the floor for negative D too
 * map_pos(29372, 32, 16) = 14174, map_disp(-3001, 16, 32) = -6002, map_disp(-3001, 32, 16) =
 * -1500, map_disp(5, 6, 5) = 4.  fdf_track_map_position / fdf_track_map_displacement: lengths
 * 1..65535 and |v| <= 2^28 (so 2 v len stays within int64), a non-NULL `out`; else FDF_ERR_ARG.
 *
 * Per point.  r = radius (1..15), n = (2 r + 1)^2, tau = ((double)min_eig * (double)n) * 1048576.0
 * (min_eig, a finite float >= 0: the smallest eigenvalue of the window's mean gradient matrix a
 * level must have, in grey levels^2 per pixel^2; 1048576 = (32 * 32)^2, the sample's and the
 * Scharr weights' gain squared).  The displacement starts at the coarsest level as
 * D = map_disp(guess - X0, len0, len_{L-1}) per axis, 0 without a guess.  Levels are visited from
 * l = L - 1 down to 0; before every level but the first, D = map_disp(D, len_{l+1}, len_l) per
 * axis.  At each level:
 *   1. Template.  (Xp, Yp) = map_pos of the level-0 position.  P(i, j) = S_prev(Xp + 2048 i,
 *      Yp + 2048 j) for |i|, |j| <= r + 1: one pair of fractional weights serves the whole patch.
 *      Scharr gradients for |i|, |j| <= r:
 *        Gx(i, j) = 3 (P(i+1, j-1) - P(i-1, j-1)) + 10 (P(i+1, j) - P(i-1, j))
 *                 + 3 (P(i+1, j+1) - P(i-1, j+1)),  Gy the transpose of that;  |G| <= 130560.
 *      A11 = sum Gx^2, A12 = sum Gx Gy, A22 = sum Gy^2 in int64: below 2^44, exact as the doubles
 *      a11, a12, a22.
 *   2. Usable level.  p = a11 - tau, q = a22 - tau; the level is usable iff p + q > 0 and
 *      p * q - a12 * a12 > 0 (each step one binary64 operation; both eigenvalues of A exceed tau,
 *      without a square root).  A level >= 1 that is not usable is skipped with D unchanged; if
 *      level 0 is not usable the point is lost with reason 2.  det = a11 * a22 - a12 * a12 is > 0
 *      whenever the test passes: then p, q > 0, so a11 >= p and a22 >= q, rounded products and
 *      differences are monotone, and det >= p * q - a12 * a12 > 0.
 *   3. Start.  (Xn, Yn) = (Xp, Yp) + D; outside [0, (W_l - 1) * 2048] x [0, (H_l - 1) * 2048] the
 *      point is lost with reason 3.
 *   4. Iterate, at most max_iters (1..64) times per level:
 *        J(i, j) = S_next(Xn + 2048 i, Yn + 2048 j), E = J - P, |i|, |j| <= r;
 *        b1 = sum E Gx, b2 = sum E Gy in int64 (|b| < 2^41, exact as doubles);
 *        dx = (a12 * b2 - a22 * b1) / det,  dy = (a12 * b1 - a11 * b2) / det;
 *        FDX = floor(dx * 65536.0 + 0.5), FDY the same (65536 = 32, the sample's fractional
 *        bits, * 2048; the Scharr gain cancels);
 *        unless |FDX| <= 2^20 and |FDY| <= 2^20 (false for a NaN) the point is lost, reason 4;
 *        Xn += FDX, Yn += FDY; outside the level the point is lost with reason 3;
 *        the level stops once |FDX| + |FDY| <= eps after the update (eps: Q11 units, 20 is about
 *        0.01 pixel).  A level that uses all its iterations is not an error.
 *      An iteration counts once its b1 and b2 are summed, whatever follows.
 *   5. Carry.  D = (Xn, Yn) - (Xp, Yp).
 * After level 0 the point is tracked with reason 1 and err = sum |S_next(Xn + 2048 i, Yn + 2048 j)
 * - P(i, j)| over the window at the final position (one more sampling pass, <= 961 * 8160).
 *
 * Outputs.  Entries at index >= min(offs[n_frames], cap) are never written.  All but d_next_q11
 * and d_status are optional.
 *   output                          tracked point                    lost or skipped point
 *   d_next_q11 (2 x int32)          (Xn, Yn)                         (-1, -1): an invalid input,
 *                                                                    a chained call skips it
 *   d_next_f32 (2 x float, the      (float)((double)Xn / 2048.0),    -1.0f, -1.0f
 *     layout of FDF_COORDS_F32)     the same for y
 *   d_status (u8)                   1                                0
 *   d_err (u32)                     err                              0xFFFFFFFF
 *   d_info (u32)                    reason | iterations << 8, the iterations summed over all levels
 *   d_matches (fdf_match)           {i, min(err / n, 0xFFFE), 0xFFFF} {FDF_MATCH_NONE, 0xFFFF, 0xFFFF}
 * Reasons: 0 skipped, 1 tracked, 2 level-0 eigenvalue test, 3 left the frame, 4 step too large.
 *
 * Into the estimator.  d_matches, the point offsets as both query and train offsets, d_status as
 * d_keep and d_next_f32 as the FDF_COORDS_F32 train coordinates go into fdf_ransac_device as they
 * are; the query side then needs an FDF_COORDS_F32 copy of the points (one format serves both
 * sides of that call).  With FDF_COORDS_U32 points on both sides instead, a second array of
 * rounded next positions is the caller's to make.
 *
 * Example.  32 x 24 frames, A(x, y) = min(255, ((x-16)^2 + 2 (y-12)^2 + (x-16)(y-12)) >> 2) and
 * B(x, y) = A(clamp(x - 2), clamp(y - 1)); the point (14, 10), r = 3, max_iters 30, eps 20,
 * min_eig 0.25, one level: A11 = 184786944, A12 = 270729216, A22 = 533045248, the first
 * b = (-24637440, -41500672), the position after one iteration (33605, 23077) (with max_iters = 1
 * the result, err 1789); the full run ends at (32773, 22529), err 0, 4 iterations.  min_eig = 1.0:
 * lost, reason 2.  Two levels 2 : 1 (16 x 12): (32773, 22530), err 0, 5 iterations.  The Q11
 * start (29372, 21780): one level (33469, 23826), err 0; two levels (33468, 23826), err 2.  A
 * constant frame is lost with reason 2 even at min_eig = 0.
 *
 * fdf_track_device: asynchronous on `stream` (NULL = the HIP null stream); like fdf_orient_device
 * it takes no context lock, uses no workspace and allocates nothing; it only binds the context's
 * device.  Whatever the points, keep bytes and guesses hold, no access leaves the frames' bytes
 * or the other buffers: taps are clamped, positions are checked before use and frames are read
 * through buffer resources of exactly a level's bytes.  FDF_ERR_ARG, synchronously and with
 * nothing launched: radius outside 1..15, max_iters outside 1..64, a negative or non-finite
 * min_eig, a bad `coords`, n_frames > 65535 or a first-frame index above 65535, n_levels outside
 * 1..32, a NULL required pointer or a NULL pyramid with n_levels > 1, misaligned arrays
 * (coordinates, guesses and matches 8 bytes; err and info 4 bytes), d_matches with cap above
 * 2^32 - 2, a frame stride (of any level) below width * height when more than one frame is
 * addressed.  FDF_ERR_SIZE: a zero level dimension, a side above 65535, width * height above
 * 2^31 - 256.  n_frames == 0: FDF_OK, nothing written.
 *
 * fdf_track_frames: two host frames of one size (rows stride_bytes apart) and n_points host
 * points (`coords` as above; `guess` optional).  Builds both pyramids for num / den and n_levels
 * with fdf_pyramid_plan, fdf_pyramid_taps and the resize kernel (num and den are not looked at
 * when n_levels == 1), then tracks; synchronous.  Its buffers are allocated and freed by the
 * call; the context's workspace and retained result are untouched, so fdf_fetch_last stays
 * valid.  out_q11 and out_status are required, the others optional.
 */
int fdf_track_map_position(int64_t x, uint32_t len0, uint32_t len_l, int64_t* out);
int fdf_track_map_displacement(int64_t d, uint32_t len_from, uint32_t len_to, int64_t* out);
int fdf_track_device(fdf_ctx* ctx, const uint8_t* d_prev_frames, const uint8_t* d_prev_pyramid,
                     uint32_t prev_first, const uint8_t* d_next_frames,
                     const uint8_t* d_next_pyramid, uint32_t next_first, uint32_t n_frames,
                     uint64_t frame_stride_bytes, const fdf_pyramid_level* levels,
                     uint32_t n_levels, const void* d_points, uint32_t coords, uint64_t cap,
                     const uint64_t* d_frame_offsets, const uint8_t* d_keep, const int32_t* d_guess,
                     uint32_t radius, uint32_t max_iters, uint32_t eps, float min_eig,
                     int32_t* d_next_q11, float* d_next_f32, uint8_t* d_status, uint32_t* d_err,
                     uint32_t* d_info, fdf_match* d_matches, void* stream);
int fdf_track_frames(fdf_ctx* ctx, const uint8_t* prev, const uint8_t* next, uint32_t width,
                     uint32_t height, size_t stride_bytes, const void* points, uint32_t coords,
                     size_t n_points, const int32_t* guess, uint32_t n_levels, uint32_t num,
                     uint32_t den, uint32_t radius, uint32_t max_iters, uint32_t eps, float min_eig,
                     int32_t* out_q11, float* out_f32, uint8_t* out_status, uint32_t* out_err,
                     uint32_t* out_info);

/*
 * Track-set maintenance between two tracking calls (extension; the reference has no tracks).
 * What a video front end does between "track" and "track again": drop lost and border tracks,
 * keep the older of two tracks that drifted onto one corner, add the strongest fresh corners that
 * no surviving track is near, up to a budget, give them new ids and hand one compact list to the
 * next fdf_track_device call.  All arithmetic is integer; the result is a pure function of the
 * inputs (atomics only count, or claim slots whose order nothing reads).
 *
 * Indexing.  n_frames independent streams (cameras, or the frames of a batch) are updated by one
 * call.  As in fdf_orient_device, stream f owns the tracks [t_offs[f], min(t_offs[f+1], t_cap))
 * and the candidates [c_offs[f], min(c_offs[f+1], c_cap)).  Priorities and d_out_src use the
 * global array indices.
 *
 * Inputs.  Tracks: d_track_q11 (two int32 each, 1/2048 pixel, as fdf_track_device writes
 * d_next_q11), d_track_status (u8, optional: NULL = every track is tracked), d_track_ids and
 * d_track_ages (u32).  Candidates: d_cand_points (fdf_point, in any order) and d_cand_scores
 * (u16), e.g. fdf_detect_device + fdf_score_device of the new frame.  d_next_id (u32 per stream,
 * in and out): the stream's next unused id.  Parameters (fdf_tracks_params): width, height 1..65535
 * (level 0), min_dist 1..255 pixels, margin with 2 * margin < min(width, height) (the tracker's
 * radius + 1 is the usual value), max_tracks >= 1 (per stream), passes 1..32.
 *
 *   1. Alive.  A track is alive iff its status byte is non-zero, margin * 2048 <= X <=
 *      (width - 1 - margin) * 2048 and margin * 2048 <= Y <= (height - 1 - margin) * 2048; a lost
 *      track (-1, -1) fails that by itself.  A candidate is eligible iff margin <= x <= width - 1 -
 *      margin and margin <= y <= height - 1 - margin.
 *   2. Pixel.  A track's pixel is px = (X + 1024) >> 11, py = (Y + 1024) >> 11.  Two points are
 *      near iff dx^2 + dy^2 < min_dist^2 (strict: (3, 4) is not near at min_dist 5, near at 6).
 *   3. Suppression by passes, the same for both lists.  A point is undecided (0), admitted (1) or
 *      rejected (2).  j dominates i iff j is near i, of the same stream and list, and of higher
 *      priority: tracks by larger age, then lower index; candidates by larger score, then lower
 *      index (a total order).  Pass p reads the states of pass p - 1 only: an undecided point
 *      becomes rejected if some dominator was admitted, else admitted if every dominator was
 *      rejected, else stays undecided.  After `passes` passes an undecided point is dropped.  Pass
 *      1 admits exactly the local maxima within min_dist; at convergence the admitted set is the
 *      sequential greedy selection in priority order (OpenCV's minDistance rule).
 *   4. Tracks.  Alive tracks start undecided, all others rejected; the kept survivors are the
 *      tracks admitted after the passes.
 *   5. Candidates.  An eligible candidate near no kept survivor starts undecided, all others
 *      rejected.  After the passes free[f] = max(0, max_tracks - kept[f]); of stream f's admitted
 *      candidates those of rank < free[f] become new tracks, the rank by score descending, ties
 *      to the lower index (fdf_select_device's rule over the whole frame).  max_tracks never
 *      removes a survivor.
 *   6. Output per stream: the kept survivors in track index order (position copied unchanged, id
 *      carried, age min(age + 1, 0xFFFFFFFF)), then the new tracks in candidate index order
 *      (position (x * 2048, y * 2048), age 0, the j-th new track's id next_id[f] + j modulo 2^32);
 *      next_id[f] then advances by the stream's full count of new tracks.
 *   7. Arrays: d_out_q11, d_out_ids, d_out_ages; optional d_out_src (u32: a survivor's track
 *      index, FDF_TRACKS_NEW | candidate index for a new track).  d_out_offsets (n_frames + 1
 *      entries) is the exclusive prefix of the streams' totals with the full total last, also
 *      beyond out_cap, as fdf_detect_device and fdf_select_device do; entries at or past
 *      min(total, out_cap) are never written.  d_out_q11 with d_out_offsets are FDF_COORDS_Q11
 *      points of fdf_track_device as they are.
 *
 * Example.  32 x 24, min_dist 5, margin 2, max_tracks 4, passes 8, next_id 7.  Tracks (X, Y; id;
 * age; status): 0 (20480, 20480; 3; 5; 1), 1 (15359, 28672; 4; 2; 1), 2 (22528, 20480; 5; 9; 1),
 * 3 (-1, -1; 6; 1; 0).  Pixels (10, 10), (7, 14) (X = 15360 would give 8), (11, 10); track 3 is
 * not alive.  Track 2 is near track 0 and older: pass 1 admits tracks 1 and 2, pass 2 rejects
 * track 0 ((7, 14) is at distance^2 25 of (10, 10): not near).  Candidates (x, y; score):
 * 0 (12, 10; 90) is near survivor 2; 1 (20, 10; 50); 2 (23, 14; 50), at distance^2 25 of
 * candidate 1; 3 (21, 11; 40), dominated by candidate 1; 4 (1, 12; 99), inside the margin;
 * 5 (28, 20; 10).  Admitted: 1, 2, 5; free = 4 - 2 = 2 takes 1 and 2.  Output (X, Y; id; age;
 * src): (15359, 28672; 4; 3; 1), (22528, 20480; 5; 10; 2), (40960, 20480; 7; 0; 0x80000001),
 * (47104, 28672; 8; 0; 0x80000002); offsets {0, 4}; next_id 9.
 *
 * fdf_tracks_update_device: asynchronous on `stream` (NULL = the HIP null stream); takes no
 * context lock, uses no workspace, allocates nothing; it only binds the context's device.  Its
 * memsets run on the stream.  d_scratch holds fdf_tracks_scratch_bytes(...) bytes, 256-byte
 * aligned.  Whatever the positions, offsets and candidates hold, no access leaves the given
 * arrays: index ranges are clamped to the caps and cell indices to the grid.  FDF_ERR_ARG,
 * synchronously and with nothing launched: a parameter out of range, n_frames > 65535, a cap above
 * 2^32 - 1 (above 2^31 - 1 when d_out_src is given), a NULL required pointer (the track arrays
 * when t_cap > 0, the candidate arrays when c_cap > 0, the output arrays when out_cap > 0, the
 * offsets, d_next_id), misaligned arrays (positions, points and offsets 8 bytes; ids, ages,
 * d_next_id and d_out_src 4; scores 2), scratch NULL, misaligned or too small.  n_frames == 0:
 * FDF_OK, nothing written.
 *
 * fdf_tracks_scratch_bytes: host only (no device).  fdf_tracks_update_points: one stream of host
 * arrays, synchronous; its buffers are allocated and freed by the call, the context's workspace
 * and retained result stay untouched.  *next_id is read and advanced; *n_out is the stream's
 * total; FDF_ERR_CAPACITY when that exceeds `cap` (the first `cap` entries are written).
 */
#define FDF_TRACKS_NEW 0x80000000u
typedef struct fdf_tracks_params {
    uint32_t width, height;   /* level 0 */
    uint32_t min_dist;        /* 1..255 pixels */
    uint32_t margin;          /* 2 * margin < min(width, height) */
    uint32_t max_tracks;      /* >= 1, per stream */
    uint32_t passes;          /* 1..32 */
} fdf_tracks_params;
int fdf_tracks_scratch_bytes(uint32_t n_frames, uint32_t width, uint32_t height,
                             uint32_t min_dist, uint64_t t_cap, uint64_t c_cap, uint64_t* bytes);
int fdf_tracks_update_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_tracks_params* params,
                             const int32_t* d_track_q11, const uint8_t* d_track_status,
                             const uint32_t* d_track_ids, const uint32_t* d_track_ages,
                             const uint64_t* d_track_offsets, uint64_t t_cap,
                             const fdf_point* d_cand_points, const uint16_t* d_cand_scores,
                             const uint64_t* d_cand_offsets, uint64_t c_cap, uint32_t* d_next_id,
                             int32_t* d_out_q11, uint32_t* d_out_ids, uint32_t* d_out_ages,
                             uint32_t* d_out_src, uint64_t out_cap, uint64_t* d_out_offsets,
                             void* d_scratch, uint64_t scratch_bytes, void* stream);
int fdf_tracks_update_points(fdf_ctx* ctx, const fdf_tracks_params* params,
                             const int32_t* track_q11, const uint8_t* track_status,
                             const uint32_t* track_ids, const uint32_t* track_ages,
                             size_t n_tracks, const fdf_point* cand_points,
                             const uint16_t* cand_scores, size_t n_cands, uint32_t* next_id,
                             int32_t* out_q11, uint32_t* out_ids, uint32_t* out_ages,
                             uint32_t* out_src, size_t cap, size_t* n_out);

/*
 * Streaming host pipeline (extension; the reference's callers detect on one
 * host image at a time, src/lib.rs:62-64, src/main.rs:58-64).  Host frames in, host
 * keypoints out, with the host->device copy of one batch, the detection of another and the
 * device->host copy of a third in flight together.  `depth` (1..16) batch slots, each with
 * pinned host staging for `max_frames` frames of width x height pixels (3 bytes per pixel
 * with FDF_PIPE_RGB, converted on the device as fdf_detect_rgb does), its own device
 * buffers, context and HIP stream.  Device output per slot holds max_points_per_frame points
 * per frame (0 = (width-6) * (height-6), the most a frame can have).
 *
 * Tickets are issued in order; ticket k uses slot k % depth, which must have been
 * collected: fdf_pipeline_acquire returns FDF_ERR_BUSY otherwise.  A pipeline is not
 * thread-safe beyond one producer and one consumer calling under the pipeline's own lock
 * (every call takes it; fdf_pipeline_collect releases it while waiting on the device).
 */
typedef struct fdf_pipeline fdf_pipeline;
enum fdf_pipe_flags {
    FDF_PIPE_RGB = 1,     /* frames are RGB8 (rows of 3 * width bytes) */
    FDF_PIPE_SCORES = 2   /* also compute each keypoint's score (as fdf_detect_scored) */
};
int fdf_pipeline_create(int device, uint32_t width, uint32_t height, uint32_t max_frames,
                        uint32_t depth, uint64_t max_points_per_frame, uint32_t flags,
                        const fdf_config* cfg, fdf_pipeline** out);
void fdf_pipeline_destroy(fdf_pipeline* p);
/* The pinned staging buffer of the next ticket: frame f at *frames + f * frame bytes. */
int fdf_pipeline_acquire(fdf_pipeline* p, uint8_t** frames, uint64_t* ticket);
/* Enqueue an acquired ticket's first n_frames (1..max_frames) frames; returns at once. */
int fdf_pipeline_submit(fdf_pipeline* p, uint64_t ticket, uint32_t n_frames);
/* acquire + copy n_frames frames (frame f at frames + f * frame_stride_bytes, rows packed)
 * into the staging buffer + submit. */
int fdf_pipeline_push(fdf_pipeline* p, const uint8_t* frames, uint32_t n_frames,
                      size_t frame_stride_bytes, uint64_t* ticket);
/*
 * Wait for a submitted ticket and copy out its keypoints (frames concatenated in order, each
 * in raster order), scores (FDF_PIPE_SCORES; `out_scores` may be NULL) and frame_offsets
 * (n_frames + 1 entries; may be NULL).  FDF_ERR_CAPACITY: `cap` is below *n_out; nothing
 * is released, call again with a larger buffer.  FDF_OK releases the slot.  FDF_ERR_DROPPED:
 * the batch had *n_out points but the slot held only the first max_points_per_frame *
 * n_frames of them (those are copied, frame_offsets are exact); the slot is released.
 */
int fdf_pipeline_collect(fdf_pipeline* p, uint64_t ticket, fdf_point* out,
                         uint16_t* out_scores, size_t cap, uint64_t* frame_offsets,
                         size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* FDF_H */
