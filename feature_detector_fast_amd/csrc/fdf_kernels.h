// fdf_kernels.h -- shared between the HIP kernels (fdf_sweep.hip, fdf_kernels.hip,
// fdf_select.hip, fdf_orient.hip, fdf_harris.hip, fdf_describe.hip, fdf_match.hip, fdf_ransac.hip) and the C-ABI host layer (fdf_api.cpp,
// fdf_stages.cpp): geometry constants, LDS layout and launch parameters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdfk {

constexpr int kNmsOff = 0;
constexpr int kNmsMaxThreshold = 1;
constexpr int kNmsSumAbsolute = 2;

constexpr int kThreads = 256;                 // 4 waves of 64 lanes
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxLds = 64 * 1024;       // default dynamic-LDS limit per workgroup
constexpr int kCompactTasks = 256;            // tasks per workgroup of the compaction kernel

// Internal ablation switches (BandParams::flags), set from the FDF_DEBUG_FLAGS environment
// variable by the host layer of the debug build only (make debug -> libfdf_debug.so, built
// with -DFDF_DEBUG_BUILD); never part of the C ABI.  Results are wrong when set.  In the
// production build the kernels see the constant 0 and the ablation branches compile away.
constexpr uint32_t kFlagNoFullTest = 1;   // candidates are never tested (no keypoints)
constexpr uint32_t kFlagNoEmit = 2;       // bands write no slot contents (counts only)
constexpr uint32_t kFlagNoPrefilter = 4;  // no units are swept (slots and compaction only)
constexpr uint32_t kFlagNoLoad = 8;       // rows are streamed and compared, no candidates
constexpr uint32_t kFlagNoNms = 16;       // NMS modes: every keypoint is kept (no band NMS pass)
constexpr uint32_t kFlagNmsPrefixOnly = 32;  // band NMS pass: rank prefixes only (timing)
constexpr uint32_t kFlagNoEval = 64;       // batches are issued (FIFO, staging, loads), never tested
#ifdef FDF_DEBUG_BUILD
__host__ __device__ inline uint32_t ablation_flags(uint32_t f) { return f; }
constexpr bool kDebugBuild = true;
#else
__host__ __device__ inline uint32_t ablation_flags(uint32_t) { return 0u; }
constexpr bool kDebugBuild = false;
#endif
// Debug builds: per-workgroup stamps of the detector (BandParams::stamps, kStampWords words per
// workgroup): shader clock and 100 MHz real time at the workgroup's start and end, its XCD
// and hardware id, its band, and the shader clock at the end of its phases as wave 0 sees
// them (setup, its sweep, NMS, look-back), and the low 32 bits of the shader clock at each
// wave's sweep end.  Written only to that buffer; no output depends on them.
constexpr uint32_t kStampWords = 12;

// Column-sweep kernel (fdf_sweep.hip).  Lane l of a wave owns kLaneCols columns; a strip is
// 62 lanes wide (lanes 0 and 63 are halo lanes).
constexpr int kLaneCols = 16;
constexpr int kStripCols = 62 * kLaneCols;
constexpr int kSweepPixelQ = 256;             // candidate pixel FIFO per wave (power of two)
constexpr uint32_t kSweepMaxLds = 160 * 1024; // gfx950 LDS per CU (and per workgroup)

// A full-test batch is issued every kSweepIssue rows once 64 candidates are queued and is
// evaluated the same number of rows later (one batch in flight per wave).
constexpr int kSweepIssue = 3;
// Pixel-row register ring of the sweep (rows in flight = kSweepRing - 4); unit sweeps are
// whole multiples of kSweepRing steps.
constexpr int kSweepRing = 8;
// Waves per SIMD of the sweep kernel (register budget 512 / kSweepWavesPerEU VGPRs).
constexpr int kSweepWavesPerEU = 4;

// Rows of keypoint bitmap above and below a band: NMS compares a band's edge rows with the
// neighbouring bands' rows, so the band also tests one row each side (scores only).
__host__ __device__ inline uint32_t band_halo(uint32_t nms) { return nms ? 1u : 0u; }

// LDS of one workgroup: the keypoint bitmap of the band's R rows plus the NMS halo rows (the
// spill and dense NMS tiers then clear the suppressed keypoints in place; one pad word after
// the bitmap lets bit look-ups read two words unconditionally), 4 candidate FIFOs (+ batch
// staging), and for NMS the band's keypoint scores: a list of kScoreListCap (position, score)
// entries and per-row / per-4-word-block keypoint counts that turn a bitmap position into its
// raster rank.  The FIFOs, staging and score list are contiguous: once the sweep is done they
// hold the scores in rank order (`nms_area`, u16 entries).  band_nms_lds (at most
// kScoreListCap keypoints) ranks into the FIFO part alone and keeps, at `stage`, one kill bit
// per rank: 64 kill words in wave 0's staging area (stage + 0 .. 255) and their 64 exclusive
// popcount prefixes in wave 1's (stage + 256 .. 511); the band's points are then written from
// the list, each at its rank less the kills below it.
constexpr uint32_t kScoreListCap = 2048;
constexpr uint32_t kRankBlock = 4;            // bitmap words per rank-prefix block
// band_nms_lds ranks the list's scores as u16 into the 4 candidate FIFOs
static_assert(kScoreListCap * 2 <= 4 * kSweepPixelQ * 4, "ranked scores must fit the FIFO area");
static_assert(kScoreListCap % 256 == 0, "the spill NMS pass holds the list 1/256 per thread");
static_assert(kScoreListCap < 4096, "the LDS NMS pass keeps rank + 1 in a list entry's 12 score bits");
struct SweepLayout {
    uint32_t pq, wave_bytes, stage, bitmap, slist, bprefix, rprefix, misc, total;
    uint32_t seltab;             // during the sweep: the 256-entry set-bit table (1 KB) in
                                 // the rank-prefix area, which NMS uses only after the sweep
    uint32_t nms_area_entries;   // u16 ranked scores that fit [pq, bprefix) after the sweep
};

__host__ __device__ inline uint32_t align16(uint32_t v);

__host__ __device__ inline SweepLayout make_sweep_layout(uint32_t R, uint32_t nw, uint32_t nms) {
    SweepLayout L;
    const uint32_t rows = R + 2 * band_halo(nms);
    const uint32_t nb = (nw + kRankBlock - 1) / kRankBlock;
    L.bitmap = 0;
    L.pq = align16(rows * nw * 4 + 4);
    L.wave_bytes = kSweepPixelQ * 4;              // 4 FIFOs = kScoreListCap u16 ranked scores
    L.stage = L.pq + 4 * L.wave_bytes;            // 4 x 64 staged batch pixels
    L.slist = L.stage + 4 * 64 * 4;
    const uint32_t cap = nms ? kScoreListCap : 0u;
    L.bprefix = L.slist + cap * 4;
    L.nms_area_entries = (L.bprefix - L.pq) / 2;
    L.rprefix = L.bprefix + (nms ? align16(rows * nb * 2) : 0u);
    L.seltab = L.bprefix;
    const uint32_t prefix_end = L.rprefix + (nms ? align16(rows * 4) : 0u);
    L.misc = prefix_end > L.seltab + 1024u ? prefix_end : L.seltab + 1024u;
    L.total = L.misc + 64;
    return L;
}

// Words per bitmap row: ceil(W / 32) rounded up to a multiple of 4, so that every row of a
// band's bitmap (LDS, and a slot holding it) starts 16-byte aligned and the emit reads 4
// words of one row per lane (the pad words stay zero).
__host__ __device__ inline uint32_t bitmap_words_per_row(uint32_t W) {
    return ((W + 31) / 32 + 3) & ~3u;
}

// Sweep steps of a unit of `rows` owned rows plus `halo` extra tested rows, in whole
// kSweepRing-step blocks (the 3 rows of vertical look-ahead are a prologue, not steps).
__host__ __device__ inline uint32_t sweep_steps(uint32_t rows, uint32_t halo) {
    return (rows + halo + kSweepRing - 1) / kSweepRing * kSweepRing;
}

__host__ __device__ inline uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

__host__ __device__ inline uint32_t score_bytes_for(uint32_t nms) {
    return nms == kNmsOff ? 0u : (nms == kNmsMaxThreshold ? 1u : 2u);
}

// Per-band output slot: the band's points (8 B each) when they fit, else its keep-bitmap.
__host__ __device__ inline uint32_t slot_bytes_for(uint32_t R, uint32_t nw) {
    const uint32_t b = align16(R * nw * 4);
    return b < 256 ? 256 : b;
}

// Bands per compaction workgroup: enough groups (~1024) to spread the copy over the chip.
__host__ __device__ inline uint32_t compact_tasks_per_group(uint32_t ntasks) {
    const uint32_t t = ntasks / 1024;
    return t < 1 ? 1u : (t > (uint32_t)kCompactTasks ? (uint32_t)kCompactTasks : t);
}
// Per-group keypoint sums the detector accumulates (one atomic add per band) so that a
// compaction group finds its output base by summing the groups before it, O(groups) instead
// of O(tasks).  Two buffers alternate between launches: a launch reads one and its
// compaction zeroes the other for the next launch.
constexpr uint32_t kMaxGroupSums = 2048;
struct CompactParams {
    uint32_t width, height, rows, bands_per_frame, ntasks, words_per_row, slot_bytes;
    uint32_t tasks_per_group;        // compact_tasks_per_group(ntasks)
    const uint8_t* slots;
    const uint32_t* counts;
    uint2* out;
    uint64_t cap;
    uint64_t* frame_offsets;         // frames + 1 entries
    const uint32_t* group_sums;      // per-group sums of this launch (NULL: sum the counts)
    uint32_t* next_sums;             // zeroed here for the next launch (kMaxGroupSums entries)
    uint32_t* kp_stats;              // NMS: the detector's keypoint total (read and reset here)
    uint64_t* stats_out;             // host-mapped: stats_seq << 32 | that total
    uint32_t stats_seq;
};

struct BandParams {
    const uint8_t* frames;       // frame f at frames + f * frame_stride, rows packed (stride = width)
    uint64_t frame_stride;
    uint32_t width, height;
    uint32_t rows;               // centre rows per band (R)
    uint32_t bands_per_frame;
    uint32_t ntasks;             // frames * bands_per_frame == grid size
    uint32_t words_per_row;      // bitmap_words_per_row(width)
    uint32_t threshold;
    uint32_t slot_bytes;
    uint8_t* slots;              // ntasks * slot_bytes
    uint32_t* counts;            // ntasks keypoint counts (band order = raster order)
    uint32_t flags;              // kFlag* ablation switches, 0 in production
    uint32_t nstrips, nsub;      // sweep kernel: column strips x sub-bands per band
    uint32_t* group_sums;        // += band count at [task / tasks_per_group] (NULL: none)
    uint32_t tasks_per_group;
    uint32_t* kp_stats;          // NMS: += each band's keypoints before suppression (NULL: off)
    uint64_t* stamps;            // debug builds: kStampWords per workgroup (NULL: off)
    // Direct output (small grids, every workgroup resident at once): each band finds its
    // output position by a decoupled look-back over the bands before it and writes its points
    // to `out` itself; no compaction launch.  The band slots are still written (a host call
    // whose output has to grow runs compact_kernel from them).
    uint32_t direct;             // 1: direct output
    uint32_t epoch;              // this launch's tag in the look-back descriptors
    uint64_t* lookback;          // ntasks descriptors: epoch << 32 | kLbAggregate / kLbPrefix | value
    uint2* out;                  // direct: the caller's points, `cap` of them
    uint64_t cap;
    uint64_t* frame_offsets;     // direct: frames + 1 entries
    // Direct output: a workgroup's band is its ticket (a device counter taken when it starts,
    // less this launch's first ticket), so bands are swept in the order workgroups start and
    // a band's look-back only ever waits on bands that started before it -- no residency
    // assumption.  Each launch takes exactly ntasks tickets; the host keeps the running base.
    uint32_t* ticket;
    uint32_t ticket_base;
    // Direct output: set when a look-back wait ran out (host-mapped; the band then publishes
    // no prefix and writes no points, and the host recovers from the slots: fdf_api.cpp)
    uint32_t* lookback_error;
    // Host frames arriving in row chunks while the kernel runs (fdf_detect's overlapped
    // upload; NULL: the frames are in place): chunk c = rows [c * chunk_rows, (c+1) *
    // chunk_rows) has landed once chunk_flags[c] == chunk_epoch (device words a 4-byte copy
    // on the copy stream writes after each chunk's copy, in order).  A band waits for the
    // chunk of the last row it reads before its first load; a wait that runs out sets
    // lookback_error.
    const uint32_t* chunk_flags;
    uint32_t chunk_rows;
    uint32_t chunk_epoch;
};
constexpr uint64_t kLbAggregate = 1ull << 30;   // value = the band's own keypoint count
constexpr uint64_t kLbPrefix = 1ull << 31;      // value = keypoints of bands 0 .. this one
constexpr uint64_t kLbValue = kLbAggregate - 1;
constexpr uint64_t kLbNoBase = ~0ull;           // band_lookback's result after a timeout
// Direct output pays off when the whole grid is resident at once (a band's look-back then
// waits only for bands running beside it): up to this many workgroups, within the CU count
// times the workgroups one CU holds by the kernel's occupancy (host side, fdf_api.cpp).
constexpr uint32_t kDirectMaxTasks = 1024;

// start / stop (optional): events the dispatch itself timestamps (hipExtLaunchKernelGGL), so
// per-kernel timing adds no packets between the kernels
hipError_t launch_compact(const CompactParams& c, hipStream_t stream, hipEvent_t start = nullptr,
                          hipEvent_t stop = nullptr);
hipError_t launch_sweep(const BandParams& p, uint32_t nms, uint32_t n, hipStream_t stream,
                        hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same detector whose units leave their last 8-step block at their last row
// (fdf_sweep_latency.hip): for grids of short units (a single frame's latency bands)
hipError_t launch_sweep_latency(const BandParams& p, uint32_t nms, uint32_t n, hipStream_t stream,
                                hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// Workgroups of the detector instance (nms, n; grey or RGB) one CU holds at once with
// `lds_bytes` of dynamic LDS (the runtime's occupancy calculator: registers, LDS, waves).
hipError_t sweep_occupancy(uint32_t nms, uint32_t n, uint32_t lds_bytes, bool rgb, int* wg_per_cu);
hipError_t sweep_occupancy_rgb(uint32_t nms, uint32_t n, uint32_t lds_bytes, int* wg_per_cu);
// RGB8 frames (3 bytes per pixel, frame_stride in bytes), luma converted on load
hipError_t launch_sweep_rgb(const BandParams& p, uint32_t nms, uint32_t n, hipStream_t stream,
                            hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t launch_rgb_to_luma(const uint8_t* rgb, uint32_t n_frames, uint32_t pixels,
                              uint64_t rgb_frame_stride, uint8_t* grey, hipStream_t stream);
hipError_t launch_score_rings(const uint8_t* centers, const uint8_t* rings, uint32_t nrings,
                              uint32_t nms, uint32_t t, uint32_t n, uint16_t* out,
                              hipStream_t stream);
hipError_t launch_score_points(const uint8_t* img, uint32_t width, const uint2* pts,
                               uint32_t npts, uint32_t nms, uint32_t t, uint32_t n,
                               uint16_t* out, hipStream_t stream);
hipError_t launch_score_frames(const uint8_t* frames, uint32_t width, uint64_t frame_stride,
                               uint32_t n_frames, const uint2* pts, const uint64_t* offsets,
                               uint64_t cap, uint32_t blocks_per_frame, uint32_t nms,
                               uint32_t t, uint32_t n, uint16_t* out, hipStream_t stream);

// Best-K selection per grid cell (fdf_select.hip; fdf_select_device).
constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelCells = 16;                 // cells of a row handled at once (16 KB of LDS)
constexpr uint32_t kSelMaxRows = 1u << 23;    // cell rows (grid.x): rows * 256 threads < 2^32
struct SelectParams {
    const uint2* pts;            // `cap` points, frames concatenated, each in raster order
    const uint16_t* scores;      // `cap` scores
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    uint32_t n_frames;
    uint32_t cw, ch;             // cell size in pixels (>= 1)
    uint32_t cells_x, rows;      // cells per cell row, cell rows per frame
    uint32_t k;
    uint8_t* keep;               // `cap` flags (the caller's, or in the scratch)
    uint64_t* frame_tot;         // scratch: n_frames kept totals, zero before the launch
    uint32_t* row_cnt;           // scratch: kept points per (frame, cell row)
    uint64_t* row_range;         // scratch: [lo, hi) index range per (frame, cell row)
    uint2* sel;
    uint16_t* sel_scores;
    uint64_t sel_cap;
    uint64_t* sel_offs;          // n_frames + 1 entries
};
// select, scan and scatter kernels on `stream` (frame_tot already zeroed there)
hipError_t launch_select(const SelectParams& p, hipStream_t stream);

// Intensity-centroid orientation (fdf_orient.hip; fdf_orient_device).
constexpr int kOrientThreads = 256;
constexpr uint32_t kOrientMaxRadius = 31;             // window of 2 r + 1 <= 64 bytes
constexpr uint64_t kOrientMaxPixels = 0x7fffff00ull;  // byte offsets of a frame fit an int
// launch_orient, launch_harris, launch_describe, launch_smooth: grid.y = n_frames, a frame an int can index
inline bool frames_fit_launch(uint32_t n_frames, uint32_t width, uint32_t height) {
    return n_frames <= 65535u && width != 0 && height != 0 &&
           (uint64_t)width * height <= kOrientMaxPixels;
}
struct OrientParams {
    const uint8_t* frames;       // frame f at frames + f * frame_stride, width * height bytes
    uint64_t frame_stride;
    const uint2* pts;            // `cap` points, frames concatenated
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    uint32_t n_frames, width, height, radius;
    float* angles;               // `cap` entries
    int32_t* moments;            // 2 * `cap` entries (m10, m01), or NULL
    uint8_t u[kOrientMaxRadius + 1];   // half-widths u[0..radius] of the disc (fdf_orient_disc)
};
// one kernel on `stream`: `chunks` workgroups per frame share the frame's points
hipError_t launch_orient(const OrientParams& p, uint32_t chunks, hipStream_t stream);

// Harris corner response of keypoints (fdf_harris.hip; fdf_harris_device).
constexpr int kHarrisThreads = 256;
constexpr uint32_t kHarrisMaxK = 255;                 // k_num <= 255, 1 <= k_den <= 255
inline bool harris_block_ok(uint32_t block) { return block == 3 || block == 5 || block == 7; }
// The u16 rank score of a response: 0 for R <= 0, R itself below 1024, else a "6.10
// minifloat" of e = floor(log2 R): (e - 9) << 10 | the 10 bits below R's leading one.
// Monotone non-decreasing in R and continuous at 1023 -> 1024; 55295 at R = 2^63 - 1.
__host__ __device__ inline uint16_t harris_code(int64_t R) {
    if (R <= 0) return 0;
    const int e = 63 - __builtin_clzll((unsigned long long)R);
    if (e < 10) return (uint16_t)R;
    return (uint16_t)(((uint32_t)(e - 9) << 10) | ((uint32_t)(R >> (e - 10)) & 1023u));
}
struct HarrisParams {
    const uint8_t* frames;       // frame f at frames + f * frame_stride, width * height bytes
    uint64_t frame_stride;
    const uint2* pts;            // `cap` points, frames concatenated
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    uint32_t n_frames, width, height;
    uint32_t block;              // 3, 5 or 7
    uint32_t k_num, k_den;       // the Harris constant k_num / k_den
    uint16_t* scores;            // `cap` rank scores
    int64_t* responses;          // `cap` exact responses, or NULL
};
// one kernel on `stream`: `chunks` workgroups per frame share the frame's points
hipError_t launch_harris(const HarrisParams& p, uint32_t chunks, hipStream_t stream);

// Steered BRIEF descriptors and 5x5 box smoothing (fdf_describe.hip; fdf_describe_device,
// fdf_smooth_device).
constexpr int kDescribeThreads = 256;                 // 4 waves, one keypoint each per pass
constexpr uint32_t kBriefTests = 256;
constexpr uint32_t kBriefBytes = kBriefTests / 8;     // descriptor bytes per keypoint
constexpr uint32_t kBriefTableBytes = kBriefTests * 4;   // one bin: (x0, y0, x1, y1) int8 per test
constexpr uint32_t kBriefMaxBins = 360;
struct DescribeParams {
    const uint8_t* frames;       // frame f at frames + f * frame_stride, width * height bytes
    uint64_t frame_stride;
    const uint2* pts;            // `cap` points, frames concatenated
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    uint32_t n_frames, width, height;
    const float* angles;         // `cap` entries, or NULL (bin 0)
    const int8_t* table;         // n_bins * kBriefTableBytes (fdf_brief_steer)
    uint32_t n_bins;
    float scale;                 // (float)(n_bins / (2 pi))
    uint8_t* desc;               // `cap` * kBriefBytes
};
// one kernel on `stream`: `chunks` workgroups per frame share the frame's points
hipError_t launch_describe(const DescribeParams& p, uint32_t chunks, hipStream_t stream);

constexpr int kSmoothThreads = 256;
constexpr uint32_t kSmoothMinWidth = 8;              // narrower frames: a thread per pixel
// Rows a thread walks when the grid is large enough (4 halo rows are read per strip).
constexpr uint32_t kSmoothStripRows = 64;
struct SmoothParams {
    const uint8_t* frames;       // frame f at frames + f * frame_stride, width * height bytes
    uint64_t frame_stride;
    uint8_t* out;                // frame f at out + f * out_stride
    uint64_t out_stride;
    uint32_t n_frames, width, height;
    uint32_t groups;             // ceil(width / 4): a thread owns 4 columns
    uint32_t strip_rows, strips; // rows a thread walks; strips = ceil(height / strip_rows)
};
hipError_t launch_smooth(const SmoothParams& p, hipStream_t stream);

// Exact bilinear resize (fdf_resize.hip; fdf_resize_device, fdf_pyramid_device).
constexpr int kResizeThreads = 256;
constexpr uint32_t kResizeOne = 2048;                // a weight of 1: taps hold frac * 2048
constexpr uint32_t kResizeShift = 22;                // two weights of 11 bits
constexpr uint32_t kResizeHalf = 1u << (kResizeShift - 1);
constexpr uint32_t kResizeMaxSide = 65535;           // a tap word's index: i0 << 12 | q
constexpr uint32_t kResizeMinSrcWidth = 8;           // the strip kernel loads 8 bytes of a row
constexpr uint32_t kResizeStripRows = 64;            // rows a thread walks when the grid is large
struct ResizeParams {
    const uint8_t* src;          // frame f at src + f * src_stride, src_w * src_h bytes
    uint64_t src_stride;
    uint8_t* dst;                // frame f at dst + f * dst_stride, dst_w * dst_h bytes
    uint64_t dst_stride;
    const uint32_t* xtaps;       // dst_w words (fdf_resize_taps), clamped on the device
    const uint32_t* ytaps;       // dst_h words
    uint32_t n_frames, src_w, src_h, dst_w, dst_h;
    uint32_t groups;             // ceil(dst_w / 4): a thread owns 4 destination columns
    uint32_t strip_rows, strips; // rows a thread walks; strips = ceil(dst_h / strip_rows)
};
// The strip kernel's shapes: a horizontal ratio of at most 2 (every other shape: a thread per
// pixel, the same integers).
bool resize_fast_path(uint32_t src_w, uint32_t dst_w);
hipError_t launch_resize(const ResizeParams& p, hipStream_t stream);

// Exact bilinear warp by a 3 x 3 model per frame (fdf_warp.hip; fdf_warp_device).  The weights,
// the rounding and the side limit are the resize's (kResizeOne, kResizeShift, kResizeMaxSide).
constexpr int kWarpThreads = 256;
constexpr uint32_t kWarpTileRows = 4;                          // destination rows a wave covers
constexpr uint32_t kWarpReplicate = 0, kWarpConstant = 1;     // FDF_BORDER_*
constexpr uint64_t kWarpModelBytes = 72;                      // nine doubles
struct WarpParams {
    const uint8_t* src;          // frame f at src + f * src_stride, src_w * src_h bytes
    uint64_t src_stride;
    uint8_t* dst;                // frame f at dst + f * dst_stride, dst_w * dst_h bytes
    uint8_t* mask;               // laid out like dst, or NULL
    uint64_t dst_stride;
    const void* models;          // frame f's nine doubles at models + f * model_stride, 8-byte aligned
    uint64_t model_stride;       // a multiple of 8, at least kWarpModelBytes
    uint32_t n_frames, src_w, src_h, dst_w, dst_h;
    uint32_t border, fill;       // kWarpReplicate / kWarpConstant; fill 0..255
    uint32_t groups;             // ceil(dst_w / 4): a thread owns 4 destination columns of a row
};
// one kernel on `stream`: destination widths below 4 run a thread per pixel (the same integers)
hipError_t launch_warp(const WarpParams& p, hipStream_t stream);

// Pyramidal Lucas-Kanade tracking of keypoints (fdf_track.hip; fdf_track_device).  Positions are
// int32 in units of 1 / kResizeOne pixel ("Q11"); the sample keeps 5 fractional bits.
constexpr int kTrackThreads = 256;                    // 4 waves, one point each per pass
constexpr uint32_t kTrackMaxRadius = 15;              // (2 r + 1)^2 <= 16 window pixels per lane
constexpr uint32_t kTrackMaxSlots = 16;
constexpr uint32_t kTrackMaxIters = 64;
constexpr uint32_t kTrackMaxLevels = 32;
constexpr uint32_t kTrackSampleShift = 17;            // two weights of 11 bits less 5 kept bits
constexpr uint32_t kTrackSampleHalf = 1u << (kTrackSampleShift - 1);
constexpr double kTrackStepScale = 65536.0;           // 32 (the sample's bits) * 2048
constexpr double kTrackStepLimit = 0x1p20;            // |FDX|, |FDY| of an accepted step
constexpr uint32_t kTrackU32 = 0, kTrackQ11 = 2;      // FDF_COORDS_U32, FDF_COORDS_Q11
constexpr uint32_t kTrackSkipped = 0, kTrackTracked = 1, kTrackEigen = 2, kTrackLeft = 3,
                   kTrackStep = 4;                    // d_info reasons
constexpr uint32_t kTrackNoErr = 0xffffffffu;

// The level maps of include/fdf.h (all int64; floor division).
__host__ __device__ inline int64_t track_floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}
__host__ __device__ inline int64_t track_map_pos(int64_t x, int64_t len0, int64_t lenl) {
    const int64_t v = track_floor_div((x + 1024) * lenl * 2 + len0, 2 * len0) - 1024;
    const int64_t hi = (lenl - 1) * (int64_t)kResizeOne;
    return v < 0 ? 0 : v > hi ? hi : v;
}
__host__ __device__ inline int64_t track_map_disp(int64_t d, int64_t from, int64_t to) {
    return track_floor_div(2 * d * to + from, 2 * from);
}

struct TrackLevel {
    const uint8_t* prev;         // the level of the call's frame 0 in the previous set
    const uint8_t* next;         // ... in the next set
    uint64_t prev_stride;        // bytes between the level's frames
    uint64_t next_stride;
    uint32_t width, height;
};
struct TrackParams {
    TrackLevel levels[kTrackMaxLevels];
    uint32_t n_levels, n_frames;
    const void* pts;             // `cap` points: 2 x u32 pixels (kTrackU32) or 2 x int32 Q11
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    const uint8_t* keep;         // `cap` flags, or NULL: all ones
    const int2* guess;           // `cap` Q11 starting positions in the next frame, or NULL
    uint32_t coords, radius, max_iters, eps;
    double tau;                  // (min_eig * n) * 2^20
    int2* next_q11;              // `cap`
    float2* next_f32;            // `cap`, or NULL
    uint8_t* status;             // `cap`
    uint32_t* err;               // `cap`, or NULL
    uint32_t* info;              // `cap`, or NULL
    uint2* matches;              // `cap` fdf_match, or NULL
};
// one kernel on `stream`: `chunks` workgroups per frame share the frame's points
hipError_t launch_track(const TrackParams& p, uint32_t chunks, hipStream_t stream);

// Track-set maintenance between two tracking calls (fdf_tracks.hip; fdf_tracks_update_device):
// prune, min-distance suppression by passes, refill from the candidates, ids and ages.
constexpr int kTracksThreads = 256;
constexpr int kTracksWaves = kTracksThreads / 64;
constexpr uint32_t kTracksMinCell = 8;                // cell side = max(min_dist, kTracksMinCell)
constexpr uint32_t kTracksMaxDist = 255;
constexpr uint32_t kTracksMaxPasses = 32;
constexpr uint32_t kTracksMaxSide = 65535;            // a pixel coordinate is a u16
constexpr uint64_t kTracksMaxCap = 0xffffffffull;     // an entry holds its index as a u32
constexpr uint32_t kTracksNewBit = 0x80000000u;       // d_out_src of a new track
constexpr uint8_t kTracksUndecided = 0, kTracksAdmitted = 1, kTracksRejected = 2;

// One list (tracks or candidates) of a call.  `ent`, `st[0..1]` are cell-sorted: stream f's
// binned points are [lo, lo + start[f * (cells + 1) + cells]) with lo the stream's first index;
// `flag` is by original index.
struct TracksList {
    const uint64_t* offs;        // n_frames + 1 entries
    uint64_t cap;
    uint32_t* cursor;            // n_frames * cells, zero before the count
    uint32_t* start;             // n_frames * (cells + 1): a cell's first entry, relative to lo
    uint4* ent;                  // cap entries {x | y << 16, priority key, original index, cell}
    uint8_t* st[2];              // cap states each, read and written alternately
    uint8_t* flag;               // cap: 1 = in the output, zero before the call's kernels
    uint32_t chunks;             // workgroups per stream of the kernels that walk the list
};
struct TracksParams {
    uint32_t n_frames, width, height, min_dist, margin, max_tracks, passes;
    uint32_t cell, cells_x, cells_y;
    const int2* t_q11;
    const uint8_t* t_status;     // or NULL
    const uint32_t* t_ids;
    const uint32_t* t_ages;
    const uint2* c_pts;
    const uint16_t* c_scores;
    TracksList t, c;
    uint32_t* next_id;           // n_frames, in and out
    uint32_t* kept;              // n_frames each: kept survivors, new tracks, the ids' base
    uint32_t* n_new;
    uint32_t* id_base;
    uint64_t* tot;               // n_frames: kept + new
    int2* out_q11;
    uint32_t* out_ids;
    uint32_t* out_ages;
    uint32_t* out_src;           // or NULL
    uint64_t out_cap;
    uint64_t* out_offs;          // n_frames + 1
};
// all kernels of one update on `stream` (the cursors and flags are zeroed by the caller)
hipError_t launch_tracks_update(const TracksParams& p, hipStream_t stream);

// Brute-force Hamming matching of the 256-bit descriptors (fdf_match.hip; fdf_match_device,
// fdf_match_filter_device).
constexpr int kMatchThreads = 256;                    // queries of a workgroup pass
constexpr uint32_t kMatchTile = 256;                  // train descriptors of an LDS tile
constexpr uint32_t kMatchNone = 0xffffffffu;          // FDF_MATCH_NONE
constexpr uint32_t kMatchNoDistance = 0xffffu;        // FDF_MATCH_NO_DISTANCE
constexpr uint64_t kMatchMaxCap = 0xfffffffeull;      // indices are u32 and kMatchNone is none
struct MatchParams {
    const uint8_t* q_desc;       // `q_cap` * kBriefBytes, 4-byte aligned
    const uint2* q_pts;          // `q_cap` points, or NULL with t_pts: no window
    const uint64_t* q_offs;      // n_frames + 1 entries
    uint64_t q_cap;
    const uint8_t* t_desc;       // `t_cap` * kBriefBytes, 4-byte aligned
    const uint2* t_pts;          // `t_cap` points, each frame's y non-decreasing
    const uint64_t* t_offs;      // n_frames + 1 entries
    uint64_t t_cap;
    uint32_t n_frames, max_dx, max_dy;
    uint2* matches;              // `q_cap` fdf_match: .x = index, .y = distance | second << 16
};
// one kernel on `stream`: `chunks` workgroups per frame share the frame's queries
hipError_t launch_match(const MatchParams& p, uint32_t chunks, hipStream_t stream);
struct MatchFilterParams {
    const uint2* matches;        // `q_cap` fdf_match
    const uint64_t* q_offs;      // n_frames + 1 entries
    uint64_t q_cap;
    const uint2* reverse;        // `t_cap` fdf_match, or NULL: no cross-check
    uint64_t t_cap;
    uint32_t n_frames, max_distance, ratio_num, ratio_den;
    uint8_t* keep;               // `q_cap` flags
};
hipError_t launch_match_filter(const MatchFilterParams& p, hipStream_t stream);

// RANSAC affine / homography estimation from matches (fdf_ransac.hip; fdf_ransac_device).
constexpr int kRansacThreads = 64;                    // hypotheses of a workgroup: one wave
constexpr int kRansacFrameThreads = 256;              // compaction and finalisation: a workgroup per frame
constexpr uint32_t kRansacTile = 256;                 // correspondences of an LDS tile (8 KB)
constexpr int kRansacWideWaves = 8;                   // waves that share a block's scoring in a small grid
constexpr uint32_t kRansacWideMaxBlocks = 128;        // ... one of at most this many blocks: 1024 waves
constexpr uint32_t kRansacMaxHyp = 65536;
constexpr uint32_t kRansacMaxDraws = 16;              // draws a sample of 3 or 4 may take
constexpr uint32_t kFundamentalMaxDraws = 32;         // ... and a sample of 8 (fdf_fundamental_device)
constexpr uint32_t kRansacInvalid = 0xffffffffu;      // count of an invalid hypothesis; no best one
constexpr uint32_t kRansacAffine = 0, kRansacHomography = 1;   // FDF_MODEL_*
constexpr uint32_t kRansacU32 = 0, kRansacF32 = 1;             // FDF_COORDS_*

// The sampling of include/fdf.h: the start state of (seed, frame, hypothesis) and the sample.
__host__ __device__ inline uint32_t ransac_start_state(uint32_t seed, uint32_t frame, uint32_t hyp) {
    uint32_t st = seed + 0x9E3779B9u * (frame + 1u) + 0x85EBCA6Bu * (hyp + 1u);
    st ^= st >> 16;
    st *= 0x85EBCA6Bu;
    st ^= st >> 13;
    st *= 0xC2B2AE35u;
    st ^= st >> 16;
    return st ? st : 0x9E3779B9u;
}
// The first S distinct draws in idx[0..S) and true, or kRansacInvalid in all of idx and false after
// kDraws draws; *draws
// (optional) gets the draws made.  Every index is a compile-time one: idx stays in registers.
template <int S, uint32_t kDraws = kRansacMaxDraws>
__host__ __device__ inline bool ransac_sample(uint32_t seed, uint32_t frame, uint32_t hyp,
                                              uint32_t m, uint32_t (&idx)[S], uint32_t* draws) {
    uint32_t st = ransac_start_state(seed, frame, hyp);
    int n = 0;
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < S; ++k) idx[k] = kRansacInvalid;
    while (d < kDraws && n < S) {
        st ^= st << 13;
        st ^= st >> 17;
        st ^= st << 5;
        ++d;
        const uint32_t j = (uint32_t)(((uint64_t)st * m) >> 32);
        bool fresh = true;
#pragma unroll
        for (int k = 0; k < S; ++k) fresh = fresh && !(k < n && idx[k] == j);
#pragma unroll
        for (int k = 0; k < S; ++k) idx[k] = (fresh && k == n) ? j : idx[k];
        n += fresh ? 1 : 0;
    }
    if (draws) *draws = d;
#pragma unroll
    for (int k = 0; k < S; ++k) idx[k] = n == S ? idx[k] : kRansacInvalid;
    return n == S;
}

struct RansacParams {
    const uint2* matches;        // `q_cap` fdf_match
    const uint8_t* keep;         // `q_cap` flags, or NULL: all ones
    const uint64_t* q_offs;      // n_frames + 1 entries
    uint64_t q_cap;
    const uint2* q_coords;       // `q_cap` points: 2 x u32 or 2 x f32 (the bits)
    const uint2* t_coords;       // `t_cap` points
    const uint64_t* t_offs;      // n_frames + 1 entries
    uint64_t t_cap;
    uint32_t n_frames, coords, model, n_hyp, seed;
    double tt;                   // the threshold as a double, squared
    double* models;              // n_frames fdf_model (11 x 8 bytes each)
    uint8_t* inliers;            // `q_cap` flags, or NULL
    double* corr;                // scratch: 4 doubles x, y, u, v per query index; frame f's
                                 // correspondences packed from its first index on
    uint32_t* n_corr;            // scratch: n_frames correspondence counts
    uint32_t* counts;            // scratch: n_frames x n_hyp inlier counts (kRansacInvalid: none)
};
// compaction, hypothesis and finalisation kernels on `stream`
hipError_t launch_ransac(const RansacParams& p, hipStream_t stream);
// the compaction kernel alone (n_frames > 0): corr and n_corr from the correspondence arrays
hipError_t launch_ransac_compact(const RansacParams& p, hipStream_t stream);

// RANSAC fundamental-matrix estimation (fdf_fundamental.hip; fdf_fundamental_device): `model` is
// unused, everything else is as above.
constexpr int kFundamentalSample = 8;
// compaction (fdf_ransac.hip's), hypothesis and finalisation kernels on `stream`
hipError_t launch_fundamental(const RansacParams& p, hipStream_t stream);
struct FundamentalCheckParams {
    RansacParams r;              // the correspondence arrays; tt; models: the output (may be
                                 // models_in); inliers; no scratch
    const double* models_in;     // n_frames fdf_model
};
// one kernel on `stream`: the caller's matrices recounted (fdf_fundamental_check_device)
hipError_t launch_fundamental_check(const FundamentalCheckParams& p, hipStream_t stream);

// Least-squares refinement of the models over their inliers (fdf_ransac.hip; fdf_refine_device).
constexpr uint32_t kRefineMaxRounds = 8;
struct RefineParams {
    RansacParams r;              // the correspondences; tt: the refinement's threshold; models:
                                 // the output (may be models_in); inliers; corr and n_corr: this
                                 // stage's scratch; n_hyp, seed and counts are unused
    const double* models_in;     // n_frames fdf_model
    uint32_t* rounds;            // n_frames accepted rounds, or NULL
    uint32_t n_rounds;           // 0..kRefineMaxRounds
};
// compaction and refinement kernels on `stream`
hipError_t launch_refine(const RefineParams& p, hipStream_t stream);

}  // namespace fdfk
