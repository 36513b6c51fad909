// fdf_ctx.h -- what the host translation units of the C ABI (fdf_api.cpp, fdf_stages.cpp)
// share: the context and the argument checks, all inline (no call across translation units
// on an asynchronous _device entry).  Internal: not part of include/fdf.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/fdf.h"
#include "fdf_kernels.h"

// Result of the last host-API detection on a context (fdf_fetch_last): its points stay in
// d_out, its offsets in d_offsets and its frames in d_in until the next host call.
struct LastResult {
    bool valid = false;
    bool host_out = false;         // the points / offsets are in the host-mapped h_out / h_offs
    uint64_t total = 0;
    uint32_t n_frames = 0, width = 0, height = 0;
    fdf_config cfg{};
    bool rgb = false;              // frames in d_rgb (RGB8); scores need their luma in d_in
    bool in_place = false;         // the frame was read in place from pinned host memory: not
                                   // in d_in, so the result has no scores (fdf_fetch_last)
    // fdf_detect_batch_multi: the call's generation (0: not a multi-context result) and this
    // context's shard of it, checked by fdf_fetch_last_multi
    uint64_t multi_gen = 0;
    uint32_t shard = 0, nshards = 0;
};

struct fdf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // device workspace, grown on demand
    uint8_t* d_in = nullptr;            size_t in_bytes = 0;       // host-API frame staging
    uint8_t* d_rgb = nullptr;           size_t rgb_bytes = 0;      // host-API RGB staging
    uint2* d_out = nullptr;             size_t out_points = 0;     // host-API output
    uint64_t* d_offsets = nullptr;      size_t offsets_n = 0;      // host-API frame offsets
    // host-API output in pinned, device-mapped host memory: the detector (direct output) or
    // the compaction writes the points and offsets there over PCIe, so a host call needs no
    // copy kernel, no device-to-host copy and one synchronisation (hd_*: device addresses)
    uint2* h_out = nullptr;             uint2* hd_out = nullptr;   size_t h_out_points = 0;
    uint64_t* h_offs = nullptr;         uint64_t* hd_offs = nullptr;   size_t h_offs_n = 0;
    // fdf_detect's overlapped upload: the frame goes up in row chunks on copy_stream, each
    // chunk's flag (pinned, device-mapped) set to the call's epoch after its copy, while the
    // detector already runs and each band waits for the chunk of its last row
    hipStream_t copy_stream = nullptr;
    uint32_t* h_flags = nullptr;        // pinned: the epoch each chunk's flag copy carries
    uint32_t* d_flags = nullptr;        // device: the chunk flags the bands poll
    uint32_t chunk_epoch = 0;
    uint32_t chunks = 0;                // upload chunks (0: kChunksDefault; 1: no overlap)
    // host frames that start in pinned memory but run past its mapping (a hipHostRegister'ed
    // range shorter than the frames) are packed into this pinned buffer by the CPU first: the
    // runtime's DMA copy rejects such a source range
    uint8_t* h_stage = nullptr;         uint8_t* hd_stage = nullptr;   size_t h_stage_bytes = 0;
    // recoveries the host entry points made on their own (fdf_ctx_recoveries): a band's wait
    // for its upload chunk ran out and the frame was detected again from one copy; a
    // direct-output look-back ran out and the compaction rebuilt the output from the slots
    uint64_t upload_fallbacks = 0, lookback_recoveries = 0;
    // an asynchronous device call's look-back ran out and a host call found the error word
    // first: kept here and returned by the next fdf_detect_device(_rgb), as fdf.h promises
    bool pending_device_error = false;
    uint16_t* d_scores = nullptr;       size_t scores_n = 0;       // host-API scores
    uint8_t* d_slots = nullptr;         size_t slots_bytes = 0;    // per-band output slots
    uint32_t* d_counts = nullptr;       size_t counts_n = 0;       // per-band keypoint counts
    // compaction bases: two alternating buffers of per-group sums (kept zero between uses)
    // and the keypoint-statistics word, all zeroed once at context creation
    uint32_t* d_sums = nullptr;         // 2 x fdfk::kMaxGroupSums, then 4 words
    int sums_parity = 0;
    bool sums_dirty = false;            // a launch failed: re-zero before the next use
    // NMS keypoint density feedback (band height): the compaction writes the last finished
    // launch's pre-NMS keypoint total to host-mapped memory, tagged with its launch number
    uint64_t* h_stats = nullptr;        // pinned, mapped; *h_stats = seq << 32 | total;
                                        // h_stats[1]: the direct output's look-back error word
    uint64_t* d_stats = nullptr;        // its device address
    uint32_t stats_seq = 0;
    struct LaunchInfo { uint32_t seq = 0, t = 0, n = 0, nms = 0, w = 0; double pixels = 0; };
    LaunchInfo hist[64];
    // the last density read, kept for its configuration: with more launches in flight than
    // `hist` holds, a read finds its launch's record overwritten (the band height then
    // alternated between launches of one configuration)
    // (one per NMS mode, so that interleaved modes keep theirs)
    LaunchInfo known[3];
    double known_density[3] = {0.0, 0.0, 0.0};
    // cross-stream ordering: the device work of the last enqueue (on any stream) completes
    // at `done`; the next enqueue on another stream waits for it first
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool done_valid = false;
    // the last enqueue's work is on done_stream but `done` is not recorded after it yet: on
    // the context's own stream and the null stream (streams that outlive every call) the
    // record waits until something needs it (another stream's call, a host wait), so a
    // stream of back-to-back calls enqueues one packet per call, not two
    bool done_pending = false;
    // the last enqueue's compaction, relaunched when the host output has to grow
    fdfk::CompactParams last_compact{};
    LastResult last;
    // grid size that counts as filling the chip (fdf_ctx_set_geometry; 0 = kDefaultMinTasks)
    uint64_t min_tasks = 0;
    uint32_t band_rows = 0;              // fdf_ctx_set_band_rows (0 = automatic)
    // optional per-kernel timing (fdf_ctx_set_timing): every `timing`-th call (0: off) records
    // its kernels' durations
    uint32_t timing = 0;
    uint64_t timing_calls = 0;            // calls since timing was enabled
    size_t timed = 0;                     // calls recorded since timing was enabled
    std::vector<hipEvent_t> ev;           // 4 per recorded call, kMaxTimedCalls at most
    std::vector<uint8_t> timed_compact;   // per recorded call: 1 if it launched the compaction
    // direct output of small grids (BandParams::direct): look-back descriptors, launch tag
    uint64_t* d_lookback = nullptr;       size_t lookback_n = 0;
    // band tickets: the device counter (a spare word of d_sums, zeroed with it) has handed out
    // ticket_next tickets, ntasks per direct launch
    uint32_t ticket_next = 0;
    uint32_t cus = 0;                     // compute units of the device
    // workgroups per CU of a detector instance (sweep_occupancy), by configuration
    struct Occupancy { uint32_t nms, n, lds; bool rgb; uint32_t wg; };
    std::vector<Occupancy> occupancy;
    // debug builds (FDF_STAMPS set): the last detector launch's workgroup stamps
    uint64_t* d_stamps = nullptr;         size_t stamps_n = 0;
    uint64_t stamps_used = 0;             // words written by the last launch
};

// Internal linkage: nothing of this header shows up among the library's symbols.
namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline int check_config(const fdf_config* cfg) {
    if (!cfg) return FDF_ERR_ARG;
    if (cfg->count < 9 || cfg->count > 16) return FDF_ERR_COUNT;
    if (cfg->nms > FDF_NMS_SUM_ABSOLUTE) return FDF_ERR_NMS;
    return FDF_OK;
}

// Shape rules derived from the reference's u32 arithmetic (SURVEY.md §7 "Errors").
inline int check_shape(uint32_t w, uint32_t h, int* empty) {
    *empty = 0;
    if (h < 3) return FDF_ERR_SIZE;        // height - 3 underflows (src/fast_simd.rs:342)
    if (h <= 6) { *empty = 1; return FDF_OK; }
    if (w < 6) return FDF_ERR_SIZE;        // width - 3 - 3 underflows (:369)
    if (w == 6) { *empty = 1; return FDF_OK; }
    return FDF_OK;
}

inline uint64_t align256(uint64_t v) { return (v + 255u) & ~255ull; }

// Frames of a _device entry lie `stride_bytes` apart; a single frame's stride is not looked at.
inline uint64_t frame_stride(uint32_t n_frames, uint64_t stride_bytes, uint64_t frame_bytes) {
    return n_frames > 1 ? stride_bytes : frame_bytes;
}

inline int status_of(hipError_t e) { return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE; }

// `rows` host rows of `row_bytes` bytes, `stride_bytes` apart, to a packed device buffer (one
// plain copy when the host rows are packed too), and the way back.
inline hipError_t upload_rows(void* dst, const void* src, size_t stride_bytes, size_t row_bytes,
                              size_t rows, hipStream_t stream) {
    return stride_bytes == row_bytes
               ? hipMemcpyAsync(dst, src, row_bytes * rows, hipMemcpyHostToDevice, stream)
               : hipMemcpy2DAsync(dst, row_bytes, src, stride_bytes, row_bytes, rows,
                                  hipMemcpyHostToDevice, stream);
}
inline hipError_t download_rows(void* dst, size_t stride_bytes, const void* src, size_t row_bytes,
                                size_t rows, hipStream_t stream) {
    return stride_bytes == row_bytes
               ? hipMemcpyAsync(dst, src, row_bytes * rows, hipMemcpyDeviceToHost, stream)
               : hipMemcpy2DAsync(dst, stride_bytes, src, row_bytes, row_bytes, rows,
                                  hipMemcpyDeviceToHost, stream);
}

}  // namespace
