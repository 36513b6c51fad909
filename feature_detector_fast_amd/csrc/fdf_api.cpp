// fdf_api.cpp -- the C ABI of include/fdf.h on top of the HIP kernels: contexts, detection,
// scoring, fetch, rings and multi-device calls (the stages behind the detector: fdf_stages.cpp).
//
// Replaces fast_simd::detector (iwanders/feature_detector_fast src/fast_simd.rs:847-859):
// validation mirrors the reference's panics (:302-305, :342, :369, :800) as status codes,
// the device work is the fused band kernel (fdf_kernels.hip), and the host side only moves
// bytes and picks the band height.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include <new>

#include "../../include/fdf.h"
#include "fdf_ctx.h"
#include "fdf_geometry.h"

constexpr size_t kMaxTimedCalls = 4096;
constexpr uint64_t kDefaultMinTasks = 1024;   // 4 workgroups on each of 256 CUs
constexpr uint32_t kMaxBandRows = 256;        // fdf_ctx_set_band_rows: the automatic path's range
constexpr uint32_t kMaxChunks = 16;           // overlapped upload: chunks at most
// Default 1 (no overlap): each chunk's ready flag costs a copy on the copy stream, which this
// runtime runs as a blit kernel (~4 us plus ~9 us of queue gap, profiles/r04/t7_*): 1080p
// max-t pinned measured p50 0.0787 / 0.0999 / 0.1406 / 0.2196 ms at 1 / 2 / 4 / 8 chunks.
constexpr uint32_t kChunksDefault = 1;
constexpr size_t kChunkMinBytes = 1u << 18;   // frames below 256 KB upload in one copy

// process-wide counters: fdf_detect_batch_multi call generations, direct-output launch tags
std::atomic<uint64_t> g_multi_gen{0};
std::atomic<uint32_t> g_launch_epoch{0};

namespace {

// `done` covers the last enqueue's work (recorded now if that was deferred).
hipError_t record_done(fdf_ctx* ctx) {
    if (!ctx->done_valid || !ctx->done_pending) return hipSuccess;
    ctx->done_pending = false;
    return hipEventRecord(ctx->done, ctx->done_stream);
}

// After enqueueing the context's work on `stream`: `done` is to follow it, now or (streams
// that outlive every call: the context's own, the null stream) when first needed.
hipError_t note_done(fdf_ctx* ctx, hipStream_t stream) {
    ctx->done_stream = stream;
    ctx->done_valid = true;
    ctx->done_pending = true;
    if (stream == ctx->stream || stream == nullptr) return hipSuccess;
    return record_done(ctx);
}

// The device work of the last enqueue (whatever stream it ran on) has finished.
void wait_done(fdf_ctx* ctx) {
    if (!ctx->done_valid) return;
    const hipError_t e = record_done(ctx) == hipSuccess ? hipEventSynchronize(ctx->done)
                                                        : hipStreamSynchronize(ctx->done_stream);
    if (e == hipSuccess) ctx->done_valid = false;    // nothing of the context is outstanding
}

// hipStreamSynchronize of the context's own stream; when the last enqueue ran there, nothing
// of the context is outstanding afterwards (the next wait_done returns at once: a host call's
// completion event is never recorded and waited on after the fact)
hipError_t sync_own_stream(fdf_ctx* ctx) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && ctx->done_valid && ctx->done_stream == ctx->stream) {
        ctx->done_valid = false;
        ctx->done_pending = false;
    }
    return e;
}

// Grow a workspace buffer to `need` elements (+1/8 headroom).  The old buffer may still be
// read by work on another stream, so everything the context enqueued is drained first.
template <typename T>
int ensure(fdf_ctx* ctx, T** buf, size_t* have, size_t need, hipStream_t stream) {
    if (*have >= need) return FDF_OK;
    if (*buf) {
        wait_done(ctx);
        (void)hipStreamSynchronize(stream);
        (void)hipFree(*buf);
        *buf = nullptr;
        *have = 0;
    }
    const size_t n = need + need / 8;
    if (hipMalloc(reinterpret_cast<void**>(buf), n * sizeof(T)) != hipSuccess) {
        *buf = nullptr;
        return FDF_ERR_ALLOC;
    }
    *have = n;
    return FDF_OK;
}

// Grow a pinned, device-mapped host buffer to `need` elements (+1/8 headroom); *dev is its
// device address.  Like ensure(), everything the context enqueued is drained first.
template <typename T>
int ensure_host(fdf_ctx* ctx, T** buf, T** dev, size_t* have, size_t need, hipStream_t stream) {
    if (*have >= need) return FDF_OK;
    if (*buf) {
        wait_done(ctx);
        (void)hipStreamSynchronize(stream);
        (void)hipHostFree(*buf);
        *buf = *dev = nullptr;
        *have = 0;
    }
    const size_t n = need + need / 8;
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, n * sizeof(T), hipHostMallocMapped) != hipSuccess) return FDF_ERR_ALLOC;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        (void)hipHostFree(hp);
        return FDF_ERR_ALLOC;
    }
    *buf = static_cast<T*>(hp);
    *dev = static_cast<T*>(dp);
    *have = n;
    return FDF_OK;
}

// The direct output's look-back error word (h_stats[1]): set by a band whose wait ran out.
volatile uint32_t* lookback_error_word(fdf_ctx* ctx) {
    return ctx->h_stats ? reinterpret_cast<volatile uint32_t*>(ctx->h_stats + 1) : nullptr;
}

// Takes (reads and clears) the look-back error word: bit 0 a direct-output band's look-back
// ran out, bit 1 a band's wait for its upload chunk, bit 2 a workgroup's start ticket lay
// past its grid (the device counter and ticket_next disagree: both are reset).
uint32_t take_lookback_error(fdf_ctx* ctx) {
    volatile uint32_t* e = lookback_error_word(ctx);
    if (!e || *e == 0) return 0;
    const uint32_t v = *e;
    *e = 0;
    if (v & 4u) ctx->sums_dirty = true;
    return v;
}

// The overlapped upload's copy stream and chunk flags (created on first use).
int ensure_chunk_flags(fdf_ctx* ctx) {
    if (!ctx->copy_stream &&
        hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        ctx->copy_stream = nullptr;
        return FDF_ERR_DEVICE;
    }
    if (!ctx->h_flags) {
        void* hp = nullptr;
        void* dp = nullptr;
        if (hipHostMalloc(&hp, kMaxChunks * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return FDF_ERR_ALLOC;
        if (hipMalloc(&dp, kMaxChunks * sizeof(uint32_t)) != hipSuccess ||
            hipMemset(dp, 0, kMaxChunks * sizeof(uint32_t)) != hipSuccess) {
            (void)hipHostFree(hp);
            if (dp) (void)hipFree(dp);
            return FDF_ERR_ALLOC;
        }
        std::memset(hp, 0, kMaxChunks * sizeof(uint32_t));
        ctx->h_flags = static_cast<uint32_t*>(hp);
        ctx->d_flags = static_cast<uint32_t*>(dp);
    }
    return FDF_OK;
}

// Workgroups one CU holds of the detector instance for (nms, n) with `lds` bytes of LDS, from
// the runtime's occupancy calculator (registers, LDS, waves), cached per configuration.
uint32_t wg_per_cu(fdf_ctx* ctx, uint32_t nms, uint32_t n, uint32_t lds, bool rgb) {
    for (const auto& o : ctx->occupancy)
        if (o.nms == nms && o.n == n && o.lds == lds && o.rgb == rgb) return o.wg;
    int wg = 0;
    if (fdfk::sweep_occupancy(nms, n, lds, rgb, &wg) != hipSuccess || wg <= 0)
        wg = (int)std::min<uint32_t>(4u, fdfk::kSweepMaxLds / std::max(lds, 1u));   // LDS bound only
    ctx->occupancy.push_back({nms, n, lds, rgb, (uint32_t)wg});
    return (uint32_t)wg;
}

struct ChunkedUpload {
    const uint32_t* flags = nullptr;   // device address of the chunk flags (NULL: none)
    uint32_t rows = 0, epoch = 0;
};

// The switches of the ablation build (libfdf_debug.so; see fdf_kernels.h), read at every call:
// tools/ablate.py changes them between calls.  The release library reads no environment and
// gets the defaults.
struct DebugKnobs {
    GeometryKnobs geo;            // FDF_NSUB, FDF_LDS_BUDGET, FDF_DENSITY_MARGIN, FDF_COMPACT_TPG, FDF_DIRECT
    bool geometry_log = false;    // FDF_GEOMETRY_LOG: one line per launch on stderr
    uint32_t flags = 0;           // FDF_DEBUG_FLAGS: BandParams::flags
    bool stamps = false;          // FDF_STAMPS: per-workgroup stamps (fdf_debug_stamps)
    bool set_chunks = false;      // FDF_CHUNKS: written to ctx->chunks (A/B of the overlapped
    uint32_t chunks = 0;          // upload, tools/host_latency.py: 1 disables it)
};

DebugKnobs debug_knobs() {
    DebugKnobs k;
#ifdef FDF_DEBUG_BUILD
    unsigned long v = 0;
    auto number = [&v](const char* name) {
        const char* e = std::getenv(name);
        if (e) v = std::strtoul(e, nullptr, 0);
        return e != nullptr;
    };
    if (number("FDF_NSUB")) k.geo.nsub = (uint32_t)std::max(1ul, v);
    if (number("FDF_LDS_BUDGET"))
        k.geo.lds_budget_nms = k.geo.lds_budget_plain = std::min<uint32_t>(fdfk::kSweepMaxLds, (uint32_t)v);
    if (const char* e = std::getenv("FDF_DENSITY_MARGIN")) k.geo.density_margin = std::strtod(e, nullptr);
    if (number("FDF_COMPACT_TPG"))
        k.geo.compact_tpg = std::max(1u, std::min((uint32_t)fdfk::kCompactTasks, (uint32_t)v));
    if (number("FDF_DIRECT")) k.geo.allow_direct = v != 0;
    k.geometry_log = std::getenv("FDF_GEOMETRY_LOG") != nullptr;
    if (number("FDF_DEBUG_FLAGS")) k.flags = (uint32_t)v;
    k.stamps = std::getenv("FDF_STAMPS") != nullptr;
    if ((k.set_chunks = number("FDF_CHUNKS"))) k.chunks = (uint32_t)v;
#endif
    return k;
}

// ---- the steps of enqueue(), in its order ------------------------------------------------

// First use: the context's two host-mapped words (h_stats[0] the NMS keypoint statistics,
// h_stats[1] the look-back error word).  Without them the launches run with neither.
void ensure_stats_word(fdf_ctx* ctx) {
    if (ctx->h_stats) return;
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
        ctx->h_stats = static_cast<uint64_t*>(hp);
        ctx->d_stats = static_cast<uint64_t*>(dp);
        std::memset(hp, 0, 64);
    } else if (hp) {
        (void)hipHostFree(hp);
    }
}

// NMS: the keypoint density (per pixel, before suppression) the last finished launch of this
// configuration measured, 0 when none did.  Takes the statistics word's news into `known`.
double known_density(fdf_ctx* ctx, const fdf_config* cfg, uint32_t w) {
    if (!cfg->nms || !ctx->h_stats) return 0.0;
    const uint64_t v = *reinterpret_cast<volatile uint64_t*>(ctx->h_stats);
    const uint32_t seq = (uint32_t)(v >> 32);
    const fdf_ctx::LaunchInfo& li = ctx->hist[seq % 64];
    if (seq != 0 && li.seq == seq && li.pixels > 0) {
        ctx->known[li.nms % 3] = li;
        ctx->known_density[li.nms % 3] = (double)(uint32_t)v / li.pixels;
    }
    const fdf_ctx::LaunchInfo& k = ctx->known[cfg->nms % 3];
    if (k.seq != 0 && k.t == cfg->threshold && k.n == cfg->count && k.nms == cfg->nms && k.w == w)
        return ctx->known_density[cfg->nms % 3];
    return 0.0;
}

// `stream` follows the context's previous device work, whatever stream that ran on.
int follow_last_enqueue(fdf_ctx* ctx, hipStream_t stream) {
    if (!ctx->done &&
        hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming) != hipSuccess) {
        ctx->done = nullptr;
        return FDF_ERR_DEVICE;
    }
    if (ctx->done_valid && ctx->done_stream != stream &&
        (record_done(ctx) != hipSuccess || hipStreamWaitEvent(stream, ctx->done, 0) != hipSuccess))
        return FDF_ERR_DEVICE;
    return FDF_OK;
}

// The launch's workspace: band slots and counts, the group sums (zeroed again after a failed
// launch), and for a direct launch the look-back descriptors and its tag (*epoch, else 0).
int ensure_workspace(fdf_ctx* ctx, const LaunchPlan& pl, hipStream_t stream, uint32_t* epoch) {
    int rc;
    if ((rc = ensure(ctx, &ctx->d_slots, &ctx->slots_bytes, (size_t)(pl.ntasks * pl.slot_bytes), stream))) return rc;
    if ((rc = ensure(ctx, &ctx->d_counts, &ctx->counts_n, (size_t)pl.ntasks, stream))) return rc;
    if (!ctx->d_sums) {
        if (hipMalloc(reinterpret_cast<void**>(&ctx->d_sums),
                      (2 * fdfk::kMaxGroupSums + 4) * sizeof(uint32_t)) != hipSuccess) {
            ctx->d_sums = nullptr;
            return FDF_ERR_ALLOC;
        }
        ctx->sums_dirty = true;
    }
    if (ctx->sums_dirty) {
        if (hipMemsetAsync(ctx->d_sums, 0, (2 * fdfk::kMaxGroupSums + 4) * sizeof(uint32_t),
                           stream) != hipSuccess)
            return FDF_ERR_DEVICE;
        ctx->sums_dirty = false;
        ctx->ticket_next = 0;                       // the ticket counter is zero again
    }
    *epoch = 0;
    if (!pl.direct) return FDF_OK;
    // a (re)allocated buffer is zeroed: recycled device memory can hold descriptors of
    // another context's launches.  Launch tags are unique in the process as well.
    const size_t had = ctx->lookback_n;
    if ((rc = ensure(ctx, &ctx->d_lookback, &ctx->lookback_n, (size_t)pl.ntasks, stream))) return rc;
    if (ctx->lookback_n != had &&
        hipMemsetAsync(ctx->d_lookback, 0, ctx->lookback_n * sizeof(uint64_t), stream) != hipSuccess)
        return FDF_ERR_DEVICE;
    *epoch = ++g_launch_epoch;
    if (*epoch == 0) *epoch = ++g_launch_epoch;                    // 0 = a zeroed descriptor
    return FDF_OK;
}

// The parameter blocks of a launch's two kernels.
struct LaunchParams {
    fdfk::BandParams p;
    fdfk::CompactParams c;
};

// Both blocks over the workspace as it stands, what they share set once for both (no keypoint
// statistics and no stamps yet).
void fill_params(const fdf_ctx* ctx, const Geometry& geo, const LaunchPlan& pl,
                 const uint8_t* d_frames, uint64_t frame_stride, uint32_t w, uint32_t h,
                 const fdf_config* cfg, uint2* d_out, uint64_t cap, uint64_t* d_offsets,
                 uint32_t epoch, const ChunkedUpload& up, uint32_t flags, LaunchParams* lp) {
    fdfk::BandParams& p = lp->p;
    fdfk::CompactParams& c = lp->c;
    uint32_t* sums_now = ctx->d_sums + (size_t)ctx->sums_parity * fdfk::kMaxGroupSums;
    uint32_t* sums_next = ctx->d_sums + (size_t)(1 - ctx->sums_parity) * fdfk::kMaxGroupSums;
    p.width = c.width = w;
    p.height = c.height = h;
    p.rows = c.rows = geo.R;
    p.bands_per_frame = c.bands_per_frame = pl.bands;
    p.ntasks = c.ntasks = (uint32_t)pl.ntasks;
    p.words_per_row = c.words_per_row = pl.nw;
    p.slot_bytes = c.slot_bytes = pl.slot_bytes;
    p.tasks_per_group = c.tasks_per_group = pl.tpg;
    c.slots = p.slots = ctx->d_slots;
    c.counts = p.counts = ctx->d_counts;
    p.out = c.out = d_out;
    p.cap = c.cap = cap;
    p.frame_offsets = c.frame_offsets = d_offsets;
    c.group_sums = p.group_sums = pl.grouped ? sums_now : nullptr;
    p.kp_stats = c.kp_stats = nullptr;
    // the detector's own
    p.frames = d_frames;
    p.frame_stride = frame_stride;
    p.threshold = cfg->threshold;
    p.flags = flags;
    p.nstrips = geo.nstrips;
    p.nsub = geo.nsub;
    p.stamps = nullptr;
    p.direct = pl.direct ? 1u : 0u;
    p.epoch = epoch;
    p.lookback = pl.direct ? ctx->d_lookback : nullptr;
    p.ticket = ctx->d_sums + 2 * fdfk::kMaxGroupSums + 2;
    p.ticket_base = ctx->ticket_next;
    p.lookback_error = ctx->h_stats ? reinterpret_cast<uint32_t*>(ctx->d_stats + 1) : nullptr;
    p.chunk_flags = up.flags;
    p.chunk_rows = up.rows;
    p.chunk_epoch = up.epoch;
    // the compaction's own
    c.next_sums = sums_next;
    c.stats_out = nullptr;
    c.stats_seq = 0;
}

// NMS with a compaction launch: the launch reports its keypoint total before suppression
// under a new sequence number, and `hist` keeps what it was measured on (known_density).
void open_density_record(fdf_ctx* ctx, const fdf_config* cfg, uint32_t n_frames, uint32_t w,
                         uint32_t h, LaunchParams* lp) {
    if (!cfg->nms || !ctx->h_stats || lp->p.direct) return;
    const uint32_t seq = ++ctx->stats_seq == 0 ? ++ctx->stats_seq : ctx->stats_seq;
    fdf_ctx::LaunchInfo& li = ctx->hist[seq % 64];
    li.seq = seq;
    li.t = cfg->threshold;
    li.n = cfg->count;
    li.nms = cfg->nms;
    li.w = w;
    li.pixels = (double)n_frames * (double)w * (double)(h - 6);
    lp->p.kp_stats = lp->c.kp_stats = ctx->d_sums + 2 * fdfk::kMaxGroupSums + 1;
    lp->c.stats_out = ctx->d_stats;
    lp->c.stats_seq = seq;
}

// per-kernel timing: 4 events per call, timestamped by the dispatches themselves
// (hipExtLaunchKernelGGL), so no marker packets sit between the kernels.  *ev: this call's
// four, or NULL when it is not a timed one.
int timing_events(fdf_ctx* ctx, hipEvent_t** ev) {
    *ev = nullptr;
    if (!ctx->timing || ctx->timing_calls++ % ctx->timing != 0 || ctx->timed >= kMaxTimedCalls)
        return FDF_OK;
    while (ctx->ev.size() < 4 * (ctx->timed + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return FDF_ERR_DEVICE;
        ctx->ev.push_back(e);
    }
    *ev = &ctx->ev[4 * ctx->timed];
    return FDF_OK;
}

// The detector, and the compaction unless the bands write their points themselves.  A failed
// launch may leave the group sums and the ticket counter half used: they are zeroed again.
int launch_kernels(fdf_ctx* ctx, const LaunchParams& lp, const LaunchPlan& pl,
                   const fdf_config* cfg, bool rgb, hipStream_t stream, hipEvent_t* ev) {
    auto launch = rgb ? fdfk::launch_sweep_rgb
                      : (pl.exit_in_block ? fdfk::launch_sweep_latency : fdfk::launch_sweep);
    if (launch(lp.p, cfg->nms, cfg->count, stream, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr) !=
            hipSuccess ||
        (!pl.direct && fdfk::launch_compact(lp.c, stream, ev ? ev[2] : nullptr,
                                            ev ? ev[3] : nullptr) != hipSuccess)) {
        ctx->sums_dirty = true;
        return FDF_ERR_DEVICE;
    }
    return FDF_OK;
}

// After the launches: tickets, the group sums' parity, the timed call, the compaction kept
// for a relaunch (run_host) and the completion event.
int note_launch(fdf_ctx* ctx, const LaunchParams& lp, const LaunchPlan& pl, bool timed,
                hipStream_t stream) {
    if (pl.direct) ctx->ticket_next += (uint32_t)pl.ntasks;   // the launch takes one per workgroup
    if (pl.grouped) ctx->sums_parity ^= 1;
    if (timed) {
        if (ctx->timed_compact.size() <= ctx->timed) ctx->timed_compact.resize(ctx->timed + 1);
        ctx->timed_compact[ctx->timed] = pl.direct ? 0 : 1;
        ++ctx->timed;
    }
    ctx->last_compact = lp.c;
    return note_done(ctx, stream) == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
}

// Enqueue detection + compaction over `n_frames` device frames (w, h >= 7) on `stream`,
// after the context's previous device work (which may have run on another stream: the
// workspace is shared).
int enqueue(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t w, uint32_t h,
            uint64_t frame_stride, const fdf_config* cfg, uint2* d_out, uint64_t cap,
            uint64_t* d_offsets, hipStream_t stream, bool rgb = false,
            const ChunkedUpload& up = ChunkedUpload{}, bool host_src = false) {
    const DebugKnobs knobs = debug_knobs();
    ensure_stats_word(ctx);
    const double density = known_density(ctx, cfg, w);
    // workgroup slots of the device: 4 per CU (4 waves per SIMD); fdf_ctx_set_geometry's
    // min_tasks replaces it (1: the tall bands of a large batch for any job)
    const uint64_t per_cu = 4;
    const uint64_t slots = ctx->min_tasks ? ctx->min_tasks
                                          : (ctx->cus ? per_cu * ctx->cus : kDefaultMinTasks);
    const uint64_t fill = ctx->min_tasks ? ctx->min_tasks : kDefaultMinTasks;
    const Geometry geo = pick_geometry(n_frames, w, h, cfg->nms, slots, density, ctx->band_rows,
                                       host_src, knobs.geo);
    if (knobs.geometry_log)
        std::fprintf(stderr, "fdf geometry: %u x %ux%u nms=%u t=%u n=%u density=%.5f R=%u nsub=%u\n",
                     n_frames, w, h, (unsigned)cfg->nms, (unsigned)cfg->threshold,
                     (unsigned)cfg->count, density, geo.R, geo.nsub);
    // (a band too large for the LDS has no occupancy to ask for: the plan reports it)
    const uint32_t lds = sweep_lds(geo, w, cfg->nms);
    const uint32_t wgs = lds <= fdfk::kSweepMaxLds ? wg_per_cu(ctx, cfg->nms, cfg->count, lds, rgb) : 0u;
    const LaunchPlan pl = make_launch_plan(geo, n_frames, w, h, cfg->nms, rgb, fill, wgs, ctx->cus,
                                           knobs.geo);
    if (pl.status) return pl.status;
    int rc;
    uint32_t epoch;
    if ((rc = follow_last_enqueue(ctx, stream))) return rc;
    if ((rc = ensure_workspace(ctx, pl, stream, &epoch))) return rc;
    LaunchParams lp;
    fill_params(ctx, geo, pl, d_frames, frame_stride, w, h, cfg, d_out, cap, d_offsets, epoch, up,
                knobs.flags, &lp);
    if (knobs.stamps) {
        const size_t words = (size_t)pl.ntasks * fdfk::kStampWords;
        if ((rc = ensure(ctx, &ctx->d_stamps, &ctx->stamps_n, words, stream))) return rc;
        lp.p.stamps = ctx->d_stamps;
        ctx->stamps_used = words;
    }
    open_density_record(ctx, cfg, n_frames, w, h, &lp);
    hipEvent_t* ev;
    if ((rc = timing_events(ctx, &ev))) return rc;
    if ((rc = launch_kernels(ctx, lp, pl, cfg, rgb, stream, ev))) return rc;
    return note_launch(ctx, lp, pl, ev != nullptr, stream);
}

// The score reported with a keypoint: the NMS mode's own, max-threshold when NMS is off.
uint32_t score_kind(uint32_t nms) {
    return nms == FDF_NMS_SUM_ABSOLUTE ? FDF_NMS_SUM_ABSOLUTE : FDF_NMS_MAX_THRESHOLD;
}
// ~4 points per thread on average, 1..64 workgroups per frame.
uint32_t score_blocks(uint64_t points, uint32_t n_frames) {
    const uint64_t per_frame = points / std::max<uint32_t>(n_frames, 1u);
    return (uint32_t)std::min<uint64_t>(64, per_frame / 1024 + 1);
}

// Validation shared by the host entry points; *empty = the reference returns no points.
int check_host_args(const uint8_t* data, uint32_t n_frames, uint32_t w, uint32_t h,
                    size_t row_stride, const fdf_config* cfg, bool rgb, int* empty) {
    int rc = check_config(cfg);
    if (rc) return rc;
    rc = check_shape(w, h, empty);
    if (rc) return rc;
    if (n_frames == 0) *empty = 1;
    if (!data && !*empty) return FDF_ERR_ARG;
    if (row_stride < (rgb ? 3ull * w : (size_t)w)) return FDF_ERR_ARG;
    return FDF_OK;
}

// ---- the steps of run_host() ---------------------------------------------------------------

// The host frames of a call: `n` frames of `h` rows of px * w bytes, the rows `row_stride`
// and the frames `frame_stride` bytes apart.
struct HostFrames {
    const uint8_t* data;
    uint32_t n, w, h;
    size_t row_stride, frame_stride;
    size_t px;                                     // bytes per pixel: 3 (RGB8) or 1
    size_t row_bytes() const { return px * w; }
    size_t frame_bytes() const { return px * w * h; }
    size_t span() const {                          // first byte to last
        return (size_t)(n - 1) * frame_stride + (size_t)(h - 1) * row_stride + px * w;
    }
};

// The output of a host detection as the kernels address it.  `host`: the pinned,
// device-mapped h_out / h_offs (the kernels write the points and offsets into host memory: no
// copy back, one synchronisation); otherwise the device buffers d_out / d_offsets (the scored
// calls, whose score kernel reads the points).
struct HostOutput {
    fdf_ctx* ctx;
    bool host;
    uint2* points() const { return host ? ctx->hd_out : ctx->d_out; }
    uint64_t* offsets() const { return host ? ctx->hd_offs : ctx->d_offsets; }
    size_t cap() const { return host ? ctx->h_out_points : ctx->out_points; }
    int grow(size_t total) const {
        return host ? ensure_host(ctx, &ctx->h_out, &ctx->hd_out, &ctx->h_out_points, total, ctx->stream)
                    : ensure(ctx, &ctx->d_out, &ctx->out_points, total, ctx->stream);
    }
    int grow_offsets(size_t n) const {
        return host ? ensure_host(ctx, &ctx->h_offs, &ctx->hd_offs, &ctx->h_offs_n, n, ctx->stream)
                    : ensure(ctx, &ctx->d_offsets, &ctx->offsets_n, n, ctx->stream);
    }
};

// Where a host range lies for the copy engines and the kernels: in pageable memory, inside
// one pinned mapping (`dev`: the device address of its first byte, `flags`: the mapping's
// allocation flags), or starting in a pinned mapping and running past it (a
// hipHostRegister'ed range shorter than the frames).
struct PinnedRange {
    enum Kind { kPageable, kWhole, kPartial } kind;
    const uint8_t* dev;
    unsigned flags;
};

// The range's first and last bytes must both be pinned and map to one contiguous device range.
PinnedRange probe_pinned(const uint8_t* p, size_t bytes) {
    hipPointerAttribute_t a, z;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // pageable memory: not an error here
        return {PinnedRange::kPageable, nullptr, 0};
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return {PinnedRange::kPageable, nullptr, 0};
    const uint8_t* dev = static_cast<const uint8_t*>(a.devicePointer);
    bool whole = false;
    if (hipPointerGetAttributes(&z, p + bytes - 1) == hipSuccess)
        whole = z.type == hipMemoryTypeHost &&
                static_cast<const uint8_t*>(z.devicePointer) == dev + (bytes - 1);
    else
        (void)hipGetLastError();   // the range runs past the pinned mapping
    return {whole ? PinnedRange::kWhole : PinnedRange::kPartial, dev, a.allocationFlags};
}

// Frames that start in pinned host memory must lie inside one pinned mapping for the DMA
// copies (the chunked upload's too): a range that runs past it is packed into the pinned
// staging buffer by the CPU first, and `in` then describes the packed copy.
int pack_to_staging(fdf_ctx* ctx, HostFrames* in) {
    const size_t fb = in->frame_bytes(), rb = in->row_bytes();
    const int rc = ensure_host(ctx, &ctx->h_stage, &ctx->hd_stage, &ctx->h_stage_bytes, fb * in->n,
                               ctx->stream);
    if (rc) return rc;
    for (uint32_t f = 0; f < in->n; ++f)
        for (uint32_t y = 0; y < in->h; ++y)
            std::memcpy(ctx->h_stage + f * fb + (size_t)y * rb,
                        in->data + f * in->frame_stride + (size_t)y * in->row_stride, rb);
    in->data = ctx->h_stage;
    in->row_stride = rb;
    in->frame_stride = fb;
    return FDF_OK;
}

// One grey frame to d_in in `nchunks` row chunks on the copy stream while the detector runs,
// each band waiting for the chunk of its last row (`up`: what the detector needs for that).
// A failure means the runtime cannot do this upload; the copy stream is drained.
int upload_chunked(fdf_ctx* ctx, const HostFrames& in, uint32_t nchunks, ChunkedUpload* up) {
    up->rows = (in.h + nchunks - 1) / nchunks;
    up->epoch = ++ctx->chunk_epoch == 0 ? ++ctx->chunk_epoch : ctx->chunk_epoch;
    up->flags = ctx->d_flags;
    for (uint32_t r0 = 0, c = 0; r0 < in.h; r0 += up->rows, ++c) {
        const uint32_t nr = std::min(up->rows, in.h - r0);
        hipError_t e = upload_rows(ctx->d_in + (size_t)r0 * in.w, in.data + (size_t)r0 * in.row_stride,
                                   in.row_stride, in.w, nr, ctx->copy_stream);
        // the chunk's flag: a 4-byte copy behind it on the same (copy-engine) queue --
        // hipStreamWriteValue32 is a kernel launch per call on this runtime (~20 us each)
        ctx->h_flags[c] = up->epoch;
        if (e == hipSuccess)
            e = hipMemcpyAsync(ctx->d_flags + c, ctx->h_flags + c, sizeof(uint32_t),
                               hipMemcpyHostToDevice, ctx->copy_stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->copy_stream);
            (void)hipGetLastError();
            return FDF_ERR_DEVICE;
        }
    }
    return FDF_OK;
}

// Every frame to `stage`, packed, on the context's stream before the launch.
int upload_frames(fdf_ctx* ctx, const HostFrames& in, uint8_t* stage) {
    for (uint32_t f = 0; f < in.n; ++f)
        if (upload_rows(stage + (size_t)f * in.frame_bytes(), in.data + (size_t)f * in.frame_stride,
                        in.row_stride, in.row_bytes(), in.h, ctx->stream) != hipSuccess)
            return FDF_ERR_DEVICE;
    return FDF_OK;
}

int run_host(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames, uint32_t w, uint32_t h,
             size_t row_stride, size_t frame_stride, const fdf_config* cfg, bool rgb,
             uint64_t* offs, bool host_out);

// The overlapped upload failed or a band's wait for its chunk ran out: the call again with
// one copy before the launch (counted; the caller's chunk setting stays).
int retry_unchunked(fdf_ctx* ctx, const HostFrames& in, const fdf_config* cfg, uint64_t* offs,
                    bool host_out) {
    ++ctx->upload_fallbacks;
    const uint32_t saved = ctx->chunks;
    ctx->chunks = 1;
    const int rc = run_host(ctx, in.data, in.n, in.w, in.h, in.row_stride, in.frame_stride, cfg,
                            in.px == 3, offs, host_out);
    ctx->chunks = saved;
    return rc;
}

// The offsets on the host, once the stream's work is done: read in place (host output) or
// copied back.
hipError_t fetch_offsets(fdf_ctx* ctx, uint64_t* offs, uint32_t n_frames, bool host_out) {
    hipError_t e = hipSuccess;
    if (!host_out)
        e = hipMemcpyAsync(offs, ctx->d_offsets, sizeof(uint64_t) * (n_frames + 1ull),
                           hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = sync_own_stream(ctx);
    if (e == hipSuccess && host_out)
        std::memcpy(offs, ctx->h_offs, sizeof(uint64_t) * (n_frames + 1ull));
    return e;
}

// Phase 1 of a host detection (lock held): frames in, detection + compaction into the
// context's output buffer, frame offsets back to the host (`offs`, n_frames + 1 entries).
// The output starts small and grows to the keypoint total; when it has to grow only the
// compaction is run again (the per-band slots still hold the detection).  On success
// ctx->last describes the result, which stays in the context until the next host call.
// `host_out`: see HostOutput.
// `rgb`: the frames are RGB8 (rows of 3 * w bytes at row_stride), converted on the device
// with image 0.24.6's to_luma8 before detection (src/main.rs:58).
int run_host(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames, uint32_t w, uint32_t h,
             size_t row_stride, size_t frame_stride, const fdf_config* cfg, bool rgb,
             uint64_t* offs, bool host_out) {
    ctx->last = LastResult{};          // invalid, and not a shard of a multi-context call
    HostFrames in{data, n_frames, w, h, row_stride, frame_stride, rgb ? 3u : 1u};
    const HostOutput out{ctx, host_out};
    const size_t frame_bytes = (size_t)w * h;
    const size_t max_points = (size_t)(w - 6) * (h - 6) * n_frames;
    // first guess: 1 keypoint per 64 pixels (real images: 0.5-1.5 per 100)
    const size_t guess = std::min(max_points, std::max<size_t>(4096, frame_bytes / 64 * n_frames));
    int rc;
    if ((rc = ensure(ctx, &ctx->d_in, &ctx->in_bytes, frame_bytes * n_frames, ctx->stream))) return rc;
    if ((rc = out.grow(guess))) return rc;
    if ((rc = out.grow_offsets(n_frames + 1ull))) return rc;
    if (rgb && (rc = ensure(ctx, &ctx->d_rgb, &ctx->rgb_bytes, 3 * frame_bytes * n_frames, ctx->stream)))
        return rc;
    // the host frames are read by the copies below: nothing else may still read d_in (nor
    // the host output, which the host reads after this call)
    wait_done(ctx);
    // an error an earlier asynchronous fdf_detect_device left in the error word belongs to
    // that call: keep it for the next device call, so this call's own check sees only its own
    if (take_lookback_error(ctx)) ctx->pending_device_error = true;
    const DebugKnobs knobs = debug_knobs();
    if (knobs.set_chunks) ctx->chunks = knobs.chunks;
    // one grey frame of >= kChunkMinBytes: upload it in row chunks on the copy stream while
    // the detector runs (the H2D of a 1080p frame is ~45 us, the detector ~20 us: DESIGN.md
    // §7.5).  The chunk count in effect must be > 1: one chunk is one copy before the launch,
    // which the plain upload does without the flag copy and the second stream
    const uint32_t nchunks = std::min<uint32_t>(ctx->chunks ? ctx->chunks : kChunksDefault, kMaxChunks);
    const bool chunked = host_out && !rgb && n_frames == 1 && frame_bytes >= kChunkMinBytes &&
                         nchunks > 1 && ctx->h_stats && ensure_chunk_flags(ctx) == FDF_OK;
    // one packed grey frame in pinned (page-locked, non-coherent) host memory, unscored: the
    // detector reads it in place over PCIe, with no copy before the launch -- its row stream
    // is the upload (1080p max-t 72-75 vs 82-83 us end to end).  Host writes
    // to the buffer before the call are visible to the launch (the dispatch's system-scope
    // acquire; a wave-level acquire fence cost ~20 us and changed no result:
    // tests/test_gpu_host_inplace.py reuses one buffer for different frames).  The frame is
    // then not in d_in: a result that does not fit the caller's buffer copies it there for
    // fdf_fetch_last (detect_host).  A range that runs past its pinned mapping is copied, not
    // read past its end.
    const PinnedRange pin = probe_pinned(in.data, in.span());
    const bool in_place = ctx->chunks == 0 && host_out && !rgb && n_frames == 1 && row_stride == w &&
                          pin.kind == PinnedRange::kWhole && !(pin.flags & hipHostMallocCoherent);
    if (pin.kind == PinnedRange::kPartial && (rc = pack_to_staging(ctx, &in))) return rc;
    ChunkedUpload up;
    if (!in_place && chunked) {
        if (upload_chunked(ctx, in, nchunks, &up)) return retry_unchunked(ctx, in, cfg, offs, host_out);
    } else if (!in_place) {
        if ((rc = upload_frames(ctx, in, rgb ? ctx->d_rgb : ctx->d_in))) return rc;
    }
    // RGB: a luma pass, then the grey detector.  The detector with luma converted in its
    // loads (fdf_detect_device_rgb) is correct but measured 1.6x slower on 256 1080p frames:
    // its 48-byte row loads need 12 registers each until converted, which spills and
    // exposes the row latency
    if (rgb && fdfk::launch_rgb_to_luma(ctx->d_rgb, n_frames, (uint32_t)frame_bytes,
                                        3 * frame_bytes, ctx->d_in, ctx->stream) != hipSuccess)
        return FDF_ERR_DEVICE;
    rc = enqueue(ctx, in_place ? pin.dev : ctx->d_in, n_frames, w, h, frame_bytes, cfg, out.points(),
                 out.cap(), out.offsets(), ctx->stream, false, up, in_place);
    if (chunked) {
        // the copies end before the detector does (it waits for the last one), but a failed
        // launch or a timed-out wait would leave them running: drain them before any return
        const hipError_t e = hipStreamSynchronize(ctx->copy_stream);
        if (!rc && e != hipSuccess) rc = FDF_ERR_DEVICE;
    }
    if (rc) return rc;
    if (fetch_offsets(ctx, offs, n_frames, host_out) != hipSuccess) return FDF_ERR_DEVICE;
    if (const uint32_t err = take_lookback_error(ctx)) {
        if (err & 4u) return FDF_ERR_DEVICE;   // a band never ran: nothing to rebuild from
        // a band's wait for its upload chunk ran out (the copies are drained now): detect
        // again from the whole frame, uploaded before the launch
        if (err & 2u) return retry_unchunked(ctx, in, cfg, offs, host_out);
        // a direct-output band's look-back ran out (band_lookback): the offsets and points of
        // its frame on are not written; the slots and counts are, so the compaction rebuilds
        // both from them
        ++ctx->lookback_recoveries;
        fdfk::CompactParams c = ctx->last_compact;
        c.kp_stats = nullptr;
        c.group_sums = nullptr;
        if (fdfk::launch_compact(c, ctx->stream) != hipSuccess ||
            fetch_offsets(ctx, offs, n_frames, host_out) != hipSuccess)
            return FDF_ERR_DEVICE;
    }
    const uint64_t total = offs[n_frames];
    if (total > out.cap()) {
        // grow the output and compact again (the offsets do not change)
        if ((rc = out.grow((size_t)total))) return rc;
        fdfk::CompactParams c = ctx->last_compact;
        c.out = out.points();
        c.cap = out.cap();
        c.kp_stats = nullptr;           // already reported (and reset) by the first compaction
        if (fdfk::launch_compact(c, ctx->stream) != hipSuccess ||
            note_done(ctx, ctx->stream) != hipSuccess)
            return FDF_ERR_DEVICE;
        // the host reads h_out next: the compaction must be done
        if (host_out && sync_own_stream(ctx) != hipSuccess) return FDF_ERR_DEVICE;
    }
    ctx->last.valid = true;
    ctx->last.host_out = host_out;
    ctx->last.total = total;
    ctx->last.n_frames = n_frames;
    ctx->last.width = w;
    ctx->last.height = h;
    ctx->last.cfg = *cfg;
    ctx->last.rgb = false;          // the luma frames are in d_in
    ctx->last.in_place = in_place;  // ... or were read in place (not in d_in)
    return FDF_OK;
}

// Phase 2 (lock held): copy the first `n` points of the last result, and their scores when
// `out_scores` is given, to the host.
int copy_out(fdf_ctx* ctx, fdf_point* out, uint16_t* out_scores, size_t n) {
    if (!n) return FDF_OK;
    const LastResult& L = ctx->last;
    if (out_scores && L.in_place) return FDF_ERR_ARG;
    hipError_t e = hipSuccess;
    if (out_scores) {
        int rc = ensure(ctx, &ctx->d_scores, &ctx->scores_n, n, ctx->stream);
        if (rc) return rc;
        if (L.rgb) {   // the scores are computed from the luma frames
            const size_t fb = (size_t)L.width * L.height;
            if ((rc = ensure(ctx, &ctx->d_in, &ctx->in_bytes, fb * L.n_frames, ctx->stream))) return rc;
            if (fdfk::launch_rgb_to_luma(ctx->d_rgb, L.n_frames, (uint32_t)fb, 3 * fb, ctx->d_in,
                                         ctx->stream) != hipSuccess)
                return FDF_ERR_DEVICE;
        }
        // (a host-output result's points and offsets are read through their device-mapped
        // addresses)
        e = fdfk::launch_score_frames(ctx->d_in, L.width, (uint64_t)L.width * L.height,
                                      L.n_frames, L.host_out ? ctx->hd_out : ctx->d_out,
                                      L.host_out ? ctx->hd_offs : ctx->d_offsets, n,
                                      score_blocks(n, L.n_frames), score_kind(L.cfg.nms),
                                      L.cfg.threshold, L.cfg.count, ctx->d_scores, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(out_scores, ctx->d_scores, n * sizeof(uint16_t),
                               hipMemcpyDeviceToHost, ctx->stream);
    }
    if (L.host_out) {
        if (e == hipSuccess && out_scores) e = sync_own_stream(ctx);
        if (e == hipSuccess) std::memcpy(out, ctx->h_out, n * sizeof(fdf_point));
        return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, ctx->d_out, n * sizeof(fdf_point), hipMemcpyDeviceToHost,
                           ctx->stream);
    if (e == hipSuccess) e = sync_own_stream(ctx);
    return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
}

// Shared body of fdf_detect / fdf_detect_batch / the scored and RGB variants: host frames
// in, host points out.  With `cap` below the total, the first `cap` points are written,
// FDF_ERR_CAPACITY is returned and the whole result stays on the device for fdf_fetch_last.
int detect_host(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames, uint32_t w, uint32_t h,
                size_t row_stride, size_t frame_stride, const fdf_config* cfg, fdf_point* out,
                size_t cap, uint64_t* frame_offsets, size_t* n_out, bool rgb = false,
                uint16_t* out_scores = nullptr, bool scored = false) {
    if (!ctx || !n_out || (cap && !out) || (scored && cap && !out_scores)) return FDF_ERR_ARG;
    int empty = 0;
    int rc = check_host_args(data, n_frames, w, h, row_stride, cfg, rgb, &empty);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (empty) {
        ctx->last = LastResult{};
        ctx->last.valid = true;
        ctx->last.cfg = *cfg;
        *n_out = 0;
        if (frame_offsets) std::memset(frame_offsets, 0, sizeof(uint64_t) * (n_frames + 1ull));
        return FDF_OK;
    }
    DeviceGuard guard(ctx->device);
    std::vector<uint64_t> local;
    uint64_t* offs = frame_offsets;
    if (!offs) {
        local.resize(n_frames + 1ull);
        offs = local.data();
    }
    // unscored calls take the host-mapped output (no copy back); the scored ones keep the
    // points on the device for the score kernel.  (Points written straight into a caller's
    // pinned output buffer, round 5 and again in round 6, came with an asynchronous device
    // error in a later test in 3 of 5 full GPU-suite runs: DESIGN.md §7.7.)
    rc = run_host(ctx, data, n_frames, w, h, row_stride, frame_stride, cfg, rgb, offs, !scored);
    if (rc) return rc;
    const uint64_t total = offs[n_frames];
    if (total > cap && ctx->last.in_place) {
        // the two-call pattern follows: keep the frame for fdf_fetch_last's scores
        if (hipMemcpyAsync(ctx->d_in, data, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream) !=
                hipSuccess ||
            sync_own_stream(ctx) != hipSuccess)
            return FDF_ERR_DEVICE;
        ctx->last.in_place = false;
    }
    rc = copy_out(ctx, out, scored ? out_scores : nullptr, (size_t)std::min<uint64_t>(total, cap));
    if (rc) return rc;
    *n_out = (size_t)total;
    return total > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

// Locks the contexts of a multi-context call in one global order (by address), whatever
// order the caller lists them in: two calls over the same contexts cannot deadlock.
std::vector<std::unique_lock<std::mutex>> lock_all(fdf_ctx* const* ctxs, uint32_t n) {
    std::vector<fdf_ctx*> order(ctxs, ctxs + n);
    std::sort(order.begin(), order.end(), std::less<fdf_ctx*>());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(n);
    for (fdf_ctx* c : order) locks.emplace_back(c->mu);
    return locks;
}


// Copy of the last host result (fdf_fetch_last), lock held.
int fetch_last(fdf_ctx* ctx, fdf_point* out, uint16_t* out_scores, size_t cap, size_t* n_out) {
    if (!ctx->last.valid) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    const uint64_t total = ctx->last.total;
    *n_out = (size_t)total;
    const int rc = copy_out(ctx, out, out_scores, (size_t)std::min<uint64_t>(total, cap));
    if (rc) return rc;
    return total > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

}  // namespace

extern "C" {

int fdf_abi_version(void) { return FDF_ABI_VERSION; }

const char* fdf_status_string(int status) {
    switch (status) {
        case FDF_OK: return "ok";
        case FDF_ERR_COUNT: return "count must be in [9, 16]";
        case FDF_ERR_SIZE: return "image size not supported by the reference (h < 3, or w < 6 with h >= 7)";
        case FDF_ERR_CAPACITY: return "output buffer too small";
        case FDF_ERR_NMS: return "unknown non-maximal suppression mode";
        case FDF_ERR_DEVICE: return "HIP device error";
        case FDF_ERR_ARG: return "invalid argument";
        case FDF_ERR_ALLOC: return "allocation failed";
        case FDF_ERR_BUSY: return "pipeline slot still holds uncollected results";
        case FDF_ERR_DROPPED: return "batch found more keypoints than the pipeline's device capacity";
        default: return "unknown status";
    }
}

int fdf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fdf_validate(uint32_t width, uint32_t height, const fdf_config* cfg, int* empty) {
    if (!empty) return FDF_ERR_ARG;
    int rc = check_config(cfg);
    if (rc) return rc;
    return check_shape(width, height, empty);
}

int fdf_ctx_create(int device, fdf_ctx** out_ctx) {
    if (!out_ctx) return FDF_ERR_ARG;
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return FDF_ERR_DEVICE;
    fdf_ctx* ctx = new (std::nothrow) fdf_ctx();
    if (!ctx) return FDF_ERR_ALLOC;
    ctx->device = device;
    DeviceGuard guard(device);
    hipDeviceProp_t prop;
    ctx->cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? (uint32_t)prop.multiProcessorCount : 0u;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return FDF_ERR_DEVICE;
    }
    *out_ctx = ctx;
    return FDF_OK;
}

void fdf_ctx_destroy(fdf_ctx* ctx) {
    if (!ctx) return;
    {
        DeviceGuard guard(ctx->device);
        wait_done(ctx);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(ctx->d_in);
        (void)hipFree(ctx->d_rgb);
        (void)hipFree(ctx->d_out);
        (void)hipFree(ctx->d_offsets);
        if (ctx->h_out) (void)hipHostFree(ctx->h_out);
        if (ctx->h_offs) (void)hipHostFree(ctx->h_offs);
        if (ctx->h_flags) (void)hipHostFree(ctx->h_flags);
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        (void)hipFree(ctx->d_flags);
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        (void)hipFree(ctx->d_scores);
        (void)hipFree(ctx->d_slots);
        (void)hipFree(ctx->d_counts);
        (void)hipFree(ctx->d_sums);
        (void)hipFree(ctx->d_stamps);
        (void)hipFree(ctx->d_lookback);
        for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
        if (ctx->done) (void)hipEventDestroy(ctx->done);
        if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
        (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

void* fdf_ctx_stream(fdf_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->stream) : nullptr; }

int fdf_ctx_set_timing(fdf_ctx* ctx, int enable) {
    if (!ctx) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->timing = enable > 0 ? (uint32_t)enable : 0u;
    ctx->timed = 0;
    ctx->timing_calls = 0;
    return FDF_OK;
}

int fdf_ctx_workspace_bytes(fdf_ctx* ctx, uint64_t* bytes) {
    if (!ctx || !bytes) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    *bytes = ctx->in_bytes + ctx->rgb_bytes + ctx->out_points * sizeof(uint2) +
             ctx->offsets_n * sizeof(uint64_t) + ctx->scores_n * sizeof(uint16_t) +
             ctx->slots_bytes + ctx->counts_n * sizeof(uint32_t) +
             (ctx->d_sums ? (2 * fdfk::kMaxGroupSums + 4) * sizeof(uint32_t) : 0);
    return FDF_OK;
}

int fdf_ctx_recoveries(fdf_ctx* ctx, uint64_t* upload_fallbacks, uint64_t* lookback_recoveries) {
    if (!ctx) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (upload_fallbacks) *upload_fallbacks = ctx->upload_fallbacks;
    if (lookback_recoveries) *lookback_recoveries = ctx->lookback_recoveries;
    return FDF_OK;
}

int fdf_ctx_test_skew_tickets(fdf_ctx* ctx, uint32_t delta) {
    if (!ctx) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->ticket_next += delta;
    return FDF_OK;
}

int fdf_ctx_set_geometry(fdf_ctx* ctx, uint32_t min_tasks) {
    if (!ctx) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->min_tasks = min_tasks;
    return FDF_OK;
}

int fdf_ctx_set_upload_chunks(fdf_ctx* ctx, uint32_t chunks) {
    if (!ctx || chunks > kMaxChunks) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->chunks = chunks;
    return FDF_OK;
}

int fdf_ctx_set_band_rows(fdf_ctx* ctx, uint32_t rows) {
    if (!ctx || rows > kMaxBandRows) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->band_rows = rows;
    return FDF_OK;
}

// Kernel durations of recorded call k (0 for a compaction the call did not launch).
static int timed_call(fdf_ctx* ctx, size_t k, float* detect_ms, float* compact_ms) {
    const hipEvent_t* e = &ctx->ev[4 * k];
    const bool compact = k < ctx->timed_compact.size() && ctx->timed_compact[k];
    *compact_ms = 0.0f;
    if (hipEventSynchronize(e[1]) != hipSuccess ||
        hipEventElapsedTime(detect_ms, e[0], e[1]) != hipSuccess)
        return FDF_ERR_DEVICE;
    if (compact && (hipEventSynchronize(e[3]) != hipSuccess ||
                    hipEventElapsedTime(compact_ms, e[2], e[3]) != hipSuccess))
        return FDF_ERR_DEVICE;
    return FDF_OK;
}

int fdf_ctx_timing_samples(fdf_ctx* ctx, float* detect_ms, float* compact_ms, uint32_t cap,
                           uint32_t* n) {
    if (!ctx || !n || (cap && (!detect_ms || !compact_ms))) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    *n = (uint32_t)ctx->timed;
    for (size_t k = 0; k < ctx->timed && k < cap; ++k)
        if (timed_call(ctx, k, &detect_ms[k], &compact_ms[k]) != FDF_OK) return FDF_ERR_DEVICE;
    return FDF_OK;
}

int fdf_ctx_timing(fdf_ctx* ctx, uint32_t* calls, float* detect_ms, float* compact_ms) {
    if (!ctx || !calls || !detect_ms || !compact_ms) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    *calls = (uint32_t)ctx->timed;
    *detect_ms = *compact_ms = 0.0f;
    for (size_t k = 0; k < ctx->timed; ++k) {
        float a = 0.0f, b = 0.0f;
        if (timed_call(ctx, k, &a, &b) != FDF_OK) return FDF_ERR_DEVICE;
        *detect_ms += a;
        *compact_ms += b;
    }
    return FDF_OK;
}

int fdf_detect(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
               size_t stride_bytes, const fdf_config* cfg, fdf_point* out, size_t cap,
               size_t* n_out) {
    return detect_host(ctx, data, 1, width, height, stride_bytes, 0, cfg, out, cap, nullptr,
                       n_out);
}

int fdf_fetch_last(fdf_ctx* ctx, fdf_point* out, uint16_t* out_scores, size_t cap,
                   size_t* n_out) {
    if (!ctx || !n_out || (cap && !out)) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    return fetch_last(ctx, out, out_scores, cap, n_out);
}

int fdf_detect_rgb(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                   size_t stride_bytes, const fdf_config* cfg, fdf_point* out, size_t cap,
                   size_t* n_out) {
    return detect_host(ctx, data, 1, width, height, stride_bytes, 0, cfg, out, cap, nullptr,
                       n_out, true);
}

int fdf_rgb_to_luma_device(fdf_ctx* ctx, const uint8_t* d_rgb, uint32_t n_frames,
                           uint32_t width, uint32_t height, uint64_t rgb_frame_stride_bytes,
                           uint8_t* d_grey, void* stream) {
    if (!ctx) return FDF_ERR_ARG;
    const uint64_t pixels = (uint64_t)width * height;
    if (n_frames == 0 || pixels == 0) return FDF_OK;
    if (!d_rgb || !d_grey || pixels > 0x7fffffffull / 3 || rgb_frame_stride_bytes < 3 * pixels ||
        n_frames > 65535u)
        return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_rgb_to_luma(d_rgb, n_frames, (uint32_t)pixels, rgb_frame_stride_bytes,
                                              d_grey, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_detect_scored(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_config* cfg, fdf_point* out,
                      uint16_t* out_scores, size_t cap, size_t* n_out) {
    return detect_host(ctx, data, 1, width, height, stride_bytes, 0, cfg, out, cap, nullptr,
                       n_out, false, out_scores, true);
}

int fdf_detect_batch_scored(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames,
                            uint32_t width, uint32_t height, size_t frame_stride_bytes,
                            const fdf_config* cfg, fdf_point* out, uint16_t* out_scores,
                            size_t cap, uint64_t* frame_offsets, size_t* n_out) {
    if (n_frames > 1 && frame_stride_bytes < (size_t)width * height) return FDF_ERR_ARG;
    if (n_frames > 65535u) return FDF_ERR_ARG;
    return detect_host(ctx, data, n_frames, width, height, width, frame_stride_bytes, cfg, out,
                       cap, frame_offsets, n_out, false, out_scores, true);
}

int fdf_score_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                     uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                     const fdf_config* cfg, const fdf_point* d_points, uint64_t cap,
                     const uint64_t* d_frame_offsets, uint16_t* d_scores, void* stream) {
    if (!ctx || !d_frame_offsets) return FDF_ERR_ARG;
    int rc = check_config(cfg);
    if (rc) return rc;
    int empty = 0;
    rc = check_shape(width, height, &empty);
    if (rc) return rc;
    if (empty || n_frames == 0 || cap == 0) return FDF_OK;
    if (!d_frames || !d_points || !d_scores || n_frames > 65535u) return FDF_ERR_ARG;
    if (n_frames > 1 && frame_stride_bytes < (uint64_t)width * height) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    const uint64_t fs = frame_stride(n_frames, frame_stride_bytes, (uint64_t)width * height);
    const uint64_t est = std::min<uint64_t>(cap, (uint64_t)width * height / 32 * n_frames);
    return status_of(fdfk::launch_score_frames(
        d_frames, width, fs, n_frames, reinterpret_cast<const uint2*>(d_points), d_frame_offsets, cap,
        score_blocks(est, n_frames), score_kind(cfg->nms), cfg->threshold, cfg->count, d_scores,
        reinterpret_cast<hipStream_t>(stream)));
}

int fdf_detect_batch(fdf_ctx* ctx, const uint8_t* data, uint32_t n_frames, uint32_t width,
                     uint32_t height, size_t frame_stride_bytes, const fdf_config* cfg,
                     fdf_point* out, size_t cap, uint64_t* frame_offsets, size_t* n_out) {
    if (n_frames > 1 && frame_stride_bytes < (size_t)width * height) return FDF_ERR_ARG;
    return detect_host(ctx, data, n_frames, width, height, width, frame_stride_bytes, cfg, out,
                       cap, frame_offsets, n_out);
}

// Shared body of fdf_detect_device and fdf_detect_device_rgb (`rgb`: RGB8 frames of 3 bytes
// per pixel, luma converted in the detector's loads).
static int detect_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                         uint32_t height, uint64_t frame_stride_bytes, const fdf_config* cfg,
                         fdf_point* d_out, uint64_t cap, uint64_t* d_frame_offsets, void* stream,
                         bool rgb) {
    if (!ctx || !d_frame_offsets) return FDF_ERR_ARG;
    int rc = check_config(cfg);
    if (rc) return rc;
    int empty = 0;
    rc = check_shape(width, height, &empty);
    if (rc) return rc;
    if (n_frames == 0) empty = 1;
    if (!empty && (!d_frames || (cap && !d_out))) return FDF_ERR_ARG;
    const uint64_t fb = (rgb ? 3ull : 1ull) * width * height;
    if (rgb && fb > 0x7fffffffull) return FDF_ERR_SIZE;
    if (n_frames > 1 && frame_stride_bytes < fb) return FDF_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // an earlier asynchronous direct-output launch of this context had a look-back wait run
    // out (band_lookback; never seen in practice): its output was incomplete -- reported once
    // (also when a host call in between found the error word first: pending_device_error)
    if (take_lookback_error(ctx) || ctx->pending_device_error) {
        ctx->pending_device_error = false;
        return FDF_ERR_DEVICE;
    }
    if (empty) return status_of(hipMemsetAsync(d_frame_offsets, 0, sizeof(uint64_t) * (n_frames + 1ull), s));
    return enqueue(ctx, d_frames, n_frames, width, height, frame_stride(n_frames, frame_stride_bytes, fb),
                   cfg, reinterpret_cast<uint2*>(d_out), cap, d_frame_offsets, s, rgb);
}

int fdf_detect_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                      uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                      const fdf_config* cfg, fdf_point* d_out, uint64_t cap,
                      uint64_t* d_frame_offsets, void* stream) {
    return detect_device(ctx, d_frames, n_frames, width, height, frame_stride_bytes, cfg, d_out, cap,
                         d_frame_offsets, stream, false);
}

int fdf_detect_device_rgb(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                          uint32_t width, uint32_t height, uint64_t frame_stride_bytes,
                          const fdf_config* cfg, fdf_point* d_out, uint64_t cap,
                          uint64_t* d_frame_offsets, void* stream) {
    return detect_device(ctx, d_frames, n_frames, width, height, frame_stride_bytes, cfg, d_out, cap,
                         d_frame_offsets, stream, true);
}

int fdf_score_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                     size_t stride_bytes, const fdf_config* cfg, const fdf_point* points,
                     size_t n_points, uint16_t* out_scores) {
    if (!ctx || !cfg || (n_points && (!points || !out_scores || !data))) return FDF_ERR_ARG;
    if (cfg->count < 9 || cfg->count > 16) return FDF_ERR_COUNT;
    if (cfg->nms != FDF_NMS_MAX_THRESHOLD && cfg->nms != FDF_NMS_SUM_ABSOLUTE) return FDF_ERR_NMS;
    if (stride_bytes < width || n_points > 0xffffffffull) return FDF_ERR_ARG;
    for (size_t k = 0; k < n_points; ++k) {
        const fdf_point p = points[k];
        if (p.x < 3 || p.y < 3 || (uint64_t)p.x + 3 >= width || (uint64_t)p.y + 3 >= height)
            return FDF_ERR_ARG;
    }
    if (n_points == 0) return FDF_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    const size_t frame_bytes = (size_t)width * height;
    ctx->last.valid = false;              // d_in / d_out are reused below
    wait_done(ctx);
    int rc;
    if ((rc = ensure(ctx, &ctx->d_in, &ctx->in_bytes, frame_bytes, ctx->stream))) return rc;
    if ((rc = ensure(ctx, &ctx->d_out, &ctx->out_points, n_points + (n_points + 3) / 4,
                     ctx->stream)))
        return rc;
    hipError_t e = upload_rows(ctx->d_in, data, stride_bytes, width, height, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ctx->d_out, points, n_points * sizeof(fdf_point), hipMemcpyHostToDevice,
                           ctx->stream);
    uint16_t* d_scores = reinterpret_cast<uint16_t*>(ctx->d_out + n_points);
    if (e == hipSuccess)
        e = fdfk::launch_score_points(ctx->d_in, width, ctx->d_out, (uint32_t)n_points, cfg->nms,
                                      cfg->threshold, cfg->count, d_scores, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_scores, d_scores, n_points * sizeof(uint16_t), hipMemcpyDeviceToHost,
                           ctx->stream);
    if (e == hipSuccess) e = sync_own_stream(ctx);
    return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
}

// ---- ring-level helpers (src/fast_simd.rs:69-110, :623, :722) ---------------------------

static constexpr int32_t kCircleDx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
static constexpr int32_t kCircleDy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};

void fdf_circle(int32_t dx[16], int32_t dy[16]) {
    for (int i = 0; i < 16; ++i) {
        if (dx) dx[i] = kCircleDx[i];
        if (dy) dy[i] = kCircleDy[i];
    }
}

void fdf_calculate_offsets(uint32_t width, int32_t offsets[16]) {
    if (!offsets) return;
    for (int i = 0; i < 16; ++i)   // same i32 arithmetic as the reference (wraps like it)
        offsets[i] = (int32_t)((uint32_t)kCircleDy[i] * width + (uint32_t)kCircleDx[i]);
}

static int check_ring_args(const fdf_config* cfg) {
    if (!cfg) return FDF_ERR_ARG;
    if (cfg->nms != FDF_NMS_MAX_THRESHOLD && cfg->nms != FDF_NMS_SUM_ABSOLUTE) return FDF_ERR_NMS;
    if (cfg->nms == FDF_NMS_MAX_THRESHOLD && (cfg->count < 9 || cfg->count > 16))
        return FDF_ERR_COUNT;
    return FDF_OK;
}

static inline uint8_t ring_count(const fdf_config* cfg) {
    return cfg->nms == FDF_NMS_MAX_THRESHOLD ? cfg->count : 9;   // SAD ignores the count
}

int fdf_score_rings_device(fdf_ctx* ctx, const uint8_t* d_centers, const uint8_t* d_rings,
                           uint64_t n_rings, const fdf_config* cfg, uint16_t* d_scores,
                           void* stream) {
    if (!ctx || n_rings > 0xffffffffull) return FDF_ERR_ARG;
    int rc = check_ring_args(cfg);
    if (rc) return rc;
    if (n_rings == 0) return FDF_OK;
    if (!d_centers || !d_rings || !d_scores || ((uintptr_t)d_rings & 15u)) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    // NULL = the HIP null stream, as for every device-pointer call (torch's default stream is
    // NULL: the context's own stream would not be ordered with it)
    const hipError_t e = fdfk::launch_score_rings(d_centers, d_rings, (uint32_t)n_rings, cfg->nms,
                                                  cfg->threshold, ring_count(cfg), d_scores,
                                                  reinterpret_cast<hipStream_t>(stream));
    return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
}

int fdf_score_rings(fdf_ctx* ctx, const uint8_t* centers, const uint8_t* rings, size_t n_rings,
                    const fdf_config* cfg, uint16_t* out_scores) {
    if (!ctx || n_rings > 0xffffffffull) return FDF_ERR_ARG;
    int rc = check_ring_args(cfg);
    if (rc) return rc;
    if (n_rings == 0) return FDF_OK;
    if (!centers || !rings || !out_scores) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ctx->last.valid = false;              // d_in / d_out are reused below
    wait_done(ctx);
    const size_t ring_bytes = n_rings * 16;
    if ((rc = ensure(ctx, &ctx->d_in, &ctx->in_bytes, ring_bytes + n_rings, ctx->stream))) return rc;
    if ((rc = ensure(ctx, &ctx->d_out, &ctx->out_points, (n_rings + 3) / 4, ctx->stream))) return rc;
    uint16_t* d_scores = reinterpret_cast<uint16_t*>(ctx->d_out);
    hipError_t e = hipMemcpyAsync(ctx->d_in, rings, ring_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ctx->d_in + ring_bytes, centers, n_rings, hipMemcpyHostToDevice,
                           ctx->stream);
    if (e == hipSuccess)
        e = fdfk::launch_score_rings(ctx->d_in + ring_bytes, ctx->d_in, (uint32_t)n_rings,
                                     cfg->nms, cfg->threshold, ring_count(cfg), d_scores,
                                     ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_scores, d_scores, n_rings * sizeof(uint16_t), hipMemcpyDeviceToHost,
                           ctx->stream);
    if (e == hipSuccess) e = sync_own_stream(ctx);
    return e == hipSuccess ? FDF_OK : FDF_ERR_DEVICE;
}

// ---- multi-device batch: contiguous frame shards, one host thread per context ----------

int fdf_detect_batch_multi(fdf_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* data,
                           uint32_t n_frames, uint32_t width, uint32_t height,
                           size_t frame_stride_bytes, const fdf_config* cfg, fdf_point* out,
                           size_t cap, uint64_t* frame_offsets, size_t* n_out) {
    if (!ctxs || n_ctx == 0 || n_ctx > 1024 || !n_out || (cap && !out)) return FDF_ERR_ARG;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        if (!ctxs[k]) return FDF_ERR_ARG;
        for (uint32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return FDF_ERR_ARG;   // each shard needs its own workspace
    }
    if (n_frames > 1 && frame_stride_bytes < (size_t)width * height) return FDF_ERR_ARG;
    int empty = 0;
    int rc = check_host_args(data, n_frames, width, height, width, cfg, false, &empty);
    if (rc) return rc;
    std::vector<uint64_t> offs(n_frames + 1ull, 0);
    const auto locks = lock_all(ctxs, n_ctx);                     // held throughout
    const uint64_t gen = ++g_multi_gen;
    auto tag = [&](uint32_t k) {
        ctxs[k]->last.multi_gen = gen;
        ctxs[k]->last.shard = k;
        ctxs[k]->last.nshards = n_ctx;
    };
    if (empty) {
        for (uint32_t k = 0; k < n_ctx; ++k) {
            ctxs[k]->last = LastResult{};
            ctxs[k]->last.valid = true;
            ctxs[k]->last.cfg = *cfg;
            tag(k);
        }
        *n_out = 0;
        if (frame_offsets) std::memset(frame_offsets, 0, sizeof(uint64_t) * (n_frames + 1ull));
        return FDF_OK;
    }
    // shard k: frames [first[k], first[k+1]) (contiguous, sizes differ by at most one)
    std::vector<uint32_t> first(n_ctx + 1);
    for (uint32_t k = 0; k <= n_ctx; ++k) first[k] = (uint32_t)((uint64_t)n_frames * k / n_ctx);
    std::vector<std::vector<uint64_t>> local(n_ctx);
    std::vector<int> status(n_ctx, FDF_OK);
    auto detect_shard = [&](uint32_t k) {
        fdf_ctx* ctx = ctxs[k];
        const uint32_t nf = first[k + 1] - first[k];
        ctx->last = LastResult{};
        if (nf == 0) {
            ctx->last.valid = true;
            ctx->last.cfg = *cfg;
            return;
        }
        DeviceGuard guard(ctx->device);
        local[k].assign(nf + 1ull, 0);
        status[k] = run_host(ctx, data + (size_t)first[k] * frame_stride_bytes, nf, width, height,
                             width, frame_stride_bytes, cfg, false, local[k].data(), true);
    };
    auto run_all = [&](auto&& fn) {
        std::vector<std::thread> pool;
        for (uint32_t k = 1; k < n_ctx; ++k) pool.emplace_back(fn, k);
        fn(0u);
        for (auto& t : pool) t.join();
    };
    run_all(detect_shard);
    for (uint32_t k = 0; k < n_ctx; ++k)
        if (status[k]) return status[k];
    for (uint32_t k = 0; k < n_ctx; ++k) tag(k);
    // global offsets: shard k's points follow shards 0 .. k-1
    std::vector<uint64_t> base(n_ctx + 1, 0);
    for (uint32_t k = 0; k < n_ctx; ++k) {
        const uint32_t nf = first[k + 1] - first[k];
        for (uint32_t f = 0; f < nf; ++f) offs[first[k] + f] = base[k] + local[k][f];
        base[k + 1] = base[k] + (nf ? local[k][nf] : 0);
    }
    const uint64_t total = base[n_ctx];
    offs[n_frames] = total;
    if (frame_offsets) std::memcpy(frame_offsets, offs.data(), sizeof(uint64_t) * (n_frames + 1ull));
    auto copy_shard = [&](uint32_t k) {
        const uint64_t b = std::min<uint64_t>(base[k], cap), e = std::min<uint64_t>(base[k + 1], cap);
        if (e <= b) return;
        DeviceGuard guard(ctxs[k]->device);
        status[k] = copy_out(ctxs[k], out + b, nullptr, (size_t)(e - b));
    };
    run_all(copy_shard);
    for (uint32_t k = 0; k < n_ctx; ++k)
        if (status[k]) return status[k];
    *n_out = (size_t)total;
    return total > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

int fdf_fetch_last_multi(fdf_ctx* const* ctxs, uint32_t n_ctx, fdf_point* out, size_t cap,
                         size_t* n_out) {
    if (!ctxs || n_ctx == 0 || n_ctx > 1024 || !n_out || (cap && !out)) return FDF_ERR_ARG;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        if (!ctxs[k]) return FDF_ERR_ARG;
        for (uint32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return FDF_ERR_ARG;
    }
    const auto locks = lock_all(ctxs, n_ctx);
    // the results must be the shards of ONE fdf_detect_batch_multi call, in its order (a
    // host call on one of the contexts since then, or a reordered array, is an error)
    const uint64_t gen = ctxs[0]->last.multi_gen;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        const LastResult& L = ctxs[k]->last;
        if (!L.valid || gen == 0 || L.multi_gen != gen || L.shard != k || L.nshards != n_ctx)
            return FDF_ERR_ARG;
    }
    uint64_t b = 0;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        const uint64_t n = ctxs[k]->last.total;
        const uint64_t lo = std::min<uint64_t>(b, cap), hi = std::min<uint64_t>(b + n, cap);
        if (hi > lo) {
            DeviceGuard guard(ctxs[k]->device);
            const int rc = copy_out(ctxs[k], out + lo, nullptr, (size_t)(hi - lo));
            if (rc) return rc;
        }
        b += n;
    }
    *n_out = (size_t)b;
    return b > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

#ifdef FDF_DEBUG_BUILD
// Debug builds only (not in include/fdf.h): the last detector launch's workgroup stamps,
// fdfk::kStampWords words per workgroup in blockIdx order (tools/stamps.py).
int fdf_debug_stamps(fdf_ctx* ctx, uint64_t* out, uint64_t cap_words, uint64_t* n_words) {
    if (!ctx || !n_words) return FDF_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    *n_words = ctx->stamps_used;
    if (!ctx->d_stamps || !out) return FDF_OK;
    wait_done(ctx);
    const size_t n = (size_t)std::min<uint64_t>(cap_words, ctx->stamps_used);
    return hipMemcpy(out, ctx->d_stamps, n * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess
               ? FDF_OK
               : FDF_ERR_DEVICE;
}
#endif

}  // extern "C"
