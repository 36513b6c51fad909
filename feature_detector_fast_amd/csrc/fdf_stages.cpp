// fdf_stages.cpp -- the C ABI of the stages behind the detector (extensions: the reference
// returns points only): best-K selection, orientation, Harris response, steered BRIEF descriptors, box
// smoothing, descriptor matching, RANSAC model estimation, the resize behind the scale pyramid, the warp by the estimated
// models, Lucas-Kanade tracking and the track-set maintenance between two tracking calls.  Each has an asynchronous _device entry on the caller's stream and memory and a
// host convenience _points entry.  Of a context they use the device, the mutex and the
// stream only: its workspace and retained result (fdf_fetch_last) are not touched.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "fdf_ctx.h"

namespace {

// One device allocation for a _points call, cut into 256-byte aligned parts.  In order:
// declare the parts, open(), transfers and kernels on the context's stream (which carries the
// call: its mutex is held and its device current while the arena lives), close().  The first
// error of a transfer or kernel is kept and skips the transfers after it.
class Arena {
public:
    template <typename T>
    struct Part { uint64_t offset, count; };

    explicit Arena(fdf_ctx* ctx) : ctx_(ctx), lock_(ctx->mu), guard_(ctx->device) {}
    ~Arena() { (void)close(); }

    template <typename T>
    Part<T> part(uint64_t count) {    // a size no allocation can have makes open() fail
        const Part<T> p{bytes_, count};
        bytes_ = count > (~0ull - bytes_ - 256u) / sizeof(T) ? ~0ull - 256u
                                                             : bytes_ + align256(count * sizeof(T));
        return p;
    }
    int open() {
        if (hipMalloc(reinterpret_cast<void**>(&d_), bytes_) == hipSuccess) return FDF_OK;
        (void)hipGetLastError();
        d_ = nullptr;
        return FDF_ERR_ALLOC;
    }
    template <typename T>
    T* at(Part<T> p) const { return reinterpret_cast<T*>(d_ + p.offset); }
    bool ok() const { return e_ == hipSuccess; }
    void note(hipError_t e) { if (ok()) e_ = e; }
    template <typename T>
    void upload(Part<T> p, const T* src) {
        if (ok()) e_ = hipMemcpyAsync(at(p), src, p.count * sizeof(T), hipMemcpyHostToDevice, ctx_->stream);
    }
    template <typename T>
    void download(T* dst, Part<T> p, uint64_t count) {
        if (ok()) e_ = hipMemcpyAsync(dst, at(p), count * sizeof(T), hipMemcpyDeviceToHost, ctx_->stream);
    }
    // a frame whose rows lie `stride_bytes` apart, packed on the device
    void upload_frame(Part<uint8_t> p, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes) {
        if (ok()) e_ = upload_rows(at(p), data, stride_bytes, width, height, ctx_->stream);
    }
    // a packed device frame to rows `stride_bytes` apart
    void download_frame(uint8_t* out, Part<uint8_t> p, uint32_t width, uint32_t height,
                        size_t stride_bytes) {
        if (ok()) e_ = download_rows(out, stride_bytes, at(p), width, height, ctx_->stream);
    }
    void upload_one_frame(Part<uint64_t> p, uint64_t n_points) {    // offsets {0, n_points}
        one_frame_[1] = n_points;
        upload(p, one_frame_);
    }
    // Drains the stream (nothing may still use the allocation) and frees; FDF_ERR_DEVICE
    // after any failed transfer or kernel.
    int close() {
        if (d_) {
            note(hipStreamSynchronize(ctx_->stream));
            (void)hipFree(d_);
            d_ = nullptr;
        }
        return ok() ? FDF_OK : FDF_ERR_DEVICE;
    }

private:
    fdf_ctx* ctx_;
    std::lock_guard<std::mutex> lock_;
    DeviceGuard guard_;
    uint8_t* d_ = nullptr;
    uint64_t bytes_ = 0;
    hipError_t e_ = hipSuccess;
    uint64_t one_frame_[2] = {0, 0};    // an asynchronous copy's source: lives as long as the call
};

bool points_inside(const fdf_point* points, size_t n_points, uint32_t width, uint32_t height) {
    for (size_t k = 0; k < n_points; ++k)
        if (points[k].x >= width || points[k].y >= height) return false;
    return true;
}

// What fdf_orient_device and fdf_describe_device check after their own parameters.  *todo is
// clear when the call is valid and has nothing to enqueue; otherwise *stride is the frames'.
inline int check_point_frames(uint32_t n_frames, uint32_t width, uint32_t height, uint64_t cap,
                              uint64_t stride_bytes, bool have_ptrs, uint64_t* stride, bool* todo) {
    *todo = false;
    int empty = 0;
    const int rc = check_shape(width, height, &empty);
    if (rc) return rc;
    if (empty || n_frames == 0 || cap == 0) return FDF_OK;
    if (!have_ptrs) return FDF_ERR_ARG;
    const uint64_t frame_bytes = (uint64_t)width * height;
    if (frame_bytes > fdfk::kOrientMaxPixels) return FDF_ERR_SIZE;
    *stride = frame_stride(n_frames, stride_bytes, frame_bytes);
    *todo = *stride >= frame_bytes;
    return *todo ? FDF_OK : FDF_ERR_ARG;
}

// Workgroups per frame of a point-list kernel: about `per_wg` points each at the detector's
// usual density, `max_chunks` at most.
inline uint32_t chunks_per_frame(uint64_t cap, uint32_t n_frames, uint32_t width, uint32_t height,
                                 uint32_t per_wg, uint32_t max_chunks) {
    const uint64_t est = std::min<uint64_t>(cap, (uint64_t)width * height / 32 * n_frames);
    return (uint32_t)std::min<uint64_t>(max_chunks, est / n_frames / per_wg + 1);
}

}  // namespace

extern "C" {

// ---- best-K selection per grid cell (fdf_select.hip) -------------------------------------
namespace {

// Scratch of one fdf_select_device call, every part 256-byte aligned: the per-frame kept
// totals (zeroed on the stream before the kernels), the kept count and the index range of
// every (frame, cell row), and `cap` keep flags for a caller that passes no d_keep.
struct SelectLayout {
    uint32_t cw = 0, ch = 0, cells_x = 0, rows = 0;
    uint64_t frame_tot = 0, row_cnt = 0, row_range = 0, keep = 0, total = 0;
};

// FDF_OK with *empty set for shapes with no keypoints; the shape's error otherwise.
int select_layout(uint32_t n_frames, uint32_t width, uint32_t height, uint32_t cell_w,
                  uint32_t cell_h, uint64_t cap, SelectLayout* L, int* empty) {
    int rc = check_shape(width, height, empty);
    if (rc) return rc;
    if (n_frames > 65535u || (uint64_t)width * height > 0xffffffffull) return FDF_ERR_ARG;
    if (n_frames == 0) *empty = 1;
    if (*empty) return FDF_OK;
    L->cw = cell_w == 0 || cell_w > width ? width : cell_w;
    L->ch = cell_h == 0 || cell_h > height ? height : cell_h;
    L->cells_x = (width + L->cw - 1) / L->cw;
    L->rows = (height + L->ch - 1) / L->ch;
    if (L->rows > fdfk::kSelMaxRows) return FDF_ERR_ARG;
    const uint64_t nrows = (uint64_t)n_frames * L->rows;
    L->frame_tot = 0;
    L->row_cnt = align256(sizeof(uint64_t) * n_frames);
    L->row_range = L->row_cnt + align256(sizeof(uint32_t) * nrows);
    L->keep = L->row_range + align256(2 * sizeof(uint64_t) * nrows);
    if (cap > ~0ull - L->keep - 256u) return FDF_ERR_ARG;
    L->total = L->keep + align256(cap);
    return FDF_OK;
}

}  // namespace

int fdf_select_scratch_bytes(uint32_t n_frames, uint32_t width, uint32_t height,
                             uint32_t cell_w, uint32_t cell_h, uint64_t cap, uint64_t* bytes) {
    if (!bytes) return FDF_ERR_ARG;
    SelectLayout L;
    int empty = 0;
    const int rc = select_layout(n_frames, width, height, cell_w, cell_h, cap, &L, &empty);
    if (rc) return rc;
    *bytes = empty ? 0 : L.total;
    return FDF_OK;
}

int fdf_select_device(fdf_ctx* ctx, uint32_t n_frames, uint32_t width, uint32_t height,
                      const fdf_point* d_points, const uint16_t* d_scores, uint64_t cap,
                      const uint64_t* d_frame_offsets, uint32_t cell_w, uint32_t cell_h,
                      uint32_t k, fdf_point* d_sel, uint16_t* d_sel_scores, uint64_t sel_cap,
                      uint64_t* d_sel_offsets, uint8_t* d_keep, void* d_scratch,
                      uint64_t scratch_bytes, void* stream) {
    if (!ctx || !d_sel_offsets || k == 0) return FDF_ERR_ARG;
    SelectLayout L;
    int empty = 0;
    const int rc = select_layout(n_frames, width, height, cell_w, cell_h, cap, &L, &empty);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);   // NULL = the HIP null stream
    if (!empty) {
        if (!d_frame_offsets || !d_scratch || scratch_bytes < L.total ||
            ((uintptr_t)d_scratch & 255u) != 0)
            return FDF_ERR_ARG;
        if (cap && (!d_points || !d_scores)) return FDF_ERR_ARG;
        if (sel_cap && (!d_sel || !d_sel_scores)) return FDF_ERR_ARG;
    }
    DeviceGuard guard(ctx->device);
    if (empty || cap == 0)
        return status_of(hipMemsetAsync(d_sel_offsets, 0, sizeof(uint64_t) * (n_frames + 1ull), s));
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    fdfk::SelectParams p{};
    p.pts = reinterpret_cast<const uint2*>(d_points);
    p.scores = d_scores;
    p.offs = d_frame_offsets;
    p.cap = cap;
    p.n_frames = n_frames;
    p.cw = L.cw;
    p.ch = L.ch;
    p.cells_x = L.cells_x;
    p.rows = L.rows;
    p.k = k;
    p.keep = d_keep ? d_keep : base + L.keep;
    p.frame_tot = reinterpret_cast<uint64_t*>(base + L.frame_tot);
    p.row_cnt = reinterpret_cast<uint32_t*>(base + L.row_cnt);
    p.row_range = reinterpret_cast<uint64_t*>(base + L.row_range);
    p.sel = reinterpret_cast<uint2*>(d_sel);
    p.sel_scores = d_sel_scores;
    p.sel_cap = sel_cap;
    p.sel_offs = d_sel_offsets;
    // the frame totals are summed into; the keep flags of indices no frame owns stay 0
    hipError_t e = hipMemsetAsync(p.frame_tot, 0, sizeof(uint64_t) * n_frames, s);
    if (e == hipSuccess) e = hipMemsetAsync(p.keep, 0, cap, s);
    if (e == hipSuccess) e = fdfk::launch_select(p, s);
    return status_of(e);
}

int fdf_select_points(fdf_ctx* ctx, const fdf_point* points, const uint16_t* scores,
                      const uint64_t* frame_offsets, uint32_t n_frames, size_t n_points,
                      uint32_t width, uint32_t height, uint32_t cell_w, uint32_t cell_h,
                      uint32_t k, fdf_point* out, uint16_t* out_scores, size_t cap,
                      uint64_t* out_offsets, size_t* n_out) {
    if (!ctx || !n_out || k == 0) return FDF_ERR_ARG;
    if (n_points && (!points || !scores)) return FDF_ERR_ARG;
    if (cap && (!out || !out_scores)) return FDF_ERR_ARG;
    if (!frame_offsets && n_frames != 1) return FDF_ERR_ARG;
    SelectLayout L;
    int empty = 0;
    const int rc = select_layout(n_frames, width, height, cell_w, cell_h, n_points, &L, &empty);
    if (rc) return rc;
    *n_out = 0;
    const uint64_t noffs = n_frames + 1ull;
    if (empty || n_points == 0) {
        if (out_offsets) std::memset(out_offsets, 0, sizeof(uint64_t) * noffs);
        return FDF_OK;
    }
    Arena a(ctx);
    const auto d_pts = a.part<fdf_point>(n_points);
    const auto d_scores = a.part<uint16_t>(n_points);
    const auto d_offs = a.part<uint64_t>(noffs);
    const auto d_sel = a.part<fdf_point>(cap);
    const auto d_sel_scores = a.part<uint16_t>(cap);
    const auto d_sel_offs = a.part<uint64_t>(noffs);
    const auto d_scratch = a.part<uint8_t>(L.total);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload(d_pts, points);
    a.upload(d_scores, scores);
    if (frame_offsets) a.upload(d_offs, frame_offsets);
    else a.upload_one_frame(d_offs, n_points);
    if (a.ok()) {
        const int status = fdf_select_device(
            ctx, n_frames, width, height, a.at(d_pts), a.at(d_scores), n_points, a.at(d_offs),
            cell_w, cell_h, k, a.at(d_sel), a.at(d_sel_scores), cap, a.at(d_sel_offs), nullptr,
            a.at(d_scratch), L.total, ctx->stream);
        if (status != FDF_OK) return status;
    }
    // two phases: the offsets tell how many points to copy
    std::vector<uint64_t> offs(noffs);
    a.download(offs.data(), d_sel_offs, noffs);
    a.note(hipStreamSynchronize(ctx->stream));
    const uint64_t total = a.ok() ? offs[n_frames] : 0;
    const uint64_t ncopy = std::min<uint64_t>(total, cap);
    if (ncopy) {
        a.download(out, d_sel, ncopy);
        a.download(out_scores, d_sel_scores, ncopy);
    }
    if (a.close() != FDF_OK) return FDF_ERR_DEVICE;
    *n_out = (size_t)total;
    if (out_offsets) std::memcpy(out_offsets, offs.data(), noffs * sizeof(uint64_t));
    return total > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

// ---- orientation by intensity centroid (fdf_orient.hip) ---------------------------------

int fdf_orient_disc(uint32_t radius, uint8_t* half_widths) {
    if (radius == 0 || radius > fdfk::kOrientMaxRadius || !half_widths) return FDF_ERR_ARG;
    // OpenCV's umax: the rounded circle for the rows up to r / sqrt(2), mirrored for the rest
    // so that the disc is symmetric about its diagonal
    const int r = (int)radius;
    const int vmax = (int)std::floor(r * std::sqrt(2.0) / 2 + 1);
    const int vmin = (int)std::ceil(r * std::sqrt(2.0) / 2);
    int u[fdfk::kOrientMaxRadius + 2] = {0};
    for (int v = 0; v <= vmax; ++v)
        u[v] = (int)std::floor(std::sqrt((double)r * r - (double)v * v) + 0.5);
    for (int v = r, v0 = 0; v >= vmin; --v) {
        while (u[v0] == u[v0 + 1]) ++v0;
        u[v] = v0;
        ++v0;
    }
    for (int v = 0; v <= r; ++v) half_widths[v] = (uint8_t)u[v];
    return FDF_OK;
}

namespace {

// The launch of fdf_orient_device / fdf_orient_points (arguments already validated).
hipError_t orient_enqueue(const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                          uint32_t height, uint64_t frame_stride, const fdf_point* d_points,
                          uint64_t cap, const uint64_t* d_offsets, uint32_t radius,
                          float* d_angles, int32_t* d_moments, hipStream_t s) {
    fdfk::OrientParams p{};
    p.frames = d_frames;
    p.frame_stride = frame_stride;
    p.pts = reinterpret_cast<const uint2*>(d_points);
    p.offs = d_offsets;
    p.cap = cap;
    p.n_frames = n_frames;
    p.width = width;
    p.height = height;
    p.radius = radius;
    p.angles = d_angles;
    p.moments = d_moments;
    if (fdf_orient_disc(radius, p.u) != FDF_OK) return hipErrorInvalidValue;
    return fdfk::launch_orient(p, chunks_per_frame(cap, n_frames, width, height, 256, 256), s);
}

}  // namespace

int fdf_orient_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                      uint64_t cap, const uint64_t* d_frame_offsets, uint32_t radius,
                      float* d_angles, int32_t* d_moments, void* stream) {
    if (!ctx || !d_frame_offsets || radius == 0 || radius > fdfk::kOrientMaxRadius ||
        n_frames > 65535u)
        return FDF_ERR_ARG;
    uint64_t fs = 0;
    bool todo = false;
    const int rc = check_point_frames(n_frames, width, height, cap, frame_stride_bytes,
                                      d_frames && d_points && d_angles, &fs, &todo);
    if (!todo) return rc;
    DeviceGuard guard(ctx->device);
    return status_of(orient_enqueue(d_frames, n_frames, width, height, fs, d_points, cap,
                                    d_frame_offsets, radius, d_angles, d_moments,
                                    reinterpret_cast<hipStream_t>(stream)));
}

int fdf_orient_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_point* points, size_t n_points,
                      uint32_t radius, float* out_angles, int32_t* out_moments) {
    if (!ctx || radius == 0 || radius > fdfk::kOrientMaxRadius) return FDF_ERR_ARG;
    if (n_points && (!points || !out_angles || !data)) return FDF_ERR_ARG;
    if (stride_bytes < width) return FDF_ERR_ARG;
    if (!points_inside(points, n_points, width, height)) return FDF_ERR_ARG;
    if (n_points == 0) return FDF_OK;
    const uint64_t frame_bytes = (uint64_t)width * height;
    if (frame_bytes > fdfk::kOrientMaxPixels) return FDF_ERR_SIZE;
    Arena a(ctx);
    const auto d_frame = a.part<uint8_t>(frame_bytes);
    const auto d_pts = a.part<fdf_point>(n_points);
    const auto d_offs = a.part<uint64_t>(2);
    const auto d_ang = a.part<float>(n_points);
    const auto d_mom = a.part<int32_t>(out_moments ? 2 * (uint64_t)n_points : 0);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload_frame(d_frame, data, width, height, stride_bytes);
    a.upload(d_pts, points);
    a.upload_one_frame(d_offs, n_points);
    if (a.ok())
        a.note(orient_enqueue(a.at(d_frame), 1, width, height, frame_bytes, a.at(d_pts), n_points,
                              a.at(d_offs), radius, a.at(d_ang),
                              out_moments ? a.at(d_mom) : nullptr, ctx->stream));
    a.download(out_angles, d_ang, n_points);
    if (out_moments) a.download(out_moments, d_mom, d_mom.count);
    return a.close();
}

// ---- Harris corner response (fdf_harris.hip) ---------------------------------------------

int fdf_harris_codes(const int64_t* responses, size_t n, uint16_t* codes) {
    if (n && (!responses || !codes)) return FDF_ERR_ARG;
    for (size_t k = 0; k < n; ++k) codes[k] = fdfk::harris_code(responses[k]);
    return FDF_OK;
}

namespace {

inline bool harris_args_ok(uint32_t block, uint32_t k_num, uint32_t k_den) {
    return fdfk::harris_block_ok(block) && k_num <= fdfk::kHarrisMaxK && k_den >= 1 &&
           k_den <= fdfk::kHarrisMaxK;
}

// The launch of fdf_harris_device / fdf_harris_points (arguments already validated).
hipError_t harris_enqueue(const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                          uint32_t height, uint64_t frame_stride, const fdf_point* d_points,
                          uint64_t cap, const uint64_t* d_offsets, uint32_t block, uint32_t k_num,
                          uint32_t k_den, uint16_t* d_scores, int64_t* d_responses,
                          hipStream_t s) {
    fdfk::HarrisParams p{};
    p.frames = d_frames;
    p.frame_stride = frame_stride;
    p.pts = reinterpret_cast<const uint2*>(d_points);
    p.offs = d_offsets;
    p.cap = cap;
    p.n_frames = n_frames;
    p.width = width;
    p.height = height;
    p.block = block;
    p.k_num = k_num;
    p.k_den = k_den;
    p.scores = d_scores;
    p.responses = d_responses;
    return fdfk::launch_harris(p, chunks_per_frame(cap, n_frames, width, height, 256, 256), s);
}

}  // namespace

int fdf_harris_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                      uint64_t cap, const uint64_t* d_frame_offsets, uint32_t block,
                      uint32_t k_num, uint32_t k_den, uint16_t* d_scores, int64_t* d_responses,
                      void* stream) {
    if (!ctx || !d_frame_offsets || !harris_args_ok(block, k_num, k_den) || n_frames > 65535u ||
        ((uintptr_t)d_responses & 7u) != 0)
        return FDF_ERR_ARG;
    uint64_t fs = 0;
    bool todo = false;
    const int rc = check_point_frames(n_frames, width, height, cap, frame_stride_bytes,
                                      d_frames && d_points && d_scores, &fs, &todo);
    if (!todo) return rc;
    DeviceGuard guard(ctx->device);
    return status_of(harris_enqueue(d_frames, n_frames, width, height, fs, d_points, cap,
                                    d_frame_offsets, block, k_num, k_den, d_scores, d_responses,
                                    reinterpret_cast<hipStream_t>(stream)));
}

int fdf_harris_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                      size_t stride_bytes, const fdf_point* points, size_t n_points,
                      uint32_t block, uint32_t k_num, uint32_t k_den, uint16_t* out_scores,
                      int64_t* out_responses) {
    if (!ctx || !harris_args_ok(block, k_num, k_den)) return FDF_ERR_ARG;
    if (n_points && (!points || !out_scores || !data)) return FDF_ERR_ARG;
    if (stride_bytes < width) return FDF_ERR_ARG;
    if (!points_inside(points, n_points, width, height)) return FDF_ERR_ARG;
    if (n_points == 0) return FDF_OK;
    const uint64_t frame_bytes = (uint64_t)width * height;
    if (frame_bytes > fdfk::kOrientMaxPixels) return FDF_ERR_SIZE;
    Arena a(ctx);
    const auto d_frame = a.part<uint8_t>(frame_bytes);
    const auto d_pts = a.part<fdf_point>(n_points);
    const auto d_offs = a.part<uint64_t>(2);
    const auto d_sc = a.part<uint16_t>(n_points);
    const auto d_resp = a.part<int64_t>(out_responses ? n_points : 0);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload_frame(d_frame, data, width, height, stride_bytes);
    a.upload(d_pts, points);
    a.upload_one_frame(d_offs, n_points);
    if (a.ok())
        a.note(harris_enqueue(a.at(d_frame), 1, width, height, frame_bytes, a.at(d_pts), n_points,
                              a.at(d_offs), block, k_num, k_den, a.at(d_sc),
                              out_responses ? a.at(d_resp) : nullptr, ctx->stream));
    a.download(out_scores, d_sc, n_points);
    if (out_responses) a.download(out_responses, d_resp, d_resp.count);
    return a.close();
}

// ---- steered BRIEF descriptors and box smoothing (fdf_describe.hip) -----------------------

int fdf_brief_pattern(int8_t pattern[1024]) {
    if (!pattern) return FDF_ERR_ARG;
    uint32_t s = 0x9E3779B9u;
    auto next = [&s]() {
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        return s;
    };
    auto coord = [&next]() {              // bell-shaped in -21..21
        int v = -21;
        for (int k = 0; k < 6; ++k) v += (int)(next() >> 29);
        return v;
    };
    uint32_t n = 0;
    while (n < fdfk::kBriefTests) {
        int t[4];
        for (int& v : t) v = coord();
        if (t[0] * t[0] + t[1] * t[1] > 13 * 13 || t[2] * t[2] + t[3] * t[3] > 13 * 13) continue;
        if (t[0] == t[2] && t[1] == t[3]) continue;
        bool seen = false;
        for (uint32_t k = 0; k < n && !seen; ++k)
            seen = pattern[4 * k] == t[0] && pattern[4 * k + 1] == t[1] &&
                   pattern[4 * k + 2] == t[2] && pattern[4 * k + 3] == t[3];
        if (seen) continue;
        for (int k = 0; k < 4; ++k) pattern[4 * n + k] = (int8_t)t[k];
        ++n;
    }
    return FDF_OK;
}

int fdf_brief_steer(const int8_t* pattern, uint32_t n_bins, int8_t* table) {
#pragma clang fp contract(off)
    if (!pattern || !table || n_bins == 0 || n_bins > fdfk::kBriefMaxBins) return FDF_ERR_ARG;
    // double products and sums, one rounding to float, then half away from zero
    auto quantise = [](double v) {
        const float r = std::round((float)v);
        return (int8_t)std::min(std::max(r, -128.0f), 127.0f);
    };
    for (uint32_t b = 0; b < n_bins; ++b) {
        const double theta = 2 * M_PI * b / n_bins;
        const double c = std::cos(theta), s = std::sin(theta);
        int8_t* row = table + (size_t)b * fdfk::kBriefTableBytes;
        for (uint32_t k = 0; k < 2 * fdfk::kBriefTests; ++k) {    // points (x, y), y pointing down
            const double x = pattern[2 * k], y = pattern[2 * k + 1];
            const double xc = x * c, ys = y * s, xs = x * s, yc = y * c;
            row[2 * k] = quantise(xc - ys);
            row[2 * k + 1] = quantise(xs + yc);
        }
    }
    return FDF_OK;
}

namespace {

hipError_t smooth_enqueue(const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                          uint32_t height, uint64_t frame_stride, uint8_t* d_out,
                          uint64_t out_stride, hipStream_t s) {
    fdfk::SmoothParams p{};
    p.frames = d_frames;
    p.frame_stride = frame_stride;
    p.out = d_out;
    p.out_stride = out_stride;
    p.n_frames = n_frames;
    p.width = width;
    p.height = height;
    p.groups = (width + 3) / 4;
    // the tallest strips (4 halo rows read per strip) that still leave 16 waves per CU
    p.strip_rows = fdfk::kSmoothStripRows;
    while (p.strip_rows > 8 &&
           (uint64_t)p.groups * ((height + p.strip_rows - 1) / p.strip_rows) * n_frames < 256 * 1024)
        p.strip_rows /= 2;
    p.strips = (height + p.strip_rows - 1) / p.strip_rows;
    return fdfk::launch_smooth(p, s);
}

// The launch of fdf_describe_device / fdf_describe_points (arguments already validated).
hipError_t describe_enqueue(const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                            uint32_t height, uint64_t frame_stride, const fdf_point* d_points,
                            uint64_t cap, const uint64_t* d_offsets, const float* d_angles,
                            const int8_t* d_table, uint32_t n_bins, uint8_t* d_desc,
                            hipStream_t s) {
    fdfk::DescribeParams p{};
    p.frames = d_frames;
    p.frame_stride = frame_stride;
    p.pts = reinterpret_cast<const uint2*>(d_points);
    p.offs = d_offsets;
    p.cap = cap;
    p.n_frames = n_frames;
    p.width = width;
    p.height = height;
    p.angles = d_angles;
    p.table = d_table;
    p.n_bins = n_bins;
    p.scale = (float)(n_bins / (2 * M_PI));
    p.desc = d_desc;
    return fdfk::launch_describe(p, chunks_per_frame(cap, n_frames, width, height, 64, 1024), s);
}

}  // namespace

int fdf_smooth_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                      uint32_t height, uint64_t frame_stride_bytes, uint8_t* d_out,
                      uint64_t out_frame_stride_bytes, void* stream) {
    const uint64_t frame_bytes = (uint64_t)width * height;
    if (!ctx || n_frames > 65535u) return FDF_ERR_ARG;
    if (frame_bytes == 0 || frame_bytes > fdfk::kOrientMaxPixels) return FDF_ERR_SIZE;
    if (n_frames == 0) return FDF_OK;
    if (!d_frames || !d_out) return FDF_ERR_ARG;
    const uint64_t fs = frame_stride(n_frames, frame_stride_bytes, frame_bytes);
    const uint64_t os = frame_stride(n_frames, out_frame_stride_bytes, frame_bytes);
    if (fs < frame_bytes || os < frame_bytes) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    return status_of(smooth_enqueue(d_frames, n_frames, width, height, fs, d_out, os,
                                    reinterpret_cast<hipStream_t>(stream)));
}

int fdf_describe_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames, uint32_t width,
                        uint32_t height, uint64_t frame_stride_bytes, const fdf_point* d_points,
                        uint64_t cap, const uint64_t* d_frame_offsets, const float* d_angles,
                        const int8_t* d_table, uint32_t n_bins, uint8_t* d_desc, void* stream) {
    if (!ctx || !d_frame_offsets || !d_table || n_bins == 0 || n_bins > fdfk::kBriefMaxBins ||
        n_frames > 65535u)
        return FDF_ERR_ARG;
    uint64_t fs = 0;
    bool todo = false;
    const int rc = check_point_frames(n_frames, width, height, cap, frame_stride_bytes,
                                      d_frames && d_points && d_desc, &fs, &todo);
    if (!todo) return rc;
    DeviceGuard guard(ctx->device);
    return status_of(describe_enqueue(d_frames, n_frames, width, height, fs, d_points, cap,
                                      d_frame_offsets, d_angles, d_table, n_bins, d_desc,
                                      reinterpret_cast<hipStream_t>(stream)));
}

int fdf_describe_points(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                        size_t stride_bytes, const fdf_point* points, size_t n_points,
                        const float* angles, const int8_t* pattern, uint32_t n_bins, int smooth,
                        uint8_t* out_desc) {
    if (!ctx || n_bins == 0 || n_bins > fdfk::kBriefMaxBins || (smooth != 0 && smooth != 1))
        return FDF_ERR_ARG;
    if (n_points && (!points || !out_desc || !data)) return FDF_ERR_ARG;
    if (stride_bytes < width) return FDF_ERR_ARG;
    if (!points_inside(points, n_points, width, height)) return FDF_ERR_ARG;
    if (n_points == 0) return FDF_OK;
    const uint64_t frame_bytes = (uint64_t)width * height;
    if (frame_bytes > fdfk::kOrientMaxPixels) return FDF_ERR_SIZE;
    int8_t default_pattern[fdfk::kBriefTableBytes];
    if (!pattern) {
        fdf_brief_pattern(default_pattern);
        pattern = default_pattern;
    }
    std::vector<int8_t> table((size_t)n_bins * fdfk::kBriefTableBytes);
    if (fdf_brief_steer(pattern, n_bins, table.data()) != FDF_OK) return FDF_ERR_ARG;
    Arena a(ctx);
    const auto d_frame = a.part<uint8_t>(frame_bytes);
    const auto d_smooth = a.part<uint8_t>(smooth ? frame_bytes : 0);
    const auto d_pts = a.part<fdf_point>(n_points);
    const auto d_offs = a.part<uint64_t>(2);
    const auto d_ang = a.part<float>(angles ? n_points : 0);
    const auto d_table = a.part<int8_t>(table.size());
    const auto d_desc = a.part<uint8_t>(n_points * (uint64_t)fdfk::kBriefBytes);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload_frame(d_frame, data, width, height, stride_bytes);
    a.upload(d_pts, points);
    a.upload_one_frame(d_offs, n_points);
    if (angles) a.upload(d_ang, angles);
    a.upload(d_table, table.data());
    if (a.ok() && smooth)
        a.note(smooth_enqueue(a.at(d_frame), 1, width, height, frame_bytes, a.at(d_smooth),
                              frame_bytes, ctx->stream));
    if (a.ok())
        a.note(describe_enqueue(a.at(smooth ? d_smooth : d_frame), 1, width, height, frame_bytes,
                                a.at(d_pts), n_points, a.at(d_offs),
                                angles ? a.at(d_ang) : nullptr, a.at(d_table), n_bins,
                                a.at(d_desc), ctx->stream));
    a.download(out_desc, d_desc, d_desc.count);
    return a.close();
}

// ---- exact bilinear resize and the scale pyramid (fdf_resize.hip) ---------------------------

int fdf_resize_taps(uint32_t src_len, uint32_t dst_len, uint32_t* taps) {
    if (!taps) return FDF_ERR_ARG;
    if (src_len == 0 || dst_len == 0 || src_len > fdfk::kResizeMaxSide) return FDF_ERR_SIZE;
    const int64_t S = src_len, D = dst_len;
    for (int64_t i = 0; i < D; ++i) {
        const int64_t N = (2 * i + 1) * S - D;          // the source position is N / (2 D)
        int64_t i0 = 0, q = 0;
        if (N >= 0) {
            i0 = N / (2 * D);
            q = (4096 * (N % (2 * D)) + 2 * D) / (4 * D);   // frac * 2048, rounded half up
        }
        if (i0 >= S - 1) {
            i0 = S > 1 ? S - 2 : 0;
            q = S > 1 ? fdfk::kResizeOne : 0;
        }
        taps[i] = (uint32_t)(i0 << 12 | q);
    }
    return FDF_OK;
}

namespace {

// What fdf_resize_device checks of its shapes and strides; *src_stride and *dst_stride are the
// frames' when the call is valid.
int check_resize(uint32_t n_frames, uint32_t src_w, uint32_t src_h, uint64_t src_stride_bytes,
                 uint32_t dst_w, uint32_t dst_h, uint64_t dst_stride_bytes, uint64_t* src_stride,
                 uint64_t* dst_stride) {
    const uint64_t src_bytes = (uint64_t)src_w * src_h, dst_bytes = (uint64_t)dst_w * dst_h;
    if (n_frames > 65535u) return FDF_ERR_ARG;
    if (src_bytes == 0 || src_bytes > fdfk::kOrientMaxPixels || dst_bytes == 0 ||
        dst_bytes > fdfk::kOrientMaxPixels || src_w > fdfk::kResizeMaxSide ||
        src_h > fdfk::kResizeMaxSide)
        return FDF_ERR_SIZE;
    *src_stride = frame_stride(n_frames, src_stride_bytes, src_bytes);
    *dst_stride = frame_stride(n_frames, dst_stride_bytes, dst_bytes);
    return *src_stride >= src_bytes && *dst_stride >= dst_bytes ? FDF_OK : FDF_ERR_ARG;
}

hipError_t resize_enqueue(const uint8_t* d_src, uint32_t n_frames, uint32_t src_w, uint32_t src_h,
                          uint64_t src_stride, uint8_t* d_dst, uint32_t dst_w, uint32_t dst_h,
                          uint64_t dst_stride, const uint32_t* d_xtaps, const uint32_t* d_ytaps,
                          hipStream_t s) {
    fdfk::ResizeParams p{};
    p.src = d_src;
    p.src_stride = src_stride;
    p.dst = d_dst;
    p.dst_stride = dst_stride;
    p.xtaps = d_xtaps;
    p.ytaps = d_ytaps;
    p.n_frames = n_frames;
    p.src_w = src_w;
    p.src_h = src_h;
    p.dst_w = dst_w;
    p.dst_h = dst_h;
    p.groups = (dst_w + 3) / 4;
    // the tallest strips that still leave 16 waves per CU
    p.strip_rows = fdfk::kResizeStripRows;
    while (p.strip_rows > 8 &&
           (uint64_t)p.groups * ((dst_h + p.strip_rows - 1) / p.strip_rows) * n_frames < 256 * 1024)
        p.strip_rows /= 2;
    p.strips = (dst_h + p.strip_rows - 1) / p.strip_rows;
    return fdfk::launch_resize(p, s);
}

// The sizes of a plan: level l from level l - 1 by the factor num / den, rounded to nearest.
int pyramid_sizes(uint32_t base_w, uint32_t base_h, uint32_t num, uint32_t den, uint32_t n_levels,
                  uint32_t* w, uint32_t* h) {
    if (den == 0 || num <= den || n_levels == 0 || n_levels > 32) return FDF_ERR_ARG;
    if (base_w == 0 || base_h == 0 || base_w > fdfk::kResizeMaxSide ||
        base_h > fdfk::kResizeMaxSide)
        return FDF_ERR_SIZE;
    w[0] = base_w;
    h[0] = base_h;
    for (uint32_t l = 1; l < n_levels; ++l) {
        w[l] = (uint32_t)(((uint64_t)w[l - 1] * den + num / 2) / num);
        h[l] = (uint32_t)(((uint64_t)h[l - 1] * den + num / 2) / num);
        if (w[l] == 0 || h[l] == 0) return FDF_ERR_SIZE;
    }
    return FDF_OK;
}

}  // namespace

int fdf_resize_device(fdf_ctx* ctx, const uint8_t* d_src, uint32_t n_frames, uint32_t src_w,
                      uint32_t src_h, uint64_t src_frame_stride_bytes, uint8_t* d_dst,
                      uint32_t dst_w, uint32_t dst_h, uint64_t dst_frame_stride_bytes,
                      const uint32_t* d_xtaps, const uint32_t* d_ytaps, void* stream) {
    if (!ctx) return FDF_ERR_ARG;
    uint64_t ss = 0, ds = 0;
    const bool ptrs = d_src && d_dst && d_xtaps && d_ytaps;
    const int rc = check_resize(n_frames, src_w, src_h, src_frame_stride_bytes, dst_w, dst_h,
                                dst_frame_stride_bytes, &ss, &ds);
    if (rc == FDF_ERR_SIZE || n_frames > 65535u) return rc;
    if (n_frames == 0) return FDF_OK;
    if (!ptrs || rc) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    return status_of(resize_enqueue(d_src, n_frames, src_w, src_h, ss, d_dst, dst_w, dst_h, ds,
                                    d_xtaps, d_ytaps, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_resize_frame(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                     size_t stride_bytes, uint8_t* out, uint32_t dst_w, uint32_t dst_h,
                     size_t out_stride_bytes) {
    if (!ctx) return FDF_ERR_ARG;
    uint64_t ss = 0, ds = 0;
    const int rc = check_resize(1, width, height, 0, dst_w, dst_h, 0, &ss, &ds);
    if (rc) return rc;
    if (!data || !out || stride_bytes < width || out_stride_bytes < dst_w) return FDF_ERR_ARG;
    std::vector<uint32_t> taps((size_t)dst_w + dst_h);  // an asynchronous copy's source
    if (fdf_resize_taps(width, dst_w, taps.data()) != FDF_OK ||
        fdf_resize_taps(height, dst_h, taps.data() + dst_w) != FDF_OK)
        return FDF_ERR_SIZE;
    Arena a(ctx);
    const auto d_src = a.part<uint8_t>(ss);
    const auto d_dst = a.part<uint8_t>(ds);
    const auto d_taps = a.part<uint32_t>(taps.size());
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload_frame(d_src, data, width, height, stride_bytes);
    a.upload(d_taps, taps.data());
    if (a.ok())
        a.note(resize_enqueue(a.at(d_src), 1, width, height, ss, a.at(d_dst), dst_w, dst_h, ds,
                              a.at(d_taps), a.at(d_taps) + dst_w, ctx->stream));
    a.download_frame(out, d_dst, dst_w, dst_h, out_stride_bytes);
    return a.close();
}

int fdf_pyramid_plan(uint32_t base_w, uint32_t base_h, uint32_t num, uint32_t den,
                     uint32_t n_levels, uint32_t n_frames, fdf_pyramid_level* levels,
                     uint64_t* total_bytes, uint64_t* total_taps) {
    if (!levels || n_frames > 65535u) return FDF_ERR_ARG;
    uint32_t w[32], h[32];
    const int rc = pyramid_sizes(base_w, base_h, num, den, n_levels, w, h);
    if (rc) return rc;
    uint64_t bytes = 0, taps = 0;
    for (uint32_t l = 0; l < n_levels; ++l) {
        fdf_pyramid_level& L = levels[l];
        L = fdf_pyramid_level{};
        L.width = w[l];
        L.height = h[l];
        if (l == 0) continue;                        // the caller's frames: nothing of the buffer
        L.frame_stride_bytes = (uint64_t)w[l] * h[l];
        L.offset_bytes = bytes;
        L.xtaps_offset = taps;
        L.ytaps_offset = taps + w[l];
        bytes += align256(L.frame_stride_bytes * n_frames);
        taps += (uint64_t)w[l] + h[l];
    }
    if (total_bytes) *total_bytes = bytes;
    if (total_taps) *total_taps = taps;
    return FDF_OK;
}

int fdf_pyramid_taps(const fdf_pyramid_level* levels, uint32_t n_levels, uint32_t base_w,
                     uint32_t base_h, uint32_t* taps) {
    if (!levels || n_levels == 0 || n_levels > 32 || levels[0].width != base_w ||
        levels[0].height != base_h || (n_levels > 1 && !taps))
        return FDF_ERR_ARG;
    for (uint32_t l = 1; l < n_levels; ++l) {
        int rc = fdf_resize_taps(levels[l - 1].width, levels[l].width, taps + levels[l].xtaps_offset);
        if (rc == FDF_OK)
            rc = fdf_resize_taps(levels[l - 1].height, levels[l].height,
                                 taps + levels[l].ytaps_offset);
        if (rc) return rc;
    }
    return FDF_OK;
}

int fdf_pyramid_device(fdf_ctx* ctx, const uint8_t* d_frames, uint32_t n_frames,
                       uint64_t frame_stride_bytes, const fdf_pyramid_level* levels,
                       uint32_t n_levels, uint8_t* d_pyramid, const uint32_t* d_taps,
                       void* stream) {
    if (!ctx || !levels || n_levels == 0 || n_levels > 32 || n_frames > 65535u) return FDF_ERR_ARG;
    // every level is checked before the first launch
    uint64_t ss[32] = {0}, ds[32] = {0};
    for (uint32_t l = 1; l < n_levels; ++l) {
        const fdf_pyramid_level& S = levels[l - 1];
        const fdf_pyramid_level& D = levels[l];
        const int rc = check_resize(n_frames, S.width, S.height,
                                    l == 1 ? frame_stride_bytes : S.frame_stride_bytes, D.width,
                                    D.height, D.frame_stride_bytes, &ss[l], &ds[l]);
        if (rc) return rc;
    }
    if (n_frames == 0 || n_levels == 1) return FDF_OK;
    if (!d_frames || !d_pyramid || !d_taps) return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (uint32_t l = 1; l < n_levels; ++l) {
        const fdf_pyramid_level& S = levels[l - 1];
        const fdf_pyramid_level& D = levels[l];
        const uint8_t* src = l == 1 ? d_frames : d_pyramid + S.offset_bytes;
        const hipError_t e = resize_enqueue(src, n_frames, S.width, S.height, ss[l],
                                            d_pyramid + D.offset_bytes, D.width, D.height, ds[l],
                                            d_taps + D.xtaps_offset, d_taps + D.ytaps_offset, s);
        if (e != hipSuccess) return FDF_ERR_DEVICE;
    }
    return FDF_OK;
}

// ---- exact bilinear warp by a model per frame (fdf_warp.hip) ---------------------------------
namespace {

static_assert(FDF_BORDER_REPLICATE == fdfk::kWarpReplicate &&
                  FDF_BORDER_CONSTANT == fdfk::kWarpConstant &&
                  offsetof(fdf_model, h) == 0 && sizeof(fdf_model) == 88,
              "the kernels' constants are the header's; an fdf_model starts with its matrix");

// What fdf_warp_device checks of its values (not of its pointers): the resize's shapes and
// strides, then the border, the fill and the model stride.
int check_warp(uint32_t n_frames, uint32_t src_w, uint32_t src_h, uint64_t src_stride_bytes,
               uint32_t dst_w, uint32_t dst_h, uint64_t dst_stride_bytes,
               uint64_t model_stride_bytes, uint32_t border, uint32_t fill, uint64_t* src_stride,
               uint64_t* dst_stride) {
    const int rc = check_resize(n_frames, src_w, src_h, src_stride_bytes, dst_w, dst_h,
                                dst_stride_bytes, src_stride, dst_stride);
    if (rc == FDF_ERR_SIZE || n_frames > 65535u) return rc;
    if (border > FDF_BORDER_CONSTANT || fill > 255u ||
        model_stride_bytes < fdfk::kWarpModelBytes || model_stride_bytes % 8)
        return FDF_ERR_ARG;
    return rc;
}

hipError_t warp_enqueue(const uint8_t* d_src, uint32_t n_frames, uint32_t src_w, uint32_t src_h,
                        uint64_t src_stride, const void* d_models, uint64_t model_stride,
                        uint8_t* d_dst, uint32_t dst_w, uint32_t dst_h, uint64_t dst_stride,
                        uint32_t border, uint32_t fill, uint8_t* d_mask, hipStream_t s) {
    fdfk::WarpParams p{};
    p.src = d_src;
    p.src_stride = src_stride;
    p.dst = d_dst;
    p.mask = d_mask;
    p.dst_stride = dst_stride;
    p.models = d_models;
    p.model_stride = model_stride;
    p.n_frames = n_frames;
    p.src_w = src_w;
    p.src_h = src_h;
    p.dst_w = dst_w;
    p.dst_h = dst_h;
    p.border = border;
    p.fill = fill;
    p.groups = (dst_w + 3) / 4;
    return fdfk::launch_warp(p, s);
}

}  // namespace

int fdf_warp_device(fdf_ctx* ctx, const uint8_t* d_src, uint32_t n_frames, uint32_t src_w,
                    uint32_t src_h, uint64_t src_frame_stride_bytes, const void* d_models,
                    uint64_t model_stride_bytes, uint8_t* d_dst, uint32_t dst_w, uint32_t dst_h,
                    uint64_t dst_frame_stride_bytes, uint32_t border, uint32_t fill,
                    uint8_t* d_mask, void* stream) {
    if (!ctx) return FDF_ERR_ARG;
    uint64_t ss = 0, ds = 0;
    const int rc = check_warp(n_frames, src_w, src_h, src_frame_stride_bytes, dst_w, dst_h,
                              dst_frame_stride_bytes, model_stride_bytes, border, fill, &ss, &ds);
    if (rc == FDF_ERR_SIZE || n_frames > 65535u) return rc;
    if (n_frames == 0 && rc == FDF_OK) return FDF_OK;
    if (rc || !d_src || !d_dst || !d_models || reinterpret_cast<uintptr_t>(d_models) % 8)
        return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    return status_of(warp_enqueue(d_src, n_frames, src_w, src_h, ss, d_models, model_stride_bytes,
                                  d_dst, dst_w, dst_h, ds, border, fill, d_mask,
                                  reinterpret_cast<hipStream_t>(stream)));
}

int fdf_warp_frame(fdf_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height,
                   size_t stride_bytes, const double h[9], uint8_t* out, uint32_t dst_w,
                   uint32_t dst_h, size_t out_stride_bytes, uint32_t border, uint32_t fill,
                   uint8_t* out_mask) {
    if (!ctx) return FDF_ERR_ARG;
    uint64_t ss = 0, ds = 0;
    const int rc = check_warp(1, width, height, 0, dst_w, dst_h, 0, fdfk::kWarpModelBytes, border,
                              fill, &ss, &ds);
    if (rc) return rc;
    if (!data || !h || !out || stride_bytes < width || out_stride_bytes < dst_w) return FDF_ERR_ARG;
    double model[9];                                     // an asynchronous copy's source
    std::copy(h, h + 9, model);
    Arena a(ctx);
    const auto d_src = a.part<uint8_t>(ss);
    const auto d_dst = a.part<uint8_t>(ds);
    const auto d_mask = a.part<uint8_t>(out_mask ? ds : 0);
    const auto d_model = a.part<double>(9);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload_frame(d_src, data, width, height, stride_bytes);
    a.upload(d_model, model);
    if (a.ok())
        a.note(warp_enqueue(a.at(d_src), 1, width, height, ss, a.at(d_model),
                            fdfk::kWarpModelBytes, a.at(d_dst), dst_w, dst_h, ds, border, fill,
                            out_mask ? a.at(d_mask) : nullptr, ctx->stream));
    a.download_frame(out, d_dst, dst_w, dst_h, out_stride_bytes);
    if (out_mask) a.download_frame(out_mask, d_mask, dst_w, dst_h, out_stride_bytes);
    return a.close();
}

int fdf_model_invert(const double h[9], double out[9]) {
#pragma clang fp contract(off)
    if (!h || !out) return FDF_ERR_ARG;
    // the adjugate, each product and each difference rounded once
    const double c[9] = {
        h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
        h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
        h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]};
    double r[9];
    for (int k = 0; k < 8; ++k) {
        r[k] = c[k] / c[8];
        if (!std::isfinite(r[k])) return FDF_ERR_ARG;
    }
    r[8] = 1.0;
    std::copy(r, r + 9, out);
    return FDF_OK;
}

// ---- pyramidal Lucas-Kanade tracking (fdf_track.hip) -----------------------------------------

int fdf_track_map_position(int64_t x, uint32_t len0, uint32_t len_l, int64_t* out) {
    if (!out || len0 == 0 || len0 > 65535u || len_l == 0 || len_l > 65535u || x > (1ll << 28) ||
        x < -(1ll << 28))
        return FDF_ERR_ARG;
    *out = fdfk::track_map_pos(x, len0, len_l);
    return FDF_OK;
}

int fdf_track_map_displacement(int64_t d, uint32_t len_from, uint32_t len_to, int64_t* out) {
    if (!out || len_from == 0 || len_from > 65535u || len_to == 0 || len_to > 65535u ||
        d > (1ll << 28) || d < -(1ll << 28))
        return FDF_ERR_ARG;
    *out = fdfk::track_map_disp(d, len_from, len_to);
    return FDF_OK;
}

namespace {

static_assert(FDF_COORDS_U32 == fdfk::kTrackU32 && FDF_COORDS_Q11 == fdfk::kTrackQ11,
              "the kernel's constants are the header's");

// What the tracker checks of its values (not of its pointers), in the order of the header.
int check_track(uint32_t n_frames, uint32_t prev_first, uint32_t next_first,
                uint64_t frame_stride_bytes, const fdf_pyramid_level* levels, uint32_t n_levels,
                uint32_t coords, uint32_t radius, uint32_t max_iters, float min_eig) {
    if (radius == 0 || radius > fdfk::kTrackMaxRadius || max_iters == 0 ||
        max_iters > fdfk::kTrackMaxIters || !(min_eig >= 0.0f) || !std::isfinite(min_eig) ||
        (coords != FDF_COORDS_U32 && coords != FDF_COORDS_Q11) || n_frames > 65535u || !levels ||
        n_levels == 0 || n_levels > fdfk::kTrackMaxLevels)
        return FDF_ERR_ARG;
    for (uint32_t l = 0; l < n_levels; ++l) {
        const uint64_t bytes = (uint64_t)levels[l].width * levels[l].height;
        if (bytes == 0 || levels[l].width > fdfk::kResizeMaxSide ||
            levels[l].height > fdfk::kResizeMaxSide || bytes > fdfk::kOrientMaxPixels)
            return FDF_ERR_SIZE;
    }
    // frames up to first + n_frames are addressed on either side
    const uint64_t addressed = (uint64_t)std::max(prev_first, next_first) + n_frames;
    if (n_frames != 0 && addressed > 1)
        for (uint32_t l = 0; l < n_levels; ++l) {
            const uint64_t stride = l == 0 ? frame_stride_bytes : levels[l].frame_stride_bytes;
            if (stride < (uint64_t)levels[l].width * levels[l].height) return FDF_ERR_ARG;
        }
    return FDF_OK;
}

struct TrackOutputs {
    int32_t* q11;
    float* f32;
    uint8_t* status;
    uint32_t* err;
    uint32_t* info;
    fdf_match* matches;
};

// The launch of fdf_track_device / fdf_track_frames (arguments already validated).
hipError_t track_enqueue(const uint8_t* d_prev_frames, const uint8_t* d_prev_pyramid,
                         uint32_t prev_first, const uint8_t* d_next_frames,
                         const uint8_t* d_next_pyramid, uint32_t next_first, uint32_t n_frames,
                         uint64_t frame_stride_bytes, const fdf_pyramid_level* levels,
                         uint32_t n_levels, const void* d_points, uint32_t coords, uint64_t cap,
                         const uint64_t* d_offsets, const uint8_t* d_keep, const int32_t* d_guess,
                         uint32_t radius, uint32_t max_iters, uint32_t eps, float min_eig,
                         const TrackOutputs& o, hipStream_t s) {
#pragma clang fp contract(off)
    fdfk::TrackParams p{};
    for (uint32_t l = 0; l < n_levels; ++l) {
        fdfk::TrackLevel& L = p.levels[l];
        const uint64_t stride = l == 0 ? frame_stride_bytes : levels[l].frame_stride_bytes;
        const uint64_t offset = l == 0 ? 0 : levels[l].offset_bytes;
        L.prev = (l == 0 ? d_prev_frames : d_prev_pyramid) + offset + prev_first * stride;
        L.next = (l == 0 ? d_next_frames : d_next_pyramid) + offset + next_first * stride;
        L.prev_stride = L.next_stride = stride;
        L.width = levels[l].width;
        L.height = levels[l].height;
    }
    p.n_levels = n_levels;
    p.n_frames = n_frames;
    p.pts = d_points;
    p.offs = d_offsets;
    p.cap = cap;
    p.keep = d_keep;
    p.guess = reinterpret_cast<const int2*>(d_guess);
    p.coords = coords;
    p.radius = radius;
    p.max_iters = max_iters;
    p.eps = eps;
    const uint32_t n = (2 * radius + 1) * (2 * radius + 1);
    p.tau = ((double)min_eig * (double)n) * 1048576.0;
    p.next_q11 = reinterpret_cast<int2*>(o.q11);
    p.next_f32 = reinterpret_cast<float2*>(o.f32);
    p.status = o.status;
    p.err = o.err;
    p.info = o.info;
    p.matches = reinterpret_cast<uint2*>(o.matches);
    // a wave per point and many iterations each: few points per workgroup
    return fdfk::launch_track(p, chunks_per_frame(cap, n_frames, levels[0].width, levels[0].height,
                                                  16, 1024), s);
}

inline bool aligned_to(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

int fdf_track_device(fdf_ctx* ctx, const uint8_t* d_prev_frames, const uint8_t* d_prev_pyramid,
                     uint32_t prev_first, const uint8_t* d_next_frames,
                     const uint8_t* d_next_pyramid, uint32_t next_first, uint32_t n_frames,
                     uint64_t frame_stride_bytes, const fdf_pyramid_level* levels,
                     uint32_t n_levels, const void* d_points, uint32_t coords, uint64_t cap,
                     const uint64_t* d_frame_offsets, const uint8_t* d_keep, const int32_t* d_guess,
                     uint32_t radius, uint32_t max_iters, uint32_t eps, float min_eig,
                     int32_t* d_next_q11, float* d_next_f32, uint8_t* d_status, uint32_t* d_err,
                     uint32_t* d_info, fdf_match* d_matches, void* stream) {
    if (!ctx) return FDF_ERR_ARG;
    const int rc = check_track(n_frames, prev_first, next_first, frame_stride_bytes, levels,
                               n_levels, coords, radius, max_iters, min_eig);
    if (rc) return rc;
    if (n_frames == 0) return FDF_OK;
    if (!d_frame_offsets || !d_prev_frames || !d_next_frames ||
        (n_levels > 1 && (!d_prev_pyramid || !d_next_pyramid)) ||
        prev_first > 65535u || next_first > 65535u)
        return FDF_ERR_ARG;
    if (cap == 0) return FDF_OK;
    if (!d_points || !d_next_q11 || !d_status || !aligned_to(d_points, 8) ||
        !aligned_to(d_guess, 8) || !aligned_to(d_next_q11, 8) || !aligned_to(d_next_f32, 8) ||
        !aligned_to(d_matches, 8) || !aligned_to(d_err, 4) || !aligned_to(d_info, 4) ||
        (d_matches && cap > fdfk::kMatchMaxCap))
        return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    const TrackOutputs o{d_next_q11, d_next_f32, d_status, d_err, d_info, d_matches};
    return status_of(track_enqueue(d_prev_frames, d_prev_pyramid, prev_first, d_next_frames,
                                   d_next_pyramid, next_first, n_frames, frame_stride_bytes, levels,
                                   n_levels, d_points, coords, cap, d_frame_offsets, d_keep, d_guess,
                                   radius, max_iters, eps, min_eig, o,
                                   reinterpret_cast<hipStream_t>(stream)));
}

int fdf_track_frames(fdf_ctx* ctx, const uint8_t* prev, const uint8_t* next, uint32_t width,
                     uint32_t height, size_t stride_bytes, const void* points, uint32_t coords,
                     size_t n_points, const int32_t* guess, uint32_t n_levels, uint32_t num,
                     uint32_t den, uint32_t radius, uint32_t max_iters, uint32_t eps, float min_eig,
                     int32_t* out_q11, float* out_f32, uint8_t* out_status, uint32_t* out_err,
                     uint32_t* out_info) {
    if (!ctx) return FDF_ERR_ARG;
    // the two frames are one batch of two: one plan, one pyramid build, frame 0 into frame 1
    fdf_pyramid_level levels[fdfk::kTrackMaxLevels];
    uint64_t pyr_bytes = 0, n_taps = 0;
    if (n_levels == 0 || n_levels > fdfk::kTrackMaxLevels) return FDF_ERR_ARG;
    if (n_levels == 1) num = 2, den = 1;                // one level needs no ratio
    int rc = fdf_pyramid_plan(width, height, num, den, n_levels, 2, levels, &pyr_bytes, &n_taps);
    if (rc) return rc;
    const uint64_t frame_bytes = (uint64_t)width * height;
    rc = check_track(1, 0, 1, frame_bytes, levels, n_levels, coords, radius, max_iters, min_eig);
    if (rc) return rc;
    if (stride_bytes < width || (n_points && (!prev || !next || !points || !out_q11 || !out_status)))
        return FDF_ERR_ARG;
    if (n_points == 0) return FDF_OK;
    std::vector<uint32_t> taps((size_t)n_taps);         // an asynchronous copy's source
    if (fdf_pyramid_taps(levels, n_levels, width, height, taps.data()) != FDF_OK) return FDF_ERR_SIZE;
    Arena a(ctx);
    const auto d_frames = a.part<uint8_t>(2 * frame_bytes);
    const auto d_pyr = a.part<uint8_t>(pyr_bytes);
    const auto d_taps = a.part<uint32_t>(taps.size());
    const auto d_pts = a.part<uint64_t>(n_points);
    const auto d_guess = a.part<uint64_t>(guess ? n_points : 0);
    const auto d_offs = a.part<uint64_t>(2);
    const auto d_q11 = a.part<uint64_t>(n_points);
    const auto d_f32 = a.part<uint64_t>(out_f32 ? n_points : 0);
    const auto d_status = a.part<uint8_t>(n_points);
    const auto d_err = a.part<uint32_t>(out_err ? n_points : 0);
    const auto d_info = a.part<uint32_t>(out_info ? n_points : 0);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    if (a.ok())
        a.note(upload_rows(a.at(d_frames), prev, stride_bytes, width, height, ctx->stream));
    if (a.ok())
        a.note(upload_rows(a.at(d_frames) + frame_bytes, next, stride_bytes, width, height,
                           ctx->stream));
    if (!taps.empty()) a.upload(d_taps, taps.data());
    a.upload(d_pts, static_cast<const uint64_t*>(points));
    if (guess) a.upload(d_guess, reinterpret_cast<const uint64_t*>(guess));
    a.upload_one_frame(d_offs, n_points);
    if (a.ok() && n_levels > 1 &&
        fdf_pyramid_device(ctx, a.at(d_frames), 2, frame_bytes, levels, n_levels, a.at(d_pyr),
                           a.at(d_taps), ctx->stream) != FDF_OK)
        a.note(hipErrorInvalidValue);
    if (a.ok()) {
        const TrackOutputs o{reinterpret_cast<int32_t*>(a.at(d_q11)),
                             out_f32 ? reinterpret_cast<float*>(a.at(d_f32)) : nullptr,
                             a.at(d_status), out_err ? a.at(d_err) : nullptr,
                             out_info ? a.at(d_info) : nullptr, nullptr};
        a.note(track_enqueue(a.at(d_frames), a.at(d_pyr), 0, a.at(d_frames), a.at(d_pyr), 1, 1,
                             frame_bytes, levels, n_levels, a.at(d_pts), coords, n_points,
                             a.at(d_offs), nullptr,
                             guess ? reinterpret_cast<const int32_t*>(a.at(d_guess)) : nullptr,
                             radius, max_iters, eps, min_eig, o, ctx->stream));
    }
    a.download(reinterpret_cast<uint64_t*>(out_q11), d_q11, n_points);
    if (out_f32) a.download(reinterpret_cast<uint64_t*>(out_f32), d_f32, n_points);
    a.download(out_status, d_status, n_points);
    if (out_err) a.download(out_err, d_err, n_points);
    if (out_info) a.download(out_info, d_info, n_points);
    return a.close();
}

// ---- track-set maintenance (fdf_tracks.hip) -----------------------------------------------
namespace {

static_assert(FDF_TRACKS_NEW == fdfk::kTracksNewBit, "the kernel's constant is the header's");

// Scratch of one fdf_tracks_update_device call, every part 256-byte aligned.  Per list (tracks,
// then candidates): the cells' cursors and the admitted flags (both zeroed on the stream before
// the kernels), the cells' starts, the sorted entries and the two state buffers; then four
// per-stream words and the per-stream totals.
struct TracksListLayout {
    uint64_t cursor = 0, start = 0, ent = 0, st0 = 0, st1 = 0, flag = 0;
};
struct TracksLayout {
    uint32_t cell = 0, cells_x = 0, cells_y = 0;
    TracksListLayout t, c;
    uint64_t kept = 0, n_new = 0, id_base = 0, tot = 0, total = 0;
};

int tracks_layout(uint32_t n_frames, uint32_t width, uint32_t height, uint32_t min_dist,
                  uint64_t t_cap, uint64_t c_cap, TracksLayout* L) {
    if (width == 0 || height == 0 || width > fdfk::kTracksMaxSide ||
        height > fdfk::kTracksMaxSide || min_dist == 0 || min_dist > fdfk::kTracksMaxDist ||
        n_frames > 65535u || t_cap > fdfk::kTracksMaxCap || c_cap > fdfk::kTracksMaxCap)
        return FDF_ERR_ARG;
    L->cell = std::max(min_dist, fdfk::kTracksMinCell);
    L->cells_x = (width + L->cell - 1) / L->cell;
    L->cells_y = (height + L->cell - 1) / L->cell;
    const uint64_t cells = (uint64_t)L->cells_x * L->cells_y;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += align256(bytes);
        return o;
    };
    const uint64_t caps[2] = {t_cap, c_cap};
    TracksListLayout* lists[2] = {&L->t, &L->c};
    for (int k = 0; k < 2; ++k) {
        lists[k]->cursor = take(sizeof(uint32_t) * cells * n_frames);
        lists[k]->start = take(sizeof(uint32_t) * (cells + 1) * n_frames);
        lists[k]->ent = take(16 * caps[k]);
        lists[k]->st0 = take(caps[k]);
        lists[k]->st1 = take(caps[k]);
        lists[k]->flag = take(caps[k]);
    }
    L->kept = take(sizeof(uint32_t) * n_frames);
    L->n_new = take(sizeof(uint32_t) * n_frames);
    L->id_base = take(sizeof(uint32_t) * n_frames);
    L->tot = take(sizeof(uint64_t) * n_frames);
    L->total = at;
    return FDF_OK;
}

inline bool tracks_values_ok(const fdf_tracks_params* p) {
    return p && p->max_tracks >= 1 && p->passes >= 1 && p->passes <= fdfk::kTracksMaxPasses &&
           p->width != 0 && p->height != 0 &&
           2ull * p->margin < std::min(p->width, p->height);
}

}  // namespace

int fdf_tracks_scratch_bytes(uint32_t n_frames, uint32_t width, uint32_t height,
                             uint32_t min_dist, uint64_t t_cap, uint64_t c_cap, uint64_t* bytes) {
    if (!bytes) return FDF_ERR_ARG;
    TracksLayout L;
    const int rc = tracks_layout(n_frames, width, height, min_dist, t_cap, c_cap, &L);
    if (rc) return rc;
    *bytes = n_frames ? L.total : 0;
    return FDF_OK;
}

int fdf_tracks_update_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_tracks_params* params,
                             const int32_t* d_track_q11, const uint8_t* d_track_status,
                             const uint32_t* d_track_ids, const uint32_t* d_track_ages,
                             const uint64_t* d_track_offsets, uint64_t t_cap,
                             const fdf_point* d_cand_points, const uint16_t* d_cand_scores,
                             const uint64_t* d_cand_offsets, uint64_t c_cap, uint32_t* d_next_id,
                             int32_t* d_out_q11, uint32_t* d_out_ids, uint32_t* d_out_ages,
                             uint32_t* d_out_src, uint64_t out_cap, uint64_t* d_out_offsets,
                             void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!ctx || !tracks_values_ok(params)) return FDF_ERR_ARG;
    TracksLayout L;
    const int rc = tracks_layout(n_frames, params->width, params->height, params->min_dist, t_cap,
                                 c_cap, &L);
    if (rc) return rc;
    if (d_out_src && (t_cap > 0x7fffffffull || c_cap > 0x7fffffffull)) return FDF_ERR_ARG;
    if (n_frames == 0) return FDF_OK;
    if (!d_track_offsets || !d_cand_offsets || !d_next_id || !d_out_offsets || !d_scratch ||
        scratch_bytes < L.total || !aligned_to(d_scratch, 256) ||
        (t_cap && (!d_track_q11 || !d_track_ids || !d_track_ages)) ||
        (c_cap && (!d_cand_points || !d_cand_scores)) ||
        (out_cap && (!d_out_q11 || !d_out_ids || !d_out_ages)) ||
        !aligned_to(d_track_q11, 8) || !aligned_to(d_cand_points, 8) || !aligned_to(d_out_q11, 8) ||
        !aligned_to(d_track_offsets, 8) || !aligned_to(d_cand_offsets, 8) ||
        !aligned_to(d_out_offsets, 8) || !aligned_to(d_track_ids, 4) ||
        !aligned_to(d_track_ages, 4) || !aligned_to(d_next_id, 4) || !aligned_to(d_out_ids, 4) ||
        !aligned_to(d_out_ages, 4) || !aligned_to(d_out_src, 4) || !aligned_to(d_cand_scores, 2))
        return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    fdfk::TracksParams p{};
    p.n_frames = n_frames;
    p.width = params->width;
    p.height = params->height;
    p.min_dist = params->min_dist;
    p.margin = params->margin;
    p.max_tracks = params->max_tracks;
    p.passes = params->passes;
    p.cell = L.cell;
    p.cells_x = L.cells_x;
    p.cells_y = L.cells_y;
    p.t_q11 = reinterpret_cast<const int2*>(d_track_q11);
    p.t_status = d_track_status;
    p.t_ids = d_track_ids;
    p.t_ages = d_track_ages;
    p.c_pts = reinterpret_cast<const uint2*>(d_cand_points);
    p.c_scores = d_cand_scores;
    auto list = [&](fdfk::TracksList& l, const TracksListLayout& at, const uint64_t* offs,
                    uint64_t cap) {
        l.offs = offs;
        l.cap = cap;
        l.cursor = reinterpret_cast<uint32_t*>(base + at.cursor);
        l.start = reinterpret_cast<uint32_t*>(base + at.start);
        l.ent = reinterpret_cast<uint4*>(base + at.ent);
        l.st[0] = base + at.st0;
        l.st[1] = base + at.st1;
        l.flag = base + at.flag;
        // about two passes of a workgroup's threads per stream of average length
        l.chunks = (uint32_t)std::min<uint64_t>(1024, cap / n_frames / (2 * fdfk::kTracksThreads) + 1);
    };
    list(p.t, L.t, d_track_offsets, t_cap);
    list(p.c, L.c, d_cand_offsets, c_cap);
    p.next_id = d_next_id;
    p.kept = reinterpret_cast<uint32_t*>(base + L.kept);
    p.n_new = reinterpret_cast<uint32_t*>(base + L.n_new);
    p.id_base = reinterpret_cast<uint32_t*>(base + L.id_base);
    p.tot = reinterpret_cast<uint64_t*>(base + L.tot);
    p.out_q11 = reinterpret_cast<int2*>(d_out_q11);
    p.out_ids = d_out_ids;
    p.out_ages = d_out_ages;
    p.out_src = d_out_src;
    p.out_cap = out_cap;
    p.out_offs = d_out_offsets;
    const uint64_t cursor_bytes = sizeof(uint32_t) * (uint64_t)L.cells_x * L.cells_y * n_frames;
    hipError_t e = hipMemsetAsync(p.t.cursor, 0, cursor_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(p.c.cursor, 0, cursor_bytes, s);
    if (e == hipSuccess && t_cap) e = hipMemsetAsync(p.t.flag, 0, t_cap, s);
    if (e == hipSuccess && c_cap) e = hipMemsetAsync(p.c.flag, 0, c_cap, s);
    if (e == hipSuccess) e = fdfk::launch_tracks_update(p, s);
    return status_of(e);
}

int fdf_tracks_update_points(fdf_ctx* ctx, const fdf_tracks_params* params,
                             const int32_t* track_q11, const uint8_t* track_status,
                             const uint32_t* track_ids, const uint32_t* track_ages,
                             size_t n_tracks, const fdf_point* cand_points,
                             const uint16_t* cand_scores, size_t n_cands, uint32_t* next_id,
                             int32_t* out_q11, uint32_t* out_ids, uint32_t* out_ages,
                             uint32_t* out_src, size_t cap, size_t* n_out) {
    if (!ctx || !n_out || !next_id || !tracks_values_ok(params)) return FDF_ERR_ARG;
    if (n_tracks && (!track_q11 || !track_ids || !track_ages)) return FDF_ERR_ARG;
    if (n_cands && (!cand_points || !cand_scores)) return FDF_ERR_ARG;
    if (cap && (!out_q11 || !out_ids || !out_ages)) return FDF_ERR_ARG;
    if (out_src && (n_tracks > 0x7fffffffull || n_cands > 0x7fffffffull)) return FDF_ERR_ARG;
    TracksLayout L;
    const int rc = tracks_layout(1, params->width, params->height, params->min_dist, n_tracks,
                                 n_cands, &L);
    if (rc) return rc;
    *n_out = 0;
    Arena a(ctx);
    const auto d_q11 = a.part<uint64_t>(n_tracks);
    const auto d_status = a.part<uint8_t>(track_status ? n_tracks : 0);
    const auto d_ids = a.part<uint32_t>(n_tracks);
    const auto d_ages = a.part<uint32_t>(n_tracks);
    const auto d_toffs = a.part<uint64_t>(2);
    const auto d_cand = a.part<fdf_point>(n_cands);
    const auto d_scores = a.part<uint16_t>(n_cands);
    const auto d_coffs = a.part<uint64_t>(2);
    const auto d_next = a.part<uint32_t>(1);
    const auto d_oq11 = a.part<uint64_t>(cap);
    const auto d_oids = a.part<uint32_t>(cap);
    const auto d_oages = a.part<uint32_t>(cap);
    const auto d_osrc = a.part<uint32_t>(out_src ? cap : 0);
    const auto d_ooffs = a.part<uint64_t>(2);
    const auto d_scratch = a.part<uint8_t>(L.total);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    const uint64_t toffs[2] = {0, n_tracks}, coffs[2] = {0, n_cands};   // live until close()
    if (n_tracks) {
        a.upload(d_q11, reinterpret_cast<const uint64_t*>(track_q11));
        if (track_status) a.upload(d_status, track_status);
        a.upload(d_ids, track_ids);
        a.upload(d_ages, track_ages);
    }
    if (n_cands) {
        a.upload(d_cand, cand_points);
        a.upload(d_scores, cand_scores);
    }
    a.upload(d_toffs, toffs);
    a.upload(d_coffs, coffs);
    a.upload(d_next, next_id);
    if (a.ok()) {
        const int status = fdf_tracks_update_device(
            ctx, 1, params, reinterpret_cast<const int32_t*>(a.at(d_q11)),
            track_status ? a.at(d_status) : nullptr, a.at(d_ids), a.at(d_ages), a.at(d_toffs),
            n_tracks, a.at(d_cand), a.at(d_scores), a.at(d_coffs), n_cands, a.at(d_next),
            reinterpret_cast<int32_t*>(a.at(d_oq11)), a.at(d_oids), a.at(d_oages),
            out_src ? a.at(d_osrc) : nullptr, cap, a.at(d_ooffs), a.at(d_scratch), L.total,
            ctx->stream);
        if (status != FDF_OK) return status;
    }
    // two phases: the offsets tell how many entries to copy
    uint64_t offs[2] = {0, 0};
    uint32_t next = *next_id;
    a.download(offs, d_ooffs, 2);
    a.download(&next, d_next, 1);
    a.note(hipStreamSynchronize(ctx->stream));
    const uint64_t total = a.ok() ? offs[1] : 0;
    const uint64_t ncopy = std::min<uint64_t>(total, cap);
    if (ncopy) {
        a.download(reinterpret_cast<uint64_t*>(out_q11), d_oq11, ncopy);
        a.download(out_ids, d_oids, ncopy);
        a.download(out_ages, d_oages, ncopy);
        if (out_src) a.download(out_src, d_osrc, ncopy);
    }
    if (a.close() != FDF_OK) return FDF_ERR_DEVICE;
    *next_id = next;
    *n_out = (size_t)total;
    return total > cap ? FDF_ERR_CAPACITY : FDF_OK;
}

// ---- brute-force Hamming matching (fdf_match.hip) ------------------------------------------
namespace {

static_assert(sizeof(fdf_match) == 8 && sizeof(fdf_match) == sizeof(uint2), "fdf_match is 8 bytes");
static_assert(FDF_MATCH_NONE == fdfk::kMatchNone && FDF_MATCH_NO_DISTANCE == fdfk::kMatchNoDistance,
              "the kernels' constants are the header's");

// The launch of fdf_match_device / fdf_match_points (arguments already validated).
hipError_t match_enqueue(uint32_t n_frames, const uint8_t* d_q_desc, const fdf_point* d_q_points,
                         uint64_t q_cap, const uint64_t* d_q_offsets, const uint8_t* d_t_desc,
                         const fdf_point* d_t_points, uint64_t t_cap, const uint64_t* d_t_offsets,
                         uint32_t max_dx, uint32_t max_dy, fdf_match* d_matches, hipStream_t s) {
    fdfk::MatchParams p{};
    p.q_desc = d_q_desc;
    p.q_pts = reinterpret_cast<const uint2*>(d_q_points);
    p.q_offs = d_q_offsets;
    p.q_cap = q_cap;
    p.t_desc = d_t_desc;
    p.t_pts = reinterpret_cast<const uint2*>(d_t_points);
    p.t_offs = d_t_offsets;
    p.t_cap = t_cap;
    p.n_frames = n_frames;
    p.max_dx = max_dx;
    p.max_dy = max_dy;
    p.matches = reinterpret_cast<uint2*>(d_matches);
    // a workgroup per 256 queries of a frame at the mean frame size, 1024 at most
    const uint32_t chunks =
        (uint32_t)std::min<uint64_t>(1024, q_cap / n_frames / fdfk::kMatchThreads + 1);
    return fdfk::launch_match(p, chunks, s);
}

}  // namespace

int fdf_match_device(fdf_ctx* ctx, uint32_t n_frames, const uint8_t* d_q_desc,
                     const fdf_point* d_q_points, uint64_t q_cap, const uint64_t* d_q_offsets,
                     const uint8_t* d_t_desc, const fdf_point* d_t_points, uint64_t t_cap,
                     const uint64_t* d_t_offsets, uint32_t max_dx, uint32_t max_dy,
                     fdf_match* d_matches, void* stream) {
    if (!ctx || !d_q_offsets || !d_t_offsets || n_frames > 65535u ||
        q_cap > fdfk::kMatchMaxCap || t_cap > fdfk::kMatchMaxCap ||
        (d_q_points == nullptr) != (d_t_points == nullptr))
        return FDF_ERR_ARG;
    if (n_frames == 0 || q_cap == 0) return FDF_OK;
    if (!d_q_desc || !d_matches || (t_cap && !d_t_desc) || ((uintptr_t)d_q_desc & 3u) != 0 ||
        ((uintptr_t)d_t_desc & 3u) != 0 || ((uintptr_t)d_matches & 7u) != 0)
        return FDF_ERR_ARG;
    DeviceGuard guard(ctx->device);
    return status_of(match_enqueue(n_frames, d_q_desc, d_q_points, q_cap, d_q_offsets, d_t_desc,
                                   d_t_points, t_cap, d_t_offsets, max_dx, max_dy, d_matches,
                                   reinterpret_cast<hipStream_t>(stream)));
}

int fdf_match_filter_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                            uint64_t q_cap, const uint64_t* d_q_offsets,
                            const fdf_match* d_reverse, uint64_t t_cap, uint32_t max_distance,
                            uint32_t ratio_num, uint32_t ratio_den, uint8_t* d_keep,
                            void* stream) {
    if (!ctx || !d_q_offsets || n_frames > 65535u || q_cap > fdfk::kMatchMaxCap ||
        t_cap > fdfk::kMatchMaxCap || ratio_num > 65535u || ratio_den > 65535u)
        return FDF_ERR_ARG;
    if (n_frames == 0 || q_cap == 0) return FDF_OK;
    if (!d_matches || !d_keep || ((uintptr_t)d_matches & 7u) != 0 ||
        ((uintptr_t)d_reverse & 7u) != 0)
        return FDF_ERR_ARG;
    fdfk::MatchFilterParams p{};
    p.matches = reinterpret_cast<const uint2*>(d_matches);
    p.q_offs = d_q_offsets;
    p.q_cap = q_cap;
    p.reverse = reinterpret_cast<const uint2*>(d_reverse);
    p.t_cap = t_cap;
    p.n_frames = n_frames;
    p.max_distance = max_distance;
    p.ratio_num = ratio_num;
    p.ratio_den = ratio_den;
    p.keep = d_keep;
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_match_filter(p, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_match_points(fdf_ctx* ctx, const uint8_t* q_desc, const fdf_point* q_points, size_t n_q,
                     const uint8_t* t_desc, const fdf_point* t_points, size_t n_t,
                     uint32_t max_dx, uint32_t max_dy, fdf_match* out) {
    if (!ctx || (q_points == nullptr) != (t_points == nullptr)) return FDF_ERR_ARG;
    if (n_q > fdfk::kMatchMaxCap || n_t > fdfk::kMatchMaxCap) return FDF_ERR_ARG;
    if (n_q && (!q_desc || !out)) return FDF_ERR_ARG;
    if (n_t && !t_desc) return FDF_ERR_ARG;
    if (n_q == 0) return FDF_OK;
    const bool window = q_points != nullptr;
    const uint64_t t_offs[2] = {0, n_t};                  // an asynchronous copy's source
    Arena a(ctx);
    const auto d_q = a.part<uint8_t>(n_q * (uint64_t)fdfk::kBriefBytes);
    const auto d_t = a.part<uint8_t>(n_t * (uint64_t)fdfk::kBriefBytes);
    const auto d_qp = a.part<fdf_point>(window ? n_q : 0);
    const auto d_tp = a.part<fdf_point>(window ? n_t : 0);
    const auto d_qo = a.part<uint64_t>(2);
    const auto d_to = a.part<uint64_t>(2);
    const auto d_out = a.part<fdf_match>(n_q);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    a.upload(d_q, q_desc);
    if (n_t) a.upload(d_t, t_desc);
    if (window) a.upload(d_qp, q_points);
    if (window && n_t) a.upload(d_tp, t_points);
    a.upload_one_frame(d_qo, n_q);
    a.upload(d_to, t_offs);
    if (a.ok())
        a.note(match_enqueue(1, a.at(d_q), window ? a.at(d_qp) : nullptr, n_q, a.at(d_qo),
                             a.at(d_t), window ? a.at(d_tp) : nullptr, n_t, a.at(d_to), max_dx,
                             max_dy, a.at(d_out), ctx->stream));
    a.download(out, d_out, n_q);
    return a.close();
}

// ---- RANSAC affine / homography estimation (fdf_ransac.hip) --------------------------------
namespace {

static_assert(sizeof(fdf_model) == 88 && alignof(fdf_model) == 8 &&
              offsetof(fdf_model, n_corr) == 72, "fdf_model is 9 doubles and 4 words");
static_assert(FDF_COORDS_U32 == fdfk::kRansacU32 && FDF_COORDS_F32 == fdfk::kRansacF32 &&
              FDF_MODEL_AFFINE == fdfk::kRansacAffine && FDF_MODEL_HOMOGRAPHY == fdfk::kRansacHomography &&
              FDF_RANSAC_NONE == fdfk::kRansacInvalid, "the kernels' constants are the header's");

// Scratch of one fdf_ransac_device call, every part 256-byte aligned: x, y, u, v per query
// index, the correspondence count per frame, the inlier count per (frame, hypothesis).
struct RansacLayout {
    uint64_t corr = 0, n_corr = 0, counts = 0, total = 0;
};

int ransac_layout(uint32_t n_frames, uint64_t q_cap, uint32_t n_hyp, RansacLayout* L) {
    if (n_frames > 65535u || q_cap > fdfk::kMatchMaxCap || n_hyp == 0 ||
        n_hyp > fdfk::kRansacMaxHyp)
        return FDF_ERR_ARG;
    L->corr = 0;                                       // all below 2^38: no overflow
    L->n_corr = L->corr + align256(4 * sizeof(double) * q_cap);
    L->counts = L->n_corr + align256(sizeof(uint32_t) * n_frames);
    L->total = L->counts + align256(sizeof(uint32_t) * (uint64_t)n_frames * n_hyp);
    return FDF_OK;
}

// What fdf_ransac_device and fdf_ransac_points check of the values.
inline bool ransac_values_ok(uint32_t coords, uint32_t model, float threshold) {
    return coords <= FDF_COORDS_F32 && model <= FDF_MODEL_HOMOGRAPHY && std::isfinite(threshold) &&
           threshold >= 0.0f;
}

}  // namespace

int fdf_ransac_sample(uint32_t seed, uint32_t frame, uint32_t hypothesis, uint32_t m, uint32_t s,
                      uint32_t idx[4], uint32_t* draws) {
    if (!idx || (s != 3 && s != 4)) return FDF_ERR_ARG;
    if (s == 3) {
        uint32_t got[3];
        fdfk::ransac_sample<3>(seed, frame, hypothesis, m, got, draws);
        std::memcpy(idx, got, sizeof(got));
        idx[3] = FDF_RANSAC_NONE;
    } else {
        uint32_t got[4];
        fdfk::ransac_sample<4>(seed, frame, hypothesis, m, got, draws);
        std::memcpy(idx, got, sizeof(got));
    }
    return FDF_OK;
}

int fdf_ransac_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint32_t n_hyp, uint64_t* bytes) {
    if (!bytes) return FDF_ERR_ARG;
    RansacLayout L;
    const int rc = ransac_layout(n_frames, q_cap, n_hyp, &L);
    if (rc) return rc;
    *bytes = L.total;
    return FDF_OK;
}

int fdf_ransac_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                      const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                      const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                      const uint64_t* d_t_offsets, uint32_t coords, uint32_t model,
                      uint32_t n_hyp, float threshold, uint32_t seed, fdf_model* d_models,
                      uint8_t* d_inliers, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    RansacLayout L;
    if (!ctx || ransac_layout(n_frames, q_cap, n_hyp, &L) != FDF_OK ||
        t_cap > fdfk::kMatchMaxCap || !ransac_values_ok(coords, model, threshold))
        return FDF_ERR_ARG;
    if (n_frames == 0) return FDF_OK;
    if (!d_matches || !d_q_offsets || !d_t_offsets || !d_q_coords || !d_t_coords || !d_models ||
        !d_scratch || scratch_bytes < L.total || ((uintptr_t)d_matches & 7u) != 0 ||
        ((uintptr_t)d_q_coords & 7u) != 0 || ((uintptr_t)d_t_coords & 7u) != 0 ||
        ((uintptr_t)d_models & 7u) != 0 || ((uintptr_t)d_scratch & 255u) != 0)
        return FDF_ERR_ARG;
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    fdfk::RansacParams p{};
    p.matches = reinterpret_cast<const uint2*>(d_matches);
    p.keep = d_keep;
    p.q_offs = d_q_offsets;
    p.q_cap = q_cap;
    p.q_coords = static_cast<const uint2*>(d_q_coords);
    p.t_coords = static_cast<const uint2*>(d_t_coords);
    p.t_offs = d_t_offsets;
    p.t_cap = t_cap;
    p.n_frames = n_frames;
    p.coords = coords;
    p.model = model;
    p.n_hyp = n_hyp;
    p.seed = seed;
    p.tt = (double)threshold * (double)threshold;
    p.models = reinterpret_cast<double*>(d_models);
    p.inliers = d_inliers;
    p.corr = reinterpret_cast<double*>(base + L.corr);
    p.n_corr = reinterpret_cast<uint32_t*>(base + L.n_corr);
    p.counts = reinterpret_cast<uint32_t*>(base + L.counts);
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_ransac(p, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_ransac_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                      size_t n_t, const fdf_match* matches, const uint8_t* keep, uint32_t coords,
                      uint32_t model, uint32_t n_hyp, float threshold, uint32_t seed,
                      fdf_model* model_out, uint8_t* inliers_out) {
    RansacLayout L;
    if (!ctx || !model_out || ransac_layout(1, n_q, n_hyp, &L) != FDF_OK ||
        n_t > fdfk::kMatchMaxCap || !ransac_values_ok(coords, model, threshold))
        return FDF_ERR_ARG;
    if (n_q && (!q_coords || !matches)) return FDF_ERR_ARG;
    if (n_t && !t_coords) return FDF_ERR_ARG;
    const uint64_t t_offs[2] = {0, n_t};                  // an asynchronous copy's source
    Arena a(ctx);
    const auto d_q = a.part<fdf_point>(n_q);
    const auto d_t = a.part<fdf_point>(n_t);
    const auto d_m = a.part<fdf_match>(n_q);
    const auto d_keep = a.part<uint8_t>(keep ? n_q : 0);
    const auto d_qo = a.part<uint64_t>(2);
    const auto d_to = a.part<uint64_t>(2);
    const auto d_model = a.part<fdf_model>(1);
    const auto d_in = a.part<uint8_t>(inliers_out ? n_q : 0);
    const auto d_scratch = a.part<uint8_t>(L.total);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    if (n_q) a.upload(d_q, static_cast<const fdf_point*>(q_coords));
    if (n_t) a.upload(d_t, static_cast<const fdf_point*>(t_coords));
    if (n_q) a.upload(d_m, matches);
    if (keep && n_q) a.upload(d_keep, keep);
    a.upload_one_frame(d_qo, n_q);
    a.upload(d_to, t_offs);
    if (a.ok()) {
        const int status = fdf_ransac_device(
            ctx, 1, a.at(d_m), keep ? a.at(d_keep) : nullptr, n_q, a.at(d_qo), a.at(d_q),
            a.at(d_t), n_t, a.at(d_to), coords, model, n_hyp, threshold, seed, a.at(d_model),
            inliers_out ? a.at(d_in) : nullptr, a.at(d_scratch), L.total, ctx->stream);
        if (status != FDF_OK) return status;
    }
    a.download(model_out, d_model, 1);
    if (inliers_out && n_q) a.download(inliers_out, d_in, n_q);
    return a.close();
}

// ---- least-squares refinement of the models over their inliers (fdf_ransac.hip) ---------------
namespace {

// Scratch of one fdf_refine_device call: RansacLayout's first two parts.
int refine_layout(uint32_t n_frames, uint64_t q_cap, RansacLayout* L) {
    const int rc = ransac_layout(n_frames, q_cap, 1, L);
    if (rc == FDF_OK) L->total = L->counts;
    return rc;
}

}  // namespace

int fdf_refine_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint64_t* bytes) {
    if (!bytes) return FDF_ERR_ARG;
    RansacLayout L;
    const int rc = refine_layout(n_frames, q_cap, &L);
    if (rc) return rc;
    *bytes = L.total;
    return FDF_OK;
}

int fdf_refine_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                      const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                      const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                      const uint64_t* d_t_offsets, uint32_t coords, uint32_t model,
                      const fdf_model* d_models_in, float threshold, uint32_t n_rounds,
                      fdf_model* d_models_out, uint8_t* d_inliers, uint32_t* d_rounds,
                      void* d_scratch, uint64_t scratch_bytes, void* stream) {
    RansacLayout L;
    if (!ctx || refine_layout(n_frames, q_cap, &L) != FDF_OK || t_cap > fdfk::kMatchMaxCap ||
        !ransac_values_ok(coords, model, threshold) || n_rounds > fdfk::kRefineMaxRounds)
        return FDF_ERR_ARG;
    if (n_frames == 0) return FDF_OK;
    if (!d_matches || !d_q_offsets || !d_t_offsets || !d_q_coords || !d_t_coords || !d_models_in ||
        !d_models_out || !d_scratch || scratch_bytes < L.total ||
        ((uintptr_t)d_matches & 7u) != 0 || ((uintptr_t)d_q_coords & 7u) != 0 ||
        ((uintptr_t)d_t_coords & 7u) != 0 || ((uintptr_t)d_models_in & 7u) != 0 ||
        ((uintptr_t)d_models_out & 7u) != 0 || ((uintptr_t)d_rounds & 3u) != 0 ||
        ((uintptr_t)d_scratch & 255u) != 0)
        return FDF_ERR_ARG;
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    fdfk::RefineParams p{};
    p.r.matches = reinterpret_cast<const uint2*>(d_matches);
    p.r.keep = d_keep;
    p.r.q_offs = d_q_offsets;
    p.r.q_cap = q_cap;
    p.r.q_coords = static_cast<const uint2*>(d_q_coords);
    p.r.t_coords = static_cast<const uint2*>(d_t_coords);
    p.r.t_offs = d_t_offsets;
    p.r.t_cap = t_cap;
    p.r.n_frames = n_frames;
    p.r.coords = coords;
    p.r.model = model;
    p.r.tt = (double)threshold * (double)threshold;
    p.r.models = reinterpret_cast<double*>(d_models_out);
    p.r.inliers = d_inliers;
    p.r.corr = reinterpret_cast<double*>(base + L.corr);
    p.r.n_corr = reinterpret_cast<uint32_t*>(base + L.n_corr);
    p.models_in = reinterpret_cast<const double*>(d_models_in);
    p.rounds = d_rounds;
    p.n_rounds = n_rounds;
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_refine(p, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_refine_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                      size_t n_t, const fdf_match* matches, const uint8_t* keep, uint32_t coords,
                      uint32_t model, const fdf_model* model_in, float threshold,
                      uint32_t n_rounds, fdf_model* model_out, uint8_t* inliers_out,
                      uint32_t* rounds_out) {
    RansacLayout L;
    if (!ctx || !model_in || !model_out || refine_layout(1, n_q, &L) != FDF_OK ||
        n_t > fdfk::kMatchMaxCap || !ransac_values_ok(coords, model, threshold) ||
        n_rounds > fdfk::kRefineMaxRounds)
        return FDF_ERR_ARG;
    if (n_q && (!q_coords || !matches)) return FDF_ERR_ARG;
    if (n_t && !t_coords) return FDF_ERR_ARG;
    const uint64_t t_offs[2] = {0, n_t};                  // an asynchronous copy's source
    Arena a(ctx);
    const auto d_q = a.part<fdf_point>(n_q);
    const auto d_t = a.part<fdf_point>(n_t);
    const auto d_m = a.part<fdf_match>(n_q);
    const auto d_keep = a.part<uint8_t>(keep ? n_q : 0);
    const auto d_qo = a.part<uint64_t>(2);
    const auto d_to = a.part<uint64_t>(2);
    const auto d_model = a.part<fdf_model>(1);
    const auto d_rounds = a.part<uint32_t>(1);
    const auto d_in = a.part<uint8_t>(inliers_out ? n_q : 0);
    const auto d_scratch = a.part<uint8_t>(L.total);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    if (n_q) a.upload(d_q, static_cast<const fdf_point*>(q_coords));
    if (n_t) a.upload(d_t, static_cast<const fdf_point*>(t_coords));
    if (n_q) a.upload(d_m, matches);
    if (keep && n_q) a.upload(d_keep, keep);
    a.upload_one_frame(d_qo, n_q);
    a.upload(d_to, t_offs);
    a.upload(d_model, model_in);
    if (a.ok()) {
        const int status = fdf_refine_device(
            ctx, 1, a.at(d_m), keep ? a.at(d_keep) : nullptr, n_q, a.at(d_qo), a.at(d_q),
            a.at(d_t), n_t, a.at(d_to), coords, model, a.at(d_model), threshold, n_rounds,
            a.at(d_model), inliers_out ? a.at(d_in) : nullptr, a.at(d_rounds), a.at(d_scratch),
            L.total, ctx->stream);
        if (status != FDF_OK) return status;
    }
    a.download(model_out, d_model, 1);
    if (rounds_out) a.download(rounds_out, d_rounds, 1);
    if (inliers_out && n_q) a.download(inliers_out, d_in, n_q);
    return a.close();
}

// ---- RANSAC fundamental-matrix estimation (fdf_fundamental.hip) -------------------------------
namespace {

// What the fundamental entries check of the values.
inline bool fundamental_values_ok(uint32_t coords, float threshold) {
    return ransac_values_ok(coords, FDF_MODEL_HOMOGRAPHY, threshold);
}

// The correspondence arrays of a call, as the kernels take them.
fdfk::RansacParams fundamental_params(uint32_t n_frames, const fdf_match* d_matches,
                                      const uint8_t* d_keep, uint64_t q_cap,
                                      const uint64_t* d_q_offsets, const void* d_q_coords,
                                      const void* d_t_coords, uint64_t t_cap,
                                      const uint64_t* d_t_offsets, uint32_t coords,
                                      float threshold, fdf_model* d_models, uint8_t* d_inliers) {
    fdfk::RansacParams p{};
    p.matches = reinterpret_cast<const uint2*>(d_matches);
    p.keep = d_keep;
    p.q_offs = d_q_offsets;
    p.q_cap = q_cap;
    p.q_coords = static_cast<const uint2*>(d_q_coords);
    p.t_coords = static_cast<const uint2*>(d_t_coords);
    p.t_offs = d_t_offsets;
    p.t_cap = t_cap;
    p.n_frames = n_frames;
    p.coords = coords;
    p.tt = (double)threshold * (double)threshold;
    p.models = reinterpret_cast<double*>(d_models);
    p.inliers = d_inliers;
    return p;
}

}  // namespace

int fdf_fundamental_sample(uint32_t seed, uint32_t frame, uint32_t hypothesis, uint32_t m,
                           uint32_t idx[8], uint32_t* draws) {
    if (!idx) return FDF_ERR_ARG;
    uint32_t got[fdfk::kFundamentalSample];
    fdfk::ransac_sample<fdfk::kFundamentalSample, fdfk::kFundamentalMaxDraws>(seed, frame, hypothesis,
                                                                            m, got, draws);
    std::memcpy(idx, got, sizeof(got));
    return FDF_OK;
}

int fdf_fundamental_scratch_bytes(uint32_t n_frames, uint64_t q_cap, uint32_t n_hyp,
                                  uint64_t* bytes) {
    return fdf_ransac_scratch_bytes(n_frames, q_cap, n_hyp, bytes);
}

int fdf_fundamental_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                           const uint8_t* d_keep, uint64_t q_cap, const uint64_t* d_q_offsets,
                           const void* d_q_coords, const void* d_t_coords, uint64_t t_cap,
                           const uint64_t* d_t_offsets, uint32_t coords, uint32_t n_hyp,
                           float threshold, uint32_t seed, fdf_model* d_models,
                           uint8_t* d_inliers, void* d_scratch, uint64_t scratch_bytes,
                           void* stream) {
    RansacLayout L;
    if (!ctx || ransac_layout(n_frames, q_cap, n_hyp, &L) != FDF_OK ||
        t_cap > fdfk::kMatchMaxCap || !fundamental_values_ok(coords, threshold))
        return FDF_ERR_ARG;
    if (n_frames == 0) return FDF_OK;
    if (!d_matches || !d_q_offsets || !d_t_offsets || !d_q_coords || !d_t_coords || !d_models ||
        !d_scratch || scratch_bytes < L.total || ((uintptr_t)d_matches & 7u) != 0 ||
        ((uintptr_t)d_q_coords & 7u) != 0 || ((uintptr_t)d_t_coords & 7u) != 0 ||
        ((uintptr_t)d_models & 7u) != 0 || ((uintptr_t)d_scratch & 255u) != 0)
        return FDF_ERR_ARG;
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    fdfk::RansacParams p =
        fundamental_params(n_frames, d_matches, d_keep, q_cap, d_q_offsets, d_q_coords, d_t_coords,
                           t_cap, d_t_offsets, coords, threshold, d_models, d_inliers);
    p.n_hyp = n_hyp;
    p.seed = seed;
    p.corr = reinterpret_cast<double*>(base + L.corr);
    p.n_corr = reinterpret_cast<uint32_t*>(base + L.n_corr);
    p.counts = reinterpret_cast<uint32_t*>(base + L.counts);
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_fundamental(p, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_fundamental_check_device(fdf_ctx* ctx, uint32_t n_frames, const fdf_match* d_matches,
                                 const uint8_t* d_keep, uint64_t q_cap,
                                 const uint64_t* d_q_offsets, const void* d_q_coords,
                                 const void* d_t_coords, uint64_t t_cap,
                                 const uint64_t* d_t_offsets, uint32_t coords,
                                 const fdf_model* d_models_in, float threshold,
                                 fdf_model* d_models_out, uint8_t* d_inliers, void* stream) {
    if (!ctx || n_frames > 65535u || q_cap > fdfk::kMatchMaxCap || t_cap > fdfk::kMatchMaxCap ||
        !fundamental_values_ok(coords, threshold))
        return FDF_ERR_ARG;
    if (n_frames == 0) return FDF_OK;
    if (!d_matches || !d_q_offsets || !d_t_offsets || !d_q_coords || !d_t_coords || !d_models_in ||
        !d_models_out || ((uintptr_t)d_matches & 7u) != 0 || ((uintptr_t)d_q_coords & 7u) != 0 ||
        ((uintptr_t)d_t_coords & 7u) != 0 || ((uintptr_t)d_models_in & 7u) != 0 ||
        ((uintptr_t)d_models_out & 7u) != 0)
        return FDF_ERR_ARG;
    fdfk::FundamentalCheckParams p{};
    p.r = fundamental_params(n_frames, d_matches, d_keep, q_cap, d_q_offsets, d_q_coords,
                             d_t_coords, t_cap, d_t_offsets, coords, threshold, d_models_out,
                             d_inliers);
    p.models_in = reinterpret_cast<const double*>(d_models_in);
    DeviceGuard guard(ctx->device);
    return status_of(fdfk::launch_fundamental_check(p, reinterpret_cast<hipStream_t>(stream)));
}

int fdf_fundamental_points(fdf_ctx* ctx, const void* q_coords, const void* t_coords, size_t n_q,
                           size_t n_t, const fdf_match* matches, const uint8_t* keep,
                           uint32_t coords, uint32_t n_hyp, float threshold, uint32_t seed,
                           fdf_model* model_out, uint8_t* inliers_out) {
    RansacLayout L;
    if (!ctx || !model_out || ransac_layout(1, n_q, n_hyp, &L) != FDF_OK ||
        n_t > fdfk::kMatchMaxCap || !fundamental_values_ok(coords, threshold))
        return FDF_ERR_ARG;
    if (n_q && (!q_coords || !matches)) return FDF_ERR_ARG;
    if (n_t && !t_coords) return FDF_ERR_ARG;
    const uint64_t t_offs[2] = {0, n_t};                  // an asynchronous copy's source
    Arena a(ctx);
    const auto d_q = a.part<fdf_point>(n_q);
    const auto d_t = a.part<fdf_point>(n_t);
    const auto d_m = a.part<fdf_match>(n_q);
    const auto d_keep = a.part<uint8_t>(keep ? n_q : 0);
    const auto d_qo = a.part<uint64_t>(2);
    const auto d_to = a.part<uint64_t>(2);
    const auto d_model = a.part<fdf_model>(1);
    const auto d_in = a.part<uint8_t>(inliers_out ? n_q : 0);
    const auto d_scratch = a.part<uint8_t>(L.total);
    if (a.open() != FDF_OK) return FDF_ERR_ALLOC;
    if (n_q) a.upload(d_q, static_cast<const fdf_point*>(q_coords));
    if (n_t) a.upload(d_t, static_cast<const fdf_point*>(t_coords));
    if (n_q) a.upload(d_m, matches);
    if (keep && n_q) a.upload(d_keep, keep);
    a.upload_one_frame(d_qo, n_q);
    a.upload(d_to, t_offs);
    if (a.ok()) {
        const int status = fdf_fundamental_device(
            ctx, 1, a.at(d_m), keep ? a.at(d_keep) : nullptr, n_q, a.at(d_qo), a.at(d_q),
            a.at(d_t), n_t, a.at(d_to), coords, n_hyp, threshold, seed, a.at(d_model),
            inliers_out ? a.at(d_in) : nullptr, a.at(d_scratch), L.total, ctx->stream);
        if (status != FDF_OK) return status;
    }
    a.download(model_out, d_model, 1);
    if (inliers_out && n_q) a.download(inliers_out, d_in, n_q);
    return a.close();
}

}  // extern "C"
