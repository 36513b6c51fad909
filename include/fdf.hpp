// fdf.hpp -- header-only C++ mirror of the reference crate API over the C ABI (fdf.h).
//
//   reference (iwanders/feature_detector_fast)          here
//   --------------------------------------------       -----------------------------------
//   Point {x: u32, y: u32}          src/lib.rs:17-20     fdf::Point
//   NonMaximalSuppression           src/lib.rs:26-36     fdf::NonMaximalSuppression
//   Config {threshold,count,nms}    src/lib.rs:40-52     fdf::Config
//   Config::detect(&img)            src/lib.rs:56-58     fdf::Config::detect(img)
//   detect(&img, &config)           src/lib.rs:62-64     fdf::detect(img, config)
//   fast_simd::detector(img, cfg)   src/fast_simd.rs:847 fdf::fast_hip::detector(img, cfg)
//   fast_simd::NORTH..WEST          src/fast_simd.rs:69  fdf::fast_hip::NORTH..WEST
//   fast_simd::circle()             src/fast_simd.rs:79  fdf::fast_hip::circle()
//   fast_simd::calculate_offsets(w) src/fast_simd.rs:104 fdf::fast_hip::calculate_offsets(w)
//   keypoint_score_max_threshold    src/fast_simd.rs:623 fdf::fast_hip::keypoint_score_max_threshold
//   keypoint_score_sum_abs_difference :722               fdf::fast_hip::keypoint_score_sum_abs_difference
//   image::GrayImage                (image 0.24.6)       fdf::GrayView (borrowed row-major u8)
//   (none: callers keep the best K)  --                   fdf::select_best(points, scores, ...)
//   (none: ORB-style callers orient) --                   fdf::keypoint_angles(img, points, ...)
//   (none: ... rank by Harris)       --                   fdf::keypoint_harris(img, points, ...)
//   (none: ... and describe)         --                   fdf::keypoint_descriptors(img, points, ...)
//   (none: ... and match)            --                   fdf::match_descriptors(q_desc, t_desc, ...)
//   (none: ... and fit a model)      --                   fdf::estimate_model(q_points, t_points, matches, ...)
//   (none: ... and refine it)        --                   fdf::refine_model(q_points, t_points, matches, estimate, ...)
//   (none: ... and fit an F matrix)  --                   fdf::estimate_fundamental(q_points, t_points, matches, ...)
//   (none: ... over a scale pyramid) --                   fdf::resize, fdf::pyramid_plan, fdf::build_pyramid
//   (none: ... and warp by the model) --                  fdf::warp, fdf::model_invert
//   (none: ... or track the points)  --                   fdf::track
//   (none: ... and keep the track set) --                 fdf::update_tracks
//
// Where the reference panics (n < 9, n > 16, degenerate sizes) these throw fdf::Error.
// Each thread lazily owns one device context per HIP device (device 0 unless
// fdf::set_device() was called), so the free functions stay pure calls like the reference's.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fdf.h"

namespace fdf {

struct Point {
    uint32_t x = 0;
    uint32_t y = 0;
    bool operator==(const Point& o) const { return x == o.x && y == o.y; }
    bool operator!=(const Point& o) const { return !(*this == o); }
};
static_assert(sizeof(Point) == sizeof(fdf_point), "Point must match the C ABI layout");

enum class NonMaximalSuppression : uint8_t {
    Off = FDF_NMS_OFF,
    MaxThreshold = FDF_NMS_MAX_THRESHOLD,
    SumAbsolute = FDF_NMS_SUM_ABSOLUTE,
};

// A borrowed 8-bit grayscale image: `stride` bytes between rows (GrayImage: == width).
struct GrayView {
    const uint8_t* data = nullptr;
    uint32_t width = 0;
    uint32_t height = 0;
    size_t stride = 0;
    GrayView() = default;
    GrayView(const uint8_t* d, uint32_t w, uint32_t h, size_t s = 0)
        : data(d), width(w), height(h), stride(s ? s : w) {}
};

class Error : public std::runtime_error {
public:
    Error(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

private:
    int status_;
};

inline void check(int status, const char* where) {
    if (status != FDF_OK)
        throw Error(status, std::string(where) + ": " + fdf_status_string(status));
}

// RAII device context (one device, one stream).
class Context {
public:
    explicit Context(int device = 0) {
        fdf_ctx* c = nullptr;
        check(fdf_ctx_create(device, &c), "fdf_ctx_create");
        ctx_.reset(c);
    }
    fdf_ctx* get() const { return ctx_.get(); }

private:
    struct Del {
        void operator()(fdf_ctx* c) const { fdf_ctx_destroy(c); }
    };
    std::unique_ptr<fdf_ctx, Del> ctx_;
};

inline int& current_device() {
    thread_local int dev = 0;
    return dev;
}
inline void set_device(int device) { current_device() = device; }

inline Context& thread_context() {
    thread_local std::vector<std::unique_ptr<Context>> per_device;
    const int dev = current_device();
    if ((int)per_device.size() <= dev) per_device.resize(dev + 1);
    if (!per_device[dev]) per_device[dev].reset(new Context(dev));
    return *per_device[dev];
}

struct Config;
std::vector<Point> detect(const GrayView& img, const Config& config);

struct Config {
    uint8_t threshold = 16;
    uint8_t count = 9;
    NonMaximalSuppression non_maximal_supression = NonMaximalSuppression::Off;

    fdf_config to_c() const {
        fdf_config c;
        c.threshold = threshold;
        c.count = count;
        c.nms = static_cast<uint8_t>(non_maximal_supression);
        return c;
    }
    std::vector<Point> detect(const GrayView& img) const { return fdf::detect(img, *this); }
};

namespace fast_hip {
// First capacity of the two-call pattern: 1 keypoint per 64 pixels (real images have
// 0.5-1.5 per 100).  A denser result is copied out of the context by fdf_fetch_last, so the
// detection runs once either way.
inline size_t capacity_guess(const GrayView& img) {
    const size_t px = (size_t)img.width * img.height;
    return px / 64 > 4096 ? px / 64 : 4096;
}

constexpr size_t NORTH = FDF_NORTH;
constexpr size_t EAST = FDF_EAST;
constexpr size_t SOUTH = FDF_SOUTH;
constexpr size_t WEST = FDF_WEST;

using CircleOffsets = std::array<int32_t, 16>;

inline std::array<std::pair<int32_t, int32_t>, 16> circle() {
    int32_t dx[16], dy[16];
    fdf_circle(dx, dy);
    std::array<std::pair<int32_t, int32_t>, 16> c;
    for (int i = 0; i < 16; ++i) c[i] = {dx[i], dy[i]};
    return c;
}

inline CircleOffsets calculate_offsets(uint32_t width) {
    CircleOffsets o;
    fdf_calculate_offsets(width, o.data());
    return o;
}

// Ring scores on the GPU (fdf_score_rings), one ring per call as the reference's functions;
// batch through fdf_score_rings for many.  `pixels` are the 16 circle pixels in circle() order.
inline uint16_t keypoint_score_max_threshold(uint8_t base_v, const std::array<uint8_t, 16>& pixels,
                                             uint8_t consecutive) {
    fdf_config c{0, consecutive, FDF_NMS_MAX_THRESHOLD};
    uint16_t s = 0;
    check(fdf_score_rings(thread_context().get(), &base_v, pixels.data(), 1, &c, &s),
          "fdf_score_rings");
    return s;
}
inline uint16_t keypoint_score_sum_abs_difference(const std::array<uint8_t, 16>& pixels,
                                                  uint8_t center, uint8_t threshold) {
    fdf_config c{threshold, 9, FDF_NMS_SUM_ABSOLUTE};
    uint16_t s = 0;
    check(fdf_score_rings(thread_context().get(), &center, pixels.data(), 1, &c, &s),
          "fdf_score_rings");
    return s;
}

// Drop-in for fast_simd::detector: result in raster order, bit-identical to the reference.
inline std::vector<Point> detector(const GrayView& img, const Config& config, Context& ctx) {
    const fdf_config c = config.to_c();
    std::vector<Point> out(capacity_guess(img));
    size_t n = 0;
    int rc = fdf_detect(ctx.get(), img.data, img.width, img.height, img.stride, &c,
                        reinterpret_cast<fdf_point*>(out.data()), out.size(), &n);
    if (rc == FDF_ERR_CAPACITY) {   // two-call pattern: copy the retained result
        out.resize(n);
        rc = fdf_fetch_last(ctx.get(), reinterpret_cast<fdf_point*>(out.data()), nullptr,
                            out.size(), &n);
    }
    check(rc, "fdf_detect");
    out.resize(n);
    return out;
}
inline std::vector<Point> detector(const GrayView& img, const Config& config) {
    return detector(img, config, thread_context());
}
}  // namespace fast_hip

// Best-K selection per grid cell (extension, fdf_select_points): of every cell_w x cell_h
// cell (0 = the whole image dimension) of one frame's raster-ordered points, the k of highest
// score, ties to the earlier point; the kept points in input order with their scores.
inline std::pair<std::vector<Point>, std::vector<uint16_t>> select_best(
    const std::vector<Point>& points, const std::vector<uint16_t>& scores, uint32_t width,
    uint32_t height, uint32_t cell_w, uint32_t cell_h, uint32_t k, Context& ctx) {
    if (points.size() != scores.size())
        throw Error(FDF_ERR_ARG, "select_best: points and scores differ in length");
    std::vector<Point> out(points.size());
    std::vector<uint16_t> out_scores(points.size());
    size_t n = 0;
    check(fdf_select_points(ctx.get(), reinterpret_cast<const fdf_point*>(points.data()),
                            scores.data(), nullptr, 1, points.size(), width, height, cell_w,
                            cell_h, k, reinterpret_cast<fdf_point*>(out.data()),
                            out_scores.data(), out.size(), nullptr, &n),
          "fdf_select_points");
    out.resize(n);
    out_scores.resize(n);
    return {std::move(out), std::move(out_scores)};
}
inline std::pair<std::vector<Point>, std::vector<uint16_t>> select_best(
    const std::vector<Point>& points, const std::vector<uint16_t>& scores, uint32_t width,
    uint32_t height, uint32_t cell_w, uint32_t cell_h, uint32_t k) {
    return select_best(points, scores, width, height, cell_w, cell_h, k, thread_context());
}

// Orientation by intensity centroid (extension, fdf_orient_points): atan2f(m01, m10) of the
// disc of `radius` (1..31; ORB's is 15) around every point of one image, radians in
// (-pi, pi] with y pointing down; `moments` (optional) gets m10, m01 per point.
inline std::vector<float> keypoint_angles(const GrayView& img, const std::vector<Point>& points,
                                          uint32_t radius, Context& ctx,
                                          std::vector<int32_t>* moments = nullptr) {
    std::vector<float> angles(points.size());
    if (moments) moments->assign(2 * points.size(), 0);
    check(fdf_orient_points(ctx.get(), img.data, img.width, img.height, img.stride,
                            reinterpret_cast<const fdf_point*>(points.data()), points.size(),
                            radius, angles.data(), moments ? moments->data() : nullptr),
          "fdf_orient_points");
    return angles;
}
inline std::vector<float> keypoint_angles(const GrayView& img, const std::vector<Point>& points,
                                          uint32_t radius = 15,
                                          std::vector<int32_t>* moments = nullptr) {
    return keypoint_angles(img, points, radius, thread_context(), moments);
}

// Harris corner response (extension, fdf_harris_points): the u16 rank score of every point of
// one image, from the `block` x `block` (3, 5 or 7; ORB's is 7) Sobel gradients around it and
// the Harris constant k_num / k_den (ORB's 0.04 is 1 / 25); the pair select_best takes.
// `responses` (optional) gets the exact int64 response per point.
inline std::vector<uint16_t> keypoint_harris(const GrayView& img, const std::vector<Point>& points,
                                             uint32_t block, uint32_t k_num, uint32_t k_den,
                                             Context& ctx,
                                             std::vector<int64_t>* responses = nullptr) {
    std::vector<uint16_t> scores(points.size());
    if (responses) responses->assign(points.size(), 0);
    check(fdf_harris_points(ctx.get(), img.data, img.width, img.height, img.stride,
                            reinterpret_cast<const fdf_point*>(points.data()), points.size(),
                            block, k_num, k_den, scores.data(),
                            responses ? responses->data() : nullptr),
          "fdf_harris_points");
    return scores;
}
inline std::vector<uint16_t> keypoint_harris(const GrayView& img, const std::vector<Point>& points,
                                             uint32_t block = 7, uint32_t k_num = 1,
                                             uint32_t k_den = 25,
                                             std::vector<int64_t>* responses = nullptr) {
    return keypoint_harris(img, points, block, k_num, k_den, thread_context(), responses);
}

// Steered BRIEF descriptors (extension, fdf_describe_points): 32 bytes per point of one image,
// test i in bit i % 8 of byte i / 8.  `angles` (optional, one per point, as keypoint_angles
// returns them) pick one of `n_bins` (1..360) rotations of `pattern` (optional, 256 tests of
// x0, y0, x1, y1; the default is fdf_brief_pattern's); with `smooth` the tests read the
// 5 x 5 box-smoothed image.
inline std::vector<uint8_t> keypoint_descriptors(const GrayView& img,
                                                 const std::vector<Point>& points,
                                                 const std::vector<float>* angles,
                                                 const std::array<int8_t, 1024>* pattern,
                                                 uint32_t n_bins, bool smooth, Context& ctx) {
    if (angles && angles->size() != points.size())
        throw Error(FDF_ERR_ARG, "keypoint_descriptors: one angle per point");
    std::vector<uint8_t> desc(32 * points.size());
    check(fdf_describe_points(ctx.get(), img.data, img.width, img.height, img.stride,
                              reinterpret_cast<const fdf_point*>(points.data()), points.size(),
                              angles ? angles->data() : nullptr,
                              pattern ? pattern->data() : nullptr, n_bins, smooth ? 1 : 0,
                              desc.data()),
          "fdf_describe_points");
    return desc;
}
inline std::vector<uint8_t> keypoint_descriptors(const GrayView& img,
                                                 const std::vector<Point>& points,
                                                 const std::vector<float>* angles = nullptr,
                                                 const std::array<int8_t, 1024>* pattern = nullptr,
                                                 uint32_t n_bins = 30, bool smooth = true) {
    return keypoint_descriptors(img, points, angles, pattern, n_bins, smooth, thread_context());
}

// Brute-force Hamming matching of two descriptor sets (extension, fdf_match_points): for
// every query descriptor (32 bytes each) the index of the nearest train descriptor (ties: the
// lowest index; FDF_MATCH_NONE without a candidate), its distance and the distance of the
// second nearest (0xFFFF: none).  With both point lists (one point per descriptor, the train
// points' y non-decreasing) only train points with |dx| <= max_dx and |dy| <= max_dy are
// candidates; without them max_dx and max_dy are ignored.
using Match = fdf_match;
inline std::vector<Match> match_descriptors(const std::vector<uint8_t>& q_desc,
                                            const std::vector<uint8_t>& t_desc,
                                            const std::vector<Point>* q_points,
                                            const std::vector<Point>* t_points, uint32_t max_dx,
                                            uint32_t max_dy, Context& ctx) {
    if (q_desc.size() % 32 || t_desc.size() % 32)
        throw Error(FDF_ERR_ARG, "match_descriptors: 32 bytes per descriptor");
    const size_t n_q = q_desc.size() / 32, n_t = t_desc.size() / 32;
    if ((q_points && q_points->size() != n_q) || (t_points && t_points->size() != n_t))
        throw Error(FDF_ERR_ARG, "match_descriptors: one point per descriptor");
    std::vector<Match> out(n_q);
    // an empty list is still a list: the C entry tells "no window" by NULL
    auto pts = [](const std::vector<Point>* v) -> const fdf_point* {
        static const fdf_point none = {0, 0};
        if (!v) return nullptr;
        return v->empty() ? &none : reinterpret_cast<const fdf_point*>(v->data());
    };
    check(fdf_match_points(ctx.get(), q_desc.data(), pts(q_points), n_q, t_desc.data(),
                           pts(t_points), n_t, max_dx, max_dy, out.data()),
          "fdf_match_points");
    return out;
}
inline std::vector<Match> match_descriptors(const std::vector<uint8_t>& q_desc,
                                            const std::vector<uint8_t>& t_desc,
                                            const std::vector<Point>* q_points = nullptr,
                                            const std::vector<Point>* t_points = nullptr,
                                            uint32_t max_dx = 0, uint32_t max_dy = 0) {
    return match_descriptors(q_desc, t_desc, q_points, t_points, max_dx, max_dy, thread_context());
}

// RANSAC estimation of the affine map or homography that takes the query points to their
// matches (extension, fdf_ransac_points; include/fdf.h has the sampling, fit and score rules:
// the result is a pure function of the inputs and the seed).  `matches` holds one entry per query
// point (match_descriptors' result), `keep` (optional) one flag per query.
struct ModelEstimate {
    fdf_model model;                  // h row-major; hypothesis == FDF_RANSAC_NONE: no model
    std::vector<uint8_t> inliers;     // 1 for the queries that are inliers of the model
    bool found() const { return model.hypothesis != FDF_RANSAC_NONE; }
};
inline ModelEstimate estimate_model(const std::vector<Point>& q_points,
                                    const std::vector<Point>& t_points,
                                    const std::vector<Match>& matches,
                                    const std::vector<uint8_t>* keep, uint32_t model,
                                    uint32_t n_hyp, float threshold, uint32_t seed, Context& ctx) {
    if (matches.size() != q_points.size() || (keep && keep->size() != q_points.size()))
        throw Error(FDF_ERR_ARG, "estimate_model: one match and keep flag per query point");
    ModelEstimate out;
    out.inliers.resize(q_points.size());
    check(fdf_ransac_points(ctx.get(), q_points.data(), t_points.data(), q_points.size(),
                            t_points.size(), matches.data(), keep ? keep->data() : nullptr,
                            FDF_COORDS_U32, model, n_hyp, threshold, seed, &out.model,
                            out.inliers.data()),
          "fdf_ransac_points");
    return out;
}
inline ModelEstimate estimate_model(const std::vector<Point>& q_points,
                                    const std::vector<Point>& t_points,
                                    const std::vector<Match>& matches,
                                    const std::vector<uint8_t>* keep = nullptr,
                                    uint32_t model = FDF_MODEL_HOMOGRAPHY, uint32_t n_hyp = 256,
                                    float threshold = 3.0f, uint32_t seed = 0) {
    return estimate_model(q_points, t_points, matches, keep, model, n_hyp, threshold, seed,
                          thread_context());
}

// Least-squares refinement of estimate_model's result over its inliers (extension,
// fdf_refine_points; include/fdf.h has the normalisation, the order of the sums and the
// acceptance rule).  The point sets, `matches` and `keep` are estimate_model's; at most
// `n_rounds` (0..8) rounds, each kept only if it loses no inlier under `threshold`.
struct RefinedModel {
    fdf_model model;                  // hypothesis and n_valid as they came
    std::vector<uint8_t> inliers;     // 1 for the queries that are inliers of the refined model
    uint32_t rounds = 0;              // rounds accepted
    bool found() const { return model.hypothesis != FDF_RANSAC_NONE; }
};
inline RefinedModel refine_model(const std::vector<Point>& q_points,
                                 const std::vector<Point>& t_points,
                                 const std::vector<Match>& matches,
                                 const std::vector<uint8_t>* keep, uint32_t model,
                                 const fdf_model& estimate, float threshold, uint32_t n_rounds,
                                 Context& ctx) {
    if (matches.size() != q_points.size() || (keep && keep->size() != q_points.size()))
        throw Error(FDF_ERR_ARG, "refine_model: one match and keep flag per query point");
    RefinedModel out;
    out.inliers.resize(q_points.size());
    check(fdf_refine_points(ctx.get(), q_points.data(), t_points.data(), q_points.size(),
                            t_points.size(), matches.data(), keep ? keep->data() : nullptr,
                            FDF_COORDS_U32, model, &estimate, threshold, n_rounds, &out.model,
                            out.inliers.data(), &out.rounds),
          "fdf_refine_points");
    return out;
}
inline RefinedModel refine_model(const std::vector<Point>& q_points,
                                 const std::vector<Point>& t_points,
                                 const std::vector<Match>& matches, const fdf_model& estimate,
                                 const std::vector<uint8_t>* keep = nullptr,
                                 uint32_t model = FDF_MODEL_HOMOGRAPHY, float threshold = 3.0f,
                                 uint32_t n_rounds = 2) {
    return refine_model(q_points, t_points, matches, keep, model, estimate, threshold, n_rounds,
                        thread_context());
}

// RANSAC estimation of the fundamental matrix F of the matches, [u v 1] F [x y 1]^T = 0 for a
// query (x, y) and its train point (u, v) (extension, fdf_fundamental_points; include/fdf.h has
// the sampling, fit and score rules): the epipolar outlier test of a moving camera or a stereo
// pair.  The arguments are estimate_model's without `model`; `threshold` is a Sampson distance in
// pixels.  model.h holds F, scaled so that its largest entry is +1.
inline ModelEstimate estimate_fundamental(const std::vector<Point>& q_points,
                                          const std::vector<Point>& t_points,
                                          const std::vector<Match>& matches,
                                          const std::vector<uint8_t>* keep, uint32_t n_hyp,
                                          float threshold, uint32_t seed, Context& ctx) {
    if (matches.size() != q_points.size() || (keep && keep->size() != q_points.size()))
        throw Error(FDF_ERR_ARG, "estimate_fundamental: one match and keep flag per query point");
    ModelEstimate out;
    out.inliers.resize(q_points.size());
    check(fdf_fundamental_points(ctx.get(), q_points.data(), t_points.data(), q_points.size(),
                                 t_points.size(), matches.data(), keep ? keep->data() : nullptr,
                                 FDF_COORDS_U32, n_hyp, threshold, seed, &out.model,
                                 out.inliers.data()),
          "fdf_fundamental_points");
    return out;
}
inline ModelEstimate estimate_fundamental(const std::vector<Point>& q_points,
                                          const std::vector<Point>& t_points,
                                          const std::vector<Match>& matches,
                                          const std::vector<uint8_t>* keep = nullptr,
                                          uint32_t n_hyp = 256, float threshold = 1.0f,
                                          uint32_t seed = 0) {
    return estimate_fundamental(q_points, t_points, matches, keep, n_hyp, threshold, seed,
                                thread_context());
}

// Exact bilinear resize and the scale pyramid (extension, fdf_resize_frame and
// fdf_pyramid_plan): integer-exact, one rounding per pixel (include/fdf.h has the rule).
struct Image {
    uint32_t width = 0;
    uint32_t height = 0;
    std::vector<uint8_t> pixels;   // rows packed
    GrayView view() const { return GrayView(pixels.data(), width, height); }
};
inline Image resize(const GrayView& img, uint32_t dst_w, uint32_t dst_h, Context& ctx) {
    Image out;
    out.width = dst_w;
    out.height = dst_h;
    out.pixels.resize((size_t)dst_w * dst_h);
    check(fdf_resize_frame(ctx.get(), img.data, img.width, img.height, img.stride,
                           out.pixels.data(), dst_w, dst_h, dst_w),
          "fdf_resize_frame");
    return out;
}
inline Image resize(const GrayView& img, uint32_t dst_w, uint32_t dst_h) {
    return resize(img, dst_w, dst_h, thread_context());
}

// The levels of a pyramid of `n_levels` at the factor num / den (> 1; ORB's 1.2 is 6 / 5) over
// n_frames frames of width x height: sizes, offsets into one pyramid buffer and one taps array.
struct PyramidPlan {
    std::vector<fdf_pyramid_level> levels;
    uint64_t total_bytes = 0;
    uint64_t total_taps = 0;
};
inline PyramidPlan pyramid_plan(uint32_t width, uint32_t height, uint32_t n_levels = 8,
                                uint32_t num = 6, uint32_t den = 5, uint32_t n_frames = 1) {
    PyramidPlan plan;
    plan.levels.resize(n_levels ? n_levels : 1);
    check(fdf_pyramid_plan(width, height, num, den, n_levels, n_frames, plan.levels.data(),
                           &plan.total_bytes, &plan.total_taps),
          "fdf_pyramid_plan");
    return plan;
}

// The pyramid of one host frame: level 0 is a packed copy of `img`, level l is level l - 1
// resized to the plan's size.
inline std::vector<Image> build_pyramid(const GrayView& img, uint32_t n_levels, uint32_t num,
                                        uint32_t den, Context& ctx) {
    const PyramidPlan plan = pyramid_plan(img.width, img.height, n_levels, num, den);
    std::vector<Image> levels(n_levels);
    levels[0].width = img.width;
    levels[0].height = img.height;
    levels[0].pixels.resize((size_t)img.width * img.height);
    for (uint32_t y = 0; y < img.height; ++y)
        std::copy(img.data + y * img.stride, img.data + y * img.stride + img.width,
                  levels[0].pixels.begin() + (size_t)y * img.width);
    for (uint32_t l = 1; l < n_levels; ++l)
        levels[l] = resize(levels[l - 1].view(), plan.levels[l].width, plan.levels[l].height, ctx);
    return levels;
}
inline std::vector<Image> build_pyramid(const GrayView& img, uint32_t n_levels = 8,
                                        uint32_t num = 6, uint32_t den = 5) {
    return build_pyramid(img, n_levels, num, den, thread_context());
}

// Exact bilinear warp by a 3 x 3 model (extension, fdf_warp_frame; include/fdf.h has the rule).
// `h` (row-major, ModelEstimate::model.h as estimated) maps a destination pixel to a source
// position: warping the train frame with it registers it onto the query frame.  `mask`
// (optional) gets 1 where the position lies inside the source frame.
inline Image warp(const GrayView& img, const double (&h)[9], uint32_t dst_w, uint32_t dst_h,
                  uint32_t border, uint32_t fill, std::vector<uint8_t>* mask, Context& ctx) {
    Image out;
    out.width = dst_w;
    out.height = dst_h;
    out.pixels.resize((size_t)dst_w * dst_h);
    if (mask) mask->assign((size_t)dst_w * dst_h, 0);
    check(fdf_warp_frame(ctx.get(), img.data, img.width, img.height, img.stride, h,
                         out.pixels.data(), dst_w, dst_h, dst_w, border, fill,
                         mask ? mask->data() : nullptr),
          "fdf_warp_frame");
    return out;
}
inline Image warp(const GrayView& img, const double (&h)[9], uint32_t dst_w, uint32_t dst_h,
                  uint32_t border = FDF_BORDER_REPLICATE, uint32_t fill = 0,
                  std::vector<uint8_t>* mask = nullptr) {
    return warp(img, h, dst_w, dst_h, border, fill, mask, thread_context());
}

// The model that warps the other way (fdf_model_invert); throws FDF_ERR_ARG for a singular one.
inline std::array<double, 9> model_invert(const double (&h)[9]) {
    std::array<double, 9> out{};
    check(fdf_model_invert(h, out.data()), "fdf_model_invert");
    return out;
}

// Pyramidal Lucas-Kanade tracking of `points` (pixels) of `prev` into `next`, two frames of one
// size (extension, fdf_track_frames; include/fdf.h has the rule).  Entry k of every array belongs
// to point k: q11 is the position in 1/2048 pixel ((-1, -1) for a lost point), xy the same in
// pixels, info = reason | iterations << 8 (reason 1 = tracked).
struct TrackOptions {
    uint32_t n_levels = 3, num = 2, den = 1;   // the pyramid: levels and the factor between them
    uint32_t radius = 10, max_iters = 30, eps = 20;
    float min_eig = 1.0f;
};
struct Tracks {
    std::vector<std::array<int32_t, 2>> q11;
    std::vector<std::array<float, 2>> xy;
    std::vector<uint8_t> status;
    std::vector<uint32_t> err, info;
};
inline Tracks track(const GrayView& prev, const GrayView& next, const std::vector<Point>& points,
                    const TrackOptions& opt, Context& ctx) {
    if (prev.width != next.width || prev.height != next.height || prev.stride != next.stride)
        throw Error(FDF_ERR_ARG, "fdf::track: the frames differ in size or stride");
    const size_t n = points.size();
    Tracks t;
    t.q11.assign(n, {-1, -1});
    t.xy.assign(n, {-1.0f, -1.0f});
    t.status.assign(n, 0);
    t.err.assign(n, 0xFFFFFFFFu);
    t.info.assign(n, 0);
    check(fdf_track_frames(ctx.get(), prev.data, next.data, prev.width, prev.height, prev.stride,
                           points.data(), FDF_COORDS_U32, n, nullptr, opt.n_levels, opt.num,
                           opt.den, opt.radius, opt.max_iters, opt.eps, opt.min_eig,
                           n ? t.q11[0].data() : nullptr, n ? t.xy[0].data() : nullptr,
                           t.status.data(), t.err.data(), t.info.data()),
          "fdf_track_frames");
    return t;
}
inline Tracks track(const GrayView& prev, const GrayView& next, const std::vector<Point>& points,
                    const TrackOptions& opt = TrackOptions()) {
    return track(prev, next, points, opt, thread_context());
}

// Track-set maintenance between two tracking calls (extension, fdf_tracks_update_points;
// include/fdf.h has the rule): lost and border tracks are dropped, of two tracks within min_dist
// the older stays, the strongest candidates no survivor is near refill the set up to max_tracks.
// Entry k of every array belongs to track k; `src` is a survivor's index in the input set or
// FDF_TRACKS_NEW | the candidate's index.  `next_id` is read and advanced.
struct TrackSetOptions {
    uint32_t min_dist = 16, margin = 11, max_tracks = 1024, passes = 8;
};
struct TrackSet {
    std::vector<std::array<int32_t, 2>> q11;
    std::vector<uint32_t> ids, ages, src;
    std::vector<uint8_t> status;               // input only: empty means every track is tracked
};
inline TrackSet update_tracks(uint32_t width, uint32_t height, const TrackSet& tracks,
                              const std::vector<Point>& candidates,
                              const std::vector<uint16_t>& scores, uint32_t& next_id,
                              const TrackSetOptions& opt, Context& ctx) {
    const size_t nt = tracks.q11.size(), nc = candidates.size();
    if (tracks.ids.size() != nt || tracks.ages.size() != nt || scores.size() != nc ||
        (!tracks.status.empty() && tracks.status.size() != nt))
        throw Error(FDF_ERR_ARG, "fdf::update_tracks: the arrays differ in length");
    const fdf_tracks_params params{width, height, opt.min_dist, opt.margin, opt.max_tracks,
                                   opt.passes};
    TrackSet out;
    size_t cap = nt + std::min<size_t>(nc, opt.max_tracks), n = 0;
    out.q11.resize(cap);
    out.ids.resize(cap);
    out.ages.resize(cap);
    out.src.resize(cap);
    check(fdf_tracks_update_points(ctx.get(), &params, nt ? tracks.q11[0].data() : nullptr,
                                   tracks.status.empty() ? nullptr : tracks.status.data(),
                                   tracks.ids.data(), tracks.ages.data(), nt,
                                   reinterpret_cast<const fdf_point*>(candidates.data()),
                                   scores.data(), nc, &next_id, cap ? out.q11[0].data() : nullptr,
                                   out.ids.data(), out.ages.data(), out.src.data(), cap, &n),
          "fdf_tracks_update_points");
    out.q11.resize(n);
    out.ids.resize(n);
    out.ages.resize(n);
    out.src.resize(n);
    return out;
}
inline TrackSet update_tracks(uint32_t width, uint32_t height, const TrackSet& tracks,
                              const std::vector<Point>& candidates,
                              const std::vector<uint16_t>& scores, uint32_t& next_id,
                              const TrackSetOptions& opt = TrackSetOptions()) {
    return update_tracks(width, height, tracks, candidates, scores, next_id, opt,
                         thread_context());
}

inline std::vector<Point> detect(const GrayView& img, const Config& config) {
    return fast_hip::detector(img, config);
}

}  // namespace fdf
