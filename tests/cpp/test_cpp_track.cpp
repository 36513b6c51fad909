// fdf::track smoke test (include/fdf.hpp), run by tests/test_gpu_track.py on a GPU box.
// Usage: test_cpp_track
// The worked example of include/fdf.h: the 32 x 24 frames A and B = A moved by (2, 1), the point
// (14, 10), r = 3, eps 20; every number the header quotes for one and two levels, max_iters = 1
// and min_eig = 1.0 is checked, then a constant frame, a point outside the frame and the
// rejected arguments.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

int failures = 0;

void expect(const fdf::Tracks& t, size_t k, int x, int y, uint32_t err, uint32_t reason,
            uint32_t iters, const char* what) {
    const bool tracked = reason == 1;
    if (t.q11[k][0] != x || t.q11[k][1] != y || t.err[k] != err || t.info[k] != (reason | iters << 8) ||
        t.status[k] != (tracked ? 1 : 0) ||
        t.xy[k][0] != (tracked ? (float)(x / 2048.0) : -1.0f) ||
        t.xy[k][1] != (tracked ? (float)(y / 2048.0) : -1.0f)) {
        std::fprintf(stderr, "%s: got (%d, %d) err %u info %#x status %u\n", what, t.q11[k][0],
                     t.q11[k][1], t.err[k], t.info[k], t.status[k]);
        ++failures;
    }
}

template <typename F>
void expect_throw(F f, int status, const char* what) {
    try {
        f();
        std::fprintf(stderr, "%s did not throw\n", what);
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != status) {
            std::fprintf(stderr, "%s threw %d\n", what, e.status());
            ++failures;
        }
    }
}

}  // namespace

int main() {
    const int w = 32, h = 24;
    std::vector<uint8_t> a(w * h), b(w * h), flat(w * h, 7);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int dx = x - 16, dy = y - 12;
            a[y * w + x] = (uint8_t)std::min(255, (dx * dx + 2 * dy * dy + dx * dy) >> 2);
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            b[y * w + x] = a[std::clamp(y - 1, 0, h - 1) * w + std::clamp(x - 2, 0, w - 1)];
    const fdf::GrayView va(a.data(), w, h), vb(b.data(), w, h), vf(flat.data(), w, h);
    const std::vector<fdf::Point> pts = {{14, 10}, {40, 10}};     // the second lies outside

    fdf::TrackOptions opt;
    opt.n_levels = 1;
    opt.radius = 3;
    opt.min_eig = 0.25f;
    const uint32_t none = 0xFFFFFFFFu;
    fdf::Tracks t = fdf::track(va, vb, pts, opt);
    expect(t, 0, 32773, 22529, 0, 1, 4, "one level");
    expect(t, 1, -1, -1, none, 0, 0, "a point outside the frame");
    opt.max_iters = 1;
    expect(fdf::track(va, vb, pts, opt), 0, 33605, 23077, 1789, 1, 1, "max_iters = 1");
    opt.max_iters = 30;
    opt.min_eig = 1.0f;
    expect(fdf::track(va, vb, pts, opt), 0, -1, -1, none, 2, 0, "min_eig = 1");
    opt.min_eig = 0.25f;
    opt.n_levels = 2;
    expect(fdf::track(va, vb, pts, opt), 0, 32773, 22530, 0, 1, 5, "two levels");
    opt.n_levels = 1;
    opt.min_eig = 0.0f;
    expect(fdf::track(vf, vf, pts, opt), 0, -1, -1, none, 2, 0, "a constant frame");
    if (!fdf::track(va, vb, {}, opt).q11.empty()) ++failures;

    opt.radius = 16;
    expect_throw([&] { (void)fdf::track(va, vb, pts, opt); }, FDF_ERR_ARG, "radius 16");
    opt.radius = 3;
    opt.max_iters = 0;
    expect_throw([&] { (void)fdf::track(va, vb, pts, opt); }, FDF_ERR_ARG, "max_iters 0");
    opt.max_iters = 30;
    opt.min_eig = -1.0f;
    expect_throw([&] { (void)fdf::track(va, vb, pts, opt); }, FDF_ERR_ARG, "min_eig -1");
    opt.min_eig = 0.25f;
    opt.n_levels = 33;
    expect_throw([&] { (void)fdf::track(va, vb, pts, opt); }, FDF_ERR_ARG, "33 levels");
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
