// fdf::resize / fdf::pyramid_plan / fdf::build_pyramid smoke test (include/fdf.hpp), run by
// tests/test_gpu_resize.py on a GPU box.
// Usage: test_cpp_pyramid
// A pseudo-random 97 x 61 frame is resized to several sizes (down, identity, exact halving, a
// ratio above 2, up) and built into a 4-level 6 / 5 pyramid; every pixel is compared with a plain
// restatement of include/fdf.h's rule.
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

struct Tap { int64_t i0, i1, q; };

Tap tap_of(int64_t S, int64_t D, int64_t i) {
    const int64_t N = (2 * i + 1) * S - D;
    Tap t{0, 0, 0};
    if (N >= 0) {
        t.i0 = N / (2 * D);
        t.q = (4096 * (N % (2 * D)) + 2 * D) / (4 * D);
    }
    if (t.i0 >= S - 1) {
        t.i0 = S > 1 ? S - 2 : 0;
        t.q = S > 1 ? 2048 : 0;
    }
    t.i1 = t.i0 + 1 < S ? t.i0 + 1 : S - 1;
    return t;
}

std::vector<uint8_t> resize_ref(const std::vector<uint8_t>& src, int sw, int sh, int dw, int dh) {
    std::vector<uint8_t> out((size_t)dw * dh);
    for (int y = 0; y < dh; ++y) {
        const Tap ty = tap_of(sh, dh, y);
        for (int x = 0; x < dw; ++x) {
            const Tap tx = tap_of(sw, dw, x);
            const int64_t h0 = src[ty.i0 * sw + tx.i0] * (2048 - tx.q) + src[ty.i0 * sw + tx.i1] * tx.q;
            const int64_t h1 = src[ty.i1 * sw + tx.i0] * (2048 - tx.q) + src[ty.i1 * sw + tx.i1] * tx.q;
            out[(size_t)y * dw + x] = (uint8_t)((h0 * (2048 - ty.q) + h1 * ty.q + (1 << 21)) >> 22);
        }
    }
    return out;
}

}  // namespace

int main() {
    const int w = 97, h = 61;
    std::vector<uint8_t> img(w * h);
    uint32_t state = 2463534242u;
    for (auto& p : img) {
        state = state * 1664525u + 1013904223u;
        p = (uint8_t)(state >> 24);
    }
    int failures = 0;
    const fdf::GrayView view(img.data(), w, h);

    const int sizes[][2] = {{81, 51}, {97, 61}, {48, 30}, {40, 25}, {131, 80}, {3, 2}, {1, 1}};
    for (const auto& s : sizes) {
        const fdf::Image got = fdf::resize(view, s[0], s[1]);
        if (got.width != (uint32_t)s[0] || got.height != (uint32_t)s[1] ||
            got.pixels != resize_ref(img, w, h, s[0], s[1])) {
            std::fprintf(stderr, "resize to %d x %d differs\n", s[0], s[1]);
            ++failures;
        }
    }
    if (fdf::resize(view, w, h).pixels != img) ++failures;           // D = S is the identity

    // a padded source: rows 5 bytes further apart
    std::vector<uint8_t> padded((w + 5) * h, 0xEE);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) padded[y * (w + 5) + x] = img[y * w + x];
    if (fdf::resize(fdf::GrayView(padded.data(), w, h, w + 5), 81, 51).pixels !=
        resize_ref(img, w, h, 81, 51))
        ++failures;

    const fdf::PyramidPlan plan = fdf::pyramid_plan(w, h, 4, 6, 5, 3);
    const uint32_t want[4][2] = {{97, 61}, {81, 51}, {68, 43}, {57, 36}};
    uint64_t end = 0;
    for (int l = 0; l < 4; ++l) {
        const fdf_pyramid_level& L = plan.levels[l];
        if (L.width != want[l][0] || L.height != want[l][1]) ++failures;
        if (l == 0) continue;
        if (L.offset_bytes % 256 || L.offset_bytes < end ||
            L.frame_stride_bytes != (uint64_t)L.width * L.height)
            ++failures;
        end = L.offset_bytes + 3 * L.frame_stride_bytes;
    }
    if (plan.total_bytes < end || plan.total_taps != 81 + 51 + 68 + 43 + 57 + 36) ++failures;

    const std::vector<fdf::Image> pyr = fdf::build_pyramid(view, 4);
    std::vector<uint8_t> level = img;
    if (pyr.size() != 4 || pyr[0].pixels != img) ++failures;
    for (size_t l = 1; l < pyr.size(); ++l) {
        level = resize_ref(level, want[l - 1][0], want[l - 1][1], want[l][0], want[l][1]);
        if (pyr[l].width != want[l][0] || pyr[l].height != want[l][1] || pyr[l].pixels != level) {
            std::fprintf(stderr, "pyramid level %zu differs\n", l);
            ++failures;
        }
    }

    for (const auto& bad : {std::pair<uint32_t, uint32_t>{5, 6}, {6, 0}}) {
        try {
            (void)fdf::pyramid_plan(w, h, 4, bad.first, bad.second);
            std::fprintf(stderr, "factor %u / %u did not throw\n", bad.first, bad.second);
            ++failures;
        } catch (const fdf::Error& e) {
            if (e.status() != FDF_ERR_ARG) ++failures;
        }
    }
    try {
        (void)fdf::resize(view, 0, 5);
        std::fprintf(stderr, "a zero width did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_SIZE) ++failures;
    }
    std::printf("levels=%zu failures=%d\n", pyr.size(), failures);
    return failures ? 1 : 0;
}
