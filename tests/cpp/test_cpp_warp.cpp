// fdf::warp / fdf::model_invert smoke test (include/fdf.hpp), run by tests/test_gpu_warp.py on a
// GPU box.
// Usage: test_cpp_warp
// A pseudo-random 97 x 61 frame is warped by the identity, an integer shift, a half-pixel shift,
// a rotation and a homography, under both borders and with the mask; every pixel is compared with
// a plain restatement of include/fdf.h's rule (this file is built for the baseline x86-64, which
// has no fused multiply-add).  The header's 4 x 4 example is checked value by value.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

struct Warped { std::vector<uint8_t> pixels, mask; };

Warped warp_ref(const std::vector<uint8_t>& src, int sw, int sh, const double (&h)[9], int dw,
                int dh, uint32_t border, uint32_t fill) {
    Warped out;
    out.pixels.resize((size_t)dw * dh);
    out.mask.resize((size_t)dw * dh);
    const double lim = 1073741824.0;
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            const double xd = x, yd = y;
            const double p = (h[0] * xd + h[1] * yd) + h[2];
            const double q = (h[3] * xd + h[4] * yd) + h[5];
            const double w = (h[6] * xd + h[7] * yd) + h[8];
            const double FX = std::floor((p / w) * 2048.0 + 0.5);
            const double FY = std::floor((q / w) * 2048.0 + 0.5);
            const bool valid = w > 0 && FX >= -lim && FX <= lim && FY >= -lim && FY <= lim;
            uint8_t value = (uint8_t)fill, inside = 0;
            if (valid) {
                const int64_t X = (int64_t)FX, Y = (int64_t)FY;
                const int64_t ix = X >> 11, iy = Y >> 11, qx = X & 2047, qy = Y & 2047;
                auto tap = [&](int64_t cx, int64_t cy) -> int64_t {
                    const bool in = cx >= 0 && cx < sw && cy >= 0 && cy < sh;
                    if (!in && border == FDF_BORDER_CONSTANT) return fill;
                    cx = cx < 0 ? 0 : cx > sw - 1 ? sw - 1 : cx;
                    cy = cy < 0 ? 0 : cy > sh - 1 ? sh - 1 : cy;
                    return src[cy * sw + cx];
                };
                const int64_t s = (2048 - qy) * ((2048 - qx) * tap(ix, iy) + qx * tap(ix + 1, iy)) +
                                  qy * ((2048 - qx) * tap(ix, iy + 1) + qx * tap(ix + 1, iy + 1));
                value = (uint8_t)((s + (1 << 21)) >> 22);
                inside = X >= 0 && X <= (int64_t)(sw - 1) * 2048 && Y >= 0 &&
                         Y <= (int64_t)(sh - 1) * 2048;
            }
            out.pixels[(size_t)y * dw + x] = value;
            out.mask[(size_t)y * dw + x] = inside;
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

    const double c = std::cos(0.5), s = std::sin(0.5);
    const double models[][9] = {
        {1, 0, 0, 0, 1, 0, 0, 0, 1},
        {1, 0, 3, 0, 1, 5, 0, 0, 1},
        {1, 0, 0.5, 0, 1, 0, 0, 0, 1},
        {c, -s, 48 - 48 * c + 30 * s, s, c, 30 - 48 * s - 30 * c, 0, 0, 1},
        {1.02, 0.03, -4.5, -0.02, 0.97, 3.25, 0.0004, -0.0003, 1},
        {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    const int sizes[][2] = {{97, 61}, {53, 40}, {3, 5}};
    for (const auto& m : models)
        for (const auto& d : sizes)
            for (uint32_t border : {FDF_BORDER_REPLICATE, FDF_BORDER_CONSTANT}) {
                std::vector<uint8_t> mask;
                const fdf::Image got = fdf::warp(view, m, d[0], d[1], border, 7, &mask);
                const Warped want = warp_ref(img, w, h, m, d[0], d[1], border, 7);
                if (got.width != (uint32_t)d[0] || got.height != (uint32_t)d[1] ||
                    got.pixels != want.pixels || mask != want.mask) {
                    std::fprintf(stderr, "warp to %d x %d, border %u differs\n", d[0], d[1], border);
                    ++failures;
                }
            }
    if (fdf::warp(view, models[0], w, h).pixels != img) ++failures;      // the identity is a copy

    // a padded source: rows 5 bytes further apart
    std::vector<uint8_t> padded((w + 5) * h, 0xEE);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) padded[y * (w + 5) + x] = img[y * w + x];
    if (fdf::warp(fdf::GrayView(padded.data(), w, h, w + 5), models[4], 53, 40).pixels !=
        warp_ref(img, w, h, models[4], 53, 40, FDF_BORDER_REPLICATE, 0).pixels)
        ++failures;

    // the header's example
    std::vector<uint8_t> ramp(16);
    for (int i = 0; i < 16; ++i) ramp[i] = (uint8_t)(16 * i);
    const double ex[9] = {0.75, 0.25, 0.5, -0.25, 0.75, 1, 0.0625, 0, 1};
    const std::vector<uint8_t> rows = {72, 64, 57, 51, 124, 113, 103, 94,
                                       176, 162, 149, 138, 223, 211, 196, 182};
    std::vector<uint8_t> ex_mask;
    if (fdf::warp(fdf::GrayView(ramp.data(), 4, 4), ex, 4, 4, FDF_BORDER_CONSTANT, 255, &ex_mask)
            .pixels != rows)
        ++failures;
    for (int i = 0; i < 16; ++i)
        if (ex_mask[i] != (i == 12 ? 0 : 1)) ++failures;

    // the inverse of the shift is the opposite shift; a singular model throws
    const std::array<double, 9> inv = fdf::model_invert(models[1]);
    const double back[9] = {1, 0, -3, 0, 1, -5, 0, 0, 1};
    for (int k = 0; k < 9; ++k)
        if (inv[k] != back[k]) ++failures;
    try {
        (void)fdf::model_invert(models[5]);
        std::fprintf(stderr, "a singular model did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    try {
        (void)fdf::warp(view, models[0], 0, 5);
        std::fprintf(stderr, "a zero width did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_SIZE) ++failures;
    }
    try {
        (void)fdf::warp(view, models[0], 5, 5, 2);
        std::fprintf(stderr, "border 2 did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("models=%zu failures=%d\n", sizeof models / sizeof models[0], failures);
    return failures ? 1 : 0;
}
