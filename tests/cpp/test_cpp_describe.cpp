// fdf::keypoint_descriptors smoke test (include/fdf.hpp), run by tests/test_gpu_describe.py on a
// GPU box.
// Usage: test_cpp_describe
// Every third pixel of a pseudo-random 67 x 41 frame (borders and corners included) is a
// point with a pseudo-random angle; the descriptors at 30 and 1 bins, smoothed and raw, are
// compared bit for bit with a plain restatement of include/fdf.h's semantics built on
// fdf_brief_pattern and fdf_brief_steer.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

int main() {
    const int w = 67, h = 41;
    std::vector<uint8_t> img(w * h);
    uint32_t state = 2463534242u;
    auto rnd = [&state]() {
        state = state * 1664525u + 1013904223u;
        return state >> 8;
    };
    for (auto& p : img) p = (uint8_t)(rnd() >> 16);
    std::vector<fdf::Point> pts;
    std::vector<float> angles;
    const double pi = std::acos(-1.0);
    for (int y = 0; y < h; ++y)
        for (int x = y % 3; x < w; x += 3) {
            fdf::Point p;
            p.x = (uint32_t)x;
            p.y = (uint32_t)y;
            pts.push_back(p);
            angles.push_back((float)((rnd() / 16777216.0 * 2 - 1) * pi));
        }
    fdf::Point corner;
    corner.x = w - 1;
    corner.y = h - 1;
    pts.push_back(corner);
    angles.push_back(-3.0f);

    auto at = [&](const std::vector<uint8_t>& f, int x, int y) {
        return f[std::min(std::max(y, 0), h - 1) * w + std::min(std::max(x, 0), w - 1)];
    };
    std::vector<uint8_t> smoothed(w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int s = 12;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) s += at(img, x + dx, y + dy);
            smoothed[y * w + x] = (uint8_t)(s / 25);
        }

    std::array<int8_t, 1024> pattern;
    int failures = fdf_brief_pattern(pattern.data()) != FDF_OK;
    const fdf::GrayView view(img.data(), w, h);
    for (uint32_t n_bins : {30u, 1u})
        for (bool smooth : {true, false}) {
            std::vector<int8_t> table(n_bins * 1024);
            if (fdf_brief_steer(pattern.data(), n_bins, table.data()) != FDF_OK) ++failures;
            const std::vector<uint8_t> desc =
                fdf::keypoint_descriptors(view, pts, &angles, nullptr, n_bins, smooth);
            if (desc.size() != 32 * pts.size()) {
                ++failures;
                continue;
            }
            const std::vector<uint8_t>& f = smooth ? smoothed : img;
            const float scale = (float)(n_bins / (2 * pi));
            for (size_t i = 0; i < pts.size(); ++i) {
                const float t = angles[i] * scale;
                int bin = (int)std::nearbyint(t) % (int)n_bins;
                if (bin < 0) bin += (int)n_bins;
                const int x = (int)pts[i].x, y = (int)pts[i].y;
                for (int k = 0; k < 256; ++k) {
                    const int8_t* e = &table[(bin * 256 + k) * 4];
                    const int bit = at(f, x + e[0], y + e[1]) < at(f, x + e[2], y + e[3]);
                    if (((desc[32 * i + k / 8] >> (k % 8)) & 1) != bit) {
                        if (failures < 5)
                            std::fprintf(stderr, "bins %u smooth %d point (%d, %d) test %d: bit %d\n",
                                         n_bins, (int)smooth, x, y, k, bit ^ 1);
                        ++failures;
                        break;
                    }
                }
            }
        }
    // the defaults: no angles, the default pattern, 30 bins, smoothed = bin 0 of the above
    if (fdf::keypoint_descriptors(view, pts) !=
        fdf::keypoint_descriptors(view, pts, nullptr, &pattern, 1, true))
        ++failures;
    try {
        std::vector<fdf::Point> bad(1);
        bad[0].x = w;
        (void)fdf::keypoint_descriptors(view, bad);
        std::fprintf(stderr, "a point at x = width did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("points=%zu failures=%d\n", pts.size(), failures);
    return failures ? 1 : 0;
}
