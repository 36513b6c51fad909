// fdf::keypoint_angles smoke test (include/fdf.hpp), run by tests/test_gpu_orient.py on a GPU box.
// Usage: test_cpp_orient
// Every third pixel of a pseudo-random 67 x 41 frame (borders and corners included) is a
// point; the moments at r = 15 and r = 4 are compared exactly, and the angles to 1e-5 rad,
// with a plain restatement of include/fdf.h's semantics.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

int main() {
    const uint32_t w = 67, h = 41;
    std::vector<uint8_t> img(w * h);
    uint32_t state = 2463534242u;
    for (auto& p : img) {
        state = state * 1664525u + 1013904223u;
        p = (uint8_t)(state >> 24);
    }
    std::vector<fdf::Point> pts;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = y % 3; x < w; x += 3) {
            fdf::Point p;
            p.x = x;
            p.y = y;
            pts.push_back(p);
        }
    fdf::Point corner;
    corner.x = w - 1;
    corner.y = h - 1;
    pts.push_back(corner);
    const fdf::GrayView view(img.data(), w, h);
    const double pi = std::acos(-1.0);
    int failures = 0;
    double worst = 0;
    for (uint32_t r : {15u, 4u}) {
        uint8_t u[32];
        if (fdf_orient_disc(r, u) != FDF_OK) ++failures;
        std::vector<int32_t> mom;
        const std::vector<float> ang = fdf::keypoint_angles(view, pts, r, &mom);
        if (ang.size() != pts.size() || mom.size() != 2 * pts.size()) {
            ++failures;
            continue;
        }
        for (size_t i = 0; i < pts.size(); ++i) {
            long m10 = 0, m01 = 0;
            for (int v = -(int)r; v <= (int)r; ++v)
                for (int d = -(int)u[std::abs(v)]; d <= (int)u[std::abs(v)]; ++d) {
                    const int cx = std::min(std::max((int)pts[i].x + d, 0), (int)w - 1);
                    const int cy = std::min(std::max((int)pts[i].y + v, 0), (int)h - 1);
                    m10 += d * (long)img[cy * w + cx];
                    m01 += v * (long)img[cy * w + cx];
                }
            if (mom[2 * i] != m10 || mom[2 * i + 1] != m01) {
                if (failures < 5)
                    std::fprintf(stderr, "r %u point (%u, %u): moments %d %d, expected %ld %ld\n", r,
                                 pts[i].x, pts[i].y, mom[2 * i], mom[2 * i + 1], m10, m01);
                ++failures;
            }
            double diff = std::fabs((double)ang[i] - std::atan2((double)m01, (double)m10));
            diff = std::min(diff, 2 * pi - diff);
            worst = std::max(worst, diff);
            if (!(diff <= 1e-5)) ++failures;
        }
    }
    try {
        std::vector<fdf::Point> bad(1);
        bad[0].x = w;
        (void)fdf::keypoint_angles(view, bad);
        std::fprintf(stderr, "a point at x = width did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("points=%zu worst_angle_error=%.3g failures=%d\n", pts.size(), worst, failures);
    return failures ? 1 : 0;
}
