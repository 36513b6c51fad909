// fdf::keypoint_harris smoke test (include/fdf.hpp), run by tests/test_gpu_harris.py on a GPU box.
// Usage: test_cpp_harris
// Every third pixel of a pseudo-random 67 x 41 frame (borders and corners included) is a
// point; the int64 responses and the u16 rank scores at blocks 7, 5 and 3 are compared exactly
// with a plain restatement of include/fdf.h's semantics.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

uint16_t code_of(int64_t R) {
    if (R <= 0) return 0;
    int e = 0;
    while ((R >> (e + 1)) != 0) ++e;
    if (e < 10) return (uint16_t)R;
    return (uint16_t)(((e - 9) << 10) | (int)((R >> (e - 10)) & 1023));
}

}  // namespace

int main() {
    const int w = 67, h = 41;
    std::vector<uint8_t> img(w * h);
    uint32_t state = 2463534242u;
    for (auto& p : img) {
        state = state * 1664525u + 1013904223u;
        p = (uint8_t)(state >> 24);
    }
    std::vector<fdf::Point> pts;
    for (int y = 0; y < h; ++y)
        for (int x = y % 3; x < w; x += 3) {
            fdf::Point p;
            p.x = (uint32_t)x;
            p.y = (uint32_t)y;
            pts.push_back(p);
        }
    fdf::Point corner;
    corner.x = w - 1;
    corner.y = h - 1;
    pts.push_back(corner);
    const fdf::GrayView view(img.data(), w, h);
    auto I = [&](int cx, int cy) {
        return (int64_t)img[std::min(std::max(cy, 0), h - 1) * w + std::min(std::max(cx, 0), w - 1)];
    };
    int failures = 0;
    size_t positive = 0;
    struct Case { uint32_t block, k_num, k_den; };
    for (const Case c : {Case{7, 1, 25}, Case{5, 1, 25}, Case{3, 0, 255}, Case{7, 255, 1}}) {
        std::vector<int64_t> resp;
        const std::vector<uint16_t> sc = fdf::keypoint_harris(view, pts, c.block, c.k_num, c.k_den,
                                                              &resp);
        if (sc.size() != pts.size() || resp.size() != pts.size()) {
            ++failures;
            continue;
        }
        const int hb = (int)c.block / 2;
        for (size_t i = 0; i < pts.size(); ++i) {
            int64_t a = 0, b = 0, cc = 0;
            for (int v = -hb; v <= hb; ++v)
                for (int d = -hb; d <= hb; ++d) {
                    const int X = (int)pts[i].x + d, Y = (int)pts[i].y + v;
                    const int64_t ix = 2 * (I(X + 1, Y) - I(X - 1, Y)) +
                                       (I(X + 1, Y - 1) - I(X - 1, Y - 1)) +
                                       (I(X + 1, Y + 1) - I(X - 1, Y + 1));
                    const int64_t iy = 2 * (I(X, Y + 1) - I(X, Y - 1)) +
                                       (I(X - 1, Y + 1) - I(X - 1, Y - 1)) +
                                       (I(X + 1, Y + 1) - I(X + 1, Y - 1));
                    a += ix * ix;
                    b += iy * iy;
                    cc += ix * iy;
                }
            const int64_t R = (int64_t)c.k_den * (a * b - cc * cc) -
                              (int64_t)c.k_num * (a + b) * (a + b);
            if (R > 0) ++positive;
            if (resp[i] != R || sc[i] != code_of(R)) {
                if (failures < 5)
                    std::fprintf(stderr, "block %u point (%u, %u): response %lld score %u, "
                                 "expected %lld %u\n", c.block, pts[i].x, pts[i].y,
                                 (long long)resp[i], sc[i], (long long)R, code_of(R));
                ++failures;
            }
        }
        // the scores alone are the same
        if (fdf::keypoint_harris(view, pts, c.block, c.k_num, c.k_den) != sc) ++failures;
    }
    if (positive == 0) ++failures;
    try {
        std::vector<fdf::Point> bad(1);
        bad[0].x = w;
        (void)fdf::keypoint_harris(view, bad);
        std::fprintf(stderr, "a point at x = width did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    try {
        (void)fdf::keypoint_harris(view, pts, 4);
        std::fprintf(stderr, "block 4 did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("points=%zu positive=%zu failures=%d\n", pts.size(), positive, failures);
    return failures ? 1 : 0;
}
