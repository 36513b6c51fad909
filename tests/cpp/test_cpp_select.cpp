// fdf::select_best smoke test (include/fdf.hpp), run by tests/test_gpu_select.py on a GPU box.
// Usage: test_cpp_select
// Every pixel of a 67 x 41 frame is a point with a score from a small set (many ties); the
// selection per 16 x 8 cell (k = 3) and of the whole frame (k = 100) is compared, ordered,
// with a stable sort by descending score per cell.
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "fdf.hpp"

static std::vector<size_t> reference(const std::vector<fdf::Point>& pts,
                                     const std::vector<uint16_t>& scores, uint32_t w, uint32_t h,
                                     uint32_t cw, uint32_t ch, uint32_t k) {
    cw = cw ? cw : w;
    ch = ch ? ch : h;
    const uint32_t cells_x = (w + cw - 1) / cw;
    std::map<uint64_t, std::vector<size_t>> cells;
    for (size_t i = 0; i < pts.size(); ++i)
        cells[(uint64_t)(pts[i].y / ch) * cells_x + pts[i].x / cw].push_back(i);
    std::vector<size_t> kept;
    for (auto& kv : cells) {
        auto& v = kv.second;
        std::stable_sort(v.begin(), v.end(), [&](size_t a, size_t b) { return scores[a] > scores[b]; });
        for (size_t j = 0; j < v.size() && j < k; ++j) kept.push_back(v[j]);
    }
    std::sort(kept.begin(), kept.end());
    return kept;
}

int main() {
    const uint32_t w = 67, h = 41;
    const uint16_t values[8] = {0, 1, 255, 256, 257, 511, 512, 65535};
    std::vector<fdf::Point> pts;
    std::vector<uint16_t> scores;
    uint32_t state = 12345u;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            fdf::Point p;
            p.x = x;
            p.y = y;
            pts.push_back(p);
            state = state * 1664525u + 1013904223u;
            scores.push_back(values[state >> 29]);
        }
    int failures = 0;
    const uint32_t cases[2][3] = {{16, 8, 3}, {0, 0, 100}};
    size_t kept_n[2] = {0, 0};
    for (int c = 0; c < 2; ++c) {
        const auto want = reference(pts, scores, w, h, cases[c][0], cases[c][1], cases[c][2]);
        const auto got = fdf::select_best(pts, scores, w, h, cases[c][0], cases[c][1], cases[c][2]);
        kept_n[c] = got.first.size();
        bool same = got.first.size() == want.size() && got.second.size() == want.size();
        for (size_t j = 0; same && j < want.size(); ++j)
            same = got.first[j] == pts[want[j]] && got.second[j] == scores[want[j]];
        if (!same) {
            std::fprintf(stderr, "cell %u x %u k %u: %zu kept, expected %zu, or a point differs\n",
                         cases[c][0], cases[c][1], cases[c][2], got.first.size(), want.size());
            ++failures;
        }
    }
    try {
        (void)fdf::select_best(pts, scores, w, h, 16, 8, 0);
        std::fprintf(stderr, "k = 0 did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("cells=%zu frame=%zu failures=%d\n", kept_n[0], kept_n[1], failures);
    return failures ? 1 : 0;
}
