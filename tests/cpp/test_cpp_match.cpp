// fdf::match_descriptors smoke test (include/fdf.hpp), run by tests/test_gpu_match.py on a GPU
// box.
// Usage: test_cpp_match
// 131 query and 309 train descriptors drawn from a pool of 6 base descriptors with up to two
// bits flipped (so equal descriptors and equal distances are common), with points on a raster
// of non-decreasing y; the matches without a window and with two windows are compared field
// by field with a plain restatement of include/fdf.h's semantics.
#include <bitset>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

uint32_t state = 2463534242u;
uint32_t rnd() {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

unsigned distance(const uint8_t* a, const uint8_t* b) {
    unsigned d = 0;
    for (int k = 0; k < 32; ++k) d += (unsigned)std::bitset<8>((unsigned)(a[k] ^ b[k])).count();
    return d;
}

uint32_t abs_diff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

}  // namespace

int main() {
    const size_t n_q = 131, n_t = 309;
    uint8_t pool[6][32];
    for (auto& d : pool)
        for (auto& b : d) b = (uint8_t)(rnd() >> 8);
    auto draw = [&](size_t n, std::vector<uint8_t>& desc, std::vector<fdf::Point>& pts) {
        desc.resize(32 * n);
        pts.resize(n);
        uint32_t y = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* base = pool[rnd() % 6];
            for (int k = 0; k < 32; ++k) desc[32 * i + k] = base[k];
            for (uint32_t flips = rnd() % 3; flips > 0; --flips) {
                const uint32_t bit = rnd() % 256;
                desc[32 * i + bit / 8] ^= (uint8_t)(1u << (bit % 8));
            }
            y += rnd() % 3;                               // non-decreasing, with repeats
            pts[i].x = rnd() % 300;
            pts[i].y = y;
        }
    };
    std::vector<uint8_t> q_desc, t_desc;
    std::vector<fdf::Point> q_pts, t_pts;
    draw(n_q, q_desc, q_pts);
    draw(n_t, t_desc, t_pts);

    int failures = 0;
    struct Case { bool window; uint32_t dx, dy; };
    for (const Case c : {Case{false, 0, 0}, Case{true, 40, 12}, Case{true, 3, 0}}) {
        const std::vector<fdf::Match> got =
            c.window ? fdf::match_descriptors(q_desc, t_desc, &q_pts, &t_pts, c.dx, c.dy)
                     : fdf::match_descriptors(q_desc, t_desc);
        if (got.size() != n_q) {
            ++failures;
            continue;
        }
        size_t none = 0;
        for (size_t i = 0; i < n_q; ++i) {
            uint32_t index = FDF_MATCH_NONE;
            unsigned best = FDF_MATCH_NO_DISTANCE, second = FDF_MATCH_NO_DISTANCE;
            for (size_t j = 0; j < n_t; ++j) {
                if (c.window && (abs_diff(q_pts[i].x, t_pts[j].x) > c.dx ||
                                 abs_diff(q_pts[i].y, t_pts[j].y) > c.dy))
                    continue;
                const unsigned d = distance(&q_desc[32 * i], &t_desc[32 * j]);
                if (d < best) {
                    second = best;
                    best = d;
                    index = (uint32_t)j;
                } else if (d < second) {
                    second = d;
                }
            }
            none += index == FDF_MATCH_NONE;
            if (got[i].index != index || got[i].distance != best || got[i].second != second) {
                if (failures < 5)
                    std::fprintf(stderr, "window %d (%u, %u) query %zu: got %u %u %u, want %u %u %u\n",
                                 (int)c.window, c.dx, c.dy, i, got[i].index, got[i].distance,
                                 got[i].second, index, best, second);
                ++failures;
            }
        }
        if (!c.window && none != 0) ++failures;
        if (c.window && c.dx == 3 && none == 0) ++failures;      // the case must hold empty windows
    }
    // no train descriptors: every query is unmatched; no queries: an empty result
    const std::vector<uint8_t> empty;
    const std::vector<fdf::Point> no_points;
    for (const fdf::Match& m : fdf::match_descriptors(q_desc, empty, &q_pts, &no_points, 5, 5))
        if (m.index != FDF_MATCH_NONE || m.distance != FDF_MATCH_NO_DISTANCE ||
            m.second != FDF_MATCH_NO_DISTANCE)
            ++failures;
    if (!fdf::match_descriptors(empty, t_desc).empty()) ++failures;
    try {
        (void)fdf::match_descriptors(q_desc, t_desc, &q_pts, nullptr, 1, 1);
        std::fprintf(stderr, "one point list without the other did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("queries=%zu train=%zu failures=%d\n", n_q, n_t, failures);
    return failures ? 1 : 0;
}
