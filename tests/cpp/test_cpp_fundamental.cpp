// fdf::estimate_fundamental smoke test (include/fdf.hpp), run by tests/test_gpu_fundamental.py on
// a GPU box.
// Usage: test_cpp_fundamental
// The worked example of include/fdf.h: twelve queries of a rectified pair, two bad matches,
// identity matches, seed 3, 8 hypotheses, T = 0.5.  Hypothesis 2 must win with 10 inliers,
// n_valid 8, the inlier flags 1 1 1 1 1 1 1 1 1 0 1 0 and F = [0 0 0; 0 0 1; 0 -1 0] up to
// rounding; the model is printed as hexadecimal doubles, which the Python test compares with the
// device entry bit for bit.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

int main() {
    const uint32_t qs[12][2] = {{0, 0}, {80, 0}, {0, 80}, {80, 80}, {40, 20}, {20, 60},
                                {60, 40}, {30, 30}, {50, 70}, {70, 10}, {10, 50}, {60, 60}};
    const uint32_t ds[12][2] = {{10, 0}, {25, 0}, {31, 0}, {12, 0}, {23, 0}, {37, 0},
                                {14, 0}, {29, 0}, {3, 0}, {20, 30}, {18, 0}, {40, 20}};
    std::vector<fdf::Point> q, t;
    std::vector<fdf::Match> matches;
    for (uint32_t i = 0; i < 12; ++i) {
        q.push_back(fdf::Point{qs[i][0], qs[i][1]});
        t.push_back(fdf::Point{qs[i][0] + ds[i][0], qs[i][1] + ds[i][1]});
        matches.push_back(fdf::Match{i, 0, 0});
    }
    const double want_f[9] = {0, 0, 0, 0, 0, 1, 0, -1, 0};
    const uint8_t want_in[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0};
    int failures = 0;
    const fdf::ModelEstimate e = fdf::estimate_fundamental(q, t, matches, nullptr, 8, 0.5f, 3);
    std::printf("hypothesis=%u inliers=%u/%u valid=%u f=", e.model.hypothesis, e.model.n_inliers,
                e.model.n_corr, e.model.n_valid);
    for (int k = 0; k < 9; ++k) std::printf("%a%c", e.model.h[k], k == 8 ? '\n' : ' ');
    if (!e.found() || e.model.hypothesis != 2 || e.model.n_inliers != 10 || e.model.n_corr != 12 ||
        e.model.n_valid != 8)
        ++failures;
    for (int k = 0; k < 9; ++k) failures += !(std::fabs(e.model.h[k] - want_f[k]) < 1e-9);
    failures += e.model.h[5] != 1.0;
    for (size_t i = 0; i < q.size(); ++i) failures += e.inliers[i] != want_in[i];
    // the two bad matches' flags cleared leave ten true pairs; seven points are no model
    std::vector<uint8_t> keep(12, 1);
    keep[9] = keep[11] = 0;
    const fdf::ModelEstimate kept = fdf::estimate_fundamental(q, t, matches, &keep, 8, 0.5f, 3);
    if (kept.model.n_corr != 10 || (kept.found() && kept.model.n_inliers != 10)) ++failures;
    const std::vector<fdf::Point> seven(q.begin(), q.begin() + 7);
    const std::vector<fdf::Match> seven_matches(matches.begin(), matches.begin() + 7);
    const fdf::ModelEstimate none = fdf::estimate_fundamental(seven, t, seven_matches);
    if (none.found() || none.model.n_corr != 7 || none.model.n_inliers != 0 || none.model.h[5] != 0)
        ++failures;
    try {
        (void)fdf::estimate_fundamental(q, t, seven_matches);
        std::fprintf(stderr, "a short match list did not throw\n");
        ++failures;
    } catch (const fdf::Error& err) {
        if (err.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
