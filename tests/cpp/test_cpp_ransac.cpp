// fdf::estimate_model smoke test (include/fdf.hpp), run by tests/test_gpu_ransac.py on a GPU box.
// Usage: test_cpp_ransac
// The worked example of include/fdf.h: six queries, trains = query + (3, 5) except the fifth,
// identity matches, seed 0, 8 hypotheses, T = 1.  Both models must give hypothesis 3, 5 inliers,
// n_valid 8, the inlier flags 1 1 1 1 0 1 and h = 1 0 3 0 1 5 0 0 1; the model is printed (a
// negative zero as 0).
#include <cstdio>
#include <vector>

#include "fdf.hpp"

int main() {
    const std::vector<fdf::Point> q = {{0, 0}, {10, 0}, {0, 10}, {10, 10}, {4, 7}, {20, 3}};
    std::vector<fdf::Point> t;
    std::vector<fdf::Match> matches;
    for (size_t i = 0; i < q.size(); ++i) {
        t.push_back(i == 4 ? fdf::Point{50, 50} : fdf::Point{q[i].x + 3, q[i].y + 5});
        matches.push_back(fdf::Match{(uint32_t)i, 0, 0});
    }
    const double want_h[9] = {1, 0, 3, 0, 1, 5, 0, 0, 1};
    const uint8_t want_in[6] = {1, 1, 1, 1, 0, 1};
    int failures = 0;
    for (const uint32_t model : {FDF_MODEL_AFFINE, FDF_MODEL_HOMOGRAPHY}) {
        const fdf::ModelEstimate e = fdf::estimate_model(q, t, matches, nullptr, model, 8, 1.0f, 0);
        std::printf("model=%u hypothesis=%u inliers=%u/%u valid=%u h=", model, e.model.hypothesis,
                    e.model.n_inliers, e.model.n_corr, e.model.n_valid);
        for (int k = 0; k < 9; ++k) std::printf("%g%c", e.model.h[k] + 0.0, k == 8 ? '\n' : ' ');
        if (!e.found() || e.model.hypothesis != 3 || e.model.n_inliers != 5 ||
            e.model.n_corr != 6 || e.model.n_valid != 8)
            ++failures;
        for (int k = 0; k < 9; ++k) failures += e.model.h[k] != want_h[k];
        for (size_t i = 0; i < q.size(); ++i) failures += e.inliers[i] != want_in[i];
    }
    // the fifth query's flag cleared leaves a perfect set; two points are no model
    const std::vector<uint8_t> keep = {1, 1, 1, 1, 0, 1};
    const fdf::ModelEstimate kept = fdf::estimate_model(q, t, matches, &keep);
    if (!kept.found() || kept.model.n_corr != 5 || kept.model.n_inliers != 5) ++failures;
    const std::vector<fdf::Point> two(q.begin(), q.begin() + 2);
    const std::vector<fdf::Match> two_matches(matches.begin(), matches.begin() + 2);
    const fdf::ModelEstimate none = fdf::estimate_model(two, t, two_matches);
    if (none.found() || none.model.n_corr != 2 || none.model.n_inliers != 0 || none.model.h[8] != 0)
        ++failures;
    try {
        (void)fdf::estimate_model(q, t, two_matches);
        std::fprintf(stderr, "a short match list did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
