// fdf::refine_model smoke test (include/fdf.hpp), run by tests/test_gpu_refine.py on a GPU box.
// Usage: test_cpp_refine
// 40 grid points and their images under the translation (3, 5), the first of them moved far
// away.  The model to refine is off by a quarter pixel; T = 1.  One round must bring both kinds
// of model back to the translation (to 1e-9: the data are exact) with 39 inliers; the refined
// model is printed with 17 digits so that the test can compare it with the device entry's bit
// for bit.  Then: no rounds, a record without a model, a short match list.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fdf.hpp"

int main() {
    std::vector<fdf::Point> q, t;
    std::vector<fdf::Match> matches;
    for (uint32_t k = 0; k < 40; ++k) {
        q.push_back(fdf::Point{7 * (k % 8) + k / 8, 11 * (k / 8) + (k % 3)});
        t.push_back(k == 0 ? fdf::Point{500, 400} : fdf::Point{q[k].x + 3, q[k].y + 5});
        matches.push_back(fdf::Match{k, 0, 0});
    }
    fdf_model start = {};
    const double start_h[9] = {1, 0, 3.25, 0, 1, 4.75, 0, 0, 1};
    for (int k = 0; k < 9; ++k) start.h[k] = start_h[k];
    start.hypothesis = 12;
    start.n_valid = 34;
    const double want_h[9] = {1, 0, 3, 0, 1, 5, 0, 0, 1};
    int failures = 0;
    for (const uint32_t model : {FDF_MODEL_AFFINE, FDF_MODEL_HOMOGRAPHY}) {
        const fdf::RefinedModel r = fdf::refine_model(q, t, matches, start, nullptr, model, 1.0f, 1);
        std::printf("model=%u rounds=%u inliers=%u/%u hypothesis=%u valid=%u h=", model, r.rounds,
                    r.model.n_inliers, r.model.n_corr, r.model.hypothesis, r.model.n_valid);
        for (int k = 0; k < 9; ++k) std::printf("%.17g%c", r.model.h[k] + 0.0, k == 8 ? '\n' : ' ');
        if (!r.found() || r.rounds != 1 || r.model.n_inliers != 39 || r.model.n_corr != 40 ||
            r.model.hypothesis != 12 || r.model.n_valid != 34)
            ++failures;
        for (int k = 0; k < 9; ++k) failures += !(std::fabs(r.model.h[k] - want_h[k]) <= 1e-9);
        for (size_t i = 0; i < q.size(); ++i) failures += r.inliers[i] != (i == 0 ? 0 : 1);
    }
    // no rounds: the model as it came, recounted
    const fdf::RefinedModel same = fdf::refine_model(q, t, matches, start, nullptr,
                                                     FDF_MODEL_HOMOGRAPHY, 1.0f, 0);
    if (same.rounds != 0 || same.model.n_inliers != 39 || same.model.n_corr != 40) ++failures;
    for (int k = 0; k < 9; ++k) failures += same.model.h[k] != start_h[k];
    // a record without a model passes through
    fdf_model none = {};
    none.hypothesis = FDF_RANSAC_NONE;
    none.n_corr = 77;
    const fdf::RefinedModel through = fdf::refine_model(q, t, matches, none);
    if (through.found() || through.rounds != 0 || through.model.n_corr != 77 ||
        through.model.n_inliers != 0 || through.model.h[8] != 0)
        ++failures;
    for (size_t i = 0; i < q.size(); ++i) failures += through.inliers[i] != 0;
    try {
        const std::vector<fdf::Match> two(matches.begin(), matches.begin() + 2);
        (void)fdf::refine_model(q, t, two, start);
        std::fprintf(stderr, "a short match list did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    try {
        (void)fdf::refine_model(q, t, matches, start, nullptr, FDF_MODEL_HOMOGRAPHY, 1.0f, 9);
        std::fprintf(stderr, "nine rounds did not throw\n");
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != FDF_ERR_ARG) ++failures;
    }
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
