// fdf::update_tracks smoke test (include/fdf.hpp), run by tests/test_gpu_tracks.py on a GPU box.
// Usage: test_cpp_tracks
// The worked example of include/fdf.h: 32 x 24, min_dist 5, margin 2, max_tracks 4, passes 8,
// next_id 7, four tracks and six candidates; every number the header quotes is checked, then
// passes = 1 (track 0 stays undecided and is dropped all the same), an empty set and the
// rejected arguments.
#include <cstdio>
#include <vector>

#include "fdf.hpp"

namespace {

int failures = 0;

struct Row { int32_t x, y; uint32_t id, age, src; };

void expect(const fdf::TrackSet& t, const std::vector<Row>& rows, const char* what) {
    bool ok = t.q11.size() == rows.size() && t.ids.size() == rows.size() &&
              t.ages.size() == rows.size() && t.src.size() == rows.size();
    for (size_t k = 0; ok && k < rows.size(); ++k)
        ok = t.q11[k][0] == rows[k].x && t.q11[k][1] == rows[k].y && t.ids[k] == rows[k].id &&
             t.ages[k] == rows[k].age && t.src[k] == rows[k].src;
    if (!ok) {
        std::fprintf(stderr, "%s: got %zu tracks\n", what, t.q11.size());
        for (size_t k = 0; k < t.q11.size(); ++k)
            std::fprintf(stderr, "  (%d, %d) id %u age %u src %#x\n", t.q11[k][0], t.q11[k][1],
                         t.ids[k], t.ages[k], t.src[k]);
        ++failures;
    }
}

template <typename F>
void expect_throw(F f, int status, const char* what) {
    try {
        f();
        std::fprintf(stderr, "%s did not throw\n", what);
        ++failures;
    } catch (const fdf::Error& e) {
        if (e.status() != status) {
            std::fprintf(stderr, "%s threw %d\n", what, e.status());
            ++failures;
        }
    }
}

}  // namespace

int main() {
    const uint32_t w = 32, h = 24;
    fdf::TrackSet in;
    in.q11 = {{20480, 20480}, {15359, 28672}, {22528, 20480}, {-1, -1}};
    in.ids = {3, 4, 5, 6};
    in.ages = {5, 2, 9, 1};
    in.status = {1, 1, 1, 0};
    const std::vector<fdf::Point> cand = {{12, 10}, {20, 10}, {23, 14}, {21, 11}, {1, 12}, {28, 20}};
    const std::vector<uint16_t> scores = {90, 50, 50, 40, 99, 10};
    fdf::TrackSetOptions opt;
    opt.min_dist = 5;
    opt.margin = 2;
    opt.max_tracks = 4;
    opt.passes = 8;
    const std::vector<Row> want = {{15359, 28672, 4, 3, 1},
                                   {22528, 20480, 5, 10, 2},
                                   {40960, 20480, 7, 0, FDF_TRACKS_NEW | 1u},
                                   {47104, 28672, 8, 0, FDF_TRACKS_NEW | 2u}};
    uint32_t next_id = 7;
    expect(fdf::update_tracks(w, h, in, cand, scores, next_id, opt), want, "the header's example");
    if (next_id != 9) {
        std::fprintf(stderr, "next_id %u\n", next_id);
        ++failures;
    }
    opt.passes = 1;       // track 0 is undecided after one pass and dropped; candidate 3 likewise
    next_id = 7;
    expect(fdf::update_tracks(w, h, in, cand, scores, next_id, opt), want, "one pass");
    opt.passes = 8;
    opt.max_tracks = 2;   // the survivors fill the budget
    next_id = 7;
    expect(fdf::update_tracks(w, h, in, cand, scores, next_id, opt),
           {want[0], want[1]}, "no room");
    if (next_id != 7) ++failures;
    opt.max_tracks = 4;
    next_id = 0xFFFFFFFFu;
    const fdf::TrackSet fresh = fdf::update_tracks(w, h, fdf::TrackSet(), cand, scores, next_id, opt);
    expect(fresh, {{24576, 20480, 0xFFFFFFFFu, 0, FDF_TRACKS_NEW | 0u},
                   {40960, 20480, 0, 0, FDF_TRACKS_NEW | 1u},
                   {47104, 28672, 1, 0, FDF_TRACKS_NEW | 2u},
                   {57344, 40960, 2, 0, FDF_TRACKS_NEW | 5u}}, "an empty set");
    if (next_id != 3) ++failures;
    next_id = 0;
    if (!fdf::update_tracks(w, h, fdf::TrackSet(), {}, {}, next_id, opt).q11.empty()) ++failures;

    opt.min_dist = 0;
    expect_throw([&] { (void)fdf::update_tracks(w, h, in, cand, scores, next_id, opt); },
                 FDF_ERR_ARG, "min_dist 0");
    opt.min_dist = 256;
    expect_throw([&] { (void)fdf::update_tracks(w, h, in, cand, scores, next_id, opt); },
                 FDF_ERR_ARG, "min_dist 256");
    opt.min_dist = 5;
    opt.margin = 12;
    expect_throw([&] { (void)fdf::update_tracks(w, h, in, cand, scores, next_id, opt); },
                 FDF_ERR_ARG, "margin 12 of height 24");
    opt.margin = 2;
    opt.passes = 33;
    expect_throw([&] { (void)fdf::update_tracks(w, h, in, cand, scores, next_id, opt); },
                 FDF_ERR_ARG, "33 passes");
    opt.passes = 8;
    opt.max_tracks = 0;
    expect_throw([&] { (void)fdf::update_tracks(w, h, in, cand, scores, next_id, opt); },
                 FDF_ERR_ARG, "max_tracks 0");
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
