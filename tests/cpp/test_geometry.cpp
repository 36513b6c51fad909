// Host-only table of the detector's tuning model (fdf_geometry.h): pick_geometry and
// make_launch_plan over a grid of shapes, batch sizes, NMS modes, chip sizes, densities,
// sources and forced heights.  One line per case (tests/golden/geometry_table.txt is the
// expected output); exits non-zero when a line contradicts itself.  No device, no libfdf.so.
#include <cstdint>
#include <cstdio>

#include "../../feature_detector_fast_amd/csrc/fdf_geometry.h"

namespace {

struct Shape { uint32_t w, h; };
// what varies within one (shape, frames, NMS mode)
struct Variant { uint64_t slots; double density; bool host; uint32_t forced, wgs; bool rgb; };

unsigned long cases = 0, failures = 0;

void run_case(Shape s, uint32_t frames, uint32_t nms, const Variant& v) {
    const uint32_t cus = 256;
    const Geometry g = pick_geometry(frames, s.w, s.h, nms, v.slots, v.density, v.forced, v.host);
    // a context's `fill` is its `slots` on a 256-CU device (both fdf_ctx_set_geometry's value,
    // or 1024)
    const LaunchPlan p = make_launch_plan(g, frames, s.w, s.h, nms, v.rgb, v.slots, v.wgs, cus);
    const uint32_t budget = nms ? 40000u : 35000u;
    const uint32_t nw = fdfk::bitmap_words_per_row(s.w);
    // how R came about: asked for, by the model, or no height fits the budget (R = nsub)
    const char* how = v.forced ? "forced"
                               : (fdfk::make_sweep_layout(g.nsub, nw, nms).total > budget ? "floor" : "model");
    std::printf("%ux%u f=%u nms=%u slots=%llu density=%.3f src=%s forced=%u wgs=%u rgb=%d : "
                "%s R=%u nstrips=%u nsub=%u : status=%d lds=%u bands=%u ntasks=%llu slot_factor=%u "
                "slot_bytes=%u tpg=%u ngroups=%llu direct=%d grouped=%d unit_steps=%u "
                "exit_in_block=%d\n",
                s.w, s.h, frames, nms, (unsigned long long)v.slots, v.density,
                v.host ? "host" : "device", v.forced, v.wgs, (int)v.rgb, how, g.R, g.nstrips,
                g.nsub, p.status, p.lds, p.bands, (unsigned long long)p.ntasks, p.slot_factor,
                p.slot_bytes, p.tpg, (unsigned long long)p.ngroups, (int)p.direct, (int)p.grouped,
                p.unit_steps, (int)p.exit_in_block);
    ++cases;
    bool ok = g.R >= g.nsub && g.R % g.nsub == 0 && g.nstrips * (uint32_t)fdfk::kStripCols >= s.w - 3 &&
              p.lds == fdfk::make_sweep_layout(g.R, nw, nms).total && p.nw == nw;
    const uint64_t bands = (s.h - 6 + g.R - 1) / g.R;
    const bool too_large = p.lds > fdfk::kSweepMaxLds || bands * frames > 0x7fffffffull;
    ok = ok && (p.status == (too_large ? FDF_ERR_SIZE : FDF_OK));
    if (p.status == FDF_OK) {
        ok = ok && (uint64_t)p.bands * g.R >= s.h - 6 && (uint64_t)(p.bands - 1) * g.R < s.h - 6 &&
             p.ntasks == (uint64_t)p.bands * frames &&
             p.slot_bytes == fdfk::slot_bytes_for(g.R, nw) * p.slot_factor &&
             p.tpg >= 1 && p.tpg <= (uint32_t)fdfk::kCompactTasks &&
             p.ngroups * p.tpg >= p.ntasks && (p.ngroups - 1) * p.tpg < p.ntasks &&
             !(p.direct && p.grouped) && (!p.direct || p.ntasks <= fdfk::kDirectMaxTasks) &&
             (!p.exit_in_block || (p.direct && !v.rgb && p.unit_steps < (uint32_t)fdfk::kSweepRing));
    }
    if (!ok) {
        ++failures;
        std::fprintf(stderr, "inconsistent: case %lu\n", cases);
    }
}

}  // namespace

int main() {
    const Shape shapes[] = {{7, 7}, {8, 7}, {64, 48}, {640, 480}, {993, 9}, {995, 100},
                            {1920, 1080}, {3840, 2160}, {8192, 64}};
    const uint32_t frame_counts[] = {1, 2, 64, 512};
    const Variant variants[] = {
        {1024, 0.0, false, 0, 4, false},     // a 256-CU device, nothing known
        {1, 0.0, false, 0, 4, false},        // fdf_ctx_set_geometry(1): the full-size geometry
        {4096, 0.002, true, 0, 1, false},
        {1024, 0.02, false, 0, 4, false},    // a dense scene: the score list limits the height
        {1024, 0.0, true, 0, 4, false},      // read in place: no latency pick
        {1024, 0.0, false, 8, 4, false},     // fdf_ctx_set_band_rows
        {1024, 0.02, true, 256, 1, false},
    };
    for (const Shape s : shapes)
        for (const uint32_t f : frame_counts)
            for (uint32_t nms = 0; nms < 3; ++nms)
                for (const Variant& v : variants) run_case(s, f, nms, v);
    // the RGB detector never takes the early-exit instances
    for (uint32_t nms = 0; nms < 3; ++nms) {
        run_case({1920, 1080}, 1, nms, {1024, 0.0, false, 0, 4, true});
        run_case({640, 480}, 2, nms, {1024, 0.0, false, 0, 4, true});
    }
    // rows so wide that no band height fits the LDS budget (R = nsub), or the LDS at all
    for (uint32_t nms = 0; nms < 3; ++nms) {
        run_case({262144, 7}, 1, nms, {1024, 0.0, false, 0, 4, false});
        run_case({262144, 9}, 1, nms, {1024, 0.0, false, 256, 4, false});
        run_case({1310720, 7}, 1, nms, {1024, 0.0, false, 0, 4, false});
    }
    std::printf("geometry: %lu cases, %lu failures\n", cases, failures);
    return failures ? 1 : 0;
}
