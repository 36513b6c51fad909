// fdf_geometry.h -- the detector's host-side tuning model: the band geometry of a launch and
// everything the launch derives from it by arithmetic alone.  Pure functions of their
// arguments over the constants of fdf_kernels.h: no environment, no HIP call, no context
// (tests/cpp/test_geometry.cpp tabulates them on the host).  Internal: not part of include/fdf.h.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/fdf.h"
#include "fdf_kernels.h"

// Internal linkage: nothing of this header shows up among the library's symbols.
namespace {

// What the ablation build (libfdf_debug.so) may override in the model; the defaults are the
// release library's constants.
struct GeometryKnobs {
    uint32_t nsub = 0;                 // FDF_NSUB: sub-bands per band (0: >= 4 units per band)
    uint32_t lds_budget_nms = 40000;   // FDF_LDS_BUDGET sets both: LDS bytes per workgroup
    uint32_t lds_budget_plain = 35000;
    double density_margin = 1.2;       // FDF_DENSITY_MARGIN
    uint32_t compact_tpg = 0;          // FDF_COMPACT_TPG: bands per compaction group, 1 .. kCompactTasks
                                       // (0: compact_tasks_per_group)
    bool allow_direct = true;          // FDF_DIRECT=0: small grids take the compaction too
};

// Band geometry of the sweep kernel.  A band is R full-width centre rows; its 4 waves take
// units = column strips (992 centres) x sub-bands.  Tall bands amortise the 8-row halo of a
// sub-band; short bands give a small job (one frame) enough workgroups.  The LDS footprint
// is kept <= 40 KB so 4 workgroups fit a CU.
struct Geometry {
    uint32_t R, nstrips, nsub;
};


inline Geometry pick_geometry(uint32_t n_frames, uint32_t w, uint32_t h, uint32_t nms,
                              uint64_t slots, double density, uint32_t forced_rows,
                              bool host_src = false, const GeometryKnobs& knobs = GeometryKnobs{}) {
    Geometry g;
    const uint32_t sc = (uint32_t)fdfk::kStripCols;
    g.nstrips = (w - 3 + sc - 1) / sc;
    // >= 4 units per band (one per wave), handed out dynamically; taller units (fewer halo
    // rows) measured faster than more, shorter units for balance
    g.nsub = (4 + g.nstrips - 1) / g.nstrips;
    if (knobs.nsub) g.nsub = knobs.nsub;
    const uint32_t centre_rows = h - 6;
    const uint32_t nw = fdfk::bitmap_words_per_row(w);
    // extra rows a unit tests: NMS bands test one row above and below (first / last unit)
    const uint32_t halo = fdfk::band_halo(nms) * (g.nsub == 1 ? 2u : 1u);
    // LDS per workgroup sets the workgroups per CU: <= 40 KB keeps 4.
    // Without NMS a 35 KB budget (bands of ~122 rows at 1080p) measured faster than the
    // tallest band that fits (more, shorter workgroups: a shorter grid tail).
    const uint32_t budget = (nms ? knobs.lds_budget_nms : knobs.lds_budget_plain);
    // The band height with the shortest modelled launch (in sweep-step units): every unit
    // costs its steps plus kUnitCost (prologue, flush, unit hand-out), every workgroup
    // kBandCost more (LDS clear, NMS pass, emit), and the grid runs on `slots` workgroup
    // slots at once -- time = max(total / slots, one workgroup) + half a workgroup of tail
    // (workgroups of one height differ with their rows' content, up to ~1.5x).  So a grid
    // that cannot fill the chip takes the shortest bands (lowest latency), a large batch
    // the tallest that waste no padding steps, and a grid near one round of the chip neither
    // spills into a second round nor leaves slots idle.  slots = 1 (fdf_ctx_set_geometry,
    // tests) gives a small job the full-size geometry (tall bands, long units); the
    // keypoints are the same either way.
    // NMS: when an earlier launch of this configuration measured the keypoint density, keep
    // a band's expected keypoints (x1.2) within the LDS score list, so that few bands
    // spill (4K t=8 n=12 SAD: 38-row bands; margins 1.5 / 1.2 / 1.0 / 0.8 measured 0.726 /
    // 0.716 / 0.715 / 0.730 ms, profiles/r03/l4_margin_4k.json)
    uint32_t max_rows = 256;
    const double margin = knobs.density_margin;
    if (nms && density > 0.0 && margin > 0.0) {
        const double rows = (double)fdfk::kScoreListCap / (margin * density * (double)w) - 2.0;
        max_rows = rows < (double)g.nsub ? g.nsub : (rows > 256.0 ? 256u : (uint32_t)rows);
    }
    if (forced_rows) {   // fdf_ctx_set_band_rows: the height asked for, as far as LDS allows
        g.R = (forced_rows + g.nsub - 1) / g.nsub * g.nsub;
        while (g.R > g.nsub && fdfk::make_sweep_layout(g.R, nw, nms).total > fdfk::kSweepMaxLds)
            g.R -= g.nsub;
        return g;
    }
    constexpr double kUnitCost = 3.0;
    const double band_cost = nms ? 4.0 : 2.0;
    const uint32_t units_per_wave = (g.nstrips * g.nsub + fdfk::kWaves - 1) / fdfk::kWaves;
    // A grid that fits one round of the chip (a single frame) is latency-bound, one wave per
    // SIMD: a unit's padding steps past its last row (the sweep runs whole 8-step blocks) load
    // nothing and cost a quarter of a real step, and every band's look-back polls the
    // descriptors of the bands before it, one round per 64.  Measured on one device-resident
    // 1080p frame (profiles/r05/e7_single_frame_rows/, sweep us at 4 / 6 / 8 / 10 / 14 / 20 rows):
    // max-t 19.0 / 17.2 / 17.8 / 18.1 / 19.4 / 22.6, NMS off 15.0 / 13.3 / 13.4 / 13.5 / 13.9 /
    // 17.1 -- this model picks 6 rows for both (14 and 16 before).  A frame read in place over
    // PCIe keeps the full-step model: its halo rows cost PCIe bytes, and 6-10 rows measured
    // within noise of 14 there (r5_e8_host_rows_*.json).
    auto wg_cost = [&](uint32_t rows, bool latency) {
        const uint32_t unit_rows = (rows + g.nsub - 1) / g.nsub;
        const double steps = (double)fdfk::sweep_steps(unit_rows, halo);
        const double real = std::min(steps, (double)(unit_rows + halo));
        return units_per_wave * ((latency ? real + 0.25 * (steps - real) : steps) + kUnitCost) +
               band_cost;
    };
    const uint64_t one_round = std::min<uint64_t>(slots, fdfk::kDirectMaxTasks);
    auto pick = [&](bool latency) {
        double best = 0.0;
        uint32_t best_R = 0;
        for (uint32_t R = g.nsub; R <= max_rows && R < centre_rows + g.nsub; R += g.nsub) {
            if (fdfk::make_sweep_layout(R, nw, nms).total > budget) break;
            const uint32_t bands = (centre_rows + R - 1) / R;
            const uint64_t ntasks = (uint64_t)n_frames * bands;
            if (latency && ntasks > one_round) continue;   // stays one round of the chip
            const double lookback = latency ? (double)((ntasks + 63) / 64) : 0.0;
            const double full = wg_cost(R, latency) + lookback;
            const double last = wg_cost(centre_rows - (bands - 1) * R, latency) + lookback;
            const double total = (double)n_frames * ((bands - 1) * full + last);
            const double t = std::max(total / (double)slots, full) + 0.5 * full;
            if (best_R == 0 || t <= best * 1.001) {  // ties: the taller band (fewer workgroups)
                best = t;
                best_R = R;
            }
        }
        return best_R;
    };
    g.R = pick(false);
    // the grid of that height fits one round of the chip: the latency model picks among the
    // heights that keep it so
    if (!host_src && g.R && (uint64_t)n_frames * ((centre_rows + g.R - 1) / g.R) <= one_round) {
        const uint32_t r = pick(true);
        if (r) g.R = r;
    }
    if (g.R == 0) g.R = g.nsub;
    return g;
}

// What a launch of `n_frames` frames with geometry `geo` derives from it by arithmetic alone.
struct LaunchPlan {
    int status;             // FDF_OK, or FDF_ERR_SIZE: the band's LDS or the grid is too large
    uint32_t nw;            // bitmap_words_per_row(w)
    uint32_t lds;           // the workgroup's LDS bytes (SweepLayout::total)
    uint32_t bands;         // per frame
    uint64_t ntasks;        // bands of the launch = workgroups of the detector
    uint32_t slot_factor;   // 4: a latency-bound grid's slots hold 4x the points
    uint32_t slot_bytes;
    uint32_t tpg;           // bands per compaction group
    uint64_t ngroups;
    bool direct;            // the bands write their points themselves: no compaction launch
    bool grouped;           // the detector accumulates the compaction's per-group sums
    uint32_t unit_steps;    // rows a unit sweeps, its NMS halo included
    bool exit_in_block;     // the instances that leave an 8-step block at the unit's last row
};

// The workgroup's LDS bytes for `geo` (what the occupancy of the instance is asked with).
inline uint32_t sweep_lds(const Geometry& geo, uint32_t w, uint32_t nms) {
    return fdfk::make_sweep_layout(geo.R, fdfk::bitmap_words_per_row(w), nms).total;
}

// `fill`: the grid size that counts as filling the chip; `wg_per_cu` x `cus`: the workgroups
// of this instance and LDS size that are resident at once.
inline LaunchPlan make_launch_plan(const Geometry& geo, uint32_t n_frames, uint32_t w, uint32_t h,
                                   uint32_t nms, bool rgb, uint64_t fill, uint32_t wg_per_cu,
                                   uint32_t cus, const GeometryKnobs& knobs = GeometryKnobs{}) {
    LaunchPlan pl{};
    const uint32_t R = geo.R;
    pl.nw = fdfk::bitmap_words_per_row(w);
    pl.lds = sweep_lds(geo, w, nms);
    pl.bands = (h - 6 + R - 1) / R;
    pl.ntasks = (uint64_t)pl.bands * n_frames;
    pl.status = FDF_ERR_SIZE;
    if (pl.lds > fdfk::kSweepMaxLds) return pl;
    if (pl.ntasks == 0 || pl.ntasks > 0x7fffffffull) return pl;
    pl.status = FDF_OK;
    // A grid too small to fill the chip (a single frame) is latency-bound: its slots hold 4x
    // the points (6% of the band's pixels instead of 1.6%), so that dense bands stay point
    // lists and the compaction takes no bitmap expansion (a few hundred KB per frame)
    // (fdf_ctx_set_geometry's forced full-size geometry keeps the full-size slots too)
    pl.slot_factor = pl.ntasks < fill ? 4u : 1u;
    pl.slot_bytes = fdfk::slot_bytes_for(R, pl.nw) * pl.slot_factor;
    pl.tpg = fdfk::compact_tasks_per_group((uint32_t)pl.ntasks);
    if (knobs.compact_tpg) pl.tpg = knobs.compact_tpg;
    // detection and compaction are two launches: a compaction fused into the detector's last
    // workgroup measured 87 us for one frame against 13 + 12 us (every workgroup's device-scope
    // release is an L2 writeback on gfx950)
    // Small grids write their points directly (look-back, no compaction launch) when every
    // workgroup is resident at once -- by the occupancy calculator for this instance and LDS
    // size (4 per CU at 4 waves per SIMD) -- so that a band's look-back only waits for bands
    // running beside it.  (Correctness does not depend on it: bands are numbered by their
    // start tickets, band_lookback.)
    pl.direct = knobs.allow_direct &&
                pl.ntasks <= std::min<uint64_t>(fdfk::kDirectMaxTasks, (uint64_t)cus * wg_per_cu);
    pl.ngroups = (pl.ntasks + pl.tpg - 1) / pl.tpg;
    pl.grouped = !pl.direct && pl.ngroups <= fdfk::kMaxGroupSums;
    // a small grid whose units are shorter than one 8-step block (a single frame's latency
    // bands) runs the instances that leave the block at the unit's last row
    // (fdf_sweep_latency.hip; 1080p NMS off 13.5 -> 12.5 us, max-t 17.3 -> 17.0 us per frame).
    // Long units keep whole blocks: the exit tests cost the batch loop more than the padding
    // steps they save (512 x 1080p NMS off, 61-row units: +0.6 %, profiles/r05/e16_*)
    pl.unit_steps = (R + geo.nsub - 1) / geo.nsub +
                    fdfk::band_halo(nms) * (geo.nsub == 1 ? 2u : 1u);
    pl.exit_in_block = !rgb && pl.direct && pl.unit_steps < fdfk::kSweepRing;
    return pl;
}

}  // namespace
