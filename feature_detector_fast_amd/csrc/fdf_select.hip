// fdf_select.hip -- grid-bucketed best-K keypoint selection on MI355X (gfx950)
// (extension, fdf_select_device: the reference returns every keypoint and has no selection).
//
// Input: the points fdf_detect_device left on the device (frames concatenated, each in raster
// order, frame f = indices [offs[f], min(offs[f+1], cap))) and one u16 score per point.  The
// image is cut into cells of cell_w x cell_h pixels; of each cell the k points of highest
// score are kept, ties at the cut going to the earlier point (a stable sort by descending
// score), and the kept points of each frame are written in their input order.
//
// Three kernels on the caller's stream, no host round trip, no allocation:
//
//   select_kernel   one workgroup per (cell row, frame).  Raster order makes a cell row's
//     points one contiguous index range, found by two binary searches on y.  The row's cells
//     are handled kSelCells at a time (a column group); per group the range is read four times:
//       1. a 256-bin histogram per cell of the scores' high bytes -> the bin holding the k-th
//          best score and how many points that bin still has to give;
//       2. the same over the low bytes of the points in that bin -> the cut score s* and the
//          number of points with score == s* to admit;
//       3. each wave counts the tied (== s*) points of every cell in its own contiguous
//          quarter of the range; an exclusive sum over the waves gives each wave the number
//          of tied points before its quarter;
//       4. each wave walks its quarter in index order, 64 points at a time: a point above s*
//          is kept; a tied point is kept iff the tied points of its cell before it (the wave's
//          running count plus a ballot of the earlier lanes of the same cell) number fewer
//          than the ties to admit.  Atomics only ever add to counters, so nothing depends on
//          the order they arrive in.
//     It writes the keep flags, the row's index range, its kept count, and adds that count to
//     the frame's total.
//   select_scan_kernel    one workgroup: exclusive prefix of the frame totals -> sel_offsets.
//   select_scatter_kernel one workgroup per (cell row, frame): its output base is the frame's
//     offset plus the kept counts of the rows before it; kept points and scores are copied in
//     index order with ballot prefixes.
//
// LDS budget of select_kernel: kSelCells = 16 histograms of 256 u32 bins = 16 KB (+ ~0.5 KB).
// A workgroup is 4 waves and a CU holds 32, so 8 workgroups per CU is the wave limit; 8 x 16.5
// KB = 132 KB fits the CU's 160 KB, so LDS never lowers the occupancy.  u32 bins: one cell
// may hold a whole frame's list (cell 0 x 0), far more than a u16 counts.  A row of more than
// 16 cells costs one more pass set per 16 cells (cell_w = 1 at width 2048: 128 groups).
//
// Input that breaks the contract (not raster order, x >= width): the frame's selection is
// unspecified, but every index stays inside [offs[f], min(offs[f+1], cap)) clamped to cap,
// cell columns are clamped, and outputs are written below sel_cap only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

constexpr uint32_t kKeepAll = 0xffffffffu;   // s_need: the cell has at most k points

// First index in [b, e) whose point has y >= y0 (all threads compute the same value).
__device__ __forceinline__ uint64_t lower_bound_y(const uint2* pts, uint64_t b, uint64_t e,
                                                  uint64_t y0) {
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if ((uint64_t)pts[mid].y < y0) b = mid + 1; else e = mid;
    }
    return b;
}

__global__ __launch_bounds__(kSelThreads) void select_kernel(SelectParams P) {
    __shared__ uint32_t hist[kSelCells * 256];
    __shared__ uint32_t s_cut[kSelCells];            // pass 1: high byte; pass 2 on: s*
    __shared__ uint32_t s_need[kSelCells];           // entries of the cut bin still needed
    __shared__ uint32_t s_run[kSelWaves * kSelCells];   // tied points before a wave's position
    __shared__ uint32_t s_kept;

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = blockIdx.x, f = blockIdx.y;
    const uint64_t row = (uint64_t)f * P.rows + r;

    const auto [b, e] = frame_range(P.offs, P.cap, f);
    // the cell row's points: y in [r * ch, (r + 1) * ch); the first row starts at the frame's
    // first point and the last ends at its last, so the rows' ranges tile [b, e)
    uint64_t lo = r == 0 ? b : lower_bound_y(P.pts, b, e, (uint64_t)r * P.ch);
    uint64_t hi = r + 1 == P.rows ? e : lower_bound_y(P.pts, b, e, ((uint64_t)r + 1) * P.ch);
    if (hi < lo) hi = lo;
    if (tid == 0) {
        P.row_range[2 * row] = lo;
        P.row_range[2 * row + 1] = hi;
        s_kept = 0;
    }
    if (lo == hi) {
        if (tid == 0) P.row_cnt[row] = 0;
        return;
    }
    // each wave's contiguous quarter of [lo, hi), in whole 64-point steps
    const uint64_t quarter = (((hi - lo) + kSelWaves - 1) / kSelWaves + 63u) & ~63ull;
    const uint64_t ws = min(lo + wave * quarter, hi), we = min(ws + quarter, hi);
    volatile uint32_t* run = s_run;

    const uint32_t ngroups = (P.cells_x + kSelCells - 1) / kSelCells;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t c0 = g * kSelCells;
        const uint32_t nc = min((uint32_t)kSelCells, P.cells_x - c0);

        // ---- 1: high-byte histograms ----
        for (uint32_t i = tid; i < nc * 256u; i += kSelThreads) hist[i] = 0;
        if (tid < kSelWaves * kSelCells) s_run[tid] = 0;
        __syncthreads();
        for (uint64_t i = lo + tid; i < hi; i += kSelThreads) {
            const uint32_t cl = min(P.pts[i].x / P.cw, P.cells_x - 1) - c0;
            if (cl < nc) atomicAdd(&hist[cl * 256u + (P.scores[i] >> 8)], 1u);
        }
        __syncthreads();
        for (uint32_t c = wave; c < nc; c += kSelWaves) {
            bool found;
            uint32_t bin, need;
            const uint32_t total = find_cut(hist + c * 256u, P.k, lane, found, bin, need);
            if (total < P.k) {
                if (lane == 0) {
                    s_cut[c] = 0;
                    s_need[c] = kKeepAll;
                    atomicAdd(&s_kept, total);
                }
            } else {
                if (found) {
                    s_cut[c] = bin;
                    s_need[c] = need;
                }
                if (lane == 0) atomicAdd(&s_kept, P.k);
            }
        }
        __syncthreads();

        // ---- 2: low-byte histograms of the cut bins ----
        for (uint32_t i = tid; i < nc * 256u; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        for (uint64_t i = lo + tid; i < hi; i += kSelThreads) {
            const uint32_t cl = min(P.pts[i].x / P.cw, P.cells_x - 1) - c0;
            if (cl < nc && s_need[cl] != kKeepAll) {
                const uint32_t s = P.scores[i];
                if ((s >> 8) == s_cut[cl]) atomicAdd(&hist[cl * 256u + (s & 255u)], 1u);
            }
        }
        __syncthreads();
        for (uint32_t c = wave; c < nc; c += kSelWaves) {
            const uint32_t kk = s_need[c];          // the same for the whole wave
            if (kk == kKeepAll) continue;
            const uint32_t hb = s_cut[c];
            bool found;
            uint32_t bin, need;
            find_cut(hist + c * 256u, kk, lane, found, bin, need);
            // every lane has read s_cut / s_need (find_cut's shuffles follow the reads)
            if (found) {
                s_cut[c] = (hb << 8) | bin;
                s_need[c] = need;
            }
        }
        __syncthreads();

        // ---- 3: tied points per cell in each wave's quarter ----
        for (uint64_t i = ws + lane; i < we; i += 64) {
            const uint32_t cl = min(P.pts[i].x / P.cw, P.cells_x - 1) - c0;
            if (cl < nc && s_need[cl] != kKeepAll && (uint32_t)P.scores[i] == s_cut[cl])
                atomicAdd(&s_run[wave * kSelCells + cl], 1u);
        }
        __syncthreads();
        if (tid < nc) {
            uint32_t before = 0;
#pragma unroll
            for (uint32_t w = 0; w < kSelWaves; ++w) {
                const uint32_t n = s_run[w * kSelCells + tid];
                s_run[w * kSelCells + tid] = before;
                before += n;
            }
        }
        __syncthreads();

        // ---- 4: keep flags, ties admitted in index order ----
        for (uint64_t i0 = ws; i0 < we; i0 += 64) {          // uniform over the wave
            const uint64_t i = i0 + lane;
            uint32_t cl = 0xffffffffu, s = 0, cut = 0, need = 0;
            bool mine = false;
            if (i < we) {
                cl = min(P.pts[i].x / P.cw, P.cells_x - 1) - c0;
                mine = cl < nc;
                if (mine) {
                    s = P.scores[i];
                    cut = s_cut[cl];
                    need = s_need[cl];
                }
            }
            bool keep = mine && (need == kKeepAll || s > cut);
            const bool tie = mine && need != kKeepAll && s == cut;
            uint64_t todo = wave_ballot(tie);
            while (todo) {                                   // one round per tied cell
                const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
                const uint32_t c = __shfl(cl, leader, 64);
                const uint64_t m = wave_ballot(tie && cl == c);
                const uint32_t before = run[wave * kSelCells + c];
                if (tie && cl == c) keep = lanes_below_plus(m, before) < need;
                __builtin_amdgcn_wave_barrier();
                if (lane == leader) run[wave * kSelCells + c] = before + (uint32_t)__popcll(m);
                __builtin_amdgcn_wave_barrier();
                todo &= ~m;
            }
            if (mine) P.keep[i] = keep ? 1 : 0;
        }
        __syncthreads();      // the next group reuses hist, s_cut, s_need, s_run
    }
    if (tid == 0) {
        const uint32_t kept = s_kept;
        P.row_cnt[row] = kept;
        atomicAdd(reinterpret_cast<unsigned long long*>(P.frame_tot + f), (unsigned long long)kept);
    }
}

// Exclusive prefix of the frame totals (one workgroup; n_frames <= 65535).
__global__ __launch_bounds__(kSelThreads) void select_scan_kernel(const uint64_t* frame_tot,
                                                                  uint32_t n_frames,
                                                                  uint64_t* sel_offs) {
    __shared__ unsigned long long s_wave[kSelWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (n_frames + kSelThreads - 1) / kSelThreads;
    const uint32_t first = min(tid * per, n_frames), last = min(first + per, n_frames);
    unsigned long long sum = 0;
    for (uint32_t i = first; i < last; ++i) sum += frame_tot[i];
    unsigned long long incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long base = incl - sum;
    for (uint32_t w = 0; w < wave; ++w) base += s_wave[w];
    for (uint32_t i = first; i < last; ++i) {
        sel_offs[i] = base;
        base += frame_tot[i];
    }
    if (tid == kSelThreads - 1) sel_offs[n_frames] = base;
}

__global__ __launch_bounds__(kSelThreads) void select_scatter_kernel(SelectParams P) {
    __shared__ unsigned long long s_part[kSelWaves];
    __shared__ uint32_t s_cnt[kSelWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = blockIdx.x, f = blockIdx.y;
    const uint64_t row0 = (uint64_t)f * P.rows;
    if (P.row_cnt[row0 + r] == 0) return;
    const uint64_t lo = P.row_range[2 * (row0 + r)], hi = P.row_range[2 * (row0 + r) + 1];
    // output base: the frame's offset plus the kept counts of the cell rows above
    unsigned long long part = 0;
    for (uint32_t i = tid; i < r; i += kSelThreads) part += P.row_cnt[row0 + i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    uint64_t o = P.sel_offs[f];
#pragma unroll
    for (uint32_t w = 0; w < kSelWaves; ++w) o += s_part[w];

    for (uint64_t i0 = lo; i0 < hi; i0 += kSelThreads) {     // uniform over the group
        const uint64_t i = i0 + tid;
        const bool kp = i < hi && P.keep[i] != 0;
        const uint64_t m = wave_ballot(kp);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSelWaves; ++w) {
            const uint32_t n = s_cnt[w];
            before += w < wave ? n : 0u;
            total += n;
        }
        if (kp) {
            const uint64_t pos = o + lanes_below_plus(m, before);
            if (pos < P.sel_cap) {
                P.sel[pos] = P.pts[i];
                P.sel_scores[pos] = P.scores[i];
            }
        }
        o += total;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_select(const SelectParams& p, hipStream_t stream) {
    if (p.n_frames == 0 || p.n_frames > 65535u || p.rows == 0 || p.rows > kSelMaxRows ||
        p.cells_x == 0 || p.cw == 0 || p.ch == 0 || p.k == 0)
        return hipErrorInvalidValue;
    const dim3 grid(p.rows, p.n_frames), block(kSelThreads);
    hipLaunchKernelGGL(select_kernel, grid, block, 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), block, 0, stream, p.frame_tot, p.n_frames,
                       p.sel_offs);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_scatter_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
