// fdf_tracks.hip -- track-set maintenance between two tracking calls on MI355X (gfx950)
// (extension, fdf_tracks_update_device; include/fdf.h has the rule): drop lost and border
// tracks, keep the older of two tracks that drifted together, refill with the strongest
// candidates no survivor is near, carry ids and ages, hand out new ids.
//
// Both lists (tracks, candidates) of a stream are binned into one grid of square cells whose
// side is >= min_dist, so the points near a point lie in the 3 x 3 cells around it: three
// contiguous ranges of a row-major cell-sorted list.  Kernels of one call, all on the caller's
// stream, no host round trip, no allocation:
//
//   tracks_count_kernel<ROLE>    a thread per point: alive / eligible points add 1 to their cell.
//   tracks_scan_kernel           a workgroup per (stream, list): exclusive prefix of the cell
//                                counts -> start; the counts go back to zero (the cursors).
//   tracks_scatter_kernel<ROLE>  a thread per point: entry {pixel, key, index, cell} to
//                                start[cell] + cursor[cell]++.  The order inside a cell comes from
//                                the atomics; every reader visits whole cells and combines with
//                                OR, so nothing depends on it.
//   tracks_pass_kernel<LAST>     a thread per sorted entry, `passes` launches per list: reads the
//                                states of the pass before (never its own pass's), visits the
//                                3 x 3 cells, writes the other state buffer.  The last pass also
//                                writes the admitted flags by original index.
//   tracks_seed_kernel           between the two lists' passes: a candidate near a kept survivor
//                                starts rejected, every other eligible one undecided.
//   tracks_cut_kernel            a workgroup per stream: kept survivors, free = max_tracks - kept,
//                                and when more candidates are admitted than that the top `free`
//                                by (score descending, index ascending): two 256-bin histograms
//                                (high byte, then low byte in the cut bin) and one walk in index
//                                order for the ties, as select_kernel does for a cell.
//   tracks_offsets_kernel        one workgroup: exclusive prefix of the streams' totals.
//   tracks_emit_kernel           a workgroup per (stream, list): walks the flags in index order,
//                                ballot prefixes give each kept point its slot; writes below
//                                out_cap only.
//
// Bounds: a stream's indices are frame_range()'s, clamped to cap; a sorted position is the
// stream's first index plus a value below its binned count, itself clamped to the range's
// length; cell coordinates are clamped to the grid; an entry's original index is checked
// against cap before it indexes the flags.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

constexpr int kRoleTracks = 0, kRoleCands = 1;

__device__ __forceinline__ uint32_t cell_of(const TracksParams& P, uint32_t px, uint32_t py) {
    return min(px / P.cell, P.cells_x - 1) | (min(py / P.cell, P.cells_y - 1) << 16);
}
__device__ __forceinline__ uint32_t cell_index(const TracksParams& P, uint32_t cell) {
    return (cell >> 16) * P.cells_x + (cell & 0xffffu);
}

// Point i of a list: false if it takes no part (a dead track, a candidate in the margin);
// otherwise its pixel and its priority key.
template <int ROLE>
__device__ __forceinline__ bool point_of(const TracksParams& P, uint64_t i, uint32_t& px,
                                         uint32_t& py, uint32_t& key) {
    if constexpr (ROLE == kRoleTracks) {
        if (P.t_status && P.t_status[i] == 0) return false;
        const int2 q = P.t_q11[i];
        const int lo = (int)(P.margin << 11);
        const int hx = (int)((P.width - 1 - P.margin) << 11);
        const int hy = (int)((P.height - 1 - P.margin) << 11);
        if (q.x < lo || q.x > hx || q.y < lo || q.y > hy) return false;
        px = (uint32_t)(q.x + 1024) >> 11;
        py = (uint32_t)(q.y + 1024) >> 11;
        key = P.t_ages[i];
    } else {
        const uint2 c = P.c_pts[i];
        if (c.x < P.margin || c.x > P.width - 1 - P.margin || c.y < P.margin ||
            c.y > P.height - 1 - P.margin)
            return false;
        px = c.x;
        py = c.y;
        key = P.c_scores[i];
    }
    return true;
}

template <int ROLE>
__device__ __forceinline__ const TracksList& list_of(const TracksParams& P) {
    if constexpr (ROLE == kRoleTracks) return P.t; else return P.c;
}

template <int ROLE>
__global__ __launch_bounds__(kTracksThreads) void tracks_count_kernel(TracksParams P) {
    const TracksList& L = list_of<ROLE>(P);
    const uint32_t f = blockIdx.y;
    const auto [b, e] = frame_range(L.offs, L.cap, f);
    const auto [lo, hi] = wg_share(b, e, blockIdx.x, gridDim.x, kTracksThreads);
    uint32_t* cnt = L.cursor + (uint64_t)f * P.cells_x * P.cells_y;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kTracksThreads) {
        uint32_t px, py, key;
        if (point_of<ROLE>(P, i, px, py, key)) atomicAdd(&cnt[cell_index(P, cell_of(P, px, py))], 1u);
    }
}

// Exclusive prefix of one (stream, list)'s cell counts; start[cells] is the binned total.
__global__ __launch_bounds__(kTracksThreads) void tracks_scan_kernel(TracksParams P) {
    __shared__ uint32_t s_wave[kTracksWaves];
    const TracksList& L = blockIdx.y ? P.c : P.t;
    const uint32_t f = blockIdx.x, cells = P.cells_x * P.cells_y;
    uint32_t* cnt = L.cursor + (uint64_t)f * cells;
    uint32_t* start = L.start + (uint64_t)f * (cells + 1ull);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (cells + kTracksThreads - 1) / kTracksThreads;
    const uint32_t first = min(tid * per, cells), last = min(first + per, cells);
    uint32_t sum = 0;
    for (uint32_t i = first; i < last; ++i) sum += cnt[i];
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (uint32_t w = 0; w < wave; ++w) base += s_wave[w];
    for (uint32_t i = first; i < last; ++i) {
        start[i] = base;
        base += cnt[i];
        cnt[i] = 0;                                  // the scatter's cursor
    }
    if (tid == kTracksThreads - 1) start[cells] = base;
}

template <int ROLE>
__global__ __launch_bounds__(kTracksThreads) void tracks_scatter_kernel(TracksParams P) {
    const TracksList& L = list_of<ROLE>(P);
    const uint32_t f = blockIdx.y, cells = P.cells_x * P.cells_y;
    const auto [b, e] = frame_range(L.offs, L.cap, f);
    const auto [lo, hi] = wg_share(b, e, blockIdx.x, gridDim.x, kTracksThreads);
    uint32_t* cursor = L.cursor + (uint64_t)f * cells;
    const uint32_t* start = L.start + (uint64_t)f * (cells + 1ull);
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kTracksThreads) {
        uint32_t px, py, key;
        if (!point_of<ROLE>(P, i, px, py, key)) continue;
        const uint32_t cell = cell_of(P, px, py), c = cell_index(P, cell);
        const uint64_t rel = (uint64_t)start[c] + atomicAdd(&cursor[c], 1u);
        if (rel >= e - b) continue;                  // cannot happen while the inputs stand still
        L.ent[b + rel] = make_uint4(px | (py << 16), key, (uint32_t)i, cell);
        if constexpr (ROLE == kRoleTracks) L.st[0][b + rel] = kTracksUndecided;
    }
}

// The stream's sorted entries: [b, b + n).
struct SortedRange { uint64_t b; uint32_t n; };
__device__ __forceinline__ SortedRange sorted_range(const TracksList& L, uint32_t f,
                                                    uint32_t cells) {
    const auto [b, e] = frame_range(L.offs, L.cap, f);
    const uint64_t n = min((uint64_t)L.start[(uint64_t)f * (cells + 1ull) + cells], e - b);
    return {b, (uint32_t)n};
}

// Calls visit(j) for every sorted position b + j of the 3 x 3 cells around `cell` until it
// returns true.  `start` is the stream's; j stays below n.
template <typename F>
__device__ __forceinline__ void for_neighbours(const TracksParams& P, const uint32_t* start,
                                               uint32_t n, uint32_t cell, F visit) {
    const uint32_t cx = cell & 0xffffu, cy = cell >> 16;
    const uint32_t x0 = max(cx, 1u) - 1u, x1 = min(cx + 1u, P.cells_x - 1u);
    const uint32_t y0 = max(cy, 1u) - 1u, y1 = min(cy + 1u, P.cells_y - 1u);
    for (uint32_t y = y0; y <= y1; ++y) {
        const uint32_t j0 = start[y * P.cells_x + x0];
        const uint32_t j1 = min(start[y * P.cells_x + x1 + 1u], n);
        for (uint32_t j = j0; j < j1; ++j)
            if (visit(j)) return;
    }
}

__device__ __forceinline__ bool near(uint32_t a, uint32_t b, uint32_t d2) {
    const int dx = (int)(a & 0xffffu) - (int)(b & 0xffffu), dy = (int)(a >> 16) - (int)(b >> 16);
    return (uint32_t)(dx * dx + dy * dy) < d2;
}

template <bool LAST>
__global__ __launch_bounds__(kTracksThreads) void tracks_pass_kernel(TracksParams P, int role,
                                                                     int from) {
    const TracksList& L = role ? P.c : P.t;
    const uint32_t f = blockIdx.y, cells = P.cells_x * P.cells_y, d2 = P.min_dist * P.min_dist;
    const SortedRange r = sorted_range(L, f, cells);
    const uint32_t n = r.n;
    const auto [lo, hi] = wg_share(r.b, r.b + n, blockIdx.x, gridDim.x, kTracksThreads);
    const uint32_t* start = L.start + (uint64_t)f * (cells + 1ull);
    const uint8_t* in = L.st[from];
    uint8_t* out = L.st[from ^ 1];
    const uint4* ent = L.ent + r.b;                  // the stream's sorted entries and states
    const uint8_t* ins = in + r.b;
    for (uint64_t pos = lo + threadIdx.x; pos < hi; pos += kTracksThreads) {
        uint8_t st = in[pos];
        uint4 me = make_uint4(0, 0, 0, 0);
        if (LAST || st == kTracksUndecided) me = L.ent[pos];
        if (st == kTracksUndecided) {
            bool admitted = false, undecided = false;
            for_neighbours(P, start, n, me.w, [&](uint32_t j) {
                const uint4 o = ent[j];
                // o dominates me: near and of higher priority (larger key, then lower index)
                if ((o.y > me.y || (o.y == me.y && o.z < me.z)) && near(o.x, me.x, d2)) {
                    const uint8_t s = ins[j];
                    admitted = s == kTracksAdmitted;
                    undecided |= s == kTracksUndecided;
                }
                return admitted;
            });
            st = admitted ? kTracksRejected : undecided ? kTracksUndecided : kTracksAdmitted;
        }
        out[pos] = st;
        if (LAST && st == kTracksAdmitted && me.z < L.cap) L.flag[me.z] = 1;
    }
}

// A candidate's first state: rejected if a kept survivor is near.  `final_t` is the state
// buffer the tracks' last pass wrote.
__global__ __launch_bounds__(kTracksThreads) void tracks_seed_kernel(TracksParams P, int final_t) {
    const uint32_t f = blockIdx.y, cells = P.cells_x * P.cells_y, d2 = P.min_dist * P.min_dist;
    const SortedRange rc = sorted_range(P.c, f, cells), rt = sorted_range(P.t, f, cells);
    const uint32_t tn = rt.n;
    const auto [lo, hi] = wg_share(rc.b, rc.b + rc.n, blockIdx.x, gridDim.x, kTracksThreads);
    const uint32_t* start = P.t.start + (uint64_t)f * (cells + 1ull);
    const uint8_t* tst = P.t.st[final_t] + rt.b;
    const uint4* tent = P.t.ent + rt.b;
    for (uint64_t pos = lo + threadIdx.x; pos < hi; pos += kTracksThreads) {
        const uint4 me = P.c.ent[pos];
        bool hit = false;
        for_neighbours(P, start, tn, me.w, [&](uint32_t j) {
            hit = tst[j] == kTracksAdmitted && near(tent[j].x, me.x, d2);
            return hit;
        });
        P.c.st[0][pos] = hit ? kTracksRejected : kTracksUndecided;
    }
}

// Sum of v over the workgroup, in every thread (s_red: kTracksWaves words; two barriers).
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();                                 // s_red's earlier readers are done
    if ((threadIdx.x & 63u) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kTracksWaves; ++w) s += s_red[w];
    return s;
}

__global__ __launch_bounds__(kTracksThreads) void tracks_cut_kernel(TracksParams P) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_red[kTracksWaves];
    __shared__ uint32_t s_cnt[kTracksWaves];
    __shared__ uint32_t s_cut, s_need;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t f = blockIdx.x;
    const auto [tb, te] = frame_range(P.t.offs, P.t.cap, f);
    const auto [cb, ce] = frame_range(P.c.offs, P.c.cap, f);
    uint32_t v = 0;
    for (uint64_t i = tb + tid; i < te; i += kTracksThreads) v += P.t.flag[i];
    const uint32_t kept = block_sum(v, s_red);
    v = 0;
    for (uint64_t i = cb + tid; i < ce; i += kTracksThreads) v += P.c.flag[i];
    const uint32_t admitted = block_sum(v, s_red);
    const uint32_t room = P.max_tracks > kept ? P.max_tracks - kept : 0u;
    if (admitted > room && room == 0) {
        for (uint64_t i = cb + tid; i < ce; i += kTracksThreads) P.c.flag[i] = 0;
    } else if (admitted > room) {
        // the room-th best score s* and how many of the points at s* still fit
        uint32_t hb = 0, kk = room;
        for (int level = 0; level < 2; ++level) {
            hist[tid] = 0;
            __syncthreads();
            for (uint64_t i = cb + tid; i < ce; i += kTracksThreads) {
                const uint32_t s = P.c_scores[i];
                if (P.c.flag[i] && (level == 0 || (s >> 8) == hb))
                    atomicAdd(&hist[level == 0 ? s >> 8 : s & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                bool found;
                uint32_t bin, need;
                find_cut(hist, kk, lane, found, bin, need);
                if (found) {
                    s_cut = bin;
                    s_need = need;
                }
            }
            __syncthreads();
            hb = (hb << 8) | s_cut;
            kk = s_need;
            __syncthreads();                         // s_cut, s_need and hist are written again
        }
        const uint32_t cut = hb, need = kk;
        uint32_t run = 0;                            // tied points before this step
        for (uint64_t i0 = cb; i0 < ce; i0 += kTracksThreads) {   // uniform over the group
            const uint64_t i = i0 + tid;
            const bool on = i < ce && P.c.flag[i] != 0;
            const uint32_t s = on ? P.c_scores[i] : 0u;
            const bool tie = on && s == cut;
            const uint64_t m = wave_ballot(tie);
            if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = run;
#pragma unroll
            for (uint32_t w = 0; w < kTracksWaves; ++w) {
                const uint32_t c = s_cnt[w];
                before += w < wave ? c : 0u;
                run += c;
            }
            if (on && !(s > cut || (tie && lanes_below_plus(m, before) < need))) P.c.flag[i] = 0;
            __syncthreads();
        }
    }
    if (tid == 0) {
        const uint32_t n_new = min(admitted, room), id = P.next_id[f];
        P.kept[f] = kept;
        P.n_new[f] = n_new;
        P.tot[f] = (uint64_t)kept + n_new;
        P.id_base[f] = id;
        P.next_id[f] = id + n_new;
    }
}

// Exclusive prefix of the streams' totals (one workgroup; n_frames <= 65535).
__global__ __launch_bounds__(kTracksThreads) void tracks_offsets_kernel(const uint64_t* tot,
                                                                        uint32_t n_frames,
                                                                        uint64_t* out_offs) {
    __shared__ unsigned long long s_wave[kTracksWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (n_frames + kTracksThreads - 1) / kTracksThreads;
    const uint32_t first = min(tid * per, n_frames), last = min(first + per, n_frames);
    unsigned long long sum = 0;
    for (uint32_t i = first; i < last; ++i) sum += tot[i];
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
        out_offs[i] = base;
        base += tot[i];
    }
    if (tid == kTracksThreads - 1) out_offs[n_frames] = base;
}

__global__ __launch_bounds__(kTracksThreads) void tracks_emit_kernel(TracksParams P) {
    __shared__ uint32_t s_cnt[kTracksWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t role = blockIdx.x, f = blockIdx.y;
    const TracksList& L = role ? P.c : P.t;
    const auto [b, e] = frame_range(L.offs, L.cap, f);
    const uint64_t base = P.out_offs[f] + (role ? P.kept[f] : 0u);
    const uint32_t id0 = P.id_base[f];
    uint64_t o = 0;
    for (uint64_t i0 = b; i0 < e; i0 += kTracksThreads) {        // uniform over the group
        const uint64_t i = i0 + tid;
        const bool kp = i < e && L.flag[i] != 0;
        const uint64_t m = wave_ballot(kp);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kTracksWaves; ++w) {
            const uint32_t c = s_cnt[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const uint64_t rank = o + lanes_below_plus(m, before);
        if (kp && base + rank < P.out_cap) {
            const uint64_t pos = base + rank;
            if (role == kRoleTracks) {
                const uint32_t age = P.t_ages[i];
                P.out_q11[pos] = P.t_q11[i];
                P.out_ids[pos] = P.t_ids[i];
                P.out_ages[pos] = age == 0xffffffffu ? age : age + 1u;
                if (P.out_src) P.out_src[pos] = (uint32_t)i;
            } else {
                const uint2 c = P.c_pts[i];
                P.out_q11[pos] = make_int2((int)(c.x << 11), (int)(c.y << 11));
                P.out_ids[pos] = id0 + (uint32_t)rank;
                P.out_ages[pos] = 0;
                if (P.out_src) P.out_src[pos] = kTracksNewBit | (uint32_t)i;
            }
        }
        o += total;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_tracks_update(const TracksParams& p, hipStream_t stream) {
    if (p.n_frames == 0 || p.n_frames > 65535u || p.cell == 0 || p.cells_x == 0 ||
        p.cells_y == 0 || p.passes == 0 || p.passes > kTracksMaxPasses || p.t.chunks == 0 ||
        p.c.chunks == 0)
        return hipErrorInvalidValue;
    const dim3 block(kTracksThreads), tgrid(p.t.chunks, p.n_frames), cgrid(p.c.chunks, p.n_frames);
    hipError_t e = hipSuccess;
    auto launched = [&]() { return (e = hipGetLastError()) == hipSuccess; };
    hipLaunchKernelGGL(tracks_count_kernel<kRoleTracks>, tgrid, block, 0, stream, p);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_count_kernel<kRoleCands>, cgrid, block, 0, stream, p);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_scan_kernel, dim3(p.n_frames, 2), block, 0, stream, p);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_scatter_kernel<kRoleTracks>, tgrid, block, 0, stream, p);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_scatter_kernel<kRoleCands>, cgrid, block, 0, stream, p);
    if (!launched()) return e;
    for (int role = 0; role < 2; ++role) {
        if (role == kRoleCands) {
            hipLaunchKernelGGL(tracks_seed_kernel, cgrid, block, 0, stream, p, (int)(p.passes & 1u));
            if (!launched()) return e;
        }
        for (uint32_t k = 0; k < p.passes; ++k) {
            if (k + 1 == p.passes)
                hipLaunchKernelGGL(tracks_pass_kernel<true>, role ? cgrid : tgrid, block, 0, stream,
                                   p, role, (int)(k & 1u));
            else
                hipLaunchKernelGGL(tracks_pass_kernel<false>, role ? cgrid : tgrid, block, 0,
                                   stream, p, role, (int)(k & 1u));
            if (!launched()) return e;
        }
    }
    hipLaunchKernelGGL(tracks_cut_kernel, dim3(p.n_frames), block, 0, stream, p);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_offsets_kernel, dim3(1), block, 0, stream, p.tot, p.n_frames,
                       p.out_offs);
    if (!launched()) return e;
    hipLaunchKernelGGL(tracks_emit_kernel, dim3(2, p.n_frames), block, 0, stream, p);
    (void)launched();
    return e;
}

}  // namespace fdfk
