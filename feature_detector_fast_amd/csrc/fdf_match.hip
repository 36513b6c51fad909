// fdf_match.hip -- brute-force Hamming matching of 256-bit descriptors on MI355X (gfx950)
// (extensions, fdf_match_device and fdf_match_filter_device: the reference returns points
// only; this is the step after fdf_describe_device).
//
// match_kernel.  Two descriptor sets, each as fdf_describe_device leaves one: 32 bytes per
// point, frames concatenated, frame f = indices [offs[f], min(offs[f+1], cap)).  Frame f of the
// query set is matched against frame f of the train set.  The grid is (query chunk, frame); a
// workgroup owns one contiguous range of its frame's queries (offsets read on the device) and
// walks it in passes of 256: a lane keeps its query's 8 descriptor words in registers for the
// whole pass.  The train descriptors stream through LDS in tiles of 256 (8 KB, plus 2 KB of
// (x, y) when a window is on): thread t fetches the 16-byte pieces t and t + 256 of a tile
// with two coalesced loads and stores them at the same piece numbers, so descriptor k of the
// tile is the 32 bytes at 32 k.  Two tile buffers: the loads of tile n + 1 are issued before
// tile n is scanned and land in the other buffer after the scan, one barrier per tile.  In the
// scan every lane reads the same descriptor at the same LDS address (identical addresses
// broadcast: no bank conflicts) with two 16-byte reads; a pair then costs 8 XORs, 8
// accumulating bit counts, the window test, and with key = d << 16 | place in the tile
//     second = min(second, max(best, key));  best = min(best, key)
// with d = 0xFFFF for a pair outside the window: the smallest key is the smallest (d, index),
// so ties go to the lowest index, and the tile's two keys are folded into the query's result
// once per tile.  One 8-byte store per query.
// With a window the workgroup reduces min / max y over the pass's queries (LDS atomics) and
// binary-searches the train frame's y (non-decreasing by contract) for the indices with
// y_min - max_dy <= y <= y_max + max_dy: only those are scanned.  Both searches stay inside
// the frame's train range whatever the y hold, so a frame that breaks the order gets wrong
// matches and nothing else.
// Every train index read is below min(offs[f+1], t_cap), every query index below
// min(offs[f+1], q_cap); writes go to the workgroup's own query range only.
//
// match_filter_kernel.  One thread per query index: the distance bound, the ratio test and
// the cross-check of include/fdf.h; the index a match holds is compared with t_cap before the
// reverse array is read at it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;       // descriptors are 4-byte aligned

static_assert(kMatchTile == (uint32_t)kMatchThreads, "a thread fetches two pieces of a tile");

// The first index in [b, e) whose y is not below `y`, e when there is none (y non-decreasing;
// any other content still gives an index in [b, e]).
__device__ __forceinline__ uint64_t first_y_not_below(const uint2* pts, uint64_t b, uint64_t e,
                                                      uint64_t y) {
    while (b < e) {
        const uint64_t m = b + (e - b) / 2;
        if ((uint64_t)pts[m].y < y) b = m + 1;
        else e = m;
    }
    return b;
}

// popcount(x) + acc in one instruction (the compiler builds a tree of counts and adds)
__device__ __forceinline__ uint32_t bcnt_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

__device__ __forceinline__ uint32_t hamming(const uint32_t (&q)[8], u32x4 a, u32x4 b) {
    uint32_t d = __builtin_popcount(q[0] ^ a.x);
    d = bcnt_add(q[1] ^ a.y, d);
    d = bcnt_add(q[2] ^ a.z, d);
    d = bcnt_add(q[3] ^ a.w, d);
    d = bcnt_add(q[4] ^ b.x, d);
    d = bcnt_add(q[5] ^ b.y, d);
    d = bcnt_add(q[6] ^ b.z, d);
    d = bcnt_add(q[7] ^ b.w, d);
    return d;
}

// scan(k) for k = 0 .. cnt - 1, four at a time so that their loads are in flight together
// (unrolled by hand: inline assembly keeps the compiler from unrolling a loop with a remainder)
template <typename F>
__device__ __forceinline__ void scan_tile(uint32_t cnt, F scan) {
    uint32_t k = 0;
    for (; k + 4 <= cnt; k += 4) {
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) scan(k + u);
    }
    for (; k < cnt; ++k) scan(k);
}

__device__ __forceinline__ uint32_t abs_diff(uint32_t a, uint32_t b) {
    return a > b ? a - b : b - a;
}

template <bool WINDOW>
__global__ __launch_bounds__(kMatchThreads) void match_kernel(MatchParams P) {
    __shared__ u32x4 s_desc[2][2 * kMatchTile];
    __shared__ uint2 s_pts[2][WINDOW ? kMatchTile : 1];
    __shared__ uint32_t s_y[2];
    const uint32_t f = blockIdx.y;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const IndexRange tr = frame_range(P.t_offs, P.t_cap, f);
    const auto [lo, hi] = wg_share(qr.lo, qr.hi, blockIdx.x, gridDim.x, kMatchThreads);
    if (lo == hi) return;
    const uint32_t tid = threadIdx.x;

    for (uint64_t i0 = lo; i0 < hi; i0 += kMatchThreads) {    // uniform over the workgroup
        const uint64_t i = i0 + tid;
        const bool live = i < hi;
        uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint2 qp = make_uint2(0u, 0u);
        if (live) {
            const u32x4_a4* src = reinterpret_cast<const u32x4_a4*>(P.q_desc + i * kBriefBytes);
            const u32x4 a = src[0], b = src[1];
            q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w;
            q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w;
            if constexpr (WINDOW) qp = P.q_pts[i];
        }
        // the train indices this pass scans: the frame's, or the rows its window reaches
        uint64_t jlo = tr.lo, jhi = tr.hi;
        if constexpr (WINDOW) {
            if (tid == 0) {
                s_y[0] = 0xffffffffu;
                s_y[1] = 0u;
            }
            __syncthreads();
            if (live) {
                atomicMin(&s_y[0], qp.y);
                atomicMax(&s_y[1], qp.y);
            }
            __syncthreads();
            const uint32_t y_min = __builtin_amdgcn_readfirstlane(s_y[0]);
            const uint32_t y_max = __builtin_amdgcn_readfirstlane(s_y[1]);
            __syncthreads();                                  // the next pass resets s_y
            const uint64_t y_first = y_min > P.max_dy ? y_min - P.max_dy : 0u;
            const uint64_t y_end = (uint64_t)y_max + P.max_dy + 1u;
            jlo = first_y_not_below(P.t_pts, tr.lo, tr.hi, y_first);
            jhi = first_y_not_below(P.t_pts, jlo, tr.hi, y_end);
        }

        // Within a tile of 256 train indices a pair is the key d << 16 | k, k its place in
        // the tile: the smallest key is the smallest (d, index) and the second smallest key
        // holds the smallest d among the others.  A pair outside the window has d = 0xFFFF.
        // After the tile the two keys are folded into the running result; strict comparisons
        // leave ties with the earlier tile.
        uint32_t best = kMatchNoDistance, second = kMatchNoDistance, idx = kMatchNone;
        uint32_t key_best = ~0u, key_second = ~0u;
        auto pair = [&](uint32_t d, uint32_t k) {
            const uint32_t key = (d << 16) | k;
            key_second = min(key_second, max(key_best, key));
            key_best = min(key_best, key);
        };
        auto fold = [&](uint32_t jbase) {
            const uint32_t d1 = key_best >> 16, d2 = key_second >> 16;
            if (d1 < best) {
                second = min(best, d2);
                best = d1;
                idx = jbase + (key_best & 0xffffu);
            } else {
                second = min(second, d1);
            }
            key_best = key_second = ~0u;
        };
        auto inside = [&](uint32_t tx, uint32_t ty) {
            return abs_diff(qp.x, tx) <= P.max_dx && abs_diff(qp.y, ty) <= P.max_dy;
        };
        // this thread's two 16-byte pieces (and point) of the tile that starts at j0
        u32x4 stage[2] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
        uint2 stage_pt = make_uint2(0u, 0u);
        auto fetch = [&](uint64_t j0) {
#pragma unroll
            for (uint32_t k = 0; k < 2; ++k) {
                const uint32_t piece = tid + k * kMatchThreads;
                const uint64_t j = j0 + piece / 2;
                if (j < jhi)
                    stage[k] = *reinterpret_cast<const u32x4_a4*>(P.t_desc + j * kBriefBytes +
                                                                  16 * (piece & 1));
            }
            if constexpr (WINDOW)
                if (j0 + tid < jhi) stage_pt = P.t_pts[j0 + tid];
        };
        auto commit = [&](uint32_t buf) {
            s_desc[buf][tid] = stage[0];
            s_desc[buf][tid + kMatchThreads] = stage[1];
            if constexpr (WINDOW) s_pts[buf][tid] = stage_pt;
        };
        // the first tile, whatever the range (an empty one stores the zeros): every load so
        // far has landed before the scan, which then waits for LDS only
        fetch(jlo);
        commit(0);
        __syncthreads();
        uint32_t buf = 0;
        for (uint64_t j0 = jlo; j0 < jhi; j0 += kMatchTile, buf ^= 1u) {
            const bool more = j0 + kMatchTile < jhi;
            if (more) fetch(j0 + kMatchTile);             // in flight while this tile is scanned
            const uint32_t cnt = (uint32_t)min((uint64_t)kMatchTile, jhi - j0);
            auto scan = [&](uint32_t k) {
                uint32_t d = hamming(q, s_desc[buf][2 * k], s_desc[buf][2 * k + 1]);
                if constexpr (WINDOW) {
                    const uint2 tp = s_pts[buf][k];
                    d = inside(tp.x, tp.y) ? d : kMatchNoDistance;
                }
                pair(d, k);
            };
            scan_tile(cnt, scan);
            fold((uint32_t)j0);
            if (more) commit(buf ^ 1u);
            __syncthreads();
        }
        if (live) P.matches[i] = make_uint2(idx, best | (second << 16));
    }
}

__global__ __launch_bounds__(kMatchThreads) void match_filter_kernel(MatchFilterParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kMatchThreads + threadIdx.x;
    const uint64_t lo = min(P.q_offs[0], P.q_cap), hi = min(P.q_offs[P.n_frames], P.q_cap);
    if (i < lo || i >= hi) return;
    const uint2 m = P.matches[i];
    const uint32_t d = m.y & 0xffffu, s = m.y >> 16;
    bool keep = m.x != kMatchNone;
    keep = keep && (P.max_distance >= 256u || d <= P.max_distance);
    keep = keep && (P.ratio_den == 0u || s == kMatchNoDistance || d * P.ratio_den < s * P.ratio_num);
    if (keep && P.reverse) keep = m.x < P.t_cap && P.reverse[m.x].x == (uint32_t)i;
    P.keep[i] = keep ? 1u : 0u;
}

}  // namespace

hipError_t launch_match(const MatchParams& p, uint32_t chunks, hipStream_t stream) {
    if (p.n_frames == 0 || p.q_cap == 0) return hipSuccess;
    if (p.n_frames > 65535u || chunks == 0 || p.q_cap > kMatchMaxCap || p.t_cap > kMatchMaxCap ||
        (p.q_pts == nullptr) != (p.t_pts == nullptr))
        return hipErrorInvalidValue;
    const dim3 grid(chunks, p.n_frames), block(kMatchThreads);
    if (p.q_pts)
        hipLaunchKernelGGL(match_kernel<true>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(match_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_match_filter(const MatchFilterParams& p, hipStream_t stream) {
    if (p.n_frames == 0 || p.q_cap == 0) return hipSuccess;
    if (p.n_frames > 65535u || p.q_cap > kMatchMaxCap || p.t_cap > kMatchMaxCap ||
        p.ratio_num > 65535u || p.ratio_den > 65535u)
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)((p.q_cap + kMatchThreads - 1) / kMatchThreads);
    hipLaunchKernelGGL(match_filter_kernel, dim3(blocks), dim3(kMatchThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
