// fdf_describe.hip -- steered BRIEF descriptors and the 5x5 box smoothing BRIEF wants, on
// MI355X (gfx950) (extensions, fdf_describe_device and fdf_smooth_device: the reference
// returns points only; this is the rBRIEF of ORB).
//
// describe_kernel.  Input as for fdf_orient_device: the points of the frames concatenated,
// frame f = indices [offs[f], min(offs[f+1], cap)), and optionally one angle per point.  The
// grid is (chunk, frame); a workgroup owns one contiguous index range of its frame, so the
// keypoints it walks are neighbours in raster order and share image rows.  One wave per
// keypoint: lane l runs the tests 64 q + l, q = 0..3.  Its table entry (x0, y0, x1, y1 as four
// int8) is one dword of a coalesced 256-byte load, its two pixels are byte loads at clamped
// coordinates, and the wave's 64-bit ballot of "first < second" is descriptor word q with
// exactly the packing of include/fdf.h (test i = bit i % 8 of byte i / 8).  Lanes 0..3 store
// one word each: 32 contiguous bytes per keypoint.
// Every pixel load goes through a buffer resource of exactly the frame's width * height
// bytes and every table load through one of n_bins * 1024 bytes (an out-of-range buffer load
// returns 0 and touches no memory); the point is clamped into the frame and the bin below
// n_bins first.  Writes go to indices of the workgroup's range only, all below
// min(offs[f+1], cap).
//
// smooth_kernel (width >= 8).  out = (sum of the 5 x 5 neighbourhood at clamped coordinates
// + 12) / 25.  A thread owns 4 adjacent columns x0 .. x0 + 3 and walks down a strip of rows.
// Per row it needs the 8 bytes of the columns clamp(x0 - 2 + k), k = 0..7.  It loads the 8
// bytes that start at column o = clamp(x0 - 2, 0, width - 8), which lie inside the row, with
// one (unaligned) 8-byte buffer load, and two byte permutes with selectors fixed per thread
// put byte clamp(x0 - 2 + k) - o in place k: the identity for every thread but those at a
// row's ends, so the replicated border costs no branch.  The four horizontal 5-sums are kept
// as two packed pairs of 16-bit values and added to the pairs of the four rows before
// (registers): the sums are at most 25 * 255 = 6375, so the halves never carry into each
// other.  Two rows of loads are in flight ahead of the row being summed.  One dword store per
// row; the last group of a width that is no multiple of 4 covers the last 4 columns, overlapping
// its neighbour with equal values.  Threads are numbered over (strip,
// column group) so that no lane idles whatever the width.
// smooth_small_kernel (width < 8): a thread per pixel, 25 clamped byte loads.
// Loads and stores go through buffer resources of the frame's width * height bytes on both
// sides; gap bytes between output frames are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

typedef uint64_t __attribute__((aligned(1))) u64_unaligned;

__global__ __launch_bounds__(kDescribeThreads) void describe_kernel(DescribeParams P) {
    constexpr uint32_t kPerPass = kDescribeThreads / 64;  // keypoints of a workgroup pass
    const uint32_t f = blockIdx.y;
    const IndexRange fr = frame_range(P.offs, P.cap, f);
    const auto [lo, hi] = wg_share(fr.lo, fr.hi, blockIdx.x, gridDim.x, kPerPass);
    if (lo == hi) return;

    const int W = (int)P.width, H = (int)P.height;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.frames + (uint64_t)f * P.frame_stride, W * H);
    const __amdgpu_buffer_rsrc_t rt = frame_rsrc(P.table, (int)(P.n_bins * kBriefTableBytes));
    const int lane = (int)(threadIdx.x % 64);

    uint64_t i = lo + threadIdx.x / 64;                   // uniform over a wave
    if (i >= hi) return;
    // the next keypoint's point and angle are fetched while this one's pixels are
    uint2 pt_next = P.pts[i];
    float a_next = P.angles ? P.angles[i] : 0.0f;
    for (; i < hi; i += kPerPass) {
        const uint2 pt = pt_next;
        const float a = a_next;
        if (i + kPerPass < hi) {
            pt_next = P.pts[i + kPerPass];
            if (P.angles) a_next = P.angles[i + kPerPass];
        }
        // the bin: round-to-nearest-even of the float product, modulo n_bins; 0 for anything
        // that is not |angle| <= 7 (NaN, infinities, far out of range)
        int bin = 0;
        if (fabsf(a) <= 7.0f) {
            bin = (int)rintf(__fmul_rn(a, P.scale)) % (int)P.n_bins;
            if (bin < 0) bin += (int)P.n_bins;
        }
        bin = min(max(bin, 0), (int)P.n_bins - 1);
        // one keypoint per wave: the scalar unit holds its position and its table row
        const int x = __builtin_amdgcn_readfirstlane((int)min(pt.x, P.width - 1u));
        const int y = __builtin_amdgcn_readfirstlane((int)min(pt.y, P.height - 1u));
        const int row = __builtin_amdgcn_readfirstlane(bin) * (int)kBriefTableBytes;
        uint64_t word[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                rt, row + 4 * (64 * q + lane), 0, 0);
            const int ax = min(max(x + (int)(int8_t)(t & 0xff), 0), W - 1);
            const int ay = min(max(y + (int)(int8_t)((t >> 8) & 0xff), 0), H - 1);
            const int bx = min(max(x + (int)(int8_t)((t >> 16) & 0xff), 0), W - 1);
            const int by = min(max(y + (int)(int8_t)(t >> 24), 0), H - 1);
            const uint32_t pa = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, ay * W + ax, 0, 0);
            const uint32_t pb = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, by * W + bx, 0, 0);
            word[q] = __ballot(pa < pb);
        }
        if (lane < 4) {
            const uint64_t v = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
            *reinterpret_cast<u64_unaligned*>(P.desc + i * kBriefBytes + 8 * lane) = v;
        }
    }
}

// Horizontal 5-sums of a thread's 4 columns from the 8 bytes of columns x0 - 2 .. x0 + 5:
// sums 0, 1 in the halves of .x, sums 2, 3 in the halves of .y.
__device__ __forceinline__ uint2 row_sums(uint32_t lo, uint32_t hi) {
    const uint32_t ones = 0x01010101u;
    const uint32_t h0 = __builtin_amdgcn_udot4(lo, ones, hi & 0xffu, false);
    const uint32_t h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 1), ones,
                                               (hi >> 8) & 0xffu, false);
    const uint32_t h2 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 2), ones,
                                               (hi >> 16) & 0xffu, false);
    const uint32_t h3 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 3), ones,
                                               hi >> 24, false);
    return make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
}

__global__ __launch_bounds__(kSmoothThreads) void smooth_kernel(SmoothParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kSmoothThreads + threadIdx.x;
    const uint32_t strip = gid / P.groups, g = gid % P.groups;
    if (strip >= P.strips) return;
    const int W = (int)P.width, H = (int)P.height;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.frames + (uint64_t)f * P.frame_stride, W * H);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.out + (uint64_t)f * P.out_stride, W * H);
    // the last group of a width that is no multiple of 4 moves left onto its neighbour (both
    // write the same values there), so every thread stores whole dwords
    const int x0 = min(4 * (int)g, W - 4);
    const int ys = (int)(strip * P.strip_rows), ye = min(ys + (int)P.strip_rows, H);
    // the 8 loaded bytes start at column o; place k takes loaded byte clamp(x0 - 2 + k) - o
    const int o = min(max(x0 - 2, 0), W - 8);
    uint32_t sel_lo = 0, sel_hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sel_lo |= (uint32_t)(min(max(x0 - 2 + k, 0), W - 1) - o) << (8 * k);
        sel_hi |= (uint32_t)(min(max(x0 + 2 + k, 0), W - 1) - o) << (8 * k);
    }
    auto issue = [&](int r) {
        return __builtin_amdgcn_raw_buffer_load_b64(rs, min(max(r, 0), H - 1) * W + o, 0, 0);
    };
    auto sums = [&](decltype(issue(0)) raw) {
        return row_sums(__builtin_amdgcn_perm((uint32_t)raw[1], (uint32_t)raw[0], sel_lo),
                        __builtin_amdgcn_perm((uint32_t)raw[1], (uint32_t)raw[0], sel_hi));
    };

    const auto q0 = issue(ys - 2), q1 = issue(ys - 1), q2 = issue(ys), q3 = issue(ys + 1);
    // two rows of look-ahead, issued in this order: the loop waits for the older one only
    // (four rows in flight timed the same on the 512-frame batch)
    __builtin_amdgcn_sched_barrier(0);
    auto ahead0 = issue(ys + 2);
    __builtin_amdgcn_sched_barrier(0);
    auto ahead1 = issue(ys + 3);
    __builtin_amdgcn_sched_barrier(0);
    // the horizontal sums of the four rows before the one a step adds
    uint2 r0 = sums(q0), r1 = sums(q1), r2 = sums(q2), r3 = sums(q3);
    auto step = [&](int y, decltype(issue(0)) raw) {
        const uint2 r4 = sums(raw);
        const uint32_t s01 = r0.x + r1.x + r2.x + r3.x + r4.x;
        const uint32_t s23 = r0.y + r1.y + r2.y + r3.y + r4.y;
        const uint32_t o0 = ((s01 & 0xffffu) + 12u) / 25u, o1 = ((s01 >> 16) + 12u) / 25u;
        const uint32_t o2 = ((s23 & 0xffffu) + 12u) / 25u, o3 = ((s23 >> 16) + 12u) / 25u;
        __builtin_amdgcn_raw_buffer_store_b32(o0 | (o1 << 8) | (o2 << 16) | (o3 << 24), ro,
                                              y * W + x0, 0, 0);
        r0 = r1;
        r1 = r2;
        r2 = r3;
        r3 = r4;
    };
    // two rows per trip, so that a load in flight is never moved between registers
    for (int y = ys; y < ye; y += 2) {
        step(y, ahead0);
        ahead0 = issue(y + 4);
        if (y + 1 < ye) step(y + 1, ahead1);
        ahead1 = issue(y + 5);
    }
}

__global__ __launch_bounds__(kSmoothThreads) void smooth_small_kernel(SmoothParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kSmoothThreads + threadIdx.x;
    const int W = (int)P.width, H = (int)P.height;
    if (gid >= P.width * P.height) return;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.frames + (uint64_t)f * P.frame_stride, W * H);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.out + (uint64_t)f * P.out_stride, W * H);
    const int x = (int)(gid % P.width), y = (int)(gid / P.width);
    uint32_t s = 12;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx)
            s += (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(
                rs, min(max(y + dy, 0), H - 1) * W + min(max(x + dx, 0), W - 1), 0, 0);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(s / 25u), ro, (int)gid, 0, 0);
}

}  // namespace

hipError_t launch_describe(const DescribeParams& p, uint32_t chunks, hipStream_t stream) {
    if (p.n_frames == 0 || p.cap == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.width, p.height) || chunks == 0 || p.n_bins == 0 ||
        p.n_bins > kBriefMaxBins)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(describe_kernel, dim3(chunks, p.n_frames), dim3(kDescribeThreads), 0,
                       stream, p);
    return hipGetLastError();
}

hipError_t launch_smooth(const SmoothParams& p, hipStream_t stream) {
    if (p.n_frames == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.width, p.height) || p.strip_rows == 0 ||
        p.groups != (p.width + 3) / 4 ||
        p.strips != (p.height + p.strip_rows - 1) / p.strip_rows)
        return hipErrorInvalidValue;
    const bool small = p.width < kSmoothMinWidth;
    const uint64_t threads = small ? (uint64_t)p.width * p.height : (uint64_t)p.groups * p.strips;
    const uint64_t blocks = (threads + kSmoothThreads - 1) / kSmoothThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks, p.n_frames), block(kSmoothThreads);
    if (small)
        hipLaunchKernelGGL(smooth_small_kernel, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(smooth_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
