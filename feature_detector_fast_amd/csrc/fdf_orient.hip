// fdf_orient.hip -- keypoint orientation by intensity centroid on MI355X (gfx950)
// (extension, fdf_orient_device: the reference returns points only; oFAST / ORB's IC_Angle).
//
// Input: the points fdf_detect_device (or fdf_select_device) left on the device, frames
// concatenated, each in raster order, frame f = indices [offs[f], min(offs[f+1], cap)).  For
// every point the moments of the disc of radius r around it,
//     m10 = sum d * I(x + d, y + v),   m01 = sum v * I(x + d, y + v),   |d| <= u[|v|], |v| <= r,
// with I read at clamped coordinates (a replicated border), and angle = atan2f(m01, m10).
//
// One kernel, one launch.  The grid is (chunk, frame); a workgroup owns one contiguous index
// range of its frame (offsets read on the device), so the keypoints it walks are neighbours
// in raster order and share image rows.  L lanes share a keypoint, L = 2, 4, 8 or 16 with
// 4 L >= 2 r + 1: lane j holds the dword of window bytes 4j .. 4j+3 of a disc row, the window
// starting at x - r, so one row of one keypoint is one request of 4 L contiguous bytes and a
// wave instruction fetches a row of 64 / L keypoints.  Per row and lane:
//     pix &= mask                       bytes outside |d| <= u[|v|] dropped (mask per |v|)
//     S += udot4(pix, 0x01010101)       sum of I
//     T += udot4(pix, bytes 4j+b)       sum of (d + r) * I
//     V += udot4(pix, bytes v+r)        sum of (v + r) * I
// so that m10 = T - r S and m01 = V - r S: three accumulating dot products and an AND per
// dword.  The L partial sums are added with DPP moves (quad permutes, then half-row and row
// mirrors): no LDS, no atomics.
//
// Two ways to fetch a row dword, giving the same integers:
//   fast     the disc lies inside the frame and all 4 L window bytes of its last row do too:
//            one (unaligned) dword buffer load per lane and row;
//   clamped  anything else: four byte loads at clamped coordinates.
// Every load goes through a buffer resource of exactly the frame's width * height bytes, so
// whatever the points hold nothing outside the frame is read (an out-of-range buffer load
// returns 0 and touches no memory); points are clamped into the frame first.  Writes go to
// indices of the workgroup's range only, all below min(offs[f+1], cap).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

// Byte mask of a lane's dword for a disc row of half-width u: the window bytes [r - u, r + u]
// are in the disc and the lane holds the bytes [4j, 4j + 4); j8 = 32 j - 8 r, so both shift
// counts, in bits, are one add and one clamp away.
__device__ __forceinline__ uint32_t row_mask(int u, int j8) {
    const int lo = min(max(-8 * u - j8, 0), 32);          // bits below the disc's first byte
    const int hi = min(max(24 - 8 * u + j8, 0), 32);      // bits above its last byte
    return (uint32_t)(0xffffffffull << lo) & (uint32_t)(0xffffffffull >> hi);
}

template <int L>
__global__ __launch_bounds__(kOrientThreads) void orient_kernel(OrientParams P) {
    constexpr uint32_t kPerPass = kOrientThreads / L;     // keypoints of a workgroup pass
    const uint32_t f = blockIdx.y;
    const IndexRange fr = frame_range(P.offs, P.cap, f);
    const auto [lo, hi] = wg_share(fr.lo, fr.hi, blockIdx.x, gridDim.x, kPerPass);
    if (lo == hi) return;

    const int W = (int)P.width, H = (int)P.height, r = (int)P.radius;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.frames + (uint64_t)f * P.frame_stride, W * H);
    const int j = (int)(threadIdx.x % L);                 // the lane's dword of the window
    const uint32_t wts = (uint32_t)(4 * j) * 0x01010101u + 0x03020100u;   // bytes d + r
    const int j8 = 32 * j - 8 * r;                        // row_mask

    for (uint64_t i0 = lo; i0 < hi; i0 += kPerPass) {     // uniform over the workgroup
        const uint64_t i = i0 + threadIdx.x / L;
        const bool live = i < hi;
        uint2 pt = live ? P.pts[i] : make_uint2(0u, 0u);
        const int x = (int)min(pt.x, P.width - 1u), y = (int)min(pt.y, P.height - 1u);
        // fast: the disc inside the frame, and the window's spare bytes of the last row too
        const bool fast = x >= r && x + r < W && y >= r && y + r < H &&
                          (y + r) * W + (x - r) + 4 * L <= W * H;
        const int x0 = x - r + 4 * j;                     // column of the lane's byte 0
        // T = sum (d + r) I, V = sum (v + r) I, S = sum I over the lane's bytes
        uint32_t T = 0, S = 0, V = 0;
        auto tally = [&](uint32_t pix, int v) {
            T = __builtin_amdgcn_udot4(pix, wts, T, false);
            S = __builtin_amdgcn_udot4(pix, 0x01010101u, S, false);
            V = __builtin_amdgcn_udot4(pix, (uint32_t)(r + v) * 0x01010101u, V, false);
        };
        if (live && fast) {
            int above = y * W + x0, below = above;
            tally((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, above, 0, 0) &
                      row_mask((int)P.u[0], j8), 0);
            // not unrolled: the kernel is bound by cache-line traffic, not by issue or latency,
            // and more rows in flight per wave cost the dense batch 4 % (x2) to 5 % (x4) and
            // r = 31 11 % while gaining 7 % on sparse lists
#pragma unroll 1
            for (int v = 1; v <= r; ++v) {
                const uint32_t mask = row_mask((int)P.u[v], j8);
                above -= W;
                below += W;
                const uint32_t pa = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, above, 0, 0);
                const uint32_t pb = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, below, 0, 0);
                tally(pa & mask, -v);
                tally(pb & mask, v);
            }
        } else if (live) {
            for (int v = -r; v <= r; ++v) {
                const int row = min(max(y + v, 0), H - 1) * W;
                uint32_t pix = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = min(max(x0 + k, 0), W - 1);
                    pix |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, row + cx, 0, 0)
                           << (8 * k);
                }
                tally(pix & row_mask((int)P.u[abs(v)], j8), v);
            }
        }
        const int m10 = group_sum<L>((int)(T - (uint32_t)r * S));
        const int m01 = group_sum<L>((int)(V - (uint32_t)r * S));
        if (live && j == 0) {
            P.angles[i] = (m10 | m01) == 0 ? 0.0f : atan2f((float)m01, (float)m10);
            if (P.moments) reinterpret_cast<int2*>(P.moments)[i] = make_int2(m10, m01);
        }
    }
}

}  // namespace

hipError_t launch_orient(const OrientParams& p, uint32_t chunks, hipStream_t stream) {
    if (p.n_frames == 0 || p.cap == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.width, p.height) || chunks == 0 || p.radius == 0 ||
        p.radius > kOrientMaxRadius)
        return hipErrorInvalidValue;
    const dim3 grid(chunks, p.n_frames), block(kOrientThreads);
    if (p.radius <= 3)
        hipLaunchKernelGGL(orient_kernel<2>, grid, block, 0, stream, p);
    else if (p.radius <= 7)
        hipLaunchKernelGGL(orient_kernel<4>, grid, block, 0, stream, p);
    else if (p.radius <= 15)
        hipLaunchKernelGGL(orient_kernel<8>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(orient_kernel<16>, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
