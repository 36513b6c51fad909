// fdf_harris.hip -- Harris corner response of keypoints on MI355X (gfx950)
// (extension, fdf_harris_device: the reference returns points only; ORB's HarrisResponses, the
// score ORB ranks its FAST keypoints by).
//
// Input: the points fdf_detect_device (or fdf_select_device) left on the device, frames
// concatenated, frame f = indices [offs[f], min(offs[f+1], cap)).  For every point the sums
//     a = sum Ix^2,   b = sum Iy^2,   c = sum Ix Iy      over the block x block pixels around it
// of the 3 x 3 Sobel gradients, pixels read at clamped coordinates (a replicated border), the
// response R = k_den (a b - c^2) - k_num (a + b)^2 in int64 and its u16 rank score
// (harris_code, fdf_kernels.h).  All of it exact: |Ix|, |Iy| <= 1020, so a lane's sums over
// its column stay below 7 * 1020^2 < 2^23 and a, b, |c| <= 49 * 1020^2 < 2^26.
//
// One kernel, one launch, the (chunk, frame) grid of fdf_orient.hip.  L lanes share a
// keypoint, L = 4 for block 3 and 8 for blocks 5 and 7; lane j < block owns column
// X = x - hb + j of the block (hb = block / 2).  Per window row Y' = y - hb - 1 .. y + hb + 1
// it fetches the dword at column X - 1, whose bytes 0, 1, 2 are that row's left, centre and
// right pixel of the column, and forms
//     h = right - left               the row's horizontal difference
//     s = left + 2 centre + right    its 1-2-1 smoothing
// so that, with the rows above and below,
//     Ix(X, Y) = h[Y-1] + 2 h[Y] + h[Y+1],     Iy(X, Y) = s[Y+1] - s[Y-1].
// The rows are unrolled (block + 2 of them: the loads of a keypoint are all in flight at
// once, the h and s of three rows live in registers).  The L partial sums are added with DPP
// moves (group_sum), lane 0 of the group does the int64 arithmetic and stores: no LDS, no
// atomics, plain vector stores.
//
// Two ways to fetch a row, giving the same integers:
//   fast     the (block + 2)^2 window lies inside the frame and so does the spare byte of the
//            last lane's dword of its last row: one (unaligned) dword buffer load per row;
//   clamped  anything else: three byte loads at clamped coordinates.
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

template <int BLOCK>
__global__ __launch_bounds__(kHarrisThreads) void harris_kernel(HarrisParams P) {
    constexpr int L = BLOCK == 3 ? 4 : 8;                 // lanes of a keypoint
    constexpr int HB = BLOCK / 2;
    constexpr int ROWS = BLOCK + 2;                       // window rows (and columns)
    constexpr uint32_t kPerPass = kHarrisThreads / L;     // keypoints of a workgroup pass
    const uint32_t f = blockIdx.y;
    const IndexRange fr = frame_range(P.offs, P.cap, f);
    const auto [lo, hi] = wg_share(fr.lo, fr.hi, blockIdx.x, gridDim.x, kPerPass);
    if (lo == hi) return;

    const int W = (int)P.width, H = (int)P.height;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.frames + (uint64_t)f * P.frame_stride, W * H);
    const int j = (int)(threadIdx.x % L);                 // the lane's column of the block

    for (uint64_t i0 = lo; i0 < hi; i0 += kPerPass) {     // uniform over the workgroup
        const uint64_t i = i0 + threadIdx.x / L;
        const bool live = i < hi;
        uint2 pt = live ? P.pts[i] : make_uint2(0u, 0u);
        const int x = (int)min(pt.x, P.width - 1u), y = (int)min(pt.y, P.height - 1u);
        const int xl = x - HB - 1 + j, y0 = y - HB - 1;   // the lane's left column, the first row
        // fast: the window inside the frame, and the last dword of its last row too
        const bool fast = x > HB && x + HB + 1 < W && y > HB && y + HB + 1 < H &&
                          (y + HB + 1) * W + (x - HB - 1) + BLOCK + 3 <= W * H;
        int hd[ROWS], sm[ROWS];                           // h and s of the window rows
#pragma unroll
        for (int r = 0; r < ROWS; ++r) hd[r] = sm[r] = 0;
        if (live && j < BLOCK) {
            if (fast) {
                uint32_t pix[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
                    pix[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                        rs, (y0 + r) * W + xl, 0, 0);
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    hd[r] = (int)((pix[r] >> 16) & 0xffu) - (int)(pix[r] & 0xffu);
                    sm[r] = (int)__builtin_amdgcn_udot4(pix[r], 0x00010201u, 0u, false);
                }
            } else {
                const int c0 = min(max(xl, 0), W - 1), c1 = min(max(xl + 1, 0), W - 1),
                          c2 = min(max(xl + 2, 0), W - 1);
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int row = min(max(y0 + r, 0), H - 1) * W;
                    const int pl = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, row + c0, 0, 0);
                    const int pc = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, row + c1, 0, 0);
                    const int pr = (int)__builtin_amdgcn_raw_buffer_load_b8(rs, row + c2, 0, 0);
                    hd[r] = pr - pl;
                    sm[r] = pl + 2 * pc + pr;
                }
            }
        }
        // lanes without a column (j >= BLOCK) and dead lanes add zeros
        int a = 0, b = 0, c = 0;
#pragma unroll
        for (int r = 1; r <= BLOCK; ++r) {
            const int ix = hd[r - 1] + 2 * hd[r] + hd[r + 1];     // |ix|, |iy| <= 1020
            const int iy = sm[r + 1] - sm[r - 1];
            a += __mul24(ix, ix);
            b += __mul24(iy, iy);
            c += __mul24(ix, iy);
        }
        a = group_sum<L>(a);
        b = group_sum<L>(b);
        c = group_sum<L>(c);
        if (live && j == 0) {
            // a, b, |c| < 2^26: a b, c^2 < 2^52; (a + b)^2 < 2^54; times 255 below 2^62
            const int64_t det = (int64_t)a * b - (int64_t)c * c;
            const int64_t tr = (int64_t)a + b;
            const int64_t R = (int64_t)P.k_den * det - (int64_t)P.k_num * (tr * tr);
            P.scores[i] = harris_code(R);
            if (P.responses) P.responses[i] = R;
        }
    }
}

}  // namespace

hipError_t launch_harris(const HarrisParams& p, uint32_t chunks, hipStream_t stream) {
    if (p.n_frames == 0 || p.cap == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.width, p.height) || chunks == 0 ||
        !harris_block_ok(p.block) || p.k_num > kHarrisMaxK || p.k_den == 0 ||
        p.k_den > kHarrisMaxK)
        return hipErrorInvalidValue;
    const dim3 grid(chunks, p.n_frames), block(kHarrisThreads);
    if (p.block == 3)
        hipLaunchKernelGGL(harris_kernel<3>, grid, block, 0, stream, p);
    else if (p.block == 5)
        hipLaunchKernelGGL(harris_kernel<5>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(harris_kernel<7>, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
