// fdf_resize.hip -- exact bilinear resize of 8-bit frames on MI355X (gfx950) (extension,
// fdf_resize_device and fdf_pyramid_device: the scale pyramid ORB-style callers run the
// detector over).
//
// out(x, y) = (sum over a, b in {0, 1} of wy_b * wx_a * I(ix_a, iy_b) + 2^21) >> 22 with the
// taps of include/fdf.h: one word per destination column and row, i0 << 12 | q, w_0 = 2048 - q,
// w_1 = q, i1 = min(i0 + 1, S - 1).  Every tap is clamped before use (i0 <= S - 1, q <= 2048),
// so whatever the tables hold the sum is below 2^30 and every index lies inside the frame.
//
// resize_kernel (source width >= 8, destination width >= 4, source width <= 2 * destination
// width).  A thread owns 4 adjacent destination columns x0 .. x0 + 3 and walks down a strip of
// destination rows; registers only, no LDS.  At a ratio of at most 2 the 8 taps of its columns
// lie within the 8 source bytes that start at its first tap (the positions of columns 3 apart
// differ by at most 6), so per source row it makes one (unaligned) 8-byte buffer load at column
// o = min(i0 of x0, S - 8) and a byte permute per column, with a selector fixed per thread, puts
// the column's two taps into the halves of a dword; a 16-bit dot product with the column's
// packed weights (2048 - q, q) is the horizontally interpolated value, at most 255 * 2048.
// A destination row needs two source rows, each loaded and interpolated horizontally, then the
// vertical sum in 24-bit multiplies.  The second row's interpolated values stay in registers:
// when the next destination row starts at that source row (5 rows of 6 at the pyramid's 6 / 5)
// it neither loads nor interpolates it again -- a branch that is uniform over a wave unless the
// wave straddles two strips (DESIGN.md 4.12 has what it is worth).  The loads of the
// next destination row are issued before the current row is summed and the y taps are fetched
// two rows ahead, two rows per trip so that no load in flight moves between registers.  One
// dword store per row; the last group of a width that is no multiple of 4 covers the last 4
// columns, overlapping its neighbour with equal values.  Threads are numbered over (strip,
// column group) so that no lane idles whatever the width.
// resize_any_kernel (every other shape: destination widths below 4, ratios above 2, sources
// narrower than 8): a thread per destination pixel, four clamped byte loads.
// Both give the same integers.  Loads and stores go through buffer resources of exactly the
// frame's width * height bytes on both sides (an out-of-range access returns 0 and touches no
// memory); gap bytes between destination frames are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

namespace fdfk {

namespace {

struct Tap { int i0, i1; uint32_t q; };

// A table word, clamped for a source axis of `len` pixels.
__device__ __forceinline__ Tap decode_tap(uint32_t word, int len) {
    Tap t;
    t.i0 = min((int)(word >> 12), len - 1);
    t.i1 = min(t.i0 + 1, len - 1);
    t.q = min(word & 0xfffu, kResizeOne);
    return t;
}

__global__ __launch_bounds__(kResizeThreads) void resize_kernel(ResizeParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kResizeThreads + threadIdx.x;
    const uint32_t strip = gid / P.groups, g = gid % P.groups;
    if (strip >= P.strips) return;
    const int SW = (int)P.src_w, SH = (int)P.src_h, DW = (int)P.dst_w, DH = (int)P.dst_h;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.src + (uint64_t)f * P.src_stride, SW * SH);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.dst + (uint64_t)f * P.dst_stride, DW * DH);
    // the last group of a width that is no multiple of 4 moves left onto its neighbour
    const int x0 = min(4 * (int)g, DW - 4);
    const int ys = (int)(strip * P.strip_rows), ye = min(ys + (int)P.strip_rows, DH);

    // the x taps, constant down the strip: the loaded bytes start at column o, column k's two
    // taps are loaded bytes i0 - o and i1 - o (clamped into the 8 loaded bytes: no table can
    // make the permute read anything else), its weights the halves of wx[k]
    uint32_t sel[4], wx[4];
    int o = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Tap t = decode_tap(P.xtaps[x0 + k], SW);
        if (k == 0) o = min(t.i0, SW - 8);
        const uint32_t b0 = (uint32_t)min(max(t.i0 - o, 0), 7), b1 = (uint32_t)min(max(t.i1 - o, 0), 7);
        sel[k] = b0 | (0x0cu << 8) | (b1 << 16) | (0x0cu << 24);      // 0x0c: a zero byte
        wx[k] = (kResizeOne - t.q) | (t.q << 16);
    }
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    struct Row { uint32_t h[4]; };
    auto issue = [&](int r) { return __builtin_amdgcn_raw_buffer_load_b64(rs, r * SW + o, 0, 0); };
    auto interp = [&](decltype(issue(0)) raw) {
        Row v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pair = __builtin_amdgcn_perm((uint32_t)raw[1], (uint32_t)raw[0], sel[k]);
            v.h[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pair),
                                            __builtin_bit_cast(u16x2, wx[k]), 0u, false);
        }
        return v;
    };
    auto yword = [&](int y) { return P.ytaps[min(y, DH - 1)]; };

    // The interpolated second source row of a step is kept: the next destination row usually
    // starts at it (5 rows of 6 at 6 / 5), and then neither loads nor interpolates it again.
    Row kept{};
    auto step = [&](int y, const Tap& t, bool fresh, decltype(issue(0)) raw0,
                    decltype(issue(0)) raw1) {
        Row r0 = kept;
        if (fresh) r0 = interp(raw0);
        const Row r1 = interp(raw1);
        const uint32_t w0 = kResizeOne - t.q, w1 = t.q;
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // h <= 255 * 2048 < 2^24 and w <= 2048: 24-bit products, the sum below 2^30
            const uint32_t s = __umul24(r0.h[k], w0) + __umul24(r1.h[k], w1) + kResizeHalf;
            out |= (s >> kResizeShift) << (8 * k);
        }
        __builtin_amdgcn_raw_buffer_store_b32(out, ro, y * DW + x0, 0, 0);
        kept = r1;
    };

    // Two rows per trip, so that a load in flight is never moved between registers.  A row's
    // pixel loads need its y tap: the tap words are fetched two rows ahead, so that the wait for
    // one is for a load older than every pixel load still in flight.
    Tap ta = decode_tap(yword(ys), SH);
    bool fresh_a = true;
    uint32_t w_odd = yword(ys + 1);
    auto a0 = issue(ta.i0), a1 = issue(ta.i1);
    for (int y = ys; y < ye; y += 2) {
        const uint32_t w_even = yword(y + 2);
        const Tap tb = decode_tap(w_odd, SH);
        const bool fresh_b = tb.i0 != ta.i1;
        decltype(issue(0)) b0 = {0, 0};
        if (fresh_b) b0 = issue(tb.i0);
        const auto b1 = issue(tb.i1);
        step(y, ta, fresh_a, a0, a1);
        w_odd = yword(y + 3);
        ta = decode_tap(w_even, SH);
        fresh_a = ta.i0 != tb.i1;
        if (fresh_a) a0 = issue(ta.i0);
        a1 = issue(ta.i1);
        if (y + 1 < ye) step(y + 1, tb, fresh_b, b0, b1);
    }
}

__global__ __launch_bounds__(kResizeThreads) void resize_any_kernel(ResizeParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kResizeThreads + threadIdx.x;
    if (gid >= P.dst_w * P.dst_h) return;
    const int SW = (int)P.src_w, SH = (int)P.src_h, DW = (int)P.dst_w, DH = (int)P.dst_h;
    const __amdgpu_buffer_rsrc_t rs = frame_rsrc(P.src + (uint64_t)f * P.src_stride, SW * SH);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.dst + (uint64_t)f * P.dst_stride, DW * DH);
    const uint32_t x = gid % P.dst_w, y = gid / P.dst_w;
    const Tap tx = decode_tap(P.xtaps[x], SW), ty = decode_tap(P.ytaps[y], SH);
    auto px = [&](int ix, int iy) {
        return (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, iy * SW + ix, 0, 0);
    };
    const uint32_t h0 = px(tx.i0, ty.i0) * (kResizeOne - tx.q) + px(tx.i1, ty.i0) * tx.q;
    const uint32_t h1 = px(tx.i0, ty.i1) * (kResizeOne - tx.q) + px(tx.i1, ty.i1) * tx.q;
    const uint32_t s = h0 * (kResizeOne - ty.q) + h1 * ty.q + kResizeHalf;
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(s >> kResizeShift), ro, (int)gid, 0, 0);
}

}  // namespace

bool resize_fast_path(uint32_t src_w, uint32_t dst_w) {
    return src_w >= kResizeMinSrcWidth && dst_w >= 4 && (uint64_t)src_w <= 2ull * dst_w;
}

hipError_t launch_resize(const ResizeParams& p, hipStream_t stream) {
    if (p.n_frames == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.src_w, p.src_h) ||
        !frames_fit_launch(p.n_frames, p.dst_w, p.dst_h) || p.src_w > kResizeMaxSide ||
        p.src_h > kResizeMaxSide || !p.src || !p.dst || !p.xtaps || !p.ytaps ||
        p.strip_rows == 0 || p.groups != (p.dst_w + 3) / 4 ||
        p.strips != (p.dst_h + p.strip_rows - 1) / p.strip_rows)
        return hipErrorInvalidValue;
    const bool fast = resize_fast_path(p.src_w, p.dst_w);
    const uint64_t threads = fast ? (uint64_t)p.groups * p.strips : (uint64_t)p.dst_w * p.dst_h;
    const uint64_t blocks = (threads + kResizeThreads - 1) / kResizeThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks, p.n_frames), block(kResizeThreads);
    if (fast)
        hipLaunchKernelGGL(resize_kernel, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(resize_any_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
