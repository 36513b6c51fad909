// fdf_warp.hip -- exact bilinear warp of 8-bit frames by a 3 x 3 model per frame on MI355X
// (gfx950) (extension, fdf_warp_device: warpAffine / warpPerspective with an integer contract;
// the step after fdf_ransac_device / fdf_refine_device).
//
// The model maps a destination pixel (x, y) to a source position (include/fdf.h has the rule):
//   P = (h0 x + h1 y) + h2,  Q = (h3 x + h4 y) + h5,  w = (h6 x + h7 y) + h8,
//   FX = floor((P / w) * 2048 + 0.5),  FY = floor((Q / w) * 2048 + 0.5),
// every step one binary64 operation; the pixel is valid iff w > 0 and |FX|, |FY| <= 2^30.  Then
// X = (int)FX, ix = X >> 11, qx = X & 2047 (the same for y) and
//   out = (sum over a, b in {0, 1} of wy_b * wx_a * T(ix + a, iy + b) + 2^21) >> 22,
// the resize kernel's sum.  T clamps the tap into the frame (replicate) or is `fill` outside it
// (constant); an invalid pixel is `fill`.  The mask byte is 1 iff the pixel is valid and the
// position lies inside the source frame.
//
// The whole file is compiled without floating-point contraction, and P, Q and w are computed per
// pixel as written (no per-column increments: they change the bits); `/` is the correctly rounded
// v_div_scale / v_div_fmas / v_div_fixup sequence.  The nine doubles of a frame's model are
// wave-uniform: scalar loads.  A model with h6 = h7 = 0 and h8 = 1 (an affine one as the estimator
// leaves it) has w = 1 for every pixel and P / 1 = P bit for bit, so warp_kernel skips the two
// divisions for it under a wave-uniform branch (0.35 -> 0.26 ms for 64 frames of 1080p).
//
// warp_kernel (destination width >= 4): a thread owns 4 adjacent destination columns of one row;
// per pixel four byte loads through the source frame's buffer resource, at indices clamped into
// the frame in both border modes (constant: the loaded value is replaced by `fill` afterwards),
// then one dword store of the 4 pixels and one of the 4 mask bytes.  The last group of a width
// that is no multiple of 4 covers the last 4 columns, overlapping its neighbour with equal
// values.  Threads are numbered over (block of 4 rows, column group, row of the block), so that a
// wave covers 64 x 4 pixels instead of 256 x 1 (under a rotation its taps cross a quarter of the
// source rows: 0.94 -> 0.55 ms at 30 degrees) and no lane idles whatever the width and height.
// warp_any_kernel (destination widths below 4): a thread per destination pixel, byte stores.
// Both call the same warp_pixel and give the same integers.  Loads and stores go through buffer
// resources of exactly the frame's width * height bytes on both sides (an out-of-range access
// returns 0 and touches no memory); gap bytes between destination frames are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

#pragma clang fp contract(off)

namespace fdfk {

namespace {

constexpr double kWarpLimit = 0x1p30;     // |FX|, |FY| of a valid pixel

struct Model { double h[9]; };

// Frame f's nine doubles (wave-uniform).
__device__ __forceinline__ Model load_model(const WarpParams& P, uint32_t f) {
    const double* m = reinterpret_cast<const double*>(
        static_cast<const uint8_t*>(P.models) + (uint64_t)f * P.model_stride);
    Model M;
#pragma unroll
    for (int k = 0; k < 9; ++k) M.h[k] = m[k];
    return M;
}

struct Pixel { uint32_t value, inside; };

// Destination pixel (x, y) of a frame whose source is behind `rs`.  UNIT: the model has
// h6 = h7 = 0 and h8 = 1.
template <bool UNIT>
__device__ __forceinline__ Pixel warp_pixel(const WarpParams& P, const Model& M,
                                            __amdgpu_buffer_rsrc_t rs, int x, int y) {
    const int SW = (int)P.src_w, SH = (int)P.src_h;
    const double xd = (double)x, yd = (double)y;
    const double* h = M.h;
    const double p = (h[0] * xd + h[1] * yd) + h[2];
    const double q = (h[3] * xd + h[4] * yd) + h[5];
    const double w = (h[6] * xd + h[7] * yd) + h[8];
    // UNIT: w is 1 for every pixel, and P / 1 is P bit for bit
    const double sx = UNIT ? p : p / w, sy = UNIT ? q : q / w;
    const double FX = floor(sx * 2048.0 + 0.5), FY = floor(sy * 2048.0 + 0.5);
    // every comparison is false for a NaN
    const bool valid = w > 0.0 && FX >= -kWarpLimit && FX <= kWarpLimit && FY >= -kWarpLimit &&
                       FY <= kWarpLimit;
    const int X = valid ? (int)FX : 0, Y = valid ? (int)FY : 0;
    const int ix = X >> 11, iy = Y >> 11;
    const uint32_t qx = (uint32_t)X & 2047u, qy = (uint32_t)Y & 2047u;
    // the taps, clamped into the frame before use in both modes: |ix|, |iy| <= 2^19
    const int cx0 = min(max(ix, 0), SW - 1), cx1 = min(max(ix + 1, 0), SW - 1);
    const int cy0 = min(max(iy, 0), SH - 1), cy1 = min(max(iy + 1, 0), SH - 1);
    auto px = [&](int cx, int cy) {
        return (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, cy * SW + cx, 0, 0);
    };
    uint32_t t00 = px(cx0, cy0), t10 = px(cx1, cy0), t01 = px(cx0, cy1), t11 = px(cx1, cy1);
    if (P.border == kWarpConstant) {
        const bool x0_in = cx0 == ix, x1_in = cx1 == ix + 1, y0_in = cy0 == iy, y1_in = cy1 == iy + 1;
        t00 = x0_in && y0_in ? t00 : P.fill;
        t10 = x1_in && y0_in ? t10 : P.fill;
        t01 = x0_in && y1_in ? t01 : P.fill;
        t11 = x1_in && y1_in ? t11 : P.fill;
    }
    // h <= 255 * 2048 and the sum is below 2^30, as in the resize kernel
    const uint32_t h0 = t00 * (kResizeOne - qx) + t10 * qx;
    const uint32_t h1 = t01 * (kResizeOne - qx) + t11 * qx;
    const uint32_t s = h0 * (kResizeOne - qy) + h1 * qy + kResizeHalf;
    Pixel r;
    r.value = valid ? s >> kResizeShift : P.fill;
    r.inside = valid && X >= 0 && X <= (SW - 1) * (int)kResizeOne && Y >= 0 &&
                       Y <= (SH - 1) * (int)kResizeOne
                   ? 1u : 0u;
    return r;
}

__global__ __launch_bounds__(kWarpThreads) void warp_kernel(WarpParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kWarpThreads + threadIdx.x;
    // Blocks of kWarpTileRows rows, and inside a block the row runs fastest: a wave covers 16
    // column groups x 4 rows.  The last block may be shorter; it then has fewer threads.
    const uint32_t per = kWarpTileRows * P.groups;
    const uint32_t rb = gid / per, rem = gid % per;
    if (kWarpTileRows * rb >= P.dst_h) return;
    const uint32_t rows = min(kWarpTileRows, P.dst_h - kWarpTileRows * rb);
    const bool full = rows == kWarpTileRows;
    const uint32_t g = full ? rem / kWarpTileRows : rem / rows;
    const uint32_t y = kWarpTileRows * rb + (full ? rem % kWarpTileRows : rem % rows);
    if (g >= P.groups) return;
    const int DW = (int)P.dst_w, DH = (int)P.dst_h;
    const __amdgpu_buffer_rsrc_t rs =
        frame_rsrc(P.src + (uint64_t)f * P.src_stride, (int)(P.src_w * P.src_h));
    const Model M = load_model(P, f);
    // the last group of a width that is no multiple of 4 moves left onto its neighbour
    const int x0 = min(4 * (int)g, DW - 4);
    uint32_t out = 0, inside = 0;
    // an affine model as the estimator leaves it: no division (wave-uniform, the same bits)
    const bool unit = M.h[6] == 0.0 && M.h[7] == 0.0 && M.h[8] == 1.0;
    if (unit) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Pixel r = warp_pixel<true>(P, M, rs, x0 + k, (int)y);
            out |= r.value << (8 * k);
            inside |= r.inside << (8 * k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Pixel r = warp_pixel<false>(P, M, rs, x0 + k, (int)y);
            out |= r.value << (8 * k);
            inside |= r.inside << (8 * k);
        }
    }
    const int at = (int)y * DW + x0;
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.dst + (uint64_t)f * P.dst_stride, DW * DH);
    __builtin_amdgcn_raw_buffer_store_b32(out, ro, at, 0, 0);
    if (P.mask) {
        const __amdgpu_buffer_rsrc_t rm = frame_rsrc(P.mask + (uint64_t)f * P.dst_stride, DW * DH);
        __builtin_amdgcn_raw_buffer_store_b32(inside, rm, at, 0, 0);
    }
}

__global__ __launch_bounds__(kWarpThreads) void warp_any_kernel(WarpParams P) {
    const uint32_t f = blockIdx.y;
    const uint32_t gid = blockIdx.x * kWarpThreads + threadIdx.x;
    if (gid >= P.dst_w * P.dst_h) return;
    const int DW = (int)P.dst_w, DH = (int)P.dst_h;
    const __amdgpu_buffer_rsrc_t rs =
        frame_rsrc(P.src + (uint64_t)f * P.src_stride, (int)(P.src_w * P.src_h));
    const Model M = load_model(P, f);
    const Pixel r = warp_pixel<false>(P, M, rs, (int)(gid % P.dst_w), (int)(gid / P.dst_w));
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc(P.dst + (uint64_t)f * P.dst_stride, DW * DH);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)r.value, ro, (int)gid, 0, 0);
    if (P.mask) {
        const __amdgpu_buffer_rsrc_t rm = frame_rsrc(P.mask + (uint64_t)f * P.dst_stride, DW * DH);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)r.inside, rm, (int)gid, 0, 0);
    }
}

}  // namespace

hipError_t launch_warp(const WarpParams& p, hipStream_t stream) {
    if (p.n_frames == 0) return hipSuccess;
    if (!frames_fit_launch(p.n_frames, p.src_w, p.src_h) ||
        !frames_fit_launch(p.n_frames, p.dst_w, p.dst_h) || p.src_w > kResizeMaxSide ||
        p.src_h > kResizeMaxSide || !p.src || !p.dst || !p.models || p.model_stride < kWarpModelBytes ||
        p.model_stride % 8 || reinterpret_cast<uintptr_t>(p.models) % 8 || p.border > kWarpConstant ||
        p.fill > 255u || p.groups != (p.dst_w + 3) / 4)
        return hipErrorInvalidValue;
    const bool wide = p.dst_w >= 4;
    const uint64_t threads = wide ? (uint64_t)p.groups * p.dst_h : (uint64_t)p.dst_w * p.dst_h;
    const uint64_t blocks = (threads + kWarpThreads - 1) / kWarpThreads;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks, p.n_frames), block(kWarpThreads);
    if (wide)
        hipLaunchKernelGGL(warp_kernel, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(warp_any_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
