// fdf_track.hip -- pyramidal Lucas-Kanade tracking of keypoints from one frame into another on
// MI355X (gfx950) (extension, fdf_track_device: calcOpticalFlowPyrLK with an integer contract; the
// other half of a FAST + KLT front end).  include/fdf.h has the rule; in short, per point and
// level, coarsest first, with positions in 1/2048 pixel ("Q11"):
//   P(i, j)  = S_prev(Xp + 2048 i, Yp + 2048 j), |i|, |j| <= r + 1      the template, sampled once
//   Gx, Gy   = Scharr of P, |i|, |j| <= r;  A11, A12, A22 = sums of Gx Gx, Gx Gy, Gy Gy
//   per iteration  E = S_next(Xn + 2048 i, Yn + 2048 j) - P,  b1 = sum E Gx,  b2 = sum E Gy,
//                  (dx, dy) = -A^-1 b,  (Xn, Yn) += floor((dx, dy) * 65536 + 0.5)
// S is the resize's bilinear sum kept to 5 fractional bits.  Every sum is an integer sum, exact in
// any order; only the 2 x 2 solve is binary64, a fixed sequence of single operations, so the file
// is compiled without floating-point contraction.
//
// One wave per point, four points per workgroup pass, a frame's points shared over `chunks`
// workgroups as in fdf_orient.hip.  Window pixel k = lane + 64 s (s < NS, the kernel's template
// argument: ceil((2 r + 1)^2 / 64) <= 16, one instance per count) belongs to the lane, which holds P, Gx and Gy of its
// pixels in registers across the iterations of a level.  The template's (2 r + 3)^2 samples are
// computed once per level, 64 per step, and shared through the wave's own 2.2 KB of LDS (in-order
// within a wave: a wave-level fence, no workgroup barrier -- the waves of a workgroup run
// different points and never meet).  The five sums are reduced over the wave with DPP moves and
// lane reads (integers: any order gives the same sum) and are then wave-uniform, so the solve,
// the tests and all control flow (level skip, loss, convergence) are scalar branches: there is
// no divergence inside a point.
//
// Bounds: a point or guess outside level 0 is skipped before any frame byte is read; positions
// are checked against the level after every update; every tap is clamped into the level and read
// through a buffer resource of exactly the level's width * height bytes (an out-of-range buffer
// load returns 0 and touches no memory).  Writes go to index i of the workgroup's range only,
// below min(offs[f + 1], cap).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

#pragma clang fp contract(off)

namespace fdfk {

namespace {

constexpr int kTrackWaves = kTrackThreads / 64;
constexpr int kTrackPatchSide = 2 * (int)kTrackMaxRadius + 3;
constexpr int kTrackPatch = (kTrackPatchSide * kTrackPatchSide + 3) / 4 * 4;   // u16 entries
constexpr uint32_t kTrackIdle = 0x10000u;             // ij of a slot past the window: pixel (0, 0), flagged

// One level of one frame behind a buffer resource, and the bilinear sample of the contract.
struct Level {
    __amdgpu_buffer_rsrc_t rs;
    int W, H;
};
struct Weights { uint32_t x0, x1, y0, y1; };         // 2048 - q, q per axis

__device__ __forceinline__ Weights weights_of(int X, int Y) {
    const uint32_t qx = (uint32_t)X & 2047u, qy = (uint32_t)Y & 2047u;
    return {kResizeOne - qx, qx, kResizeOne - qy, qy};
}

// S at integer tap (cx, cy) (any value: clamped here) with the position's fractional weights.
__device__ __forceinline__ int sample(const Level& L, const Weights& w, int cx, int cy) {
    const int x0 = min(max(cx, 0), L.W - 1), x1 = min(max(cx + 1, 0), L.W - 1);
    const int y0 = min(max(cy, 0), L.H - 1) * L.W, y1 = min(max(cy + 1, 0), L.H - 1) * L.W;
    auto px = [&](int at) {
        return (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(L.rs, at, 0, 0);
    };
    const uint32_t t00 = px(y0 + x0), t10 = px(y0 + x1), t01 = px(y1 + x0), t11 = px(y1 + x1);
    // h <= 255 * 2048 and the sum is below 2^30, as in the resize kernel
    const uint32_t h0 = t00 * w.x0 + t10 * w.x1, h1 = t01 * w.x0 + t11 * w.x1;
    return (int)((h0 * w.y0 + h1 * w.y1 + kTrackSampleHalf) >> kTrackSampleShift);
}

// The sum of an int over the wave as a scalar: DPP moves inside each row of 16 lanes (no LDS
// permutes), then the four rows' sums read into SGPRs.  Every lane of the wave is active here.
__device__ __forceinline__ int wave_sum32(int v) {
    v = group_sum<16>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// The same for a lane's int64 partial sum, |v| < 2^44 (a lane adds at most 16 terms below 2^35),
// as two int sums: the low 20 bits (below 2^26 over the wave) and the rest (below 2^30).
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    const int lo = (int)(v & 0xfffff), hi = (int)(v >> 20);
    return (int64_t)wave_sum32(hi) * (1 << 20) + wave_sum32(lo);
}

struct Tracked { uint32_t reason, iters, err; int X, Y; };

__device__ __forceinline__ bool inside(int X, int Y, int W, int H) {
    return X >= 0 && Y >= 0 && X <= (W - 1) * (int)kResizeOne && Y <= (H - 1) * (int)kResizeOne;
}

// One point through the levels (every argument and every branch wave-uniform but `lane`, `ij`).
template <int NS>
__device__ __forceinline__ Tracked track_point(const TrackParams& P, uint32_t f, int X0, int Y0,
                                               bool guessed, int GX, int GY, uint16_t* patch,
                                               const uint32_t (&ij)[NS], int lane) {
    const int r = (int)P.radius, side = 2 * r + 1, pside = side + 2;
    const int W0 = (int)P.levels[0].width, H0 = (int)P.levels[0].height;
    const int top = (int)P.n_levels - 1;
    Tracked out{kTrackSkipped, 0u, kTrackNoErr, -1, -1};
    int64_t Dx = 0, Dy = 0;
    if (guessed) {
        Dx = track_map_disp((int64_t)GX - X0, W0, (int)P.levels[top].width);
        Dy = track_map_disp((int64_t)GY - Y0, H0, (int)P.levels[top].height);
    }
    int p[NS], gx[NS], gy[NS];
    int Xn = 0, Yn = 0;
    Level next{};
    for (int l = top; l >= 0; --l) {
        const TrackLevel& T = P.levels[l];
        const int W = (int)T.width, H = (int)T.height;
        if (l < top) {
            Dx = track_map_disp(Dx, (int)P.levels[l + 1].width, W);
            Dy = track_map_disp(Dy, (int)P.levels[l + 1].height, H);
        }
        const int Xp = (int)track_map_pos(X0, W0, W), Yp = (int)track_map_pos(Y0, H0, H);

        // the template's samples: one pair of fractional weights serves the whole patch
        {
            const Level prev{frame_rsrc(T.prev + (uint64_t)f * T.prev_stride, W * H), W, H};
            const Weights w = weights_of(Xp, Yp);
            const int bx = (Xp >> 11) - (r + 1), by = (Yp >> 11) - (r + 1);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the last level's reads are done
            __builtin_amdgcn_wave_barrier();
            // four samples per lane and step, so that their loads are in flight together
            const int total = pside * pside;
            for (int k0 = lane; k0 - lane < total; k0 += 256) {
                int v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = min(k0 + 64 * u, total - 1), pj = k / pside;
                    v[u] = sample(prev, w, bx + (k - pj * pside), by + pj);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + 64 * u < total) patch[k0 + 64 * u] = (uint16_t)v[u];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        int64_t s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            {   // no branch: an idle slot reads the patch's first pixel and keeps zeros
                const bool act = !(ij[s] & kTrackIdle);
                const int c = (int)(ij[s] >> 8 & 255u) * pside + (int)(ij[s] & 255u);   // the patch's (i - 1, j - 1)
                const int t00 = patch[c], t10 = patch[c + 1], t20 = patch[c + 2];
                const int t01 = patch[c + pside], t21 = patch[c + pside + 2];
                const int t02 = patch[c + 2 * pside], t12 = patch[c + 2 * pside + 1],
                          t22 = patch[c + 2 * pside + 2];
                p[s] = act ? patch[c + pside + 1] : 0;
                gx[s] = act ? 3 * (t20 - t00) + 10 * (t21 - t01) + 3 * (t22 - t02) : 0;
                gy[s] = act ? 3 * (t02 - t00) + 10 * (t12 - t10) + 3 * (t22 - t20) : 0;
                s11 += (int64_t)gx[s] * gx[s];
                s12 += (int64_t)gx[s] * gy[s];
                s22 += (int64_t)gy[s] * gy[s];
            }
        }
        // below 2^44: exact as doubles
        const double a11 = (double)wave_sum(s11), a12 = (double)wave_sum(s12),
                     a22 = (double)wave_sum(s22);
        const double pe = a11 - P.tau, qe = a22 - P.tau;
        const bool usable = pe + qe > 0.0 && pe * qe - a12 * a12 > 0.0;
        if (!usable) {
            if (l > 0) continue;
            out.reason = kTrackEigen;
            return out;
        }
        const double det = a11 * a22 - a12 * a12;
        Xn = Xp + (int)Dx;
        Yn = Yp + (int)Dy;
        if (!inside(Xn, Yn, W, H)) {
            out.reason = kTrackLeft;
            return out;
        }
        next = Level{frame_rsrc(T.next + (uint64_t)f * T.next_stride, W * H), W, H};
        for (uint32_t it = 0; it < P.max_iters; ++it) {
            const Weights w = weights_of(Xn, Yn);
            const int bx = (Xn >> 11) - r, by = (Yn >> 11) - r;
            int64_t t1 = 0, t2 = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                // no branch, all loads of the lane in flight together; an idle slot has Gx = Gy = 0
                const int e = sample(next, w, bx + (int)(ij[s] & 255u), by + (int)(ij[s] >> 8 & 255u)) - p[s];
                t1 += (int64_t)e * gx[s];          // one term fits an int32, the total does not
                t2 += (int64_t)e * gy[s];
            }
            const double b1 = (double)wave_sum(t1), b2 = (double)wave_sum(t2);
            ++out.iters;
            const double dx = (a12 * b2 - a22 * b1) / det, dy = (a12 * b1 - a11 * b2) / det;
            const double FDX = floor(dx * kTrackStepScale + 0.5), FDY = floor(dy * kTrackStepScale + 0.5);
            // every comparison is false for a NaN
            if (!(FDX >= -kTrackStepLimit && FDX <= kTrackStepLimit && FDY >= -kTrackStepLimit &&
                  FDY <= kTrackStepLimit)) {
                out.reason = kTrackStep;
                return out;
            }
            const int fdx = (int)FDX, fdy = (int)FDY;
            Xn += fdx;
            Yn += fdy;
            if (!inside(Xn, Yn, W, H)) {
                out.reason = kTrackLeft;
                return out;
            }
            if ((uint32_t)(abs(fdx) + abs(fdy)) <= P.eps) break;
        }
        Dx = Xn - Xp;
        Dy = Yn - Yp;
    }
    // tracked: the residual at the final position, against level 0's template (still in p)
    const Weights w = weights_of(Xn, Yn);
    const int bx = (Xn >> 11) - r, by = (Yn >> 11) - r;
    int64_t e1 = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int e = sample(next, w, bx + (int)(ij[s] & 255u), by + (int)(ij[s] >> 8 & 255u)) - p[s];
        e1 += ij[s] & kTrackIdle ? 0 : abs(e);
    }
    out.reason = kTrackTracked;
    out.err = (uint32_t)wave_sum(e1);
    out.X = Xn;
    out.Y = Yn;
    return out;
}

template <int NS>
__global__ __launch_bounds__(kTrackThreads) void track_kernel(TrackParams P) {
    __shared__ uint16_t s_patch[kTrackWaves][kTrackPatch];
    const uint32_t f = blockIdx.y;
    const IndexRange fr = frame_range(P.offs, P.cap, f);
    const auto [lo, hi] = wg_share(fr.lo, fr.hi, blockIdx.x, gridDim.x, kTrackWaves);
    if (lo == hi) return;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    const int side = 2 * (int)P.radius + 1, n = side * side;
    const int W0 = (int)P.levels[0].width, H0 = (int)P.levels[0].height;
    // window pixel k = lane + 64 s of the lane: j << 8 | i, both from 0
    uint32_t ij[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int k = lane + 64 * s, j = k / side;
        ij[s] = k < n ? (uint32_t)(j << 8 | (k - j * side)) : kTrackIdle;
    }
    for (uint64_t i = lo + wave; i < hi; i += kTrackWaves) {    // uniform over the wave
        // Positions as int64 first: a u32 coordinate times 2048 may not fit an int
        int64_t X, Y;
        if (P.coords == kTrackU32) {
            const uint2 pt = static_cast<const uint2*>(P.pts)[i];
            X = (int64_t)pt.x * kResizeOne;
            Y = (int64_t)pt.y * kResizeOne;
        } else {
            const int2 pt = static_cast<const int2*>(P.pts)[i];
            X = pt.x;
            Y = pt.y;
        }
        const int64_t XM = (int64_t)(W0 - 1) * kResizeOne, YM = (int64_t)(H0 - 1) * kResizeOne;
        bool live = X >= 0 && Y >= 0 && X <= XM && Y <= YM && (!P.keep || P.keep[i] != 0);
        int2 g = make_int2(0, 0);
        if (P.guess) {
            g = P.guess[i];
            live = live && inside(g.x, g.y, W0, H0);
        }
        Tracked t{kTrackSkipped, 0u, kTrackNoErr, -1, -1};
        if (live)
            t = track_point<NS>(P, f, (int)X, (int)Y, P.guess != nullptr, g.x, g.y, s_patch[wave],
                                ij, lane);
        if (lane == 0) {
            const bool ok = t.reason == kTrackTracked;
            P.next_q11[i] = make_int2(t.X, t.Y);
            P.status[i] = ok ? 1 : 0;
            if (P.next_f32)
                P.next_f32[i] = ok ? make_float2((float)((double)t.X / 2048.0),
                                                 (float)((double)t.Y / 2048.0))
                                   : make_float2(-1.0f, -1.0f);
            if (P.err) P.err[i] = t.err;
            if (P.info) P.info[i] = t.reason | t.iters << 8;
            if (P.matches)
                P.matches[i] = ok ? make_uint2((uint32_t)i, min(t.err / (uint32_t)n, 0xfffeu) |
                                                                kMatchNoDistance << 16)
                                  : make_uint2(kMatchNone, kMatchNoDistance | kMatchNoDistance << 16);
        }
    }
}

}  // namespace

hipError_t launch_track(const TrackParams& p, uint32_t chunks, hipStream_t stream) {
    if (p.n_frames == 0 || p.cap == 0) return hipSuccess;
    if (p.n_frames > 65535u || chunks == 0 || p.radius == 0 || p.radius > kTrackMaxRadius ||
        p.max_iters == 0 || p.max_iters > kTrackMaxIters || p.n_levels == 0 ||
        p.n_levels > kTrackMaxLevels || (p.coords != kTrackU32 && p.coords != kTrackQ11) ||
        !p.pts || !p.offs || !p.next_q11 || !p.status || !(p.tau >= 0.0))
        return hipErrorInvalidValue;
    for (uint32_t l = 0; l < p.n_levels; ++l) {
        const TrackLevel& L = p.levels[l];
        if (!L.prev || !L.next || L.width == 0 || L.height == 0 || L.width > kResizeMaxSide ||
            L.height > kResizeMaxSide || (uint64_t)L.width * L.height > kOrientMaxPixels)
            return hipErrorInvalidValue;
    }
    const dim3 grid(chunks, p.n_frames), block(kTrackThreads);
    const uint32_t n = (2 * p.radius + 1) * (2 * p.radius + 1), slots = (n + 63) / 64;
    switch (slots) {        // the slot counts of r = 1..15: every instance uses all its slots
#define FDF_TRACK_CASE(NS) \
    case NS: hipLaunchKernelGGL(track_kernel<NS>, grid, block, 0, stream, p); break;
        FDF_TRACK_CASE(1) FDF_TRACK_CASE(2) FDF_TRACK_CASE(3) FDF_TRACK_CASE(4) FDF_TRACK_CASE(5)
        FDF_TRACK_CASE(6) FDF_TRACK_CASE(7) FDF_TRACK_CASE(9) FDF_TRACK_CASE(10) FDF_TRACK_CASE(12)
        FDF_TRACK_CASE(14) FDF_TRACK_CASE(16)
#undef FDF_TRACK_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fdfk
