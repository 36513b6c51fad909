// fdf_ransac.hip -- RANSAC estimation of an affine map or a homography from matches on MI355X
// (gfx950) (extension, fdf_ransac_device: the reference returns points only; this is the step
// after fdf_match_device / fdf_match_filter_device).  The contract is include/fdf.h's: integer
// sampling, a fit and a score that are fixed sequences of binary64 operations, ties by index.
// Three launches in stream order; no kernel waits for another workgroup.
//
// ransac_compact_kernel.  One workgroup per frame walks the frame's query range in passes of
// 256: a query is a correspondence iff its keep byte is set, its match is not FDF_MATCH_NONE and
// the index lies in the frame's train range (checked before the train coordinates are read).
// Ballots and a per-wave count in LDS give every correspondence its number j in index order;
// x, y, u, v, already doubles, go to corr[lo + j] (lo = the frame's first query index: j never
// exceeds the query's own place, so the frames' parts stay apart), the count to n_corr[f].
//
// ransac_hypothesis_kernel<S, WAVES>.  Grid (hypothesis block of 64, frame), one hypothesis per
// lane: sample, gather the sample's rows, eliminate, substitute, then count the inliers over all
// of the frame's correspondences.  WAVES = 1 (one wave per workgroup) whenever the grid has more
// than kRansacWideMaxBlocks blocks; a smaller grid cannot give every SIMD a wave, so there
// WAVES = 8 waves fit the same 64 hypotheses each (the same bits) and score every eighth
// correspondence of a tile, and their integer counts are added through LDS.  The
// correspondences stream through LDS in tiles of 256 (8 KB): thread t fetches the 16-byte halves
// t, t + threads, ... of the tile with coalesced loads, and in the scoring loop every lane reads
// the same correspondence at the same address (a broadcast: no bank conflicts) while its model
// sits in registers.  The N x N system
// lives in registers too: every loop of the elimination is unrolled and the run-time pivot row
// is applied by selects, so no array is indexed dynamically.  An invalid hypothesis walks the
// same loop (uniform control flow) and its count is replaced by kRansacInvalid.
//
// ransac_finalise_kernel.  One workgroup per frame: the largest count, ties to the lowest
// hypothesis, by a 64-bit key count << 32 | ~h reduced through LDS, and the number of valid
// hypotheses.  Every thread re-fits the winner (the fit is a pure function of its inputs: the
// same bits; the loads are broadcasts), thread 0 writes the fdf_model, and thread t decides the
// inlier bytes of the frame's queries t, t + 256, ... from the original arrays: one store per
// byte of the range, none outside.
//
// The whole file is compiled without floating-point contraction: a - b * c stays v_mul_f64 +
// v_add_f64, as numpy computes it; `/` is the correctly rounded v_div_scale / v_div_fmas /
// v_div_fixup sequence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"

#pragma clang fp contract(off)

namespace fdfk {

namespace {

constexpr double kRansacMinPivot = 0x1p-20;

struct Corr { double x, y, u, v; };

// The bits of a coordinate as a double: exact for both types.
__device__ __forceinline__ double coord(uint32_t bits, uint32_t coords) {
    return coords == kRansacF32 ? (double)__uint_as_float(bits) : (double)bits;
}

// Is query i (inside the frame's query range) a correspondence of the frame whose train range is
// `tr`?  Yes: *c holds it.  The match's index is compared with the range before t_coords is read.
__device__ __forceinline__ bool correspondence(const RansacParams& P, uint64_t i, IndexRange tr,
                                               Corr* c) {
    if (P.keep && P.keep[i] == 0) return false;
    const uint32_t j = P.matches[i].x;
    if (j == kMatchNone || j < tr.lo || j >= tr.hi) return false;
    const uint2 q = P.q_coords[i], t = P.t_coords[j];
    c->x = coord(q.x, P.coords);
    c->y = coord(q.y, P.coords);
    c->u = coord(t.x, P.coords);
    c->v = coord(t.y, P.coords);
    return true;
}

__global__ __launch_bounds__(kRansacFrameThreads) void ransac_compact_kernel(RansacParams P) {
    __shared__ uint32_t s_wave[kRansacFrameThreads / 64];
    const uint32_t f = blockIdx.x, tid = threadIdx.x, wave = tid / 64;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const IndexRange tr = frame_range(P.t_offs, P.t_cap, f);
    uint32_t base = 0;                                        // correspondences before this pass
    for (uint64_t i0 = qr.lo; i0 < qr.hi; i0 += kRansacFrameThreads) {   // uniform
        const uint64_t i = i0 + tid;
        Corr c{0.0, 0.0, 0.0, 0.0};
        const bool is = i < qr.hi && correspondence(P, i, tr, &c);
        const uint64_t mask = wave_ballot(is);
        if ((tid & 63u) == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(mask);
        __syncthreads();
        uint32_t before = base, total = base;
#pragma unroll
        for (uint32_t w = 0; w < kRansacFrameThreads / 64; ++w) {
            const uint32_t n = s_wave[w];
            before += w < wave ? n : 0u;
            total += n;
        }
        if (is) {
            double2* dst = reinterpret_cast<double2*>(P.corr + 4 * (qr.lo + lanes_below_plus(mask, before)));
            dst[0] = make_double2(c.x, c.y);
            dst[1] = make_double2(c.u, c.v);
        }
        base = total;
        __syncthreads();                                      // the next pass rewrites s_wave
    }
    if (tid == 0) P.n_corr[f] = base;
}

// The model of the sample `c` (S = 3: affine, 4: homography) by Gaussian elimination with
// partial pivoting and back substitution, every operation as include/fdf.h writes it.  False:
// a pivot below 2^-20 (or no pivot that is a number).  Everything is unrolled; rows are swapped
// by selects on the run-time pivot row.
template <int S>
__device__ __forceinline__ bool ransac_fit(const Corr (&c)[S], double (&h)[9]) {
    constexpr int N = 2 * S;
    double A[N][N], b[N];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const double row0[8] = {c[k].x, c[k].y, 1.0, 0.0, 0.0, 0.0, -(c[k].u * c[k].x), -(c[k].u * c[k].y)};
        const double row1[8] = {0.0, 0.0, 0.0, c[k].x, c[k].y, 1.0, -(c[k].v * c[k].x), -(c[k].v * c[k].y)};
#pragma unroll
        for (int j = 0; j < N; ++j) {
            A[2 * k][j] = row0[j];
            A[2 * k + 1][j] = row1[j];
        }
        b[2 * k] = c[k].u;
        b[2 * k + 1] = c[k].v;
    }
    bool valid = true;
#pragma unroll
    for (int col = 0; col < N; ++col) {
        // the lowest row with the largest magnitude; a NaN compares false and never wins
        double best = -1.0;
        int p = col;
#pragma unroll
        for (int r = col; r < N; ++r) {
            const double mag = __builtin_fabs(A[r][col]);
            const bool wins = mag > best;
            best = wins ? mag : best;
            p = wins ? r : p;
        }
        valid = valid && best >= kRansacMinPivot;
        // swap rows col and p (columns below col are dead)
#pragma unroll
        for (int j = col; j <= N; ++j) {
            double& top = j < N ? A[col][j] : b[col];
            double pv = top;
#pragma unroll
            for (int r = col + 1; r < N; ++r) {
                double& cell = j < N ? A[r][j] : b[r];
                const bool hit = r == p;
                pv = hit ? cell : pv;
                cell = hit ? top : cell;
            }
            top = pv;
        }
#pragma unroll
        for (int r = col + 1; r < N; ++r) {
            const double m = A[r][col] / A[col][col];
#pragma unroll
            for (int j = col + 1; j < N; ++j) A[r][j] = A[r][j] - m * A[col][j];
            b[r] = b[r] - m * b[col];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = k == 8 ? 1.0 : 0.0;
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double t = b[i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) t = t - A[i][j] * h[j];
        h[i] = t / A[i][i];
    }
    return valid;
}

// Forward transfer error of at most T pixels, without a division; false for any NaN.
__device__ __forceinline__ bool ransac_inlier(const double (&h)[9], double x, double y, double u,
                                              double v, double tt) {
    const double P = (h[0] * x + h[1] * y) + h[2];
    const double Q = (h[3] * x + h[4] * y) + h[5];
    const double w = (h[6] * x + h[7] * y) + h[8];
    const double rx = P - u * w;
    const double ry = Q - v * w;
    const double e = rx * rx + ry * ry;
    const double lim = tt * (w * w);
    return w > 0.0 && e <= lim;
}

// Sample and fit hypothesis `hyp` of frame `f` over the `m` correspondences at `corr`.
template <int S>
__device__ __forceinline__ bool ransac_model(const double* corr, uint32_t m, uint32_t seed,
                                             uint32_t f, uint32_t hyp, double (&h)[9]) {
    uint32_t idx[S];
    const bool drawn = ransac_sample<S>(seed, f, hyp, m, idx, nullptr);
    Corr c[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        c[k] = Corr{0.0, 0.0, 0.0, 0.0};
        if (drawn) {                                          // idx[k] < m
            const double2* src = reinterpret_cast<const double2*>(corr + 4 * (uint64_t)idx[k]);
            const double2 a = src[0], b = src[1];
            c[k] = Corr{a.x, a.y, b.x, b.y};
        }
    }
    const bool fitted = ransac_fit<S>(c, h);
    return drawn && fitted;
}

template <int S, int WAVES>
__global__ __launch_bounds__(kRansacThreads * WAVES) void ransac_hypothesis_kernel(RansacParams P) {
    constexpr uint32_t kThreadsHere = kRansacThreads * WAVES;
    __shared__ double2 s_corr[2 * kRansacTile];
    __shared__ uint32_t s_count[WAVES][kRansacThreads];
    const uint32_t f = blockIdx.y, tid = threadIdx.x;
    const uint32_t lane = tid % kRansacThreads;
    // the wave's number in an SGPR: the scoring loop's counter stays scalar
    const uint32_t wave = WAVES == 1 ? 0u : __builtin_amdgcn_readfirstlane(tid / kRansacThreads);
    const uint32_t hyp = blockIdx.x * kRansacThreads + lane;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const uint32_t m = __builtin_amdgcn_readfirstlane(
        min(P.n_corr[f], (uint32_t)min(qr.hi - qr.lo, (uint64_t)kMatchMaxCap)));
    const double* corr = P.corr + 4 * qr.lo;
    const bool live = hyp < P.n_hyp;
    double h[9];
    const bool valid = ransac_model<S>(corr, live ? m : 0u, P.seed, f, hyp, h) && live;

    const double2* src = reinterpret_cast<const double2*>(corr);
    uint32_t count = 0;
    for (uint32_t j0 = 0; j0 < m; j0 += kRansacTile) {        // uniform over the workgroup
        const uint32_t cnt = min(kRansacTile, m - j0);
#pragma unroll
        for (uint32_t k = 0; k < 2 * kRansacTile / kThreadsHere; ++k) {
            const uint32_t piece = tid + k * kThreadsHere;
            if (piece < 2 * cnt) s_corr[piece] = src[2 * (uint64_t)j0 + piece];
        }
        __syncthreads();
        for (uint32_t k = wave; k < cnt; k += WAVES) {        // uniform over the wave
            const double2 xy = s_corr[2 * k], uv = s_corr[2 * k + 1];
            count += ransac_inlier(h, xy.x, xy.y, uv.x, uv.y, P.tt) ? 1u : 0u;
        }
        __syncthreads();                                      // the next tile overwrites s_corr
    }
    if constexpr (WAVES > 1) {                                // the waves' shares of a hypothesis
        s_count[wave][lane] = count;
        __syncthreads();
        count = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) count += s_count[w][lane];
    }
    if (live && wave == 0) P.counts[(uint64_t)f * P.n_hyp + hyp] = valid ? count : kRansacInvalid;
}

template <int S>
__global__ __launch_bounds__(kRansacFrameThreads) void ransac_finalise_kernel(RansacParams P) {
    __shared__ uint64_t s_key[kRansacFrameThreads];
    __shared__ uint32_t s_valid[kRansacFrameThreads];
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const IndexRange tr = frame_range(P.t_offs, P.t_cap, f);
    const uint32_t m = min(P.n_corr[f], (uint32_t)min(qr.hi - qr.lo, (uint64_t)kMatchMaxCap));
    const uint32_t* counts = P.counts + (uint64_t)f * P.n_hyp;

    // the best (count, lowest hypothesis) as the largest count << 32 | ~hypothesis; 0: none
    uint64_t key = 0;
    uint32_t n_valid = 0;
    for (uint32_t hyp = tid; hyp < P.n_hyp; hyp += kRansacFrameThreads) {
        const uint32_t cnt = counts[hyp];
        if (cnt != kRansacInvalid) {
            ++n_valid;
            key = max(key, ((uint64_t)cnt << 32) | (uint32_t)~hyp);
        }
    }
    s_key[tid] = key;
    s_valid[tid] = n_valid;
    __syncthreads();
#pragma unroll
    for (uint32_t step = kRansacFrameThreads / 2; step > 0; step /= 2) {
        if (tid < step) {
            s_key[tid] = max(s_key[tid], s_key[tid + step]);
            s_valid[tid] += s_valid[tid + step];
        }
        __syncthreads();
    }
    key = s_key[0];
    n_valid = s_valid[0];
    const bool found = n_valid != 0;
    const uint32_t best = found ? ~(uint32_t)key : kRansacInvalid;
    const uint32_t n_inliers = found ? (uint32_t)(key >> 32) : 0u;

    double h[9];
    const bool refit = ransac_model<S>(P.corr + 4 * qr.lo, found ? m : 0u, P.seed, f, best, h);
    const bool have = found && refit;
    if (tid == 0) {
        double* out = P.models + 11 * (uint64_t)f;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = have ? h[k] : 0.0;
        uint2* tail = reinterpret_cast<uint2*>(out + 9);
        tail[0] = make_uint2(m, have ? n_inliers : 0u);
        tail[1] = make_uint2(have ? best : kRansacInvalid, n_valid);
    }
    if (P.inliers) {
        for (uint64_t i = qr.lo + tid; i < qr.hi; i += kRansacFrameThreads) {
            Corr c{0.0, 0.0, 0.0, 0.0};
            const bool in = correspondence(P, i, tr, &c) && have &&
                            ransac_inlier(h, c.x, c.y, c.u, c.v, P.tt);
            P.inliers[i] = in ? 1u : 0u;
        }
    }
}

}  // namespace

hipError_t launch_ransac(const RansacParams& p, hipStream_t stream) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.n_frames > 65535u || p.q_cap > kMatchMaxCap || p.t_cap > kMatchMaxCap || p.n_hyp == 0 ||
        p.n_hyp > kRansacMaxHyp || p.model > kRansacHomography || p.coords > kRansacF32)
        return hipErrorInvalidValue;
    const dim3 frames(p.n_frames);
    const dim3 hyps((p.n_hyp + kRansacThreads - 1) / kRansacThreads, p.n_frames);
    hipLaunchKernelGGL(ransac_compact_kernel, frames, dim3(kRansacFrameThreads), 0, stream, p);
    // a grid too small to give every SIMD a wave: kRansacWideWaves waves share a block's scoring
    const bool wide = (uint64_t)hyps.x * hyps.y <= kRansacWideMaxBlocks;
    const dim3 narrow_block(kRansacThreads), wide_block(kRansacThreads * kRansacWideWaves);
    if (p.model == kRansacAffine) {
        if (wide)
            hipLaunchKernelGGL((ransac_hypothesis_kernel<3, kRansacWideWaves>), hyps, wide_block, 0, stream, p);
        else
            hipLaunchKernelGGL((ransac_hypothesis_kernel<3, 1>), hyps, narrow_block, 0, stream, p);
        hipLaunchKernelGGL(ransac_finalise_kernel<3>, frames, dim3(kRansacFrameThreads), 0, stream, p);
    } else {
        if (wide)
            hipLaunchKernelGGL((ransac_hypothesis_kernel<4, kRansacWideWaves>), hyps, wide_block, 0, stream, p);
        else
            hipLaunchKernelGGL((ransac_hypothesis_kernel<4, 1>), hyps, narrow_block, 0, stream, p);
        hipLaunchKernelGGL(ransac_finalise_kernel<4>, frames, dim3(kRansacFrameThreads), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace fdfk
