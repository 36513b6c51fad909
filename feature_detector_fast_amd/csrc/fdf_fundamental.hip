// fdf_fundamental.hip -- RANSAC estimation of a fundamental matrix from matches or tracks on
// MI355X (gfx950) (extension, fdf_fundamental_device: the epipolar outlier test of a moving
// camera or a stereo pair, where no single homography fits).  The contract is include/fdf.h's:
// integer sampling of 8 correspondences, a fit and a score that are fixed sequences of binary64
// operations, ties by index.  The shape is fdf_ransac.hip's: its compaction kernel, then
//
// fundamental_hypothesis_kernel<WAVES>.  Grid (hypothesis block of 64, frame), one hypothesis per
// lane: sample, normalise, build the 8 x 9 system, find its null vector by Gauss-Jordan
// elimination with full pivoting, denormalise, scale, then count the inliers over all of the
// frame's correspondences, which stream through LDS in tiles of 256 and are read as broadcasts.
// WAVES = 1 or kRansacWideWaves by fdf_ransac.hip's grid rule.  The 72 doubles of the system live
// in registers: every loop of the elimination is unrolled, and a step's run-time pivot row and
// column are exchanged with the step's own by selects, so no array is indexed dynamically.  An
// invalid hypothesis walks the same code (uniform control flow) and its count is replaced by
// kRansacInvalid.
//
// fundamental_finalise_kernel.  One workgroup per frame: the largest count, ties to the lowest
// hypothesis, every thread re-fits the winner (the same bits), thread 0 writes the fdf_model and
// thread t decides the inlier bytes of queries t, t + 256, ... from the original arrays.
//
// fundamental_check_kernel (fdf_fundamental_check_device).  One workgroup per frame and no
// scratch: the caller's matrix scores the frame's queries straight from the original arrays; the
// two integer counts add through LDS.
//
// The whole file is compiled without floating-point contraction, as fdf_ransac.hip is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"
#include "fdf_ransac_impl.h"

#pragma clang fp contract(off)

namespace fdfk {

namespace {

constexpr double kFundInf = __builtin_huge_val();

// Step `step` of the Gauss-Jordan elimination with full pivoting (include/fdf.h): the pivot comes
// to A[step][step] by exchanging two rows and two columns (selects on the run-time pivot), so the
// rows and columns not yet used are the physical ones from `step` on and every index is a
// compile-time one; row_id and col_id remember where a physical row or column came from, for the
// tie rule and the result.  False: the pivot is below 2^-20, or no magnitude is a number.
template <int step>
__device__ __forceinline__ bool fundamental_step(double (&A)[8][9], uint32_t (&row_id)[8],
                                                 uint32_t (&col_id)[9]) {
    // the largest magnitude, ties to the lowest row, then column, of the system as built; a
    // NaN never wins
    double best = -1.0;
    uint32_t best_id = 0, at = (uint32_t)(step * 16 + step);   // physical row * 16 + column
#pragma unroll
    for (int r = step; r < 8; ++r) {
#pragma unroll
        for (int j = step; j < 9; ++j) {
            const double mag = __builtin_fabs(A[r][j]);
            const uint32_t id = row_id[r] * 16u + col_id[j];
            const bool wins = mag > best || (mag == best && id < best_id);
            best = wins ? mag : best;
            best_id = wins ? id : best_id;
            at = wins ? (uint32_t)(r * 16 + j) : at;
        }
    }
    const uint32_t pr = at >> 4, pc = at & 15u;
    // exchange rows step and pr (their columns below step are dead)
#pragma unroll
    for (int r = step + 1; r < 8; ++r) {
        const bool hit = pr == (uint32_t)r;
#pragma unroll
        for (int j = step; j < 9; ++j) {
            const double top = A[step][j];
            A[step][j] = hit ? A[r][j] : top;
            A[r][j] = hit ? top : A[r][j];
        }
        const uint32_t top_id = row_id[step];
        row_id[step] = hit ? row_id[r] : top_id;
        row_id[r] = hit ? top_id : row_id[r];
    }
    // exchange columns step and pc, in the used rows too
#pragma unroll
    for (int j = step + 1; j < 9; ++j) {
        const bool hit = pc == (uint32_t)j;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const double left = A[r][step];
            A[r][step] = hit ? A[r][j] : left;
            A[r][j] = hit ? left : A[r][j];
        }
        const uint32_t left_id = col_id[step];
        col_id[step] = hit ? col_id[j] : left_id;
        col_id[j] = hit ? left_id : col_id[j];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r == step) continue;                              // compile time
        const double m = A[r][step] / A[step][step];
#pragma unroll
        for (int j = step + 1; j < 9; ++j) A[r][j] = A[r][j] - m * A[step][j];
    }
    return best >= kRansacMinPivot;
}

// The fundamental matrix of the sample `c`, every operation as include/fdf.h writes it.
__device__ __forceinline__ bool fundamental_fit(const Corr (&c)[8], double (&F)[9]) {
    // 1. normalise both sides over the 8 points
    double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sx = sx + c[k].x;
        sy = sy + c[k].y;
        su = su + c[k].u;
        sv = sv + c[k].v;
    }
    const double cx = sx / 8.0, cy = sy / 8.0, cu = su / 8.0, cv = sv / 8.0;
    double d = 0.0, e = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        d = d + (__builtin_fabs(c[k].x - cx) + __builtin_fabs(c[k].y - cy));
        e = e + (__builtin_fabs(c[k].u - cu) + __builtin_fabs(c[k].v - cv));
    }
    bool valid = d > 0.0 && d < kFundInf && e > 0.0 && e < kFundInf;
    const double s = 16.0 / d, t = 16.0 / e;

    // 2. the rows of [u v 1] F [x y 1]^T = 0
    double A[8][9];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double X = (c[k].x - cx) * s, Y = (c[k].y - cy) * s;
        const double U = (c[k].u - cu) * t, V = (c[k].v - cv) * t;
        A[k][0] = U * X;
        A[k][1] = U * Y;
        A[k][2] = U;
        A[k][3] = V * X;
        A[k][4] = V * Y;
        A[k][5] = V;
        A[k][6] = X;
        A[k][7] = Y;
        A[k][8] = 1.0;
    }

    // 3. Gauss-Jordan with full pivoting, 8 steps
    uint32_t row_id[8], col_id[9];
#pragma unroll
    for (int r = 0; r < 8; ++r) row_id[r] = (uint32_t)r;
#pragma unroll
    for (int j = 0; j < 9; ++j) col_id[j] = (uint32_t)j;
    valid = fundamental_step<0>(A, row_id, col_id) && valid;
    valid = fundamental_step<1>(A, row_id, col_id) && valid;
    valid = fundamental_step<2>(A, row_id, col_id) && valid;
    valid = fundamental_step<3>(A, row_id, col_id) && valid;
    valid = fundamental_step<4>(A, row_id, col_id) && valid;
    valid = fundamental_step<5>(A, row_id, col_id) && valid;
    valid = fundamental_step<6>(A, row_id, col_id) && valid;
    valid = fundamental_step<7>(A, row_id, col_id) && valid;
    // physical column 8 is the one left unused
    double fn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fn[k] = col_id[8] == (uint32_t)k ? 1.0 : 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const double v = -(A[r][8] / A[r][r]);
#pragma unroll
        for (int k = 0; k < 9; ++k) fn[k] = col_id[r] == (uint32_t)k ? v : fn[k];
    }

    // 4. F = T2^T Fn T1: rows, then columns
    double B[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        B[r][0] = fn[3 * r] * s;
        B[r][1] = fn[3 * r + 1] * s;
        B[r][2] = (fn[3 * r + 2] - B[r][0] * cx) - B[r][1] * cy;
    }
    double G[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double g0 = t * B[0][j], g1 = t * B[1][j];
        G[j] = g0;
        G[3 + j] = g1;
        G[6 + j] = (B[2][j] - g0 * cu) - g1 * cv;
    }

    // 5. the entry of largest magnitude (the lowest on a tie) becomes +1
    double top = -1.0, div = G[0];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double mag = __builtin_fabs(G[k]);
        const bool wins = mag > top;
        top = wins ? mag : top;
        div = wins ? G[k] : div;
    }
    valid = valid && top > 0.0 && top < kFundInf;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        F[k] = G[k] / div;
        valid = valid && __builtin_fabs(F[k]) < kFundInf;
    }
    return valid;
}

// Sampson distance of at most T pixels, without a division; false for any NaN.
__device__ __forceinline__ bool fundamental_inlier(const double (&f)[9], double x, double y,
                                                   double u, double v, double tt) {
    const double l0 = (f[0] * x + f[1] * y) + f[2];
    const double l1 = (f[3] * x + f[4] * y) + f[5];
    const double l2 = (f[6] * x + f[7] * y) + f[8];
    const double m0 = (f[0] * u + f[3] * v) + f[6];
    const double m1 = (f[1] * u + f[4] * v) + f[7];
    const double r = (u * l0 + v * l1) + l2;
    const double g = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    const double e = r * r;
    const double lim = tt * g;
    return g > 0.0 && e <= lim;
}

// Sample and fit hypothesis `hyp` of frame `f` over the `m` correspondences at `corr`.
__device__ __forceinline__ bool fundamental_model(const double* corr, uint32_t m, uint32_t seed,
                                                  uint32_t f, uint32_t hyp, double (&F)[9]) {
    uint32_t idx[8];
    const bool drawn = ransac_sample<8, kFundamentalMaxDraws>(seed, f, hyp, m, idx, nullptr);
    Corr c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[k] = Corr{0.0, 0.0, 0.0, 0.0};
        if (drawn) {                                          // idx[k] < m
            const double2* src = reinterpret_cast<const double2*>(corr + 4 * (uint64_t)idx[k]);
            const double2 a = src[0], b = src[1];
            c[k] = Corr{a.x, a.y, b.x, b.y};
        }
    }
    const bool fitted = fundamental_fit(c, F);
    return drawn && fitted;
}

template <int WAVES>
__global__ __launch_bounds__(kRansacThreads * WAVES) void fundamental_hypothesis_kernel(RansacParams P) {
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
    double F[9];
    const bool valid = fundamental_model(corr, live ? m : 0u, P.seed, f, hyp, F) && live;

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
            count += fundamental_inlier(F, xy.x, xy.y, uv.x, uv.y, P.tt) ? 1u : 0u;
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

__global__ __launch_bounds__(kRansacFrameThreads) void fundamental_finalise_kernel(RansacParams P) {
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

    double F[9];
    const bool refit = fundamental_model(P.corr + 4 * qr.lo, found ? m : 0u, P.seed, f, best, F);
    const bool have = found && refit;
    if (tid == 0) {
        double* out = P.models + 11 * (uint64_t)f;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = have ? F[k] : 0.0;
        uint2* tail = reinterpret_cast<uint2*>(out + 9);
        tail[0] = make_uint2(m, have ? n_inliers : 0u);
        tail[1] = make_uint2(have ? best : kRansacInvalid, n_valid);
    }
    if (P.inliers) {
        for (uint64_t i = qr.lo + tid; i < qr.hi; i += kRansacFrameThreads) {
            Corr c{0.0, 0.0, 0.0, 0.0};
            const bool in = correspondence(P, i, tr, &c) && have &&
                            fundamental_inlier(F, c.x, c.y, c.u, c.v, P.tt);
            P.inliers[i] = in ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(kRansacFrameThreads) void fundamental_check_kernel(FundamentalCheckParams C) {
    __shared__ uint32_t s_corr[kRansacFrameThreads];
    __shared__ uint32_t s_in[kRansacFrameThreads];
    const RansacParams& P = C.r;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const IndexRange tr = frame_range(P.t_offs, P.t_cap, f);

    const double* in = C.models_in + 11 * (uint64_t)f;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = in[k];
    const uint2* in_tail = reinterpret_cast<const uint2*>(in + 9);
    const uint2 tail0 = in_tail[0], tail1 = in_tail[1];       // n_corr, n_inliers; hypothesis, n_valid
    __syncthreads();                                          // models may be models_in
    const bool have = tail1.x != kRansacInvalid;              // uniform

    uint32_t n_corr = 0, n_in = 0;
    for (uint64_t i = qr.lo + tid; i < qr.hi; i += kRansacFrameThreads) {
        Corr c{0.0, 0.0, 0.0, 0.0};
        const bool is = correspondence(P, i, tr, &c);
        const bool inl = is && have && fundamental_inlier(F, c.x, c.y, c.u, c.v, P.tt);
        n_corr += is ? 1u : 0u;
        n_in += inl ? 1u : 0u;
        if (P.inliers) P.inliers[i] = inl ? 1u : 0u;
    }
    s_corr[tid] = n_corr;
    s_in[tid] = n_in;
    __syncthreads();
#pragma unroll
    for (uint32_t step = kRansacFrameThreads / 2; step > 0; step /= 2) {
        if (tid < step) {
            s_corr[tid] += s_corr[tid + step];
            s_in[tid] += s_in[tid + step];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* out = P.models + 11 * (uint64_t)f;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = F[k];
        uint2* tail = reinterpret_cast<uint2*>(out + 9);
        tail[0] = have ? make_uint2(s_corr[0], s_in[0]) : tail0;
        tail[1] = tail1;
    }
}

}  // namespace

hipError_t launch_fundamental(const RansacParams& p, hipStream_t stream) {
    if (p.n_frames == 0) return hipSuccess;
    if (p.n_frames > 65535u || p.q_cap > kMatchMaxCap || p.t_cap > kMatchMaxCap || p.n_hyp == 0 ||
        p.n_hyp > kRansacMaxHyp || p.coords > kRansacF32)
        return hipErrorInvalidValue;
    const dim3 frames(p.n_frames);
    const dim3 hyps((p.n_hyp + kRansacThreads - 1) / kRansacThreads, p.n_frames);
    const hipError_t err = launch_ransac_compact(p, stream);
    if (err != hipSuccess) return err;
    // fdf_ransac.hip's rule: a grid too small to give every SIMD a wave shares a block's scoring
    if ((uint64_t)hyps.x * hyps.y <= kRansacWideMaxBlocks)
        hipLaunchKernelGGL(fundamental_hypothesis_kernel<kRansacWideWaves>, hyps,
                           dim3(kRansacThreads * kRansacWideWaves), 0, stream, p);
    else
        hipLaunchKernelGGL(fundamental_hypothesis_kernel<1>, hyps, dim3(kRansacThreads), 0, stream, p);
    hipLaunchKernelGGL(fundamental_finalise_kernel, frames, dim3(kRansacFrameThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_fundamental_check(const FundamentalCheckParams& p, hipStream_t stream) {
    const RansacParams& r = p.r;
    if (r.n_frames == 0) return hipSuccess;
    if (r.n_frames > 65535u || r.q_cap > kMatchMaxCap || r.t_cap > kMatchMaxCap ||
        r.coords > kRansacF32)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fundamental_check_kernel, dim3(r.n_frames), dim3(kRansacFrameThreads), 0,
                       stream, p);
    return hipGetLastError();
}

}  // namespace fdfk
