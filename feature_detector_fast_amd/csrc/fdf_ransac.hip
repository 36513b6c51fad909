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
// refine_kernel<S> (fdf_refine_device: the compaction kernel again, then this one).  One
// workgroup per frame refits the frame's model over its inliers by least squares, all rounds
// inside the workgroup.  A round is four passes over the frame's compacted correspondences,
// thread t taking j = t, t + 256, ...: the inliers' count and coordinate sums, their mean absolute
// deviations, the 28 (affine: 11) different sums of the normalised normal equations, and the
// count under the new model.  Each pass ends in refine_sum: the 256 lane sums of every quantity
// fold through LDS in the fixed halving order (28 x 256 doubles: 56 KB), the additions of a step
// spread over the workgroup, and every thread reads the totals back and solves redundantly with
// the shared elimination.  Every branch depends on those totals alone, so it is uniform.
//
// The whole file is compiled without floating-point contraction: a - b * c stays v_mul_f64 +
// v_add_f64, as numpy computes it; `/` is the correctly rounded v_div_scale / v_div_fmas /
// v_div_fixup sequence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdf_common.h"
#include "fdf_kernels.h"
#include "fdf_ransac_impl.h"

#pragma clang fp contract(off)

namespace fdfk {

namespace {

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

// Solves the N x N system A h = b by Gaussian elimination with partial pivoting and back
// substitution, every operation as include/fdf.h writes it; h[N..8) = 0 and h[8] = 1.  False: a
// pivot below 2^-20 (or no pivot that is a number).  Everything is unrolled; rows are swapped by
// selects on the run-time pivot row.  fill(A, b) writes the system into the solver's own arrays.
template <int N, typename Fill>
__device__ __forceinline__ bool ransac_solve(Fill fill, double (&h)[9]) {
    double A[N][N], b[N];
    fill(A, b);
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

// The model of the sample `c` (S = 3: affine, 4: homography): its 2 S rows, solved.
template <int S>
__device__ __forceinline__ bool ransac_fit(const Corr (&c)[S], double (&h)[9]) {
    constexpr int N = 2 * S;
    return ransac_solve<N>([&c](double (&A)[N][N], double (&b)[N]) {
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
    }, h);
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

// ---- least-squares refinement of a model over its inliers (fdf_refine_device) -----------------

constexpr double kRefineInf = __builtin_huge_val();

// The frame's sums of K quantities in include/fdf.h's fixed order: acc[k] is this thread's lane
// sum (correspondence j belongs to lane j mod 256); the 256 lane sums fold as
// sum[t] = sum[t] + sum[t + step] for step = 128 .. 1, the K x step additions of a step spread
// over the workgroup.  Every thread leaves with the K totals.
template <int K>
__device__ __forceinline__ void refine_sum(double (&acc)[K], double (*s)[kRansacFrameThreads],
                                           uint32_t tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k][tid] = acc[k];
    __syncthreads();
    for (uint32_t step = kRansacFrameThreads / 2; step > 0; step /= 2) {
        const uint32_t shift = 31u - (uint32_t)__builtin_clz(step);
        for (uint32_t e = tid; e < (uint32_t)K * step; e += kRansacFrameThreads) {
            const uint32_t k = e >> shift, t = e & (step - 1u);
            s[k][t] = s[k][t] + s[k][t + step];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = s[k][0];
    __syncthreads();                                          // the next sum rewrites s
}

__device__ __forceinline__ Corr refine_load(const double* corr, uint64_t j) {
    const double2* src = reinterpret_cast<const double2*>(corr + 4 * j);
    const double2 a = src[0], b = src[1];
    return Corr{a.x, a.y, b.x, b.y};
}

// a[0..5) = the inliers of `h` among the m correspondences: their number, sum x, y, u, v.
__device__ __forceinline__ void refine_score(const double (&h)[9], const double* corr, uint32_t m,
                                             double tt, double (*s)[kRansacFrameThreads],
                                             uint32_t tid, double (&a)[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] = 0.0;
    for (uint64_t j = tid; j < m; j += kRansacFrameThreads) {
        const Corr c = refine_load(corr, j);
        const bool in = ransac_inlier(h, c.x, c.y, c.u, c.v, tt);
        a[0] = a[0] + (in ? 1.0 : 0.0);
        a[1] = a[1] + (in ? c.x : 0.0);
        a[2] = a[2] + (in ? c.y : 0.0);
        a[3] = a[3] + (in ? c.u : 0.0);
        a[4] = a[4] + (in ? c.v : 0.0);
    }
    refine_sum<5>(a, s, tid);
}

// The sums of the normal equations that differ (S = 4: 28, S = 3: 11), with a = (X, Y, 1),
// p = (-(U X), -(U Y)) and q = (-(V X), -(V Y)) the tails of a correspondence's two rows:
//   0..4    XX XY X YY Y        G[i][j] = G[3 + i][3 + j], i <= j < 3 (G[2][2] = n)
//   5..10   XU YU U XV YV V     g[0..6)
//   11..16  X p0, X p1, Y p0, Y p1, p0, p1      G[0..3)[6..8)
//   17..22  X q0, X q1, Y q0, Y q1, q0, q1      G[3..6)[6..8)
//   23..25  p0 p0 + q0 q0, p0 p1 + q0 q1, p1 p1 + q1 q1      G[6][6], G[6][7], G[7][7]
//   26..27  p0 U + q0 V, p1 U + q1 V            g[6], g[7]
template <int S>
constexpr int kRefineSums = S == 4 ? 28 : 11;

// One refit of `h` over its inliers: normalise, accumulate, solve, denormalise into `out`.
// False: the round failed (include/fdf.h).  n and the sums a[1..5) are refine_score's of `h`.
// Uniform over the workgroup: every value a branch depends on comes out of refine_sum.
template <int S>
__device__ __forceinline__ bool refine_round(const double (&h)[9], const double (&a)[5],
                                             const double* corr, uint32_t m, double tt,
                                             double (*s)[kRansacFrameThreads], uint32_t tid,
                                             double (&out)[9]) {
    constexpr int N = 2 * S, K = kRefineSums<S>;
    const double n = a[0];
    const double cx = a[1] / n, cy = a[2] / n, cu = a[3] / n, cv = a[4] / n;
    double d[2] = {0.0, 0.0};
    for (uint64_t j = tid; j < m; j += kRansacFrameThreads) {
        const Corr c = refine_load(corr, j);
        const bool in = ransac_inlier(h, c.x, c.y, c.u, c.v, tt);
        const double dq = __builtin_fabs(c.x - cx) + __builtin_fabs(c.y - cy);
        const double dt = __builtin_fabs(c.u - cu) + __builtin_fabs(c.v - cv);
        d[0] = d[0] + (in ? dq : 0.0);
        d[1] = d[1] + (in ? dt : 0.0);
    }
    refine_sum<2>(d, s, tid);
    if (!(n >= (double)S && d[0] > 0.0 && d[0] < kRefineInf && d[1] > 0.0 && d[1] < kRefineInf))
        return false;
    const double sq = (n + n) / d[0], st = (n + n) / d[1];

    double g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = 0.0;
    for (uint64_t j = tid; j < m; j += kRansacFrameThreads) {
        const Corr c = refine_load(corr, j);
        const bool in = ransac_inlier(h, c.x, c.y, c.u, c.v, tt);
        const double X = (c.x - cx) * sq, Y = (c.y - cy) * sq;
        const double U = (c.u - cu) * st, V = (c.v - cv) * st;
        double term[K];
        term[0] = X * X;
        term[1] = X * Y;
        term[2] = X;
        term[3] = Y * Y;
        term[4] = Y;
        term[5] = X * U;
        term[6] = Y * U;
        term[7] = U;
        term[8] = X * V;
        term[9] = Y * V;
        term[10] = V;
        if constexpr (S == 4) {
            const double p0 = -(U * X), p1 = -(U * Y), q0 = -(V * X), q1 = -(V * Y);
            term[11] = X * p0;
            term[12] = X * p1;
            term[13] = Y * p0;
            term[14] = Y * p1;
            term[15] = p0;
            term[16] = p1;
            term[17] = X * q0;
            term[18] = X * q1;
            term[19] = Y * q0;
            term[20] = Y * q1;
            term[21] = q0;
            term[22] = q1;
            term[23] = p0 * p0 + q0 * q0;
            term[24] = p0 * p1 + q0 * q1;
            term[25] = p1 * p1 + q1 * q1;
            term[26] = p0 * U + q0 * V;
            term[27] = p1 * U + q1 * V;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = g[k] + (in ? term[k] : 0.0);
    }
    refine_sum<K>(g, s, tid);

    double hn[9];
    const bool solved = ransac_solve<N>([&g, n](double (&G)[N][N], double (&b)[N]) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) G[i][j] = 0.0;
        const double aa[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], n}};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                G[i][j] = aa[i][j];
                G[3 + i][3 + j] = aa[i][j];
            }
            b[i] = g[5 + i];
            b[3 + i] = g[8 + i];
        }
        if constexpr (S == 4) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    G[i][6 + j] = g[11 + 2 * i + j];
                    G[6 + j][i] = g[11 + 2 * i + j];
                }
            }
            G[6][6] = g[23];
            G[6][7] = g[24];
            G[7][6] = g[24];
            G[7][7] = g[25];
            b[6] = g[26];
            b[7] = g[27];
        }
    }, hn);

    // H = T2^-1 Hn T1, then / H[8]
    double A[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[r][0] = hn[3 * r] * sq;
        A[r][1] = hn[3 * r + 1] * sq;
        A[r][2] = (hn[3 * r + 2] - A[r][0] * cx) - A[r][1] * cy;
    }
    bool ok = solved;
    if constexpr (S == 4) {
        double H[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            H[c] = A[0][c] / st + cu * A[2][c];
            H[3 + c] = A[1][c] / st + cv * A[2][c];
            H[6 + c] = A[2][c];
        }
        const double w = __builtin_fabs(H[8]);
        ok = ok && w >= kRansacMinPivot && w < kRefineInf;
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = H[k] / H[8];
    } else {
        out[0] = A[0][0] / st;
        out[1] = A[0][1] / st;
        out[2] = A[0][2] / st + cu;
        out[3] = A[1][0] / st;
        out[4] = A[1][1] / st;
        out[5] = A[1][2] / st + cv;
        out[6] = 0.0;
        out[7] = 0.0;
    }
    out[8] = 1.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok = ok && __builtin_fabs(out[k]) < kRefineInf;
    return ok;
}

// One workgroup per frame; all rounds inside it.  The correspondences are the compaction
// kernel's, in the stage's own scratch; the inlier bytes come from the original arrays as in the
// finalise kernel.
template <int S>
__global__ __launch_bounds__(kRansacFrameThreads) void refine_kernel(RefineParams R) {
    __shared__ double s_sum[kRefineSums<S>][kRansacFrameThreads];
    const RansacParams& P = R.r;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const IndexRange qr = frame_range(P.q_offs, P.q_cap, f);
    const IndexRange tr = frame_range(P.t_offs, P.t_cap, f);
    const uint32_t m = min(P.n_corr[f], (uint32_t)min(qr.hi - qr.lo, (uint64_t)kMatchMaxCap));
    const double* corr = P.corr + 4 * qr.lo;

    const double* in = R.models_in + 11 * (uint64_t)f;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = in[k];
    const uint2* in_tail = reinterpret_cast<const uint2*>(in + 9);
    const uint2 tail0 = in_tail[0], tail1 = in_tail[1];       // n_corr, n_inliers; hypothesis, n_valid
    __syncthreads();                                          // models_out may be models_in
    const bool have = tail1.x != kRansacInvalid;              // uniform

    uint32_t count = 0, rounds = 0;
    if (have) {
        double a[5];
        refine_score(h, corr, m, P.tt, s_sum, tid, a);
        count = (uint32_t)a[0];
        for (uint32_t r = 0; r < R.n_rounds; ++r) {
            double h2[9], a2[5];
            if (!refine_round<S>(h, a, corr, m, P.tt, s_sum, tid, h2)) break;
            refine_score(h2, corr, m, P.tt, s_sum, tid, a2);
            const uint32_t count2 = (uint32_t)a2[0];
            if (count2 < count) break;
#pragma unroll
            for (int k = 0; k < 9; ++k) h[k] = h2[k];
#pragma unroll
            for (int k = 0; k < 5; ++k) a[k] = a2[k];
            count = count2;
            ++rounds;
        }
    }
    if (tid == 0) {
        double* out = P.models + 11 * (uint64_t)f;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = h[k];
        uint2* tail = reinterpret_cast<uint2*>(out + 9);
        tail[0] = have ? make_uint2(m, count) : tail0;
        tail[1] = tail1;
        if (R.rounds) R.rounds[f] = rounds;
    }
    if (P.inliers) {
        for (uint64_t i = qr.lo + tid; i < qr.hi; i += kRansacFrameThreads) {
            Corr c{0.0, 0.0, 0.0, 0.0};
            const bool is = correspondence(P, i, tr, &c) && have &&
                            ransac_inlier(h, c.x, c.y, c.u, c.v, P.tt);
            P.inliers[i] = is ? 1u : 0u;
        }
    }
}

}  // namespace

hipError_t launch_ransac_compact(const RansacParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(ransac_compact_kernel, dim3(p.n_frames), dim3(kRansacFrameThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_refine(const RefineParams& p, hipStream_t stream) {
    const RansacParams& r = p.r;
    if (r.n_frames == 0) return hipSuccess;
    if (r.n_frames > 65535u || r.q_cap > kMatchMaxCap || r.t_cap > kMatchMaxCap ||
        r.model > kRansacHomography || r.coords > kRansacF32 || p.n_rounds > kRefineMaxRounds)
        return hipErrorInvalidValue;
    const dim3 frames(r.n_frames), block(kRansacFrameThreads);
    hipLaunchKernelGGL(ransac_compact_kernel, frames, block, 0, stream, r);
    if (r.model == kRansacAffine)
        hipLaunchKernelGGL(refine_kernel<3>, frames, block, 0, stream, p);
    else
        hipLaunchKernelGGL(refine_kernel<4>, frames, block, 0, stream, p);
    return hipGetLastError();
}

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
