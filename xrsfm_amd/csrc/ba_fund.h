// Batched fundamental-matrix verification of matched image pairs on the GPU: SolveFundamnetalCOLMAP ->
// colmap::LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator> (reference
// src/geometry/epipolar_geometry.hpp:10-27, called for every matched pair by FeatureMatching, src/feature/feature_processing.cc:
// 256-296).  The decisions and the sampler are in ba_fund_scan.h, the geometry in ba_fund_geom.h; this file spreads them over one
// 256-thread workgroup per pair.
//
// Matches stay in global memory (32 bytes each: x_a y_a x_b y_b, L2-resident).  The generator's state and the pair's index array
// live in LDS; thread 192 (wave 3, which has no model to score) draws the septuples of the NEXT block while (b) runs, into the
// other half of a double buffer.  Trials run in blocks of 64:
//   (a) lane = trial on wave 0: the 7-point solver of ba_fund_geom.h on a workspace of kWs7 doubles per trial in LDS, element-major
//       (double e of trial l at ws[64 e + l]): the lanes of the wave never share a bank and nothing dynamically indexed sits in
//       private memory; the models (up to 3 per trial, ascending root) go to LDS;
//   (b) thread = (trial, model slot), 192 of the 256: walks the n matches in index order and keeps the count and the residual sum,
//       so the sum is bit-identical to a sequential evaluation; no mask is kept per model;
//   (c) every thread runs the scan over the block's supports in (trial, ascending root) order from the same LDS data: the same
//       decisions, so control flow stays workgroup-uniform without a broadcast;
//   (d) the 8-point model is computed by the whole workgroup: threads over matches, every sum over the inliers reduced in a fixed
//       order (per-thread strided partials, wave butterfly, the four waves in order), the dense stage (9 x 9 Jacobi, 3 x 3 SVD) by
//       thread 0 on an LDS workspace;
//   (e) the block loop ends at the aborting trial.
// The inlier mask is computed once, from the final best model.  Every loop is bounded (kBisect, kPolish, sweep caps, trials <=
// 16384, matches <= 8192, at most kMaxRedraws rejected words per bounded draw of the sampler); nothing waits for another workgroup;
// no floating-point atomics; a pair's result depends on nothing but the pair.
#pragma once
#include "ba_fund_geom.h"

namespace xba {

constexpr int kFundThreads = 256;
constexpr int kFundBlock = 64;                 // trials per block
constexpr int kFundSlots = 3;                  // models per trial
constexpr int kFundSampler = 192;              // the thread that draws

struct FundPair {
    int32_t beg, n;            // matches beg .. beg + n
    int32_t dyn_off;           // row of dyn(k, n), k = 0 .. n
    int32_t skip_status;       // 0: attempted; 2 or 3: not
    uint32_t seed;
    int32_t pad;
    double max_residual;       // max_error^2
};

struct FundParams {
    int32_t trial_cap;         // min(max_num_trials, the bound from min_inlier_ratio)
    int32_t min_trials;
};

struct FundShared {
    double ws[kFundBlock * xfund::kWs7];
    double model[kFundBlock * kFundSlots * 9];
    double sum[kFundBlock * kFundSlots];
    double best[9];
    double part[4 * 48];
    xfund::Eight w8;
    int32_t cnt[kFundBlock * kFundSlots];
    int32_t nmodel[kFundBlock];
    int32_t tuples[2][kFundBlock * xfund::kSample];
    uint32_t mt[624];
    int32_t idx[xfund::kMaxMatches];
    int32_t ok;
    unsigned char inl[xfund::kMaxMatches];
};

struct FundLdsWs {
    double* p;                 // &ws[lane]
    __device__ __forceinline__ double& operator()(int e) const { return p[e * kFundBlock]; }
};

// every thread's acc[M] summed over the workgroup into w8.red[0..M) in a fixed order; ends with a barrier
template <int M>
__device__ __forceinline__ void fund_block_sum(FundShared& S, const double (&acc)[M]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < M; ++e) {
        double s = acc[e];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) S.part[wave * 48 + e] = s;
    }
    __syncthreads();
    if (threadIdx.x < M) S.w8.red[threadIdx.x] = ((S.part[threadIdx.x] + S.part[48 + threadIdx.x]) + S.part[96 + threadIdx.x]) + S.part[144 + threadIdx.x];
    __syncthreads();
}

// count and residual sum of model F over all matches, by the whole workgroup (fixed order); optionally the mask
__device__ __forceinline__ void fund_block_support(FundShared& S, const double* F, const double* __restrict__ m, int n, double max_res, bool write_inl,
                                                   int& count, double& sum) {
    double acc[2] = {0.0, 0.0};
    double Fm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Fm[k] = F[k];
    for (int k = threadIdx.x; k < n; k += kFundThreads) {
        const double r = xfund::sampson(Fm, m[4 * (size_t)k], m[4 * (size_t)k + 1], m[4 * (size_t)k + 2], m[4 * (size_t)k + 3]);
        const bool in = xfund::is_inlier(r, max_res);
        if (in) { acc[0] += 1.0; acc[1] += r; }
        if (write_inl) S.inl[k] = in ? 1 : 0;
    }
    fund_block_sum<2>(S, acc);
    count = (int)S.w8.red[0]; sum = S.w8.red[1];
    __syncthreads();               // (red is overwritten by the next sum)
}

// (d): FundamentalMatrixEightPointEstimator::Estimate on the inliers flagged in S.inl; the model goes to S.w8.F.  Returns whether
// there is one (workgroup-uniform).
__device__ __forceinline__ bool fund_local_model(FundShared& S, const double* __restrict__ m, int n) {
    xfund::Eight& w = S.w8;
    const int tid = threadIdx.x;
#define XBA_FUND_SUM(M, TERM)                                                                                                 \
    {                                                                                                                         \
        double acc[M];                                                                                                        \
        _Pragma("unroll") for (int e = 0; e < M; ++e) acc[e] = 0.0;                                                           \
        for (int k = tid; k < n; k += kFundThreads)                                                                           \
            if (S.inl[k]) {                                                                                                   \
                const double xa = m[4 * (size_t)k], ya = m[4 * (size_t)k + 1], xb = m[4 * (size_t)k + 2], yb = m[4 * (size_t)k + 3]; \
                TERM;                                                                                                         \
            }                                                                                                                 \
        fund_block_sum<M>(S, acc);                                                                                            \
    }
    XBA_FUND_SUM(5, xfund::eight_terms1(xa, ya, xb, yb, acc))
    if (tid == 0) xfund::eight_stage_centroid(w);
    __syncthreads();
    XBA_FUND_SUM(2, xfund::eight_terms2(w, xa, ya, xb, yb, acc))
    if (tid == 0) xfund::eight_stage_scale(w);
    __syncthreads();
    XBA_FUND_SUM(45, xfund::eight_terms3(w, xa, ya, xb, yb, acc))
    if (tid == 0) S.ok = xfund::eight_stage_model(w) ? 1 : 0;
    __syncthreads();
#undef XBA_FUND_SUM
    return S.ok != 0;
}

__global__ __launch_bounds__(kFundThreads) void k_verify_pairs(
        const FundPair* __restrict__ pairs, int n_pairs, FundParams prm, const double* __restrict__ m_all, const int32_t* __restrict__ dyn_tab,
        double* __restrict__ F_out, unsigned char* __restrict__ status, unsigned char* __restrict__ mask_out, int* __restrict__ num_inliers,
        int* __restrict__ num_trials, int* __restrict__ best_trial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fund_smem[];
    FundShared& S = *reinterpret_cast<FundShared*>(fund_smem);
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= n_pairs) return;
    const FundPair pr = pairs[f];
    const int n = pr.n;
    if (pr.skip_status != 0) {                              // fewer than min_matches or more than XRSFM_BA_FUND_MAX_MATCHES matches
        if (tid == 0) { status[f] = (unsigned char)pr.skip_status; num_inliers[f] = 0; num_trials[f] = 0; best_trial[f] = -1; }
        for (int k = tid; k < n; k += kFundThreads) mask_out[pr.beg + k] = 0;
        return;
    }
    const double* __restrict__ m = m_all + 4 * (size_t)pr.beg;
    xfund::Scan sc(dyn_tab + pr.dyn_off, prm.trial_cap, prm.min_trials);
    xfund::Sampler gen{S.mt, S.idx, 0, n};
    for (int k = tid; k < n; k += kFundThreads) S.idx[k] = k;
    __syncthreads();
    if (tid == kFundSampler) {
        gen.seed(pr.seed);
        const int cnt0 = min(kFundBlock, sc.max_trials);
        for (int l = 0; l < cnt0; ++l) gen.draw(&S.tuples[0][l * xfund::kSample]);
    }
    __syncthreads();
    int buf = 0;
#pragma unroll 1
    for (int t0 = 0; t0 < sc.max_trials; t0 += kFundBlock, buf ^= 1) {
        // (a)
        if (tid < kFundBlock) {
            int nm = 0;
            if (t0 + tid < sc.max_trials) {
                FundLdsWs ws;
                ws.p = S.ws + tid;
#pragma unroll 1
                for (int j = 0; j < xfund::kSample; ++j) {
                    const int i = S.tuples[buf][tid * xfund::kSample + j];
                    xfund::seven_point_row(ws, j, m[4 * (size_t)i], m[4 * (size_t)i + 1], m[4 * (size_t)i + 2], m[4 * (size_t)i + 3]);
                }
                nm = xfund::seven_point_models(ws, S.model + (size_t)tid * (kFundSlots * 9));
            }
            S.nmodel[tid] = nm;
        }
        __syncthreads();
        // (b), and the next block's septuples
        if (tid < kFundBlock * kFundSlots) {
            const int l = tid / kFundSlots, slot = tid - l * kFundSlots;
            int cnt = 0;
            double sum = 0.0;
            if (slot < S.nmodel[l]) {
                double F[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) F[k] = S.model[(size_t)l * (kFundSlots * 9) + slot * 9 + k];
#pragma unroll 1
                for (int k = 0; k < n; ++k) {
                    const double r = xfund::sampson(F, m[4 * (size_t)k], m[4 * (size_t)k + 1], m[4 * (size_t)k + 2], m[4 * (size_t)k + 3]);
                    if (xfund::is_inlier(r, pr.max_residual)) { ++cnt; sum += r; }
                }
            }
            S.cnt[tid] = cnt; S.sum[tid] = sum;
        } else if (tid == kFundSampler) {
            const int cnt1 = min(kFundBlock, sc.max_trials - (t0 + kFundBlock));
            for (int l = 0; l < cnt1; ++l) gen.draw(&S.tuples[buf ^ 1][l * xfund::kSample]);
        }
        __syncthreads();
        // (c)
        const int live = min(kFundBlock, sc.max_trials - t0);
        for (int l = 0; l < live && !sc.abort; ++l) {
            const int nm = S.nmodel[l];
            for (int slot = 0; slot < nm; ++slot) {
                const xfund::Offer o = sc.offer(t0 + l, S.cnt[kFundSlots * l + slot], S.sum[kFundSlots * l + slot]);
                if (o != xfund::kIgnored) {
                    __syncthreads();
                    if (tid < 9) S.best[tid] = S.model[(size_t)l * (kFundSlots * 9) + slot * 9 + tid];
                    __syncthreads();
                    if (o == xfund::kNewBestLocal) {
                        // (d) the inliers of the sample model, the 8-point model and its support
                        int sc0 = 0;
                        double ss0 = 0.0;
                        fund_block_support(S, S.best, m, n, pr.max_residual, true, sc0, ss0);
                        if (fund_local_model(S, m, n)) {
                            int lc = 0;
                            double ls = 0.0;
                            fund_block_support(S, S.w8.F, m, n, pr.max_residual, false, lc, ls);
                            if (sc.offer_local(lc, ls)) {
                                if (tid < 9) S.best[tid] = S.w8.F[tid];
                                __syncthreads();
                            }
                        }
                    }
                }
                if (sc.after_model(t0 + l)) break;
            }
        }
        __syncthreads();                 // the next block overwrites the models and supports
        if (sc.abort) break;             // (e)
    }
    // the mask of the final best model; success needs seven inliers and a finite model
    bool ok = sc.finish();
    int fc = 0;
    double fs = 0.0;
    if (ok) {
        fund_block_support(S, S.best, m, n, pr.max_residual, true, fc, fs);
        if (tid == 0) {
            xfund::normalise_model(S.best, S.w8.F);
            S.ok = xpnp::all_finite(S.w8.F, 9) ? 1 : 0;
        }
        __syncthreads();
        ok = S.ok != 0;
    }
    for (int k = tid; k < n; k += kFundThreads) mask_out[pr.beg + k] = ok ? S.inl[k] : 0;
    if (ok && tid < 9) F_out[9 * (size_t)f + tid] = S.w8.F[tid];
    if (tid == 0) {
        status[f] = ok ? 1 : 0;
        num_inliers[f] = ok ? fc : 0;
        num_trials[f] = ok ? sc.num_trials : 0;
        best_trial[f] = ok ? sc.best_trial_code() : -1;
    }
}

}  // namespace xba
