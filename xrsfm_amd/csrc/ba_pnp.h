// Batched absolute pose of frames from 2D-3D correspondences on the GPU: the "pose estimate [init]" of RegisterImage, that is
// SolvePnP_colmap -> colmap::LORANSAC<P3PEstimator, EPNPEstimator> (reference src/geometry/pnp.cc:29-36, 253-316).  The decisions
// are in ba_pnp_scan.h, the geometry in ba_pnp_geom.h; this file spreads them over one 256-thread workgroup per frame.
//
// Correspondences stay in global memory (40 bytes each, L2-resident).  Trials run in blocks of 64:
//   (a) lane = trial on wave 0: the P3P coefficients, the quartic's roots and up to four rigid fits; the models (12 doubles each,
//       ascending root) go to LDS;
//   (b) thread = (trial, root slot): walks the n correspondences in index order and keeps the count and the residual sum, so the
//       sum is bit-identical to a sequential evaluation; no mask is kept per model;
//   (c) every thread runs the scan over the block's supports in (trial, ascending root) order: the same LDS data, the same
//       decisions, so control flow stays workgroup-uniform without a broadcast;
//   (d) a local optimisation is done by the whole workgroup: threads over correspondences, every sum of ba_pnp_geom.h's stages
//       reduced in a fixed order (per-thread strided partials, wave butterfly, the four waves in order), the dense stages (Jacobi
//       eigen-decompositions, least-squares solves) by thread 0 on an LDS workspace;
//   (e) the block loop ends at the aborting trial.
// The inlier mask is computed once, from the final best model.  Every loop is bounded (root-finder cap, sweep caps, trials <=
// 16384); nothing waits for another workgroup; no floating-point atomics; a frame's result depends on nothing but the frame.
#pragma once
#include "ba_pnp_geom.h"

namespace xba {

constexpr int kPnpThreads = 256;
constexpr int kPnpBlock = 64;                  // trials per block

struct PnpFrame {
    int32_t beg, n;            // correspondences beg .. beg + n
    int32_t tri_off;           // first triple of the frame in the triples array (in triples), -1: not attempted
    int32_t dyn_off;           // row of dyn(k, n), k = 0 .. n
    double max_residual;       // max_error^2
};

struct PnpParams {
    int32_t trial_cap;         // min(max_num_trials, the bound from min_inlier_ratio)
    int32_t min_trials;
};

struct PnpShared {
    double model[kPnpBlock * 4 * 12];
    double sum[kPnpThreads];
    int32_t cnt[kPnpThreads];
    int32_t nmodel[kPnpBlock];
    double best[12], local[12];
    double part[4 * 40];
    xpnp::Epnp ws;
    int32_t first;
    int32_t ok;
    unsigned char inl[xpnp::kMaxCorr];
};

// every thread's acc[M] summed over the workgroup into ws.red[0..M) in a fixed order; ends with a barrier
template <int M>
__device__ __forceinline__ void pnp_block_sum(PnpShared& S, const double (&acc)[M]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < M; ++e) {
        double s = acc[e];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) S.part[wave * 40 + e] = s;
    }
    __syncthreads();
    if (threadIdx.x < M) S.ws.red[threadIdx.x] = ((S.part[threadIdx.x] + S.part[40 + threadIdx.x]) + S.part[80 + threadIdx.x]) + S.part[120 + threadIdx.x];
    __syncthreads();
}

// count and residual sum of model P over all correspondences, by the whole workgroup (fixed order); optionally the mask
__device__ __forceinline__ void pnp_block_support(PnpShared& S, const double* P, const double* __restrict__ xy, const double* __restrict__ X3,
                                                  int n, double max_res, bool write_inl, int& count, double& sum) {
    double acc[2] = {0.0, 0.0};
    double Pm[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Pm[k] = P[k];
    for (int k = threadIdx.x; k < n; k += kPnpThreads) {
        const double r = xpnp::residual(Pm, X3 + 3 * (size_t)k, xy[2 * (size_t)k], xy[2 * (size_t)k + 1]);
        const bool in = r <= max_res;
        if (in) { acc[0] += 1.0; acc[1] += r; }
        if (write_inl) S.inl[k] = in ? 1 : 0;
    }
    pnp_block_sum<2>(S, acc);
    count = (int)S.ws.red[0]; sum = S.ws.red[1];
    __syncthreads();               // (red is overwritten by the next sum)
}

// (d): EPNPEstimator::Estimate on the inliers flagged in S.inl (S.ws.n of them, the first at S.first); the model goes to S.local.
// Returns whether there is one (workgroup-uniform).
__device__ __forceinline__ bool pnp_local_model(PnpShared& S, const double* __restrict__ xy, const double* __restrict__ X3, int n) {
    xpnp::Epnp& w = S.ws;
    const int tid = threadIdx.x;
#define XBA_PNP_SUM(M, TERM)                                                                                                  \
    {                                                                                                                         \
        double acc[M];                                                                                                        \
        _Pragma("unroll") for (int e = 0; e < M; ++e) acc[e] = 0.0;                                                           \
        for (int k = tid; k < n; k += kPnpThreads)                                                                            \
            if (S.inl[k]) {                                                                                                   \
                const double* X = X3 + 3 * (size_t)k;                                                                         \
                const double x = xy[2 * (size_t)k], y = xy[2 * (size_t)k + 1];                                                \
                (void)x; (void)y;                                                                                             \
                TERM;                                                                                                         \
            }                                                                                                                 \
        pnp_block_sum<M>(S, acc);                                                                                             \
    }
    XBA_PNP_SUM(4, (acc[0] += X[0], acc[1] += X[1], acc[2] += X[2], acc[3] += 1.0))
    if (tid == 0) xpnp::epnp_stage_centroid(w);
    __syncthreads();
    XBA_PNP_SUM(6, xpnp::epnp_terms1(w, X, acc))
    if (tid == 0) S.ok = xpnp::epnp_stage_control(w) ? 1 : 0;
    __syncthreads();
    if (!S.ok) return false;
    XBA_PNP_SUM(40, xpnp::epnp_terms2(w, X, x, y, acc))
    if (tid == 0) xpnp::epnp_stage_solve(w, X3 + 3 * (size_t)min(S.first, n - 1));
    __syncthreads();
    XBA_PNP_SUM(9, xpnp::epnp_terms3(w, X, acc))
    if (tid == 0) xpnp::epnp_stage_means(w);
    __syncthreads();
    XBA_PNP_SUM(27, xpnp::epnp_terms4(w, X, acc))
    if (tid == 0) xpnp::epnp_stage_rt(w);
    __syncthreads();
    XBA_PNP_SUM(3, xpnp::epnp_terms5(w, X, x, y, acc))
    if (tid == 0) S.ok = xpnp::epnp_stage_pick(w, S.local) ? 1 : 0;
    __syncthreads();
#undef XBA_PNP_SUM
    return S.ok != 0;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_frames(
        const PnpFrame* __restrict__ frames, int n_frames, PnpParams prm, const double* __restrict__ xy_all, const double* __restrict__ X_all,
        const int32_t* __restrict__ triples, const int32_t* __restrict__ dyn_tab, double* __restrict__ q_out, double* __restrict__ t_out,
        unsigned char* __restrict__ status, unsigned char* __restrict__ mask_out, int* __restrict__ num_inliers, int* __restrict__ num_trials,
        int* __restrict__ best_trial) {
    __shared__ PnpShared S;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= n_frames) return;
    const PnpFrame fr = frames[f];
    const int n = fr.n;
    if (fr.tri_off < 0) {                                   // fewer than 3 or more than XRSFM_BA_POSE_MAX_CORR correspondences
        if (tid == 0) { status[f] = n < 3 ? 2 : 3; num_inliers[f] = 0; num_trials[f] = 0; best_trial[f] = -1; }
        for (int k = tid; k < n; k += kPnpThreads) mask_out[fr.beg + k] = 0;
        return;
    }
    const double* __restrict__ xy = xy_all + 2 * (size_t)fr.beg;
    const double* __restrict__ X3 = X_all + 3 * (size_t)fr.beg;
    const int32_t* __restrict__ tri = triples + 3 * (size_t)fr.tri_off;
    xpnp::Scan sc(dyn_tab + fr.dyn_off, prm.trial_cap, prm.min_trials);
#pragma unroll 1
    for (int t0 = 0; t0 < sc.max_trials; t0 += kPnpBlock) {
        // (a)
        if (tid < kPnpBlock) {
            int nm = 0;
            if (t0 + tid < sc.max_trials) {
                double sxy[6], sX[9];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int i = tri[3 * (size_t)(t0 + tid) + k];
                    sxy[2 * k] = xy[2 * (size_t)i]; sxy[2 * k + 1] = xy[2 * (size_t)i + 1];
                    sX[3 * k] = X3[3 * (size_t)i]; sX[3 * k + 1] = X3[3 * (size_t)i + 1]; sX[3 * k + 2] = X3[3 * (size_t)i + 2];
                }
                nm = xpnp::p3p_models(sxy, sX, S.model + (size_t)tid * 48);
            }
            S.nmodel[tid] = nm;
        }
        __syncthreads();
        // (b)
        {
            const int l = tid >> 2, slot = tid & 3;
            int cnt = 0;
            double sum = 0.0;
            if (slot < S.nmodel[l]) {
                double P[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) P[k] = S.model[(size_t)l * 48 + slot * 12 + k];
#pragma unroll 1
                for (int k = 0; k < n; ++k) {
                    const double r = xpnp::residual(P, X3 + 3 * (size_t)k, xy[2 * (size_t)k], xy[2 * (size_t)k + 1]);
                    if (r <= fr.max_residual) { ++cnt; sum += r; }
                }
            }
            S.cnt[tid] = cnt; S.sum[tid] = sum;
        }
        __syncthreads();
        // (c)
        const int live = min(kPnpBlock, sc.max_trials - t0);
        for (int l = 0; l < live && !sc.abort; ++l) {
            const int nm = S.nmodel[l];
            for (int slot = 0; slot < nm; ++slot) {
                const xpnp::Offer o = sc.offer(t0 + l, S.cnt[4 * l + slot], S.sum[4 * l + slot]);
                if (o != xpnp::kIgnored) {
                    __syncthreads();
                    if (tid < 12) S.best[tid] = S.model[(size_t)l * 48 + slot * 12 + tid];
                    if (tid == 0) S.first = n;
                    __syncthreads();
                    if (o == xpnp::kNewBestLocal) {
                        // (d) the inliers of the sample model, the first of them, the local model and its support
                        double Pm[12];
#pragma unroll
                        for (int k = 0; k < 12; ++k) Pm[k] = S.best[k];
                        for (int k = tid; k < n; k += kPnpThreads) {
                            const bool in = xpnp::residual(Pm, X3 + 3 * (size_t)k, xy[2 * (size_t)k], xy[2 * (size_t)k + 1]) <= fr.max_residual;
                            S.inl[k] = in ? 1 : 0;
                            if (in) atomicMin(&S.first, k);
                        }
                        __syncthreads();
                        if (pnp_local_model(S, xy, X3, n)) {
                            int lc = 0;
                            double ls = 0.0;
                            pnp_block_support(S, S.local, xy, X3, n, fr.max_residual, false, lc, ls);
                            if (sc.offer_local(lc, ls)) {
                                if (tid < 12) S.best[tid] = S.local[tid];
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
    // the mask of the final best model; success needs three inliers and a finite pose
    bool ok = sc.finish();
    int fc = 0;
    double fs = 0.0;
    if (ok) {
        pnp_block_support(S, S.best, xy, X3, n, fr.max_residual, true, fc, fs);
        ok = xpnp::all_finite(S.best, 12);
    }
    for (int k = tid; k < n; k += kPnpThreads) mask_out[fr.beg + k] = ok ? S.inl[k] : 0;
    if (tid == 0) {
        status[f] = ok ? 1 : 0;
        if (ok) {
            double q[4];
            xpnp::quat_from_pose(S.best, q);
            q_out[4 * (size_t)f] = q[0]; q_out[4 * (size_t)f + 1] = q[1]; q_out[4 * (size_t)f + 2] = q[2]; q_out[4 * (size_t)f + 3] = q[3];
            t_out[3 * (size_t)f] = S.best[3]; t_out[3 * (size_t)f + 1] = S.best[7]; t_out[3 * (size_t)f + 2] = S.best[11];
        }
        num_inliers[f] = ok ? fc : 0;
        num_trials[f] = ok ? sc.num_trials : 0;
        best_trial[f] = ok ? sc.best_trial_code() : -1;
    }
}

}  // namespace xba
