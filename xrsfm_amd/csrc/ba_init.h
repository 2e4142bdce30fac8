// Batched two-view initialisation on the GPU: what CheckInitFramePair / InitializeMap compute for one candidate pair (reference
// src/geometry/map_initializer.cc:13-65, 141-206; essential.cc:283-487), for all pairs of a call in one launch.  The decisions
// are in ba_init_scan.h, the geometry in ba_init_geom.h; this file spreads them over one 256-thread workgroup per pair.
//
// Matches stay in global memory (32 bytes each: x1 y1 x2 y2).  At most 64 trials per pair, in sub-blocks of 32:
//   (a) eight lanes of each of the four waves take one trial each: the 5-point solver of ba_init_geom.h on a workspace of
//       kWsDoubles doubles per trial in LDS, element-major (double e of trial l at ws[32 e + l]), so that the lanes of a wave
//       never share a bank and nothing dynamically indexed sits in private memory.  32 x 316 doubles are 79 KiB; all 64 trials
//       at once would need 158 KiB and leave no room for the supports (the CU has 160 KiB), so the trials run in two sub-blocks
//       and are spread over the four waves, which keeps all four SIMDs busy.  The models (up to 10 per trial, 9 doubles each)
//       go to a per-pair block in global memory;
//   (b) thread = (trial, model slot), 320 per sub-block in two rounds: walks the n matches in index order and keeps count and
//       score, bit-identical to a sequential evaluation;
//   (c) every thread runs the scan over the sub-block's supports from the same LDS data: workgroup-uniform control flow; the
//       sub-block loop ends when the trial bound has dropped below its first trial;
//   (d) the best E: threads over matches write the essential inlier mask; thread 0 normalises and decomposes E; one pass over
//       the matches keeps the four check_point results as four bits per match and four integer counters (integer atomics on
//       LDS: order-free); the winning candidate's points, mask and angle counts are written in a second pass.
// Every loop is bounded (kNullSweeps, kQrItersPerValue per eigenvalue, kSvd3Sweeps, kDltSweeps, trials <= 64, matches <= 8192);
// nothing waits for another workgroup; no floating-point atomics; a pair's result depends on nothing but the pair.
#pragma once
#include "ba_init_geom.h"

namespace xba {

constexpr int kInitThreads = 256;
constexpr int kInitSub = 32;                   // trials per sub-block
constexpr int kInitLanesPerWave = kInitSub / 4;
constexpr int kInitSupports = kInitSub * xinit::kMaxModels;

struct InitPair {
    int32_t beg, n;            // matches beg .. beg + n
    int32_t quint_off;         // first quintuple of the pair (in quintuples), -1: not attempted
    int32_t row_off;           // row of the trial bound, k = 0 .. n
    int32_t skip_status;       // 2 or 3 when not attempted
    int32_t pad;
    double th2;                // 2 th^2
};

struct InitParams {
    double max_depth, min_front_ratio, min_angle_ratio;
    double min_angle[4];
    int32_t max_iterations, n_angles, min_num_valid;
};

struct InitShared {
    double ws[kInitSub * xinit::kWsDoubles];
    double score[kInitSupports];
    int32_t cnt[kInitSupports];
    int32_t nmodel[kInitSub];
    double E[9], En[9], R1[9], R2[9], T[3];
    int32_t front[4], valid[4];
    int32_t ok;
    unsigned char flags[xinit::kMaxMatches];
};

struct InitLdsWs {
    double* p;                 // &ws[lane]
    __device__ __forceinline__ double& operator()(int e) const { return p[e * kInitSub]; }
};

__global__ __launch_bounds__(kInitThreads) void k_init_pairs(
        const InitPair* __restrict__ pairs, int n_pairs, InitParams prm, const double* __restrict__ m_all, const int32_t* __restrict__ quintuples,
        const int32_t* __restrict__ rows, double* __restrict__ models_all, unsigned char* __restrict__ status, double* __restrict__ E_out,
        double* __restrict__ q_out, double* __restrict__ t_out, double* __restrict__ points, unsigned char* __restrict__ ess_mask,
        unsigned char* __restrict__ front_mask, int* __restrict__ counts, unsigned char* __restrict__ accepted, int* __restrict__ num_trials,
        int* __restrict__ best_trial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char init_smem[];
    InitShared& S = *reinterpret_cast<InitShared*>(init_smem);
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= n_pairs) return;
    const InitPair pr = pairs[f];
    const int n = pr.n;
    if (tid < 8) counts[8 * (size_t)f + tid] = 0;
    for (int k = tid; k < n; k += kInitThreads) { ess_mask[pr.beg + k] = 0; front_mask[pr.beg + k] = 0; }
    if (pr.quint_off < 0) {
        if (tid == 0) { status[f] = (unsigned char)pr.skip_status; accepted[f] = 0; num_trials[f] = 0; best_trial[f] = -1; }
        return;
    }
    const double* __restrict__ m = m_all + 4 * (size_t)pr.beg;
    const int32_t* __restrict__ quint = quintuples + 5 * (size_t)pr.quint_off;
    double* __restrict__ models = models_all + (size_t)f * (xinit::kMaxTrials * xinit::kMaxModels * 9);
    xinit::Scan sc(rows + pr.row_off, prm.max_iterations);
    int executed = 0;
#pragma unroll 1
    for (int t0 = 0; t0 < prm.max_iterations && sc.more(t0); t0 += kInitSub) {
        // (a)
        {
            const int wl = tid & 63, l = (tid >> 6) * kInitLanesPerWave + wl;
            if (wl < kInitLanesPerWave) {
                int nm = 0;
                if (t0 + l < prm.max_iterations) {
                    double pts[20];
#pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        const int i = quint[5 * (size_t)(t0 + l) + k];
#pragma unroll
                        for (int e = 0; e < 4; ++e) pts[4 * k + e] = m[4 * (size_t)i + e];
                    }
                    InitLdsWs ws;
                    ws.p = S.ws + l;
                    nm = xinit::five_point_models(ws, pts, models + (size_t)(t0 + l) * (xinit::kMaxModels * 9));
                }
                S.nmodel[l] = nm;
            }
        }
        __threadfence_block();
        __syncthreads();
        // (b)
#pragma unroll 1
        for (int idx = tid; idx < kInitSupports; idx += kInitThreads) {
            const int l = idx / xinit::kMaxModels, slot = idx - l * xinit::kMaxModels;
            xinit::Support sp;
            if (slot < S.nmodel[l]) {
                double E[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) E[e] = models[(size_t)(t0 + l) * (xinit::kMaxModels * 9) + 9 * slot + e];
#pragma unroll 1
                for (int k = 0; k < n; ++k)
                    sp.add(xinit::sampson(E, m[4 * (size_t)k], m[4 * (size_t)k + 1], m[4 * (size_t)k + 2], m[4 * (size_t)k + 3]), pr.th2);
            }
            S.cnt[idx] = sp.count; S.score[idx] = sp.score;
        }
        __syncthreads();
        // (c)
        const int live = min(kInitSub, prm.max_iterations - t0);
        for (int l = 0; l < live && sc.more(t0 + l); ++l) {
            const int nm = S.nmodel[l];
            for (int slot = 0; slot < nm; ++slot) sc.offer(t0 + l, slot, S.cnt[l * xinit::kMaxModels + slot], S.score[l * xinit::kMaxModels + slot]);
            executed = t0 + l + 1;
        }
        __syncthreads();                 // the next sub-block overwrites the supports
    }
    // (d)
    const bool have = sc.best_code >= 0;
    if (tid == 0) {
        S.ok = 0;
        for (int k = 0; k < 4; ++k) { S.front[k] = 0; S.valid[k] = 0; }
        if (have) {
            const int bt = sc.best_code / xinit::kSlotStride, bs = sc.best_code % xinit::kSlotStride;
            double nn = 0.0;
            for (int e = 0; e < 9; ++e) { S.E[e] = models[(size_t)bt * (xinit::kMaxModels * 9) + 9 * bs + e]; nn += S.E[e] * S.E[e]; }
            const double inv = 1.0 / sqrt(nn);
            for (int e = 0; e < 9; ++e) S.En[e] = S.E[e] * inv;
            xinit::decompose_essential(S.En, S.R1, S.R2, S.T);
            S.ok = (xinit::finite9(S.En) && xinit::finite9(S.R1) && xinit::finite9(S.R2)) ? 1 : 0;
        }
        num_trials[f] = executed;
        best_trial[f] = sc.best_code;
    }
    __syncthreads();
    if (!S.ok) {                                            // best_E stayed NaN (or has no finite decomposition): no E is returned
        if (tid < 9) E_out[9 * (size_t)f + tid] = 0.0;
        if (tid == 0) { status[f] = 0; accepted[f] = 0; }
        return;
    }
    {
        double E[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) E[e] = S.E[e];
        int c4[4] = {0, 0, 0, 0};
        for (int k = tid; k < n; k += kInitThreads) {
            const double x1 = m[4 * (size_t)k], y1 = m[4 * (size_t)k + 1], x2 = m[4 * (size_t)k + 2], y2 = m[4 * (size_t)k + 3];
            ess_mask[pr.beg + k] = xinit::sampson(E, x1, y1, x2, y2) < pr.th2 ? 1 : 0;
            unsigned fl = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double R[9], t[3], ctr[3], p[3];
                xinit::candidate(S.R1, S.R2, S.T, c, R, t, ctr);
                if (xinit::check_point(R, t, x1, y1, x2, y2, prm.max_depth, p)) { fl |= 1u << c; ++c4[c]; }
            }
            S.flags[k] = (unsigned char)fl;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c4[c]) atomicAdd(&S.front[c], c4[c]);
    }
    __syncthreads();
    int best_k = 0, best_num = 0;
    for (int c = 0; c < 4; ++c)
        if (S.front[c] > best_num) { best_num = S.front[c]; best_k = c; }
    if (tid < 9) E_out[9 * (size_t)f + tid] = S.En[tid];
    if (tid == 0) counts[8 * (size_t)f] = sc.best_count;
    if (best_num == 0) {                                    // no candidate with a point in front
        if (tid == 0) { status[f] = 0; accepted[f] = 0; }
        return;
    }
    double R[9], t[3], ctr[3];
    xinit::candidate(S.R1, S.R2, S.T, best_k, R, t, ctr);
    const double zero[3] = {0.0, 0.0, 0.0};
    int v4[4] = {0, 0, 0, 0};
    for (int k = tid; k < n; k += kInitThreads) {
        if (!((S.flags[k] >> best_k) & 1)) continue;
        double p[3];
        xinit::check_point(R, t, m[4 * (size_t)k], m[4 * (size_t)k + 1], m[4 * (size_t)k + 2], m[4 * (size_t)k + 3], prm.max_depth, p);
        front_mask[pr.beg + k] = 1;
        points[3 * (size_t)(pr.beg + k)] = p[0]; points[3 * (size_t)(pr.beg + k) + 1] = p[1]; points[3 * (size_t)(pr.beg + k) + 2] = p[2];
        const double ang = xinit::tri_angle(zero, ctr, p);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (a < prm.n_angles && ang > prm.min_angle[a]) ++v4[a];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (v4[a]) atomicAdd(&S.valid[a], v4[a]);
    __syncthreads();
    if (tid == 0) {
        double q[4];
        xinit::quat_of(R, q);
        for (int k = 0; k < 4; ++k) q_out[4 * (size_t)f + k] = q[k];
        for (int k = 0; k < 3; ++k) t_out[3 * (size_t)f + k] = t[k];
        counts[8 * (size_t)f + 1] = best_num; counts[8 * (size_t)f + 2] = best_k;
        unsigned acc = 0;
        for (int a = 0; a < 4; ++a) {
            counts[8 * (size_t)f + 4 + a] = S.valid[a];
            if (a < prm.n_angles && xinit::accept(n, best_num, S.valid[a], prm.min_front_ratio, prm.min_angle_ratio, prm.min_num_valid)) acc |= 1u << a;
        }
        accepted[f] = (unsigned char)acc;
        status[f] = 1;
    }
}

}  // namespace xba
