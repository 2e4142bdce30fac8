// Batched robust triangulation of new tracks on the GPU: the creation of a 3-D point from the observations of an untriangulated
// key point.  Restates colmap::EstimateTriangulation as CreatePoint3d1 calls it
// (/root/reference/src/geometry/track_processor.cc:109-161; estimators/triangulation.cc:67-144; base/triangulation.cc:40-90,124-147):
// a LO-RANSAC over the pairs of observations in lexicographic order (CombinationSampler: deterministic), two-view DLT per pair,
// squared angular residuals, multi-view refit of the inliers of every new best.  The decisions are in ba_tri_scan.h.
//
// One wave per track, four tracks per workgroup.  A track's observations sit in the wave's own part of LDS as {P (3x4, row-major),
// projection centre, normalised xy}: 136 bytes each, 17 KiB per wave.  Trials run in blocks of 64:
//   (a) lane l unranks pair t0 + l, forms the 4x4 DLT in registers and takes its null vector by a one-sided (Hestenes) Jacobi SVD
//       with a fixed cap of sweeps, then tests the two depths and the triangulation angle;
//   (b) every lane walks the observations in LDS (one address per step: a broadcast) and accumulates count, residual sum and the
//       128-bit inlier mask of its model, in observation order;
//   (c) a wave-uniform loop over the lanes that have a model, in trial order, feeds xtri::Scan;
//   (d) a refit is done by the whole wave: lane = observation (two per lane above 64), butterfly sum of the 10 entries of the 4x4
//       normal matrix, the same two-sided Jacobi eigen-decomposition on every lane, depth test by ballot, "any pair of inlier
//       centres with enough angle" by lanes over pairs, support by lanes over observations;
//   (e) the block loop ends at the trial the scan aborts on.
// Every loop is bounded (sweep caps, trials <= min(cap, 8128)); no wave waits for another; no floating-point atomics; a track's
// result depends on nothing but the track.
#pragma once
#include "ba_filter.h"
#include "ba_tri_scan.h"

namespace xba {

constexpr int kTriWave = 64;
constexpr int kTriWaves = 4;                   // tracks per workgroup
constexpr int kTriRec = 17;                    // doubles per observation in LDS: P 0..11, centre 12..14, xy 15..16
constexpr int kTriSvdSweeps = 12;              // cyclic sweeps of 6 rotations; a 4x4 converges in 5 to 7
constexpr int kTriEigSweeps = 12;
constexpr double kTriRotTol = 1e-15;           // a pair of columns counts as orthogonal below this cosine
constexpr double kTriDepthMin = 2.220446049250313e-16;   // DBL_EPSILON (HasPointPositiveDepth)

// -DXBA_TRI_PHASES (build variant "tri_phases", tools/triangulate_timing.py): every wave adds the clock ticks it spent in the blocks
// (a), (b), (c) and (d) to phase[0..3] with integer atomics.  Timing only; the default build compiles none of it.
#ifdef XBA_TRI_PHASES
#define XBA_TRI_TICK() ((long long)wall_clock64())
#else
#define XBA_TRI_TICK() 0ll
#endif

struct TriParams {
    double min_angle;        // min_tri_angle_rad
    double max_residual;     // max_error_rad^2
    int32_t trial_cap;       // min(max_num_trials, the bound from min_inlier_ratio)
    int32_t exhaustive_threshold;
};

// Null vector of a 4x4 (row-major) by one-sided Jacobi: columns are rotated until they are mutually orthogonal, A V = U S; the
// column of V that belongs to the shortest column of A V is the right singular vector of the smallest singular value.
// Constant indices only, so a and v live in registers.
__device__ __forceinline__ void tri_null_svd(double a[16], double x[4]) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kTriSvdSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) { al += a[4 * r + p] * a[4 * r + p]; be += a[4 * r + q] * a[4 * r + q]; ga += a[4 * r + p] * a[4 * r + q]; }
                if (fabs(ga) > kTriRotTol * sqrt(al * be)) {
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ap = a[4 * r + p], aq = a[4 * r + q], vp = v[4 * r + p], vq = v[4 * r + q];
                        a[4 * r + p] = c * ap - s * aq; a[4 * r + q] = s * ap + c * aq;
                        v[4 * r + p] = c * vp - s * vq; v[4 * r + q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!__any(rotated)) break;
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double nn = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) nn += a[4 * r + c] * a[4 * r + c];
        if (c == 0 || nn < best) {
            best = nn;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = v[4 * r + c];
        }
    }
}

// Eigenvector of the smallest eigenvalue of a symmetric positive semi-definite 4x4 (full storage) by cyclic two-sided Jacobi.
__device__ __forceinline__ void tri_min_eigvec(double m[16], double x[4]) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    const double floor_abs = 1e-18 * (m[0] + m[5] + m[10] + m[15]);
#pragma unroll 1
    for (int sweep = 0; sweep < kTriEigSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double mpq = m[4 * p + q], mpp = m[4 * p + p], mqq = m[4 * q + q];
                if (fabs(mpq) > kTriRotTol * sqrt(fabs(mpp * mqq)) + floor_abs) {
                    rotated = true;
                    const double theta = (mqq - mpp) / (2.0 * mpq);
                    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {                 // M J and V J
                        const double mp = m[4 * r + p], mq = m[4 * r + q], vp = v[4 * r + p], vq = v[4 * r + q];
                        m[4 * r + p] = c * mp - s * mq; m[4 * r + q] = s * mp + c * mq;
                        v[4 * r + p] = c * vp - s * vq; v[4 * r + q] = s * vp + c * vq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {                 // J^T (M J)
                        const double mp = m[4 * p + k], mq = m[4 * q + k];
                        m[4 * p + k] = c * mp - s * mq; m[4 * q + k] = s * mp + c * mq;
                    }
                    m[4 * p + q] = 0.0; m[4 * q + p] = 0.0;
                }
            }
        }
        if (!__any(rotated)) break;
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c == 0 || m[5 * c] < best) {
            best = m[5 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = v[4 * r + c];
        }
    }
}

// acos(r1^ . r2^)^2 with r1 = (x, y, 1) and r2 = P (X, 1); no depth test and no clamp of the cosine, like the reference: a cosine
// rounded above 1 gives NaN, which is no inlier
__device__ __forceinline__ double tri_residual(const double* __restrict__ o, const double X[3]) {
    const double rx = o[0] * X[0] + o[1] * X[1] + o[2] * X[2] + o[3];
    const double ry = o[4] * X[0] + o[5] * X[1] + o[6] * X[2] + o[7];
    const double rz = o[8] * X[0] + o[9] * X[1] + o[10] * X[2] + o[11];
    const double x = o[15], y = o[16];
    const double i1 = 1.0 / sqrt(x * x + y * y + 1.0), i2 = 1.0 / sqrt(rx * rx + ry * ry + rz * rz);
    const double ang = acos((x * i1) * (rx * i2) + (y * i1) * (ry * i2) + i1 * (rz * i2));
    return ang * ang;
}

__device__ __forceinline__ double tri_depth(const double* __restrict__ o, const double X[3]) {
    return o[8] * X[0] + o[9] * X[1] + o[10] * X[2] + o[11];
}

__device__ __forceinline__ double tri_wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kTriWave);     // every lane ends with the same bits
    return s;
}

// (d): the multi-view estimator on the observations of mask (m0: 0..63, m1: 64..127), by the whole wave.  Returns whether the
// refit has a model; X, its support (cnt, sum) and its own inlier mask (r0, r1) are then valid on every lane.
__device__ __forceinline__ bool tri_refit(const double* __restrict__ so, int n, int lane, unsigned long long m0, unsigned long long m1,
                                          const TriParams& prm, double X[3], int& cnt, double& sum, unsigned long long& r0,
                                          unsigned long long& r1) {
    const int k0 = lane, k1 = lane + 64;
    const bool in0 = (m0 >> lane) & 1ull, in1 = (m1 >> lane) & 1ull;       // (bits at or above n are never set)
    double acc[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) acc[e] = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h ? in1 : in0) {
            const double* o = so + (h ? k1 : k0) * kTriRec;
            const double x = o[15], y = o[16], inv = 1.0 / sqrt(x * x + y * y + 1.0);
            const double p[3] = {x * inv, y * inv, inv};
            double T[12];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double w = p[0] * o[c] + p[1] * o[4 + c] + p[2] * o[8 + c];
#pragma unroll
                for (int r = 0; r < 3; ++r) T[4 * r + c] = o[4 * r + c] - p[r] * w;
            }
            int e = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = c; d < 4; ++d, ++e) acc[e] += T[c] * T[d] + T[4 + c] * T[4 + d] + T[8 + c] * T[8 + d];
        }
    }
    double M[16];
    {
        int e = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int d = c; d < 4; ++d, ++e) { const double s = tri_wave_sum(acc[e]); M[4 * c + d] = s; M[4 * d + c] = s; }
    }
    double hv[4];
    tri_min_eigvec(M, hv);
    X[0] = hv[0] / hv[3]; X[1] = hv[1] / hv[3]; X[2] = hv[2] / hv[3];
    // depth of every inlier view
    bool bad = false;
    if (in0) bad = bad || !(tri_depth(so + k0 * kTriRec, X) >= kTriDepthMin);
    if (in1) bad = bad || !(tri_depth(so + k1 * kTriRec, X) >= kTriDepthMin);
    if (__any(bad)) return false;
    // any pair of inlier centres with enough angle (the reference stops at the first; existence does not depend on the order)
    bool found = false;
    for (int b = 0; b < n && !found; ++b) {
        if (!(((b < 64 ? m0 : m1) >> (b & 63)) & 1ull)) continue;
        const double* cb = so + b * kTriRec + 12;
        bool f = false;
        if (in0 && k0 > b) f = f || tri_angle(so + k0 * kTriRec + 12, cb, X) >= prm.min_angle;
        if (in1 && k1 > b) f = f || tri_angle(so + k1 * kTriRec + 12, cb, X) >= prm.min_angle;
        found = __any(f);
    }
    if (!found) return false;
    // support over ALL observations
    double v0 = 0.0, v1 = 0.0;
    bool i0 = false, i1 = false;
    if (k0 < n) { const double r = tri_residual(so + k0 * kTriRec, X); i0 = r <= prm.max_residual; v0 = i0 ? r : 0.0; }
    if (k1 < n) { const double r = tri_residual(so + k1 * kTriRec, X); i1 = r <= prm.max_residual; v1 = i1 ? r : 0.0; }
    r0 = __ballot(i0); r1 = __ballot(i1);
    cnt = __popcll(r0) + __popcll(r1);
    sum = tri_wave_sum(v0 + v1);
    return true;
}

__global__ __launch_bounds__(kTriWave * kTriWaves) void k_tri_tracks(
        const CamRec* __restrict__ cam, const double* __restrict__ centre, const int* __restrict__ trk_ptr, const int* __restrict__ obs_cam,
        const double* __restrict__ obs_xy, int n_tracks, TriParams prm, const int32_t* __restrict__ dyn_tab, double* __restrict__ points,
        unsigned char* __restrict__ status, unsigned char* __restrict__ mask_out, int* __restrict__ num_inliers,
        int* __restrict__ num_trials, int* __restrict__ best_trial, unsigned long long* __restrict__ phase) {
    __shared__ double s_obs[kTriWaves][xtri::kMaxObs * kTriRec];
    const int lane = threadIdx.x & (kTriWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.x * kTriWaves + wave;
    int beg = 0, n = 0;
    if (j < n_tracks) {
        beg = __builtin_amdgcn_readfirstlane(trk_ptr[j]);
        n = __builtin_amdgcn_readfirstlane(trk_ptr[j + 1]) - beg;
    }
    const bool attempt = n >= 2 && n <= xtri::kMaxObs;
    double* so = s_obs[wave];
    if (attempt) {
        for (int k = lane; k < n; k += kTriWave) {
            const int c = obs_cam[beg + k];
            const double q[4] = {cam[c].q[0], cam[c].q[1], cam[c].q[2], cam[c].q[3]};
            double R[9];
            quat_to_mat(q, R);
            double* o = so + k * kTriRec;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                o[4 * r + 0] = R[3 * r + 0]; o[4 * r + 1] = R[3 * r + 1]; o[4 * r + 2] = R[3 * r + 2]; o[4 * r + 3] = cam[c].t[r];
                o[12 + r] = centre[3 * (size_t)c + r];
            }
            o[15] = obs_xy[2 * (size_t)(beg + k)]; o[16] = obs_xy[2 * (size_t)(beg + k) + 1];
        }
    }
    __syncthreads();                 // the only barrier: after it a wave touches nothing but its own part of LDS, read-only
    if (j >= n_tracks) return;
    if (!attempt) {
        if (lane == 0) {
            status[j] = n < 2 ? 2 : 3;
            points[3 * (size_t)j] = 0.0; points[3 * (size_t)j + 1] = 0.0; points[3 * (size_t)j + 2] = 0.0;
            num_inliers[j] = 0; num_trials[j] = 0; best_trial[j] = -1;
        }
        for (int k = lane; k < n; k += kTriWave) mask_out[beg + k] = 0;
        return;
    }

    xtri::Scan sc(dyn_tab + n * (xtri::kMaxObs + 1), n, prm.trial_cap, prm.exhaustive_threshold);
    double bX[3] = {0.0, 0.0, 0.0};
    unsigned long long bm0 = 0, bm1 = 0;
    const int two_n1 = 2 * n - 1;
    long long tick_a = 0, tick_b = 0, tick_c = 0, tick_d = 0;
#pragma unroll 1
    for (int t0 = 0; t0 < sc.max_trials; t0 += kTriWave) {
        const long long tk0 = XBA_TRI_TICK();
        // (a) the pair of trial t0 + lane: rank(i, j) = i (2n - i - 1) / 2 + (j - i - 1)
        const bool live = t0 + lane < sc.max_trials;
        const int t = live ? t0 + lane : 0;
        int pi = (int)(((double)two_n1 - sqrt((double)(two_n1 * two_n1 - 8 * t))) * 0.5);
        pi = max(0, min(pi, n - 2));
        if (pi * (two_n1 - pi) / 2 > t) --pi;
        if ((pi + 1) * (two_n1 - pi - 1) / 2 <= t) ++pi;
        pi = max(0, min(pi, n - 2));
        const int pj = max(pi + 1, min(t - pi * (two_n1 - pi) / 2 + pi + 1, n - 1));
        const double* oi = so + pi * kTriRec;
        const double* oj = so + pj * kTriRec;
        double X[3];
        {
            double a[16], hv[4];
            const double xi = oi[15], yi = oi[16], xj = oj[15], yj = oj[16];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                a[c] = xi * oi[8 + c] - oi[c];      a[4 + c] = yi * oi[8 + c] - oi[4 + c];
                a[8 + c] = xj * oj[8 + c] - oj[c];  a[12 + c] = yj * oj[8 + c] - oj[4 + c];
            }
            tri_null_svd(a, hv);
            X[0] = hv[0] / hv[3]; X[1] = hv[1] / hv[3]; X[2] = hv[2] / hv[3];
        }
        const bool has = live && tri_depth(oi, X) >= kTriDepthMin && tri_depth(oj, X) >= kTriDepthMin &&
                         tri_angle(oi + 12, oj + 12, X) >= prm.min_angle;
        const long long tk1 = XBA_TRI_TICK();
        // (b) support of this lane's model over the track, in observation order
        int cnt = 0;
        double sum = 0.0;
        unsigned long long m0 = 0, m1 = 0;
#pragma unroll 1
        for (int k = 0; k < n; ++k) {
            const double r = tri_residual(so + k * kTriRec, X);
            const bool inl = r <= prm.max_residual;
            if (inl) { ++cnt; sum += r; }
            if (k < 64) m0 |= (unsigned long long)inl << k; else m1 |= (unsigned long long)inl << (k - 64);
        }
        const long long tk2 = XBA_TRI_TICK();
        long long refit_ticks = 0;
        // (c) the scan, in trial order over the lanes that have a model
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const xtri::Offer r = sc.offer(t0 + l, true, __shfl(cnt, l, kTriWave), __shfl(sum, l, kTriWave));
            if (r != xtri::kIgnored) {
                bX[0] = __shfl(X[0], l, kTriWave); bX[1] = __shfl(X[1], l, kTriWave); bX[2] = __shfl(X[2], l, kTriWave);
                bm0 = __shfl(m0, l, kTriWave); bm1 = __shfl(m1, l, kTriWave);
                if (r == xtri::kNewBestRefit) {
                    double lX[3] = {0.0, 0.0, 0.0}, lsum = 0.0;
                    int lcnt = 0;
                    unsigned long long l0 = 0, l1 = 0;
                    const long long tr0 = XBA_TRI_TICK();
                    const bool has_local = tri_refit(so, n, lane, bm0, bm1, prm, lX, lcnt, lsum, l0, l1);
                    refit_ticks += XBA_TRI_TICK() - tr0;
                    if (has_local && sc.offer_local(lcnt, lsum)) {
                        bX[0] = lX[0]; bX[1] = lX[1]; bX[2] = lX[2];
                        bm0 = l0; bm1 = l1;
                    }
                }
            }
            if (sc.after_trial(t0 + l)) break;
        }
        const long long tk3 = XBA_TRI_TICK();
        tick_a += tk1 - tk0; tick_b += tk2 - tk1; tick_c += tk3 - tk2 - refit_ticks; tick_d += refit_ticks;
        if (sc.abort) break;             // (e)
    }
#ifdef XBA_TRI_PHASES
    if (phase && lane == 0) {
        atomicAdd(phase + 0, (unsigned long long)tick_a); atomicAdd(phase + 1, (unsigned long long)tick_b);
        atomicAdd(phase + 2, (unsigned long long)tick_c); atomicAdd(phase + 3, (unsigned long long)tick_d);
    }
#endif
    const bool ok = sc.finish() && isfinite(bX[0]) && isfinite(bX[1]) && isfinite(bX[2]);
    if (lane == 0) {
        status[j] = ok ? 1 : 0;
        points[3 * (size_t)j] = ok ? bX[0] : 0.0; points[3 * (size_t)j + 1] = ok ? bX[1] : 0.0; points[3 * (size_t)j + 2] = ok ? bX[2] : 0.0;
        num_inliers[j] = ok ? sc.best_count : 0;
        num_trials[j] = ok ? sc.num_trials : 0;
        best_trial[j] = ok ? sc.best_trial_code() : -1;
    }
    for (int k = lane; k < n; k += kTriWave) mask_out[beg + k] = ok ? (unsigned char)(((k < 64 ? bm0 : bm1) >> (k & 63)) & 1ull) : 0;
}

}  // namespace xba
