// The decision rule of the 5-point RANSAC that starts a reconstruction (find_essential_matrix, reference
// src/geometry/essential.cc:306-387, as solve_essential :389-404 calls it), restated without any geometry: it sees, model by model
// and in (trial, model slot) order, the support (inlier count, score) of an essential matrix and decides which model is the best
// and when the loop stops.  The kernel (ba_init.h: k_init_pairs, workgroup-uniform) and the host drivers of the CPU tests are
// compiled from this file.  Plain C++ without HIP types.
//
// Restated literally, quirks included:
//   support   se = sampson_error(E, p1, p2), already a squared quantity; inlier iff se < 2 th^2; score = sum over ALL matches, in
//             index order, of log(1.0 + se * se / (2 th^2)) (the squared error is squared once more);
//   offer     "more inliers, or as many with best_inlier > 0 and a strictly smaller score"; every model of a trial is offered, an
//             update does not skip the trial's remaining models;
//   bound     starts at max_iterations; after a new best of k inliers out of n, N = log(1 - confidence) / log(1 - (k / n)^5) and
//             `if (N < bound) bound = ceil(N)`; the loop test is `t < bound` at the top of each trial; num_trials is the number of
//             trials executed.
// N depends on integers only: the host tabulates ceil(N) for k = 0 .. n per distinct n (init_bound_row: its own log and pow), so
// no device transcendental sits in a stop decision.  Defined meaning where the reference has none: N is NaN (confidence 1 with
// k = n), or -inf (pow underflows, log(1) = +0: the reference casts -inf to size_t) -> "no information", kUnbounded.
//
// Two points where the reference has no portable meaning (include/xrsfm_ba.h documents them for the caller):
//   1. Sampler.  LotBox (utility/random.h:90-135) uses std::default_random_engine and std::uniform_int_distribution<size_t>, both
//      chosen by the standard library.  Here every pair gets a fresh xpnp::Mt19937(seed) and the sampler of ba_pnp_scan.h with
//      five draws: the index array persists across the trials of a pair (refill_all only resets cap), five Fisher-Yates steps per
//      trial, the same bounded draw.  Host only (init_sample_quintuples); the kernel reads the quintuples.
//   2. Model order.  The models of one trial are offered in ascending real eigenvalue (ba_init_geom.h); Eigen's order is not
//      portable.  The order decides exact ties only.
#pragma once
#include "ba_pnp_scan.h"

#ifdef __HIPCC__
#define XINIT_HD __host__ __device__
#else
#define XINIT_HD
#endif

namespace xinit {

constexpr int kMaxMatches = 8192;             // XRSFM_BA_INIT_MAX_MATCHES
constexpr int kMaxTrials = 64;                // XRSFM_BA_INIT_MAX_TRIALS
constexpr int kMaxModels = 10;                // real eigenvalues of the 10x10 action matrix
constexpr int kSlotStride = 16;               // best_trial = trial * 16 + model slot
constexpr int32_t kUnbounded = INT32_MAX;

// one row of the trial bound: row[k] = ceil(N(k, n)), k = 0 .. n; host only (log, pow)
inline void init_bound_row(int n, double confidence, int32_t* row) {
    const double K = std::log(1.0 - confidence);
    for (int k = 0; k <= n; ++k) {
        const double ratio = (double)k / (double)n;
        const double N = K / std::log(1.0 - std::pow(ratio, 5));
        row[k] = (N != N || N < 0.0 || std::ceil(N) >= (double)kUnbounded) ? kUnbounded : (int32_t)std::ceil(N);
    }
}

// deviation 1: the sample quintuples of the first n_trials trials of a pair of n >= 5 matches; idx is scratch of n entries
inline void init_sample_quintuples(uint32_t seed, int n, int n_trials, int32_t* idx, int32_t* quintuples) {
    xpnp::pnp_sample_tuples(seed, n, n_trials, 5, idx, quintuples);
}

// sampson_error (essential.cc:283-290); E row-major
XINIT_HD inline double sampson(const double* E, double x1, double y1, double x2, double y2) {
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double r = x2 * a0 + y2 * a1 + a2;
    return r * r * (1.0 / (a0 * a0 + a1 * a1) + 1.0 / (b0 * b0 + b1 * b1));
}

// the support of one model, match by match in index order
struct Support {
    int32_t count = 0;
    double score = 0.0;
    XINIT_HD void add(double se, double th2) {
        score += log(1.0 + se * se / th2);
        if (se < th2) ++count;
    }
};

struct Scan {
    const int32_t* row;           // ceil(N(k, n)) for k = 0 .. n
    int32_t bound;                // iter_max
    int32_t best_count = 0;
    double best_score = DBL_MAX;
    int32_t best_code = -1;       // trial * kSlotStride + slot of the best model, -1 without one

    XINIT_HD Scan(const int32_t* bound_row, int32_t max_iterations) : row(bound_row), bound(max_iterations) {}
    XINIT_HD bool more(int32_t t) const { return t < bound; }         // the loop test at the top of trial t
    // model `slot` of trial t with its support over all matches: true when it is the new best
    XINIT_HD bool offer(int32_t t, int32_t slot, int32_t count, double score) {
        if (!(count > best_count || (count == best_count && best_count > 0 && score < best_score))) return false;
        best_count = count; best_score = score; best_code = t * kSlotStride + slot;
        const int32_t N = row[count];
        if (N < bound) bound = N;
        return true;
    }
};

}  // namespace xinit
