// The decision rule of the LO-RANSAC that creates a 3-D point from the observations of a key point
// (/root/reference/src/geometry/colmap/optim/loransac.h:129-205, ransac.h:141-167, support_measurement.cc), restated without any
// geometry: it sees, trial by trial and in trial order, whether the sample had a model and the support (inlier count, sum of the
// inlier residuals) of that model and of its locally optimised refit, and decides which model is the best, when a refit is due
// and when the scan stops.  The kernel (ba_tri.h: k_tri_tracks, wave-uniform) and a host driver of the CPU tests are compiled
// from this file.  Plain C++ without HIP types.
//
// The adaptive trial bound dyn(k, n) = ceil(log(1 - confidence) / log(1 - (k / n)^2)) depends on integers only; the host tabulates
// it with its own log() (tri_dyn_trials) and the scan reads the row of its n, so no device transcendental sits in a decision.
//
// Defined meaning where the reference has none: a sample model without a single inlier still beats the initial best (0 == 0 and
// 0.0 < DBL_MAX), and the reference then evaluates log(1 - 0) = 0 in the denominator and casts -inf to size_t.  Here k = 0 means
// "no information": dyn is unbounded.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define XTRI_HD __host__ __device__
#else
#define XTRI_HD
#endif

namespace xtri {

constexpr int kMaxObs = 128;                  // XRSFM_BA_TRI_MAX_OBS: C(128, 2) = 8128 trials, below the reference's cap of 10000
constexpr int32_t kUnbounded = INT32_MAX;     // "never" for a trial index (trials <= 8128)
constexpr int32_t kLocalBit = 1 << 30;        // best_trial: the locally optimised model of that trial is the one returned

// ComputeNumTrials(k, n, confidence) of ransac.h:151-167, clamped to kUnbounded; host only (log)
inline int32_t tri_dyn_trials(int k, int n, double confidence) {
    const double nom = 1.0 - confidence;
    if (nom <= 0.0 || k <= 0) return kUnbounded;                    // (k == 0: the defined meaning above)
    const double ratio = (double)k / (double)n;
    const double denom = 1.0 - ratio * ratio;
    if (denom <= 0.0) return 1;
    const double v = std::ceil(std::log(nom) / std::log(denom));
    return v >= (double)kUnbounded ? kUnbounded : (int32_t)v;
}

// the constructor's bound from min_inlier_ratio (ransac.h:141-147): 23022 with the reference's options
inline int32_t tri_ratio_trials(double min_inlier_ratio, double confidence) {
    const long long k = (long long)(min_inlier_ratio * 100000.0);
    const double nom = 1.0 - confidence;
    if (nom <= 0.0 || k <= 0) return kUnbounded;
    const double ratio = (double)k / 100000.0;
    const double denom = 1.0 - ratio * ratio;
    if (denom <= 0.0) return 1;
    const double v = std::ceil(std::log(nom) / std::log(denom));
    return v >= (double)kUnbounded ? kUnbounded : (int32_t)v;
}

XTRI_HD inline int32_t tri_num_pairs(int n) { return n * (n - 1) / 2; }

enum Offer { kIgnored = 0, kNewBest = 1, kNewBestRefit = 2 };

struct Scan {
    const int32_t* dyn_row;       // dyn(k, n) for k = 0 .. n
    int32_t max_trials;           // min(options' cap, the min_inlier_ratio bound, C(n, 2))
    int32_t min_trials;           // C(n, 2) for tracks up to the exhaustive threshold, else 0
    int32_t dyn;
    int32_t best_count = 0;
    double best_sum = DBL_MAX;
    int32_t best_trial = -1;
    bool best_local = false;
    bool had_model = false;       // of the trial being scanned
    bool abort = false;
    int32_t num_trials = 0;

    XTRI_HD Scan(const int32_t* row, int n, int32_t trial_cap, int exhaustive_threshold) : dyn_row(row) {
        const int32_t pairs = tri_num_pairs(n);
        max_trials = trial_cap < pairs ? trial_cap : pairs;
        min_trials = n <= exhaustive_threshold ? pairs : 0;
        dyn = max_trials;
        num_trials = max_trials;          // what the loop's counter holds when no trial aborts
    }
    XTRI_HD static bool beats(int32_t ca, double sa, int32_t cb, double sb) { return ca > cb || (ca == cb && sa < sb); }

    // the sample of trial t: its support over all observations, if it has a model
    XTRI_HD Offer offer(int32_t t, bool has_model, int32_t count, double sum) {
        had_model = has_model;
        if (!has_model || !beats(count, sum, best_count, best_sum)) return kIgnored;
        best_count = count; best_sum = sum; best_trial = t; best_local = false;
        dyn = dyn_row[best_count];
        return count > 2 ? kNewBestRefit : kNewBest;
    }
    // the refit of that sample's inliers, if it has a model: true when it replaces the sample model
    XTRI_HD bool offer_local(int32_t count, double sum) {
        if (!beats(count, sum, best_count, best_sum)) return false;
        best_count = count; best_sum = sum; best_local = true;
        dyn = dyn_row[best_count];
        return true;
    }
    // after trial t (and its refit): true when the scan stops.  The reference notices the flag at the top of the next trial and
    // counts that trial too, unless the loop's own bound ends it first.
    XTRI_HD bool after_trial(int32_t t) {
        if (had_model && t >= dyn && t >= min_trials) {
            abort = true;
            num_trials = t + 1 < max_trials ? t + 2 : t + 1;
        }
        return abort;
    }
    XTRI_HD bool finish() const { return best_count >= 2; }          // success
    XTRI_HD int32_t best_trial_code() const { return best_trial < 0 ? -1 : (best_local ? (best_trial | kLocalBit) : best_trial); }
};

}  // namespace xtri
