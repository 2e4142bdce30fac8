// The decision rule of the LO-RANSAC that estimates the absolute pose of a frame from 2D-3D correspondences
// (colmap::LORANSAC<P3PEstimator, EPNPEstimator>::Estimate, reference src/geometry/colmap/optim/loransac.h:92-239, with
// InlierSupportMeasurer and ransac.h:141-167), restated without any geometry: it sees, model by model and in (trial, ascending
// root) order, the support (inlier count, sum of the inlier residuals) of a sample model and of its locally optimised model, and
// decides which model is the best, when a local optimisation is due and when the scan stops.  The kernel (ba_pnp.h: k_pnp_frames,
// workgroup-uniform) and the host drivers of the CPU tests are compiled from this file.  Plain C++ without HIP types.
//
// Restated literally: Compare is "more inliers, or as many and a strictly smaller residual sum"; a local optimisation runs only for a
// new best with more than 3 inliers; the abort test `trials >= dyn && trials >= min_num_trials` sits inside the model loop, so it is
// made after every model (never in a trial without one) and the reference counts one further trial; success needs 3 inliers.
//
// The adaptive trial bound dyn(k, n) = ceil(log(1 - confidence) / log(1 - (k / n)^3)) depends on integers only; the host tabulates
// it per frame with its own log() (pnp_dyn_trials) and the scan reads the row, so no device transcendental sits in a decision.
//
// Three points where the reference has no portable meaning (include/xrsfm_ba.h documents them for the caller):
//   1. Sampler.  The reference draws from one process-wide std::mt19937 that is never re-seeded, through
//      std::uniform_int_distribution, whose algorithm the standard library chooses.  Here every frame gets a fresh MT19937
//      (standard recurrence, init_genrand(seed)) and replays RandomSampler (optim/random_sampler.cc:43-62, util/random.h:114-122):
//      the index array persists across the trials of a frame, three Fisher-Yates steps per trial.  Bounded draw for
//      m = last - i + 1: s = 0xFFFFFFFF / m; draw 32-bit words until x < m s; j = i + x / s.  Host only (pnp_sample_triples below); the kernel
//      reads the triples.
//   2. Root order and acceptance: ba_pnp_geom.h (p3p_models).
//   3. EPnP's sign step: ba_pnp_geom.h (epnp_stage_solve).
// Defined meaning where the reference has none: a model without a single inlier still beats the initial best (0 == 0 and
// 0.0 < DBL_MAX), and the reference then evaluates log(1 - 0) = 0 in the denominator and casts -inf to size_t.  Here k = 0 means
// "no information": dyn is unbounded (the convention of ba_tri_scan.h).  A model with a non-finite entry is never offered.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define XPNP_HD __host__ __device__
#else
#define XPNP_HD
#endif

namespace xpnp {

constexpr int kMaxCorr = 8192;                // XRSFM_BA_POSE_MAX_CORR
constexpr int kMaxTrials = 16384;             // XRSFM_BA_POSE_MAX_TRIALS
constexpr int32_t kUnbounded = INT32_MAX;     // "never" for a trial index
constexpr int32_t kLocalBit = 1 << 30;        // best_trial: the locally optimised model of that trial is the one returned

// ComputeNumTrials(k, n, confidence) of ransac.h:151-167 for a minimal sample of 3, clamped to kUnbounded; host only (log, pow)
inline int32_t pnp_dyn_trials(long long k, long long n, double confidence) {
    const double nom = 1.0 - confidence;
    if (nom <= 0.0 || k <= 0) return kUnbounded;                    // (k == 0: the defined meaning above)
    const double ratio = (double)k / (double)n;
    const double denom = 1.0 - std::pow(ratio, 3);
    if (denom <= 0.0) return 1;
    const double v = std::ceil(std::log(nom) / std::log(denom));
    return v >= (double)kUnbounded ? kUnbounded : (int32_t)v;
}

// the constructor's bound from min_inlier_ratio (ransac.h:141-147): 585 with the reference's options
inline int32_t pnp_ratio_trials(double min_inlier_ratio, double confidence) {
    return pnp_dyn_trials((long long)(min_inlier_ratio * 100000.0), 100000, confidence);
}

// MT19937 (Matsumoto & Nishimura 1998): the recurrence std::mt19937 is specified to have, seeded by init_genrand
struct Mt19937 {
    uint32_t mt[624];
    int idx;
    explicit Mt19937(uint32_t seed) {
        mt[0] = seed;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
};

// deviation 1: the samples of m distinct indices of the first n_trials trials of a set of n >= m entries; idx is scratch of n
// entries.  m = 3 here; the two-view initialisation (ba_init_scan.h) draws m = 5 from the same generator and bounded draw.
inline void pnp_sample_tuples(uint32_t seed, int n, int n_trials, int m_draws, int32_t* idx, int32_t* tuples) {
    Mt19937 g(seed);
    for (int i = 0; i < n; ++i) idx[i] = i;
    const uint32_t last = (uint32_t)(n - 1);
    for (int t = 0; t < n_trials; ++t) {
        for (uint32_t i = 0; i < (uint32_t)m_draws; ++i) {
            const uint32_t m = last - i + 1, s = 0xFFFFFFFFu / m;
            uint32_t x;
            do x = g.next(); while (x >= m * s);              // (m s <= 0xFFFFFFFF: no overflow)
            const uint32_t j = i + x / s;
            const int32_t tmp = idx[i]; idx[i] = idx[j]; idx[j] = tmp;
        }
        for (int i = 0; i < m_draws; ++i) tuples[(size_t)m_draws * t + i] = idx[i];
    }
}
inline void pnp_sample_triples(uint32_t seed, int n, int n_trials, int32_t* idx, int32_t* triples) {
    pnp_sample_tuples(seed, n, n_trials, 3, idx, triples);
}

enum Offer { kIgnored = 0, kNewBest = 1, kNewBestLocal = 2 };

struct Scan {
    const int32_t* dyn_row;       // dyn(k, n) for k = 0 .. n
    int32_t max_trials;           // min(options' cap, the min_inlier_ratio bound)
    int32_t min_trials;
    int32_t dyn;
    int32_t best_count = 0;
    double best_sum = DBL_MAX;
    int32_t best_trial = -1;
    bool best_local = false;
    bool abort = false;
    int32_t num_trials = 0;

    XPNP_HD Scan(const int32_t* row, int32_t trial_cap, int32_t min_num_trials) : dyn_row(row), max_trials(trial_cap), min_trials(min_num_trials) {
        dyn = max_trials;
        num_trials = max_trials;          // what the loop's counter holds when no trial aborts
    }
    XPNP_HD static bool beats(int32_t ca, double sa, int32_t cb, double sb) { return ca > cb || (ca == cb && sa < sb); }

    // a sample model of trial t: its support over all correspondences
    XPNP_HD Offer offer(int32_t t, int32_t count, double sum) {
        if (!beats(count, sum, best_count, best_sum)) return kIgnored;
        best_count = count; best_sum = sum; best_trial = t; best_local = false;
        dyn = dyn_row[best_count];
        return count > 3 ? kNewBestLocal : kNewBest;
    }
    // the locally optimised model of that sample model's inliers, if it has one: true when it replaces the sample model
    XPNP_HD bool offer_local(int32_t count, double sum) {
        if (!beats(count, sum, best_count, best_sum)) return false;
        best_count = count; best_sum = sum; best_local = true;
        dyn = dyn_row[best_count];
        return true;
    }
    // after every model of trial t (and its local optimisation): true when the scan stops; the rest of the trial's models are
    // not looked at.  The reference notices the flag at the top of the next trial and counts that trial too, unless the loop's
    // own bound ends it first.
    XPNP_HD bool after_model(int32_t t) {
        if (t >= dyn && t >= min_trials) {
            abort = true;
            num_trials = t + 1 < max_trials ? t + 2 : t + 1;
        }
        return abort;
    }
    XPNP_HD bool finish() const { return best_count >= 3; }          // success
    XPNP_HD int32_t best_trial_code() const { return best_trial < 0 ? -1 : (best_local ? (best_trial | kLocalBit) : best_trial); }
};

}  // namespace xpnp
