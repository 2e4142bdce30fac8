// The decision rule of the LO-RANSAC that verifies a matched image pair by a fundamental matrix
// (colmap::LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator>::Estimate, reference
// src/geometry/colmap/optim/loransac.h:92-239, with InlierSupportMeasurer and ransac.h:136-167), restated without any geometry, and
// the sampler.  The scan is xpnp::Scan (ba_pnp_scan.h) with the minimal sample of 3 replaced by 7 and the local estimator's
// minimum by 8; it is written out here on its own so that k_pnp_frames and k_init_pairs are compiled from unchanged text.  The
// kernel (ba_fund.h: k_verify_pairs, workgroup-uniform) and the host drivers of the CPU tests are compiled from this file.  Plain
// C++ without HIP types.
//
// Restated literally: Compare is "more inliers, or as many and a strictly smaller residual sum"; a local optimisation runs for a
// new best with more than 7 and at least 8 inliers; the abort test `trials >= dyn && trials >= min_num_trials` sits inside the
// model loop, so it is made after every model (never in a trial without one) and the reference counts one further trial; success
// needs 7 inliers.
//
// The adaptive trial bound dyn(k, n) = ceil(log(1 - confidence) / log(1 - (k / n)^7)) depends on integers only; the host tabulates
// it per pair with its own log() (fund_dyn_trials) and the scan reads the row, so no device transcendental sits in a decision.  As
// in ba_pnp_scan.h, k = 0 means "no information": the bound stays unbounded.  A model with a non-finite entry is never offered.
//
// Sampler (deviation 1 of include/xrsfm_ba.h): every pair gets a fresh MT19937 (init_genrand(seed)) and replays RandomSampler with
// seven Fisher-Yates steps per trial on an index array that persists across the trials of the pair; the bounded draw is that of
// pnp_sample_tuples, with a cap on the words it may reject (kMaxRedraws: never reached, it only bounds the device loop).  Unlike
// the pose call the tuples are drawn where they are used: Sampler works on storage the caller owns (LDS in the kernel, plain
// arrays on the host), integers only, so host and device produce the same tuples.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define XFUND_HD __host__ __device__
#else
#define XFUND_HD
#endif

namespace xfund {

constexpr int kMaxMatches = 8192;             // XRSFM_BA_FUND_MAX_MATCHES
constexpr int kMaxTrials = 16384;             // XRSFM_BA_FUND_MAX_TRIALS
constexpr int kSample = 7;                    // FundamentalMatrixSevenPointEstimator::kMinNumSamples
constexpr int kLocalMin = 8;                  // FundamentalMatrixEightPointEstimator::kMinNumSamples
constexpr int kMaxRedraws = 16;               // rejected words of one bounded draw before the last one is clamped
constexpr int32_t kUnbounded = INT32_MAX;     // "never" for a trial index
constexpr int32_t kLocalBit = 1 << 30;        // best_trial: the 8-point local model of that trial is the one returned

// ComputeNumTrials(k, n, confidence) of ransac.h:151-167 for a minimal sample of 7, clamped to kUnbounded; host only (log, pow)
inline int32_t fund_dyn_trials(long long k, long long n, double confidence) {
    const double nom = 1.0 - confidence;
    if (nom <= 0.0 || k <= 0) return kUnbounded;
    const double ratio = (double)k / (double)n;
    const double denom = 1.0 - std::pow(ratio, kSample);
    if (denom <= 0.0) return 1;
    const double v = std::ceil(std::log(nom) / std::log(denom));
    return v >= (double)kUnbounded ? kUnbounded : (int32_t)v;
}

// the constructor's bound from min_inlier_ratio (ransac.h:141-147): 113174 with the reference's options, above its max_num_trials
inline int32_t fund_ratio_trials(double min_inlier_ratio, double confidence) {
    return fund_dyn_trials((long long)(min_inlier_ratio * 100000.0), 100000, confidence);
}

// MT19937 and the persistent index array on caller-owned storage: mt[624], idx[n]
struct Sampler {
    uint32_t* mt;
    int32_t* idx;
    int32_t pos, n;

    // the generator's state; idx[i] = i is left to the caller (the kernel fills it with all threads)
    XFUND_HD void seed(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        pos = 624;
    }
    XFUND_HD uint32_t next() {
        if (pos >= 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[i + 1 < 624 ? i + 1 : 0] & 0x7fffffffu);
                mt[i] = mt[i + 397 < 624 ? i + 397 : i - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        uint32_t y = mt[pos++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
    // the next trial's sample: seven distinct indices
    XFUND_HD void draw(int32_t* tuple) {
        const uint32_t last = (uint32_t)(n - 1);
        for (uint32_t i = 0; i < (uint32_t)kSample; ++i) {
            const uint32_t m = last - i + 1, s = 0xFFFFFFFFu / m;
            uint32_t x = next();                              // (m s <= 0xFFFFFFFF: no overflow; a word is rejected with p < 2^-18)
            for (int redraw = 0; redraw < kMaxRedraws && x >= m * s; ++redraw) x = next();
            if (x >= m * s) x = m * s - 1;                    // kMaxRedraws rejections in a row (p < 2^-288): the loop stays bounded
            const uint32_t j = i + x / s;
            const int32_t tmp = idx[i]; idx[i] = idx[j]; idx[j] = tmp;
        }
        for (int i = 0; i < kSample; ++i) tuple[i] = idx[i];
    }
};

// the septuples of the first n_trials trials of a pair of n >= 7 matches; mt is scratch of 624 words, idx of n entries (host)
inline void fund_sample_tuples(uint32_t seed, int n, int n_trials, uint32_t* mt, int32_t* idx, int32_t* tuples) {
    Sampler g{mt, idx, 0, n};
    g.seed(seed);
    for (int i = 0; i < n; ++i) idx[i] = i;
    for (int t = 0; t < n_trials; ++t) g.draw(tuples + (size_t)kSample * t);
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

    XFUND_HD Scan(const int32_t* row, int32_t trial_cap, int32_t min_num_trials) : dyn_row(row), max_trials(trial_cap), min_trials(min_num_trials) {
        dyn = max_trials;
        num_trials = max_trials;          // what the loop's counter holds when no trial aborts
    }
    XFUND_HD static bool beats(int32_t ca, double sa, int32_t cb, double sb) { return ca > cb || (ca == cb && sa < sb); }

    // a sample model of trial t: its support over all matches
    XFUND_HD Offer offer(int32_t t, int32_t count, double sum) {
        if (!beats(count, sum, best_count, best_sum)) return kIgnored;
        best_count = count; best_sum = sum; best_trial = t; best_local = false;
        dyn = dyn_row[best_count];
        return (count > kSample && count >= kLocalMin) ? kNewBestLocal : kNewBest;
    }
    // the 8-point model of that sample model's inliers, if it has one: true when it replaces the sample model
    XFUND_HD bool offer_local(int32_t count, double sum) {
        if (!beats(count, sum, best_count, best_sum)) return false;
        best_count = count; best_sum = sum; best_local = true;
        dyn = dyn_row[best_count];
        return true;
    }
    // after every model of trial t (and its local optimisation): true when the scan stops; the rest of the trial's models are
    // not looked at.  The reference notices the flag at the top of the next trial and counts that trial too, unless the loop's
    // own bound ends it first.
    XFUND_HD bool after_model(int32_t t) {
        if (t >= dyn && t >= min_trials) {
            abort = true;
            num_trials = t + 1 < max_trials ? t + 2 : t + 1;
        }
        return abort;
    }
    XFUND_HD bool finish() const { return best_count >= kSample; }          // success
    XFUND_HD int32_t best_trial_code() const { return best_trial < 0 ? -1 : (best_local ? (best_trial | kLocalBit) : best_trial); }
};

}  // namespace xfund
