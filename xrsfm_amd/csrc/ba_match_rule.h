// The rule of the SIFT descriptor matcher (SiftMatchGPU::GetSiftMatch as FeatureMatching calls it, reference
// src/feature/feature_processing.cc:118-154, 240-255; 3rdparty/SiftGPU/ProgramCU.cu:1491-1884: MultiplyDescriptor_Kernel,
// RowMatch_Kernel, ColMatch_Kernel; SiftMatchCU.cpp:186-215: GetBestMatch), restated on integers.  The kernels (ba_match.h) and the
// host drivers of the CPU tests are compiled from this file.  Plain C++ without HIP types.
//
// Score: dot(i, j) = sum_k a[i][k] b[j][k] over 128 uint8 components, an exact integer of at most 128 * 255^2 = 8 323 200.
// Top-2 of a row over all columns (and of a column over all rows): the triple (best, idx, next) starts at (0, -1, 0); the update is
// strict (v > best), RowMatch_Kernel:1804-1807; two triples merge as in :1819-1825 and ColMatch_Kernel:1861-1863.  So best is
// max(0, max dot), next the second largest value counted with multiplicity and floored at 0, idx the position of best or -1 when
// no dot is positive.  Of several positions holding the best, idx is the LOWEST (the reference's choice depends on its 32-lane
// walk; with max_ratio <= 1 a tied best never passes the ratio test, so the difference cannot be observed in a match).  top_merge
// is written so that it may be applied in any order and grouping: it decides a tie by the index.
//
// Distance: dist(d) = (float) acos(min((double) ((float) d * 2^-18f), 1.0)), :1830-1831.  Only d clamped to [0, 262144] matters;
// the host tabulates it once with its own acos (match_build_table) and the device reads the table, so no transcendental runs on
// the device and none sits in a decision.  Test: dist(best) < max_distance && dist(best) < dist(next) * max_ratio, all float: one
// rounded multiply and two compares, :1833.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define XMATCH_HD __host__ __device__
#else
#define XMATCH_HD
#endif

namespace xmatch {

constexpr int kDim = 128;                     // XRSFM_BA_MATCH_DIM
constexpr int kMaxFeatures = 16384;           // XRSFM_BA_MATCH_MAX_FEATURES
constexpr int kTabMax = 262144;               // 2^18: the score from which the distance is 0
constexpr int kTabSize = kTabMax + 1;

struct Top {
    int32_t best, idx, next;
};

XMATCH_HD inline Top top_init() { return Top{0, -1, 0}; }

// RowMatch_Kernel:1804-1807; positions offered in ascending order keep the lowest index of a tied best
XMATCH_HD inline void top_update(Top& t, int32_t v, int32_t pos) {
    const bool test = v > t.best;
    t.next = test ? t.best : (t.next > v ? t.next : v);
    t.idx = test ? pos : t.idx;
    t.best = test ? v : t.best;
}

// ColMatch_Kernel:1861-1863 with the tie decided by the lower index (-1, "none", is the highest: it only meets best == 0)
XMATCH_HD inline Top top_merge(const Top& a, const Top& b) {
    const bool take_b = b.best > a.best || (b.best == a.best && (uint32_t)b.idx < (uint32_t)a.idx);
    Top r;
    r.best = take_b ? b.best : a.best;
    r.idx = take_b ? b.idx : a.idx;
    r.next = take_b ? (a.best > b.next ? a.best : b.next) : (a.next > b.best ? a.next : b.best);
    return r;
}

// dist(d) for d = 0 .. 2^18; host only (acos)
inline void match_build_table(float* tab) {
    for (int d = 0; d <= kTabMax; ++d) {
        const double x = (double)((float)d * 0.000003814697265625f);
        tab[d] = (float)std::acos(x < 1.0 ? x : 1.0);
    }
}

XMATCH_HD inline bool match_keep(const float* tab, int32_t best, int32_t next, float max_distance, float max_ratio) {
    const float dist = tab[best < kTabMax ? best : kTabMax], distn = tab[next < kTabMax ? next : kTabMax];
    return dist < max_distance && dist < distn * max_ratio;
}

// row_match / col_match of a triple
XMATCH_HD inline int32_t match_of(const float* tab, const Top& t, float max_distance, float max_ratio) {
    return match_keep(tab, t.best, t.next, max_distance, max_ratio) ? t.idx : -1;
}

// whether (i, row_match[i]) is a match (GetBestMatch, SiftMatchCU.cpp:199-213)
XMATCH_HD inline bool match_is(int32_t i, int32_t rm, const int32_t* col_match, int mutual_best) {
    return rm >= 0 && (!mutual_best || col_match[rm] == i);
}

// the matches of a pair in ascending i; returns their number
inline int32_t match_compact(int32_t n_a, const int32_t* row_match, const int32_t* col_match, int mutual_best, int32_t* out) {
    int32_t n = 0;
    for (int32_t i = 0; i < n_a; ++i)
        if (match_is(i, row_match[i], col_match, mutual_best)) { out[2 * n] = i; out[2 * n + 1] = row_match[i]; ++n; }
    return n;
}

}  // namespace xmatch
