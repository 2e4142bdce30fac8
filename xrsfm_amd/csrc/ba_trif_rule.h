// The rules of frame triangulation (ba_trif.h): what Point3dProcessor::TriangulateFramePoint of the reference decides
// (src/geometry/track_processor.cc:163-251) for a list of frames, restated on the flat map state of ba_merge_rule.h (the track of every
// key point, the point and the outlier flag of every track).  Plain C++, shared by the host and the kernels; tests/trif_host_driver.py
// compiles this file alone, with the address and undefined-behaviour sanitizers.
//
//   rule      the dot product of GetMaxAngle's two rays, the order of the candidates and the threshold as a bound on the dot product
//   check     what is wrong with a call's arguments
//   plan      the slots (the untracked key points of the listed frames with two or more observations), their observation lists, and
//             the steps: per listed frame its slots cut into maximal contiguous runs that hold no two coupled key points (two slots
//             whose lists share an entry that carries no track when the call begins: only such an entry can be given a track by a
//             create, and so change the other slot's branch; an entry that carries a track keeps it throughout the call)
//   program   the steps as plain loops (the stand-alone program runs them; the library runs the kernels of ba_trif.h)
//
// DEVIATION from the literal comparison of angles.  The reference orders the candidates by acos(dot) and accepts acos(dot) < th.
// No kernel evaluates acos: candidates are ordered by the dot product (larger is better, the smaller id on equal dot products), and
// the threshold is dot >= dot_bound(th), the smallest double whose acos, taken with the host's libm, is below th.  For a monotone
// acos the acceptance is the literal one bit for bit.  The order can differ only where two different dot products round to the same
// acos (there the reference keeps the smaller id, this rule the larger dot product), that is at differences of an ulp of the angle;
// tests/trif_yardstick.py records every decision's margin and tests/test_trif_cpu.py shows none of the catalogue near it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define XTRIF_HD __host__ __device__
#else
#define XTRIF_HD
#endif
// the comparisons are made on values rounded once per operation, on the host and on the device alike
#if defined(__clang__)
#define XTRIF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define XTRIF_NO_CONTRACT
#endif
// held[] changes while a claim kernel runs: its lanes read it past the caches of their compute unit
#ifdef __HIP_DEVICE_COMPILE__
#define XTRIF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define XTRIF_LOAD(p) (*(p))
#endif

namespace xtrif {

struct TriOpt { double min_tri_angle_rad, max_error_rad, confidence, min_inlier_ratio; int32_t max_num_trials, exhaustive_threshold; };
struct Opt { double extend_angle_rad; TriOpt tri; };                    // xrsfm_ba_trif_options, field for field
constexpr double kExtendAngle = 8.0 * 0.0174532925199432954743716805978692718781530857086181640625;   // DegToRad(8.0), run_triangulation.cc:144

// key_status
constexpr uint8_t kNotVisited = 0, kCreated = 1, kFewObs = 2, kTooMany = 3, kNoModel = 4, kExtended = 5, kNoneAccepted = 6;
// the branch of a slot in its step
constexpr int32_t kClsNone = 0, kClsCreate = 1, kClsOne = 2, kClsMulti = 3;
constexpr int32_t kMaxObs = 128;              // XRSFM_BA_TRI_MAX_OBS: a longer list is status 3
constexpr int32_t kNoBid = 0x7f7f7f7f;       // a track nobody bids on (the bytes a memset writes)

// ---- rule
// ray1 = (q X + t).normalized(), ray2 = (xn, yn, 1).normalized(), Eigen's normalized(): a zero vector stays zero.  q X by the
// rotation matrix, as in ba_merge_rule.h.
XTRIF_HD inline double ray_dot(const double* q, const double* t, const double* P, double xn, double yn) {
    XTRIF_NO_CONTRACT
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double M0 = 1.0 - 2.0 * (y * y + z * z), M1 = 2.0 * (x * y - w * z), M2 = 2.0 * (x * z + w * y);
    const double M3 = 2.0 * (x * y + w * z), M4 = 1.0 - 2.0 * (x * x + z * z), M5 = 2.0 * (y * z - w * x);
    const double M6 = 2.0 * (x * z - w * y), M7 = 2.0 * (y * z + w * x), M8 = 1.0 - 2.0 * (x * x + y * y);
    double a0 = M0 * P[0] + M1 * P[1] + M2 * P[2] + t[0];
    double a1 = M3 * P[0] + M4 * P[1] + M5 * P[2] + t[1];
    double a2 = M6 * P[0] + M7 * P[1] + M8 * P[2] + t[2];
    const double s1 = a0 * a0 + a1 * a1 + a2 * a2;
    if (s1 > 0.0) { const double n1 = sqrt(s1); a0 = a0 / n1; a1 = a1 / n1; a2 = a2 / n1; }
    const double n2 = sqrt(xn * xn + yn * yn + 1.0);
    return a0 * (xn / n2) + a1 * (yn / n2) + a2 * (1.0 / n2);
}
// acos(d) is a number (above 1 it is NaN, and a NaN is never the best angle)
XTRIF_HD inline bool dot_valid(double d) { return d >= -1.0 && d <= 1.0; }
// candidate (d, t) against the best so far (bd, bt; bt < 0: none)
XTRIF_HD inline bool better(double d, int32_t t, double bd, int32_t bt) { return bt < 0 || d > bd || (d == bd && t < bt); }
XTRIF_HD inline bool accepts(double d, double dot_min) { return d >= dot_min; }

// the smallest double d of [-1, 1] with acos(d) < th by this host's libm; 2.0 where there is none
inline double dot_bound(double th) {
    if (!(std::acos(1.0) < th)) return 2.0;
    if (std::acos(-1.0) < th) return -1.0;
    double lo = -1.0, hi = 1.0;                       // acos(lo) >= th, acos(hi) < th
    for (int it = 0; it < 4096; ++it) {
        const double mid = lo + (hi - lo) / 2.0;
        if (!(mid > lo && mid < hi)) break;
        if (std::acos(mid) < th) hi = mid; else lo = mid;
    }
    return hi;
}

// ---- check
struct In {
    const Opt* opt;
    int32_t n_frames;
    const int64_t* key_ptr;
    const double* key_xyn;
    const uint8_t* registered;
    const double *cam_q, *cam_t;
    const int64_t* corr_ptr;
    const int32_t* corr_key;
    int32_t n_list;
    const int32_t* frame_list;
    int32_t n_tracks;
    int64_t track_capacity;
    const double* points;
    const uint8_t* track_outlier;
    const int32_t* track_of_key;
};

inline bool finite_all(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// null, or what is wrong (the capacity is checked with the plan); *too_big: a count above INT32_MAX.  frame_of_key [N] is filled.
inline const char* fault(const In& in, std::vector<int32_t>* frame_of_key, bool* too_big) {
    *too_big = false;
    if (!in.opt) return "NULL options";
    const Opt& o = *in.opt;
    const TriOpt& t = o.tri;
    if (!std::isfinite(o.extend_angle_rad) || !std::isfinite(t.min_tri_angle_rad) || !std::isfinite(t.max_error_rad) || !std::isfinite(t.confidence) ||
        !std::isfinite(t.min_inlier_ratio)) return "a non-finite option";
    if (o.extend_angle_rad < 0.0 || o.extend_angle_rad > 3.2) return "extend_angle_rad outside [0, 3.2]";
    if (t.max_error_rad <= 0.0) return "max_error_rad <= 0";
    if (t.confidence < 0.0 || t.confidence > 1.0) return "confidence outside [0, 1]";
    if (t.min_inlier_ratio < 0.0 || t.min_inlier_ratio > 1.0) return "min_inlier_ratio outside [0, 1]";
    if (t.max_num_trials < 1) return "max_num_trials < 1";
    if (t.exhaustive_threshold < 0) return "exhaustive_threshold < 0";
    if (t.min_tri_angle_rad < 0.0) return "min_tri_angle_rad < 0";
    if (in.n_frames < 0 || in.n_tracks < 0 || in.n_list < 0 || in.track_capacity < 0) return "a negative count";
    if (in.track_capacity > 0x7fffffff) { *too_big = true; return "track_capacity above INT32_MAX"; }
    if (in.track_capacity < in.n_tracks) return "track_capacity below n_tracks";
    if (!in.key_ptr) return "NULL key_ptr";
    const int32_t n = in.n_frames, T = in.n_tracks;
    if (in.key_ptr[0] != 0) return "key_ptr does not start at 0";
    for (int32_t f = 0; f < n; ++f) if (in.key_ptr[f + 1] < in.key_ptr[f]) return "key_ptr decreases";
    const int64_t N = in.key_ptr[n];
    if (N > 0x7fffffff) { *too_big = true; return "key points above INT32_MAX"; }
    if (n > 0 && (!in.registered || !in.cam_q || !in.cam_t)) return "NULL frame array";
    if (in.track_capacity > 0 && (!in.points || !in.track_outlier)) return "NULL track array";
    if (N > 0 && (!in.key_xyn || !in.track_of_key || !in.corr_ptr)) return "NULL key point array";
    if (in.n_list > 0 && !in.frame_list) return "NULL frame list";
    {
        std::vector<uint8_t> listed((size_t)n, 0);
        for (int32_t i = 0; i < in.n_list; ++i) {
            const int32_t f = in.frame_list[i];
            if (f < 0 || f >= n) return "a listed frame out of range";
            if (!in.registered[f]) return "a listed frame is not registered";
            if (listed[(size_t)f]) return "a frame is listed twice";
            listed[(size_t)f] = 1;
        }
    }
    if (!finite_all(in.cam_q, 4 * (size_t)n) || !finite_all(in.cam_t, 3 * (size_t)n)) return "a non-finite pose";
    if (!finite_all(in.points, 3 * (size_t)T)) return "a non-finite point";
    if (!finite_all(in.key_xyn, 2 * (size_t)N)) return "a non-finite key point coordinate";
    frame_of_key->assign((size_t)N, 0);
    if (N == 0) return nullptr;
    if (in.corr_ptr[0] != 0) return "corr_ptr does not start at 0";
    for (int64_t k = 0; k < N; ++k) if (in.corr_ptr[k + 1] < in.corr_ptr[k]) return "corr_ptr decreases";
    const int64_t E = in.corr_ptr[N];
    if (E > 0x7fffffff - N) { *too_big = true; return "correspondence entries above INT32_MAX"; }
    if (E > 0 && !in.corr_key) return "NULL corr_key";
    for (int32_t f = 0; f < n; ++f)
        for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k) {
            (*frame_of_key)[(size_t)k] = f;
            const int32_t t2 = in.track_of_key[k];
            if (t2 < -1 || t2 >= T) return "a track index out of range";
            if (t2 >= 0 && in.track_outlier[t2]) return "a key point carries an outlier track";
        }
    const int32_t* fk = frame_of_key->data();
    for (int64_t k = 0; k < N; ++k)
        for (int64_t e = in.corr_ptr[k]; e < in.corr_ptr[k + 1]; ++e) {
            const int32_t b = in.corr_key[e];
            if (b < 0 || b >= N) return "a key point index out of range";
            if (fk[b] == fk[k]) return "a list entry points to the key point's own frame";
        }
    for (int64_t k = 0; k < N; ++k)
        for (int64_t e = in.corr_ptr[k]; e < in.corr_ptr[k + 1]; ++e) {
            const int32_t b = in.corr_key[e];
            bool back = false;
            for (int64_t r = in.corr_ptr[b]; r < in.corr_ptr[b + 1] && !back; ++r) back = in.corr_key[r] == k;
            if (!back) return "a non-symmetric list";
        }
    return nullptr;
}

// ---- plan
// The observation lists depend on `registered` alone, so they are built once for every step.  A slot's list is the registered
// entries of its key point's list in stored order, then the key point itself.
struct Plan {
    std::vector<int32_t> slot_key;             // [n_slots] the key point of a slot; slots in the order they are visited
    std::vector<int32_t> trk_ptr;              // [n_slots + 1] into obs_*
    std::vector<int32_t> obs_cam, obs_key;     // the frame and the key point of an observation
    std::vector<double> obs_xy;                // its normalised coordinates
    std::vector<int32_t> step_slot0;           // [n_steps + 1] the slots of a step (a run of one listed frame)
    std::vector<int32_t> step_frame;           // [n_steps]
    std::vector<uint8_t> status0;              // [N] key_status before the first step: kFewObs where the host can tell, else 0
    int32_t frames_multi = 0;                  // listed frames cut into more than one run
    int32_t max_step = 0;                      // slots of the largest step
    int32_t n_slots() const { return (int32_t)slot_key.size(); }
    int32_t n_steps() const { return (int32_t)step_frame.size(); }
};

inline Plan make_plan(const In& in, const std::vector<int32_t>& frame_of_key) {
    Plan P;
    const int64_t N = in.key_ptr[in.n_frames];
    P.status0.assign((size_t)N, kNotVisited);
    P.trk_ptr.push_back(0);
    P.step_slot0.push_back(0);
    std::vector<int32_t> mark((size_t)N, -1);                 // the step whose run holds a slot with this entry
    for (int32_t i = 0; i < in.n_list; ++i) {
        const int32_t f = in.frame_list[i];
        int32_t runs = 0;
        bool open = false;
        for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k) {
            if (in.track_of_key[k] != -1) continue;
            const size_t o0 = P.obs_key.size();
            for (int64_t e = in.corr_ptr[k]; e < in.corr_ptr[k + 1]; ++e) {
                const int32_t b = in.corr_key[e];
                if (!in.registered[frame_of_key[(size_t)b]]) continue;
                P.obs_key.push_back(b); P.obs_cam.push_back(frame_of_key[(size_t)b]);
            }
            if (P.obs_key.size() == o0) { P.status0[(size_t)k] = kFewObs; continue; }
            P.obs_key.push_back((int32_t)k); P.obs_cam.push_back(f);
            // coupled with a slot of the open run: the run ends before this slot
            bool coupled = false;
            const int32_t step = P.n_steps();
            for (size_t e = o0; e + 1 < P.obs_key.size() && !coupled; ++e) coupled = open && mark[(size_t)P.obs_key[e]] == step;      // (only entries without a track are marked)
            if (coupled) {
                P.step_frame.push_back(f); P.step_slot0.push_back(P.n_slots());
                open = false;
            }
            if (!open) { open = true; ++runs; }
            for (size_t e = o0; e + 1 < P.obs_key.size(); ++e) if (in.track_of_key[P.obs_key[e]] == -1) mark[(size_t)P.obs_key[e]] = P.n_steps();
            P.slot_key.push_back((int32_t)k);
            P.trk_ptr.push_back((int32_t)P.obs_key.size());
        }
        if (open) { P.step_frame.push_back(f); P.step_slot0.push_back(P.n_slots()); }
        P.frames_multi += runs > 1;
    }
    P.obs_xy.resize(2 * P.obs_key.size());
    for (size_t e = 0; e < P.obs_key.size(); ++e) {
        P.obs_xy[2 * e] = in.key_xyn[2 * (size_t)P.obs_key[e]]; P.obs_xy[2 * e + 1] = in.key_xyn[2 * (size_t)P.obs_key[e] + 1];
    }
    for (int32_t s = 0; s < P.n_steps(); ++s) P.max_step = std::max(P.max_step, P.step_slot0[(size_t)s + 1] - P.step_slot0[(size_t)s]);
    return P;
}

// every new track has room: n_tracks and one per slot
inline const char* capacity_fault(const In& in, const Plan& P) {
    return in.track_capacity < (int64_t)in.n_tracks + P.n_slots() ? "track_capacity below n_tracks plus the key points that may create a track" : nullptr;
}

// ---- program
// A slot's branch and, in the extend branch, its candidates: per observation entry the track (or -1) and the dot product.  An entry
// is a candidate when its key point carries a track that no earlier entry of the list carries, the track does not hold the step's
// frame (held[t] == stamp), the dot product is a valid cosine and it meets the threshold: a candidate below the threshold is never
// accepted, and the best of the available ones is below it only if all are, so leaving them out changes no decision.
XTRIF_HD inline int32_t classify_slot(const int32_t* trk_ptr, const int32_t* obs_key, const int32_t* track_of_key, const int32_t* held, int32_t stamp,
                                      const double* q, const double* t, const double* pts_old, const double* pts_new, int32_t n_old, const double* xyn, double dot_min,
                                      int32_t s, int32_t p, int32_t* cand_trk, double* cand_dot) {
    const int32_t b0 = trk_ptr[s], b1 = trk_ptr[s + 1] - 1;            // (the last observation is the key point itself)
    for (int32_t e = b0; e <= b1; ++e) cand_trk[e] = -1;
    if (track_of_key[p] != -1) return kClsNone;
    int32_t distinct = 0;
    for (int32_t e = b0; e < b1; ++e) {
        const int32_t tr = track_of_key[obs_key[e]];
        if (tr < 0) continue;
        bool seen = false;
        for (int32_t r = b0; r < e && !seen; ++r) seen = track_of_key[obs_key[r]] == tr;
        if (seen) continue;
        ++distinct;
        if (held[tr] == stamp) continue;
        const double d = ray_dot(q, t, tr < n_old ? pts_old + 3 * (size_t)tr : pts_new + 3 * (size_t)(tr - n_old), xyn[0], xyn[1]);
        if (!dot_valid(d) || !accepts(d, dot_min)) continue;
        cand_trk[e] = tr; cand_dot[e] = d;
    }
    return distinct == 0 ? kClsCreate : distinct == 1 ? kClsOne : kClsMulti;
}

// the best candidate of a slot that is still available, or -1
XTRIF_HD inline int32_t best_available(const int32_t* trk_ptr, const int32_t* cand_trk, const double* cand_dot, const int32_t* held, int32_t stamp, int32_t s) {
    int32_t bt = -1;
    double bd = 0.0;
    for (int32_t e = trk_ptr[s]; e < trk_ptr[s + 1] - 1; ++e) {
        const int32_t tr = cand_trk[e];
        if (tr < 0 || XTRIF_LOAD(held + tr) == stamp) continue;
        if (better(cand_dot[e], tr, bd, bt)) { bt = tr; bd = cand_dot[e]; }
    }
    return bt;
}

// what a create gives for a slot's list (xrsfm_ba_triangulate_tracks on the list): the program takes it as data
struct Created { const uint8_t* status; const double* points; const uint8_t* mask; };    // [n_slots], [n_slots][3], [n_obs]; status 255: not supplied

struct State {
    std::vector<int32_t> track_of_key;
    std::vector<double> points;               // [capacity][3]
    std::vector<uint8_t> outlier, key_status;
    int32_t n_tracks = 0;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool missing = false;                     // a create result was needed that was not supplied
};

inline State run_host(const In& in, const Plan& P, const Created& cr) {
    State S;
    const int64_t N = in.key_ptr[in.n_frames];
    S.track_of_key.assign(in.track_of_key, in.track_of_key + N);
    S.points.assign(3 * (size_t)in.track_capacity, 0.0);
    S.outlier.assign((size_t)in.track_capacity, 0);
    for (int32_t t = 0; t < in.n_tracks; ++t) { S.outlier[(size_t)t] = in.track_outlier[t]; for (int k = 0; k < 3; ++k) S.points[3 * (size_t)t + k] = in.points[3 * (size_t)t + k]; }
    S.key_status = P.status0;
    S.n_tracks = in.n_tracks;
    const double dot_min = dot_bound(in.opt->extend_angle_rad);
    std::vector<int32_t> held((size_t)in.track_capacity, 0), bid((size_t)in.track_capacity, kNoBid), cls((size_t)P.n_slots(), 0), cand_trk(P.obs_key.size(), -1);
    std::vector<double> cand_dot(P.obs_key.size(), 0.0);
    std::vector<uint8_t> undecided((size_t)P.n_slots(), 0);
    int32_t* tok = S.track_of_key.data();
    for (int32_t step = 0; step < P.n_steps(); ++step) {
        const int32_t f = P.step_frame[(size_t)step], s0 = P.step_slot0[(size_t)step], s1 = P.step_slot0[(size_t)step + 1], stamp = step + 1;
        for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k) if (tok[k] >= 0) held[(size_t)tok[k]] = stamp;
        for (int32_t s = s0; s < s1; ++s) {
            const int32_t p = P.slot_key[(size_t)s];
            cls[(size_t)s] = classify_slot(P.trk_ptr.data(), P.obs_key.data(), tok, held.data(), stamp, in.cam_q + 4 * (size_t)f, in.cam_t + 3 * (size_t)f, S.points.data(),
                                           S.points.data() + 3 * (size_t)in.n_tracks, in.n_tracks, in.key_xyn + 2 * (size_t)p, dot_min, s, p, cand_trk.data(), cand_dot.data());
        }
        // create: ids in key order
        for (int32_t s = s0; s < s1; ++s) {
            const int32_t p = P.slot_key[(size_t)s], c = cls[(size_t)s];
            S.stats[1] += c == kClsCreate; S.stats[3] += c == kClsOne; S.stats[4] += c == kClsMulti;
            undecided[(size_t)s] = c == kClsOne || c == kClsMulti;
            if (c != kClsCreate) continue;
            const int32_t n = P.trk_ptr[(size_t)s + 1] - P.trk_ptr[(size_t)s];
            if (n > kMaxObs) { S.key_status[(size_t)p] = kTooMany; continue; }
            if (cr.status[s] == 255) { S.missing = true; continue; }
            if (cr.status[s] != 1) { S.key_status[(size_t)p] = kNoModel; continue; }
            const int32_t id = S.n_tracks++;
            for (int k = 0; k < 3; ++k) S.points[3 * (size_t)id + k] = cr.points[3 * (size_t)s + k];
            S.outlier[(size_t)id] = 0;
            for (int32_t e = P.trk_ptr[(size_t)s]; e < P.trk_ptr[(size_t)s + 1]; ++e) if (cr.mask[e]) tok[P.obs_key[(size_t)e]] = id;
            S.key_status[(size_t)p] = kCreated; ++S.stats[0];
        }
        // claims: rounds of bids, exactly the kernel's
        int64_t rounds = 0;
        for (int32_t round = 0; round <= s1 - s0; ++round) {
            bool any = false;
            for (int32_t s = s0; s < s1; ++s) {
                if (!undecided[(size_t)s]) continue;
                any = true;
                for (int32_t e = P.trk_ptr[(size_t)s]; e < P.trk_ptr[(size_t)s + 1] - 1; ++e) {
                    const int32_t tr = cand_trk[(size_t)e];
                    if (tr >= 0 && held[(size_t)tr] != stamp) bid[(size_t)tr] = std::min(bid[(size_t)tr], s);
                }
            }
            if (!any) break;
            ++rounds;
            std::vector<int32_t> won;
            for (int32_t s = s0; s < s1; ++s) {
                if (!undecided[(size_t)s]) continue;
                const int32_t bt = best_available(P.trk_ptr.data(), cand_trk.data(), cand_dot.data(), held.data(), stamp, s);
                if (bt < 0) { undecided[(size_t)s] = 0; S.key_status[(size_t)P.slot_key[(size_t)s]] = kNoneAccepted; }
                else if (bid[(size_t)bt] == s) { won.push_back(s); won.push_back(bt); }
            }
            for (int32_t s = s0; s < s1; ++s)
                for (int32_t e = P.trk_ptr[(size_t)s]; e < P.trk_ptr[(size_t)s + 1] - 1; ++e) if (cand_trk[(size_t)e] >= 0) bid[(size_t)cand_trk[(size_t)e]] = kNoBid;
            for (size_t i = 0; i < won.size(); i += 2) {
                const int32_t s = won[i], bt = won[i + 1], p = P.slot_key[(size_t)s];
                undecided[(size_t)s] = 0; held[(size_t)bt] = stamp; tok[p] = bt; S.key_status[(size_t)p] = kExtended; ++S.stats[2];
            }
        }
        S.stats[7] = std::max(S.stats[7], rounds);
    }
    S.stats[5] = P.n_steps(); S.stats[6] = P.frames_multi;
    return S;
}

}  // namespace xtrif
