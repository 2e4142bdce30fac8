// The host-side rules of track completion and merging (ba_merge.h): what Point3dProcessor::ContinueTrack, MergeTrack
// and MergeTracks of the reference decide (src/geometry/track_processor.cc:426-618), restated on three flat arrays (the track of every
// key point, the point and the outlier flag of every track).  Plain C++: tests/merge_host_driver.py compiles this file alone, with
// the address and undefined-behaviour sanitizers.
//
//   error     Reprojection_Error (track_processor.cc:19-26) and the candidate point of a merge, shared with the kernel
//   check     what is wrong with a call's arguments
//   plan      the connected components (key points; edges: correspondence entries and "same track"), largest first, and for every
//             component that is processed its keys ascending, its lists with local indices, its tracks ascending and its seeds
//   program   the three driver loops as plain loops over a component's local arrays (the stand-alone program and the timing tool
//             run them; the library runs k_merge_components), and the counts that follow from the final state
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#ifdef __HIPCC__
#define XMERGE_HD __host__ __device__
#else
#define XMERGE_HD
#endif
// the comparisons are made on values rounded once per operation, on the host and on the device alike
#if defined(__clang__)
#define XMERGE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define XMERGE_NO_CONTRACT
#endif

namespace xmerge {

constexpr int32_t kMaxKeys = 1024;            // XRSFM_BA_MERGE_MAX_KEYS: key points of a component k_merge_components attempts
constexpr int32_t kMaxTracks = 512;           // XRSFM_BA_MERGE_MAX_TRACKS
constexpr int32_t kContinue = 1, kMerge = 2, kFrame = 4;

struct Opt { double max_reproj_error; int32_t mode, frame; };          // xrsfm_ba_merge_options, field for field
inline Opt default_options() { return Opt{8.0, kContinue | kMerge, -1}; }

struct Cam { double q[4], t[3], k[8]; int32_t model, registered; };    // a frame: pose (x, y, z, w; t), its camera's parameters

// ---- error
// q * X + t by the rotation matrix, hnormalized() without a depth test, NormalizedToImage (the pinhole models add the
// undistorted point to itself: du = xn), the norm of the residual: the arithmetic of k_filter_tracks up to `re`.
XMERGE_HD inline double reprojection_error(const Cam& c, const double* P, double u, double v) {
    XMERGE_NO_CONTRACT
    const double x = c.q[0], y = c.q[1], z = c.q[2], w = c.q[3];
    const double M0 = 1.0 - 2.0 * (y * y + z * z), M1 = 2.0 * (x * y - w * z), M2 = 2.0 * (x * z + w * y);
    const double M3 = 2.0 * (x * y + w * z), M4 = 1.0 - 2.0 * (x * x + z * z), M5 = 2.0 * (y * z - w * x);
    const double M6 = 2.0 * (x * z - w * y), M7 = 2.0 * (y * z + w * x), M8 = 1.0 - 2.0 * (x * x + y * y);
    const double X = M0 * P[0] + M1 * P[1] + M2 * P[2] + c.t[0];
    const double Y = M3 * P[0] + M4 * P[1] + M5 * P[2] + c.t[1];
    const double Z = M6 * P[0] + M7 * P[1] + M8 * P[2] + c.t[2];
    const double xn = X / Z, yn = Y / Z, r2 = xn * xn + yn * yn;
    const double* k = c.k;
    double fx, fy, cx, cy, du, dv;
    switch (c.model) {
    case 0: fx = k[0]; fy = k[0]; cx = k[1]; cy = k[2]; du = xn; dv = yn; break;
    case 1: fx = k[0]; fy = k[1]; cx = k[2]; cy = k[3]; du = xn; dv = yn; break;
    case 2: fx = k[0]; fy = k[0]; cx = k[1]; cy = k[2]; du = xn * (k[3] * r2); dv = yn * (k[3] * r2); break;
    case 3: fx = k[0]; fy = k[1]; cx = k[2]; cy = k[3]; du = xn * (k[4] * r2); dv = yn * (k[4] * r2); break;
    default: {
        fx = k[0]; fy = k[1]; cx = k[2]; cy = k[3];
        const double rad = k[4] * r2 + k[5] * r2 * r2, xy = xn * yn;
        du = xn * rad + 2.0 * k[6] * xy + k[7] * (r2 + 2.0 * xn * xn);
        dv = yn * rad + 2.0 * k[7] * xy + k[6] * (r2 + 2.0 * yn * yn);
    } }
    const double e0 = fx * (xn + du) + cx - u, e1 = fy * (yn + dv) + cy - v;
    return sqrt(e0 * e0 + e1 * e1);
}

// (w1 * P1 + w2 * P2) / (w1 + w2)
XMERGE_HD inline void merged_point(double w1, const double* P1, double w2, const double* P2, double* m) {
    XMERGE_NO_CONTRACT
    const double s = w1 + w2;
    for (int k = 0; k < 3; ++k) m[k] = (w1 * P1[k] + w2 * P2[k]) / s;
}

// the three comparison forms, as written (a NaN passes the first two and fails the third)
XMERGE_HD inline bool merge_rejects(double re, double max_re) { return re > max_re; }
XMERGE_HD inline bool continue_accepts(double re, double max_re, bool frame_mode) { return frame_mode ? re < max_re : !(re > max_re); }

// ---- check
struct In {
    const Opt* opt;
    int32_t n_frames;
    const int64_t* key_ptr;
    const double* key_xy;
    const uint8_t* registered;
    const double *cam_q, *cam_t;
    const int32_t* cam_intr;
    int32_t n_intr;
    const int32_t* intr_model;
    const double* intr_params;
    const int64_t* corr_ptr;
    const int32_t* corr_key;
    int32_t n_tracks;
    const double* points;
    const uint8_t* track_outlier;
    const int32_t* track_of_key;
};

inline bool finite_all(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// null, or what is wrong; *too_big: the fault is a count above INT32_MAX.  frame_of_key [N] is filled on the way.
inline const char* fault(const In& in, std::vector<int32_t>* frame_of_key, bool* too_big) {
    *too_big = false;
    if (!in.opt) return "NULL options";
    const Opt& o = *in.opt;
    if (!(o.max_reproj_error > 0.0) || !std::isfinite(o.max_reproj_error)) return "max_reproj_error not positive";
    if (o.mode != 1 && o.mode != 2 && o.mode != 3 && o.mode != 4) return "mode outside {1, 2, 3, 4}";
    if (in.n_frames < 0 || in.n_tracks < 0 || in.n_intr < 0) return "a negative count";
    if (!in.key_ptr) return "NULL key_ptr";
    const int32_t n = in.n_frames, T = in.n_tracks;
    if (in.key_ptr[0] != 0) return "key_ptr does not start at 0";
    for (int32_t f = 0; f < n; ++f) if (in.key_ptr[f + 1] < in.key_ptr[f]) return "key_ptr decreases";
    const int64_t N = in.key_ptr[n];
    if (N > 0x7fffffff) { *too_big = true; return "key points above INT32_MAX"; }
    if (n > 0 && (!in.registered || !in.cam_q || !in.cam_t || !in.cam_intr)) return "NULL frame array";
    if (in.n_intr > 0 && (!in.intr_model || !in.intr_params)) return "NULL camera array";
    if (T > 0 && (!in.points || !in.track_outlier)) return "NULL track array";
    if (N > 0 && (!in.key_xy || !in.track_of_key || !in.corr_ptr)) return "NULL key point array";
    if (o.mode == kFrame && (o.frame < 0 || o.frame >= n)) return "frame out of range";
    if (o.mode == kFrame && !in.registered[o.frame]) return "frame not registered";
    for (int32_t f = 0; f < n; ++f) if (in.cam_intr[f] < 0 || in.cam_intr[f] >= in.n_intr) return "a camera index out of range";
    for (int32_t c = 0; c < in.n_intr; ++c) if (in.intr_model[c] < 0 || in.intr_model[c] > 4) return "a camera model outside 0..4";
    if (!finite_all(in.cam_q, 4 * (size_t)n) || !finite_all(in.cam_t, 3 * (size_t)n)) return "a non-finite pose";
    if (!finite_all(in.intr_params, 8 * (size_t)in.n_intr)) return "a non-finite camera parameter";
    if (!finite_all(in.points, 3 * (size_t)T)) return "a non-finite point";
    if (!finite_all(in.key_xy, 2 * (size_t)N)) return "a non-finite key point coordinate";
    frame_of_key->assign((size_t)N, 0);
    if (N == 0) return nullptr;
    if (in.corr_ptr[0] != 0) return "corr_ptr does not start at 0";
    for (int64_t k = 0; k < N; ++k) if (in.corr_ptr[k + 1] < in.corr_ptr[k]) return "corr_ptr decreases";
    const int64_t E = in.corr_ptr[N];
    if (E > 0x7fffffff) { *too_big = true; return "correspondence entries above INT32_MAX"; }
    if (E > 0 && !in.corr_key) return "NULL corr_key";
    std::vector<int32_t> last((size_t)T, -1);                 // the last frame in which a track was seen
    for (int32_t f = 0; f < n; ++f)
        for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k) {
            (*frame_of_key)[(size_t)k] = f;
            const int32_t t = in.track_of_key[k];
            if (t < -1 || t >= T) return "a track index out of range";
            if (t < 0) continue;
            if (in.track_outlier[t]) return "a key point carries an outlier track";
            if (last[(size_t)t] == f) return "two key points of one frame on one track";
            last[(size_t)t] = f;
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

inline Cam cam_of(const In& in, int32_t f) {
    Cam c;
    const int32_t ci = in.cam_intr[f];
    for (int k = 0; k < 4; ++k) c.q[k] = in.cam_q[4 * (size_t)f + k];
    for (int k = 0; k < 3; ++k) c.t[k] = in.cam_t[3 * (size_t)f + k];
    for (int k = 0; k < 8; ++k) c.k[k] = in.intr_params[8 * (size_t)ci + k];
    c.model = in.intr_model[ci]; c.registered = in.registered[f] ? 1 : 0;
    return c;
}

// ---- plan
struct Labels {
    std::vector<int32_t> comp_of_key;          // [N]: the component of every key point, components by size (largest first, then first key)
    std::vector<int32_t> size, first;          // per component: its key points, its first key point
};

inline Labels label_components(const In& in) {
    const int64_t N = in.key_ptr[in.n_frames];
    std::vector<int32_t> parent((size_t)N);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t a) {
        while (parent[(size_t)a] != a) { parent[(size_t)a] = parent[(size_t)parent[(size_t)a]]; a = parent[(size_t)a]; }
        return a;
    };
    auto join = [&](int32_t a, int32_t b) {          // the smaller index is the root: a root is its component's first key point
        a = find(a); b = find(b);
        if (a < b) parent[(size_t)b] = a; else parent[(size_t)a] = b;
    };
    std::vector<int32_t> seen((size_t)in.n_tracks, -1);
    for (int64_t k = 0; k < N; ++k) {
        for (int64_t e = in.corr_ptr[k]; e < in.corr_ptr[k + 1]; ++e) join((int32_t)k, in.corr_key[e]);
        const int32_t t = in.track_of_key[k];
        if (t >= 0) { if (seen[(size_t)t] < 0) seen[(size_t)t] = (int32_t)k; else join((int32_t)k, seen[(size_t)t]); }
    }
    std::vector<int32_t> count((size_t)N, 0), roots;
    for (int64_t k = 0; k < N; ++k) { const int32_t r = find((int32_t)k); if (count[(size_t)r]++ == 0) roots.push_back(r); }
    std::stable_sort(roots.begin(), roots.end(), [&](int32_t a, int32_t b) { return count[(size_t)a] > count[(size_t)b]; });     // (roots ascending before)
    std::vector<int32_t> id((size_t)N, -1);
    Labels L;
    for (size_t c = 0; c < roots.size(); ++c) { id[(size_t)roots[c]] = (int32_t)c; L.size.push_back(count[(size_t)roots[c]]); L.first.push_back(roots[c]); }
    L.comp_of_key.resize((size_t)N);
    for (int64_t k = 0; k < N; ++k) L.comp_of_key[(size_t)k] = id[(size_t)find((int32_t)k)];
    return L;
}

// The processed components behind one another.  A component is processed when it holds a track (frame mode: a key point of the
// frame that carries one) and is within the limits; local indices count inside a component.
struct Plan {
    int32_t n_comp = 0, n_skipped = 0, largest = 0;
    std::vector<int32_t> key0, trk0;           // [n_comp + 1]: first key / track of a component in the arrays below
    std::vector<int32_t> seed;                 // [n_comp][2]: the local keys [s0, s1) of the frame (frame mode; 0, 0 otherwise)
    std::vector<int32_t> key_glob, key_frame, key_trk;   // per key: its global index, its frame, its local track or -1
    std::vector<double> key_xy;                // [keys][2]
    std::vector<int32_t> lptr, lidx;           // per key its list: entries lptr[k] .. lptr[k + 1] of lidx, local key indices
    std::vector<int32_t> trk_glob;             // per local track its global index
    std::vector<int32_t> skipped_tracks;       // the tracks of the components above a limit
};

inline Plan make_plan(const In& in, const std::vector<int32_t>& frame_of_key, const Labels& L) {
    Plan P;
    const int64_t N = in.key_ptr[in.n_frames];
    const size_t C = L.size.size();
    // a component's keys ascending: a counting sort by component
    std::vector<int64_t> start(C + 1, 0);
    for (size_t c = 0; c < C; ++c) start[c + 1] = start[c] + L.size[c];
    std::vector<int32_t> keys((size_t)N), local((size_t)N);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t k = 0; k < N; ++k) { const int32_t c = L.comp_of_key[(size_t)k]; local[(size_t)k] = (int32_t)(at[(size_t)c] - start[(size_t)c]); keys[(size_t)at[(size_t)c]++] = (int32_t)k; }
    }
    const bool frame_mode = in.opt->mode == kFrame;
    std::vector<int32_t> ltrk((size_t)in.n_tracks, -1);
    P.key0.push_back(0); P.trk0.push_back(0); P.lptr.push_back(0);
    if (!frame_mode) {                         // (most of a map is processed; a frame's components are a small part of it)
        for (std::vector<int32_t>* v : {&P.key_glob, &P.key_frame, &P.key_trk, &P.lptr}) v->reserve((size_t)N + 1);
        P.key_xy.reserve(2 * (size_t)N); P.lidx.reserve((size_t)in.corr_ptr[N]); P.trk_glob.reserve((size_t)in.n_tracks);
    }
    std::vector<int32_t> tracks;
    for (size_t c = 0; c < C; ++c) {
        const int32_t* ck = keys.data() + start[c];
        const int32_t nk = L.size[c];
        tracks.clear();
        bool wanted = false;
        for (int32_t i = 0; i < nk; ++i) {
            const int32_t t = in.track_of_key[ck[i]];
            if (t < 0) continue;
            tracks.push_back(t);
            if (!frame_mode || frame_of_key[(size_t)ck[i]] == in.opt->frame) wanted = true;
        }
        if (!wanted) continue;
        std::sort(tracks.begin(), tracks.end());
        tracks.erase(std::unique(tracks.begin(), tracks.end()), tracks.end());
        if (nk > kMaxKeys || (int32_t)tracks.size() > kMaxTracks) {
            ++P.n_skipped;
            P.skipped_tracks.insert(P.skipped_tracks.end(), tracks.begin(), tracks.end());
            continue;
        }
        for (size_t j = 0; j < tracks.size(); ++j) ltrk[(size_t)tracks[j]] = (int32_t)j;
        int32_t s0 = 0, s1 = 0;
        for (int32_t i = 0; i < nk; ++i) {
            const int32_t g = ck[i], f = frame_of_key[(size_t)g];
            P.key_glob.push_back(g); P.key_frame.push_back(f);
            P.key_trk.push_back(in.track_of_key[g] < 0 ? -1 : ltrk[(size_t)in.track_of_key[g]]);
            P.key_xy.push_back(in.key_xy[2 * (size_t)g]); P.key_xy.push_back(in.key_xy[2 * (size_t)g + 1]);
            for (int64_t e = in.corr_ptr[g]; e < in.corr_ptr[g + 1]; ++e) P.lidx.push_back(local[(size_t)in.corr_key[e]]);
            P.lptr.push_back((int32_t)P.lidx.size());
            if (frame_mode && f < in.opt->frame) s0 = i + 1;
            if (frame_mode && f <= in.opt->frame) s1 = i + 1;
        }
        P.seed.push_back(s0); P.seed.push_back(s1);
        P.trk_glob.insert(P.trk_glob.end(), tracks.begin(), tracks.end());
        P.key0.push_back((int32_t)P.key_glob.size()); P.trk0.push_back((int32_t)P.trk_glob.size());
        ++P.n_comp;
        P.largest = std::max(P.largest, nk);
    }
    return P;
}

// ---- program
// The state of the processed components, in the plan's order: what k_merge_components keeps in LDS and writes back.
struct State {
    std::vector<int32_t> key_trk;              // per key: local track or -1
    std::vector<double> pts;                   // [tracks][3]
    std::vector<uint8_t> outlier;              // per track: merged away
    int64_t counters[4] = {0, 0, 0, 0};        // merged / connected tracks, continued / connected measurements
};

inline State initial_state(const In& in, const Plan& P) {
    State S;
    S.key_trk = P.key_trk;
    S.pts.resize(3 * P.trk_glob.size());
    for (size_t j = 0; j < P.trk_glob.size(); ++j) for (int k = 0; k < 3; ++k) S.pts[3 * j + k] = in.points[3 * (size_t)P.trk_glob[j] + k];
    S.outlier.assign(P.trk_glob.size(), 0);
    return S;
}

struct Comp {                                  // one component's arrays (local indices)
    int32_t nk, nt, s0, s1;
    const int32_t *frame, *lptr, *lidx;        // lptr holds offsets into the plan's lidx; lidx local key indices
    const double* xy;
    int32_t* trk;                              // state
    double* pts;
    uint8_t* outlier;
};

inline Comp component(const Plan& P, State& S, int32_t c) {
    const int32_t k0 = P.key0[(size_t)c], t0 = P.trk0[(size_t)c];
    return Comp{P.key0[(size_t)c + 1] - k0, P.trk0[(size_t)c + 1] - t0, P.seed[2 * (size_t)c], P.seed[2 * (size_t)c + 1], P.key_frame.data() + k0, P.lptr.data() + k0,
                P.lidx.data(), P.key_xy.data() + 2 * (size_t)k0, S.key_trk.data() + k0, S.pts.data() + 3 * (size_t)t0, S.outlier.data() + t0};
}

struct Scratch { std::vector<int32_t> size; std::vector<uint8_t> snap, key_mark, trk_mark; };

inline bool has_frame(const Comp& c, int32_t t, int32_t f) {          // track.observations_.count(f) != 0
    for (int32_t k = 0; k < c.nk; ++k) if (c.trk[k] == t && c.frame[k] == f) return true;
    return false;
}

// the next observation of t beyond local key `pos` (the keys ascend frame-major: std::map order), or nk
inline int32_t next_observation(const Comp& c, int32_t t, int32_t pos, const uint8_t* snap) {
    for (int32_t k = pos + 1; k < c.nk; ++k) if (snap ? snap[k] != 0 : c.trk[k] == t) return k;
    return c.nk;
}

// MergeTrack (snapshot) / the first loop of MergeTracks (live)
inline void merge_loop(const Comp& c, const Cam* cams, double max_re, int32_t t, bool live, Scratch& W, int64_t* counters) {
    std::fill(W.trk_mark.begin(), W.trk_mark.end(), 0);
    for (int32_t k = 0; k < c.nk; ++k) W.snap[(size_t)k] = c.trk[k] == t;
    for (int32_t k = next_observation(c, t, -1, live ? nullptr : W.snap.data()); k < c.nk; k = next_observation(c, t, k, live ? nullptr : W.snap.data()))
        for (int32_t e = c.lptr[k]; e < c.lptr[k + 1]; ++e) {
            const int32_t ck = c.lidx[e], cf = c.frame[ck];
            if (has_frame(c, t, cf) || !cams[cf].registered) continue;
            const int32_t t2 = c.trk[ck];
            if (t2 < 0 || W.trk_mark[(size_t)t2]) continue;
            W.trk_mark[(size_t)t2] = 1;
            ++counters[1];
            double m[3];
            merged_point((double)W.size[(size_t)t], c.pts + 3 * (size_t)t, (double)W.size[(size_t)t2], c.pts + 3 * (size_t)t2, m);
            bool ok = true;
            for (int32_t j = 0; j < c.nk && ok; ++j)
                if (c.trk[j] == t || c.trk[j] == t2) ok = !merge_rejects(reprojection_error(cams[c.frame[j]], m, c.xy[2 * (size_t)j], c.xy[2 * (size_t)j + 1]), max_re);
            if (!ok) continue;
            ++counters[0];
            for (int q = 0; q < 3; ++q) c.pts[3 * (size_t)t + q] = m[q];
            for (int32_t j = 0; j < c.nk; ++j) {
                if (c.trk[j] != t2) continue;
                if (has_frame(c, t, c.frame[j])) c.trk[j] = -1; else { c.trk[j] = t; ++W.size[(size_t)t]; }
            }
            W.size[(size_t)t2] = 0;
            c.outlier[t2] = 1;
        }
}

// ContinueTrack (snapshot, rejects on re > max) / the second loop of MergeTracks (live, accepts on re < max)
inline void continue_loop(const Comp& c, const Cam* cams, double max_re, int32_t t, bool live, Scratch& W, int64_t* counters) {
    std::fill(W.key_mark.begin(), W.key_mark.end(), 0);
    for (int32_t k = 0; k < c.nk; ++k) W.snap[(size_t)k] = c.trk[k] == t;
    for (int32_t k = next_observation(c, t, -1, live ? nullptr : W.snap.data()); k < c.nk; k = next_observation(c, t, k, live ? nullptr : W.snap.data()))
        for (int32_t e = c.lptr[k]; e < c.lptr[k + 1]; ++e) {
            const int32_t ck = c.lidx[e], cf = c.frame[ck];
            if (has_frame(c, t, cf) || !cams[cf].registered) continue;
            if (c.trk[ck] >= 0 || W.key_mark[(size_t)ck]) continue;
            W.key_mark[(size_t)ck] = 1;
            ++counters[3];
            const double re = reprojection_error(cams[cf], c.pts + 3 * (size_t)t, c.xy[2 * (size_t)ck], c.xy[2 * (size_t)ck + 1]);
            if (!continue_accepts(re, max_re, live)) continue;
            ++counters[2];
            c.trk[ck] = t; ++W.size[(size_t)t];
        }
}

// one component, the reference's own sequential program
inline void run_component(const Comp& c, const Cam* cams, const Opt& o, int64_t* counters) {
    Scratch W;
    W.size.assign((size_t)c.nt, 0); W.snap.assign((size_t)c.nk, 0); W.key_mark.assign((size_t)c.nk, 0); W.trk_mark.assign((size_t)c.nt, 0);
    for (int32_t k = 0; k < c.nk; ++k) if (c.trk[k] >= 0) ++W.size[(size_t)c.trk[k]];
    if (o.mode == kFrame) {
        for (int32_t k = c.s0; k < c.s1; ++k) {
            const int32_t t = c.trk[k];            // read live: an earlier seed's merge may have reset it
            if (t < 0) continue;
            merge_loop(c, cams, o.max_reproj_error, t, true, W, counters);
            continue_loop(c, cams, o.max_reproj_error, t, true, W, counters);
        }
        return;
    }
    if (o.mode & kContinue) for (int32_t t = 0; t < c.nt; ++t) if (!c.outlier[t]) continue_loop(c, cams, o.max_reproj_error, t, false, W, counters);
    if (o.mode & kMerge) for (int32_t t = 0; t < c.nt; ++t) if (!c.outlier[t]) merge_loop(c, cams, o.max_reproj_error, t, false, W, counters);
}

inline void run_host(const Plan& P, const Cam* cams, const Opt& o, State* S) {
    for (int32_t c = 0; c < P.n_comp; ++c) run_component(component(P, *S, c), cams, o, S->counters);
}

// the state's arrays after a run: the caller's three arrays and the status of every track
inline void scatter(const Plan& P, const int32_t* key_trk, const double* pts, const uint8_t* outlier, double* points, uint8_t* track_outlier, int32_t* track_of_key,
                    uint8_t* track_status) {
    for (int32_t c = 0; c < P.n_comp; ++c) {
        const int32_t t0 = P.trk0[(size_t)c];
        for (int32_t k = P.key0[(size_t)c]; k < P.key0[(size_t)c + 1]; ++k) track_of_key[P.key_glob[(size_t)k]] = key_trk[k] < 0 ? -1 : P.trk_glob[(size_t)(t0 + key_trk[k])];
    }
    for (size_t j = 0; j < P.trk_glob.size(); ++j) {
        const int32_t g = P.trk_glob[j];
        for (int q = 0; q < 3; ++q) points[3 * (size_t)g + q] = pts[3 * j + q];
        if (outlier[j]) track_outlier[g] = 1;
        if (track_status) track_status[g] = outlier[j] ? 2 : 1;
    }
    if (track_status) for (int32_t g : P.skipped_tracks) track_status[g] = 3;
}

// num_correspondences_have_point3D_ of every key point; per frame num_visible_points3D_ and the key points that carry a track
template <typename Offset> XMERGE_HD inline int32_t count_of_key(const Offset* corr_ptr, const int32_t* corr_key, const int32_t* track_of_key, int64_t k) {
    int32_t n = 0;
    for (Offset e = corr_ptr[k]; e < corr_ptr[k + 1]; ++e) n += track_of_key[corr_key[e]] >= 0;
    return n;
}

inline void counts_host(const In& in, const int32_t* track_of_key, int32_t* have, int32_t* visible, int32_t* measured) {
    for (int32_t f = 0; f < in.n_frames; ++f) {
        int32_t vis = 0, mea = 0;
        for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k) {
            const int32_t n = count_of_key(in.corr_ptr, in.corr_key, track_of_key, k);
            if (have) have[k] = n;
            vis += n > 0; mea += track_of_key[k] >= 0;
        }
        if (visible) visible[f] = vis;
        if (measured) measured[f] = mea;
    }
}

}  // namespace xmerge
