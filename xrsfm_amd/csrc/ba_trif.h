// Frame triangulation on the GPU: Point3dProcessor::TriangulateFramePoint of the reference
// (reference src/geometry/track_processor.cc:163-251) for a list of frames, on the flat map state of ba_merge.h.  The rules are
// in ba_trif_rule.h; the create arithmetic is k_tri_tracks of ba_tri.h, launched as it stands on the lists that k_trif_select packs.
//
// A step is one run of one listed frame (ba_trif_rule.h: plan).  Its launches, in stream order:
//   k_trif_held      a thread per key point of the frame: the tracks that hold the frame get the step's stamp
//   k_trif_classify  a thread per slot: the distinct tracks among its observations choose its branch; in the extend branch the dot
//                    product of every candidate that may still be accepted
//   k_trif_select    one workgroup: the slots of the create branch, in key order, and their lists packed behind one another
//   k_tri_tracks     the unchanged kernel on the packed lists (waves past the packed ones meet an empty list)
//   k_trif_resolve   one workgroup: new track ids in key order by a prefix sum, the inliers' track_of_key, then the claims
// The claims are rounds inside the one workgroup.  In a round every undecided slot bids its index with an integer atomicMin on each
// of its candidates that is still available; a slot whose best available candidate carries its own bid takes it (no smaller
// undecided slot has that track among its candidates, and the larger ones come after it in the sequential program), a slot without
// an available candidate ends with status 6.  The smallest undecided slot always decides, so a step of n slots ends within n rounds.
// No workgroup waits for another; every loop is bounded; the only atomics are integer; state is written with plain stores.
#pragma once
#include "ba_filter.h"
#include "ba_trif_rule.h"

namespace xba {

constexpr int kTrifThreads = 256;
constexpr int kTrifWave = 64;

struct TrifArgs {
    // the plan
    const CamRec* cams;
    const int32_t *first, *slot_key, *trk_ptr, *obs_cam, *obs_key;
    const double* obs_xy;
    // the state
    const double* pts_old;        // [n_old][3] the points of the tracks before the call
    double* pts_new;              // [n_slots][3] the points of the tracks it creates
    int32_t* track_of_key;
    uint8_t* key_status;
    int32_t *held, *bid;          // [n_old + n_slots]
    int32_t* counters;            // 0..4 the reference's, 7 the most claim rounds, 8 the number of tracks
    // per slot
    int32_t *cls, *undecided, *win, *diag;    // diag [n_slots][3]: num_inliers, num_trials, best_trial
    int32_t* cand_trk;            // [n_obs]
    double* cand_dot;             // [n_obs]
    // the packed lists of the step's create branch and what k_tri_tracks writes for them
    int32_t *c_count, *c_sel, *c_ptr, *c_cam;
    double* c_xy;
    const double* c_pts;
    const uint8_t *c_stat, *c_mask;
    const int32_t *c_ninl, *c_ntr, *c_best;
    int32_t n_old;
    double dot_min;
};

__device__ __forceinline__ int32_t trif_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void trif_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive prefix sum of v over the workgroup and the sum; every thread calls it
__device__ __forceinline__ int trif_block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & (kTrifWave - 1), wv = threadIdx.x / kTrifWave;
    int inc = v;
    for (int off = 1; off < kTrifWave; off <<= 1) { const int u = __shfl_up(inc, off, kTrifWave); if (lane >= off) inc += u; }
    __syncthreads();
    if (lane == kTrifWave - 1) s_wave[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < kTrifThreads / kTrifWave; ++k) { if (k < wv) base += s_wave[k]; total += s_wave[k]; }
    return base + inc - v;
}

__global__ __launch_bounds__(kTrifThreads) void k_trif_held(TrifArgs a, int32_t frame, int32_t stamp) {
    const int32_t k = a.first[frame] + (int32_t)(blockIdx.x * kTrifThreads + threadIdx.x);
    if (k >= a.first[frame + 1]) return;
    const int32_t t = a.track_of_key[k];
    if (t >= 0) a.held[t] = stamp;
}

__global__ __launch_bounds__(kTrifThreads) void k_trif_classify(TrifArgs a, int32_t frame, int32_t stamp, int32_t s0, int32_t s1) {
    const int32_t s = s0 + (int32_t)(blockIdx.x * kTrifThreads + threadIdx.x);
    if (s >= s1) return;
    const int32_t p = a.slot_key[s];
    const CamRec& c = a.cams[frame];
    const double q[4] = {c.q[0], c.q[1], c.q[2], c.q[3]}, t[3] = {c.t[0], c.t[1], c.t[2]};
    const double* xyn = a.obs_xy + 2 * (size_t)(a.trk_ptr[s + 1] - 1);          // the slot's own observation is the last of its list
    const int32_t cls = xtrif::classify_slot(a.trk_ptr, a.obs_key, a.track_of_key, a.held, stamp, q, t, a.pts_old, a.pts_new, a.n_old, xyn, a.dot_min, s, p, a.cand_trk,
                                             a.cand_dot);
    a.cls[s] = cls;
    a.undecided[s] = cls == xtrif::kClsOne || cls == xtrif::kClsMulti;
    if (cls == xtrif::kClsCreate) atomicAdd(a.counters + 1, 1);
    if (cls == xtrif::kClsOne) atomicAdd(a.counters + 3, 1);
    if (cls == xtrif::kClsMulti) atomicAdd(a.counters + 4, 1);
}

__global__ __launch_bounds__(kTrifThreads) void k_trif_select(TrifArgs a, int32_t s0, int32_t s1) {
    __shared__ int s_wave[kTrifThreads / kTrifWave];
    const int tid = threadIdx.x;
    int count = 0, entries = 0;
    for (int32_t b = s0; b < s1; b += kTrifThreads) {
        const int32_t s = b + tid;
        int n = 0;
        bool take = false;
        if (s < s1 && a.cls[s] == xtrif::kClsCreate) {
            n = a.trk_ptr[s + 1] - a.trk_ptr[s];
            take = n <= xtrif::kMaxObs;
            if (!take) a.key_status[a.slot_key[s]] = xtrif::kTooMany;
        }
        int n_take = 0, n_obs = 0;
        const int pos = count + trif_block_scan(take ? 1 : 0, s_wave, n_take);
        const int at = entries + trif_block_scan(take ? n : 0, s_wave, n_obs);
        if (take) {
            a.c_sel[pos] = s; a.c_ptr[pos] = at;
            const int32_t e0 = a.trk_ptr[s];
            for (int k = 0; k < n; ++k) {
                a.c_cam[at + k] = a.obs_cam[e0 + k];
                a.c_xy[2 * (size_t)(at + k)] = a.obs_xy[2 * (size_t)(e0 + k)]; a.c_xy[2 * (size_t)(at + k) + 1] = a.obs_xy[2 * (size_t)(e0 + k) + 1];
            }
        }
        count += n_take; entries += n_obs;
    }
    for (int32_t i = count + tid; i <= s1 - s0; i += kTrifThreads) a.c_ptr[i] = entries;      // the end of the last list; empty lists behind it
    if (tid == 0) *a.c_count = count;
}

__global__ __launch_bounds__(kTrifThreads) void k_trif_resolve(TrifArgs a, int32_t stamp, int32_t s0, int32_t s1) {
    __shared__ int s_wave[kTrifThreads / kTrifWave];
    const int tid = threadIdx.x;
    const int count = *a.c_count, n_tracks = a.counters[8];
    // new track ids in key order; the inlier observations carry the new track
    int created = 0;
    for (int b = 0; b < count; b += kTrifThreads) {
        const int pos = b + tid;
        const bool ok = pos < count && a.c_stat[pos] == 1;
        int n_ok = 0;
        const int id = n_tracks + created + trif_block_scan(ok ? 1 : 0, s_wave, n_ok);
        if (pos < count) {
            const int32_t s = a.c_sel[pos], p = a.slot_key[s];
            a.key_status[p] = ok ? xtrif::kCreated : xtrif::kNoModel;
            a.diag[3 * (size_t)s] = a.c_ninl[pos]; a.diag[3 * (size_t)s + 1] = a.c_ntr[pos]; a.diag[3 * (size_t)s + 2] = a.c_best[pos];
            if (ok) {
                double* P = a.pts_new + 3 * (size_t)(id - a.n_old);
                P[0] = a.c_pts[3 * (size_t)pos]; P[1] = a.c_pts[3 * (size_t)pos + 1]; P[2] = a.c_pts[3 * (size_t)pos + 2];
                const int32_t e0 = a.trk_ptr[s], c0 = a.c_ptr[pos], n = a.trk_ptr[s + 1] - e0;
                for (int k = 0; k < n; ++k) if (a.c_mask[c0 + k]) a.track_of_key[a.obs_key[e0 + k]] = id;
            }
        }
        created += n_ok;
    }
    // the claims
    int rounds = 0, extended = 0;
    for (int round = 0; round <= s1 - s0; ++round) {
        int mine = 0;
        for (int32_t s = s0 + tid; s < s1; s += kTrifThreads) {
            if (!a.undecided[s]) continue;
            mine = 1;
            for (int32_t e = a.trk_ptr[s]; e < a.trk_ptr[s + 1] - 1; ++e) {
                const int32_t tr = a.cand_trk[e];
                if (tr >= 0 && trif_load(a.held + tr) != stamp) atomicMin(a.bid + tr, s);
            }
        }
        if (!__syncthreads_or(mine)) break;
        ++rounds;
        for (int32_t s = s0 + tid; s < s1; s += kTrifThreads) {
            if (!a.undecided[s]) continue;
            const int32_t bt = xtrif::best_available(a.trk_ptr, a.cand_trk, a.cand_dot, a.held, stamp, s);
            a.win[s] = bt < 0 ? -2 : (trif_load(a.bid + bt) == s ? bt : -1);
        }
        __syncthreads();
        for (int32_t s = s0 + tid; s < s1; s += kTrifThreads) {
            if (!a.undecided[s]) continue;
            for (int32_t e = a.trk_ptr[s]; e < a.trk_ptr[s + 1] - 1; ++e) if (a.cand_trk[e] >= 0) trif_store(a.bid + a.cand_trk[e], xtrif::kNoBid);
            const int32_t w = a.win[s], p = a.slot_key[s];
            if (w == -2) { a.undecided[s] = 0; a.key_status[p] = xtrif::kNoneAccepted; }
            else if (w >= 0) { a.undecided[s] = 0; trif_store(a.held + w, stamp); a.track_of_key[p] = w; a.key_status[p] = xtrif::kExtended; ++extended; }
        }
        __syncthreads();
    }
    if (extended) atomicAdd(a.counters + 2, extended);
    if (tid == 0) {
        a.counters[0] += created; a.counters[8] = n_tracks + created;
        if (rounds > a.counters[7]) a.counters[7] = rounds;
    }
}

}  // namespace xba
