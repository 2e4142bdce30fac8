// Track completion and merging on the GPU: ContinueTrack, MergeTrack and MergeTracks of the reference
// (src/geometry/track_processor.cc:426-618) over the connected components that ba_merge_rule.h builds on the host.
//
//   k_merge_components   one wave (one 64-thread workgroup) per component.  The component's mutable state lives in LDS for the whole
//                        run: the local track of every key (int16), its frame, a byte of marks per key (the snapshot of the track in
//                        hand, the visited pairs of a continue loop), and per track its point, its size and a byte of marks (visited
//                        by the merge loop in hand, merged away).  The driver loops are the sequential program of run_component();
//                        their control flow is wave-uniform.  The lanes share the scans over the key list by ballot (the next
//                        observation of t beyond a position, whether t has a key in a frame) and the reprojection tests of a merge
//                        (one observation of t or t2 per lane, in chunks of 64, any failure by ballot).  The state is written back
//                        once at the end with plain vector stores; nothing a lane wrote to global memory is read again.  No wave waits
//                        for another; the only global atomics are the four counters.
//                        LDS per wave: 2 KiB tracks + 4 KiB frames + 1 KiB key marks + 12 KiB points + 1 KiB sizes + 0.5 KiB track
//                        marks = 20.5 KiB; one wave per workgroup, so seven workgroups (143.5 KiB) fit the 160 KiB of a compute unit.
//   k_merge_counts       over the final state: one thread per key point (the entries of its list whose key point carries a track) and
//                        one workgroup per frame (its key points with such an entry, its key points that carry a track: the threads
//                        stride over the frame's key points, wave sums, four partials in LDS).  No atomics.
#pragma once
#include <cstdint>

#include "ba_merge_rule.h"

namespace xba {

constexpr int kMergeWave = 64;
constexpr int kMergeCountThreads = 256;

struct MergeArgs {
    const int32_t *key0, *trk0, *seed, *key_glob, *key_frame, *key_trk, *lptr, *lidx, *trk_glob;
    const double *key_xy, *pts_in;
    const xmerge::Cam* cams;
    double max_re;
    int32_t mode;
    int32_t* track_of_key;             // [N] the whole map's, already holding the input: the processed keys are overwritten
    double* pts_out;                   // per plan track
    uint8_t* outlier_out;
    int32_t* counters;                 // [4]
};

struct MergeLds {
    double pts[3 * xmerge::kMaxTracks];
    int32_t frame[xmerge::kMaxKeys];
    int16_t trk[xmerge::kMaxKeys];
    int16_t size[xmerge::kMaxTracks];
    uint8_t key_mark[xmerge::kMaxKeys];        // bit 0: an observation of the snapshot, bit 1: a visited pair
    uint8_t trk_mark[xmerge::kMaxTracks];      // bit 0: visited by the merge loop in hand, bit 1: merged away
};

// track.observations_.count(f) != 0, by all lanes
__device__ __forceinline__ bool merge_has_frame(const MergeLds& s, int nk, int t, int f, int lane) {
    for (int b = 0; b < nk; b += kMergeWave) {
        const int k = b + lane;
        if (__ballot(k < nk && s.trk[k] == t && s.frame[k] == f) != 0) return true;
    }
    return false;
}

// the next observation of t beyond key `pos` (snapshot: the marked keys), or nk
__device__ __forceinline__ int merge_next_observation(const MergeLds& s, int nk, int t, int pos, bool live, int lane) {
    for (int b = (pos + 1) & ~(kMergeWave - 1); b < nk; b += kMergeWave) {
        const int k = b + lane;
        const unsigned long long m = __ballot(k < nk && k > pos && (live ? s.trk[k] == t : (s.key_mark[k] & 1) != 0));
        if (m != 0) return b + (int)__builtin_ctzll(m);
    }
    return nk;
}

// the snapshot of t's observations; clears the visited pairs
__device__ __forceinline__ void merge_snapshot(MergeLds& s, int nk, int nt, int t, int lane) {
    __syncthreads();
    for (int k = lane; k < nk; k += kMergeWave) s.key_mark[k] = s.trk[k] == t ? 1 : 0;
    for (int j = lane; j < nt; j += kMergeWave) s.trk_mark[j] &= 2;
    __syncthreads();
}

__device__ void merge_loop(MergeLds& s, const MergeArgs& a, int k0, int nk, int nt, int t, bool live, int lane, int* counters) {
    merge_snapshot(s, nk, nt, t, lane);
    for (int k = merge_next_observation(s, nk, t, -1, live, lane); k < nk; k = merge_next_observation(s, nk, t, k, live, lane)) {
        const int e1 = a.lptr[k0 + k + 1];
        for (int e = a.lptr[k0 + k]; e < e1; ++e) {
            const int ck = a.lidx[e], cf = s.frame[ck];
            if (merge_has_frame(s, nk, t, cf, lane) || !a.cams[cf].registered) continue;
            const int t2 = s.trk[ck];
            if (t2 < 0 || (s.trk_mark[t2] & 1)) continue;
            __syncthreads();
            if (lane == 0) s.trk_mark[t2] |= 1;
            ++counters[1];
            double m[3];
            xmerge::merged_point((double)s.size[t], s.pts + 3 * t, (double)s.size[t2], s.pts + 3 * t2, m);
            bool failed = false;
            for (int b = 0; b < nk && !failed; b += kMergeWave) {
                const int j = b + lane;
                bool bad = false;
                if (j < nk && (s.trk[j] == t || s.trk[j] == t2))
                    bad = xmerge::merge_rejects(xmerge::reprojection_error(a.cams[s.frame[j]], m, a.key_xy[2 * (size_t)(k0 + j)], a.key_xy[2 * (size_t)(k0 + j) + 1]), a.max_re);
                failed = __ballot(bad) != 0;
            }
            __syncthreads();
            if (failed) continue;
            ++counters[0];
            int moved = 0;
            for (int b = 0; b < nk; b += kMergeWave) {
                const int j = b + lane;
                int act = 0;                           // 1: the key goes to t, 2: t has a key in that frame already
                if (j < nk && s.trk[j] == t2) {
                    const int f = s.frame[j];          // the keys ascend frame-major: the frame's keys are neighbours
                    bool has = false;
                    for (int i = j - 1; i >= 0 && s.frame[i] == f; --i) has |= s.trk[i] == t;
                    for (int i = j + 1; i < nk && s.frame[i] == f; ++i) has |= s.trk[i] == t;
                    act = has ? 2 : 1;
                }
                __syncthreads();
                if (act) s.trk[j] = act == 1 ? (int16_t)t : (int16_t)-1;
                moved += __popcll(__ballot(act == 1));
                __syncthreads();
            }
            if (lane == 0) {
                s.pts[3 * t] = m[0]; s.pts[3 * t + 1] = m[1]; s.pts[3 * t + 2] = m[2];
                s.size[t] = (int16_t)(s.size[t] + moved); s.size[t2] = 0;
                s.trk_mark[t2] |= 2;
            }
            __syncthreads();
        }
    }
}

__device__ void continue_loop(MergeLds& s, const MergeArgs& a, int k0, int nk, int nt, int t, bool live, int lane, int* counters) {
    merge_snapshot(s, nk, nt, t, lane);
    for (int k = merge_next_observation(s, nk, t, -1, live, lane); k < nk; k = merge_next_observation(s, nk, t, k, live, lane)) {
        const int e1 = a.lptr[k0 + k + 1];
        for (int e = a.lptr[k0 + k]; e < e1; ++e) {
            const int ck = a.lidx[e], cf = s.frame[ck];
            if (merge_has_frame(s, nk, t, cf, lane) || !a.cams[cf].registered) continue;
            if (s.trk[ck] >= 0 || (s.key_mark[ck] & 2)) continue;
            ++counters[3];
            const double re = xmerge::reprojection_error(a.cams[cf], s.pts + 3 * t, a.key_xy[2 * (size_t)(k0 + ck)], a.key_xy[2 * (size_t)(k0 + ck) + 1]);
            const bool accept = xmerge::continue_accepts(re, a.max_re, live);
            if (accept) ++counters[2];
            __syncthreads();
            if (lane == 0) {
                s.key_mark[ck] |= 2;
                if (accept) { s.trk[ck] = (int16_t)t; s.size[t] = (int16_t)(s.size[t] + 1); }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kMergeWave) void k_merge_components(const MergeArgs a) {
    __shared__ MergeLds s;
    const int c = blockIdx.x, lane = threadIdx.x;
    const int k0 = a.key0[c], nk = a.key0[c + 1] - k0, t0 = a.trk0[c], nt = a.trk0[c + 1] - t0;
    if (nk > xmerge::kMaxKeys || nt > xmerge::kMaxTracks) return;          // (the host plans no such component)
    for (int j = lane; j < nt; j += kMergeWave) {
        s.size[j] = 0; s.trk_mark[j] = 0;
        for (int q = 0; q < 3; ++q) s.pts[3 * j + q] = a.pts_in[3 * (size_t)(t0 + j) + q];
    }
    for (int k = lane; k < nk; k += kMergeWave) { s.trk[k] = (int16_t)a.key_trk[k0 + k]; s.frame[k] = a.key_frame[k0 + k]; s.key_mark[k] = 0; }
    __syncthreads();
    for (int j = 0; j < nt; ++j) {                     // |t|: the keys that carry it
        int n = 0;
        for (int b = 0; b < nk; b += kMergeWave) n += __popcll(__ballot(b + lane < nk && s.trk[b + lane] == j));
        if (lane == 0) s.size[j] = (int16_t)n;
    }
    __syncthreads();
    int counters[4] = {0, 0, 0, 0};
    if (a.mode == xmerge::kFrame) {
        const int s1 = a.seed[2 * c + 1];
        for (int k = a.seed[2 * c]; k < s1; ++k) {
            const int t = s.trk[k];                    // read live: an earlier seed's merge may have reset it
            if (t < 0) continue;
            merge_loop(s, a, k0, nk, nt, t, true, lane, counters);
            continue_loop(s, a, k0, nk, nt, t, true, lane, counters);
        }
    } else {
        if (a.mode & xmerge::kContinue)
            for (int t = 0; t < nt; ++t) if (!(s.trk_mark[t] & 2)) continue_loop(s, a, k0, nk, nt, t, false, lane, counters);
        if (a.mode & xmerge::kMerge)
            for (int t = 0; t < nt; ++t) if (!(s.trk_mark[t] & 2)) merge_loop(s, a, k0, nk, nt, t, false, lane, counters);
    }
    __syncthreads();
    for (int k = lane; k < nk; k += kMergeWave) a.track_of_key[a.key_glob[k0 + k]] = s.trk[k] < 0 ? -1 : a.trk_glob[t0 + s.trk[k]];
    for (int j = lane; j < nt; j += kMergeWave) {
        for (int q = 0; q < 3; ++q) a.pts_out[3 * (size_t)(t0 + j) + q] = s.pts[3 * j + q];
        a.outlier_out[t0 + j] = (s.trk_mark[j] >> 1) & 1;
    }
    if (lane == 0)
        for (int q = 0; q < 4; ++q) if (counters[q]) atomicAdd(a.counters + q, counters[q]);
}

__global__ __launch_bounds__(kMergeCountThreads) void k_merge_counts(int32_t n_keys, int32_t n_frames, const int32_t* __restrict__ first, const int32_t* __restrict__ corr_ptr,
                                                                   const int32_t* __restrict__ corr_key, const int32_t* __restrict__ track_of_key, int32_t* __restrict__ have,
                                                                   int32_t* __restrict__ visible, int32_t* __restrict__ measured) {
    __shared__ int32_t part[2][kMergeCountThreads / kMergeWave];
    const int key_blocks = (n_keys + kMergeCountThreads - 1) / kMergeCountThreads, tid = threadIdx.x;
    if ((int)blockIdx.x < key_blocks) {            // the first blocks: a thread per key point
        const int64_t i = (int64_t)blockIdx.x * kMergeCountThreads + tid;
        if (i < n_keys) have[i] = xmerge::count_of_key(corr_ptr, corr_key, track_of_key, i);
        return;
    }
    const int f = (int)blockIdx.x - key_blocks;    // the others: a block per frame, its threads stride over the frame's key points
    if (f >= n_frames) return;
    int32_t vis = 0, mea = 0;
    for (int32_t k = first[f] + tid; k < first[f + 1]; k += kMergeCountThreads) {
        bool any = false;
        for (int32_t e = corr_ptr[k]; e < corr_ptr[k + 1] && !any; ++e) any = track_of_key[corr_key[e]] >= 0;
        vis += any; mea += track_of_key[k] >= 0;
    }
    for (int off = kMergeWave / 2; off > 0; off >>= 1) { vis += __shfl_down(vis, off); mea += __shfl_down(mea, off); }
    if ((tid & (kMergeWave - 1)) == 0) { part[0][tid / kMergeWave] = vis; part[1][tid / kMergeWave] = mea; }
    __syncthreads();
    if (tid == 0) {
        int32_t v = 0, m = 0;
        for (int w = 0; w < kMergeCountThreads / kMergeWave; ++w) { v += part[0][w]; m += part[1][w]; }
        visible[f] = v; measured[f] = m;
    }
}

}  // namespace xba
