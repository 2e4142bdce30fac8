// Match expansion on the device: the item-parallel phases of MatchExpansionSolver::Run.  The rules of one item are in
// ba_expand_rule.h; AddTrack is order-dependent and stays on the host (xexpand::make_tracks).
//
// k_expand_patch    one thread per key point: its frame (binary search in the frames' first key points) and its patch byte.  A key
//                   point the reference would index out of its patches raises the error word and gets patch 0.
// k_expand_count / k_expand_fill   the correspondence lists as a CSR over the key points of the set: a count per key point, an
//                   exclusive scan between the two launches, a fill through a per-key-point cursor.  The order inside a list is
//                   that of the atomics and never reaches an output: a key point fires when ANY entry lies in a registered frame
//                   and then marks ALL entries, both symmetric in the list's entries.
// k_expand_select   one thread per frame: an unregistered frame with min_visible marks registers and joins the round's work list
//                   (its position there is that of an atomic and decides nothing).
// k_expand_fire     blockIdx.y: a frame of the work list; a thread per key point.  A firing key point ORs the mark word of every
//                   entry and raises the entry's frame only when the OR returns 0.  The flags it reads were written by the launch
//                   before; marks are never read by the firing rule.  Integer atomics only: the counts are order-free.
// k_expand_covis    one workgroup per connected frame i.  LDS: a bit per frame "paired with i, or i itself", and for a window of W
//                   third frames two sets of 128 bits each, "seen once" and "seen twice".  Every observation (t, m) of the valid
//                   tracks of i's key points with t in the window and not paired ORs its bit in the first set and, when the OR
//                   returns the bit set, in the second.  After a barrier the wanted set is compacted: every thread counts the bits
//                   of its run of words, an exclusive scan over the 256 counts gives its offset, and it writes its codes
//                   t * patches + patch, which ascend by construction (word order is frame order, bit order is patch order,
//                   windows ascend).  The codes go to the frame's own room (the host knows items / min_patch_obs bounds them), the
//                   count beside them: no global atomic.  More frames than W: several passes over the items.
// k_expand_pairs    one wave per directed candidate (id1, id2): lanes stride over id1's key points and binary-search id2 in the
//                   frame-sorted observations of the key point's valid track (GetMatcheNum); then the shorter code list is searched
//                   in the longer; two wave reductions.
//
// No floating-point arithmetic beyond the conversion in the patch rule; nothing waits for another workgroup.
#pragma once
#include <cstdint>

#include "ba_expand_rule.h"

namespace xba {

constexpr int kExpandThreads = 256;
constexpr int kExpandWave = 64;
constexpr int kExpandLdsBytes = 160 * 1024 - 2048;          // dynamic LDS of k_expand_covis at most: the CU's 160 KiB less its static arrays and slack

__global__ __launch_bounds__(kExpandThreads) void k_expand_patch(int32_t n_frames, int32_t n_keys, const int32_t* __restrict__ first, const int2* __restrict__ size,
                                                                 const float4* __restrict__ keys, int32_t cols, int32_t rows, uint8_t* __restrict__ patch,
                                                                 int32_t* __restrict__ key_frame, int32_t* __restrict__ err) {
    const int32_t k = (int32_t)(blockIdx.x * kExpandThreads + threadIdx.x);
    if (k >= n_keys) return;
    const int32_t f = xexpand::frame_of(first, n_frames, k);
    const float4 key = keys[k];
    const int2 wh = size[f];
    int32_t p = xexpand::patch_of(key.x, key.y, wh.x, wh.y, cols, rows);
    if (p < 0) { atomicOr(err, 1); p = 0; }
    patch[k] = (uint8_t)p;
    key_frame[k] = f;
}

__global__ __launch_bounds__(kExpandThreads) void k_expand_count(int64_t n_matches, const int2* __restrict__ mkeys, int32_t* __restrict__ count) {
    const int64_t m = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x;
    if (m >= n_matches) return;
    const int2 mk = mkeys[m];
    atomicAdd(&count[mk.x], 1);
    atomicAdd(&count[mk.y], 1);
}

__global__ __launch_bounds__(kExpandThreads) void k_expand_fill(int64_t n_matches, const int2* __restrict__ mkeys, const int32_t* __restrict__ ptr, int32_t* __restrict__ cursor,
                                                                int32_t* __restrict__ ent) {
    const int64_t m = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x;
    if (m >= n_matches) return;
    const int2 mk = mkeys[m];
    ent[ptr[mk.x] + atomicAdd(&cursor[mk.x], 1)] = mk.y;
    ent[ptr[mk.y] + atomicAdd(&cursor[mk.y], 1)] = mk.x;
}

__global__ __launch_bounds__(kExpandThreads) void k_expand_select(int32_t n_frames, int32_t min_visible, const int32_t* __restrict__ visible, uint8_t* __restrict__ registered,
                                                                  int32_t* __restrict__ work, int32_t* __restrict__ n_new) {
    const int32_t f = (int32_t)(blockIdx.x * kExpandThreads + threadIdx.x);
    if (f >= n_frames || registered[f] || visible[f] < min_visible) return;
    registered[f] = 1;
    work[atomicAdd(n_new, 1)] = f;
}

__global__ __launch_bounds__(kExpandThreads) void k_expand_fire(const int32_t* __restrict__ work, const int32_t* __restrict__ first, const int32_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ ent, const int32_t* __restrict__ key_frame, const uint8_t* __restrict__ registered,
                                                                int32_t* __restrict__ mark, int32_t* __restrict__ visible) {
    const int32_t f = work[blockIdx.y];
    const int32_t k = first[f] + (int32_t)(blockIdx.x * kExpandThreads + threadIdx.x);
    if (k >= first[f + 1]) return;
    const int32_t beg = ptr[k], len = ptr[k + 1] - beg;
    if (!xexpand::fires(ent + beg, len, key_frame, registered)) return;
    for (int32_t e = 0; e < len; ++e) {
        const int32_t m = ent[beg + e];
        if (atomicOr(&mark[m], 1) == 0) atomicAdd(&visible[key_frame[m]], 1);
    }
}

struct ExpandCovisArgs {
    const int32_t* list;            // the connected frames
    const int32_t* first;           // [n_frames + 1]
    const int32_t* adj_ptr;         // [n_frames + 1]: the paired frames of every frame
    const int32_t* adj;
    const int32_t* key_track;       // [N]: the valid track of a key point, or -1
    const int32_t* track_ptr;       // [T + 1]
    const int32_t* obs_frame;
    const int32_t* obs_key;         // as a key point of the set
    const uint8_t* patch;           // [N]
    const int64_t* code_off;        // [n_frames + 1]: the room of every frame's codes
    int32_t* codes;
    int32_t* code_count;            // [n_frames]
    int32_t n_frames, window, patches, min_obs;
};

__global__ __launch_bounds__(kExpandThreads) void k_expand_covis(const ExpandCovisArgs a) {
    extern __shared__ uint32_t s_bits[];                       // paired [ceil(n / 32)] | once [window * 4] | twice [window * 4]
    __shared__ int32_t s_scan[kExpandThreads];
    const int tid = (int)threadIdx.x;
    const int32_t i = a.list[blockIdx.x];
    const int32_t pw = (a.n_frames + 31) / 32;
    uint32_t* const paired = s_bits;
    uint32_t* const once = s_bits + pw;
    uint32_t* const twice = once + (size_t)a.window * 4;
    for (int32_t w = tid; w < pw; w += kExpandThreads) paired[w] = 0;
    __syncthreads();
    if (tid == 0) atomicOr(&paired[i >> 5], 1u << (i & 31));
    for (int32_t e = a.adj_ptr[i] + tid; e < a.adj_ptr[i + 1]; e += kExpandThreads) { const int32_t t = a.adj[e]; atomicOr(&paired[t >> 5], 1u << (t & 31)); }
    const int64_t room0 = a.code_off[i], room = a.code_off[i + 1] - room0;
    const int32_t k0 = a.first[i], k1 = a.first[i + 1];
    int32_t base = 0;                                          // codes written so far: the same in every thread
    for (int32_t w0 = 0; w0 < a.n_frames; w0 += a.window) {
        const int32_t wn = min(a.window, a.n_frames - w0), words = wn * 4;
        __syncthreads();                                       // the paired bits are set; the last window has been compacted
        for (int32_t w = tid; w < words; w += kExpandThreads) { once[w] = 0; twice[w] = 0; }
        __syncthreads();
        for (int32_t k = k0 + tid; k < k1; k += kExpandThreads) {
            const int32_t tr = a.key_track[k];
            if (tr < 0) continue;
            for (int32_t o = a.track_ptr[tr]; o < a.track_ptr[tr + 1]; ++o) {
                const int32_t t = a.obs_frame[o];
                if (t < w0 || t >= w0 + wn || ((paired[t >> 5] >> (t & 31)) & 1u)) continue;
                const int32_t bit = (t - w0) * xexpand::kMaxPatches + a.patch[a.obs_key[o]];
                const uint32_t m = 1u << (bit & 31);
                if (atomicOr(&once[bit >> 5], m) & m) atomicOr(&twice[bit >> 5], m);
            }
        }
        __syncthreads();
        const uint32_t* const want = a.min_obs >= 2 ? twice : once;
        const int32_t run = (words + kExpandThreads - 1) / kExpandThreads;
        const int32_t wb = min(tid * run, words), we = min(wb + run, words);
        int32_t mine = 0;
        for (int32_t w = wb; w < we; ++w) mine += __popc(want[w]);
        s_scan[tid] = mine;
        __syncthreads();
        for (int d = 1; d < kExpandThreads; d <<= 1) {         // inclusive scan of the 256 counts
            const int32_t add = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        int32_t at = base + s_scan[tid] - mine;
        for (int32_t w = wb; w < we; ++w) {
            uint32_t bits = want[w];
            const int32_t frame = w0 + (w >> 2), p0 = (w & 3) * 32;
            while (bits) {
                const int32_t b = __ffs((int)bits) - 1;
                bits &= bits - 1;
                if (at < room) a.codes[room0 + at] = xexpand::code_of(frame, p0 + b, a.patches);          // (at < room always: see above)
                ++at;
            }
        }
        base += s_scan[kExpandThreads - 1];
    }
    if (tid == 0) a.code_count[i] = (int32_t)min((int64_t)base, room);
}

struct ExpandPairsArgs {
    const int2* cand;               // (id1, id2)
    const int32_t* first;
    const int32_t* key_track;
    const int32_t* track_ptr;
    const int32_t* obs_frame;
    const int64_t* code_off;
    const int32_t* codes;
    const int32_t* code_count;
    int2* out;                      // (shared matches, covisible patches)
    int32_t n_cand;
};

__device__ inline int32_t expand_wave_sum(int32_t v) {
    for (int d = kExpandWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kExpandWave);
    return v;
}

__global__ __launch_bounds__(kExpandThreads) void k_expand_pairs(const ExpandPairsArgs a) {
    const int lane = (int)threadIdx.x % kExpandWave;
    const int32_t c = (int32_t)blockIdx.x * (kExpandThreads / kExpandWave) + (int)threadIdx.x / kExpandWave;
    if (c >= a.n_cand) return;                                 // (the whole wave)
    const int2 cd = a.cand[c];
    int32_t shared = 0;
    for (int32_t k = a.first[cd.x] + lane; k < a.first[cd.x + 1]; k += kExpandWave) {
        const int32_t tr = a.key_track[k];
        if (tr >= 0 && xexpand::sorted_has(a.obs_frame + a.track_ptr[tr], a.track_ptr[tr + 1] - a.track_ptr[tr], cd.y)) shared += 1;
    }
    int32_t covis = xexpand::common_codes(a.codes + a.code_off[cd.x], a.code_count[cd.x], a.codes + a.code_off[cd.y], a.code_count[cd.y], lane, kExpandWave);
    shared = expand_wave_sum(shared);
    covis = expand_wave_sum(covis);
    if (lane == 0) a.out[c] = make_int2(shared, covis);
}

}  // namespace xba
