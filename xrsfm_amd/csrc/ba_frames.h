// Device-resident frame sets: the features of n frames held on the device between FeatureExtract and any number of
// FeatureMatching calls.  The rules are in ba_frames_rule.h; this file holds the two kernels that keep the data on
// the device where the chain of entry points goes through the host.
//
// k_frames_order: after k_siftd_desc the key points of a chunk sit image-major and level-major, and inside a level in the order
// in which the tiles emitted them.  One 256-thread workgroup per work item (segment = one (image, level), slice of 256 of its key
// points): every thread takes one key point, walks the codes row * width + col of the whole segment through LDS in slices of 256
// (one broadcast read per comparison; a slice's padding holds INT64_MAX, which is below no code) and counts those below its own:
// its rank.  Then the key, the location, the sign and the orientation go to first + rank, and the 128 descriptor bytes follow,
// eight lanes of 16 bytes per key point.  The codes are unique within a level, so the ranks are a permutation of 0 .. count - 1
// whatever the order of emission; a rank stays below count even if they were not, so no store can leave the segment.
//
// k_frames_gather: one workgroup per pair.  For every match that k_match_select wrote at the pair's upper-bound offset it widens
// the two key points to FP64 into the double[4]-per-match array that k_verify_pairs reads, and copies the match to its compacted
// place, so that one read-back fetches matches, masks and results.  (double) of a float is exact: the values are those the host
// computes from the downloaded key points.
//
// Integer compares and copies only; no atomics; no floating-point arithmetic but the widening; nothing waits for another workgroup.
#pragma once
#include <cstdint>

#include "ba_frames_rule.h"

namespace xba {

constexpr int kFramesThreads = 256;

struct FramesSeg { int64_t first; int32_t count, width; };          // key points first .. first + count of one (image, level)
struct FramesOrderItem { int32_t seg, slice; };

struct FramesGatherPair {
    int64_t row_off;           // of the pair in the matching launch: its matches start at 2 * row_off
    int64_t key_a, key_b;      // first key point of either frame in the set
    int32_t beg, n;            // matches beg .. beg + n of the gathered arrays
    int32_t n_a, n_b;          // key points of either frame that took part
};

__global__ __launch_bounds__(kFramesThreads) void k_frames_order(
        const FramesOrderItem* __restrict__ items, const FramesSeg* __restrict__ segs, const float4* __restrict__ keys, const int4* __restrict__ loc,
        const float4* __restrict__ off, const float4* __restrict__ okeys, const uint8_t* __restrict__ desc, float4* __restrict__ out_keys,
        int4* __restrict__ out_loc, int8_t* __restrict__ out_sign, float* __restrict__ out_w, uint8_t* __restrict__ out_desc) {
    __shared__ int64_t s_code[kFramesThreads];
    __shared__ int32_t s_rank[kFramesThreads];
    const FramesOrderItem it = items[blockIdx.x];
    const FramesSeg sg = segs[it.seg];
    const int tid = (int)threadIdx.x;
    const int k = it.slice * kFramesThreads + tid;
    const bool mine = k < sg.count;
    int4 l = make_int4(0, 0, 0, 0);
    int64_t code = 0;
    if (mine) { l = loc[sg.first + k]; code = xframes::order_code(l.z, l.w, sg.width); }
    int32_t rank = 0;
    for (int base = 0; base < sg.count; base += kFramesThreads) {
        const int j = base + tid;
        int64_t c = INT64_MAX;
        if (j < sg.count) { const int4 lj = loc[sg.first + j]; c = xframes::order_code(lj.z, lj.w, sg.width); }
        __syncthreads();                       // the previous slice has been read
        s_code[tid] = c;
        __syncthreads();
        rank += xframes::order_below(s_code, kFramesThreads, code);
    }
    if (mine) {
        const int64_t src = sg.first + k, dst = sg.first + rank;
        out_keys[dst] = keys[src];
        out_loc[dst] = l;
        out_sign[dst] = (int8_t)(int)off[src].x;
        out_w[dst] = okeys[src].w;
    }
    s_rank[tid] = mine ? rank : -1;
    __syncthreads();
    const int part = tid & 7;
    for (int p = tid >> 3; p < kFramesThreads; p += kFramesThreads / 8) {
        const int r = s_rank[p];
        if (r < 0) continue;
        const int64_t src = sg.first + (int64_t)it.slice * kFramesThreads + p;
        reinterpret_cast<uint4*>(out_desc)[(sg.first + r) * 8 + part] = reinterpret_cast<const uint4*>(desc)[src * 8 + part];
    }
}

__global__ __launch_bounds__(kFramesThreads) void k_frames_gather(
        const FramesGatherPair* __restrict__ pairs, const int32_t* __restrict__ matches, const float4* __restrict__ keys, double2* __restrict__ m_out,
        int2* __restrict__ matches_out) {
    const FramesGatherPair pr = pairs[blockIdx.x];
    for (int m = (int)threadIdx.x; m < pr.n; m += kFramesThreads) {
        int i = matches[2 * (pr.row_off + m)], j = matches[2 * (pr.row_off + m) + 1];
        if ((unsigned)i >= (unsigned)pr.n_a) i = 0;          // (k_match_select writes none such; no load may leave the frame)
        if ((unsigned)j >= (unsigned)pr.n_b) j = 0;
        const float4 a = keys[pr.key_a + i], b = keys[pr.key_b + j];
        m_out[2 * (int64_t)(pr.beg + m)] = make_double2((double)a.x, (double)a.y);
        m_out[2 * (int64_t)(pr.beg + m) + 1] = make_double2((double)b.x, (double)b.y);
        matches_out[pr.beg + m] = make_int2(matches[2 * (pr.row_off + m)], matches[2 * (pr.row_off + m) + 1]);
    }
}

}  // namespace xba
