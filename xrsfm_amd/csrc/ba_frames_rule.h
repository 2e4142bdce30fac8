// The host-side rules of a device-resident frame set (ba_frames.h).  Plain C++: tests/frames_host_driver.py compiles
// this file alone, with the address and undefined-behaviour sanitizers.
//
//   order   a level's key points leave the detection in the order of its tiles; the interface hands them out by row * width + col
//           of their sample (xrsfm_ba_extract_features).  The code is unique within a level, so the rank of a key point is the
//           number of codes of its (image, level) segment below its own: exact, and independent of the order of emission.
//   plan    the offsets of a sub-batch of pairs in the per-row, per-column and per-strip buffers of the matching launch, the split of
//           a pair list into sub-batches under a workspace budget, and the offsets of the gathered coordinates of a sub-batch.
//   accept  FeatureMatching's threshold on the inliers of a verified pair (reference feature_processing.cc:284-290).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define XFRAMES_HD __host__ __device__
#else
#define XFRAMES_HD
#endif

namespace xframes {

// ---- order
XFRAMES_HD inline int64_t order_code(int32_t row, int32_t col, int32_t width) { return (int64_t)row * width + col; }

// codes below `code` among n (every thread of k_frames_order sums this over the slices of its segment)
XFRAMES_HD inline int32_t order_below(const int64_t* codes, int32_t n, int64_t code) {
    int32_t r = 0;
    for (int32_t k = 0; k < n; ++k) r += codes[k] < code ? 1 : 0;
    return r;
}

// ---- plan
struct PairSpan {              // of one pair inside its sub-batch
    int64_t part_off;          // first triple of its column partials [strips][n_b]
    int64_t row_off, col_off;  // first row / column in the per-row and per-column buffers
    int64_t item_off;          // first work item (one per strip)
    int32_t strips;
};

struct BatchSize { int64_t pairs = 0, rows = 0, cols = 0, parts = 0, items = 0; };

inline int32_t strips_of(int32_t n_a, int32_t strip) { return (n_a + strip - 1) / strip; }

// the pair (n_a rows, n_b columns) goes behind what `size` holds
inline PairSpan plan_append(BatchSize& size, int32_t n_a, int32_t n_b, int32_t strip) {
    PairSpan s;
    s.strips = strips_of(n_a, strip);
    s.part_off = size.parts; s.row_off = size.rows; s.col_off = size.cols; s.item_off = size.items;
    size.pairs += 1; size.rows += n_a; size.cols += n_b; size.parts += (int64_t)s.strips * n_b; size.items += s.strips;
    return s;
}

// the pairs with rows and columns (clip[f]: descriptors of frame f that take part), in the caller's order, with their sizes
inline void plan_live(int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int32_t* clip, std::vector<int32_t>* live, std::vector<int32_t>* n_a,
                      std::vector<int32_t>* n_b) {
    for (int32_t p = 0; p < n_pairs; ++p)
        if (clip[pair_a[p]] > 0 && clip[pair_b[p]] > 0) { live->push_back(p); n_a->push_back(clip[pair_a[p]]); n_b->push_back(clip[pair_b[p]]); }
}

struct Batch { size_t first, last; BatchSize size; };          // pairs first .. last - 1 of the list

// Consecutive pairs share a sub-batch while bytes(size) stays within the budget; a pair above it runs alone.
template <typename Bytes>
inline std::vector<Batch> plan_split(size_t n_pairs, const int32_t* n_a, const int32_t* n_b, int32_t strip, size_t budget, Bytes&& bytes) {
    std::vector<Batch> out;
    size_t first = 0;
    BatchSize size;
    for (size_t k = 0; k < n_pairs; ++k) {
        BatchSize with = size;
        plan_append(with, n_a[k], n_b[k], strip);
        if (k > first && bytes(with) > budget) {
            out.push_back(Batch{first, k, size});
            first = k; size = BatchSize();
            plan_append(size, n_a[k], n_b[k], strip);
        } else {
            size = with;
        }
    }
    if (n_pairs > first) out.push_back(Batch{first, n_pairs, size});
    return out;
}

// the first gathered match of every pair of a sub-batch; false when the total leaves int32
inline bool plan_gather(size_t n_pairs, const int32_t* count, int32_t* beg, int64_t* total) {
    int64_t at = 0;
    for (size_t k = 0; k < n_pairs; ++k) {
        if (at > 0x7fffffff) return false;
        beg[k] = (int32_t)at;
        at += count[k];
    }
    *total = at;
    return at <= 0x7fffffff;
}

// ---- accept
inline int32_t accept_threshold(int32_t min_num_inliers, double min_accept_ratio, int32_t n_matches) {
    const int32_t by_ratio = (int32_t)(min_accept_ratio * (double)n_matches);
    return min_num_inliers > by_ratio ? min_num_inliers : by_ratio;
}

}  // namespace xframes
