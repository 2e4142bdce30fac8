// The host-side rules of match expansion (ba_expand.h): what MatchExpansionSolver::Run of the reference decides
// (src/feature/match_expansion.cc:407-454), restated on flat arrays.  Plain C++: tests/expand_host_driver.py compiles this file
// alone, with the address and undefined-behaviour sanitizers.
//
//   patch     the patch of a key point (PatchInit) and the code of a (frame, patch)
//   fire      when a key point of a newly registered frame marks its correspondence list (tri_points)
//   window    how many third frames one pass of k_expand_covis holds in LDS, and how many passes that makes
//   rank      the rank table (GetId2RankVec: 1-based position, the last one of a duplicated id), the bands of GetMayreg
//   pairs     the pair index (MakeIdPair), the component of the initial pair (GetConnectedFrames), the set of tried pairs
//   tracks    MakeTrack / AddTrack: sequential over pairs in list order and matches in order, every quirk kept (below)
//   search    the phases the kernels run, as plain loops over the same per-item rules (the stand-alone program and the timing
//             tool run them; the library runs the kernels), and the final merge, de-duplication and sort
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define XEXPAND_HD __host__ __device__
#else
#define XEXPAND_HD
#endif

namespace xexpand {

constexpr int32_t kMaxPatches = 128;          // bits of a third frame in one LDS bit set of k_expand_covis

struct Opt {                                  // xrsfm_ba_expand_options, field for field
    int32_t patch_cols, patch_rows, min_patch_obs, min_visible, max_shared_matches, min_covisible_patches, similarity_rank_max;
    int32_t mayreg_rank_lo, mayreg_rank_mid, mayreg_rank_hi, mayreg_count_mid, mayreg_count_sum;
};

inline Opt default_options() { return Opt{10, 10, 2, 30, 50, 1, 40, 5, 25, 50, 15, 35}; }

// null, or what is wrong with the options
inline const char* options_fault(const Opt& o) {
    if (o.patch_cols < 1 || o.patch_rows < 1 || (int64_t)o.patch_cols * o.patch_rows > kMaxPatches) return "patch_cols * patch_rows outside 1..128";
    if (o.min_patch_obs < 1 || o.min_patch_obs > 2) return "min_patch_obs outside {1, 2} (the kernel keeps two bit sets: seen once, seen twice)";
    if (o.min_visible < 1) return "min_visible below 1";
    if (o.max_shared_matches < 0 || o.min_covisible_patches < 0 || o.similarity_rank_max < 0) return "a negative threshold";
    if (o.mayreg_rank_lo < 0 || o.mayreg_rank_mid < o.mayreg_rank_lo || o.mayreg_rank_hi < o.mayreg_rank_mid) return "may-register ranks not ascending";
    return nullptr;
}

// ---- patch
// PatchInit: step = size / grid (integer), cell = (int)coordinate / step (C division: toward zero), clamped above only.
// -1: the reference would index outside the frame's patches (a negative cell) or convert a value no int holds.
XEXPAND_HD inline int32_t patch_of(float x, float y, int32_t width, int32_t height, int32_t cols, int32_t rows) {
    if (!(x >= -2147483648.f && x < 2147483648.f) || !(y >= -2147483648.f && y < 2147483648.f)) return -1;
    const int32_t step_x = width / cols, step_y = height / rows;          // (>= 1: the entry refuses sizes below the grid)
    int32_t px = (int32_t)x / step_x, py = (int32_t)y / step_y;
    if (px < 0 || py < 0) return -1;
    if (px >= cols) px = cols - 1;
    if (py >= rows) py = rows - 1;
    return py * cols + px;
}

XEXPAND_HD inline int32_t code_of(int32_t frame, int32_t patch, int32_t patches) { return frame * patches + patch; }

// the frame of key point k: the f with first[f] <= k < first[f + 1] (empty frames share a first)
XEXPAND_HD inline int32_t frame_of(const int32_t* first, int32_t n_frames, int32_t k) {
    int32_t lo = 0, hi = n_frames;                                          // first[lo] <= k < first[hi]
    while (hi - lo > 1) { const int32_t mid = lo + (hi - lo) / 2; if (first[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

// ---- fire
// tri_points(f, g) marks the whole list of a key point of f that has a correspondent in g.  Run for every registered g paired with
// f, that is: the key point fires when any correspondent lies in a frame registered by now.  (At the start only the two initial
// frames are registered and only the first one walks its key points, so "registered" there means the second initial frame.)
XEXPAND_HD inline bool fires(const int32_t* list, int32_t n, const int32_t* key_frame, const uint8_t* registered) {
    for (int32_t e = 0; e < n; ++e) if (registered[key_frame[list[e]]]) return true;
    return false;
}

// ---- window
// k_expand_covis holds per third frame 2 x 128 bits, beside one bit per frame for "paired with this frame"
inline int64_t window_fixed_bytes(int32_t n_frames) { return 4 * (((int64_t)n_frames + 31) / 32); }
// third frames per pass (0: the paired bit set alone does not fit); forced > 0 lowers it
inline int32_t window_frames(int64_t lds_bytes, int32_t n_frames, int32_t forced) {
    int64_t w = (lds_bytes - window_fixed_bytes(n_frames)) / 32;
    if (w < 0) w = 0;
    if (forced > 0 && forced < w) w = forced;
    if (w > n_frames) w = n_frames;
    return (int32_t)w;
}
inline int32_t window_passes(int32_t n_frames, int32_t w) { return w > 0 ? (n_frames + w - 1) / w : 0; }

// ---- rank
struct RankTable { std::vector<int64_t> ptr; std::vector<int32_t> id, rank; };     // per frame its ids ascending, each once

inline RankTable rank_table(int32_t n, const int64_t* rank_ptr, const int32_t* rank_ids) {
    RankTable t;
    t.ptr.assign((size_t)n + 1, 0);
    std::vector<std::pair<int32_t, int32_t>> row;
    for (int32_t f = 0; f < n; ++f) {
        row.clear();
        for (int64_t k = rank_ptr[f]; k < rank_ptr[f + 1]; ++k) row.emplace_back(rank_ids[k], (int32_t)(k - rank_ptr[f]) + 1);
        std::sort(row.begin(), row.end());
        for (size_t k = 0; k < row.size(); ++k)
            if (k + 1 == row.size() || row[k + 1].first != row[k].first) { t.id.push_back(row[k].first); t.rank.push_back(row[k].second); }      // the last position wins
        t.ptr[(size_t)f + 1] = (int64_t)t.id.size();
    }
    return t;
}

// 0: id is not in the list of f
inline int32_t rank_of(const RankTable& t, int32_t f, int32_t id) {
    const int32_t* b = t.id.data() + t.ptr[(size_t)f];
    const int32_t* e = t.id.data() + t.ptr[(size_t)f + 1];
    const int32_t* it = std::lower_bound(b, e, id);
    return it != e && *it == id ? t.rank[(size_t)(it - t.id.data())] : 0;
}

// GetMayreg's bands: 0 up to rank_lo (counted and unused), 1 up to rank_mid, 2 up to rank_hi, 3 beyond
inline int32_t rank_band(int32_t rank, const Opt& o) { return rank <= o.mayreg_rank_lo ? 0 : rank <= o.mayreg_rank_mid ? 1 : rank <= o.mayreg_rank_hi ? 2 : 3; }
inline bool may_register(int32_t count_mid, int32_t count_hi, const Opt& o) { return count_mid >= o.mayreg_count_mid || count_mid + count_hi >= o.mayreg_count_sum; }

// ---- pairs
inline int64_t pair_key(int32_t a, int32_t b) { return a < b ? ((int64_t)a << 32) | (uint32_t)b : ((int64_t)b << 32) | (uint32_t)a; }

struct PairIndex { std::vector<int32_t> ptr, nbr, pid; };          // per frame its paired frames ascending, with the pair's index

// false: a pair is listed twice (the reference's map would silently keep the first)
inline bool pair_index(int32_t n, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, PairIndex* out) {
    std::vector<std::pair<int64_t, int32_t>> e;
    e.reserve(2 * (size_t)n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) { e.emplace_back(((int64_t)pair_a[p] << 32) | (uint32_t)pair_b[p], p); e.emplace_back(((int64_t)pair_b[p] << 32) | (uint32_t)pair_a[p], p); }
    std::sort(e.begin(), e.end());
    out->ptr.assign((size_t)n + 1, 0); out->nbr.clear(); out->pid.clear();
    for (size_t k = 0; k < e.size(); ++k) {
        if (k > 0 && e[k].first == e[k - 1].first) return false;
        out->ptr[(size_t)(e[k].first >> 32) + 1] += 1;
        out->nbr.push_back((int32_t)(e[k].first & 0xffffffff)); out->pid.push_back(e[k].second);
    }
    for (int32_t f = 0; f < n; ++f) out->ptr[(size_t)f + 1] += out->ptr[(size_t)f];
    return true;
}

// the pair's index, or -1
inline int32_t pair_find(const PairIndex& ix, int32_t a, int32_t b) {
    const int32_t* s = ix.nbr.data() + ix.ptr[(size_t)a];
    const int32_t* e = ix.nbr.data() + ix.ptr[(size_t)a + 1];
    const int32_t* it = std::lower_bound(s, e, b);
    return it != e && *it == b ? ix.pid[(size_t)(it - ix.nbr.data())] : -1;
}

// GetConnectedFrames: the component of `seed` in the pair graph
inline std::vector<uint8_t> connected_frames(int32_t n, const PairIndex& ix, int32_t seed) {
    std::vector<uint8_t> in((size_t)n, 0);
    std::vector<int32_t> stack(1, seed);
    in[(size_t)seed] = 1;
    while (!stack.empty()) {
        const int32_t f = stack.back(); stack.pop_back();
        for (int32_t k = ix.ptr[(size_t)f]; k < ix.ptr[(size_t)f + 1]; ++k)
            if (!in[(size_t)ix.nbr[(size_t)k]]) { in[(size_t)ix.nbr[(size_t)k]] = 1; stack.push_back(ix.nbr[(size_t)k]); }
    }
    return in;
}

inline std::vector<int64_t> tried_set(int32_t n_tried, const int32_t* a, const int32_t* b) {
    std::vector<int64_t> s((size_t)n_tried);
    for (int32_t k = 0; k < n_tried; ++k) s[(size_t)k] = pair_key(a[k], b[k]);
    std::sort(s.begin(), s.end());
    return s;
}
inline bool is_tried(const std::vector<int64_t>& s, int32_t a, int32_t b) { return std::binary_search(s.begin(), s.end(), pair_key(a, b)); }

// ---- tracks
// AddTrack keeps a std::map<frame, key point> per track.  Here every track is a list of nodes ascending by frame in three flat
// arrays; a track's list only grows (a merged track keeps its own and turns invalid).  The quirks that decide outputs:
//   - insert does not overwrite: a key point can point at a track whose observation in that frame is another key point;
//   - a merge moves track2's observations into track1; one whose frame track1 holds with another key point loses its track (-1);
//     key points that point at track2 without being among its observations keep pointing at it, and it is invalid from then on;
//   - nothing ever makes an invalid track valid again, and it still takes observations.
struct Tracks {
    std::vector<int32_t> key_track;                       // [N]: -1, or a track (which may be invalid)
    std::vector<int64_t> track_ptr;                       // [T + 1]
    std::vector<int32_t> obs_frame, obs_key;              // ascending by frame within a track; obs_key: the key point within its frame
    std::vector<uint8_t> invalid;                         // [T]
    int64_t valid_tracks = 0;
};

struct TrackBuilder {
    std::vector<int32_t> head, node_frame, node_key, node_next;
    std::vector<uint8_t> invalid;
    // the key point track t holds for `frame`, or -1
    int32_t find(int32_t t, int32_t frame) const {
        for (int32_t q = head[(size_t)t]; q >= 0 && node_frame[(size_t)q] <= frame; q = node_next[(size_t)q])
            if (node_frame[(size_t)q] == frame) return node_key[(size_t)q];
        return -1;
    }
    // std::map::insert: nothing happens when the frame is there
    void insert(int32_t t, int32_t frame, int32_t key) {
        int32_t prev = -1, q = head[(size_t)t];
        while (q >= 0 && node_frame[(size_t)q] < frame) { prev = q; q = node_next[(size_t)q]; }
        if (q >= 0 && node_frame[(size_t)q] == frame) return;
        const int32_t nn = (int32_t)node_frame.size();
        node_frame.push_back(frame); node_key.push_back(key); node_next.push_back(q);
        if (prev < 0) head[(size_t)t] = nn; else node_next[(size_t)prev] = nn;
    }
    int32_t create() { head.push_back(-1); invalid.push_back(0); return (int32_t)head.size() - 1; }
};

inline Tracks make_tracks(int32_t n_frames, const int64_t* key_ptr, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* match_ptr,
                          const int32_t* matches) {
    Tracks out;
    out.key_track.assign((size_t)key_ptr[n_frames], -1);
    TrackBuilder b;
    std::vector<int32_t>& kt = out.key_track;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t f1 = pair_a[p], f2 = pair_b[p];
        for (int64_t m = match_ptr[p]; m < match_ptr[p + 1]; ++m) {
            const int32_t i1 = matches[2 * m], i2 = matches[2 * m + 1];
            int32_t& t1 = kt[(size_t)(key_ptr[f1] + i1)];
            int32_t& t2 = kt[(size_t)(key_ptr[f2] + i2)];
            if (t1 == -1 && t2 == -1) {
                const int32_t t = b.create();
                t1 = t2 = t;
                b.insert(t, f1, i1); b.insert(t, f2, i2);
            } else if (t1 == -1) {
                t1 = t2;
                b.insert(t1, f1, i1);
            } else if (t2 == -1) {
                t2 = t1;
                b.insert(t2, f2, i2);
            } else if (t1 != t2) {
                const int32_t into = t1, from = t2;          // (t1 and t2 are references into kt, which the loop below writes)
                for (int32_t q = b.head[(size_t)from]; q >= 0; q = b.node_next[(size_t)q]) {
                    const int32_t fr = b.node_frame[(size_t)q], ky = b.node_key[(size_t)q];
                    const int32_t held = b.find(into, fr);
                    if (held < 0) { b.insert(into, fr, ky); kt[(size_t)(key_ptr[fr] + ky)] = into; }
                    else if (held == ky) kt[(size_t)(key_ptr[fr] + ky)] = into;
                    else kt[(size_t)(key_ptr[fr] + ky)] = -1;
                }
                b.invalid[(size_t)from] = 1;
            }
        }
    }
    const size_t T = b.head.size();
    out.invalid = b.invalid;
    out.track_ptr.assign(T + 1, 0);
    out.obs_frame.reserve(b.node_frame.size()); out.obs_key.reserve(b.node_frame.size());
    for (size_t t = 0; t < T; ++t) {
        for (int32_t q = b.head[t]; q >= 0; q = b.node_next[(size_t)q]) { out.obs_frame.push_back(b.node_frame[(size_t)q]); out.obs_key.push_back(b.node_key[(size_t)q]); }
        out.track_ptr[t + 1] = (int64_t)out.obs_frame.size();
        out.valid_tracks += b.invalid[t] ? 0 : 1;
    }
    return out;
}

// the track of a key point if it "has a valid track", else -1 (what the kernels read)
inline int32_t valid_track(const Tracks& t, int64_t key) { const int32_t id = t.key_track[(size_t)key]; return id >= 0 && !t.invalid[(size_t)id] ? id : -1; }

// whether the frame-sorted observations obs[0 .. n) hold `frame` (GetMatcheNum; lanes of k_expand_pairs)
XEXPAND_HD inline bool sorted_has(const int32_t* v, int32_t n, int32_t x) {
    int32_t lo = 0, hi = n;
    while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (v[mid] < x) lo = mid + 1; else hi = mid; }
    return lo < n && v[lo] == x;
}

// ---- search: the phases of the kernels as loops
struct Corr { std::vector<int32_t> ptr, ent; };          // per key point (of the whole set) its correspondents, as key points of the set

inline Corr corr_graph(int64_t n_keys, const int64_t* key_ptr, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* match_ptr, const int32_t* matches) {
    Corr c;
    c.ptr.assign((size_t)n_keys + 1, 0);
    for (int32_t p = 0; p < n_pairs; ++p)
        for (int64_t m = match_ptr[p]; m < match_ptr[p + 1]; ++m) { c.ptr[(size_t)(key_ptr[pair_a[p]] + matches[2 * m]) + 1] += 1; c.ptr[(size_t)(key_ptr[pair_b[p]] + matches[2 * m + 1]) + 1] += 1; }
    for (int64_t k = 0; k < n_keys; ++k) c.ptr[(size_t)k + 1] += c.ptr[(size_t)k];
    c.ent.assign((size_t)c.ptr[(size_t)n_keys], 0);
    std::vector<int32_t> at(c.ptr.begin(), c.ptr.end() - 1);
    for (int32_t p = 0; p < n_pairs; ++p)
        for (int64_t m = match_ptr[p]; m < match_ptr[p + 1]; ++m) {
            const int32_t ka = (int32_t)(key_ptr[pair_a[p]] + matches[2 * m]), kb = (int32_t)(key_ptr[pair_b[p]] + matches[2 * m + 1]);
            c.ent[(size_t)at[(size_t)ka]++] = kb; c.ent[(size_t)at[(size_t)kb]++] = ka;
        }
    return c;
}

// SimulationSfM in synchronous rounds; first / second: the initial pair as the pair list stores it.  Returns the rounds that
// registered a frame; visible: the final mark counts.
inline int32_t simulate(int32_t n, const int32_t* first, const int32_t* key_frame, const Corr& c, int32_t init_first, int32_t init_second, int32_t min_visible,
                        std::vector<int32_t>* visible) {
    std::vector<uint8_t> registered((size_t)n, 0), mark((size_t)first[n], 0);
    visible->assign((size_t)n, 0);
    std::vector<int32_t> work(1, init_first);
    registered[(size_t)init_first] = registered[(size_t)init_second] = 1;
    int32_t rounds = 0;
    for (;;) {
        for (int32_t f : work)
            for (int32_t k = first[f]; k < first[f + 1]; ++k) {
                const int32_t* list = c.ent.data() + c.ptr[(size_t)k];
                const int32_t len = c.ptr[(size_t)k + 1] - c.ptr[(size_t)k];
                if (!fires(list, len, key_frame, registered.data())) continue;
                for (int32_t e = 0; e < len; ++e)
                    if (!mark[(size_t)list[e]]) { mark[(size_t)list[e]] = 1; (*visible)[(size_t)key_frame[list[e]]] += 1; }
            }
        work.clear();
        for (int32_t f = 0; f < n; ++f)
            if (!registered[(size_t)f] && (*visible)[(size_t)f] >= min_visible) work.push_back(f);
        if (work.empty()) break;
        for (int32_t f : work) registered[(size_t)f] = 1;          // all of them before any of them walks its key points
        rounds += 1;
    }
    return rounds;
}

// GetCovisibilityInfo(i) reduced to what is read of it: the ascending codes of the (frame, patch) counted min_obs times or more
inline void covis_codes(int32_t i, const int32_t* first, const Tracks& t, const PairIndex& ix, const uint8_t* patch, const int64_t* key_ptr, int32_t patches, int32_t min_obs,
                        std::vector<int32_t>* codes) {
    std::vector<int32_t> all;
    for (int32_t k = first[i]; k < first[i + 1]; ++k) {
        const int32_t tr = valid_track(t, k);
        if (tr < 0) continue;
        for (int64_t o = t.track_ptr[(size_t)tr]; o < t.track_ptr[(size_t)tr + 1]; ++o) {
            const int32_t f = t.obs_frame[(size_t)o];
            if (f == i || pair_find(ix, i, f) >= 0) continue;
            all.push_back(code_of(f, patch[(size_t)(key_ptr[f] + t.obs_key[(size_t)o])], patches));
        }
    }
    std::sort(all.begin(), all.end());
    codes->clear();
    for (size_t k = 0; k < all.size();) {
        size_t e = k;
        while (e < all.size() && all[e] == all[k]) ++e;
        if ((int64_t)(e - k) >= min_obs) codes->push_back(all[k]);
        k = e;
    }
}

// the items k_expand_covis walks for frame i: the observations of the valid tracks of its key points (skipped ones included)
inline int64_t covis_items(int32_t i, const int32_t* first, const Tracks& t) {
    int64_t items = 0;
    for (int32_t k = first[i]; k < first[i + 1]; ++k) { const int32_t tr = valid_track(t, k); if (tr >= 0) items += t.track_ptr[(size_t)tr + 1] - t.track_ptr[(size_t)tr]; }
    return items;
}

// GetMatcheNum(id1, id2): not symmetric
inline int32_t shared_matches(int32_t id1, int32_t id2, const int32_t* first, const Tracks& t) {
    int32_t count = 0;
    for (int32_t k = first[id1]; k < first[id1 + 1]; ++k) {
        const int32_t tr = valid_track(t, k);
        if (tr >= 0 && sorted_has(t.obs_frame.data() + t.track_ptr[(size_t)tr], (int32_t)(t.track_ptr[(size_t)tr + 1] - t.track_ptr[(size_t)tr]), id2)) count += 1;
    }
    return count;
}

// codes in both ascending lists (the shorter searched in the longer)
XEXPAND_HD inline int32_t common_codes(const int32_t* a, int32_t na, const int32_t* b, int32_t nb, int32_t lane, int32_t lanes) {
    if (na > nb) { const int32_t* p = a; a = b; b = p; const int32_t q = na; na = nb; nb = q; }
    int32_t count = 0;
    for (int32_t k = lane; k < na; k += lanes) count += sorted_has(b, nb, a[k]) ? 1 : 0;
    return count;
}

// The directed candidates of GetCandidateCovisibility that pass the tests before GetMatcheNum, ascending in (id1, id2): id2 in the
// rank list of id1, not itself, not tried, one of them registered, both connected.
inline std::vector<int32_t> directed_candidates(int32_t n, const RankTable& rt, const std::vector<int64_t>& tried, const uint8_t* registered, const uint8_t* connected) {
    std::vector<int32_t> out;
    for (int32_t id1 = 0; id1 < n; ++id1)
        for (int64_t k = rt.ptr[(size_t)id1]; k < rt.ptr[(size_t)id1 + 1]; ++k) {
            const int32_t id2 = rt.id[(size_t)k];
            if (id1 == id2 || is_tried(tried, id1, id2)) continue;
            if (!registered[id1] && !registered[id2]) continue;
            if (!connected[id1] || !connected[id2]) continue;
            out.push_back(id1); out.push_back(id2);
        }
    return out;
}

struct Result {
    std::vector<uint8_t> registered, may_register;
    std::vector<int32_t> out_a, out_b;
    std::vector<uint8_t> out_source;
};

// What follows the counts.  cand: rows (id1, id2, shared matches, covisible patches).  A directed candidate passes with at most
// max_shared_matches shared matches and at least min_covisible_patches patches; the reference marks an emitted pair as tried in
// both directions and de-duplicates, so an unordered pair is out exactly when one of its directed forms passes.  Then GetMayreg
// and GetCandidateSimilarity; the two stages cannot meet (the first needs both frames connected, the second one that is not).
inline void finish(int32_t n, const Opt& o, const RankTable& rt, const std::vector<int64_t>& tried, const uint8_t* connected, const int32_t* visible, const int32_t* cand,
                   int64_t n_cand, Result* r) {
    r->registered.assign((size_t)n, 0); r->may_register.assign((size_t)n, 0);
    for (int32_t f = 0; f < n; ++f) r->registered[(size_t)f] = visible[f] >= o.min_visible ? 1 : 0;
    std::vector<std::pair<int64_t, uint8_t>> pairs;
    for (int64_t c = 0; c < n_cand; ++c)
        if (cand[4 * c + 2] <= o.max_shared_matches && cand[4 * c + 3] >= o.min_covisible_patches) pairs.emplace_back(pair_key(cand[4 * c], cand[4 * c + 1]), (uint8_t)1);
    for (int32_t f = 0; f < n; ++f) {
        if (connected[f]) continue;
        int32_t band[4] = {0, 0, 0, 0};
        for (int64_t k = rt.ptr[(size_t)f]; k < rt.ptr[(size_t)f + 1]; ++k)
            if (r->registered[(size_t)rt.id[(size_t)k]]) band[rank_band(rt.rank[(size_t)k], o)] += 1;
        if (!may_register(band[1], band[2], o)) continue;
        r->may_register[(size_t)f] = 1;
        for (int32_t g = 0; g < n; ++g) {
            if (!r->registered[(size_t)g] || is_tried(tried, f, g)) continue;
            const int32_t r1 = rank_of(rt, f, g), r2 = rank_of(rt, g, f);
            if ((r1 > 0 && r1 <= o.similarity_rank_max) || (r2 > 0 && r2 <= o.similarity_rank_max)) pairs.emplace_back(pair_key(f, g), (uint8_t)2);
        }
    }
    std::sort(pairs.begin(), pairs.end());
    r->out_a.clear(); r->out_b.clear(); r->out_source.clear();
    for (size_t k = 0; k < pairs.size(); ++k) {
        if (k > 0 && pairs[k].first == pairs[k - 1].first) continue;
        r->out_a.push_back((int32_t)(pairs[k].first >> 32)); r->out_b.push_back((int32_t)(pairs[k].first & 0xffffffff)); r->out_source.push_back(pairs[k].second);
    }
}

}  // namespace xexpand
