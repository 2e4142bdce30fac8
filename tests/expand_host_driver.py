"""A stand-alone host program around ba_expand_rule.h (no HIP, no GPU): one whole search of a case read from stdin, by the loops of the
rule header that restate the kernels' phases, every intermediate printed.  tests/test_expand_cpu.py builds it with the address and
undefined-behaviour sanitizers; tools/match_expansion_timing.py builds it at -O2 and reads its clock."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OPT_FIELDS = ("patch_cols", "patch_rows", "min_patch_obs", "min_visible", "max_shared_matches", "min_covisible_patches", "similarity_rank_max",
              "mayreg_rank_lo", "mayreg_rank_mid", "mayreg_rank_hi", "mayreg_count_mid", "mayreg_count_sum")

DRIVER = r"""
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_expand_rule.h"
// stdin: the 12 options; n; key_ptr; x y per key point; width height per frame; n_pairs; a b per pair; match_ptr; i j per match;
// rank_ptr; rank_ids; n_tried; a b per tried pair; init_a init_b; lds_bytes forced_window; repeats.
// stdout: one line per array, its name first.
using namespace xexpand;
template <typename T> static bool rd(std::vector<T>& v) { for (auto& x : v) { long long q; if (std::scanf("%lld", &q) != 1) return false; x = (T)q; } return true; }
template <typename V> static void line(const char* name, const V& v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); }
int main() {
    std::vector<int32_t> ov(12);
    if (!rd(ov)) return 1;
    Opt o;
    static_assert(sizeof(Opt) == 12 * sizeof(int32_t), "twelve fields");
    std::memcpy(&o, ov.data(), sizeof(o));
    if (const char* fault = options_fault(o)) { std::printf("fault %s\n", fault); return 0; }
    int n;
    if (std::scanf("%d", &n) != 1) return 1;
    std::vector<int64_t> key_ptr((size_t)n + 1);
    if (!rd(key_ptr)) return 1;
    const int64_t N = key_ptr[(size_t)n];
    std::vector<float> xy(2 * (size_t)N);
    for (auto& v : xy) if (std::scanf("%f", &v) != 1) return 1;
    std::vector<int32_t> wh(2 * (size_t)n);
    if (!rd(wh)) return 1;
    int np;
    if (std::scanf("%d", &np) != 1) return 1;
    std::vector<int32_t> pab(2 * (size_t)np), pa((size_t)np), pb((size_t)np);
    if (!rd(pab)) return 1;
    for (int p = 0; p < np; ++p) { pa[(size_t)p] = pab[2 * (size_t)p]; pb[(size_t)p] = pab[2 * (size_t)p + 1]; }
    std::vector<int64_t> match_ptr((size_t)np + 1);
    if (!rd(match_ptr)) return 1;
    std::vector<int32_t> matches(2 * (size_t)match_ptr[(size_t)np]);
    if (!rd(matches)) return 1;
    std::vector<int64_t> rank_ptr((size_t)n + 1);
    if (!rd(rank_ptr)) return 1;
    std::vector<int32_t> rank_ids((size_t)rank_ptr[(size_t)n]);
    if (!rd(rank_ids)) return 1;
    int nt;
    if (std::scanf("%d", &nt) != 1) return 1;
    std::vector<int32_t> tab(2 * (size_t)nt), ta((size_t)nt), tb((size_t)nt);
    if (!rd(tab)) return 1;
    for (int k = 0; k < nt; ++k) { ta[(size_t)k] = tab[2 * (size_t)k]; tb[(size_t)k] = tab[2 * (size_t)k + 1]; }
    int ia, ib, forced, repeats;
    long long lds;
    if (std::scanf("%d %d %lld %d %d", &ia, &ib, &lds, &forced, &repeats) != 5) return 1;

    std::vector<int32_t> first((size_t)n + 1), key_frame((size_t)N);
    for (int f = 0; f <= n; ++f) first[(size_t)f] = (int32_t)key_ptr[(size_t)f];
    std::vector<uint8_t> patch((size_t)N);
    const int32_t patches = o.patch_cols * o.patch_rows;
    Tracks T;
    std::vector<int32_t> visible, cand;
    std::vector<uint8_t> connected;
    std::vector<std::vector<int32_t>> codes((size_t)n);
    Result R;
    int32_t rounds = 0;
    PairIndex ix;
    double ms_tracks = 0, ms_total = 0;
    std::vector<double> all_tracks, all_total;          // of every repeat
    for (int rep = 0; rep < (repeats > 0 ? repeats : 1); ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int64_t k = 0; k < N; ++k) {
            const int32_t f = frame_of(first.data(), n, (int32_t)k);
            const int32_t p = patch_of(xy[2 * (size_t)k], xy[2 * (size_t)k + 1], wh[2 * (size_t)f], wh[2 * (size_t)f + 1], o.patch_cols, o.patch_rows);
            if (p < 0) { std::printf("fault patch\n"); return 0; }
            patch[(size_t)k] = (uint8_t)p; key_frame[(size_t)k] = f;
        }
        if (!pair_index(n, np, pa.data(), pb.data(), &ix)) { std::printf("fault twice\n"); return 0; }
        const int32_t ip = pair_find(ix, ia, ib);
        if (ip < 0) { std::printf("fault init\n"); return 0; }
        connected = connected_frames(n, ix, pa[(size_t)ip]);
        const Corr C = corr_graph(N, key_ptr.data(), np, pa.data(), pb.data(), match_ptr.data(), matches.data());
        rounds = simulate(n, first.data(), key_frame.data(), C, pa[(size_t)ip], pb[(size_t)ip], o.min_visible, &visible);
        const auto t1 = std::chrono::steady_clock::now();
        T = make_tracks(n, key_ptr.data(), np, pa.data(), pb.data(), match_ptr.data(), matches.data());
        ms_tracks = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        for (int f = 0; f < n; ++f) {
            codes[(size_t)f].clear();
            if (connected[(size_t)f]) covis_codes(f, first.data(), T, ix, patch.data(), key_ptr.data(), patches, o.min_patch_obs, &codes[(size_t)f]);
        }
        const RankTable rt = rank_table(n, rank_ptr.data(), rank_ids.data());
        const std::vector<int64_t> tried = tried_set(nt, ta.data(), tb.data());
        std::vector<uint8_t> reg((size_t)n);
        for (int f = 0; f < n; ++f) reg[(size_t)f] = visible[(size_t)f] >= o.min_visible;
        const std::vector<int32_t> dc = directed_candidates(n, rt, tried, reg.data(), connected.data());
        cand.clear();
        for (size_t c = 0; c < dc.size() / 2; ++c) {
            const int32_t a = dc[2 * c], b = dc[2 * c + 1];
            int32_t common = 0;
            for (int lane = 0; lane < 64; ++lane)            // the kernel's lanes, one after the other
                common += common_codes(codes[(size_t)a].data(), (int32_t)codes[(size_t)a].size(), codes[(size_t)b].data(), (int32_t)codes[(size_t)b].size(), lane, 64);
            cand.push_back(a); cand.push_back(b); cand.push_back(shared_matches(a, b, first.data(), T)); cand.push_back(common);
        }
        finish(n, o, rt, tried, connected.data(), visible.data(), cand.data(), (int64_t)cand.size() / 4, &R);
        ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        all_tracks.push_back(ms_tracks); all_total.push_back(ms_total);
    }
    line("patch", patch);
    line("key_track", T.key_track); line("track_ptr", T.track_ptr); line("obs_frame", T.obs_frame); line("obs_key", T.obs_key); line("invalid", T.invalid);
    line("connected", connected); line("visible", visible); std::printf("rounds %d\n", rounds);
    line("registered", R.registered); line("may_register", R.may_register);
    std::vector<int64_t> code_ptr(1, 0), all, items;
    for (int f = 0; f < n; ++f) { all.insert(all.end(), codes[(size_t)f].begin(), codes[(size_t)f].end()); code_ptr.push_back((int64_t)all.size()); items.push_back(covis_items(f, first.data(), T)); }
    line("code_ptr", code_ptr); line("codes", all); line("items", items); line("cand", cand);
    line("out_a", R.out_a); line("out_b", R.out_b); line("out_source", R.out_source);
    const int32_t w = window_frames(lds, n, forced);
    std::printf("window %d %d\n", w, window_passes(n, w));
    std::printf("ms %.4f %.4f\n", ms_tracks, ms_total);
    std::printf("ms_tracks"); for (double v : all_tracks) std::printf(" %.4f", v); std::printf("\n");
    std::printf("ms_total"); for (double v : all_total) std::printf(" %.4f", v); std::printf("\n");
    return 0;
}
"""


def build(directory, name="expand_rule", text=DRIVER, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def case_input(case, opt, lds_bytes=160 * 1024 - 2048, forced=0, repeats=1):
    j = lambda a: " ".join(str(int(x)) for x in np.asarray(a).ravel())
    xy = " ".join("%.9g" % float(v) for v in np.asarray(case["keys"], np.float32)[:, :2].ravel())
    pairs = np.stack([case["pair_a"], case["pair_b"]], axis=1) if len(case["pair_a"]) else np.zeros((0, 2), np.int32)
    return "\n".join([j([opt[k] for k in OPT_FIELDS]), str(case["n"]), j(case["key_ptr"]), xy, j(case["sizes"]), str(len(pairs)), j(pairs), j(case["match_ptr"]),
                      j(case["matches"]), j(case["rank_ptr"]), j(case["rank_ids"]), str(len(case["tried"])), j(case["tried"]),
                      "%d %d %d %d %d" % (case["init"][0], case["init"][1], lds_bytes, forced, repeats)]) + "\n"


def run(exe, text):
    """-> {name: [ints]} (ms: floats; fault: words)"""
    out = {}
    for ln in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines():
        w = ln.split()
        out[w[0]] = w[1:] if w[0] == "fault" else [float(x) for x in w[1:]] if w[0].startswith("ms") else [int(x) for x in w[1:]]
    return out
