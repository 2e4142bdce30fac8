"""A stand-alone host program around ba_frames_rule.h (no HIP, no GPU): the rank rule of k_frames_order walked in the kernel's slices,
the plan of the sub-batches of a pair list, and the acceptance threshold.  tests/test_frames_cpu.py builds it with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SLICE = 256          # kFramesThreads

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_frames_rule.h"
// Commands on stdin, one answer line each on stdout:
//   rank n width, then n (row col) in the order of emission      -> the n ranks, summed over slices of 256 codes padded with INT64_MAX
//   plan n_frames n_pairs strip budget, then the clip of every frame, then n_pairs (a b), then n_pairs counts
//        -> "live", then per sub-batch "| first last pairs rows cols parts items" and per pair of it "p row col part item strips beg"
//   accept min_num_inliers ratio n                                -> the threshold
using namespace xframes;
int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "rank")) {
            int n, w;
            if (std::scanf("%d %d", &n, &w) != 2) return 1;
            std::vector<int64_t> code((size_t)n);
            for (int k = 0; k < n; ++k) { int r, c; if (std::scanf("%d %d", &r, &c) != 2) return 1; code[(size_t)k] = order_code(r, c, w); }
            for (int k = 0; k < n; ++k) {
                int32_t rank = 0;
                for (int base = 0; base < n; base += 256) {
                    int64_t slice[256];
                    for (int t = 0; t < 256; ++t) slice[t] = base + t < n ? code[(size_t)(base + t)] : INT64_MAX;
                    rank += order_below(slice, 256, code[(size_t)k]);
                }
                std::printf("%d ", rank);
            }
            std::printf("\n");
        } else if (!std::strcmp(cmd, "plan")) {
            int nf, np, strip;
            long long budget;
            if (std::scanf("%d %d %d %lld", &nf, &np, &strip, &budget) != 4) return 1;
            std::vector<int32_t> clip((size_t)nf), pa((size_t)np), pb((size_t)np), cnt((size_t)np);
            for (auto& x : clip) if (std::scanf("%d", &x) != 1) return 1;
            for (int p = 0; p < np; ++p) if (std::scanf("%d %d", &pa[(size_t)p], &pb[(size_t)p]) != 2) return 1;
            for (auto& x : cnt) if (std::scanf("%d", &x) != 1) return 1;
            std::vector<int32_t> live, na, nb;
            plan_live(np, pa.data(), pb.data(), clip.data(), &live, &na, &nb);
            auto bytes = [](const BatchSize& s) { return (size_t)(64 * s.pairs + 8 * s.rows + 4 * s.cols + 12 * s.parts + 8 * s.items); };
            std::printf("live");
            for (const Batch& b : plan_split(live.size(), na.data(), nb.data(), strip, (size_t)budget, bytes)) {
                std::printf(" | %zu %zu %lld %lld %lld %lld %lld", b.first, b.last, (long long)b.size.pairs, (long long)b.size.rows, (long long)b.size.cols,
                            (long long)b.size.parts, (long long)b.size.items);
                BatchSize s;
                std::vector<int32_t> c, beg(b.last - b.first);
                for (size_t k = b.first; k < b.last; ++k) c.push_back(cnt[(size_t)live[k]]);
                int64_t total = 0;
                if (!plan_gather(c.size(), c.data(), beg.data(), &total)) return 2;
                for (size_t k = b.first; k < b.last; ++k) {
                    const PairSpan sp = plan_append(s, na[k], nb[k], strip);
                    std::printf(" %d %lld %lld %lld %lld %d %d", live[k], (long long)sp.row_off, (long long)sp.col_off, (long long)sp.part_off, (long long)sp.item_off,
                                sp.strips, beg[k - b.first]);
                }
                if (s.rows != b.size.rows || s.cols != b.size.cols || s.parts != b.size.parts || s.items != b.size.items || s.pairs != b.size.pairs) return 3;
            }
            std::printf("\n");
        } else if (!std::strcmp(cmd, "accept")) {
            int mn, n;
            double ratio;
            if (std::scanf("%d %lf %d", &mn, &ratio, &n) != 3) return 1;
            std::printf("%d\n", accept_threshold(mn, ratio, n));
        } else {
            return 1;
        }
    }
    return 0;
}
"""


def build(directory, name="frames_rule", text=DRIVER, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def rank_input(rows, cols, width):
    return "rank %d %d\n%s\n" % (len(rows), width, " ".join("%d %d" % rc for rc in zip(rows, cols)))


def plan_input(clip, pair_a, pair_b, counts, strip, budget):
    return "plan %d %d %d %d\n%s\n%s\n%s\n" % (len(clip), len(pair_a), strip, budget, " ".join(map(str, clip)),
                                             " ".join("%d %d" % ab for ab in zip(pair_a, pair_b)), " ".join(map(str, counts)))


def parse_plan(line):
    """-> [dict(first, last, size (pairs, rows, cols, parts, items), pairs [(p, row, col, part, item, strips, beg)])]"""
    parts = line.split("|")
    assert parts[0].strip() == "live"
    out = []
    for blk in parts[1:]:
        w = [int(x) for x in blk.split()]
        out.append(dict(first=w[0], last=w[1], size=tuple(w[2:7]), pairs=[tuple(w[k:k + 7]) for k in range(7, len(w), 7)]))
    return out
