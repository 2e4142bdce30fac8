"""A stand-alone host program around ba_match_rule.h (no HIP, no GPU): a sequential driver of whole pairs with scalar dot products.
tests/test_match_cpu.py builds it with the address and undefined-behaviour sanitizers; tools/descriptor_match_timing.py builds it
with -O2 as the CPU column of its table."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PAIR_DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_match_rule.h"
// Per pair on stdin: "n_a n_b max_distance max_ratio mutual_best max_features" (the two floats as the hexadecimal of their bits),
// then (n_a + n_b) * 128 components.  Per pair on stdout: "n_match num_row num_col", then the row triples, the column triples and
// the matches, all integers on one line.  With the argument "time" the total time of the pairs goes to stderr in milliseconds.
using namespace xmatch;
int main(int argc, char** argv) {
    const bool timing = argc > 1 && !std::strcmp(argv[1], "time");
    std::vector<float> tab(kTabSize);
    match_build_table(tab.data());
    double total_ms = 0.0;
    int na, nb, mutual, maxf;
    unsigned dbits, rbits;
    while (std::scanf("%d %d %x %x %d %d", &na, &nb, &dbits, &rbits, &mutual, &maxf) == 6) {
        float max_distance, max_ratio;
        std::memcpy(&max_distance, &dbits, 4); std::memcpy(&max_ratio, &rbits, 4);
        std::vector<uint8_t> a((size_t)na * kDim), b((size_t)nb * kDim);
        for (auto* v : {&a, &b})
            for (auto& x : *v) { int c; if (std::scanf("%d", &c) != 1) return 1; x = (uint8_t)c; }
        const auto t0 = std::chrono::steady_clock::now();
        const int ca = na < maxf ? na : maxf, cb = nb < maxf ? nb : maxf;
        std::vector<Top> rt((size_t)ca, top_init()), ct((size_t)cb, top_init());
        for (int i = 0; i < ca; ++i)
            for (int j = 0; j < cb; ++j) {
                int32_t d = 0;
                for (int k = 0; k < kDim; ++k) d += (int32_t)a[(size_t)i * kDim + k] * (int32_t)b[(size_t)j * kDim + k];
                top_update(rt[i], d, j);
                top_update(ct[j], d, i);
            }
        std::vector<int32_t> rm((size_t)ca), cm((size_t)cb), m(2 * (size_t)ca + 2);
        int nrow = 0, ncol = 0;
        for (int i = 0; i < ca; ++i) { rm[i] = match_of(tab.data(), rt[i], max_distance, max_ratio); nrow += rm[i] >= 0; }
        for (int j = 0; j < cb; ++j) { cm[j] = match_of(tab.data(), ct[j], max_distance, max_ratio); ncol += cm[j] >= 0; }
        const int n = match_compact(ca, rm.data(), cm.data(), mutual, m.data());
        total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        // the merge: two halves of the columns merged in both orders give the row's triple again
        for (int i = 0; i < ca; ++i) {
            Top lo = top_init(), hi = top_init();
            for (int j = 0; j < cb; ++j) {
                int32_t d = 0;
                for (int k = 0; k < kDim; ++k) d += (int32_t)a[(size_t)i * kDim + k] * (int32_t)b[(size_t)j * kDim + k];
                top_update(j < cb / 2 ? lo : hi, d, j);
            }
            const Top x = top_merge(lo, hi), y = top_merge(hi, lo);
            if (x.best != rt[i].best || x.idx != rt[i].idx || x.next != rt[i].next || y.best != x.best || y.idx != x.idx || y.next != x.next) return 2;
        }
        std::printf("%d %d %d", n, nrow, ncol);
        for (int i = 0; i < ca; ++i) std::printf(" %d %d %d", rt[i].best, rt[i].idx, rt[i].next);
        for (int j = 0; j < cb; ++j) std::printf(" %d %d %d", ct[j].best, ct[j].idx, ct[j].next);
        for (int k = 0; k < 2 * n; ++k) std::printf(" %d", m[k]);
        std::printf("\n");
    }
    if (timing) std::fprintf(stderr, "ms %.3f\n", total_ms);
    return 0;
}
"""


def build(directory, name="match_pairs", text=PAIR_DRIVER, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def pair_input(a, b, opt):
    """the stdin text of one pair; opt a dict with the fields of xrsfm_ba_match_options"""
    bits = lambda x: "%x" % int(np.float32(x).view(np.uint32))
    head = "%d %d %s %s %d %d" % (len(a), len(b), bits(opt["max_distance"]), bits(opt["max_ratio"]), opt["mutual_best"], opt["max_features"])
    return head + "\n" + " ".join(map(str, np.concatenate([a.ravel(), b.ravel()]).tolist()))


def parse_pair(line, n_a, n_b):
    w = np.array(line.split(), np.int64)
    n = int(w[0])
    assert len(w) == 3 + 3 * (n_a + n_b) + 2 * n
    return dict(num_row=int(w[1]), num_col=int(w[2]), row_top=w[3:3 + 3 * n_a].reshape(-1, 3).astype(np.int32),
                col_top=w[3 + 3 * n_a:3 + 3 * (n_a + n_b)].reshape(-1, 3).astype(np.int32),
                matches=w[3 + 3 * (n_a + n_b):].reshape(-1, 2).astype(np.int32))
