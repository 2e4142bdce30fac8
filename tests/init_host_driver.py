"""Stand-alone host programs around ba_init_scan.h and ba_init_geom.h (no HIP, no GPU): the scan fed with per-model records, and a
sequential driver of whole pairs.  tests/test_init_cpu.py builds them with the address and undefined-behaviour sanitizers;
tools/two_view_timing.py builds the pair driver with -O2 as the CPU column of its table."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

SCAN_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_init_scan.h"
// per pair: "n max_iterations confidence R", then R records "trial slot count score" in the order the models were offered (slot -1:
// a trial without a model); one line "best_code bound num_trials best_count err".  A record of a trial the scan would not have run,
// or records that end before the scan does, are errors.
int main() {
    int n, maxit, R;
    double conf;
    while (std::scanf("%d %d %lf %d", &n, &maxit, &conf, &R) == 4) {
        std::vector<int32_t> row(n + 1);
        xinit::init_bound_row(n, conf, row.data());
        xinit::Scan sc(row.data(), maxit);
        int err = 0, trials = 0;
        for (int i = 0; i < R; ++i) {
            int t, slot, cnt;
            double score;
            if (std::scanf("%d %d %d %lf", &t, &slot, &cnt, &score) != 4) return 1;
            if (t + 1 > trials) {                          // a new trial: the loop test at its top
                if (t != trials || !sc.more(t)) err |= 1;
                trials = t + 1;
            }
            if (slot >= 0) sc.offer(t, slot, cnt, score);
        }
        if (sc.more(trials)) err |= 2;                     // the records end where the loop ends
        std::printf("%d %d %d %d %d\n", sc.best_code, sc.bound, trials, sc.best_count, err);
    }
    return 0;
}
"""

PAIR_DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_init_geom.h"
// ba_init_scan.h and ba_init_geom.h in a sequential driver of whole pairs.  Per pair: "n max_iterations confidence seed th max_depth
// n_angles a0 a1 a2 a3 min_front_ratio min_angle_ratio min_num_valid min_matches", then n lines "x1 y1 x2 y2"; one line per pair:
// "status num_trials best_trial accepted counts[8] E[9] q[4] t[3] e<mask> f<mask> points of the front mask".  With the argument
// "time" the total time of the solves goes to stderr in milliseconds.
using namespace xinit;
int main(int argc, char** argv) {
    const bool timing = argc > 1 && !std::strcmp(argv[1], "time");
    double total_ms = 0.0;
    int n, maxit, nang, minvalid, minmatches; unsigned seed;
    double conf, th, maxdepth, ang[4], fr, ar;
    while (std::scanf("%d %d %lf %u %lf %lf %d %lf %lf %lf %lf %lf %lf %d %d", &n, &maxit, &conf, &seed, &th, &maxdepth, &nang, &ang[0], &ang[1], &ang[2],
                      &ang[3], &fr, &ar, &minvalid, &minmatches) == 15) {
        std::vector<double> m(4 * (size_t)n);
        for (int k = 0; k < n; ++k)
            if (std::scanf("%lf %lf %lf %lf", &m[4 * k], &m[4 * k + 1], &m[4 * k + 2], &m[4 * k + 3]) != 4) return 1;
        int status = 0, trials = 0, best = -1, accepted = 0, counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double En[9] = {0}, q[4] = {0}, t[3] = {0};
        std::vector<unsigned char> em(n, 0), fm(n, 0);
        std::vector<double> pts(3 * (size_t)n, 0.0);
        const auto t0 = std::chrono::steady_clock::now();
        if (n < minmatches) status = 2;
        else if (n > kMaxMatches) status = 3;
        else {
            std::vector<int32_t> row(n + 1), idx(n), quint(5 * (size_t)maxit);
            init_bound_row(n, conf, row.data());
            init_sample_quintuples(seed, n, maxit, idx.data(), quint.data());
            std::vector<double> w(kWsDoubles);
            PlainWs ws{w.data()};
            Scan sc(row.data(), maxit);
            const double th2 = 2.0 * th * th;
            double bestE[9], models[9 * kMaxModels];
            for (; sc.more(trials); ++trials) {
                double p5[20];
                for (int k = 0; k < 5; ++k) for (int e = 0; e < 4; ++e) p5[4 * k + e] = m[4 * (size_t)quint[5 * trials + k] + e];
                const int nm = five_point_models(ws, p5, models);
                for (int s = 0; s < nm; ++s) {
                    Support sp;
                    for (int k = 0; k < n; ++k) sp.add(sampson(models + 9 * s, m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]), th2);
                    if (sc.offer(trials, s, sp.count, sp.score)) for (int e = 0; e < 9; ++e) bestE[e] = models[9 * s + e];
                }
            }
            best = sc.best_code;
            double R1[9], R2[9], T[3];
            bool ok = best >= 0;
            if (ok) {
                double nn = 0.0;
                for (int e = 0; e < 9; ++e) nn += bestE[e] * bestE[e];
                for (int e = 0; e < 9; ++e) En[e] = bestE[e] * (1.0 / sqrt(nn));
                decompose_essential(En, R1, R2, T);
                ok = finite9(En) && finite9(R1) && finite9(R2);
                if (!ok) for (int e = 0; e < 9; ++e) En[e] = 0.0;
            }
            if (ok) {
                counts[0] = sc.best_count;
                int front[4] = {0, 0, 0, 0};
                std::vector<unsigned char> flags(n, 0);
                for (int k = 0; k < n; ++k) {
                    em[k] = sampson(bestE, m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]) < th2;
                    for (int c = 0; c < 4; ++c) {
                        double R[9], tt[3], ctr[3], p[3];
                        candidate(R1, R2, T, c, R, tt, ctr);
                        if (check_point(R, tt, m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3], maxdepth, p)) { flags[k] |= 1 << c; ++front[c]; }
                    }
                }
                int bk = 0, bn = 0;
                for (int c = 0; c < 4; ++c) if (front[c] > bn) { bn = front[c]; bk = c; }
                if (bn > 0) {
                    status = 1;
                    double R[9], ctr[3];
                    const double zero[3] = {0.0, 0.0, 0.0};
                    candidate(R1, R2, T, bk, R, t, ctr);
                    quat_of(R, q);
                    counts[1] = bn; counts[2] = bk;
                    for (int k = 0; k < n; ++k) {
                        if (!((flags[k] >> bk) & 1)) continue;
                        fm[k] = 1;
                        check_point(R, t, m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3], maxdepth, &pts[3 * (size_t)k]);
                        const double a = tri_angle(zero, ctr, &pts[3 * (size_t)k]);
                        for (int i = 0; i < nang; ++i) if (a > ang[i]) ++counts[4 + i];
                    }
                    for (int i = 0; i < nang; ++i) if (accept(n, bn, counts[4 + i], fr, ar, minvalid)) accepted |= 1 << i;
                }
            }
        }
        total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%d %d %d %d", status, trials, best, accepted);
        for (int k = 0; k < 8; ++k) std::printf(" %d", counts[k]);
        for (int k = 0; k < 9; ++k) std::printf(" %.17g", En[k]);
        for (int k = 0; k < 4; ++k) std::printf(" %.17g", q[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", t[k]);
        std::printf(" e");
        for (int k = 0; k < n; ++k) std::printf("%d", (int)em[k]);
        std::printf(" f");
        for (int k = 0; k < n; ++k) std::printf("%d", (int)fm[k]);
        for (int k = 0; k < n; ++k) if (fm[k]) std::printf(" %.17g %.17g %.17g", pts[3 * (size_t)k], pts[3 * (size_t)k + 1], pts[3 * (size_t)k + 2]);
        std::printf("\n");
    }
    if (timing) std::fprintf(stderr, "ms %.3f\n", total_ms);
    return 0;
}
"""


def build(directory, name, text, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def pair_input(xa, xb, th, opt):
    """the stdin text of one pair for PAIR_DRIVER; opt has the fields of init_yardstick.Options"""
    ang = list(opt.min_angle_rad) + [0.0] * (4 - len(opt.min_angle_rad))
    head = "%d %d %r %d %r %r %d %r %r %r %r %r %r %d %d" % (len(xa), opt.max_iterations, opt.confidence, opt.seed, float(th), opt.max_depth,
                                                               len(opt.min_angle_rad), *ang, opt.min_front_ratio, opt.min_angle_ratio,
                                                               opt.min_num_valid, opt.min_matches)
    return "\n".join([head] + ["%r %r %r %r" % (float(a[0]), float(a[1]), float(b[0]), float(b[1])) for a, b in zip(xa, xb)])


def parse_pair(line, n):
    w = line.split()
    r = dict(status=int(w[0]), num_trials=int(w[1]), best_trial=int(w[2]), accepted=int(w[3]), counts=np.array([int(x) for x in w[4:12]], np.int32),
             E=np.array([float(x) for x in w[12:21]]), q=np.array([float(x) for x in w[21:25]]), t=np.array([float(x) for x in w[25:28]]))
    r["essential_mask"] = np.array([int(c) for c in w[28][1:]], np.uint8)
    r["front_mask"] = np.array([int(c) for c in w[29][1:]], np.uint8)
    assert len(r["essential_mask"]) == n and len(r["front_mask"]) == n
    r["points"] = np.zeros((n, 3))
    r["points"][r["front_mask"].astype(bool)] = np.array([float(x) for x in w[30:]]).reshape(-1, 3)
    return r
