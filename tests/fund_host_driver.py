"""Stand-alone host programs around ba_fund_scan.h and ba_fund_geom.h (no HIP, no GPU): the scan fed with per-model records, and a
sequential driver of whole pairs.  tests/test_fund_cpu.py builds them with the address and undefined-behaviour sanitizers;
tools/pair_verify_timing.py builds the pair driver with -O2 as the CPU column of its table."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

SCAN_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_fund_scan.h"
// per pair: "n trial_cap min_num_trials confidence R", then R records "trial count sum local_count local_sum" in the order the
// models were offered (local_count -2: no local optimisation was due, -1: it gave no model); one line
// "best_trial_code num_trials best_count success err".  err bit 0: a record after the scan has stopped; bit 1: a local
// optimisation due where the record has none, or the reverse; bit 2: the records end and the scan has not seen its last model.
int main() {
    int n, cap, mint, R;
    double conf;
    while (std::scanf("%d %d %d %lf %d", &n, &cap, &mint, &conf, &R) == 5) {
        std::vector<int32_t> row(n + 1);
        for (int k = 0; k <= n; ++k) row[k] = xfund::fund_dyn_trials(k, n, conf);
        xfund::Scan sc(row.data(), cap, mint);
        int err = 0, last_t = -1;
        for (int i = 0; i < R; ++i) {
            int t, cnt, lcnt;
            double sum, lsum;
            if (std::scanf("%d %d %lf %d %lf", &t, &cnt, &sum, &lcnt, &lsum) != 5) return 1;
            if (sc.abort || t >= sc.max_trials || t < last_t) err |= 1;
            last_t = t;
            const xfund::Offer o = sc.offer(t, cnt, sum);
            if ((o == xfund::kNewBestLocal) != (lcnt != -2)) err |= 2;
            if (o == xfund::kNewBestLocal && lcnt >= 0) sc.offer_local(lcnt, lsum);
            sc.after_model(t);
        }
        std::printf("%d %d %d %d %d\n", sc.best_trial_code(), sc.num_trials, sc.best_count, sc.finish() ? 1 : 0, err);
    }
    return 0;
}
"""

PAIR_DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_fund_geom.h"
// ba_fund_scan.h and ba_fund_geom.h in a sequential driver of whole pairs.  Per pair: "n max_error confidence min_inlier_ratio
// min_num_trials max_num_trials seed min_matches min_num_inliers min_accept_ratio", then n lines "x_a y_a x_b y_b"; one line per
// pair: "status num_inliers num_trials best_trial accepted F[9] m<mask>".  With the argument "time" the total time of the solves
// goes to stderr in milliseconds.
using namespace xfund;
static void support(const double* F, const std::vector<double>& m, int n, double max_res, int& cnt, double& sum, unsigned char* inl) {
    cnt = 0; sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double r = sampson(F, m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
        const bool in = is_inlier(r, max_res);
        if (in) { ++cnt; sum += r; }
        if (inl) inl[k] = in ? 1 : 0;
    }
}
template <int M, class Fn>
static void inlier_sum(Eight& w, const std::vector<double>& m, int n, const unsigned char* inl, Fn term) {
    double acc[M];
    for (int e = 0; e < M; ++e) acc[e] = 0.0;
    for (int k = 0; k < n; ++k) if (inl[k]) term(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3], acc);
    for (int e = 0; e < M; ++e) w.red[e] = acc[e];
}
int main(int argc, char** argv) {
    const bool timing = argc > 1 && !std::strcmp(argv[1], "time");
    double total_ms = 0.0;
    int n, mint, maxt, minmatches, mininl; unsigned seed;
    double maxerr, conf, ratio, accratio;
    while (std::scanf("%d %lf %lf %lf %d %d %u %d %d %lf", &n, &maxerr, &conf, &ratio, &mint, &maxt, &seed, &minmatches, &mininl, &accratio) == 10) {
        std::vector<double> m(4 * (size_t)n + 4);
        for (int k = 0; k < n; ++k)
            if (std::scanf("%lf %lf %lf %lf", &m[4 * k], &m[4 * k + 1], &m[4 * k + 2], &m[4 * k + 3]) != 4) return 1;
        int status = 0, ninl = 0, ntr = 0, best = -1, accepted = 0;
        double Fn[9] = {0};
        std::vector<unsigned char> mask(n, 0), inl(n + 1, 0);
        const auto t0 = std::chrono::steady_clock::now();
        if (n < minmatches) status = 2;
        else if (n > kMaxMatches) status = 3;
        else {
            const int cap = maxt < fund_ratio_trials(ratio, conf) ? maxt : fund_ratio_trials(ratio, conf);
            std::vector<int32_t> row(n + 1), idx(n);
            std::vector<uint32_t> mt(624);
            for (int k = 0; k <= n; ++k) row[k] = fund_dyn_trials(k, n, conf);
            Sampler gen{mt.data(), idx.data(), 0, n};
            gen.seed(seed);
            for (int k = 0; k < n; ++k) idx[k] = k;
            std::vector<double> w(kWs7);
            PlainWs ws{w.data()};
            Scan sc(row.data(), cap, mint);
            const double max_res = maxerr * maxerr;
            double bestF[9], models[27];
            Eight e8;
            for (int t = 0; t < cap && !sc.abort; ++t) {
                int32_t tup[7];
                gen.draw(tup);
                for (int j = 0; j < 7; ++j) seven_point_row(ws, j, m[4 * (size_t)tup[j]], m[4 * (size_t)tup[j] + 1], m[4 * (size_t)tup[j] + 2], m[4 * (size_t)tup[j] + 3]);
                const int nm = seven_point_models(ws, models);
                for (int s = 0; s < nm; ++s) {
                    int cnt; double sum;
                    support(models + 9 * s, m, n, max_res, cnt, sum, nullptr);
                    const Offer o = sc.offer(t, cnt, sum);
                    if (o != kIgnored) {
                        for (int e = 0; e < 9; ++e) bestF[e] = models[9 * s + e];
                        if (o == kNewBestLocal) {
                            support(bestF, m, n, max_res, cnt, sum, inl.data());
                            inlier_sum<5>(e8, m, n, inl.data(), [&](double xa, double ya, double xb, double yb, double* acc) { eight_terms1(xa, ya, xb, yb, acc); });
                            eight_stage_centroid(e8);
                            inlier_sum<2>(e8, m, n, inl.data(), [&](double xa, double ya, double xb, double yb, double* acc) { eight_terms2(e8, xa, ya, xb, yb, acc); });
                            eight_stage_scale(e8);
                            inlier_sum<45>(e8, m, n, inl.data(), [&](double xa, double ya, double xb, double yb, double* acc) { eight_terms3(e8, xa, ya, xb, yb, acc); });
                            if (eight_stage_model(e8)) {
                                int lc; double ls;
                                support(e8.F, m, n, max_res, lc, ls, nullptr);
                                if (sc.offer_local(lc, ls)) for (int e = 0; e < 9; ++e) bestF[e] = e8.F[e];
                            }
                        }
                    }
                    if (sc.after_model(t)) break;
                }
            }
            if (sc.finish()) {
                normalise_model(bestF, Fn);
                if (xpnp::all_finite(Fn, 9)) {
                    double fs;
                    support(bestF, m, n, max_res, ninl, fs, mask.data());
                    status = 1; ntr = sc.num_trials; best = sc.best_trial_code();
                    const int thr = mininl > (int)(accratio * (double)n) ? mininl : (int)(accratio * (double)n);
                    accepted = ninl >= thr;
                } else {
                    for (int e = 0; e < 9; ++e) Fn[e] = 0.0;
                }
            }
        }
        total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%d %d %d %d %d", status, ninl, ntr, best, accepted);
        for (int k = 0; k < 9; ++k) std::printf(" %.17g", Fn[k]);
        std::printf(" m");
        for (int k = 0; k < n; ++k) std::printf("%d", (int)mask[k]);
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


def pair_input(xa, xb, opt, max_error=None, seed=None):
    """the stdin text of one pair for PAIR_DRIVER; opt has the fields of fund_yardstick.Options"""
    head = "%d %r %r %r %d %d %d %d %d %r" % (len(xa), float(opt.max_error if max_error is None else max_error), opt.confidence, opt.min_inlier_ratio,
                                               opt.min_num_trials, opt.max_num_trials, opt.seed if seed is None else seed, opt.min_matches,
                                               opt.min_num_inliers, opt.min_accept_ratio)
    return "\n".join([head] + ["%r %r %r %r" % (float(a[0]), float(a[1]), float(b[0]), float(b[1])) for a, b in zip(xa, xb)])


def parse_pair(line, n):
    w = line.split()
    r = dict(status=int(w[0]), num_inliers=int(w[1]), num_trials=int(w[2]), best_trial=int(w[3]), accepted=int(w[4]),
             F=np.array([float(x) for x in w[5:14]]))
    r["mask"] = np.array([int(c) for c in w[14][1:]], np.uint8)
    assert len(r["mask"]) == n
    return r
