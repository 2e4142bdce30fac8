"""A stand-alone host program around ba_merge_rule.h (no HIP, no GPU): the checks, the components and the three driver loops on a case
read from stdin, every output printed (the points as their bits).  tests/test_merge_cpu.py builds it with the address and
undefined-behaviour sanitizers and contraction off; tools/track_merge_timing.py builds it at -O2 and reads its clock."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRIVER = r"""
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_merge_rule.h"
// stdin: max_re mode frame repeats; n; key_ptr; u v per key; registered; q per frame; t per frame; cam_intr; n_intr; models; 8 parameters
// per camera; corr_ptr; corr_key; T; x y z per track; outlier per track; track_of_key.  Doubles as hexadecimal floats.
// stdout: one line per array, its name first.
using namespace xmerge;
template <typename T> static bool rd(std::vector<T>& v) { for (auto& x : v) { long long q; if (std::scanf("%lld", &q) != 1) return false; x = (T)q; } return true; }
static bool rdd(std::vector<double>& v) { for (auto& x : v) if (std::scanf("%la", &x) != 1) return false; return true; }
template <typename V> static void line(const char* name, const V& v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); }
int main() {
    Opt o;
    int repeats, n;
    if (std::scanf("%la %d %d %d %d", &o.max_reproj_error, &o.mode, &o.frame, &repeats, &n) != 5) return 1;
    std::vector<int64_t> key_ptr((size_t)n + 1);
    if (!rd(key_ptr)) return 1;
    const size_t N = (size_t)key_ptr[(size_t)n];
    std::vector<double> xy(2 * N), q(4 * (size_t)n), t(3 * (size_t)n);
    std::vector<uint8_t> reg((size_t)n);
    std::vector<int32_t> cam_intr((size_t)n);
    if (!rdd(xy) || !rd(reg) || !rdd(q) || !rdd(t) || !rd(cam_intr)) return 1;
    int n_intr;
    if (std::scanf("%d", &n_intr) != 1) return 1;
    std::vector<int32_t> model((size_t)n_intr);
    std::vector<double> prm(8 * (size_t)n_intr);
    if (!rd(model) || !rdd(prm)) return 1;
    std::vector<int64_t> corr_ptr(N + 1);
    if (!rd(corr_ptr)) return 1;
    std::vector<int32_t> corr_key((size_t)corr_ptr[N]);
    if (!rd(corr_key)) return 1;
    int T;
    if (std::scanf("%d", &T) != 1) return 1;
    std::vector<double> points(3 * (size_t)T);
    std::vector<uint8_t> outlier((size_t)T);
    std::vector<int32_t> tok(N);
    if (!rdd(points) || !rd(outlier) || !rd(tok)) return 1;

    const In in{&o, n, key_ptr.data(), xy.data(), reg.data(), q.data(), t.data(), cam_intr.data(), n_intr, model.data(), prm.data(), corr_ptr.data(), corr_key.data(), T,
                points.data(), outlier.data(), tok.data()};
    std::vector<int32_t> frame_of_key;
    bool too_big = false;
    if (const char* f = fault(in, &frame_of_key, &too_big)) { std::printf("fault %s\n", f); return 0; }
    std::vector<double> out_points;
    std::vector<uint8_t> out_outlier, status;
    std::vector<int32_t> out_tok, have(N), visible((size_t)n), measured((size_t)n);
    std::vector<int64_t> stats(8, 0);
    std::vector<double> ms_plan, ms_run;
    Labels L;
    for (int rep = 0; rep < (repeats > 0 ? repeats : 1); ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        L = label_components(in);
        const Plan P = make_plan(in, frame_of_key, L);
        std::vector<Cam> cams((size_t)n);
        for (int f = 0; f < n; ++f) cams[(size_t)f] = cam_of(in, f);
        State S = initial_state(in, P);
        const auto t1 = std::chrono::steady_clock::now();
        run_host(P, cams.data(), o, &S);
        out_points = points; out_outlier = outlier; out_tok = tok; status.assign((size_t)T, 0);
        scatter(P, S.key_trk.data(), S.pts.data(), S.outlier.data(), out_points.data(), out_outlier.data(), out_tok.data(), status.data());
        if (N) counts_host(in, out_tok.data(), have.data(), visible.data(), measured.data());
        const auto t2 = std::chrono::steady_clock::now();
        for (int k = 0; k < 4; ++k) stats[(size_t)k] = S.counters[k];
        stats[4] = P.n_comp; stats[5] = P.n_skipped; stats[6] = P.largest;
        ms_plan.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        ms_run.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::vector<unsigned long long> bits(out_points.size());
    if (!bits.empty()) std::memcpy(bits.data(), out_points.data(), sizeof(double) * bits.size());
    std::printf("point_bits"); for (auto b : bits) std::printf(" %llu", b); std::printf("\n");
    line("track_of_key", out_tok); line("track_outlier", out_outlier); line("track_status", status); line("corr_have_point3d", have);
    line("visible", visible); line("measured", measured); line("stats", stats); line("comp_of_key", L.comp_of_key);
    std::printf("ms_plan"); for (double v : ms_plan) std::printf(" %.4f", v); std::printf("\n");
    std::printf("ms_run"); for (double v : ms_run) std::printf(" %.4f", v); std::printf("\n");
    return 0;
}
"""


def build(directory, name="merge_rule", flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def case_input(case, mode, repeats=1, frame=None, max_re=None):
    j = lambda a: " ".join(str(int(x)) for x in np.asarray(a).ravel())
    d = lambda a: " ".join(float(x).hex() for x in np.asarray(a, np.float64).ravel())
    n = len(case["key_ptr"]) - 1
    return "\n".join(["%s %d %d %d %d" % (float(case["max_re"] if max_re is None else max_re).hex(), mode, case["frame"] if frame is None else frame, repeats, n),
                      j(case["key_ptr"]), d(case["key_xy"]), j(case["registered"]), d(case["cam_q"]), d(case["cam_t"]), j(case["cam_intr"]), str(len(case["intr_model"])),
                      j(case["intr_model"]), d(case["intr_params"]), j(case["corr_ptr"]), j(case["corr_key"]), str(len(case["points"])), d(case["points"]),
                      j(case["track_outlier"]), j(case["track_of_key"])]) + "\n"


def run(exe, text):
    """-> {name: [ints]} (ms_*: floats; fault: words)"""
    out = {}
    for ln in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines():
        w = ln.split()
        out[w[0]] = w[1:] if w[0] == "fault" else [float(x) for x in w[1:]] if w[0].startswith("ms") else [int(x) for x in w[1:]]
    return out
