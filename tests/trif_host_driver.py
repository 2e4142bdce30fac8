"""A stand-alone host program around ba_trif_rule.h (no HIP, no GPU): the checks, the plan and the steps as plain loops on a case read
from stdin, every output printed (the points as their bits); the create results are data (the yardstick's, per slot).  A second mode
evaluates the dot-product rule on given values.  tests/test_trif_cpu.py builds it with the address and undefined-behaviour sanitizers
and contraction off and runs it as a process."""
import os
import subprocess

import numpy as np

from tests import trif_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRIVER = r"""
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_trif_rule.h"
// stdin, "case": extend_angle_rad; n; key_ptr; x y per key; registered; q per frame; t per frame; corr_ptr; corr_key; n_list; the list; T;
// capacity; x y z per track; outlier per track; track_of_key; n_slots; per slot status (255: not supplied) and x y z; n_obs; the masks.
// stdin, "unit": th; k; k dot products.  Doubles as hexadecimal floats.  stdout: one line per array, its name first.
using namespace xtrif;
template <typename T> static bool rd(std::vector<T>& v) { for (auto& x : v) { long long q; if (std::scanf("%lld", &q) != 1) return false; x = (T)q; } return true; }
static bool rdd(std::vector<double>& v) { for (auto& x : v) if (std::scanf("%la", &x) != 1) return false; return true; }
template <typename V> static void line(const char* name, const V& v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); }
static unsigned long long bits_of(double d) { unsigned long long b; std::memcpy(&b, &d, sizeof b); return b; }
int main() {
    char mode[16];
    if (std::scanf("%15s", mode) != 1) return 1;
    if (!std::strcmp(mode, "unit")) {
        double th; int k;
        if (std::scanf("%la %d", &th, &k) != 2) return 1;
        std::vector<double> d((size_t)k);
        if (!rdd(d)) return 1;
        const double bound = dot_bound(th);
        std::printf("bound %llu\n", bits_of(bound));
        std::vector<int> valid, acc, b01, b10;
        for (int i = 0; i < k; ++i) {
            const double e = d[(size_t)((i + 1) % k)];
            valid.push_back(dot_valid(d[(size_t)i])); acc.push_back(accepts(d[(size_t)i], bound));
            b01.push_back(better(d[(size_t)i], 1, e, 0)); b10.push_back(better(d[(size_t)i], 0, e, 1));
        }
        line("valid", valid); line("accepts", acc); line("better_larger_id", b01); line("better_smaller_id", b10);
        return 0;
    }
    Opt o{};
    o.tri = TriOpt{0.0261799387799149, 0.0349065850398866, 0.9999, 0.02, 10000, 15};
    int n;
    if (std::scanf("%la %d", &o.extend_angle_rad, &n) != 2) return 1;
    std::vector<int64_t> key_ptr((size_t)n + 1);
    if (!rd(key_ptr)) return 1;
    const size_t N = (size_t)key_ptr[(size_t)n];
    std::vector<double> xy(2 * N), q(4 * (size_t)n), t(3 * (size_t)n);
    std::vector<uint8_t> reg((size_t)n);
    if (!rdd(xy) || !rd(reg) || !rdd(q) || !rdd(t)) return 1;
    std::vector<int64_t> corr_ptr(N + 1);
    if (!rd(corr_ptr)) return 1;
    std::vector<int32_t> corr_key((size_t)corr_ptr[N]);
    if (!rd(corr_key)) return 1;
    int n_list;
    if (std::scanf("%d", &n_list) != 1) return 1;
    std::vector<int32_t> list((size_t)n_list);
    if (!rd(list)) return 1;
    int T; long long cap;
    if (std::scanf("%d %lld", &T, &cap) != 2) return 1;
    std::vector<double> points(3 * (size_t)T);
    std::vector<uint8_t> outlier((size_t)T);
    std::vector<int32_t> tok(N);
    if (!rdd(points) || !rd(outlier) || !rd(tok)) return 1;
    if (cap > T) { points.resize(3 * (size_t)cap, 0.0); outlier.resize((size_t)cap, 0); }      // the caller's arrays have the capacity
    int n_slots;
    if (std::scanf("%d", &n_slots) != 1) return 1;
    std::vector<uint8_t> cr_status((size_t)n_slots);
    std::vector<double> cr_points(3 * (size_t)n_slots);
    for (int s = 0; s < n_slots; ++s) {
        int st;
        if (std::scanf("%d %la %la %la", &st, &cr_points[3 * (size_t)s], &cr_points[3 * (size_t)s + 1], &cr_points[3 * (size_t)s + 2]) != 4) return 1;
        cr_status[(size_t)s] = (uint8_t)st;
    }
    int n_obs;
    if (std::scanf("%d", &n_obs) != 1) return 1;
    std::vector<uint8_t> cr_mask((size_t)n_obs);
    if (!rd(cr_mask)) return 1;

    const In in{&o, n, key_ptr.data(), xy.data(), reg.data(), q.data(), t.data(), corr_ptr.data(), corr_key.data(), n_list, list.data(), T, cap, points.data(), outlier.data(),
                tok.data()};
    std::vector<int32_t> frame_of_key;
    bool too_big = false;
    if (const char* f = fault(in, &frame_of_key, &too_big)) { std::printf("fault %s\n", f); return 0; }
    const auto t0 = std::chrono::steady_clock::now();
    const Plan P = make_plan(in, frame_of_key);
    const double ms_plan = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (const char* f = capacity_fault(in, P)) { std::printf("fault %s\n", f); return 0; }
    if (P.n_slots() != n_slots || (int)P.obs_key.size() != n_obs) { std::printf("fault the plan has %d slots and %d observations\n", P.n_slots(), (int)P.obs_key.size()); return 0; }
    const State S = run_host(in, P, Created{cr_status.data(), cr_points.data(), cr_mask.data()});
    if (S.missing) { std::printf("fault a create result was needed that was not supplied\n"); return 0; }
    std::printf("point_bits"); for (int32_t i = 0; i < 3 * S.n_tracks; ++i) std::printf(" %llu", bits_of(S.points[(size_t)i])); std::printf("\n");
    std::vector<int64_t> stats(S.stats, S.stats + 8), nt(1, S.n_tracks);
    std::vector<uint8_t> out(S.outlier.begin(), S.outlier.begin() + S.n_tracks);
    line("track_of_key", S.track_of_key); line("track_outlier", out); line("key_status", S.key_status); line("n_tracks", nt); line("stats", stats);
    line("slot_key", P.slot_key); line("step_slot0", P.step_slot0); line("step_frame", P.step_frame);
    std::printf("ms_plan %.4f\n", ms_plan);
    return 0;
}
"""


def build(directory, name="trif_rule", flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def _j(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def _d(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).ravel())


def case_input(case, frames, expected=None, create=None, capacity=None, **changed):
    """the program's input for a case; the create results of the slots that `expected` (a run_flat result) created or failed to create
    come from the callback, the others are not supplied"""
    c = dict(case, **changed)
    P = Y.plan(case, [f for f in frames if 0 <= f < len(case["registered"])]) if expected is not None else dict(slot_key=[], lists=[])
    fok = Y.frame_of_key(case)
    rows, mask = [], []
    for p, l in zip(P["slot_key"], P["lists"]):
        if expected["key_status"][p] in (1, 4):
            r = create([(fok[l], case["key_xyn"][l])])[0]
            rows.append("%d %s" % (r["status"], _d(r["point"]))); mask += [int(m) for m in r["mask"]]
        else:
            rows.append("255 %s" % _d(np.zeros(3))); mask += [0] * len(l)
    cap = Y.capacity(case, [f for f in frames if 0 <= f < len(case["registered"])]) if capacity is None else capacity
    return "\n".join(["case %s %d" % (float(c.get("extend_angle_rad", Y.EXTEND_ANGLE)).hex(), len(c["key_ptr"]) - 1), _j(c["key_ptr"]), _d(c["key_xyn"]), _j(c["registered"]),
                      _d(c["cam_q"]), _d(c["cam_t"]), _j(c["corr_ptr"]), _j(c["corr_key"]), str(len(frames)), _j(frames), "%d %d" % (len(c["points"]), cap), _d(c["points"]),
                      _j(c["track_outlier"]), _j(c["track_of_key"]), str(len(rows)), "\n".join(rows), str(len(mask)), _j(mask)]) + "\n"


def unit_input(th, dots):
    return "unit %s %d %s\n" % (float(th).hex(), len(dots), _d(dots))


def run(exe, text):
    """-> {name: [ints]} (ms_*: floats; fault: words)"""
    out = {}
    for ln in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines():
        w = ln.split()
        out[w[0]] = w[1:] if w[0] == "fault" else [float(x) for x in w[1:]] if w[0].startswith("ms") else [int(x) for x in w[1:]]
    return out
