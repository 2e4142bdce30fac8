"""A stand-alone host program around ba_sift_desc_rule.h (no HIP, no GPU): gradient, orientation, descriptor, normalisation and bytes
of given keypoints, sequentially and in the reference's loop order.  tests/test_desc_cpu.py builds it with the address and
undefined-behaviour sanitizers and feeds it the Gaussian levels and keypoints that the program of tests/sift_host_driver.py wrote;
tools/feature_extract_timing.py builds both with -O2 as the CPU column of its table."""
import os
import struct
import subprocess

import numpy as np

from tests import sift_host_driver as H
from tests import sift_yardstick as Y

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_sift_desc_rule.h"
// argv: input file, output file, ["time"].  Input: int32 mode, upright, n_oct; float key_sigma[3], step; per octave int32 w, h and
// three planes: mode 0 the Gaussian levels G[1..3] (w * h floats each), mode 1 the gradient planes themselves (w * h float2 each);
// int32 n_keys; per keypoint int32 loc[4] (octave, level, row, col) and float v[4]: mode 0 (sign, dx, dy, ds), mode 1 the
// octave-space key (x, y, sigma, w) whose w the descriptor is to use.  Output: per octave the three gradient planes; per keypoint
// float okey[4] (with the w the descriptor used), float w of the histogram, float vote[36], int32 dropped samples, float raw[128],
// unit[128], desc_float[128], uint8 desc[128].  With "time" only the time goes to stderr in milliseconds.
using namespace xsiftd;
int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const bool timing = argc > 3 && !std::strcmp(argv[3], "time");
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t hd[3];
    float prm[4];
    if (std::fread(hd, 4, 3, in) != 3 || std::fread(prm, 4, 4, in) != 4) return 1;
    const int mode = hd[0], upright = hd[1], n_oct = hd[2];
    std::vector<int32_t> W((size_t)n_oct), Hh((size_t)n_oct);
    std::vector<std::vector<float>> src((size_t)n_oct * 3), grad((size_t)n_oct * 3);
    for (int o = 0; o < n_oct; ++o) {
        if (std::fread(&W[(size_t)o], 4, 1, in) != 1 || std::fread(&Hh[(size_t)o], 4, 1, in) != 1) return 1;
        const size_t n = (size_t)W[(size_t)o] * Hh[(size_t)o];
        for (int j = 0; j < 3; ++j) {
            std::vector<float>& s = src[(size_t)o * 3 + j];
            s.resize(n * (mode ? 2 : 1));
            if (std::fread(s.data(), 4, s.size(), in) != s.size()) return 1;
        }
    }
    int32_t n_keys = 0;
    if (std::fread(&n_keys, 4, 1, in) != 1) return 1;
    struct K { int32_t loc[4]; float v[4]; };
    std::vector<K> keys((size_t)n_keys);
    if (n_keys && std::fread(keys.data(), sizeof(K), keys.size(), in) != keys.size()) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int o = 0; o < n_oct; ++o)
        for (int j = 0; j < 3; ++j) {
            const int w = W[(size_t)o], h = Hh[(size_t)o];
            std::vector<float>& g = grad[(size_t)o * 3 + j];
            const std::vector<float>& s = src[(size_t)o * 3 + j];
            if (mode) { g = s; continue; }
            g.assign((size_t)w * h * 2, 0.0f);
            for (int r = 1; r < h - 1; ++r)
                for (int c = 1; c < w - 1; ++c) {
                    const size_t at = (size_t)r * w + c;
                    gradient(s[at + 1], s[at - 1], s[at + w], s[at - w], &g[2 * at], &g[2 * at + 1]);
                }
        }
    struct Out { float okey[4], w_hist, vote[36]; int32_t dropped; float raw[128], unit[128], fl[128]; uint8_t desc[128]; };
    std::vector<Out> res((size_t)n_keys);
    for (int k = 0; k < n_keys; ++k) {
        const K& q = keys[(size_t)k];
        Out& r = res[(size_t)k];
        const int o = q.loc[0], j = q.loc[1], w = W[(size_t)o], h = Hh[(size_t)o];
        const float* g = grad[(size_t)o * 3 + j].data();
        auto got = [&](int x, int y, float* grd, float* rot) { const size_t at = (size_t)y * w + x; *grd = g[2 * at]; *rot = g[2 * at + 1]; };
        if (mode) { r.okey[0] = q.v[0]; r.okey[1] = q.v[1]; r.okey[2] = q.v[2]; }
        else octave_key(q.loc[2], q.loc[3], q.v[1], q.v[2], q.v[3], prm[j], prm[3], &r.okey[0], &r.okey[1], &r.okey[2]);
        r.w_hist = orientation(got, w, h, r.okey[0], r.okey[1], r.okey[2], r.vote);
        r.okey[3] = mode ? q.v[3] : (upright ? 0.0f : r.w_hist);
        const DescFrame f = desc_frame(r.okey[2], r.okey[3]);
        r.dropped = 0;
        for (int cell = 0; cell < kCells; ++cell) descriptor_cell(got, w, h, r.okey[0], r.okey[1], f, cell & 3, cell >> 2, r.raw + 8 * cell, &r.dropped);
        normalize(r.raw, r.unit);
        l1_root_and_bytes(r.unit, r.fl, r.desc);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (timing) std::fprintf(stderr, "ms %.3f\n", ms);
    else {
        for (const std::vector<float>& g : grad) std::fwrite(g.data(), 4, g.size(), out);
        for (const Out& r : res) {
            std::fwrite(r.okey, 4, 4, out); std::fwrite(&r.w_hist, 4, 1, out); std::fwrite(r.vote, 4, 36, out); std::fwrite(&r.dropped, 4, 1, out);
            std::fwrite(r.raw, 4, 128, out); std::fwrite(r.unit, 4, 128, out); std::fwrite(r.fl, 4, 128, out); std::fwrite(r.desc, 1, 128, out);
        }
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
"""

REC = np.dtype([("okeys", np.float32, 4), ("w_hist", np.float32), ("vote", np.float32, 36), ("dropped", np.int32), ("raw", np.float32, 128),
                ("unit", np.float32, 128), ("desc_float", np.float32, 128), ("desc", np.uint8, 128)])


def build(directory, flags=None):
    return H.build(directory, name="desc_images", text=DRIVER, flags=flags)


def run(exe, directory, planes, loc, values, first_octave=-1, mode=0, upright=0, timing=False):
    """planes: per octave [3][h][w] (mode 0: G[1..3]) or [3][h][w][2] (mode 1); loc [n][4]; values [n][4] (see DRIVER).
    -> dict(planes per octave [3][h][w][2], and the fields of REC); with timing: milliseconds"""
    inp, outp = os.path.join(str(directory), "desc_in.bin"), os.path.join(str(directory), "desc_out.bin")
    P = Y.params(first_octave)
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i", mode, upright, len(planes)))
        f.write(np.array([*P["key_sigma"], P["step"]], np.float32).tobytes())
        for p in planes:
            p = np.ascontiguousarray(p, np.float32)
            f.write(struct.pack("<2i", p.shape[2], p.shape[1]))
            f.write(p.tobytes())
        f.write(struct.pack("<i", len(loc)))
        rec = np.zeros(len(loc), np.dtype([("loc", np.int32, 4), ("v", np.float32, 4)]))
        if len(loc):
            rec["loc"], rec["v"] = loc, values
        f.write(rec.tobytes())
    r = subprocess.run([exe, inp, outp] + (["time"] if timing else []), capture_output=True, text=True, check=True)
    if timing:
        return float(r.stderr.split("ms")[1])
    buf, at, out = open(outp, "rb").read(), 0, dict(planes=[])
    for p in planes:
        n = 3 * p.shape[1] * p.shape[2] * 2
        out["planes"].append(np.frombuffer(buf, np.float32, n, at).reshape(3, p.shape[1], p.shape[2], 2).copy())
        at += 4 * n
    rec = np.frombuffer(buf, REC, len(loc), at)
    assert at + rec.nbytes == len(buf)
    out.update({k: rec[k].copy() for k in REC.names})
    out["loc"] = np.asarray(loc, np.int32).reshape(-1, 4)
    return out


def run_image(sift_exe, desc_exe, directory, image, opt, upright=0):
    """both programs on one image: the result of run() on the levels and keypoints that the first program found"""
    s = H.run(sift_exe, directory, [image], [opt])[0]
    planes = [G[1:4] for G, _ in s["levels"]]
    return run(desc_exe, directory, planes, s["loc"], s["off"], opt["first_octave"], 0, upright), s
