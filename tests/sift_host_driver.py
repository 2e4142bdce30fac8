"""Two stand-alone host programs around ba_sift_rule.h (no HIP, no GPU): a sequential driver of whole images, and one that puts single
queries to xsift::geometry and xsift::key_decide.  tests/test_sift_cpu.py builds them with the address and undefined-behaviour sanitizers; tools/keypoint_timing.py builds it with -O2 as the CPU column of its
table."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ba_sift_rule.h"
// argv: input file, output file, ["time"].  Input: int32 n_images, then per image int32 width, height, first_octave, num_octaves,
// max_num_features, float peak_threshold, edge_threshold, and width * height bytes.  Output per image: int32 n_oct; the parameters
// (float sigma0, step, level_sigma[5], init_sigma, key_sigma[3], T, T0, E); per octave int32 w, h and the planes G[6], D[5]; int32
// level_count[n_oct * 3]; int32 n_keys; per keypoint int32 loc[4], float sign, dx, dy, ds, X, Y, S.  With "time" the planes are not
// written and the total time of the images goes to stderr in milliseconds.
using namespace xsift;
struct ByteSrc { const uint8_t* p; int w, stride; float operator()(int i) const { return pixel_value(p[(size_t)(i / w) * stride + (i % w)]); } };
static void filter(const std::vector<float>& src, std::vector<float>& dst, std::vector<float>& tmp, int w, int h, const Taps& t) {
    const int sz = t.width >> 1;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            float value = 0;
            for (int i = 0; i < t.width; ++i) value += src[(size_t)r * w + clampi(c - sz + i, 0, w - 1)] * t.w[i];
            tmp[(size_t)r * w + c] = value;
        }
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            float value = 0;
            for (int i = 0; i < t.width; ++i) value += tmp[(size_t)clampi(r - sz + i, 0, h - 1) * w + c] * t.w[i];
            dst[(size_t)r * w + c] = value;
        }
}
int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const bool timing = argc > 3 && !std::strcmp(argv[3], "time");
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t n_images = 0;
    if (std::fread(&n_images, 4, 1, in) != 1) return 1;
    double total_ms = 0.0;
    for (int im = 0; im < n_images; ++im) {
        int32_t hd[5];
        float th[2];
        if (std::fread(hd, 4, 5, in) != 5 || std::fread(th, 4, 2, in) != 2) return 1;
        const int W = hd[0], H = hd[1], fo = hd[2];
        std::vector<uint8_t> pix((size_t)W * H);
        if (std::fread(pix.data(), 1, pix.size(), in) != pix.size()) return 1;
        const auto t0 = std::chrono::steady_clock::now();
        const Params P = make_params(fo, th[0], th[1]);
        const Geometry g = geometry(W, H, fo, hd[3]);
        std::vector<std::vector<float>> G((size_t)g.n_oct * kGauss), D((size_t)g.n_oct * kDog);
        std::vector<float> tmp, base((size_t)g.w[0] * g.h[0]);
        const ByteSrc src{pix.data(), g.w_in, W};
        for (int r = 0; r < g.h[0]; ++r)
            for (int c = 0; c < g.w[0]; ++c)
                base[(size_t)r * g.w[0] + c] = fo < 0 ? upsample_at(src, g.w_in, g.h_in, r, c) : pixel_value(pix[(size_t)r * W + c]);
        Taps t;
        for (int o = 0; o < g.n_oct; ++o) {
            const int w = g.w[o], h = g.h[o];
            const size_t n = (size_t)w * h;
            tmp.assign(n, 0.0f);
            std::vector<float>* L = &G[(size_t)o * kGauss];
            for (int i = 0; i < kGauss; ++i) L[i].assign(n, 0.0f);
            if (o == 0) {
                if (P.init_sigma > 0.0f) { build_taps(P.init_sigma, &t); filter(base, L[0], tmp, w, h, t); }
                else L[0] = base;
            } else {
                const std::vector<float>& s = G[(size_t)(o - 1) * kGauss + kDownLevel];
                for (int r = 0; r < h; ++r)
                    for (int c = 0; c < w; ++c) L[0][(size_t)r * w + c] = s[(size_t)down_src_row(r) * g.w[o - 1] + down_src_col(c, g.w[o - 1])];
            }
            for (int i = 0; i < kDog; ++i) {
                build_taps(P.level_sigma[i], &t);
                filter(L[i], L[i + 1], tmp, w, h, t);
                std::vector<float>& d = D[(size_t)o * kDog + i];
                d.resize(n);
                for (size_t k = 0; k < n; ++k) d[k] = L[i + 1][k] - L[i][k];
            }
        }
        struct K { int32_t loc[4]; float v[7]; };
        std::vector<std::vector<K>> keys((size_t)g.n_oct * kKeyLevels);
        std::vector<int32_t> level_count((size_t)g.n_oct * kKeyLevels, 0);
        for (int o = 0; o < g.n_oct; ++o)
            for (int j = 0; j < kKeyLevels; ++j) {
                const int w = g.w[o], h = g.h[o];
                const float *p = D[(size_t)o * kDog + j].data(), *c = D[(size_t)o * kDog + j + 1].data(), *n = D[(size_t)o * kDog + j + 2].data();
                for (int row = 1; row < h - 1; ++row)
                    for (int col = 1; col < w - 1; ++col) {
                        const size_t a = (size_t)(row - 1) * w + col, b = a + w, d = b + w;
                        const Key k = key_decide(p[a - 1], p[a], p[a + 1], p[b - 1], p[b], p[b + 1], p[d - 1], p[d], p[d + 1],
                                                 c[a - 1], c[a], c[a + 1], c[b - 1], c[b], c[b + 1], c[d - 1], c[d], c[d + 1],
                                                 n[a - 1], n[a], n[a + 1], n[b - 1], n[b], n[b + 1], n[d - 1], n[d], n[d + 1], P.T0, P.T, P.E);
                        if (k.sign == 0.0f) continue;
                        K x{{o, j, row, col}, {k.sign, k.dx, k.dy, k.ds, 0, 0, 0}};
                        key_values(row, col, k.dx, k.dy, k.ds, P.key_sigma[j], P.step, octave_scale(fo, o), &x.v[4], &x.v[5], &x.v[6]);
                        keys[(size_t)o * kKeyLevels + j].push_back(x);
                    }
                level_count[(size_t)o * kKeyLevels + j] = (int32_t)keys[(size_t)o * kKeyLevels + j].size();
            }
        uint8_t take[kMaxOctaves * kKeyLevels] = {};
        const int32_t n_keys = (int32_t)budget(level_count.data(), g.n_oct, hd[4], take);
        total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fwrite(&g.n_oct, 4, 1, out);
        std::fwrite(&P, sizeof(float), 14, out);
        for (int o = 0; o < g.n_oct; ++o) {
            std::fwrite(&g.w[o], 4, 1, out); std::fwrite(&g.h[o], 4, 1, out);
            if (timing) continue;
            for (int i = 0; i < kGauss; ++i) std::fwrite(G[(size_t)o * kGauss + i].data(), 4, (size_t)g.w[o] * g.h[o], out);
            for (int i = 0; i < kDog; ++i) std::fwrite(D[(size_t)o * kDog + i].data(), 4, (size_t)g.w[o] * g.h[o], out);
        }
        std::fwrite(level_count.data(), 4, level_count.size(), out);
        std::fwrite(&n_keys, 4, 1, out);
        for (size_t l = 0; l < keys.size(); ++l)
            if (take[l]) for (const K& x : keys[l]) { std::fwrite(x.loc, 4, 4, out); std::fwrite(x.v, 4, 7, out); }
    }
    std::fclose(in); std::fclose(out);
    if (timing) std::fprintf(stderr, "ms %.3f\n", total_ms);
    return 0;
}
"""


RULE_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_sift_rule.h"
// argv: input file, output file.  Input: int32 n_geo, then n_geo x (int32 width, height, first_octave, num_octaves); int32 n_dec, then
// n_dec x 30 floats: the neighbourhoods [row][col] of the previous, the own and the next DoG level, then T0, T, E.  Output: per
// geometry int32 w_in, h_in, n_oct, w[8], h[8] (xsift::geometry); per decision float sign, dx, dy, ds and int32 why (xsift::key_decide).
using namespace xsift;
int main(int argc, char** argv) {
    if (argc < 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1) return 1;
    for (int i = 0; i < n; ++i) {
        int32_t q[4];
        if (std::fread(q, 4, 4, in) != 4) return 1;
        const Geometry g = geometry(q[0], q[1], q[2], q[3]);
        std::fwrite(&g.w_in, 4, 1, out); std::fwrite(&g.h_in, 4, 1, out); std::fwrite(&g.n_oct, 4, 1, out);
        std::fwrite(g.w, 4, kMaxOctaves, out); std::fwrite(g.h, 4, kMaxOctaves, out);
    }
    if (std::fread(&n, 4, 1, in) != 1) return 1;
    for (int i = 0; i < n; ++i) {
        float v[30];
        if (std::fread(v, 4, 30, in) != 30) return 1;
        const Key k = key_decide(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15], v[16], v[17],
                                 v[18], v[19], v[20], v[21], v[22], v[23], v[24], v[25], v[26], v[27], v[28], v[29]);
        std::fwrite(&k.sign, 4, 4, out);
        std::fwrite(&k.why, 4, 1, out);
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
"""


def run_rule(exe, directory, geo_queries, Pn, Cn, Nn, thresholds):
    """geo_queries: (width, height, first_octave, num_octaves); Pn, Cn, Nn [n][3][3] float32; thresholds [n][3] (T0, T, E).
    -> ([(w_in, h_in, [(w, h)] per octave)], dict(sign, dx, dy, ds, why))"""
    inp, outp = os.path.join(str(directory), "rule_in.bin"), os.path.join(str(directory), "rule_out.bin")
    n = len(Cn)
    rec = np.concatenate([np.asarray(x, np.float32).reshape(n, 9) for x in (Pn, Cn, Nn)] + [np.asarray(thresholds, np.float32).reshape(n, 3)], 1)
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(geo_queries)))
        f.write(np.asarray(geo_queries, np.int32).reshape(-1, 4).tobytes())
        f.write(struct.pack("<i", n))
        f.write(np.ascontiguousarray(rec).tobytes())
    subprocess.run([exe, inp, outp], check=True)
    buf = open(outp, "rb").read()
    g = np.frombuffer(buf, np.int32, 19 * len(geo_queries)).reshape(-1, 19)
    geo = [(int(r[0]), int(r[1]), [(int(r[3 + o]), int(r[11 + o])) for o in range(int(r[2]))]) for r in g]
    d = np.frombuffer(buf, np.dtype([("v", np.float32, 4), ("why", np.int32)]), n, g.nbytes)
    assert g.nbytes + d.nbytes == len(buf)
    return geo, dict(sign=d["v"][:, 0].copy(), dx=d["v"][:, 1].copy(), dy=d["v"][:, 2].copy(), ds=d["v"][:, 3].copy(), why=d["why"].copy())


def build(directory, name="sift_images", text=DRIVER, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def write_input(path, images, opts):
    """images: 2-D uint8 arrays; opts: per image a dict with the fields of xrsfm_ba_sift_options"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(images)))
        for a, o in zip(images, opts):
            a = np.ascontiguousarray(a, np.uint8)
            f.write(struct.pack("<5i2f", a.shape[1], a.shape[0], o["first_octave"], o["num_octaves"], o["max_num_features"], o["peak_threshold"], o["edge_threshold"]))
            f.write(a.tobytes())


def run(exe, directory, images, opts, timing=False):
    """-> per image dict(params [14], levels [(G, D)], level_count, loc, off (sign, dx, dy, ds), keys (X, Y, S)); with timing
    (levels empty, milliseconds)"""
    inp, outp = os.path.join(str(directory), "sift_in.bin"), os.path.join(str(directory), "sift_out.bin")
    write_input(inp, images, opts)
    r = subprocess.run([exe, inp, outp] + (["time"] if timing else []), capture_output=True, text=True, check=True)
    buf, at, res = open(outp, "rb").read(), 0, []

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(buf, dtype, n, at)
        at += a.nbytes
        return a
    for _ in images:
        n_oct = int(take(np.int32, 1)[0])
        d = dict(params=take(np.float32, 14).copy(), levels=[])
        for _o in range(n_oct):
            w, h = (int(x) for x in take(np.int32, 2))
            d.setdefault("geometry", []).append((w, h))
            if not timing:
                d["levels"].append((take(np.float32, 6 * h * w).reshape(6, h, w).copy(), take(np.float32, 5 * h * w).reshape(5, h, w).copy()))
        d["level_count"] = take(np.int32, n_oct * 3).copy()
        n = int(take(np.int32, 1)[0])
        rec = take(np.dtype([("loc", np.int32, 4), ("v", np.float32, 7)]), n)
        d["loc"], d["off"], d["keys"] = rec["loc"].copy(), rec["v"][:, :4].copy(), rec["v"][:, 4:].copy()
        res.append(d)
    assert at == len(buf)
    if timing:
        return res, float(r.stderr.split("ms")[1])
    return res
