"""A stand-alone host program around ba_stage.h (no HIP, no GPU): the block layout of a one-shot call, the view over its read-back
buffer, the trial-bound rows and the check of an offsets array.  tests/test_stage_cpu.py builds it with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrsfm_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ba_stage.h"
// Commands on stdin, one answer line each on stdout:
//   layout k, then k tokens: a byte count (one take), I (end_inputs), O (begin_outputs) or E (end_outputs)
//        -> the offset of every take, "|", in_bytes out0 out_bytes total, "|", and for every take between O and E the distance of
//           view.at(offset) from the start of a read-back buffer of out_bytes bytes (every such byte is written: in bounds)
//   rows k, then k values of n      -> the offset of every n, "|", the rows behind one another (fill_row writes 1000 n + i)
//   offsets32 | offsets64 name k, then k values      -> "ok", or the name and what is wrong with the array
using namespace xstage;
int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "layout")) {
            int k;
            if (std::scanf("%d", &k) != 1) return 1;
            Layout L;
            std::vector<size_t> offs, outs;
            bool in_out = false;
            for (int i = 0; i < k; ++i) {
                char tok[32];
                if (std::scanf("%31s", tok) != 1) return 1;
                if (!std::strcmp(tok, "I")) L.end_inputs();
                else if (!std::strcmp(tok, "O")) { L.begin_outputs(); in_out = true; }
                else if (!std::strcmp(tok, "E")) { L.end_outputs(); in_out = false; }
                else { offs.push_back(L.take((size_t)std::strtoull(tok, nullptr, 10))); if (in_out) outs.push_back(offs.back()); }
            }
            for (size_t o : offs) std::printf("%zu ", o);
            std::printf("| %zu %zu %zu %zu |", L.in_bytes, L.out0, L.out_bytes, L.total());
            std::vector<unsigned char> back(L.out_bytes);
            const View v{back.data(), L.out0};
            for (size_t o : outs) {
                unsigned char* p = const_cast<unsigned char*>(v.at<unsigned char>(o));
                *p = 1;
                std::printf(" %td", p - back.data());
            }
            std::printf("\n");
        } else if (!std::strcmp(cmd, "rows")) {
            int k;
            if (std::scanf("%d", &k) != 1) return 1;
            TrialRows R;
            for (int i = 0; i < k; ++i) {
                int n;
                if (std::scanf("%d", &n) != 1) return 1;
                std::printf("%d ", R.offset_for(n, [](int m, int32_t* row) { for (int j = 0; j <= m; ++j) row[j] = 1000 * m + j; }));
            }
            std::printf("|");
            for (int32_t x : R.rows) std::printf(" %d", x);
            std::printf("\n");
        } else if (!std::strcmp(cmd, "offsets32") || !std::strcmp(cmd, "offsets64")) {
            char name[32];
            int k;
            if (std::scanf("%31s %d", name, &k) != 2 || k < 1) return 1;
            std::vector<int64_t> v64((size_t)k);
            for (auto& x : v64) { long long y; if (std::scanf("%lld", &y) != 1) return 1; x = y; }
            std::vector<int32_t> v32(v64.begin(), v64.end());
            const char* fault = !std::strcmp(cmd, "offsets32") ? offsets_fault(v32.data(), k - 1) : offsets_fault(v64.data(), k - 1);
            if (fault) std::printf("%s %s\n", name, fault); else std::printf("ok\n");
        } else {
            return 1;
        }
    }
    return 0;
}
"""


def build(directory, name="stage_rule", text=DRIVER, flags=None):
    src, exe = os.path.join(str(directory), name + ".cc"), os.path.join(str(directory), name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["g++", "-std=c++17", *(SANITIZE if flags is None else flags), "-I", CSRC, src, "-o", exe], check=True)
    return exe


def run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def layout_input(tokens):
    """tokens: byte counts and the marks "I", "O", "E" in the order of the calls"""
    return "layout %d\n%s\n" % (len(tokens), " ".join(str(t) for t in tokens))


def parse_layout(line):
    """-> (offsets of every take, (in_bytes, out0, out_bytes, total), distances of the output arrays in the read-back buffer)"""
    offs, marks, rel = (part.split() for part in line.split("|"))
    return [int(x) for x in offs], tuple(int(x) for x in marks), [int(x) for x in rel]


def rows_input(ns):
    return "rows %d\n%s\n" % (len(ns), " ".join(map(str, ns)))


def parse_rows(line):
    offs, rows = (part.split() for part in line.split("|"))
    return [int(x) for x in offs], [int(x) for x in rows]


def offsets_input(name, values, wide=False):
    return "%s %s %d\n%s\n" % ("offsets64" if wide else "offsets32", name, len(values), " ".join(map(str, values)))
