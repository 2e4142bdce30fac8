// The gfx950 kernels of xrsfm_ba_extract_features after the keypoint list exists: gradient planes, orientation and descriptor (the
// rule: ba_sift_desc_rule.h).  The kernels of ba_sift.h run first and are not changed.
//
//   k_siftd_grad    over the 64 x 32 tile work list of an octave, lane = column, grid (tiles, 3 levels): the (grd, rot) plane of
//                   G[j + 1] for every (image, level) that keeps a keypoint after the budget (need); atan2 runs once per pixel and
//                   both consumers read that value.  Border pixels are written as (0, 0); no window reads them.
//   k_siftd_record  one block per (image, level) with keypoints: the octave-space key (x, y, sigma) of each keypoint and the plane,
//                   stored width and height it is to be read with go into a 32-byte record, so that the two kernels below run over
//                   the keypoints of the whole chunk, all images, octaves and levels, in one launch each.
//   k_siftd_orient  16 lanes per keypoint, 16 keypoints per block.  The lanes split the window by flat index.  Every lane owns 36
//                   partial bins in LDS, bin b of thread t at [b][t]: a lane's bins sit in its own bank (256 threads, 64 banks) and
//                   nothing is an indexed private array.  The 16 partials of a bin are summed in a fixed (rotated, so bank-conflict
//                   free) order; the six smoothing passes alternate between two LDS copies; lane 0 takes the arg-max.
//   k_siftd_desc    one wave per keypoint, four lanes per cell, lane s of a cell takes rows ymin + s, + 4, ...  des[0..8] stay in
//                   registers through the reference's static select; the four lanes are summed as ((0 + 1) + 2) + 3; the norms are
//                   summed over the wave in cell order.  The normalisations, the L1 root and the byte conversion follow on the 128
//                   values the wave holds; a wave writes its 128 bytes (and the optional 512-byte float rows) contiguously.
//                   The gradient planes are read through L2, not staged in LDS (a cell's box is rotated and of data-dependent
//                   size); the staged alternative was not measured.
// No floating-point atomics anywhere: no result depends on arrival order.
#pragma once

#include <hip/hip_runtime.h>

#include "ba_sift.h"
#include "ba_sift_desc_rule.h"

constexpr int kSiftdGradPlanes = xsift::kKeyLevels;                  // of an octave: (grd, rot) of G[1..3], each w * h float2
constexpr int kSiftdGroup = 16, kSiftdOrientKeys = kSiftThreads / kSiftdGroup;
constexpr int kSiftdDescKeys = kSiftThreads / 64;

struct SiftdImg { int64_t grad[xsift::kMaxOctaves]; };               // first float2 of the octave's gradient planes
struct SiftdLevel { int64_t first, plane; int32_t count, w, h, pad; float sigma, step; };
struct SiftdRec { int64_t plane; int32_t w, h; float x, y, s, a; };  // a: the orientation w of the reference's key

__global__ __launch_bounds__(kSiftThreads) void k_siftd_grad(const SiftImg* __restrict__ imgs, const SiftdImg* __restrict__ dimgs, const SiftTile* __restrict__ tiles,
                                                             const float* __restrict__ planes, float2* __restrict__ grad, const int32_t* __restrict__ need, int oct, int nl) {
    const int j = (int)blockIdx.y;
    const SiftTile tl = tiles[blockIdx.x];
    if (!need[(int64_t)tl.img * nl + oct * xsift::kKeyLevels + j]) return;
    const SiftImg& im = imgs[tl.img];
    const int w = im.w[oct], h = im.h[oct], col = tl.tx * kSiftTW + (int)(threadIdx.x & 63);
    if (col >= w) return;
    const int64_t n = (int64_t)w * h;
    const float* G = planes + im.plane[oct] + (j + 1) * n;
    float2* dst = grad + dimgs[tl.img].grad[oct] + j * n;
    for (int r = (int)(threadIdx.x >> 6); r < kSiftTH; r += kSiftWaves) {
        const int row = tl.ty * kSiftTH + r;
        if (row >= h) break;
        const int64_t at = (int64_t)row * w + col;
        float2 v = make_float2(0.0f, 0.0f);
        if (row > 0 && col > 0 && row < h - 1 && col < w - 1) xsiftd::gradient(G[at + 1], G[at - 1], G[at + w], G[at - w], &v.x, &v.y);
        dst[at] = v;
    }
}

__global__ __launch_bounds__(kSiftThreads) void k_siftd_record(const SiftdLevel* __restrict__ levels, const int4* __restrict__ loc, const float4* __restrict__ off,
                                                               SiftdRec* __restrict__ rec) {
    const SiftdLevel L = levels[blockIdx.x];
    for (int k = (int)threadIdx.x; k < L.count; k += kSiftThreads) {
        const int64_t at = L.first + k;
        const int4 l = loc[at];
        const float4 o = off[at];
        SiftdRec r{L.plane, L.w, L.h, 0.0f, 0.0f, 0.0f, 0.0f};
        xsiftd::octave_key(l.z, l.w, o.y, o.z, o.w, L.sigma, L.step, &r.x, &r.y, &r.s);
        rec[at] = r;
    }
}

__global__ __launch_bounds__(kSiftThreads) void k_siftd_orient(SiftdRec* __restrict__ rec, int64_t n_keys, const float2* __restrict__ grad) {
    __shared__ float s_h[xsiftd::kBins * kSiftThreads];
    __shared__ float s_v[2][kSiftdOrientKeys][xsiftd::kBins + 1];
    const int tid = (int)threadIdx.x, g = tid / kSiftdGroup, l = tid % kSiftdGroup;
    const int64_t k = (int64_t)blockIdx.x * kSiftdOrientKeys + g;
    const bool valid = k < n_keys;
    for (int b = 0; b < xsiftd::kBins; ++b) s_h[b * kSiftThreads + tid] = 0.0f;
    if (valid) {
        const SiftdRec R = rec[k];
        const xsiftd::OrientFrame f = xsiftd::orient_frame(R.x, R.y, R.s, R.w, R.h);
        const int nxw = max(0, (int)(f.win.xmax - f.win.xmin) + 1), nyw = max(0, (int)(f.win.ymax - f.win.ymin) + 1);
        const float2* P = grad + R.plane;
        for (int i = l; i < nxw * nyw; i += kSiftdGroup) {
            const int yi = i / nxw, xi = i - yi * nxw;
            const float x = f.win.xmin + (float)xi, y = f.win.ymin + (float)yi;
            float sq;
            if (!xsiftd::orient_inside(f, R.x, R.y, x, y, &sq)) continue;
            const float2 v = P[(int64_t)(int)y * R.w + (int)x];          // (1.5 .. w - 1.5, 1.5 .. h - 1.5: inside the plane)
            const int bin = min(max(xsiftd::orient_bin(v.y), 0), xsiftd::kBins - 1);          // (rot lies in -pi .. pi: the clamp never acts)
            s_h[bin * kSiftThreads + tid] += xsiftd::orient_weight(f, sq, v.x);
        }
    }
    __syncthreads();
    for (int b = l; b < xsiftd::kBins; b += kSiftdGroup) {
        float v = 0.0f;
        for (int t = 0; t < kSiftdGroup; ++t) v += s_h[b * kSiftThreads + g * kSiftdGroup + ((l + t) & (kSiftdGroup - 1))];
        s_v[0][g][b] = v;
    }
    for (int p = 0; p < xsiftd::kSmoothPasses; ++p) {
        __syncthreads();
        const float* src = s_v[p & 1][g];
        float* dst = s_v[(p + 1) & 1][g];
        for (int b = l; b < xsiftd::kBins; b += kSiftdGroup)
            dst[b] = xsiftd::orient_smooth(src[b == 0 ? xsiftd::kBins - 1 : b - 1], src[b], src[b == xsiftd::kBins - 1 ? 0 : b + 1]);
    }
    __syncthreads();
    if (valid && l == 0) {
        const float* vote = s_v[xsiftd::kSmoothPasses & 1][g];
        int index_max = 0;
        float max_vote = vote[0];
        for (int i = 1; i < xsiftd::kBins; ++i) {
            const float v = vote[i];
            index_max = v > max_vote ? i : index_max;
            max_vote = fmaxf(max_vote, v);
        }
        rec[k].a = xsiftd::orient_angle(index_max, vote[index_max == 0 ? xsiftd::kBins - 1 : index_max - 1], max_vote,
                                        vote[index_max == xsiftd::kBins - 1 ? 0 : index_max + 1]);
    }
}

// raw, unit, desc_float: may be null
__global__ __launch_bounds__(kSiftThreads) void k_siftd_desc(const SiftdRec* __restrict__ rec, int64_t n_keys, const float2* __restrict__ grad, int upright,
                                                             float4* __restrict__ okeys, uint8_t* __restrict__ desc, float* __restrict__ desc_float,
                                                             float* __restrict__ raw, float* __restrict__ unit) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t k = (int64_t)blockIdx.x * kSiftdDescKeys + (int)(threadIdx.x >> 6);
    if (k >= n_keys) return;
    const SiftdRec R = rec[k];
    const float kw = upright ? 0.0f : R.a;
    const int cell = lane >> 2, sub = lane & 3;
    const xsiftd::DescFrame f = xsiftd::desc_frame(R.s, kw);
    const xsiftd::DescCell c = xsiftd::desc_cell(f, R.x, R.y, cell & 3, cell >> 2, R.w, R.h);
    const float2* P = grad + R.plane;
    float des[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) des[i] = 0.0f;
    for (float y = c.win.ymin + (float)sub; y <= c.win.ymax; y += 4.0f)
        for (float x = c.win.xmin; x <= c.win.xmax; x += 1.0f) {
            float nx, ny;
            if (!xsiftd::desc_inside(f, c, x, y, &nx, &ny)) continue;
            const float2 v = P[(int64_t)(int)y * R.w + (int)x];          // (clamped to 1.5 .. w - 1.5, 1.5 .. h - 1.5: inside the plane)
            float weight, theta;
            xsiftd::desc_sample(f, c, nx, ny, v.x, v.y, &weight, &theta);
            XSIFTD_ACCUMULATE(des, weight, theta);
        }
    const int base = lane & ~3;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float a0 = __shfl(des[i], base), a1 = __shfl(des[i], base + 1), a2 = __shfl(des[i], base + 2), a3 = __shfl(des[i], base + 3);
        des[i] = ((a0 + a1) + a2) + a3;
    }
    des[0] += des[8];
    // every lane of a cell now holds the cell's eight sums; lane s hands out bins 2 s and 2 s + 1
#define XSIFTD_MINE(v0, v1)                                                                  \
    v0 = sub == 0 ? des[0] : (sub == 1 ? des[2] : (sub == 2 ? des[4] : des[6]));             \
    v1 = sub == 0 ? des[1] : (sub == 1 ? des[3] : (sub == 2 ? des[5] : des[7]))
    auto over_cells = [](float q0, float q1) {          // the sum over the wave in the order of the 32 float4 of a row
        float s = 0.0f;
#pragma unroll
        for (int cc = 0; cc < xsiftd::kCells; ++cc) { s += __shfl(q0, 4 * cc); s += __shfl(q1, 4 * cc); }
        return s;
    };
    const int64_t at = k * xsiftd::kDesc + cell * 8 + 2 * sub;
    float v0, v1;
    if (raw) { XSIFTD_MINE(v0, v1); *(float2*)(raw + at) = make_float2(v0, v1); }
    const float norm1 = xsiftd::rsqrt_of(over_cells(xsiftd::sumsq4(des[0], des[1], des[2], des[3]), xsiftd::sumsq4(des[4], des[5], des[6], des[7])));
#pragma unroll
    for (int i = 0; i < 8; ++i) des[i] = xsiftd::clamp_unit(des[i], norm1);
    const float norm2 = xsiftd::rsqrt_of(over_cells(xsiftd::sumsq4(des[0], des[1], des[2], des[3]), xsiftd::sumsq4(des[4], des[5], des[6], des[7])));
#pragma unroll
    for (int i = 0; i < 8; ++i) des[i] *= norm2;
    if (unit) { XSIFTD_MINE(v0, v1); *(float2*)(unit + at) = make_float2(v0, v1); }
    const float l1 = over_cells(xsiftd::abs_sum4(des[0], des[1], des[2], des[3]), xsiftd::abs_sum4(des[4], des[5], des[6], des[7]));
    XSIFTD_MINE(v0, v1);
    v0 = xsiftd::l1_root(v0, l1); v1 = xsiftd::l1_root(v1, l1);
    if (desc_float) *(float2*)(desc_float + at) = make_float2(v0, v1);
#undef XSIFTD_MINE
    ((uint16_t*)desc)[k * 64 + lane] = (uint16_t)((uint16_t)xsiftd::to_byte(v0) | ((uint16_t)xsiftd::to_byte(v1) << 8));
    if (lane == 0) okeys[k] = make_float4(R.x, R.y, R.s, kw);
}
