// The gfx950 kernels of xrsfm_ba_detect_keypoints: scale space, difference of Gaussians and keypoint detection of a batch of
// 8-bit images (the rule: ba_sift_rule.h).  These are FP32 streaming kernels; the work is bandwidth.
//
// Every kernel runs over a WORK LIST of tiles (image, tile column, tile row) of one octave, so all images of a call that own the
// octave, whatever their sizes, go through the same launch.  A tile is 64 x 32 pixels and a block 256 threads (4 waves): lane =
// column, so that every global and LDS access of a wave is 64 consecutive floats, and wave k takes rows k, k + 4, ...
//
//   k_sift_base    the first octave's unsmoothed plane: bytes / 255, up-sampled x2 for first_octave -1
//   k_sift_filter  one separable Gaussian: the source tile with a halo of half the filter goes to LDS (at most 64 x 96 floats), the
//                  horizontal pass writes its result to a second LDS tile (64 x 64 floats) and the vertical pass reads it from
//                  there: the horizontal result never goes to HBM.  The DoG plane D[i] = G[i+1] - G[i] is formed here, where
//                  G[i+1] is produced, from the centre of the source tile already in LDS: 4 bytes read, 8 written per pixel.
//   k_sift_down    G[0] of octave o from G[3] of octave o - 1
//   k_sift_key     three DoG levels with a one-pixel halo in LDS (3 x 34 x 66 floats); COUNT: the keypoints of the tile and level
//                  go to tile_count; EMIT: with the tile's first slot from the host (budget and prefix sum between the two
//                  passes; a negative slot: the level was cut), the keypoints are written and their number is reported again.  Within a tile the slots are given out
//                  by an LDS counter in no fixed order; the host puts each level into row-major order when it hands it out.
//
// LDS: filter 40 KiB (by LDS alone 160 / 40 = 4 blocks = 16 waves per CU; the occupancy reached was not measured), key 26.3 KiB.  Only what the descriptor stage will need is
// kept per octave: the six Gaussian levels, next to the five DoG levels the key test reads; no gradient planes.
#pragma once

#include <hip/hip_runtime.h>

#include "ba_sift_rule.h"

constexpr int kSiftTW = 64, kSiftTH = 32, kSiftThreads = 256, kSiftWaves = 4;
constexpr int kSiftHalo = xsift::kMaxTaps >> 1;                     // 16
constexpr int kSiftSrcW = kSiftTW + 2 * kSiftHalo, kSiftSrcH = kSiftTH + 2 * kSiftHalo;
constexpr int kSiftPlanes = xsift::kGauss + xsift::kDog;            // of an octave: G[0..5], D[0..4], each w * h floats
constexpr int kSiftScratchPlane = xsift::kGauss;                    // the unsmoothed first octave lives in D[0] until G[1] is made

struct SiftImg {
    int64_t pix_off;                          // first byte of the image in the chunk's pixels
    int64_t plane[xsift::kMaxOctaves];        // first float of the octave's planes
    int32_t stride, w_in, h_in, n_oct;        // row stride of the input; the part that is read
    int32_t w[xsift::kMaxOctaves], h[xsift::kMaxOctaves];
};
struct SiftTile { int32_t img, tx, ty, pad; };
struct SiftKeyParams { float T0, T, E, step, os, key_sigma0, key_sigma1, key_sigma2; };

struct SiftByteSrc {
    const uint8_t* p; int w, stride;
    __device__ float operator()(int i) const { return xsift::pixel_value(p[(int64_t)(i / w) * stride + (i % w)]); }
};

__global__ __launch_bounds__(kSiftThreads) void k_sift_base(const SiftImg* __restrict__ imgs, const SiftTile* __restrict__ tiles,
                                                            const uint8_t* __restrict__ pixels, float* __restrict__ planes, int first_octave, int dst_idx) {
    const SiftTile tl = tiles[blockIdx.x];
    const SiftImg& im = imgs[tl.img];
    const int w = im.w[0], h = im.h[0], c = (int)(threadIdx.x & 63), col = tl.tx * kSiftTW + c;
    if (col >= w) return;
    float* dst = planes + im.plane[0] + (int64_t)dst_idx * w * h;
    const uint8_t* pix = pixels + im.pix_off;
    const SiftByteSrc src{pix, im.w_in, im.stride};
    for (int r = (int)(threadIdx.x >> 6); r < kSiftTH; r += kSiftWaves) {
        const int row = tl.ty * kSiftTH + r;
        if (row >= h) break;
        dst[(int64_t)row * w + col] = first_octave < 0 ? xsift::upsample_at(src, im.w_in, im.h_in, row, col)
                                                       : xsift::pixel_value(pix[(int64_t)row * im.stride + col]);
    }
}

__global__ __launch_bounds__(kSiftThreads) void k_sift_filter(const SiftImg* __restrict__ imgs, const SiftTile* __restrict__ tiles, float* __restrict__ planes,
                                                              int oct, int src_idx, int dst_idx, int dog_idx, const float* __restrict__ taps, int width) {
    __shared__ float s_src[kSiftSrcH][kSiftSrcW];
    __shared__ float s_h[kSiftSrcH][kSiftTW];
    const SiftTile tl = tiles[blockIdx.x];
    const SiftImg& im = imgs[tl.img];
    const int w = im.w[oct], h = im.h[oct], sz = width >> 1, r0 = tl.ty * kSiftTH, c0 = tl.tx * kSiftTW;
    const int64_t n = (int64_t)w * h;
    float* base = planes + im.plane[oct];
    const float* src = base + src_idx * n;
    const int c = (int)(threadIdx.x & 63), rg = (int)(threadIdx.x >> 6), nrow = kSiftTH + 2 * sz, ncol = kSiftTW + 2 * sz;
    for (int rr = rg; rr < nrow; rr += kSiftWaves) {
        const int64_t row = xsift::clampi(r0 - sz + rr, 0, h - 1);
        for (int cc = c; cc < ncol; cc += 64) s_src[rr][cc] = src[row * w + xsift::clampi(c0 - sz + cc, 0, w - 1)];
    }
    __syncthreads();
    for (int rr = rg; rr < nrow; rr += kSiftWaves) {                 // FilterH: value += data * tap from tap 0 upward
        float value = 0.0f;
        for (int i = 0; i < width; ++i) value += s_src[rr][c + i] * taps[i];
        s_h[rr][c] = value;
    }
    __syncthreads();
    const int col = c0 + c;
    if (col >= w) return;
    for (int r = rg; r < kSiftTH; r += kSiftWaves) {                 // FilterV
        const int row = r0 + r;
        if (row >= h) break;
        float value = 0.0f;
        for (int i = 0; i < width; ++i) value += s_h[r + i][c] * taps[i];
        const int64_t at = (int64_t)row * w + col;
        base[dst_idx * n + at] = value;
        if (dog_idx >= 0) base[dog_idx * n + at] = value - s_src[r + sz][c + sz];          // ComputeDOG_Kernel: v - vp
    }
}

__global__ __launch_bounds__(kSiftThreads) void k_sift_down(const SiftImg* __restrict__ imgs, const SiftTile* __restrict__ tiles, float* __restrict__ planes, int oct) {
    const SiftTile tl = tiles[blockIdx.x];
    const SiftImg& im = imgs[tl.img];
    const int w = im.w[oct], h = im.h[oct], sw = im.w[oct - 1], sh = im.h[oct - 1];
    const int col = tl.tx * kSiftTW + (int)(threadIdx.x & 63);
    if (col >= w) return;
    const float* src = planes + im.plane[oct - 1] + (int64_t)xsift::kDownLevel * sw * sh;
    float* dst = planes + im.plane[oct];
    const int sc = xsift::down_src_col(col, sw);
    for (int r = (int)(threadIdx.x >> 6); r < kSiftTH; r += kSiftWaves) {
        const int row = tl.ty * kSiftTH + r;
        if (row >= h) break;
        dst[(int64_t)row * w + col] = src[(int64_t)xsift::down_src_row(row) * sw + sc];
    }
}

// grid (tiles of the octave, 3 levels); the per-tile arrays are indexed level * n_tiles + tile.  COUNT: tile_count receives the number
// of keypoints.  EMIT: tile_first holds the first slot (negative: nothing is written), keys / loc / off receive at most tile_count
// keypoints and tile_emitted the number decided, which the host compares with tile_count.
template <bool EMIT>
__global__ __launch_bounds__(kSiftThreads) void k_sift_key(const SiftImg* __restrict__ imgs, const SiftTile* __restrict__ tiles, const float* __restrict__ planes,
                                                           int oct, int n_tiles, SiftKeyParams prm, int32_t* __restrict__ tile_count, const int32_t* __restrict__ tile_first,
                                                           int32_t* __restrict__ tile_emitted, float4* __restrict__ keys, int4* __restrict__ loc, float4* __restrict__ off) {
    __shared__ float s_d[3][kSiftTH + 2][kSiftTW + 2];
    __shared__ int s_n;
    const int j = (int)blockIdx.y;
    const int64_t slot_at = (int64_t)j * n_tiles + blockIdx.x;
    int64_t first = 0;
    int limit = 0;
    if (EMIT) {
        first = tile_first[slot_at];
        if (first < 0) return;
        limit = tile_count[slot_at];
    }
    const SiftTile tl = tiles[blockIdx.x];
    const SiftImg& im = imgs[tl.img];
    const int w = im.w[oct], h = im.h[oct], r0 = tl.ty * kSiftTH, c0 = tl.tx * kSiftTW;
    const int64_t n = (int64_t)w * h;
    const float* dog = planes + im.plane[oct] + (xsift::kGauss + j) * n;          // D[j], D[j+1], D[j+2]
    const int c = (int)(threadIdx.x & 63), rg = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) s_n = 0;
    for (int l = 0; l < 3; ++l)
        for (int rr = rg; rr < kSiftTH + 2; rr += kSiftWaves) {
            const int64_t row = xsift::clampi(r0 - 1 + rr, 0, h - 1);
            for (int cc = c; cc < kSiftTW + 2; cc += 64) s_d[l][rr][cc] = dog[l * n + row * w + xsift::clampi(c0 - 1 + cc, 0, w - 1)];
        }
    __syncthreads();
    const int col = c0 + c;
    for (int r = rg; r < kSiftTH; r += kSiftWaves) {
        const int row = r0 + r;
        if (!(row > 0 && col > 0 && row < h - 1 && col < w - 1)) continue;
        if (fabsf(s_d[1][r + 1][c + 1]) <= prm.T0) continue;
#define XSIFT_N9(l) s_d[l][r][c], s_d[l][r][c + 1], s_d[l][r][c + 2], s_d[l][r + 1][c], s_d[l][r + 1][c + 1], s_d[l][r + 1][c + 2], \
                    s_d[l][r + 2][c], s_d[l][r + 2][c + 1], s_d[l][r + 2][c + 2]
        const xsift::Key k = xsift::key_decide(XSIFT_N9(0), XSIFT_N9(1), XSIFT_N9(2), prm.T0, prm.T, prm.E);
#undef XSIFT_N9
        if (k.sign == 0.0f) continue;
        const int mine = atomicAdd(&s_n, 1);
        if (EMIT) {
            if (mine >= limit) continue;          // (never beyond the tile's own slots; the host sees the mismatch in tile_emitted)
            const int64_t at = first + mine;
            float X, Y, S;
            xsift::key_values(row, col, k.dx, k.dy, k.ds, j == 0 ? prm.key_sigma0 : (j == 1 ? prm.key_sigma1 : prm.key_sigma2), prm.step, prm.os, &X, &Y, &S);
            keys[at] = make_float4(X, Y, S, 0.0f);
            loc[at] = make_int4(oct, j, row, col);
            off[at] = make_float4(k.sign, k.dx, k.dy, k.ds);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) (EMIT ? tile_emitted : tile_count)[slot_at] = s_n;
}
