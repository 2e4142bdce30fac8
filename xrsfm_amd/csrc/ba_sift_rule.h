// The rule of the SIFT scale space and keypoint detection (SiftGPU::RunSIFT as SiftExtractor calls it with orientation fixed;
// reference 3rdparty/SiftGPU/SiftGPU.cpp:390-440 ParseSiftParam, PyramidCU.cpp:93-130, 252-295 geometry, :912-963 BuildPyramid,
// :756-800 the feature budget, :643-679 DownloadKeypoints; ProgramCU.cu:122-234 FilterH/FilterV, :236-277 UpsampleKernel,
// :305-317 DownsampleKernel, :408-433 CreateFilterKernel, :542-553 ComputeDOG_Kernel, :574-729 ComputeKEY_Kernel, :873-897 the keypoint
// values), restated.  Everything here is a rule and not a schedule: the kernels (ba_sift.h), the entry points and the sequential
// host driver of the CPU tests are compiled from this one text.  Plain C++ without HIP types; all arithmetic is float unless the
// reference's own expression promotes to double (the two "+ 0.001" tests, the exponential of a tap, the three 1e-10 guards).
//
// Quirks kept: the up-sample addresses its right-hand neighbour by FLAT index (at the last column that is the next row's first
// pixel); octave o is stored with its width rounded up to 4 and every kernel sees the stored width; the extremum tests of the 24
// outer neighbours let a tie pass where the centre-row test is strict, and a tie met on the maximum side moves the pixel to the
// minimum side for the rows that follow (so it survives only in the very last row read, and is then signed -1); the budget is
// tested BEFORE a level and can be overshot by part of one level.  Defined here where the reference is undefined: the up-sample's
// flat neighbour is clamped to the last pixel of the image and its lower row to the last row.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define XSIFT_HD __host__ __device__
#else
#define XSIFT_HD
#endif

namespace xsift {

constexpr int kGauss = 6;                     // Gaussian levels of an octave (level_min -1 .. level_max 4)
constexpr int kDog = 5;                       // their differences
constexpr int kKeyLevels = 3;                 // dog_level_num: D[1], D[2], D[3] are searched
constexpr int kDownLevel = 3;                 // level_ds - level_min: the Gaussian level the next octave is sampled from
constexpr int kMaxTaps = 33, kMinTaps = 5;    // KERNEL_MAX_WIDTH, KERNEL_MIN_WIDTH
constexpr int kMaxOctaves = 8;
constexpr int kMinSide = 16;

struct Taps {
    float w[kMaxTaps];
    int32_t width;
};

// CreateFilterKernel; host only (exp in double on the float argument, rounded once)
inline void build_taps(float sigma, Taps* t) {
    int sz = (int)std::ceil(4.0f * sigma - 0.5);
    int width = 2 * sz + 1;
    if (width > kMaxTaps) { sz = kMaxTaps >> 1; width = kMaxTaps; }
    else if (width < kMinTaps) { sz = kMinTaps >> 1; width = kMinTaps; }
    float rv = 1.0f / (sigma * sigma), ksum = 0.0f;
    for (int i = 0; i < kMaxTaps; ++i) t->w[i] = 0.0f;
    for (int i = -sz; i <= sz; ++i) {
        const float v = (float)std::exp((double)(-0.5f * i * i * rv));
        t->w[i + sz] = v;
        ksum += v;
    }
    rv = 1.0f / ksum;
    for (int i = 0; i < width; ++i) t->w[i] *= rv;
    t->width = width;
}

struct Params {
    float sigma0, step;                       // 1.6 * 2^(1/3), 2^(1/3)
    float level_sigma[kDog];                  // the filter from G[i] to G[i+1]
    float init_sigma;                         // of the first octave's smoothing; 0: skipped
    float key_sigma[kKeyLevels];              // GetLevelSigma(j)
    float T, T0, E;                           // peak threshold, 0.8 of it, (e + 1)^2 / e
};

// ParseSiftParam, GetInitialSmoothSigma, GetLevelSigma, ComputeKEY; host only (powf, sqrtf)
inline Params make_params(int first_octave, float peak_threshold, float edge_threshold) {
    Params p;
    const float k = powf(2.0f, 1.0f / 3);
    p.sigma0 = 1.6f * k;
    p.step = k;
    const float dsigma0 = p.sigma0 * sqrtf(1.0f - 1.0f / (k * k));
    for (int i = 0; i < kDog; ++i) p.level_sigma[i] = dsigma0 * powf(k, (float)i);
    const float sa = p.sigma0 * powf(2.0f, -1.0f / 3.0f), sb = 0.5f / powf(2.0f, (float)first_octave);
    p.init_sigma = sa > sb + 0.001 ? sqrtf(sa * sa - sb * sb) : 0.0f;
    for (int j = 0; j < kKeyLevels; ++j) p.key_sigma[j] = p.sigma0 * powf(2.0f, (float)j / 3.0f);
    p.T = peak_threshold;
    p.T0 = 0.8f * peak_threshold;
    p.E = (edge_threshold + 1) * (edge_threshold + 1) / edge_threshold;
    return p;
}

XSIFT_HD inline int truncate_width(int w) { return w & ~3; }          // TruncateWidthCU
XSIFT_HD inline int roundup4(int w) { return ((w + 3) / 4) * 4; }
XSIFT_HD inline int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct Geometry {
    int32_t w_in, h_in;                       // the part of the input that is read
    int32_t n_oct;
    int32_t w[kMaxOctaves], h[kMaxOctaves];   // stored width, height
};

// PyramidCU::ResizePyramid / FitPyramid
inline Geometry geometry(int width, int height, int first_octave, int num_octaves) {
    Geometry g{};
    g.w_in = truncate_width(width);
    g.h_in = height;
    const int w0 = first_octave < 0 ? g.w_in << 1 : g.w_in, h0 = first_octave < 0 ? g.h_in << 1 : g.h_in;
    int lg = 0;
    for (int m = w0 < h0 ? w0 : h0; m > 1; m >>= 1) ++lg;
    const int most = lg - 3 > 1 ? lg - 3 : 1;
    g.n_oct = num_octaves < most ? num_octaves : most;
    for (int o = 0; o < g.n_oct; ++o) { g.w[o] = roundup4(w0 >> o); g.h[o] = h0 >> o; }
    return g;
}

XSIFT_HD inline float pixel_value(uint8_t b) { return (float)b / 255.0f; }

// UpsampleKernel<1>: destination pixel (dr, dc) of the 2w x 2h image; src(i) is pixel i (flat, row-major) of the w x h source
template <class Src>
XSIFT_HD inline float upsample_at(const Src& src, int w, int h, int dr, int dc) {
    const int last = w * h - 1, row = dr >> 1, index = row * w + (dc >> 1);
    const int right = index + 1 < last ? index + 1 : last;
    float v1 = src(index), v2 = src(right);
    if (dr & 1) {
        const int row2 = row + 1 < h - 1 ? row + 1 : h - 1, index2 = row2 * w + (dc >> 1);
        const int right2 = index2 + 1 < last ? index2 + 1 : last;
        const float v21 = src(index2), v22 = src(right2);
        const float w1 = 0.5f * 1, w2 = (float)(1.0 - w1);
        v1 = v21 * w1 + w2 * v1;
        v2 = v22 * w1 + w2 * v2;
    }
    if (!(dc & 1)) return v1;
    const float r2 = 1 * 0.5f, r1 = 1.0f - r2;
    return v1 * r1 + v2 * r2;
}

// DownsampleKernel<1>
XSIFT_HD inline int down_src_col(int dst_col, int src_w) { return (dst_col << 1) < src_w - 1 ? (dst_col << 1) : src_w - 1; }
XSIFT_HD inline int down_src_row(int dst_row) { return dst_row << 1; }

// one row of READ_CMP_DOG_DATA; true: rejected
XSIFT_HD inline bool cmp_row(float a, float b, float c, float v, float& nmax, float& nmin) {
    if (v > nmax) {
        nmax = fmaxf(nmax, a); nmax = fmaxf(nmax, b); nmax = fmaxf(nmax, c);
        if (v < nmax) return true;
    } else {
        nmin = fminf(nmin, a); nmin = fminf(nmin, b); nmin = fminf(nmin, c);
        if (v > nmin) return true;
    }
    return false;
}

struct Key {
    float sign, dx, dy, ds;                   // sign 0: no keypoint
    int32_t why;                              // the branch that decided (KeyWhy); for the tests' coverage only
};
enum KeyWhy : int32_t { kKept = 0, kThreshold = 1, kCentreRow = 2, kNeighbour = 3, kEdgeDet = 4, kEdgeRatio = 5, kContrast = 6, kOffDs = 7,
                        kOffDx = 8, kOffDy = 9, kKeptGuard = 10 };

// ComputeKEY_Kernel on one pixel: p, c, n are the 3 x 3 neighbourhoods [row][col] of the previous, the pixel's own and the next
// DoG level, passed as nine scalars each so that no indexed private array is formed on the device.
XSIFT_HD inline Key key_decide(float p00, float p01, float p02, float p10, float p11, float p12, float p20, float p21, float p22,
                               float c00, float c01, float c02, float c10, float c11, float c12, float c20, float c21, float c22,
                               float n00, float n01, float n02, float n10, float n11, float n12, float n20, float n21, float n22,
                               float T0, float T, float E) {
    Key k{0.0f, 0.0f, 0.0f, 0.0f, kThreshold};
    const float v = c11;
    if (fabsf(v) <= T0) return k;
    float nmax = fmaxf(c10, c12), nmin = fminf(c10, c12);
    k.why = kCentreRow;
    if (v <= nmax && v >= nmin) return k;
    k.why = kNeighbour;
    if (cmp_row(c00, c01, c02, v, nmax, nmin)) return k;
    if (cmp_row(c20, c21, c22, v, nmax, nmin)) return k;
    const float vx2 = v * 2.0f;
    const float fxx = c10 + c12 - vx2, fyy = c01 + c21 - vx2, fxy = 0.25f * (c22 + c00 - c20 - c02);
    const float temp1 = fxx * fyy - fxy * fxy, temp2 = (fxx + fyy) * (fxx + fyy);
    k.why = kEdgeDet;
    if (temp1 <= 0) return k;
    k.why = kEdgeRatio;
    if (temp2 > E * temp1) return k;
    k.why = kNeighbour;
    if (cmp_row(p00, p01, p02, v, nmax, nmin)) return k;
    if (cmp_row(p10, p11, p12, v, nmax, nmin)) return k;
    if (cmp_row(p20, p21, p22, v, nmax, nmin)) return k;
    if (cmp_row(n00, n01, n02, v, nmax, nmin)) return k;
    if (cmp_row(n10, n11, n12, v, nmax, nmin)) return k;
    if (cmp_row(n20, n21, n22, v, nmax, nmin)) return k;
    const float fx = 0.5f * (c12 - c10), fy = 0.5f * (c21 - c01), fs = 0.5f * (n11 - p11);
    const float fss = n11 + p11 - vx2, fxs = 0.25f * (n12 + p10 - n10 - p12), fys = 0.25f * (n21 + p01 - n01 - p21);
    // rows (x, y, z, w) of the augmented system, each with its first entry made non-negative
    float a0x, a0y, a0z, a0w, a1x, a1y, a1z, a1w, a2x, a2y, a2z, a2w;
    if (fxx > 0) { a0x = fxx; a0y = fxy; a0z = fxs; a0w = -fx; } else { a0x = -fxx; a0y = -fxy; a0z = -fxs; a0w = fx; }
    if (fxy > 0) { a1x = fxy; a1y = fyy; a1z = fys; a1w = -fy; } else { a1x = -fxy; a1y = -fyy; a1z = -fys; a1w = fy; }
    if (fxs > 0) { a2x = fxs; a2y = fys; a2z = fss; a2w = -fs; } else { a2x = -fxs; a2y = -fys; a2z = -fss; a2w = fs; }
    const float maxa = fmaxf(fmaxf(a0x, a1x), a2x);
    float dx = 0.0f, dy = 0.0f, ds = 0.0f;
    bool passed = true;
    k.why = kKeptGuard;
    if ((double)maxa >= 1e-10) {
        float t;
        if (maxa == a1x) {
            t = a1x; a1x = a0x; a0x = t; t = a1y; a1y = a0y; a0y = t; t = a1z; a1z = a0z; a0z = t; t = a1w; a1w = a0w; a0w = t;
        } else if (maxa == a2x) {
            t = a2x; a2x = a0x; a0x = t; t = a2y; a2y = a0y; a0y = t; t = a2z; a2z = a0z; a0z = t; t = a2w; a2w = a0w; a0w = t;
        }
        a0y /= a0x; a0z /= a0x; a0w /= a0x;
        a1y -= a1x * a0y; a1z -= a1x * a0z; a1w -= a1x * a0w;
        a2y -= a2x * a0y; a2z -= a2x * a0z; a2w -= a2x * a0w;
        if (fabsf(a2y) > fabsf(a1y)) {
            t = a2x; a2x = a1x; a1x = t; t = a2y; a2y = a1y; a1y = t; t = a2z; a2z = a1z; a1z = t; t = a2w; a2w = a1w; a1w = t;
        }
        if ((double)fabsf(a1y) >= 1e-10) {
            a1z /= a1y; a1w /= a1y;
            a2z -= a2y * a1z; a2w -= a2y * a1w;
            if ((double)fabsf(a2z) >= 1e-10) {
                ds = a2w / a2z;
                dy = a1w - ds * a1z;
                dx = a0w - ds * a0z - dy * a0y;
                k.why = kKept;
                if (!(fabsf(v + 0.5f * (dx * fx + dy * fy + ds * fs)) > T)) { passed = false; k.why = kContrast; }
                else if (!(fabsf(ds) < 1.0f)) { passed = false; k.why = kOffDs; }
                else if (!(fabsf(dx) < 1.0f)) { passed = false; k.why = kOffDx; }
                else if (!(fabsf(dy) < 1.0f)) { passed = false; k.why = kOffDy; }
            }
        }
    }
    k.dx = dx; k.dy = dy; k.ds = ds;          // (the reference stores the offsets of a pixel the offset test rejects, too)
    if (passed) k.sign = v > nmax ? 1.0f : -1.0f;
    return k;
}

// ComputeOrientation_Kernel with num_orientation 0, then DownloadKeypoints: (X, Y, S) in input-image coordinates.
// os = 2^(first_octave + octave).  powf runs where the caller runs.
XSIFT_HD inline void key_values(int row, int col, float dx, float dy, float ds, float level_sigma, float step, float os, float* X, float* Y, float* S) {
    float x = col + 0.5f, y = row + 0.5f, s = level_sigma;
    x += dx; y += dy; s *= powf(step, ds);
    *X = os * (x - 0.5f) + 0.5f;
    *Y = os * (y - 0.5f) + 0.5f;
    *S = os * s;
}

XSIFT_HD inline float octave_scale(int first_octave, int octave) {
    const int e = first_octave + octave;
    return e >= 0 ? (float)(1 << e) : 1.0f / (float)(1 << (-e));
}

// GenerateFeatureList with _TruncateMethod 1: take[o * 3 + j] says whether level j of octave o contributes; returns the total
inline int64_t budget(const int32_t* level_count, int n_oct, int max_num_features, uint8_t* take) {
    int64_t total = 0;
    for (int o = n_oct - 1; o >= 0; --o)
        for (int j = kKeyLevels - 1; j >= 0; --j) {
            const int idx = o * kKeyLevels + j;
            take[idx] = total > max_num_features ? 0 : 1;
            if (take[idx]) total += level_count[idx];
        }
    return total;
}

}  // namespace xsift
