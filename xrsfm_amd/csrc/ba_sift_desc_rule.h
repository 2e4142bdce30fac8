// The rule of SIFT orientation and descriptors (the second half of SiftGPU::RunSIFT and what SiftExtractor does after it; reference
// 3rdparty/SiftGPU/ProgramCU.cu:521-540 the `got` half of ComputeDOG_Kernel, :861-957 ComputeOrientation_Kernel with num_orientation
// 1, :1053-1132 ComputeDescriptor_Kernel<false>, :1202-1237 NormalizeDescriptor_Kernel; PyramidCU.cpp:379-417 GetFeatureDescriptors,
// :1092-1120 GetFeatureOrientations, :643-679 DownloadKeypoints; src/feature/sift_extractor.cc:99-110 L1RootNormalizeFeatureDescriptors,
// sift_extractor.h:16-34 TruncateCast and FeatureDescriptorsToUnsignedByte), restated.  Like ba_sift_rule.h this is a rule and not a
// schedule: the kernels (ba_sift_desc.h), the entry points and the sequential host program of the CPU tests are compiled from this
// one text.  Plain C++ without HIP types; FP32 throughout, with the reference's order of operations; double only where the
// reference's own expression promotes (dist_threshold's "+ 0.5", the wrap of the angle at pi, "1.0 - nxn", the mirror's fmod).
//
// Quirks kept: ComputeDescriptor_Kernel<false> (_UseDynamicIndexing 0) matches the bin against k = 0..7 only, so a theta that rounds
// to exactly 8.0f (a tiny negative angle difference plus 8) is DROPPED with its whole weight; the smoothing of the histogram reads
// the unsmoothed predecessor and successor and takes vote[36] = vote[0] at the start of a pass; the strict arg-max takes the first
// of equals; the windows clamp to 1.5 .. w - 1.5 of the STORED width, so border pixels of a gradient plane are never read.
// Defined here where the reference is undefined: the parabola through an arg-max whose denominator 2 max - next - pre is zero (the
// reference divides and hands out a NaN, from all-zero votes for instance) has the offset 0.
// Deviations: sin, cos, exp, atan2 and rsqrt are the accurate functions of the library this text is compiled for (the reference
// calls __sincosf); a kernel sums a window in its own fixed order, not in the single-thread order of the loops below.
#pragma once

#include <cmath>
#include <cstdint>

#include "ba_sift_rule.h"

namespace xsiftd {

constexpr float kTenDegPerRad = 5.7295779513082320876798154814105;
constexpr float kRadPerTenDeg = 1.0 / 5.7295779513082320876798154814105;
constexpr float kOneThird = 1.0 / 3.0;
constexpr float kRpi = 4.0 / 3.14159265358979323846;
constexpr float kOrientGauss = 1.5f, kOrientWindow = 2.0f;          // _OrientationGaussianFactor, _OrientationWindowFactor
constexpr float kDescWindow = 3.0f;                                  // _DescriptorWindowFactor
constexpr int kBins = 36, kSmoothPasses = 6, kCells = 16, kDesc = 128;

// ComputeDOG_Kernel, the got half: xn, xp, yn, yp are G at index + 1, - 1, + w, - w
XSIFT_HD inline void gradient(float xn, float xp, float yn, float yp, float* grd, float* rot) {
    const float dx = xn - xp, dy = yn - yp;
    const float g = 0.5f * sqrtf(dx * dx + dy * dy);
    *grd = g;
    *rot = g == 0.0f ? 0.0f : atan2f(dy, dx);
}

// the key ComputeOrientation_Kernel forms from the list and the offsets (subpixel 1, keepsign 0)
XSIFT_HD inline void octave_key(int row, int col, float dx, float dy, float ds, float level_sigma, float step, float* x, float* y, float* s) {
    float kx = col + 0.5f, ky = row + 0.5f, kz = level_sigma;
    kx += dx; ky += dy; kz *= powf(step, ds);
    *x = kx; *y = ky; *s = kz;
}

struct Window { float xmin, ymin, xmax, ymax; };

struct OrientFrame {
    float dist_threshold, factor;
    Window win;
};

XSIFT_HD inline OrientFrame orient_frame(float kx, float ky, float kz, int width, int height) {
    OrientFrame f;
    const float gsigma = kz * kOrientGauss;
    const float win = fabsf(kz) * (kOrientGauss * kOrientWindow);
    f.dist_threshold = (float)(win * win + 0.5);
    f.factor = -0.5f / (gsigma * gsigma);
    f.win.xmin = fmaxf(1.5f, floorf(kx - win) + 0.5f);
    f.win.ymin = fmaxf(1.5f, floorf(ky - win) + 0.5f);
    f.win.xmax = fminf(width - 1.5f, floorf(kx + win) + 0.5f);
    f.win.ymax = fminf(height - 1.5f, floorf(ky + win) + 0.5f);
    return f;
}

// is the sample (x, y) inside the circle?  (sq_dist is handed back for the weight)
XSIFT_HD inline bool orient_inside(const OrientFrame& f, float kx, float ky, float x, float y, float* sq_dist) {
    const float dx = x - kx, dy = y - ky;
    *sq_dist = dx * dx + dy * dy;
    return !(*sq_dist >= f.dist_threshold);
}
XSIFT_HD inline float orient_weight(const OrientFrame& f, float sq_dist, float grd) { return grd * expf(sq_dist * f.factor); }
XSIFT_HD inline int orient_bin(float rot) {
    int oidx = (int)floorf(rot * kTenDegPerRad);
    if (oidx < 0) oidx += kBins;
    return oidx;
}
// one value of one smoothing pass: the unsmoothed predecessor, the bin and the unsmoothed successor
XSIFT_HD inline float orient_smooth(float pre, float v, float next) { return kOneThird * (pre + v + next); }
// the parabola through the arg-max and its neighbours
XSIFT_HD inline float orient_angle(int index_max, float pre, float max_vote, float next) {
    const float den = max_vote + max_vote - next - pre;
    const float off = den == 0.0f ? 0.0f : 0.5f * ((next - pre) / den);
    return kRadPerTenDeg * (index_max + 0.5f + off);
}

// the whole histogram of one keypoint in the reference's order; host only (vote is indexed)
template <class Got>
inline float orientation(const Got& got, int width, int height, float kx, float ky, float kz, float* vote_out /* [36], may be null */) {
    const OrientFrame f = orient_frame(kx, ky, kz, width, height);
    float vote[kBins + 1];
    for (int i = 0; i <= kBins; ++i) vote[i] = 0.0f;
    for (float y = f.win.ymin; y <= f.win.ymax; y += 1.0f)
        for (float x = f.win.xmin; x <= f.win.xmax; x += 1.0f) {
            float sq;
            if (!orient_inside(f, kx, ky, x, y, &sq)) continue;
            float grd, rot;
            got((int)x, (int)y, &grd, &rot);
            vote[orient_bin(rot)] += orient_weight(f, sq, grd);
        }
    for (int i = 0; i < kSmoothPasses; ++i) {
        vote[kBins] = vote[0];
        float pre = vote[kBins - 1];
        for (int j = 0; j < kBins; ++j) {
            const float temp = orient_smooth(pre, vote[j], vote[j + 1]);
            pre = vote[j];
            vote[j] = temp;
        }
    }
    vote[kBins] = vote[0];
    int index_max = 0;
    float max_vote = vote[0];
    for (int i = 1; i < kBins; ++i) {
        index_max = vote[i] > max_vote ? i : index_max;
        max_vote = fmaxf(max_vote, vote[i]);
    }
    if (vote_out) for (int i = 0; i < kBins; ++i) vote_out[i] = vote[i];
    return orient_angle(index_max, vote[index_max == 0 ? kBins - 1 : index_max - 1], max_vote, vote[index_max + 1]);
}

// ComputeDescriptor_Kernel: what all sixteen cells of a keypoint share
struct DescFrame {
    float anglef, cspt, sspt, crspt, srspt, bsz;
};

XSIFT_HD inline DescFrame desc_frame(float kz, float kw) {
    DescFrame f;
    const float spt = fabsf(kz * kDescWindow);
    const float s = sinf(kw), c = cosf(kw);
    f.anglef = (float)(kw > 3.14159265358979323846 ? kw - (2.0 * 3.14159265358979323846) : kw);
    f.cspt = c * spt; f.sspt = s * spt;
    f.crspt = c / spt; f.srspt = s / spt;
    f.bsz = fabsf(f.cspt) + fabsf(f.sspt);
    return f;
}

struct DescCell { float offx, offy, ptx, pty; Window win; };

XSIFT_HD inline DescCell desc_cell(const DescFrame& f, float kx, float ky, int ix, int iy, int width, int height) {
    DescCell c;
    c.offx = ix - 1.5f; c.offy = iy - 1.5f;
    c.ptx = f.cspt * c.offx - f.sspt * c.offy + kx;
    c.pty = f.cspt * c.offy + f.sspt * c.offx + ky;
    c.win.xmin = fmaxf(1.5f, floorf(c.ptx - f.bsz) + 0.5f);
    c.win.ymin = fmaxf(1.5f, floorf(c.pty - f.bsz) + 0.5f);
    c.win.xmax = fminf(width - 1.5f, floorf(c.ptx + f.bsz) + 0.5f);
    c.win.ymax = fminf(height - 1.5f, floorf(c.pty + f.bsz) + 0.5f);
    return c;
}

// the position of a sample in the cell's frame; false: outside the cell, the gradient is not read
XSIFT_HD inline bool desc_inside(const DescFrame& f, const DescCell& c, float x, float y, float* nx, float* ny) {
    const float dx = x - c.ptx, dy = y - c.pty;
    *nx = f.crspt * dx + f.srspt * dy;
    *ny = f.crspt * dy - f.srspt * dx;
    return fabsf(*nx) < 1.0f && fabsf(*ny) < 1.0f;
}

// the sample's weight and its place among the eight bins: theta, of which floor(theta) is the bin.  theta == 8.0f: dropped
XSIFT_HD inline void desc_sample(const DescFrame& f, const DescCell& c, float nx, float ny, float grd, float rot, float* weight, float* theta) {
    const float dnx = nx + c.offx, dny = ny + c.offy;
    const float ww = expf(-0.125f * (dnx * dnx + dny * dny));
    const float wx = (float)(1.0 - fabsf(nx)), wy = (float)(1.0 - fabsf(ny));
    *weight = ww * wx * wy * grd;
    float th = (f.anglef - rot) * kRpi;
    if (th < 0) th += 8.0f;
    *theta = th;
}

// the static select of the reference: des0 .. des8 are nine scalars so that no indexed private array is formed on the device
#define XSIFTD_ACCUMULATE_ONE(des, k)  if (fidx_ == k) { des[k] += w1_; des[k + 1] += w2_; }
#define XSIFTD_ACCUMULATE(des, weight, theta)                                     \
    do {                                                                          \
        const float fo_ = floorf(theta);                                          \
        const int fidx_ = (int)fo_;                                               \
        const float w1_ = (fo_ + 1.0f - (theta)) * (weight), w2_ = ((theta) - fo_) * (weight); \
        XSIFTD_ACCUMULATE_ONE(des, 0) XSIFTD_ACCUMULATE_ONE(des, 1) XSIFTD_ACCUMULATE_ONE(des, 2) XSIFTD_ACCUMULATE_ONE(des, 3) \
        XSIFTD_ACCUMULATE_ONE(des, 4) XSIFTD_ACCUMULATE_ONE(des, 5) XSIFTD_ACCUMULATE_ONE(des, 6) XSIFTD_ACCUMULATE_ONE(des, 7) \
    } while (0)

// one cell in the reference's order: des [8]
template <class Got>
inline void descriptor_cell(const Got& got, int width, int height, float kx, float ky, const DescFrame& f, int ix, int iy, float* des8, int* dropped) {
    const DescCell c = desc_cell(f, kx, ky, ix, iy, width, height);
    float des[9];
    for (int i = 0; i < 9; ++i) des[i] = 0.0f;
    for (float y = c.win.ymin; y <= c.win.ymax; y += 1.0f)
        for (float x = c.win.xmin; x <= c.win.xmax; x += 1.0f) {
            float nx, ny;
            if (!desc_inside(f, c, x, y, &nx, &ny)) continue;
            float grd, rot, weight, theta;
            got((int)x, (int)y, &grd, &rot);
            desc_sample(f, c, nx, ny, grd, rot, &weight, &theta);
            if (dropped && !(theta < 8.0f)) ++*dropped;
            XSIFTD_ACCUMULATE(des, weight, theta);
        }
    des[0] += des[8];
    for (int i = 0; i < 8; ++i) des8[i] = des[i];
}

XSIFT_HD inline float rsqrt_of(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return rsqrtf(v);
#else
    return 1.0f / sqrtf(v);
#endif
}
XSIFT_HD inline float sumsq4(float a, float b, float c, float d) { return a * a + b * b + c * c + d * d; }
XSIFT_HD inline float abs_sum4(float a, float b, float c, float d) { return fabsf(a) + fabsf(b) + fabsf(c) + fabsf(d); }
XSIFT_HD inline float clamp_unit(float v, float norm1) { return fminf(0.2f, v * norm1); }

// NormalizeDescriptor_Kernel on the 128 sums (the norm is summed float4 by float4); host order
inline void normalize(const float* raw, float* unit) {
    float norm1 = 0.0f, norm2 = 0.0f;
    for (int i = 0; i < kDesc; i += 4) norm1 += sumsq4(raw[i], raw[i + 1], raw[i + 2], raw[i + 3]);
    norm1 = rsqrt_of(norm1);
    for (int i = 0; i < kDesc; ++i) unit[i] = clamp_unit(raw[i], norm1);
    for (int i = 0; i < kDesc; i += 4) norm2 += sumsq4(unit[i], unit[i + 1], unit[i + 2], unit[i + 3]);
    norm2 = rsqrt_of(norm2);
    for (int i = 0; i < kDesc; ++i) unit[i] *= norm2;
}

// L1RootNormalizeFeatureDescriptors on one value, given the row's sum of absolute values
XSIFT_HD inline float l1_root(float v, float l1) { return sqrtf(v / l1); }
// FeatureDescriptorsToUnsignedByte: std::round rounds half away from zero; TruncateCast clamps to 0 .. 255
XSIFT_HD inline uint8_t to_byte(float v) {
    const float scaled = roundf(512.0f * v);
    return (uint8_t)fminf(255.0f, fmaxf(0.0f, scaled));
}

inline void l1_root_and_bytes(const float* unit, float* desc_float, uint8_t* desc) {
    float l1 = 0.0f;          // (lpNorm<1> leaves the order to Eigen; here: four by four, like the norms above)
    for (int i = 0; i < kDesc; i += 4) l1 += abs_sum4(unit[i], unit[i + 1], unit[i + 2], unit[i + 3]);
    for (int i = 0; i < kDesc; ++i) { desc_float[i] = l1_root(unit[i], l1); desc[i] = to_byte(desc_float[i]); }
}

// DownloadKeypoints: the orientation as it is handed out
inline float mirror(float w) {
    const double twopi = 2.0 * 3.14159265358979323846;
    return (float)fmod(twopi - w, twopi);
}

}  // namespace xsiftd
