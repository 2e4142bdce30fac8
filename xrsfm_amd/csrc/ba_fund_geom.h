// The geometry of the pair verification (ba_fund.h: k_verify_pairs): the 7-point sample models, the stages of the 8-point local
// model and the Sampson residual of reference src/geometry/colmap/estimators/fundamental_matrix.cc:47-295.  Plain C++ for host and
// device; the kernel and the host drivers of the CPU tests are compiled from this file.  A model is 9 doubles, row-major, with
// x_b' F x_a = 0; coordinates are pixels.
//
// 7-point model (:47-142).  The 7 x 9 system is that of :56-71, on raw coordinates.  Its null space comes from the matrix itself:
// Householder QR of the transpose (9 x 7, one reflector per column, the sign of the reflector opposite to the pivot's), g1 = Q e7,
// g2 = Q e8; then f1 = g1 - g2, f2 = g2 and the cubic det(lambda f1 + f2) = 0 of :84-107.  Roots: leading zeros lower the degree
// (RemoveLeadingZeros); a cubic is made monic, one real root is bracketed by [-R, R], R = 1 + max |coefficient|, and found by
// kBisect bisection steps; the deflated quadratic is solved in closed form; every real root gets kPolish Newton steps on the
// original polynomial.  A complex pair is taken (as its real part, twice) when |Im| <= 1e-10.  A root is dropped when
// |F(2,2)| < 1e-10; F is divided by F(2,2).  Deviation 2 of include/xrsfm_ba.h: the models of one trial are offered in ascending
// root on THIS basis (the reference's basis is whatever its SVD returns).
//
// 8-point model (:150-194), in stages so that the kernel can reduce the sums over the inliers with the whole workgroup:
// CenterAndNormalizeImagePoints on both images (sums 1 and 2), the 9 x 9 Gram matrix of the constraint rows (sum 3: 45 entries)
// and its eigenvector of smallest eigenvalue by cyclic Jacobi (xpnp::jacobi_eig) in place of the SVD of the n x 9 matrix; the
// rank-2 projection by a one-sided Jacobi SVD of the 3 x 3, F' = a1 v1' + a2 v2' over the two columns of largest image: no third
// singular vector is formed, so nothing depends on how a library signs one (deviation 3); F = T2' F' T1.
#pragma once

#include "ba_fund_scan.h"
#include "ba_pnp_geom.h"

namespace xfund {

constexpr int kWs7 = 88;                      // doubles of workspace per 7-point solve: M[63] (column j at 9 j), vn[7], g1[9], g2[9]
constexpr int kBisect = 128;
constexpr int kPolish = 2;
constexpr double kRootMaxImag = 1e-10;
constexpr double kF22Eps = 1e-10;
constexpr int kSvdSweeps = 20;

struct PlainWs {
    double* p;
    XFUND_HD double& operator()(int e) const { return p[e]; }
};

// ComputeSquaredSampsonError (:202-246) for one match
XFUND_HD inline double sampson(const double* F, double xa, double ya, double xb, double yb) {
    const double Fx0 = F[0] * xa + F[1] * ya + F[2];
    const double Fx1 = F[3] * xa + F[4] * ya + F[5];
    const double Fx2 = F[6] * xa + F[7] * ya + F[8];
    const double Ft0 = F[0] * xb + F[3] * yb + F[6];
    const double Ft1 = F[1] * xb + F[4] * yb + F[7];
    const double e = xb * Fx0 + yb * Fx1 + Fx2;
    return e * e / (Fx0 * Fx0 + Fx1 * Fx1 + Ft0 * Ft0 + Ft1 * Ft1);
}
XFUND_HD inline bool is_inlier(double r, double max_res) { return r <= max_res; }             // (false for NaN)

// row j of the 7 x 9 system = column j of M
template <class W>
XFUND_HD inline void seven_point_row(W ws, int j, double xa, double ya, double xb, double yb) {
    ws(9 * j + 0) = xb * xa; ws(9 * j + 1) = xb * ya; ws(9 * j + 2) = xb;
    ws(9 * j + 3) = yb * xa; ws(9 * j + 4) = yb * ya; ws(9 * j + 5) = yb;
    ws(9 * j + 6) = xa;      ws(9 * j + 7) = ya;      ws(9 * j + 8) = 1.0;
}

XFUND_HD inline double poly_polish(double c0, double c1, double c2, double c3, double r) {
    for (int it = 0; it < kPolish; ++it) {
        const double p = ((c0 * r + c1) * r + c2) * r + c3;
        const double d = (3.0 * c0 * r + 2.0 * c1) * r + c2;
        const double step = p / d;
        if (d != 0.0 && fabs(step) <= DBL_MAX) r -= step;
    }
    return r;
}

// the roots taken of c0 x^3 + c1 x^2 + c2 x + c3, ascending; returns their number
XFUND_HD inline int cubic_roots(double c0, double c1, double c2, double c3, double& r0, double& r1, double& r2) {
    int nr = 0;
    double B, Cq;                       // the quadratic x^2 + B x + Cq left to solve
    bool quad = false;
    if (c0 != 0.0) {
        const double a = c1 / c0, b = c2 / c0, c = c3 / c0;
        const double R = 1.0 + fmax(fabs(a), fmax(fabs(b), fabs(c)));
        if (!(R <= DBL_MAX)) return 0;
        double lo = -R, hi = R;
        for (int it = 0; it < kBisect; ++it) {
            const double mid = 0.5 * (lo + hi);
            const double pm = ((mid + a) * mid + b) * mid + c;
            if (pm < 0.0) lo = mid; else hi = mid;
        }
        const double r = poly_polish(c0, c1, c2, c3, 0.5 * (lo + hi));
        r0 = r; nr = 1;
        B = a + r; Cq = b + r * B; quad = true;
    } else if (c1 != 0.0) {
        B = c2 / c1; Cq = c3 / c1; quad = true;
    } else if (c2 != 0.0) {
        r0 = -c3 / c2; nr = 1;
    }
    if (quad) {
        const double disc = B * B - 4.0 * Cq;
        double q1, q2;
        bool two = false;
        if (disc >= 0.0) {
            const double qq = -0.5 * (B + copysign(sqrt(disc), B));
            q1 = poly_polish(c0, c1, c2, c3, qq);
            q2 = poly_polish(c0, c1, c2, c3, qq != 0.0 ? Cq / qq : 0.0);
            two = true;
        } else if (0.5 * sqrt(-disc) <= kRootMaxImag) {
            q1 = q2 = -0.5 * B;
            two = true;
        }
        if (two) {
            if (nr == 0) { r0 = q1; r1 = q2; } else { r1 = q1; r2 = q2; }
            nr += 2;
        }
    }
    // ascending (three compare-exchanges at most)
    if (nr >= 2 && r1 < r0) { const double t = r0; r0 = r1; r1 = t; }
    if (nr == 3 && r2 < r1) { const double t = r1; r1 = r2; r2 = t; }
    if (nr == 3 && r1 < r0) { const double t = r0; r0 = r1; r1 = t; }
    return nr;
}

// FundamentalMatrixSevenPointEstimator::Estimate on the rows set by seven_point_row: up to three models (9 doubles each) written to
// out in ascending order of the root; returns their number.  Non-finite models are dropped.
template <class W>
XFUND_HD inline int seven_point_models(W ws, double* out) {
    for (int j = 0; j < 7; ++j) {
        double nn = 0.0;
        for (int i = j; i < 9; ++i) nn += ws(9 * j + i) * ws(9 * j + i);
        const double x0 = ws(9 * j + j);
        const double alpha = x0 > 0.0 ? -sqrt(nn) : sqrt(nn);
        ws(9 * j + j) = x0 - alpha;
        double vn = 0.0;
        for (int i = j; i < 9; ++i) vn += ws(9 * j + i) * ws(9 * j + i);
        ws(63 + j) = vn;
        if (!(vn > 0.0)) continue;
        for (int c = j + 1; c < 7; ++c) {
            double d = 0.0;
            for (int i = j; i < 9; ++i) d += ws(9 * j + i) * ws(9 * c + i);
            d = 2.0 * d / vn;
            for (int i = j; i < 9; ++i) ws(9 * c + i) -= d * ws(9 * j + i);
        }
    }
    for (int k = 0; k < 2; ++k) {
        const int g = 70 + 9 * k;
        for (int i = 0; i < 9; ++i) ws(g + i) = (i == 7 + k) ? 1.0 : 0.0;
        for (int j = 6; j >= 0; --j) {
            const double vn = ws(63 + j);
            if (!(vn > 0.0)) continue;
            double d = 0.0;
            for (int i = j; i < 9; ++i) d += ws(9 * j + i) * ws(g + i);
            d = 2.0 * d / vn;
            for (int i = j; i < 9; ++i) ws(g + i) -= d * ws(9 * j + i);
        }
    }
    const double b0 = ws(79), b1 = ws(80), b2 = ws(81), b3 = ws(82), b4 = ws(83), b5 = ws(84), b6 = ws(85), b7 = ws(86), b8 = ws(87);
    const double a0 = ws(70) - b0, a1 = ws(71) - b1, a2 = ws(72) - b2, a3 = ws(73) - b3, a4 = ws(74) - b4, a5 = ws(75) - b5, a6 = ws(76) - b6,
                 a7 = ws(77) - b7, a8 = ws(78) - b8;
    const double t0 = a4 * a8 - a5 * a7, t1 = a3 * a8 - a5 * a6, t2 = a3 * a7 - a4 * a6;
    const double t3 = b4 * b8 - b5 * b7, t4 = b3 * b8 - b5 * b6, t5 = b3 * b7 - b4 * b6;
    const double c0 = a0 * t0 - a1 * t1 + a2 * t2;
    const double c1 = b0 * t0 - b1 * t1 + b2 * t2 - b3 * (a1 * a8 - a2 * a7) + b4 * (a0 * a8 - a2 * a6) - b5 * (a0 * a7 - a1 * a6) +
                      b6 * (a1 * a5 - a2 * a4) - b7 * (a0 * a5 - a2 * a3) + b8 * (a0 * a4 - a1 * a3);
    const double c2 = a0 * t3 - a1 * t4 + a2 * t5 - a3 * (b1 * b8 - b2 * b7) + a4 * (b0 * b8 - b2 * b6) - a5 * (b0 * b7 - b1 * b6) +
                      a6 * (b1 * b5 - b2 * b4) - a7 * (b0 * b5 - b2 * b3) + a8 * (b0 * b4 - b1 * b3);
    const double c3 = b0 * t3 - b1 * t4 + b2 * t5;
    if (!(fabs(c0) <= DBL_MAX && fabs(c1) <= DBL_MAX && fabs(c2) <= DBL_MAX && fabs(c3) <= DBL_MAX)) return 0;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    const int nr = cubic_roots(c0, c1, c2, c3, r0, r1, r2);
    int nm = 0;
    for (int k = 0; k < nr; ++k) {
        const double lam = k == 0 ? r0 : (k == 1 ? r1 : r2);
        const double f8 = lam * a8 + b8;
        if (!(fabs(f8) >= kF22Eps)) continue;
        double* m = out + 9 * nm;
        m[0] = (lam * a0 + b0) / f8; m[1] = (lam * a1 + b1) / f8; m[2] = (lam * a2 + b2) / f8;
        m[3] = (lam * a3 + b3) / f8; m[4] = (lam * a4 + b4) / f8; m[5] = (lam * a5 + b5) / f8;
        m[6] = (lam * a6 + b6) / f8; m[7] = (lam * a7 + b7) / f8; m[8] = f8 / f8;
        if (xpnp::all_finite(m, 9)) ++nm;
    }
    return nm;
}

// ---- the 8-point model in stages; the sums over the inliers are the caller's (red[] holds the last one)
struct Eight {
    double red[48];
    double n;                   // number of inliers
    double ca[2], cb[2];        // centroids
    double sa, sb;              // sqrt(2) / rms distance
    double g[81], v[81];
    double F[9];
};

// sum 1: x_a, y_a, x_b, y_b, 1
XFUND_HD inline void eight_terms1(double xa, double ya, double xb, double yb, double* acc) {
    acc[0] += xa; acc[1] += ya; acc[2] += xb; acc[3] += yb; acc[4] += 1.0;
}
XFUND_HD inline void eight_stage_centroid(Eight& w) {
    w.n = w.red[4];
    w.ca[0] = w.red[0] / w.n; w.ca[1] = w.red[1] / w.n; w.cb[0] = w.red[2] / w.n; w.cb[1] = w.red[3] / w.n;
}
// sum 2: the squared distances to the centroids
XFUND_HD inline void eight_terms2(const Eight& w, double xa, double ya, double xb, double yb, double* acc) {
    const double da0 = xa - w.ca[0], da1 = ya - w.ca[1], db0 = xb - w.cb[0], db1 = yb - w.cb[1];
    acc[0] += da0 * da0 + da1 * da1; acc[1] += db0 * db0 + db1 * db1;
}
XFUND_HD inline void eight_stage_scale(Eight& w) {
    w.sa = 1.4142135623730951 / sqrt(w.red[0] / w.n);
    w.sb = 1.4142135623730951 / sqrt(w.red[1] / w.n);
}
// sum 3: the upper triangle of r r', r the constraint row of the normalised match, row by row (45 entries)
XFUND_HD inline void eight_terms3(const Eight& w, double xa, double ya, double xb, double yb, double* acc) {
    const double pa0 = w.sa * xa + (-w.sa * w.ca[0]), pa1 = w.sa * ya + (-w.sa * w.ca[1]);
    const double pb0 = w.sb * xb + (-w.sb * w.cb[0]), pb1 = w.sb * yb + (-w.sb * w.cb[1]);
    const double r[9] = {pb0 * pa0, pb0 * pa1, pb0, pb1 * pa0, pb1 * pa1, pb1, pa0, pa1, 1.0};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) acc[e++] += r[i] * r[j];
}
// the null vector, the rank-2 projection and the de-normalisation; false when the model is not finite.  One thread.
XFUND_HD inline bool eight_stage_model(Eight& w) {
    int e = 0;
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j) { w.g[9 * i + j] = w.red[e]; w.g[9 * j + i] = w.red[e]; ++e; }
    xpnp::jacobi_eig(w.g, w.v, 9);
    int best = 0;
    for (int i = 1; i < 9; ++i)
        if (w.g[10 * i] < w.g[10 * best]) best = i;
    double a[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) a[i] = w.v[9 * i + best];
    for (int sweep = 0; sweep < kSvdSweeps; ++sweep) {
        bool rotated = false;
#define XFUND_ROT3(p, q)                                                                                                      \
        {                                                                                                                     \
            const double al = a[p] * a[p] + a[3 + p] * a[3 + p] + a[6 + p] * a[6 + p];                                        \
            const double be = a[q] * a[q] + a[3 + q] * a[3 + q] + a[6 + q] * a[6 + q];                                        \
            const double ga = a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];                                        \
            if (fabs(ga) > xpnp::kRotTol * sqrt(al * be)) {                                                                   \
                rotated = true;                                                                                               \
                const double zeta = (be - al) / (2.0 * ga);                                                                   \
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));                                \
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;                                                          \
                for (int r = 0; r < 3; ++r) {                                                                                 \
                    const double ap = a[3 * r + p], aq = a[3 * r + q], vp = v[3 * r + p], vq = v[3 * r + q];                  \
                    a[3 * r + p] = c * ap - s * aq; a[3 * r + q] = s * ap + c * aq;                                           \
                    v[3 * r + p] = c * vp - s * vq; v[3 * r + q] = s * vp + c * vq;                                           \
                }                                                                                                             \
            }                                                                                                                 \
        }
        XFUND_ROT3(0, 1) XFUND_ROT3(0, 2) XFUND_ROT3(1, 2)
#undef XFUND_ROT3
        if (!rotated) break;
    }
    const double n0 = a[0] * a[0] + a[3] * a[3] + a[6] * a[6], n1 = a[1] * a[1] + a[4] * a[4] + a[7] * a[7],
                 n2 = a[2] * a[2] + a[5] * a[5] + a[8] * a[8];
    const int drop = (n0 <= n1 && n0 <= n2) ? 0 : (n1 <= n2 ? 1 : 2);
    const double k0 = drop == 0 ? 0.0 : 1.0, k1 = drop == 1 ? 0.0 : 1.0, k2 = drop == 2 ? 0.0 : 1.0;
    double Fp[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Fp[3 * r + c] = k0 * a[3 * r] * v[3 * c] + k1 * a[3 * r + 1] * v[3 * c + 1] + k2 * a[3 * r + 2] * v[3 * c + 2];
    // T2' Fp T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1]
    const double ta = -w.sa * w.ca[0], tb = -w.sa * w.ca[1], ua = -w.sb * w.cb[0], ub = -w.sb * w.cb[1];
    double G[9];                                            // Fp T1
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = Fp[3 * r] * w.sa; G[3 * r + 1] = Fp[3 * r + 1] * w.sa;
        G[3 * r + 2] = Fp[3 * r] * ta + Fp[3 * r + 1] * tb + Fp[3 * r + 2];
    }
    for (int c = 0; c < 3; ++c) {
        w.F[c] = w.sb * G[c]; w.F[3 + c] = w.sb * G[3 + c];
        w.F[6 + c] = ua * G[c] + ub * G[3 + c] + G[6 + c];
    }
    return xpnp::all_finite(w.F, 9);
}

// the model as it is returned: unit Frobenius norm, the entry of largest magnitude (the first of them) positive
XFUND_HD inline void normalise_model(const double* F, double* out) {
    double nn = 0.0;
    int big = 0;
    for (int e = 0; e < 9; ++e) { nn += F[e] * F[e]; if (fabs(F[e]) > fabs(F[big])) big = e; }
    const double s = (F[big] < 0.0 ? -1.0 : 1.0) / sqrt(nn);
    for (int e = 0; e < 9; ++e) out[e] = F[e] * s;
}

}  // namespace xfund
