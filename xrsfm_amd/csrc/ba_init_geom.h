// The geometry of the two-view initialisation, plain C++ for host and device: the 5-point essential-matrix solver
// (solve_essential_5pt, reference src/geometry/essential.cc:99-218, 292-304), decompose_essential (:221-281, SVD branch),
// check_point (:406-430) and the triangulation angle of CheckInitFramePair (map_initializer.cc:47-49), restated step by step.
// The kernel (ba_init.h) and the sequential host driver of the CPU tests are compiled from this file.
//
// Every dynamically indexed array lives in a workspace WS handed in by the caller: ws(e) is a reference to double number e of
// kWsDoubles.  On the device that is LDS, strided so that the lanes of a wave never share a bank; on the host a plain array.
// Layout (doubles): kB 36 the null-space basis as the four coefficients (x, y, z, 1) of every entry of E (row-major);
// kQ 60: six quadratic polynomials, later the six non-trivial rows of the action matrix; kP 200: the 5x9 epipolar matrix and its
// 9x9 V, then the 10x20 polynomial rows, then the Hessenberg form (100 real + 100 imaginary), then A - lambda I and its null
// vector; kPerm 10: the row permutation, later the real eigenvalues; kTmp 10: a Householder vector.
//
// Steps and caps:
//   null space     one-sided (Hestenes) Jacobi on the columns of the 5x9 matrix A(i, 3 j + k) = p1h[j] p2h[k], at most kNullSweeps
//                  cyclic sweeps; the basis is the four columns of V whose images are shortest.  The solutions do not depend on
//                  the choice of basis.  vec -> E as the reference's to_matrix: E(k, j) = vec[3 j + k].
//   polynomials    the nine entries of E E' E - 0.5 tr(E E') E and det E in the monomial order
//                  XXX XXY XYY YYY XXZ XYZ YYZ XZZ YZZ ZZZ XX XY YY XZ YZ ZZ X Y Z I (GRevLex, as the reference)
//   elimination    the reference's Gauss-Jordan literally: row permutation instead of row swaps, the pivot search by
//                  successive `<` swaps, the `== 0` skip, every operation on all 20 columns
//   action matrix  rows 0..5 = -rows perm[XXX, XXY, XYY, XXZ, XYZ, XZZ], columns XX..I; rows 6..9 = unit(XX, XY, XZ, X)
//   eigenvalues    Householder reduction to Hessenberg form, then the complex single-shift QR iteration (Wilkinson shift,
//                  exceptional shifts at iterations 10 and 20) with deflation from the bottom, at most kQrItersPerValue
//                  iterations per eigenvalue; a matrix that does not converge gives no model.  A solution is taken when
//                  |Im lambda| < 1e-10; the models of a trial are in ascending Re lambda (the model-order deviation).
//   eigenvector    null vector of A - lambda I: Gaussian elimination with partial pivoting over columns 0..8, h[I] = 1, back
//                  substitution; (x, y, z) = h[X, Y, Z] / h[I]; E = basis (x, y, z, 1).  A non-finite E is dropped.
//
// Deviation (decomposition).  Eigen's JacobiSVD signs and orders the singular vectors as it likes; the reference then flips U
// and V' to determinant +1.  Here the SVD is a one-sided Jacobi on the 3x3 (kSvd3Sweeps), the column with the shortest image is
// dropped, (u1, u2) and (v1, v2) are the remaining two, u3 = u1 x u2 and v3 = v1 x v2.  Both determinants are then +1, the
// reference's flips are no-ops and nothing depends on how a library signs a null vector.  R1 = U W V', R2 = U W' V', T = u3;
// candidates (R1, +T), (R1, -T), (R2, +T), (R2, -T).  Rotating (u1, u2) and (v1, v2) in their plane changes nothing.  Which of the
// twisted pair is called R1 and which way T points is fixed by two sign conventions (essential_sign, kOrient below), so that the
// candidate index is a function of the model and not of the iteration.
//
// The null-space basis is made canonical (the projections of e0..e3 onto the null space, orthonormalised in that order): the
// eigenvalue of a solution is its x coordinate in the basis, so "ascending eigenvalue" needs a basis that is a function of the
// five matches and not of the Jacobi iteration.
//
// check_point: the 4x4 DLT null vector by one-sided Jacobi (kDltSweeps; the routine of ba_tri.h without its wave vote), the depth
// tests q1z q3 > 0, q2z q3 > 0, both depths < max_depth, all invariant to the sign of q; p = q.hnormalized().
#pragma once
#include "ba_init_scan.h"
#include "ba_pnp_geom.h"

#ifdef __HIPCC__
#define XINIT_UNROLL _Pragma("unroll")
#define XINIT_UNROLL1 _Pragma("unroll 1")
#else
#define XINIT_UNROLL
#define XINIT_UNROLL1
#endif

namespace xinit {

constexpr int kB = 0, kQ = 36, kP = 96, kPerm = 296, kTmp = 306, kWsDoubles = 316;
constexpr int kNullSweeps = 30;
constexpr int kSvd3Sweeps = 20;
constexpr int kDltSweeps = 12;
constexpr int kQrItersPerValue = 30;
constexpr double kRotTol = 1e-15;             // two columns count as orthogonal below this cosine
constexpr double kMaxImag = 1e-10;

XINIT_HD inline bool finite9(const double* p) {
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && (fabs(p[i]) <= DBL_MAX);
    return ok;
}

// a workspace over a plain array (host drivers)
struct PlainWs {
    double* p;
    XINIT_HD double& operator()(int e) const { return p[e]; }
};

// product of two linear polynomials (x, y, z, 1) -> quadratic (XX XY YY XZ YZ ZZ X Y Z I), added with sign sg to ws(o ..)
template <class WS>
XINIT_HD inline void lin_lin(const WS& ws, int a, int b, int o, double sg) {
    const double a0 = ws(a), a1 = ws(a + 1), a2 = ws(a + 2), a3 = ws(a + 3), b0 = sg * ws(b), b1 = sg * ws(b + 1), b2 = sg * ws(b + 2), b3 = sg * ws(b + 3);
    ws(o) += a0 * b0; ws(o + 1) += a0 * b1 + a1 * b0; ws(o + 2) += a1 * b1; ws(o + 3) += a0 * b2 + a2 * b0; ws(o + 4) += a1 * b2 + a2 * b1;
    ws(o + 5) += a2 * b2; ws(o + 6) += a0 * b3 + a3 * b0; ws(o + 7) += a1 * b3 + a3 * b1; ws(o + 8) += a2 * b3 + a3 * b2; ws(o + 9) += a3 * b3;
}

// quadratic times linear, added to the cubic ws(o ..) (20 coefficients)
#define XINIT_QL(F) F(0, 0, 0) F(0, 1, 1) F(0, 2, 4) F(0, 3, 10) F(1, 0, 1) F(1, 1, 2) F(1, 2, 5) F(1, 3, 11) F(2, 0, 2) F(2, 1, 3) F(2, 2, 6) F(2, 3, 12) \
    F(3, 0, 4) F(3, 1, 5) F(3, 2, 7) F(3, 3, 13) F(4, 0, 5) F(4, 1, 6) F(4, 2, 8) F(4, 3, 14) F(5, 0, 7) F(5, 1, 8) F(5, 2, 9) F(5, 3, 15)                 \
    F(6, 0, 10) F(6, 1, 11) F(6, 2, 13) F(6, 3, 16) F(7, 0, 11) F(7, 1, 12) F(7, 2, 14) F(7, 3, 17) F(8, 0, 13) F(8, 1, 14) F(8, 2, 15) F(8, 3, 18)         \
    F(9, 0, 16) F(9, 1, 17) F(9, 2, 18) F(9, 3, 19)
template <class WS>
XINIT_HD inline void quad_lin(const WS& ws, int q, int l, int o, double sg) {
    const double l0 = sg * ws(l), l1 = sg * ws(l + 1), l2 = sg * ws(l + 2), l3 = sg * ws(l + 3);
#define XINIT_F(qi, li, ti) ws(o + ti) += ws(q + qi) * l##li;
    XINIT_QL(XINIT_F)
#undef XINIT_F
}

// the null-space basis of the five matches pts[5][4] = {x1, y1, x2, y2} into ws(kB ..)
template <class WS>
XINIT_HD inline void null_basis(const WS& ws, const double* pts) {
    const int A = kP, V = kP + 45;                       // A 5x9 and V 9x9, row-major
    XINIT_UNROLL
    for (int i = 0; i < 5; ++i) {
        const double p1[3] = {pts[4 * i], pts[4 * i + 1], 1.0}, p2[3] = {pts[4 * i + 2], pts[4 * i + 3], 1.0};
        XINIT_UNROLL
        for (int j = 0; j < 3; ++j) {
            XINIT_UNROLL
            for (int k = 0; k < 3; ++k) ws(A + 9 * i + 3 * j + k) = p1[j] * p2[k];
        }
    }
    for (int i = 0; i < 81; ++i) ws(V + i) = (i % 10 == 0) ? 1.0 : 0.0;
    double tr = 0.0;
    for (int i = 0; i < 45; ++i) tr += ws(A + i) * ws(A + i);
    const double floor_abs = 0x1p-60 * tr;               // columns of the null space have no direction worth a rotation
    for (int sweep = 0; sweep < kNullSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 5; ++r) {
                    const double ap = ws(A + 9 * r + p), aq = ws(A + 9 * r + q);
                    al += ap * ap; be += aq * aq; ga += ap * aq;
                }
                if (fabs(ga) > kRotTol * sqrt(al * be) && fabs(ga) > floor_abs) {
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                    for (int r = 0; r < 5; ++r) {
                        const double ap = ws(A + 9 * r + p), aq = ws(A + 9 * r + q);
                        ws(A + 9 * r + p) = c * ap - s * aq; ws(A + 9 * r + q) = s * ap + c * aq;
                    }
                    for (int r = 0; r < 9; ++r) {
                        const double vp = ws(V + 9 * r + p), vq = ws(V + 9 * r + q);
                        ws(V + 9 * r + p) = c * vp - s * vq; ws(V + 9 * r + q) = s * vp + c * vq;
                    }
                }
            }
        if (!rotated) break;
    }
    int pick[4];
    unsigned used = 0;
    XINIT_UNROLL
    for (int b = 0; b < 4; ++b) {                        // the four shortest images, shortest first
        int pk = -1;
        double best = 0.0;
        for (int c = 0; c < 9; ++c) {
            if ((used >> c) & 1u) continue;
            double nn = 0.0;
            for (int r = 0; r < 5; ++r) nn += ws(A + 9 * r + c) * ws(A + 9 * r + c);
            if (pk < 0 || nn < best) { pk = c; best = nn; }
        }
        used |= 1u << pk;
        pick[b] = pk;
    }
    // the canonical basis of that null space: the projections of the unit vectors e0..e3 onto it, orthonormalised in that order
    const int W = kP;                                    // W 4x9, row-major (A is no longer needed)
    XINIT_UNROLL
    for (int k = 0; k < 4; ++k)
        for (int r = 0; r < 9; ++r) {
            double w = 0.0;
            XINIT_UNROLL
            for (int b = 0; b < 4; ++b) w += ws(V + 9 * r + pick[b]) * ws(V + 9 * k + pick[b]);
            ws(W + 9 * k + r) = w;
        }
    for (int k = 0; k < 4; ++k) {
        for (int j = 0; j < k; ++j) {
            double d = 0.0;
            for (int r = 0; r < 9; ++r) d += ws(W + 9 * j + r) * ws(W + 9 * k + r);
            for (int r = 0; r < 9; ++r) ws(W + 9 * k + r) -= d * ws(W + 9 * j + r);
        }
        double nn = 0.0;
        for (int r = 0; r < 9; ++r) nn += ws(W + 9 * k + r) * ws(W + 9 * k + r);
        const double inv = 1.0 / sqrt(nn);
        for (int r = 0; r < 9; ++r) ws(W + 9 * k + r) *= inv;
    }
    for (int b = 0; b < 4; ++b)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) ws(kB + 4 * (3 * i + j) + b) = ws(W + 9 * b + 3 * j + i);          // E(i, j) = vec[3 j + i]
}

// the ten cubic constraints into ws(kP ..), rows of 20
template <class WS>
XINIT_HD inline void build_polynomials(const WS& ws) {
    for (int i = 0; i < 200; ++i) ws(kP + i) = 0.0;
    auto e = [](int i, int j) { return kB + 4 * (3 * i + j); };
    // det E: the three minors of row 0 as quadratics in ws(kQ ..)
    for (int i = 0; i < 30; ++i) ws(kQ + i) = 0.0;
    lin_lin(ws, e(1, 1), e(2, 2), kQ, 1.0);       lin_lin(ws, e(1, 2), e(2, 1), kQ, -1.0);
    lin_lin(ws, e(1, 2), e(2, 0), kQ + 10, 1.0);  lin_lin(ws, e(1, 0), e(2, 2), kQ + 10, -1.0);
    lin_lin(ws, e(1, 0), e(2, 1), kQ + 20, 1.0);  lin_lin(ws, e(1, 1), e(2, 0), kQ + 20, -1.0);
    for (int j = 0; j < 3; ++j) quad_lin(ws, kQ + 10 * j, e(0, j), kP + 180, 1.0);
    // Q = E E' - 0.5 tr(E E') I (symmetric: 00 01 02 11 12 22), then Q E
    for (int i = 0; i < 60; ++i) ws(kQ + i) = 0.0;
    int o = kQ;
    for (int i = 0; i < 3; ++i)
        for (int k = i; k < 3; ++k, o += 10)
            for (int j = 0; j < 3; ++j) lin_lin(ws, e(i, j), e(k, j), o, 1.0);
    for (int m = 0; m < 10; ++m) {
        const double h = 0.5 * (ws(kQ + m) + ws(kQ + 30 + m) + ws(kQ + 50 + m));
        ws(kQ + m) -= h; ws(kQ + 30 + m) -= h; ws(kQ + 50 + m) -= h;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) {
                const int lo = i < k ? i : k, hi = i < k ? k : i;
                const int sym = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
                quad_lin(ws, kQ + 10 * sym, e(k, j), kP + 20 * (3 * i + j), 1.0);
            }
}

// generate_action_matrix: the elimination on ws(kP ..); the six non-trivial rows of the action matrix go to ws(kQ ..)
template <class WS>
XINIT_HD inline void action_matrix(const WS& ws) {
    auto perm = [&](int i) { return (int)ws(kPerm + i); };
    auto P = [&](int r, int c) -> double& { return ws(kP + 20 * r + c); };
    for (int i = 0; i < 10; ++i) ws(kPerm + i) = (double)i;
    for (int i = 0; i < 10; ++i) {
        for (int j = i + 1; j < 10; ++j)
            if (fabs(P(perm(i), i)) < fabs(P(perm(j), i))) { const double tmp = ws(kPerm + i); ws(kPerm + i) = ws(kPerm + j); ws(kPerm + j) = tmp; }
        const int pi = perm(i);
        const double piv = P(pi, i);
        if (piv == 0.0) continue;
        for (int c = 0; c < 20; ++c) P(pi, c) /= piv;
        for (int j = i + 1; j < 10; ++j) {
            const int pj = perm(j);
            const double f = P(pj, i);
            for (int c = 0; c < 20; ++c) P(pj, c) -= P(pi, c) * f;
        }
    }
    for (int i = 9; i > 0; --i) {
        const int pi = perm(i);
        for (int j = 0; j < i; ++j) {
            const int pj = perm(j);
            const double f = P(pj, i);
            for (int c = 0; c < 20; ++c) P(pj, c) -= P(pi, c) * f;
        }
    }
    const int src[6] = {0, 1, 2, 4, 5, 7};               // XXX XXY XYY XXZ XYZ XZZ
XINIT_UNROLL
    for (int r = 0; r < 6; ++r) {
        const int pr = perm(src[r]);
        for (int c = 0; c < 10; ++c) ws(kQ + 10 * r + c) = -P(pr, 10 + c);
    }
}

// entry (r, c) of the action matrix
template <class WS>
XINIT_HD inline double action_at(const WS& ws, int r, int c) {
    if (r < 6) return ws(kQ + 10 * r + c);
    const int one = r == 6 ? 0 : (r == 7 ? 1 : (r == 8 ? 3 : 6));
    return c == one ? 1.0 : 0.0;
}

struct Cx { double r, i; };
XINIT_HD inline Cx cx(double r, double i) { Cx z; z.r = r; z.i = i; return z; }
XINIT_HD inline Cx operator+(Cx a, Cx b) { return cx(a.r + b.r, a.i + b.i); }
XINIT_HD inline Cx operator-(Cx a, Cx b) { return cx(a.r - b.r, a.i - b.i); }
XINIT_HD inline Cx operator*(Cx a, Cx b) { return cx(a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r); }
XINIT_HD inline Cx conj(Cx a) { return cx(a.r, -a.i); }
XINIT_HD inline Cx scale(Cx a, double s) { return cx(a.r * s, a.i * s); }
XINIT_HD inline double abs2(Cx a) { return a.r * a.r + a.i * a.i; }
XINIT_HD inline double abs1(Cx a) { return fabs(a.r) + fabs(a.i); }
XINIT_HD inline Cx cdiv(Cx a, Cx b) { const double d = abs2(b); return cx((a.r * b.r + a.i * b.i) / d, (a.i * b.r - a.r * b.i) / d); }
XINIT_HD inline Cx csqrt(Cx z) {
    const double m = sqrt(abs2(z)), re = sqrt(0.5 * (m + fabs(z.r)));
    if (re == 0.0) return cx(0.0, 0.0);
    const double im = z.i / (2.0 * re);
    return z.r >= 0.0 ? cx(re, im) : cx(fabs(im), copysign(re, z.i));
}

// eigenvalues of the action matrix: the real ones (|Im| < kMaxImag) in ascending order into ws(kPerm ..); returns their number,
// 0 when the iteration does not converge within its cap
template <class WS>
XINIT_HD inline int real_eigenvalues(const WS& ws) {
    const int n = 10, HR = kP, HI = kP + 100;
    auto Hr = [&](int r, int c) -> double& { return ws(HR + 10 * r + c); };
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) { Hr(r, c) = action_at(ws, r, c); ws(HI + 10 * r + c) = 0.0; }
    // Householder reduction: column k below the subdiagonal
    for (int k = 0; k < n - 2; ++k) {
        double nn = 0.0;
        for (int r = k + 1; r < n; ++r) nn += Hr(r, k) * Hr(r, k);
        const double x0 = Hr(k + 1, k), alpha = x0 > 0.0 ? -sqrt(nn) : sqrt(nn);
        double vv = 0.0;
        for (int r = k + 1; r < n; ++r) { const double v = Hr(r, k) - (r == k + 1 ? alpha : 0.0); ws(kTmp + r) = v; vv += v * v; }
        if (vv == 0.0) continue;
        const double beta = 2.0 / vv;
        for (int c = 0; c < n; ++c) {                    // (I - beta v v') H
            double d = 0.0;
            for (int r = k + 1; r < n; ++r) d += ws(kTmp + r) * Hr(r, c);
            d *= beta;
            for (int r = k + 1; r < n; ++r) Hr(r, c) -= d * ws(kTmp + r);
        }
        for (int r = 0; r < n; ++r) {                    // H (I - beta v v')
            double d = 0.0;
            for (int c = k + 1; c < n; ++c) d += Hr(r, c) * ws(kTmp + c);
            d *= beta;
            for (int c = k + 1; c < n; ++c) Hr(r, c) -= d * ws(kTmp + c);
        }
        for (int r = k + 2; r < n; ++r) Hr(r, k) = 0.0;
    }
    auto get = [&](int r, int c) { return cx(ws(HR + 10 * r + c), ws(HI + 10 * r + c)); };
    auto put = [&](int r, int c, Cx z) { ws(HR + 10 * r + c) = z.r; ws(HI + 10 * r + c) = z.i; };
    double hnorm = 0.0;
    for (int i = 0; i < 100; ++i) hnorm += fabs(ws(HR + i));
    int hi = n - 1, its = 0;
    while (hi >= 0) {
        int lo = hi;
        for (; lo > 0; --lo) {
            double s = abs1(get(lo - 1, lo - 1)) + abs1(get(lo, lo));
            if (s == 0.0) s = hnorm;
            if (abs1(get(lo, lo - 1)) <= DBL_EPSILON * s) { put(lo, lo - 1, cx(0.0, 0.0)); break; }
        }
        if (lo == hi) { --hi; its = 0; continue; }
        if (its >= kQrItersPerValue) return 0;
        ++its;
        const Cx a = get(hi - 1, hi - 1), b = get(hi - 1, hi), c = get(hi, hi - 1), d = get(hi, hi);
        Cx mu;
        if (its == 10 || its == 20) mu = cx(d.r + abs1(c), d.i);
        else {
            const Cx h = scale(a - d, 0.5), bc = b * c, sq = csqrt(h * h + bc);
            const Cx dp = h + sq, dm = h - sq, den = abs2(dp) >= abs2(dm) ? dp : dm;
            mu = abs2(den) == 0.0 ? d : d - cdiv(bc, den);
        }
        for (int k = lo; k <= hi; ++k) put(k, k, get(k, k) - mu);
        double pc = 1.0;
        Cx ps = cx(0.0, 0.0);
        for (int k = lo; k < hi; ++k) {
            const Cx x = get(k, k), y = get(k + 1, k);
            double c1 = 1.0;
            Cx s1 = cx(0.0, 0.0);
            if (abs2(y) != 0.0) {
                const double ax = sqrt(abs2(x)), nrm = sqrt(abs2(x) + abs2(y));
                if (ax == 0.0) { c1 = 0.0; s1 = scale(conj(y), 1.0 / sqrt(abs2(y))); }
                else { c1 = ax / nrm; s1 = scale(scale(x, 1.0 / ax) * conj(y), 1.0 / nrm); }
            }
            for (int j = k; j <= hi; ++j) {              // rows k, k + 1
                const Cx u = get(k, j), v = get(k + 1, j);
                put(k, j, scale(u, c1) + s1 * v); put(k + 1, j, scale(v, c1) - conj(s1) * u);
            }
            put(k + 1, k, cx(0.0, 0.0));
            if (k > lo)
                for (int r = lo; r <= k; ++r) {          // the previous rotation from the right: columns k - 1, k
                    const Cx u = get(r, k - 1), v = get(r, k);
                    put(r, k - 1, scale(u, pc) + v * conj(ps)); put(r, k, scale(v, pc) - u * ps);
                }
            pc = c1; ps = s1;
        }
        for (int r = lo; r <= hi; ++r) {
            const Cx u = get(r, hi - 1), v = get(r, hi);
            put(r, hi - 1, scale(u, pc) + v * conj(ps)); put(r, hi, scale(v, pc) - u * ps);
        }
        for (int k = lo; k <= hi; ++k) put(k, k, get(k, k) + mu);
    }
    int m = 0;
    for (int k = 0; k < n; ++k) {
        const Cx z = get(k, k);
        if (!(fabs(z.i) < kMaxImag) || !(fabs(z.r) <= DBL_MAX)) continue;
        int p = m++;
        for (; p > 0 && ws(kPerm + p - 1) > z.r; --p) ws(kPerm + p) = ws(kPerm + p - 1);
        ws(kPerm + p) = z.r;
    }
    return m;
}

// the model of the real eigenvalue lam: E (row-major) from the null vector of A - lam I; false when it is not finite
template <class WS>
XINIT_HD inline bool model_of(const WS& ws, double lam, double* E) {
    const int n = 10, M = kP, H = kP + 100;
    auto A = [&](int r, int c) -> double& { return ws(M + 10 * r + c); };
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) A(r, c) = action_at(ws, r, c) - (r == c ? lam : 0.0);
    for (int k = 0; k < n - 1; ++k) {
        int p = k;
        for (int r = k + 1; r < n; ++r)
            if (fabs(A(r, k)) > fabs(A(p, k))) p = r;
        if (p != k)
            for (int c = k; c < n; ++c) { const double tmp = A(k, c); A(k, c) = A(p, c); A(p, c) = tmp; }
        const double piv = A(k, k);
        for (int r = k + 1; r < n; ++r) {
            const double f = A(r, k) / piv;
            for (int c = k; c < n; ++c) A(r, c) -= f * A(k, c);
        }
    }
    ws(H + 9) = 1.0;
    for (int r = n - 2; r >= 0; --r) {
        double s = 0.0;
        for (int c = r + 1; c < n; ++c) s += A(r, c) * ws(H + c);
        ws(H + r) = -s / A(r, r);
    }
    const double w = ws(H + 9), x = ws(H + 6) / w, y = ws(H + 7) / w, z = ws(H + 8) / w;
XINIT_UNROLL
    for (int e = 0; e < 9; ++e) E[e] = ws(kB + 4 * e) * x + ws(kB + 4 * e + 1) * y + ws(kB + 4 * e + 2) * z + ws(kB + 4 * e + 3);
    return finite9(E);
}

// solve_essential_5pt for pts[5][4] = {x1, y1, x2, y2}: up to kMaxModels models in ascending eigenvalue, models[9 * slot + e]
// row-major; returns their number
template <class WS>
XINIT_HD inline int five_point_models(const WS& ws, const double* pts, double* models) {
    null_basis(ws, pts);
    build_polynomials(ws);
    action_matrix(ws);
    const int m = real_eigenvalues(ws);
    int nm = 0;
    for (int k = 0; k < m; ++k) {
        double E[9];
        if (!model_of(ws, ws(kPerm + k), E)) continue;
XINIT_UNROLL
        for (int e = 0; e < 9; ++e) models[9 * nm + e] = E[e];
        ++nm;
    }
    return nm;
}

XINIT_HD inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// the two sign conventions of the decomposition: E and -E are the same model, and so are the two orientations of the singular
// pair; which of the twisted pair is called R1 and which way T points depend on both.  E is taken with a positive product with a
// fixed generic matrix, the pair so that v3 has a positive product with a fixed generic vector: both choices are continuous in E
// except on a set of measure zero, and neither depends on how the SVD iteration happens to end.
constexpr double kSignE[9] = {0.31, -0.17, 0.23, 0.41, 0.13, -0.29, 0.19, 0.37, 0.11};
constexpr double kOrient[3] = {0.6, 0.48, 0.64};
XINIT_HD inline double essential_sign(const double* E) {
    const double d = E[0] * kSignE[0] + E[1] * kSignE[1] + E[2] * kSignE[2] + E[3] * kSignE[3] + E[4] * kSignE[4] + E[5] * kSignE[5] +
                     E[6] * kSignE[6] + E[7] * kSignE[7] + E[8] * kSignE[8];
    return d < 0.0 ? -1.0 : 1.0;
}

// decompose_essential (see the deviation above): R1, R2 row-major, T
XINIT_HD inline void decompose_essential(const double* E, double* R1, double* R2, double* T) {
    double a[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    const double sgE = essential_sign(E);
    for (int i = 0; i < 9; ++i) a[i] = sgE * E[i];
    for (int sweep = 0; sweep < kSvd3Sweeps; ++sweep) {
        bool rotated = false;
#define XINIT_ROT3(p, q)                                                                                                      \
        {                                                                                                                     \
            const double al = a[p] * a[p] + a[3 + p] * a[3 + p] + a[6 + p] * a[6 + p];                                        \
            const double be = a[q] * a[q] + a[3 + q] * a[3 + q] + a[6 + q] * a[6 + q];                                        \
            const double ga = a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];                                        \
            if (fabs(ga) > kRotTol * sqrt(al * be)) {                                                                         \
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
        XINIT_ROT3(0, 1) XINIT_ROT3(0, 2) XINIT_ROT3(1, 2)
#undef XINIT_ROT3
        if (!rotated) break;
    }
    const double n0 = a[0] * a[0] + a[3] * a[3] + a[6] * a[6], n1 = a[1] * a[1] + a[4] * a[4] + a[7] * a[7],
                 n2 = a[2] * a[2] + a[5] * a[5] + a[8] * a[8];
    const int drop = (n0 <= n1 && n0 <= n2) ? 0 : (n1 <= n2 ? 1 : 2);
    const double i1 = 1.0 / sqrt(drop == 0 ? n1 : n0), i2 = 1.0 / sqrt(drop == 2 ? n1 : n2);
    double u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
    for (int r = 0; r < 3; ++r) {
        u1[r] = (drop == 0 ? a[3 * r + 1] : a[3 * r]) * i1; u2[r] = (drop == 2 ? a[3 * r + 1] : a[3 * r + 2]) * i2;
        v1[r] = drop == 0 ? v[3 * r + 1] : v[3 * r];        v2[r] = drop == 2 ? v[3 * r + 1] : v[3 * r + 2];
    }
    cross3(u1, u2, u3); cross3(v1, v2, v3);
    // the orientation of the pair: v3 on the positive side of kOrient (swapping the pair negates u3, v3 and the twist)
    const double o = (v3[0] * kOrient[0] + v3[1] * kOrient[1] + v3[2] * kOrient[2]) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) { u3[r] *= o; v3[r] *= o; }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            const double tw = o * (u1[r] * v2[c] - u2[r] * v1[c]), ax = u3[r] * v3[c];
            R1[3 * r + c] = tw + ax; R2[3 * r + c] = ax - tw;
        }
        T[r] = u3[r];
    }
}

// null vector of a 4x4 (row-major) by one-sided Jacobi; constant indices only
XINIT_HD inline void null4(double a[16], double x[4]) {
    double v[16];
XINIT_UNROLL
    for (int i = 0; i < 16; ++i) v[i] = (i % 5 == 0) ? 1.0 : 0.0;
XINIT_UNROLL1
    for (int sweep = 0; sweep < kDltSweeps; ++sweep) {
        bool rotated = false;
XINIT_UNROLL
        for (int p = 0; p < 3; ++p) {
XINIT_UNROLL
            for (int q = p + 1; q < 4; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
XINIT_UNROLL
                for (int r = 0; r < 4; ++r) { al += a[4 * r + p] * a[4 * r + p]; be += a[4 * r + q] * a[4 * r + q]; ga += a[4 * r + p] * a[4 * r + q]; }
                if (fabs(ga) > kRotTol * sqrt(al * be)) {
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
XINIT_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        const double ap = a[4 * r + p], aq = a[4 * r + q], vp = v[4 * r + p], vq = v[4 * r + q];
                        a[4 * r + p] = c * ap - s * aq; a[4 * r + q] = s * ap + c * aq;
                        v[4 * r + p] = c * vp - s * vq; v[4 * r + q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double best = 0.0;
XINIT_UNROLL
    for (int c = 0; c < 4; ++c) {
        const double nn = a[c] * a[c] + a[4 + c] * a[4 + c] + a[8 + c] * a[8 + c] + a[12 + c] * a[12 + c];
        if (c == 0 || nn < best) {
            best = nn;
            x[0] = v[c]; x[1] = v[4 + c]; x[2] = v[8 + c]; x[3] = v[12 + c];
        }
    }
}

// check_point with P1 = [I | 0], P2 = [R | T]
XINIT_HD inline bool check_point(const double* R, const double* T, double x1, double y1, double x2, double y2, double max_depth, double* p) {
    double a[16] = {-1.0, 0.0, x1, 0.0, 0.0, -1.0, y1, 0.0,
                    x2 * R[6] - R[0], x2 * R[7] - R[1], x2 * R[8] - R[2], x2 * T[2] - T[0],
                    y2 * R[6] - R[3], y2 * R[7] - R[4], y2 * R[8] - R[5], y2 * T[2] - T[1]};
    double q[4];
    null4(a, q);
    const double q1z = q[2], q2z = R[6] * q[0] + R[7] * q[1] + R[8] * q[2] + T[2] * q[3];
    if (q1z * q[3] > 0.0 && q2z * q[3] > 0.0 && q1z / q[3] < max_depth && q2z / q[3] < max_depth) {
        p[0] = q[0] / q[3]; p[1] = q[1] / q[3]; p[2] = q[2] / q[3];
        return fabs(p[0]) <= DBL_MAX && fabs(p[1]) <= DBL_MAX && fabs(p[2]) <= DBL_MAX;
    }
    return false;
}

// colmap::CalculateTriangulationAngle (base/triangulation.cc:124-147; the routine of ba_filter.h for host and device)
XINIT_HD inline double tri_angle(const double* c1, const double* c2, const double* P) {
    double b2 = 0, r1 = 0, r2 = 0;
    for (int k = 0; k < 3; ++k) {
        const double b = c1[k] - c2[k], a1 = P[k] - c1[k], a2 = P[k] - c2[k];
        b2 += b * b; r1 += a1 * a1; r2 += a2 * a2;
    }
    const double den = 2.0 * sqrt(r1 * r2);
    if (den == 0.0) return 0.0;
    const double ang = fabs(acos((r1 + r2 - b2) / den));
    return fmin(ang, 3.14159265358979323846 - ang);
}

// candidate k of decompose_rt: Rs = {R1, R1, R2, R2}, Ts = {T, -T, T, -T}; also the second projection centre -R' t
XINIT_HD inline void candidate(const double* R1, const double* R2, const double* T, int k, double* R, double* t, double* centre) {
    for (int i = 0; i < 9; ++i) R[i] = k < 2 ? R1[i] : R2[i];
    for (int i = 0; i < 3; ++i) t[i] = (k & 1) ? -T[i] : T[i];
    for (int i = 0; i < 3; ++i) centre[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
}

// the acceptance test of CheckInitFramePair (map_initializer.cc:58-59)
XINIT_HD inline bool accept(int n, int num_p3d, int num_valid, double min_front_ratio, double min_angle_ratio, int min_num_valid) {
    return (double)num_p3d >= min_front_ratio * (double)n && (double)num_valid >= min_angle_ratio * (double)num_p3d && num_valid > min_num_valid;
}

// the unit quaternion (x, y, z, w), w >= 0, of a row-major 3x3 rotation (the four-branch rule of xpnp::quat_from_pose)
XINIT_HD inline void quat_of(const double* R, double q[4]) {
    const double P[12] = {R[0], R[1], R[2], 0.0, R[3], R[4], R[5], 0.0, R[6], R[7], R[8], 0.0};
    xpnp::quat_from_pose(P, q);
}

}  // namespace xinit
