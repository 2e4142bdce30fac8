// The geometry of the absolute-pose LO-RANSAC, plain C++ for host and device: the squared reprojection error, the P3P sample
// models (reference src/geometry/colmap/estimators/absolute_pose.cc:49-179) and the EPnP local model (:210-619), the latter cut
// into scalar stages between sums over the inliers, so that the kernel (ba_pnp.h) can form every sum with the whole workgroup and a
// host driver can form it sequentially.  Nothing here allocates or keeps a dynamically indexed local array: workspaces are handed
// in (LDS on the device).
//
// Deviation 2, root order and acceptance.  The quartic's four roots are computed as complex numbers by Aberth-Ehrlich iteration on
// the monic polynomial from fixed starting points, with a cap of kRootIters sweeps.  A root is taken when |Im| <= 1e-10 and
// Re >= 0; the models of one trial are offered in ascending Re (the reference's order is that of its eigenvalue routine).  A
// vanishing leading coefficient or a non-finite coefficient gives no model.  The rigid fit of the three points is Umeyama without
// scale, the sign taken from det(U) det(V): with u3 = u1 x u2 and v3 = v1 x v2 both determinants are +1 and
// R = u1 v1' + u2 v2' + u3 v3'.  (det(Sigma) must never decide the sign: Sigma has rank 2 for three points.)
//
// Deviation 3, EPnP's sign step.  SolveForSign (:548-557) negates whenever the first depth is non-zero, so its result depends on
// the sign the SVD routine gives the null vectors.  Here the control points are negated iff the first inlier's depth is negative
// (Lepetit, Moreno-Noguer & Fua 2009).
#pragma once
#include "ba_pnp_scan.h"

namespace xpnp {

constexpr int kRootIters = 100;               // Aberth sweeps
constexpr double kRootTol = 0x1p-50;          // a root has converged when its update is below this fraction of its modulus
constexpr double kRootMaxImag = 1e-10;
constexpr int kSvd3Sweeps = 20;
constexpr int kEigSweeps = 30;
constexpr int kLsSweeps = 30;
constexpr double kRotTol = 1e-15;             // two columns count as orthogonal below this cosine

XPNP_HD inline bool all_finite(const double* p, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && (fabs(p[i]) <= DBL_MAX);              // (false for NaN and Inf)
    return ok;
}

// ComputeSquaredReprojectionError (estimators/utils.cc:157-181) for one correspondence; P row-major 3x4
XPNP_HD inline double residual(const double* P, const double* X, double x, double y) {
    const double pz = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    if (pz > DBL_EPSILON) {
        const double px = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
        const double py = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
        const double inv = 1.0 / pz;
        const double dx = x - px * inv, dy = y - py * inv;
        return dx * dx + dy * dy;
    }
    return DBL_MAX;
}

// The proper rotation R = U V' of the 3x3 (row-major) a = U S V' by one-sided Jacobi; a is destroyed.  The column with the
// shortest image is dropped and replaced by the cross products (see deviation 2).  Constant indices only.
XPNP_HD inline void rotation_from_cov(double a[9], double R[9]) {
    double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < kSvd3Sweeps; ++sweep) {
        bool rotated = false;
#define XPNP_ROT3(p, q)                                                                                                       \
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
        XPNP_ROT3(0, 1) XPNP_ROT3(0, 2) XPNP_ROT3(1, 2)
#undef XPNP_ROT3
        if (!rotated) break;
    }
    const double n0 = a[0] * a[0] + a[3] * a[3] + a[6] * a[6], n1 = a[1] * a[1] + a[4] * a[4] + a[7] * a[7],
                 n2 = a[2] * a[2] + a[5] * a[5] + a[8] * a[8];
    const int drop = (n0 <= n1 && n0 <= n2) ? 0 : (n1 <= n2 ? 1 : 2);
    const double i1 = 1.0 / sqrt(drop == 0 ? n1 : n0), i2 = 1.0 / sqrt(drop == 2 ? n1 : n2);
    double u1[3], u2[3], v1[3], v2[3];
    for (int r = 0; r < 3; ++r) {
        u1[r] = (drop == 0 ? a[3 * r + 1] : a[3 * r]) * i1; u2[r] = (drop == 2 ? a[3 * r + 1] : a[3 * r + 2]) * i2;
        v1[r] = drop == 0 ? v[3 * r + 1] : v[3 * r];        v2[r] = drop == 2 ? v[3 * r + 1] : v[3 * r + 2];
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
}

// P3PEstimator::Estimate for the sample {xy[k], X[k]}, k = 0..2: up to four models (3x4, row-major, 12 doubles each) written to
// out in ascending order of the root; returns their number.  Non-finite models are dropped.
XPNP_HD inline int p3p_models(const double* xy, const double* Xw, double* out) {
    double lift[9];
    for (int k = 0; k < 3; ++k) {
        const double inv = 1.0 / sqrt(xy[2 * k] * xy[2 * k] + xy[2 * k + 1] * xy[2 * k + 1] + 1.0);
        lift[3 * k] = xy[2 * k] * inv; lift[3 * k + 1] = xy[2 * k + 1] * inv; lift[3 * k + 2] = inv;
    }
    const double* u = lift; const double* v = lift + 3; const double* w = lift + 6;
    const double cos_uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2], cos_uw = u[0] * w[0] + u[1] * w[1] + u[2] * w[2],
                 cos_vw = v[0] * w[0] + v[1] * w[1] + v[2] * w[2];
    double dAB2 = 0.0, dAC2 = 0.0, dBC2 = 0.0;
    for (int r = 0; r < 3; ++r) {
        const double ab = Xw[r] - Xw[3 + r], ac = Xw[r] - Xw[6 + r], bc = Xw[3 + r] - Xw[6 + r];
        dAB2 += ab * ab; dAC2 += ac * ac; dBC2 += bc * bc;
    }
    const double dAB = sqrt(dAB2), a = dBC2 / dAB2, b = dAC2 / dAB2;
    const double a2 = a * a, b2 = b * b, p = 2 * cos_vw, q = 2 * cos_uw, r = 2 * cos_uv, p2 = p * p, p3 = p2 * p, q2 = q * q, r2 = r * r,
                 r3 = r2 * r, r4 = r3 * r, r5 = r4 * r;
    const double c0 = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a;
    const double c1 = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q;
    const double c2 = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2;
    const double c3 = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q;
    const double c4 = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1;
    const double m3 = c1 / c0, m2 = c2 / c0, m1 = c3 / c0, m0 = c4 / c0;       // z^4 + m3 z^3 + m2 z^2 + m1 z + m0
    if (c0 == 0.0 || !(fabs(m3) <= DBL_MAX) || !(fabs(m2) <= DBL_MAX) || !(fabs(m1) <= DBL_MAX) || !(fabs(m0) <= DBL_MAX)) return 0;
    const double rad = 1.0 + fmax(fmax(fabs(m3), fabs(m2)), fmax(fabs(m1), fabs(m0)));
    const double kc = 0.9210609940028851, ks = 0.3894183423086505;              // cos 0.4, sin 0.4
    double zr0 = rad * kc, zi0 = rad * ks, zr1 = -rad * ks, zi1 = rad * kc, zr2 = -rad * kc, zi2 = -rad * ks, zr3 = rad * ks, zi3 = -rad * kc;
    for (int it = 0; it < kRootIters; ++it) {
        bool moved = false;
        // one Aberth step of root (zr, zi) against the three others: w = N / (1 - N S), N = p / p', S = sum 1 / (z - z_j)
#define XPNP_ABERTH(zr, zi, ar, ai, br, bi, cr, ci)                                                                           \
        {                                                                                                                     \
            double pr = zr + m3, pi = zi, dr = 1.0, di = 0.0, tr, ti;                                                         \
            for (int k = 0; k < 3; ++k) {                                                                                     \
                tr = dr * zr - di * zi + pr; ti = dr * zi + di * zr + pi; dr = tr; di = ti;                                   \
                const double mk = k == 0 ? m2 : (k == 1 ? m1 : m0);                                                           \
                tr = pr * zr - pi * zi + mk; ti = pr * zi + pi * zr; pr = tr; pi = ti;                                        \
            }                                                                                                                 \
            const double dd = dr * dr + di * di;                                                                              \
            const double nr = (pr * dr + pi * di) / dd, ni = (pi * dr - pr * di) / dd;                                        \
            double sr = 0.0, si = 0.0, er, ei, ee;                                                                            \
            er = zr - ar; ei = zi - ai; ee = er * er + ei * ei; sr += er / ee; si -= ei / ee;                                 \
            er = zr - br; ei = zi - bi; ee = er * er + ei * ei; sr += er / ee; si -= ei / ee;                                 \
            er = zr - cr; ei = zi - ci; ee = er * er + ei * ei; sr += er / ee; si -= ei / ee;                                 \
            const double qr = 1.0 - (nr * sr - ni * si), qi = -(nr * si + ni * sr), qq = qr * qr + qi * qi;                    \
            const double wr = (nr * qr + ni * qi) / qq, wi = (ni * qr - nr * qi) / qq;                                        \
            if (dd != 0.0 && (pr != 0.0 || pi != 0.0)) {                                                                      \
                if (!(wr * wr + wi * wi <= kRootTol * kRootTol * (zr * zr + zi * zi))) moved = true;                          \
                zr -= wr; zi -= wi;                                                                                           \
            }                                                                                                                 \
        }
        XPNP_ABERTH(zr0, zi0, zr1, zi1, zr2, zi2, zr3, zi3)
        XPNP_ABERTH(zr1, zi1, zr0, zi0, zr2, zi2, zr3, zi3)
        XPNP_ABERTH(zr2, zi2, zr0, zi0, zr1, zi1, zr3, zi3)
        XPNP_ABERTH(zr3, zi3, zr0, zi0, zr1, zi1, zr2, zi2)
#undef XPNP_ABERTH
        if (!moved) break;
        if (!(fabs(zr0) <= DBL_MAX && fabs(zr1) <= DBL_MAX && fabs(zr2) <= DBL_MAX && fabs(zr3) <= DBL_MAX)) return 0;
    }
    // ascending real part (a stable network: equal parts keep their order)
#define XPNP_CSWAP(ar, ai, br, bi) if (br < ar) { double t_ = ar; ar = br; br = t_; t_ = ai; ai = bi; bi = t_; }
    XPNP_CSWAP(zr0, zi0, zr1, zi1) XPNP_CSWAP(zr2, zi2, zr3, zi3) XPNP_CSWAP(zr0, zi0, zr2, zi2) XPNP_CSWAP(zr1, zi1, zr3, zi3)
    XPNP_CSWAP(zr1, zi1, zr2, zi2)
#undef XPNP_CSWAP
    const double bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2;
    const double b1 = b * bb1 * bb1;
    double ms[3];
    for (int k = 0; k < 3; ++k) ms[k] = (Xw[k] + Xw[3 + k] + Xw[6 + k]) / 3.0;
    int count = 0;
    for (int s = 0; s < 4; ++s) {
        const double x = s == 0 ? zr0 : (s == 1 ? zr1 : (s == 2 ? zr2 : zr3)), xi = s == 0 ? zi0 : (s == 1 ? zi1 : (s == 2 ? zi2 : zi3));
        if (!(fabs(xi) <= kRootMaxImag) || !(x >= 0.0)) continue;
        const double x2 = x * x, x3 = x2 * x;
        const double b0 =
            ((1 - a - b) * x2 + (a - 1) * q * x - a + b + 1) *
            (r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
             r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a +
                   q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) * x2 +
             (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
              r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
              r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) * x +
             (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
             (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a + (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b +
             (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b + p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q);
        const double y = b0 / b1, y2 = y * y;
        const double nu = x2 + y2 - 2 * x * y * cos_uv;
        const double dPC = dAB / sqrt(nu), dPB = y * dPC, dPA = x * dPC;
        double cam[9], md[3], sig[9], R[9];
        for (int k = 0; k < 3; ++k) { cam[k] = u[k] * dPA; cam[3 + k] = v[k] * dPB; cam[6 + k] = w[k] * dPC; }
        for (int k = 0; k < 3; ++k) md[k] = (cam[k] + cam[3 + k] + cam[6 + k]) / 3.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                sig[3 * i + j] = ((cam[i] - md[i]) * (Xw[j] - ms[j]) + (cam[3 + i] - md[i]) * (Xw[3 + j] - ms[j]) +
                                  (cam[6 + i] - md[i]) * (Xw[6 + j] - ms[j])) / 3.0;
        rotation_from_cov(sig, R);
        double* P = out + 12 * count;
        bool ok = true;
        for (int i = 0; i < 3; ++i) {
            const double t = md[i] - (R[3 * i] * ms[0] + R[3 * i + 1] * ms[1] + R[3 * i + 2] * ms[2]);
            P[4 * i] = R[3 * i]; P[4 * i + 1] = R[3 * i + 1]; P[4 * i + 2] = R[3 * i + 2]; P[4 * i + 3] = t;
            ok = ok && fabs(R[3 * i]) <= DBL_MAX && fabs(R[3 * i + 1]) <= DBL_MAX && fabs(R[3 * i + 2]) <= DBL_MAX && fabs(t) <= DBL_MAX;
        }
        if (ok) ++count;
    }
    return count;
}

// ------------------------------------------------------------------------------------------------ EPnP in stages
// Workspace of one local optimisation.  A stage reads the sums of the per-inlier terms before it from red[].
struct Epnp {
    int n;                 // inliers
    double cw[12];         // control points, world (cws_)
    double cci[9];         // CC^-1
    double M[144], V[144]; // M'M and its eigenvectors (columns); the 3x3 of the control points before that
    int order[4];          // columns of V for the four smallest eigenvalues, smallest first (Ut rows 11, 10, 9, 8)
    double L[60], rho[6];
    double cc[36];         // control points, camera (ccs_), of the three candidates, sign step applied
    double pc0[9];
    double Rt[36];
    double err[3];
    double la[30], lv[25], lb[6], lx[5], ls[5];
    double red[40];
};

// cyclic two-sided Jacobi on the symmetric N x N m (full storage, stride N); v receives the eigenvectors as columns
XPNP_HD inline void jacobi_eig(double* m, double* v, int N) {
    for (int i = 0; i < N * N; ++i) v[i] = 0.0;
    double tr = 0.0;
    for (int i = 0; i < N; ++i) { v[i * N + i] = 1.0; tr += fabs(m[i * N + i]); }
    const double floor_abs = 1e-18 * tr;
    for (int sweep = 0; sweep < kEigSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double mpq = m[p * N + q], mpp = m[p * N + p], mqq = m[q * N + q];
                if (!(fabs(mpq) > kRotTol * sqrt(fabs(mpp * mqq)) + floor_abs)) continue;
                rotated = true;
                const double theta = (mqq - mpp) / (2.0 * mpq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < N; ++r) {
                    const double mp = m[r * N + p], mq = m[r * N + q], vp = v[r * N + p], vq = v[r * N + q];
                    m[r * N + p] = c * mp - s * mq; m[r * N + q] = s * mp + c * mq;
                    v[r * N + p] = c * vp - s * vq; v[r * N + q] = s * vp + c * vq;
                }
                for (int k = 0; k < N; ++k) {
                    const double mp = m[p * N + k], mq = m[q * N + k];
                    m[p * N + k] = c * mp - s * mq; m[q * N + k] = s * mp + c * mq;
                }
                m[p * N + q] = 0.0; m[q * N + p] = 0.0;
            }
        if (!rotated) break;
    }
}

// minimum-norm least squares of the 6 x c system w.la (stride 5) x = w.lb by one-sided Jacobi SVD; singular values at or below
// thr times the largest are dropped (JacobiSVD::solve: thr = c eps; ColPivHouseholderQR::solve drops exact zeros only: thr = 0)
XPNP_HD inline void ls_solve(Epnp& w, int c, double thr) {
    double* a = w.la; double* v = w.lv;
    for (int i = 0; i < 25; ++i) v[i] = 0.0;
    for (int i = 0; i < c; ++i) v[5 * i + i] = 1.0;
    for (int sweep = 0; sweep < kLsSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < c - 1; ++p)
            for (int q = p + 1; q < c; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 6; ++r) { al += a[5 * r + p] * a[5 * r + p]; be += a[5 * r + q] * a[5 * r + q]; ga += a[5 * r + p] * a[5 * r + q]; }
                if (!(fabs(ga) > kRotTol * sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 6; ++r) {
                    const double ap = a[5 * r + p], aq = a[5 * r + q];
                    a[5 * r + p] = cs * ap - sn * aq; a[5 * r + q] = sn * ap + cs * aq;
                }
                for (int r = 0; r < c; ++r) {
                    const double vp = v[5 * r + p], vq = v[5 * r + q];
                    v[5 * r + p] = cs * vp - sn * vq; v[5 * r + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    double smax = 0.0;
    for (int j = 0; j < c; ++j) {
        double s2 = 0.0;
        for (int r = 0; r < 6; ++r) s2 += a[5 * r + j] * a[5 * r + j];
        w.ls[j] = s2;
        smax = fmax(smax, s2);
    }
    for (int i = 0; i < c; ++i) w.lx[i] = 0.0;
    for (int j = 0; j < c; ++j) {
        if (!(w.ls[j] > 0.0) || !(sqrt(w.ls[j]) > thr * sqrt(smax))) continue;
        double d = 0.0;
        for (int r = 0; r < 6; ++r) d += a[5 * r + j] * w.lb[r];
        d /= w.ls[j];
        for (int i = 0; i < c; ++i) w.lx[i] += v[5 * i + j] * d;
    }
}

// stage 0 terms: X and 1 (4)
XPNP_HD inline void epnp_stage_centroid(Epnp& w) {
    w.n = (int)w.red[3];
    for (int k = 0; k < 3; ++k) w.cw[k] = w.red[k] / w.n;
}
// stage 1 terms: the upper triangle of (X - c0)(X - c0)' (6)
XPNP_HD inline void epnp_terms1(const Epnp& w, const double* X, double* acc) {
    const double d0 = X[0] - w.cw[0], d1 = X[1] - w.cw[1], d2 = X[2] - w.cw[2];
    acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
}
// ChooseControlPoints and ComputeBarycentricCoordinates' matrices; false when CC has rank < 3 at Eigen's default threshold
XPNP_HD inline bool epnp_stage_control(Epnp& w) {
    double* m = w.M; double* v = w.V;
    m[0] = w.red[0]; m[1] = m[3] = w.red[1]; m[2] = m[6] = w.red[2]; m[4] = w.red[3]; m[5] = m[7] = w.red[4]; m[8] = w.red[5];
    jacobi_eig(m, v, 3);
    // singular values of the symmetric matrix, descending
    int o0 = 0, o1 = 1, o2 = 2;
    if (fabs(m[4 * o1]) > fabs(m[4 * o0])) { const int t = o0; o0 = o1; o1 = t; }
    if (fabs(m[4 * o2]) > fabs(m[4 * o1])) { const int t = o1; o1 = o2; o2 = t; }
    if (fabs(m[4 * o1]) > fabs(m[4 * o0])) { const int t = o0; o0 = o1; o1 = t; }
    const int ord[3] = {o0, o1, o2};
    for (int i = 1; i < 4; ++i) {
        const double k = sqrt(fabs(m[4 * ord[i - 1]]) / w.n);
        for (int r = 0; r < 3; ++r) w.cw[3 * i + r] = w.cw[r] + k * v[3 * r + ord[i - 1]];
    }
    double CC[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 1; j < 4; ++j) CC[3 * i + j - 1] = w.cw[3 * j + i] - w.cw[i];
    {   // rank by column-pivoted orthogonalisation: pivots at or below 3 eps times the largest do not count (colPivHouseholderQr().rank())
        double c0[3] = {CC[0], CC[3], CC[6]}, c1[3] = {CC[1], CC[4], CC[7]}, c2[3] = {CC[2], CC[5], CC[8]};
        auto nrm2 = [](const double* c) { return c[0] * c[0] + c[1] * c[1] + c[2] * c[2]; };
        auto swp = [](double* a, double* b) { for (int r = 0; r < 3; ++r) { const double t = a[r]; a[r] = b[r]; b[r] = t; } };
        auto project = [](double* c, const double* b, double bn) {
            const double d = (b[0] * c[0] + b[1] * c[1] + b[2] * c[2]) / bn;
            for (int r = 0; r < 3; ++r) c[r] -= d * b[r];
        };
        if (nrm2(c1) > nrm2(c0) && nrm2(c1) >= nrm2(c2)) swp(c0, c1);
        else if (nrm2(c2) > nrm2(c0)) swp(c0, c2);
        const double p0 = nrm2(c0);
        if (!(p0 > 0.0)) return false;
        const double thr = sqrt(p0) * (3.0 * DBL_EPSILON);
        project(c1, c0, p0); project(c2, c0, p0);
        if (nrm2(c2) > nrm2(c1)) swp(c1, c2);
        const double p1 = nrm2(c1);
        if (!(sqrt(p1) > thr)) return false;
        project(c2, c1, p1);
        if (!(sqrt(nrm2(c2)) > thr)) return false;
    }
    const double det = CC[0] * (CC[4] * CC[8] - CC[5] * CC[7]) - CC[1] * (CC[3] * CC[8] - CC[5] * CC[6]) + CC[2] * (CC[3] * CC[7] - CC[4] * CC[6]);
    const double id = 1.0 / det;
    w.cci[0] = (CC[4] * CC[8] - CC[5] * CC[7]) * id; w.cci[1] = (CC[2] * CC[7] - CC[1] * CC[8]) * id; w.cci[2] = (CC[1] * CC[5] - CC[2] * CC[4]) * id;
    w.cci[3] = (CC[5] * CC[6] - CC[3] * CC[8]) * id; w.cci[4] = (CC[0] * CC[8] - CC[2] * CC[6]) * id; w.cci[5] = (CC[2] * CC[3] - CC[0] * CC[5]) * id;
    w.cci[6] = (CC[3] * CC[7] - CC[4] * CC[6]) * id; w.cci[7] = (CC[1] * CC[6] - CC[0] * CC[7]) * id; w.cci[8] = (CC[0] * CC[4] - CC[1] * CC[3]) * id;
    return all_finite(w.cci, 9);
}
XPNP_HD inline void epnp_alpha(const Epnp& w, const double* X, double al[4]) {
    const double d0 = X[0] - w.cw[0], d1 = X[1] - w.cw[1], d2 = X[2] - w.cw[2];
    al[1] = w.cci[0] * d0 + w.cci[1] * d1 + w.cci[2] * d2;
    al[2] = w.cci[3] * d0 + w.cci[4] * d1 + w.cci[5] * d2;
    al[3] = w.cci[6] * d0 + w.cci[7] * d1 + w.cci[8] * d2;
    al[0] = 1.0 - al[1] - al[2] - al[3];
}
// stage 2 terms: for the ten pairs j <= l of barycentric coordinates, a_j a_l times {1, x, y, x^2 + y^2} (40): M'M of ComputeM
XPNP_HD inline void epnp_terms2(const Epnp& w, const double* X, double x, double y, double* acc) {
    double al[4];
    epnp_alpha(w, X, al);
    const double rr = x * x + y * y;
    int e = 0;
    for (int j = 0; j < 4; ++j)
        for (int l = j; l < 4; ++l, e += 4) {
            const double aa = al[j] * al[l];
            acc[e] += aa; acc[e + 1] += aa * x; acc[e + 2] += aa * y; acc[e + 3] += aa * rr;
        }
}
XPNP_HD inline void epnp_gauss_newton(Epnp& w, double be[4]) {
    for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < 6; ++i) {
            const double* l = w.L + 10 * i;
            w.la[5 * i] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            w.la[5 * i + 1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            w.la[5 * i + 2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
            w.la[5 * i + 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
            w.lb[i] = w.rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                                  l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        ls_solve(w, 4, 0.0);
        for (int k = 0; k < 4; ++k) be[k] += w.lx[k];
    }
}
// M'M, its four smallest eigenvectors, L6x10, rho, the three beta approximations with five Gauss-Newton steps each, ComputeCcs
// and the sign step (deviation 3) with the first inlier Xfirst
XPNP_HD inline void epnp_stage_solve(Epnp& w, const double* Xfirst) {
    for (int i = 0; i < 144; ++i) w.M[i] = 0.0;
    {
        int e = 0;
        for (int j = 0; j < 4; ++j)
            for (int l = j; l < 4; ++l, e += 4) {
                const double s1 = w.red[e], sx = w.red[e + 1], sy = w.red[e + 2], sr = w.red[e + 3];
                for (int h = 0; h < 2; ++h) {
                    const int a = h ? l : j, b = h ? j : l;
                    double* blk = w.M + (3 * a) * 12 + 3 * b;
                    blk[0] = s1; blk[13] = s1; blk[2] = -sx; blk[24] = -sx; blk[14] = -sy; blk[25] = -sy; blk[26] = sr;
                }
            }
    }
    jacobi_eig(w.M, w.V, 12);
    {   // the four smallest eigenvalues, smallest first (stable selection)
        bool taken[12];
        for (int i = 0; i < 12; ++i) taken[i] = false;
        for (int s = 0; s < 4; ++s) {
            int best = -1;
            for (int i = 0; i < 12; ++i)
                if (!taken[i] && (best < 0 || w.M[13 * i] < w.M[13 * best])) best = i;
            taken[best] = true; w.order[s] = best;
        }
    }
    auto ut = [&](int i, int c) { return w.V[12 * c + w.order[i]]; };     // Ut(11 - i, c)
    for (int j = 0, a = 0, b = 1; j < 6; ++j) {
        double dv[4][3];
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 3; ++k) dv[i][k] = ut(i, 3 * a + k) - ut(i, 3 * b + k);
        auto dot = [&](int i, int k) { return dv[i][0] * dv[k][0] + dv[i][1] * dv[k][1] + dv[i][2] * dv[k][2]; };
        double* l = w.L + 10 * j;
        l[0] = dot(0, 0); l[1] = 2.0 * dot(0, 1); l[2] = dot(1, 1); l[3] = 2.0 * dot(0, 2); l[4] = 2.0 * dot(1, 2); l[5] = dot(2, 2);
        l[6] = 2.0 * dot(0, 3); l[7] = 2.0 * dot(1, 3); l[8] = 2.0 * dot(2, 3); l[9] = dot(3, 3);
        double d = 0.0;
        for (int k = 0; k < 3; ++k) { const double e = w.cw[3 * a + k] - w.cw[3 * b + k]; d += e * e; }
        w.rho[j] = d;
        b += 1;
        if (b > 3) { a += 1; b = a + 1; }
    }
    for (int cand = 0; cand < 3; ++cand) {
        double be[4] = {0.0, 0.0, 0.0, 0.0};
        const int cols = cand == 0 ? 4 : (cand == 1 ? 3 : 5);
        for (int i = 0; i < 6; ++i) {
            const double* l = w.L + 10 * i;
            if (cand == 0) { w.la[5 * i] = l[0]; w.la[5 * i + 1] = l[1]; w.la[5 * i + 2] = l[3]; w.la[5 * i + 3] = l[6]; }
            else for (int k = 0; k < cols; ++k) w.la[5 * i + k] = l[k];
            w.lb[i] = w.rho[i];
        }
        ls_solve(w, cols, cols * DBL_EPSILON);
        const double* x = w.lx;
        if (cand == 0) {
            if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = -x[1] / be[0]; be[2] = -x[2] / be[0]; be[3] = -x[3] / be[0]; }
            else { be[0] = sqrt(x[0]); be[1] = x[1] / be[0]; be[2] = x[2] / be[0]; be[3] = x[3] / be[0]; }
        } else {
            if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
            else { be[0] = sqrt(x[0]); be[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) be[0] = -be[0];
            be[2] = cand == 2 ? x[3] / be[0] : 0.0;
        }
        epnp_gauss_newton(w, be);
        double* cc = w.cc + 12 * cand;
        for (int j = 0; j < 12; ++j) cc[j] = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 12; ++j) cc[j] += be[i] * ut(i, j);
        double al[4];
        epnp_alpha(w, Xfirst, al);
        const double depth = al[0] * cc[2] + al[1] * cc[5] + al[2] * cc[8] + al[3] * cc[11];
        if (depth < 0.0)
            for (int j = 0; j < 12; ++j) cc[j] = -cc[j];
    }
}
XPNP_HD inline void epnp_pc(const Epnp& w, int cand, const double al[4], double pc[3]) {
    const double* cc = w.cc + 12 * cand;
    for (int j = 0; j < 3; ++j) pc[j] = al[0] * cc[j] + al[1] * cc[3 + j] + al[2] * cc[6 + j] + al[3] * cc[9 + j];
}
// stage 3 terms: the camera-frame points of the three candidates (9)
XPNP_HD inline void epnp_terms3(const Epnp& w, const double* X, double* acc) {
    double al[4], pc[3];
    epnp_alpha(w, X, al);
    for (int c = 0; c < 3; ++c) { epnp_pc(w, c, al, pc); acc[3 * c] += pc[0]; acc[3 * c + 1] += pc[1]; acc[3 * c + 2] += pc[2]; }
}
XPNP_HD inline void epnp_stage_means(Epnp& w) { for (int k = 0; k < 9; ++k) w.pc0[k] = w.red[k] / w.n; }
// stage 4 terms: (pc - pc0)(X - pw0)' of the three candidates (27); pw0 is the centroid cw[0..2]
XPNP_HD inline void epnp_terms4(const Epnp& w, const double* X, double* acc) {
    double al[4], pc[3];
    epnp_alpha(w, X, al);
    const double d[3] = {X[0] - w.cw[0], X[1] - w.cw[1], X[2] - w.cw[2]};
    for (int c = 0; c < 3; ++c) {
        epnp_pc(w, c, al, pc);
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) acc[9 * c + 3 * j + k] += (pc[j] - w.pc0[3 * c + j]) * d[k];
    }
}
// EstimateRT of the three candidates
XPNP_HD inline void epnp_stage_rt(Epnp& w) {
    for (int c = 0; c < 3; ++c) {
        double a[9], R[9];
        for (int k = 0; k < 9; ++k) a[k] = w.red[9 * c + k];
        rotation_from_cov(a, R);
        double* P = w.Rt + 12 * c;
        for (int i = 0; i < 3; ++i) {
            P[4 * i] = R[3 * i]; P[4 * i + 1] = R[3 * i + 1]; P[4 * i + 2] = R[3 * i + 2];
            P[4 * i + 3] = w.pc0[3 * c + i] - (R[3 * i] * w.cw[0] + R[3 * i + 1] * w.cw[1] + R[3 * i + 2] * w.cw[2]);
        }
    }
}
// stage 5 terms: the square roots of the residuals of the three candidates (3)
XPNP_HD inline void epnp_terms5(const Epnp& w, const double* X, double x, double y, double* acc) {
    for (int c = 0; c < 3; ++c) acc[c] += sqrt(residual(w.Rt + 12 * c, X, x, y));
}
// the best of the three; false when it is not finite
XPNP_HD inline bool epnp_stage_pick(Epnp& w, double* P) {
    for (int c = 0; c < 3; ++c) w.err[c] = w.red[c];
    int best = 0;
    if (w.err[1] < w.err[0]) best = 1;
    if (w.err[2] < w.err[best]) best = 2;
    for (int k = 0; k < 12; ++k) P[k] = w.Rt[12 * best + k];
    return all_finite(P, 12);
}

// the unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (row-major, stride 4) by the usual four-branch rule
XPNP_HD inline void quat_from_pose(const double* P, double q[4]) {
    const double m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9], m22 = P[10];
    const double tr = m00 + m11 + m22;
    double x, y, z, w;
    if (tr > 0.0) { const double s = sqrt(tr + 1.0) * 2.0; w = 0.25 * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s; }
    else if (m00 > m11 && m00 > m22) { const double s = sqrt(1.0 + m00 - m11 - m22) * 2.0; w = (m21 - m12) / s; x = 0.25 * s; y = (m01 + m10) / s; z = (m02 + m20) / s; }
    else if (m11 > m22) { const double s = sqrt(1.0 + m11 - m00 - m22) * 2.0; w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25 * s; z = (m12 + m21) / s; }
    else { const double s = sqrt(1.0 + m22 - m00 - m11) * 2.0; w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25 * s; }
    const double inv = (w < 0.0 ? -1.0 : 1.0) / sqrt(x * x + y * y + z * z + w * w);
    q[0] = x * inv; q[1] = y * inv; q[2] = z * inv; q[3] = w * inv;
}

}  // namespace xpnp
