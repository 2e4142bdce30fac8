// Marginal covariance of selected cameras from the tile-Cholesky factor of the UNDAMPED reduced camera matrix
// (include/xrsfm_ba.h: xrsfm_ba_covariance).
//
// With S = L L^T and E_c the 6 unit columns of camera c in elimination order, Z_c = L^-1 E_c and block (c,c) of S^-1 is
// Z_c^T Z_c: a forward substitution with a right-hand-side PANEL, no backward pass.  The panel holds 6 columns per camera,
// at most 10 cameras (60 of 64 columns) per chunk, so that a chunk's rows of one tile column are one 64x64 operand next to a
// 64x64 factor tile and both steps of a tile column are the FP64 MFMA tile product of the factorisation (tile_abt_mfma):
//     X_k = E_k - sum_{j < k, L_kj != 0} L_kj Z_j,      Z_k = Linv_k X_k        (Linv_k: what potrf_lds left behind)
// The panel is kept TRANSPOSED in global memory (Zt_k = Z_k^T, row = panel column): tile_abt_mfma forms A B^T from two
// row-major operands, and  (L_kj Z_j)^T = Zt_j L_kj^T,  Zt_k = Xt_k Linv_k^T  are of that form with no transposition anywhere.
// A panel column is a ROW of the A operand, and an element of an MFMA result depends on its own row of A only: the values
// of a camera's columns do not depend on which other cameras share its chunk (bit-identical for any selection).
//
// Sparsity: column block c of L^-1 is non-zero only on c's tile column and its ancestors in the elimination tree.  The
// host marks the tile columns a chunk reaches (ba_cov_chunk_lists), gives them compact panel slots and launches, per
// level, one workgroup per reached column with a list of the reached columns j it reads; nothing else is touched.
#pragma once
#include "ba_chol.h"

namespace xba {

constexpr int kCovCamsPerChunk = 10;      // 6 columns each: 60 of the 64 panel columns
constexpr int kCovPanel = kNB * kNB;      // doubles per panel slot (Zt_k, row-major, ld = 64)

// Undamped point blocks and the unit "damping" of rows that are not in the program.  The run path never inverts Hpp itself
// (it adds clamp(diag) / radius first); here the damping is an explicit zero, so a point block must be positive definite on
// its own: a free point whose 3x3 block is not (one observation gives rank 2) is counted in singular[0], the smallest such
// point index lands in singular[1].  Constant points have E = 0:
// their factor is never multiplied by anything but zero and is stored as zero.  Rows of constant camera blocks and of
// cameras without observations are all-zero in J: they get a unit diagonal (Dc2 = 1), which decouples them from the rest,
// and the caller zeroes them in the output (or refuses the camera).
// The pivots are compared with 64 eps times their diagonal entry: an exactly rank-deficient block leaves a pivot of the order
// of eps times the entry after rounding, of either sign.
__global__ void k_cov_prep(Dev d, int n_pt_blocks, int* __restrict__ singular) {
    if ((int)blockIdx.x >= n_pt_blocks) {
        const int i = (blockIdx.x - n_pt_blocks) * blockDim.x + threadIdx.x;
        if (i < d.n_cams * 6) {
            const int cam = i / 6, r = i % 6;
            const unsigned cc = d.cam_const[cam];
            const bool out = !(d.cam_act[cam] > 0.0) || (r < 3 ? (cc & 1u) : (cc & 2u)) != 0;
            d.Dc2[i] = out ? 1.0 : 0.0;
        }
        return;
    }
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.n_pts) return;
    double* o = d.Hinv + 6 * (size_t)p;
    double* oc = d.Hc + 6 * (size_t)p;
    if (d.pt_const[p]) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { o[k] = 0.0; oc[k] = 0.0; }
        return;
    }
    const double* H = d.Hpp + 6 * (size_t)p;
    const double h[6] = {H[0], H[1], H[2], H[3], H[4], H[5]};
    constexpr double kTol = 64.0 * 2.220446049250313e-16;
    const double p0 = h[0];
    const double l10 = h[1] / p0, l20 = h[2] / p0;
    const double p1 = h[3] - l10 * h[1];
    const double l21 = (h[4] - l20 * h[1]) / p1;
    const double p2 = h[5] - l20 * h[2] - l21 * (h[4] - l20 * h[1]);
    if (!(p0 > 0.0) || !(p1 > kTol * h[3]) || !(p2 > kTol * h[5]) || !isfinite(p0 + p1 + p2)) {
        atomicAdd(singular, 1);
        atomicMin(singular + 1, p);
#pragma unroll
        for (int k = 0; k < 6; ++k) { o[k] = 0.0; oc[k] = 0.0; }
        return;
    }
    double inv[6];
    sym3_inverse(h, inv);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = inv[k];
    // Hinv = C C^T, C lower {c00 c10 c20 c11 c21 c22} (what k_point_prep stores for the S assembly)
    const double c00 = sqrt(fmax(inv[0], 0.0)), r0 = c00 > 0.0 ? 1.0 / c00 : 0.0;
    const double c10 = inv[1] * r0, c20 = inv[2] * r0;
    const double c11 = sqrt(fmax(inv[3] - c10 * c10, 0.0)), r1 = c11 > 0.0 ? 1.0 / c11 : 0.0;
    const double c21 = (inv[4] - c20 * c10) * r1;
    const double c22 = sqrt(fmax(inv[5] - c20 * c20 - c21 * c21, 0.0));
    oc[0] = c00; oc[1] = c10; oc[2] = c20; oc[3] = c11; oc[4] = c21; oc[5] = c22;
}

// One workgroup per reached tile column k of one elimination-tree level (every L_kj and Zt_j it reads belongs to a lower level:
// the kernel boundary is the only synchronisation).
//   ent [b]      = {k, panel slot of k, q0, q1}: its list lj[q0 .. q1)
//   lj  [q]      = {j, panel slot of j}, j ascending: the reached columns j < k with a structurally non-zero tile (k, j)
//   sel_row [ci] = first elimination row of the chunk's camera ci (panel columns 6 ci .. 6 ci + 5), n_chunk <= 10 of them
// LDS: two 64 x 66 operand tiles (67 584 B = 66 KiB: two workgroups per compute unit); the next operands are in registers while the
// matrix cores work on the current ones, as in lv_factor_body.
__global__ __launch_bounds__(256) void k_lv_fwd_multi(CholDev c, const int4* __restrict__ ent, const int2* __restrict__ lj,
                                                      double* __restrict__ Zt, const int* __restrict__ sel_row, int n_chunk) {
    __shared__ __attribute__((aligned(16))) double As[kNB * kLdT];
    __shared__ __attribute__((aligned(16))) double Bs[kNB * kLdT];
    const int4 en = ent[blockIdx.x];
    const int k = en.x, q0 = en.z, q1 = en.w;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int r0 = (wave >> 1) * 32, c0 = (wave & 1) * 32;
    v4d acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) acc[m][n2] = (v4d){0.0, 0.0, 0.0, 0.0};
    double2 ra[8], rb[8];
    if (q0 < q1) {
        const int2 e = lj[q0];
        load_tile_regs(ra, Zt + (size_t)e.y * kCovPanel, kNB);
        load_tile_regs(rb, tile_ptr(c, k, e.x), c.ld);
    }
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                       // the previous product no longer reads LDS
        store_tile_lds(As, ra);
        store_tile_lds(Bs, rb);
        __syncthreads();
        if (q + 1 < q1) {
            const int2 e = lj[q + 1];
            load_tile_regs(ra, Zt + (size_t)e.y * kCovPanel, kNB);
            load_tile_regs(rb, tile_ptr(c, k, e.x), c.ld);
        }
        tile_abt_mfma(As, Bs, acc);            // += Zt_j L_kj^T
    }
    load_tile_regs(rb, c.Linv + (size_t)k * kNB * kNB, kNB);
    __syncthreads();
    // Xt_k = Et_k - sum (row = panel column, column = row of tile column k)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) As[(r0 + 16 * m + lk + 4 * g) * kLdT + c0 + 16 * n2 + li] = -acc[m][n2][g];
    store_tile_lds(Bs, rb);
    __syncthreads();
    if (t < 6 * n_chunk) {
        const int row = sel_row[t / 6] + t % 6;
        if ((row >> 6) == k) As[t * kLdT + (row & 63)] += 1.0;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) acc[m][n2] = (v4d){0.0, 0.0, 0.0, 0.0};
    tile_abt_mfma(As, Bs, acc);                // Zt_k = Xt_k Linv_k^T
    double* out = Zt + (size_t)en.y * kCovPanel;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(r0 + 16 * m + lk + 4 * g) * kNB + c0 + 16 * n2 + li] = acc[m][n2][g];
}

// cov_c = D_c Z_c^T Z_c D_c: one workgroup per camera of the chunk, the reached panel slots in elimination order
// (slots [0, n_slots): the host numbers them by ascending tile column), 64 rows each.  Thread = (entry (a, b), quarter of
// the 64 rows); the quarters are added by two shuffles: one fixed order, so two calls agree bit for bit, and entries (a, b)
// and (b, a) add the same products in the same order.  Slots outside the camera's own ancestors hold exact zeros.
// D_c = the Jacobi scale of the camera's columns (the solve ran in scaled coordinates), 0 on constant blocks.
__global__ __launch_bounds__(256) void k_cov_gram(Dev d, const double* __restrict__ Zt, int n_slots, const int* __restrict__ sel_cam,
                                                  double* __restrict__ cov) {
    const int ci = blockIdx.x, t = threadIdx.x;
    if (t >= 144) return;
    const int e = t >> 2, part = t & 3, a = e / 6, b = e % 6;
    const double* za = Zt + (size_t)(6 * ci + a) * kNB + part * 16;
    const double* zb = Zt + (size_t)(6 * ci + b) * kNB + part * 16;
    double s = 0.0;
    for (int sl = 0; sl < n_slots; ++sl) {
        const double* pa = za + (size_t)sl * kCovPanel;
        const double* pb = zb + (size_t)sl * kCovPanel;
#pragma unroll
        for (int m = 0; m < 16; ++m) s = fma(pa[m], pb[m], s);
    }
    s += __shfl_xor(s, 1, kWave);
    s += __shfl_xor(s, 2, kWave);
    if (part == 0) {
        const int cam = sel_cam[ci];
        const unsigned cc = d.cam_const[cam];
        const double* sc = d.scale_c + 6 * (size_t)cam;
        const double da = (a < 3 ? (cc & 1u) : (cc & 2u)) ? 0.0 : sc[a];
        const double db = (b < 3 ? (cc & 1u) : (cc & 2u)) ? 0.0 : sc[b];
        cov[36 * (size_t)ci + e] = (da == 0.0 || db == 0.0) ? 0.0 : s * (da * db);      // (da * db: the same factor for (a, b) and (b, a))
    }
}

}  // namespace xba
