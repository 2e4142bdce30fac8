// Marginal covariance of selected cameras from the tile-Cholesky factor of the UNDAMPED reduced camera matrix
// (include/xrsfm_ba.h: xrsfm_ba_covariance), and of selected points through the same forward substitution with a general
// right-hand side (xrsfm_ba_point_covariance: the second half of this file).  Then the joint matrix of a selection
// (xrsfm_ba_joint_covariance) and, last, every camera and point block of the whole map by selected inversion of the factor
// (xrsfm_ba_map_covariance: k_selinv_off / k_selinv_diag and the point pass k_cov_map_points).
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
// host marks the tile columns a chunk reaches (cov_build_lists, xrsfm_ba.hip), gives them compact panel slots and launches, per
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
// RHS = false: the unit columns of the selected cameras (sel_row, n_chunk).  RHS = true (point covariance): a general right-hand
// side, Xt_k = Bt_k - sum: the panel slot of k holds Bt_k on entry (k_cov_pt_scatter into zero-filled slots) and Zt_k on exit; only
// this workgroup touches the slot during its level.  sel_row / n_chunk are not read.
template <bool RHS>
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
    if constexpr (RHS) load_tile_regs(ra, Zt + (size_t)en.y * kCovPanel, kNB);      // Bt_k
    __syncthreads();
    if constexpr (RHS) {
        store_tile_lds(As, ra);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                for (int g = 0; g < 4; ++g) As[(r0 + 16 * m + lk + 4 * g) * kLdT + c0 + 16 * n2 + li] -= acc[m][n2][g];
        store_tile_lds(Bs, rb);
        __syncthreads();
    } else {
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
    }
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

// ---------------------------------------------------------------- marginal covariance of selected points (xrsfm_ba_point_covariance)
// Sigma_pp = Hinv_p + Y_p^T Y_p,  Y_p = L^-1 (W_p Hinv_p),  W_p = sum_obs F_c^T E_p (6 N_c x 3, rows of the observing cameras):
// three right-hand-side columns per point, 21 points (63 of the 64 panel columns) per chunk, forward substitution only.
constexpr int kCovPtsPerChunk = 21;

// One streaming pass over the packed slots: every observation of a selected point (pt_col[packed point] >= 0: its index in the
// selection) yields one record {selection index, camera} + the scaled 6x3 block F_c^T E_p Hinv_p (row-major, [a][b]), F / E as every
// other consumer rebuilds them (load_FE_rc: stored or recomputed J).  blk == nullptr: count only (the host sizes the record arrays).
// The record ORDER follows an integer ticket and is arbitrary; the values are not, and every (point, camera) cell of the panel has
// exactly one record (a track observed twice by one camera is refused before), so nothing downstream depends on the order.
__global__ __launch_bounds__(kBlock) void k_cov_pt_rhs(Dev d, const int* __restrict__ pt_col, int cap, int* __restrict__ counter,
                                                       int2* __restrict__ rec_id, double* __restrict__ blk) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= d.n_slots) return;
    const int cam = d.slot_cam[slot];
    if (cam < 0) return;
    const int pt = d.slot_pt[slot];
    const int si = pt_col[pt];
    if (si < 0) return;
    const int r = atomicAdd(counter, 1);
    if (!blk || r >= cap) return;
    double F[12], E[6], r0, r1;
    load_FE_rc(d, slot, cam, pt, F, E, r0, r1);
    const double* Hi = d.Hinv + 6 * (size_t)pt;
    const double h[6] = {Hi[0], Hi[1], Hi[2], Hi[3], Hi[4], Hi[5]};
    rec_id[r] = make_int2(si, cam);
    double* o = blk + 18 * (size_t)r;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double w0 = F[a] * E[0] + F[6 + a] * E[3], w1 = F[a] * E[1] + F[6 + a] * E[4], w2 = F[a] * E[2] + F[6 + a] * E[5];
        o[3 * a + 0] = w0 * h[0] + w1 * h[1] + w2 * h[2];
        o[3 * a + 1] = w0 * h[1] + w1 * h[3] + w2 * h[4];
        o[3 * a + 2] = w0 * h[2] + w1 * h[4] + w2 * h[5];
    }
}

// Records of one chunk into its zero-filled panel slots: ent = {record, panel slot, row of the camera in its tile column, 3 x index
// of the point in the chunk}; thread = (entry, element of the 6x3 block).  Bt[slot][3 i + b][row + a].
__global__ __launch_bounds__(256) void k_cov_pt_scatter(const int4* __restrict__ ent, int n_ent, const double* __restrict__ blk, double* __restrict__ Bt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 18 * n_ent) return;
    const int4 e = ent[i / 18];
    const int q = i % 18, a = q / 3, b = q % 3;
    Bt[(size_t)e.y * kCovPanel + (size_t)(e.w + b) * kNB + e.z + a] = blk[18 * (size_t)e.x + q];
}

// cov_p = D_p (Hinv_p + Y_p^T Y_p) D_p: one wave per point of the chunk (4 points per workgroup), the reached panel slots in
// elimination order, 64 rows each.  Thread = (entry (a, b), quarter of the 64 rows), the quarters added by two shuffles as in
// k_cov_gram: one fixed order, (a, b) and (b, a) add the same products in the same order.  D_p = the Jacobi scale of the point.
__global__ __launch_bounds__(256) void k_cov_pt_gram(Dev d, const double* __restrict__ Zt, int n_slots, const int* __restrict__ sel_pt, int n_chunk,
                                                     double* __restrict__ cov) {
    const int pi = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
    if (pi >= n_chunk || t >= 36) return;
    const int e = t >> 2, part = t & 3, a = e / 3, b = e % 3;
    const double* za = Zt + (size_t)(3 * pi + a) * kNB + part * 16;
    const double* zb = Zt + (size_t)(3 * pi + b) * kNB + part * 16;
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
        const int pt = sel_pt[pi];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const double hv = d.Hinv[6 * (size_t)pt + (lo == 0 ? hi : lo + hi + 1)];      // upper storage: 00 01 02 11 12 22
        const double* sp = d.scale_p + 3 * (size_t)pt;
        cov[9 * (size_t)pi + e] = (hv + s) * (sp[a] * sp[b]);
    }
}

// Hinv (6) and the Jacobi scale (3) of selected points, for the fallback's host arithmetic
__global__ void k_cov_pt_gather(Dev d, const int* __restrict__ sel_pt, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pt = sel_pt[i];
    for (int k = 0; k < 6; ++k) out[9 * (size_t)i + k] = d.Hinv[6 * (size_t)pt + k];
    for (int k = 0; k < 3; ++k) out[9 * (size_t)i + 6 + k] = d.scale_p[3 * (size_t)pt + k];
}

// ---------------------------------------------------------------- joint covariance with cross blocks (xrsfm_ba_joint_covariance)
// Every chunk of the selection (10 cameras with unit injection, 21 free points with the scattered right-hand side) keeps panel
// slots of its own, so that after the forward substitutions the panels X = L^-1 [E_c .. | W_p Hinv_p ..] of ALL chunks are resident.
// In the scaled coordinates of the front half
//     Sigma_cc' = X_c^T X_c',    Sigma_cp = -X_c^T X_p,    Sigma_pp' = delta_pp' Hinv_p + X_p^T X_p':
// the Gram between the panels of two chunks, one 64x64x64 FP64 A B^T product per tile column both chunks reach.
constexpr int kCovJointMaxCols = XRSFM_BA_JOINT_COV_MAX_COLS;      // columns of one joint call (include/xrsfm_ba.h states the memory this bounds)

// One workgroup per chunk pair (A <= B): G_AB = sum_k Zt_A[k] Zt_B[k]^T over the tile columns k both chunks reach.
//   ent  [pair] = {q0, q1}: its list slots[q0 .. q1)
//   slots [q]   = {panel slot of k in A, panel slot of k in B}, k ascending (elimination order)
// A panel column is a row of the A or of the B operand, an element of an MFMA result depends on its own row of A and of B only, and
// a slot holds exact zeros in the panel columns that do not reach its tile column: a product with such a slot adds exact zeros.  So
// an entry depends on its two columns only, not on what shares their chunks, and the sum over k is not split: one workgroup adds
// the tile columns in ascending order whatever the chunks reach.  Staging as in k_lv_fwd_multi: two 64 x 66 operand tiles in LDS
// (66 KiB: two workgroups per compute unit), the next operands in registers while the matrix cores work on the current ones.
__global__ __launch_bounds__(256) void k_cov_joint_gram(const int2* __restrict__ ent, const int2* __restrict__ slots, const double* __restrict__ Zt,
                                                        double* __restrict__ G) {
    __shared__ __attribute__((aligned(16))) double As[kNB * kLdT];
    __shared__ __attribute__((aligned(16))) double Bs[kNB * kLdT];
    const int2 en = ent[blockIdx.x];
    const int q0 = en.x, q1 = en.y;
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
        const int2 e = slots[q0];
        load_tile_regs(ra, Zt + (size_t)e.x * kCovPanel, kNB);
        load_tile_regs(rb, Zt + (size_t)e.y * kCovPanel, kNB);
    }
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                       // the previous product no longer reads LDS
        store_tile_lds(As, ra);
        store_tile_lds(Bs, rb);
        __syncthreads();
        if (q + 1 < q1) {
            const int2 e = slots[q + 1];
            load_tile_regs(ra, Zt + (size_t)e.x * kCovPanel, kNB);
            load_tile_regs(rb, Zt + (size_t)e.y * kCovPanel, kNB);
        }
        tile_abt_mfma(As, Bs, acc);            // += Zt_A[k] Zt_B[k]^T
    }
    double* out = G + (size_t)blockIdx.x * kCovPanel;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(r0 + 16 * m + lk + 4 * g) * kNB + c0 + 16 * n2 + li] = acc[m][n2][g];
}

// The N x N result in the caller's order from the chunk-pair Grams.  col [i] = {panel column of row / column i (64 x chunk + column
// in the chunk, chunks in the order of the pairs; -1: a constant point), camera or packed point, degree of freedom in its block,
// 0 camera / 1 point}.  Thread = one entry (i <= j) of the upper triangle: it reads the entry of the pair (the earlier panel column
// is the row: one location whatever the caller's order), negates camera-point entries, adds Hinv_p on a point's own block,
// applies the two Jacobi scales (0 on constant degrees of freedom: exact zeros) and writes (i, j) and its mirror image (j, i).
__global__ __launch_bounds__(256) void k_cov_joint_finish(Dev d, const int4* __restrict__ col, int N, int n_chunks, const double* __restrict__ G,
                                                          double* __restrict__ cov) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)N * N) return;
    const int i = (int)(id / N), j = (int)(id % N);
    if (i > j) return;
    const int4 ci = col[i], cj = col[j];
    auto scale = [&](const int4& cl) {
        if (cl.x < 0) return 0.0;
        if (cl.w) return d.scale_p[3 * (size_t)cl.y + cl.z];
        const unsigned cc = d.cam_const[cl.y];
        return (cl.z < 3 ? (cc & 1u) : (cc & 2u)) ? 0.0 : d.scale_c[6 * (size_t)cl.y + cl.z];
    };
    const double di = scale(ci), dj = scale(cj);
    double v = 0.0;
    if (di != 0.0 && dj != 0.0) {
        const int lo = ci.x < cj.x ? ci.x : cj.x, hi = ci.x < cj.x ? cj.x : ci.x;
        const int A = lo >> 6, B = hi >> 6;
        const size_t pair = (size_t)A * n_chunks - (size_t)A * (A - 1) / 2 + (B - A);      // pairs (A, B >= A) row by row
        double s = G[pair * kCovPanel + (size_t)(lo & 63) * kNB + (hi & 63)];
        if (ci.w != cj.w) s = -s;
        else if (ci.w && ci.y == cj.y) {
            const int a = ci.z < cj.z ? ci.z : cj.z, b = ci.z < cj.z ? cj.z : ci.z;
            s = d.Hinv[6 * (size_t)ci.y + (a == 0 ? b : a + b + 1)] + s;      // upper storage: 00 01 02 11 12 22
        }
        v = s * (di * dj);
    }
    cov[(size_t)i * N + j] = v;
    cov[(size_t)j * N + i] = v;
}

// ---------------------------------------------------------------- whole-map covariance by selected inversion (xrsfm_ba_map_covariance)
// Z = S^-1 on the tile pattern of the factor (Takahashi recurrence).  From Z L = L^-T, with I_k the rows of the off-diagonal tiles
// of tile column k:
//     Z_ik = -(sum_{m in I_k} Z_im L_mk) Linv_k                      i in I_k        (k_selinv_off)
//     Z_kk = Linv_k^T (Linv_k - sum_{m in I_k} L_mk^T Z_mk)                          (k_selinv_diag)
// (the issue's N_mk = L_mk Linv_k with Linv_k taken out of the sum: one product with Linv_k per target tile, and L stays as the
// factorisation left it).  Z_im is tile (i, m) of Z for m <= i and tile (m, i) transposed for m > i; both lie on the pattern (the
// fill closure of the factorisation) and belong to ancestors of k, that is to higher levels: the levels are walked from the root
// down, per level one launch for the off-diagonal tiles and one for the diagonal tiles (which read the former), one workgroup
// per target tile, the kernel boundary the only synchronisation.  Z lives in a second tile storage with the factor's own layout
// (tile_ptr with S replaced): dense and packed tiles run the same instructions on the same values.  m ascends: two calls agree
// bit for bit.  The products are A B^T on the FP64 matrix cores (tile_abt_mfma); an operand that the formula wants transposed
// is transposed on its way from the registers into LDS (store_tile_lds_t).  LDS and staging as in k_lv_fwd_multi.
__device__ __forceinline__ void store_tile_lds_t(double* dst, const double2 (&v)[8]) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int e = threadIdx.x + 256 * it;
        const int r = e >> 5, c2 = (e & 31) * 2;
        dst[c2 * kLdT + r] = v[it].x; dst[(c2 + 1) * kLdT + r] = v[it].y;
    }
}

//   ent [b] = {i, k, q0, q1}: target tile (i, k), i > k, and its list lm[q0 .. q1) = I_k, ascending
__global__ __launch_bounds__(256) void k_selinv_off(CholDev c, double* __restrict__ Zs, const int4* __restrict__ ent, const int* __restrict__ lm) {
    __shared__ __attribute__((aligned(16))) double As[kNB * kLdT];
    __shared__ __attribute__((aligned(16))) double Bs[kNB * kLdT];
    const int4 en = ent[blockIdx.x];
    const int i = en.x, k = en.y, q0 = en.z, q1 = en.w;
    CholDev z = c; z.S = Zs;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int r0 = (wave >> 1) * 32, c0 = (wave & 1) * 32;
    v4d acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) acc[m][n2] = (v4d){0.0, 0.0, 0.0, 0.0};
    double2 ra[8], rb[8];
    int m_cur = lm[q0];
    load_tile_regs(ra, m_cur <= i ? tile_ptr(z, i, m_cur) : tile_ptr(z, m_cur, i), c.ld);
    load_tile_regs(rb, tile_ptr(c, m_cur, k), c.ld);
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                       // the previous product no longer reads LDS
        if (m_cur <= i) store_tile_lds(As, ra); else store_tile_lds_t(As, ra);      // Z_im
        store_tile_lds_t(Bs, rb);                                                    // L_mk^T
        __syncthreads();
        if (q + 1 < q1) {
            m_cur = lm[q + 1];
            load_tile_regs(ra, m_cur <= i ? tile_ptr(z, i, m_cur) : tile_ptr(z, m_cur, i), c.ld);
            load_tile_regs(rb, tile_ptr(c, m_cur, k), c.ld);
        }
        tile_abt_mfma(As, Bs, acc);            // += Z_im L_mk
    }
    load_tile_regs(rb, c.Linv + (size_t)k * kNB * kNB, kNB);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) As[(r0 + 16 * m + lk + 4 * g) * kLdT + c0 + 16 * n2 + li] = acc[m][n2][g];
    store_tile_lds_t(Bs, rb);                  // Linv_k^T
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) acc[m][n2] = (v4d){0.0, 0.0, 0.0, 0.0};
    tile_abt_mfma(As, Bs, acc);                // (sum) Linv_k
    double* out = tile_ptr(z, i, k);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(size_t)(r0 + 16 * m + lk + 4 * g) * c.ld + c0 + 16 * n2 + li] = -acc[m][n2][g];
}

//   ent [b] = {k, 0, q0, q1}: diagonal tile k and its list lm[q0 .. q1) = I_k, ascending (empty at a root).  The tile is written
// symmetrised, 0.5 (X + X^T) with both halves from one sum: the camera blocks read from it are exactly symmetric.
__global__ __launch_bounds__(256) void k_selinv_diag(CholDev c, double* __restrict__ Zs, const int4* __restrict__ ent, const int* __restrict__ lm) {
    __shared__ __attribute__((aligned(16))) double As[kNB * kLdT];
    __shared__ __attribute__((aligned(16))) double Bs[kNB * kLdT];
    const int4 en = ent[blockIdx.x];
    const int k = en.x, q0 = en.z, q1 = en.w;
    CholDev z = c; z.S = Zs;
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
        const int m0 = lm[q0];
        load_tile_regs(ra, tile_ptr(c, m0, k), c.ld);
        load_tile_regs(rb, tile_ptr(z, m0, k), c.ld);
    }
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                       // the previous product no longer reads LDS
        store_tile_lds_t(As, ra);              // L_mk^T
        store_tile_lds_t(Bs, rb);              // Z_mk^T
        __syncthreads();
        if (q + 1 < q1) {
            const int m1 = lm[q + 1];
            load_tile_regs(ra, tile_ptr(c, m1, k), c.ld);
            load_tile_regs(rb, tile_ptr(z, m1, k), c.ld);
        }
        tile_abt_mfma(As, Bs, acc);            // += L_mk^T Z_mk
    }
    load_tile_regs(rb, c.Linv + (size_t)k * kNB * kNB, kNB);
    __syncthreads();
    store_tile_lds_t(As, rb);                  // Linv_k^T
    store_tile_lds_t(Bs, rb);
    __syncthreads();
    // Bs = (Linv_k - sum)^T: every element has one owner
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) Bs[(c0 + 16 * n2 + li) * kLdT + r0 + 16 * m + lk + 4 * g] -= acc[m][n2][g];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) acc[m][n2] = (v4d){0.0, 0.0, 0.0, 0.0};
    tile_abt_mfma(As, Bs, acc);                // Linv_k^T (Linv_k - sum)
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int g = 0; g < 4; ++g) As[(r0 + 16 * m + lk + 4 * g) * kLdT + c0 + 16 * n2 + li] = acc[m][n2][g];
    __syncthreads();
    double* out = tile_ptr(z, k, k);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int e = t + 256 * it, r = e >> 6, cc = e & 63;
        out[(size_t)r * c.ld + cc] = 0.5 * (As[r * kLdT + cc] + As[cc * kLdT + r]);
    }
}

// Camera blocks of the whole map: D_c Z_cc D_c from the diagonal tile of the camera's elimination row; thread = (camera, entry).
// Zeros on constant degrees of freedom and for cameras that are not in the program.
__global__ __launch_bounds__(256) void k_cov_map_cams(Dev d, CholDev c, const double* __restrict__ Zs, double* __restrict__ cov) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= d.n_cams * 36) return;
    const int cam = id / 36, e = id % 36, a = e / 6, b = e % 6;
    const unsigned cc = d.cam_const[cam];
    const double* sc = d.scale_c + 6 * (size_t)cam;
    const double da = (a < 3 ? (cc & 1u) : (cc & 2u)) ? 0.0 : sc[a];
    const double db = (b < 3 ? (cc & 1u) : (cc & 2u)) ? 0.0 : sc[b];
    double v = 0.0;
    if (d.cam_act[cam] > 0.0 && da != 0.0 && db != 0.0) {
        CholDev z = c; z.S = const_cast<double*>(Zs);
        const int row = c.cam_off[cam], tk = row >> 6, o = row & 63;
        v = tile_ptr(z, tk, tk)[(size_t)(o + a) * c.ld + o + b] * (da * db);
    }
    cov[id] = v;
}

// First and last slot of every packed point (a track's slots are consecutive; the walk below tests every slot all the same).
// first[] starts at INT_MAX, last[] at -1.
__global__ __launch_bounds__(kBlock) void k_cov_map_ranges(Dev d, int* __restrict__ first, int* __restrict__ last) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= d.n_slots || d.slot_cam[slot] < 0) return;
    const int pt = d.slot_pt[slot];
    atomicMin(first + pt, slot);
    atomicMax(last + pt, slot);
}

// V_c = F_c^T E_p Hinv_p of one observation (6x3, [a][b]: what k_cov_pt_rhs records)
__device__ __forceinline__ void cov_map_v(const Dev& d, int slot, int cam, int pt, double (&V)[18]) {
    double F[12], E[6], r0, r1;
    load_FE_rc(d, slot, cam, pt, F, E, r0, r1);
    const double* Hi = d.Hinv + 6 * (size_t)pt;
    const double h[6] = {Hi[0], Hi[1], Hi[2], Hi[3], Hi[4], Hi[5]};
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double w0 = F[a] * E[0] + F[6 + a] * E[3], w1 = F[a] * E[1] + F[6 + a] * E[4], w2 = F[a] * E[2] + F[6 + a] * E[5];
        V[3 * a + 0] = w0 * h[0] + w1 * h[1] + w2 * h[2];
        V[3 * a + 1] = w0 * h[1] + w1 * h[3] + w2 * h[4];
        V[3 * a + 2] = w0 * h[2] + w1 * h[4] + w2 * h[5];
    }
}

// M += V_o^T sum_{o'} Z(c_o, c_o') V_o' for one observation o (elimination row `row`, block V) against the n observations of its
// track (rows Rs[], < 0: no observation; blocks Vs[][18]), o' ascending.  The 6x6 block of Z: tile (row >> 6, row' >> 6) at
// (row & 63, row' & 63) when row >= row', otherwise tile (row' >> 6, row >> 6) read transposed; two cameras of one tile column
// meet in its (symmetric) diagonal tile.
__device__ __forceinline__ void cov_map_pairs(const CholDev& z, int row, const double (&V)[18], int n, const int* Rs, const double* Vs, double (&M)[9]) {
    double U[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) U[q] = 0.0;
    for (int o = 0; o < n; ++o) {
        const int ro = Rs[o];
        if (ro < 0) continue;
        const bool low = row >= ro;
        const int hi = low ? row : ro, lo = low ? ro : row;
        const double* base = tile_ptr(z, hi >> 6, lo >> 6) + (size_t)(hi & 63) * z.ld + (lo & 63);
        const size_t sa = low ? z.ld : 1, sb = low ? 1 : z.ld;
        const double* vo = Vs + 18 * (size_t)o;
        double W[18];
#pragma unroll
        for (int q = 0; q < 18; ++q) W[q] = vo[q];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const double zab = base[a * sa + b * sb];
#pragma unroll
                for (int j = 0; j < 3; ++j) U[3 * a + j] = fma(zab, W[3 * b + j], U[3 * a + j]);
            }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = M[3 * i + j];
#pragma unroll
            for (int a = 0; a < 6; ++a) s = fma(V[3 * a + i], U[3 * a + j], s);
            M[3 * i + j] = s;
        }
}

// cov_p = D_p (Hinv_p + sum_{c, c'} V_c^T Z_cc' V_c') D_p from the 9 sums of a point; (a, b) and (b, a) from one value
__device__ __forceinline__ void cov_map_write(const Dev& d, int pt, const double (&M)[9], double* __restrict__ cov) {
    const double* Hi = d.Hinv + 6 * (size_t)pt;
    const double* sp = d.scale_p + 3 * (size_t)pt;
    double* o = cov + 9 * (size_t)pt;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const double s = a == b ? M[3 * a + a] : 0.5 * (M[3 * a + b] + M[3 * b + a]);
            const double v = (Hi[a == 0 ? b : a + b + 1] + s) * (sp[a] * sp[b]);      // upper storage: 00 01 02 11 12 22
            o[3 * a + b] = v; o[3 * b + a] = v;
        }
}

// The point pass of the whole map: one wave per packed point whose track spans at most 64 slots (4 points per workgroup), lane =
// observation.  The wave keeps the track's V_c and elimination rows in LDS, every lane adds its row of pairs (c, c') in ascending
// order of c', and the lanes are added by the fixed shuffle tree of wave_sum.  Constant points and longer tracks are left to the
// zero fill and to k_cov_map_long.  cov [n_pts][9], packed point order.
__global__ __launch_bounds__(256) void k_cov_map_points(Dev d, CholDev c, const double* __restrict__ Zs, const int* __restrict__ first, const int* __restrict__ last,
                                                        double* __restrict__ cov) {
    __shared__ double Vs[4][kWave * 18];
    __shared__ int Rs[4][kWave];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pt = blockIdx.x * 4 + wave;
    int s0 = 0, n = 0;
    if (pt < d.n_pts && !d.pt_const[pt]) { s0 = first[pt]; n = last[pt] - s0 + 1; }
    const bool active = n > 0 && n <= kWave;
    CholDev z = c; z.S = const_cast<double*>(Zs);
    double V[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) V[q] = 0.0;
    int row = -1;
    if (active && lane < n) {
        const int slot = s0 + lane, cam = d.slot_cam[slot];
        if (cam >= 0 && d.slot_pt[slot] == pt) { cov_map_v(d, slot, cam, pt, V); row = c.cam_off[cam]; }
    }
    Rs[wave][lane] = row;
#pragma unroll
    for (int q = 0; q < 18; ++q) Vs[wave][18 * lane + q] = V[q];
    __syncthreads();
    double M[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) M[q] = 0.0;
    if (active && row >= 0) cov_map_pairs(z, row, V, n, Rs[wave], Vs[wave], M);
#pragma unroll
    for (int q = 0; q < 9; ++q) M[q] = wave_sum(M[q]);
    if (active && lane == 0) cov_map_write(d, pt, M, cov);
}

// ... and one workgroup per point of a longer track (ent = {packed point, offset of its span in the scratch arrays}): the V_c and
// rows of the span go to global scratch (Vg [18 per slot], Rg), thread = observations t, t + 256, ..., the threads' sums are added
// in LDS by a fixed tree.
__global__ __launch_bounds__(256) void k_cov_map_long(Dev d, CholDev c, const double* __restrict__ Zs, const int* __restrict__ first, const int* __restrict__ last,
                                                      const int2* __restrict__ ent, double* __restrict__ Vg, int* __restrict__ Rg, double* __restrict__ cov) {
    __shared__ double red[256][9];
    const int2 en = ent[blockIdx.x];
    const int pt = en.x, t = threadIdx.x;
    const int s0 = first[pt], n = last[pt] - s0 + 1;
    double* Vp = Vg + 18 * (size_t)en.y;
    int* Rp = Rg + en.y;
    CholDev z = c; z.S = const_cast<double*>(Zs);
    for (int o = t; o < n; o += 256) {
        const int slot = s0 + o, cam = d.slot_cam[slot];
        double V[18];
#pragma unroll
        for (int q = 0; q < 18; ++q) V[q] = 0.0;
        int row = -1;
        if (cam >= 0 && d.slot_pt[slot] == pt) { cov_map_v(d, slot, cam, pt, V); row = c.cam_off[cam]; }
        Rp[o] = row;
#pragma unroll
        for (int q = 0; q < 18; ++q) Vp[18 * (size_t)o + q] = V[q];
    }
    __threadfence();
    __syncthreads();
    double M[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) M[q] = 0.0;
    for (int o = t; o < n; o += 256) {
        const int row = Rp[o];
        if (row < 0) continue;
        double V[18];
#pragma unroll
        for (int q = 0; q < 18; ++q) V[q] = Vp[18 * (size_t)o + q];
        cov_map_pairs(z, row, V, n, Rp, Vp, M);
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) red[t][q] = M[q];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off)
#pragma unroll
            for (int q = 0; q < 9; ++q) red[t][q] += red[t + off][q];
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 9; ++q) M[q] = red[0][q];
        cov_map_write(d, pt, M, cov);
    }
}

}  // namespace xba
