// Resident solver for local-BA-sized problems (BASolver::LBA, /root/reference/src/mapper/incremental_mapper.cc:71): the whole
// Levenberg-Marquardt loop of ba_run_impl in ONE launch of ONE workgroup, for problems whose reduced camera system is a single
// tile (at most kLbaMaxCams cameras = 60 unknowns).  xrsfm_ba_options::linear_solver = XRSFM_BA_SOLVER_RESIDENT selects it; the
// run path (xrsfm_ba.hip / ba_kernels.h / ba_chol.h) is not touched and stays its cross-check.
//
// Same arithmetic per observation as the engine (ba_math.h: project, huber, quat_plus; the blocks of linearize_item, the point
// factor of point_factor()), the same restated Ceres loop (Jacobi scaling from the first linearisation, D^2 = clamp(diag) /
// radius, ba_trust_region.h), read from the context's packed arrays as xrsfm_ba_create left them: tiles of 64 slots, whole
// tracks per tile, lane = observation.
//
// One workgroup of kLbaBlock threads = kLbaWaves waves; there is no other workgroup and therefore nothing to wait for: every
// loop is bounded by the tile count, the camera count or max_iterations.  For the same reason N problems run as N workgroups of
// one launch (k_lba_batch at the end of this file, xrsfm_ba_run_batch): both kernels call lba_resident_solve.
//
//   pass A (lba_linearize): a chunk = kLbaWaves tiles, one per wave.  Every lane forms r, F (2x6), E (2x3) of its observation;
//     H_pp / g_p per track by segmented wave sums; the head lane factors the damped point block (H_pp + D^2)^-1 = C C^T and
//     hands C to its track; every lane stages V = (F^T E) C (6x3), F and r in LDS, the head z = C^T g_p, and a table
//     track x camera -> lane.  After a barrier the GATHER: thread = (row of a 6x6 block of S | row of a camera's H_cc, g_c,
//     V z) x slice of the tracks, accumulating in registers over all chunks in a fixed order: no floating-point atomics,
//     the slices are added in slice order at the end.  S = H_cc + D^2 - sum V_a V_b^T, b = g_c - sum V_a z.
//   factor / solve: right-looking Cholesky of the 6 n_cams square system in LDS (one barrier per column), the two triangular
//     solves in wave 0 with the right-hand side in registers (lane = row).
//   pass C (lba_backsub): wave-local; J and r recomputed as in pass A, y_p = C C^T (g_p - sum E^T F y_c), candidate points,
//     model decrease, and the candidate's cost in the same pass (the candidate cameras are in LDS before it starts).
//   Lane 0 of wave 0 keeps the trust region and decides; the decision reaches the others through LDS.
//
// LDS map (doubles; kLbaSmemBytes in all, one workgroup on the CU's 160 KiB):
//   [0, 9216)       V      [512 slots][18]            | after the last chunk of a pass A the staging area is dead and holds
//   [9216, 16384)   F | r  [512 slots][14]            | part [512][8] (slice partials), S [60][61], L [60][61]
//   [16384, 17920)  z      [8 tiles][64 tracks][3]
//   [17920, 18944)  table  [8 tiles][64 tracks][16] bytes: lane of the track's observation by camera, 255 = none
//   [18944, ...)    cameras (current and candidate q, t, M, intrinsics, scales), H_cc rows, g_c, b, y, pivots, reduction
//                   scratch, the controller's scalars
#pragma once

#include "ba_kernels.h"
#include "ba_trust_region.h"

namespace xba {

constexpr int kLbaBlock = 512;
constexpr int kLbaWaves = kLbaBlock / kWave;
constexpr int kLbaMaxCams = 10;          // one tile column of the reduced system (ba_plan.h: 10 cameras per 64x64 tile)
constexpr int kLbaMaxObs = 32768;        // cap on the observation count: one CU streams them three times per LM iteration
constexpr int kLbaLd = 61;               // row stride of S and L in LDS (odd: a column walk changes bank)

struct LbaOpt { int max_it, want_rows; double ftol, ptol, gtol, radius0, huber_a; };
struct LbaRow { double cost, change, gmax, step, rho, radius; int it, pad; };
struct LbaResult {
    double initial_cost, final_cost;
    int n_successful, n_unsuccessful, termination, reason, attempted, status, n_rows, pad;     // status 1: a track observed twice by one camera
};

constexpr int kLbaOffF = kLbaBlock * 18, kLbaOffZ = kLbaOffF + kLbaBlock * 14, kLbaOffTab = kLbaOffZ + kLbaWaves * kWave * 3;
constexpr int kLbaOffSm = kLbaOffTab + kLbaWaves * kWave * 16 / 8;
constexpr int kLbaOffPart = 0, kLbaOffS = kLbaBlock * 8, kLbaOffL = kLbaOffS + 60 * kLbaLd;
static_assert(kLbaOffL + 60 * kLbaLd <= kLbaOffZ, "the solve phase lives in the dead staging area");

// small state behind the staging area
struct LbaSm {
    double q[kLbaMaxCams][4], t[kLbaMaxCams][3], intr[kLbaMaxCams][8], M[kLbaMaxCams][9];
    double sc[kLbaMaxCams][6];        // Jacobi scale of the camera columns
    double scm[kLbaMaxCams][6];       // ... times the 0/1 mask of constant blocks
    double cq[kLbaMaxCams][4], ct[kLbaMaxCams][3], cM[kLbaMaxCams][9];     // candidate
    double Hcc[60][6];                // rows of the camera blocks J_c^T J_c
    double gc[60], rhs[60], y[64], dinv[64];
    double cstep2[kLbaMaxCams], cxn2[kLbaMaxCams], cgm[kLbaMaxCams];
    double red[kLbaWaves][4];
    double tot[4];                    // pass totals: cost (sum rho), |x_points|^2, point gradient max | model, |step_points|^2, candidate cost
    double radius;
    int model[kLbaMaxCams], cconst[kLbaMaxCams], act[kLbaMaxCams];
    int ntrk[kLbaWaves];
    int dup, go, solve_ok, pad;
    // the controller's state (thread 0 alone reads and writes it; in LDS so that it holds no registers through the passes)
    xtr::TrustRegion tr;
    double cost, gmax, xn2_pts, initial_cost, cost_change, step_norm, rel;
    int it, n_succ, n_unsucc, attempted, term, reason, n_rows, pad2;
};
constexpr size_t kLbaSmemBytes = (size_t)kLbaOffSm * 8 + ((sizeof(LbaSm) + 15) & ~(size_t)15);
static_assert(kLbaSmemBytes <= 160 * 1024, "one workgroup on one CU");

// what the kernel reads of the context's Dev (the whole struct as an argument kept ~120 scalar registers busy)
struct LbaDev {
    int n_cams, n_pts, n_tiles;
    const int* slot_cam; const int* slot_pt; const double* slot_u; const double* slot_v; const int* tile_maxlen;
    CamRec* cam; const int* cam_model; const unsigned char* cam_const; const double* cam_act;
    double* P; double* P_cand; const unsigned char* pt_const; double* scale_p; double* Hpp; double* gp;
};
inline LbaDev lba_dev(const Dev& d) {
    return LbaDev{d.n_cams, d.n_pts, d.n_tiles, d.slot_cam, d.slot_pt, d.slot_u, d.slot_v, d.tile_maxlen, d.cam, d.cam_model, d.cam_const,
                  d.cam_act, d.P, d.P_cand, d.pt_const, d.scale_p, d.Hpp, d.gp};
}

struct LbaObs { double F[12], E[6], r0, r1, rho; };

// r, F, E of one observation at (M, t, Pw): the expressions of linearize_item
__device__ __forceinline__ void lba_obs(const double (&M)[9], const double (&t)[3], const double* intr, int model, const double (&Pw)[3],
                                        double u, double v, double huber_a, const double (&scm)[6], const double (&spm)[3], LbaObs& o) {
    Proj pr;
    project<true>(M, t, intr, model, Pw, u, v, pr);
    double rho1;
    o.rho = huber(pr.r0 * pr.r0 + pr.r1 * pr.r1, huber_a, rho1);
    const double sw = sqrt(rho1);
    o.r0 = pr.r0 * sw; o.r1 = pr.r1 * sw;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const double* j = pr.jp + 3 * row;
        o.F[6 * row + 0] = -2.0 * (j[1] * pr.rp[2] - j[2] * pr.rp[1]) * sw * scm[0];
        o.F[6 * row + 1] = -2.0 * (j[2] * pr.rp[0] - j[0] * pr.rp[2]) * sw * scm[1];
        o.F[6 * row + 2] = -2.0 * (j[0] * pr.rp[1] - j[1] * pr.rp[0]) * sw * scm[2];
        o.F[6 * row + 3] = j[0] * sw * scm[3];
        o.F[6 * row + 4] = j[1] * sw * scm[4];
        o.F[6 * row + 5] = j[2] * sw * scm[5];
        o.E[3 * row + 0] = (j[0] * M[0] + j[1] * M[3] + j[2] * M[6]) * sw * spm[0];
        o.E[3 * row + 1] = (j[0] * M[1] + j[1] * M[4] + j[2] * M[7]) * sw * spm[1];
        o.E[3 * row + 2] = (j[0] * M[2] + j[1] * M[5] + j[2] * M[8]) * sw * spm[2];
    }
}

struct LbaSlot { int slot, cam, pt, hl, trk; bool valid, head, var; unsigned long long heads; };

__device__ __forceinline__ LbaSlot lba_slot(const LbaDev& d, int tile, bool active, int lane) {
    LbaSlot s;
    s.slot = tile * kWave + lane;
    s.cam = active ? d.slot_cam[s.slot] : -1;
    s.pt = active ? d.slot_pt[s.slot] : -1;
    s.valid = s.cam >= 0;
    const int prev = __shfl_up(s.pt, 1, kWave);
    s.head = s.valid && (lane == 0 || prev != s.pt);
    s.heads = __ballot(s.head);
    s.hl = seg_head_lane(s.head || !s.valid, lane);
    s.trk = __popcll(s.heads & ((1ull << s.hl) - 1ull));        // number of the lane's track within the tile
    s.var = s.valid && !d.pt_const[s.pt];
    return s;
}

// the lane's observation at the state (cameras sm.q/t/M or the candidate ones, points P)
__device__ __forceinline__ void lba_obs_at(const LbaDev& d, const LbaSm& sm, const LbaSlot& s, const double* __restrict__ P, double huber_a,
                                           double (&Pw)[3], double (&spv)[3], LbaObs& o) {
    double M[9], t[3], scm[6], spm[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = sm.M[s.cam][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = sm.t[s.cam][k];
#pragma unroll
    for (int k = 0; k < 6; ++k) scm[k] = sm.scm[s.cam][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Pw[k] = P[3 * (size_t)s.pt + k]; spv[k] = d.scale_p[3 * (size_t)s.pt + k]; spm[k] = s.var ? spv[k] : 0.0; }
    lba_obs(M, t, sm.intr[s.cam], sm.model[s.cam], Pw, d.slot_u[s.slot], d.slot_v[s.slot], huber_a, scm, spm, o);
}

// fixed-order sum (or maximum) of one value per lane over the workgroup; every thread returns with the result
// (max_mask: bit k set = value k is a maximum)
template <int N>
__device__ __forceinline__ void lba_block_reduce(LbaSm& sm, double (&v)[N], unsigned max_mask, double* out) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(x, off, kWave); x = ((max_mask >> k) & 1u) ? fmax(x, o) : x + o; }
        if (lane == 0) sm.red[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double x = sm.red[0][threadIdx.x];
        const bool mx = ((max_mask >> threadIdx.x) & 1u) != 0;
        for (int w = 1; w < kLbaWaves; ++w) x = mx ? fmax(x, sm.red[w][threadIdx.x]) : x + sm.red[w][threadIdx.x];
        out[threadIdx.x] = x;
    }
    __syncthreads();
}

// what a thread gathers: kind 0 = row r of block (a, b), a <= b, of sum V_a V_b^T; kind 1 = row r of camera a's H_cc, g_c and V z
struct LbaItem { int kind, a, b, r, slice, nslice; };     // kind -1: no item

// Pass A.  Leaves sm.tot = {sum rho, |x_points|^2, point gradient max}, H_pp / g_p in d.Hpp / d.gp, sm.Hcc / sm.gc, and with
// schur: S (lower triangle) and sm.rhs for the radius.  Ends with a barrier.
__device__ __forceinline__ void lba_linearize(const LbaDev& d, LbaSm& sm, double* __restrict__ smem, const double* __restrict__ P, double huber_a,
                                              double radius, bool schur, const LbaItem& item, int n_items) {
    double* sV = smem; double* sF = smem + kLbaOffF; double* sZ = smem + kLbaOffZ;
    unsigned char* tab = reinterpret_cast<unsigned char*>(smem + kLbaOffTab);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int cb = 0; cb < d.n_tiles; cb += kLbaWaves) {
        const int tile = cb + wave;
        const bool active = tile < d.n_tiles;
        const LbaSlot s = lba_slot(d, tile, active, lane);
        const int maxlen = active ? d.tile_maxlen[tile] : 1;
        const int ls = wave * kWave + lane;
        double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        double Pw[3], spv[3] = {1.0, 1.0, 1.0};
        LbaObs o;
        if (s.valid) {
            lba_obs_at(d, sm, s, P, huber_a, Pw, spv, o);
            tot[0] += o.rho;
            const double* E = o.E;
            v[0] = E[0] * E[0] + E[3] * E[3]; v[1] = E[0] * E[1] + E[3] * E[4]; v[2] = E[0] * E[2] + E[3] * E[5];
            v[3] = E[1] * E[1] + E[4] * E[4]; v[4] = E[1] * E[2] + E[4] * E[5]; v[5] = E[2] * E[2] + E[5] * E[5];
            v[6] = E[0] * o.r0 + E[3] * o.r1; v[7] = E[1] * o.r0 + E[4] * o.r1; v[8] = E[2] * o.r0 + E[5] * o.r1;
            if (s.head && s.var) tot[1] += Pw[0] * Pw[0] + Pw[1] * Pw[1] + Pw[2] * Pw[2];
#pragma unroll
            for (int k = 0; k < 12; ++k) sF[ls * 14 + k] = o.F[k];
            sF[ls * 14 + 12] = o.r0; sF[ls * 14 + 13] = o.r1;
        }
        seg_reduce<9>(v, s.pt, lane, maxlen);
        double cf[6] = {0, 0, 0, 0, 0, 0};
        if (s.head) {
            double* H = d.Hpp + 6 * (size_t)s.pt;
#pragma unroll
            for (int k = 0; k < 6; ++k) H[k] = v[k];
            double* g = d.gp + 3 * (size_t)s.pt;
            g[0] = v[6]; g[1] = v[7]; g[2] = v[8];
            tot[2] = fmax(tot[2], fmax(fabs(v[6] / spv[0]), fmax(fabs(v[7] / spv[1]), fabs(v[8] / spv[2]))));
            const double hh[6] = {v[0], v[1], v[2], v[3], v[4], v[5]};
            point_factor(hh, radius, cf);
            double* z = sZ + (wave * kWave + s.trk) * 3;          // z = C^T g_p
            z[0] = cf[0] * v[6]; z[1] = cf[1] * v[6] + cf[3] * v[7]; z[2] = cf[2] * v[6] + cf[4] * v[7] + cf[5] * v[8];
            unsigned long long* row = reinterpret_cast<unsigned long long*>(tab + (wave * kWave + s.trk) * 16);
            row[0] = ~0ull; row[1] = ~0ull;
        }
        if (lane == 0) sm.ntrk[wave] = __popcll(s.heads);
#pragma unroll
        for (int k = 0; k < 6; ++k) cf[k] = __shfl(cf[k], s.hl, kWave);
        if (s.valid) {
            const double* F = o.F; const double* E = o.E;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double w0 = F[r] * E[0] + F[6 + r] * E[3], w1 = F[r] * E[1] + F[6 + r] * E[4], w2 = F[r] * E[2] + F[6 + r] * E[5];
                sV[ls * 18 + 3 * r + 0] = w0 * cf[0];
                sV[ls * 18 + 3 * r + 1] = w0 * cf[1] + w1 * cf[3];
                sV[ls * 18 + 3 * r + 2] = w0 * cf[2] + w1 * cf[4] + w2 * cf[5];
            }
        }
        __syncthreads();                         // (the table rows are cleared)
        if (s.valid) tab[(wave * kWave + s.trk) * 16 + s.cam] = (unsigned char)lane;
        __syncthreads();
        if (s.valid && tab[(wave * kWave + s.trk) * 16 + s.cam] != (unsigned char)lane) sm.dup = 1;      // two lanes of a track on one camera
        if (item.kind == 0 && schur) {
#pragma unroll 1
            for (int w = 0; w < kLbaWaves; ++w) {
                const int nt = sm.ntrk[w];
#pragma unroll 1
                for (int t = item.slice; t < nt; t += item.nslice) {
                    const unsigned char* row = tab + (w * kWave + t) * 16;
                    const int sa = row[item.a], sb = row[item.b];
                    if (sa == 255 || sb == 255) continue;
                    const double* Va = sV + (w * kWave + sa) * 18 + 3 * item.r;
                    const double* Vb = sV + (w * kWave + sb) * 18;
                    const double a0 = Va[0], a1 = Va[1], a2 = Va[2];
#pragma unroll
                    for (int c = 0; c < 6; ++c) acc[c] += a0 * Vb[3 * c] + a1 * Vb[3 * c + 1] + a2 * Vb[3 * c + 2];
                }
            }
        } else if (item.kind == 1) {
#pragma unroll 1
            for (int w = 0; w < kLbaWaves; ++w) {
                const int nt = sm.ntrk[w];
#pragma unroll 1
                for (int t = item.slice; t < nt; t += item.nslice) {
                    const int sa = tab[(w * kWave + t) * 16 + item.a];
                    if (sa == 255) continue;
                    const double* F = sF + (w * kWave + sa) * 14;
                    const double f0 = F[item.r], f1 = F[6 + item.r];
#pragma unroll
                    for (int c = 0; c < 6; ++c) acc[c] += f0 * F[c] + f1 * F[6 + c];
                    acc[6] += f0 * F[12] + f1 * F[13];
                    const double* Va = sV + (w * kWave + sa) * 18 + 3 * item.r;
                    const double* z = sZ + (w * kWave + t) * 3;
                    acc[7] += Va[0] * z[0] + Va[1] * z[1] + Va[2] * z[2];
                }
            }
        }
        __syncthreads();                         // (the staging area is free for the next chunk)
    }
    lba_block_reduce<3>(sm, tot, 4u, sm.tot);
    // slice partials -> S, b (the staging area is dead)
    double* part = smem + kLbaOffPart; double* S = smem + kLbaOffS;
#pragma unroll
    for (int k = 0; k < 8; ++k) part[threadIdx.x * 8 + k] = acc[k];
    for (int e = threadIdx.x; e < 60 * kLbaLd; e += kLbaBlock) S[e] = 0.0;
    __syncthreads();
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (item.kind >= 0 && item.slice == 0) {
        for (int sl = 0; sl < item.nslice; ++sl)
#pragma unroll
            for (int k = 0; k < 8; ++k) sum[k] += part[(threadIdx.x + sl * n_items) * 8 + k];
        if (item.kind == 1) {
            const int i = 6 * item.a + item.r;
#pragma unroll
            for (int c = 0; c < 6; ++c) sm.Hcc[i][c] = sum[c];
            sm.gc[i] = sum[6];
            sm.rhs[i] = sum[6] - sum[7];
        }
    }
    __syncthreads();
    if (schur && item.kind == 0 && item.slice == 0) {
        const int i = 6 * item.a + item.r;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int j = 6 * item.b + c;
            double val = -sum[c];
            if (item.a == item.b) {
                if (c > item.r) continue;
                val += sm.Hcc[i][c];
                if (c == item.r) val += clampd(sm.Hcc[i][c], kLmDiagMin, kLmDiagMax) / radius;
                S[i * kLbaLd + j] = val;
            } else {
                S[j * kLbaLd + i] = val;         // b > a: row of the later camera
            }
        }
    }
    __syncthreads();
}

// S = L L^T (lower triangle of S in place, L and the reciprocal pivots apart), then S y = b in wave 0.  sm.solve_ok = 0 on a
// non-positive pivot or a non-finite solution.  Ends with a barrier.
__device__ __forceinline__ void lba_factor_solve(LbaSm& sm, double* __restrict__ smem, int n) {
    double* S = smem + kLbaOffS; double* L = smem + kLbaOffL;
    const int tid = threadIdx.x;
    bool ok = true;
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        const double s = S[j * kLbaLd + j];
        if (!(s > 0.0)) { ok = false; break; }      // (the same value in every thread)
        const double inv = 1.0 / sqrt(s);
        const int m = n - 1 - j;
#pragma unroll 1
        for (int idx = tid; idx < m * m; idx += kLbaBlock) {
            const int i = j + 1 + idx / m, k = j + 1 + idx % m;
            if (i >= k) S[i * kLbaLd + k] -= (S[i * kLbaLd + j] * inv) * (S[k * kLbaLd + j] * inv);
        }
        if (tid < m) L[(j + 1 + tid) * kLbaLd + j] = S[(j + 1 + tid) * kLbaLd + j] * inv;
        if (tid == 0) sm.dinv[j] = inv;
        __syncthreads();
    }
    if (tid == 0) sm.solve_ok = ok ? 1 : 0;
    __syncthreads();
    if (ok && tid < kWave) {
        double b = tid < n ? sm.rhs[tid] : 0.0;
        for (int j = 0; j < n; ++j) {
            const double zj = __shfl(b, j, kWave) * sm.dinv[j];
            if (tid > j && tid < n) b -= L[tid * kLbaLd + j] * zj;
            if (tid == j) b = zj;
        }
        for (int j = n - 1; j >= 0; --j) {
            const double yj = __shfl(b, j, kWave) * sm.dinv[j];
            if (tid < j) b -= L[j * kLbaLd + tid] * yj;
            if (tid == j) b = yj;
        }
        sm.y[tid] = b;
        if (__ballot(!isfinite(b)) != 0ull && tid == 0) sm.solve_ok = 0;
    }
    __syncthreads();
}

// Candidate cameras from y (cam_update_one): sm.cq / ct / cM, and the cameras' squared step and |x|^2.
__device__ __forceinline__ void lba_cam_update(LbaSm& sm, int c) {
    const double q[4] = {sm.q[c][0], sm.q[c][1], sm.q[c][2], sm.q[c][3]};
    const double t[3] = {sm.t[c][0], sm.t[c][1], sm.t[c][2]};
    const unsigned cc = (unsigned)sm.cconst[c];
    const bool active = sm.act[c] != 0;
    double step2 = 0.0, xn2 = 0.0;
    double qn[4] = {q[0], q[1], q[2], q[3]}, tn[3] = {t[0], t[1], t[2]};
    if (active && !(cc & 1u)) {
        const double dl[3] = {-sm.y[6 * c] * sm.sc[c][0], -sm.y[6 * c + 1] * sm.sc[c][1], -sm.y[6 * c + 2] * sm.sc[c][2]};
        quat_plus(q, dl, qn);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double df = qn[k] - q[k]; step2 += df * df; xn2 += q[k] * q[k]; }
    }
    if (active && !(cc & 2u)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tn[k] = t[k] + (-sm.y[6 * c + 3 + k] * sm.sc[c][3 + k]);
            const double df = tn[k] - t[k]; step2 += df * df; xn2 += t[k] * t[k];
        }
    }
    double M[9];
    quat_to_mat(qn, M);
#pragma unroll
    for (int k = 0; k < 4; ++k) sm.cq[c][k] = qn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) sm.ct[c][k] = tn[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) sm.cM[c][k] = M[k];
    sm.cstep2[c] = step2; sm.cxn2[c] = xn2;
}

// Ceres' gradient max-norm of one camera (cam_gradmax_one)
__device__ __forceinline__ void lba_cam_gradmax(LbaSm& sm, int c) {
    double m = 0.0;
    const unsigned cc = (unsigned)sm.cconst[c];
    const bool active = sm.act[c] != 0;
    if (active && !(cc & 1u)) {
        const double q[4] = {sm.q[c][0], sm.q[c][1], sm.q[c][2], sm.q[c][3]};
        const double dl[3] = {-sm.gc[6 * c] / sm.sc[c][0], -sm.gc[6 * c + 1] / sm.sc[c][1], -sm.gc[6 * c + 2] / sm.sc[c][2]};
        double qn[4];
        quat_plus(q, dl, qn);
#pragma unroll
        for (int k = 0; k < 4; ++k) m = fmax(m, fabs(q[k] - qn[k]));
    }
    if (active && !(cc & 2u))
#pragma unroll
        for (int k = 0; k < 3; ++k) m = fmax(m, fabs(sm.gc[6 * c + 3 + k] / sm.sc[c][3 + k]));
    sm.cgm[c] = m;
}

// Pass C: back-substitution at (sm cameras, P) with the solution sm.y, candidate points into Pc, and the candidate's cost with
// the candidate cameras.  Leaves sm.tot = {model decrease, |step_points|^2, sum rho at the candidate}.  Ends with a barrier.
__device__ __forceinline__ void lba_backsub(const LbaDev& d, LbaSm& sm, const double* __restrict__ P, double* __restrict__ Pc, double huber_a, double radius) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int cb = 0; cb < d.n_tiles; cb += kLbaWaves) {
        const int tile = cb + wave;
        const bool active = tile < d.n_tiles;
        const LbaSlot s = lba_slot(d, tile, active, lane);
        const int maxlen = active ? d.tile_maxlen[tile] : 1;
        double w[3] = {0, 0, 0};
        double Pw[3] = {0, 0, 0}, spv[3] = {1.0, 1.0, 1.0}, v0 = 0.0, v1 = 0.0;
        LbaObs o;
        if (s.valid) {
            lba_obs_at(d, sm, s, P, huber_a, Pw, spv, o);
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double y = sm.y[6 * s.cam + k]; v0 += o.F[k] * y; v1 += o.F[6 + k] * y; }
            w[0] = o.E[0] * v0 + o.E[3] * v1; w[1] = o.E[1] * v0 + o.E[4] * v1; w[2] = o.E[2] * v0 + o.E[5] * v1;
        }
        seg_reduce<3>(w, s.pt, lane, maxlen);
        double u[3] = {0, 0, 0}, pn[3] = {0, 0, 0};
        if (s.head) {
            const double* H = d.Hpp + 6 * (size_t)s.pt;          // (this lane stored them in pass A)
            const double* g = d.gp + 3 * (size_t)s.pt;
            const double hh[6] = {H[0], H[1], H[2], H[3], H[4], H[5]};
            const double a0 = g[0] - w[0], a1 = g[1] - w[1], a2 = g[2] - w[2];
            double cf[6];
            point_factor(hh, radius, cf);
            const double s0 = cf[0] * a0, s1 = cf[1] * a0 + cf[3] * a1, s2 = cf[2] * a0 + cf[4] * a1 + cf[5] * a2;
            u[0] = cf[0] * s0 + cf[1] * s1 + cf[2] * s2;
            u[1] = cf[3] * s1 + cf[4] * s2;
            u[2] = cf[5] * s2;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double dl = s.var ? -u[k] * spv[k] : 0.0;
                pn[k] = Pw[k] + dl;
                Pc[3 * (size_t)s.pt + k] = pn[k];
                const double df = pn[k] - Pw[k];
                tot[1] += df * df;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { u[k] = __shfl(u[k], s.hl, kWave); pn[k] = __shfl(pn[k], s.hl, kWave); }
        if (s.valid) {
            const double m0 = v0 + o.E[0] * u[0] + o.E[1] * u[1] + o.E[2] * u[2];
            const double m1 = v1 + o.E[3] * u[0] + o.E[4] * u[1] + o.E[5] * u[2];
            tot[0] += m0 * (o.r0 - 0.5 * m0) + m1 * (o.r1 - 0.5 * m1);
            double M[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = sm.cM[s.cam][k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = sm.ct[s.cam][k];
            Proj pr;
            project<false>(M, t, sm.intr[s.cam], sm.model[s.cam], pn, d.slot_u[s.slot], d.slot_v[s.slot], pr);
            double rho1;
            tot[2] += huber(pr.r0 * pr.r0 + pr.r1 * pr.r1, huber_a, rho1);
        }
    }
    lba_block_reduce<3>(sm, tot, 0u, sm.tot);
}

// The whole solve of ONE problem by ONE workgroup on the LDS block lba_smem (kLbaSmemBytes): what both kernels below run.  Reads
// and writes nothing but the arrays of d, *result and rows[0 .. max_it].
__device__ __forceinline__ void lba_resident_solve(const LbaDev& d, const LbaOpt& opt, LbaResult* __restrict__ result, LbaRow* __restrict__ rows,
                                                   double* __restrict__ lba_smem) {
    LbaSm& sm = *reinterpret_cast<LbaSm*>(lba_smem + kLbaOffSm);
    const int tid = threadIdx.x;
    const int nc = d.n_cams, n = 6 * nc;
    // the thread's gather item: 6 rows of each of the nc (nc + 1) / 2 blocks, then 6 rows per camera, times the slices
    LbaItem item{-1, 0, 0, 0, 0, 1};
    const int n_blk = nc * (nc + 1) / 2, n_items = 6 * (n_blk + nc);
    {
        const int nslice = n_items > 0 ? kLbaBlock / n_items : 1;        // (>= 1: n_items <= 390)
        item.nslice = nslice;
        if (tid < n_items * nslice) {
            const int it = tid % n_items;
            item.slice = tid / n_items;
            item.r = it % 6;
            int blk = it / 6;
            if (blk < n_blk) {
                item.kind = 0;
                int a = 0;
                for (int len = nc; a < nc && blk >= len; ++a, --len) blk -= len;        // row a of the block triangle holds nc - a blocks
                item.a = a; item.b = a + blk;
            } else {
                item.kind = 1; item.a = blk - n_blk; item.b = item.a;
            }
        }
    }
    if (tid < nc) {
        const CamRec& c = d.cam[tid];
        double q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { q[k] = c.q[k]; sm.q[tid][k] = q[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) sm.t[tid][k] = c.t[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) sm.intr[tid][k] = c.intr[k];
        double M[9];
        quat_to_mat(q, M);
#pragma unroll
        for (int k = 0; k < 9; ++k) sm.M[tid][k] = M[k];
        const unsigned cc = d.cam_const[tid];
        sm.cconst[tid] = (int)cc; sm.model[tid] = d.cam_model[tid]; sm.act[tid] = d.cam_act[tid] > 0.0 ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { sm.sc[tid][k] = 1.0; sm.scm[tid][k] = (cc & (k < 3 ? 1u : 2u)) ? 0.0 : 1.0; }
    }
    if (tid == 0) { sm.dup = 0; sm.go = 1; sm.solve_ok = 0; sm.radius = opt.radius0; }
    for (int i = tid; i < 3 * d.n_pts; i += kLbaBlock) d.scale_p[i] = 1.0;
    __syncthreads();
    double* Pcur = d.P; double* Pcand = d.P_cand;
    if (tid == 0) {
        sm.tr = xtr::TrustRegion{opt.radius0};
        sm.cost = sm.gmax = sm.xn2_pts = sm.initial_cost = sm.cost_change = sm.step_norm = sm.rel = 0.0;
        sm.it = sm.n_succ = sm.n_unsucc = sm.attempted = sm.term = sm.reason = sm.n_rows = 0;
    }
#define LBA_ROW(i_, c_, ch_, g_, st_, rho_, rad_)                                                             \
    do { if (opt.want_rows && sm.n_rows <= opt.max_it) { LbaRow& w_ = rows[sm.n_rows]; w_.cost = (c_); w_.change = (ch_); w_.gmax = (g_); \
         w_.step = (st_); w_.rho = (rho_); w_.radius = (rad_); w_.it = (i_); w_.pad = 0; ++sm.n_rows; } } while (0)
    // Round 0 linearises without scaling (Jacobi scaling from the unscaled column norms), round 1 at the start, every later
    // round after a step test: one linearisation and at most one step per round, at most max_it steps.
    int go = 1;                              // what the last step test said: 1 the point is new, 2 same point with another radius
    for (int round = 0; round < opt.max_it + 2; ++round) {
        lba_linearize(d, sm, lba_smem, Pcur, opt.huber_a, round == 0 ? 1.0 : sm.radius, round != 0, item, n_items);
        if (round == 0) {
            if (sm.dup) {         // (nothing of the state has been written)
                if (tid == 0) { LbaResult r{}; r.status = 1; *result = r; __threadfence_system(); }
                return;
            }
            if (tid < n) {
                const int c = tid / 6, k = tid % 6;
                const double sc = 1.0 / (1.0 + sqrt(sm.Hcc[tid][k]));
                sm.sc[c][k] = sc;
                sm.scm[c][k] = ((unsigned)sm.cconst[c] & (k < 3 ? 1u : 2u)) ? 0.0 : sc;
            }
            for (int i = tid; i < 3 * d.n_pts; i += kLbaBlock) {
                const int p = i / 3, k = i % 3;
                d.scale_p[i] = 1.0 / (1.0 + sqrt(d.Hpp[6 * (size_t)p + (k == 0 ? 0 : (k == 1 ? 3 : 5))]));
            }
            __syncthreads();
            continue;
        }
        if (go == 1) {                       // a new point: its sm.cost and gradient
            if (tid < nc) lba_cam_gradmax(sm, tid);
            __syncthreads();
            if (tid == 0) {
                sm.cost = 0.5 * sm.tot[0]; sm.xn2_pts = sm.tot[1];
                sm.gmax = sm.tot[2];
                for (int c = 0; c < nc; ++c) sm.gmax = fmax(sm.gmax, sm.cgm[c]);
                if (round == 1) sm.initial_cost = sm.cost;
                LBA_ROW(sm.it, sm.cost, sm.cost_change, sm.gmax, sm.step_norm, sm.rel, sm.tr.radius);
                if (sm.gmax <= opt.gtol) { sm.term = XRSFM_BA_CONVERGENCE; sm.reason = 1; sm.go = 0; }
                else if (sm.it >= opt.max_it) { sm.term = XRSFM_BA_NO_CONVERGENCE; sm.reason = 5; sm.go = 0; }
            }
            __syncthreads();
            if (sm.go == 0) break;
        }
        const double radius = sm.radius;
        lba_factor_solve(sm, lba_smem, n);
        const bool solved = sm.solve_ok != 0;
        if (solved) {
            if (tid < nc) lba_cam_update(sm, tid);
            __syncthreads();
            lba_backsub(d, sm, Pcur, Pcand, opt.huber_a, radius);
        }
        if (tid == 0) {
            ++sm.it; ++sm.attempted;
            const double model = solved ? sm.tot[0] : -1.0;
            if (!(model > 0.0) || !isfinite(model)) {
                ++sm.n_unsucc;
                LBA_ROW(sm.it, sm.cost, 0.0, sm.gmax, 0.0, 0.0, sm.tr.radius);
                if (const int r = sm.tr.invalid_step()) { sm.term = XRSFM_BA_FAILURE; sm.reason = r; sm.go = 0; }
                else sm.go = 2;
            } else {
                sm.tr.invalid = 0;
                double step2c = 0.0, xn2c = 0.0;
                for (int c = 0; c < nc; ++c) { step2c += sm.cstep2[c]; xn2c += sm.cxn2[c]; }
                const double cost_cand = 0.5 * sm.tot[2];
                sm.step_norm = sqrt(sm.tot[1] + step2c);
                const double xnorm = sqrt(sm.xn2_pts + xn2c);
                sm.cost_change = sm.cost - cost_cand;
                if (const int r = xtr::TrustRegion::tolerance_exit(sm.step_norm, xnorm, opt.ptol, sm.cost_change, sm.cost, opt.ftol)) {
                    sm.term = XRSFM_BA_CONVERGENCE; sm.reason = r; sm.go = 0;
                } else {
                    sm.rel = sm.cost_change / model;
                    if (xtr::TrustRegion::successful(sm.rel)) { sm.tr.grow_cubed(sm.rel); ++sm.n_succ; sm.go = 1; }
                    else {
                        const int r = sm.tr.shrink();
                        ++sm.n_unsucc;
                        LBA_ROW(sm.it, sm.cost, sm.cost_change, sm.gmax, sm.step_norm, sm.rel, sm.tr.radius);
                        if (r) { sm.term = XRSFM_BA_CONVERGENCE; sm.reason = r; sm.go = 0; }
                        else sm.go = 2;
                    }
                }
            }
            if (sm.go == 2 && sm.it >= opt.max_it) { sm.term = XRSFM_BA_NO_CONVERGENCE; sm.reason = 5; sm.go = 0; }
            sm.radius = sm.tr.radius;
        }
        __syncthreads();
        go = sm.go;
        if (go == 0) break;
        if (go == 1) {        // the candidate becomes the point
            if (tid < nc) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sm.q[tid][k] = sm.cq[tid][k];
#pragma unroll
                for (int k = 0; k < 3; ++k) sm.t[tid][k] = sm.ct[tid][k];
#pragma unroll
                for (int k = 0; k < 9; ++k) sm.M[tid][k] = sm.cM[tid][k];
            }
            double* tmp = Pcur; Pcur = Pcand; Pcand = tmp;
        }
        __syncthreads();
    }
#undef LBA_ROW
    __syncthreads();
    // the state a run of the engine would have left: cameras and points at the last accepted point
    if (tid < nc) {
        CamRec& c = d.cam[tid];
#pragma unroll
        for (int k = 0; k < 4; ++k) c.q[k] = sm.q[tid][k];
#pragma unroll
        for (int k = 0; k < 3; ++k) c.t[k] = sm.t[tid][k];
    }
    if (Pcur != d.P)
        for (int i = tid; i < 3 * d.n_pts; i += kLbaBlock) d.P[i] = Pcur[i];
    if (tid == 0) {
        LbaResult r{};
        r.initial_cost = sm.initial_cost; r.final_cost = sm.cost;
        r.n_successful = sm.n_succ; r.n_unsuccessful = sm.n_unsucc; r.termination = sm.term; r.reason = sm.reason; r.attempted = sm.attempted;
        r.status = 0; r.n_rows = sm.n_rows;
        *result = r;
        __threadfence_system();
    }
}

__global__ __launch_bounds__(kLbaBlock) void k_lba_resident(LbaDev d, LbaOpt opt, LbaResult* __restrict__ result, LbaRow* __restrict__ rows) {
    __shared__ __attribute__((aligned(16))) double lba_smem[kLbaSmemBytes / 8];        // static: the code object states the whole group segment
    lba_resident_solve(d, opt, result, rows, lba_smem);
}

// N independent problems as N workgroups of one launch (xrsfm_ba_run_batch): workgroup b solves problem p = order[b] (the host's
// permutation by descending tile count, so that the longest start first when the grid exceeds the compute units) with the
// descriptor devs[p], and writes results[p] and, with opt.want_rows, rows[p * rows_stride ...].  A workgroup touches nothing of
// another problem and waits for none: every loop is bounded as in the single launch, whose arithmetic this is instruction for
// instruction.  The descriptor is read once, at a workgroup-uniform address.
__global__ __launch_bounds__(kLbaBlock) void k_lba_batch(const LbaDev* __restrict__ devs, const int* __restrict__ order, LbaOpt opt,
                                                         LbaResult* __restrict__ results, LbaRow* __restrict__ rows, int rows_stride) {
    __shared__ __attribute__((aligned(16))) double lba_smem[kLbaSmemBytes / 8];
    const int p = order[blockIdx.x];
    const LbaDev d = devs[p];
    lba_resident_solve(d, opt, results + p, rows + (size_t)p * (size_t)rows_stride, lba_smem);
}

}  // namespace xba
