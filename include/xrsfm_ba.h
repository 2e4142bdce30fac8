/*
 * xrsfm_ba.h — C-ABI of the MI355X-native bundle-adjustment engine.
 *
 * Drop-in boundary for the global/local BA step of openxrlab/xrsfm.  The
 * reference has no FFI for this path: it is the C++ class xrsfm::BASolver
 * (/root/reference/src/optimization/ba_solver.h:14-30) whose GBA/KGBA/LBA
 * methods build a ceres::Problem out of raw pointers into Map storage
 * (/root/reference/src/optimization/ba_solver.cc:345-347) and call
 * ceres::Solve (ba_solver.cc:591,636,672).  The entry points below are what a
 * binding for that path has to call instead of Ceres: the same parameter
 * blocks, handed over as flat FP64/int32 arrays (caller-owned, results written
 * in place like Ceres does), the same solver options the reference sets
 * (ba_solver.cc:70-77, 586-589, 626-634, 667-670), and a summary carrying the
 * quantities PrintSolverSummary prints (ba_solver.cc:14-68).
 * The source-compatible adapter on top is xrsfm_amd/csrc/compat/.
 *
 * Plain C, no torch / HIP types in any signature.  All functions return 0 on
 * success or a negative XRSFM_BA_E* code; nothing throws across the boundary.
 */
#ifndef XRSFM_BA_H
#define XRSFM_BA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRSFM_BA_VERSION 1

/* error codes */
#define XRSFM_BA_OK 0
#define XRSFM_BA_EINVAL (-1)   /* bad argument / inconsistent indices            */
#define XRSFM_BA_ENODEV (-2)   /* no HIP device, or the HIP runtime reported an error */
#define XRSFM_BA_ENOMEM (-3)
#define XRSFM_BA_ECOMM (-4)    /* RCCL unavailable or a collective failed         */
#define XRSFM_BA_ESTATE (-5)   /* call order violated                            */
#define XRSFM_BA_ETOOBIG (-6)  /* explicit reduced camera matrix requested (CHOLESKY) but it does not fit: use AUTO or PCG */
#define XRSFM_BA_EINTERNAL (-7) /* an unexpected C++ exception was stopped at the boundary (never the termination code +2) */
#define XRSFM_BA_ESINGULAR (-8) /* S(0) is not positive definite: gauge not fixed, a selected camera is unobserved, or a free point's undamped block is singular */

/* camera models: ids of /root/reference/src/base/camera_model.hpp:93-209 */
#define XRSFM_BA_SIMPLE_PINHOLE 0 /* {f,cx,cy}             uv = 2f*xn + c (reference quirk, :102-105) */
#define XRSFM_BA_PINHOLE 1        /* {fx,fy,cx,cy}         same quirk (:121-124)                       */
#define XRSFM_BA_SIMPLE_RADIAL 2  /* {f,cx,cy,k}                                                      */
#define XRSFM_BA_RADIAL 3         /* {fx,fy,cx,cy,k}       single k (:155-177)                         */
#define XRSFM_BA_OPENCV 4         /* {fx,fy,cx,cy,k1,k2,p1,p2}                                         */

/* cam_const bits: which parameter blocks of a frame are held constant
 * (problem.SetParameterBlockConstant, ba_solver.cc:611-621) */
#define XRSFM_BA_CONST_Q 1u
#define XRSFM_BA_CONST_T 2u
/* bal9 mode (BASELINE.json north_star "2x9 camera blocks") — NOT something the reference does: it
 * always holds the intrinsics block of ReProjectionCost (cost_factor_ceres.h:42-46, kNumParams) constant (ba_solver.cc:
 * 602-606, 655-659, 389).  A camera with this bit keeps its intrinsics VARIABLE and contributes a 9-wide block {rotation 3,
 * translation 3, f, k1, k2}.  Requirements (XRSFM_BA_EINVAL otherwise): camera model 5 below, one intrinsics entry per such
 * camera; exact solver on one rank.  The refined {f, k1, k2} come back in problem->intr_params (xrsfm_ba_solve) /
 * xrsfm_ba_download_intrinsics.  The adapter never sets it. */
#define XRSFM_BA_INTR_VARIABLE 4u
/* Camera models: 0..4 = the reference's (camera_model.hpp:93-209); 5 = extension for BAL-style problems: params {f, k1, k2},
 * no principal point, uv = f (1 + k1 r^2 + k2 r^4) xy with the reference's sign convention xy = pc.hnormalized(). */
#define XRSFM_BA_MODEL_BAL 5

/* One BA call = one ceres::Problem of the reference (ba_solver.cc:596,645,536).
 * Observation order is free (the reference's is frame-major, ba_solver.cc:598-601). */
typedef struct xrsfm_ba_problem {
    int32_t n_cams;   /* frames added by SetUp/SetUpLBA (ba_solver.cc:330-391)          */
    int32_t n_points; /* tracks referenced by those frames                             */
    int32_t n_obs;    /* residual blocks = ReProjectionCost instances                  */
    int32_t n_intr;   /* distinct camera_id's (intrinsics always constant, :602-606)   */
    double *cam_q;              /* [n_cams][4]  Tcw.q.coeffs() = x,y,z,w   in/out        */
    double *cam_t;              /* [n_cams][3]  Tcw.t                      in/out        */
    const uint8_t *cam_const;   /* [n_cams]     XRSFM_BA_CONST_* bits, NULL = all free   */
    const int32_t *cam_intr;    /* [n_cams]     index into intr_*                        */
    const int32_t *intr_model;  /* [n_intr]     XRSFM_BA_<MODEL>                         */
    double *intr_params;        /* [n_intr][8]  camera.params_ (zero padded); read only, except in bal9 mode (XRSFM_BA_INTR_VARIABLE): in/out */
    double *points;             /* [n_points][3] track.point3d_            in/out        */
    const uint8_t *point_const; /* [n_points]   non-zero = constant (SetUpLBA :380-382), NULL = all free */
    const int32_t *obs_cam;     /* [n_obs] */
    const int32_t *obs_pt;      /* [n_obs] */
    const double *obs_uv;       /* [n_obs][2]   frame.points[i]                          */
} xrsfm_ba_problem;

#define XRSFM_BA_SOLVER_PCG 0      /* implicit-Schur PCG on the reduced camera system (any size)            */
#define XRSFM_BA_SOLVER_CHOLESKY 1 /* explicit reduced camera matrix + tile Cholesky (exact, what Ceres SPARSE_SCHUR
                                      computes).  Any camera graph up to 6*n_cams <= 12288; beyond that only band /
                                      ring graphs (sequential data: shallow elimination tree) while the tile storage
                                      fits (XRSFM_BA_ETOOBIG otherwise)                                      */
#define XRSFM_BA_SOLVER_AUTO 2     /* CHOLESKY whenever the rule above allows it, else PCG                  */
#define XRSFM_BA_SOLVER_RESIDENT 3 /* the whole LM loop in ONE kernel launch of one workgroup (ba_lba.h): linearisation,
                                      damped point blocks, reduced camera system, its Cholesky factorisation and solve,
                                      back-substitution, candidate cost, step test, radius update and the tolerance
                                      exits all run on the device; the host passes the options with the launch and
                                      reads one result block (summary fields and, with verbose, the iteration rows)
                                      back.  The same restated Ceres loop and the same exact reduced system as
                                      _CHOLESKY, for local-BA-sized problems.  Opt-in only: AUTO never selects it.
                                      Eligibility (else XRSFM_BA_EINVAL, one line on stderr, state untouched):
                                      a 6-wide context (not bal9 mode); one rank (no communicator, no test hook);
                                      n_cams <= 10 (the reduced system is one 64x64 tile: what
                                      xrsfm_ba_debug_chol_plan reports as stats[0] == 1); no track observed twice by
                                      one camera (as for _CHOLESKY); n_obs <= 32768 (one compute unit streams the
                                      observations three times per LM step).  Measured (profiles/lba_resident.md):
                                      same result as _CHOLESKY to 1e-11, but 9-38 x SLOWER per call at 6000-30000
                                      observations: a cross-check and a base for further work, not a fast path.  After the call the context holds what a _CHOLESKY run
                                      would have left: download, reset, a further run with any solver and the
                                      covariance calls work on it unchanged.  profile != 0: xrsfm_ba_profile_entry
                                      lists k_lba_resident with one launch and no other kernel                    */

typedef struct xrsfm_ba_options {
    int32_t max_iterations;      /* GBA accurate 50 / fast 20 / KGBA 20 / LBA 5        */
    double function_tolerance;   /* 1e-5 / 1e-4                                       */
    double parameter_tolerance;  /* 1e-6 / 1e-5                                       */
    double gradient_tolerance;   /* Ceres default 1e-10                               */
    double initial_radius;       /* Ceres default 1e4, KGBA 1e6 (ba_solver.cc:667)    */
    double huber_a;              /* 5.99 (ba_solver.cc:343,374)                       */
    int32_t linear_solver;       /* XRSFM_BA_SOLVER_*                                 */
    double pcg_tolerance;        /* |r|_2 <= tol*|b|_2; 1e-12 follows the exact solve */
    int32_t pcg_max_iterations;
    int32_t profile;             /* !=0: HIP-event timing of the dominant kernel      */
    int32_t verbose;             /* !=0: Ceres-style progress table on stdout         */
} xrsfm_ba_options;

/* termination codes (ceres::TerminationType as printed by ba_solver.cc:41-66) */
#define XRSFM_BA_CONVERGENCE 0
#define XRSFM_BA_NO_CONVERGENCE 1
#define XRSFM_BA_FAILURE 2

typedef struct xrsfm_ba_summary {
    double initial_cost;   /* 1/2 sum rho(|r|^2) at entry                              */
    double final_cost;     /* ... at the last accepted state                           */
    int32_t num_residuals;          /* num_residuals_reduced = 2*n_obs                 */
    int32_t num_effective_params;   /* num_effective_parameters_reduced                */
    int32_t n_successful;           /* LM steps accepted.  Iteration 0 (the evaluation at the initial point) is NOT counted: a RECALLED
                                       detail of Ceres' num_successful_steps (UNPINNED, oracle/ba_oracle.py ALT_DETAILS
                                       "iteration_zero_counted"): if Ceres counts it, the reference's "Iterations :" line
                                       (ba_solver.cc:22-25) reads one more than n_successful + n_unsuccessful here */
    int32_t n_unsuccessful;         /* LM steps rejected or invalid                    */
    int32_t termination;            /* XRSFM_BA_CONVERGENCE / ...                      */
    int32_t termination_reason;     /* 1 gradient, 2 parameter, 3 function tolerance, 4 min radius, 5 max iterations, 6 invalid steps */
    int32_t pcg_iterations;         /* total over all LM steps                         */
    int32_t lm_steps_attempted;     /* incl. the step that triggered a tolerance exit  */
    double total_time_s;            /* wall time of the solve, device-resident inputs  */
    double dom_kernel_ms;           /* profile!=0: sum of HIP-event durations of the costliest kernel */
    int32_t dom_kernel_launches;    /* profile!=0: launches counted in dom_kernel_ms   */
    int32_t dom_kernel_id;          /* profile!=0: index for xrsfm_ba_profile_entry    */
    int32_t linear_solver_used;     /* XRSFM_BA_SOLVER_PCG, _CHOLESKY or _RESIDENT     */
    int32_t reserved;
} xrsfm_ba_summary;

typedef struct xrsfm_ba_context xrsfm_ba_context; /* opaque: device buffers, stream, communicator */

/* Fill `opt` with the reference's GBA(accurate=true) settings + Ceres defaults. */
void xrsfm_ba_default_options(xrsfm_ba_options *opt);

/* Library / device probe: returns XRSFM_BA_VERSION, *n_devices = visible HIP devices (0 if none). */
int xrsfm_ba_version(int *n_devices);

/* Optional: pay the one-off costs of the first call of a process NOW — HIP runtime start-up, loading the library's code
 * object, a stream with its pinned scalar block, the kernels' dynamic-LDS attributes and, with n_obs_hint > 0, the device
 * buffers of a problem of about that many observations / n_points_hint points / n_cams_hint cameras (they go to the
 * allocation cache the next xrsfm_ba_create draws from; capped at a quarter of the device memory that is free at the time of
 * the call).  The adapter calls it from BASolver's constructor (the reference
 * pays the equivalent when ceres::Problem is first used).  Returns XRSFM_BA_ENODEV without a device; never required. */
int xrsfm_ba_warmup(int device, int64_t n_obs_hint, int64_t n_points_hint, int64_t n_cams_hint);

/* Build a device-resident problem on HIP device `device`: validates indices,
 * orders tracks, uploads everything.  The host arrays are only read. */
int xrsfm_ba_create(const xrsfm_ba_problem *problem, int device, xrsfm_ba_context **out);

/* Multi-GPU (points sharded by rank, cameras replicated): attach an RCCL
 * communicator.  `unique_id` is the 128-byte ncclUniqueId obtained from
 * xrsfm_ba_comm_unique_id on rank 0 and distributed by the caller. */
int xrsfm_ba_comm_unique_id(unsigned char id[128]);
int xrsfm_ba_comm_init(xrsfm_ba_context *ctx, int n_ranks, int rank, const unsigned char id[128]);
/* Watchdog of multi-rank contexts (environment XRSFM_BA_WATCHDOG_S = seconds, default 300 with several ranks and OFF on one
 * rank; an explicit value applies to every context, 0 switches it off): a rank that waits that long for its device without
 * progress — an all-reduce a peer never joined — gets XRSFM_BA_ECOMM (XRSFM_BA_ENODEV on one rank) from xrsfm_ba_run.  The
 * context is then POISONED: run / reset / download return XRSFM_BA_ESTATE, and xrsfm_ba_destroy aborts the communicator and
 * releases the host side only (the stream and the device buffers the stuck work may still touch are leaked on purpose, never
 * waited for). */

/* TEST HOOK: replace the RCCL all-reduce of this context by a caller-supplied one working on a HOST copy of the buffer
 * (op 0 = sum, 1 = max; return 0 on success).  Lets several ranks share ONE GPU — RCCL refuses two ranks on one device — so the
 * multi-rank logic (sharded points, replicated cameras, union block pattern, identical LM decisions on every rank) can be
 * verified on a 1-GPU box with any host transport (the tests use torch.distributed/gloo).  Not a production path. */
typedef int (*xrsfm_ba_allreduce_fn)(void *user, double *host_buf, uint64_t n, int op);
int xrsfm_ba_debug_comm_hook(xrsfm_ba_context *ctx, int n_ranks, int rank, xrsfm_ba_allreduce_fn fn, void *user);

/* Run Levenberg-Marquardt on the device-resident state (blocking). */
int xrsfm_ba_run(xrsfm_ba_context *ctx, const xrsfm_ba_options *opt, xrsfm_ba_summary *summary);

/* Restore the device-resident state to the values uploaded by xrsfm_ba_create. */
int xrsfm_ba_reset(xrsfm_ba_context *ctx);

/* Copy the current state back into caller arrays laid out like the problem
 * (cam_q [n_cams][4], cam_t [n_cams][3], points [n_points][3]); NULL skips one. */
int xrsfm_ba_download(xrsfm_ba_context *ctx, double *cam_q, double *cam_t, double *points);

/* bal9 mode: intrinsics {f, k1, k2} of the cameras with XRSFM_BA_INTR_VARIABLE into intr_params [n_intr][8] (other rows and
 * columns untouched); a no-op for ordinary problems. */
int xrsfm_ba_download_intrinsics(xrsfm_ba_context *ctx, double *intr_params);

/* Marginal covariance of selected cameras at the CURRENT device state (after create, run or reset):
 * block (c,c) of (J^T J)^-1 with J the robustified Jacobian (Huber huber_a) in the tangent space of the
 * library's Plus (rotation 3, translation 3: the order of debug_linearize's Jc columns), UNSCALED
 * coordinates, no damping, no sigma^2 factor: what ceres::Covariance::GetCovarianceBlockInTangentSpace
 * returns for (q,t) of one frame.  cov [n_sel][6][6] row-major, symmetric.  Rows/columns of a constant
 * block (XRSFM_BA_CONST_Q / _T) are zero.  Does not change the state or the trust region of a later run.
 *
 * How: the state is linearised like the first iteration of a run (Jacobi scaling), the reduced camera matrix S is assembled
 * with the damping an explicit ZERO (the point blocks are inverted undamped, all-zero rows of constant blocks get a unit
 * diagonal) and factored by the tile Cholesky of XRSFM_BA_SOLVER_CHOLESKY.  With Z_c = L^-1 E_c (E_c: the 6 unit columns of
 * camera c) the block is D_c Z_c^T Z_c D_c, D_c the Jacobi scale: a forward substitution with a 64-column panel (10 cameras)
 * through the level-scheduled factor, dense or packed tile storage (xrsfm_amd/csrc/ba_cov.h), restricted to the tile columns the
 * selected cameras reach in the elimination tree.  Plans on a panel / look-ahead panel schedule (xrsfm_ba_debug_chol_plan
 * stats[6] bit 0 clear, more than one tile column) take a slow exact fallback instead: S x = e_j for the 6 unit vectors of each
 * camera with the run path's factor-and-solve, 6 factorisations per camera; XRSFM_BA_COV_FALLBACK=1 (environment, read per call)
 * forces it everywhere (A/B check of the panel kernel).  The result does not depend on the order of cam_sel, and on the kernel
 * path a camera's block is bit-identical whatever else is selected with it.
 *
 * Errors: XRSFM_BA_EINVAL — index out of range, duplicate in cam_sel, n_sel < 0, NULL cam_sel / cov with n_sel > 0, bal9 context,
 * multi-rank context (communicator or test hook), a track observed twice by one camera; XRSFM_BA_ETOOBIG exactly where
 * XRSFM_BA_SOLVER_CHOLESKY returns it (there is no PCG variant); XRSFM_BA_ESINGULAR — a selected camera has no observation, a
 * free point's undamped 3x3 block is singular (a track of one observation), or the factorisation met a non-positive pivot
 * (recognised like an invalid step of a run: the solution of the factored system is not finite), or a block would hold a NaN / Inf
 * (a nearly singular S whose Z^T Z overflows).  The result is staged and checked before it is copied: on every error code cov is
 * left UNTOUCHED, it never receives a NaN or an Inf.  A singular point block is named on stderr (how many, and the first one's
 * index).  n_sel == 0 is success and touches nothing.
 * Cross blocks between cameras (and between cameras and points): xrsfm_ba_joint_covariance.  Every camera of the map at once:
 * xrsfm_ba_map_covariance.  Not built: bal9, several ranks, a PCG variant. */
int xrsfm_ba_covariance(xrsfm_ba_context *ctx, double huber_a, int32_t n_sel, const int32_t *cam_sel, double *cov);

/* Marginal covariance of selected 3-D points at the CURRENT device state: block (p,p) of (J^T J)^-1 with the conventions of
 * xrsfm_ba_covariance (robustified J, UNSCALED coordinates, no damping, no sigma^2 factor): what
 * ceres::Covariance::GetCovarianceBlock returns for one track's point3d_.  pt_sel holds the caller's point indices,
 * cov [n_sel][3][3] row-major, exactly symmetric.  A constant point (point_const) gets an all-zero block; a point whose observing
 * cameras are all constant gets exactly D_p Hinv_p D_p.  Does not change the state or the trust region of a later run.
 *
 * How: the front half of xrsfm_ba_covariance (linearisation with Jacobi scaling, undamped point inverses Hinv_p, undamped S = L L^T
 * by the tile Cholesky).  With W_p = sum_obs F_c^T E_p the 6 n_cams x 3 block column of the point (non-zero on the rows of the
 * cameras that observe it, zero on constant blocks) the block is
 *     D_p (Hinv_p + Y_p^T Y_p) D_p,   Y_p = L^-1 (W_p Hinv_p),   D_p the Jacobi scale of the point:
 * one streaming pass over the observations forms the 6x3 blocks F_c^T E_p Hinv_p of the selected points, they are scattered into
 * a 64-column right-hand-side panel (3 columns per point, 21 points per chunk) and go through the level-scheduled forward
 * substitution of the camera call with a general right-hand side (xrsfm_amd/csrc/ba_cov.h), restricted to the tile columns of the
 * cameras that observe a point of the chunk and their ancestors in the elimination tree; no backward pass.  Panel / look-ahead
 * panel plans and XRSFM_BA_COV_FALLBACK=1 take the slow exact fallback: per point and column b one factor-and-solve S x_b = w_b
 * (w_b: column b of W_p Hinv_p), Sigma_ab = Hinv_ab + w_a^T x_b, symmetrised: 3 factorisations per point.  The result does not
 * depend on the order of pt_sel, on the kernel path a point's block is bit-identical whatever else is selected with it, and two
 * calls agree bit for bit.
 *
 * Errors: XRSFM_BA_EINVAL — index out of range, duplicate in pt_sel, n_sel < 0, NULL pt_sel / cov with n_sel > 0, bal9 context,
 * multi-rank context (communicator or test hook), a track observed twice by one camera; XRSFM_BA_ETOOBIG exactly where
 * XRSFM_BA_SOLVER_CHOLESKY returns it; XRSFM_BA_ESINGULAR — a selected point has no observation in the program (constant or not:
 * it is not part of it), ANY free point's undamped 3x3 block is singular (named on stderr like the camera call does), the solution
 * of the factored system is not finite, or a block would hold a NaN / Inf.  The result is staged: on every error code cov is left
 * UNTOUCHED.  n_sel == 0 is success and touches nothing.
 * Cross blocks between points (and between cameras and points): xrsfm_ba_joint_covariance.  Every point of the map at once:
 * xrsfm_ba_map_covariance.  Not built: bal9, several ranks, a PCG variant. */
int xrsfm_ba_point_covariance(xrsfm_ba_context *ctx, double huber_a, int32_t n_sel, const int32_t *pt_sel, double *cov);

/* Joint covariance of selected cameras AND points with every cross block: the sub-matrix of (J^T J)^-1 on the selected parameter
 * blocks, in the conventions of the two calls above (robustified J with Huber huber_a, tangent space of the cameras, UNSCALED
 * coordinates, no damping, no sigma^2 factor, current device state): what ceres::Covariance::Compute with every pair of the selected
 * blocks followed by GetCovarianceBlock[InTangentSpace] returns.  cov is [N][N] row-major, N = 6 n_cam_sel + 3 n_pt_sel: the
 * cameras first, in the order of cam_sel (rotation 3, translation 3), then the points in the order of pt_sel (the caller's point
 * indices).  Rows and columns of constant degrees of freedom (XRSFM_BA_CONST_Q / _T, point_const) are exact zeros; a point whose
 * observing cameras are all constant has exact zero cross blocks and the diagonal block D_p Hinv_p D_p.  The result is exactly
 * symmetric (cov[i][j] == cov[j][i] bit for bit).  Does not change the state or the trust region of a later run.
 *
 * How: the front half of the two calls above, once.  In its Jacobi-scaled coordinates, with S = L L^T undamped,
 *     X_c = L^-1 E_c (the 6 unit columns of a camera),   X_p = L^-1 (W_p Hinv_p) (the 3 columns of the point call),
 *     Sigma_cc' = X_c^T X_c',   Sigma_cp = -X_c^T X_p,   Sigma_pp' = delta_pp' Hinv_p + X_p^T X_p',
 * each entry times the Jacobi scales of its row and of its column: forward substitutions only.  The selection is cut into 64-column
 * chunks (10 cameras, or 21 free points), every chunk runs the level-scheduled forward substitution of the calls above into panel
 * storage of its own, and one workgroup per chunk pair forms the Gram between the two panels on the FP64 matrix cores, one 64x64x64
 * product per tile column both chunks reach, in ascending elimination order (xrsfm_amd/csrc/ba_cov.h: k_cov_joint_gram); an
 * epilogue applies signs, Hinv_p and scales, writes the upper triangle in the caller's order and copies it into the lower.  An
 * entry depends on its two columns only: on the kernel path it is bit-identical whatever else is selected and in whatever order,
 * and two calls agree bit for bit.  Panel / look-ahead panel plans and XRSFM_BA_COV_FALLBACK=1 (read per call) take the slow exact
 * fallback: one factor-and-solve S x = rhs per free selected column (N factorisations), the entries assembled from the rows of x
 * with the same signs and scales, symmetrised.
 *
 * Size: N <= XRSFM_BA_JOINT_COV_MAX_COLS.  Device scratch of one call: 32 KiB per chunk and reached tile column for the panels plus
 * 32 KiB per chunk pair and 8 N^2 bytes for the result.  At the cap (18 chunks at most, 171 pairs) on bench config L (112 tile
 * columns) that is at most 63 MiB + 5.4 MiB + 8 MiB whatever the selection reaches; XRSFM_BA_ENOMEM if the device cannot give it.
 *
 * Errors: XRSFM_BA_EINVAL — NULL context, an index out of range, a duplicate within cam_sel or within pt_sel, a negative count, a
 * NULL selection with a positive count, NULL cov with N > 0, N above the cap, bal9 context, multi-rank context (communicator or
 * test hook), a track observed twice by one camera; XRSFM_BA_ETOOBIG exactly where XRSFM_BA_SOLVER_CHOLESKY returns it;
 * XRSFM_BA_ESINGULAR — a selected camera has no observation, a selected point has no observation in the program, ANY free point's
 * undamped 3x3 block is singular (named on stderr like the calls above), the solution of the factored system is not finite, or the
 * result would hold a NaN / Inf.  The result is staged and checked: on every error code cov is left UNTOUCHED.  N == 0 is success
 * and touches nothing; either count may be zero on its own.
 * The marginal blocks of the WHOLE map (no cross blocks): xrsfm_ba_map_covariance.
 * Not built: bal9, several ranks, a PCG variant, a kernel path on panel plans. */
#define XRSFM_BA_JOINT_COV_MAX_COLS 1024
int xrsfm_ba_joint_covariance(xrsfm_ba_context *ctx, double huber_a, int32_t n_cam_sel, const int32_t *cam_sel, int32_t n_pt_sel,
                              const int32_t *pt_sel, double *cov);

/* Marginal covariance of EVERY camera and EVERY point of the map in one call: the diagonal blocks of (J^T J)^-1 with the conventions
 * of the three calls above (current device state, robustified J with Huber huber_a, tangent space of the library's Plus for the
 * cameras: rotation 3, translation 3, UNSCALED coordinates, no damping, no sigma^2 factor).  cam_cov [n_cams][6][6] and
 * pt_cov [n_points][3][3] row-major, rows in the caller's indexing whatever the packing did to it; every block is exactly
 * symmetric, constant degrees of freedom give exact zero rows and columns.  Any of the four outputs may be NULL.
 * cam_status [n_cams] / pt_status [n_points]:
 *     0  estimated,
 *     1  every degree of freedom constant (zero block),
 *     2  not in the program (zero block): a camera without an observation, a point without one.  The selected calls return
 *        ESINGULAR there because the caller asked for that block; this call has no selection and reports the case instead.
 * Does not change the state or the trust region of a later run.
 *
 * How: the front half of the calls above, once (S = L L^T undamped, in Jacobi-scaled coordinates).  With Z = S^-1,
 *     Sigma_pp = Hinv_p + sum over the observers c, c' of p:  V_c^T Z_cc' V_c',    V_c = F_c^T E_p Hinv_p  (6x3),
 * needs only the 6x6 blocks Z_cc' of camera pairs that observe a common point: the structurally non-zero blocks of S, hence
 * entries of S^-1 on the pattern of the factor, and the diagonal blocks Z_cc are the camera covariances.  The Takahashi recurrence
 * forms exactly these entries from L (SELECTED INVERSION, xrsfm_amd/csrc/ba_cov.h: k_selinv_off / k_selinv_diag): with I_k the
 * rows of the off-diagonal tiles of tile column k,
 *     Z_ik = -(sum_{m in I_k} Z_im L_mk) Linv_k   (i in I_k),      Z_kk = Linv_k^T (Linv_k - sum_{m in I_k} L_mk^T Z_mk),
 * the levels of the elimination tree from the root down, two launches per level, one workgroup per tile, 64x64x64 products on the
 * FP64 matrix cores, m ascending (two calls agree bit for bit).  Z lives in a SECOND tile storage with the factor's own layout,
 * dense or packed (as many bytes as the factor: xrsfm_ba_device_memory's tile storage once more for the duration of the call;
 * XRSFM_BA_ENOMEM if the device cannot give it); dense and packed tiles give bit-identical results.  One streaming pass over
 * the packed tracks then forms the point blocks (k_cov_map_points: one wave per point, lane = observation, the track's V_c in LDS,
 * the pairs in a fixed order; one workgroup per track of more than 64 slots), looking Z_cc' up through the cameras' elimination
 * rows, and the camera blocks are D_c Z_cc D_c.  Cost: about two factorisations plus that pass, against one forward
 * substitution per 21 points of xrsfm_ba_point_covariance.
 * Panel / look-ahead panel plans and XRSFM_BA_COV_FALLBACK=1 (read per call) take the fallback: xrsfm_ba_covariance and
 * xrsfm_ba_point_covariance with everything that is in the program selected (slow, exact: the A/B oracle of the kernels).
 *
 * Errors: XRSFM_BA_EINVAL — NULL context, bal9 context, multi-rank context (communicator or test hook), a track observed twice by
 * one camera; XRSFM_BA_ESTATE — poisoned context; XRSFM_BA_ETOOBIG exactly where XRSFM_BA_SOLVER_CHOLESKY returns it;
 * XRSFM_BA_ENOMEM — the second tile storage does not fit; XRSFM_BA_ESINGULAR — ANY free point's undamped 3x3 block is singular
 * (named on stderr like the calls above), the solution of the factored system is not finite, or the result would hold a NaN / Inf.
 * The result is staged and checked: on every error code all four outputs are left UNTOUCHED.  All four pointers NULL is success
 * and touches nothing.
 * Not built: cross blocks of the whole map (xrsfm_ba_joint_covariance has them for a selection), bal9, several ranks, a PCG
 * variant, a kernel path on panel plans, an adapter method, any use inside the LM loop. */
int xrsfm_ba_map_covariance(xrsfm_ba_context *ctx, double huber_a, double *cam_cov, double *pt_cov, uint8_t *cam_status,
                            uint8_t *pt_status);

void xrsfm_ba_destroy(xrsfm_ba_context *ctx);

/* The library keeps process-wide caches between calls (the reference builds a fresh ceres::Problem per call,
 * ba_solver.cc:596,645,536; BASolver::LBA runs once per registered frame): device blocks and streams returned by
 * xrsfm_ba_destroy, and — for contexts above 200k observations — the release of their host arrays on one library-owned
 * thread.  xrsfm_ba_quiesce() waits for every deferred release and frees the cached device memory; it also returns the
 * bytes that were cached (device) through *cached_bytes (may be NULL).  Never required for correctness: the thread is joined
 * when the library is unloaded (dlclose / process exit), so no library code runs after the unload; cached device blocks
 * that were not released through this call stay with the process until it exits (the library does not call into the HIP
 * runtime from a static destructor).  An embedder that dlcloses the library should call this first. */
int xrsfm_ba_quiesce(uint64_t *cached_bytes);

/* Free and total memory of HIP device `device` as the runtime reports them (hipMemGetInfo): for embedders that watch the
 * footprint of a long mapping session (tests/test_mapper_replay.py asserts that replaying a reconstruction twice leaves it
 * unchanged).  XRSFM_BA_ENODEV without a device. */
int xrsfm_ba_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* One-shot convenience = create + run + download into problem->{cam_q,cam_t,points} + destroy:
 * the call that replaces ceres::Solve(options, &problem, &summary). */
int xrsfm_ba_solve(const xrsfm_ba_options *opt, xrsfm_ba_problem *problem, xrsfm_ba_summary *summary);

/* Many local-BA-sized problems in ONE launch: every context of ctxs [n_ctx] gets exactly the result (bit for bit: state and every
 * summary field but the times) of its own xrsfm_ba_run with XRSFM_BA_SOLVER_RESIDENT, whatever its position in the batch and
 * whatever else is in it: windows of a trajectory after a loop correction, the sub-maps of a partitioned reconstruction, the
 * candidates of a local BA.  One `opt` for the whole batch; opt->linear_solver must be XRSFM_BA_SOLVER_RESIDENT.
 * summaries [n_ctx]: filled like xrsfm_ba_run fills them; total_time_s is the wall time of the whole call, the same value in every
 * summary; with profile != 0 dom_kernel_ms is the HIP-event time of the one launch and dom_kernel_launches is 1, and
 * xrsfm_ba_profile_entry of the FIRST context lists k_lba_resident with that one launch (the other contexts list nothing).
 * codes [n_ctx] (may be NULL): 0, or XRSFM_BA_EINVAL for a problem the kernel refused (below).  With verbose != 0 the progress
 * tables are printed one after another in index order, each under a line "problem <index>".
 *
 * How: the resident kernel has one workgroup and nothing in it waits for another, so N problems are N workgroups of one grid
 * (xrsfm_amd/csrc/ba_lba.h: k_lba_batch): no protocol between workgroups, no floating-point atomics, every loop bounded as in the
 * single launch.  The contexts' streams are drained; the kernel's descriptors of the contexts and the launch order (problems by
 * descending tile count, ties by index: with more problems than compute units the longest start first) are uploaded from one
 * pinned block; one launch on the first context's stream; one pinned block of results (and, with verbose, iteration rows) is read
 * back.  One workgroup occupies one compute unit (157.6 KiB of LDS): a batch is as fast as its longest problem up to 256 problems
 * on an MI355X and proceeds in waves beyond.  Afterwards every context holds what a _CHOLESKY run would have left: download,
 * reset, a further run with any solver and the covariance calls work on it unchanged.  Measured against n_ctx sequential _CHOLESKY
 * runs on the same contexts (profiles/lba_batch.md): 7 cameras / 6000 observations: 3.9 against 5.9 ms at 16 problems, 4.2 against
 * 92.9 ms at 256, 16.3 against 359 ms at 1024 (22 x); 5 cameras / 600 observations: 0.52 against 5.0 ms at 16, 0.72 against 82.9 ms
 * at 256 (115 x); crossover near 11 and 2 problems.  A batch of ONE is XRSFM_BA_SOLVER_RESIDENT again: slower than the engine.
 *
 * Errors, checked before anything is launched or written (one line on stderr naming the first offending index; every context's
 * state, summaries and codes stay untouched): XRSFM_BA_EINVAL — n_ctx < 0 or above XRSFM_BA_BATCH_MAX, a NULL ctxs / opt /
 * summaries with n_ctx > 0, another linear_solver, a NULL entry, the same context twice, contexts on different devices, a context
 * XRSFM_BA_SOLVER_RESIDENT refuses (bal9, communicator or test hook, more than 10 cameras, more than 32768 observations, negative
 * max_iterations); XRSFM_BA_ESTATE — a poisoned context.  n_ctx == 0 is success, touches nothing, needs no device and is checked
 * first.  Found by the kernel: a track observed twice by one camera — before anything of THAT problem's state is written; it gets
 * codes[i] = XRSFM_BA_EINVAL and an all-zero summary, its state stays untouched, the other problems are solved, and the call
 * returns XRSFM_BA_EINVAL: the batch is then PARTLY ADVANCED, and codes says where (pass it whenever a duplicate observation is
 * possible).  XRSFM_BA_ENODEV: the HIP runtime reported an error; XRSFM_BA_ENOMEM: no staging memory.
 * Not built: per-problem options, an adapter method, contexts on several devices, bal9. */
#define XRSFM_BA_BATCH_MAX 4096
int xrsfm_ba_run_batch(int32_t n_ctx, xrsfm_ba_context *const *ctxs, const xrsfm_ba_options *opt,
                       xrsfm_ba_summary *summaries /* [n_ctx] */, int32_t *codes /* [n_ctx], may be NULL */);
/* One-shot convenience = xrsfm_ba_create for each problem (device 0) + xrsfm_ba_run_batch + xrsfm_ba_download into each problem's
 * {cam_q, cam_t, points} + destroy.  A problem whose create fails (codes[i] = that code, summary zeroed) or that the kernel refuses
 * (codes[i] = XRSFM_BA_EINVAL) keeps its arrays untouched while the others are solved; the call then returns the first such code.
 * On a failing host check of xrsfm_ba_run_batch no array, summary or code of any problem is touched. */
int xrsfm_ba_solve_batch(const xrsfm_ba_options *opt, int32_t n_problems, xrsfm_ba_problem *problems,
                         xrsfm_ba_summary *summaries /* [n_problems] */, int32_t *codes /* [n_problems], may be NULL */);

/* Pose-only refinement of one frame against fixed 3-D points: the "pose estimate [refine]" block of RegisterImage
 * (/root/reference/src/geometry/pnp.cc:38-71): one ReProjectionCost + HuberLoss(5.99) per inlier correspondence, points
 * and intrinsics constant, EigenQuaternionParameterization on q, ceres::Solver::Options defaults with
 * max_num_iterations = 10.  xrsfm_ba_refine_pose_options fills exactly those settings (function_tolerance 1e-6,
 * parameter_tolerance 1e-8, gradient_tolerance 1e-10, initial radius 1e4).
 *   model, intr_params[8]   camera model id 0..4 and its parameters (unused tail ignored)
 *   points3d [n][3], uv [n][2], inlier_mask [n] (NULL = all inliers; only non-zero entries enter, like pnp.cc:43-45)
 *   q[4] (x,y,z,w), t[3]    in: the RANSAC pose; out: the refined pose
 * summary->initial_cost / final_cost with num_residuals give the two "[px]" values the reference prints (pnp.cc:63-70).
 * One persistent workgroup runs the whole LM loop on the device (xrsfm_amd/csrc/ba_refine.h: normal equations by block reduction,
 * 6x6 damped solve and trust-region bookkeeping on one lane, candidate linearised in the pass that yields its cost): one
 * upload, one launch, one read-back, ~0.12 ms per call.  Same arithmetic and loop semantics as xrsfm_ba_solve on the
 * one-camera problem, which stays available as the cross-check (environment variable XRSFM_BA_REFINE_ENGINE=1). */
void xrsfm_ba_refine_pose_options(xrsfm_ba_options *opt);
int xrsfm_ba_refine_pose(const xrsfm_ba_options *opt, int32_t model, const double *intr_params, int32_t n,
                         const double *points3d, const double *uv, const uint8_t *inlier_mask, double *q, double *t,
                         xrsfm_ba_summary *summary);
/* The same for several frames in one upload / launch / read-back (one workgroup per frame): e.g. the candidate next frames of
 * incremental_mapper.cc:41-46 or the frames of a loop correction.  Frame f owns the correspondences corr_ptr[f] ..
 * corr_ptr[f+1] of the concatenated arrays (corr_ptr[0] = 0); models [n_frames], intr_params [n_frames][8], q [n_frames][4],
 * t [n_frames][3], summaries [n_frames].  Every frame gets exactly the result of its own xrsfm_ba_refine_pose call. */
int xrsfm_ba_refine_poses(const xrsfm_ba_options *opt, int32_t n_frames, const int32_t *models, const double *intr_params,
                          const int32_t *corr_ptr, const double *points3d, const double *uv, const uint8_t *inlier_mask,
                          double *q, double *t, xrsfm_ba_summary *summaries);

/* ---- Scaled pose graph of BASolver::ScalePoseGraphUnorder (/root/reference/src/optimization/ba_solver.cc:147-328; SURVEY 8f
 * row f4).  HOST code (O(frames) unknowns; no GPU needed or used): it completes the BASolver interface without Ceres.
 * Poses are T_wc (twc_vec of the reference).  Rotations are constant (ba_solver.cc:248-249), positions and scales are the
 * unknowns.  An edge is one PoseGraphCost(q_mea, p_mea, weight_o) residual block (cost_factor_ceres.h:117-198) between
 * pose1 = frame edge_a (scale edge_sa) and pose2 = frame edge_b (scale edge_sb); a scale cost is one ScaleCost(s12)
 * (cost_factor_ceres.h:200-221).  n_scales >= n_frames: scale i < n_frames belongs to frame i, the rest are the loop
 * scales (s_vec_loop). */
typedef struct xrsfm_pg_problem {
    int32_t n_frames, n_scales, n_edges, n_scale_costs;
    const double *rot_q;        /* [n_frames][4] x,y,z,w, constant */
    double *pos;                /* [n_frames][3] in/out */
    double *scale;              /* [n_scales]    in/out */
    const uint8_t *pos_const;   /* [n_frames] 1 = constant (NULL: none) */
    const uint8_t *scale_const; /* [n_scales] */
    const double *scale_lower;  /* [n_scales] lower bounds (-HUGE_VAL = none); NULL = unconstrained problem */
    const int32_t *edge_a, *edge_b, *edge_sa, *edge_sb;   /* [n_edges] */
    const double *edge_q_mea;   /* [n_edges][4] x,y,z,w */
    const double *edge_p_mea;   /* [n_edges][3] */
    double weight_o;            /* weight of the scale prior row (ba_solver.cc:221-229) */
    const int32_t *sc_a, *sc_b; /* [n_scale_costs] scale indices */
    const double *sc_s12;       /* [n_scale_costs] */
} xrsfm_pg_problem;

typedef struct xrsfm_pg_options {
    int32_t max_iterations;     /* 100 (InitSolverOptions, ba_solver.cc:73) */
    double function_tolerance, parameter_tolerance, gradient_tolerance;   /* Ceres defaults 1e-6, 1e-8, 1e-10 */
    double initial_radius;      /* 1e16 (ba_solver.cc:261) */
    int32_t verbose;
    /* 0 (default): bounded parameters are handled as Ceres handles them — projection in Plus + projected Armijo line search on
     * every step, nothing else (trust_region_minimizer.cc); with an active bound the loop may stop above the constrained minimum,
     * exactly as upstream does.  1: additionally hold a parameter that sits on its bound while the gradient pushes it outwards
     * (projected-Newton active set) — a deliberate DEVIATION from the reference that reaches the constrained minimum. */
    int32_t bounds_active_set;
} xrsfm_pg_options;

typedef struct xrsfm_pg_summary {
    double initial_cost, final_cost;
    int32_t iterations, n_successful, n_unsuccessful;
    int32_t termination;        /* 1 gradient, 2 parameter, 3 function tolerance, 4 radius, 5 max iterations, 6 failure (linear solver, non-finite input) */
} xrsfm_pg_summary;

void xrsfm_pg_default_options(xrsfm_pg_options *opt);
int xrsfm_pg_solve(const xrsfm_pg_options *opt, xrsfm_pg_problem *problem, xrsfm_pg_summary *summary);

/* ---- Metric-scale refinement against AprilTag corners: the two ceres::Solve calls of tag_refine
 * (/root/reference/src/tag/tag_extract.hpp:193-265).  HOST code like the pose graph.  Detection
 * (apriltag/OpenCV) and the RANSAC triangulation of the corners (CreatePoint3dRAW, tag_extract.hpp:176-192) stay with the
 * caller; this entry point takes the normalised observations and the triangulated corners.
 *   stage 1 (tag_extract.hpp:197-234): per tag 4 x TagCost(get_tag(tag_length)[i], 1.0) on (tag_q, tag_t, scale) with the
 *            corners constant, QuatParam on tag_q, scale >= scale_lower; max_num_iterations 500, other options default
 *   stage 2 (tag_extract.hpp:236-265): the corners become variable and carry one ProjectionCost per observing frame; every
 *            track point carries one ProjectionCost per observation; all frame poses stay constant
 * The caller then divides frame translations and points by the returned scale (tag_extract.hpp:267-275). */
typedef struct xrsfm_tag_problem {
    int32_t n_frames;
    const double *frame_q;      /* [n_frames][4] x,y,z,w  Tcw, constant */
    const double *frame_t;      /* [n_frames][3] */
    int32_t n_tags;
    double tag_length;
    double *tag_corners;        /* [n_tags][4][3] in: triangulated world corners (pt_world_vec); out (stage 2): refined */
    double *tag_q, *tag_t;      /* [n_tags][4], [n_tags][3]  T_w_tag in/out (the reference starts at identity / zero) */
    double scale;               /* in/out (the reference starts at 1.0) */
    double scale_lower;         /* 0.2 (tag_extract.hpp:227) */
    int32_t n_tag_obs;          /* (tag, frame) pairs */
    const int32_t *tag_obs_tag, *tag_obs_frame;
    const double *tag_obs_xy;   /* [n_tag_obs][4][2] normalised image coordinates of the four corners */
    int32_t n_points, n_obs;    /* tracks of the map (used by stage 2 only; n_obs may be 0) */
    double *points;             /* [n_points][3] in/out */
    const int32_t *obs_frame, *obs_pt;
    const double *obs_xy;       /* [n_obs][2] normalised image coordinates (Frame::points_normalized) */
} xrsfm_tag_problem;

void xrsfm_tag_default_options(xrsfm_pg_options *opt);   /* 500 iterations, radius 1e4, tolerances 1e-6 / 1e-8 / 1e-10 */
/* stages = 1: only the first solve; 2: both, like the reference.  summaries[stages]. termination codes as xrsfm_pg_summary. */
int xrsfm_tag_refine(const xrsfm_pg_options *opt, xrsfm_tag_problem *problem, int32_t stages, xrsfm_pg_summary *summaries);

/* Post-BA track filter on the same flat arrays (Point3dProcessor::FilterPoints3d,
 * /root/reference/src/geometry/track_processor.cc:280-332, called after every KGBA at incremental_mapper.cc:83-85).
 * The problem here is the whole map: every registered frame and every observation of every non-outlier track.
 *   obs_delete[i]    1: observation i has reprojection error > max_reproj_error or depth outside [1e-3, 1e3]
 *   track_outlier[j] 0 keep; 1: at most one observation would remain; 2: max pairwise triangulation angle of the kept
 *                    observations < min_tri_angle_rad (for 1 every observation of the track goes, like SetTrackOutlier)
 *   track_error[j]   mean reprojection error of the kept observations (-1 if outlier 1 / no observation)   (may be NULL)
 *   track_angle[j]   Track::angle_ as UpdateTrackAngle leaves it (early exit above the threshold)          (may be NULL)
 *   num_filtered[2]  the two counters the reference prints ("Outlier num1 / num2")                          (may be NULL) */
int xrsfm_ba_filter_tracks(const xrsfm_ba_problem *problem, double max_reproj_error, double min_tri_angle_rad,
                           uint8_t *obs_delete, uint8_t *track_outlier, double *track_error, double *track_angle,
                           int32_t *num_filtered);

/* Batched robust triangulation of new tracks: the creation of a 3-D point from the observations of an untriangulated key point
 * (CreatePoint3d1, /root/reference/src/geometry/track_processor.cc:109-161, called by Point3dProcessor::TriangulateFramePoint once
 * per registered frame before the local BA and by run_triangulation over every frame of a map).  Restates
 * colmap::EstimateTriangulation: LO-RANSAC over the pairs (i, j), i < j, of a track's observations in lexicographic order
 * (CombinationSampler, deterministic), two-view DLT per pair, residual = squared angle between the observed ray and the ray to the
 * model, multi-view refit of the inliers of every new best with more than two inliers.  One wave per track on the device, all
 * tracks of a call in one launch; FP64 throughout.
 *
 * The observations of track j are trk_ptr[j] .. trk_ptr[j+1] in the caller's order (the order of `observations` in
 * TriangulateFramePoint: it fixes the trial order).  obs_xy are NORMALISED image coordinates (GetPointNormalized of the key point:
 * undistortion stays with the caller, as for xrsfm_tag_problem).  cam_q / cam_t are Tcw of the registered frames, q = x,y,z,w.
 *
 *   status[j]       0 no model (the reference's `return false`); 1 point created; 2 fewer than two observations (the `continue`
 *                   at track_processor.cc:222); 3 more than XRSFM_BA_TRI_MAX_OBS observations: not attempted, the call still
 *                   succeeds.  (128: C(128, 2) = 8128 pairs stay below the reference's cap of 10000 trials, which starts to bite
 *                   at 142 observations, so the combination sampler never wraps.)
 *   on status 1     points[j] the model; inlier_mask the reference's report.inlier_mask (AddTrack takes the observations it
 *                   marks); num_inliers[j] the best support's count; num_trials[j] report.num_trials; best_trial[j] the 0-based
 *                   trial whose sample model became the final best, plus bit 30 when the locally optimised model of that trial
 *                   is the one returned
 *   on 0, 2, 3      points[j] untouched, the track's mask entries 0, counts 0, best_trial -1
 * On any negative return code no output is touched.  No output ever receives a NaN or an Inf: a status-1 model that is not
 * finite becomes status 0.  A track's outputs are bit-identical whatever else is in the batch and in whatever order.
 *
 * Documented deviation (defined meaning where the reference has none): a sample model without a single inlier still beats the
 * initial best support (0 == 0 inliers and 0.0 < DBL_MAX), after which the reference's ComputeNumTrials(0, ...) divides by
 * log(1) = 0 and casts -inf to size_t.  An outlier pair whose rays are skew by more than max_error_rad reaches this.  The library
 * takes zero inliers as "no information": the adaptive trial bound stays unbounded there.
 *
 * Errors: XRSFM_BA_EINVAL (checked on the host before the device is touched, one line on stderr) — NULL opt; NULL points, status
 * or inlier_mask with n_tracks > 0; a negative count; trk_ptr not starting at 0 or decreasing; an obs_cam out of range; a
 * non-finite pose, coordinate or option; max_error_rad <= 0; confidence or min_inlier_ratio outside [0, 1]; max_num_trials < 1;
 * exhaustive_threshold < 0; min_tri_angle_rad < 0.  XRSFM_BA_ENODEV without a device (there is no CPU path); XRSFM_BA_ENOMEM when
 * staging memory cannot be had.  n_tracks == 0 is success and needs no device. */
typedef struct xrsfm_ba_tri_options {
    double  min_tri_angle_rad;    /* DegToRad(1.5)   track_processor.cc:132 */
    double  max_error_rad;        /* DegToRad(2): bound on the angular error; residual = angle^2  :135 */
    double  confidence;           /* 0.9999          :136 */
    double  min_inlier_ratio;     /* 0.02            :137 */
    int32_t max_num_trials;       /* 10000           :138 */
    int32_t exhaustive_threshold; /* 15: tracks of at most this many observations try every pair  :140-144 */
} xrsfm_ba_tri_options;
#define XRSFM_BA_TRI_MAX_OBS 128
void xrsfm_ba_triangulate_options(xrsfm_ba_tri_options *opt);   /* the values above */
int xrsfm_ba_triangulate_tracks(const xrsfm_ba_tri_options *opt, int32_t n_cams, const double *cam_q /* [n_cams][4] */,
                                const double *cam_t /* [n_cams][3] */, int32_t n_tracks, const int32_t *trk_ptr /* [n_tracks+1] */,
                                const int32_t *obs_cam /* [n_obs] */, const double *obs_xy /* [n_obs][2] */,
                                double *points /* [n_tracks][3] */, uint8_t *status /* [n_tracks] */, uint8_t *inlier_mask /* [n_obs] */,
                                int32_t *num_inliers /* [n_tracks], may be NULL */, int32_t *num_trials /* [n_tracks], may be NULL */,
                                int32_t *best_trial /* [n_tracks], may be NULL */);

/* Batched absolute pose of frames from 2D-3D correspondences: the "pose estimate [init]" of RegisterImage, that is
 * SolvePnP_colmap -> EstimateAbsolutePose -> colmap::LORANSAC<P3PEstimator, EPNPEstimator> (reference src/geometry/pnp.cc:29-36,
 * 253-316), for all frames of a call in one launch: one workgroup per frame, FP64 throughout.  The result is the pose that
 * xrsfm_ba_refine_pose(s) starts from.  Restates LORANSAC::Estimate (optim/loransac.h:92-239) with InlierSupportMeasurer and
 * ComputeSquaredReprojectionError (residual DBL_MAX at depth <= DBL_EPSILON): P3P sample models from three correspondences, an
 * EPnP model from the inliers of every new best with more than 3 inliers, the adaptive trial bound.
 *
 * The correspondences of frame f are corr_ptr[f] .. corr_ptr[f+1] in the caller's order (what SearchCorrespondences hands to
 * SolvePnP_colmap).  xy are NORMALISED image coordinates: undistortion stays with the caller, as for xrsfm_ba_triangulate_tracks.
 *
 *   status[f]       0 no model (the reference's `return false`: !report.success || num_inliers == 0); 1 pose found; 2 fewer than
 *                   3 correspondences; 3 more than XRSFM_BA_POSE_MAX_CORR correspondences: not attempted, the call still succeeds
 *   on status 1     q[f] (unit quaternion x,y,z,w with w >= 0, from the 3x3 matrix by the usual four-branch rule) and t[f] the
 *                   model (Tcw); inlier_mask the reference's report.inlier_mask, recomputed from the returned model;
 *                   num_inliers[f] its sum; num_trials[f] report.num_trials; best_trial[f] the 0-based trial of the final best,
 *                   plus bit 30 when the locally optimised model is the one returned (the convention of best_trial above)
 *   on 0, 2, 3      q[f], t[f] untouched, the frame's mask entries 0, counts 0, best_trial -1
 * On any negative return code no output is touched.  No output ever receives a NaN or an Inf: a non-finite sample or local model
 * is discarded.  A frame's outputs are bit-identical whatever else is in the batch, in whatever order, and across calls.
 *
 * Documented deviations (defined meaning where the reference has no portable one):
 *   1. Sampler.  The reference draws from one process-wide std::mt19937 that is never re-seeded between calls, through
 *      std::uniform_int_distribution.  Here every frame gets a fresh MT19937 (init_genrand(seed), seed from frame_seed or
 *      opt->seed) and replays RandomSampler: the index array persists across the trials of a frame, three Fisher-Yates steps per
 *      trial; bounded draw for m = last - i + 1: s = 0xFFFFFFFF / m, draw 32-bit words until x < m s, j = i + x / s.
 *   2. Root order and acceptance.  The quartic's roots are found as complex numbers by a bounded iteration; a root is taken when
 *      |Im| <= 1e-10 and Re >= 0; the models of one trial are offered in ascending Re.  A vanishing leading coefficient gives no
 *      model.  The rigid fit is Umeyama without scale with the sign from det(U) det(V).
 *   3. EPnP's sign step negates iff the first inlier's depth is negative (the published rule), not whenever it is non-zero.
 *   As for the triangulation, a model without a single inlier leaves the adaptive trial bound unbounded.
 *
 * Errors: XRSFM_BA_EINVAL (checked on the host before the device is touched, one line on stderr) — NULL opt; NULL q, t, status or
 * inlier_mask with n_frames > 0; a negative count; corr_ptr not starting at 0 or decreasing; a non-finite coordinate, max_error or
 * option; max_error <= 0 (option or per frame); confidence or min_inlier_ratio outside [0, 1]; min_num_trials < 0;
 * max_num_trials < 1 or above XRSFM_BA_POSE_MAX_TRIALS; min_num_trials > max_num_trials.  XRSFM_BA_ENODEV without a device (there
 * is no CPU path); XRSFM_BA_ENOMEM when staging memory cannot be had.  n_frames == 0 is success and needs no device. */
typedef struct xrsfm_ba_pose_options {
    double  max_error;         /* normalised image units: 8 / fx (RegisterImage, pnp.cc:30), 16 / fx (RegisterNextImageLocal); default 8 / 800 */
    double  confidence;        /* 0.9999  pnp.cc:265 */
    double  min_inlier_ratio;  /* 0.25    pnp.cc:261 */
    int32_t min_num_trials;    /* 100     pnp.cc:264 */
    int32_t max_num_trials;    /* XRSFM_BA_POSE_MAX_TRIALS; the effective cap is min(this, the constructor's bound from
                                  min_inlier_ratio: 585 at the defaults) */
    uint32_t seed;             /* 0 */
} xrsfm_ba_pose_options;
#define XRSFM_BA_POSE_MAX_CORR   8192
#define XRSFM_BA_POSE_MAX_TRIALS 16384
void xrsfm_ba_absolute_pose_options(xrsfm_ba_pose_options *opt);   /* the values above */
int xrsfm_ba_absolute_pose(const xrsfm_ba_pose_options *opt, int32_t n_frames, const int32_t *corr_ptr /* [n_frames+1] */,
                           const double *xy /* [n][2] normalised */, const double *points3d /* [n][3] */,
                           const double *frame_max_error /* [n_frames] or NULL = opt->max_error */,
                           const uint32_t *frame_seed /* [n_frames] or NULL = opt->seed */, double *q /* [n_frames][4] x,y,z,w */,
                           double *t /* [n_frames][3] */, uint8_t *status /* [n_frames] */, uint8_t *inlier_mask /* [n] */,
                           int32_t *num_inliers /* [n_frames], may be NULL */, int32_t *num_trials /* [n_frames], may be NULL */,
                           int32_t *best_trial /* [n_frames], may be NULL */);
/* TEST ENTRY, no GPU: the sample triples of the first n_trials trials for n correspondences and one seed (deviation 1). */
int xrsfm_ba_debug_pose_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t *triples /* [n_trials][3] */);

/* Batched two-view initialisation: what FindInitFramePair computes for every candidate pair and InitializeMap for the chosen one,
 * that is CheckInitFramePair -> solve_essential (a 5-point RANSAC) -> decompose_rt (four-way decomposition, triangulation of
 * every match) -> the triangulation-angle counts (reference src/geometry/map_initializer.cc:13-65, 141-206; essential.cc:283-487),
 * for all pairs of a call in one launch: one workgroup per pair, FP64 throughout.
 *
 * The matches of pair p are match_ptr[p] .. match_ptr[p+1]: the matches the reference keeps (frame_pair.inlier_mask), in its
 * order.  xy_a, xy_b are NORMALISED image coordinates in frame 1 and frame 2; pair_threshold[p] is 10 / fx of frame 1
 * (map_initializer.cc:32).  Restated literally: the inlier test is sampson_error < 2 th^2 (the error is already squared); the score
 * is the sum over all matches of log(1 + se^2 / (2 th^2)); a model wins with more inliers, or with as many (and best_inlier > 0)
 * and a strictly smaller score; after a new best of k of n the trial bound becomes ceil(log(1 - confidence) / log(1 - (k / n)^5))
 * if that is smaller; decompose_rt runs over ALL matches and picks the candidate with strictly more points in front, in the order
 * (R1,+T), (R1,-T), (R2,+T), (R2,-T); a point is in front when both depths are positive and below max_depth.
 *
 *   status[p]     0 no E (best_E stayed NaN) or no candidate with a point in front (the reference then takes k = 0 of an
 *                 arbitrary order; the pair is rejected either way); 1 geometry found, accepted[p] says whether it qualifies;
 *                 2 fewer than min_matches matches; 3 more than XRSFM_BA_INIT_MAX_MATCHES: not attempted, the call still succeeds
 *   on status 1   E[p] the best essential matrix scaled to unit Frobenius norm (x_b' E x_a = 0); q[p] (x,y,z,w, w >= 0) and t[p]
 *                 the pose of frame 2 (frame 1 is the identity); points[i] the triangulated point of every match with
 *                 front_mask[i] (written only there); essential_mask[i] the reference's solve_essential mask;
 *                 counts[p] = {essential inliers, num_p3d, winning candidate k, 0, num_p3d_valid at min_angle_rad[0..3]};
 *                 accepted[p] bit a: num_p3d >= min_front_ratio n && num_p3d_valid[a] >= min_angle_ratio num_p3d &&
 *                 num_p3d_valid[a] > min_num_valid; num_trials[p] the trials executed; best_trial[p] = trial * 16 + model slot
 *   on status 0   q, t, points untouched, front_mask 0, accepted 0; E, essential_mask, counts[0], num_trials and best_trial are
 *                 those of the best E if there is one, otherwise E is untouched, the masks and counts are 0 and best_trial is -1
 *   on 2, 3       E, q, t, points untouched, masks and counts 0, num_trials 0, best_trial -1
 * On any negative return code no output is touched.  No output ever receives a NaN or an Inf: a non-finite model is never
 * offered.  A pair's outputs are bit-identical whatever else is in the batch, in whatever order, and across calls.
 *
 * Documented deviations (defined meaning where the reference has no portable one):
 *   1. Sampler.  LotBox draws through std::default_random_engine and std::uniform_int_distribution<size_t>, both chosen by the
 *      standard library.  Here every pair gets a fresh MT19937 (init_genrand(seed), seed from pair_seed or opt->seed) and the
 *      sampler of xrsfm_ba_absolute_pose with five draws: the index array persists across the trials of a pair, five
 *      Fisher-Yates steps per trial, the same bounded draw.
 *   2. Model order.  The up to ten models of one trial are offered in ascending real eigenvalue of the action matrix (found by a
 *      bounded Hessenberg / shifted-QR iteration; a root is taken when |Im| < 1e-10).  The order decides exact ties only.
 *   3. Decomposition.  SVD branch only.  The third singular vectors are u3 = u1 x u2 and v3 = v1 x v2, so both determinants are
 *      +1 and nothing depends on how a library signs a null vector; T = u3, R1 = U W V', R2 = U W' V'.
 *   A trial bound that is NaN or -inf in the reference (confidence 1; a ratio whose fifth power underflows) counts as unbounded.
 *
 * Errors: XRSFM_BA_EINVAL (checked on the host before the device is touched, one line on stderr) — NULL opt; a negative count;
 * NULL status, E, q, t, points, essential_mask, front_mask or counts with n_pairs > 0; NULL match_ptr or pair_threshold;
 * match_ptr not starting at 0 or decreasing; NULL xy_a or xy_b with matches; a non-finite coordinate, threshold or option; a
 * threshold <= 0; confidence outside [0, 1]; max_iterations < 1 or above XRSFM_BA_INIT_MAX_TRIALS; min_matches < 5;
 * max_depth <= 0; n_angles outside [1, 4]; a negative min_angle_rad, min_front_ratio or min_angle_ratio; min_num_valid < 0.
 * XRSFM_BA_ENODEV without a device (there is no CPU path); XRSFM_BA_ENOMEM when staging memory cannot be had.  n_pairs == 0 is
 * success and needs no device. */
typedef struct xrsfm_ba_two_view_options {
    double  confidence;          /* 0.9   essential.cc:393 */
    int32_t max_iterations;      /* 50    :393; at most XRSFM_BA_INIT_MAX_TRIALS (64) */
    uint32_t seed;               /* 0     :393 */
    int32_t min_matches;         /* 10    map_initializer.cc:30; at least 5 */
    double  max_depth;           /* 100   essential.cc:424 */
    int32_t n_angles;            /* 2, at most 4 */
    double  min_angle_rad[4];    /* DegToRad(16), DegToRad(8)  map_initializer.cc:119,132 */
    double  min_front_ratio;     /* 0.5   :58 num_p3d >= ratio * n */
    double  min_angle_ratio;     /* 0.5   :58 */
    int32_t min_num_valid;       /* 200   :59, strict > */
} xrsfm_ba_two_view_options;
#define XRSFM_BA_INIT_MAX_MATCHES 8192
#define XRSFM_BA_INIT_MAX_TRIALS  64
void xrsfm_ba_two_view_options_default(xrsfm_ba_two_view_options *opt);   /* the values above */
int xrsfm_ba_two_view_init(const xrsfm_ba_two_view_options *opt, int32_t n_pairs, const int32_t *match_ptr /* [n_pairs+1] */,
                           const double *xy_a /* [n][2] normalised, frame 1 */, const double *xy_b /* [n][2] normalised, frame 2 */,
                           const double *pair_threshold /* [n_pairs]: 10 / fx of frame 1 */,
                           const uint32_t *pair_seed /* [n_pairs] or NULL = opt->seed */, uint8_t *status /* [n_pairs] */,
                           double *E /* [n_pairs][9] row-major, unit Frobenius norm */, double *q /* [n_pairs][4] x,y,z,w, w >= 0 */,
                           double *t /* [n_pairs][3] */, double *points /* [n][3] */, uint8_t *essential_mask /* [n] */,
                           uint8_t *front_mask /* [n]: result_status of decompose_rt */, int32_t *counts /* [n_pairs][4 + 4] */,
                           uint8_t *accepted /* [n_pairs]: bit a = CheckInitFramePair true at min_angle_rad[a]; may be NULL */,
                           int32_t *num_trials /* [n_pairs], may be NULL */, int32_t *best_trial /* [n_pairs], may be NULL */);
/* TEST ENTRY, no GPU: the sample quintuples of the first n_trials trials for n matches and one seed (deviation 1). */
int xrsfm_ba_debug_two_view_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t *quintuples /* [n_trials][5] */);

/* Batched fundamental-matrix verification of matched image pairs: what FeatureMatching computes for every candidate pair, that is
 * SolveFundamnetalCOLMAP -> colmap::LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator>
 * (reference src/geometry/epipolar_geometry.hpp:10-27; src/feature/feature_processing.cc:256-296; run_triangulation.cc:91), for
 * all pairs of a call in one launch: one workgroup per pair, FP64 throughout.  Its inlier masks are the matches that
 * xrsfm_ba_two_view_init expects.  Restates LORANSAC::Estimate (optim/loransac.h:92-239) with InlierSupportMeasurer and
 * ComputeSquaredSampsonError: 7-point sample models (up to three per trial), an 8-point model from the inliers of every new best
 * with at least 8 inliers, the adaptive trial bound with exponent 7.
 *
 * The matches of pair p are match_ptr[p] .. match_ptr[p+1] in the caller's order.  xy_a, xy_b are PIXEL coordinates in the first
 * and second image (frame.points; max_error is in pixels).
 *
 *   status[p]       0 no model (!report.success); 1 model found; 2 fewer than min_matches matches; 3 more than
 *                   XRSFM_BA_FUND_MAX_MATCHES matches: not attempted, the call still succeeds
 *   on status 1     F[p] row-major with x_b' F x_a = 0, scaled to unit Frobenius norm, the entry of largest magnitude positive
 *                   (the reference returns the 7-point model with F(2,2) = 1 and the 8-point model at the scale and sign of its
 *                   SVD); inlier_mask the reference's report.inlier_mask (residual <= max_error^2, from the model before that
 *                   scaling); num_inliers[p] its sum; num_trials[p] report.num_trials; best_trial[p] the 0-based trial of the
 *                   final best, plus bit 30 when the 8-point local model is the one returned; accepted[p] whether
 *                   num_inliers >= max(min_num_inliers, (int)(min_accept_ratio n)) (feature_processing.cc:284-290)
 *   on 0, 2, 3      F[p] untouched, the pair's mask entries 0, counts 0, best_trial -1, accepted 0
 * On any negative return code no output is touched.  No output ever receives a NaN or an Inf: a non-finite sample or local model
 * is discarded.  A pair's outputs are bit-identical whatever else is in the batch, in whatever order, and across calls.
 *
 * Documented deviations (defined meaning where the reference has no portable one):
 *   1. Sampler.  That of xrsfm_ba_absolute_pose with seven draws: a fresh MT19937 per pair (init_genrand(seed), seed from
 *      pair_seed or opt->seed), an index array that persists across the trials of the pair, seven Fisher-Yates steps per trial,
 *      the same bounded draw (with a cap of 16 rejected words per draw, never reached, so that the device loop is bounded).
 *      The septuples are drawn on the device.
 *   2. Null space, roots and model order.  The null space of the 7 x 9 system is spanned by Q e7, Q e8 of the Householder QR of
 *      its transpose (the reference takes two columns of an SVD; the models are the same, the cubic's variable is not).  The
 *      cubic is solved by bisection for one real root, the closed form for the remaining quadratic and two Newton steps per
 *      root; a complex pair is taken when |Im| <= 1e-10; leading zero coefficients lower the degree.  The models of one trial
 *      are offered in ascending root on that basis.  The order decides ties and what is seen at the aborting trial.
 *   3. 8-point model.  The null vector is the eigenvector of smallest eigenvalue of the 9 x 9 Gram matrix of the normalised
 *      constraint rows (cyclic Jacobi); the rank-2 projection keeps the two largest terms of a one-sided Jacobi SVD of the 3 x 3
 *      matrix and forms no third singular vector, so nothing depends on how a library signs one.
 *   As for the pose, a model without a single inlier leaves the adaptive trial bound unbounded.
 *
 * Errors: XRSFM_BA_EINVAL (checked on the host before the device is touched, one line on stderr) — NULL opt; NULL status, F or
 * inlier_mask with n_pairs > 0; a negative count; NULL match_ptr, or one not starting at 0 or decreasing; NULL xy_a or xy_b with
 * matches; a non-finite coordinate, max_error or option; max_error <= 0 (option or per pair); confidence or min_inlier_ratio
 * outside [0, 1]; min_num_trials < 0; max_num_trials < 1 or above XRSFM_BA_FUND_MAX_TRIALS; min_num_trials > max_num_trials;
 * min_matches < 7; min_num_inliers < 0; min_accept_ratio < 0.  XRSFM_BA_ENODEV without a device (there is no CPU path);
 * XRSFM_BA_ENOMEM when staging memory cannot be had.  n_pairs == 0 is success and needs no device. */
typedef struct xrsfm_ba_fund_options {
    double  max_error;         /* 4.0 pixels   epipolar_geometry.hpp:14 */
    double  confidence;        /* 0.999        :17 */
    double  min_inlier_ratio;  /* 0.25         :18; its constructor bound (113174 trials) is above max_num_trials */
    int32_t min_num_trials;    /* 100          :16 */
    int32_t max_num_trials;    /* 10000        :15; at most XRSFM_BA_FUND_MAX_TRIALS */
    uint32_t seed;             /* 0 */
    int32_t min_matches;       /* 15           feature_processing.cc:226; at least 7 */
    int32_t min_num_inliers;   /* 15           :227 */
    double  min_accept_ratio;  /* 0.25         :228 */
} xrsfm_ba_fund_options;
#define XRSFM_BA_FUND_MAX_MATCHES 8192
#define XRSFM_BA_FUND_MAX_TRIALS  16384
void xrsfm_ba_verify_pairs_options(xrsfm_ba_fund_options *opt);   /* the values above */
int xrsfm_ba_verify_pairs(const xrsfm_ba_fund_options *opt, int32_t n_pairs, const int32_t *match_ptr /* [n_pairs+1] */,
                          const double *xy_a /* [n][2] pixels, first image */, const double *xy_b /* [n][2] pixels, second image */,
                          const double *pair_max_error /* [n_pairs] or NULL = opt->max_error */,
                          const uint32_t *pair_seed /* [n_pairs] or NULL = opt->seed */, uint8_t *status /* [n_pairs] */,
                          double *F /* [n_pairs][9] row-major */, uint8_t *inlier_mask /* [n] */,
                          int32_t *num_inliers /* [n_pairs], may be NULL */, int32_t *num_trials /* [n_pairs], may be NULL */,
                          int32_t *best_trial /* [n_pairs], may be NULL */, uint8_t *accepted /* [n_pairs], may be NULL */);
/* TEST ENTRY, no GPU: the sample septuples of the first n_trials trials for n matches and one seed (deviation 1). */
int xrsfm_ba_debug_fund_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t *tuples /* [n_trials][7] */);

/* Batched SIFT descriptor matching: what FeatureMatching computes for every candidate pair before the verification above, that is
 * SiftMatchGPU::GetSiftMatch (reference src/feature/feature_processing.cc:118-154, 240-255; the kernels MultiplyDescriptor_Kernel,
 * RowMatch_Kernel and ColMatch_Kernel of 3rdparty/SiftGPU/ProgramCU.cu:1491-1884 and the host loop of SiftMatchCU::GetBestMatch,
 * SiftMatchCU.cpp:186-215), for all pairs of a call, with the 128-byte products on the int8 matrix cores.  Every output is an
 * integer and is exactly defined:
 *
 *   dot(i, j)       sum_k a[i][k] b[j][k] over the 128 uint8 components: at most 8 323 200
 *   (best, idx, next) of a row over all columns, and of a column over all rows, from (0, -1, 0): best = max(0, max dot), next the
 *                   second largest value counted with multiplicity and floored at 0, idx the lowest position holding best, -1 when
 *                   no dot is positive (ProgramCU.cu:1804-1826, 1861-1863)
 *   dist(d)         (float) acos(min((double) ((float) d * 2^-18f), 1.0)) (:1830), from a table over d = 0 .. 2^18
 *   row_match[i]    idx when dist(best) < max_distance && dist(best) < dist(next) * max_ratio (all float, :1833), else -1;
 *                   col_match[j] likewise
 *   matches         (i, row_match[i]) in ascending i where row_match[i] >= 0 and, with mutual_best, col_match[row_match[i]] == i
 *                   (SiftMatchCU.cpp:199-213)
 *
 * Frame f holds the descriptors desc_ptr[f] .. desc_ptr[f+1]; only its first max_features take part (SetDescriptors:113-114).  Pair
 * p matches frame pair_a[p] (rows, i) against pair_b[p] (columns, j); a pair may name one frame twice; a frame without descriptors
 * gives its pairs no matches.  The matches of pair p are rows match_ptr[p] .. match_ptr[p+1] of `matches`: as int32, the
 * match_ptr that xrsfm_ba_verify_pairs takes.  A capacity of sum_p min(n_a(p), max_features) always suffices.  num_row[p] / num_col[p]: the rows /
 * columns that pass their own test.  On any negative return code no output is touched.  A pair's outputs are bit-identical whatever
 * else is in the batch, in whatever order, and across calls.
 *
 * Documented deviations:
 *   1. The distance table is built on the host with its acos, once per process (the reference calls the device's acos per row).
 *      No transcendental runs on the device and none sits in a decision.
 *   2. Of several positions holding the best, idx is the lowest (the reference's depends on its 32-lane walk).  With max_ratio <= 1
 *      a tied best always fails dist < dist_next * max_ratio, so the index of a tied best is never returned in a match; a
 *      max_ratio outside (0, 1] is refused.
 *   3. All pairs of a call go in one submission and every frame is prepared once (the reference uploads both descriptor sets for
 *      every pair).  The call is split into several launches when its workspace would exceed 1 GiB (environment
 *      XRSFM_BA_MATCH_WORKSPACE_MB: another bound); the results do not depend on the split.
 *   The reference's cap on the number of matches (max_match = 16384 = the most rows) never binds and is not restated.
 *
 * Errors: XRSFM_BA_EINVAL (checked on the host before the device is touched, one line on stderr) — NULL opt; a negative count;
 * non-finite or non-positive max_distance; max_ratio outside (0, 1]; max_features outside 1 .. XRSFM_BA_MATCH_MAX_FEATURES; with
 * n_pairs > 0: NULL match_ptr, pair_a, pair_b or desc_ptr, a desc_ptr that does not start at 0 or decreases, NULL desc with
 * descriptors, NULL matches with a capacity, a frame index out of range.  XRSFM_BA_EINVAL after the computation, with one line on
 * stderr that names the needed size, when the matches do not fit matches_capacity.  XRSFM_BA_ENODEV without a device (there is no
 * CPU path); XRSFM_BA_ENOMEM when descriptors plus workspace cannot be had.  n_pairs == 0 is success and needs no device. */
typedef struct xrsfm_ba_match_options {
    float   max_distance;   /* 0.7    feature_processing.cc:122 */
    float   max_ratio;      /* 0.8    :123; in (0, 1] */
    int32_t mutual_best;    /* 1      :146 */
    int32_t max_features;   /* 16384  :23; 1 .. XRSFM_BA_MATCH_MAX_FEATURES */
} xrsfm_ba_match_options;
#define XRSFM_BA_MATCH_MAX_FEATURES 16384
#define XRSFM_BA_MATCH_DIM 128
void xrsfm_ba_match_options_default(xrsfm_ba_match_options *opt);   /* the values above */
int xrsfm_ba_match_descriptors(const xrsfm_ba_match_options *opt, int32_t n_frames, const int64_t *desc_ptr /* [n_frames+1] */,
                               const uint8_t *desc /* [n][128] */, int32_t n_pairs, const int32_t *pair_a,
                               const int32_t *pair_b /* [n_pairs] frame indices */, int64_t matches_capacity,
                               int64_t *match_ptr /* [n_pairs+1] */, int32_t *matches /* [capacity][2]: (i, j) */,
                               int32_t *num_row /* [n_pairs], may be NULL */, int32_t *num_col /* [n_pairs], may be NULL */);
/* TEST ENTRY, no GPU: dist(0 .. 2^18), the table of the test. */
int xrsfm_ba_debug_match_table(float *table /* [262145] */);
/* TEST ENTRY: one pair through the kernels of xrsfm_ba_match_descriptors; the triples (best, idx, next) of its rows and columns.
 * n_a, n_b in 0 .. XRSFM_BA_MATCH_MAX_FEATURES. */
int xrsfm_ba_debug_match_top2(int32_t n_a, const uint8_t *desc_a, int32_t n_b, const uint8_t *desc_b,
                              int32_t *row_top /* [n_a][3] */, int32_t *col_top /* [n_b][3] */);

/* Batched SIFT scale space and keypoint detection: the first half of what SiftExtractor computes for every image
 * (SiftGPU::RunSIFT: reference 3rdparty/SiftGPU/PyramidCU.cpp BuildPyramid, DetectKeypointsEX, GenerateFeatureList and
 * DownloadKeypoints; ProgramCU.cu FilterH/FilterV, UpsampleKernel, DownsampleKernel, ComputeDOG_Kernel, ComputeKEY_Kernel), with the
 * orientation fixed to 0: the keypoint list of the reference's upright mode.  All arithmetic is FP32; the rule is restated in
 * xrsfm_amd/csrc/ba_sift_rule.h and DESIGN.md 5m.  All images of a call, whatever their sizes, go through the same kernel launches.
 *
 * Image i is width[i] x height[i] 8-bit grey, row-major and packed, at pixels + pixel_ptr[i]; pixel_ptr[i+1] - pixel_ptr[i] =
 * width[i] * height[i].  The width is truncated to a multiple of 4 (the columns beyond are ignored).  Octave o of the pyramid has
 * height h0 >> o and the STORED width roundup4(w0 >> o), (w0, h0) = (W, H) << 1 for first_octave -1; there are
 * min(num_octaves, max(1, floor(log2(min(w0, h0))) - 3)) octaves.
 *   keys[k]         (X, Y, S, 0): position and scale in input-image pixels (DownloadKeypoints), orientation 0
 *   loc[k]          (octave, DoG level j in 0..2, row, col): the integer location in the octave, for the descriptor stage
 *   sign[k]         +1 maximum, -1 minimum
 *   key_ptr         the keypoints of image i are key_ptr[i] .. key_ptr[i+1], in the order octave, level, row, column ascending
 *                   (the reference's order within a level is that of its histogram pyramid and is not reproduced)
 *   level_count     [n_images][num_octaves * 3], may be NULL: the keypoints of every level BEFORE the budget (0 for octaves the
 *                   image does not have).  The budget: levels are visited from the last octave to the first and from j = 2 to 0;
 *                   a level contributes nothing if the total already exceeds max_num_features, else all of its keypoints
 * If the pyramids of the call exceed XRSFM_BA_SIFT_WORKSPACE_MB (environment, default 4096) the call runs in chunks of images
 * (an image larger than the budget runs alone); the results do not depend on the split by a bit.
 *
 * XRSFM_BA_EINVAL, checked before the device is touched, one line on stderr, outputs untouched: NULL opt; a negative n_images or
 * capacity; first_octave outside {-1, 0}; num_octaves outside 1 .. 8; a non-finite or non-positive threshold; max_num_features or
 * max_image_size < 1; with n_images > 0: NULL width, height, pixel_ptr, pixels or key_ptr, NULL keys, loc or sign with a capacity,
 * a truncated width or a height below 16, a side above max_image_size (the reference down-samples such images: not built), a
 * pixel_ptr that does not start at 0 or disagrees with the sizes.  XRSFM_BA_EINVAL after the computation, with one line on stderr
 * that names the needed size, when the keypoints do not fit capacity: key_ptr and level_count are written, keys, loc and sign are
 * not.  XRSFM_BA_ENODEV without a device (there is no CPU path); XRSFM_BA_ENOMEM when the workspace cannot be had.  n_images == 0
 * is success and needs no device. */
typedef struct xrsfm_ba_sift_options {
    int32_t first_octave;      /* -1      sift_extractor.h; -1 or 0 */
    int32_t num_octaves;       /* 4       1 .. 8 */
    float   peak_threshold;    /* 0.02/3  */
    float   edge_threshold;    /* 10      */
    int32_t max_num_features;  /* 8192    */
    int32_t max_image_size;    /* 3200    */
} xrsfm_ba_sift_options;
#define XRSFM_BA_SIFT_MAX_TAPS 33
#define XRSFM_BA_SIFT_MAX_OCTAVES 8
void xrsfm_ba_sift_options_default(xrsfm_ba_sift_options *opt);   /* the values above */
int xrsfm_ba_detect_keypoints(const xrsfm_ba_sift_options *opt, int32_t n_images, const int32_t *width, const int32_t *height /* [n_images] */,
                              const int64_t *pixel_ptr /* [n_images+1] */, const uint8_t *pixels, int64_t capacity,
                              int64_t *key_ptr /* [n_images+1] */, float *keys /* [capacity][4] */, int32_t *loc /* [capacity][4] */,
                              int8_t *sign /* [capacity] */, int32_t *level_count /* [n_images][num_octaves*3], may be NULL */);
/* TEST ENTRY, no GPU: the taps of the Gaussian filter of one sigma (CreateFilterKernel); taps beyond *width are 0. */
int xrsfm_ba_debug_sift_taps(float sigma, float *taps /* [33] */, int32_t *width);
/* TEST ENTRY: the six Gaussian and the five DoG levels of one octave of one image, [level][h][w] with w the stored width. */
int xrsfm_ba_debug_sift_levels(const xrsfm_ba_sift_options *opt, int32_t width, int32_t height, const uint8_t *pixels, int32_t octave,
                               float *gauss /* [6][h][w] */, float *dog /* [5][h][w] */);
/* TEST ENTRY: the keypoints of one image as xrsfm_ba_detect_keypoints orders them, with the sub-pixel offsets the interface
 * folds into keys: offsets[k] = (sign, dx, dy, ds).  *n_keys is written even when capacity is too small (XRSFM_BA_EINVAL). */
int xrsfm_ba_debug_sift_offsets(const xrsfm_ba_sift_options *opt, int32_t width, int32_t height, const uint8_t *pixels, int64_t capacity,
                                int64_t *n_keys, int32_t *loc /* [capacity][4] */, float *offsets /* [capacity][4] */);

/* Batched SIFT orientation and descriptors: images to uint8 features, the whole of FeatureExtract (SiftExtractor::ExtractUINT8:
 * SiftGPU::RunSIFT with one orientation per keypoint, reference 3rdparty/SiftGPU/ProgramCU.cu ComputeDOG_Kernel's gradient half,
 * ComputeOrientation_Kernel, ComputeDescriptor_Kernel<false>, NormalizeDescriptor_Kernel, PyramidCU.cpp DownloadKeypoints; then
 * sift_extractor.cc L1RootNormalizeFeatureDescriptors and sift_extractor.h FeatureDescriptorsToUnsignedByte).  The rule is restated
 * in xrsfm_amd/csrc/ba_sift_desc_rule.h and DESIGN.md 5n; FP32 throughout.
 *
 * key_ptr, loc, sign, level_count and keys[k][0..2] are what xrsfm_ba_detect_keypoints returns for the same images and options, bit
 * for bit and in the same order.
 *   keys[k][3]      the orientation as DownloadKeypoints hands it out: (float) fmod(2 pi - w, 2 pi) in double on the float w of the
 *                   orientation histogram's parabola; 0 with upright
 *   desc[k]         the 128 bytes of ExtractUINT8, [cell = 4 iy + ix][8 bins]: desc with key_ptr is the desc / desc_ptr that
 *                   xrsfm_ba_match_descriptors takes
 *   desc_float[k]   may be NULL: what ExtractFLOAT returns, after the L1 root
 * A parabola whose denominator is zero (the reference: NaN) has the offset 0.  A descriptor sample whose bin position theta rounds
 * to exactly 8.0f is dropped, as ComputeDescriptor_Kernel<false> drops it.  Chunking under XRSFM_BA_SIFT_WORKSPACE_MB works as in
 * xrsfm_ba_detect_keypoints, the budget counts the gradient planes (6 more floats per pixel of an octave), and the results do not
 * depend on the split by a bit.
 *
 * Errors as in xrsfm_ba_detect_keypoints; XRSFM_BA_EINVAL before the device is touched, outputs untouched, also for a NULL dopt, an
 * upright outside {0, 1} and a NULL desc with a capacity; when capacity is too small key_ptr and level_count are written and
 * nothing else.  Not built: max_num_orientations 2, affine shape, domain-size pooling, the RECT descriptor, L2 as the final
 * normalisation, existing-keypoint input. */
typedef struct xrsfm_ba_sift_desc_options {
    int32_t upright;   /* 0   sift_extractor.h; 1 = "-ofix": orientation 0, descriptors at angle 0 */
} xrsfm_ba_sift_desc_options;
void xrsfm_ba_sift_desc_options_default(xrsfm_ba_sift_desc_options *opt);
int xrsfm_ba_extract_features(const xrsfm_ba_sift_options *opt, const xrsfm_ba_sift_desc_options *dopt, int32_t n_images,
                              const int32_t *width, const int32_t *height, const int64_t *pixel_ptr, const uint8_t *pixels,
                              int64_t capacity, int64_t *key_ptr, float *keys /* [capacity][4] */, int32_t *loc, int8_t *sign,
                              uint8_t *desc /* [capacity][128] */, float *desc_float /* [capacity][128], may be NULL */,
                              int32_t *level_count);
/* TEST ENTRY: (grd, rot) of G[1..3] of one octave of one image, [3][h][w][2] with w the stored width; border pixels are (0, 0). */
int xrsfm_ba_debug_sift_gradient(const xrsfm_ba_sift_options *opt, int32_t width, int32_t height, const uint8_t *pixels, int32_t octave,
                                 float *grad /* [3][h][w][2] */);
/* TEST ENTRY: per keypoint of one image, in the interface's order: okeys the octave-space key (x, y, sigma, w) the descriptor kernel
 * read, raw the 128 sums before normalisation, unit the vector after the NormalizeDescriptor_Kernel arithmetic (what
 * GetFeatureVector gives).  *n_keys is written even when capacity is too small (XRSFM_BA_EINVAL). */
int xrsfm_ba_debug_sift_describe(const xrsfm_ba_sift_options *opt, const xrsfm_ba_sift_desc_options *dopt, int32_t width, int32_t height,
                                 const uint8_t *pixels, int64_t capacity, int64_t *n_keys, int32_t *loc /* [capacity][4] */,
                                 float *okeys /* [capacity][4] */, float *raw /* [capacity][128] */, float *unit /* [capacity][128] */);

/* Device-resident frame sets: the features of n frames held on device 0, filled from pixels or from existing features, on which
 * FeatureMatching (match, gather of the matched key points, verification, acceptance) runs any number of times with only pair
 * lists going up and matches and verdicts coming down (reference FeatureExtract + FeatureMatching + ExpansionAndMatching,
 * src/feature/feature_processing.cc:118-377).  Every output equals, bit for bit, what the chain
 * xrsfm_ba_extract_features -> xrsfm_ba_match_descriptors -> gather on the host -> xrsfm_ba_verify_pairs gives.
 *
 * A set is immutable after its creation.  It may be used from one thread at a time (two threads may use two sets).  Its device
 * memory comes from the library's allocation cache and returns to it with xrsfm_ba_frames_destroy; xrsfm_ba_quiesce does not free
 * live sets.  A set holds, per key point, the 16 bytes of its key, its 128 descriptor bytes and 4 bytes of the matching kernels'
 * per-descriptor term, computed once at creation; a set made from images holds 21 bytes more (loc, sign, the orientation).
 *
 * The coordinate of key point k in the verification is ((double) keys[k][0], (double) keys[k][1]).  opt->max_features of the match
 * options clips a frame at match time as in xrsfm_ba_match_descriptors; the set stores every key point.
 *
 * Errors: every argument check runs on the host before the device is touched and prints one line on stderr that names the entry;
 * on any negative code no output is touched, and the creators do not write *out.  n_frames == 0 gives a valid empty set without a
 * device, and so does a set without key points; n_pairs == 0 is success.  Without a device the creators with work to do and
 * xrsfm_ba_frames_match return XRSFM_BA_ENODEV: there is no CPU path.  A frame above INT32_MAX key points, or a call whose matches
 * exceed INT32_MAX, is XRSFM_BA_ETOOBIG. */
typedef struct xrsfm_ba_frames xrsfm_ba_frames;   /* opaque */

/* From existing features: keys [n][4] float as xrsfm_ba_extract_features returns them (x, y, scale, orientation; the matching reads
 * x and y, which must be finite), desc [n][128]; frame f owns rows key_ptr[f] .. key_ptr[f+1]. */
int xrsfm_ba_frames_create(int32_t n_frames, const int64_t *key_ptr, const float *keys, const uint8_t *desc, xrsfm_ba_frames **out);

/* From pixels: xrsfm_ba_extract_features straight into a set, with the arguments and argument checks of that call and no capacity.
 * The key points are put into the interface's order on the device (k_frames_order) and never visit the host. */
int xrsfm_ba_frames_from_images(const xrsfm_ba_sift_options *opt, const xrsfm_ba_sift_desc_options *dopt, int32_t n_images,
                                const int32_t *width, const int32_t *height, const int64_t *pixel_ptr, const uint8_t *pixels,
                                xrsfm_ba_frames **out);

int xrsfm_ba_frames_info(const xrsfm_ba_frames *fs, int32_t *n_frames, int64_t *key_ptr /* [n_frames+1], may be NULL */,
                         uint64_t *device_bytes /* may be NULL: bytes held from the allocation cache */);

/* What xrsfm_ba_extract_features would have returned (each output may be NULL: not wanted).  loc, sign and level_count exist only
 * for sets made from images (they must be NULL otherwise: XRSFM_BA_EINVAL); a capacity below key_ptr[n_frames] is XRSFM_BA_EINVAL,
 * outputs untouched. */
int xrsfm_ba_frames_download(const xrsfm_ba_frames *fs, int64_t capacity, float *keys, uint8_t *desc, int32_t *loc, int8_t *sign,
                             int32_t *level_count);

/* FeatureMatching on resident frames: xrsfm_ba_match_descriptors, the gather of the matched key points, and, with vopt != NULL,
 * xrsfm_ba_verify_pairs on them.  Outputs and their meaning are those of the two calls (match_ptr [n_pairs+1], matches
 * [matches_capacity][2]; a capacity below the matches of the call is XRSFM_BA_EINVAL and the line on stderr names the need); the
 * verification outputs must be NULL when vopt is NULL. */
int xrsfm_ba_frames_match(const xrsfm_ba_frames *fs, const xrsfm_ba_match_options *mopt, const xrsfm_ba_fund_options *vopt,
                          int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                          const double *pair_max_error, const uint32_t *pair_seed, int64_t matches_capacity,
                          int64_t *match_ptr, int32_t *matches, int32_t *num_row, int32_t *num_col,
                          uint8_t *status, double *F, uint8_t *inlier_mask, int32_t *num_inliers, int32_t *num_trials,
                          int32_t *best_trial, uint8_t *accepted);

void xrsfm_ba_frames_destroy(xrsfm_ba_frames *fs);   /* NULL is fine */

/* Match expansion: from the verified pairs so far to the pairs to try next (reference MatchExpansionSolver::Run,
 * src/feature/match_expansion.cc:407-454, the first half of every iteration of ExpansionAndMatching).  One call is one
 * Run of a freshly constructed solver: the component of the initial pair, the simulated incremental reconstruction in synchronous
 * rounds (a frame registers with min_visible marks), the tracks of AddTrack in list order with every quirk of the original, the
 * per-patch covisibility of every connected frame, the covisibility candidates and the similarity candidates.  All of it is integer
 * work and every output is exact.  The second simulation of the reference (100 marks) feeds only a printf and is not computed.
 *
 * Frames: key_ptr [n_frames+1], keys [N][4] float (x and y are read), width and height [n_frames].  Verified pairs: pair_a, pair_b
 * [n_pairs] (id1, id2 as stored: the order matters to the tracks and to the first step of the simulation), match_ptr [n_pairs+1],
 * matches [M][2] (key point in pair_a's frame, key point in pair_b's frame), as xrsfm_ba_frames_match returns them for the accepted
 * pairs with the inliers alone.  rank_ptr [n_frames+1], rank_ids: the retrieval list of every frame, best first; a rank is the 1-based
 * position, the last one for an id listed twice.  tried_a, tried_b [n_tried]: pairs not to propose again, in either order.
 * init_a, init_b: the initial pair, in either order; it must be among the pairs.
 *
 * Outputs: *n_out unordered pairs out_a < out_b ascending in (out_a, out_b), each once, out_source 1 (covisibility) or 2 (similarity);
 * capacity is their room.  Per frame, each may be NULL: connected, registered, may_register (0 / 1), visible (the final mark counts).
 * cand (may be NULL, then cand_capacity and n_cand are not read): one row (id1, id2, shared matches, covisible patches) for every
 * directed candidate that passed the tests before GetMatcheNum (id2 in the list of id1, not itself, not tried, one of them
 * registered, both connected), ascending in (id1, id2).  The number of rank_ids bounds both *n_out and *n_cand.  stats [8], may be
 * NULL: rounds that registered a frame, tracks, valid tracks, correspondence entries, observations walked by the covisibility kernel
 * per pass, codes kept, passes per frame, 0.
 *
 * Errors: every check runs on the host before the device is touched and prints one line on stderr that names the entry; on any
 * negative code no output is touched.  XRSFM_BA_EINVAL: NULL opt or needed array; options out of range (patch_cols * patch_rows
 * outside 1..128, min_patch_obs outside {1, 2}, min_visible < 1, a negative threshold, ranks not ascending); an index out of range; a
 * pair with a == b; an unordered pair listed twice; a width or height below the patch grid; a key point whose patch index would be
 * negative or whose coordinate no int holds; the initial pair not among the pairs; a capacity below the need (the line names the
 * need).  XRSFM_BA_ETOOBIG: key points, matches or observations above INT32_MAX, or more frames than one workgroup's LDS holds
 * bits for.  n_frames == 0 is success with nothing out and needs no device; otherwise XRSFM_BA_ENODEV without one (no CPU path).
 * XRSFM_BA_EXPAND_WINDOW=W (read per call) lowers the third frames per pass of the covisibility kernel: a test aid. */
typedef struct {
    int32_t patch_cols;            /* 10  col_num                                                 */
    int32_t patch_rows;            /* 10  row_num                                                 */
    int32_t min_patch_obs;         /* 2   _T_: observations that make a (frame, patch) covisible  */
    int32_t min_visible;           /* 30  marks that register a frame in the simulation           */
    int32_t max_shared_matches;    /* 50  GetMatcheNum above this: the pair is skipped            */
    int32_t min_covisible_patches; /* 1                                                           */
    int32_t similarity_rank_max;   /* 40                                                          */
    int32_t mayreg_rank_lo;        /* 5   ranks up to here are counted and unused                 */
    int32_t mayreg_rank_mid;       /* 25  count2: ranks lo+1 .. mid                               */
    int32_t mayreg_rank_hi;        /* 50  count3: ranks mid+1 .. hi                               */
    int32_t mayreg_count_mid;      /* 15  count2 >= this, or                                      */
    int32_t mayreg_count_sum;      /* 35  count2 + count3 >= this                                 */
} xrsfm_ba_expand_options;
void xrsfm_ba_expand_options_default(xrsfm_ba_expand_options *opt);   /* the values above */

int xrsfm_ba_expand_candidates(const xrsfm_ba_expand_options *opt, int32_t n_frames, const int64_t *key_ptr, const float *keys,
                               const int32_t *width, const int32_t *height, int32_t n_pairs, const int32_t *pair_a,
                               const int32_t *pair_b, const int64_t *match_ptr, const int32_t *matches, const int64_t *rank_ptr,
                               const int32_t *rank_ids, int32_t n_tried, const int32_t *tried_a, const int32_t *tried_b,
                               int32_t init_a, int32_t init_b, int64_t capacity, int64_t *n_out, int32_t *out_a, int32_t *out_b,
                               uint8_t *out_source, uint8_t *connected, uint8_t *registered, uint8_t *may_register,
                               int32_t *visible, int64_t cand_capacity, int64_t *n_cand, int32_t *cand, int64_t *stats);

/* The same call on a resident frame set: the patches come from the key points on the device and no key point is uploaded.  The
 * patch check of the key points is made by the kernel here: XRSFM_BA_EINVAL after its launch, outputs untouched. */
int xrsfm_ba_frames_expand(const xrsfm_ba_frames *fs, const xrsfm_ba_expand_options *opt, const int32_t *width,
                           const int32_t *height, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                           const int64_t *match_ptr, const int32_t *matches, const int64_t *rank_ptr, const int32_t *rank_ids,
                           int32_t n_tried, const int32_t *tried_a, const int32_t *tried_b, int32_t init_a, int32_t init_b,
                           int64_t capacity, int64_t *n_out, int32_t *out_a, int32_t *out_b, uint8_t *out_source,
                           uint8_t *connected, uint8_t *registered, uint8_t *may_register, int32_t *visible,
                           int64_t cand_capacity, int64_t *n_cand, int32_t *cand, int64_t *stats);

/* ---- track completion and merging ----
 * Point3dProcessor::ContinueTrack and MergeTrack over every track (run_triangulation.cc:151-164) or MergeTracks(frame) of the
 * incremental mapper (incremental_mapper.cc:65-66; track_processor.cc:426-618), on three flat arrays that are read and written:
 * track_of_key [N] (Frame::track_ids_, frame-major as key_ptr; -1: none), points [n_tracks][3], track_outlier [n_tracks].  No track
 * is created.  One wave per connected component (key points; edges: correspondence entries and "same track") runs the reference's
 * own sequential program, so a track's and a key point's outputs do not depend on what else is in the call: the call may be given
 * any union of whole components of a map.
 *
 * Inputs: key_ptr [n_frames+1], key_xy [N][2] pixels; per frame registered (0 / 1), cam_q [n_frames][4] (x, y, z, w), cam_t
 * [n_frames][3], cam_intr (its camera); n_intr cameras with intr_model (0..4) and intr_params [n_intr][8] as in xrsfm_ba_problem;
 * corr_ptr [N+1] and corr_key [E]: the correspondence list of every key point in stored order, entries as global key indices
 * (CorrespondenceGraph::corrs_vector; symmetric, never into the key point's own frame).
 *
 * Outputs besides the three arrays, each may be NULL: track_status [n_tracks] (0 not in a processed component, 1 processed and
 * alive, 2 merged away, 3 in a component above the limits: such a component is not attempted and its state stays bit for bit);
 * corr_have_point3d [N] (the entries of a key point's list whose key point carries a track), visible [n_frames] (key points with
 * such an entry), measured [n_frames] (key points that carry a track), all three of the final state; stats [8]: merged tracks,
 * connected tracks, continued measurements, connected measurements (the counters MergeTracks prints), components processed,
 * components above the limits, key points of the largest processed component, 0.  Map modes process every component that holds
 * a track; frame mode those that hold a key point of the frame with a track.
 *
 * Errors: every check runs on the host before the device is touched and prints one line on stderr that names the entry; on any
 * negative code no output is touched.  XRSFM_BA_EINVAL: NULL opt or needed array; offsets not starting at 0 or decreasing; a key
 * or track index out of range; a key point carrying an outlier track; two key points of one frame on one track; a list entry
 * pointing into the key point's own frame; a non-symmetric list; a non-finite pose, point, coordinate or parameter;
 * max_reproj_error not positive; a mode outside {1, 2, 3, 4}; in frame mode a frame out of range or not registered; a model
 * outside 0..4.  XRSFM_BA_ETOOBIG: key points or entries above INT32_MAX.  Nothing to do (no key point, no track, or frame mode
 * on a frame without a track) is success and needs no device; otherwise XRSFM_BA_ENODEV without one (no CPU path). */
#define XRSFM_BA_MERGE_CONTINUE 1   /* ContinueTrack over every track                */
#define XRSFM_BA_MERGE_MERGE    2   /* MergeTrack over every track (3 = both, in the reference's order) */
#define XRSFM_BA_MERGE_FRAME    4   /* MergeTracks(frame)                             */
#define XRSFM_BA_MERGE_MAX_KEYS 1024   /* key points of a component k_merge_components attempts */
#define XRSFM_BA_MERGE_MAX_TRACKS 512  /* tracks of such a component                            */
typedef struct {
    double max_reproj_error;       /* 8.0  pixels (th_rpe_lba in the mapper)                      */
    int32_t mode;                  /* 3    XRSFM_BA_MERGE_*                                       */
    int32_t frame;                 /* -1   the frame of XRSFM_BA_MERGE_FRAME                      */
} xrsfm_ba_merge_options;
void xrsfm_ba_merge_options_default(xrsfm_ba_merge_options *opt);   /* 8.0, 3, -1: run_triangulation */

int xrsfm_ba_merge_tracks(const xrsfm_ba_merge_options *opt, int32_t n_frames, const int64_t *key_ptr, const double *key_xy,
                          const uint8_t *registered, const double *cam_q, const double *cam_t, const int32_t *cam_intr,
                          int32_t n_intr, const int32_t *intr_model, const double *intr_params, const int64_t *corr_ptr,
                          const int32_t *corr_key, int32_t n_tracks, double *points, uint8_t *track_outlier,
                          int32_t *track_of_key, uint8_t *track_status, int32_t *corr_have_point3d, int32_t *visible,
                          int32_t *measured, int64_t *stats);

/* TEST ENTRY, host only (needs no device).  The host's labelling of the components: comp_of_key [N], components numbered by size
 * (largest first, then by first key point), and their number.  Inputs and checks as in xrsfm_ba_merge_tracks. */
int xrsfm_ba_debug_merge_components(const xrsfm_ba_merge_options *opt, int32_t n_frames, const int64_t *key_ptr,
                                    const double *key_xy, const uint8_t *registered, const double *cam_q, const double *cam_t,
                                    const int32_t *cam_intr, int32_t n_intr, const int32_t *intr_model,
                                    const double *intr_params, const int64_t *corr_ptr, const int32_t *corr_key,
                                    int32_t n_tracks, const double *points, const uint8_t *track_outlier,
                                    const int32_t *track_of_key, int32_t *comp_of_key, int32_t *n_comp);

/* ---- frame triangulation ----
 * Point3dProcessor::TriangulateFramePoint (track_processor.cc:163-251) for a list of frames in the caller's order: the mapper passes
 * the frame it has just registered (incremental_mapper.cc:60), run_triangulation every registered frame ascending
 * (run_triangulation.cc:141-148).  The frames are processed one after another and each sees the state the earlier ones left; the
 * result is that of the sequential program.  The state is that of xrsfm_ba_merge_tracks, read and written: track_of_key [N], points
 * [track_capacity][3], track_outlier [track_capacity], of which the first n_tracks are in use; new tracks are appended.
 *
 * Within a frame the key points p with track_of_key == -1 are visited ascending.  The observations of p are the entries of its
 * correspondence list, in stored order, whose frame is registered, then (frame, p); with fewer than two p is skipped (status 2).
 *   create   no observation carries a track: CreatePoint3d1 on the observations, exactly what xrsfm_ba_triangulate_tracks computes
 *            for that list (status 3 above XRSFM_BA_TRI_MAX_OBS observations, 4 without a model).  On success (status 1) the new
 *            track gets the id "current number of tracks", its point is the model, its outlier flag 0, and track_of_key is set
 *            for the INLIER observations only (AddTrack).
 *   extend   otherwise (GetMaxAngle, ContinueTrackUpdate): candidates are the distinct tracks of the observations; one that already
 *            has a key point in this frame is skipped.  ray1 = (q X + t).normalized(), ray2 = (x_n, y_n, 1).normalized() (Eigen: a
 *            zero vector stays zero); the best candidate has the smallest angle acos(ray1 . ray2), the smaller id on equal angles;
 *            a NaN angle (a dot product above 1) is never best.  Below extend_angle_rad track_of_key[p] = best (status 5), else
 *            nothing happens (status 6).  No track is created in this branch, even when no track is eligible.
 * Documented deviation: no acos is evaluated on the device.  Candidates are ordered by the dot product (larger is better, the
 * smaller id on equal dot products) and accepted by dot >= the smallest double whose acos, by the host's libm, is below
 * extend_angle_rad.  The acceptance is the literal one; the order differs only where two different dot products have the same
 * acos (csrc/ba_trif_rule.h).
 *
 * Inputs as for xrsfm_ba_merge_tracks, but key_xyn [N][2] are NORMALISED coordinates (undistortion stays with the caller, as for
 * xrsfm_ba_triangulate_tracks) and no camera model is needed.  frame_list [n_list]: registered frames, none twice.
 * track_capacity must cover n_tracks plus the key points without a track of the listed frames that have two or more observations.
 *
 * Outputs besides the three arrays, each may be NULL: n_tracks_out; key_status [N] (0 not visited, 1 created, 2 fewer than two
 * observations, 3 above the observation limit, 4 no model, 5 extended, 6 tracks seen, none accepted); num_inliers, num_trials,
 * best_trial [N]: the diagnostics of xrsfm_ba_triangulate_tracks for the key points of the create branch with status 1 or 4
 * (elsewhere 0, 0, -1); corr_have_point3d [N], visible and measured [n_frames] of the final state, as for xrsfm_ba_merge_tracks;
 * stats [8]: created, key points of the create branch, extended, key points that saw one track, that saw several (the five
 * counters the reference prints), steps, listed frames that needed more than one step, the most claim rounds of a step.
 *
 * Two key points of a frame whose lists share an entry are coupled (a track the first creates changes the second's branch): the
 * host cuts a frame into maximal runs without a coupled pair, one step each; one-to-one matches give one step per frame.
 *
 * Errors: every check runs on the host before the device is touched and prints one line on stderr that names the entry; on any
 * negative code no output is touched.  XRSFM_BA_EINVAL: NULL opt or needed array; a negative count; offsets not starting at 0 or
 * decreasing; a key or track index out of range; a listed frame out of range, not registered or listed twice; a key point carrying
 * an outlier track; a list entry pointing into the key point's own frame; a non-symmetric list; a non-finite pose, point,
 * coordinate or option; extend_angle_rad outside [0, 3.2]; the option faults of xrsfm_ba_triangulate_tracks; track_capacity below
 * the bound above.  XRSFM_BA_ETOOBIG: key points or entries above INT32_MAX.  Nothing to do (no listed frame, or none of their key
 * points without a track has two observations) is success and needs no device; otherwise XRSFM_BA_ENODEV without one. */
typedef struct xrsfm_ba_trif_options {
    double extend_angle_rad;       /* DegToRad(8.0)   run_triangulation.cc:144 */
    xrsfm_ba_tri_options tri;      /* xrsfm_ba_triangulate_options: CreatePoint3d1 */
} xrsfm_ba_trif_options;
void xrsfm_ba_trif_options_default(xrsfm_ba_trif_options *opt);

int xrsfm_ba_triangulate_frames(const xrsfm_ba_trif_options *opt, int32_t n_frames, const int64_t *key_ptr, const double *key_xyn,
                                const uint8_t *registered, const double *cam_q, const double *cam_t, const int64_t *corr_ptr,
                                const int32_t *corr_key, int32_t n_list, const int32_t *frame_list, int32_t n_tracks,
                                int32_t track_capacity, double *points, uint8_t *track_outlier, int32_t *track_of_key,
                                int32_t *n_tracks_out, uint8_t *key_status, int32_t *num_inliers, int32_t *num_trials,
                                int32_t *best_trial, int32_t *corr_have_point3d, int32_t *visible, int32_t *measured,
                                int64_t *stats);

/* profile != 0 in the last xrsfm_ba_run: per-kernel totals measured with HIP events on the
 * library's stream.  Returns 0 and fills the outputs for index < number of kernel classes,
 * XRSFM_BA_EINVAL past the end. */
int xrsfm_ba_profile_entry(xrsfm_ba_context *ctx, int index, const char **name, double *total_ms, int *launches);

/* ---- test/diagnostic entry points (kernel-level parity against the oracle) ---- */

/* Linearise at the current state with Jacobi scaling `use_scaling` (0: scale = 1).
 * Outputs are in the caller's observation / point / camera order; any may be NULL.
 *   r [n_obs][2], Jc [n_obs][2][6], Jp [n_obs][2][3]   robustified, scaled
 *   Hpp [n_points][6] (upper: 00 01 02 11 12 22), gp [n_points][3]
 *   Hcc_diag [n_cams][6], gc [n_cams][6], *cost */
int xrsfm_ba_debug_linearize(xrsfm_ba_context *ctx, double huber_a, int use_scaling, double *r, double *Jc,
                             double *Jp, double *Hpp, double *gp, double *Hcc_diag, double *gc, double *cost);

/* After debug_linearize: y = S(radius) * x for a caller vector x [n_cams][6]; also returns rhs b [n_cams][6]. */
int xrsfm_ba_debug_schur_product(xrsfm_ba_context *ctx, double radius, const double *x, double *y, double *b);

/* Host-side packing only (no GPU needed): runs the track-tile packing of xrsfm_ba_create and reports
 * stats[0] tiles, [1] slots (= 64*tiles), [2] work items, [3] regular tiles, [4] long items (tracks > 64 observations),
 * [5] camera-major partial entries, [6] longest track, [7] active points.  slot_obs (may be NULL) receives, for each of
 * the `slots` slots, the caller's observation index stored there or -1 for padding; it must hold n_obs + 64*(n_points+1)
 * entries at most (upper bound of the slot count). */
int xrsfm_ba_debug_pack(const xrsfm_ba_problem *problem, int32_t stats[8], int32_t *slot_obs);

/* The S-assembly side of the packing (no GPU needed): Gram tiles and the item classes of k_schur_pairs.
 * stats[0] Gram tiles, [1] cells of their C x C destination tables, [2] camera-major entries of the S assembly (one per
 * distinct camera of a Gram tile), [3] largest C, [4]/[5]/[6] items in the small-LDS Gram class / big-LDS Gram class /
 * per-pair + long class, [7] partial blocks written per pass.  tile_ncam (may be NULL): [tiles]; slot_cidx (may be NULL):
 * [slots], 255 outside Gram tiles; slot_campos_g (may be NULL): [slots], -1 for non-writers. */
/* Tile groups of the S assembly's merged Gram launch (G tiles per workgroup) on the host-packed tables: per launch position its tile
 * and code (index in its run | run length << 4), per tile L and the cameras / cidx of its first min(L, 4) slots ([n_tiles][4], -1
 * beyond), stats = {positions, camera entries, camera entries kept}, cam_ptr_s [n_cams + 1]. */
int xrsfm_ba_debug_sgroup(const xrsfm_ba_problem *problem, int G, int32_t stats[3], int32_t *pos_tile, int32_t *pos_code,
                          int32_t *tile_stride, int32_t *tile_cams, int32_t *tile_cidx, int32_t *cam_ptr_s);
int xrsfm_ba_debug_pack_gram(const xrsfm_ba_problem *problem, int32_t stats[8], int32_t *tile_ncam, uint8_t *slot_cidx,
                             int32_t *slot_campos_g);

/* TEST ENTRY (no GPU needed): the schedule of 4x4 result blocks by which k_schur_pairs forms the camera-pair blocks of a Gram tile
 * of n_cams cameras (6 operand rows per camera, groups of 4 rows; csrc/ba_chol.h: gram_tile4).  entries [4 * *n_inst]: four blocks
 * per matrix instruction, row group | column group << 8, padded with block (0, 0).  *n_inst = 0 when the tile takes the 16x16 form
 * (more than 6 instructions).  Returns XRSFM_BA_EINVAL for n_cams outside 1..10; entries must hold 128 values. */
int xrsfm_ba_debug_gram_schedule(int n_cams, int32_t *n_inst, int32_t *n_inst_all, uint16_t *entries);

/* Host-side plan of the Cholesky path (no GPU needed): stats[0] tiles T, [1] elimination-tree levels, [2] ordering
 * (0 natural, 1 nested dissection of a band/ring, 2 reverse Cuthill-McKee of an unordered collection, 3 nested dissection of an unordered collection's camera graph), [3] hub cameras, [4] band width in cameras, [5] off-diagonal blocks,
 * [6] schedule BITS: bit 0 (value 1) = level schedule (one launch per elimination-tree level; clear = the panel schedule of
 * deep elimination trees: dense / unordered patterns), bit 1 (value 2) = look-ahead panel schedule (one launch per tile
 * column, k_panel_slot) — test the bits, not the value: a look-ahead plan reports 2, [7] structurally
 * non-zero tiles after fill.  cam_offset (may be NULL):
 * [n_cams] first row of each camera in the elimination order.  facts (may be NULL): [16] the schedule facts of
 * xrsfm_ba_debug_reduced_system, as far as the plan and the environment decide them. */
int xrsfm_ba_debug_chol_plan(const xrsfm_ba_problem *problem, int32_t stats[8], int32_t *cam_offset, int32_t *facts);

/* TEST ENTRY: device-side packing (large problems: xrsfm_ba_create sorts and lays out the observations on the GPU) against the host
 * packing it replaces: packs `problem` both ways and compares every array.  Returns 0 with *field = 0 when they are identical,
 * *field > 0 = the first array that differs (see xrsfm_ba.hip), *field = -100 when the device path declines the problem. */
int xrsfm_ba_debug_device_pack_check(const xrsfm_ba_problem *problem, int32_t *field, int32_t *index);

/* Multi-GPU emulation for tests: supply the union of all ranks' off-diagonal camera pairs (row > col) before the first
 * Cholesky solve, exactly what xrsfm_ba_run obtains with an all-reduce when n_ranks > 1. */
int xrsfm_ba_debug_set_block_pattern(xrsfm_ba_context *ctx, int n_pairs, const int32_t *row_col);

/* After debug_linearize: solve S(radius) y = b with the Cholesky path; y [n_cams][6].  If S_dense != NULL it
 * receives the assembled reduced camera matrix before factorisation, [6 n_cams][6 n_cams] row-major, symmetric. */
int xrsfm_ba_debug_cholesky_solve(xrsfm_ba_context *ctx, double radius, double *y, double *S_dense);

/* TEST ENTRY.  After debug_linearize (bal9 contexts: after debug_wide): the damped reduced system S(radius) y = b exactly as the
 * tile factorisation reads it, and optionally its solution by the same factorisation.  Runs the set-up, the step preparation and the
 * assembly with a materialised tile storage (k_tile_fill), like debug_cholesky_solve with S_dense.  Outputs in camera order with
 * cw = 6 (9 in bal9 mode) unknowns per camera: diag [n_cams][cw][cw] the diagonal blocks; blk_rc [n_blocks][2] the structurally
 * non-zero off-diagonal blocks (row camera > column camera) and blk [n_blocks][cw][cw] their values, block (row, column) of S;
 * b [n_cams][cw]; y [n_cams][cw] (may be NULL: no factorisation).  *n_blocks: capacity in, block count out; with blk_rc, blk, diag
 * or b NULL only the set-up runs and the count and facts are returned.  Leaves no solved step behind (debug_backsub refuses).
 * facts [16]: [0] tile columns T, [1] levels, [2] ordering (as debug_chol_plan), [3] schedule (0 level, 1 panel, 2 look-ahead
 * panel), [4] levels with a macro-panel launch (k_panel2_part), [5] split levels (partials + fixed-order sum), [6] level
 * look-ahead depth, [7] tiles composed outside the first level's columns, [8] 1 = those get a launch of their own (k_tile_fill:
 * more than 4096 of them on a level schedule), [9] 1 = packed tile storage, [10] backward substitution (0 only inside the
 * last factor launch, 1 one launch per level, 2 one launch for all levels, 3 per level in chunks, 4 push form), [11] bit m set =
 * a tile column holds m cameras, [12] cw, [13] off-diagonal blocks, [14] unknowns, [15] structurally non-zero tiles. */
int xrsfm_ba_debug_reduced_system(xrsfm_ba_context *ctx, double radius, int32_t facts[16], int32_t *n_blocks, int32_t *blk_rc,
                                  double *blk, double *diag, double *b, double *y);

/* bal9 contexts: linearise at the current state with Jacobi scaling (cost; per observation r [n_obs][2], Jc [n_obs][2][9],
 * Jp [n_obs][2][3]; per camera diag(Hcc), g_c [n_cams][9]) and, if y != NULL, solve the reduced system at `radius`
 * (y [n_cams][9], scaled coordinates).  Any output pointer may be NULL. */
int xrsfm_ba_debug_wide(xrsfm_ba_context *ctx, double huber_a, double radius, double *cost, double *r, double *Jc, double *Jp,
                        double *Hcc_diag, double *gc, double *y);

/* After debug_cholesky_solve (bal9 contexts: after a debug_wide that solved a step, y != NULL, which launches k9_backsub at that
 * radius): one back-substitution (k_backsub) from the camera solution it left.  Outputs in the
 * library's PACKED order (for comparing two builds of the library on the same problem, tools/backsub_waves_probe.py):
 * per work item the model-decrease and squared point-step partials [n_items] (n_items = debug_pack stats), candidate
 * points and scaled point steps [n_points_packed][3], candidate cameras [n_cams][4] / [n_cams][3].  Any pointer may be NULL. */
int xrsfm_ba_debug_backsub(xrsfm_ba_context *ctx, double *part_model, double *part_step2, double *cand_points,
                           double *point_step, double *cand_cam_q, double *cand_cam_t);

/* TEST ENTRY.  What a context holds next to the packed-order outputs of debug_backsub, so that a caller can put them into its
 * own order; every output may be NULL.  pt_orig [n_points_packed]: the caller's point index of every packed point.  item_tiles
 * [n_items][2]: first tile and number of tiles of every work item (with slot_obs of debug_pack: the caller's observations of the
 * item, 64 slots per tile).  flags [2]: [0] 1 = the last step's kernels form the point factors themselves (k_backsub<true>;
 * always 1 for bal9 contexts), [1] 1 = the per-observation residual and Jacobian are stored (always 1 for bal9 contexts).
 * Of the last debug_backsub on the current step (XRSFM_BA_ESTATE without one): campart [2][n_cams] the per-camera squared step
 * and squared norm partials; cand_intr [n_cams][3] the candidate {f, k1, k2} (bal9 contexts; the current values otherwise).
 * Of the current linearisation (XRSFM_BA_ESTATE without one): the Jacobi scales scale_c [n_cams][cw], cw = 6 (9 for bal9
 * contexts), and scale_p [n_points_packed][3]. */
int xrsfm_ba_debug_backsub_layout(xrsfm_ba_context *ctx, int32_t *pt_orig, int32_t *item_tiles, double *campart, int32_t flags[2],
                                  double *cand_intr, double *scale_c, double *scale_p);

/* TEST ENTRY.  counts = {tiles whose camera records k_backsub stages in LDS once per tile, tiles whose lanes gather their camera's
 * operands themselves}: single-tile Gram items of at most 8 cameras take the first route unless the environment says
 * XRSFM_BA_CAM_STAGE=0 (read when the context is created); bal9 contexts report {0, 0}.  Counted on the host with the predicate
 * the kernels evaluate (cam_staged), not by the kernels.  The merged k_schur_pairs launch stages the same tiles; with
 * XRSFM_BA_GRAM_MERGE=0 there is no merged launch and the S assembly gathers every tile, whatever this entry reports. */
int xrsfm_ba_debug_cam_stage(xrsfm_ba_context *ctx, int32_t counts[2]);

/* Whether the context currently keeps the per-observation residual and Jacobian stored (1) or recomputes them in the
 * consumers (0, the J-free linearisation of the Cholesky path): after xrsfm_ba_run, the mode its last iterations used. */
int xrsfm_ba_debug_stored_j(xrsfm_ba_context *ctx, int32_t *stored);

/* TEST ENTRY.  The scalars the LM controller decides on, of the context's current linearisation (after xrsfm_ba_debug_linearize
 * or xrsfm_ba_debug_wide; XRSFM_BA_ESTATE without one): out = {sum of rho (twice the cost), |x_points|^2 over the variable points
 * that have an observation, the gradient max-norm over the points, the gradient max-norm over the cameras}.  Fetched the way
 * xrsfm_ba_run fetches them after iteration 0: a fused context reads what the tail of the linearisation left, an unfused or
 * bal9 context launches the camera gradient kernel. */
int xrsfm_ba_debug_lin_scalars(xrsfm_ba_context *ctx, double out[4]);

/* TEST ENTRY.  xrsfm_ba_run with linear_solver = XRSFM_BA_SOLVER_RESIDENT (the field of opt is ignored): the same single launch,
 * the same state and summary bit for bit, plus the iteration rows the kernel keeps for the progress table.  rows
 * [max_iterations + 1][7] = {cost, cost change, gradient max-norm, step norm, rho, radius after the decision, iteration}: one row
 * per evaluated point (iteration 0 and every accepted step) and one per rejected or invalid step; a tolerance exit writes none.
 * *n_rows: how many were written.  The refusals of the resident solver apply (XRSFM_BA_EINVAL, nothing written). */
int xrsfm_ba_debug_resident_rows(xrsfm_ba_context *ctx, const xrsfm_ba_options *opt, xrsfm_ba_summary *summary, double *rows, int32_t *n_rows);

/* TEST ENTRY, host only (needs no device).  The tracks that match expansion builds from the pairs in list order (MakeTrack /
 * AddTrack): key_track [N] (-1, or a track, which may be invalid), *n_tracks, track_ptr [track_capacity+1], invalid
 * [track_capacity], obs_frame and obs_key [obs_capacity] ascending by frame within a track (obs_key: the key point within its
 * frame).  *n_tracks <= M and *n_obs <= 2 M for M matches.  Argument checks as in xrsfm_ba_expand_candidates; a capacity below the
 * need is XRSFM_BA_EINVAL and the line names it. */
int xrsfm_ba_debug_expand_tracks(int32_t n_frames, const int64_t *key_ptr, int32_t n_pairs, const int32_t *pair_a,
                                 const int32_t *pair_b, const int64_t *match_ptr, const int32_t *matches, int32_t *key_track,
                                 int64_t track_capacity, int64_t *n_tracks, int64_t *track_ptr, uint8_t *invalid,
                                 int64_t obs_capacity, int64_t *n_obs, int32_t *obs_frame, int32_t *obs_key);

/* TEST ENTRY.  What k_expand_covis leaves: per frame (unconnected frames: nothing) the ascending codes t * patches + patch of
 * the (third frame t, patch) seen min_patch_obs times or more: code_ptr [n_frames+1], codes [code_capacity].  Arguments and checks
 * as in xrsfm_ba_expand_candidates. */
int xrsfm_ba_debug_expand_covis(const xrsfm_ba_expand_options *opt, int32_t n_frames, const int64_t *key_ptr, const float *keys,
                                const int32_t *width, const int32_t *height, int32_t n_pairs, const int32_t *pair_a,
                                const int32_t *pair_b, const int64_t *match_ptr, const int32_t *matches, int32_t init_a,
                                int32_t init_b, int64_t code_capacity, int64_t *code_ptr, int32_t *codes);

#ifdef __cplusplus
}
#endif
#endif /* XRSFM_BA_H */
