/*
 * penguin_hip.h -- C ABI of libpenguin_hip.so: the MI355X (gfx950) implementation of
 * Penguin.jl's hot path  Mesh -> Capacity -> DiffusionOps -> DiffusionUnsteadyMono/Diph ->
 * solve_DiffusionUnsteady*!.
 *
 * The reference (100 % Julia) has no FFI for this path; its boundary is the exported Julia API
 * (src/Penguin.jl:25-75).  Each entry point below names the reference item it replaces
 * (paths relative to the reference tree).  julia/PenguinHIP.jl ccall's exactly these symbols;
 * penguin/jl_amd/_lib.py binds the same symbols with ctypes.  See INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int32 status, 0 = ok; on failure pg_last_error() holds a
 *     thread-local message (the Julia wrapper turns it into error(msg)).
 *   - handles are opaque and owned by the library; every array argument is a HOST pointer
 *     owned by the caller and borrowed for the duration of the call only.
 *   - all fields live on the padded node grid  M = prod(n_d + 1), linear index
 *     i + j*(nx+1) + k*(nx+1)*(ny+1) (0-based here; src/solver.jl:362-372, src/utils.jl:21).
 *   - float64 / int64 across the ABI (SparseMatrixCSC{Float64,Int}).  No torch types.
 *   - one process drives one GPU; with nranks > 1 every rank owns a slab of planes of the
 *     slowest dimension and the library exchanges halos / dot products over RCCL itself.
 *   - handles are not thread-safe; one call at a time per handle.
 */
#ifndef PENGUIN_HIP_H
#define PENGUIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_mesh pg_mesh;         /* Penguin.Mesh{N}            src/mesh.jl:41-79        */
typedef struct pg_capacity pg_capacity; /* Penguin.Capacity{N}        src/capacity.jl:25-36    */
typedef struct pg_diffops pg_diffops;   /* Penguin.DiffusionOps{N}    src/operators.jl:49-55   */
typedef struct pg_solver pg_solver;     /* Penguin.Solver             src/solver.jl:33-42      */
typedef struct pg_streamvort pg_streamvort; /* Penguin.StreamVorticity{2} src/solver/streamfunction_vorticity.jl:37-54 */

/* ---- enums --------------------------------------------------------------------------- */
enum { PG_BODY_BALL = 1, PG_BODY_MULTIBALL = 2, PG_BODY_HALFSPACE = 3, PG_BODY_ELLIPSOID = 4, PG_BODY_PLANE = 5 }; /* closed-form level sets evaluated in-kernel */
enum { PG_BODY_PROGRAM = 6 };                     /* a traced level set: pg_capacity_create_program */
enum { PG_BODY_POLYGON = 7 };                     /* a closed polygon of markers: pg_capacity_create_polygon */
enum { PG_FLAG_COMPLEMENT = 1, PG_FLAG_NO_CENTROIDS = 2 };
/* capacity fields for pg_capacity_get (d = dimension for A,B,W,C_omega,C_gamma) */
enum { PG_CAP_V = 0, PG_CAP_GAMMA = 1, PG_CAP_CELL_TYPES = 2, PG_CAP_A = 3, PG_CAP_B = 4,
       PG_CAP_W = 5, PG_CAP_C_OMEGA = 6, PG_CAP_C_GAMMA = 7,
       /* space-time capacities only: A_(N+1) at the lower / upper time face ("Vn_1", "Vn"), time component of C_ω / C_γ */
       PG_CAP_ST_V0 = 8, PG_CAP_ST_V1 = 9, PG_CAP_ST_CT_OMEGA = 10, PG_CAP_ST_CT_GAMMA = 11 };
enum { PG_OP_G = 0, PG_OP_H = 1, PG_OP_WINV = 2,
       PG_OP_C0 = 3 /* C_d: PG_OP_C0 + d */, PG_OP_K0 = 6 /* K_d: PG_OP_K0 + d */ };   /* ConvectionOps */
/* interface / border condition kinds                         src/boundary.jl:12-50 */
enum { PG_BC_NONE = 0, PG_BC_DIRICHLET = 1, PG_BC_NEUMANN = 2, PG_BC_ROBIN = 3, PG_BC_PERIODIC = 4 };
/* border keys, in the reference's (unusual) naming           src/solver.jl:379-409 */
enum { PG_KEY_LEFT = 0 /* dim2 = 1 */, PG_KEY_RIGHT = 1 /* dim2 = n2 */, PG_KEY_BOTTOM = 2 /* dim1 = 1 */,
       PG_KEY_TOP = 3 /* dim1 = n1 */, PG_KEY_BACKWARD = 4 /* dim3 = 1 */, PG_KEY_FORWARD = 5 /* dim3 = n3 */ };
enum { PG_SCHEME_BE = 0, PG_SCHEME_CN = 1,                   /* "BE" / "CN" strings of the reference */
       PG_SCHEME_STEADY = 2 };                                /* internal: the steady constructors */
enum { PG_SV_PSI = 0, PG_SV_OMEGA = 1, PG_SV_U = 2, PG_SV_V = 3 };   /* fields / systems of a pg_streamvort */
enum { PG_METHOD_BICGSTAB = 0, PG_METHOD_CG = 1, PG_METHOD_GMRES = 2, PG_METHOD_BICGSTABL = 3,
       PG_METHOD_IDRS = 4 };   /* IterativeSolvers methods
   kept: bicgstab (also serves `\`, bicgstabl when no l is given and idrs when no s is given), cg, gmres (solve_system!'s default,
   src/solver.jl:158),
   bicgstabl with l = pg_krylov_opts.restart (BiCGStab(l), DESIGN.md "BiCGStab(l)"): opt-in, one rank, zero initial guess
   (warm_start is ignored), plain -- refused together with precond = m >= 1, PG_PRECOND_MG, PG_PRECOND_MG_CELL,
   PG_PRECOND_MG_STEP or PG_PRECOND_POLY_EST; with precond = 0 or -1 it runs unpreconditioned.  Its `iters` count BiCG sub-steps, two products each
   (the unit of BiCGStab's iterations: l = 1 is directly comparable) and maxiter caps that unit (no outer iteration starts at
   iters >= maxiter); products = 2 iters + the products that confirm the true residual before convergence is reported;
   idrs with s = pg_krylov_opts.restart (IDR(s) with biorthogonalisation, DESIGN.md "IDR(s)"; replaces `idrs` of IterativeSolvers
   passed through solve_system!, src/solver.jl:158-188): s <= 0 means 8 (IterativeSolvers' default), s > 8 is refused; opt-in, one
   rank, plain -- refused together with precond = m >= 1, PG_PRECOND_MG, PG_PRECOND_MG_CELL, PG_PRECOND_MG_STEP or
   PG_PRECOND_POLY_EST; with precond = 0 or -1 it runs unpreconditioned.  With warm_start != 0 a steady re-solve and a time
   step start from the previous state.  Its `iters` count updates of x, one product each, and maxiter caps exactly that unit
   (<= 0: 200000); products = iters + restarts + confirmations of the true residual (+ 1 for the product of a warm start) */

/* ---- plain structs ------------------------------------------------------------------- */
typedef struct {
  int32_t kind;   /* PG_BC_DIRICHLET / NEUMANN / ROBIN   (build_I_bc, src/solver.jl:203-223) */
  double alpha;   /* Robin only */
  double beta;    /* Robin only */
  double value;   /* constant value, used when value_array == NULL */
  const double* value_array; /* M host values g(C_gamma, t) or NULL (build_g_g, src/solver.jl:293-323) */
} pg_bc_desc;

typedef struct {
  int32_t key;    /* PG_KEY_*  */
  int32_t kind;   /* PG_BC_DIRICHLET / PERIODIC / NEUMANN(1-D only)  (src/solver.jl:450-499) */
  double value;   /* constant; per-cell values may be set later with pg_solver_set_border_values */
} pg_border_desc;

typedef struct {
  double alpha1, alpha2, g;  /* ScalarJump  src/boundary.jl:96-100 ; row 2 of the 4-block system */
  double beta1, beta2, h;    /* FluxJump    src/boundary.jl:111-115; row 4 */
  const double* g_array;     /* M values or NULL */
  const double* h_array;     /* M values or NULL */
} pg_jump_desc;

typedef struct {
  int32_t method;   /* PG_METHOD_*                                  */
  double reltol;    /* ||r|| <= max(reltol*||b||, abstol)            */
  double abstol;
  int32_t maxiter;  /* <= 0: size of the reduced system              */
  int32_t check_every; /* host convergence poll period in iterations (<=0: default 4) */
  int32_t warm_start;  /* != 0: pg_solver_step starts BiCGStab from the previous time level instead of zero
                          (IterativeSolvers starts from zero; same solution to reltol, fewer iterations) */
  int32_t restart;     /* GMRES: Krylov vectors per restart cycle (<= 0: 20, IterativeSolvers' default);
                          BiCGStab(l): l, <= 0 means 2, more than 8 is refused */
  int32_t precond;     /* BiCGStab only: polynomial right preconditioner in Â (DESIGN.md "Krylov driver").  0: automatic
                          (on where Gershgorin bounds the spectrum; degree 6 for a first solve, then chosen per solve of the
                          warm time loop from the previous solve's convergence rate, 4 .. 32); -1: off (the plain
                          iteration IterativeSolvers runs); m >= 1: m products with Â per application where admissible (<= 40);
                          PG_PRECOND_MG: the aggregation multigrid V-cycle (DESIGN.md "Multigrid") -- steady monophasic diffusion
                          with a Dirichlet interface and the stream-function solve of a pg_streamvort, one rank; refused with an
                          error that names the failed condition anywhere else, never replaced by another iteration.  Such a
                          solve reports poly_degree = 0 and poly_xspace = 0 like a plain one (pg_solver_mg_info tells whether a
                          hierarchy exists); with profiling on, each V-cycle counts as one lean launch in spmv_lean_*;
                          PG_PRECOND_MG_CELL: the same V-cycle on a cell-aggregated hierarchy (DESIGN.md "Cell-aggregated
                          multigrid") -- steady monophasic diffusion (DarcyFlow included) with a Dirichlet, Robin or Neumann
                          interface, one rank; refused like PG_PRECOND_MG anywhere else, a pg_streamvort included;
                          PG_PRECOND_POLY_EST: the polynomial preconditioner of precond = 0, admitted on an estimated spectral disc
                          where Gershgorin refuses it (DESIGN.md "Estimated spectral interval") -- diphasic systems and Robin /
                          Neumann interfaces of the unsteady diffusion solvers.  Where Gershgorin admits the matrix the solve IS
                          the precond = 0 solve and no estimate runs; where it refuses, the first solve on a matrix runs 30
                          Arnoldi steps (pg_solver_spectral_estimate) and the polynomial runs on |z - 1| <= g_ritz + margin when
                          that is < 0.95, the plain iteration otherwise (no error).  One rank, BiCGStab, DiffusionOps, no moving
                          body: refused with an error that names the failed condition anywhere else;
                          PG_PRECOND_MG_STEP: the cell-aggregated V-cycle INSIDE the unsteady time loop (DESIGN.md "Multigrid in
                          the time loop"), meant for steps far above h² where the system approaches the Poisson system --
                          DiffusionUnsteadyMono (DarcyFlowUnsteady included; Dirichlet, Robin or Neumann interface) and
                          DiffusionUnsteadyDiph, BE and CN, DiffusionOps, one rank, BiCGStab.  One hierarchy per assembled matrix (pg_solver_mg_step_info); the
                          iteration runs on the full system, warm-started from the previous state.  Refused with an error that
                          names the failed condition anywhere else (steady and moving solvers, a ConvectionOps, a
                          pg_streamvort, CG / GMRES / BiCGStab(l)) and where a coarse diagonal entry is not positive; reports
                          like the other multigrid solves */
} pg_krylov_opts;
enum { PG_PRECOND_MG = -2 };   /* a value of pg_krylov_opts.precond */
/* a value of pg_krylov_opts.precond: multigrid whose first coarsening merges ALL unknowns, bulk and interface, of a 2 x 2 (x 2)
   block of cells into one coarse unknown.  With a Robin or Neumann interface the interface rows are equations of their own and
   the kind-separated aggregates of PG_PRECOND_MG give non-positive coarse diagonals; this rule serves those systems.  A solver
   holds one hierarchy per value: a solve with one neither reuses nor disturbs the other's. */
enum { PG_PRECOND_MG_CELL = -3 };
/* a value of pg_krylov_opts.precond: the polynomial preconditioner of precond = 0, admitted on an estimated spectral disc where
   Gershgorin refuses it.  Opt-in; a flag of its own on the matrix: nothing else that Gershgorin's verdict switches on (the
   elimination of rows alone on their diagonal, the compact loop system) starts because of it. */
enum { PG_PRECOND_POLY_EST = -4 };
/* a value of pg_krylov_opts.precond: the V-cycle of PG_PRECOND_MG_CELL as right preconditioner of the time steps of an unsteady
   diffusion solver, monophasic or diphasic.  A name of its own: PG_PRECOND_MG and PG_PRECOND_MG_CELL keep refusing every unsteady system.  Its
   hierarchies (one for the constructor's system, one for the run system) are its own as well. */
enum { PG_PRECOND_MG_STEP = -5 };
/* added to the largest |theta - 1| of the Ritz values before the test against 0.95: twice the largest shortfall of the estimate
   against the true spectrum measured on the oracle's systems (DESIGN.md "Estimated spectral interval" has the table) */
#define PG_SPECEST_MARGIN 0.0205

/* the spectral estimate of one matrix of a solver (pg_solver_spectral_estimate) */
typedef struct {
  int32_t steps;              /* Arnoldi steps taken (30, or fewer after a happy breakdown); 0: no estimate has run       */
  int32_t admitted;           /* 1: g_used < 0.95 -- PG_PRECOND_POLY_EST runs the polynomial on this matrix               */
  int32_t gershgorin_admits;  /* 1: Gershgorin admits the matrix (pg_system_info.neumann_ok): the estimate is not used    */
  int32_t reserved;
  double g_ritz;              /* max |theta - 1| over the Ritz values theta (complex modulus)                              */
  double g_used;              /* g_ritz + margin: the radius the Chebyshev nodes are placed on                             */
  double margin;              /* PG_SPECEST_MARGIN                                                                         */
  double gershgorin;          /* pg_system_info.gershgorin of the same matrix                                              */
  double ritz_re_min, ritz_re_max, ritz_im_max;   /* smallest / largest real part, largest |imaginary part| of the Ritz values */
  double estimate_ms;         /* wall time the estimate took (once per assembled matrix)                                   */
} pg_specest_info;

/* the multigrid hierarchy of a solver (pg_solver_mg_info), built by the first solve that asks for PG_PRECOND_MG */
#define PG_MG_MAX_LEVELS 16
typedef struct {
  int32_t levels;                    /* 0: no hierarchy has been built                                             */
  int32_t tail_level;                /* first level of the fused tail: the levels [tail_level, levels) run in one launch by one
                                        workgroup with their vectors in LDS; the last level is solved exactly there  */
  int64_t rows[PG_MG_MAX_LEVELS];    /* per level; level 0 is the Krylov matrix Â itself                            */
  int64_t nnz[PG_MG_MAX_LEVELS];
  double setup_ms;                   /* wall time of the set-up (device kernels + the host inverse of the last level) */
  int64_t bytes;                     /* device memory held by the hierarchy (level 0's matrix not counted)           */
} pg_mg_info;

typedef struct {
  int32_t iters;      /* Krylov iterations of this step                        */
  int32_t converged;
  double resnorm;     /* final ||r||                                           */
  double bnorm;
  double extremum;    /* maximum(abs.(s.x)) -- the "Solver Extremum" line, src/solver/diffusion.jl:279 */
  double time;        /* t after the step (fp64 accumulation t += dt, :287)     */
} pg_step_info;

typedef struct {
  int64_t steps;            /* number of loop iterations executed (states = steps + 1)         */
  int64_t total_iters;
  double t_final;
  double extremum;
  double solve_ms;          /* wall time of the whole run on this rank                          */
  /* profiling (pg_set_profiling(1)): HIP-event time of the sampled SpMV launches that carry fused dots (the plain
     iteration's only kind; with the polynomial preconditioner the launch that closes each chain of products)      */
  double spmv_ms_total;
  int64_t spmv_launches;
  int64_t unconverged_steps; /* solves of this run that ended without meeting the tolerance (maxiter / breakdown) */
  double worst_relres;       /* max over the run's solves of ||r|| / ||b|| at exit                                */
  double spmv_lean_ms_total; /* profiling: the sampled LEAN launches -- factors of the preconditioner polynomial, one   */
  int64_t spmv_lean_launches;/* vector in, one out, no dots (DESIGN.md "Krylov driver")                                 */
  int64_t poly_degree;       /* products with Â per application of the preconditioned operator in the last solve (0: plain) */
  int64_t half_exits;        /* solves that met the tolerance after the first half of their last iteration (such an
                                iteration counts as one in total_iters but runs only one application of the operator)  */
  int64_t poly_xspace;       /* 1: the last solve ran the polynomial preconditioner: the m - 1 launches of a chain are Horner
                                steps (x, the chain's input and the matrix in, one vector out; the first of a chain reads one
                                vector) and the iteration updates x itself; 0: plain iteration                                   */
  int64_t products;          /* products with the system matrix inside the run's solves (the one product per step that builds the
                                right-hand side and the start residual not counted)                                             */
  int64_t guess_states_read; /* older states read by the extrapolated starts of the run's quiet steps (pg_solver_guess_info):
                                each is two more vector reads of the step's first kernel                                        */
  /* mixed-precision Horner chain (PG_POLY_F32): */
  int64_t poly_f32_launches; /* Horner launches that read or wrote an fp32 vector (first, middle and hand-over launches)        */
  double poly_f32_ms_total;  /* profiling: HIP-event time of the sampled ones -- a bracket of their own: spmv_lean_* keeps the  */
  int64_t poly_f32_timed;    /* fp64 Horner launches only -- and how many launches that time covers                             */
  int64_t poly_f32_chains;   /* applications of the preconditioner that ran the mixed chain                                      */
  int64_t poly_f32_tail_sum; /* sum over those of j, the launches of the chain's fp64 tail (hand-over included)                  */
} pg_run_info;

typedef struct {
  int64_t n_own;      /* rows of the reduced system owned by this rank (n of BASELINE.md)       */
  int64_t nnz;        /* stored entries of those rows                                           */
  int64_t n_ghost;    /* ghost unknowns received from neighbours per SpMV                       */
  int64_t n_omega;    /* owned active bulk unknowns                                             */
  int64_t n_gamma;    /* owned active interface unknowns                                        */
  int64_t M_global;   /* prod(n_d+1)                                                            */
  /* stencil-sliced SpMV image of the matrix (DESIGN.md "SpMV"):                                */
  int64_t spmv_bytes;     /* bytes one y = A x launch has to move with this format               */
  int64_t spmv_slices;    /* U + P slices + G chunks                                             */
  int64_t rows_uniform;   /* rows in U slices (shared offsets and values, nothing streamed)      */
  int64_t rows_pattern;   /* rows in P slices (shared offsets, 8 B/entry value stream) + rows_edge */
  int64_t rows_irregular; /* rows in G chunks (packed CSR, 12 B/entry)                           */
  int64_t neumann_ok;     /* 1: the spectrum of the preconditioned matrix is provably inside |z - 1| < 0.95: BiCGStab
                             runs right-preconditioned with a Chebyshev polynomial in Â (pg_krylov_opts.precond)   */
  double gershgorin;      /* the largest Gershgorin radius that decision rests on (all ranks)     */
  int64_t spmv_units;     /* marching units (DESIGN.md "SpMV"): <= 11 planes x 126 uniform stencil rows each      */
  int64_t rows_marched;   /* rows covered by them (counted in rows_uniform too; they are in no slice)             */
  int64_t rows_matrix;    /* rows of the matrix the other SpMV figures describe: n_own, or fewer for which = 6 / 7 (the
                             warm loop's matrix without the rows that are alone on their diagonal)                   */
  int64_t n_ghost_loop;   /* ghost unknowns of the vectors that matrix works on (which = 6 / 7: the compact loop system
                             keeps the remaining ghosts only; otherwise = n_ghost)                                      */
  int64_t loop_is_compact;/* 1: the warm loop of this system iterates on the compact system (rows alone on their diagonal
                             solved in the right-hand-side pass, pg_reduce.hip) -- on several ranks with halos too     */
  int64_t rows_edge;      /* edge rows of the marching units: rows at the ends of the marched ranges that share their offsets
                             but not their values, computed by the units from an 8 B/entry value stream (counted in
                             rows_pattern too; they are in no slice)                                                    */
} pg_system_info;

typedef struct {
  int64_t steps;            /* steps executed by this call                                                  */
  int64_t psi_iters;        /* Krylov iterations of the stream-function (Poisson) solves                    */
  int64_t omega_iters;      /* ... of the vorticity solves                                                  */
  int64_t psi_products;     /* products with the system matrix inside the Poisson solves                    */
  int64_t omega_products;   /* ... inside the vorticity solves                                              */
  int64_t unconverged;      /* solves (of either system) that ended without meeting the tolerance           */
  double worst_relres;      /* max over the call's solves of ||r|| / ||b|| at exit                          */
  double t_final;
  double total_ms;          /* wall time of the call, and its split (the device is waited for at each boundary): */
  double psi_ms;            /* right-hand side from ω and the Poisson solve                                 */
  double velocity_ms;       /* u, v from ψ and the convection operators                                     */
  double build_ms;          /* construction of the step's vorticity solver (numbering, assembly, b)         */
  double omega_ms;          /* the vorticity solve, the hand-over of its state, the saved state             */
} pg_streamvort_run_info;

/* ---- library / device -------------------------------------------------------------------- */
int32_t pg_last_error(char* buf, size_t n);
/* single-GPU: pg_init(device).  multi-GPU: rank 0 calls pg_get_unique_id, the launcher broadcasts
   the 128 bytes (torch.distributed in bench.py), every rank calls pg_init_distributed. */
int32_t pg_init(int32_t device_id);
int32_t pg_get_unique_id(void* out128);
int32_t pg_init_distributed(int32_t device_id, int32_t rank, int32_t nranks, const void* unique_id128);
int32_t pg_finalize(void);
int32_t pg_device_synchronize(void);
int32_t pg_set_profiling(int32_t on);
int32_t pg_device_name(char* buf, size_t n);
/* the tuning / variant selectors this process runs with (read once from the PG_* environment, pg_common.h Config), as
   "name=value ..." -- so that a measurement can say exactly which variant of the path it timed */
int32_t pg_config_string(char* buf, size_t n);

/* ---- Mesh                                       replaces Mesh(n, L, x0), src/mesh.jl:47-78 ---- */
int32_t pg_mesh_create(int32_t N, const int64_t* n, const double* L, const double* x0, pg_mesh** out);
int32_t pg_mesh_destroy(pg_mesh* m);
int32_t pg_mesh_get_centers(const pg_mesh* m, int32_t d, double* out, int64_t len);   /* len = n_d     */
int32_t pg_mesh_get_nodes(const pg_mesh* m, int32_t d, double* out, int64_t len);     /* len = n_d + 1 */
int32_t pg_mesh_num_border_cells(const pg_mesh* m, int64_t* out);
/* idx: nb*N 1-based Cartesian indices, pos: nb*N centre coordinates, key: nb PG_KEY_*, in the
   reference's order (src/mesh.jl:57-74 + unique!) */
int32_t pg_mesh_get_border_cells(const pg_mesh* m, int64_t* idx, double* pos, int32_t* key);

/* ---- Capacity                      replaces Capacity(body, mesh; method="VOFI"), capacity.jl:51-123 */
/* BALL: params = {c_1..c_N, r}.  MULTIBALL: params = {r, nballs, c^1_1..c^1_N, c^2_1, ...}.
   HALFSPACE: params = {axis (0-based), position, sign}: f(x) = sign (x_axis - position), fluid where f < 0 -- the
   reference's 1-D diphasic bodies `(x,_=0) -> x - xint` (test/convergence_test.jl:111,230) and their N-D extrusions.
   ELLIPSOID: params = {c_1..c_N, a_1..a_N}: f(x) = sqrt(sum ((x_d - c_d)/a_d)^2) - 1, axis-aligned semi-axes a_d > 0
   (volumes, faces, sections exact through the unit ball of the scaled coordinates; the interface measure by
   Gauss-Legendre along the arcs with the weight of the affine map).
   PLANE: params = {n_1..n_N, offset}: f(x) = n.x - offset, fluid where f < 0 (PG_FLAG_COMPLEMENT: -f) -- an oblique half
   space, the level sets `(x, y) -> a x + b y - c` a `Capacity(body, mesh)` of src/capacity.jl:51-123 accepts like any
   other.  n is used as given (never normalised; non-zero and finite); every capacity of a cut cell is closed form. */
int32_t pg_capacity_create_levelset(pg_mesh* m, int32_t body_kind, const double* params, int32_t nparams,
                                    int32_t flags, pg_capacity** out);
/* fallback for arbitrary Julia bodies: arrays computed by the caller (single rank only).
   A,B,W,C_omega,C_gamma: N pointers each to M doubles; C_gamma may be NULL. */
int32_t pg_capacity_create_from_arrays(pg_mesh* m, const double* V, const double* const* A,
                                       const double* const* B, const double* const* W, const double* Gamma,
                                       const double* const* C_omega, const double* const* C_gamma,
                                       const double* cell_types, pg_capacity** out);
/* Capacity(body, SpaceTimeMesh(mesh, [t0, t1])), prescribedmotionsolver/diffusion.jl:251-252 (mesh.jl:129-146): the first
   time layer of the (N+1)-D capacity of a MOVING ball / half space, N = 1 or 2.  The host evaluates the motion at the
   time-quadrature nodes it chooses (composite Gauss-Legendre inside (t0, t1), weights adding up to t1 - t0) and at the
   two time faces; space is integrated exactly as by pg_capacity_create_levelset, time by the given rule.
   nodes: nq x 10 doubles {tau, weight, c_1, c_2, c_3, r, dc_1/dt, dc_2/dt, dc_3/dt, dr/dt}; half space: c_1 = position,
   dc_1/dt = its speed, r ignored.  body0 / body1 = {c_1, c_2, c_3, r} at t0 / t1.
   pg_capacity_get: V, A_d, B_d, W_d, Γ are the first-layer space-time measures, C_ω / C_γ the spatial centroid components;
   PG_CAP_ST_* give A_(N+1) at the two time faces and the time components of the centroids. */
typedef struct {
  int32_t body_kind;   /* PG_BODY_BALL | PG_BODY_HALFSPACE */
  int32_t flags;       /* PG_FLAG_COMPLEMENT | PG_FLAG_NO_CENTROIDS */
  int32_t axis;        /* half space: 0-based axis */
  int32_t nq;
  double sign;         /* half space: f = sign (x_axis - position(t)) */
  double t0, t1;
  const double* nodes; /* nq x 10 */
  double body0[4], body1[4];
} pg_motion_desc;
int32_t pg_capacity_create_spacetime(pg_mesh* m, const pg_motion_desc* motion, pg_capacity** out);
/* marks a capacity built by pg_capacity_create_from_arrays as the first layer of a space-time capacity (arbitrary moving
   bodies integrated by the caller): V_t0 / V_t1 = A_(N+1) at the time faces (M doubles each), Ct_* may be NULL */
int32_t pg_capacity_set_spacetime(pg_capacity* c, double t0, double t1, const double* V_t0, const double* V_t1,
                                  const double* Ct_omega, const double* Ct_gamma);
int32_t pg_capacity_destroy(pg_capacity* c);
/* out: M doubles (global padded layout; with nranks>1 only the planes this rank stores are filled,
   the rest are left untouched) */
int32_t pg_capacity_get(const pg_capacity* c, int32_t field, int32_t d, double* out, int64_t len);
int32_t pg_capacity_kernel_ms(const pg_capacity* c, double* ms); /* device time of K1-K5 for the bench */
/* the same per kernel, each between its own pair of events: ms[0..4] = classification, cut cells, sections, staggered volumes,
   cut staggered boxes; 0 where an empty work list launched nothing.  Zeros for capacities not built by pg_capacity_create_levelset
   or pg_capacity_create_program. */
int32_t pg_capacity_kernel_ms_parts(const pg_capacity* c, double* ms /* 5 */);

/* ---- DiffusionOps                         replaces DiffusionOps(capacity), operators.jl:127-178 */
int32_t pg_diffops_create(pg_capacity* c, pg_diffops** out);
int32_t pg_diffops_destroy(pg_diffops* o);
/* two-call pattern: nzval == NULL -> only *nnz is written.  CSC of G, H (N*M x M) or Winv (N*M x N*M),
   0-based colptr (ncols+1) / rowval, single rank only. */
int32_t pg_diffops_export_csc(const pg_diffops* o, int32_t which, int64_t* colptr, int64_t* rowval,
                              double* nzval, int64_t* nnz);
/* ConvectionOps(capacity, uₒ, uᵧ), operators.jl:194-210: C_d = δ_p[d]·diag(Σ_m[d] A_d uₒ_d)·Σ_m[d], K_d = diag(Σ_p[d] Hᵀuᵧ).
   u_omega: N pointers to M doubles, u_gamma: N*M doubles (block d = component d).  A solver created from an operator
   with a velocity assembles the advection-diffusion blocks (advectiondiffusion.jl:29-44,180-213: conv_bulk = ΣC_d and
   conv_iface = ½ΣK_d on the bulk rows); pg_diffops_export_csc(PG_OP_C0 + d / PG_OP_K0 + d) returns C_d / K_d. */
int32_t pg_diffops_set_velocity(pg_diffops* o, const double* const* u_omega, const double* u_gamma);
/* ConvectionOps(capacity, uₒ, uᵧ) of a SPACE-TIME capacity (2-D+t), as A_/b_*_unstead_advdiff_moving read it
   (prescribedmotionsolver/advectiondiffusion.jl:94-95,158-159: the blocks C[1][L1,L1], C[2][L2,L2], C[3][L1,L2] and the same
   of K, of which only K[1] is used; L1 = first time layer, L2 = time padding).  u_omega: N+1 pointers to 2M doubles (x, y, t),
   u_gamma: (N+1)*2M doubles (block d = component d).  Stored: C_x from the first layer (C[1]) and ½K_x (K[1] = diag(Σ_p[x] h),
   h = Hᵀuᵧ on the first layer); C[2] is C_y on the time padding, where A_y = 0: zero whatever uₒy is (no bulk y-advection, as
   in the reference).  Refused: a non-zero time component of uₒ or time block of uᵧ (C[3] / H_t, which needs B_t), N = 1 (the
   reference's C[3] of a 2-tuple: BoundsError), N = 3, a static capacity.  pg_diffops_export_csc returns C_x / K_x of the
   first layer (PG_OP_C0 / PG_OP_K0) and refuses the other directions.  The moving DIFFUSION constructors refuse such
   operators; the moving advection-diffusion constructors below need them. */
int32_t pg_diffops_set_velocity_spacetime(pg_diffops* o, const double* const* u_omega, const double* u_gamma);
int32_t pg_diffops_grad(const pg_diffops* o, const double* p /*2M*/, double* out /*N*M*/);      /* ∇  :20-23 */
int32_t pg_diffops_div(const pg_diffops* o, const double* qw /*N*M*/, const double* qg /*N*M*/,
                       double* out /*M*/);                                                     /* ∇₋ :30-34 */

/* ---- Solver          replaces DiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme), diffusion.jl:192-210
   Dcoef: M values D(C_omega) or NULL (=1).  source: M values f(C_omega, Δt) for the first step or NULL (=0).
   T0: 2M, or NULL for zeros.  Builds A (scheme), b(t=0) and applies the border rows with t = 0 exactly as the ctor does. */
int32_t pg_solver_create_unsteady_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                       const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                       const double* source, double dt, const double* T0, int32_t scheme,
                                       pg_solver** out);
/* DiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, scheme), diffusion.jl:319-332.  T0: 4M. */
int32_t pg_solver_create_unsteady_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                       const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                       const double* D1, const double* D2, const double* f1, const double* f2,
                                       double dt, const double* T0, int32_t scheme, pg_solver** out);
/* DiffusionSteadyMono(phase, bc_b, bc_i), diffusion.jl:14-28 (A_mono_stead_diff :30-43, b_mono_stead_diff :45-58):
   the same blocks without V and Δt; source = f(C_ω) (no time).  solve_DiffusionSteadyMono! (:60-71) =
   pg_solver_initial_solve; pg_solver_step / _run refuse a steady solver. */
/* MovingDiffusionUnsteadyDiph + A_/b_diph_unstead_diff_moving (prescribedmotionsolver/diffusion.jl:272-498): ONE space-time
   slab of the two-phase moving problem.  c1 / c2: space-time capacities of the body and of its complement on the same slab
   (pg_capacity_create_spacetime); T_prev: the previous state [Tω¹; Tγ¹; Tω²; Tγ²] (4M, host) or NULL with `previous` = the
   previous slab's solver (state handed over on the device); f*_n / f*_np1: sources at t and t + Δt evaluated at the
   space-time centroids (NULL = 0).  Solve with pg_solver_initial_solve; the next slab is a new solver. */
int32_t pg_solver_create_moving_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2, const pg_jump_desc* ic,
                                     const pg_border_desc* borders, int32_t nborders, const double* D1, const double* D2,
                                     const double* f1_n, const double* f1_np1, const double* f2_n, const double* f2_np1,
                                     const double* T_prev, pg_solver* previous, int32_t scheme, pg_solver** out);
int32_t pg_solver_create_steady_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                     const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                     const double* source, pg_solver** out);
/* DiffusionSteadyDiph(phase1, phase2, bc_b, ic), diffusion.jl:88-101 (A_diph_stead_diff :103-144,
   b_diph_stead_diff :146-162); solve_DiffusionSteadyDiph! (:164-175) = pg_solver_initial_solve. */
int32_t pg_solver_create_steady_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                     const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                     const double* D1, const double* D2, const double* f1, const double* f2,
                                     pg_solver** out);
/* One space-time step of solve_MovingDiffusionUnsteadyMono! (prescribedmotionsolver/diffusion.jl:16-35, 100-160, 163-225,
   249-258): A = [Vn_1 + Id GᵀWꜝG Ψ, -(Vn_1 - Vn) + Id GᵀWꜝH Ψ; Iᵦ HᵀWꜝG, Iᵦ HᵀWꜝH + Iₐ Γ] on the space-time capacity c
   (Δt is inside it), b from T_prev (2M, or NULL for zeros), border rows as BC_border_mono!.  source_n / source_np1 =
   f(C_ω.., t) and f(C_ω.., t+Δt) (M doubles or NULL = 0; the first is read by "CN" only).  pg_solver_initial_solve solves
   it; pg_solver_get_state(-1) is the new state, the T_prev of the next slab's solver.  pg_solver_step refuses.
   `previous` (or NULL): the previous slab's solver (solved, same mesh), whose state is taken as T_prev -- device to device:
   the time loop then moves no state over PCIe unless the caller asks for one (pg_solver_get_state).  With both given, the
   active unknowns of `previous` overwrite T_prev's; the same holds for every moving constructor. */
int32_t pg_solver_create_moving_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                     const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                     const double* source_n, const double* source_np1, const double* T_prev,
                                     pg_solver* previous, int32_t scheme, pg_solver** out);
/* One space-time step of solve_MovingAdvDiffusionUnsteadyMono! (prescribedmotionsolver/advectiondiffusion.jl:15-33
   constructor, 64-129 A, 131-199 b, 201-242 loop): the arguments of pg_solver_create_moving_mono, o = the space-time
   ConvectionOps of c (pg_diffops_set_velocity_spacetime).  A = the moving blocks with - (ΣC + ½K[1]) Ψc and - ½K[1] Ψc in the
   bulk rows, Ψc = psip_conv.(Vn, Vn_1) (:35-47; 1 only where Vn = 0, Vn_1 ≠ 0); b subtracts the explicit convection of the
   previous state: BE (:194) ½K[1] Ψm Tω + ½K[1] Tγ + ΣC Ψm Tω with Ψm = psim_conv.(Vn, Vn_1) (:49-61), CN (:192)
   ½K[1] Ψn Tω + ½K[1] Tγ + ΣC Tω with Ψn = psim_cn -- on the device, from T_prev or from the previous solver. */
int32_t pg_solver_create_moving_advdiff_mono(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface,
                                             const pg_border_desc* borders, int32_t nborders, const double* Dcoef,
                                             const double* source_n, const double* source_np1, const double* T_prev,
                                             pg_solver* previous, int32_t scheme, pg_solver** out);
/* MovingAdvDiffusionUnsteadyDiph + A_/b_diph_unstead_advdiff_moving (prescribedmotionsolver/advectiondiffusion.jl:246-507): one
   slab, the arguments of pg_solver_create_moving_diph with space-time ConvectionOps o1 / o2.  Differs from the moving
   diffusion blocks beyond the convection terms (as mono per phase; CN: - ΣC Tω - ½K[1] Tω - ½K[1] Tγ, no Ψ): the flux row
   has no -(Vn_1 - Vn) term (:362-365) and the CN γ term of b is -½ Id GᵀWꜝH Tγ without Ψ (:494-495). */
int32_t pg_solver_create_moving_advdiff_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                             const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                             const double* D1, const double* D2, const double* f1_n, const double* f1_np1,
                                             const double* f2_n, const double* f2_np1, const double* T_prev,
                                             pg_solver* previous, int32_t scheme, pg_solver** out);
/* MovingLiquidDiffusionUnsteadyDiph + A_/b_diph_unstead_diff_moving_stef (liquidmotionsolver/diffusion.jl:445-673): one slab
   of the two-phase Stefan problem, the arguments of pg_solver_create_moving_diph (`previous`: device hand-over).  Differs
   from the moving diphasic blocks in row block 4 = [0 0 0 Iα₂] (:542; the flux blocks 5-8 are built there but not used),
   b₂ = b₄ = gᵧ (:646-647) and, under CN, b₁ / b₃ = (Vn - Id GᵀWꜝG Ψn) Tω - ½ Id GᵀWꜝH Tγ + ½ V (fₙ + fₙ₊₁) with no Ψ on
   the γ term (:637-642).  BE: Vn Tω + V fₙ₊₁. */
int32_t pg_solver_create_moving_stefan_diph(pg_capacity* c1, pg_diffops* o1, pg_capacity* c2, pg_diffops* o2,
                                            const pg_jump_desc* ic, const pg_border_desc* borders, int32_t nborders,
                                            const double* D1, const double* D2, const double* f1_n, const double* f1_np1,
                                            const double* f2_n, const double* f2_np1, const double* T_prev,
                                            pg_solver* previous, int32_t scheme, pg_solver** out);
/* The Stefan terms of a 1-D slab of a moving diffusion solver (mono, diph or Stefan diph), computed on the device from its
   space-time capacities, operators, D and current state: its solution, or before the first solve the state it was built
   from (liquidmotionsolver/diffusion.jl:240-255, 318-330; height_tracking.jl:23-31).  out: 4 doubles per phase, {Σ A_t(t0), Σ A_t(t1), Σᵢ qᵢ, maxᵢ |qᵢ|} with
   q = Id Hᵀ Wꜝ (G Tω + H Tγ) on the first time layer.  Σ A_t(t0) is the capacity's Vn_1 summed: the reference's "Hₙ₊₁";
   Σ A_t(t1) (Vn) is its "Hₙ".  Fixed-order reduction: the same state gives bitwise the same out.  Refuses a solver that is
   not a space-time diffusion slab, several ranks and N ≠ 1. */
int32_t pg_solver_stefan_terms(const pg_solver* s, double* out);
int32_t pg_solver_destroy(pg_solver* s);

/* ---- StreamVorticity                replaces src/solver/streamfunction_vorticity.jl (2-D incompressible flow: ∇²ψ = -ω,
   u = ∂ψ/∂y, v = -∂ψ/∂x, ω advected and diffused with (u, v)).  One rank, N = 2.  Both states, the velocity and the convection
   operators stay on the device from step to step; the host sees them when it asks (pg_streamvort_get). */
/* StreamVorticity(capacity, ν, Δt; bc_stream, bc_vorticity, bc_stream_border, bc_vorticity_border, ψ0, ω0), :73-98 with
   assemble_laplacian :105-117 (the steady diffusion blocks, D = 1): o = DiffusionOps(c) WITHOUT a velocity; nu: M values
   ν(C_ω); psi0 / omega0: 2M doubles or NULL (zeros).  states[0] = (0, ψ0, ω0).  Refuses N ≠ 2 and several ranks. */
int32_t pg_streamvort_create(pg_capacity* c, pg_diffops* o, const double* nu, double dt, const pg_bc_desc* bc_stream,
                             const pg_bc_desc* bc_vorticity, const pg_border_desc* borders_stream, int32_t nborders_stream,
                             const pg_border_desc* borders_vorticity, int32_t nborders_vorticity, const double* psi0,
                             const double* omega0, pg_streamvort** out);
int32_t pg_streamvort_destroy(pg_streamvort* sv);
/* `solver.ω = ...` after construction (test/solver/stream_vorticity_test.jl:30): 2M doubles; the next step starts from it */
int32_t pg_streamvort_set_omega(pg_streamvort* sv, const double* omega);
/* data of time-dependent closures, evaluated by the host at the reference's points: the vorticity source at t and t + Δt
   (:228-229; NULL keeps what is there), interface values of ψ (which = PG_SV_PSI: g(C_γ, t), :134, only g_np1 is read) or of
   ω (PG_SV_OMEGA: g at t and t + Δt), border values of either system (mesh border order; BC_border_mono! is called without
   t, :198, :231) */
int32_t pg_streamvort_set_source(pg_streamvort* sv, const double* f_n /*M*/, const double* f_np1 /*M*/);
int32_t pg_streamvort_set_interface_values(pg_streamvort* sv, int32_t which, const double* g_n /*M*/, const double* g_np1 /*M*/);
int32_t pg_streamvort_set_border_values(pg_streamvort* sv, int32_t which, const double* values /*nb*/);
/* solve_StreamVorticity! (:273-275) = _solve_streamfunction! (:191-206): b = [-V ωω; Γ g], border rows, ψ = Aψ⁻¹ b (from
   the second solve on started from the previous ψ), then update_velocity! (:146-159): u = (∇ψ)_y, v = -(∇ψ)_x */
int32_t pg_streamvort_solve_stream(pg_streamvort* sv, const pg_krylov_opts* opts, pg_step_info* info);
/* step_StreamVorticity! (:282-284) = _step! (:216-242): the above, ConvectionOps(capacity, (u, v), [u; v]) (:167-182), the
   unsteady advection-diffusion system of ω with D = ν (the D that the call at :228 leaves out: read by "CN" only), its
   solve, time += Δt, push!(states, (time, ψ, ω)) */
int32_t pg_streamvort_step(pg_streamvort* sv, int32_t scheme, const pg_krylov_opts* opts, pg_step_info* info_psi,
                           pg_step_info* info_omega);
/* run_StreamVorticity! (:291-293) with constant-in-time data: `steps` steps; every save_every-th state of the call is kept
   (save_every <= 0: none) */
int32_t pg_streamvort_run(pg_streamvort* sv, int64_t steps, int32_t scheme, const pg_krylov_opts* opts, int32_t save_every,
                          pg_streamvort_run_info* info);
/* field = PG_SV_PSI / PG_SV_OMEGA: len = 2M, state_index < 0: the current s.ψ / s.ω, else states[state_index];
   PG_SV_U / PG_SV_V: len = M, the current s.velocity (state_index < 0 only) */
int32_t pg_streamvort_get(const pg_streamvort* sv, int32_t field, int64_t state_index, double* out, int64_t len);
int32_t pg_streamvort_num_states(const pg_streamvort* sv, int64_t* out);
/* s.time (state_index < 0) or states[state_index].time */
int32_t pg_streamvort_time(const pg_streamvort* sv, int64_t state_index, double* out);
/* the solver of the last Poisson solve (PG_SV_PSI) or of the last vorticity step (PG_SV_OMEGA; NULL before the first step),
   BORROWED: for pg_solver_get_system_csr / pg_solver_system_info / pg_solver_get_state; never destroy it, and do not keep
   it across a step (the vorticity solver is replaced by every step) */
int32_t pg_streamvort_solver(pg_streamvort* sv, int32_t which, pg_solver** borrowed);

/* per-step data for time-dependent closures; the host evaluates them at the reference's points and
   times (C_omega / C_gamma / mesh.centers; t+Δt -- diffusion.jl:248-249) and passes arrays.
   f_n, g_n (values at t) are only read by the CN scheme; NULL keeps the previous / constant data. */
int32_t pg_solver_set_source(pg_solver* s, int32_t phase, const double* f_n /*M*/, const double* f_np1 /*M*/);
int32_t pg_solver_set_interface_value(pg_solver* s, const double* g_n /*M*/, const double* g_np1 /*M*/);
int32_t pg_solver_set_border_values(pg_solver* s, const double* values /*nb, mesh border order*/);

/* Time-separable data  sum_k phi_k(x) a_k(t),  k = 1..K <= PG_TD_MAX_TERMS: the spatial parts go to the device once, every step
   then costs K scalars and one streaming kernel -- no per-step transfer (DESIGN.md "Time-separable data").
   which: PG_TD_SOURCE (phase 0 / 1), PG_TD_INTERFACE (the monophasic interface value; phase = 0), PG_TD_BORDER (phase = 0).
   modes: K x M padded fields (the source's phi_k at C_omega, the interface value's at C_gamma), or K x nb border values in the
          mesh's border order (as pg_solver_set_border_values takes them: EVERY border value of the solver, the constant ones
          as a term whose coefficients are 1).
   coef : nrows x 2 x K, row q = the coefficients of step q: a_k at the step's "t" and at its "t + dt" -- the two times at which
          the caller of pg_solver_set_source / _interface_value / _border_values evaluates its closures for that step (border
          values are taken at "t" alone).  The library attaches no clock to the rows.
   Every time step (pg_solver_step, or one step of pg_solver_run) consumes one row, the same row for every slot; a step past the
   last row of an installed table fails and reuses nothing.  Installing a table rewinds the cursor to row 0.  Install after
   pg_solver_initial_solve (the constructor's system has its data from the host).  pg_solver_set_source / _interface_value /
   _border_values on a slot that holds separable data clear that slot.  Steps with separable data are steps with changed data:
   no folded start, no extrapolated start.
   Refused: K > PG_TD_MAX_TERMS; steady, moving and Stefan solvers; PG_TD_INTERFACE on a diphasic solver (its jump rows carry no
   time); more than one rank (virtual ranks included). */
enum { PG_TD_SOURCE = 0, PG_TD_INTERFACE = 1, PG_TD_BORDER = 2 };
enum { PG_TD_MAX_TERMS = 8 };
int32_t pg_solver_set_separable(pg_solver* s, int32_t which, int32_t phase, int32_t K, const double* modes, int64_t nrows,
                                const double* coef);
int32_t pg_solver_clear_separable(pg_solver* s, int32_t which, int32_t phase);
/* terms: 4 counts -- source of phase 0, source of phase 1, interface value, border values (0: the slot is empty);
   nrows: rows of the shortest installed table (0: none installed); cursor: the row the next step consumes */
int32_t pg_solver_time_data_info(const pg_solver* s, int32_t* terms /*4*/, int64_t* nrows, int64_t* cursor);
/* measurement: the per-step combine of the last consumed row, `repeats` launches between two events; modes = J installed terms,
   bytes = (J + 2) * 8 * n_own, what one combine streams */
int32_t pg_debug_td_combine_ms(pg_solver* s, int32_t scheme, int32_t repeats, double* ms_per_combine, int32_t* modes,
                               int64_t* bytes);

/* Device functions: a scalar expression in (x0, x1, x2, t) shipped once as a small postfix program and evaluated on the device
   every step at the points where the reference evaluates the closure (DESIGN.md "Device functions").  pg_program is a POD of
   fixed size, handed BY VALUE to the kernel that runs it: no upload, no read-back.
   Instruction q is (op[q], arg[q]); arg is read by PG_OP_CONST (index into konst, < n_const) and PG_OP_VAR (0, 1, 2: the
   coordinates of the point, missing ones 0.0; 3: t) only.  Unary operations replace the top of the operand stack, binary ones
   (a below b) pop two and push one, the comparisons give 1.0 / 0.0, PG_OP_SELECT pops (c, a, b) and pushes a if c != 0 else b.
   A valid program never underflows the stack, never holds more than PG_PROG_MAX_STACK values and ends with exactly one. */
enum { PG_PROG_MAX_OPS = 96, PG_PROG_MAX_CONST = 32, PG_PROG_MAX_STACK = 16 };
enum {
  PG_OP_CONST = 0, PG_OP_VAR = 1, PG_OP_ADD = 2, PG_OP_SUB = 3, PG_OP_MUL = 4, PG_OP_DIV = 5, PG_OP_NEG = 6, PG_OP_ABS = 7,
  PG_OP_SQRT = 8, PG_OP_EXP = 9, PG_OP_LOG = 10, PG_OP_SIN = 11, PG_OP_COS = 12, PG_OP_TANH = 13, PG_OP_POW = 14,
  PG_OP_ATAN2 = 15, PG_OP_ERF = 16, PG_OP_ERFC = 17, PG_OP_MIN = 18, PG_OP_MAX = 19, PG_OP_LT = 20, PG_OP_LE = 21,
  PG_OP_GT = 22, PG_OP_GE = 23, PG_OP_SELECT = 24, PG_OP_COUNT = 25
};
typedef struct pg_program {
  int32_t n_ops;                       /* 1 .. PG_PROG_MAX_OPS */
  int32_t n_const;                     /* 0 .. PG_PROG_MAX_CONST */
  uint8_t op[PG_PROG_MAX_OPS];
  uint8_t arg[PG_PROG_MAX_OPS];
  double konst[PG_PROG_MAX_CONST];
} pg_program;
/* 0 when the program is valid; otherwise 1 and the reason in pg_last_error.  Host only, needs no device. */
int32_t pg_program_validate(const pg_program* prog);
/* the host interpreter: out[i] = P(xyz[3i], xyz[3i+1], xyz[3i+2], t).  Validates first; needs no device. */
int32_t pg_program_eval_host(const pg_program* prog, int64_t npts, const double* xyz /* npts x 3 */, double t, double* out);
/* A program in a slot of time-dependent data, with the which / phase values of pg_solver_set_separable.  A slot holds separable
   terms OR programs: installing one clears the other, and pg_solver_clear_separable, pg_solver_set_source / _interface_value /
   _border_values clear a program slot as they clear a separable one.  times: 2 x nrows, row q = the "t" and "t + dt" of step q
   (the two times at which the host-driven loop evaluates its closures for that step).  Table discipline as above: one row per
   step, installing rewinds the cursor, a step past the last row fails.  At install one kernel lists the rows that carry the
   slot's data with their weights and points (source: bulk rows of the phase that are not fixed, V, C_omega; interface: interface
   rows, Gamma, C_gamma; border: the fixed rows of the border cells, 1, the cell centres); every step one kernel adds
   weight * (c0 P(p, t) + c1 P(p, t + dt)) to the right-hand side of those rows, c0 and c1 being the scheme's factors of
   separable data.  PG_TD_BORDER gives every border cell the program's value; pg_solver_set_border_program gives it to the
   cells of one border key (PG_KEY_*) and leaves the others what pg_solver_set_border_values set -- at most one program per key.
   Refused: what pg_solver_set_separable refuses, an invalid program, a capacity without C_gamma (PG_TD_INTERFACE). */
int32_t pg_solver_set_program(pg_solver* s, int32_t which, int32_t phase, const pg_program* prog, int64_t nrows,
                              const double* times /* 2 x nrows */);
int32_t pg_solver_set_border_program(pg_solver* s, int32_t key, const pg_program* prog, int64_t nrows,
                                     const double* times /* 2 x nrows */);
/* programs: 4 counts of installed programs per slot (as `terms` of pg_solver_time_data_info; the border slot: one per key or 1);
   entries: 4 counts of listed rows; nrows / cursor as pg_solver_time_data_info, over separable and program slots together */
int32_t pg_solver_program_info(const pg_solver* s, int32_t* programs /*4*/, int64_t* entries /*4*/, int64_t* nrows,
                               int64_t* cursor);
/* test support: the kernel-side evaluator (same instantiation and stack layout as the per-step kernel) on caller-supplied
   points: out[i] = P(xyz[3i .. 3i+2], t) */
int32_t pg_debug_program_eval(const pg_program* prog, int64_t npts, const double* xyz /* npts x 3 */, double t, double* out);
/* Capacity(body, mesh) of an ARBITRARY level set (PG_BODY_PROGRAM): phi(x_1 .. x_N) as a program and the N programs of its
   partial derivatives d phi / d x_d (grad[0 .. N-1]); fluid where phi <= 0, PG_FLAG_COMPLEMENT: -phi and -grad phi,
   PG_FLAG_NO_CENTROIDS as for the closed-form kinds.  1-D and 2-D.  The kernels of pg_capacity_create_levelset run with the
   body evaluated to rounding where the geometry needs it: a cell is classified on a lattice of 9 samples per edge and its centre
   (a feature of the body narrower than h / 8 is not seen), the roots of phi along cell edges and quadrature lines are found
   to an ulp of their coordinate, cut cells are integrated with 16 Gauss-Legendre nodes per smooth piece.
   Refused before anything is allocated, each with its own message: an invalid program; a program that reads t (PG_OP_VAR 3) or
   a coordinate >= N; a 3-D mesh; grad == NULL; more than one rank or a communicator; a gradient that disagrees with central
   differences of phi (step 1e-6 h) by more than 1e-4 max(|grad phi|, 1) at the centres of up to 64 cells spread over the mesh
   (evaluated on the host with pg_program_eval_host's interpreter: it catches a wrong derivative, not rounding).
   The programs of the capacity under construction sit in one __constant__ table per process: concurrent calls from several
   host threads are serialised by a mutex inside, each holding it until its last kernel has run. */
int32_t pg_capacity_create_program(pg_mesh* m, const pg_program* phi, const pg_program* grad /* N programs */, int32_t flags,
                                   pg_capacity** out);
/* Capacity(body::Function, mesh) of the reference (src/capacity.jl:51-123) for an ARBITRARY level set in 3-D: phi(x, y, z) as a
   program and the 3 programs of d phi / dx, d phi / dy, d phi / dz; fluid where phi <= 0, flags as pg_capacity_create_program.
   The same five kernels with the 3-D rule of csrc/pg_geom_program3.h: a cell is classified on 9 samples
   of each of its 12 edges, its 6 face centres and its centre; a cut box is integrated by one wave, heights along the axis with
   the largest |d phi / d x_d| at the box centre, the 2-D rule of pg_capacity_create_program in the plane of every outer
   Gauss-Legendre node, outer breakpoints at the roots of phi on the 4 box edges along the outer axis; a face is the 2-D rule on
   the slice x_d = const, 16 lanes per face.  Cells in which the trace of the interface on a face turns back along the outer
   axis, or the derivative along the height axis vanishes (around the "poles" of a closed body), are integrated across a
   square-root singularity: about 1e-3 of a cell there, rounding elsewhere.  Results are bitwise repeatable.  Refused before
   anything is allocated, each with its own message: a missing or invalid program; a program that reads t; a mesh that is not
   3-D; grad == NULL; more than one rank or a communicator; a gradient that disagrees with central differences of phi
   (pg_capacity_create_program's rule and tolerance).  *out is NULL after a refusal.  The __constant__ table and its mutex are
   pg_capacity_create_program's, which keeps refusing a 3-D mesh. */
int32_t pg_capacity_create_program3(pg_mesh* m, const pg_program* phi, const pg_program* grad /* 3 programs */, int32_t flags,
                                    pg_capacity** out);
/* Capacity(front::FrontTracker, mesh) (PG_BODY_POLYGON): a simple closed polygon of M >= 3 markers in 2-D, xy = x0 y0 x1 y1 ...;
   fluid is the interior (the reference's get_fluid_polygon), PG_FLAG_COMPLEMENT: the exterior, PG_FLAG_NO_CENTROIDS as for the
   other kinds.  A closing duplicate of the first marker is dropped and the orientation is normalised to counter-clockwise.  The
   kernels of pg_capacity_create_levelset run with the polygon itself as the body (csrc/pg_geom_polygon.h states the crossing,
   touching and half-open rules): no transcendental, every capacity a finite sum of polynomial terms, a
   corner inside a cell exact.  An edge lookup (the edges of every column, row and cell, ascending) is built on the device
   first; its time is entry 5 of pg_capacity_polygon_ms_parts, outside the five of pg_capacity_kernel_ms_parts.  Results are
   bitwise repeatable.  Refused before anything is allocated, each with its own message: a mesh that is not 2-D; more than one
   rank or a communicator; M < 3; a non-finite coordinate; a zero-length edge; zero signed area; a polygon that intersects
   itself (an O(M^2) test on the host).  *out is NULL after a refusal. */
int32_t pg_capacity_create_polygon(pg_mesh* m, const double* xy /* 2 M */, int64_t M, int32_t flags, pg_capacity** out);
/* the five kernel times of pg_capacity_kernel_ms_parts and, in ms[5], the time of the edge lookup (count, scan, fill, order) */
int32_t pg_capacity_polygon_ms_parts(const pg_capacity* c, double* ms /* 6 */);
/* Capacity(body, SpaceTimeMesh(mesh, [t0, t1])) of an ARBITRARY moving level set phi(x_1 .. x_N, t) (t: PG_OP_VAR 3): phi, the N
   programs of d phi / d x_d and the program of d phi / dt; fluid where phi <= 0, flags as pg_capacity_create_program.  The
   space-time kernels of pg_capacity_create_spacetime run with "the body at time node k" = phi(., tau_k) measured by the
   primitives of pg_capacity_create_program, with the conventions of the closed-form moving kinds: every first-layer capacity is
   the composite-rule time integral sum_k w_k (spatial measure at tau_k), V_t0 / V_t1 are the spatial volumes at the two faces,
   a cell is FULL / EMPTY only if it is so at every node and both faces, Gamma = sum_k w_k Gamma(tau_k) sqrt(1 + v_n^2) with
   v_n = - d_t phi / |grad phi| at (C_gamma(tau_k), tau_k) (0 where |grad phi| is zero or not finite).  The cheap pass finishes a
   cell only if its sample lattice (9 points in 1-D, 33 in 2-D) has one strict sign at t0, mid time and t1 and min |phi| over
   those samples exceeds (t1 - t0) max |d phi / dt| over them: a body that crosses a whole cell AND comes back within half a slab,
   or a feature narrower than h / 8, is not seen.  tau_w: nq rows (tau_k, w_k), t0 < tau_k < t1.
   1-D+t and 2-D+t.  Refused before anything is allocated, each with its own message: N not 1 or 2; a NULL mesh or out; a NULL
   phi, grad, dphidt or tau_w (each named); an invalid
   program; a program reading a coordinate >= N; nq outside 1 .. 4096; t1 <= t0; a node outside (t0, t1); weights that do not add
   up to t1 - t0 within 1e-12 (t1 - t0); more than one rank or a communicator; a spatial or time derivative that disagrees with
   central differences of phi (pg_capacity_create_program's rule and tolerance at t0, mid time and t1; the time step is
   1e-6 (t1 - t0)).  *out is NULL after a refusal.  The __constant__ table and its mutex are pg_capacity_create_program's. */
int32_t pg_capacity_create_spacetime_program(pg_mesh* m, const pg_program* phi, const pg_program* grad /* N programs */,
                                             const pg_program* dphidt, int32_t flags, double t0, double t1, int32_t nq,
                                             const double* tau_w /* nq x 2 */, pg_capacity** out);
/* Capacity(front_n, front_np1, SpaceTimeMesh(mesh, [t0, t1])) of a MOVING marker polygon -- the reference's
   compute_spacetime_capacities(mesh, front_n, front_np1, dt) (src/front_tracking.jl:1472) with interpolate_front (:2289): xy0 and
   xy1 are the M markers at t0 and at t1, the same count and order; inside the slab every marker moves on a straight line at
   constant speed, vertex i at tau is xy0_i + s (xy1_i - xy0_i) with s = (tau - t0) / (t1 - t0), and the two time faces read xy0
   and xy1 themselves.  A closing duplicate is dropped where both arrays close; the orientation is normalised to
   counter-clockwise by the signed area at t0, the same reversal applied to both.  Fluid is the interior, PG_FLAG_COMPLEMENT: the
   exterior.  The space-time kernels of pg_capacity_create_spacetime run with "the body at time node k" = that polygon measured
   by the primitives of pg_capacity_create_polygon, with the conventions of pg_capacity_create_spacetime_program (time integrals
   by the composite rule, V_t0 / V_t1 the spatial volumes at the faces -- a FULL face takes the full cells' measure, so V_t1 of
   one slab and V_t0 of the next are the same bits --, FULL / EMPTY only if so at every node and both faces), except Gamma: it is
   sum_k w_k sum_pieces len_p sqrt(1 + v_n,p^2) over the pieces the cell owns at tau_k, v_n,p the normal speed of the edge at the
   piece's midpoint -- one speed per piece, exact for a rigid translation -- and C_gamma the mean with the same weights; a cell
   that is never CUT may own a piece (an edge along its lower or left face) and then has Gamma > 0.  One edge lookup of the SWEPT
   edges (the bounding box of an edge's two ends at t0 and t1) is built on the device per slab and serves every node and both
   faces; a cell whose swept list is empty is finished by the cheap pass with the parity of its centre at t0.  Bitwise
   repeatable.  Limits: straight marker paths within a slab; 2-D; closed fronts; one rank.  Refused before anything is allocated,
   each with its own message: a NULL mesh, out, xy0, xy1 or tau_w (each named); M < 3; a non-finite coordinate; a mesh that is
   not 2-D; nq outside 1 .. 4096; t1 <= t0; a node outside (t0, t1); weights that do not add up to t1 - t0 within
   1e-12 (t1 - t0); more than one rank or a communicator; a zero-length edge, zero signed area or a self-intersection
   (pg_capacity_create_polygon's rules) at t0, at t1 or at mid time -- NOT at the times in between --; an orientation that
   differs between t0 and t1.  *out is NULL after a refusal.  pg_debug_capacity_spacetime_ms_parts gives the six kernel times
   (with the timing below on) and entry 5 of pg_capacity_polygon_ms_parts the time of the edge lookup. */
int32_t pg_capacity_create_spacetime_polygon(pg_mesh* m, const double* xy0 /* 2 M */, const double* xy1 /* 2 M */, int64_t M,
                                             int32_t flags, double t0, double t1, int32_t nq, const double* tau_w /* nq x 2 */,
                                             pg_capacity** out);
/* measurement, off by default: while on, pg_capacity_create_spacetime_program and pg_capacity_create_spacetime_polygon bracket
   each of their six kernels with events */
int32_t pg_debug_spacetime_kernel_timing(int32_t on);
/* capacities of pg_capacity_create_spacetime_program: the number of cells the cheap pass left to the list and, when built with
   the timing on, ms of k_st_classify, k_st_cells, k_st_sections, k_st_sections_cut, k_st_stagger, k_st_stagger_cut (0: not
   launched, or not timed) */
int32_t pg_debug_capacity_spacetime_ms_parts(const pg_capacity* c, double* ms /*6*/, int64_t* n_listed);
/* measurement: the per-step evaluation of every installed program at the last consumed row, `repeats` times between two
   events; entries = listed rows summed over the programs, instructions = entries x n_ops x evaluations summed likewise */
int32_t pg_debug_td_eval_ms(pg_solver* s, int32_t scheme, int32_t repeats, double* ms_per_eval, int64_t* entries,
                            int64_t* instructions);

/* Monitors: per-step observables evaluated on the device (DESIGN.md "Monitors").  They replace the post-processing loops over
   solver.states of the reference's scripts -- the volume-weighted phase means of examples/2D/Diffusion/Heat_2ph.jl (its
   Sherwood number), the interface flux  sum_i [Id (H' W! G Tw + H' W! H Tg)]_i  the Stefan and species solvers sum per step,
   the extremum benchmark/Heat3D.jl tracks -- each a linear or weighted-quadratic functional of the state:
     PG_MON_SUM    sum_i w_i x_i          PG_MON_SUMSQ   sum_i w_i x_i^2
   weights: K x len, len = 2M (mono) / 4M (diph), the layout of pg_solver_get_state; entries on unknowns that are no row of
   the system are dropped (the state is 0 there).  Each monitor is stored dense (n_own doubles) or as a sorted (row, weight)
   list, whichever streams fewer bytes per step.  After EVERY completed solve -- pg_solver_initial_solve, pg_solver_step, and
   each of them inside pg_solver_run -- one kernel appends one row to a series kept on the device: row 0 is the state after
   the first solve (states[1] of the reference), row q the state after step q, when the monitors are installed before the
   first solve.  No atomics; the same run gives the same bits.  Installing monitors clears any earlier series.
   Refused: K < 1 or K > PG_MON_MAX, an unknown kind, NULL arguments, len != 2M / 4M; steady, moving, Stefan and
   stream-function - vorticity solvers; more than one rank (virtual ranks included). */
enum { PG_MON_SUM = 0, PG_MON_SUMSQ = 1 };
enum { PG_MON_MAX = 8 };
int32_t pg_solver_set_monitors(pg_solver* s, int32_t K, const int32_t* kinds, const double* weights /* K x len */, int64_t len);
/* removes the monitors and the series */
int32_t pg_solver_clear_monitors(pg_solver* s);
/* K: installed monitors (0: none); rows: rows of the series; per monitor (PG_MON_MAX entries each; any pointer may be NULL):
   sparse = 1 for a (row, weight) list, 0 for dense; stored = entries of the list / n_own */
int32_t pg_solver_monitor_info(const pg_solver* s, int32_t* K, int64_t* rows, int32_t* sparse /*[8]*/, int64_t* stored /*[8]*/);
/* rows row0 .. row0 + nrows - 1 of the series: values nrows x K, times (the solver's time of each row) nrows or NULL.
   A range past the last row is an error. */
int32_t pg_solver_get_monitor_series(const pg_solver* s, int64_t row0, int64_t nrows, double* values /* nrows x K */,
                                     double* times /* nrows or NULL */);
/* releases the states pg_solver_run kept (save_every > 0) once the caller has fetched them: pg_solver_num_states is 0
   afterwards.  (The reference keeps every state in solver.states for the life of the solver.) */
int32_t pg_solver_drop_states(pg_solver* s);
/* measurement: the evaluation of the installed monitors on the current state, `repeats` launches between two events;
   bytes = what one evaluation streams (as pg_debug_td_combine_ms) */
int32_t pg_debug_monitor_ms(pg_solver* s, int32_t repeats, double* ms_per_eval, int64_t* bytes);
/* test support: the installed monitors evaluated once on the current state (K values), the series untouched; x_form (may be
   NULL) = 1 when the kernel read the unscaled x (valid after a state download), 0 when it read z and its scaling */
int32_t pg_debug_monitor_eval(pg_solver* s, double* values /* K */, int32_t* x_form);

/* first solve of solve_DiffusionUnsteadyMono! (diffusion.jl:275): uses the ctor's A, b. */
int32_t pg_solver_initial_solve(pg_solver* s, const pg_krylov_opts* opts, pg_step_info* info);
/* one loop iteration (diffusion.jl:286-300): t += Δt; b; border rows; solve. scheme = run scheme. */
int32_t pg_solver_step(pg_solver* s, int32_t scheme, const pg_krylov_opts* opts, pg_step_info* info);
/* whole loop `while t < Tend` with constant-in-time data; max_steps < 0: unbounded.
   do_initial != 0 runs the initial solve first.  save_every > 0 keeps every k-th state on the device. */
int32_t pg_solver_run(pg_solver* s, double Tend, int32_t scheme, const pg_krylov_opts* opts, int32_t do_initial,
                      int64_t max_steps, int32_t save_every, pg_run_info* info);
int32_t pg_solver_num_states(const pg_solver* s, int64_t* out);
/* x: full unknown vector (2M mono / 4M diph) with zeros at eliminated unknowns (solver.jl:186-187).
   state_index < 0: current s.x.  With nranks>1 only owned entries are written (others untouched). */
int32_t pg_solver_get_state(const pg_solver* s, int64_t state_index, double* x, int64_t len);
/* which: 0 = constructor system, 1 = run (loop) system: the reference's reduced A x = b;
          2 / 3 = the same two systems as the Krylov solver iterates on them, left-preconditioned and
          equilibrated: (B^-1 S A S) y = B^-1 S b, x = S y (DESIGN.md "Preconditioner"); nnz differs.
          pg_solver_system_info only: 6 / 7 = what the warm time loop iterates on: the same matrix without the interface
          unknowns of a Dirichlet problem (rows of the identity, solved before the iteration -- DESIGN.md "Dirichlet
          interface rows") once a loop step has built it; identical to 2 / 3 otherwise. */
int32_t pg_solver_system_info(const pg_solver* s, int32_t which, pg_system_info* out);
/* reduced system of this rank as CSR (rowptr n_own+1, col nnz (local numbering: owned then ghosts), val nnz)
   plus b (n_own) and the map idx[n_own] -> index in the full 2M/4M vector (the reference's common_idx).
   which = 6 / 7: the matrix pg_solver_system_info(6 / 7) describes, i.e. what the warm loop multiplies by: rowptr has
   rows_matrix + 1 entries, col is in THAT matrix's local numbering (pg_debug_spmv_sizes gives the vector length), nnz as
   pg_solver_system_info(6 / 7); b and idx belong to the full system and must be NULL. */
int32_t pg_solver_get_system_csr(const pg_solver* s, int32_t which, int64_t* rowptr, int64_t* col, double* val,
                                 double* b, int64_t* idx);
/* S = diag(|a_ii|^-1/2) of system `which` (0 constructor, 1 run): the weights of the convergence test
   ||S r̂|| <= reltol ||S b̂|| (DESIGN.md "Krylov driver") and the map x = S y of the preconditioned system.  ds: n_own. */
int32_t pg_solver_get_row_scaling(const pg_solver* s, int32_t which, double* ds);
/* the multigrid hierarchy of the solver's constructor system (levels = 0 before the first PG_PRECOND_MG solve) */
int32_t pg_solver_mg_info(const pg_solver* s, pg_mg_info* out);
/* ... and the hierarchy of `precond` = PG_PRECOND_MG (the call above) or PG_PRECOND_MG_CELL */
int32_t pg_solver_mg_info_for(const pg_solver* s, int32_t precond, pg_mg_info* out);
/* the hierarchies of PG_PRECOND_MG_STEP: which = 0 the constructor's system, 1 the run system (levels = 0 while the first
   solve with the option on that matrix has not run) */
int32_t pg_solver_mg_step_info(const pg_solver* s, int32_t which, pg_mg_info* out);
/* The spectral estimate behind PG_PRECOND_POLY_EST of system `which` (0 constructor, 1 run system; + 4: report only).  Runs the
   estimate if it has not run on that matrix (a solve with PG_PRECOND_POLY_EST runs it only where Gershgorin refuses; this call
   runs it on any matrix) and refuses what the option refuses.  With + 4 nothing runs: steps = 0 says no estimate exists. */
int32_t pg_solver_spectral_estimate(pg_solver* s, int32_t which, pg_specest_info* out);
/* bench helper: `reps` launches of y = A x on the run matrix, HIP-event timed on the library stream. */
int32_t pg_solver_time_spmv(pg_solver* s, int32_t which, int32_t reps, double* avg_ms);

/* host-logic helper (no GPU needed): slab partition of `nplanes` planes with per-plane weights
   (active rows) into nranks contiguous ranges; bounds has nranks+1 entries. */
int32_t pg_partition_planes(const int64_t* weight, int64_t nplanes, int32_t nranks, int64_t* bounds);
/* host-logic helper (no GPU needed): the local numbering of the slab that owns planes [p0, p1) of `nplanes` planes of
   `plane` cells -- segment offsets, ghost segments and the contiguous chunks exchanged with the neighbours (SURVEY 8e;
   the code path build_numbering on the device ends in).  active: K * Mloc flags, kind-major, over the slab's STORED planes
   [max(p0 - 3, 0), min(p1 + 3, nplanes)), Mloc = stored planes * plane.  out (2 + 10 K int64): n_own, n_ghost, then K
   entries each of cnt_own, off_own, cntL, offL, cntU, offU, sendL_off, sendL_cnt, sendU_off, sendU_cnt (offsets into the
   local vector [owned kinds | lower ghosts | upper ghosts]). */
int32_t pg_slab_numbering_host(int32_t K, int64_t plane, int64_t nplanes, int64_t p0, int64_t p1, const uint8_t* active,
                               int64_t* out);

/* ---- diagnostics (not part of the reference-facing boundary) ------------------------------------------------ */
/* y = A x with two kernel variants (PG_SPMV_VARIANT numbering: 70 stencil slices, 38 chunked CSR, 1 first CSR kernel)
   on the same deterministic vector: max |y_a - y_b| and max |y_a|.  which: 0 constructor matrix, bit 0 run matrix, bit 2
   the matrix the warm loop iterates on (as pg_solver_system_info) */
int32_t pg_debug_spmv_compare(pg_solver* s, int32_t which, int32_t variant_a, int32_t variant_b, double* max_abs_diff,
                              double* max_abs);
/* one launch mode of the slice kernel (0 plain, 1 and 3 with fused dots, 8 Horner step) against the chunked CSR kernel on the
   same deterministic vectors: max |y_a - y_b| (the products are accumulated in the same order: 0 is expected), max |y_a|,
   and the largest relative difference of the fused dot sums (0 for the modes without dots; the partial sums are formed
   in another order).  which as above.  Kernel against kernel on one vector pattern: launch mode 2, a dot operand other than
   x (FinArgs::dotx), the scalar phase folded into the launch and the done flag are not reached from here -- they are covered
   by pg_debug_spmv_apply and its tests against a host product (tests/test_gpu_spmv_host_reference.py) */
int32_t pg_debug_spmv_mode_compare(pg_solver* s, int32_t which, int32_t mode, double* max_abs_diff, double* max_abs,
                                   double* max_dot_rel);
/* sizes of the matrix pg_debug_spmv_compare / _apply work on (which as above): its rows n, the length n_vec >= n of the
   vectors it multiplies (own rows, then ghosts, in its own local numbering), its entries, and the grid (blocks) the Krylov
   driver launches the product with = the number of partial sums per dot slot */
int32_t pg_debug_spmv_sizes(pg_solver* s, int32_t which, int64_t* n, int64_t* n_vec, int64_t* nnz, int32_t* grid);
/* ONE product launch as the Krylov driver issues it (launch_spmv of pg_spmv.h, grid as above), on host data, with everything
   it wrote handed back: what the kernel-vs-kernel comparisons above cannot see -- launch mode 2, a (y, .) dot whose operand
   is not the launch's x, mode 8 with base == x, the scalar phase folded into the launch, the return at the done flag -- is
   checked against an extended-precision product on the host (tests/spmv_reference.py, tests/test_gpu_spmv_host_reference.py).
     variant  70 slices, 38 / 2 chunked CSR, 1 first CSR kernel.  Mode 8, dotx and fold exist in the slice kernel only: refused
              elsewhere, never emulated.
     mode     0: y = A x; 1: + (aux, y); 2: + (d, y), (y, y); 3: + (d, y), (y, y), (aux, y), d = dotx or, when NULL, x;
              8: y = pc2 base + pc0 x + pc1 A x (base NULL: base is the device copy of x itself, as the first step of the
              preconditioner's chain passes it).
     x n_vec; aux (modes 1, 3), dotx (modes 2, 3; optional), base (mode 8; optional): n each, NULL otherwise.
     fold     0: partial sums only.  1 (modes 1 - 3): the last block sums the slots [0, nslots) of the partials into the scalar
              block, nslots = 1 / 2 / 5 for modes 1 / 2 / 3 (mode 3 writes slots 0, 1 and 4; 2 and 3 hold zeros here), without
              deriving a phase.
     done     stored at the done flag of the scalar block before the launch (!= 0: the kernel must return at once).
     repeat   1 or 2 launches back to back on the same buffers.
   Out: y (n + 64: 64 guard words behind row n), partials (5 * grid, slot-major; may be NULL), slot_sums (5: every slot's
   partials summed on the host in index order), folded (5: what the launch left in the scalar block's sum slots) and the
   ticket word after the last launch.  y, partials and the sum slots are filled with PG_DEBUG_SPMV_SENTINEL (a NaN) before
   the first launch: whatever the launch did not write still holds it. */
#define PG_DEBUG_SPMV_SENTINEL 0x7FF8C0DE5EED0BADull
int32_t pg_debug_spmv_apply(pg_solver* s, int32_t which, int32_t variant, int32_t mode, const double* x, const double* aux,
                            const double* dotx, const double* base, double pc0, double pc1, double pc2, int32_t fold,
                            int32_t done, int32_t repeat, double* y, double* partials, double* slot_sums, double* folded,
                            int64_t* ticket);
/* pg_debug_spmv_apply for the Horner launches with an element type per vector stream (launch_spmv_typed of pg_spmv.h: the
   mixed-precision chain), y = pc2 base + pc0 x + pc1 A x with the arithmetic of launch mode 8 on the converted inputs:
     kind 1  first launch: x n_vec doubles, base IS x (pass NULL); y32 = (float)y and p32 = (float)(sigma x) for every row
          2  middle launch: x n_vec floats, base n floats; y32 = (float)y
          3  hand-over launch: x n_vec floats, base n doubles; y64 = y
   pc0, pc1, pc2 go to the kernel as given (the caller folds sigma in).  done as above.  Out: y32 / p32 (n + 64 floats) or y64
   (n + 64 doubles), the others NULL; filled with PG_DEBUG_SPMV_SENTINEL_F32 / PG_DEBUG_SPMV_SENTINEL before the launch. */
#define PG_DEBUG_SPMV_SENTINEL_F32 0x7FC5EED0u
int32_t pg_debug_spmv_apply_typed(pg_solver* s, int32_t which, int32_t kind, const void* x, const void* base, double pc0, double pc1,
                                  double pc2, double sigma, int32_t done, double* y64, float* y32, float* p32);
/* read-only streaming probe: `bytes` read `reps` times with elem_bytes (4|8) per lane, optional non-temporal hint */
int32_t pg_debug_read_probe(int64_t bytes, int32_t elem_bytes, int32_t nt, int32_t blocks, int32_t reps, double* gbs);
/* run the slab-decomposed monophasic path with `nranks` VIRTUAL ranks (host threads sharing this GPU, in-process
   halo exchange / all-reduce standing in for RCCL): Dirichlet(interface_value) on the body, Dirichlet(border_value)
   on `keys`, T0 = 0, initial solve with scheme_ctor then `steps` steps with scheme_run.  x_out: 2M, or NULL (full-size
   rehearsals: sizes and iteration counts only). */
int32_t pg_debug_run_virtual_ranks(int32_t nranks, int32_t N, const int64_t* n, const double* L, int32_t body_kind,
                                   const double* params, int32_t nparams, double interface_value, double border_value,
                                   int32_t nkeys, const int32_t* keys, double dt, int32_t scheme_ctor, int32_t scheme_run,
                                   int64_t steps, double* x_out, int64_t* n_own_out, int64_t* nnz_out,
                                   int64_t* n_ghost_out, int64_t* iters_out);
/* Krylov method (PG_METHOD_*) and GMRES restart length of the virtual-rank runs that follow (default BiCGStab) */
int32_t pg_debug_set_virtual_rank_method(int32_t method, int32_t restart);
/* pg_krylov_opts.precond of the virtual-rank runs that follow (default 0).  PG_PRECOND_MG, PG_PRECOND_MG_CELL and PG_PRECOND_MG_STEP make
   pg_debug_run_virtual_ranks fail with the multigrid's one-rank refusal before any rank starts, PG_PRECOND_POLY_EST with its own */
int32_t pg_debug_set_virtual_rank_precond(int32_t precond);
/* ramp != 0: the virtual-rank runs that follow change the interface value every step, g = interface_value (1 + ramp step)
   (host-driven steps): rows alone on their diagonal move in every step, on every rank */
int32_t pg_debug_set_virtual_rank_ramp(double ramp);
/* step >= 1: the virtual-rank runs that follow take single steps with constant data, and before step `step` (1 = the first)
   every rank multiplies the state at its rows alone on their diagonal by `factor` (pg_debug_scale_diagonal_rows; a rank
   whose loop keeps no such row skips it): the step must end at the state one rank ends at.  step < 0 (default): off */
int32_t pg_debug_set_virtual_rank_kick(int64_t step, double factor);
/* per virtual rank of the last run: rows of the full system, rows / bytes per launch / ghost entries of the system the
   warm loop iterated on (the compact one when loop_rows < full_rows) */
int32_t pg_debug_virtual_rank_info(int32_t rank, int64_t* full_rows, int64_t* loop_rows, int64_t* loop_bytes,
                                   int64_t* loop_ghosts);
/* test hook: multiply the state at every row that is alone on its diagonal by `factor` WITHOUT telling the time loop --
   the next quiet step must notice (S_MOVED) and still end at the right state */
int32_t pg_debug_scale_diagonal_rows(pg_solver* s, double factor);
/* test hook, process-global: iterations > 0 replaces the count (40 + 400 / degree) after which a solve preconditioned with
   the polynomial is given up as stagnated and continues with the plain iteration -- on the full system when it ran on the
   compact one; 0 restores the built-in rule */
int32_t pg_debug_set_poly_give_up(int32_t iterations);

/* Multigrid diagnostics (tests/test_gpu_multigrid.py compares them with the numpy restatement tests/mg_reference.py).  All
   build the hierarchy of the solver's constructor system when it does not exist yet, and refuse what PG_PRECOND_MG refuses.
   Two-call size pattern: with the array arguments NULL only the sizes are written.
   pg_debug_mg_aggregates: agg[i] = the row of level + 1 that row i of `level` belongs to (n rows; level < levels - 1).
   pg_debug_mg_level_csr: the matrix of `level` (0: Â; l >= 1: the Galerkin product P_(l-1)ᵀ A_(l-1) P_(l-1), not equilibrated).
   pg_debug_mg_apply: z = M⁻¹ r, ONE application of the V-cycle as the Krylov loop runs it; r, z: n_own host doubles. */
int32_t pg_debug_mg_aggregates(pg_solver* s, int32_t level, int64_t* n, int32_t* agg);
int32_t pg_debug_mg_level_csr(pg_solver* s, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col, double* val);
int32_t pg_debug_mg_apply(pg_solver* s, const double* r, double* z);
/* the same three on the hierarchy of `precond` = PG_PRECOND_MG (the calls above) or PG_PRECOND_MG_CELL (compared with
   tests/mgc_reference.py by tests/test_gpu_mg_cell.py); they refuse what that value refuses */
int32_t pg_debug_mg_aggregates_for(pg_solver* s, int32_t precond, int32_t level, int64_t* n, int32_t* agg);
int32_t pg_debug_mg_level_csr_for(pg_solver* s, int32_t precond, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col,
                                  double* val);
int32_t pg_debug_mg_apply_for(pg_solver* s, int32_t precond, const double* r, double* z);
/* the same three on the hierarchies of PG_PRECOND_MG_STEP (tests/test_gpu_mg_step.py): which = 0 the constructor's system, 1 the
   run system (it must exist: take a step first).  They build the hierarchy when it does not exist yet and refuse what
   PG_PRECOND_MG_STEP refuses. */
int32_t pg_debug_mg_step_aggregates(pg_solver* s, int32_t which, int32_t level, int64_t* n, int32_t* agg);
int32_t pg_debug_mg_step_level_csr(pg_solver* s, int32_t which, int32_t level, int64_t* n, int64_t* nnz, int64_t* rowptr, int64_t* col,
                                   double* val);
int32_t pg_debug_mg_step_apply(pg_solver* s, int32_t which, const double* r, double* z);

/* The Hessenberg matrix of the estimate pg_solver_spectral_estimate(s, which) describes (tests/test_gpu_specest.py compares it
   with the numpy restatement tests/specest_reference.py): (steps + 1) x steps doubles, column major.  Two-call size pattern:
   with H NULL only `steps` is written. */
int32_t pg_debug_specest_hessenberg(pg_solver* s, int32_t which, int32_t* steps, double* H);

/* The extrapolated start of the time loop's quiet steps (constant data, one rank; no reference counterpart: the reference
   starts every Krylov solve from zero, solver.jl:158-181): `kept` older states are held; the next step starts from
   z^n + sum_j coef[j] (z^(n-offsets[j]) - z^n), j < nstates <= 4, chosen by a least-squares fit of this step's plain start
   residual (sampled weighted squares: rr_plain without, rr_taken with this step's extrapolation).  PG_GUESS_STATES=0: off. */
int32_t pg_solver_guess_info(pg_solver* s, int32_t* kept, int32_t* nstates, int32_t* offsets /* [4] */, double* coef /* [4] */,
                             double* rr_plain, double* rr_taken);

/* Rows whose per-row constants are one value (PG_ROW_CONST, default 1; no reference counterpart): the compact loop's kernels
   take the equilibration weight, the mass, the constant part of the right-hand side and the index maps of such rows from
   their arguments instead of streaming them, in groups of 16 consecutive rows.  out[0], out[1]: groups and qualifying groups
   of the full system's table; out[2], out[3]: of the loop system's -- for the compact system the last step ran on (zeros:
   the last step did not take the compact loop, or PG_ROW_CONST=0). */
int32_t pg_solver_row_const_info(pg_solver* s, int64_t* out /* [4] */);
/* (tests) The mark that says where the constant part of the right-hand side is one value as well, for the same system.  It is
   data, not matrix: valid for one version of that vector, built at the second step in a row that finds the same version (later
   where marks were dropped sooner than they waited).  out[0]: 1 if the last step's launch took a mark; out[1]: groups it marks;
   out[2]: marks built so far on this system; out[3]: launches that took the standing mark. */
int32_t pg_debug_row_const_bconst(pg_solver* s, int64_t* out /* [4] */);

#ifdef __cplusplus
}
#endif
#endif /* PENGUIN_HIP_H */
