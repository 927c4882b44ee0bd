// pg_streamvort.hip -- StreamVorticity (src/solver/streamfunction_vorticity.jl): 2-D incompressible flow around cut-cell bodies,
//   ∇²ψ = -ω,   u = ∂ψ/∂y, v = -∂ψ/∂x,   ∂ω/∂t + (u·∇)ω = ν∇²ω + f
//
//   reference                                                         here
//   StreamVorticity ctor + assemble_laplacian       :73-117            pg_streamvort_create (a steady solver, D = 1, kept for the run)
//   poisson_rhs                                     :126-138           k_sv_source (f = -ωω, so that b₁ = V f) + the solver's b
//   _solve_streamfunction!                          :191-206           solver_solve_again (started from the previous ψ)
//   update_velocity!                                :146-159           k_sv_velocity (∇'s stencil and the rotation in one pass)
//   build_convection                                :167-182           diffops_convection_from_device (uᵧ = [u; v] IS the u, v buffer)
//   A_/b_mono_unstead_advdiff + solve               :226-237           a new unsteady solver per step, state handed over on the device
//   _run! / states                                  :238-254           pg_streamvort_run, padded device copies
//
// ψ, ω, (u, v) and the convection operators never leave the device between steps.  Single rank (Mloc = M), N = 2.
#include <chrono>
#include <memory>
#include <vector>

#include "pg_solver_internal.h"

using namespace pg;

struct pg_streamvort {
  pg_capacity* cap = nullptr;
  pg_diffops* ops_psi = nullptr;     // the caller's DiffusionOps (borrowed): the Poisson system
  pg_diffops* ops_omega = nullptr;   // the handle's own: carries the ConvectionOps of the current velocity
  i64 M = 0;
  double dt = 0.0, t = 0.0;
  pg_bc_desc bc_omega{};
  std::vector<pg_border_desc> borders_omega;
  std::vector<double> border_values_omega;   // per border cell, when the caller gave functions (else empty)
  DevBuf<double> nu;                 // M: ν(C_ω)
  DevBuf<double> f_n, f_np1;         // M each: vorticity source at t / t + Δt (empty: 0)
  DevBuf<double> g_n, g_np1;         // M each: interface values of ω at t / t + Δt (empty: the descriptor's constant)
  pg_solver* psi_solver = nullptr;
  pg_solver* omega_solver = nullptr; // the last step's (its state is the next step's initial state)
  std::vector<double> omega_host;    // the initial / assigned ω (2M) until the first step has consumed it
  bool omega_from_host = true;
  DevBuf<double> psi, omega;         // 2M each: the current [·ω; ·γ] vectors, zeros at eliminated unknowns
  DevBuf<double> uv;                 // 2M: u then v -- the bulk velocity AND uᵧ = [u; v]
  struct State { double t; DevBuf<double> psi, omega; };
  std::vector<State> states;
  ~pg_streamvort() {
    if (omega_solver) (void)pg_solver_destroy(omega_solver);
    if (psi_solver) (void)pg_solver_destroy(psi_solver);
    if (ops_omega) (void)pg_diffops_destroy(ops_omega);
  }
};

namespace {

constexpr int SV_BLOCK = 256;

// the source of the Poisson system from the current vorticity: f = -ωω on the padded layout (b₁ = V f = -V ωω, :131-132)
__global__ void k_sv_source(i64 M, const double* __restrict__ omega, double* __restrict__ f) {
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < M; lc += (i64)gridDim.x * blockDim.x) f[lc] = -omega[lc];
}

// (u, v) = (∂ψ/∂y, -∂ψ/∂x) with ∇ψ = Wꜝ(G ψω + H ψγ) (operators.jl:20-23, the stencil of k_grad) -- :146-156.
// psi: [ψω; ψγ] padded, zeros at eliminated unknowns.  uv: u in [0, M), v in [M, 2M).
__global__ void k_sv_velocity(CapView c, i64 M, const double* __restrict__ psi, double* __restrict__ uv) {
  for (i64 lc = blockIdx.x * (i64)blockDim.x + threadIdx.x; lc < M; lc += (i64)gridDim.x * blockDim.x) {
    i64 idx[3];
    decode_cell(c.N, c.ext, c.plane, c.s0, lc, idx);
    double g[2];
    for (int d = 0; d < 2; ++d) {
      const Line L = load_line(c, d, lc, idx[d]);
      const i64 st = c.stride[d];
      double s = L.gd_j * psi[lc] + L.hd_j * psi[M + lc];
      if (L.has_m) s += L.gl_j * psi[lc - st] + L.hl_j * psi[M + lc - st];
      g[d] = L.w_j * s;
    }
    uv[lc] = g[1];
    uv[M + lc] = -g[0];
  }
}

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  // wall time since the last call, the device's queue drained first
  double lap() {
    PG_HIP(hipStreamSynchronize(ctx().stream));
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};

struct Split {
  double psi_ms = 0.0, velocity_ms = 0.0, build_ms = 0.0, omega_ms = 0.0;
};

void check_status(int32_t rc) {
  if (rc == 0) return;
  char buf[4096];
  pg_last_error(buf, sizeof(buf));
  throw Error(std::string(buf));
}

void upload_m(DevBuf<double>& dst, const double* h, i64 M) {
  if (dst.n != M) dst.alloc(M);
  dst.upload(h, M);
}

// steps 1-3: b from ω, ψ = Aψ⁻¹ b, (u, v)
void solve_stream(pg_streamvort* sv, const pg_krylov_opts* opts, SolveStats& st, Clock* clk, Split* sp) {
  // (before anything is launched: every entry point that takes options comes through here first)
  PG_REQUIRE(!(opts && opts->precond == PG_PRECOND_MG_CELL),
             "multigrid preconditioner (precond = PG_PRECOND_MG_CELL) refused: a StreamVorticity solver -- its stream-function solve "
             "has a Dirichlet interface and is served by PG_PRECOND_MG");
  PG_REQUIRE(!(opts && opts->precond == PG_PRECOND_MG_STEP),
             "multigrid preconditioner (precond = PG_PRECOND_MG_STEP) refused: a StreamVorticity solver -- its stream-function solve "
             "is a steady system (served by PG_PRECOND_MG) and its vorticity solve a new ConvectionOps matrix every step");
  PG_REQUIRE(!(opts && opts->precond == PG_PRECOND_POLY_EST),
             "estimated polynomial preconditioner (precond = PG_PRECOND_POLY_EST) refused: a StreamVorticity solver -- one set of options "
             "serves both of its solves, and the operator of the vorticity solve is a ConvectionOps (DiffusionOps only); the "
             "stream-function solve is a steady system, which the estimate does not admit");
  hipStream_t stream = ctx().stream;
  const i64 M = sv->M;
  const int gr = grid_for(M, SV_BLOCK);
  hipLaunchKernelGGL(k_sv_source, dim3(gr), dim3(SV_BLOCK), 0, stream, M, (const double*)sv->omega.p, solver_source_dev(sv->psi_solver));
  PG_HIP(hipGetLastError());
  solver_data_changed(sv->psi_solver);
  solver_solve_again(sv->psi_solver, opts, st);
  solver_state_padded(sv->psi_solver, sv->psi.p);
  if (clk) sp->psi_ms += clk->lap();
  hipLaunchKernelGGL(k_sv_velocity, dim3(gr), dim3(SV_BLOCK), 0, stream, cap_view(sv->cap), M, (const double*)sv->psi.p, sv->uv.p);
  PG_HIP(hipGetLastError());
}

void keep_state(pg_streamvort* sv) {
  hipStream_t stream = ctx().stream;
  pg_streamvort::State s;
  s.t = sv->t;
  s.psi.alloc(2 * sv->M);
  s.omega.alloc(2 * sv->M);
  PG_HIP(hipMemcpyAsync(s.psi.p, sv->psi.p, sizeof(double) * (size_t)(2 * sv->M), hipMemcpyDeviceToDevice, stream));
  PG_HIP(hipMemcpyAsync(s.omega.p, sv->omega.p, sizeof(double) * (size_t)(2 * sv->M), hipMemcpyDeviceToDevice, stream));
  sv->states.emplace_back(std::move(s));
}

// one step (:216-242); `keep`: push!(states, ...)
void do_step(pg_streamvort* sv, int scheme, const pg_krylov_opts* opts, SolveStats& st_psi, SolveStats& st_omega, bool keep,
             Clock* clk, Split* sp) {
  hipStream_t stream = ctx().stream;
  const i64 M = sv->M;
  solve_stream(sv, opts, st_psi, clk, sp);
  const double* up[3] = {sv->uv.p, sv->uv.p + M, nullptr};
  diffops_convection_from_device(sv->ops_omega, up, sv->uv.p, stream);      // uₒ = (u, v), uᵧ = [u; v]   :176-179
  if (clk) sp->velocity_ms += clk->lap();
  // the vorticity system of this step: a new solver, built from the previous one's state (or from the ω the host gave)
  SolverDeviceData dev;
  dev.D = sv->nu.p;
  dev.f_n = sv->f_n.p; dev.f_np1 = sv->f_np1.p;
  dev.g_n = sv->g_n.p; dev.g_np1 = sv->g_np1.p;
  pg_solver* next = nullptr;
  pg_solver* prev = sv->omega_from_host ? nullptr : sv->omega_solver;
  check_status(solver_create_unsteady_mono_dev(sv->cap, sv->ops_omega, &sv->bc_omega, sv->borders_omega.data(),
                                               (int32_t)sv->borders_omega.size(), dev, sv->dt,
                                               prev ? nullptr : sv->omega_host.data(), prev, scheme, &next));
  std::unique_ptr<pg_solver, int32_t (*)(pg_solver*)> guard(next, pg_solver_destroy);
  if (!sv->border_values_omega.empty()) check_status(pg_solver_set_border_values(next, sv->border_values_omega.data()));
  if (clk) sp->build_ms += clk->lap();
  // the call's one set of options serves both solves: PG_PRECOND_MG is meant for ψ, the vorticity solve runs as with precond = 0
  pg_krylov_opts o_omega;
  const pg_krylov_opts* opts_omega = opts;
  if (opts && opts->precond == PG_PRECOND_MG) { o_omega = *opts; o_omega.precond = 0; opts_omega = &o_omega; }
  solver_first_solve_from_state(next, opts_omega, st_omega);
  solver_state_padded(next, sv->omega.p);
  if (sv->omega_solver) (void)pg_solver_destroy(sv->omega_solver);          // the new one has taken its state
  sv->omega_solver = guard.release();
  sv->omega_from_host = false;
  sv->t += sv->dt;                                                          // :238
  if (keep) keep_state(sv);                                                 // :239
  if (clk) sp->omega_ms += clk->lap();
}

void account(pg_streamvort_run_info& r, const SolveStats& a, const SolveStats& b) {
  r.psi_iters += a.iters; r.psi_products += a.products;
  r.omega_iters += b.iters; r.omega_products += b.products;
  for (const SolveStats* s : {&a, &b}) {
    if (!s->converged) ++r.unconverged;
    if (s->bnorm > 0.0) r.worst_relres = std::max(r.worst_relres, s->resnorm / s->bnorm);
  }
}

}  // namespace

extern "C" {

int32_t pg_streamvort_create(pg_capacity* c, pg_diffops* o, const double* nu, double dt, const pg_bc_desc* bc_stream,
                             const pg_bc_desc* bc_vorticity, const pg_border_desc* borders_stream, int32_t nborders_stream,
                             const pg_border_desc* borders_vorticity, int32_t nborders_vorticity, const double* psi0,
                             const double* omega0, pg_streamvort** out) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(c && o && nu && bc_stream && bc_vorticity && out, "pg_streamvort_create: NULL argument");
  PG_REQUIRE(nborders_stream >= 0 && nborders_vorticity >= 0 && (nborders_stream == 0 || borders_stream) &&
             (nborders_vorticity == 0 || borders_vorticity), "pg_streamvort_create: bad border descriptors");
  PG_REQUIRE(c->N == 2, "StreamVorticity: only the two-dimensional case is supported (the reference's constructor is a "
             "Capacity{2} method), got N = " + std::to_string(c->N));
  PG_REQUIRE(!c->spacetime, "StreamVorticity: a space-time capacity is not a Capacity{2}");
  PG_REQUIRE(ctx().nranks == 1 && !ctx().comm, "StreamVorticity: single rank only");
  PG_REQUIRE(o->cap == c, "pg_streamvort_create: operators were built from a different capacity");
  PG_REQUIRE(!o->has_velocity, "pg_streamvort_create: the operator must be a DiffusionOps without a velocity (the handle builds "
             "the ConvectionOps of its own velocity)");
  PG_REQUIRE(dt > 0.0, "pg_streamvort_create: dt must be positive");
  std::unique_ptr<pg_streamvort> sv(new pg_streamvort());
  sv->cap = c;
  sv->ops_psi = o;
  sv->M = c->slab.M;
  PG_REQUIRE(c->slab.Mloc() == sv->M, "StreamVorticity: single rank only");
  const i64 M = sv->M;
  sv->dt = dt;
  check_status(pg_diffops_create(c, &sv->ops_omega));
  upload_m(sv->nu, nu, M);
  sv->bc_omega = *bc_vorticity;
  if (bc_vorticity->value_array) {
    upload_m(sv->g_n, bc_vorticity->value_array, M);
    upload_m(sv->g_np1, bc_vorticity->value_array, M);
  }
  sv->bc_omega.value_array = nullptr;
  sv->borders_omega.assign(borders_vorticity, borders_vorticity + nborders_vorticity);
  // Aψ = assemble_laplacian(operator, capacity, bc_stream, 1.0) with the border rows of bc_stream_border: the steady
  // monophasic system with D = 1; its source is written from ω before every solve
  check_status(pg_solver_create_steady_mono(c, o, bc_stream, borders_stream, nborders_stream, nullptr, nullptr, &sv->psi_solver));
  sv->psi.alloc(2 * M); sv->omega.alloc(2 * M); sv->uv.alloc(2 * M);
  sv->psi.zero(); sv->omega.zero(); sv->uv.zero();                          // velocity = (zeros(n), zeros(n))   :87
  if (psi0) sv->psi.upload(psi0, 2 * M);
  sv->omega_host.assign(2 * M, 0.0);
  if (omega0) {
    sv->omega_host.assign(omega0, omega0 + 2 * M);
    sv->omega.upload(omega0, 2 * M);
  }
  keep_state(sv.get());                                                     // states = [(0.0, ψ0, ω0)]   :91
  PG_HIP(hipStreamSynchronize(ctx().stream));
  *out = sv.release();
  PG_API_END
}

int32_t pg_streamvort_destroy(pg_streamvort* sv) {
  PG_API_BEGIN
  delete sv;
  PG_API_END
}

int32_t pg_streamvort_set_omega(pg_streamvort* sv, const double* omega) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv && omega, "pg_streamvort_set_omega: NULL argument");
  sv->omega_host.assign(omega, omega + 2 * sv->M);
  sv->omega.upload(omega, 2 * sv->M);
  sv->omega_from_host = true;
  PG_API_END
}

int32_t pg_streamvort_set_source(pg_streamvort* sv, const double* f_n, const double* f_np1) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv, "pg_streamvort_set_source: NULL argument");
  if (f_np1) upload_m(sv->f_np1, f_np1, sv->M);
  if (f_n) upload_m(sv->f_n, f_n, sv->M);
  if (sv->f_n.p && !sv->f_np1.p) { sv->f_np1.alloc(sv->M); sv->f_np1.zero(); }
  PG_API_END
}

int32_t pg_streamvort_set_interface_values(pg_streamvort* sv, int32_t which, const double* g_n, const double* g_np1) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv && (which == PG_SV_PSI || which == PG_SV_OMEGA), "pg_streamvort_set_interface_values: bad arguments");
  if (which == PG_SV_PSI) {
    // build_g_g(operator, bc_stream, capacity, t) (:134): one value per solve
    if (g_np1) check_status(pg_solver_set_interface_value(sv->psi_solver, nullptr, g_np1));
  } else {
    PG_REQUIRE(g_np1 || sv->g_np1.p, "pg_streamvort_set_interface_values: the values at t + Δt are needed first");
    if (g_np1) upload_m(sv->g_np1, g_np1, sv->M);
    if (g_n) upload_m(sv->g_n, g_n, sv->M);
  }
  PG_API_END
}

int32_t pg_streamvort_set_border_values(pg_streamvort* sv, int32_t which, const double* values) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv && values && (which == PG_SV_PSI || which == PG_SV_OMEGA), "pg_streamvort_set_border_values: bad arguments");
  if (which == PG_SV_PSI) {
    check_status(pg_solver_set_border_values(sv->psi_solver, values));
  } else {
    pg_mesh* m = sv->cap->mesh;
    mesh_build_border(m);
    sv->border_values_omega.assign(values, values + m->border_key.size());
  }
  PG_API_END
}

int32_t pg_streamvort_solve_stream(pg_streamvort* sv, const pg_krylov_opts* opts, pg_step_info* info) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv, "pg_streamvort_solve_stream: NULL argument");
  SolveStats st;
  solve_stream(sv, opts, st, nullptr, nullptr);
  solver_step_info(sv->psi_solver, st, sv->t, info);
  PG_API_END
}

int32_t pg_streamvort_step(pg_streamvort* sv, int32_t scheme, const pg_krylov_opts* opts, pg_step_info* info_psi,
                           pg_step_info* info_omega) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv, "pg_streamvort_step: NULL argument");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "Unknown scheme.");
  AsyncAllocScope pool;             // a solver per step: freed blocks are handed out again without synchronising the device
  SolveStats sp, so;
  do_step(sv, scheme, opts, sp, so, true, nullptr, nullptr);
  solver_step_info(sv->psi_solver, sp, sv->t, info_psi);
  solver_step_info(sv->omega_solver, so, sv->t, info_omega);
  PG_API_END
}

int32_t pg_streamvort_run(pg_streamvort* sv, int64_t steps, int32_t scheme, const pg_krylov_opts* opts, int32_t save_every,
                          pg_streamvort_run_info* info) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv, "pg_streamvort_run: NULL argument");
  PG_REQUIRE(scheme == PG_SCHEME_BE || scheme == PG_SCHEME_CN, "Unknown scheme.");
  AsyncAllocScope pool;
  pg_streamvort_run_info r{};
  Clock total, clk;
  Split sp;
  for (int64_t i = 1; i <= steps; ++i) {
    SolveStats a, b;
    do_step(sv, scheme, opts, a, b, save_every > 0 && i % save_every == 0, &clk, &sp);
    account(r, a, b);
    ++r.steps;
  }
  r.total_ms = total.lap();
  r.t_final = sv->t;
  r.psi_ms = sp.psi_ms; r.velocity_ms = sp.velocity_ms; r.build_ms = sp.build_ms; r.omega_ms = sp.omega_ms;
  if (info) *info = r;
  PG_API_END
}

int32_t pg_streamvort_get(const pg_streamvort* sv, int32_t field, int64_t state_index, double* out, int64_t len) {
  PG_API_BEGIN
  require_init();
  PG_REQUIRE(sv && out, "pg_streamvort_get: NULL argument");
  const i64 M = sv->M;
  if (field == PG_SV_U || field == PG_SV_V) {
    PG_REQUIRE(len == M, "pg_streamvort_get: a velocity component has M entries");
    PG_REQUIRE(state_index < 0, "pg_streamvort_get: only the current velocity is kept");
    sv->uv.download(out, M, field == PG_SV_U ? 0 : M);
    return 0;
  }
  PG_REQUIRE(field == PG_SV_PSI || field == PG_SV_OMEGA, "pg_streamvort_get: unknown field");
  PG_REQUIRE(len == 2 * M, "pg_streamvort_get: len must be 2M");
  if (state_index < 0) {
    (field == PG_SV_PSI ? sv->psi : sv->omega).download(out, 2 * M);
  } else {
    PG_REQUIRE(state_index < (i64)sv->states.size(), "pg_streamvort_get: state index out of range");
    const pg_streamvort::State& s = sv->states[(size_t)state_index];
    (field == PG_SV_PSI ? s.psi : s.omega).download(out, 2 * M);
  }
  PG_API_END
}

int32_t pg_streamvort_num_states(const pg_streamvort* sv, int64_t* out) {
  PG_API_BEGIN
  PG_REQUIRE(sv && out, "pg_streamvort_num_states: NULL argument");
  *out = (int64_t)sv->states.size();
  PG_API_END
}

int32_t pg_streamvort_time(const pg_streamvort* sv, int64_t state_index, double* out) {
  PG_API_BEGIN
  PG_REQUIRE(sv && out, "pg_streamvort_time: NULL argument");
  if (state_index < 0) *out = sv->t;
  else {
    PG_REQUIRE(state_index < (i64)sv->states.size(), "pg_streamvort_time: state index out of range");
    *out = sv->states[(size_t)state_index].t;
  }
  PG_API_END
}

int32_t pg_streamvort_solver(pg_streamvort* sv, int32_t which, pg_solver** borrowed) {
  PG_API_BEGIN
  PG_REQUIRE(sv && borrowed && (which == PG_SV_PSI || which == PG_SV_OMEGA), "pg_streamvort_solver: bad arguments");
  *borrowed = which == PG_SV_PSI ? sv->psi_solver : sv->omega_solver;
  PG_API_END
}

}  // extern "C"
