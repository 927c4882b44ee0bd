// pg_solver_internal.h -- what a composite handle (pg_streamvort.hip) needs of a pg_solver without seeing inside it.
// Implemented at the end of pg_solver.hip; nothing here crosses the C ABI.
#pragma once
#include "pg_krylov.h"

struct pg_solver;

namespace pg {

// data of one phase that already lives on the device: Mloc doubles each in the local layout, or nullptr (D: 1, sources: 0,
// interface values: the constant of the descriptor; g_n == nullptr with g_np1 set: g_n = g_np1)
struct SolverDeviceData {
  const double* D = nullptr;
  const double* f_n = nullptr;
  const double* f_np1 = nullptr;
  const double* g_n = nullptr;
  const double* g_np1 = nullptr;
};

// pg_solver_create_unsteady_mono with device-resident data and, optionally, the state of a solved solver on the same mesh
// as the initial state (device to device; its active unknowns overwrite T0's).  The system is planned for ONE solve.
// Returns the status of an ABI call (pg_last_error holds the message).
int32_t solver_create_unsteady_mono_dev(pg_capacity* c, pg_diffops* o, const pg_bc_desc* bc_interface, const pg_border_desc* borders,
                                        int32_t nborders, const SolverDeviceData& dev, double dt, const double* T0,
                                        pg_solver* previous, int32_t scheme, pg_solver** out);
i64 solver_mloc(const pg_solver* s);
double* solver_source_dev(pg_solver* s);       // the source f(t+Δt) of phase 1 (Mloc, zero when first asked for): written by the caller ...
void solver_data_changed(pg_solver* s);        // ... who then says so
void solver_solve_again(pg_solver* s, const pg_krylov_opts* opts, SolveStats& st);
void solver_first_solve_from_state(pg_solver* s, const pg_krylov_opts* opts, SolveStats& st);
void solver_state_padded(pg_solver* s, double* padded /* K * Mloc, device */);
void solver_step_info(pg_solver* s, const SolveStats& st, double time, pg_step_info* info);

// device functions (pg_program.hip): entry e of a list: out[row_e] += w_e (c0 P(p_e, t0) + c1 P(p_e, t1)), c0 == 0 skipping
// the first evaluation; n == 0 launches nothing.  row == nullptr: out[e] = the sum itself.
constexpr int TD_EVAL_BLOCK = 256;
void td_eval_launch(const pg_program& P, i64 n, const int* row, const double* w, const double* p0, const double* p1,
                    const double* p2, double c0, double c1, double t0, double t1, double* out, hipStream_t st);

}  // namespace pg
