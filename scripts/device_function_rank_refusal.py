"""pg_solver_set_program and pg_solver_set_border_program behind a 1-rank RCCL communicator, for
tests/test_gpu_device_function.py: the library is initialised once per process, so the communicator needs a process of its own.

    python scripts/device_function_rank_refusal.py

A small unsteady heat solver, its first solve, then both installs: each has to be refused with the "one rank only" message and
leave nothing installed.  Exit status 0 when all of that holds.
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api

pj.init_distributed(0, 0, 1, pj.get_unique_id())
lib = L.lib()


def last_error():
    buf = C.create_string_buffer(4096)
    lib.pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


n = 12
mesh = pj.Mesh((n, n, n), (4.0, 4.0, 4.0))
cap = pj.Capacity(pj.Sphere((2.01, 2.01, 2.01), 1.3), mesh)
bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in ("left", "right", "top", "bottom")})
ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
dt = 0.75 * (4.0 / n) ** 2
s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, None, "BE")
opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
info = L.pg_step_info()
L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))

prog = pj.DeviceFunction(lambda x, y, z, t: 1.0 + x * t).program
times = np.array([[dt, 2 * dt], [2 * dt, 3 * dt]])
for which in (0, 1, 2):
    rc = lib.pg_solver_set_program(s._h, C.c_int32(which), C.c_int32(0), C.byref(prog), C.c_int64(2), L.dptr(times))
    msg = last_error()
    assert rc != 0 and "pg_solver_set_program refused" in msg and "one rank only" in msg, (which, rc, msg)
rc = lib.pg_solver_set_border_program(s._h, C.c_int32(L.PG_KEY["left"]), C.byref(prog), C.c_int64(2), L.dptr(times))
msg = last_error()
assert rc != 0 and "pg_solver_set_border_program refused" in msg and "one rank only" in msg, (rc, msg)

progs, entries = (C.c_int32 * 4)(), (C.c_int64 * 4)()
nrows, cursor = C.c_int64(-1), C.c_int64(-1)
L.check(lib.pg_solver_program_info(s._h, progs, entries, C.byref(nrows), C.byref(cursor)))
assert list(progs) == [0, 0, 0, 0] and list(entries) == [0, 0, 0, 0] and nrows.value == 0, (list(progs), list(entries), nrows.value)
# the solver is none the worse for it: the next step runs on the constructor's data
L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
print("refused behind a 1-rank communicator:", msg, flush=True)
