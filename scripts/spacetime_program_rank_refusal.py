"""pg_capacity_create_spacetime_program behind a 1-rank RCCL communicator, for tests/test_gpu_spacetime_program.py: the library is
initialised once per process, so the communicator needs a process of its own.

    python scripts/spacetime_program_rank_refusal.py

A valid moving body (a disc with its traced derivatives) on a 12 x 10 mesh: the entry has to refuse it with its "single rank only"
message and hand back no capacity, through the C entry and through Capacity(DeviceFunction, SpaceTimeMesh).  Exit status 0 when
all of that holds.
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd.devfn import pg_program
from penguin.jl_amd.moving import time_rule

pj.init_distributed(0, 0, 1, pj.get_unique_id())
lib = L.lib()


def last_error():
    buf = C.create_string_buffer(4096)
    lib.pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


mesh = pj.Mesh((12, 10), (4.0, 4.0), (0.1, 0.05))
df = pj.DeviceFunction(lambda x, y, t: np.sqrt((x - 2.013 - 0.8 * t) ** 2 + (y - 1.968) ** 2) - (1.0 + 0.4 * t))
phi, d = df.moving_body_program(2), df.moving_gradient_programs(2)
grad = (pg_program * 2)(*d[:2])
tw = np.ascontiguousarray(np.column_stack(time_rule(0.1, 0.15, 4, 4)))
h = C.c_void_p()
rc = lib.pg_capacity_create_spacetime_program(mesh._h, C.byref(phi), grad, C.byref(d[2]), C.c_int32(0), C.c_double(0.1),
                                              C.c_double(0.15), C.c_int32(len(tw)), L.dptr(tw), C.byref(h))
msg = last_error()
assert rc != 0 and "pg_capacity_create_spacetime_program: single rank only" in msg and not h.value, (rc, msg, h.value)
try:
    pj.Capacity(df, pj.SpaceTimeMesh(mesh, [0.1, 0.15]))
except pj.PenguinHipError as e:
    assert "single rank only" in str(e), str(e)
else:
    raise AssertionError("Capacity(DeviceFunction, SpaceTimeMesh) was built behind a communicator")
print("refused behind a 1-rank communicator:", msg, flush=True)
