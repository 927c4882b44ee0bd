"""pg_capacity_create_program behind a 1-rank RCCL communicator, for tests/test_gpu_levelset.py: the library is initialised once
per process, so the communicator needs a process of its own.

    python scripts/levelset_rank_refusal.py

A valid body (a circle with its traced gradient) on a 16^2 mesh: the entry has to refuse it with its "single rank only" message
and hand back no capacity, through the C entry and through Capacity(DeviceFunction(...)).  A closed-form body on the same mesh
is still built.  Exit status 0 when all of that holds.
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd.devfn import pg_program

pj.init_distributed(0, 0, 1, pj.get_unique_id())
lib = L.lib()


def last_error():
    buf = C.create_string_buffer(4096)
    lib.pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
df = pj.DeviceFunction(lambda x, y: np.sqrt((x - 2.01) ** 2 + (y - 2.01) ** 2) - 1.0)
phi, grad = df.body_program(2), (pg_program * 2)(*df.gradient_programs(2))
h = C.c_void_p()
rc = lib.pg_capacity_create_program(mesh._h, C.byref(phi), grad, C.c_int32(0), C.byref(h))
msg = last_error()
assert rc != 0 and "pg_capacity_create_program: single rank only" in msg and not h.value, (rc, msg, h.value)
try:
    pj.Capacity(df, mesh)
except pj.PenguinHipError as e:
    assert "single rank only" in str(e), str(e)
else:
    raise AssertionError("Capacity(DeviceFunction) was built behind a communicator")
cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)          # the closed-form kinds are none the worse for it
assert abs(cap.V.sum() - np.pi) < 1e-12
print("refused behind a 1-rank communicator:", msg, flush=True)
