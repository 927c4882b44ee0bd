"""pg_capacity_create_polygon behind a 1-rank RCCL communicator, for tests/test_gpu_polygon.py: the library is initialised once
per process, so the communicator needs a process of its own.

    python scripts/polygon_rank_refusal.py

A valid polygon (a circle of 40 markers) on a 16^2 mesh: the entry has to refuse it with its "single rank only" message and hand
back no capacity, through the C entry and through Capacity(FrontTracker).  A closed-form body on the same mesh is still built.
Exit status 0 when all of that holds.
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L

pj.init_distributed(0, 0, 1, pj.get_unique_id())
lib = L.lib()


def last_error():
    buf = C.create_string_buffer(4096)
    lib.pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
front = pj.create_circle_b(pj.FrontTracker(), 2.01, 2.01, 1.0, 40)
xy = np.ascontiguousarray(front.polygon().reshape(-1))
h = C.c_void_p()
rc = lib.pg_capacity_create_polygon(mesh._h, L.dptr(xy), C.c_int64(len(xy) // 2), C.c_int32(0), C.byref(h))
msg = last_error()
assert rc != 0 and "pg_capacity_create_polygon: single rank only" in msg and not h.value, (rc, msg, h.value)
try:
    pj.Capacity(front, mesh)
except pj.PenguinHipError as e:
    assert "single rank only" in str(e), str(e)
else:
    raise AssertionError("Capacity(FrontTracker) was built behind a communicator")
cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)          # the closed-form kinds are none the worse for it
assert abs(cap.V.sum() - np.pi) < 1e-12
print("refused behind a 1-rank communicator:", msg, flush=True)
