"""pg_capacity_create_spacetime_polygon behind a 1-rank RCCL communicator, for tests/test_gpu_moving_polygon.py: the library is
initialised once per process, so the communicator needs a process of its own.

    python scripts/moving_polygon_rank_refusal.py

A valid moving polygon (a translating circle of 40 markers) on a 16^2 mesh: the entry has to refuse it with its "single rank only"
message and hand back no capacity, through the C entry and through Capacity(MovingFront, SpaceTimeMesh).  Exit status 0 when
all of that holds.
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd.moving import time_rule

pj.init_distributed(0, 0, 1, pj.get_unique_id())
lib = L.lib()


def last_error():
    buf = C.create_string_buffer(4096)
    lib.pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
base = pj.create_circle_b(pj.FrontTracker(), 2.01, 2.01, 1.0, 40)
mf = pj.MovingFront.rigid(base, shift=lambda t: (0.5 * t, 0.2 * t))
t0, t1 = 0.1, 0.15
xy0, xy1 = (np.ascontiguousarray(mf.markers(t).reshape(-1)) for t in (t0, t1))
tw = np.ascontiguousarray(np.column_stack(time_rule(t0, t1, 2, 2)))
h = C.c_void_p()
rc = lib.pg_capacity_create_spacetime_polygon(mesh._h, L.dptr(xy0), L.dptr(xy1), C.c_int64(len(xy0) // 2), C.c_int32(0), C.c_double(t0),
                                              C.c_double(t1), C.c_int32(len(tw)), L.dptr(tw), C.byref(h))
msg = last_error()
assert rc != 0 and "pg_capacity_create_spacetime_polygon: single rank only" in msg and not h.value, (rc, msg, h.value)
try:
    pj.Capacity(mf, pj.SpaceTimeMesh(mesh, [t0, t1]))
except pj.PenguinHipError as e:
    assert "single rank only" in str(e), str(e)
else:
    raise AssertionError("Capacity(MovingFront) was built behind a communicator")
print("refused behind a 1-rank communicator:", msg, flush=True)
