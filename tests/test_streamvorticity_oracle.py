"""The reference's three stream function - vorticity testsets (test/solver/stream_vorticity_test.jl) restated on the oracle
composition (tests/streamvorticity_oracle.py), the ABI mirrors of the struct the new entry points pass, and the loud failure
of the product without a GPU.  No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import geometry as og
from oracle import penguin_oracle as po
from tests.streamvorticity_oracle import OracleStreamVorticity

ROOT = Path(__file__).resolve().parent.parent
KEYS = ("left", "right", "bottom", "top")


def _zero_borders():
    return po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS})


def _all_fluid(n):
    mesh = po.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    return po.make_capacity(og.HalfSpace(0, 10.0, N=2), mesh)      # f = x - 10 < 0 everywhere: `body = (x, y) -> -1.0`


def test_uniform_poisson_residual_and_velocity():
    """:8-52 -- 12², ω = sin(πx) sin(πy) at C_ω: the Poisson residual and the velocity's shape."""
    cap = _all_fluid(12)
    s = OracleStreamVorticity(cap, 0.01, 5e-3, bc_stream_border=_zero_borders(), bc_vorticity_border=_zero_borders())
    M = s.M
    s.omega = np.concatenate([np.sin(np.pi * cap.C_w[:, 0]) * np.sin(np.pi * cap.C_w[:, 1]), np.zeros(M)])
    s.solve_stream()
    sys = s.poisson_system(s.omega, s.time)
    residual = np.linalg.norm(sys.A @ s.psi - sys.b) / max(np.linalg.norm(sys.b), 1.0)
    assert residual <= 1e-8                                        # :43
    u, v = s.velocity
    assert len(u) == M and len(v) == M                             # :46-47
    assert np.max(np.abs(u)) > 0 and np.max(np.abs(v)) > 0


def test_step_bookkeeping_on_a_quiescent_field():
    """:54-92 -- 10², ω0 = 0: time, number of states, ω stays zero, times sorted."""
    cap = _all_fluid(10)
    dt = 1e-2
    s = OracleStreamVorticity(cap, 0.02, dt, bc_stream_border=_zero_borders(), bc_vorticity_border=_zero_borders(),
                              omega0=np.zeros(2 * 11 * 11))
    s.step()
    assert abs(s.time - dt) <= 1e-12 and len(s.states) == 2 and np.linalg.norm(s.omega) <= 1e-12    # :82-84
    s.run(2)
    assert abs(s.time - 3 * dt) <= 1e-12 and len(s.states) == 4                                     # :87-88
    times = [st[0] for st in s.states]
    assert times == sorted(times)                                                                   # :91


def test_cut_cell_evolution():
    """:94-134 -- 24², disc r = 0.2 at (0.5, 0.5): a velocity appears, ω stays finite; and the ψ of a state is the Poisson
    solution of the ω of the state before."""
    mesh = po.Mesh((24, 24), (1.0, 1.0), (0.0, 0.0))
    cap = po.make_capacity(og.Ball((0.5, 0.5), 0.2), mesh)
    M = 25 * 25
    r2 = (cap.C_w[:, 0] - 0.5) ** 2 + (cap.C_w[:, 1] - 0.5) ** 2
    w0 = np.concatenate([np.exp(-r2 / 0.04), np.zeros(M)])
    s = OracleStreamVorticity(cap, 5e-3, 5e-3, bc_stream_border=_zero_borders(), bc_vorticity_border=_zero_borders(), omega0=w0)
    s.solve_stream()
    u, v = s.velocity
    assert np.max(np.abs(u)) > 0 and np.max(np.abs(v)) > 0         # :128-129
    s.step()
    assert np.all(np.isfinite(s.omega))                            # :133
    s.step("CN")
    assert np.all(np.isfinite(s.omega))
    for k in (1, 2):
        assert np.array_equal(s.states[k][1], s.poisson(s.states[k - 1][2], s.states[k - 1][0]))
    with pytest.raises(ValueError, match="Unknown scheme"):
        s.step("RK4")


def test_run_info_struct_is_mirrored_field_for_field():
    """pg_streamvort_run_info: the same field names, order and types in include/penguin_hip.h, the ctypes binding and the
    Julia twin."""
    from penguin.jl_amd import _lib as L

    hdr = (ROOT / "include" / "penguin_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} pg_streamvort_run_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [(nm.strip(), typ) for typ, decl in re.findall(r"\b(int64_t|int32_t|double)\s*([^;]+);", body) for nm in decl.split(",")]
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    py = L.pg_streamvort_run_info._fields_
    assert [f[0] for f in py] == [f[0] for f in c_fields]
    assert all(pt is want[ct] for (_, pt), (_, ct) in zip(py, c_fields))
    jl = (ROOT / "julia" / "PenguinHIP.jl").read_text(encoding="utf-8")
    m = re.search(r"struct pg_streamvort_run_info\b(.*?)\bend\b", jl, re.S)
    assert m, "julia/PenguinHIP.jl has no pg_streamvort_run_info"
    jf = re.findall(r"(\w+)::(\w+)", m.group(1).split("pg_streamvort_run_info(")[0])
    jwant = {"int64_t": "Int64", "int32_t": "Int32", "double": "Float64"}
    assert jf == [(n, jwant[t]) for n, t in c_fields]


def test_julia_twin_exports_the_reference_names():
    jl = (ROOT / "julia" / "PenguinHIP.jl").read_text(encoding="utf-8")
    exported = {n.strip() for n in re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1).replace("\n", " ").split(",")}
    for name in ("StreamVorticity", "solve_StreamVorticity!", "step_StreamVorticity!", "run_StreamVorticity!",
                 "run_until_StreamVorticity!"):
        assert name in exported, name
    for sym in ("pg_streamvort_create", "pg_streamvort_step", "pg_streamvort_run", "pg_streamvort_solve_stream",
                "pg_streamvort_get", "pg_streamvort_set_omega"):
        assert "ccall((:%s, libpg)" % sym in jl, sym


def test_streamvorticity_fails_loudly_without_gpu():
    """No CPU fallback: without a HIP device the constructor raises before anything is computed."""
    import penguin.jl_amd as pj
    from penguin.jl_amd import _lib as L

    L.lib()
    n = C.c_int(0)
    ndev = n.value if C.CDLL(None).hipGetDeviceCount(C.byref(n)) == 0 else 0
    if ndev > 0:
        pytest.skip("a GPU is visible: the loud-failure path is exercised on CPU-only boxes")
    mesh = pj.Mesh((4, 4), (1.0, 1.0))
    cap = object.__new__(pj.Capacity)          # (a Capacity cannot be built without a GPU either)
    cap.mesh = mesh
    cap._h = None
    with pytest.raises(pj.PenguinHipError, match="no HIP device|not initialised"):
        pj.StreamVorticity(cap, 0.01, 1e-3)
