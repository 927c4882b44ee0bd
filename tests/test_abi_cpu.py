"""CPU checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/penguin_hip.h declares, its host-only entry points (Mesh, slab partition) reproduce the
reference's golden vectors, and compute calls fail loudly without a GPU (no CPU fallback)."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "reference_pins.json").read_text())


@pytest.fixture(scope="module")
def L():
    from penguin.jl_amd import _lib

    if not _lib.LIB_PATH.exists():
        from penguin.jl_amd.build import build_library

        build_library()
    return _lib


def test_library_exports_every_declared_symbol(L):
    syms = L.declared_symbols()
    assert len(syms) >= 35
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in syms if s not in exported]
    assert not missing, f"declared in include/penguin_hip.h but not exported: {missing}"
    lib = L.lib()
    for s in syms:
        assert hasattr(lib, s)


def test_product_does_not_import_oracle():
    for p in (ROOT / "penguin").rglob("*.py"):
        txt = p.read_text()
        assert "import oracle" not in txt and "from oracle" not in txt, f"{p} must not use the oracle"
    for p in (ROOT / "penguin").rglob("*.hip"):
        assert "oracle/" not in p.read_text().replace("oracle/geometry.py", "").replace("the oracle", "")


@pytest.mark.parametrize("N", [1, 2, 3])
def test_mesh_through_abi_matches_reference_vectors(L, N):
    import penguin.jl_amd as pj

    g = GOLD["mesh"][str(N)]
    mesh = pj.Mesh((5,) * N, (1.0,) * N, (0.0,) * N)
    for d in range(N):
        assert mesh.centers[d].tolist() == g["centers"]
    assert mesh.nodes[0].tolist() == GOLD["mesh"]["nodes_1d"]
    assert pj.nC(mesh) == g["nC"]
    b = mesh.tag.border_cells
    assert len(b) == g["n_border"]
    assert [list(b[0][0]), list(b[0][1])] == g["border0"]
    assert [list(b[1][0]), list(b[1][1])] == g["border1"]


def test_mesh_border_order_equals_oracle(L):
    import penguin.jl_amd as pj
    from oracle import penguin_oracle as po

    for dims in [(7,), (4, 6), (3, 5, 4), (2, 2, 2), (1, 3)]:
        N = len(dims)
        a = pj.Mesh(dims, (1.0,) * N, (0.25,) * N)
        b = po.Mesh(dims, (1.0,) * N, (0.25,) * N)
        assert a.tag.border_cells == b.border_cells
        _, _, key = a._border_arrays()
        inv = {v: k for k, v in L.PG_KEY.items()}
        assert [inv[int(k)] for k in key] == [po.classify_boundary_cell_fast(ci, b) for ci, _ in b.border_cells]


def test_partition_planes_balances_weights(L):
    lib = L.lib()
    w = np.zeros(513, dtype=np.int64)
    w[128:385] = 1000           # a sphere occupying the middle planes
    for nr in (1, 2, 4, 8):
        bounds = np.zeros(nr + 1, dtype=np.int64)
        L.check(lib.pg_partition_planes(L.iptr(w), C.c_int64(513), C.c_int32(nr), L.iptr(bounds)))
        assert bounds[0] == 0 and bounds[-1] == 513 and np.all(np.diff(bounds) >= 1)
        loads = [w[bounds[r]:bounds[r + 1]].sum() for r in range(nr)]
        assert max(loads) <= 1.25 * (w.sum() / nr) + 1000
    # more ranks than planes is an error with a message, not a crash
    bounds = np.zeros(9, dtype=np.int64)
    assert lib.pg_partition_planes(L.iptr(w), C.c_int64(4), C.c_int32(8), L.iptr(bounds)) != 0
    buf = C.create_string_buffer(256)
    lib.pg_last_error(buf, 256)
    assert b"fewer planes" in buf.value


def test_compute_fails_loudly_without_gpu(L):
    """No CPU fallback: on a box without a HIP device every compute entry point raises."""
    import penguin.jl_amd as pj

    lib = L.lib()
    # ask the HIP runtime the library is bound to (loaded RTLD_GLOBAL, possibly torch's copy): a second load of
    # libamdhip64.so by file name can fail next to it, which would hide a visible GPU
    n = C.c_int(0)
    ndev = n.value if C.CDLL(None).hipGetDeviceCount(C.byref(n)) == 0 else 0
    if ndev > 0:
        pytest.skip("a GPU is visible: the loud-failure path is exercised on CPU-only boxes")
    mesh = pj.Mesh((4, 4), (1.0, 1.0))
    with pytest.raises(pj.PenguinHipError, match="no HIP device|not initialised"):
        pj.Capacity(pj.Sphere((0.5, 0.5), 0.3), mesh)
    with pytest.raises(pj.PenguinHipError):
        pj.Capacity(lambda x, y: x + y, mesh)    # arbitrary callables are refused, never evaluated on the CPU


@pytest.mark.parametrize("order", ["lib,torch", "torch,lib"])
def test_one_hip_runtime_whichever_of_torch_and_the_library_comes_first(order):
    """A PyTorch-ROCm wheel bundles its own libamdhip64 / libhsa-runtime64 / librccl.  The binding loads torch's HIP runtime
    first when torch is installed, so both orders map exactly one copy of each; and the library no longer brings librccl
    into the process at load time (mapped before torch it made the interpreter abort at exit, round 2): both orders exit 0."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "which_hip_runtime.py"), order], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    mapped = [l.split("mapped:")[1].strip() for l in r.stdout.splitlines() if "mapped:" in l]
    for name in ("libamdhip64", "libhsa-runtime64", "librccl"):
        copies = [m for m in mapped if name in m.rsplit("/", 1)[-1]]
        assert len(copies) == 1, (name, copies)


def test_library_is_not_linked_against_rccl(L):
    """RCCL is dlopen'ed when the first communicator is created (csrc/pg_rccl.h): a single-GPU host never maps it."""
    out = subprocess.run(["readelf", "-d", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    needed = [l for l in out.splitlines() if "NEEDED" in l]
    assert needed and not any("rccl" in l for l in needed), needed


@pytest.mark.parametrize("name", ["pg_bc_desc", "pg_border_desc", "pg_jump_desc", "pg_motion_desc", "pg_krylov_opts", "pg_step_info",
                                  "pg_run_info", "pg_system_info"])
def test_ctypes_structs_match_the_header_field_for_field(L, name):
    """The Python binding's ctypes mirror of every struct that crosses the ABI: same field names, order and types as
    include/penguin_hip.h (a field appended on one side only shifts everything behind it silently)."""
    import re

    hdr = (ROOT / "include" / "penguin_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = []
    for typ, decl in re.findall(r"\b(const double\s*\*|int64_t|int32_t|double)\s*([^;]+);", body):
        for nm in decl.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", nm)
            assert m, (name, nm)
            c_fields.append((m.group(1), typ.replace(" ", ""), int(m.group(2)) if m.group(2) else 0))
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "constdouble*": C.POINTER(C.c_double)}
    py_fields = getattr(L, name)._fields_
    assert [f[0] for f in py_fields] == [f[0] for f in c_fields], (py_fields, c_fields)
    for (pn, pt), (cn, ct, cl) in zip(py_fields, c_fields):
        if cl:
            assert issubclass(pt, C.Array) and pt._length_ == cl and pt._type_ is want[ct], (name, pn, pt)
        else:
            assert pt is want[ct] or (ct == "constdouble*" and pt._type_ is C.c_double), (name, pn, pt, ct)
