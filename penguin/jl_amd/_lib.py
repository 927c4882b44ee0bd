"""ctypes binding of libpenguin_hip.so -- the same symbols julia/PenguinHIP.jl ccall's.

There is NO CPU fallback: if the shared library is missing, or no HIP device is visible
when a device function is called, the call raises.  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["PG_LIB_PATH"]) if os.environ.get("PG_LIB_PATH") else _HERE / "lib" / "libpenguin_hip.so"   # override: A/B runs of two builds
HEADER_PATH = _HERE.parent.parent / "include" / "penguin_hip.h"


class PenguinHipError(RuntimeError):
    pass


# ---- enums (mirror include/penguin_hip.h) ---------------------------------------------------
PG_BODY_BALL, PG_BODY_MULTIBALL, PG_BODY_HALFSPACE, PG_BODY_ELLIPSOID, PG_BODY_PLANE = 1, 2, 3, 4, 5
PG_BODY_PROGRAM, PG_BODY_POLYGON = 6, 7
PG_FLAG_COMPLEMENT, PG_FLAG_NO_CENTROIDS = 1, 2
PG_CAP_V, PG_CAP_GAMMA, PG_CAP_CELL_TYPES, PG_CAP_A, PG_CAP_B, PG_CAP_W, PG_CAP_C_OMEGA, PG_CAP_C_GAMMA = range(8)
PG_CAP_ST_V0, PG_CAP_ST_V1, PG_CAP_ST_CT_OMEGA, PG_CAP_ST_CT_GAMMA = 8, 9, 10, 11   # space-time capacities only
PG_OP_G, PG_OP_H, PG_OP_WINV = 0, 1, 2
PG_OP_C0, PG_OP_K0 = 3, 6            # ConvectionOps: C_d = PG_OP_C0 + d, K_d = PG_OP_K0 + d
PG_BC_NONE, PG_BC_DIRICHLET, PG_BC_NEUMANN, PG_BC_ROBIN, PG_BC_PERIODIC = 0, 1, 2, 3, 4
PG_KEY = {"left": 0, "right": 1, "bottom": 2, "top": 3, "backward": 4, "forward": 5}
PG_SCHEME = {"BE": 0, "CN": 1, "STEADY": 2}
PG_METHOD = {"bicgstab": 0, "cg": 1, "gmres": 2, "bicgstabl": 3}   # "bicgstabl": BiCGStab(l), chosen by api._krylov_opts when l is given
PG_METHOD_IDRS = 4                   # IDR(s), chosen by api._krylov_opts when nshadow is given; not in PG_METHOD: the bare name "idrs" stays BiCGStab
PG_SV_PSI, PG_SV_OMEGA, PG_SV_U, PG_SV_V = 0, 1, 2, 3   # fields / systems of a pg_streamvort
PG_PRECOND_MG = -2                   # pg_krylov_opts.precond: the aggregation multigrid V-cycle
PG_PRECOND_MG_CELL = -3              # ... on the cell-aggregated hierarchy (Dirichlet, Robin and Neumann interfaces)
PG_PRECOND_POLY_EST = -4             # ... the polynomial of precond = 0, admitted on an estimated spectral disc where Gershgorin refuses
PG_PRECOND_MG_STEP = -5              # ... the cell-aggregated V-cycle inside the unsteady time loop (large steps)
PG_SPECEST_MARGIN = 0.0205           # added to the estimate's max |theta - 1| before the test against 0.95
PG_MG_MAX_LEVELS = 16

c_double_p = C.POINTER(C.c_double)
c_i64_p = C.POINTER(C.c_int64)
c_i32_p = C.POINTER(C.c_int32)


class pg_bc_desc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("alpha", C.c_double), ("beta", C.c_double), ("value", C.c_double),
                ("value_array", c_double_p)]


class pg_border_desc(C.Structure):
    _fields_ = [("key", C.c_int32), ("kind", C.c_int32), ("value", C.c_double)]


class pg_jump_desc(C.Structure):
    _fields_ = [("alpha1", C.c_double), ("alpha2", C.c_double), ("g", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("h", C.c_double), ("g_array", c_double_p), ("h_array", c_double_p)]


class pg_motion_desc(C.Structure):
    _fields_ = [("body_kind", C.c_int32), ("flags", C.c_int32), ("axis", C.c_int32), ("nq", C.c_int32), ("sign", C.c_double),
                ("t0", C.c_double), ("t1", C.c_double), ("nodes", c_double_p), ("body0", C.c_double * 4),
                ("body1", C.c_double * 4)]


class pg_krylov_opts(C.Structure):
    _fields_ = [("method", C.c_int32), ("reltol", C.c_double), ("abstol", C.c_double), ("maxiter", C.c_int32),
                ("check_every", C.c_int32), ("warm_start", C.c_int32), ("restart", C.c_int32), ("precond", C.c_int32)]


class pg_step_info(C.Structure):
    _fields_ = [("iters", C.c_int32), ("converged", C.c_int32), ("resnorm", C.c_double), ("bnorm", C.c_double),
                ("extremum", C.c_double), ("time", C.c_double)]


class pg_run_info(C.Structure):
    _fields_ = [("steps", C.c_int64), ("total_iters", C.c_int64), ("t_final", C.c_double), ("extremum", C.c_double),
                ("solve_ms", C.c_double), ("spmv_ms_total", C.c_double), ("spmv_launches", C.c_int64),
                ("unconverged_steps", C.c_int64), ("worst_relres", C.c_double), ("spmv_lean_ms_total", C.c_double),
                ("spmv_lean_launches", C.c_int64), ("poly_degree", C.c_int64), ("half_exits", C.c_int64),
                ("poly_xspace", C.c_int64), ("products", C.c_int64), ("guess_states_read", C.c_int64),
                ("poly_f32_launches", C.c_int64), ("poly_f32_ms_total", C.c_double), ("poly_f32_timed", C.c_int64),
                ("poly_f32_chains", C.c_int64), ("poly_f32_tail_sum", C.c_int64)]


class pg_system_info(C.Structure):
    _fields_ = [("n_own", C.c_int64), ("nnz", C.c_int64), ("n_ghost", C.c_int64), ("n_omega", C.c_int64),
                ("n_gamma", C.c_int64), ("M_global", C.c_int64), ("spmv_bytes", C.c_int64), ("spmv_slices", C.c_int64),
                ("rows_uniform", C.c_int64), ("rows_pattern", C.c_int64), ("rows_irregular", C.c_int64),
                ("neumann_ok", C.c_int64), ("gershgorin", C.c_double), ("spmv_units", C.c_int64),
                ("rows_marched", C.c_int64), ("rows_matrix", C.c_int64), ("n_ghost_loop", C.c_int64),
                ("loop_is_compact", C.c_int64), ("rows_edge", C.c_int64)]


class pg_streamvort_run_info(C.Structure):
    _fields_ = [("steps", C.c_int64), ("psi_iters", C.c_int64), ("omega_iters", C.c_int64), ("psi_products", C.c_int64),
                ("omega_products", C.c_int64), ("unconverged", C.c_int64), ("worst_relres", C.c_double), ("t_final", C.c_double),
                ("total_ms", C.c_double), ("psi_ms", C.c_double), ("velocity_ms", C.c_double), ("build_ms", C.c_double),
                ("omega_ms", C.c_double)]


class pg_mg_info(C.Structure):
    _fields_ = [("levels", C.c_int32), ("tail_level", C.c_int32), ("rows", C.c_int64 * PG_MG_MAX_LEVELS),
                ("nnz", C.c_int64 * PG_MG_MAX_LEVELS), ("setup_ms", C.c_double), ("bytes", C.c_int64)]


class pg_specest_info(C.Structure):
    _fields_ = [("steps", C.c_int32), ("admitted", C.c_int32), ("gershgorin_admits", C.c_int32), ("reserved", C.c_int32),
                ("g_ritz", C.c_double), ("g_used", C.c_double), ("margin", C.c_double), ("gershgorin", C.c_double),
                ("ritz_re_min", C.c_double), ("ritz_re_max", C.c_double), ("ritz_im_max", C.c_double), ("estimate_ms", C.c_double)]


def declared_symbols() -> list[str]:
    """Every `pg_*` function declared in include/penguin_hip.h."""
    txt = HEADER_PATH.read_text()
    return sorted(set(re.findall(r"\bint32_t\s+(pg_[a-z0-9_]+)\s*\(", txt)))


_lib = None
hip_runtime_source = "system"      # which libamdhip64 the library is bound to ("system", "torch wheel", "already mapped by torch")


def _share_the_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  A PyTorch-ROCm wheel ships its own libamdhip64 / libhsa-runtime64 (SONAMEs
    libamdhip64.so.7, ... -- the system ROCm's SONAMEs) and its libraries ask for them by FILE name (`libamdhip64.so`,
    RPATH $ORIGIN).  Loaded first, torch's copies satisfy libpenguin_hip.so's NEEDED entries by SONAME: one runtime.  Loaded
    second, the file-name lookup does not match the system copy we brought in and a second HIP + HSA runtime is mapped into
    the process.  So when torch is installed but not imported yet, its runtime files are loaded here, before ours resolves
    its dependencies: whichever side comes first, both end up on the same copies (scripts/which_hip_runtime.py lists them).
    PG_HIP_RUNTIME=system keeps the system ROCm.
    (The abort at interpreter exit that round 2 met when torch was imported after the library had another cause -- librccl
    mapped before torch -- and is gone because RCCL is loaded on first use now: csrc/pg_rccl.h.)"""
    global hip_runtime_source
    import sys

    if "torch" in sys.modules:
        hip_runtime_source = "already mapped by torch"
        return
    if os.environ.get("PG_HIP_RUNTIME", "auto") == "system":
        return
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = Path(list(spec.submodule_search_locations)[0]) / "lib"
    if not (libdir / "libamdhip64.so").exists():
        return                                            # a CPU / CUDA build of torch: nothing to share
    mode = C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        if (libdir / name).exists():
            C.CDLL(str(libdir / name), mode=mode)
    hip_runtime_source = "torch wheel"


def lib() -> C.CDLL:
    """Load the shared library (no GPU needed for loading)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise PenguinHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  penguin.jl_amd has no CPU fallback.")
        _share_the_hip_runtime_with_torch()
        _lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
        for name in declared_symbols():
            getattr(_lib, name).restype = C.c_int32
    return _lib


def check(status: int) -> None:
    if status != 0:
        buf = C.create_string_buffer(4096)
        lib().pg_last_error(buf, 4096)
        raise PenguinHipError(buf.value.decode("utf-8", "replace"))


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def iptr(a: np.ndarray):
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_i64_p)


_initialised = False


def init(device: int | None = None) -> None:
    """pg_init on LOCAL_RANK (or `device`); idempotent."""
    global _initialised
    if _initialised:
        return
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    check(lib().pg_init(C.c_int32(device)))
    _initialised = True


def init_distributed(device: int, rank: int, nranks: int, unique_id: bytes | None) -> None:
    global _initialised
    buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
    check(lib().pg_init_distributed(C.c_int32(device), C.c_int32(rank), C.c_int32(nranks), buf))
    _initialised = True


def get_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(lib().pg_get_unique_id(buf))
    return buf.raw


def finalize() -> None:
    global _initialised
    if _initialised:
        check(lib().pg_finalize())
        _initialised = False


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(lib().pg_device_name(buf, 256))
    return buf.value.decode()


def config_string() -> str:
    """Every PG_* tuning / variant selector this process runs with (read once by the library), as `name=value ...`."""
    buf = C.create_string_buffer(2048)
    check(lib().pg_config_string(buf, 2048))
    return buf.value.decode() + f" hip_runtime={hip_runtime_source}"


# ---- diagnostics: the multigrid hierarchy against the numpy restatement (tests/mg_reference.py) -----------------------------
# (precond: PG_PRECOND_MG or PG_PRECOND_MG_CELL, the hierarchy that is meant)
def solver_mg_info(handle, precond: int = PG_PRECOND_MG) -> dict:
    """pg_solver_mg_info_for: levels, first level of the fused tail, rows and nnz per level, set-up ms, device bytes."""
    info = pg_mg_info()
    check(lib().pg_solver_mg_info_for(handle, C.c_int32(precond), C.byref(info)))
    n = info.levels
    return {"levels": n, "tail_level": info.tail_level, "rows": list(info.rows[:n]), "nnz": list(info.nnz[:n]),
            "setup_ms": info.setup_ms, "bytes": info.bytes}


def debug_mg_aggregates(handle, level: int, precond: int = PG_PRECOND_MG) -> np.ndarray:
    """pg_debug_mg_aggregates_for: the row of level + 1 every row of `level` belongs to."""
    n = C.c_int64(0)
    check(lib().pg_debug_mg_aggregates_for(handle, C.c_int32(precond), C.c_int32(level), C.byref(n), None))
    agg = np.zeros(max(n.value, 1), dtype=np.int32)
    check(lib().pg_debug_mg_aggregates_for(handle, C.c_int32(precond), C.c_int32(level), C.byref(n), agg.ctypes.data_as(c_i32_p)))
    return agg[: n.value]


def debug_mg_level_csr(handle, level: int, precond: int = PG_PRECOND_MG):
    """pg_debug_mg_level_csr_for: (rowptr, col, val) of the matrix of `level` (0: the Krylov matrix)."""
    n, nnz = C.c_int64(0), C.c_int64(0)
    pc = C.c_int32(precond)
    check(lib().pg_debug_mg_level_csr_for(handle, pc, C.c_int32(level), C.byref(n), C.byref(nnz), None, None, None))
    rowptr, col, val = np.zeros(n.value + 1, dtype=np.int64), np.zeros(max(nnz.value, 1), dtype=np.int64), np.zeros(max(nnz.value, 1))
    check(lib().pg_debug_mg_level_csr_for(handle, pc, C.c_int32(level), C.byref(n), C.byref(nnz), iptr(rowptr), iptr(col), dptr(val)))
    return rowptr, col[: nnz.value], val[: nnz.value]


def debug_mg_apply(handle, r: np.ndarray, precond: int = PG_PRECOND_MG) -> np.ndarray:
    """pg_debug_mg_apply_for: z = M⁻¹ r, one application of the V-cycle as the Krylov loop runs it."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    z = np.zeros_like(r)
    check(lib().pg_debug_mg_apply_for(handle, C.c_int32(precond), dptr(r), dptr(z)))
    return z


# ---- the same for the hierarchies of PG_PRECOND_MG_STEP (which: 0 the constructor's system, 1 the run system) -----------------
def _mg_info_dict(info) -> dict:
    n = info.levels
    return {"levels": n, "tail_level": info.tail_level, "rows": list(info.rows[:n]), "nnz": list(info.nnz[:n]),
            "setup_ms": info.setup_ms, "bytes": info.bytes}


def solver_mg_step_info(handle, which: int = 0) -> dict:
    """pg_solver_mg_step_info: as solver_mg_info, for the hierarchy of system `which`."""
    info = pg_mg_info()
    check(lib().pg_solver_mg_step_info(handle, C.c_int32(which), C.byref(info)))
    return _mg_info_dict(info)


def debug_mg_step_aggregates(handle, which: int, level: int) -> np.ndarray:
    """pg_debug_mg_step_aggregates: the row of level + 1 every row of `level` belongs to."""
    n = C.c_int64(0)
    check(lib().pg_debug_mg_step_aggregates(handle, C.c_int32(which), C.c_int32(level), C.byref(n), None))
    agg = np.zeros(max(n.value, 1), dtype=np.int32)
    check(lib().pg_debug_mg_step_aggregates(handle, C.c_int32(which), C.c_int32(level), C.byref(n), agg.ctypes.data_as(c_i32_p)))
    return agg[: n.value]


def debug_mg_step_level_csr(handle, which: int, level: int):
    """pg_debug_mg_step_level_csr: (rowptr, col, val) of the matrix of `level` (0: the Krylov matrix of system `which`)."""
    n, nnz = C.c_int64(0), C.c_int64(0)
    w = C.c_int32(which)
    check(lib().pg_debug_mg_step_level_csr(handle, w, C.c_int32(level), C.byref(n), C.byref(nnz), None, None, None))
    rowptr, col, val = np.zeros(n.value + 1, dtype=np.int64), np.zeros(max(nnz.value, 1), dtype=np.int64), np.zeros(max(nnz.value, 1))
    check(lib().pg_debug_mg_step_level_csr(handle, w, C.c_int32(level), C.byref(n), C.byref(nnz), iptr(rowptr), iptr(col), dptr(val)))
    return rowptr, col[: nnz.value], val[: nnz.value]


def debug_mg_step_apply(handle, which: int, r: np.ndarray) -> np.ndarray:
    """pg_debug_mg_step_apply: z = M⁻¹ r, one application of the V-cycle of system `which` as the time loop runs it."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    z = np.zeros_like(r)
    check(lib().pg_debug_mg_step_apply(handle, C.c_int32(which), dptr(r), dptr(z)))
    return z


# ---- the spectral estimate behind precond = PG_PRECOND_POLY_EST against the numpy restatement (tests/specest_reference.py) ----
def solver_spectral_estimate(handle, which: int = 0, run: bool = True) -> dict:
    """pg_solver_spectral_estimate of system `which` (0 constructor, 1 run system).  run=False: report only (steps = 0 when no
    estimate has run on that matrix)."""
    info = pg_specest_info()
    check(lib().pg_solver_spectral_estimate(handle, C.c_int32(which | (0 if run else 4)), C.byref(info)))
    return {k: getattr(info, k) for k, _ in pg_specest_info._fields_ if k != "reserved"}


def debug_specest_hessenberg(handle, which: int = 0, run: bool = True) -> np.ndarray:
    """pg_debug_specest_hessenberg: the (steps + 1) x steps Hessenberg matrix of that estimate."""
    w = C.c_int32(which | (0 if run else 4))
    k = C.c_int32(0)
    check(lib().pg_debug_specest_hessenberg(handle, w, C.byref(k), None))
    H = np.zeros((k.value + 1) * max(k.value, 1))
    check(lib().pg_debug_specest_hessenberg(handle, w, C.byref(k), dptr(H)))
    return H[: (k.value + 1) * k.value].reshape((k.value + 1, k.value), order="F")


# ---- diagnostics: one SpMV launch against the host ---------------------------------------------------------------------------
DEBUG_SPMV_SENTINEL = 0x7FF8C0DE5EED0BAD      # PG_DEBUG_SPMV_SENTINEL
DEBUG_SPMV_GUARD = 64


def debug_spmv_sizes(handle, which: int) -> tuple[int, int, int, int]:
    """pg_debug_spmv_sizes: (rows n, vector length n_vec, entries, grid) of the matrix pg_solver_system_info(which) describes.
    pg_system_info has no n_vec of the loop matrix's own numbering (its layout is pinned by the Julia twin): this gives it."""
    n, nv, nnz, grid = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    check(lib().pg_debug_spmv_sizes(handle, C.c_int32(which), C.byref(n), C.byref(nv), C.byref(nnz), C.byref(grid)))
    return n.value, nv.value, nnz.value, grid.value


def loop_system_csr(handle, which: int):
    """pg_solver_get_system_csr for the preconditioned matrices, 6 / 7 included (the matrix the warm loop multiplies by, which
    no host could form before): (rowptr, col, val) with the columns in that matrix's own local numbering."""
    n, _, nnz, _ = debug_spmv_sizes(handle, which)
    rowptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1))
    check(lib().pg_solver_get_system_csr(handle, C.c_int32(which), iptr(rowptr), iptr(col), dptr(val), None, None))
    return rowptr, col[:nnz], val[:nnz]


def debug_spmv_apply(handle, which: int, variant: int, mode: int, x, aux=None, dotx=None, base=None, pc=(0.0, 0.0, 0.0),
                     fold: int = 0, done: int = 0, repeat: int = 1) -> dict:
    """pg_debug_spmv_apply: ONE launch of the product as the Krylov driver issues it, on host vectors, everything it wrote
    handed back.  Checks what pg_debug_spmv_compare / _mode_compare (kernel against kernel, device-made vectors, two numbers
    back) cannot: launch mode 2, a dot operand that is not x, mode 8 on aliased vectors, the folded scalar phase, the done
    flag -- against a host product (tests/spmv_reference.py).  Returns y (n + 64 guard words), partials (5 x grid),
    slot_sums (5), folded (5), ticket."""
    n, nv, _, grid = debug_spmv_sizes(handle, which)

    def arr(a, length, name):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != length:
            raise ValueError(f"debug_spmv_apply: {name} has {a.size} entries, the matrix needs {length}")
        return a, dptr(a)

    xs, xp = arr(x, nv, "x")
    auxs, auxp = arr(aux, n, "aux")
    dots, dotp = arr(dotx, n, "dotx")
    bases, basep = arr(base, n, "base")
    y = np.zeros(n + DEBUG_SPMV_GUARD)
    partials = np.zeros((5, grid))
    sums, folded = np.zeros(5), np.zeros(5)
    ticket = C.c_int64(-1)
    check(lib().pg_debug_spmv_apply(handle, C.c_int32(which), C.c_int32(variant), C.c_int32(mode), xp, auxp, dotp, basep,
                                    C.c_double(pc[0]), C.c_double(pc[1]), C.c_double(pc[2]), C.c_int32(fold), C.c_int32(done),
                                    C.c_int32(repeat), dptr(y), dptr(partials), dptr(sums), dptr(folded), C.byref(ticket)))
    return {"y": y, "partials": partials, "slot_sums": sums, "folded": folded, "ticket": ticket.value, "grid": grid, "n": n}


DEBUG_SPMV_SENTINEL_F32 = 0x7FC5EED0           # PG_DEBUG_SPMV_SENTINEL_F32
TYPED_FIRST, TYPED_MIDDLE, TYPED_HANDOVER = 1, 2, 3


def debug_spmv_apply_typed(handle, which: int, kind: int, x, base=None, pc=(0.0, 0.0, 0.0), sigma: float = 1.0, done: int = 0) -> dict:
    """pg_debug_spmv_apply_typed: ONE Horner launch of the mixed-precision chain (kind 1 first, 2 middle, 3 hand-over) on host
    vectors.  x: n_vec float64 (kind 1) or float32 (kinds 2, 3); base: None (kind 1: base is x), n float32 (kind 2), n float64
    (kind 3); the arrays must already have these dtypes -- nothing is converted here.  Returns y (n + 64 guard words: float32 for
    kinds 1 and 2, float64 for kind 3) and, for kind 1, p32 (n + 64 float32)."""
    n, nv, _, _ = debug_spmv_sizes(handle, which)
    want_x = np.float64 if kind == TYPED_FIRST else np.float32
    want_b = {TYPED_FIRST: None, TYPED_MIDDLE: np.float32, TYPED_HANDOVER: np.float64}[kind]
    x = np.ascontiguousarray(x)
    if x.dtype != want_x or x.size != nv:
        raise ValueError(f"debug_spmv_apply_typed: x must be {nv} x {np.dtype(want_x).name}")
    if (base is None) != (want_b is None):
        raise ValueError("debug_spmv_apply_typed: base goes with kinds 2 and 3, and only with them")
    bp = None
    if base is not None:
        base = np.ascontiguousarray(base)
        if base.dtype != want_b or base.size != n:
            raise ValueError(f"debug_spmv_apply_typed: base must be {n} x {np.dtype(want_b).name}")
        bp = base.ctypes.data_as(C.c_void_p)
    y64 = np.zeros(n + DEBUG_SPMV_GUARD) if kind == TYPED_HANDOVER else None
    y32 = np.zeros(n + DEBUG_SPMV_GUARD, dtype=np.float32) if kind != TYPED_HANDOVER else None
    p32 = np.zeros(n + DEBUG_SPMV_GUARD, dtype=np.float32) if kind == TYPED_FIRST else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    check(lib().pg_debug_spmv_apply_typed(handle, C.c_int32(which), C.c_int32(kind), x.ctypes.data_as(C.c_void_p), bp,
                                          C.c_double(pc[0]), C.c_double(pc[1]), C.c_double(pc[2]), C.c_double(sigma), C.c_int32(done),
                                          ptr(y64), ptr(y32), ptr(p32)))
    return {"y": y64 if kind == TYPED_HANDOVER else y32, "p32": p32}
