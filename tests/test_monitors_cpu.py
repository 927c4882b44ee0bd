"""Monitors without a GPU: the argument errors the drivers raise before any call into the library, and the weight layout of
Probe and Monitor (lengths, block offsets for `phase` and `kind`).  Mesh is a host-only object of the library; nothing here
needs a device."""
import numpy as np
import pytest

from penguin.jl_amd import api


@pytest.fixture(scope="module")
def pj():
    import penguin.jl_amd as pj

    return pj


def test_monitor_classes_are_exported(pj):
    for name in ("Monitor", "VolumeIntegral", "InterfaceFlux", "Probe"):
        assert getattr(pj, name) is getattr(api, name)
    assert api.MON_MAX == 8 and api._MON_KINDS == {"sum": 0, "sumsq": 1}


def test_unknown_kind_is_refused_at_construction(pj):
    with pytest.raises(ValueError, match="unknown monitor kind"):
        pj.Monitor(np.ones(8), kind="max")
    m = pj.Monitor(np.ones(8))
    m.kind = "l1"                                       # (changed behind the constructor's back)
    with pytest.raises(ValueError, match="unknown monitor kind"):
        api._check_monitor_args([m], None, False, False, 8)


def test_too_many_monitors(pj):
    mons = [pj.Monitor(np.ones(8)) for _ in range(9)]
    with pytest.raises(ValueError, match="at most 8 monitors"):
        api._check_monitor_args(mons, None, False, False, 8)
    assert len(api._check_monitor_args(mons[:8], None, False, False, 8)[0]) == 8


def test_wrong_length_and_wrong_type(pj):
    with pytest.raises(ValueError, match="length of Solver.x, 10, not 8"):
        api._check_monitor_args([pj.Monitor(np.ones(8))], None, False, False, 10)
    with pytest.raises(ValueError, match="length of Solver.x, 10, not 8"):
        api._monitor_weights([pj.Monitor(np.ones(8))], 10)
    with pytest.raises(TypeError, match="Monitor objects"):
        api._check_monitor_args([np.ones(8)], None, False, False, 8)


@pytest.mark.parametrize("bad", [0, -3, 1.5, "2", True])
def test_save_every_must_be_a_positive_integer(bad):
    with pytest.raises(ValueError, match="save_every must be an integer >= 1"):
        api._check_monitor_args(None, bad, False, False)


def test_save_every_is_refused_with_verbose_or_log():
    for verbose, log in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="verbose / log"):
            api._check_monitor_args(None, 2, verbose, log)
    assert api._check_monitor_args(None, np.int64(3), False, False) == ([], 3)
    assert api._check_monitor_args(None, None, True, True) == ([], None)


class _FakeSolver:
    """What the drivers look at before their first call into the library."""
    _h = 1
    _nunk = 8


@pytest.mark.parametrize("driver,nargs", [("solve_DiffusionUnsteadyMono_b", 6), ("solve_DiffusionUnsteadyDiph_b", 7),
                                          ("solve_AdvectionDiffusionUnsteadyMono_b", 6), ("solve_AdvectionDiffusionUnsteadyDiph_b", 7),
                                          ("solve_DarcyFlowUnsteady_b", 6)])
def test_the_drivers_raise_before_any_device_call(pj, driver, nargs):
    """Every argument after the solver is None: anything but the argument check would fail on them with another error."""
    fn = getattr(pj, driver)
    rest = [None] * (nargs - 1)
    with pytest.raises(ValueError, match="at most 8 monitors"):
        fn(_FakeSolver(), *rest, "BE", monitors=[pj.Monitor(np.ones(8))] * 9)
    with pytest.raises(ValueError, match="length of Solver.x"):
        fn(_FakeSolver(), *rest, "BE", monitors=[pj.Monitor(np.ones(7))])
    with pytest.raises(ValueError, match="save_every must be"):
        fn(_FakeSolver(), *rest, "BE", save_every=0)
    with pytest.raises(ValueError, match="verbose / log"):
        fn(_FakeSolver(), *rest, "BE", save_every=2, log=True)


def test_block_offsets():
    M = 20
    assert [api._block_offset(M, 2 * M, 0, k) for k in ("omega", "gamma")] == [0, M]
    assert [api._block_offset(M, 4 * M, p, k) for p in (0, 1) for k in ("omega", "gamma")] == [0, M, 2 * M, 3 * M]
    with pytest.raises(ValueError, match="phase 1"):
        api._block_offset(M, 2 * M, 1, "omega")
    with pytest.raises(ValueError, match="kind must be"):
        api._block_offset(M, 2 * M, 0, "border")
    with pytest.raises(ValueError, match="unknowns"):
        api._block_offset(M, 3 * M, 0, "omega")


def test_probe_weight_layout(pj):
    mesh = pj.Mesh((4, 3), (1.0, 1.0))                  # 5 x 4 cells with the padding: M = 20, first coordinate fastest
    M = 20
    for nunk in (2 * M, 4 * M):
        w = pj.Probe(mesh, (1, 2))._weights(nunk)
        assert w.shape == (nunk,) and np.flatnonzero(w).tolist() == [11] and w[11] == 1.0
        w = pj.Probe(mesh, (1, 2), kind="gamma")._weights(nunk)
        assert np.flatnonzero(w).tolist() == [M + 11]
    assert np.flatnonzero(pj.Probe(mesh, 11, kind="omega", phase=1)._weights(4 * M)).tolist() == [2 * M + 11]
    assert np.flatnonzero(pj.Probe(mesh, 11, kind="gamma", phase=1)._weights(4 * M)).tolist() == [3 * M + 11]
    # a point: the cell whose node interval holds it (nodes at x0 + (j + 1/2) h, the reference's mesh)
    x = 0.5 * (mesh.nodes[0][1] + mesh.nodes[0][2])
    y = 0.5 * (mesh.nodes[1][2] + mesh.nodes[1][3])
    assert np.flatnonzero(pj.Probe(mesh, (x, y))._weights(2 * M)).tolist() == [1 + 2 * 5]
    assert pj.Probe(mesh, (x, y)).name == "probe_omega_0_11"
    with pytest.raises(ValueError, match="phase 1"):
        pj.Probe(mesh, 3, phase=1)._weights(2 * M)      # a monophasic solver has no phase 1
    with pytest.raises(ValueError):
        pj.Probe(mesh, 20)
    with pytest.raises(ValueError):
        pj.Probe(mesh, (5, 0))
    with pytest.raises(ValueError):
        pj.Probe(mesh, (1, 2, 3))
    with pytest.raises(ValueError, match="kind must be"):
        pj.Probe(mesh, 3, kind="face")


def test_raw_monitor_weights_are_passed_through(pj):
    a, b = np.arange(8.0), -np.arange(8.0)
    mons = [pj.Monitor(a, name="first"), pj.Monitor(list(b), kind="sumsq")]
    W = api._monitor_weights(mons, 8)
    assert W.shape == (2, 8) and W.dtype == np.float64 and W.flags["C_CONTIGUOUS"]
    assert np.array_equal(W[0], a) and np.array_equal(W[1], b)
    assert [api._MON_KINDS[m.kind] for m in mons] == [0, 1]
