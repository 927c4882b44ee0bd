"""Host parts of the liquid-motion solvers (penguin/jl_amd/liquid.py) against the literal restatement (tests/liquid_oracle.py):
the learning-rate strategies of liquidmotionsolver/diffusion.jl:3-136, adapt_timestep (src/solver.jl:611-662) and the
refusal of N >= 2 meshes.  No GPU needed."""
import math

import numpy as np
import pytest

import penguin.jl_amd as pj
from penguin.jl_amd import liquid
from tests import liquid_oracle as lo

GRADS = [0.3, -0.12, 0.05, 0.05, -1e-3, 2.0e-9, 0.0, 0.7, -0.7, 1e-12, 3.0, float("nan"), 0.2, float("inf"), -0.4]


def _xf_sequence(strategy, opts, grads):
    st = liquid.init_learning_rate_state(strategy, 0.8, **opts)
    so = lo.LRState(strategy, 0.8, **opts)
    xf = xo = 0.4
    out, ref = [], []
    for g in grads:
        s1, s2 = liquid.apply_learning_rate_step_b(st, xf, g), lo.lr_step(so, xo, g)
        xf, xo = xf + s1, xo + s2
        out.append((s1, st.last_lr, xf))
        ref.append((s2, so.last_lr, xo))
    return out, ref


@pytest.mark.parametrize("strategy", ["fixed", "constant", "adagrad", "rmsprop", "rms_prop", "nadam", "barzilai_borwein", "bb",
                                      "secant"])
@pytest.mark.parametrize("opts", [{}, {"decay": 0.1, "min_lr": 0.05, "max_lr": 2.0}, {"min_lr": 0.5, "max_lr": 0.1},
                                  {"eps": 1e-3, "beta1": 0.5, "beta2": 0.9}])
def test_learning_rate_strategies_equal_the_restatement_bit_for_bit(strategy, opts):
    out, ref = _xf_sequence(strategy, opts, GRADS)
    for k, (a, b) in enumerate(zip(out, ref)):
        for u, v in zip(a, b):
            assert (u == v) or (math.isnan(u) and math.isnan(v)), f"{strategy} {opts} step {k}: {a} vs {b}"
    assert all(math.isfinite(s) for s, _, _ in out)        # !isfinite(step) -> 0


def test_secant_clamps_and_guards():
    st = liquid.init_learning_rate_state("secant", 1.0, min_lr=0.5, max_lr=2.0)
    assert liquid.apply_learning_rate_step_b(st, 1.0, 1.0) == 1.0          # no history yet: the fixed step lr * grad
    # Δx = 0.1, Δg = -0.9: proposed = -0.1 * (0.1 / -0.9) = 0.0111.. < min_lr |grad| = 0.05 -> sign * 0.05
    assert liquid.apply_learning_rate_step_b(st, 1.1, 0.1) == 0.5 * 0.1
    # Δx = 1e-3, Δg = 1e-12 <= eps: no secant step, the fixed step clamped to [0.5, 2.0]
    assert liquid.apply_learning_rate_step_b(st, 1.101, 0.1 + 1e-12) == 1.0 * (0.1 + 1e-12)
    st2 = liquid.init_learning_rate_state("secant", 1.0, max_lr=2.0)
    liquid.apply_learning_rate_step_b(st2, 0.0, 1.0)
    # Δx = 1, Δg = -0.999: proposed = -1e-3 * (1 / -0.999) ~ 1e-3 ... large grad instead: clamp at max_lr |grad|
    liquid.apply_learning_rate_step_b(st2, 1.0, 0.999)
    s = liquid.apply_learning_rate_step_b(st2, 1.001, 0.998)                # proposed = -0.998 * (0.001 / -0.001) = 0.998
    assert s == lo.jclamp(-0.998 * ((1.001 - 1.0) / (0.998 - 0.999)), -2.0 * 0.998, 2.0 * 0.998)
    st3 = liquid.init_learning_rate_state("fixed", 1.0)
    assert liquid.apply_learning_rate_step_b(st3, 0.0, float("inf")) == 0.0
    assert liquid.normalize_lr_strategy("Barzilai-Borwein") == "barzilai_borwein"
    assert liquid.normalize_lr_options([("decay", 0.5)]) == {"decay": 0.5}
    with pytest.raises(ValueError):
        liquid.normalize_lr_options(3.0)


@pytest.fixture(scope="module")
def mesh1d():
    return pj.Mesh((40,), (1.0,), (0.0,))


@pytest.mark.parametrize("v,dt,dt_min,dt_max", [
    (1e-12, 0.01, 1e-4, 1.0),     # static interface: grow, CFL 0
    (1e-12, 0.95, 1e-4, 1.0),     # ... up to Δt_max
    (0.1, 0.01, 1e-4, 1.0),       # optimal (0.1125) > current: the reference SHRINKS to 0.8 Δt
    (10.0, 0.01, 1e-4, 1.0),      # optimal (0.001125) < current: the reference GROWS to 1.1 Δt
    (10.0, 0.01, 1e-4, 0.005),    # ... and the clamp to Δt_max
    (1000.0, 1e-5, 1e-4, 1.0),    # clamp to Δt_min
    (0.1, 0.01, 0.5, 0.2),        # Δt_min > Δt_max (the time left): Julia's clamp gives Δt_max
    (1.0, 0.001, 0.5, 0.2),       # ... and Δt_min where the step is below both
])
def test_adapt_timestep_branches(mesh1d, v, dt, dt_min, dt_max):
    got = liquid.adapt_timestep(np.array([v, -0.5 * v]), mesh1d, 0.5, dt, dt_min, dt_max)
    ref = lo.adapt_timestep(np.array([v, -0.5 * v]), mesh1d.nodes, 0.5, dt, dt_min, dt_max)
    assert got == ref
    if v > 1e-10 and dt_min < dt_max:
        opt = 0.9 * 0.5 * (1.0 / 40) / v
        expect = min(opt, 0.8 * dt) if opt > dt else max(opt, 1.1 * dt)
        assert got[0] == lo.jclamp(expect, dt_min, dt_max)


def test_two_dimensional_meshes_are_refused():
    m2 = pj.Mesh((8, 8), (1.0, 1.0), (0.0, 0.0))
    with pytest.raises(pj.PenguinHipError, match="1-D only"):
        pj.MovingLiquidDiffusionUnsteadyMono(None, pj.BorderConditions({}), pj.Dirichlet(0.0), 0.1, None, m2, "BE")
    with pytest.raises(pj.PenguinHipError, match="1-D only"):
        pj.MovingLiquidDiffusionUnsteadyDiph(None, None, pj.BorderConditions({}), None, 0.1, None, m2, "BE")
