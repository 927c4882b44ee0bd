"""Mass transfer between a disc (phase 1, the "gas") and the fluid around it (phase 2, the "liquid"): the set-up of the
reference's examples/2D/Diffusion/Heat_2ph.jl -- 8 x 8 box, disc of radius 2, jump conditions [[α T]] = 0 with α = (1, 0.5) and
equal fluxes, phase 1 starting at 1 and phase 2 at 0, backward Euler -- and its Sherwood number per step,

    Sh_n = | (c̄g_n − c̄g_{n−1}) / (Γ Δt (He c̄g_{n−1/2} − c̄l_{n−1/2})) | · L / D,

from the volume-weighted phase means c̄g, c̄l.  The reference gets the means by looping over `solver.states`; here they are two
`VolumeIntegral` monitors evaluated on the device after every solve, the time loop runs in one call (`save_every` keeps every
20th state for a picture) and the script never touches `solver.states` for the means.  (The reference's loop weighs only the
first nx + 1 cells, `capacity.V[i, i] for i in 1:nx+1`; the monitors weigh every cell, which is what its comments describe.)

    python examples/sherwood_two_phase.py [n] [steps]        (needs a GPU and the built library; n = 160, steps = 100 by default)
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, DiffusionUnsteadyDiph, Dirichlet, FluxJump, InterfaceConditions,
                            InterfaceFlux, Mesh, Phase, ScalarJump, Sphere, VolumeIntegral, solve_DiffusionUnsteadyDiph_b)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 160
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
lx = 8.0
mesh = Mesh((n, n), (lx, lx), (0.0, 0.0))
centre, radius = (lx / 2, lx / 2), lx / 4
capacity, capacity_c = Capacity(Sphere(centre, radius), mesh), Capacity(Sphere(centre, radius, complement=True), mesh)
gas = Phase(capacity, DiffusionOps(capacity), lambda x, y, z: 0.0, lambda x, y, z: 1.0)
liquid = Phase(capacity_c, DiffusionOps(capacity_c), lambda x, y, z: 0.0, lambda x, y, z: 1.0)
bc_b = BorderConditions({k: Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
He, D = 2.0, 1.0
ic = InterfaceConditions(ScalarJump(1.0, 1.0 / He, 0.0), FluxJump(1.0, 1.0, 0.0))
M = (n + 1) ** 2
u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
dt = 0.5 * (lx / n) ** 2
Tend = (steps - 0.5) * dt

monitors = [VolumeIntegral(capacity, phase=0, name="gas_mean"), VolumeIntegral(capacity_c, phase=1, name="liquid_mean"),
            InterfaceFlux(gas, phase=0, name="gas_interface_flux")]
solver = DiffusionUnsteadyDiph(gas, liquid, bc_b, ic, dt, u0, "BE")
t0 = time.perf_counter()
solve_DiffusionUnsteadyDiph_b(solver, gas, liquid, dt, Tend, bc_b, ic, "BE", monitors=monitors, save_every=20)
secs = time.perf_counter() - t0

cg, cl, flux = (solver.monitor_series[:, k] for k in range(3))
Γ = float(np.sum(capacity.Γ))
cg_half, cl_half = 0.5 * (cg[1:] + cg[:-1]), 0.5 * (cl[1:] + cl[:-1])
Sh = np.abs((cg[1:] - cg[:-1]) / (Γ * dt * (He * cg_half - cl_half))) * lx / D

print(f"{n}^2, {steps} steps in {secs:.2f} s ({steps / secs:.0f} steps/s): {len(solver.monitor_series)} rows of "
      f"{solver.monitor_names}, states kept at steps {solver.state_steps}")
print("    t          gas mean      liquid mean   interface flux   Sh")
for q in sorted(set(list(range(1, len(Sh) + 1, max(1, len(Sh) // 10))) + [len(Sh)])):
    print(f"  {solver.monitor_times[q]:9.5f}   {cg[q]:.8f}    {cl[q]:.8f}    {flux[q]: .6e}   {Sh[q - 1]:.6f}")
# the gas loses what crosses the interface: d/dt (Vg c̄g) against the interface flux of the same step (backward Euler)
Vg = float(np.sum(capacity.V))
balance = Vg * (cg[1:] - cg[:-1]) / dt
print(f"Vg d(c̄g)/dt against the monitored interface flux, last step: {balance[-1]: .6e}  {flux[-1]: .6e}")
