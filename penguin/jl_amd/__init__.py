"""penguin.jl_amd -- MI355X (gfx950) implementation of Penguin.jl's cut-cell operator assembly and
unsteady-diffusion time-step hot path behind the reference's Mesh/Capacity/Phase/DiffusionOps/Solver API.

All arithmetic runs in libpenguin_hip.so (hand-written HIP kernels, C ABI in include/penguin_hip.h).
There is no CPU fallback: importing works without a GPU (so the ABI can be inspected), any compute
call without the shared library or a HIP device raises PenguinHipError.
"""
from ._lib import PenguinHipError, config_string, device_name, finalize, get_unique_id, init, init_distributed, lib  # noqa: F401
from .api import (  # noqa: F401
    AdvectionDiffusionSteadyDiph, AdvectionDiffusionSteadyMono, AdvectionDiffusionUnsteadyDiph,
    AdvectionDiffusionUnsteadyMono, ConvectionOps, solve_AdvectionDiffusionUnsteadyDiph_b,
    solve_AdvectionDiffusionSteadyDiph_b, solve_AdvectionDiffusionSteadyMono_b, solve_AdvectionDiffusionUnsteadyMono_b,
    BorderConditions, Capacity, Circle, Ellipse, Ellipsoid, DarcyFlow, DarcyFlowUnsteady, DiffusionOps, DiffusionSteadyDiph, DiffusionSteadyMono, DiffusionUnsteadyDiph,
    DiffusionUnsteadyMono, Dirichlet,
    FluxJump, HalfSpace, InterfaceConditions, Mesh, MultiSphere, Neumann, Periodic, Phase, Plane, Robin, ScalarJump, Solver, Sphere,
    check_convergence, check_convergence_diph, div, grad, lp_norm, nC, solve_DarcyFlow_b, solve_DarcyFlowUnsteady_b, solve_darcy_velocity, solve_DiffusionSteadyDiph_b, solve_DiffusionSteadyMono_b,
    solve_DiffusionUnsteadyDiph_b, solve_DiffusionUnsteadyMono_b, TimeSeparable,
    InterfaceFlux, Monitor, Probe, VolumeIntegral,
    DeviceFunction, dev,
)
from .front import (  # noqa: F401,E402
    FrontTracker, MovingFront, add_marker_b, create_circle_b, create_crystal_b, create_ellipse_b, create_rectangle_b, get_markers,
    is_point_inside, sdf, set_markers_b,
)
from .utils import (  # noqa: F401,E402
    cfl_restriction, initialize_poiseuille_velocity_field, initialize_radial_velocity_field,
    initialize_rotating_velocity_field, initialize_temperature_circle_b, initialize_temperature_function_b,
    initialize_temperature_square_b, initialize_temperature_uniform_b,
)
from .vtk import write_vtk  # noqa: F401,E402
from .moving import (  # noqa: F401,E402
    MovingAdvDiffusionUnsteadyDiph, MovingAdvDiffusionUnsteadyMono, MovingCircle, MovingDiffusionUnsteadyDiph,
    MovingDiffusionUnsteadyMono, MovingHalfSpace, MovingSphere, SpaceTimeCapacity, SpaceTimeMesh,
    solve_MovingAdvDiffusionUnsteadyDiph_b, solve_MovingAdvDiffusionUnsteadyMono_b, solve_MovingDiffusionUnsteadyDiph_b,
    solve_MovingDiffusionUnsteadyMono_b,
)
from .liquid import (  # noqa: F401,E402
    LearningRateState, MovingLiquidDiffusionUnsteadyDiph, MovingLiquidDiffusionUnsteadyMono, adapt_timestep,
    apply_learning_rate_step_b, extract_height_profiles, init_learning_rate_state, normalize_lr_options, normalize_lr_strategy,
    solve_MovingLiquidDiffusionUnsteadyDiph_b, solve_MovingLiquidDiffusionUnsteadyMono_b, stefan_terms,
)
from .streamvorticity import (  # noqa: F401,E402
    StreamVorticity, run_StreamVorticity_b, run_until_StreamVorticity_b, solve_StreamVorticity_b, step_StreamVorticity_b,
)
