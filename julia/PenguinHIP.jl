# PenguinHIP.jl -- drop-in replacement of Penguin.jl's hot path
#     Mesh -> Capacity -> DiffusionOps -> Phase -> DiffusionUnsteadyMono / Diph -> solve_DiffusionUnsteady*!
# (and the steady twins) on AMD MI355X: same exported names, positional / keyword signatures and field names as
# Penguin.jl (src/Penguin.jl:25-75); every numeric operation is done by libpenguin_hip.so through `ccall`
# (C ABI: include/penguin_hip.h).
#
# STATUS: there is no Julia in the authoring container (`which julia` is empty), so this file has never been parsed or
# executed.  It is the reference-side binding a maintainer would add (INTEGRATION.md); the Python mirror
# penguin/jl_amd/api.py binds the SAME symbols with ctypes, follows the same steps in the same order and is what the
# test-suite drives on the GPU.  Everything a caller can reach below is bound to the ABI -- nothing is stubbed; inputs
# the GPU path cannot take (arbitrary level-set closures) raise instead of being replaced by something else.
module PenguinHIP

using SparseArrays, StaticArrays, LinearAlgebra, Libdl

export FrontTracker, get_markers, set_markers!, add_marker!, create_circle!, create_ellipse!, create_crystal!, is_point_inside, sdf
export Mesh, nC, Capacity, capacity_from_arrays, Sphere, MultiSphere, HalfSpace, Ellipsoid, Plane, plane_through, DiffusionOps, Phase,
       Dirichlet, Neumann, Robin, Periodic, ScalarJump, FluxJump, BorderConditions, InterfaceConditions, Solver,
       DiffusionUnsteadyMono, solve_DiffusionUnsteadyMono!, DiffusionUnsteadyDiph, solve_DiffusionUnsteadyDiph!,
       DiffusionSteadyMono, solve_DiffusionSteadyMono!, DiffusionSteadyDiph, solve_DiffusionSteadyDiph!,
       ConvectionOps, AdvectionDiffusionSteadyMono, solve_AdvectionDiffusionSteadyMono!, AdvectionDiffusionSteadyDiph,
       solve_AdvectionDiffusionSteadyDiph!, AdvectionDiffusionUnsteadyMono, solve_AdvectionDiffusionUnsteadyMono!,
       AdvectionDiffusionUnsteadyDiph, solve_AdvectionDiffusionUnsteadyDiph!,
       SpaceTimeMesh, MovingSphere, MovingHalfSpace, SpaceTimeCapacity, MovingDiffusionUnsteadyMono,
       solve_MovingDiffusionUnsteadyMono!, MovingDiffusionUnsteadyDiph, solve_MovingDiffusionUnsteadyDiph!,
       MovingAdvDiffusionUnsteadyMono, solve_MovingAdvDiffusionUnsteadyMono!, MovingAdvDiffusionUnsteadyDiph,
       solve_MovingAdvDiffusionUnsteadyDiph!, MovingLiquidDiffusionUnsteadyMono, solve_MovingLiquidDiffusionUnsteadyMono!,
       MovingLiquidDiffusionUnsteadyDiph, solve_MovingLiquidDiffusionUnsteadyDiph!, config_string, guess_info, mg_info, mg_step_info, spectral_estimate,
       StreamVorticity, solve_StreamVorticity!, step_StreamVorticity!, run_StreamVorticity!, run_until_StreamVorticity!,
       set_separable!, clear_separable!, time_data_info, Monitor, VolumeIntegral, InterfaceFlux, Probe, set_monitors!,
       clear_monitors!, monitor_info, monitor_series, drop_states!, ∇, ∇₋, gmres, bicgstabl, cg, idrs

const libpg = get(ENV, "PENGUIN_HIP_LIB", joinpath(@__DIR__, "..", "penguin", "jl_amd", "lib", "libpenguin_hip.so"))

function check(status::Int32)
    if status != 0
        buf = zeros(UInt8, 4096)
        ccall((:pg_last_error, libpg), Int32, (Ptr{UInt8}, Csize_t), buf, length(buf))
        error(unsafe_string(pointer(buf)))          # Penguin.jl raises with error(...) too
    end
    nothing
end

const _initialised = Ref(false)
function init(device::Integer=0)
    _initialised[] && return
    check(ccall((:pg_init, libpg), Int32, (Int32,), device))
    _initialised[] = true
    nothing
end

# Markers with IterativeSolvers' names: `method = gmres` (the default of solve_system!, src/solver.jl:158), `bicgstabl`, `cg`,
# `idrs`.
# Passing the real IterativeSolvers functions works too: only the NAME of the function is looked at.
function gmres end
function bicgstabl end
function cg end
function idrs end
# method -> PG_METHOD_*: cg -> 1, gmres -> 2 (restarted GMRES on the device), bicgstabl WITH the keyword l -> 3 (BiCGStab(l),
# l = 1 .. 8, DESIGN.md "BiCGStab(l)"), idrs WITH the keyword s -> 4 (IDR(s), s = 1 .. 8, DESIGN.md "IDR(s)"), everything else
# (`\`, bicgstabl without l, idrs without s) -> 0 = BiCGStab
function _method_name(m)
    m isa Symbol ? String(m) : (m isa Function ? String(nameof(m)) : "")
end
function _method_id(m, kw = NamedTuple())
    n = _method_name(m)
    n == "cg" && return Int32(1)
    n == "gmres" && return Int32(2)
    (n == "idrs" && haskey(kw, :s)) && return Int32(4)
    (n == "bicgstabl" && haskey(kw, :l)) ? Int32(3) : Int32(0)
end

# ---------------------------------------------------------------------------------- plain structs of the ABI
struct pg_bc_desc; kind::Int32; alpha::Float64; beta::Float64; value::Float64; value_array::Ptr{Float64}; end
struct pg_border_desc; key::Int32; kind::Int32; value::Float64; end
struct pg_jump_desc
    alpha1::Float64; alpha2::Float64; g::Float64; beta1::Float64; beta2::Float64; h::Float64
    g_array::Ptr{Float64}; h_array::Ptr{Float64}
end
struct pg_krylov_opts
    method::Int32; reltol::Float64; abstol::Float64; maxiter::Int32; check_every::Int32; warm_start::Int32
    restart::Int32; precond::Int32
end
mutable struct pg_step_info
    iters::Int32; converged::Int32; resnorm::Float64; bnorm::Float64; extremum::Float64; time::Float64
    pg_step_info() = new(0, 0, 0.0, 0.0, 0.0, 0.0)
end
mutable struct pg_run_info
    steps::Int64; total_iters::Int64; t_final::Float64; extremum::Float64; solve_ms::Float64
    spmv_ms_total::Float64; spmv_launches::Int64; unconverged_steps::Int64; worst_relres::Float64
    spmv_lean_ms_total::Float64; spmv_lean_launches::Int64; poly_degree::Int64; half_exits::Int64; poly_xspace::Int64
    products::Int64; guess_states_read::Int64
    poly_f32_launches::Int64; poly_f32_ms_total::Float64; poly_f32_timed::Int64; poly_f32_chains::Int64; poly_f32_tail_sum::Int64
    pg_run_info() = new(0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0)
end
mutable struct pg_streamvort_run_info
    steps::Int64; psi_iters::Int64; omega_iters::Int64; psi_products::Int64; omega_products::Int64; unconverged::Int64
    worst_relres::Float64; t_final::Float64; total_ms::Float64; psi_ms::Float64; velocity_ms::Float64; build_ms::Float64
    omega_ms::Float64
    pg_streamvort_run_info() = new(0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
end
# kwargs... of solve_system! (src/solver.jl:158-188) -> the options of the device Krylov solve.  reltol defaults to 1e-12,
# not IterativeSolvers' sqrt(eps): the parity target is the direct-solve path; warm_start and precond are not in the
# reference (warm_start=false, precond=-1 give IterativeSolvers' plain iteration from a zero initial guess).
# precond = :mg (PG_PRECOND_MG): the aggregation multigrid V-cycle -- steady monophasic diffusion with a Dirichlet interface and
# the stream-function solve of a StreamVorticity; the library refuses it anywhere else.
# precond = :mg_cell (PG_PRECOND_MG_CELL): the same V-cycle on the cell-aggregated hierarchy -- steady monophasic diffusion
# (DarcyFlow included) with a Dirichlet, Robin or Neumann interface.
# precond = :poly_est (PG_PRECOND_POLY_EST): the polynomial preconditioner of precond = 0, admitted on an estimated spectral disc
# where Gershgorin refuses it -- diphasic systems and Robin / Neumann interfaces of the unsteady diffusion solvers; one rank,
# BiCGStab, DiffusionOps, no moving body; the library refuses it anywhere else (spectral_estimate tells what the estimate found).
# precond = :mg_step (PG_PRECOND_MG_STEP): the cell-aggregated V-cycle inside the time loop of DiffusionUnsteadyMono /
# DarcyFlowUnsteady (Dirichlet, Robin or Neumann interface) and DiffusionUnsteadyDiph (BE and CN; DiffusionOps, one rank, BiCGStab)
# for steps far above h²; one hierarchy per assembled matrix (mg_step_info).  The library refuses it on steady and moving solvers, a
# ConvectionOps, a StreamVorticity, cg / gmres / bicgstabl with l, and where a coarse diagonal entry is not positive.
const PG_PRECOND_MG = Int32(-2)
const PG_PRECOND_MG_CELL = Int32(-3)
const PG_PRECOND_POLY_EST = Int32(-4)
const PG_PRECOND_MG_STEP = Int32(-5)
function _precond_id(p)
    p isa Symbol || return Int32(p)
    p === :mg && return PG_PRECOND_MG
    p === :poly_est && return PG_PRECOND_POLY_EST
    p === :mg_step && return PG_PRECOND_MG_STEP
    p === :mg_cell || error("precond must be an integer, :mg, :mg_cell, :mg_step or :poly_est, not :$(p)")
    PG_PRECOND_MG_CELL
end
# method = bicgstabl, l = 2 (4, ...): BiCGStab(l) -- one rank, zero initial guess, plain (refused with precond = m >= 1, :mg,
# :mg_cell, :mg_step, :poly_est; l > 8 is refused).  Its iteration counts are BiCG sub-steps, two products each, the unit maxiter caps;
# max_mv_products (IterativeSolvers' spelling) is converted: maxiter = max_mv_products ÷ 2.  Without l the name means BiCGStab.
# method = idrs, s = 4 (8, ...): IDR(s) -- one rank, plain (refused with the same preconditioners; s > 8 is refused, s <= 0 means
# 8); s travels in `restart`.  Its iteration counts are updates of x, one product each: maxiter is passed unchanged and caps that
# unit.  With warm_start a steady re-solve and a time step start from the previous state.  Without s the name means BiCGStab.
function _opts(method, kw; warm_default::Bool=true)
    id = _method_id(method, kw)
    maxiter = haskey(kw, :maxiter) ? Int32(kw[:maxiter]) :
              ((id != Int32(4) && haskey(kw, :max_mv_products)) ? Int32(max(1, Int(kw[:max_mv_products]) ÷ 2)) : Int32(0))
    restart = id == Int32(3) ? Int32(kw[:l]) : (id == Int32(4) ? Int32(kw[:s]) : Int32(get(kw, :restart, 0)))
    pg_krylov_opts(id, Float64(get(kw, :reltol, 1e-12)), Float64(get(kw, :abstol, 0.0)),
                   maxiter, Int32(4), Int32(get(kw, :warm_start, warm_default) ? 1 : 0),
                   restart, _precond_id(get(kw, :precond, 0)))
end

# ---------------------------------------------------------------------------------- Mesh  (src/mesh.jl:41-79)
struct MeshTag{N}
    border_cells::Vector{Tuple{CartesianIndex{N}, NTuple{N, Float64}}}
end
abstract type AbstractMesh end
mutable struct Mesh{N} <: AbstractMesh
    centers::NTuple{N, Vector{Float64}}
    nodes::NTuple{N, Vector{Float64}}
    tag::MeshTag{N}
    dims::NTuple{N, Int}
    border_keys::Vector{Int32}        # PG_KEY_* of every border cell, in tag.border_cells order (not a Penguin.jl field)
    handle::Ptr{Cvoid}
end
function Mesh(n::NTuple{N, Int}, domain_size::NTuple{N, Float64}, x0::NTuple{N, Float64}=ntuple(_ -> 0.0, N)) where N
    h = Ref{Ptr{Cvoid}}(C_NULL)
    nv, Lv, xv = collect(Int64, n), collect(Float64, domain_size), collect(Float64, x0)
    check(ccall((:pg_mesh_create, libpg), Int32, (Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                N, nv, Lv, xv, h))
    centers = ntuple(N) do d
        v = Vector{Float64}(undef, n[d])
        check(ccall((:pg_mesh_get_centers, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64), h[], d - 1, v, n[d]))
        v
    end
    nodes = ntuple(N) do d
        v = Vector{Float64}(undef, n[d] + 1)
        check(ccall((:pg_mesh_get_nodes, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64), h[], d - 1, v, n[d] + 1))
        v
    end
    nb = Ref{Int64}(0)
    check(ccall((:pg_mesh_num_border_cells, libpg), Int32, (Ptr{Cvoid}, Ptr{Int64}), h[], nb))
    idx = Matrix{Int64}(undef, N, nb[]); pos = Matrix{Float64}(undef, N, nb[]); key = Vector{Int32}(undef, nb[])
    check(ccall((:pg_mesh_get_border_cells, libpg), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}), h[], idx, pos, key))
    border = [(CartesianIndex(ntuple(d -> Int(idx[d, q]), N)), ntuple(d -> pos[d, q], N)) for q in 1:nb[]]
    m = Mesh{N}(centers, nodes, MeshTag{N}(border), n, key, h[])
    finalizer(x -> ccall((:pg_mesh_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), m)
    m
end
nC(mesh::AbstractMesh) = prod(mesh.dims)

# ---------------------------------------------------------------------------------- bodies
# Tagged level sets the GPU can evaluate; calling one gives the signed function a Penguin.jl closure would.
abstract type TaggedBody <: Function end
struct Sphere{N} <: TaggedBody
    center::NTuple{N, Float64}
    radius::Float64
    complement::Bool
end
Sphere(center::NTuple{N, Float64}, radius::Float64; complement::Bool=false) where N = Sphere{N}(center, radius, complement)
function (s::Sphere{N})(x...) where N
    f = sqrt(sum((x[d] - s.center[d])^2 for d in 1:N)) - s.radius
    s.complement ? -f : f
end
_abi(s::Sphere{N}, ::Val{N}) where N = (Int32(1), vcat(collect(s.center), s.radius), s.complement)

# union of pairwise disjoint spheres of one radius, f = min_s f_s (the weak-scaling body of the benchmark)
struct MultiSphere{N} <: TaggedBody
    centers::Vector{NTuple{N, Float64}}
    radius::Float64
end
(s::MultiSphere{N})(x...) where N = minimum(sqrt(sum((x[d] - c[d])^2 for d in 1:N)) - s.radius for c in s.centers)
_abi(s::MultiSphere{N}, ::Val{N}) where N =
    (Int32(2), vcat(s.radius, Float64(length(s.centers)), [c[d] for c in s.centers for d in 1:N]), false)

# f(x) = sign * (x[axis] - position): the 1-D diphasic bodies `(x,_=0) -> x - xint` (test/convergence_test.jl:111) and their
# extrusions.  `axis` is 1-based here (Julia), 0-based in the ABI.
struct HalfSpace <: TaggedBody
    axis::Int
    position::Float64
    sign::Float64
    complement::Bool
end
HalfSpace(axis::Int, position::Float64, sign::Real=1.0; complement::Bool=false) =
    HalfSpace(axis, position, sign < 0 ? -1.0 : 1.0, complement)
function (s::HalfSpace)(x...)
    f = s.sign * (x[s.axis] - s.position)
    s.complement ? -f : f
end
function _abi(s::HalfSpace, ::Val{N}) where N
    1 <= s.axis <= N || error("HalfSpace: axis $(s.axis) does not exist on a $(N)-D mesh")
    (Int32(3), [Float64(s.axis - 1), s.position, s.sign], s.complement)
end
"f(x) = sqrt(sum(((x_d - c_d) / a_d)^2)) - 1 with axis-aligned semi-axes (PG_BODY_ELLIPSOID); complement: -f"
struct Ellipsoid{N} <: TaggedBody
    center::NTuple{N, Float64}
    semi_axes::NTuple{N, Float64}
    complement::Bool
end
Ellipsoid(center::NTuple{N, Float64}, semi_axes::NTuple{N, Float64}; complement::Bool=false) where N = Ellipsoid{N}(center, semi_axes, complement)
function (s::Ellipsoid{N})(x...) where N
    f = sqrt(sum(((x[d] - s.center[d]) / s.semi_axes[d])^2 for d in 1:N)) - 1.0
    s.complement ? -f : f
end
_abi(s::Ellipsoid{N}, ::Val{N}) where N = (Int32(4), Float64[s.center..., s.semi_axes...], s.complement)
"f(x) = normal . x - offset, an oblique half space (PG_BODY_PLANE); the normal is used as given, never normalised; complement: -f"
struct Plane{N} <: TaggedBody
    normal::NTuple{N, Float64}
    offset::Float64
    complement::Bool
end
Plane(normal::NTuple{N, Float64}, offset::Float64; complement::Bool=false) where N = Plane{N}(normal, offset, complement)
"the plane through `point` with the given normal: offset = normal . point"
plane_through(point::NTuple{N, Float64}, normal::NTuple{N, Float64}; complement::Bool=false) where N =
    Plane{N}(normal, sum(normal[d] * point[d] for d in 1:N), complement)
function (s::Plane{N})(x...) where N
    f = sum(s.normal[d] * x[d] for d in 1:N) - s.offset
    s.complement ? -f : f
end
_abi(s::Plane{N}, ::Val{N}) where N = (Int32(5), Float64[s.normal..., s.offset], s.complement)
_abi(s::Plane{K}, ::Val{N}) where {K, N} = error("PG_BODY_PLANE: a normal of $(K) components on a $(N)-D mesh")

# ---------------------------------------------------------------------------------- Capacity (src/capacity.jl:25-36)
abstract type AbstractCapacity end
mutable struct Capacity{N} <: AbstractCapacity
    A::NTuple{N, SparseMatrixCSC{Float64, Int}}
    B::NTuple{N, SparseMatrixCSC{Float64, Int}}
    V::SparseMatrixCSC{Float64, Int}
    W::NTuple{N, SparseMatrixCSC{Float64, Int}}
    C_ω::Vector{SVector{N, Float64}}
    C_γ::Vector{SVector{N, Float64}}
    Γ::SparseMatrixCSC{Float64, Int}
    cell_types::Vector{Float64}
    mesh::AbstractMesh
    body::Function
    handle::Ptr{Cvoid}
end
const PG_CAP_V, PG_CAP_GAMMA, PG_CAP_CELL_TYPES, PG_CAP_A, PG_CAP_B, PG_CAP_W, PG_CAP_C_OMEGA, PG_CAP_C_GAMMA = 0:7
function _field(h, field, d, M)
    v = zeros(M)
    check(ccall((:pg_capacity_get, libpg), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int64), h, field, d, v, M))
    v
end
_diag(v) = spdiagm(0 => v)          # diagonal matrices store explicit zeros, as `spdiagm` does in the reference
function _wrap_capacity(h::Ptr{Cvoid}, mesh::Mesh{N}, body, compute_centroids::Bool) where N
    M = prod(mesh.dims .+ 1)
    A = ntuple(d -> _diag(_field(h, PG_CAP_A, d - 1, M)), N)
    B = ntuple(d -> _diag(_field(h, PG_CAP_B, d - 1, M)), N)
    W = ntuple(d -> _diag(_field(h, PG_CAP_W, d - 1, M)), N)
    cw = [_field(h, PG_CAP_C_OMEGA, d - 1, M) for d in 1:N]
    C_ω = [SVector{N, Float64}(ntuple(d -> cw[d][i], N)) for i in 1:M]
    C_γ = if compute_centroids
        cg = [_field(h, PG_CAP_C_GAMMA, d - 1, M) for d in 1:N]
        [SVector{N, Float64}(ntuple(d -> cg[d][i], N)) for i in 1:M]
    else
        Vector{SVector{N, Float64}}(undef, 0)
    end
    c = Capacity{N}(A, B, _diag(_field(h, PG_CAP_V, 0, M)), W, C_ω, C_γ, _diag(_field(h, PG_CAP_GAMMA, 0, M)),
                    _field(h, PG_CAP_CELL_TYPES, 0, M), mesh, body, h)
    finalizer(x -> ccall((:pg_capacity_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), c)
    c
end
function Capacity(body::TaggedBody, mesh::Mesh{N}; method::String="VOFI", compute_centroids::Bool=true) where N
    init()
    kind, params, complement = _abi(body, Val(N))
    flags = Int32((complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_capacity_create_levelset, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Int32, Ptr{Ptr{Cvoid}}),
                mesh.handle, kind, params, length(params), flags, h))
    _wrap_capacity(h[], mesh, body, compute_centroids)
end
# Arbitrary Julia closures cannot run on the GPU.  Nothing is substituted: build the capacity with Penguin.jl itself
# (`Penguin.Capacity(body, penguin_mesh)`, the libvofi path) and hand its arrays over with capacity_from_arrays.
function Capacity(body::Function, mesh::Mesh{N}; kwargs...) where N
    error("PenguinHIP.Capacity: arbitrary level-set closures cannot run on the GPU; pass a Sphere / MultiSphere / " *
          "Ellipsoid / HalfSpace / Plane, wrap the closure in DeviceFunction (1-D and 2-D: it is traced and evaluated in the " *
          "kernels), or build the capacity with Penguin.Capacity and call PenguinHIP.capacity_from_arrays(cap, mesh)")
end
"""
    capacity_from_arrays(cap, mesh::Mesh{N})

`cap`: anything with Penguin.jl's Capacity fields (`A, B, W::NTuple{N}` of diagonal matrices, `V, Γ` diagonal matrices,
`C_ω, C_γ::Vector{SVector{N}}`, `cell_types`, `body`) -- typically a `Penguin.Capacity` computed by libvofi on a mesh with
the same `n, L, x0`.  The arrays are copied to the device (pg_capacity_create_from_arrays); single rank only.
"""
function capacity_from_arrays(cap, mesh::Mesh{N}) where N
    init()
    M = prod(mesh.dims .+ 1)
    dv(m) = Vector{Float64}(diag(m))
    V, Γ = dv(cap.V), dv(cap.Γ)
    A, B, W = [dv(cap.A[d]) for d in 1:N], [dv(cap.B[d]) for d in 1:N], [dv(cap.W[d]) for d in 1:N]
    Cω = [Float64[c[d] for c in cap.C_ω] for d in 1:N]
    has_cg = length(cap.C_γ) == M
    Cγ = has_cg ? [Float64[c[d] for c in cap.C_γ] for d in 1:N] : Vector{Float64}[]
    ct = Vector{Float64}(cap.cell_types)
    all(length(v) == M for v in (V, Γ, ct)) || error("capacity_from_arrays: the capacity does not live on this mesh")
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve V Γ A B W Cω Cγ ct begin
        pa, pb, pw, pcw = pointer.(A), pointer.(B), pointer.(W), pointer.(Cω)
        pcg = has_cg ? pointer.(Cγ) : Ptr{Float64}[]
        check(ccall((:pg_capacity_create_from_arrays, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64},
                     Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                    mesh.handle, V, pa, pb, pw, Γ, pcw, has_cg ? pcg : C_NULL, ct, h))
    end
    _wrap_capacity(h[], mesh, cap.body, has_cg)
end

# ---------------------------------------------------------------------------------- DiffusionOps (src/operators.jl:49-55)
abstract type AbstractOperators end
mutable struct DiffusionOps{N} <: AbstractOperators
    G::SparseMatrixCSC{Float64, Int}
    H::SparseMatrixCSC{Float64, Int}
    Wꜝ::SparseMatrixCSC{Float64, Int}
    V::SparseMatrixCSC{Float64, Int}
    size::NTuple{N, Int}
    handle::Ptr{Cvoid}
end
function _export_csc(h, which, nrows, ncols)
    nnz = Ref{Int64}(0)
    check(ccall((:pg_diffops_export_csc, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                h, which, C_NULL, C_NULL, C_NULL, nnz))
    colptr = Vector{Int64}(undef, ncols + 1); rowval = Vector{Int64}(undef, nnz[]); nzval = Vector{Float64}(undef, nnz[])
    check(ccall((:pg_diffops_export_csc, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                h, which, colptr, rowval, nzval, nnz))
    SparseMatrixCSC(nrows, ncols, colptr .+ 1, rowval .+ 1, nzval)
end
function DiffusionOps(cap::Capacity{N}) where N
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_diffops_create, libpg), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), cap.handle, h))
    sz = cap.mesh.dims .+ 1
    M = prod(sz)
    op = DiffusionOps{N}(_export_csc(h[], 0, N * M, M), _export_csc(h[], 1, N * M, M), _export_csc(h[], 2, N * M, N * M),
                         cap.V, sz, h[])
    finalizer(x -> ccall((:pg_diffops_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), op)
    op
end
function ∇(op::AbstractOperators, p::Vector{Float64})
    out = Vector{Float64}(undef, length(op.size) * prod(op.size))
    check(ccall((:pg_diffops_grad, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), op.handle, p, out))
    out
end
function ∇₋(op::AbstractOperators, qω::Vector{Float64}, qγ::Vector{Float64})
    out = Vector{Float64}(undef, prod(op.size))
    check(ccall((:pg_diffops_div, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), op.handle, qω, qγ, out))
    out
end

# ---------------------------------------------------------------------------------- boundary / phase (src/boundary.jl, src/phase.jl)
abstract type AbstractBoundary end
struct Dirichlet <: AbstractBoundary; value::Union{Function, Float64}; end
struct Neumann <: AbstractBoundary; value::Union{Function, Float64}; end
struct Robin <: AbstractBoundary; α::Union{Function, Float64}; β::Union{Function, Float64}; value::Union{Function, Float64}; end
struct Periodic <: AbstractBoundary end
abstract type AbstractInterfaceBC end
struct ScalarJump <: AbstractInterfaceBC; α₁::Float64; α₂::Float64; value::Union{Function, Float64}; end
struct FluxJump <: AbstractInterfaceBC; β₁::Float64; β₂::Float64; value::Union{Function, Float64}; end
struct BorderConditions; borders::Dict{Symbol, AbstractBoundary}; end
struct InterfaceConditions; scalar::ScalarJump; flux::FluxJump; end
struct Phase
    capacity::AbstractCapacity
    operator::AbstractOperators
    source::Function
    Diffusion_coeff::Function
end

# ---------------------------------------------------------------------------------- Solver (src/solver.jl:33-42)
const KEYS = Dict(:left => 0, :right => 1, :bottom => 2, :top => 3, :backward => 4, :forward => 5)   # src/solver.jl:379-409

mutable struct Solver
    time_type; phase_type; equation_type
    A; b
    x::Union{Vector{Float64}, Nothing}
    ch::Vector{Any}
    states::Vector{Any}
    handle::Ptr{Cvoid}
    nunk::Int
    # monitors=[...] of the last unsteady solve: rows x K values (row 1: the first solve), the solver's time of each row, the
    # monitors' names; state_steps: with save_every=k the step each entry of `states` belongs to ([0, k, 2k, ...])
    monitor_series::Matrix{Float64}
    monitor_times::Vector{Float64}
    monitor_names::Vector{String}
    state_steps::Union{Vector{Int}, Nothing}
end
function _new_solver(tt, pt, et, h::Ptr{Cvoid}, nunk::Int)
    s = Solver(tt, pt, et, nothing, nothing, nothing, [], [], h, nunk, zeros(0, 0), Float64[], String[], nothing)
    finalizer(x -> ccall((:pg_solver_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), s)
    s
end

# closures are evaluated on the host at the reference's points and times, exactly as it does:
# interface / source functions receive 3 padded coordinates (src/solver.jl:230-248), `try f(x..., t) catch f(x...)`
coords3(c) = length(c) == 1 ? (c[1], 0.0, 0.0) : length(c) == 2 ? (c[1], c[2], 0.0) : (c[1], c[2], c[3])
function _call_t(f, x, t)
    try
        return Float64(f(x..., t))
    catch e
        e isa MethodError || rethrow()
        return Float64(f(x...))
    end
end
evalf(f, C, t) = Float64[_call_t(f, coords3(c), t) for c in C]
evalf0(f, C) = Float64[Float64(f(coords3(c)...)) for c in C]                 # build_source / build_g_g without t

_bkind(v::AbstractBoundary) = v isa Dirichlet ? Int32(1) : v isa Neumann ? Int32(2) : v isa Robin ? Int32(3) : Int32(4)
_bvalue(v::AbstractBoundary) = (v isa Periodic || v.value isa Function) ? 0.0 : Float64(v.value)
# unknown keys (:front / :back of examples/3D/Diffusion/Heat.jl:26) are silently ignored, as the reference does
_border_descs(bc_b::BorderConditions) =
    pg_border_desc[pg_border_desc(Int32(KEYS[k]), _bkind(v), _bvalue(v)) for (k, v) in bc_b.borders if haskey(KEYS, k)]
_has_border_functions(bc_b::BorderConditions) =
    any(!(v isa Periodic) && v.value isa Function for (k, v) in bc_b.borders if haskey(KEYS, k))
# eval_bc_value at every border cell (src/solver.jl:441-448): value(pos..., t) with the N UNPADDED coordinates of
# mesh.centers, falling back to value(pos...); t === nothing: the diphasic drivers call BC_border_diph! without t
function _border_values(bc_b::BorderConditions, mesh::Mesh, t)
    inv = Dict(v => k for (k, v) in KEYS)
    vals = zeros(length(mesh.border_keys))
    for (q, (_, pos)) in enumerate(mesh.tag.border_cells)
        cond = get(bc_b.borders, inv[Int(mesh.border_keys[q])], nothing)
        (cond === nothing || cond isa Periodic) && continue
        v = cond.value
        vals[q] = v isa Function ? (t === nothing ? Float64(v(pos...)) : _call_t(v, pos, t)) : Float64(v)
    end
    vals
end
# Data handed over at every step of a host-driven loop: closures with a time parameter are re-evaluated every step, as the
# reference does, but what they returned is only sent when it differs from what the library already holds
# (`f = (x, y, z, t) -> 0.0`, the reference's own benchmark source, is time-dependent by its signature and constant by its
# values).  A step whose data did not change is a quiet step of the device loop (folded start, extrapolated start).
function _changed!(sent::Dict{Any,Any}, key, arrays...)
    old = get(sent, key, nothing)
    same = old !== nothing && length(old) == length(arrays) && all(isequal(a, b) for (a, b) in zip(old, arrays))
    sent[key] = map(copy, arrays)
    !same
end
function _set_border_values!(s::Solver, bc_b::BorderConditions, mesh::Mesh, t)
    vals = _border_values(bc_b, mesh, t)
    check(ccall((:pg_solver_set_border_values, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.handle, vals))
end
# Time-separable data Σ_k φ_k(x) a_k(t) (include/penguin_hip.h, DESIGN.md "Time-separable data"): the spatial parts once, then
# one table row per step and no per-step transfer.  which: PG_TD_SOURCE (phase 0 / 1), PG_TD_INTERFACE, PG_TD_BORDER.
# modes: M x K (padded fields at C_ω / C_γ) or nb x K (border values in the mesh's border order), one COLUMN per term;
# coef: K x 2 x nrows, coef[k, 1, q] = a_k at step q's "t", coef[k, 2, q] = a_k at its "t + Δt" (column-major: the C layout
# nrows x 2 x K).  Install after the first solve; every pg_solver_step / step of pg_solver_run consumes one row.
const PG_TD_SOURCE = Int32(0)
const PG_TD_INTERFACE = Int32(1)
const PG_TD_BORDER = Int32(2)
function set_separable!(s::Solver, which::Integer, phase::Integer, modes::Matrix{Float64}, coef::Array{Float64,3})
    K = size(modes, 2)
    (size(coef, 1) == K && size(coef, 2) == 2) || error("set_separable!: coef must be K x 2 x nrows with K = size(modes, 2)")
    check(ccall((:pg_solver_set_separable, libpg), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Int64, Ptr{Float64}),
                s.handle, which, phase, K, modes, size(coef, 3), coef))
end
clear_separable!(s::Solver, which::Integer, phase::Integer = 0) =
    check(ccall((:pg_solver_clear_separable, libpg), Int32, (Ptr{Cvoid}, Int32, Int32), s.handle, which, phase))
# (terms per slot: source of phase 0, source of phase 1, interface value, border values; table rows; the next step's row)
function time_data_info(s::Solver)
    terms = zeros(Int32, 4)
    nrows, cursor = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:pg_solver_time_data_info, libpg), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ref{Int64}, Ref{Int64}), s.handle, terms, nrows, cursor))
    (terms = Int.(terms), nrows = nrows[], cursor = cursor[])
end
# Device functions (include/penguin_hip.h, DESIGN.md "Device functions"): a scalar closure of (coordinates..., t) traced ONCE
# into a postfix program that a kernel evaluates every step at the reference's points.  DeviceFunction(f) calls f with Sym
# operands -- a Number type whose arithmetic, comparisons and elementary functions record themselves -- and keeps f: the object
# is callable and forwards to the ORIGINAL closure, so constructors and the host-driven loop use it as a plain closure.
# dev_select / dev_erf / dev_erfc / dev_atan2 work on Sym and on numbers alike.  What cannot be traced (a branch on a Sym, a
# function without an opcode, more than 96 instructions) is an error naming the operation: nothing falls back silently.
const PG_PROG_MAX_OPS = 96
const PG_PROG_MAX_CONST = 32
const PG_PROG_MAX_STACK = 16
const PG_OP_CONST = UInt8(0)
const PG_OP_VAR = UInt8(1)
const PG_OP_ADD = UInt8(2)
const PG_OP_SUB = UInt8(3)
const PG_OP_MUL = UInt8(4)
const PG_OP_DIV = UInt8(5)
const PG_OP_NEG = UInt8(6)
const PG_OP_ABS = UInt8(7)
const PG_OP_SQRT = UInt8(8)
const PG_OP_EXP = UInt8(9)
const PG_OP_LOG = UInt8(10)
const PG_OP_SIN = UInt8(11)
const PG_OP_COS = UInt8(12)
const PG_OP_TANH = UInt8(13)
const PG_OP_POW = UInt8(14)
const PG_OP_ATAN2 = UInt8(15)
const PG_OP_ERF = UInt8(16)
const PG_OP_ERFC = UInt8(17)
const PG_OP_MIN = UInt8(18)
const PG_OP_MAX = UInt8(19)
const PG_OP_LT = UInt8(20)
const PG_OP_LE = UInt8(21)
const PG_OP_GT = UInt8(22)
const PG_OP_GE = UInt8(23)
const PG_OP_SELECT = UInt8(24)
struct Sym <: Real
    op::UInt8
    args::Vector{Sym}
    value::Float64      # PG_OP_CONST: the constant; PG_OP_VAR: the index 0 .. 3
end
Sym(v::Real) = Sym(PG_OP_CONST, Sym[], Float64(v))
_symvar(i::Integer) = Sym(PG_OP_VAR, Sym[], Float64(i))
_sym(op::UInt8, args...) = Sym(op, Sym[a isa Sym ? a : Sym(a) for a in args], 0.0)
Base.promote_rule(::Type{Sym}, ::Type{<:Real}) = Sym
Base.convert(::Type{Sym}, v::Real) = Sym(v)
Base.convert(::Type{Sym}, v::Sym) = v
Base.:+(a::Sym, b::Sym) = _sym(PG_OP_ADD, a, b)
Base.:-(a::Sym, b::Sym) = _sym(PG_OP_SUB, a, b)
Base.:*(a::Sym, b::Sym) = _sym(PG_OP_MUL, a, b)
Base.:/(a::Sym, b::Sym) = _sym(PG_OP_DIV, a, b)
Base.:-(a::Sym) = _sym(PG_OP_NEG, a)
Base.:+(a::Sym) = a
Base.abs(a::Sym) = _sym(PG_OP_ABS, a)
Base.sqrt(a::Sym) = _sym(PG_OP_SQRT, a)
Base.exp(a::Sym) = _sym(PG_OP_EXP, a)
Base.log(a::Sym) = _sym(PG_OP_LOG, a)
Base.sin(a::Sym) = _sym(PG_OP_SIN, a)
Base.cos(a::Sym) = _sym(PG_OP_COS, a)
Base.tanh(a::Sym) = _sym(PG_OP_TANH, a)
Base.min(a::Sym, b::Sym) = _sym(PG_OP_MIN, a, b)
Base.max(a::Sym, b::Sym) = _sym(PG_OP_MAX, a, b)
Base.atan(a::Sym, b::Sym) = _sym(PG_OP_ATAN2, a, b)
Base.:^(a::Sym, b::Sym) = _sym(PG_OP_POW, a, b)
# x^k, k = 0 .. 4 an integer: multiplications; anything else: POW
function Base.:^(a::Sym, k::Integer)
    (0 <= k <= 4) || return _sym(PG_OP_POW, a, k)
    k == 0 && return Sym(1.0)
    out = a
    for _ in 2:k
        out = _sym(PG_OP_MUL, out, a)
    end
    out
end
# the comparisons give a Sym worth 1.0 / 0.0 -- not a Bool: `if x < y` on traced values fails in the `if`, by design
Base.:<(a::Sym, b::Sym) = _sym(PG_OP_LT, a, b)
Base.:<=(a::Sym, b::Sym) = _sym(PG_OP_LE, a, b)
Base.:<(a::Sym, b::Real) = _sym(PG_OP_LT, a, b)
Base.:<(a::Real, b::Sym) = _sym(PG_OP_LT, a, b)
Base.:<=(a::Sym, b::Real) = _sym(PG_OP_LE, a, b)
Base.:<=(a::Real, b::Sym) = _sym(PG_OP_LE, a, b)
dev_gt(a, b) = _sym(PG_OP_GT, a, b)
dev_ge(a, b) = _sym(PG_OP_GE, a, b)
_traced(args...) = any(a -> a isa Sym, args)
dev_select(c, a, b) = _traced(c, a, b) ? _sym(PG_OP_SELECT, c, a, b) : (c != 0 ? a : b)
dev_erf(x) = _traced(x) ? _sym(PG_OP_ERF, x) : error("dev_erf of a number: use SpecialFunctions.erf")
dev_erfc(x) = _traced(x) ? _sym(PG_OP_ERFC, x) : error("dev_erfc of a number: use SpecialFunctions.erfc")
dev_atan2(y, x) = _traced(y, x) ? _sym(PG_OP_ATAN2, y, x) : atan(y, x)
Base.Float64(::Sym) = error("DeviceFunction: cannot trace a conversion of a traced value to Float64 (a function without an opcode?)")
Base.Bool(::Sym) = error("DeviceFunction: cannot trace a branch on a traced value; use dev_select(cond, a, b), min or max")

# the bytes of a pg_program: n_ops::Int32, n_const::Int32, op[96]::UInt8, arg[96]::UInt8, konst[32]::Float64
const PG_PROGRAM_BYTES = 8 + 2 * PG_PROG_MAX_OPS + 8 * PG_PROG_MAX_CONST
function _compile_program(root::Sym)
    ops, args, consts = UInt8[], UInt8[], Float64[]
    deepest = Ref(0)
    function emit(node::Sym, depth::Int)            # operands left to right, then the operation; returns the depth after it
        if node.op == PG_OP_CONST
            k = findfirst(c -> reinterpret(UInt64, c) == reinterpret(UInt64, node.value), consts)
            if k === nothing
                length(consts) == PG_PROG_MAX_CONST && error("DeviceFunction: more than $PG_PROG_MAX_CONST distinct constants")
                push!(consts, node.value)
                k = length(consts)
            end
            push!(ops, PG_OP_CONST); push!(args, UInt8(k - 1))
            depth += 1
        elseif node.op == PG_OP_VAR
            push!(ops, PG_OP_VAR); push!(args, UInt8(node.value))
            depth += 1
        else
            d = depth
            for a in node.args
                d = emit(a, d)
            end
            push!(ops, node.op); push!(args, 0x00)
            depth += 1
        end
        length(ops) > PG_PROG_MAX_OPS && error("DeviceFunction: more than $PG_PROG_MAX_OPS instructions")
        deepest[] = max(deepest[], depth)
        depth
    end
    emit(root, 0)
    deepest[] > PG_PROG_MAX_STACK && error("DeviceFunction: an operand stack of $(deepest[]) values, more than $PG_PROG_MAX_STACK")
    buf = zeros(UInt8, PG_PROGRAM_BYTES)
    buf[1:4] .= reinterpret(UInt8, Int32[length(ops)])
    buf[5:8] .= reinterpret(UInt8, Int32[length(consts)])
    buf[9:8 + length(ops)] .= ops
    buf[9 + PG_PROG_MAX_OPS:8 + PG_PROG_MAX_OPS + length(args)] .= args
    kb = reinterpret(UInt8, consts)
    buf[9 + 2 * PG_PROG_MAX_OPS:8 + 2 * PG_PROG_MAX_OPS + length(kb)] .= kb
    check(ccall((:pg_program_validate, libpg), Int32, (Ptr{Cvoid},), buf))
    buf
end
struct DeviceFunction <: Function
    f::Function
    programs::Dict{Int,Vector{UInt8}}      # by the number of space coordinates the closure is called with
    # as a MOVING body f(x_1 .. x_N, t), by N: (phi, the N spatial derivative programs then d/dt, contiguous as the C arrays)
    moving::Dict{Int,Tuple{Vector{UInt8},Vector{UInt8}}}
end
DeviceFunction(f::Function) = DeviceFunction(f, Dict{Int,Vector{UInt8}}(), Dict{Int,Tuple{Vector{UInt8},Vector{UInt8}}}())
(df::DeviceFunction)(args...) = df.f(args...)
function program(df::DeviceFunction, nspace::Integer = 3)
    get!(df.programs, Int(nspace)) do
        out = df.f((_symvar(d) for d in 0:nspace - 1)..., _symvar(3))
        _compile_program(out isa Sym ? out : Sym(out))
    end
end
# the host interpreter of the library on the rows of xyz (3 x npts, one point per COLUMN: the C layout npts x 3)
function evaluate_program(df::DeviceFunction, xyz::Matrix{Float64}, t::Real; nspace::Integer = 3)
    size(xyz, 1) == 3 || error("evaluate_program: xyz must be 3 x npts")
    out = zeros(size(xyz, 2))
    check(ccall((:pg_program_eval_host, libpg), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Float64}),
                program(df, nspace), size(xyz, 2), xyz, t, out))
    out
end
# ---- DeviceFunction as the BODY of a Capacity (1-D, 2-D): the closure of the coordinates alone is traced, differentiated rule
# by rule (the twin of penguin/jl_amd/devfn.py `differentiate`) and evaluated inside the capacity kernels; fluid where it is <= 0
_isk(s::Sym) = s.op == PG_OP_CONST
_isk(s::Sym, v) = s.op == PG_OP_CONST && s.value == v
_dadd(a::Sym, b::Sym) = _isk(a) && _isk(b) ? Sym(a.value + b.value) : _isk(a, 0.0) ? b : _isk(b, 0.0) ? a : _sym(PG_OP_ADD, a, b)
_dneg(a::Sym) = _isk(a) ? Sym(-a.value) : a.op == PG_OP_NEG ? a.args[1] : _sym(PG_OP_NEG, a)
_dsub(a::Sym, b::Sym) = _isk(a) && _isk(b) ? Sym(a.value - b.value) : _isk(b, 0.0) ? a : _isk(a, 0.0) ? _dneg(b) : _sym(PG_OP_SUB, a, b)
function _dmul(a::Sym, b::Sym)
    _isk(a) && _isk(b) && return Sym(a.value * b.value)
    (_isk(a, 0.0) || _isk(b, 0.0)) && return Sym(0.0)
    _isk(a, 1.0) && return b
    _isk(b, 1.0) && return a
    _isk(a, -1.0) && return _dneg(b)
    _isk(b, -1.0) && return _dneg(a)
    _sym(PG_OP_MUL, a, b)
end
_ddiv(a::Sym, b::Sym) = _isk(a, 0.0) ? Sym(0.0) : _isk(b, 1.0) ? a : (_isk(a) && _isk(b) && b.value != 0.0) ? Sym(a.value / b.value) : _sym(PG_OP_DIV, a, b)
_dsel(c::Sym, a::Sym, b::Sym) = (_isk(a) && _isk(b) && a.value == b.value) ? a : _sym(PG_OP_SELECT, c, a, b)
function differentiate(node::Sym, var::Int)
    op, a = node.op, node.args
    op == PG_OP_CONST && return Sym(0.0)
    op == PG_OP_VAR && return Sym(Int(node.value) == var ? 1.0 : 0.0)
    op in (PG_OP_LT, PG_OP_LE, PG_OP_GT, PG_OP_GE) && return Sym(0.0)
    d = [differentiate(x, var) for x in a]
    op == PG_OP_SELECT && return _dsel(a[1], d[2], d[3])
    op == PG_OP_ADD && return _dadd(d[1], d[2])
    op == PG_OP_SUB && return _dsub(d[1], d[2])
    op == PG_OP_NEG && return _dneg(d[1])
    op == PG_OP_MUL && return _dadd(_dmul(d[1], a[2]), _dmul(a[1], d[2]))
    if op == PG_OP_DIV
        _isk(d[2], 0.0) && return _ddiv(d[1], a[2])
        return _ddiv(_dsub(_dmul(d[1], a[2]), _dmul(a[1], d[2])), _dmul(a[2], a[2]))
    end
    op == PG_OP_MIN && return _dsel(_sym(PG_OP_LE, a[1], a[2]), d[1], d[2])
    op == PG_OP_MAX && return _dsel(_sym(PG_OP_GE, a[1], a[2]), d[1], d[2])
    if op == PG_OP_POW
        if _isk(a[2])
            e = a[2].value
            return _dmul(_dmul(Sym(e), _sym(PG_OP_POW, a[1], Sym(e - 1.0))), d[1])
        end
        out = _dmul(_dmul(node, _sym(PG_OP_LOG, a[1])), d[2])
        _isk(d[1], 0.0) || (out = _dadd(out, _dmul(node, _ddiv(_dmul(a[2], d[1]), a[1]))))
        return out
    end
    op == PG_OP_ATAN2 && return _ddiv(_dsub(_dmul(a[2], d[1]), _dmul(a[1], d[2])), _dadd(_dmul(a[1], a[1]), _dmul(a[2], a[2])))
    u, du = a[1], d[1]
    _isk(du, 0.0) && return Sym(0.0)
    op == PG_OP_ABS && return _dsel(_sym(PG_OP_GE, u, Sym(0.0)), du, _dneg(du))
    op == PG_OP_SQRT && return _ddiv(du, _dmul(Sym(2.0), node))
    op == PG_OP_EXP && return _dmul(node, du)
    op == PG_OP_LOG && return _ddiv(du, u)
    op == PG_OP_SIN && return _dmul(_sym(PG_OP_COS, u), du)
    op == PG_OP_COS && return _dneg(_dmul(_sym(PG_OP_SIN, u), du))
    op == PG_OP_TANH && return _dmul(_dsub(Sym(1.0), _dmul(node, node)), du)
    if op == PG_OP_ERF || op == PG_OP_ERFC
        g = _dmul(Sym((op == PG_OP_ERF ? 2.0 : -2.0) / sqrt(pi)), _sym(PG_OP_EXP, _dneg(_dmul(u, u))))
        return _dmul(g, du)
    end
    error("DeviceFunction: no derivative rule for opcode $op")
end
function _body_trace(df::DeviceFunction, N::Integer)
    out = df.f((_symvar(d) for d in 0:N - 1)...)
    out isa Sym ? out : Sym(out)
end
body_program(df::DeviceFunction, N::Integer) = _compile_program(_body_trace(df, N))
function gradient_programs(df::DeviceFunction, N::Integer)
    root = _body_trace(df, N)
    out = Vector{Vector{UInt8}}()
    for d in 0:N - 1
        try
            push!(out, _compile_program(differentiate(root, d)))
        catch e
            error("DeviceFunction: the derivative along coordinate $d of the body $(df.f) does not fit: $(sprint(showerror, e))")
        end
    end
    out
end
# quadrature="height": the 3-D rule of a traced level set (csrc/pg_geom_program3.h, pg_capacity_create_program3), opt-in under its
# own name; without it a 3-D mesh keeps its refusal, and with it a 1-D or 2-D mesh is refused (they need no keyword)
function Capacity(body::DeviceFunction, mesh::Mesh{N}; method::String="VOFI", compute_centroids::Bool=true, complement::Bool=false,
                  quadrature::Union{Nothing, String}=nothing) where N
    if quadrature !== nothing
        quadrature == "height" || error("PenguinHIP.Capacity(quadrature=$(repr(quadrature))): the only rule to choose is \"height\", for a DeviceFunction body on a 3-D mesh")
        N == 3 || error("PenguinHIP.Capacity(quadrature=\"height\") is the rule of a 3-D mesh; this mesh is $N-D and needs no keyword")
    end
    N == 3 && quadrature === nothing &&
        error("PenguinHIP.Capacity(DeviceFunction): 3-D program bodies are not supported yet (1-D and 2-D) without quadrature=\"height\", the keyword that chooses the 3-D rule")
    init()
    phi = body_program(body, N)
    grad = reduce(vcat, gradient_programs(body, N))          # N programs, contiguous as the C array
    flags = Int32((complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if N == 3
        check(ccall((:pg_capacity_create_program3, libpg), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}),
                    mesh.handle, phi, grad, flags, h))
    else
        check(ccall((:pg_capacity_create_program, libpg), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}),
                    mesh.handle, phi, grad, flags, h))
    end
    _wrap_capacity(h[], mesh, body, compute_centroids)
end
# ---- FrontTracker (src/front_tracking.jl:5-266): a closed polyline of markers whose interior is the fluid.  Capacity(front, mesh)
# sends the markers to pg_capacity_create_polygon; the capacity kernels measure the polygon itself (csrc/pg_geom_polygon.h).
mutable struct FrontTracker <: Function      # (callable as its signed distance, negative inside: cap.body behaves like the other bodies)
    markers::Vector{Tuple{Float64, Float64}}
    is_closed::Bool
end
function _polygon(ft::FrontTracker)
    p = ft.markers
    length(p) >= 2 && p[1] == p[end] ? p[1:end-1] : p
end
"even-odd with the kernels' crossing rule: (p_y <= y) != (q_y <= y), the crossing at or left of x"
function is_point_inside(ft::FrontTracker, x::Real, y::Real)
    p = _polygon(ft)
    M = length(p)
    M < 3 && return false
    below = 0
    for k in 1:M
        (px, py), (qx, qy) = p[k], p[mod1(k + 1, M)]
        (py <= y) != (qy <= y) || continue
        c = clamp(px + (y - py) * (qx - px) / (qy - py), min(px, qx), max(px, qx))
        c <= x && (below += 1)
    end
    isodd(below)
end
function sdf(ft::FrontTracker, x::Real, y::Real)
    p = _polygon(ft)
    M = length(p)
    M < 3 && return Inf
    dist = Inf
    for k in 1:(ft.is_closed ? M : M - 1)
        (px, py), (qx, qy) = p[k], p[mod1(k + 1, M)]
        ex, ey = qx - px, qy - py
        ee = ex * ex + ey * ey
        t = ee > 0 ? clamp(((x - px) * ex + (y - py) * ey) / ee, 0.0, 1.0) : 0.0
        dist = min(dist, hypot(x - (px + t * ex), y - (py + t * ey)))
    end
    is_point_inside(ft, x, y) ? -dist : dist
end
(ft::FrontTracker)(x, y, _...) = sdf(ft, x, y)
FrontTracker() = FrontTracker(Tuple{Float64, Float64}[], true)
FrontTracker(markers::AbstractVector) = FrontTracker(convert(Vector{Tuple{Float64, Float64}}, markers), true)
get_markers(ft::FrontTracker) = ft.markers
function set_markers!(ft::FrontTracker, markers::AbstractVector, is_closed = nothing)
    ft.markers = convert(Vector{Tuple{Float64, Float64}}, markers)
    is_closed === nothing || (ft.is_closed = is_closed)
    ft
end
add_marker!(ft::FrontTracker, x::Real, y::Real) = (push!(ft.markers, (Float64(x), Float64(y))); ft)
function create_circle!(ft::FrontTracker, center_x::Real, center_y::Real, radius::Real, n_markers::Integer = 100)
    set_markers!(ft, [(center_x + radius * cos(2.0 * π * (i / n_markers)), center_y + radius * sin(2.0 * π * (i / n_markers)))
                      for i in 0:n_markers-1], true)
end
function create_ellipse!(ft::FrontTracker, center_x::Real, center_y::Real, radius_x::Real, radius_y::Real, n_markers::Integer = 100)
    theta = range(0, 2π, length = n_markers + 1)[1:end-1]
    set_markers!(ft, [(center_x + radius_x * cos(t), center_y + radius_y * sin(t)) for t in theta], true)
end
function create_crystal!(ft::FrontTracker, center_x::Real, center_y::Real, base_radius::Real, n_lobes::Integer = 6,
                         amplitude::Real = 0.2, n_markers::Integer = 100)
    markers = Vector{Tuple{Float64, Float64}}(undef, n_markers + 1)
    for i in 1:n_markers
        θ = 2.0 * π * (i - 1) / n_markers
        r = base_radius * (1.0 + amplitude * cos(n_lobes * θ))
        markers[i] = (center_x + r * cos(θ), center_y + r * sin(θ))
    end
    markers[n_markers + 1] = markers[1]
    set_markers!(ft, markers, true)
end
function Capacity(front::FrontTracker, mesh::Mesh{N}; method::String="VOFI", compute_centroids::Bool=true, complement::Bool=false) where N
    front.is_closed || error("PenguinHIP.Capacity(FrontTracker): is_closed=false is not supported (the reference substitutes the " *
                             "convex hull of the markers for an open front; close the front or pass the hull's markers)")
    pts = front.markers
    length(pts) >= 2 && pts[1] == pts[end] && (pts = pts[1:end-1])
    length(pts) >= 3 || error("PenguinHIP.Capacity(FrontTracker): a polygon needs at least 3 markers (got $(length(pts)))")
    N == 2 || error("PenguinHIP.Capacity(FrontTracker): a marker polygon is a 2-D body, the mesh is $(N)-D")
    init()
    xy = Float64[p[k] for p in pts for k in 1:2]              # x0 y0 x1 y1 ...
    flags = Int32((complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_capacity_create_polygon, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Ptr{Ptr{Cvoid}}),
                mesh.handle, xy, length(pts), flags, h))
    _wrap_capacity(h[], mesh, front, compute_centroids)
end
# times: 2 x nrows, times[1, q] = step q's "t", times[2, q] = its "t + Δt" (column-major: the C layout nrows x 2)
function set_program!(s::Solver, which::Integer, phase::Integer, df::DeviceFunction, times::Matrix{Float64}; nspace::Integer = 3)
    size(times, 1) == 2 || error("set_program!: times must be 2 x nrows")
    check(ccall((:pg_solver_set_program, libpg), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Int64, Ptr{Float64}),
                s.handle, which, phase, program(df, nspace), size(times, 2), times))
end
function set_border_program!(s::Solver, key::Integer, df::DeviceFunction, times::Matrix{Float64}, nspace::Integer)
    size(times, 1) == 2 || error("set_border_program!: times must be 2 x nrows")
    check(ccall((:pg_solver_set_border_program, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Float64}),
                s.handle, key, program(df, nspace), size(times, 2), times))
end
# (programs and listed rows per slot; table rows over separable and program slots together; the next step's row)
function program_info(s::Solver)
    programs, entries = zeros(Int32, 4), zeros(Int64, 4)
    nrows, cursor = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:pg_solver_program_info, libpg), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ref{Int64}, Ref{Int64}),
                s.handle, programs, entries, nrows, cursor))
    (programs = Int.(programs), entries = Int.(entries), nrows = nrows[], cursor = cursor[])
end
# Monitors (include/penguin_hip.h, DESIGN.md "Monitors"): observables Σ w_i x_i (:sum) / Σ w_i x_i² (:sumsq) of the state,
# evaluated on the device after every solve -- what the reference's scripts compute by looping over solver.states
# (examples/2D/Diffusion/Heat_2ph.jl: volume-weighted phase means; the Stefan and species solvers: the interface flux).
# `weights(nunk)` gives the nunk = 2M / 4M weights in the layout of solver.x.
const PG_MON_SUM = Int32(0)
const PG_MON_SUMSQ = Int32(1)
const PG_MON_MAX = 8
struct Monitor
    weights::Function
    kind::Int32
    name::String
end
_mon_kind(kind::Symbol) = kind == :sum ? PG_MON_SUM : kind == :sumsq ? PG_MON_SUMSQ : error("unknown monitor kind $kind: :sum or :sumsq")
Monitor(w::Vector{Float64}; kind::Symbol=:sum, name::String="monitor") = Monitor(nunk -> w, _mon_kind(kind), name)
# start (0-based) of block (phase, kind) in [Tω, Tγ] (2M) or [T1ω, T1γ, T2ω, T2γ] (4M); phase is 0 or 1 as in the C ABI
function _block_offset(M::Int, nunk::Int, phase::Int, kind::Symbol)
    kind in (:omega, :gamma, :ω, :γ) || error("kind must be :omega or :gamma")
    (nunk == 2M || nunk == 4M) || error("a solver on this mesh has 2*$M or 4*$M unknowns, not $nunk")
    (phase == 0 || (phase == 1 && nunk == 4M)) || error("phase $phase: no such phase in this solver")
    (2 * phase + (kind in (:gamma, :γ) ? 1 : 0)) * M
end
# Σ V_i T_i over the ω unknowns of one phase, divided by Σ V when `mean` (c̄ of Heat_2ph.jl); `square`: of T_i²
function VolumeIntegral(capacity::AbstractCapacity; phase::Int=0, mean::Bool=true, square::Bool=false, name::String="volume_$phase")
    V = Vector{Float64}(diag(capacity.V))
    M = length(V)
    Monitor(square ? PG_MON_SUMSQ : PG_MON_SUM, name) do nunk
        w = zeros(nunk)
        off = _block_offset(M, nunk, phase, :omega)
        w[off+1:off+M] .= mean ? V ./ sum(V) : V
        w
    end
end
# Σ_i [Id (Hᵀ Wꜝ G Tω + Hᵀ Wꜝ H Tγ)]_i with d = D(C_ω), q = Wꜝ H d = ∇(op, (0, d)):  w_γ = ∇₋(op, 0, q) = Hᵀq,
# w_ω = -∇₋(op, q, 0) - w_γ = Gᵀq
function InterfaceFlux(ph::Phase; phase::Int=0, name::String="interface_flux_$phase")
    Monitor(PG_MON_SUM, name) do nunk
        op = ph.operator
        M = prod(op.size)
        d = evalf0(ph.Diffusion_coeff, ph.capacity.C_ω)
        q = ∇(op, vcat(zeros(M), d))
        wγ = ∇₋(op, zeros(length(q)), q)
        wω = -∇₋(op, q, zeros(length(q))) .- wγ
        w = zeros(nunk)
        ow, og = _block_offset(M, nunk, phase, :omega), _block_offset(M, nunk, phase, :gamma)
        w[ow+1:ow+M] .= wω
        w[og+1:og+M] .= wγ
        w
    end
end
# unit weight on one unknown: `index` a 1-based CartesianIndex / tuple of the cell, or a point (tuple of Float64) -- the cell
# whose node interval holds it
function Probe(mesh::Mesh{N}, point_or_index; kind::Symbol=:omega, phase::Int=0, name::String="probe") where N
    ext = mesh.dims .+ 1
    idx = if point_or_index isa CartesianIndex
        Tuple(point_or_index)
    elseif all(v -> v isa Integer, point_or_index)
        Tuple(Int.(collect(point_or_index)))
    else
        ntuple(d -> clamp(searchsortedlast(mesh.nodes[d], Float64(point_or_index[d])), 1, mesh.dims[d]), N)
    end
    all(1 .<= idx .<= ext) || error("cell $idx is outside the $ext cells of the mesh")
    lin = LinearIndices(ext)[idx...]
    M = prod(ext)
    Monitor(PG_MON_SUM, name) do nunk
        w = zeros(nunk)
        w[_block_offset(M, nunk, phase, kind) + lin] = 1.0
        w
    end
end
function set_monitors!(s::Solver, mons::Vector{Monitor})
    1 <= length(mons) <= PG_MON_MAX || error("1 .. $PG_MON_MAX monitors per solver, not $(length(mons))")
    W = zeros(s.nunk, length(mons))                  # one COLUMN per monitor: the C layout K x len
    for (k, m) in enumerate(mons)
        w = m.weights(s.nunk)
        length(w) == s.nunk || error("monitor weights must have the length of solver.x, $(s.nunk), not $(length(w))")
        W[:, k] .= w
    end
    kinds = Int32[m.kind for m in mons]
    check(ccall((:pg_solver_set_monitors, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Int64),
                s.handle, length(mons), kinds, W, s.nunk))
    s.monitor_names = String[m.name for m in mons]
    s.monitor_series, s.monitor_times = zeros(0, length(mons)), Float64[]
    nothing
end
function clear_monitors!(s::Solver)
    check(ccall((:pg_solver_clear_monitors, libpg), Int32, (Ptr{Cvoid},), s.handle))
    s.monitor_names, s.monitor_series, s.monitor_times = String[], zeros(0, 0), Float64[]
    nothing
end
# (K, rows of the series, per monitor: stored as a (row, weight) list?, entries stored)
function monitor_info(s::Solver)
    K, rows = Ref{Int32}(0), Ref{Int64}(0)
    sparse, stored = zeros(Int32, PG_MON_MAX), zeros(Int64, PG_MON_MAX)
    check(ccall((:pg_solver_monitor_info, libpg), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ptr{Int32}, Ptr{Int64}),
                s.handle, K, rows, sparse, stored))
    (K = Int(K[]), rows = Int(rows[]), sparse = Bool.(sparse[1:K[]]), stored = Int.(stored[1:K[]]))
end
# the whole series: (rows x K values, the solver's time of each row)
function monitor_series(s::Solver)
    info = monitor_info(s)
    vals, times = zeros(info.K, info.rows), zeros(info.rows)       # column q = row q of the C layout rows x K
    info.K > 0 && info.rows > 0 &&
        check(ccall((:pg_solver_get_monitor_series, libpg), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                    s.handle, 0, info.rows, vals, times))
    (Matrix(vals'), times)
end
drop_states!(s::Solver) = check(ccall((:pg_solver_drop_states, libpg), Int32, (Ptr{Cvoid},), s.handle))
function _kept_state(s::Solver, q::Integer)
    x = zeros(s.nunk)
    check(ccall((:pg_solver_get_state, libpg), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), s.handle, q, x, s.nunk))
    x
end
# monitors= / save_every= of the unsteady drivers: argument errors first, then this call's monitors (or none)
function _begin_monitors!(s::Solver, monitors, save_every, log)
    mons = monitors === nothing ? Monitor[] : Vector{Monitor}(monitors)
    length(mons) <= PG_MON_MAX || error("at most $PG_MON_MAX monitors per solver, not $(length(mons))")
    if save_every !== nothing
        (save_every isa Integer && save_every >= 1) || error("save_every must be an integer >= 1")
        log && error("save_every keeps the time loop on the device; log needs the per-step branch")
    end
    if !isempty(mons)
        set_monitors!(s, mons)
    elseif !isempty(s.monitor_names)
        clear_monitors!(s)
    end
    s.state_steps = save_every === nothing ? nothing : Int[0]
    save_every === nothing || empty!(s.states)        # states and state_steps describe THIS call, entry for entry
    nothing
end
function _end_monitors!(s::Solver)
    isempty(s.monitor_names) && return nothing
    s.monitor_series, s.monitor_times = monitor_series(s)
    nothing
end
# after pg_solver_run with save_every = k: the kept states (steps k, 2k, ...) follow the first solve's, the device copies go
function _fetch_kept_states!(s::Solver, k::Integer)
    n = Ref{Int64}(0)
    check(ccall((:pg_solver_num_states, libpg), Int32, (Ptr{Cvoid}, Ref{Int64}), s.handle, n))
    for q in 0:n[]-1
        push!(s.states, _kept_state(s, q))
        push!(s.state_steps, (q + 1) * k)
    end
    drop_states!(s)
end
function _interface_desc(bc_i::AbstractBoundary, g::Vector{Float64})
    kind = bc_i isa Dirichlet ? Int32(1) : bc_i isa Neumann ? Int32(2) : bc_i isa Robin ? Int32(3) :
           error("unsupported interface condition $(typeof(bc_i))")
    if bc_i isa Robin && (bc_i.α isa Function || bc_i.β isa Function)
        error("PenguinHIP: function-valued Robin coefficients are not supported on the GPU path")
    end
    α, β = bc_i isa Robin ? (Float64(bc_i.α), Float64(bc_i.β)) : (0.0, 0.0)
    pg_bc_desc(kind, α, β, bc_i.value isa Function ? 0.0 : Float64(bc_i.value), isempty(g) ? Ptr{Float64}(C_NULL) : pointer(g))
end
function _state(s::Solver)
    x = zeros(s.nunk)
    check(ccall((:pg_solver_get_state, libpg), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), s.handle, -1, x, s.nunk))
    x
end
function _record!(s::Solver, info::pg_step_info, log::Bool)
    info.converged == 0 && @warn "PenguinHIP: a solve did not converge" iters = info.iters relres = info.resnorm / max(info.bnorm, floatmin())
    log && push!(s.ch, (iters = info.iters, resnorm = info.resnorm, isconverged = info.converged != 0))
    s.x = _state(s)
    push!(s.states, s.x)
    nothing
end
_scheme(s::String) = s == "CN" ? Int32(1) : Int32(0)          # diffusion.jl:200-206: anything but "CN" is BE

# ---------------------------------------------------------------------------------- DiffusionUnsteadyMono (diffusion.jl:192-210)
function DiffusionUnsteadyMono(phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary, Δt::Float64, Tᵢ::Vector{Float64}, scheme::String)
    println("Solver creation:"); println("- Monophasic problem"); println("- Unsteady problem"); println("- Diffusion problem")
    cap = phase.capacity
    g = bc_i.value isa Function ? evalf(bc_i.value, cap.C_γ, Δt) : Float64[]      # b(t=0) uses g(0+Δt)   diffusion.jl:249
    D = evalf0(phase.Diffusion_coeff, cap.C_ω)
    f = evalf(phase.source, cap.C_ω, Δt)                                          # f(0+Δt)
    borders = _border_descs(bc_b)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g D f Tᵢ borders begin
        desc = Ref(_interface_desc(bc_i, g))
        check(ccall((:pg_solver_create_unsteady_mono, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_bc_desc}, Ptr{pg_border_desc}, Int32, Ptr{Float64}, Ptr{Float64}, Float64,
                     Ptr{Float64}, Int32, Ptr{Ptr{Cvoid}}),
                    cap.handle, phase.operator.handle, desc, borders, length(borders), D, f, Δt, Tᵢ, _scheme(scheme), h))
    end
    s = _new_solver(:Unsteady, :Monophasic, :Diffusion, h[], length(Tᵢ))
    if scheme == "CN"                                   # the CN right-hand side also needs f(0) and g(0)
        f0 = evalf(phase.source, cap.C_ω, 0.0)
        check(ccall((:pg_solver_set_source, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, 0, f0, C_NULL))
        if bc_i.value isa Function
            g0 = evalf(bc_i.value, cap.C_γ, 0.0)
            check(ccall((:pg_solver_set_interface_value, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, g0, C_NULL))
        end
    end
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, cap.mesh, 0.0)    # ctor applies borders with t = 0  (:207)
    s
end

# solve_DiffusionUnsteadyMono!(s, phase, Δt, Tₑ, bc_b, bc, scheme; method=gmres, algorithm=nothing, kwargs...)  diffusion.jl:268-301
# Extra keywords (not in the reference): `save_states=true`; with `save_states=false` and no function-valued data the
# whole loop runs on the device (pg_solver_run) and only the last state is fetched.  `monitors=[...]`: observables evaluated on
# the device after every solve, in whichever branch runs (s.monitor_series, s.monitor_times, s.monitor_names).  `save_every=k`:
# the device loop (same conditions on the data) keeps every k-th state; s.states holds the first solve's state and those,
# s.state_steps = [0, k, 2k, ...].
function solve_DiffusionUnsteadyMono!(s::Solver, phase::Phase, Δt::Float64, Tₑ, bc_b::BorderConditions, bc::AbstractBoundary, scheme::String;
                                      method::Function=gmres, algorithm=nothing, save_states::Bool=true, monitors=nothing,
                                      save_every=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    _begin_monitors!(s, monitors, save_every, log)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    cap, mesh = phase.capacity, phase.capacity.mesh
    t = 0.0
    check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
    _record!(s, info, log)                                                        # states[1]   (:275-277)
    println("Time: ", t); println("Solver Extremum: ", info.extremum)
    if (!save_states || save_every !== nothing) && !(bc.value isa Function) && !_has_border_functions(bc_b) && get(kw, :constant_source, false)
        run = pg_run_info()
        check(ccall((:pg_solver_run, libpg), Int32, (Ptr{Cvoid}, Float64, Int32, Ptr{pg_krylov_opts}, Int32, Int64, Int32, Ref{pg_run_info}),
                    s.handle, Float64(Tₑ), _scheme(scheme), opts, 0, -1, save_every === nothing ? 0 : save_every, run))
        run.unconverged_steps == 0 || @warn "PenguinHIP: $(run.unconverged_steps) of $(run.steps) time-step solves did not converge"
        s.x = _state(s)
        if save_every === nothing
            s.states[end] = s.x
        else
            _fetch_kept_states!(s, save_every)
        end
        _end_monitors!(s)
        return s
    end
    steps = 0
    sent = Dict{Any,Any}()
    while t < Tₑ
        t += Δt                                                                    # :287
        println("Time: ", t)
        fn, fn1 = evalf(phase.source, cap.C_ω, t), evalf(phase.source, cap.C_ω, t + Δt)    # f(t+Δt), t already advanced (:248)
        _changed!(sent, :f, fn, fn1) &&
            check(ccall((:pg_solver_set_source, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, 0, fn, fn1))
        if bc.value isa Function
            gn, gn1 = evalf(bc.value, cap.C_γ, t), evalf(bc.value, cap.C_γ, t + Δt)
            _changed!(sent, :g, gn, gn1) &&
                check(ccall((:pg_solver_set_interface_value, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, gn, gn1))
        end
        if _has_border_functions(bc_b)                                            # BC_border_mono!(...; t=t)   (:292)
            bv = _border_values(bc_b, mesh, t)
            _changed!(sent, :b, bv) &&
                check(ccall((:pg_solver_set_border_values, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.handle, bv))
        end
        check(ccall((:pg_solver_step, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, _scheme(scheme), opts, info))
        _record!(s, info, log)
        steps += 1
        _thin_states!(s, save_every, steps)
        println("Solver Extremum: ", info.extremum)
    end
    _end_monitors!(s)
    s
end
# the host-driven loop under save_every = k: the state of a step that is no multiple of k does not stay in s.states
function _thin_states!(s::Solver, save_every, steps::Int)
    save_every === nothing && return nothing
    steps % save_every == 0 ? push!(s.state_steps, steps) : pop!(s.states)
    nothing
end

# ---------------------------------------------------------------------------------- DiffusionUnsteadyDiph (diffusion.jl:319-454)
function _jump_desc(ic::InterfaceConditions, cap1, cap2, g::Vector{Float64}, hh::Vector{Float64})
    pg_jump_desc(ic.scalar.α₁, ic.scalar.α₂, ic.scalar.value isa Function ? 0.0 : Float64(ic.scalar.value),
                 ic.flux.β₁, ic.flux.β₂, ic.flux.value isa Function ? 0.0 : Float64(ic.flux.value),
                 isempty(g) ? Ptr{Float64}(C_NULL) : pointer(g), isempty(hh) ? Ptr{Float64}(C_NULL) : pointer(hh))
end
function DiffusionUnsteadyDiph(phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64, Tᵢ::Vector{Float64}, scheme::String)
    println("Solver creation:"); println("- Diphasic problem"); println("- Unsteady problem"); println("- Diffusion problem")
    c1, c2 = phase1.capacity, phase2.capacity
    g = ic.scalar.value isa Function ? evalf0(ic.scalar.value, c1.C_γ) : Float64[]       # g, h are built WITHOUT t (:397)
    hh = ic.flux.value isa Function ? evalf0(ic.flux.value, c2.C_γ) : Float64[]
    D1, D2 = evalf0(phase1.Diffusion_coeff, c1.C_ω), evalf0(phase2.Diffusion_coeff, c2.C_ω)
    f1, f2 = evalf(phase1.source, c1.C_ω, Δt), evalf(phase2.source, c2.C_ω, Δt)
    borders = _border_descs(bc_b)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g hh D1 D2 f1 f2 Tᵢ borders begin
        desc = Ref(_jump_desc(ic, c1, c2, g, hh))
        check(ccall((:pg_solver_create_unsteady_diph, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_jump_desc}, Ptr{pg_border_desc}, Int32,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Int32, Ptr{Ptr{Cvoid}}),
                    c1.handle, phase1.operator.handle, c2.handle, phase2.operator.handle, desc, borders, length(borders),
                    D1, D2, f1, f2, Δt, Tᵢ, _scheme(scheme), h))
    end
    s = _new_solver(:Unsteady, :Diphasic, :Diffusion, h[], length(Tᵢ))
    if scheme == "CN"
        for (q, ph) in enumerate((phase1, phase2))
            f0 = evalf(ph.source, ph.capacity.C_ω, 0.0)
            check(ccall((:pg_solver_set_source, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, q - 1, f0, C_NULL))
        end
    end
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, c1.mesh, nothing)   # BC_border_diph! is called without t (:330)
    s
end

function solve_DiffusionUnsteadyDiph!(s::Solver, phase1::Phase, phase2::Phase, Δt::Float64, Tₑ, bc_b::BorderConditions, ic::InterfaceConditions, scheme::String;
                                      method::Function=gmres, algorithm=nothing, monitors=nothing, save_every=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    _begin_monitors!(s, monitors, save_every, log)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    t = 0.0
    println("Time: ", t)
    check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
    _record!(s, info, log)
    println("Solver Extremum: ", info.extremum)
    if save_every !== nothing && get(kw, :constant_source, false)       # (monitors=, save_every=: as the monophasic driver)
        run = pg_run_info()
        check(ccall((:pg_solver_run, libpg), Int32, (Ptr{Cvoid}, Float64, Int32, Ptr{pg_krylov_opts}, Int32, Int64, Int32, Ref{pg_run_info}),
                    s.handle, Float64(Tₑ), _scheme(scheme), opts, 0, -1, save_every, run))
        run.unconverged_steps == 0 || @warn "PenguinHIP: $(run.unconverged_steps) of $(run.steps) time-step solves did not converge"
        s.x = _state(s)
        _fetch_kept_states!(s, save_every)
        _end_monitors!(s)
        return s
    end
    sent = Dict{Any,Any}()
    steps = 0
    while t < Tₑ
        t += Δt
        println("Time: ", t)
        for (q, ph) in enumerate((phase1, phase2))                                 # f(t+Δt) and, for CN, f(t)   (:401-421)
            fn, fn1 = evalf(ph.source, ph.capacity.C_ω, t), evalf(ph.source, ph.capacity.C_ω, t + Δt)
            _changed!(sent, (:f, q), fn, fn1) &&
                check(ccall((:pg_solver_set_source, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, q - 1, fn, fn1))
        end
        check(ccall((:pg_solver_step, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, _scheme(scheme), opts, info))
        _record!(s, info, log)
        steps += 1
        _thin_states!(s, save_every, steps)
        println("Solver Extremum: ", info.extremum)
    end
    _end_monitors!(s)
    s
end

# ---------------------------------------------------------------------------------- steady diffusion (diffusion.jl:14-175)
function DiffusionSteadyMono(phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary)
    println("Solver creation:"); println("- Monophasic problem"); println("- Steady problem"); println("- Diffusion problem")
    cap = phase.capacity
    g = bc_i.value isa Function ? evalf0(bc_i.value, cap.C_γ) : Float64[]
    D = evalf0(phase.Diffusion_coeff, cap.C_ω)
    f = evalf0(phase.source, cap.C_ω)
    borders = _border_descs(bc_b)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g D f borders begin
        desc = Ref(_interface_desc(bc_i, g))
        check(ccall((:pg_solver_create_steady_mono, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_bc_desc}, Ptr{pg_border_desc}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                    cap.handle, phase.operator.handle, desc, borders, length(borders), D, f, h))
    end
    s = _new_solver(:Steady, :Monophasic, :Diffusion, h[], 2 * length(cap.C_ω))
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, cap.mesh, nothing)
    s
end
function DiffusionSteadyDiph(phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions)
    println("Solver creation:"); println("- Diphasic problem"); println("- Steady problem"); println("- Diffusion problem")
    c1, c2 = phase1.capacity, phase2.capacity
    g = ic.scalar.value isa Function ? evalf0(ic.scalar.value, c1.C_γ) : Float64[]
    hh = ic.flux.value isa Function ? evalf0(ic.flux.value, c2.C_γ) : Float64[]
    D1, D2 = evalf0(phase1.Diffusion_coeff, c1.C_ω), evalf0(phase2.Diffusion_coeff, c2.C_ω)
    f1, f2 = evalf0(phase1.source, c1.C_ω), evalf0(phase2.source, c2.C_ω)
    borders = _border_descs(bc_b)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g hh D1 D2 f1 f2 borders begin
        desc = Ref(_jump_desc(ic, c1, c2, g, hh))
        check(ccall((:pg_solver_create_steady_diph, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_jump_desc}, Ptr{pg_border_desc}, Int32,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                    c1.handle, phase1.operator.handle, c2.handle, phase2.operator.handle, desc, borders, length(borders),
                    D1, D2, f1, f2, h))
    end
    s = _new_solver(:Steady, :Diphasic, :Diffusion, h[], 4 * length(c1.C_ω))
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, c1.mesh, nothing)
    s
end
function _solve_steady!(s::Solver, method, kwargs, banner)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    println("Solving the system:"); println(banner); println("- Steady problem"); println("- Diffusion problem")
    kw = Dict{Symbol, Any}(kwargs)
    opts = Ref(_opts(method, kw; warm_default=false))
    info = pg_step_info()
    check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
    info.converged == 0 && @warn "PenguinHIP: the steady solve did not converge" iters = info.iters
    get(kw, :log, false) && push!(s.ch, (iters = info.iters, resnorm = info.resnorm, isconverged = info.converged != 0))
    s.x = _state(s)
    s
end
solve_DiffusionSteadyMono!(s::Solver; method::Function=gmres, algorithm=nothing, kwargs...) =
    _solve_steady!(s, method, kwargs, "- Monophasic problem")
solve_DiffusionSteadyDiph!(s::Solver; method::Function=gmres, algorithm=nothing, kwargs...) =
    _solve_steady!(s, method, kwargs, "- Diphasic problem")

# ---------------------------------------------------------------------------------- ConvectionOps + advection-diffusion
# src/operators.jl:194-210: C_d = δ_p[d] diag(Σ_m[d] A_d uₒ_d) Σ_m[d], K_d = diag(Σ_p[d] Hᵀuᵧ).  A solver built from such an
# operator assembles the advection-diffusion blocks (src/solver/advectiondiffusion.jl:29-44,95-126,180-213): the diffusion
# constructors and loops above, called with this operator.
mutable struct ConvectionOps{N} <: AbstractOperators
    C::NTuple{N, SparseMatrixCSC{Float64, Int}}
    K::NTuple{N, SparseMatrixCSC{Float64, Int}}
    G::SparseMatrixCSC{Float64, Int}
    H::SparseMatrixCSC{Float64, Int}
    Wꜝ::SparseMatrixCSC{Float64, Int}
    V::SparseMatrixCSC{Float64, Int}
    size::NTuple{N, Int}
    handle::Ptr{Cvoid}
end
function ConvectionOps(capacity::Capacity{N}, uₒ::NTuple{N, Vector{Float64}}, uᵧ::Vector{Float64}) where N
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_diffops_create, libpg), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), capacity.handle, h))
    sz = capacity.mesh.dims .+ 1
    M = prod(sz)
    GC.@preserve uₒ uᵧ begin
        ptrs = [pointer(u) for u in uₒ]
        check(ccall((:pg_diffops_set_velocity, libpg), Int32, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Float64}), h[], ptrs, uᵧ))
    end
    op = ConvectionOps{N}(ntuple(d -> _export_csc(h[], 3 + d - 1, M, M), N), ntuple(d -> _export_csc(h[], 6 + d - 1, M, M), N),
                          _export_csc(h[], 0, N * M, M), _export_csc(h[], 1, N * M, M), _export_csc(h[], 2, N * M, N * M),
                          capacity.V, sz, h[])
    finalizer(x -> ccall((:pg_diffops_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), op)
    op
end
_adv(s::Solver) = (s.equation_type = :DiffusionAdvection; s)
_need_conv(ph::Phase) = ph.operator isa ConvectionOps || error("the advection-diffusion drivers need a Phase built on ConvectionOps")
AdvectionDiffusionSteadyMono(phase::Phase, bc_b, bc_i) = (_need_conv(phase); _adv(DiffusionSteadyMono(phase, bc_b, bc_i)))
solve_AdvectionDiffusionSteadyMono!(s::Solver; kwargs...) = solve_DiffusionSteadyMono!(s; kwargs...)
AdvectionDiffusionSteadyDiph(p1::Phase, p2::Phase, bc_b, ic) = (_need_conv(p1); _need_conv(p2); _adv(DiffusionSteadyDiph(p1, p2, bc_b, ic)))
solve_AdvectionDiffusionSteadyDiph!(s::Solver; kwargs...) = solve_DiffusionSteadyDiph!(s; kwargs...)
function AdvectionDiffusionUnsteadyMono(phase::Phase, bc_b, bc_i, Δt::Float64, Tᵢ::Vector{Float64}, scheme::String)
    _need_conv(phase)
    scheme in ("BE", "CN") || error("Unknown scheme.")                              # advectiondiffusion.jl:203-205
    _adv(DiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme))
end
solve_AdvectionDiffusionUnsteadyMono!(s::Solver, phase::Phase, Δt::Float64, Tₑ, bc_b, bc, scheme::String; kwargs...) =
    solve_DiffusionUnsteadyMono!(s, phase, Δt, Tₑ, bc_b, bc, scheme; kwargs...)
# Backward Euler only: the reference's Crank-Nicolson right-hand side for the diphasic driver keeps the convection terms but
# drops the diffusion part of the explicit half step (advectiondiffusion.jl:375-377); it is refused, not approximated.
function AdvectionDiffusionUnsteadyDiph(p1::Phase, p2::Phase, bc_b, ic, Δt::Float64, Tᵢ::Vector{Float64}, scheme::String)
    _need_conv(p1); _need_conv(p2)
    scheme == "BE" || error("AdvectionDiffusionUnsteadyDiph: only scheme \"BE\" is available on the HIP path")
    _adv(DiffusionUnsteadyDiph(p1, p2, bc_b, ic, Δt, Tᵢ, "BE"))
end
function solve_AdvectionDiffusionUnsteadyDiph!(s::Solver, p1::Phase, p2::Phase, Δt::Float64, Tₑ, bc_b, ic, scheme::String; kwargs...)
    scheme == "BE" || error("solve_AdvectionDiffusionUnsteadyDiph!: only scheme \"BE\" is available on the HIP path")
    solve_DiffusionUnsteadyDiph!(s, p1, p2, Δt, Tₑ, bc_b, ic, "BE"; kwargs...)
end

# ---------------------------------------------------------------------------------- prescribed motion (prescribedmotionsolver/diffusion.jl)
# SpaceTimeMesh (src/mesh.jl:129-146), Capacity(body, STmesh), MovingDiffusionUnsteadyMono (:16-35) and
# solve_MovingDiffusionUnsteadyMono! (:227-268).  The moving level set is a tagged body whose parameters are functions of
# time; every slab's capacity is built on the GPU (pg_capacity_create_spacetime: exact in space, composite Gauss-Legendre
# in time) and the moving blocks are assembled there (pg_solver_create_moving_mono).  1-D and 2-D in space.
struct SpaceTimeMesh{M} <: AbstractMesh
    nodes::NTuple{M, Vector{Float64}}
    centers::NTuple{M, Vector{Float64}}
    tag
    dims::NTuple{M, Int}
    space::Mesh
end
function SpaceTimeMesh(spaceMesh::Mesh{N}, time::Vector{Float64}; tag=spaceMesh.tag) where N
    length(time) == 2 || error("SpaceTimeMesh: one time cell [t, t+Δt]")
    nodes = ntuple(i -> i <= N ? spaceMesh.nodes[i] : time, N + 1)
    centers = ntuple(i -> i <= N ? spaceMesh.centers[i] : [(time[1] + time[2]) / 2], N + 1)
    SpaceTimeMesh{N + 1}(nodes, centers, tag, ntuple(i -> length(centers[i]), N + 1), spaceMesh)
end
nC(m::SpaceTimeMesh) = prod(m.dims)

abstract type MovingBody <: Function end
"f(x, t) = |x - center(t)| - radius(t)  (complement: -f, the growing disc of examples/2D/SolidMoving/MovingHeat.jl:19)"
struct MovingSphere <: MovingBody
    center::Function; radius::Function; complement::Bool
end
MovingSphere(center, radius; complement::Bool=false) = MovingSphere(center, radius, complement)
"f(x, t) = sign (x_axis - position(t))  (examples/1D/SolidMoving/MovingHeat.jl:18); axis is 1-based as everywhere in Julia"
struct MovingHalfSpace <: MovingBody
    axis::Int; position::Function; sign::Float64; complement::Bool
end
MovingHalfSpace(axis, position; sign::Float64=1.0, complement::Bool=false) = MovingHalfSpace(axis, position, sign, complement)
function (b::MovingSphere)(xt...)
    x, t = xt[1:end-1], xt[end]
    c = b.center(t)
    f = sqrt(sum((x[d] - c[d])^2 for d in 1:length(c))) - b.radius(t)
    b.complement ? -f : f
end
function (b::MovingHalfSpace)(xt...)
    f = b.sign * (xt[b.axis] - b.position(xt[end]))
    b.complement ? -f : f
end
_mstate(b::MovingSphere, t, N) = (c = b.center(t); Float64[ntuple(d -> d <= N ? Float64(c[d]) : 0.0, 3)..., Float64(b.radius(t))])
_mstate(b::MovingHalfSpace, t, N) = Float64[Float64(b.position(t)), 0.0, 0.0, 1.0]
_mrate(b::MovingBody, t, N, h) = (_mstate(b, t + h, N) .- _mstate(b, t - h, N)) ./ (2h)       # only enters Γ

struct pg_motion_desc
    body_kind::Int32; flags::Int32; axis::Int32; nq::Int32
    sign::Float64; t0::Float64; t1::Float64
    nodes::Ptr{Float64}
    body0::NTuple{4, Float64}; body1::NTuple{4, Float64}
end
const PG_CAP_ST_V0, PG_CAP_ST_V1, PG_CAP_ST_CT_OMEGA, PG_CAP_ST_CT_GAMMA = 8:11

# Gauss-Legendre nodes / weights on [-1, 1] (Newton on P_n; no package needed)
function _gauss(n::Int)
    x, w = zeros(n), zeros(n)
    for i in 1:n
        z = cos(π * (i - 0.25) / (n + 0.5))
        dp = 1.0
        for _ in 1:100
            p0, p1 = 1.0, z
            for k in 2:n
                p0, p1 = p1, ((2k - 1) * z * p1 - (k - 1) * p0) / k
            end
            dp = n * (z * p1 - p0) / (z^2 - 1)
            dz = p1 / dp
            z -= dz
            abs(dz) < 1e-15 && break
        end
        x[i], w[i] = z, 2 / ((1 - z^2) * dp^2)
    end
    x, w
end

"The first time layer of the (N+1)-D capacity: the N-D fields of `Capacity{N}` plus the time-face capacities and the time
components of the centroids.  `A_st` has the reference's layout (N+1 diagonal matrices of size 2M, the last = [Vn_1; Vn])."
mutable struct SpaceTimeCapacity{N} <: AbstractCapacity
    layer::Capacity{N}
    Vn_1::Vector{Float64}; Vn::Vector{Float64}
    Ct_ω::Vector{Float64}; Ct_γ::Vector{Float64}
    mesh::SpaceTimeMesh
    body::Function
end
function Base.getproperty(c::SpaceTimeCapacity{N}, s::Symbol) where N
    s in (:layer, :Vn_1, :Vn, :Ct_ω, :Ct_γ, :mesh, :body) && return getfield(c, s)
    s === :handle && return getfield(c, :layer).handle
    if s === :A_st
        l = getfield(c, :layer); z = zeros(length(getfield(c, :Vn)))
        return (ntuple(d -> _diag(vcat(Vector(diag(l.A[d])), z)), N)..., _diag(vcat(getfield(c, :Vn_1), getfield(c, :Vn))))
    end
    getproperty(getfield(c, :layer), s)              # A, B, V, W, Γ, C_ω, C_γ, cell_types of the layer
end

function Capacity(body::MovingBody, mesh::SpaceTimeMesh; method::String="VOFI", compute_centroids::Bool=true,
                  time_panels::Int=16, time_order::Int=4)
    init()
    sp = mesh.space
    N = length(sp.dims)
    t0, t1 = mesh.nodes[end][1], mesh.nodes[end][2]
    gx, gw = _gauss(time_order)
    edges = range(t0, t1; length=time_panels + 1)
    nq = time_panels * time_order
    nodes = zeros(10, nq)                              # column k = {tau, w, c1, c2, c3, r, dc1, dc2, dc3, dr}
    h = 1e-6 * (t1 - t0)
    k = 0
    for p in 1:time_panels, i in 1:time_order
        k += 1
        a, b = edges[p], edges[p + 1]
        τ = (a + b) / 2 + (b - a) / 2 * gx[i]
        nodes[1, k], nodes[2, k] = τ, (b - a) / 2 * gw[i]
        nodes[3:6, k] .= _mstate(body, τ, N)
        nodes[7:10, k] .= _mrate(body, τ, N, h)
    end
    nodes[2, :] .*= (t1 - t0) / sum(nodes[2, :])
    flags = Int32((body.complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    kind = body isa MovingSphere ? Int32(1) : Int32(3)
    axis = body isa MovingHalfSpace ? Int32(body.axis - 1) : Int32(0)
    sgn = body isa MovingHalfSpace ? body.sign : 1.0
    hnd = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve nodes begin
        desc = Ref(pg_motion_desc(kind, flags, axis, Int32(nq), sgn, t0, t1, pointer(nodes),
                                  Tuple(_mstate(body, t0, N)), Tuple(_mstate(body, t1, N))))
        check(ccall((:pg_capacity_create_spacetime, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_motion_desc}, Ptr{Ptr{Cvoid}}), sp.handle, desc, hnd))
    end
    layer = _wrap_capacity(hnd[], sp, body, compute_centroids)
    M = prod(sp.dims .+ 1)
    SpaceTimeCapacity{N}(layer, _field(hnd[], PG_CAP_ST_V0, 0, M), _field(hnd[], PG_CAP_ST_V1, 0, M),
                         _field(hnd[], PG_CAP_ST_CT_OMEGA, 0, M), compute_centroids ? _field(hnd[], PG_CAP_ST_CT_GAMMA, 0, M) : Float64[],
                         mesh, body)
end

# A moving body of any shape: body = DeviceFunction((x, y, t) -> ...), the reference's `body = (x, y, t) -> ...` traced once.
# phi, its N spatial derivatives and d phi / dt are evaluated inside the space-time kernels
# (pg_capacity_create_spacetime_program); the programs are cached in the DeviceFunction (`moving`, by N), so a solve
# compiles them once, not once per slab.  The other phase of a two-phase problem: body_c = MovingComplement(body).
function _moving_trace(df::DeviceFunction, N::Integer)
    out = df.f((_symvar(d) for d in 0:N - 1)..., _symvar(3))
    out isa Sym ? out : Sym(out)
end
function _moving_programs(df::DeviceFunction, N::Integer)
    get!(df.moving, Int(N)) do
        root = _moving_trace(df, N)
        derivs = UInt8[]
        for (var, name) in [((d, "coordinate $d") for d in 0:N - 1)..., (3, "t")]
            try
                append!(derivs, _compile_program(differentiate(root, var)))
            catch e
                error("DeviceFunction: the derivative along $name of the moving body $(df.f) does not fit: $(sprint(showerror, e))")
            end
        end
        (_compile_program(root), derivs)
    end
end
moving_body_program(df::DeviceFunction, N::Integer) = _moving_programs(df, N)[1]
"N + 1 programs, contiguous as the C arrays: the N spatial partial derivatives, then d/dt"
moving_gradient_programs(df::DeviceFunction, N::Integer) = _moving_programs(df, N)[2]
struct MovingComplement <: Function
    body::DeviceFunction
end
(b::MovingComplement)(xt...) = -b.body.f(xt...)
function Capacity(body::DeviceFunction, mesh::SpaceTimeMesh; method::String="VOFI", compute_centroids::Bool=true,
                  time_panels::Int=16, time_order::Int=4, complement::Bool=false, reported_body::Function=body)
    init()
    sp = mesh.space
    N = length(sp.dims)
    t0, t1 = mesh.nodes[end][1], mesh.nodes[end][2]
    gx, gw = _gauss(time_order)
    edges = range(t0, t1; length=time_panels + 1)
    nq = time_panels * time_order
    tau_w = zeros(2, nq)                               # column k = {tau, w}: the C layout nq x 2
    k = 0
    for p in 1:time_panels, i in 1:time_order
        k += 1
        a, b = edges[p], edges[p + 1]
        tau_w[1, k], tau_w[2, k] = (a + b) / 2 + (b - a) / 2 * gx[i], (b - a) / 2 * gw[i]
    end
    tau_w[2, :] .*= (t1 - t0) / sum(tau_w[2, :])
    flags = Int32((complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    hnd = Ref{Ptr{Cvoid}}(C_NULL)
    if N == 1 || N == 2
        phi, derivs = moving_body_program(body, N), moving_gradient_programs(body, N)
        np = length(phi)                               # bytes of one program
        GC.@preserve derivs begin
            check(ccall((:pg_capacity_create_spacetime_program, libpg), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64, Int32, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                        sp.handle, phi, pointer(derivs), pointer(derivs) + N * np, flags, t0, t1, Int32(nq), tau_w, hnd))
        end
    else
        error("space-time capacities: 1-D+t and 2-D+t (the reference's 3-D+t blocks drop the z direction)")
    end
    layer = _wrap_capacity(hnd[], sp, reported_body, compute_centroids)
    M = prod(sp.dims .+ 1)
    SpaceTimeCapacity{N}(layer, _field(hnd[], PG_CAP_ST_V0, 0, M), _field(hnd[], PG_CAP_ST_V1, 0, M),
                         _field(hnd[], PG_CAP_ST_CT_OMEGA, 0, M), compute_centroids ? _field(hnd[], PG_CAP_ST_CT_GAMMA, 0, M) : Float64[],
                         mesh, reported_body)
end
Capacity(b::MovingComplement, mesh::SpaceTimeMesh; kwargs...) = Capacity(b.body, mesh; complement=true, reported_body=b, kwargs...)

# A marker polygon that moves: Capacity(front_n, front_np1, stmesh), the reference's compute_spacetime_capacities(mesh, front_n,
# front_np1, dt) (src/front_tracking.jl:1472).  The two fronts hold the markers at the slab's two times, the same count and order;
# inside the slab every marker moves on a straight line at constant speed (interpolate_front, :2289) and
# pg_capacity_create_spacetime_polygon measures the polygon at every time node.  Fluid is the interior, complement=true: the
# exterior.  2-D, closed fronts, one rank.  cap.body is front_n.
function Capacity(front_n::FrontTracker, front_np1::FrontTracker, mesh::SpaceTimeMesh; method::String="VOFI",
                  compute_centroids::Bool=true, time_panels::Int=16, time_order::Int=4, complement::Bool=false)
    (front_n.is_closed && front_np1.is_closed) || error("PenguinHIP.Capacity(front_n, front_np1, SpaceTimeMesh): is_closed=false is not supported")
    sp = mesh.space
    N = length(sp.dims)
    N == 2 || error("PenguinHIP.Capacity(front_n, front_np1, SpaceTimeMesh): a moving marker polygon is a 2-D body, the mesh is $(N)-D")
    p0, p1 = front_n.markers, front_np1.markers
    length(p0) == length(p1) || error("PenguinHIP.Capacity(front_n, front_np1, SpaceTimeMesh): the fronts have $(length(p0)) and " *
                                      "$(length(p1)) markers; both need the same count and order")
    init()
    t0, t1 = mesh.nodes[end][1], mesh.nodes[end][2]
    gx, gw = _gauss(time_order)
    edges = range(t0, t1; length=time_panels + 1)
    nq = time_panels * time_order
    tau_w = zeros(2, nq)                               # column k = {tau, w}: the C layout nq x 2
    k = 0
    for p in 1:time_panels, i in 1:time_order
        k += 1
        a, b = edges[p], edges[p + 1]
        tau_w[1, k], tau_w[2, k] = (a + b) / 2 + (b - a) / 2 * gx[i], (b - a) / 2 * gw[i]
    end
    tau_w[2, :] .*= (t1 - t0) / sum(tau_w[2, :])
    xy0 = Float64[p[c] for p in p0 for c in 1:2]       # x0 y0 x1 y1 ...; a closing duplicate is dropped by the entry
    xy1 = Float64[p[c] for p in p1 for c in 1:2]
    flags = Int32((complement ? 1 : 0) | (compute_centroids ? 0 : 2))
    hnd = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_capacity_create_spacetime_polygon, libpg), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Float64, Float64, Int32, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                sp.handle, xy0, xy1, length(p0), flags, t0, t1, Int32(nq), tau_w, hnd))
    layer = _wrap_capacity(hnd[], sp, front_n, compute_centroids)
    M = prod(sp.dims .+ 1)
    SpaceTimeCapacity{N}(layer, _field(hnd[], PG_CAP_ST_V0, 0, M), _field(hnd[], PG_CAP_ST_V1, 0, M),
                         _field(hnd[], PG_CAP_ST_CT_OMEGA, 0, M), compute_centroids ? _field(hnd[], PG_CAP_ST_CT_GAMMA, 0, M) : Float64[],
                         mesh, front_n)
end
DiffusionOps(cap::SpaceTimeCapacity) = DiffusionOps(cap.layer)

# ConvectionOps(capacity, uₒ, uᵧ) of a space-time capacity (2-D+t), as the moving advection-diffusion blocks slice it
# (prescribedmotionsolver/advectiondiffusion.jl:94-95): C = (C[1][L1,L1], C[2][L2,L2], C[3][L1,L2]) = (C_x of the first layer,
# 0, 0) and the same of K; uₒ = (uₒx, uₒy, uₒt) of 2M each, uᵧ of 3·2M.  A non-zero uₒt or time block of uᵧ, and 1-D+t (the
# reference's BoundsError), are refused by pg_diffops_set_velocity_spacetime.
function ConvectionOps(cap::SpaceTimeCapacity{N}, uₒ::NTuple{3, Vector{Float64}}, uᵧ::Vector{Float64}) where N
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pg_diffops_create, libpg), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), cap.handle, h))
    sz = cap.layer.mesh.dims .+ 1
    M = prod(sz)
    GC.@preserve uₒ uᵧ begin
        ptrs = [pointer(u) for u in uₒ]
        check(ccall((:pg_diffops_set_velocity_spacetime, libpg), Int32, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Float64}), h[], ptrs, uᵧ))
    end
    Z = spzeros(M, M)
    op = ConvectionOps{3}((_export_csc(h[], 3, M, M), Z, Z), (_export_csc(h[], 6, M, M), Z, Z), _export_csc(h[], 0, N * M, M),
                          _export_csc(h[], 1, N * M, M), _export_csc(h[], 2, N * M, N * M), cap.V, (sz..., 2), h[])
    finalizer(x -> ccall((:pg_diffops_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), op)
    op
end

# The moving constructors of the library, one argument list per arity; `sym` names the variant (a computed name cannot stand
# in ccall's (name, library) tuple, so it is looked up with dlsym).  T_prev comes from the host, `previous` is not used here.
_create_moving_mono(sym::Symbol, cap, op, desc, borders, D, fn, fn1, Tᵢ, scheme, h) =
    check(ccall(Libdl.dlsym(Libdl.dlopen(libpg), sym), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_bc_desc}, Ptr{pg_border_desc}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}),
                cap.handle, op.handle, desc, borders, length(borders), D, fn, fn1, Tᵢ, C_NULL, _scheme(scheme), h))
_create_moving_diph(sym::Symbol, c1, o1, c2, o2, desc, borders, D1, D2, f1n, f1n1, f2n, f2n1, Tᵢ, scheme, h) =
    check(ccall(Libdl.dlsym(Libdl.dlopen(libpg), sym), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{pg_jump_desc}, Ptr{pg_border_desc}, Int32, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}),
                c1.handle, o1.handle, c2.handle, o2.handle, desc, borders, length(borders), D1, D2, f1n, f1n1, f2n, f2n1, Tᵢ, C_NULL,
                _scheme(scheme), h))

# closures see the space-time centroids padded to three coordinates (build_source / build_g_g on the (N+1)-D capacity)
_st_coords(C, Ct) = [coords3((c..., Ct[i])) for (i, c) in enumerate(C)]
function _moving_step!(s::Solver, phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary, Δt::Float64, Tᵢ::Vector{Float64},
                       mesh::Mesh, scheme::String, t::Float64; advdiff::Bool=false)
    cap = phase.capacity
    cap isa SpaceTimeCapacity || error("the moving solver needs a space-time capacity: Capacity(body, SpaceTimeMesh(mesh, [t, t+Δt]))")
    advdiff && _need_st_conv(phase)
    Cω = _st_coords(cap.C_ω, cap.Ct_ω)
    g = bc_i.value isa Function ? Float64[Float64(bc_i.value(c...)) for c in _st_coords(cap.C_γ, cap.Ct_γ)] : Float64[]   # :172
    D = Float64[Float64(phase.Diffusion_coeff(c...)) for c in Cω]
    fn1 = Float64[Float64(phase.source(c..., t + Δt)) for c in Cω]                                                       # :171
    fn = Float64[Float64(phase.source(c..., t)) for c in Cω]                                                             # :170
    borders = _border_descs(bc_b)
    s.handle != C_NULL && ccall((:pg_solver_destroy, libpg), Int32, (Ptr{Cvoid},), s.handle)
    s.handle = C_NULL
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g D fn fn1 Tᵢ borders begin
        desc = Ref(_interface_desc(bc_i, g))
        # advdiff: A_/b_mono_unstead_advdiff_moving (advectiondiffusion.jl:64-199)
        _create_moving_mono(advdiff ? :pg_solver_create_moving_advdiff_mono : :pg_solver_create_moving_mono, cap, phase.operator,
                            desc, borders, D, fn, fn1, Tᵢ, scheme, h)
    end
    s.handle = h[]
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, mesh, t)
    s.A = (cap, phase.operator)          # keeps the device capacity alive as long as this slab's solver
    s
end

function MovingDiffusionUnsteadyMono(phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary, Δt::Float64, Tᵢ::Vector{Float64},
                                     mesh::AbstractMesh, scheme::String)
    println("Solver Creation:"); println("- Moving problem"); println("- Monophasic problem"); println("- Unsteady problem"); println("- Diffusion problem")
    s = _new_solver(:Unsteady, :Monophasic, :Diffusion, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _moving_step!(s, phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme, 0.0)          # t = 0.0 in b and in the border rows (:27-33)
end

function solve_MovingDiffusionUnsteadyMono!(s::Solver, phase::Phase, body::Function, Δt::Float64, Tₛ::Float64, Tₑ::Float64,
                                            bc_b::BorderConditions, bc::AbstractBoundary, mesh::AbstractMesh, scheme::String;
                                            method::Function=gmres, algorithm=nothing, geometry_method="VOFI", kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    function solve!()
        check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
        _record!(s, info, log)
        println("Solver Extremum : ", maximum(abs.(s.x)))
    end
    t = Tₛ
    println("Time : $(t)")
    solve!()                                                                 # :240-244
    Tᵢ = s.x
    while t < Tₑ                                                             # :247
        t += Δt
        println("Time : $(t)")
        capacity = Capacity(body, SpaceTimeMesh(mesh, [t, t + Δt], tag=mesh.tag); compute_centroids=true, method=geometry_method)
        ph = Phase(capacity, DiffusionOps(capacity), phase.source, phase.Diffusion_coeff)
        _moving_step!(s, ph, bc_b, bc, Δt, Tᵢ, mesh, scheme, t)              # A, b, BC_border_mono!(...; t=t)   :254-258
        solve!()
        Tᵢ = s.x
    end
    s
end

# ---- two phases: MovingDiffusionUnsteadyDiph (:272-290), A_/b_diph_unstead_diff_moving (:292-498),
# solve_MovingDiffusionUnsteadyDiph! (:501-535) -----------------------------------------------------------------------------------
function _moving_step_diph!(s::Solver, phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64,
                            Tᵢ::Vector{Float64}, mesh::Mesh, scheme::String, t::Float64; advdiff::Bool=false)
    c1, c2 = phase1.capacity, phase2.capacity
    advdiff && (_need_st_conv(phase1); _need_st_conv(phase2))
    (c1 isa SpaceTimeCapacity && c2 isa SpaceTimeCapacity) ||
        error("the moving solver needs space-time capacities: Capacity(body, SpaceTimeMesh(mesh, [t, t+Δt]))")
    Cω1, Cω2 = _st_coords(c1.C_ω, c1.Ct_ω), _st_coords(c2.C_ω, c2.Ct_ω)
    # build_g_g(operator, jump, capacity): value(C_γ...) at the space-time interface centroids, no time argument (:423-424)
    g = ic.scalar.value isa Function ? Float64[Float64(ic.scalar.value(c...)) for c in _st_coords(c1.C_γ, c1.Ct_γ)] : Float64[]
    hh = ic.flux.value isa Function ? Float64[Float64(ic.flux.value(c...)) for c in _st_coords(c2.C_γ, c2.Ct_γ)] : Float64[]
    D1 = Float64[Float64(phase1.Diffusion_coeff(c...)) for c in Cω1]
    D2 = Float64[Float64(phase2.Diffusion_coeff(c...)) for c in Cω2]
    f1n1 = Float64[Float64(phase1.source(c..., t + Δt)) for c in Cω1]                                       # :416
    f2n1 = Float64[Float64(phase2.source(c..., t + Δt)) for c in Cω2]                                       # :418
    f1n = Float64[Float64(phase1.source(c..., t)) for c in Cω1]                                             # :415
    f2n = Float64[Float64(phase2.source(c..., t)) for c in Cω2]                                             # :417
    borders = _border_descs(bc_b)
    s.handle != C_NULL && ccall((:pg_solver_destroy, libpg), Int32, (Ptr{Cvoid},), s.handle)
    s.handle = C_NULL
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g hh D1 D2 f1n f2n f1n1 f2n1 Tᵢ borders begin
        desc = Ref(_jump_desc(ic, c1, c2, g, hh))
        # advdiff: A_/b_diph_unstead_advdiff_moving (advectiondiffusion.jl:266-507)
        _create_moving_diph(advdiff ? :pg_solver_create_moving_advdiff_diph : :pg_solver_create_moving_diph, c1, phase1.operator, c2,
                            phase2.operator, desc, borders, D1, D2, f1n, f1n1, f2n, f2n1, Tᵢ, scheme, h)
    end
    s.handle = h[]
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, mesh, nothing)   # BC_border_diph!(s.A, s.b, bc_b, mesh): no t (:288, :523)
    s.A = (c1, c2, phase1.operator, phase2.operator)     # keeps the device capacities alive as long as this slab's solver
    s
end

function MovingDiffusionUnsteadyDiph(phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64,
                                     Tᵢ::Vector{Float64}, mesh::AbstractMesh, scheme::String)
    println("Solver Creation:"); println("- Moving problem"); println("- Diphasic problem"); println("- Unsteady problem"); println("- Diffusion problem")
    s = _new_solver(:Unsteady, :Diphasic, :Diffusion, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _moving_step_diph!(s, phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme, 0.0)          # t = 0.0 in b (:282, :285)
end

function solve_MovingDiffusionUnsteadyDiph!(s::Solver, phase1::Phase, phase2::Phase, body::Function, body_c::Function, Δt::Float64,
                                            Tₑ::Float64, bc_b::BorderConditions, ic::InterfaceConditions, mesh::AbstractMesh,
                                            scheme::String; method::Function=gmres, algorithm=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    function solve!()
        check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
        _record!(s, info, log)
        println("Solver Extremum : ", maximum(abs.(s.x)))
    end
    t = 0.0                                                                  # :513
    println("Time : $(t)")
    solve!()
    Tᵢ = s.x
    while t < Tₑ                                                             # :517
        t += Δt
        println("Time : $(t)")
        STmesh = SpaceTimeMesh(mesh, [t, t + Δt], tag=mesh.tag)
        capacity1, capacity2 = Capacity(body, STmesh), Capacity(body_c, STmesh)
        ph1 = Phase(capacity1, DiffusionOps(capacity1), phase1.source, phase1.Diffusion_coeff)
        ph2 = Phase(capacity2, DiffusionOps(capacity2), phase2.source, phase2.Diffusion_coeff)
        _moving_step_diph!(s, ph1, ph2, bc_b, ic, Δt, Tᵢ, mesh, scheme, t)   # A, b, BC_border_diph!(A, b, bc_b, mesh)   :519-523
        solve!()
        Tᵢ = s.x
    end
    s
end

# ---- prescribed-motion advection-diffusion: MovingAdvDiffusionUnsteadyMono / Diph and their loops
# (prescribedmotionsolver/advectiondiffusion.jl:15-33, 201-242, 246-264, 510-553); the operators are ConvectionOps of the
# space-time capacities, rebuilt per slab from the same uₒ, uᵧ ----------------------------------------------------------------
_need_st_conv(ph::Phase) = (ph.operator isa ConvectionOps && ph.capacity isa SpaceTimeCapacity) ||
    error("the moving advection-diffusion solver needs phase.operator = ConvectionOps(capacity, uₒ, uᵧ) of a space-time capacity")

function MovingAdvDiffusionUnsteadyMono(phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary, Δt::Float64, Tᵢ::Vector{Float64},
                                        mesh::AbstractMesh, scheme::String)
    println("Solver Creation:"); println("- Moving problem"); println("- Monophasic problem"); println("- Unsteady problem"); println("- Advection-Diffusion problem")
    s = _new_solver(:Unsteady, :Monophasic, :DiffusionAdvection, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _moving_step!(s, phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme, 0.0; advdiff=true)   # t = 0.0 in b and in the border rows (:24-31)
end

function solve_MovingAdvDiffusionUnsteadyMono!(s::Solver, phase::Phase, body::Function, Δt::Float64, Tₛ::Float64, Tₑ::Float64,
                                               bc_b::BorderConditions, bc::AbstractBoundary, mesh::AbstractMesh, scheme::String, uₒ, uᵧ;
                                               method::Function=gmres, algorithm=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    function solve!()
        check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
        _record!(s, info, log)
        println("Solver Extremum : ", maximum(abs.(s.x)))
    end
    t = Tₛ                                                                   # :213
    println("Time : $(t)")
    solve!()
    Tᵢ = s.x
    while t < Tₑ
        t += Δt
        println("Time : $(t)")
        capacity = Capacity(body, SpaceTimeMesh(mesh, [t, t + Δt], tag=mesh.tag); compute_centroids=true)
        ph = Phase(capacity, ConvectionOps(capacity, uₒ, uᵧ), phase.source, phase.Diffusion_coeff)      # :225-227
        _moving_step!(s, ph, bc_b, bc, Δt, Tᵢ, mesh, scheme, t; advdiff=true)    # A, b, BC_border_mono!(...; t=t)   :229-232
        solve!()
        Tᵢ = s.x
    end
    s
end

function MovingAdvDiffusionUnsteadyDiph(phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64,
                                        Tᵢ::Vector{Float64}, mesh::AbstractMesh, scheme::String)
    println("Solver Creation:"); println("- Moving problem"); println("- Diphasic problem"); println("- Unsteady problem"); println("- Advection-Diffusion problem")
    s = _new_solver(:Unsteady, :Diphasic, :DiffusionAdvection, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _moving_step_diph!(s, phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme, 0.0; advdiff=true)     # t = 0.0 in b (:255-262)
end

function solve_MovingAdvDiffusionUnsteadyDiph!(s::Solver, phase1::Phase, phase2::Phase, body::Function, body_c::Function, Δt::Float64,
                                               Tₛ::Float64, Tₑ::Float64, bc_b::BorderConditions, ic::InterfaceConditions,
                                               mesh::AbstractMesh, scheme::String, uₒ, uᵧ; method::Function=gmres, algorithm=nothing,
                                               kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    kw = Dict{Symbol, Any}(kwargs)
    log = get(kw, :log, false)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    function solve!()
        check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
        _record!(s, info, log)
        println("Solver Extremum : ", maximum(abs.(s.x)))
    end
    t = Tₛ                                                                   # :522 (the diffusion twin starts at 0.0)
    println("Time : $(t)")
    solve!()
    Tᵢ = s.x
    while t < Tₑ
        t += Δt
        println("Time : $(t)")
        STmesh = SpaceTimeMesh(mesh, [t, t + Δt], tag=mesh.tag)
        capacity1, capacity2 = Capacity(body, STmesh), Capacity(body_c, STmesh)
        ph1 = Phase(capacity1, ConvectionOps(capacity1, uₒ, uᵧ), phase1.source, phase1.Diffusion_coeff)   # :537-538
        ph2 = Phase(capacity2, ConvectionOps(capacity2, uₒ, uᵧ), phase2.source, phase2.Diffusion_coeff)
        _moving_step_diph!(s, ph1, ph2, bc_b, ic, Δt, Tᵢ, mesh, scheme, t; advdiff=true)   # BC_border_diph!(A, b, bc_b, mesh)  :543
        solve!()
        Tᵢ = s.x
    end
    s
end

# ---- liquid motion, 1-D (liquidmotionsolver/diffusion.jl): MovingLiquidDiffusionUnsteadyMono (:152-171) and its loop
# (:173-442), MovingLiquidDiffusionUnsteadyDiph (:653-673) with A_/b_diph_unstead_diff_moving_stef (:445-651) and its loop
# (:675-946).  Every Newton iteration solves one slab and reads its Stefan terms on the device (pg_solver_stefan_terms:
# Σ A_t(t0) = Hₙ₊₁, Σ A_t(t1) = Hₙ, Σq, max|q| per phase).  The learning rate here is the fixed one (α); the Python package
# carries all six strategies, adapt_timestep and the border rows at tₙ₊₁ of the Newton rebuilds (penguin/jl_amd/liquid.py);
# here the border rows take b's time.
function _stefan_terms(s::Solver, nphase::Int)
    out = zeros(Float64, 4 * nphase)
    check(ccall((:pg_solver_stefan_terms, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.handle, out))
    out
end

function _liquid_1d(mesh)
    length(mesh.nodes) == 1 || error("the liquid-motion solvers are 1-D only: the reference's N ≥ 2 call feeds y into the body's time argument")
end

_front_body(xf, new_xf, tn, tn1, Δt; complement::Bool=false) =
    MovingHalfSpace(1, tt -> xf * (tn1 - tt) / Δt + new_xf * (tt - tn) / Δt; complement=complement)

function _stefan_step_diph!(s::Solver, phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64,
                            Tᵢ::Vector{Float64}, mesh::Mesh, scheme::String, t::Float64)
    c1, c2 = phase1.capacity, phase2.capacity
    Cω1, Cω2 = _st_coords(c1.C_ω, c1.Ct_ω), _st_coords(c2.C_ω, c2.Ct_ω)
    g = ic.scalar.value isa Function ? Float64[Float64(ic.scalar.value(c...)) for c in _st_coords(c1.C_γ, c1.Ct_γ)] : Float64[]
    hh = Float64[]
    D1 = Float64[Float64(phase1.Diffusion_coeff(c...)) for c in Cω1]
    D2 = Float64[Float64(phase2.Diffusion_coeff(c...)) for c in Cω2]
    f1n1 = Float64[Float64(phase1.source(c..., t + Δt)) for c in Cω1]
    f2n1 = Float64[Float64(phase2.source(c..., t + Δt)) for c in Cω2]
    f1n = Float64[Float64(phase1.source(c..., t)) for c in Cω1]
    f2n = Float64[Float64(phase2.source(c..., t)) for c in Cω2]
    borders = _border_descs(bc_b)
    s.handle != C_NULL && ccall((:pg_solver_destroy, libpg), Int32, (Ptr{Cvoid},), s.handle)
    s.handle = C_NULL
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve g hh D1 D2 f1n f2n f1n1 f2n1 Tᵢ borders begin
        desc = Ref(_jump_desc(ic, c1, c2, g, hh))
        _create_moving_diph(:pg_solver_create_moving_stefan_diph, c1, phase1.operator, c2, phase2.operator, desc, borders, D1, D2,
                            f1n, f1n1, f2n, f2n1, Tᵢ, scheme, h)
    end
    s.handle = h[]
    _has_border_functions(bc_b) && _set_border_values!(s, bc_b, mesh, nothing)
    s.A = (c1, c2, phase1.operator, phase2.operator)
    s
end

function MovingLiquidDiffusionUnsteadyMono(phase::Phase, bc_b::BorderConditions, bc_i::AbstractBoundary, Δt::Float64,
                                           Tᵢ::Vector{Float64}, mesh::AbstractMesh, scheme::String)
    _liquid_1d(mesh)
    println("Solver Creation:"); println("- Moving problem"); println("- Non prescibed motion"); println("- Monophasic problem")
    println("- Unsteady problem"); println("- Diffusion problem")
    s = _new_solver(:Unsteady, :Monophasic, :Diffusion, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _moving_step!(s, phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme, 0.0)            # BC_border_mono!(...; t=0.0)   :165-169
end

function solve_MovingLiquidDiffusionUnsteadyMono!(s::Solver, phase::Phase, xf, Δt::Float64, Tₛ::Float64, Tₑ::Float64,
                                                  bc_b::BorderConditions, bc::AbstractBoundary, ic::InterfaceConditions,
                                                  mesh::AbstractMesh, scheme::String; Newton_params=(1000, 1e-10, 1e-10, 1.0),
                                                  method::Function=gmres, algorithm=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    _liquid_1d(mesh)
    kw = Dict{Symbol, Any}(kwargs)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    ρL = ic.flux.value
    max_iter, tol, reltol, α = Newton_params
    residuals = Dict{Int, Vector{Float64}}()
    xf_log = Float64[]
    timestep_history = Tuple{Float64, Float64}[(Tₛ, Δt)]
    t = Tₛ
    new_xf = Float64(xf)
    k = 1
    while true
        err = Inf; iter = 0; current_xf = new_xf; xf0 = current_xf
        while (iter < max_iter) && (err > tol) && (err > reltol * abs(current_xf))
            iter += 1
            check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
            _record!(s, info, false)
            Tᵢ = s.x
            r = _stefan_terms(s, 1)
            res = r[1] - r[2] - 1 / ρL * r[3]                                # Hₙ₊₁ - Hₙ - Interface_term
            step = α * res
            new_xf = current_xf + step
            err = k == 1 ? abs(res) : abs(step)
            push!(get!(residuals, k, Float64[]), err)
            if (err <= tol) || (err <= reltol * abs(current_xf)) || (iter == max_iter)
                push!(xf_log, new_xf)
                break
            end
            tn1, tn = t + Δt, t
            capacity = Capacity(_front_body(xf0, new_xf, tn, tn1, Δt), SpaceTimeMesh(mesh, [tn, tn1], tag=mesh.tag))
            ph = Phase(capacity, DiffusionOps(capacity), phase.source, phase.Diffusion_coeff)
            _moving_step!(s, ph, bc_b, bc, Δt, Tᵢ, mesh, scheme, t)
            current_xf = new_xf
        end
        t < Tₑ || break
        t += Δt
        capacity = Capacity(MovingHalfSpace(1, tt -> new_xf), SpaceTimeMesh(mesh, [Δt, 2Δt], tag=mesh.tag))
        ph = Phase(capacity, DiffusionOps(capacity), phase.source, phase.Diffusion_coeff)
        _moving_step!(s, ph, bc_b, bc, Δt, s.x, mesh, scheme, 0.0)
        k += 1
    end
    return s, residuals, xf_log, timestep_history
end

function MovingLiquidDiffusionUnsteadyDiph(phase1::Phase, phase2::Phase, bc_b::BorderConditions, ic::InterfaceConditions, Δt::Float64,
                                           Tᵢ::Vector{Float64}, mesh::AbstractMesh, scheme::String)
    _liquid_1d(mesh)
    println("Solver Creation:"); println("- Moving problem"); println("- Non prescibed motion"); println("- Diphasic problem")
    println("- Unsteady problem"); println("- Diffusion problem")
    s = _new_solver(:Unsteady, :Diphasic, :Diffusion, Ptr{Cvoid}(C_NULL), length(Tᵢ))
    _stefan_step_diph!(s, phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme, 0.0)
end

function solve_MovingLiquidDiffusionUnsteadyDiph!(s::Solver, phase1::Phase, phase2::Phase, xf, Δt::Float64, Tₛ::Float64, Tₑ::Float64,
                                                  bc_b::BorderConditions, ic::InterfaceConditions, mesh::AbstractMesh, scheme::String;
                                                  Newton_params=(1000, 1e-10, 1e-10, 1.0), method::Function=gmres,
                                                  algorithm=nothing, kwargs...)
    (s.handle == C_NULL) && error("Solver is not initialized. Call a solver constructor first.")
    _liquid_1d(mesh)
    kw = Dict{Symbol, Any}(kwargs)
    opts = Ref(_opts(method, kw))
    info = pg_step_info()
    ρL = ic.flux.value
    max_iter, tol, reltol, α = Newton_params
    residuals = Dict{Int, Vector{Float64}}()
    xf_log = Float64[]
    t = Tₛ
    new_xf = Float64(xf)
    Tᵢ = Float64[]
    k = 1
    while true
        err = Inf; iter = 0; current_xf = new_xf; xf0 = current_xf
        while (iter < max_iter) && (err > tol) && (err > reltol * abs(current_xf))
            iter += 1
            check(ccall((:pg_solver_initial_solve, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
            _record!(s, info, false)
            Tᵢ = s.x
            r = _stefan_terms(s, 2)
            res = r[1] - r[2] - (1 / ρL * r[3] + 1 / ρL * r[7])              # Hₙ, Hₙ₊₁ of phase 1 only
            step = α * res
            new_xf = current_xf + step
            err = k == 1 ? abs(res) : abs(step)
            push!(get!(residuals, k, Float64[]), err)
            if (err <= tol) || (err <= reltol * abs(current_xf))
                push!(xf_log, new_xf)
                break
            end
            tn1, tn = t + Δt, t
            current_xf = new_xf
            ((iter < max_iter) && (err > tol) && (err > reltol * abs(current_xf))) || break   # the rebuilt slab is never solved
            STmesh = SpaceTimeMesh(mesh, [tn, tn1], tag=mesh.tag)
            c1 = Capacity(_front_body(xf0, new_xf, tn, tn1, Δt), STmesh)
            c2 = Capacity(_front_body(xf0, new_xf, tn, tn1, Δt; complement=true), STmesh)
            ph1 = Phase(c1, DiffusionOps(c1), phase1.source, phase1.Diffusion_coeff)
            ph2 = Phase(c2, DiffusionOps(c2), phase2.source, phase2.Diffusion_coeff)
            _stefan_step_diph!(s, ph1, ph2, bc_b, ic, Δt, Tᵢ, mesh, scheme, t)
        end
        t < Tₑ || break
        t += Δt
        STmesh = SpaceTimeMesh(mesh, [Δt, 2Δt], tag=mesh.tag)
        c1 = Capacity(MovingHalfSpace(1, tt -> new_xf), STmesh)
        c2 = Capacity(MovingHalfSpace(1, tt -> new_xf; complement=true), STmesh)
        ph1 = Phase(c1, DiffusionOps(c1), phase1.source, phase1.Diffusion_coeff)
        ph2 = Phase(c2, DiffusionOps(c2), phase2.source, phase2.Diffusion_coeff)
        _stefan_step_diph!(s, ph1, ph2, bc_b, ic, Δt, Tᵢ, mesh, scheme, 0.0)
        k += 1
    end
    return s, residuals, xf_log
end

# ---------------------------------------------------------------------------------- StreamVorticity
# src/solver/streamfunction_vorticity.jl: ∇²ψ = -ω, u = ∂ψ/∂y, v = -∂ψ/∂x, ω advected and diffused with (u, v).  ψ, ω, the
# velocity and the convection operators stay on the device between steps (pg_streamvort); the fields below are refreshed
# after every call.  Kept as the reference has them: the ψ of a state is solved from the ω of the state before (:222, :239);
# uᵧ = [u; v] (:176-179); border values without a time (:198, :231).  The reference's call at :228 leaves the D of
# b_mono_unstead_advdiff out (a MethodError); D = ν runs here -- never read under "BE", the explicit diffusion under "CN".
mutable struct StreamVorticity{N}
    capacity::Capacity{N}
    operator::DiffusionOps{N}
    ν::Union{Float64, Function}
    Δt::Float64
    bc_stream::AbstractBoundary
    bc_vorticity::AbstractBoundary
    bc_stream_border::BorderConditions
    bc_vorticity_border::BorderConditions
    ψ::Vector{Float64}
    ω::Vector{Float64}
    velocity::NTuple{N, Vector{Float64}}
    source::Function
    time::Float64
    states::Vector{NamedTuple}
    Aψ::Union{Nothing, SparseMatrixCSC{Float64, Int}}     # (not exported from the device: the Poisson system is pg_streamvort_solver(0))
    last_convection::Union{Nothing, ConvectionOps{N}}
    handle::Ptr{Cvoid}
    ω_device::Vector{Float64}                              # the ω the library holds (s.ω may be assigned or broadcast into)
    nstates_device::Int
    sent::Dict{Any,Any}
end

function StreamVorticity(capacity::Capacity{2}, ν, Δt;
                         bc_stream::AbstractBoundary = Dirichlet(0.0),
                         bc_vorticity::AbstractBoundary = Dirichlet(0.0),
                         bc_stream_border::BorderConditions = BorderConditions(Dict{Symbol,AbstractBoundary}()),
                         bc_vorticity_border::BorderConditions = BorderConditions(Dict{Symbol,AbstractBoundary}()),
                         ψ0::Union{Nothing,Vector{Float64}} = nothing,
                         ω0::Union{Nothing,Vector{Float64}} = nothing,
                         source::Function = (args...)->0.0)
    operator = DiffusionOps(capacity)
    n = prod(operator.size)
    ψ_init = isnothing(ψ0) ? zeros(2n) : copy(ψ0)
    ω_init = isnothing(ω0) ? zeros(2n) : copy(ω0)
    nu = ν isa Function ? evalf0(ν, capacity.C_ω) : fill(Float64(ν), n)                     # build_I_D
    gs = bc_stream.value isa Function ? evalf(bc_stream.value, capacity.C_γ, 0.0) : Float64[]
    gw = bc_vorticity.value isa Function ? evalf(bc_vorticity.value, capacity.C_γ, Float64(Δt)) : Float64[]
    bs, bw = _border_descs(bc_stream_border), _border_descs(bc_vorticity_border)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve nu gs gw bs bw ψ_init ω_init begin
        ds, dw = Ref(_interface_desc(bc_stream, gs)), Ref(_interface_desc(bc_vorticity, gw))
        check(ccall((:pg_streamvort_create, libpg), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Float64, Ptr{pg_bc_desc}, Ptr{pg_bc_desc}, Ptr{pg_border_desc}, Int32,
                     Ptr{pg_border_desc}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
                    capacity.handle, operator.handle, nu, Float64(Δt), ds, dw, bs, length(bs), bw, length(bw), ψ_init, ω_init, h))
    end
    s = StreamVorticity{2}(capacity, operator, ν, Float64(Δt), bc_stream, bc_vorticity, bc_stream_border, bc_vorticity_border,
                           ψ_init, ω_init, (zeros(n), zeros(n)), source, 0.0,
                           NamedTuple[(time = 0.0, ψ = copy(ψ_init), ω = copy(ω_init))], nothing, nothing, h[], copy(ω_init), 1,
                           Dict{Any,Any}())
    finalizer(x -> ccall((:pg_streamvort_destroy, libpg), Int32, (Ptr{Cvoid},), x.handle), s)
    _has_border_functions(bc_stream_border) &&
        check(ccall((:pg_streamvort_set_border_values, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}), s.handle, 0,
                    _border_values(bc_stream_border, capacity.mesh, nothing)))
    _has_border_functions(bc_vorticity_border) &&
        check(ccall((:pg_streamvort_set_border_values, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}), s.handle, 1,
                    _border_values(bc_vorticity_border, capacity.mesh, nothing)))
    s
end

function _sv_get(s::StreamVorticity, field::Integer, index::Integer, len::Integer)
    out = zeros(len)
    check(ccall((:pg_streamvort_get, libpg), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64), s.handle, field, index, out, len))
    out
end
# what the library needs before a solve: the ω the caller may have assigned, and the data of the closures at s.time
function _sv_push!(s::StreamVorticity)
    n = prod(s.operator.size)
    if s.ω != s.ω_device
        check(ccall((:pg_streamvort_set_omega, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.handle, s.ω))
        s.ω_device = copy(s.ω)
    end
    t, cap = s.time, s.capacity
    fn, fn1 = evalf(s.source, cap.C_ω, t), evalf(s.source, cap.C_ω, t + s.Δt)
    if _changed!(s.sent, :f, fn, fn1) && (haskey(s.sent, :f_sent) || any(!iszero, fn) || any(!iszero, fn1))
        check(ccall((:pg_streamvort_set_source, libpg), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, fn, fn1))
        s.sent[:f_sent] = (true,)
    end
    if s.bc_stream.value isa Function
        g = evalf(s.bc_stream.value, cap.C_γ, t)
        _changed!(s.sent, :gs, g) &&
            check(ccall((:pg_streamvort_set_interface_values, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}),
                        s.handle, 0, Ptr{Float64}(C_NULL), g))
    end
    if s.bc_vorticity.value isa Function
        g0, g1 = evalf(s.bc_vorticity.value, cap.C_γ, t), evalf(s.bc_vorticity.value, cap.C_γ, t + s.Δt)
        _changed!(s.sent, :gw, g0, g1) &&
            check(ccall((:pg_streamvort_set_interface_values, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}),
                        s.handle, 1, g0, g1))
    end
    nothing
end
# the fields after a call: ψ, ω, velocity, time and the states the library has added
function _sv_pull!(s::StreamVorticity)
    n = prod(s.operator.size)
    s.ψ, s.ω = _sv_get(s, 0, -1, 2n), _sv_get(s, 1, -1, 2n)
    s.ω_device = copy(s.ω)
    s.velocity = (_sv_get(s, 2, -1, n), _sv_get(s, 3, -1, n))
    s.last_convection = nothing
    t = Ref{Float64}(0.0)
    check(ccall((:pg_streamvort_time, libpg), Int32, (Ptr{Cvoid}, Int64, Ref{Float64}), s.handle, -1, t))
    s.time = t[]
    ns = Ref{Int64}(0)
    check(ccall((:pg_streamvort_num_states, libpg), Int32, (Ptr{Cvoid}, Ref{Int64}), s.handle, ns))
    for k in s.nstates_device:(ns[] - 1)
        check(ccall((:pg_streamvort_time, libpg), Int32, (Ptr{Cvoid}, Int64, Ref{Float64}), s.handle, k, t))
        push!(s.states, (time = t[], ψ = _sv_get(s, 0, k, 2n), ω = _sv_get(s, 1, k, 2n)))
    end
    s.nstates_device = Int(ns[])
    nothing
end
_sv_scheme(scheme::String) = scheme == "BE" ? Int32(0) : scheme == "CN" ? Int32(1) : error("Unknown scheme.")

"ConvectionOps(capacity, (u, v), [u; v]) of the current velocity (build_convection, :167-182), cached until the next ψ solve."
function build_convection(s::StreamVorticity{2})
    s.last_convection !== nothing && return s.last_convection
    u, v = s.velocity
    s.last_convection = ConvectionOps(s.capacity, (u, v), vcat(u, v))
end

function solve_StreamVorticity!(s::StreamVorticity; method = bicgstabl, algorithm = nothing, kwargs...)
    opts = Ref(_opts(method, kwargs))
    info = pg_step_info()
    _sv_push!(s)
    check(ccall((:pg_streamvort_solve_stream, libpg), Int32, (Ptr{Cvoid}, Ptr{pg_krylov_opts}, Ref{pg_step_info}), s.handle, opts, info))
    info.converged == 0 && @warn "PenguinHIP: the stream-function solve did not converge" iters = info.iters
    _sv_pull!(s)
    s.ψ
end

function step_StreamVorticity!(s::StreamVorticity; scheme::String = "BE", method = bicgstabl, algorithm = nothing, kwargs...)
    opts = Ref(_opts(method, kwargs))
    ip, iw = pg_step_info(), pg_step_info()
    _sv_push!(s)
    check(ccall((:pg_streamvort_step, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{pg_krylov_opts}, Ref{pg_step_info}, Ref{pg_step_info}),
                s.handle, _sv_scheme(scheme), opts, ip, iw))
    (ip.converged == 0 || iw.converged == 0) && @warn "PenguinHIP: a solve of the step did not converge" psi = ip.iters omega = iw.iters
    _sv_pull!(s)
    s.ω
end

# constant-in-time data (no closure among source and interface values takes part): the loop runs inside the library
_sv_constant(s::StreamVorticity) = !(s.bc_stream.value isa Function) && !(s.bc_vorticity.value isa Function) &&
                                   all(iszero, evalf(s.source, s.capacity.C_ω, s.time)) && !haskey(s.sent, :f_sent)

function run_StreamVorticity!(s::StreamVorticity, steps::Integer; scheme::String = "BE", method = bicgstabl, algorithm = nothing,
                              constant_data::Bool = _sv_constant(s), kwargs...)
    if !constant_data
        for _ in 1:steps
            step_StreamVorticity!(s; scheme = scheme, method = method, algorithm = algorithm, kwargs...)
        end
        return s
    end
    opts = Ref(_opts(method, kwargs))
    run = pg_streamvort_run_info()
    _sv_push!(s)
    check(ccall((:pg_streamvort_run, libpg), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{pg_krylov_opts}, Int32, Ptr{Cvoid}),
                s.handle, steps, _sv_scheme(scheme), opts, 1, pointer_from_objref(run)))
    run.unconverged > 0 && @warn "PenguinHIP: solves of the run did not converge" count = run.unconverged worst = run.worst_relres
    _sv_pull!(s)
    s
end

function run_until_StreamVorticity!(s::StreamVorticity, t_end::Float64; kwargs...)
    while s.time < t_end - 1e-12
        step_StreamVorticity!(s; kwargs...)
    end
    s
end

"Every PG_* tuning / variant selector the library runs with (`pg_config_string`)."
function config_string()
    buf = Vector{UInt8}(undef, 2048)
    check(ccall((:pg_config_string, libpg), Int32, (Ptr{UInt8}, Csize_t), buf, length(buf)))
    unsafe_string(pointer(buf))
end

"""
What the extrapolated start of the time loop's quiet steps is doing (`pg_solver_guess_info`): older states kept, the offsets
and coefficients the next step starts from, the sampled start residual without / with this step's extrapolation.
"""
function guess_info(s)
    kept = Ref{Int32}(0); ns = Ref{Int32}(0); ru = Ref{Float64}(0.0); rw = Ref{Float64}(0.0)
    off = zeros(Int32, 4); cf = zeros(Float64, 4)
    check(ccall((:pg_solver_guess_info, libpg), Int32,
                (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
                s.handle, kept, ns, off, cf, ru, rw))
    (kept = Int(kept[]), offsets = Int.(off[1:ns[]]), coef = cf[1:ns[]], rr_plain = ru[], rr_taken = rw[])
end

"""
The multigrid hierarchy of a solver's constructor system (`pg_solver_mg_info`): levels (0 before the first solve with
that `precond`), the first level of the fused tail, rows and nnz per level, set-up time, device memory.  `precond`: `:mg` or
`:mg_cell` -- a solver holds one hierarchy per value.
"""
function mg_info(s; precond=:mg)
    # pg_mg_info: int32 levels, int32 tail_level, int64 rows[16], int64 nnz[16], double setup_ms, int64 bytes = 35 words
    buf = zeros(Int64, 35)
    GC.@preserve buf begin
        check(ccall((:pg_solver_mg_info_for, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), s.handle, _precond_id(precond), pointer(buf)))
    end
    levels = Int(buf[1] & 0xffffffff); tail = Int((buf[1] >> 32) & 0xffffffff)
    (levels = levels, tail_level = tail, rows = buf[2:1 + levels], nnz = buf[18:17 + levels],
     setup_ms = reinterpret(Float64, buf[34]), bytes = buf[35])
end

function _mg_info_tuple(buf)
    levels = Int(buf[1] & 0xffffffff); tail = Int((buf[1] >> 32) & 0xffffffff)
    (levels = levels, tail_level = tail, rows = buf[2:1 + levels], nnz = buf[18:17 + levels],
     setup_ms = reinterpret(Float64, buf[34]), bytes = buf[35])
end

"""
The hierarchy of `precond = :mg_step` of system `which` (0 constructor, 1 run system; `pg_solver_mg_step_info`), as `mg_info`
reports it: levels = 0 while no solve with the option has run on that matrix.
"""
function mg_step_info(s, which::Integer=0)
    buf = zeros(Int64, 35)
    GC.@preserve buf begin
        check(ccall((:pg_solver_mg_step_info, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), s.handle, Int32(which), pointer(buf)))
    end
    _mg_info_tuple(buf)
end

"""
The spectral estimate behind `precond = :poly_est` of system `which` (0 constructor, 1 run system; `pg_solver_spectral_estimate`).
Runs the estimate if it has not run on that matrix; `run = false` only reports (`steps == 0`: none has run).
"""
function spectral_estimate(s, which::Integer=0; run::Bool=true)
    # pg_specest_info: int32 steps, admitted, gershgorin_admits, reserved; double g_ritz, g_used, margin, gershgorin,
    # ritz_re_min, ritz_re_max, ritz_im_max, estimate_ms = 10 words
    buf = zeros(Int64, 10)
    GC.@preserve buf begin
        check(ccall((:pg_solver_spectral_estimate, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), s.handle,
                    Int32(which | (run ? 0 : 4)), pointer(buf)))
    end
    f(k) = reinterpret(Float64, buf[k])
    (steps = Int(buf[1] & 0xffffffff), admitted = ((buf[1] >> 32) & 0xffffffff) != 0, gershgorin_admits = (buf[2] & 0xffffffff) != 0,
     g_ritz = f(3), g_used = f(4), margin = f(5), gershgorin = f(6), ritz_re_min = f(7), ritz_re_max = f(8), ritz_im_max = f(9),
     estimate_ms = f(10))
end

"`pg_krylov_opts.precond` of the virtual-rank diagnostic runs that follow (`:mg`, `:mg_cell` and `:mg_step` make them fail with the one-rank refusal)."
set_virtual_rank_precond(p) = check(ccall((:pg_debug_set_virtual_rank_precond, libpg), Int32, (Int32,), _precond_id(p)))

"One application z = M⁻¹ r of the multigrid V-cycle on host vectors (`pg_debug_mg_apply_for`; builds the hierarchy if need be)."
function mg_apply(s, r::Vector{Float64}; precond=:mg)
    z = zeros(Float64, length(r))
    check(ccall((:pg_debug_mg_apply_for, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, _precond_id(precond), r, z))
    z
end

"Aggregate map of `level` (`pg_debug_mg_aggregates`): the 0-based row of level + 1 every row of `level` belongs to."
function mg_aggregates(s, level::Integer)
    n = Ref{Int64}(0)
    check(ccall((:pg_debug_mg_aggregates, libpg), Int32, (Ptr{Cvoid}, Int32, Ref{Int64}, Ptr{Int32}), s.handle, level, n, C_NULL))
    agg = zeros(Int32, n[])
    check(ccall((:pg_debug_mg_aggregates, libpg), Int32, (Ptr{Cvoid}, Int32, Ref{Int64}, Ptr{Int32}), s.handle, level, n, agg))
    agg
end

"The matrix of `level` of the hierarchy (`pg_debug_mg_level_csr`) as a SparseMatrixCSC."
function mg_level_matrix(s, level::Integer)
    n = Ref{Int64}(0); nnz = Ref{Int64}(0)
    check(ccall((:pg_debug_mg_level_csr, libpg), Int32,
                (Ptr{Cvoid}, Int32, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                s.handle, level, n, nnz, C_NULL, C_NULL, C_NULL))
    rowptr = zeros(Int64, n[] + 1); col = zeros(Int64, max(nnz[], 1)); val = zeros(Float64, max(nnz[], 1))
    check(ccall((:pg_debug_mg_level_csr, libpg), Int32,
                (Ptr{Cvoid}, Int32, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                s.handle, level, n, nnz, rowptr, col, val))
    rows = [i for i in 1:n[] for _ in rowptr[i] + 1:rowptr[i + 1]]
    sparse(rows, col[1:nnz[]] .+ 1, val[1:nnz[]], n[], n[])
end

"One application z = M⁻¹ r of the `:mg_step` V-cycle of system `which` (`pg_debug_mg_step_apply`; builds the hierarchy if need be)."
function mg_step_apply(s, which::Integer, r::Vector{Float64})
    z = zeros(Float64, length(r))
    check(ccall((:pg_debug_mg_step_apply, libpg), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), s.handle, Int32(which), r, z))
    z
end

"Aggregate map of `level` of the `:mg_step` hierarchy of system `which` (`pg_debug_mg_step_aggregates`), 0-based rows of level + 1."
function mg_step_aggregates(s, which::Integer, level::Integer)
    n = Ref{Int64}(0)
    check(ccall((:pg_debug_mg_step_aggregates, libpg), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int64}, Ptr{Int32}),
                s.handle, Int32(which), Int32(level), n, C_NULL))
    agg = zeros(Int32, n[])
    check(ccall((:pg_debug_mg_step_aggregates, libpg), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int64}, Ptr{Int32}),
                s.handle, Int32(which), Int32(level), n, agg))
    agg
end

"The matrix of `level` of the `:mg_step` hierarchy of system `which` (`pg_debug_mg_step_level_csr`) as a SparseMatrixCSC."
function mg_step_level_matrix(s, which::Integer, level::Integer)
    n = Ref{Int64}(0); nnz = Ref{Int64}(0)
    check(ccall((:pg_debug_mg_step_level_csr, libpg), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                s.handle, Int32(which), Int32(level), n, nnz, C_NULL, C_NULL, C_NULL))
    rowptr = zeros(Int64, n[] + 1); col = zeros(Int64, max(nnz[], 1)); val = zeros(Float64, max(nnz[], 1))
    check(ccall((:pg_debug_mg_step_level_csr, libpg), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                s.handle, Int32(which), Int32(level), n, nnz, rowptr, col, val))
    rows = [i for i in 1:n[] for _ in rowptr[i] + 1:rowptr[i + 1]]
    sparse(rows, col[1:nnz[]] .+ 1, val[1:nnz[]], n[], n[])
end

end # module
