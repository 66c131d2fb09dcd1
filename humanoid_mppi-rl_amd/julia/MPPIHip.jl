"""
    MPPIHip

Julia `ccall` binding of libmppi_hip.so (include/mppi.h) that reproduces the reference's Julia controller API:

    mppi_step!(m, d)         src/Humanoid_mppi_v3.jl:154-171, src/cartpole_mppi.jl:103-115
    mppi_controller!(m, d)   src/Humanoid_mppi_v3.jl:173-179  (the `controller=` callback of visualise!)
    mppi_update!(m, d)       src/mppi.jl:83-99

so a reference script switches with

    using MPPIHip
    ctl = MPPIHip.Controller("humanoid_v3"; dynamics = :cross_attention, weights = "ca_humanoid.blob")
    visualise!(model, data; controller = (m, d) -> MPPIHip.mppi_controller!(ctl, m, d))

The humanoid costs read the REAL environment's kinematics on every call (src/Humanoid_mppi_v3.jl:53-99 reads the
global `data`'s cvel / xpos; src/Humanoid_mppi.jl:89-106 its xpos).  Every humanoid solve therefore builds the
per-solve context row from `d` with the reference's own index expressions (`humanoid_v3_context`,
`humanoid_v1_context`, evaluated on MuJoCo.jl's arrays exactly as the reference evaluates them) and passes it
through mppi_solve_ex.  Body ids come from MuJoCo.body(m, name).id on the first call (or `body_ids=` at
construction).

Arrays stay in Julia's column-major layout: U is (nu, H) and injected noise (nu, H, K), passed with
MPPI_FLAG_COLMAJOR. The engine computes in Float32 (Float64 states are converted at the boundary; that
conversion is part of the parity tolerance, DESIGN.md). Untested in this build image (no Julia toolchain).
"""
module MPPIHip

const LIB = get(ENV, "MPPI_HIP_LIB", joinpath(@__DIR__, "..", "lib", "libmppi_hip.so"))

const DYN_CARTPOLE, DYN_MLP, DYN_CROSS_ATTN, DYN_FEATURE_ATTN = Cint(1), Cint(2), Cint(3), Cint(4)
const COST = Dict(:cartpole => Cint(1), :cartpole_est => Cint(2), :humanoid_v3 => Cint(3),
                  :quad_jl => Cint(4), :quad_est => Cint(5), :humanoid_v1 => Cint(6))
const FLAG_SHIFT, FLAG_COLMAJOR, FLAG_U0_BEFORE = Cint(0x1), Cint(0x2), Cint(0x10)
const FLAG_STATS = Cint(0x200)   # also compute the solve's diagnostics (solve_stats)
const FLAG_CROSS = Cint(0x400)   # ... and the weighted cross moments of its noise (cross_moments); implies FLAG_STATS
const FLAG_STEP_MOMENTS = Cint(0x800)   # ... and the weighted per-step moments (step_moments); implies FLAG_STATS
const CTX_MAX = 8

# must match `mppi_io` in include/mppi.h (7 pointers)
struct MPPIIo
    x0::Ptr{Float32}; U::Ptr{Float32}; noise::Ptr{Float32}; costs::Ptr{Float32}
    weights::Ptr{Float32}; u0::Ptr{Float32}; ctx::Ptr{Float32}
end

# must match `mppi_config` in include/mppi.h field for field
mutable struct Config
    nx::Int32; nu::Int32; H::Int32; K::Int32; max_batch::Int32
    lambda::Float32; sigma::Float32; ctrl_clamp::Float32; U_clamp::Float32; norm_eps::Float32
    shift_fill::Float32; terminal_weight::Float32; update_mode::Int32; precision::Int32
    r0::Int32; r1::Int32; r2::Int32; r3::Int32
    Config() = new(0, 0, 0, 0, 0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0, 0, 0, 0, 0, 0)
end

# must match `mppi_solve_stats` in include/mppi.h field for field (40 bytes)
struct SolveStats
    cost_min::Float32; cost_max::Float32; cost_mean::Float32; cost_std::Float32
    cost_weighted::Float32; ess::Float32; entropy::Float32; free_energy::Float32
    n_finite::Int32; k_best::Int32
end

struct MPPIError <: Exception
    code::Cint
    msg::String
end
Base.showerror(io::IO, e::MPPIError) = print(io, "MPPI error ", e.code, ": ", e.msg)

function check(rc::Cint)
    rc == 0 && return rc
    throw(MPPIError(rc, unsafe_string(ccall((:mppi_last_error, LIB), Cstring, ()))))
end

function preset(name::AbstractString; kw...)
    cfg = Config()
    check(ccall((:mppi_preset, LIB), Cint, (Cstring, Ref{Config}), name, cfg))
    for (k, v) in kw
        setfield!(cfg, k, convert(fieldtype(Config, k), v))
    end
    return cfg
end

mutable struct Controller
    handle::Ptr{Cvoid}
    cfg::Config
    preset::String
    U::Matrix{Float32}          # nominal sequence (nu, H): the reference's U_global
    seed::UInt64
    calls::UInt64
    ctx::Vector{Float32}        # per-solve cost context (humanoid real-env terms), CTX_MAX floats
    cost::Symbol
    body_ids::Any               # (shin_left, shin_right, foot_left, foot_right) 0-based MuJoCo ids, or nothing
    u0_before::Bool             # src/quadruped_datacollection.py:170: apply U[:,1] before the update
end

"""
    Controller(preset; dynamics=:cartpole, weights=nothing, cost=nothing, device=0, seed=0, kw...)

`weights` is a weight blob written by mppi_hip.nets.pack_blob (Python) for :mlp / :cross_attention.
"""
function Controller(name::AbstractString; dynamics::Symbol = :cartpole, weights = nothing, cost = nothing,
                    device::Integer = 0, seed::Integer = 0, body_ids = nothing, u0_before::Bool = false, kw...)
    cfg = preset(name; kw...)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mppi_create, LIB), Cint, (Ref{Config}, Cint, Ref{Ptr{Cvoid}}), cfg, device, h))
    ck = cost === nothing ? (name == "humanoid_v1" ? :humanoid_v1 : startswith(name, "humanoid") ? :humanoid_v3 :
                             startswith(name, "quad") ? :quad_jl : endswith(name, "_est") ? :cartpole_est :
                             :cartpole) : cost
    c = Controller(h[], cfg, String(name), zeros(Float32, cfg.nu, cfg.H), UInt64(seed), 0,
                   zeros(Float32, CTX_MAX), ck, body_ids, u0_before)
    finalizer(c -> ccall((:mppi_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.handle), c)
    if dynamics == :cartpole
        check(ccall((:mppi_load_dynamics, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), c.handle,
                    DYN_CARTPOLE, C_NULL, 0))
    else
        blob = read(weights)
        kind = dynamics == :mlp ? DYN_MLP : dynamics == :feature_attention ? DYN_FEATURE_ATTN : DYN_CROSS_ATTN
        check(ccall((:mppi_load_dynamics, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}, Csize_t), c.handle, kind,
                    blob, length(blob)))
    end
    check(ccall((:mppi_set_cost, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Cint), c.handle, COST[ck],
                C_NULL, 0))
    return c
end

state(d) = Float32.(vcat(vec(d.qpos), vec(d.qvel)))

# src/Humanoid_mppi_v3.jl:22-25, verbatim in meaning: the flat index into MuJoCo.jl's cvel array
get_body_vx(d, body_id) = d.cvel[body_id * 6 - 5 + 3]

"0-based MuJoCo body ids the humanoid costs read, via MuJoCo.body(m, name).id (the reference's own lookups)."
function humanoid_body_ids(m)
    mj = getfield(Main, :MuJoCo)
    bid(n) = Base.invokelatest(mj.body, m, n).id
    return (shin_left = bid("shin_left"), shin_right = bid("shin_right"), foot_left = bid("foot_left"),
            foot_right = bid("foot_right"))
end

"""Context row of MPPI_COST_HUMANOID_V3 from the real environment `d`: src/Humanoid_mppi_v3.jl:53-99 evaluated
as the reference evaluates it (cvel / xpos of the global data), [2, 0, 1.28, swing_foot_x, swing_knee_x, const,
0, 0] with const = -0.15 swing_vx + 2 clr^2 [clr < 0.05] + 0.5 lat^2 [lat < 0] (the terms constant over k, t)."""
function humanoid_v3_context(d, ids)
    if get_body_vx(d, ids.shin_left) > get_body_vx(d, ids.shin_right)
        swing, stance, knee = ids.foot_left, ids.foot_right, ids.shin_left
    else
        swing, stance, knee = ids.foot_right, ids.foot_left, ids.shin_right
    end
    k = -0.15 * get_body_vx(d, swing)                                  # :78-79
    clearance = d.xpos[swing + 1, 3] - d.xpos[stance + 1, 3]           # :86-91
    clearance < 0.05 && (k += 2.0 * abs2(clearance))
    lateral = d.xpos[ids.foot_left + 1, 2] - d.xpos[ids.foot_right + 1, 2]  # :93-99
    lateral < 0 && (k += 0.5 * abs2(lateral))
    return Float32[2.0, 0.0, 1.28, d.xpos[swing + 1, 1], d.xpos[knee + 1, 1], k, 0, 0]
end

"""Context row of MPPI_COST_HUMANOID_V1 (src/Humanoid_mppi.jl:89-106): [2, 0, 1.28, left_foot_x, right_foot_x,
0.01 (right_z - left_z), 0.1 |left_y - right_y|, 0]; the kernel picks the swing side per rollout step t."""
function humanoid_v1_context(d, ids)
    l, r = ids.foot_left + 1, ids.foot_right + 1
    return Float32[2.0, 0.0, 1.28, d.xpos[l, 1], d.xpos[r, 1], 0.01 * (d.xpos[r, 3] - d.xpos[l, 3]),
                   0.1 * abs(d.xpos[l, 2] - d.xpos[r, 2]), 0]
end

function _context!(c::Controller, m, d)
    (c.cost == :humanoid_v3 || c.cost == :humanoid_v1) || return C_NULL
    c.body_ids === nothing && (c.body_ids = humanoid_body_ids(m))
    c.ctx .= c.cost == :humanoid_v3 ? humanoid_v3_context(d, c.body_ids) : humanoid_v1_context(d, c.body_ids)
    return pointer(c.ctx)
end

# (`stats = true` of mppi_step! / mppi_controller! adds FLAG_STATS here; solve_stats reads the result)
function _solve!(c::Controller, m, d; flags::Cint = Cint(0), noise = nothing)
    x0 = state(d)
    u0 = zeros(Float32, c.cfg.nu)
    c.calls += 1
    seed = xor(c.seed << 32, c.calls)
    nz = noise === nothing ? Float32[] : Float32.(noise)   # (nu, H, K) column-major, already scaled
    GC.@preserve x0 u0 nz c begin
        io = MPPIIo(pointer(x0), pointer(c.U), noise === nothing ? C_NULL : pointer(nz), C_NULL, C_NULL,
                    pointer(u0), _context!(c, m, d))
        check(ccall((:mppi_solve_ex, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{MPPIIo}, UInt64, Cint),
                    c.handle, 1, io, seed, flags | FLAG_COLMAJOR))
    end
    return u0
end

"mppi_step!: noise -> rollout -> softmin -> U update (no shift); U_global kept in `c.U`."
mppi_step!(c::Controller, m, d; noise = nothing, stats::Bool = false) =
    (_solve!(c, m, d; flags = stats ? FLAG_STATS : Cint(0), noise = noise); nothing)

"mppi_controller!: mppi_step!, then d.ctrl .= U[:,1] and the receding-horizon shift (0.1 decay or zero fill)."
function mppi_controller!(c::Controller, m, d; noise = nothing, stats::Bool = false)
    flags = FLAG_SHIFT | (c.u0_before ? FLAG_U0_BEFORE : Cint(0)) | (stats ? FLAG_STATS : Cint(0))
    u0 = _solve!(c, m, d; flags = flags, noise = noise)
    d.ctrl .= u0
    return nothing
end

mppi_update!(c::Controller, m, d; kw...) = mppi_controller!(c, m, d; kw...)

"x3_layer1: (products, probe error) of the split CA's layer 1 (mppi_x3_layer1; ABI 3)."
function x3_layer1(c::Controller)
    prod = Ref{Cint}(0)
    err = Ref{Cfloat}(0)
    check(ccall((:mppi_x3_layer1, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cfloat}), c.handle, prod, err))
    return (Int(prod[]), Float32(err[]))
end

"""
    set_noise_model!(c; sigma_u = nothing, rho = 0.0)

The sampling law of the device noise (mppi_set_noise_model): per-actuator standard deviations `sigma_u` (length nu;
`nothing` = the preset's sigma for all) and the AR(1) correlation `rho` in [0, 1) along the horizon.
`set_noise_model!(c)` restores the default white noise.
"""
function set_noise_model!(c::Controller; sigma_u = nothing, rho::Real = 0.0)
    if sigma_u === nothing
        check(ccall((:mppi_set_noise_model, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat), c.handle, C_NULL, rho))
    else
        s = Float32.(vec(collect(sigma_u)))
        length(s) == c.cfg.nu || throw(ArgumentError("sigma_u must have nu = $(c.cfg.nu) entries"))
        GC.@preserve s check(ccall((:mppi_set_noise_model, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat), c.handle,
                                   pointer(s), rho))
    end
    return c
end

"""
    set_noise_adapt!(c, rate; sigma_min = 1e-3, sigma_max = 10.0, rho_max = 0.95)

Adapt the sampling law on the device behind every solve (mppi_set_noise_adapt): `rate` in (0, 1] enables, 0 disables
and keeps the law as it stands.  Chained solves and graph streams adapt step by step with no host round trip.
"""
function set_noise_adapt!(c::Controller, rate::Real; sigma_min::Real = 1e-3, sigma_max::Real = 10.0,
                          rho_max::Real = 0.95)
    check(ccall((:mppi_set_noise_adapt, LIB), Cint, (Ptr{Cvoid}, Cfloat, Cfloat, Cfloat, Cfloat), c.handle, rate,
                sigma_min, sigma_max, rho_max))
    return c
end

"""
    noise_adapt(c) -> (rate, sigma_min, sigma_max, rho_max)

The settings of `set_noise_adapt!` (mppi_get_noise_adapt); `rate` is 0 while adaptation is off.
"""
function noise_adapt(c::Controller)
    v = [Ref{Cfloat}(0) for _ in 1:4]
    check(ccall((:mppi_get_noise_adapt, LIB), Cint, (Ptr{Cvoid}, Ref{Cfloat}, Ref{Cfloat}, Ref{Cfloat}, Ref{Cfloat}),
                c.handle, v[1], v[2], v[3], v[4]))
    return (v[1][], v[2][], v[3][], v[4][])
end

"""
    noise_law(c; step = 0) -> (sigma_u::Vector{Float32}, rho::Float32)

The law the adapting solve `step` drew its noise from (mppi_get_noise_law; waits for the stream).
"""
function noise_law(c::Controller; step::Integer = 0)
    s = zeros(Float32, c.cfg.nu)
    rho = Ref{Cfloat}(0)
    GC.@preserve s check(ccall((:mppi_get_noise_law, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Ref{Cfloat}),
                               c.handle, step, pointer(s), rho))
    return (s, rho[])
end

"""
    set_noise_knots!(c, n_knots; order = 1)

Knot-parameterised sampling noise (mppi_set_noise_knots): the device noise is drawn at `n_knots` knots along the horizon
(1..H) and interpolated, `order` 0 (hold), 1 (linear) or 3 (Catmull-Rom).  `n_knots = 0` disables and keeps sigma_u and
rho.  Not together with `set_control_cost!` or `set_noise_adapt!`.
"""
function set_noise_knots!(c::Controller, n_knots::Integer; order::Integer = 1)
    check(ccall((:mppi_set_noise_knots, LIB), Cint, (Ptr{Cvoid}, Cint, Cint), c.handle, n_knots, order))
    return c
end

"""
    noise_knots(c) -> (n_knots, order, idx::Matrix{Int32}, w::Matrix{Float32})

The knot law and its table, four taps per horizon step as (4, H) column-major arrays (mppi_get_noise_knots; 0-based knot
indices as in C); `n_knots` is 0 and the arrays are zero while the law is off.
"""
function noise_knots(c::Controller)
    n = Ref{Cint}(0)
    order = Ref{Cint}(0)
    idx = zeros(Int32, 4, c.cfg.H)
    w = zeros(Float32, 4, c.cfg.H)
    GC.@preserve idx w check(ccall((:mppi_get_noise_knots, LIB), Cint,
                                   (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ptr{Int32}, Ptr{Float32}), c.handle, n, order,
                                   pointer(idx), pointer(w)))
    return (Int(n[]), Int(order[]), idx, w)
end

"""
    set_noise_basis!(c, M)

Horizon-basis sampling noise (mppi_set_noise_basis): the device noise of one sample is `M` (H x R, indexed [t, r],
1 <= R <= min(H, 128), finite) applied along the horizon to R white normals and scaled by sigma_u -- coloured noise,
temporal kernels, spline or cosine bases.  `nothing` disables and keeps sigma_u.  Not together with rho != 0,
`set_noise_knots!`, `set_noise_cov!`, `set_noise_adapt!` or `set_control_cost!`.
"""
function set_noise_basis!(c::Controller, M::Union{Nothing, AbstractMatrix})
    if M === nothing
        check(ccall((:mppi_set_noise_basis, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 0, C_NULL))
        return c
    end
    size(M, 1) == c.cfg.H || throw(ArgumentError("M must be H x R"))
    A = Matrix{Float32}(permutedims(M))   # the C ABI's [H][R] is row-major
    GC.@preserve A check(ccall((:mppi_set_noise_basis, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle,
                               size(M, 2), pointer(A)))
    return c
end

"""
    noise_basis(c) -> M::Matrix{Float32} or nothing

The table of the handle's basis law as set (mppi_get_noise_basis), H x R indexed [t, r] as in C; `nothing` while the
law is off.
"""
function noise_basis(c::Controller)
    n = Ref{Cint}(0)
    check(ccall((:mppi_get_noise_basis, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float32}), c.handle, n, C_NULL))
    n[] == 0 && return nothing
    A = zeros(Float32, Int(n[]), c.cfg.H)
    GC.@preserve A check(ccall((:mppi_get_noise_basis, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float32}), c.handle, n,
                               pointer(A)))
    return permutedims(A)   # row-major C -> [t, r]
end

"""
    set_noise_steps!(c, S)

A sampling scale per actuator and horizon step (mppi_set_noise_steps): `eps[u, t, k] = S[u, t] * e[t]` with `e` the
handle's unit-variance AR(1) row -- the distribution of CEM / iCEM.  `S` is nu x H, finite and >= 0; every batch slot of
the handle takes it.  `nothing` disables and keeps sigma_u and rho.  While on, sigma_u is the scale a step entering the
horizon starts with.  Not together with `set_noise_knots!`, `set_noise_basis!`, `set_noise_cov!`, `set_noise_adapt!`
or `set_control_cost!`.
"""
function set_noise_steps!(c::Controller, S::Union{Nothing, AbstractMatrix})
    if S === nothing
        check(ccall((:mppi_set_noise_steps, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 0, C_NULL))
        return c
    end
    size(S) == (c.cfg.nu, c.cfg.H) || throw(ArgumentError("S must be nu x H"))
    A = Matrix{Float32}(permutedims(S))   # the C ABI's [nu][H] is row-major
    GC.@preserve A check(ccall((:mppi_set_noise_steps, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 1,
                               pointer(A)))
    return c
end

"""
    noise_steps(c) -> S::Matrix{Float32} or nothing

The live table of the handle's per-step scales (mppi_get_noise_steps; waits for the stream), nu x H indexed [u, t];
`nothing` while the law is off.
"""
function noise_steps(c::Controller)
    active = Ref{Cint}(0)
    A = zeros(Float32, c.cfg.H, c.cfg.nu)
    GC.@preserve A check(ccall((:mppi_get_noise_steps, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Ref{Cint}),
                               c.handle, 1, pointer(A), active))
    return active[] == 0 ? nothing : permutedims(A)   # row-major C -> [u, t]
end

"""
    set_noise_steps_adapt!(c, rate; sigma_min = 1f-3, sigma_max = 10f0, centred = true)

Refit the table on the device behind every solve from the solve's own per-step moments and shift it with the nominal
(mppi_set_noise_steps_adapt): CEM's variance update with momentum.  `rate` in (0, 1] enables (needs `set_noise_steps!`
first), 0 disables and keeps the table as it stands.
"""
function set_noise_steps_adapt!(c::Controller, rate::Real; sigma_min::Real = 1f-3, sigma_max::Real = 10f0,
                                centred::Bool = true)
    check(ccall((:mppi_set_noise_steps_adapt, LIB), Cint, (Ptr{Cvoid}, Cfloat, Cfloat, Cfloat, Cint), c.handle,
                Float32(rate), Float32(sigma_min), Float32(sigma_max), centred ? 1 : 0))
    return c
end

"""
    step_moments(c, step = 0) -> (m1, m2)

The weighted per-step moments of the last solve made with FLAG_STEP_MOMENTS or with the refit on
(mppi_get_step_moments): `sum_k w_k eps` and `sum_k w_k eps^2`, each nu x H indexed [u, t].
"""
function step_moments(c::Controller, step::Integer = 0)
    m1 = zeros(Float32, c.cfg.H, c.cfg.nu)
    m2 = zeros(Float32, c.cfg.H, c.cfg.nu)
    GC.@preserve m1 m2 check(ccall((:mppi_get_step_moments, LIB), Cint,
                                   (Ptr{Cvoid}, Cint, Cint, Ptr{Float32}, Ptr{Float32}), c.handle, 1, step,
                                   pointer(m1), pointer(m2)))
    return (permutedims(m1), permutedims(m2))
end

"""
    set_noise_cov!(c, Sigma)

Cross-actuator sampling covariance (mppi_set_noise_cov): the device noise of one step is drawn with the full covariance
`Sigma` (nu x nu, Float32: symmetric bit for bit, positive definite), `eps[:, t, k] = L e[:, t, k]` with
`Sigma = L L'` and `e` the handle's unit-variance AR(1) rows.  `nothing` disables and keeps sigma_u = sqrt(diag Sigma)
and rho.  Not together with `set_noise_knots!` or `set_noise_adapt!`.
"""
function set_noise_cov!(c::Controller, Sigma::Union{Nothing, AbstractMatrix})
    if Sigma === nothing
        check(ccall((:mppi_set_noise_cov, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), c.handle, C_NULL))
        return c
    end
    size(Sigma) == (c.cfg.nu, c.cfg.nu) || throw(ArgumentError("Sigma must be nu x nu"))
    S = Matrix{Float32}(permutedims(Sigma))   # the C ABI's [nu][nu] is row-major
    GC.@preserve S check(ccall((:mppi_set_noise_cov, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), c.handle, pointer(S)))
    return c
end

"""
    noise_cov(c) -> (Sigma, L, Sinv) or nothing

The handle's covariance as given, its lower Cholesky factor and its inverse (mppi_get_noise_cov), nu x nu Float32
matrices indexed [u, v] as in C; `nothing` while the law is off.
"""
function noise_cov(c::Controller)
    nu = c.cfg.nu
    S = zeros(Float32, nu, nu)
    L = zeros(Float32, nu, nu)
    Si = zeros(Float32, nu, nu)
    active = Ref{Cint}(0)
    GC.@preserve S L Si check(ccall((:mppi_get_noise_cov, LIB), Cint,
                                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Cint}), c.handle,
                                    pointer(S), pointer(L), pointer(Si), active))
    active[] == 0 && return nothing
    return (permutedims(S), permutedims(L), permutedims(Si))   # row-major C -> [u, v]
end

"""
    set_noise_cov_adapt!(c, rate; sigma_min = 1f-3, sigma_max = 10f0)

Adapt the full sampling covariance on the device behind every solve (mppi_set_noise_cov_adapt): Sigma moves towards the
weighted cross moments of the solve's noise, its standard deviations are clipped to [sigma_min, sigma_max] with the
correlations kept, and L and Sigma^-1 are factored again on the device.  `rate` in (0, 1] enables (after
`set_noise_cov!`), 0 disables and keeps the law as it stands.
"""
function set_noise_cov_adapt!(c::Controller, rate::Real; sigma_min::Real = 1f-3, sigma_max::Real = 10f0)
    check(ccall((:mppi_set_noise_cov_adapt, LIB), Cint, (Ptr{Cvoid}, Cfloat, Cfloat, Cfloat), c.handle,
                Float32(rate), Float32(sigma_min), Float32(sigma_max)))
    return c
end

"""
    noise_cov_adapt(c) -> (rate, sigma_min, sigma_max, rejects)

The settings of mppi_get_noise_cov_adapt (rate 0 while off) and the number of steps the device rejected.
"""
function noise_cov_adapt(c::Controller)
    r, lo, hi = Ref{Cfloat}(0), Ref{Cfloat}(0), Ref{Cfloat}(0)
    n = Ref{UInt64}(0)
    check(ccall((:mppi_get_noise_cov_adapt, LIB), Cint,
                (Ptr{Cvoid}, Ref{Cfloat}, Ref{Cfloat}, Ref{Cfloat}, Ref{UInt64}), c.handle, r, lo, hi, n))
    return (r[], lo[], hi[], Int(n[]))
end

"""
    noise_cov_law(c, step = 0) -> Matrix{Float32}

The Sigma (nu x nu, indexed [u, v]) the adapting solve `step` drew its noise from (mppi_get_noise_cov_law).
"""
function noise_cov_law(c::Controller, step::Integer = 0)
    nu = c.cfg.nu
    S = zeros(Float32, nu, nu)
    GC.@preserve S check(ccall((:mppi_get_noise_cov_law, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle,
                               Cint(step), pointer(S)))
    return permutedims(S)
end

"""
    cross_moments(c, step = 0) -> Matrix{Float32}

The weighted cross moments eps_mx (nu x nu, symmetric) of the last solve made with `FLAG_CROSS`
(mppi_get_cross_moments): 1/H sum_t sum_k w_k eps_u eps_v; its diagonal is eps_m2.
"""
function cross_moments(c::Controller, step::Integer = 0)
    nu = c.cfg.nu
    mx = zeros(Float32, nu, nu)
    GC.@preserve mx check(ccall((:mppi_get_cross_moments, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float32}),
                                c.handle, Cint(1), Cint(step), pointer(mx)))
    return mx   # (symmetric: row-major C == column-major)
end

"""
    cross_moments_eval(c, costs, noise) -> Matrix{Float32}

The same kernels on host arrays (mppi_cross_moments_eval): `costs` (K), `noise` (nu, H, K) column-major as everywhere
in this module.  Touches no solve state and never adapts.
"""
function cross_moments_eval(c::Controller, costs::AbstractVector, noise::AbstractArray{<:Real, 3})
    nu, H, K = c.cfg.nu, c.cfg.H, c.cfg.K
    (length(costs) == K && size(noise) == (nu, H, K)) || throw(ArgumentError("costs (K), noise (nu, H, K)"))
    cs = Vector{Float32}(costs)
    nz = Array{Float32}(permutedims(noise, (3, 2, 1)))   # C's [nu][H][K]: K fastest
    mx = zeros(Float32, nu, nu)
    GC.@preserve cs nz mx check(ccall((:mppi_cross_moments_eval, LIB), Cint,
                                      (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), c.handle, Cint(1),
                                      pointer(cs), pointer(nz), pointer(mx)))
    return mx
end

"""
    noise_eval(c, seed) -> Array{Float32, 3}

The noise (nu, H, K), column-major as everywhere in this module, that the handle's generator draws for the key `seed`
under the law in effect (mppi_noise_eval): a solve's noise for that key, ahead of bounds and kept elites.
"""
function noise_eval(c::Controller, seed::Integer)
    nz = zeros(Float32, c.cfg.K, c.cfg.H, c.cfg.nu)   # the C ABI's [nu][H][K]: k fastest
    GC.@preserve nz check(ccall((:mppi_noise_eval, LIB), Cint, (Ptr{Cvoid}, Cint, UInt64, Ptr{Float32}), c.handle, 1,
                                UInt64(seed), pointer(nz)))
    return permutedims(nz, (3, 2, 1))
end

"""
    set_ess_target!(c, ess_frac; lambda_min = 1e-3, lambda_max = 1e3)

Choose the softmin temperature on the device, per solve, so that the solve's own costs give the effective sample size
max(1, ess_frac * n_finite), within [lambda_min, lambda_max] (mppi_set_ess_target): `ess_frac` in (0, 1] enables, 0
disables and the configured lambda runs again.
"""
function set_ess_target!(c::Controller, ess_frac::Real; lambda_min::Real = 1e-3, lambda_max::Real = 1e3)
    check(ccall((:mppi_set_ess_target, LIB), Cint, (Ptr{Cvoid}, Cfloat, Cfloat, Cfloat), c.handle, ess_frac,
                lambda_min, lambda_max))
    return c
end

"""
    ess_target(c) -> (ess_frac, lambda_min, lambda_max)

The settings of `set_ess_target!` (mppi_get_ess_target); `ess_frac` is 0 while targeting is off.
"""
function ess_target(c::Controller)
    v = [Ref{Cfloat}(0) for _ in 1:3]
    check(ccall((:mppi_get_ess_target, LIB), Cint, (Ptr{Cvoid}, Ref{Cfloat}, Ref{Cfloat}, Ref{Cfloat}), c.handle,
                v[1], v[2], v[3]))
    return (v[1][], v[2][], v[3][])
end

"""
    solve_lambda(c; step = 0) -> Float32

The lambda the targeting solve `step` updated with (mppi_get_lambda; waits for the stream).
"""
function solve_lambda(c::Controller; step::Integer = 0)
    lam = zeros(Float32, 1)
    GC.@preserve lam check(ccall((:mppi_get_lambda, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float32}), c.handle, 1,
                                 step, pointer(lam)))
    return lam[1]
end

"""
    lambda_eval(c, costs) -> Float32

The search kernel on a given cost vector (length K; non-finite entries allowed) (mppi_lambda_eval); needs targeting
enabled.
"""
function lambda_eval(c::Controller, costs)
    cs = Float32.(vec(collect(costs)))
    length(cs) == c.cfg.K || throw(ArgumentError("costs must have K = $(c.cfg.K) entries"))
    lam = zeros(Float32, 1)
    GC.@preserve cs lam check(ccall((:mppi_lambda_eval, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}),
                                    c.handle, 1, pointer(cs), pointer(lam)))
    return lam[1]
end

"""
    set_control_cost!(c, gamma)

Add the control-cost term of information-theoretic MPPI, `gamma * sum U Sigma^-1 eps`, to the costs the softmin weighs
(mppi_set_control_cost): a finite `gamma > 0` (cost units, absolute) enables, 0 disables.  Any change destroys captured
graphs; a prefetched noise is kept.
"""
function set_control_cost!(c::Controller, gamma::Real)
    check(ccall((:mppi_set_control_cost, LIB), Cint, (Ptr{Cvoid}, Cfloat), c.handle, gamma))
    return c
end

"""
    control_cost(c) -> Float32

`gamma` of `set_control_cost!` (mppi_get_control_cost); 0 while the term is off.
"""
function control_cost(c::Controller)
    g = Ref{Cfloat}(0)
    check(ccall((:mppi_get_control_cost, LIB), Cint, (Ptr{Cvoid}, Ref{Cfloat}), c.handle, g))
    return g[]
end

"""
    control_term(c) -> (term::Vector{Float32}, lin::Matrix{Float32})

The term (length K) and its coefficients `lin` (nu, H) of the last solve made with the term on
(mppi_get_control_term; waits for the stream).
"""
function control_term(c::Controller)
    term = zeros(Float32, c.cfg.K)
    lin = zeros(Float32, c.cfg.H, c.cfg.nu)  # the library's [nu][H], row-major
    GC.@preserve term lin check(ccall((:mppi_get_control_term, LIB), Cint,
                                      (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}), c.handle, 1, pointer(term),
                                      pointer(lin)))
    return (term, permutedims(lin))
end

"""
    control_term_eval(c, U, noise) -> (term::Vector{Float32}, lin::Matrix{Float32})

The term's kernels on a given `U` (nu, H) and `noise` (nu, H, K) with the handle's current law and gamma
(mppi_control_term_eval); needs the term enabled.
"""
function control_term_eval(c::Controller, U, noise)
    nu, H, K = c.cfg.nu, c.cfg.H, c.cfg.K
    size(U) == (nu, H) || throw(ArgumentError("U must be ($nu, $H)"))
    size(noise) == (nu, H, K) || throw(ArgumentError("noise must be ($nu, $H, $K)"))
    Ur = Float32.(permutedims(U))                  # (H, nu) column-major = the library's [nu][H]
    nz = Float32.(permutedims(noise, (3, 2, 1)))   # (K, H, nu) column-major = the library's [nu][H][K]
    term = zeros(Float32, K)
    lin = zeros(Float32, H, nu)
    GC.@preserve Ur nz term lin check(ccall((:mppi_control_term_eval, LIB), Cint,
                                            (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                            c.handle, 1, pointer(Ur), pointer(nz), pointer(term), pointer(lin)))
    return (term, permutedims(lin))
end

"""
    set_control_bounds!(c, lo, hi)

Keep every sampled control `U + eps` and the nominal `U` inside the box `[lo[u], hi[u]]` (mppi_set_control_bounds): the
solve's noise is projected on the device ahead of the rollout, `U` and `u0` are clipped behind the update.  `lo`, `hi`:
numbers or length-nu vectors (the columns of a model's `actuator_ctrlrange`); `nothing` leaves that side unbounded,
`(nothing, nothing)` disables.  Any change destroys captured graphs; a prefetched noise is kept.  Needs nu <= 32.
"""
function set_control_bounds!(c::Controller, lo, hi)
    nu = c.cfg.nu
    side(v) = v === nothing ? nothing : (v isa Real ? fill(Float32(v), nu) : Float32.(vec(collect(v))))
    l, h = side(lo), side(hi)
    (l === nothing || length(l) == nu) && (h === nothing || length(h) == nu) ||
        throw(ArgumentError("lo and hi must be numbers or have nu = $nu entries"))
    GC.@preserve l h check(ccall((:mppi_set_control_bounds, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}),
                                 c.handle, l === nothing ? Ptr{Float32}(C_NULL) : pointer(l),
                                 h === nothing ? Ptr{Float32}(C_NULL) : pointer(h)))
    return c
end

"""
    control_bounds(c) -> (lo::Vector{Float32}, hi::Vector{Float32}, active::Bool)

The box of `set_control_bounds!` (mppi_get_control_bounds); -Inf / Inf while the bounds are off.
"""
function control_bounds(c::Controller)
    lo, hi = zeros(Float32, c.cfg.nu), zeros(Float32, c.cfg.nu)
    active = Ref{Cint}(0)
    GC.@preserve lo hi check(ccall((:mppi_get_control_bounds, LIB), Cint,
                                   (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ref{Cint}), c.handle, pointer(lo),
                                   pointer(hi), active))
    return (lo, hi, active[] != 0)
end

"""
    bound_counts(c) -> Vector{UInt32}

Per actuator, the number of (t, k) noise elements the last bounded solve projected (mppi_get_bound_counts; waits for the
stream).
"""
function bound_counts(c::Controller)
    n = zeros(UInt32, c.cfg.nu)
    GC.@preserve n check(ccall((:mppi_get_bound_counts, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt32}), c.handle, 1,
                               pointer(n)))
    return n
end

"""
    bounds_eval(c, U, noise) -> (noise_out::Array{Float32,3}, counts::Vector{UInt32})

The projection kernel alone on a given `U` (nu, H) and `noise` (nu, H, K) with the handle's box (mppi_bounds_eval);
needs the bounds set.
"""
function bounds_eval(c::Controller, U, noise)
    nu, H, K = c.cfg.nu, c.cfg.H, c.cfg.K
    size(U) == (nu, H) || throw(ArgumentError("U must be ($nu, $H)"))
    size(noise) == (nu, H, K) || throw(ArgumentError("noise must be ($nu, $H, $K)"))
    Ur = Float32.(permutedims(U))                  # (H, nu) column-major = the library's [nu][H]
    nz = Float32.(permutedims(noise, (3, 2, 1)))   # (K, H, nu) column-major = the library's [nu][H][K]
    out = zeros(Float32, K, H, nu)
    n = zeros(UInt32, nu)
    GC.@preserve Ur nz out n check(ccall((:mppi_bounds_eval, LIB), Cint,
                                         (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt32}),
                                         c.handle, 1, pointer(Ur), pointer(nz), pointer(out), pointer(n)))
    return (permutedims(out, (3, 2, 1)), n)
end

"""
    set_rate_cost!(c, weights; anchor = true)

Add a penalty on the rate of the sampled controls, `sum_u r[u] sum_t (v[u, t] - v[u, t-1])^2` with `v = clamp(U + eps)`,
to the costs the softmin weighs (mppi_set_rate_cost).  `weights`: a number or a length-nu vector, finite, >= 0, not all
zero; `nothing` disables.  With `anchor` the first control is differenced against the previously applied one
(`set_prev_control!`, or the u0 of the last shift solve).  Any change destroys captured graphs; a prefetched noise is
kept.  Needs nu <= 32.
"""
function set_rate_cost!(c::Controller, weights; anchor::Bool = true)
    nu = c.cfg.nu
    if weights === nothing
        check(ccall((:mppi_set_rate_cost, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cint), c.handle, Ptr{Float32}(C_NULL), 0))
        return c
    end
    r = weights isa Real ? fill(Float32(weights), nu) : Float32.(vec(collect(weights)))
    length(r) == nu || throw(ArgumentError("weights must be a number or have nu = $nu entries"))
    GC.@preserve r check(ccall((:mppi_set_rate_cost, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cint), c.handle, pointer(r),
                               anchor ? 1 : 0))
    return c
end

"""
    rate_cost(c) -> (weights::Vector{Float32}, anchor::Bool, active::Bool)

The settings of `set_rate_cost!` (mppi_get_rate_cost); zeros and false while the term is off.
"""
function rate_cost(c::Controller)
    r = zeros(Float32, c.cfg.nu)
    anchor, active = Ref{Cint}(0), Ref{Cint}(0)
    GC.@preserve r check(ccall((:mppi_get_rate_cost, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ref{Cint}, Ref{Cint}),
                               c.handle, pointer(r), anchor, active))
    return (r, anchor[] != 0, active[] != 0)
end

"""
    set_prev_control!(c, u)

The control applied the step before (length nu) -> the handle's `u_prev` (mppi_set_prev_control), which the anchored
rate term differences t = 0 against.  Data, not a setting: captured graphs stay.
"""
function set_prev_control!(c::Controller, u)
    v = Float32.(vec(collect(u)))
    length(v) == c.cfg.nu || throw(ArgumentError("u must have nu = $(c.cfg.nu) entries"))
    GC.@preserve v check(ccall((:mppi_set_prev_control, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 1,
                               pointer(v)))
    return c
end

"""
    prev_control(c) -> Vector{Float32}

The handle's `u_prev` (mppi_get_prev_control; waits for the stream): zeros until set or stored by a shift solve.
"""
function prev_control(c::Controller)
    v = zeros(Float32, c.cfg.nu)
    GC.@preserve v check(ccall((:mppi_get_prev_control, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 1,
                               pointer(v)))
    return v
end

"""
    rate_term(c) -> Vector{Float32}

The rate term (length K) of the last solve made with the term on (mppi_get_rate_term; waits for the stream).
"""
function rate_term(c::Controller)
    term = zeros(Float32, c.cfg.K)
    GC.@preserve term check(ccall((:mppi_get_rate_term, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 1,
                                  pointer(term)))
    return term
end

"""
    rate_term_eval(c, U, noise; u_prev = nothing) -> Vector{Float32}

The term's kernel on a given `U` (nu, H), `noise` (nu, H, K) as the rollout would see it and `u_prev` (length nu;
`nothing`: the handle's) with the handle's weights, anchor and ctrl_clamp (mppi_rate_term_eval); needs the term enabled.
"""
function rate_term_eval(c::Controller, U, noise; u_prev = nothing)
    nu, H, K = c.cfg.nu, c.cfg.H, c.cfg.K
    size(U) == (nu, H) || throw(ArgumentError("U must be ($nu, $H)"))
    size(noise) == (nu, H, K) || throw(ArgumentError("noise must be ($nu, $H, $K)"))
    Ur = Float32.(permutedims(U))                  # (H, nu) column-major = the library's [nu][H]
    nz = Float32.(permutedims(noise, (3, 2, 1)))   # (K, H, nu) column-major = the library's [nu][H][K]
    up = u_prev === nothing ? Float32[] : Float32.(vec(collect(u_prev)))
    u_prev === nothing || length(up) == nu || throw(ArgumentError("u_prev must have nu = $nu entries"))
    term = zeros(Float32, K)
    GC.@preserve Ur nz up term check(ccall((:mppi_rate_term_eval, LIB), Cint,
                                           (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                           c.handle, 1, pointer(Ur), pointer(nz),
                                           u_prev === nothing ? Ptr{Float32}(C_NULL) : pointer(up), pointer(term)))
    return term
end

"""
    set_elites!(c, n_elite)

Weigh only the `n_elite` best samples of each solve (mppi_set_elites): the selection runs on the device, exact, ties
admitted by ascending sample index; every other sample's weight is 0.  `n_elite` in 1:K enables, 0 disables.  With a
large lambda this is CEM's elite mean, with `set_ess_target!` a scale-free softmin over the elites.  Any change
destroys captured graphs; a prefetched noise is kept.
"""
function set_elites!(c::Controller, n_elite::Integer)
    check(ccall((:mppi_set_elites, LIB), Cint, (Ptr{Cvoid}, Cint), c.handle, n_elite))
    return c
end

"""
    elites(c) -> Int

`n_elite` of `set_elites!` (mppi_get_elites); 0 while off.
"""
function elites(c::Controller)
    n = Ref{Cint}(0)
    check(ccall((:mppi_get_elites, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), c.handle, n))
    return Int(n[])
end

"""
    elite_set(c) -> (idx::Vector{Int32}, tau::Float32)

The elite set of the last solve made with elites on (mppi_get_elite_set; waits for the stream): its members as 1-based
sample indices in ascending order, and the threshold cost.
"""
function elite_set(c::Controller)
    n = elites(c)
    idx = fill(Int32(-1), max(n, 1))
    count, tau = Ref{Int32}(0), Ref{Float32}(0)
    GC.@preserve idx check(ccall((:mppi_get_elite_set, LIB), Cint,
                                 (Ptr{Cvoid}, Cint, Ptr{Int32}, Ref{Int32}, Ref{Float32}), c.handle, 1, pointer(idx),
                                 count, tau))
    return (idx[1:count[]] .+ Int32(1), tau[])
end

"""
    elites_eval(c, costs) -> (idx::Vector{Int32}, tau::Float32, ecost::Vector{Float32})

The selection kernel on `costs` (length K; ties, NaN and infinities allowed) with the handle's `n_elite`
(mppi_elites_eval): the members as 1-based indices, the threshold, and the costs with `Inf32` off the set.  Needs
elites enabled.
"""
function elites_eval(c::Controller, costs)
    cs = Float32.(vec(collect(costs)))
    length(cs) == c.cfg.K || throw(ArgumentError("costs must have K = $(c.cfg.K) entries"))
    n = elites(c)
    idx = fill(Int32(-1), max(n, 1))
    ecost = zeros(Float32, c.cfg.K)
    count, tau = Ref{Int32}(0), Ref{Float32}(0)
    GC.@preserve cs idx ecost check(ccall((:mppi_elites_eval, LIB), Cint,
                                          (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Int32}, Ref{Int32}, Ref{Float32},
                                           Ptr{Float32}), c.handle, 1, pointer(cs), pointer(idx), count, tau,
                                          pointer(ecost)))
    return (idx[1:count[]] .+ Int32(1), tau[], ecost)
end

"""
    set_elite_keep!(c, n_keep)

Carry the `n_keep` best sampled control sequences of each solve into the next one (mppi_set_elite_keep; iCEM's keep /
shift elites): gathered on the device, time-shifted when the solve shifts, and injected into the first columns of the
next solve's noise.  `n_keep` in 1:K enables, 0 disables.  The first solve with the feature on is bit for bit the solve
without it.  Any change destroys captured graphs and empties the stored set.
"""
function set_elite_keep!(c::Controller, n_keep::Integer)
    check(ccall((:mppi_set_elite_keep, LIB), Cint, (Ptr{Cvoid}, Cint), c.handle, n_keep))
    return c
end

"""
    elite_keep(c) -> Int

`n_keep` of `set_elite_keep!` (mppi_get_elite_keep); 0 while off.
"""
function elite_keep(c::Controller)
    n = Ref{Cint}(0)
    check(ccall((:mppi_get_elite_keep, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), c.handle, n))
    return Int(n[])
end

"""
    kept(c) -> (v::Array{Float32,3}, kcost::Vector{Float32}, idx::Vector{Int32}, steps::Int)

The set stored by the last solve made with `set_elite_keep!` on (mppi_get_kept; waits for the stream): the planned
candidate control sequences `v` (nu, H, count) -- entries at steps beyond `steps` are 0 --, their costs, and their
1-based sample indices in ascending order.
"""
function kept(c::Controller)
    n = max(elite_keep(c), 1)
    nu, H = c.cfg.nu, c.cfg.H
    v = zeros(Float32, n, H, nu)  # the engine's [nu][H][n_keep], row-major
    kcost = zeros(Float32, n)
    idx = fill(Int32(-1), n)
    count, steps = Ref{Int32}(0), Ref{Int32}(0)
    GC.@preserve v kcost idx check(ccall((:mppi_get_kept, LIB), Cint,
                                         (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ref{Int32},
                                          Ref{Int32}), c.handle, 1, pointer(v), pointer(kcost), pointer(idx), count,
                                         steps))
    m = Int(count[])
    return (permutedims(v, (3, 2, 1))[:, :, 1:m], kcost[1:m], idx[1:m] .+ Int32(1), Int(steps[]))
end

"""
    set_iterations!(c, n_iter; return_best = false, add_mean = false)

Refine the distribution `n_iter` (1:16) times per control step on the device (mppi_set_iterations; CEM / iCEM proper): a
step is bit for bit `n_iter` consecutive solves on the same state, all but the last without shift, each with a fresh
noise key.  `return_best`: the step executes the first control of the best sample seen during the step; `add_mean`: the
last iteration enters the nominal itself as a candidate.  Injected noise with `n_iter > 1` and `u0_before` with
`n_iter > 1` or `return_best` are refused.  Any change destroys captured graphs.
"""
function set_iterations!(c::Controller, n_iter::Integer; return_best::Bool = false, add_mean::Bool = false)
    check(ccall((:mppi_set_iterations, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Cint), c.handle, n_iter,
                Cint(return_best), Cint(add_mean)))
    return c
end

"""
    iterations(c) -> (n_iter::Int, return_best::Bool, add_mean::Bool)

The setting of `set_iterations!` (mppi_get_iterations); `(1, false, false)` by default.
"""
function iterations(c::Controller)
    n, rb, am = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:mppi_get_iterations, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), c.handle, n, rb, am))
    return (Int(n[]), rb[] != 0, am[] != 0)
end

"""
    set_population!(c, schedule)

A sample count per inner iteration (mppi_set_population; iCEM's shrinking budget): iteration `i` of every control step
draws, rolls out and weighs `schedule[i]` samples, bit for bit the solve of a controller created with `K = schedule[i]`.
`length(schedule)` must equal `n_iter` of `set_iterations!`, `schedule[1] == K`, every entry in `1:K` and at least
`n_elite` and `n_keep` (`n_keep + 1` with `add_mean`).  `nothing` turns it off; `K` throughout is the feature off.  Any
change destroys captured graphs.
"""
function set_population!(c::Controller, schedule::Union{Nothing, AbstractVector{<:Integer}})
    if schedule === nothing
        check(ccall((:mppi_set_population, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint), c.handle, C_NULL, 0))
        return c
    end
    tab = Vector{Int32}(schedule)
    GC.@preserve tab check(ccall((:mppi_set_population, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint), c.handle,
                                 pointer(tab), length(tab)))
    return c
end

"""
    population(c) -> Union{Nothing, Vector{Int}}

The schedule of `set_population!` (mppi_get_population); `nothing` while it is off.
"""
function population(c::Controller)
    tab, n = zeros(Int32, 16), Ref{Cint}(0)
    GC.@preserve tab check(ccall((:mppi_get_population, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ref{Cint}), c.handle,
                                 pointer(tab), n))
    return n[] == 0 ? nothing : Int.(tab[1:n[]])
end

"""
    best(c) -> (v::Matrix{Float32}, cost::Float32, k::Int, iter::Int)

The best sampled control sequence of the last control step made with `set_iterations!` on (mppi_get_best; waits for
the stream): the planned trajectory `v` (nu, H), its cost, its 1-based sample index and the 1-based iteration that drew
it (both 0 when no sample of the step was finite).
"""
function best(c::Controller)
    nu, H = c.cfg.nu, c.cfg.H
    v = zeros(Float32, H, nu)  # the engine's [nu][H], row-major
    cost, k, it = Ref{Float32}(Inf32), Ref{Int32}(-1), Ref{Int32}(-1)
    GC.@preserve v check(ccall((:mppi_get_best, LIB), Cint,
                               (Ptr{Cvoid}, Cint, Ptr{Float32}, Ref{Float32}, Ref{Int32}, Ref{Int32}), c.handle, 1,
                               pointer(v), cost, k, it))
    return (permutedims(v, (2, 1)), cost[], Int(k[]) + 1, Int(it[]) + 1)
end

const ENS_MODES = Dict(:mean => 0, :mean_std => 1, :worst => 2)  # MPPI_ENS_*

"""
    load_member!(c, e, kind, weights)

Member `e` (1:7) of a dynamics-model ensemble (mppi_load_member): a weight blob file of the kind the controller was
created with (`:mlp`, `:feature_attention`, `:cross_attention`), or for `:cartpole` a vector of its 10 parameters
(`nothing`: the defaults).  Member 0 is the model the controller loaded; members are loaded densely.
"""
function load_member!(c::Controller, e::Integer, kind::Symbol, weights)
    if kind == :cartpole
        p = weights === nothing ? Float32[] : Vector{Float32}(weights)
        GC.@preserve p check(ccall((:mppi_load_member, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Csize_t),
                                   c.handle, e, DYN_CARTPOLE, isempty(p) ? C_NULL : pointer(p), sizeof(p)))
        return c
    end
    blob = read(weights)
    k = kind == :mlp ? DYN_MLP : kind == :feature_attention ? DYN_FEATURE_ATTN : DYN_CROSS_ATTN
    check(ccall((:mppi_load_member, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Csize_t), c.handle, e, k, blob,
                length(blob)))
    return c
end

"""
    set_ensemble!(c, n; mode = :mean, kappa = 0, env_member = 0)

Roll every sample under members `0:n-1` and combine their costs per sample on the device (mppi_set_ensemble; the PE of
PETS): `:mean`, `:mean_std` (mean + kappa * population std; a negative kappa is an optimism bonus) or `:worst`.
`n == 1` turns it off.  `env_member` (0-based, as the ABI) steps the environment.  Any change destroys captured graphs.
"""
function set_ensemble!(c::Controller, n::Integer; mode::Symbol = :mean, kappa::Real = 0, env_member::Integer = 0)
    haskey(ENS_MODES, mode) || throw(ArgumentError("mode must be :mean, :mean_std or :worst"))
    check(ccall((:mppi_set_ensemble, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Cfloat, Cint), c.handle, n, ENS_MODES[mode],
                Float32(kappa), env_member))
    return c
end

"""
    ensemble(c) -> (n, mode::Symbol, kappa::Float32, env_member, n_loaded)

The setting of `set_ensemble!` and the number of members loaded, member 0 included (mppi_get_ensemble).
"""
function ensemble(c::Controller)
    n, mode, env, loaded, kappa = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cfloat}(0)
    check(ccall((:mppi_get_ensemble, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cfloat}, Ref{Cint}, Ref{Cint}),
                c.handle, n, mode, kappa, env, loaded))
    name = first(k for (k, v) in ENS_MODES if v == mode[])
    return (Int(n[]), name, Float32(kappa[]), Int(env[]), Int(loaded[]))
end

"""
    member_costs(c, e) -> Vector{Float32}        ensemble_spread(c) -> Vector{Float32}

Member `e`'s (0-based) costs and the members' population std per sample, length K, of the last solve made with an
ensemble on (mppi_get_member_costs, mppi_get_ensemble_spread; both wait for the stream).
"""
function member_costs(c::Controller, e::Integer)
    out = zeros(Float32, c.cfg.K)
    GC.@preserve out check(ccall((:mppi_get_member_costs, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float32}), c.handle,
                                 1, e, pointer(out)))
    return out
end
function ensemble_spread(c::Controller)
    out = zeros(Float32, c.cfg.K)
    GC.@preserve out check(ccall((:mppi_get_ensemble_spread, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}), c.handle, 1,
                                 pointer(out)))
    return out
end

"""
    solve_stats(c) -> (stats::SolveStats, eps_m2::Vector{Float32}, eps_m11::Vector{Float32})

The diagnostics of the last solve made with `stats = true` (mppi_get_stats): the softmin statistics of its costs and
the weighted moments of the noise it used, per actuator, taken about the nominal U:
`sqrt.(eps_m2)` estimates sigma_u and `eps_m11 ./ eps_m2` the AR(1) correlation of the samples that won.
"""
function solve_stats(c::Controller)
    st = Ref{SolveStats}()
    m2 = zeros(Float32, c.cfg.nu)
    m11 = zeros(Float32, c.cfg.nu)
    GC.@preserve m2 m11 check(ccall((:mppi_get_stats, LIB), Cint,
                                    (Ptr{Cvoid}, Cint, Cint, Ref{SolveStats}, Ptr{Float32}, Ptr{Float32}),
                                    c.handle, 1, 0, st, pointer(m2), pointer(m11)))
    return (st[], m2, m11)
end

"""
    stats_eval(c, costs; noise = nothing)

The same statistics of a given cost vector (length K; non-finite entries allowed) and, optionally, noise (nu, H, K)
column-major as everywhere in this module (mppi_stats_eval).  Without noise only the SolveStats is returned.
"""
function stats_eval(c::Controller, costs; noise = nothing)
    cs = Float32.(vec(collect(costs)))
    length(cs) == c.cfg.K || throw(ArgumentError("costs must have K = $(c.cfg.K) entries"))
    st = Ref{SolveStats}()
    if noise === nothing
        GC.@preserve cs check(ccall((:mppi_stats_eval, LIB), Cint,
                                    (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ref{SolveStats}, Ptr{Float32},
                                     Ptr{Float32}), c.handle, 1, pointer(cs), C_NULL, st, C_NULL, C_NULL))
        return st[]
    end
    size(noise) == (c.cfg.nu, c.cfg.H, c.cfg.K) || throw(ArgumentError("noise must be (nu, H, K)"))
    nz = Float32.(permutedims(noise, (3, 2, 1)))   # the C ABI's [nu][H][K]: k fastest
    m2 = zeros(Float32, c.cfg.nu)
    m11 = zeros(Float32, c.cfg.nu)
    GC.@preserve cs nz m2 m11 check(ccall((:mppi_stats_eval, LIB), Cint,
                                          (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ref{SolveStats},
                                           Ptr{Float32}, Ptr{Float32}), c.handle, 1, pointer(cs), pointer(nz), st,
                                          pointer(m2), pointer(m11)))
    return (st[], m2, m11)
end

"rollout_kernel: the kernel the last solve was routed to (mppi_rollout_kernel; ABI 3)."
rollout_kernel(c::Controller) = unsafe_string(ccall((:mppi_rollout_kernel, LIB), Cstring, (Ptr{Cvoid},), c.handle))
"gen_route: where the last chained solve generated the next solve's noise, \"overlap\" or \"fused\" (mppi_gen_route)."
gen_route(c::Controller) = unsafe_string(ccall((:mppi_gen_route, LIB), Cstring, (Ptr{Cvoid},), c.handle))

"x3_f16: (form, probe error) of the split CA's fp16 form (mppi_x3_f16; ABI 4): 2 / 1 = on with a one- / two-product last layer, 0 = off."
function x3_f16(c::Controller)
    on = Ref{Cint}(0)
    err = Ref{Cfloat}(0)
    check(ccall((:mppi_x3_f16, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cfloat}), c.handle, on, err))
    return (Int(on[]), Float32(err[]))
end

end # module
