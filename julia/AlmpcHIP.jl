# AlmpcHIP.jl -- thin Julia shim over libalmpc.so (include/almpc.h).
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no `julia`.  Every behaviour of the ABI is exercised
# through the same entry points from Python (tests/test_gpu_parity.py) and from C (tests/capi_harness.c, which passes
# column-major arrays exactly as `ccall` does); this file is the binding a maintainer of
# AutomationLabsModelPredictiveControl.jl would add, and julia/reference_hip.patch wires it into the reference.  It keeps the reference's names and call shapes
# (src/main/main_mpc.jl:22-53, src/sub/design_mpc.jl:54-129, src/main/computation_mpc.jl:17-55) and adds the
# solver tag "hip" next to osqp/scip/ipopt/auto (src/sub/solver_selection.jl:9-14).
module AlmpcHIP

export hip_solver_def, HipModeler, AlmpcOpts, design_hip, terminal_weight, set_state_rows!, design_batched!, design_sqp_fnn!, sqp_start!, sqp_iterate!, sqp_solve!, set_sqp_hessian!, set_sqp_row_multipliers!, state_multipliers,
       design_relin_fnn!, relin_step!, relin_advance!, update_initialization!, calculate!, read_results!,
       _model_predictive_control_computation, comm_unique_id, comm_init!, comm_summary, comm_allgather_first_input,
       calculate_async!, synchronize!, relin_step_async!, advance_plant!, start_from!, update_initialization_device!, device_results, set_step_fusion!,
       set_structured_fallback!, sqp_skipped, design_instance, gradient_instance, design_ltv!, fnn_linearize, dare, default_opts,
       get_timing, timing_reset!, timing_set_stride!, timing_summary, timing_samples, relin_timing, debug_poison_lds!,
       update_initialization_async!, x0_staging, results_async, results_wait!, host_results, first_input, first_input!, ALLOW_UNSOLVED,
       HipGroup, group_design_hip, group_handle, group_shard, group_update_initialization!, group_calculate!, group_calculate_async!,
       group_synchronize!, group_read_results!, group_set_state_rows!, group_set_rho_profile!, group_set_structured_fallback!,
       group_design_batched!, design_batched_weighted!, weights_instance, group_design_batched_weighted!, group_design_relin_fnn!, group_relin_step!, group_relin_advance!, group_advance_plant!, group_design_sqp_fnn!,
       group_sqp_start!, group_sqp_iterate!, group_sqp_solve!, group_set_sqp_hessian!, group_set_sqp_row_multipliers!, group_state_multipliers, group_sqp_skipped, group_x0_staging, group_update_initialization_staged!, group_results_async,
       group_results_wait!, sensitivity, device_sensitivity, sensitivity_vjp, group_sensitivity, group_sensitivity_vjp,
       sensitivity_rows, sensitivity_rows_vjp, group_sensitivity_rows, group_sensitivity_rows_vjp, sensitivity_params_vjp,
       group_sensitivity_params_vjp, dare_vjp, dare_vjp_batched, sensitivity_stagewise, sensitivity_stagewise_vjp,
       group_sensitivity_stagewise, group_sensitivity_stagewise_vjp, sensitivity_stagewise_rate, sensitivity_stagewise_rate_vjp,
       group_sensitivity_stagewise_rate, group_sensitivity_stagewise_rate_vjp, certificate, certificate!, device_certificate,
       group_certificate, group_certificate!, set_keep_stage_models, certificate_ltv, certificate_ltv!, device_certificate_ltv,
       relin_fnn_certificate, relin_fnn_certificate!, group_relin_fnn_certificate, group_relin_fnn_certificate!,
       sensitivity_ltv, sensitivity_ltv_vjp, design_ltv_stagewise!, ltv_stagewise_update!

const libalmpc = get(ENV, "ALMPC_LIB", "libalmpc.so")

# Network code of the calls that take an activation (include/almpc.h ALMPC_NET_CODE): kind << 8 | activation.  The kinds share the
# Fnn weight layout and differ in the hidden layer: :fnn (also Icnn), :resnet y' = y + act(a), :polynet p = act(a), y' = y + p + act(W p + b).
const NET_KINDS = Dict(:fnn => 0, :resnet => 1, :polynet => 2)
net_code(net::Symbol, activation::Integer) = (NET_KINDS[net] << 8) | Int(activation)
# net = :densenet: a DenseNet (y_{l+1} = [act(W_h[l] y_l + b_h[l]); y_l], new features first) has its own weight layout and its own
# setup calls (the almpc_*densenet* entry points, a bare `activation`), not a network code.  `W_h` is then a vector of the L blocks,
# block l H x l H (1-based), packed column-major one after another (include/almpc.h); `W_out` is n x (L+1) H.
densenet_pack(W_h::AbstractVector{<:AbstractMatrix}) = isempty(W_h) ? zeros(1) : Vector{Float64}(reduce(vcat, vec.(W_h)))

struct hip_solver_def end            # new tag, to be made <: AbstractSolvers in src/types/types.jl:162-192

Base.@kwdef struct AlmpcOpts         # mirrors `almpc_opts` (72 bytes)
    rho::Cdouble = 0.1
    sigma::Cdouble = 1e-6
    alpha::Cdouble = 1.6
    eps_abs::Cdouble = 1e-3
    eps_rel::Cdouble = 1e-3
    max_iter::Int32 = 25
    check_every::Int32 = 25
    polish::Int32 = 1
    polish_max_iter::Int32 = 0
    warm_start::Int32 = 0
    reserved::NTuple{3,Int32} = (0, 0, 0)
end

# flag bits of opts.reserved[1] (C: opts.reserved[0]; include/almpc.h: ALMPC_OPT_*), e.g. reserved = (ALMPC_OPT_NO_WARM_STATE, 0, 0)
const ALMPC_OPT_NO_WARM_STATE = Int32(0x1)       # the step keeps no ADMM state for a warm start of the next one
const ALMPC_OPT_FULL_FIRST_PRODUCT = Int32(0x2)  # A/B control: the cold start's first ADMM iterate as a full product
const ALMPC_OPT_HBM_HANDOFF = Int32(0x4)         # A/B control: the one-kernel step hands its ADMM results on through global memory

mutable struct HipModeler            # what sits in tuning.modeler (`modeler::Any`, src/types/types.jl:115)
    handle::Ptr{Cvoid}
    n::Int; m::Int; N::Int; batch::Int
    opts::AlmpcOpts
    # what `calculate!` runs: :linear (almpc_calculate on the design in place), :relin (per-step re-linearisation of a black-box
    # model, almpc_relin_fnn_step), :sqp (the NonLinearProgramming branch: almpc_sqp_fnn_start from the last x0 + `sqp_iterations`)
    mode::Symbol
    sqp_iterations::Int
    x0::Vector{Float64}              # :sqp only: the last initialisation (the loop restarts from it in every calculate!)
end
HipModeler(h, n, m, N, batch, opts) = HipModeler(h, n, m, N, batch, opts, :linear, 20, Float64[])

function check(h, rc)
    rc == 0 && return
    msg = unsafe_string(ccall((:almpc_last_error, libalmpc), Cstring, (Ptr{Cvoid},), h))
    error("libalmpc error $rc: $msg")   # the reference throws from JuMP.value when no solution exists
end

"""
    design_hip(A, B, Q, R, S, umin, umax, N; batch = 1, device = 0, x_ref, u_ref, opts,
               xmin = nothing, xmax = nothing, terminal = "none", rho_profile = "scalar", P = nothing)

Design for `ConstrainedLinearControlDiscreteSystem` (replaces the JuMP model built at
src/sub/model_modeler_implementation/linear/mpc_modeler_implementation_linear.jl:20-103 and the objective of
src/sub/design_mpc.jl:405-468).  `P = nothing`: computed inside (DARE, src/sub/design_mpc.jl:327).
`xmin`/`xmax`: the state box of kw `mpc_state_constraint` (..linear.jl:62-70, stages 1..N+1).  `terminal = "equality"`:
`e_x[:, end] .== 0` (src/sub/design_mpc.jl:330-331); "none" / "neighborhood" add nothing, as in the reference; "contractive" is a
quadratic constraint and is refused.  `rho_profile`: "scalar" (OSQP) or "stiffness" (`almpc_set_rho_profile`).
"""
function design_hip(A::Matrix{Float64}, B::Matrix{Float64}, Q::Matrix{Float64}, R::Matrix{Float64},
                    S::Matrix{Float64}, umin::Vector{Float64}, umax::Vector{Float64}, N::Int;
                    batch::Int = 1, device::Int = 0, x_ref::Matrix{Float64}, u_ref::Matrix{Float64},
                    opts::AlmpcOpts = AlmpcOpts(), xmin::Union{Nothing,Vector{Float64}} = nothing,
                    xmax::Union{Nothing,Vector{Float64}} = nothing, terminal::String = "none",
                    rho_profile::String = "scalar", P::Union{Nothing,Matrix{Float64}} = nothing)
    n, m = size(B)
    terminal == "contractive" && error("terminal ingredient \"contractive\" is a quadratic constraint (src/sub/design_mpc.jl:333-340), not a QP row")
    (xmin === nothing) == (xmax === nothing) || error("give both xmin and xmax or neither")
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:almpc_create, libalmpc), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, UInt32),
               href, n, m, N, batch, device, 0)
    rc == 0 || error("almpc_create failed ($rc): no gfx950 device? (there is no CPU fallback)")
    h = href[]
    mod = HipModeler(h, n, m, N, batch, opts)
    finalizer(x -> ccall((:almpc_destroy, libalmpc), Cvoid, (Ptr{Cvoid},), x.handle), mod)
    check(h, ccall((:almpc_set_terminal_equality, libalmpc), Cint, (Ptr{Cvoid}, Cint), h, terminal == "equality" ? 1 : 0))
    check(h, ccall((:almpc_set_rho_profile, libalmpc), Cint, (Ptr{Cvoid}, Cint), h, rho_profile == "stiffness" ? 1 : 0))
    pP = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    pxmin = xmin === nothing ? Ptr{Float64}(C_NULL) : pointer(xmin)
    pxmax = xmax === nothing ? Ptr{Float64}(C_NULL) : pointer(xmax)
    GC.@preserve P xmin xmax check(h, ccall((:almpc_design_shared, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   h, A, B, Q, R, S, pP, umin, umax, pxmin, pxmax, opts.rho, opts.sigma))
    # references: n x (N+1) and m x N Julia matrices are already the ABI's [N+1][n] / [N][m] memory
    check(h, ccall((:almpc_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                   h, x_ref, u_ref, 0))
    return mod
end

"""
    set_state_rows!(mod; xmin = nothing, xmax = nothing, terminal = "none")

State box (kw `mpc_state_constraint`; .../fnn/mpc_modeler_implementation_fnn.jl:52-58,146-153) and terminal equality
(src/sub/design_mpc.jl:330-331) of the designs without `xmin`/`xmax` arguments: call before `design_batched!`, `design_sqp_fnn!`,
`design_relin_fnn!`.
"""
function set_state_rows!(mod::HipModeler; xmin::Union{Nothing,Vector{Float64}} = nothing, xmax::Union{Nothing,Vector{Float64}} = nothing,
                         terminal::String = "none")
    (xmin === nothing) == (xmax === nothing) || error("give both xmin and xmax or neither")
    check(mod.handle, ccall((:almpc_set_terminal_equality, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, terminal == "equality" ? 1 : 0))
    pmin = xmin === nothing ? Ptr{Float64}(C_NULL) : pointer(xmin)
    pmax = xmax === nothing ? Ptr{Float64}(C_NULL) : pointer(xmax)
    GC.@preserve xmin xmax check(mod.handle, ccall((:almpc_set_state_box, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                                                   mod.handle, pmin, pmax))
    return mod
end

"terminal weight P (n x n) of the current design: what `_create_terminal_ingredient` returns as `P_cost` (src/sub/design_mpc.jl:327,393)"
function terminal_weight(mod::HipModeler)
    P = Matrix{Float64}(undef, mod.n, mod.n)
    check(mod.handle, ccall((:almpc_get_design, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, C_NULL, C_NULL, P, C_NULL))
    return P
end

"""
    design_batched!(mod, A_batch, B_batch, Q, R, S, P, umin, umax; x_ref, u_ref)

One model per instance (`A_batch` n x n x batch, `B_batch` n x m x batch: Julia's column-major 3-arrays are the ABI's
[batch][n*n] / [batch][n*m] blocks): the linear-programming design of the reference for the linearisation of a black-box model at
every instance's own point (src/sub/model_modeler_implementation/fnn/mpc_modeler_implementation_fnn.jl:38-46 linearises once; the
per-step re-linearisation is BASELINE configs[3]).  `P` = nothing (DARE per instance), an n x n matrix, or n x n x batch.
"""
function design_batched!(mod::HipModeler, A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q::Matrix{Float64},
                         R::Matrix{Float64}, S::Matrix{Float64}, P, umin::Vector{Float64}, umax::Vector{Float64};
                         x_ref::Matrix{Float64}, u_ref::Matrix{Float64})
    size(A_batch, 3) == mod.batch && size(B_batch, 3) == mod.batch || throw(DimensionMismatch("one model per instance"))
    pptr = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    pinst = (P !== nothing && ndims(P) == 3) ? 1 : 0
    GC.@preserve P check(mod.handle, ccall((:almpc_design_batched, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                    Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   mod.handle, A_batch, B_batch, Q, R, S, pptr, pinst, umin, umax, mod.opts.rho, mod.opts.sigma))
    check(mod.handle, ccall((:almpc_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                            mod.handle, x_ref, u_ref, 0))
    return mod
end

"""
    design_batched_weighted!(mod, A_batch, B_batch, Q_batch, R_batch, S_batch, P, umin, umax; x_ref, u_ref)

`design_batched!` with one weight set per instance (`almpc_design_batched_weighted`): `Q_batch` n x n x batch, `R_batch` and `S_batch`
m x m x batch, `S_batch` = nothing for S = 0 everywhere.  Every instance must take the same R[1,1] == 0 / S[1,1] == 0 branch.
"""
function design_batched_weighted!(mod::HipModeler, A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q_batch::Array{Float64,3},
                                  R_batch::Array{Float64,3}, S_batch::Union{Nothing,Array{Float64,3}}, P, umin::Vector{Float64},
                                  umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64})
    all(size(M, 3) == mod.batch for M in (A_batch, B_batch, Q_batch, R_batch)) || throw(DimensionMismatch("one model and one weight set per instance"))
    S_batch === nothing || size(S_batch, 3) == mod.batch || throw(DimensionMismatch("one S per instance"))
    pptr = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    sptr = S_batch === nothing ? Ptr{Float64}(C_NULL) : pointer(S_batch)
    pinst = (P !== nothing && ndims(P) == 3) ? 1 : 0
    GC.@preserve P S_batch check(mod.handle, ccall((:almpc_design_batched_weighted, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                    Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   mod.handle, A_batch, B_batch, Q_batch, R_batch, sptr, pptr, pinst, umin, umax, mod.opts.rho, mod.opts.sigma))
    check(mod.handle, ccall((:almpc_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                            mod.handle, x_ref, u_ref, 0))
    return mod
end
"the weights instance `i` is designed on, as the design kernels read them (parity hook): (Q, R, S)"
function weights_instance(mod::HipModeler, i::Integer)
    Q, R, S = Matrix{Float64}(undef, mod.n, mod.n), Matrix{Float64}(undef, mod.m, mod.m), Matrix{Float64}(undef, mod.m, mod.m)
    check(mod.handle, ccall((:almpc_get_weights_instance, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, i - 1, Q, R, S))
    return Q, R, S
end

"""
    design_sqp_fnn!(mod, W_in, W_h, b_h, W_out, activation, Q, R, S, P, umin, umax; x_ref, u_ref)

NonLinearProgramming branch for an Fnn model (src/sub/model_modeler_implementation/fnn/mpc_modeler_implementation_fnn.jl:73-189,
which the reference solves with Ipopt): the same NLP by Gauss-Newton SQP on the device.  `W_in` H x (n+m), `W_h` H x H x L,
`b_h` H x L, `W_out` n x H as read from Flux.params (:88-107); `activation` 0 identity, 1 relu, 2 tanh, 3 sigmoid, 4 swish;
keyword `net` (:fnn, :resnet, :polynet) the network kind in the same layout (`net_code`), or :densenet (`densenet_pack`).
Then per step:  `sqp_start!(mod, x0)`;  `sqp_iterate!(mod, iters)`;  results through `calculate!`'s readers (`almpc_get_results`).
"""
function design_sqp_fnn!(mod::HipModeler, W_in::Matrix{Float64}, W_h::Union{Array{Float64,3},Vector{Matrix{Float64}}}, b_h::Matrix{Float64}, W_out::Matrix{Float64},
                         activation::Integer, Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64}, P::Matrix{Float64},
                         umin::Vector{Float64}, umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64}, net::Symbol = :fnn,
                         structured_qp::Bool = false)
    # structured_qp: every iteration's QP in the multiple-shooting form (k_riccati) instead of the condensed one
    check(mod.handle, ccall((:almpc_sqp_fnn_set_structured, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, structured_qp ? 1 : 0))
    if net === :densenet
        check(mod.handle, ccall((:almpc_sqp_densenet_setup, libalmpc), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                       mod.handle, size(W_in, 1), length(W_h), activation, W_in, densenet_pack(W_h), b_h, W_out, x_ref, u_ref, Q, R, S, P, 0,
                       umin, umax, mod.opts.rho, mod.opts.sigma))
        return mod
    end
    check(mod.handle, ccall((:almpc_sqp_fnn_setup, libalmpc), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   mod.handle, size(W_in, 1), size(W_h, 3), net_code(net, activation), W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, 0, umin, umax,
                   mod.opts.rho, mod.opts.sigma))
    return mod
end

sqp_start!(mod::HipModeler, x0::VecOrMat{Float64}) =
    check(mod.handle, ccall((:almpc_sqp_fnn_start, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), mod.handle, x0, C_NULL))

function sqp_iterate!(mod::HipModeler, iters::Integer; step::Float64 = 1.0, merit_safeguard::Bool = true)
    check(mod.handle, ccall((:almpc_sqp_fnn_set_step_rule, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, merit_safeguard ? 1 : 0))
    st, de = zeros(iters), zeros(iters)
    o = Ref(mod.opts)
    check(mod.handle, ccall((:almpc_sqp_fnn_iterate, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{AlmpcOpts}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, iters, step, o, st, de))
    return st, de
end

"""
    sqp_solve!(mod, max_iters, tol; merit_safeguard = true) -> (status, iters, kkt)

Solve to a first-order tolerance (`almpc_sqp_fnn_solve`): at most `max_iters` full steps, every instance frozen once its iterate
has zero defects and a projected adjoint-gradient residual <= `tol`.  Per instance: status 0 converged, 1 iteration limit,
2 skipped, 3 infeasible QP; QP iterations taken; residual of the last test.
"""
"Hessian of the SQP loop's QPs: `:gauss_newton` (default) or `:exact` (`almpc_sqp_fnn_set_hessian`)"
set_sqp_hessian!(mod::HipModeler, mode::Symbol) =
    check(mod.handle, ccall((:almpc_sqp_fnn_set_hessian, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, mode === :exact ? 1 : 0))
"State rows in the SQP loop's stopping test and exact Hessian: the finishes hand the row multipliers of every QP out (`almpc_sqp_fnn_set_row_multipliers`, default off)"
set_sqp_row_multipliers!(mod::HipModeler, on::Bool = true) =
    check(mod.handle, ccall((:almpc_sqp_fnn_set_row_multipliers, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, on ? 1 : 0))
"Multipliers of the state rows in each instance's last solved QP, `Array{Float64,3}(n, N, batch)`: `[i, k, b]` belongs to the row of `x[i, k+1]`"
function state_multipliers(mod::HipModeler)
    mu = Array{Float64,3}(undef, mod.n, mod.N, mod.batch)
    check(mod.handle, ccall((:almpc_sqp_fnn_state_multipliers, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), mod.handle, mu))
    return mu
end
function sqp_solve!(mod::HipModeler, max_iters::Integer, tol::Float64; merit_safeguard::Bool = true)
    check(mod.handle, ccall((:almpc_sqp_fnn_set_step_rule, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, merit_safeguard ? 1 : 0))
    st, it, kk = Vector{Int32}(undef, mod.batch), Vector{Int32}(undef, mod.batch), Vector{Float64}(undef, mod.batch)
    o = Ref(mod.opts)
    check(mod.handle, ccall((:almpc_sqp_fnn_solve, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{AlmpcOpts}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                            mod.handle, max_iters, tol, o, st, it, kk))
    return st, it, kk
end

# update_initialization!(C, x0): x0 is a Vector (batch 1) or an n x batch Matrix (src/main/computation_mpc.jl:17-29)
function update_initialization!(mod::HipModeler, x0::VecOrMat{Float64})
    length(x0) == mod.n * mod.batch || throw(DimensionMismatch("x0 must hold n x batch values"))
    if mod.mode === :sqp
        mod.x0 = vec(copy(x0))      # the SQP loop uploads it in sqp_start! (almpc_sqp_fnn_start)
        return
    end
    check(mod.handle, ccall((:almpc_update_initialization, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), mod.handle, x0))
end

# The library writes batch * n * (N+1) / batch * m * N doubles through these pointers: anything shorter would be a heap overflow
# (the reference allocates ONE instance's matrices, src/sub/design_mpc.jl:515-529; a batched caller must allocate the batch).
function check_result_sizes(mod::HipModeler, x, e_x, u, e_u)
    nx, nu = mod.n * (mod.N + 1) * mod.batch, mod.m * mod.N * mod.batch
    for (name, a, want) in (("x", x, nx), ("e_x", e_x, nx), ("u", u, nu), ("e_u", e_u, nu))
        a === nothing && continue
        length(a) == want || throw(DimensionMismatch("$name holds $(length(a)) values, the handle writes $want (n or m x horizon x batch = $(mod.batch))"))
    end
end

# What a per-instance status means to a caller of the reference's API.  The reference never checks the solver status and lets
# JuMP.value throw when there is no primal (src/main/computation_mpc.jl:41-53): it returns a solution or throws.  Here:
#   2 (non-finite) and 3 (infeasible: state box / terminal equality)  -> error, as JuMP.value would;
#   1 (no certificate: an iteration cap or a working set beyond 128 rows, after the stage-wise redo that libalmpc runs by default,
#      include/almpc.h almpc_set_structured_fallback)                  -> error as well, unless ALLOW_UNSOLVED[] is set: the arrays then hold
#      the best iterate (inputs inside their box, trajectory consistent with them) and the status vector says which instances.
#      With the exact finish switched off (opts.polish = 0) status 1 is OSQP's ITERATION_LIMIT, with which JuMP.value still returns: no error.
const ALLOW_UNSOLVED = Ref(false)
function throw_on_status(status; strict::Bool = true)
    any(==(2), status) && error("calculate!: non-finite values in at least one instance (no solution to read)")
    any(==(3), status) && error("calculate!: infeasible problem in at least one instance (state box / terminal equality)")
    if strict && !ALLOW_UNSOLVED[] && any(==(1), status)
        error("calculate!: $(count(==(1), status)) instance(s) without an optimality certificate (set AlmpcHIP.ALLOW_UNSOLVED[] = true to read the iterate)")
    end
    return status
end

# calculate!(C): fills u, e_u (m x N x batch) and x, e_x (n x (N+1) x batch) in place (src/main/computation_mpc.jl:38-55).
# first_move_only = true: only u[:, 1, :] is brought back (m x batch values, written into the first stage of `u`; 131 KB instead of
# 32 MB at the benchmark shape) -- what a receding-horizon caller applies; x, e_x, e_u are left untouched.
function calculate!(mod::HipModeler, x::Array{Float64}, e_x::Array{Float64}, u::Array{Float64}, e_u::Array{Float64};
                    first_move_only::Bool = false)
    check_result_sizes(mod, x, e_x, u, e_u)
    o = Ref(mod.opts)
    status = Vector{Int32}(undef, mod.batch)
    if mod.mode === :relin || mod.mode === :sqp
        if mod.mode === :relin
            relin_step!(mod)
        else
            length(mod.x0) == mod.n * mod.batch || error("calculate!: update_initialization! first")
            sqp_start!(mod, mod.x0)
            sqp_iterate!(mod, mod.sqp_iterations)
        end
        return throw_on_status(read_results!(mod, x, e_x, u, e_u); strict = mod.opts.polish != 0)
    end
    if first_move_only
        check(mod.handle, ccall((:almpc_calculate_async, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), mod.handle, o))
        t = results_async(mod; u0 = true, status = true)
        u0 = Matrix{Float64}(undef, mod.m, mod.batch)
        results_wait!(mod, t; u0 = u0, status = status)
        ur = reshape(u, mod.m, mod.N, mod.batch)
        @views ur[:, 1, :] .= u0
    else
        check(mod.handle, ccall((:almpc_calculate, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), mod.handle, o))
        check(mod.handle, ccall((:almpc_get_results, libalmpc), Cint,
                                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                                mod.handle, x, e_x, u, e_u, status, C_NULL, C_NULL))
    end
    return throw_on_status(status)
end

# ---- host-facing step path: pinned staging owned by the handle, transfers on copy streams (include/almpc.h) ----
"x0 (n x batch) -> pinned slot -> upload on the copy-in stream; returns at once, the next step waits for it on the device"
function update_initialization_async!(mod::HipModeler, x0::VecOrMat{Float64})
    length(x0) == mod.n * mod.batch || throw(DimensionMismatch("x0 must hold n x batch values"))
    check(mod.handle, ccall((:almpc_update_initialization_async, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), mod.handle, x0))
end

"zero-copy input: an n x batch matrix over the pinned slot the next `update_initialization_async!` will use -- write the states into it (e.g.
straight from the plant simulation) and pass it on: the staging copy is skipped.  Valid until that call."
function x0_staging(mod::HipModeler)
    slot = Ref{Ptr{Float64}}(C_NULL)
    check(mod.handle, ccall((:almpc_x0_staging, libalmpc), Cint, (Ptr{Cvoid}, Ref{Ptr{Float64}}), mod.handle, slot))
    return unsafe_wrap(Array, slot[], (mod.n, mod.batch))
end

const WANT_X, WANT_E_X, WANT_U, WANT_E_U, WANT_STATUS, WANT_ITERS, WANT_POLISH_ITERS, WANT_FIRST_INPUT =
    UInt32(0x01), UInt32(0x02), UInt32(0x04), UInt32(0x08), UInt32(0x10), UInt32(0x20), UInt32(0x40), UInt32(0x80)

"ask for results of the last enqueued step (read-back on the copy-out stream, the next step may start meanwhile); returns a ticket"
function results_async(mod::HipModeler; x::Bool = false, e_x::Bool = false, u::Bool = false, e_u::Bool = false, u0::Bool = false,
                       status::Bool = false, iters::Bool = false, polish_iters::Bool = false)
    want = (x ? WANT_X : UInt32(0)) | (e_x ? WANT_E_X : UInt32(0)) | (u ? WANT_U : UInt32(0)) | (e_u ? WANT_E_U : UInt32(0)) |
           (u0 ? WANT_FIRST_INPUT : UInt32(0)) | (status ? WANT_STATUS : UInt32(0)) | (iters ? WANT_ITERS : UInt32(0)) |
           (polish_iters ? WANT_POLISH_ITERS : UInt32(0))
    t = ccall((:almpc_get_results_async, libalmpc), Cint, (Ptr{Cvoid}, UInt32), mod.handle, want)
    t < 0 && check(mod.handle, t)
    return t
end

"wait for a ticket and copy the given arrays out of the pinned slot (`nothing`: not wanted); sizes are checked"
function results_wait!(mod::HipModeler, ticket::Integer; x = nothing, e_x = nothing, u = nothing, e_u = nothing, u0 = nothing,
                       status = nothing, iters = nothing, polish_iters = nothing)
    check_result_sizes(mod, x, e_x, u, e_u)
    u0 === nothing || length(u0) == mod.m * mod.batch || throw(DimensionMismatch("u0 must hold m x batch values"))
    for (name, a) in (("status", status), ("iters", iters), ("polish_iters", polish_iters))
        a === nothing || length(a) == mod.batch || throw(DimensionMismatch("$name must hold batch values"))
    end
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    pi(a) = a === nothing ? Ptr{Int32}(C_NULL) : pointer(a)
    GC.@preserve x e_x u e_u u0 status iters polish_iters check(mod.handle, ccall((:almpc_get_results_wait, libalmpc), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        mod.handle, ticket, pf(x), pf(e_x), pf(u), pf(e_u), pf(u0), pi(status), pi(iters), pi(polish_iters)))
end

"zero-copy views of a ticket's pinned slot (after `results_wait!(mod, ticket)`): arrays that were not asked for come back as `nothing`; valid until two more requests"
function host_results(mod::HipModeler, ticket::Integer)
    pd = [Ref{Ptr{Float64}}(C_NULL) for _ in 1:5]; pn = [Ref{Ptr{Int32}}(C_NULL) for _ in 1:3]
    check(mod.handle, ccall((:almpc_host_results, libalmpc), Cint,
        (Ptr{Cvoid}, Cint, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Int32}},
         Ref{Ptr{Int32}}, Ref{Ptr{Int32}}), mod.handle, ticket, pd[1], pd[2], pd[3], pd[4], pd[5], pn[1], pn[2], pn[3]))
    w(p, dims) = p[] == C_NULL ? nothing : unsafe_wrap(Array, p[], dims)
    return (x = w(pd[1], (mod.n, mod.N + 1, mod.batch)), e_x = w(pd[2], (mod.n, mod.N + 1, mod.batch)), u = w(pd[3], (mod.m, mod.N, mod.batch)),
            e_u = w(pd[4], (mod.m, mod.N, mod.batch)), u0 = w(pd[5], (mod.m, mod.batch)), status = w(pn[1], (mod.batch,)),
            iters = w(pn[2], (mod.batch,)), polish_iters = w(pn[3], (mod.batch,)))
end

"u[:, 1] of every instance of the last step, m x batch (`almpc_get_first_input`)"
function first_input!(mod::HipModeler, u0::Matrix{Float64})
    length(u0) == mod.m * mod.batch || throw(DimensionMismatch("u0 must hold m x batch values"))
    check(mod.handle, ccall((:almpc_get_first_input, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), mod.handle, u0))
    return u0
end
first_input(mod::HipModeler) = first_input!(mod, Matrix{Float64}(undef, mod.m, mod.batch))

"""
    design_relin_fnn!(mod, W_in, W_h, b_h, W_out, activation, Q, R, S, P, umin, umax; x_ref, u_ref)

BASELINE configs[3]: the black-box model is re-linearised at every instance's own state in every step, on the device
(`almpc_relin_fnn_*`).  `P` as the reference takes it: DARE at the linearisation about the LAST reference
(src/sub/design_mpc.jl:312-327).  Then per step: `update_initialization!(mod, X0)`; `relin_step!(mod)`; `read_results!`.
"""
function design_relin_fnn!(mod::HipModeler, W_in::Matrix{Float64}, W_h::Union{Array{Float64,3},Vector{Matrix{Float64}}}, b_h::Matrix{Float64},
                           W_out::Matrix{Float64}, activation::Integer, Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64}, P::Matrix{Float64},
                           umin::Vector{Float64}, umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64}, net::Symbol = :fnn)
    if net === :densenet
        check(mod.handle, ccall((:almpc_relin_densenet_setup, libalmpc), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                       mod.handle, size(W_in, 1), length(W_h), activation, W_in, densenet_pack(W_h), b_h, W_out, x_ref, u_ref, Q, R, S, P,
                       umin, umax, mod.opts.rho, mod.opts.sigma))
        return mod
    end
    check(mod.handle, ccall((:almpc_relin_fnn_setup, libalmpc), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   mod.handle, size(W_in, 1), size(W_h, 3), net_code(net, activation), W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax,
                   mod.opts.rho, mod.opts.sigma))
    return mod
end

"one step; `warm = true` after a solved step: working-set guess from the previous inputs shifted one stage, no ADMM phase"
function relin_step!(mod::HipModeler; warm::Bool = false)
    o0 = mod.opts
    o = Ref(AlmpcOpts(o0.rho, o0.sigma, o0.alpha, o0.eps_abs, o0.eps_rel, o0.max_iter, o0.check_every, o0.polish, o0.polish_max_iter,
                      Int32(warm), o0.reserved))
    check(mod.handle, ccall((:almpc_relin_fnn_step, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), mod.handle, o))
end

"x0 <- fnn(x0, u[:,1]) on the device: the closed loop of the black-box model itself (simulation studies)"
relin_advance!(mod::HipModeler) = check(mod.handle, ccall((:almpc_relin_fnn_advance, libalmpc), Cint, (Ptr{Cvoid},), mod.handle))

"copy the results of the last step into caller-owned arrays (m x N x batch, n x (N+1) x batch); returns the per-instance status"
function read_results!(mod::HipModeler, x::Array{Float64}, e_x::Array{Float64}, u::Array{Float64}, e_u::Array{Float64})
    check_result_sizes(mod, x, e_x, u, e_u)
    status = Vector{Int32}(undef, mod.batch)
    check(mod.handle, ccall((:almpc_get_results, libalmpc), Cint,
                            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                            mod.handle, x, e_x, u, e_u, status, C_NULL, C_NULL))
    return status
end

# ---- multi-GPU: one Julia process per GPU, each with its own handle on its shard of the batch; RCCL inside the library ----
"rank 0 makes the id and hands the 128 bytes to the other ranks (MPI.jl, Distributed, a file: any channel)"
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    rc = ccall((:almpc_comm_unique_id, libalmpc), Cint, (Ptr{UInt8},), id)
    rc == 0 || error("almpc_comm_unique_id failed ($rc): librccl not loadable?")
    return id
end

comm_init!(mod::HipModeler, id::Vector{UInt8}, rank::Integer, world::Integer) =
    check(mod.handle, ccall((:almpc_comm_init, libalmpc), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), mod.handle, id, rank, world))

"(ranks, unsolved instances over all ranks, max ADMM iterations, max polish iterations) of the last step, all-reduced over RCCL"
function comm_summary(mod::HipModeler)
    out = Vector{Int64}(undef, 4)
    check(mod.handle, ccall((:almpc_comm_summary, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Int64}), mod.handle, out))
    return out
end

"u[:, 1] of every instance of every rank (m x batch x world), all-gathered over RCCL: what a plant simulator on any rank needs next"
function comm_allgather_first_input(mod::HipModeler, world::Integer)
    out = Array{Float64,3}(undef, mod.m, mod.batch, world)
    check(mod.handle, ccall((:almpc_comm_allgather_first_input, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Ptr{Float64}}),
                            mod.handle, out, C_NULL))
    return out
end

# ---- the rest of the ABI: asynchronous stepping, timing, parity hooks, device-resident results, helpers ----
"launch a step on the handle's stream and return at once; `synchronize!` waits for it"
function calculate_async!(mod::HipModeler)
    o = Ref(mod.opts)
    check(mod.handle, ccall((:almpc_calculate_async, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), mod.handle, o))
end
synchronize!(mod::HipModeler) = check(mod.handle, ccall((:almpc_synchronize, libalmpc), Cint, (Ptr{Cvoid},), mod.handle))
function relin_step_async!(mod::HipModeler)
    o = Ref(mod.opts)
    check(mod.handle, ccall((:almpc_relin_fnn_step_async, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), mod.handle, o))
end
"x0 <- A x0 + B u[:,1] on the device (shared-model designs): the closed loop without a host round trip"
advance_plant!(mod::HipModeler) = check(mod.handle, ccall((:almpc_advance_plant, libalmpc), Cint, (Ptr{Cvoid},), mod.handle))
"x0 already in device memory (`d_x0`: device pointer to batch x n doubles)"
update_initialization_device!(mod::HipModeler, d_x0::Ptr{Float64}) =
    check(mod.handle, ccall((:almpc_update_initialization_device, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), mod.handle, d_x0))
"device pointers of the result arrays of the last step (x, e_x, u, e_u): for callers that keep the loop on the GPU"
function device_results(mod::HipModeler)
    px, pex, pu, peu = Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL)
    check(mod.handle, ccall((:almpc_device_results, libalmpc), Cint,
                            (Ptr{Cvoid}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}), mod.handle, px, pex, pu, peu))
    return px[], pex[], pu[], peu[]
end
"structured handle: the next step starts from `src`'s last inputs (same batch, horizon <= this one's): horizon continuation"
start_from!(mod::HipModeler, src::HipModeler) =
    check(mod.handle, ccall((:almpc_set_start_from, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), mod.handle, src.handle))
set_step_fusion!(mod::HipModeler, on::Bool) = check(mod.handle, ccall((:almpc_set_step_fusion, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, on ? 1 : 0))
"instances the condensed path leaves unsolved (open-loop unstable linearisations) are redone in the multiple-shooting form; before the design"
set_structured_fallback!(mod::HipModeler, on::Bool) =
    check(mod.handle, ccall((:almpc_set_structured_fallback, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, on ? 1 : 0))
"instances whose SQP iteration was skipped (indefinite condensed Hessian, non-finite or infeasible QP)"
function sqp_skipped(mod::HipModeler)
    out = Vector{Int32}(undef, mod.batch)
    check(mod.handle, ccall((:almpc_sqp_fnn_skipped, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Int32}), mod.handle, out))
    return out
end
"(H_i, F_i, d_i) of one instance of a per-instance design; `gradient_instance`: q_i of a time-varying design (parity hooks)"
function design_instance(mod::HipModeler, i::Integer)
    nz = mod.m * mod.N
    H, F, d = Matrix{Float64}(undef, nz, nz), Matrix{Float64}(undef, nz, mod.n), Vector{Float64}(undef, nz)
    check(mod.handle, ccall((:almpc_get_design_instance, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, i - 1, H, F, d))
    return H, F, d
end
function gradient_instance(mod::HipModeler, i::Integer)
    q = Vector{Float64}(undef, mod.m * mod.N)
    check(mod.handle, ccall((:almpc_get_gradient_instance, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), mod.handle, i - 1, q))
    return q
end
"""
    design_ltv!(mod, A_all, B_all, c_all, xbar, ubar, Q, R, S, P, umin, umax; x_ref, u_ref)

Time-varying models per instance (`A_all` n x n x N x batch, `B_all` n x m x N x batch, `c_all` n x N x batch or `nothing`,
`xbar` n x (N+1) x batch, `ubar` m x N x batch): the QP of one SQP / multiple-shooting iteration in v = u - ubar (`almpc_design_ltv`).
"""
function design_ltv!(mod::HipModeler, A_all::Array{Float64,4}, B_all::Array{Float64,4}, c_all, xbar::Array{Float64,3}, ubar::Array{Float64,3},
                     Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64}, P::Matrix{Float64}, umin::Vector{Float64}, umax::Vector{Float64};
                     x_ref::Matrix{Float64}, u_ref::Matrix{Float64})
    pc = c_all === nothing ? Ptr{Float64}(C_NULL) : pointer(c_all)
    GC.@preserve c_all check(mod.handle, ccall((:almpc_design_ltv, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   mod.handle, A_all, B_all, pc, xbar, ubar, x_ref, u_ref, Q, R, S, P, 0, umin, umax, mod.opts.rho, mod.opts.sigma))
    return mod
end
"""
    design_ltv_stagewise!(mod, A_all, B_all, c_all, xbar, ubar, Q, R, S, P, umin, umax; x_ref, u_ref)

`design_ltv!`'s problem on the stage-wise solvers of a structured modeler (`almpc_design_ltv_stagewise`): no `m N <= 128` limit, no
rho / sigma; `x_ref` / `u_ref` may be `nothing`.  State box and terminal equality: `set_state_rows!` first.  Afterwards `results` has
every output: `u = ubar + v`, `e_u = v`, `x = xbar + dx`, `e_x = dx`.  The five trajectory arrays are host arrays as in `design_ltv!`,
or -- all five (`c_all` may stay `nothing`) -- `Ptr{Float64}` into device memory of the modeler's device in the same layout
(`on_device = 1`).  No group form.
"""
function design_ltv_stagewise!(mod::HipModeler, A_all, B_all, c_all, xbar, ubar, Q::Matrix{Float64}, R::Matrix{Float64},
                               S::Union{Nothing,Matrix{Float64}}, P::Matrix{Float64}, umin::Vector{Float64}, umax::Vector{Float64};
                               x_ref::Union{Nothing,Matrix{Float64}} = nothing, u_ref::Union{Nothing,Matrix{Float64}} = nothing)
    on_device = ltv_stage_form(A_all, B_all, c_all, xbar, ubar)
    null = Ptr{Float64}(C_NULL)
    GC.@preserve A_all B_all c_all xbar ubar x_ref u_ref S check(mod.handle, ccall((:almpc_design_ltv_stagewise, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cint),
                   mod.handle, ltv_stage_ptr(A_all), ltv_stage_ptr(B_all), ltv_stage_ptr(c_all), ltv_stage_ptr(xbar), ltv_stage_ptr(ubar),
                   x_ref === nothing ? null : pointer(x_ref), u_ref === nothing ? null : pointer(u_ref), Q, R,
                   S === nothing ? null : pointer(S), P, 0, umin, umax, on_device))
    return mod
end
"""
    ltv_stagewise_update!(mod, A_all, B_all, c_all, xbar, ubar)

New trajectory data into the design of `design_ltv_stagewise!` (`almpc_ltv_stagewise_update`): the per-iteration call of a caller's outer
loop.  With device pointers nothing is waited for: the arrays must be complete before the call and may be overwritten after
`synchronize`.  `c_all` is `nothing` exactly when the design's was.
"""
function ltv_stagewise_update!(mod::HipModeler, A_all, B_all, c_all, xbar, ubar)
    on_device = ltv_stage_form(A_all, B_all, c_all, xbar, ubar)
    GC.@preserve A_all B_all c_all xbar ubar check(mod.handle, ccall((:almpc_ltv_stagewise_update, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                   mod.handle, ltv_stage_ptr(A_all), ltv_stage_ptr(B_all), ltv_stage_ptr(c_all), ltv_stage_ptr(xbar), ltv_stage_ptr(ubar), on_device))
    return mod
end
"parity hook (`almpc_get_ltv_stagewise_prepared`): `ebar` n x N x batch and `qadd` m x N x batch as `k_ltv_stage_prepare` left them"
function ltv_stagewise_prepared(mod::HipModeler)
    ebar = Array{Float64,3}(undef, mod.n, mod.N, mod.batch)
    qadd = Array{Float64,3}(undef, mod.m, mod.N, mod.batch)
    check(mod.handle, ccall((:almpc_get_ltv_stagewise_prepared, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, ebar, qadd, Ptr{Float64}(C_NULL)))
    return ebar, qadd
end
ltv_stage_ptr(a::Nothing) = Ptr{Float64}(C_NULL)
ltv_stage_ptr(a::Ptr{Float64}) = a
ltv_stage_ptr(a::Array{Float64}) = pointer(a)
"1 when the four required trajectory arrays are device pointers, 0 when they are host arrays; a mixture is an error"
function ltv_stage_form(A_all, B_all, c_all, xbar, ubar)
    dev = [a isa Ptr{Float64} for a in (A_all, B_all, xbar, ubar)]
    all(dev) || !any(dev) || throw(ArgumentError("give the trajectory arrays as host arrays or as device pointers, not both"))
    c_all === nothing || (c_all isa Ptr{Float64}) == dev[1] || throw(ArgumentError("c_all is of the other form"))
    return Cint(dev[1] ? 1 : 0)
end
"Jacobians (A_i, B_i) and values of an Fnn at `x` (n x batch), `u` (m x batch) on device `device` (the batched `proceed_system_linearization`)"
function fnn_linearize(W_in::Matrix{Float64}, W_h::Union{Array{Float64,3},Vector{Matrix{Float64}}}, b_h::Matrix{Float64}, W_out::Matrix{Float64},
                       activation::Integer, x::Matrix{Float64}, u::Matrix{Float64}; device::Integer = 0, net::Symbol = :fnn)
    n, m, b = size(x, 1), size(u, 1), size(x, 2)
    A, B, f = Array{Float64,3}(undef, n, n, b), Array{Float64,3}(undef, n, m, b), Matrix{Float64}(undef, n, b)
    if net === :densenet
        rc = ccall((:almpc_densenet_linearize, libalmpc), Cint,
                   (Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   device, n, m, size(W_in, 1), length(W_h), activation, W_in, densenet_pack(W_h), b_h, W_out, b, x, u, A, B, f)
        rc == 0 || error("almpc_densenet_linearize failed ($rc)")
        return A, B, f
    end
    rc = ccall((:almpc_fnn_linearize, libalmpc), Cint,
               (Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               device, n, m, size(W_in, 1), size(W_h, 3), net_code(net, activation), W_in, W_h, b_h, W_out, b, x, u, A, B, f)
    rc == 0 || error("almpc_fnn_linearize failed ($rc)")
    return A, B, f
end
"P = DARE(A, B, Q, R) as the library computes it (host; src/sub/design_mpc.jl:327)"
function dare(A::Matrix{Float64}, B::Matrix{Float64}, Q::Matrix{Float64}, R::Matrix{Float64})
    n, m = size(B)
    P = Matrix{Float64}(undef, n, n)
    rc = ccall((:almpc_dare, libalmpc), Cint, (Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), n, m, A, B, Q, R, P)
    rc == 0 || error("almpc_dare: no convergence ($rc)")
    return P
end
"""
    dare_batched(A_batch, B_batch, Q, R; device = 0) -> (P, status)

P_i = DARE(A_i, B_i, Q, R) on the GPU, one wave per instance (`almpc_dare_batched`): `A_batch` n x n x batch, `B_batch` n x m x batch.
`status[i] != 0`: no stabilising solution to working precision; slice i of `P` is then NaN.
"""
function dare_batched(A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q::Matrix{Float64}, R::Matrix{Float64}; device::Integer = 0)
    n, m, b = size(B_batch, 1), size(B_batch, 2), size(B_batch, 3)
    size(A_batch) == (n, n, b) || throw(DimensionMismatch("A_batch must be n x n x batch"))
    P, status = fill(NaN, n, n, b), Vector{Int32}(undef, b)
    rc = ccall((:almpc_dare_batched, libalmpc), Cint,
               (Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
               device, n, m, b, A_batch, B_batch, Q, R, P, status)
    rc == 0 || error("almpc_dare_batched failed ($rc)")
    return P, status
end
"""
    dare_vjp(A, B, Q, R, P, g_P) -> (g_A, g_B, g_Q, g_R)

The adjoint of `dare` (`almpc_dare_vjp`, host): for P = DARE(A, B, Q, R) and a symmetric g_P = dL/dP, what the loss gains through P in
A, B, Q, R.  An error when P is not the stabilising solution of this model.
"""
function dare_vjp(A::Matrix{Float64}, B::Matrix{Float64}, Q::Matrix{Float64}, R::Matrix{Float64}, P::Matrix{Float64}, g_P::Matrix{Float64})
    n, m = size(B)
    g_A, g_B, g_Q, g_R = Matrix{Float64}(undef, n, n), Matrix{Float64}(undef, n, m), Matrix{Float64}(undef, n, n), Matrix{Float64}(undef, m, m)
    rc = ccall((:almpc_dare_vjp, libalmpc), Cint, (Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), n, m, A, B, Q, R, P, g_P, g_A, g_B, g_Q, g_R)
    rc == 0 || error("almpc_dare_vjp: " * unsafe_string(ccall((:almpc_last_error, libalmpc), Cstring, (Ptr{Cvoid},), C_NULL)) * " ($rc)")
    return g_A, g_B, g_Q, g_R
end
"""
    dare_vjp_batched(A_batch, B_batch, Q, R, P_batch, gP_batch; device = 0) -> (g_A, g_B, g_Q, g_R, status)

`dare_vjp` on the GPU, one wave per instance (`almpc_dare_vjp_batched`): batch last.  `status[i] != 0` (1 singular R + B'PB, 2 closed loop
not stable, 3 P does not solve the equation): the slices i are then NaN.
"""
function dare_vjp_batched(A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q::Matrix{Float64}, R::Matrix{Float64},
                          P_batch::Array{Float64,3}, gP_batch::Array{Float64,3}; device::Integer = 0)
    n, m, b = size(B_batch, 1), size(B_batch, 2), size(B_batch, 3)
    size(A_batch) == size(P_batch) == size(gP_batch) == (n, n, b) || throw(DimensionMismatch("A_batch, P_batch, gP_batch must be n x n x batch"))
    g_A, g_B, g_Q, g_R, status = fill(NaN, n, n, b), fill(NaN, n, m, b), fill(NaN, n, n, b), fill(NaN, m, m, b), Vector{Int32}(undef, b)
    rc = ccall((:almpc_dare_vjp_batched, libalmpc), Cint,
               (Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), device, n, m, b, A_batch, B_batch, Q, R, P_batch, gP_batch, g_A, g_B, g_Q, g_R, status)
    rc == 0 || error("almpc_dare_vjp_batched failed ($rc)")
    return g_A, g_B, g_Q, g_R, status
end
"""
    set_terminal_weight!(mod, mode)

Before a design: `:given` (default) or `:dare_device` -- `design_batched!` without a P and every step of the re-linearisation pipeline
take each instance's terminal weight from the DARE of its own model, solved on the device (`almpc_set_terminal_weight`).
"""
set_terminal_weight!(mod::HipModeler, mode::Symbol) =
    check(mod.handle, ccall((:almpc_set_terminal_weight, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, mode === :dare_device ? 1 : 0))
"after a step of the re-linearisation pipeline with `:dare_device`: 0 = the instance's own DARE solution, 1 = the setup's P"
function relin_terminal_status(mod::HipModeler)
    out = Vector{Int32}(undef, mod.batch)
    check(mod.handle, ccall((:almpc_relin_fnn_terminal_status, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Int32}), mod.handle, out))
    return out
end
"the terminal weight instance `i` was designed with (parity hook beside `design_instance`)"
function terminal_weight_instance(mod::HipModeler, i::Integer)
    P = Matrix{Float64}(undef, mod.n, mod.n)
    check(mod.handle, ccall((:almpc_get_terminal_weight_instance, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), mod.handle, i - 1, P))
    return P
end
"""
    c2d(Ac, Bc, Ts) -> (Ad, Bd)

Exact zero-order hold of x' = Ac x + Bc u at the sample time `Ts` (`almpc_c2d`, host math): [Ad Bd; 0 I] = exp([Ac Bc; 0 0] Ts).
"""
function c2d(Ac::Matrix{Float64}, Bc::Matrix{Float64}, Ts::Real)
    n, m = size(Bc)
    size(Ac) == (n, n) || throw(DimensionMismatch("Ac must be n x n"))
    Ad, Bd = Matrix{Float64}(undef, n, n), Matrix{Float64}(undef, n, m)
    rc = ccall((:almpc_c2d, libalmpc), Cint, (Cint, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
               n, m, Ac, Bc, Ts, Ad, Bd)
    rc == 0 || error("almpc_c2d failed ($rc)")
    return Ad, Bd
end
"""
    c2d_batched(Ac_batch, Bc_batch, Ts; device = 0) -> (Ad, Bd, status)

The same for a batch of models on the GPU, one wave per instance (`almpc_c2d_batched`): `Ac_batch` n x n x batch, `Bc_batch`
n x m x batch.  `status[i] != 0`: the discretisation of model i failed; slices i of `Ad` and `Bd` are then NaN.
"""
function c2d_batched(Ac_batch::Array{Float64,3}, Bc_batch::Array{Float64,3}, Ts::Real; device::Integer = 0)
    n, m, b = size(Bc_batch, 1), size(Bc_batch, 2), size(Bc_batch, 3)
    size(Ac_batch) == (n, n, b) || throw(DimensionMismatch("Ac_batch must be n x n x batch"))
    Ad, Bd, status = fill(NaN, n, n, b), fill(NaN, n, m, b), Vector{Int32}(undef, b)
    rc = ccall((:almpc_c2d_batched, libalmpc), Cint,
               (Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
               device, n, m, b, Ac_batch, Bc_batch, Ts, Ad, Bd, status)
    rc == 0 || error("almpc_c2d_batched failed ($rc)")
    return Ad, Bd, status
end
"""
    set_model_time!(mod, mode, Ts = 0.0)

Before a design: `:discrete` (default) or `:continuous` with the sample time `Ts` -- the models given to the designs and the network of
the re-linearisation pipeline are continuous-time and are discretised by zero-order hold at `Ts` (`almpc_set_model_time`).
"""
set_model_time!(mod::HipModeler, mode::Symbol, Ts::Real = 0.0) =
    check(mod.handle, ccall((:almpc_set_model_time, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble), mod.handle, mode === :continuous ? 1 : 0, Ts))
"the DISCRETE model instance `i` is designed on (parity hook beside `design_instance`): (A, B)"
function model_instance(mod::HipModeler, i::Integer)
    A, B = Matrix{Float64}(undef, mod.n, mod.n), Matrix{Float64}(undef, mod.n, mod.m)
    check(mod.handle, ccall((:almpc_get_model_instance, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), mod.handle, i - 1, A, B))
    return A, B
end
# ---- sensitivities of the last step to x0 (include/almpc.h "Sensitivities"; an extension beyond the reference's surface) ----
const SENS_K0, SENS_DU, SENS_DX = UInt32(1), UInt32(2), UInt32(4)   # ALMPC_SENS_*
sens_mask(K0::Bool, dU::Bool, dX::Bool) = (K0 ? SENS_K0 : UInt32(0)) | (dU ? SENS_DU : UInt32(0)) | (dX ? SENS_DX : UInt32(0))
function sens_arrays(n, m, N, batch, K0::Bool, dU::Bool, dX::Bool)
    (K0 || dU || dX) || error("sensitivity: nothing asked for")
    return (K0 ? Array{Float64,3}(undef, m, n, batch) : nothing, dU ? Array{Float64,4}(undef, m, N, n, batch) : nothing,
            dX ? Array{Float64,4}(undef, n, N + 1, n, batch) : nothing, Vector{Int32}(undef, batch))
end
function check_sens_sizes(n, m, N, batch, g_u, g_x)
    length(g_u) == m * N * batch || throw(DimensionMismatch("g_u holds $(length(g_u)) values, the solver reads $(m * N * batch)"))
    g_x === nothing || length(g_x) == n * (N + 1) * batch ||
        throw(DimensionMismatch("g_x holds $(length(g_x)) values, the solver reads $(n * (N + 1) * batch)"))
end
"""
    sensitivity(mod; K0 = true, dU = false, dX = false, act_tol = 0.0) -> (K0, dU, dX, rows)

Derivatives of the last step's solution with respect to x0 (`almpc_sensitivity` + `almpc_get_sensitivity`): `K0` m x n x batch
(the first-move gain), `dU` m x N x n x batch, `dX` n x (N+1) x n x batch (`nothing` for what was not asked for) and `rows`, the
number of rows at a bound per instance (-1: instance not solved, zeros).
"""
function sensitivity(mod::HipModeler; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(mod.n, mod.m, mod.N, mod.batch, K0, dU, dX)
    check(mod.handle, ccall((:almpc_sensitivity, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), mod.handle, sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx check(mod.handle, ccall((:almpc_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), mod.handle, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"device pointers of the last `sensitivity` call's buffers (K0, dU, dX, rows; C_NULL for what was not computed)"
function device_sensitivity(mod::HipModeler)
    pk, pu, px, pr = Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Int32}}(C_NULL)
    check(mod.handle, ccall((:almpc_device_sensitivity, libalmpc), Cint,
                            (Ptr{Cvoid}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Int32}}), mod.handle, pk, pu, px, pr))
    return pk[], pu[], px[], pr[]
end
"""
    sensitivity_vjp(mod, g_u, g_x = nothing; act_tol = 0.0) -> (g_x0, rows)

dL/dx0 (n x batch) for a loss with gradients `g_u` (m x N x batch) and `g_x` (n x (N+1) x batch, or nothing) on the returned
trajectories (`almpc_sensitivity_vjp`: no Jacobian is formed).
"""
function sensitivity_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, mod.n, mod.batch), Vector{Int32}(undef, mod.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x check(mod.handle, ccall((:almpc_sensitivity_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), mod.handle, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"""
    sensitivity_rows(mod; K0 = true, dU = false, dX = false, act_tol_u = 0.0, act_tol_x = 0.0) -> (K0, dU, dX, rows)

`sensitivity` for designs with `mpc_state_constraint` and / or `mpc_terminal_ingredient = "equality"` as well
(`almpc_sensitivity_rows` + `almpc_get_sensitivity`): `rows` counts input, state-box and terminal-equality rows at a bound;
`act_tol_x` is the state rows' threshold (0: 1e-7 of max(1, |bound|)).  Without state rows it is `sensitivity` with `act_tol_u`.
"""
function sensitivity_rows(mod::HipModeler; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol_u::Real = 0.0, act_tol_x::Real = 0.0)
    k, du, dx, rows = sens_arrays(mod.n, mod.m, mod.N, mod.batch, K0, dU, dX)
    check(mod.handle, ccall((:almpc_sensitivity_rows, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble, Cdouble), mod.handle,
                            sens_mask(K0, dU, dX), act_tol_u, act_tol_x))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx check(mod.handle, ccall((:almpc_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), mod.handle, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_vjp` in the rows form (`almpc_sensitivity_rows_vjp`)"
function sensitivity_rows_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing;
                              act_tol_u::Real = 0.0, act_tol_x::Real = 0.0)
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, mod.n, mod.batch), Vector{Int32}(undef, mod.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x check(mod.handle, ccall((:almpc_sensitivity_rows_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Int32}), mod.handle, g_u, px, act_tol_u, act_tol_x, g_x0, rows))
    return g_x0, rows
end
"""
    sensitivity_stagewise(mod; K0 = true, dU = false, dX = false, act_tol = 0.0) -> (K0, dU, dX, rows)

`sensitivity` on a structured modeler (`almpc_sensitivity_stagewise` + `almpc_get_sensitivity`): the Riccati recursion on the face where
the inputs at a bound are held, for any m N; input box only, S = 0.  `act_tol` is relative to the width of the input box (0: 1e-7).
"""
function sensitivity_stagewise(mod::HipModeler; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(mod.n, mod.m, mod.N, mod.batch, K0, dU, dX)
    check(mod.handle, ccall((:almpc_sensitivity_stagewise, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), mod.handle,
                            sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx check(mod.handle, ccall((:almpc_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), mod.handle, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_vjp` on a structured modeler (`almpc_sensitivity_stagewise_vjp`)"
function sensitivity_stagewise_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, mod.n, mod.batch), Vector{Int32}(undef, mod.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x check(mod.handle, ccall((:almpc_sensitivity_stagewise_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), mod.handle, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"""
    sensitivity_stagewise_rate(mod; K0 = true, dU = false, dX = false, act_tol = 0.0) -> (K0, dU, dX, rows)

`sensitivity_stagewise` for every structured input-box design, with or without the input-rate weight S
(`almpc_sensitivity_stagewise_rate` + `almpc_get_sensitivity`): with S the Riccati recursion on the face runs in the stage state
`[dx_k; du_(k-1)]`; without it the call returns the bits of `sensitivity_stagewise`.
"""
function sensitivity_stagewise_rate(mod::HipModeler; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(mod.n, mod.m, mod.N, mod.batch, K0, dU, dX)
    check(mod.handle, ccall((:almpc_sensitivity_stagewise_rate, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), mod.handle,
                            sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx check(mod.handle, ccall((:almpc_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), mod.handle, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"""
    sensitivity_stagewise_rate_vjp(mod, g_u, g_x = nothing; act_tol = 0.0) -> (g_x0, rows)

`sensitivity_stagewise_vjp` for designs with or without S (`almpc_sensitivity_stagewise_rate_vjp`): the adjoint rides the backward
sweep of the recursion in `[dx_k; du_(k-1)]`.
"""
function sensitivity_stagewise_rate_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, mod.n, mod.batch), Vector{Int32}(undef, mod.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x check(mod.handle, ccall((:almpc_sensitivity_stagewise_rate_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), mod.handle, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"""
    sensitivity_ltv(mod; K0 = true, dU = false, dX = false, act_tol = 0.0) -> (K0, dU, dX, rows)

The sensitivities of the last step of a `design_ltv!` design made with `set_keep_stage_models` in its initial deviation
(`almpc_sensitivity_ltv` + `almpc_get_sensitivity`): the Riccati recursion on the face with the stage models `A_k, B_k`, with or without
the input-rate weight S.  `K0` is the gain of a real-time iteration: apply `clamp.(u_0 + K0 * (x_meas - xbar_0), u_min, u_max)`.
`act_tol` is relative to the width of the input box (0: 1e-7).
"""
function sensitivity_ltv(mod::HipModeler; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(mod.n, mod.m, mod.N, mod.batch, K0, dU, dX)
    check(mod.handle, ccall((:almpc_sensitivity_ltv, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), mod.handle,
                            sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx check(mod.handle, ccall((:almpc_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), mod.handle, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"""
    sensitivity_ltv_vjp(mod, g_u, g_x = nothing; act_tol = 0.0) -> (g_x0, rows)

`sensitivity_vjp` of the same step (`almpc_sensitivity_ltv_vjp`): `g_x` is a loss gradient on the predicted states `xbar + dx` of
`certificate_ltv`; the adjoint rides the backward sweep, no Jacobian is formed.
"""
function sensitivity_ltv_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, mod.n, mod.batch), Vector{Int32}(undef, mod.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x check(mod.handle, ccall((:almpc_sensitivity_ltv_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), mod.handle, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end

# ---- certificate of the last step (include/almpc.h "Certificate of the last step"): ALMPC_CERT_* bits
cert_mask(cost, res, grad, costate) =
    UInt32((cost === nothing ? 0 : 1) | (res === nothing ? 0 : 2) | (grad === nothing ? 0 : 4) | (costate === nothing ? 0 : 8))
function check_cert_sizes(n, m, N, batch, cost, res, grad, costate)
    for (name, a, len) in (("cost", cost, batch), ("res", res, batch), ("grad", grad, m * N * batch), ("costate", costate, n * (N + 1) * batch))
        a === nothing || length(a) == len || throw(DimensionMismatch("$name holds $(length(a)) values, the solver writes $len"))
    end
    cert_mask(cost, res, grad, costate) != 0 || error("certificate: nothing asked for")
end
"""
    certificate!(mod, cost, res, grad, costate)

The certificate of the last `calculate!` into the caller's arrays (`almpc_certificate` + `almpc_get_certificate`); `nothing` = not
wanted.  `cost` (batch): the objective value JuMP would report; `res` (batch): the KKT residual of the returned inputs, whatever the
solver's own status says; `grad` (m x N x batch): the gradient of the objective in the inputs (its negative at an input that sits at a
bound is that bound's multiplier, positive at `u_max`); `costate` (n x (N+1) x batch), whose first column is d cost / d x0.
"""
function certificate!(mod::HipModeler, cost::Union{Nothing,Array{Float64}}, res::Union{Nothing,Array{Float64}},
                      grad::Union{Nothing,Array{Float64}}, costate::Union{Nothing,Array{Float64}})
    check_cert_sizes(mod.n, mod.m, mod.N, mod.batch, cost, res, grad, costate)
    check(mod.handle, ccall((:almpc_certificate, libalmpc), Cint, (Ptr{Cvoid}, UInt32), mod.handle, cert_mask(cost, res, grad, costate)))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve cost res grad costate check(mod.handle, ccall((:almpc_get_certificate, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mod.handle, pf(cost), pf(res), pf(grad), pf(costate)))
    return cost, res, grad, costate
end
"`certificate!` into fresh arrays: `certificate(mod; cost = true, res = true, grad = false, costate = false) -> (cost, res, grad, costate)`"
function certificate(mod::HipModeler; cost::Bool = true, res::Bool = true, grad::Bool = false, costate::Bool = false)
    return certificate!(mod, cost ? Vector{Float64}(undef, mod.batch) : nothing, res ? Vector{Float64}(undef, mod.batch) : nothing,
                        grad ? Array{Float64,3}(undef, mod.m, mod.N, mod.batch) : nothing,
                        costate ? Array{Float64,3}(undef, mod.n, mod.N + 1, mod.batch) : nothing)
end
"device pointers of the last certificate (`almpc_device_certificate`): `C_NULL` for what was not computed"
function device_certificate(mod::HipModeler)
    pc, pr, pg, pl = Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL), Ref{Ptr{Float64}}(C_NULL)
    check(mod.handle, ccall((:almpc_device_certificate, libalmpc), Cint,
                            (Ptr{Cvoid}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}), mod.handle, pc, pr, pg, pl))
    return pc[], pr[], pg[], pl[]
end

# ---- ... of a step of a time-varying design (include/almpc.h "Certificate of a step of a time-varying design"): ALMPC_CERT_STATES = 16
"`almpc_set_keep_stage_models`: the next `almpc_design_ltv` keeps its stage models on the device for `certificate_ltv` (batch N n (n + m + 1) doubles)"
set_keep_stage_models(mod::HipModeler, on::Bool = true) =
    check(mod.handle, ccall((:almpc_set_keep_stage_models, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, on ? 1 : 0))
"""
    certificate_ltv!(mod, cost, res, grad, costate, x, e_x)

The certificate of the last step of an `almpc_design_ltv` design made with `set_keep_stage_models` (`almpc_certificate_ltv` +
`almpc_get_certificate_ltv`) into the caller's arrays; `nothing` = not wanted.  `cost`, `res` (batch), `grad` (m x N x batch) and
`costate` (n x (N+1) x batch; `costate[:, k+1]` is d cost / d c_k) as `certificate!`'s; `x`, `e_x` (n x (N+1) x batch): the predicted
states xbar + dx of the linearised dynamics and x - x_ref.
"""
function certificate_ltv!(mod::HipModeler, cost::Union{Nothing,Array{Float64}}, res::Union{Nothing,Array{Float64}},
                          grad::Union{Nothing,Array{Float64}}, costate::Union{Nothing,Array{Float64}},
                          x::Union{Nothing,Array{Float64}}, e_x::Union{Nothing,Array{Float64}})
    traj = mod.n * (mod.N + 1) * mod.batch
    for (name, a, len) in (("cost", cost, mod.batch), ("res", res, mod.batch), ("grad", grad, mod.m * mod.N * mod.batch), ("costate", costate, traj),
                           ("x", x, traj), ("e_x", e_x, traj))
        a === nothing || length(a) == len || throw(DimensionMismatch("$name holds $(length(a)) values, the solver writes $len"))
    end
    want = cert_mask(cost, res, grad, costate) | UInt32((x === nothing && e_x === nothing) ? 0 : 16)
    want != 0 || error("certificate_ltv: nothing asked for")
    check(mod.handle, ccall((:almpc_certificate_ltv, libalmpc), Cint, (Ptr{Cvoid}, UInt32), mod.handle, want))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve cost res grad costate x e_x check(mod.handle, ccall((:almpc_get_certificate_ltv, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        mod.handle, pf(cost), pf(res), pf(grad), pf(costate), pf(x), pf(e_x)))
    return cost, res, grad, costate, x, e_x
end
"`certificate_ltv!` into fresh arrays: `certificate_ltv(mod; cost, res, grad, costate, states) -> (cost, res, grad, costate, x, e_x)`"
function certificate_ltv(mod::HipModeler; cost::Bool = true, res::Bool = true, grad::Bool = false, costate::Bool = false, states::Bool = true)
    traj() = Array{Float64,3}(undef, mod.n, mod.N + 1, mod.batch)
    return certificate_ltv!(mod, cost ? Vector{Float64}(undef, mod.batch) : nothing, res ? Vector{Float64}(undef, mod.batch) : nothing,
                            grad ? Array{Float64,3}(undef, mod.m, mod.N, mod.batch) : nothing, costate ? traj() : nothing,
                            states ? traj() : nothing, states ? traj() : nothing)
end
"device pointers of the last `certificate_ltv` (`almpc_device_certificate_ltv`): `C_NULL` for what was not computed"
function device_certificate_ltv(mod::HipModeler)
    ps = ntuple(_ -> Ref{Ptr{Float64}}(C_NULL), 6)
    check(mod.handle, ccall((:almpc_device_certificate_ltv, libalmpc), Cint,
                            (Ptr{Cvoid}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}, Ref{Ptr{Float64}}),
                            mod.handle, ps[1], ps[2], ps[3], ps[4], ps[5], ps[6]))
    return map(p -> p[], ps)
end
"""
    relin_fnn_certificate!(mod, cost, res, grad, costate)

`certificate!` for the last step of the re-linearisation pipeline (`almpc_relin_fnn_certificate` + `almpc_get_certificate`): with that
step's own models, terminal weights and weights.
"""
function relin_fnn_certificate!(mod::HipModeler, cost::Union{Nothing,Array{Float64}}, res::Union{Nothing,Array{Float64}},
                                grad::Union{Nothing,Array{Float64}}, costate::Union{Nothing,Array{Float64}})
    check_cert_sizes(mod.n, mod.m, mod.N, mod.batch, cost, res, grad, costate)
    check(mod.handle, ccall((:almpc_relin_fnn_certificate, libalmpc), Cint, (Ptr{Cvoid}, UInt32), mod.handle, cert_mask(cost, res, grad, costate)))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve cost res grad costate check(mod.handle, ccall((:almpc_get_certificate, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mod.handle, pf(cost), pf(res), pf(grad), pf(costate)))
    return cost, res, grad, costate
end
"`relin_fnn_certificate!` into fresh arrays"
function relin_fnn_certificate(mod::HipModeler; cost::Bool = true, res::Bool = true, grad::Bool = false, costate::Bool = false)
    return relin_fnn_certificate!(mod, cost ? Vector{Float64}(undef, mod.batch) : nothing, res ? Vector{Float64}(undef, mod.batch) : nothing,
                                  grad ? Array{Float64,3}(undef, mod.m, mod.N, mod.batch) : nothing,
                                  costate ? Array{Float64,3}(undef, mod.n, mod.N + 1, mod.batch) : nothing)
end

# almpc_param_grads (include/almpc.h): host pointers, C_NULL = not wanted
struct ParamGrads
    x0::Ptr{Float64}; f::Ptr{Float64}; u_ref::Ptr{Float64}; u_min::Ptr{Float64}; u_max::Ptr{Float64}
    Q::Ptr{Float64}; P::Ptr{Float64}; A::Ptr{Float64}; R::Ptr{Float64}; S::Ptr{Float64}; B::Ptr{Float64}
    rows::Ptr{Int32}
end
const PARAM_GROUPS = (:x0, :f, :u_ref, :u_min, :u_max, :Q, :P, :A, :R, :S, :B)
# the arrays of the wanted groups (batch last) and the struct that points at them; keep the arrays alive around the call
function param_grad_arrays(n, m, N, batch, want)
    all(k -> k in PARAM_GROUPS, want) || error("sensitivity_params_vjp: want must be a subset of $(PARAM_GROUPS)")
    dims = Dict(:x0 => (n, batch), :f => (m, N, batch), :u_ref => (m, N, batch), :u_min => (m, batch), :u_max => (m, batch),
                :Q => (n, n, batch), :P => (n, n, batch), :A => (n, n, batch), :R => (m, m, batch), :S => (m, m, batch), :B => (n, m, batch))
    out = Dict{Symbol,Any}(k => Array{Float64}(undef, dims[k]...) for k in want)
    out[:rows] = Vector{Int32}(undef, batch)
    pf(k) = haskey(out, k) ? pointer(out[k]) : Ptr{Float64}(C_NULL)
    return out, ParamGrads(pf(:x0), pf(:f), pf(:u_ref), pf(:u_min), pf(:u_max), pf(:Q), pf(:P), pf(:A), pf(:R), pf(:S), pf(:B), pointer(out[:rows]))
end
"""
    sensitivity_params_vjp(mod, g_u, g_x = nothing; want = PARAM_GROUPS, act_tol = 0.0, terminal = :data) -> Dict

Gradients of the loss of `sensitivity_vjp` in the problem data, per instance (`almpc_sensitivity_params_vjp`): `:x0` n x batch, `:f` and
`:u_ref` m x N x batch, `:u_min`, `:u_max` m x batch, `:Q`, `:P`, `:A` n x n x batch, `:R`, `:S` m x m x batch, `:B` n x m x batch, and
`:rows`.  For a shared design the caller sums over the batch.  `terminal = :dare` (`almpc_sensitivity_params_vjp_dare`): the terminal
weight P = are(Discrete, A, B, Q, R) of the reference's own problem is followed into `:Q`, `:R`, `:A`, `:B`, and the Dict carries
`:dare_status` (0: followed; else that instance keeps its `:data` values).
"""
function sensitivity_params_vjp(mod::HipModeler, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing;
                                want = PARAM_GROUPS, act_tol::Real = 0.0, terminal::Symbol = :data)
    terminal in (:data, :dare) || error("sensitivity_params_vjp: terminal must be :data or :dare")
    check_sens_sizes(mod.n, mod.m, mod.N, mod.batch, g_u, g_x)
    out, pg = param_grad_arrays(mod.n, mod.m, mod.N, mod.batch, want)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    if terminal === :dare
        st = out[:dare_status] = Vector{Int32}(undef, mod.batch)
        GC.@preserve g_x out check(mod.handle, ccall((:almpc_sensitivity_params_vjp_dare, libalmpc), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ref{ParamGrads}, Ptr{Int32}), mod.handle, g_u, px, act_tol, Ref(pg), st))
        return out
    end
    GC.@preserve g_x out check(mod.handle, ccall((:almpc_sensitivity_params_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ref{ParamGrads}), mod.handle, g_u, px, act_tol, Ref(pg)))
    return out
end

"library defaults of the options (OSQP's, plus the documented changes)"
function default_opts()
    o = Ref(AlmpcOpts())
    ccall((:almpc_default_opts, libalmpc), Cvoid, (Ref{AlmpcOpts},), o)
    return o[]
end
# timing (handles created with ALMPC_FLAG_TIMING = 0x1): per-stage milliseconds of the last step / sums since the last reset
function get_timing(mod::HipModeler)
    t = zeros(Float32, 4)
    check(mod.handle, ccall((:almpc_get_timing, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                            mod.handle, pointer(t, 1), pointer(t, 2), pointer(t, 3), pointer(t, 4)))
    return (admm_ms = t[1], polish_ms = t[2], rollout_ms = t[3], total_ms = t[4])
end
timing_reset!(mod::HipModeler, reserve_steps::Integer = 0) =
    check(mod.handle, ccall((:almpc_timing_reset, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, reserve_steps))
timing_set_stride!(mod::HipModeler, every::Integer) =
    check(mod.handle, ccall((:almpc_timing_set_stride, libalmpc), Cint, (Ptr{Cvoid}, Cint), mod.handle, every))
function timing_summary(mod::HipModeler)
    steps = Ref{Cint}(0); t = zeros(Float64, 4)
    check(mod.handle, ccall((:almpc_timing_summary, libalmpc), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mod.handle, steps, pointer(t, 1), pointer(t, 2), pointer(t, 3), pointer(t, 4)))
    return (steps = Int(steps[]), admm_ms = t[1], polish_ms = t[2], rollout_ms = t[3], total_ms = t[4])
end
"per recorded step its four stage times in ms (rows: admm, polish, rollout, total), at most `cap` steps"
function timing_samples(mod::HipModeler, cap::Integer = 4096)
    cnt = Ref{Cint}(0); t = zeros(Float32, cap, 4)
    check(mod.handle, ccall((:almpc_timing_samples, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                            mod.handle, cap, cnt, pointer(t, 1), pointer(t, cap + 1), pointer(t, 2cap + 1), pointer(t, 3cap + 1)))
    return t[1:min(cap, Int(cnt[])), :]
end
function relin_timing(mod::HipModeler)
    t = zeros(Float32, 3)
    check(mod.handle, ccall((:almpc_relin_fnn_timing, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                            mod.handle, pointer(t, 1), pointer(t, 2), pointer(t, 3)))
    return (jacobian_ms = t[1], design_ms = t[2], step_ms = t[3])
end
"diagnostic: fill the LDS of every CU with NaN patterns before a step (a kernel that reads LDS it did not write then shows)"
debug_poison_lds!(mod::HipModeler) = check(mod.handle, ccall((:almpc_debug_poison_lds, libalmpc), Cint, (Ptr{Cvoid},), mod.handle))

# ---- one Julia process, several GPUs (almpc_group_*): the reference API is one process, one call (src/main/main_mpc.jl:22-53) ----
mutable struct HipGroup
    group::Ptr{Cvoid}
    n::Int; m::Int; N::Int; batch::Int
    opts::AlmpcOpts
end

function gcheck(g, rc)
    rc == 0 && return
    error("libalmpc group error $rc: " * unsafe_string(ccall((:almpc_group_last_error, libalmpc), Cstring, (Ptr{Cvoid},), g)))
end

"handle i (1-based) of the group as a HipModeler on its shard: for the per-handle options and anything the group calls do not cover"
function group_handle(g::HipGroup, i::Integer)
    h = ccall((:almpc_group_handle, libalmpc), Ptr{Cvoid}, (Ptr{Cvoid}, Cint), g.group, i - 1)
    h == C_NULL && throw(BoundsError(g, i))
    return HipModeler(h, g.n, g.m, g.N, group_shard(g, i)[2], g.opts)    # (no finalizer: the group owns the handle)
end
"(first instance (1-based), count) of handle i's contiguous shard"
function group_shard(g::HipGroup, i::Integer)
    f, c = Ref{Cint}(0), Ref{Cint}(0)
    gcheck(g.group, ccall((:almpc_group_shard, libalmpc), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ref{Cint}), g.group, i - 1, f, c))
    return Int(f[]) + 1, Int(c[])
end

"`design_hip` over several devices: `devices` lists one HIP device id per shard (`mpc_batch` instances are cut into contiguous shards)"
function group_design_hip(A::Matrix{Float64}, B::Matrix{Float64}, Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64},
                          umin::Vector{Float64}, umax::Vector{Float64}, N::Int; batch::Int, devices::Vector{Int},
                          x_ref::Matrix{Float64}, u_ref::Matrix{Float64}, opts::AlmpcOpts = AlmpcOpts(),
                          xmin::Union{Nothing,Vector{Float64}} = nothing, xmax::Union{Nothing,Vector{Float64}} = nothing,
                          terminal::String = "none", rho_profile::String = "scalar", P::Union{Nothing,Matrix{Float64}} = nothing)
    n, m = size(B)
    terminal == "contractive" && error("terminal ingredient \"contractive\" is a quadratic constraint (src/sub/design_mpc.jl:333-340), not a QP row")
    gref = Ref{Ptr{Cvoid}}(C_NULL)
    devs = Cint.(devices)
    rc = ccall((:almpc_group_create, libalmpc), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Ptr{Cint}, UInt32),
               gref, n, m, N, batch, length(devs), devs, 0)
    rc == 0 || error("almpc_group_create failed ($rc): are the devices visible? (there is no CPU fallback)")
    g = HipGroup(gref[], n, m, N, batch, opts)
    finalizer(x -> ccall((:almpc_group_destroy, libalmpc), Cvoid, (Ptr{Cvoid},), x.group), g)
    for i in 1:ccall((:almpc_group_size, libalmpc), Cint, (Ptr{Cvoid},), g.group)
        h = group_handle(g, i).handle
        check(h, ccall((:almpc_set_terminal_equality, libalmpc), Cint, (Ptr{Cvoid}, Cint), h, terminal == "equality" ? 1 : 0))
        check(h, ccall((:almpc_set_rho_profile, libalmpc), Cint, (Ptr{Cvoid}, Cint), h, rho_profile == "stiffness" ? 1 : 0))
    end
    pP = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    pxmin = xmin === nothing ? Ptr{Float64}(C_NULL) : pointer(xmin)
    pxmax = xmax === nothing ? Ptr{Float64}(C_NULL) : pointer(xmax)
    GC.@preserve P xmin xmax gcheck(g.group, ccall((:almpc_group_design_shared, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   g.group, A, B, Q, R, S, pP, umin, umax, pxmin, pxmax, opts.rho, opts.sigma))
    gcheck(g.group, ccall((:almpc_group_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), g.group, x_ref, u_ref, 0))
    return g
end

function group_update_initialization!(g::HipGroup, x0::VecOrMat{Float64})
    length(x0) == g.n * g.batch || throw(DimensionMismatch("x0 must hold n x batch values"))
    gcheck(g.group, ccall((:almpc_group_update_initialization, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), g.group, x0))
end
function group_calculate_async!(g::HipGroup)
    o = Ref(g.opts)
    gcheck(g.group, ccall((:almpc_group_calculate_async, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), g.group, o))
end
group_synchronize!(g::HipGroup) = gcheck(g.group, ccall((:almpc_group_synchronize, libalmpc), Cint, (Ptr{Cvoid},), g.group))
function group_calculate!(g::HipGroup)
    o = Ref(g.opts)
    gcheck(g.group, ccall((:almpc_group_calculate, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), g.group, o))
end
"results of the whole batch (any array may be `nothing`); `u0`: m x batch first inputs; returns the per-instance status"
function group_read_results!(g::HipGroup; x = nothing, e_x = nothing, u = nothing, e_u = nothing, u0 = nothing)
    nx, nu = g.n * (g.N + 1) * g.batch, g.m * g.N * g.batch
    for (name, a, want) in (("x", x, nx), ("e_x", e_x, nx), ("u", u, nu), ("e_u", e_u, nu), ("u0", u0, g.m * g.batch))
        a === nothing || length(a) == want || throw(DimensionMismatch("$name holds $(length(a)) values, the group writes $want"))
    end
    status = Vector{Int32}(undef, g.batch)
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve x e_x u e_u u0 gcheck(g.group, ccall((:almpc_group_get_results, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        g.group, pf(x), pf(e_x), pf(u), pf(e_u), pf(u0), status, C_NULL, C_NULL))
    return throw_on_status(status; strict = g.opts.polish != 0)
end


# ---- group forms of everything a handle can do (include/almpc.h: almpc_group_*) ----
"options of every handle of the group (take effect at the next design)"
function group_set_state_rows!(g::HipGroup; xmin::Union{Nothing,Vector{Float64}} = nothing, xmax::Union{Nothing,Vector{Float64}} = nothing,
                               terminal::String = "none")
    (xmin === nothing) == (xmax === nothing) || error("give both xmin and xmax or neither")
    gcheck(g.group, ccall((:almpc_group_set_terminal_equality, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, terminal == "equality" ? 1 : 0))
    pmin = xmin === nothing ? Ptr{Float64}(C_NULL) : pointer(xmin)
    pmax = xmax === nothing ? Ptr{Float64}(C_NULL) : pointer(xmax)
    GC.@preserve xmin xmax gcheck(g.group, ccall((:almpc_group_set_state_box, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), g.group, pmin, pmax))
    return g
end
group_set_rho_profile!(g::HipGroup, profile::String) =
    gcheck(g.group, ccall((:almpc_group_set_rho_profile, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, profile == "stiffness" ? 1 : 0))
group_set_terminal_weight!(g::HipGroup, mode::Symbol) =
    gcheck(g.group, ccall((:almpc_group_set_terminal_weight, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, mode === :dare_device ? 1 : 0))
group_set_model_time!(g::HipGroup, mode::Symbol, Ts::Real = 0.0) =
    gcheck(g.group, ccall((:almpc_group_set_model_time, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble), g.group, mode === :continuous ? 1 : 0, Ts))
group_set_structured_fallback!(g::HipGroup, on::Bool) =
    gcheck(g.group, ccall((:almpc_group_set_structured_fallback, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, on ? 1 : 0))

"`sensitivity` for the whole batch (`almpc_group_sensitivity` + `almpc_group_get_sensitivity`)"
function group_sensitivity(g::HipGroup; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(g.n, g.m, g.N, g.batch, K0, dU, dX)
    gcheck(g.group, ccall((:almpc_group_sensitivity, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), g.group, sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx gcheck(g.group, ccall((:almpc_group_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), g.group, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_vjp` for the whole batch (`almpc_group_sensitivity_vjp`)"
function group_sensitivity_vjp(g::HipGroup, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(g.n, g.m, g.N, g.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, g.n, g.batch), Vector{Int32}(undef, g.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x gcheck(g.group, ccall((:almpc_group_sensitivity_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), g.group, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"`sensitivity_stagewise` for the whole batch (`almpc_group_sensitivity_stagewise` + `almpc_group_get_sensitivity`)"
function group_sensitivity_stagewise(g::HipGroup; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(g.n, g.m, g.N, g.batch, K0, dU, dX)
    gcheck(g.group, ccall((:almpc_group_sensitivity_stagewise, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), g.group,
                          sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx gcheck(g.group, ccall((:almpc_group_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), g.group, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_stagewise_vjp` for the whole batch (`almpc_group_sensitivity_stagewise_vjp`)"
function group_sensitivity_stagewise_vjp(g::HipGroup, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(g.n, g.m, g.N, g.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, g.n, g.batch), Vector{Int32}(undef, g.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x gcheck(g.group, ccall((:almpc_group_sensitivity_stagewise_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), g.group, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"`sensitivity_stagewise_rate` for the whole batch (`almpc_group_sensitivity_stagewise_rate` + `almpc_group_get_sensitivity`)"
function group_sensitivity_stagewise_rate(g::HipGroup; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol::Real = 0.0)
    k, du, dx, rows = sens_arrays(g.n, g.m, g.N, g.batch, K0, dU, dX)
    gcheck(g.group, ccall((:almpc_group_sensitivity_stagewise_rate, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble), g.group,
                          sens_mask(K0, dU, dX), act_tol))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx gcheck(g.group, ccall((:almpc_group_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), g.group, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_stagewise_rate_vjp` for the whole batch (`almpc_group_sensitivity_stagewise_rate_vjp`)"
function group_sensitivity_stagewise_rate_vjp(g::HipGroup, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing; act_tol::Real = 0.0)
    check_sens_sizes(g.n, g.m, g.N, g.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, g.n, g.batch), Vector{Int32}(undef, g.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x gcheck(g.group, ccall((:almpc_group_sensitivity_stagewise_rate_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Int32}), g.group, g_u, px, act_tol, g_x0, rows))
    return g_x0, rows
end
"`certificate!` for the whole batch (`almpc_group_certificate` + `almpc_group_get_certificate`)"
function group_certificate!(g::HipGroup, cost::Union{Nothing,Array{Float64}}, res::Union{Nothing,Array{Float64}},
                            grad::Union{Nothing,Array{Float64}}, costate::Union{Nothing,Array{Float64}})
    check_cert_sizes(g.n, g.m, g.N, g.batch, cost, res, grad, costate)
    gcheck(g.group, ccall((:almpc_group_certificate, libalmpc), Cint, (Ptr{Cvoid}, UInt32), g.group, cert_mask(cost, res, grad, costate)))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve cost res grad costate gcheck(g.group, ccall((:almpc_group_get_certificate, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), g.group, pf(cost), pf(res), pf(grad), pf(costate)))
    return cost, res, grad, costate
end
"`certificate` for the whole batch"
function group_certificate(g::HipGroup; cost::Bool = true, res::Bool = true, grad::Bool = false, costate::Bool = false)
    return group_certificate!(g, cost ? Vector{Float64}(undef, g.batch) : nothing, res ? Vector{Float64}(undef, g.batch) : nothing,
                              grad ? Array{Float64,3}(undef, g.m, g.N, g.batch) : nothing,
                              costate ? Array{Float64,3}(undef, g.n, g.N + 1, g.batch) : nothing)
end
"`relin_fnn_certificate!` for the whole batch (`almpc_group_relin_fnn_certificate` + `almpc_group_get_certificate`)"
function group_relin_fnn_certificate!(g::HipGroup, cost::Union{Nothing,Array{Float64}}, res::Union{Nothing,Array{Float64}},
                                      grad::Union{Nothing,Array{Float64}}, costate::Union{Nothing,Array{Float64}})
    check_cert_sizes(g.n, g.m, g.N, g.batch, cost, res, grad, costate)
    gcheck(g.group, ccall((:almpc_group_relin_fnn_certificate, libalmpc), Cint, (Ptr{Cvoid}, UInt32), g.group, cert_mask(cost, res, grad, costate)))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve cost res grad costate gcheck(g.group, ccall((:almpc_group_get_certificate, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), g.group, pf(cost), pf(res), pf(grad), pf(costate)))
    return cost, res, grad, costate
end
"`relin_fnn_certificate` for the whole batch"
function group_relin_fnn_certificate(g::HipGroup; cost::Bool = true, res::Bool = true, grad::Bool = false, costate::Bool = false)
    return group_relin_fnn_certificate!(g, cost ? Vector{Float64}(undef, g.batch) : nothing, res ? Vector{Float64}(undef, g.batch) : nothing,
                                        grad ? Array{Float64,3}(undef, g.m, g.N, g.batch) : nothing,
                                        costate ? Array{Float64,3}(undef, g.n, g.N + 1, g.batch) : nothing)
end
"`sensitivity_params_vjp` for the whole batch (`almpc_group_sensitivity_params_vjp`, `almpc_group_sensitivity_params_vjp_dare`)"
function group_sensitivity_params_vjp(g::HipGroup, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing;
                                      want = PARAM_GROUPS, act_tol::Real = 0.0, terminal::Symbol = :data)
    terminal in (:data, :dare) || error("group_sensitivity_params_vjp: terminal must be :data or :dare")
    check_sens_sizes(g.n, g.m, g.N, g.batch, g_u, g_x)
    out, pg = param_grad_arrays(g.n, g.m, g.N, g.batch, want)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    if terminal === :dare
        st = out[:dare_status] = Vector{Int32}(undef, g.batch)
        GC.@preserve g_x out gcheck(g.group, ccall((:almpc_group_sensitivity_params_vjp_dare, libalmpc), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ref{ParamGrads}, Ptr{Int32}), g.group, g_u, px, act_tol, Ref(pg), st))
        return out
    end
    GC.@preserve g_x out gcheck(g.group, ccall((:almpc_group_sensitivity_params_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ref{ParamGrads}), g.group, g_u, px, act_tol, Ref(pg)))
    return out
end
"`sensitivity_rows` for the whole batch (`almpc_group_sensitivity_rows` + `almpc_group_get_sensitivity`)"
function group_sensitivity_rows(g::HipGroup; K0::Bool = true, dU::Bool = false, dX::Bool = false, act_tol_u::Real = 0.0, act_tol_x::Real = 0.0)
    k, du, dx, rows = sens_arrays(g.n, g.m, g.N, g.batch, K0, dU, dX)
    gcheck(g.group, ccall((:almpc_group_sensitivity_rows, libalmpc), Cint, (Ptr{Cvoid}, UInt32, Cdouble, Cdouble), g.group,
                          sens_mask(K0, dU, dX), act_tol_u, act_tol_x))
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve k du dx gcheck(g.group, ccall((:almpc_group_get_sensitivity, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), g.group, pf(k), pf(du), pf(dx), rows))
    return k, du, dx, rows
end
"`sensitivity_rows_vjp` for the whole batch (`almpc_group_sensitivity_rows_vjp`)"
function group_sensitivity_rows_vjp(g::HipGroup, g_u::Array{Float64}, g_x::Union{Nothing,Array{Float64}} = nothing;
                                    act_tol_u::Real = 0.0, act_tol_x::Real = 0.0)
    check_sens_sizes(g.n, g.m, g.N, g.batch, g_u, g_x)
    g_x0, rows = Matrix{Float64}(undef, g.n, g.batch), Vector{Int32}(undef, g.batch)
    px = g_x === nothing ? Ptr{Float64}(C_NULL) : pointer(g_x)
    GC.@preserve g_x gcheck(g.group, ccall((:almpc_group_sensitivity_rows_vjp, libalmpc), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Ptr{Float64}, Ptr{Int32}), g.group, g_u, px, act_tol_u, act_tol_x, g_x0, rows))
    return g_x0, rows
end

"`design_batched!` for the whole batch: `A_batch` n x n x batch, `B_batch` n x m x batch, `P` nothing | n x n | n x n x batch"
function group_design_batched!(g::HipGroup, A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q::Matrix{Float64}, R::Matrix{Float64},
                               S::Matrix{Float64}, P, umin::Vector{Float64}, umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64})
    size(A_batch, 3) == g.batch && size(B_batch, 3) == g.batch || throw(DimensionMismatch("one model per instance"))
    pptr = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    pinst = (P !== nothing && ndims(P) == 3) ? 1 : 0
    GC.@preserve P gcheck(g.group, ccall((:almpc_group_design_batched, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                    Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   g.group, A_batch, B_batch, Q, R, S, pptr, pinst, umin, umax, g.opts.rho, g.opts.sigma))
    gcheck(g.group, ccall((:almpc_group_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), g.group, x_ref, u_ref, 0))
    return g
end

"`design_batched_weighted!` for the whole batch: `Q_batch` n x n x batch, `R_batch` / `S_batch` m x m x batch (`S_batch` may be nothing)"
function group_design_batched_weighted!(g::HipGroup, A_batch::Array{Float64,3}, B_batch::Array{Float64,3}, Q_batch::Array{Float64,3},
                                        R_batch::Array{Float64,3}, S_batch::Union{Nothing,Array{Float64,3}}, P, umin::Vector{Float64},
                                        umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64})
    all(size(M, 3) == g.batch for M in (A_batch, B_batch, Q_batch, R_batch)) || throw(DimensionMismatch("one model and one weight set per instance"))
    S_batch === nothing || size(S_batch, 3) == g.batch || throw(DimensionMismatch("one S per instance"))
    pptr = P === nothing ? Ptr{Float64}(C_NULL) : pointer(P)
    sptr = S_batch === nothing ? Ptr{Float64}(C_NULL) : pointer(S_batch)
    pinst = (P !== nothing && ndims(P) == 3) ? 1 : 0
    GC.@preserve P S_batch gcheck(g.group, ccall((:almpc_group_design_batched_weighted, libalmpc), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                    Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   g.group, A_batch, B_batch, Q_batch, R_batch, sptr, pptr, pinst, umin, umax, g.opts.rho, g.opts.sigma))
    gcheck(g.group, ccall((:almpc_group_set_reference, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), g.group, x_ref, u_ref, 0))
    return g
end

"`design_relin_fnn!` on every device (BASELINE configs[3]); then `group_relin_step!`, `group_relin_advance!`"
function group_design_relin_fnn!(g::HipGroup, W_in::Matrix{Float64}, W_h::Union{Array{Float64,3},Vector{Matrix{Float64}}}, b_h::Matrix{Float64},
                                 W_out::Matrix{Float64}, activation::Integer, Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64}, P::Matrix{Float64},
                                 umin::Vector{Float64}, umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64}, net::Symbol = :fnn)
    if net === :densenet
        gcheck(g.group, ccall((:almpc_group_relin_densenet_setup, libalmpc), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                       g.group, size(W_in, 1), length(W_h), activation, W_in, densenet_pack(W_h), b_h, W_out, x_ref, u_ref, Q, R, S, P,
                       umin, umax, g.opts.rho, g.opts.sigma))
        return g
    end
    gcheck(g.group, ccall((:almpc_group_relin_fnn_setup, libalmpc), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   g.group, size(W_in, 1), size(W_h, 3), net_code(net, activation), W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax,
                   g.opts.rho, g.opts.sigma))
    return g
end
function group_relin_step!(g::HipGroup; warm::Bool = false, async::Bool = false)
    o0 = g.opts
    o = Ref(AlmpcOpts(o0.rho, o0.sigma, o0.alpha, o0.eps_abs, o0.eps_rel, o0.max_iter, o0.check_every, o0.polish, o0.polish_max_iter,
                      Int32(warm), o0.reserved))
    if async
        gcheck(g.group, ccall((:almpc_group_relin_fnn_step_async, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), g.group, o))
    else
        gcheck(g.group, ccall((:almpc_group_relin_fnn_step, libalmpc), Cint, (Ptr{Cvoid}, Ref{AlmpcOpts}), g.group, o))
    end
end
group_relin_advance!(g::HipGroup) = gcheck(g.group, ccall((:almpc_group_relin_fnn_advance, libalmpc), Cint, (Ptr{Cvoid},), g.group))
group_advance_plant!(g::HipGroup) = gcheck(g.group, ccall((:almpc_group_advance_plant, libalmpc), Cint, (Ptr{Cvoid},), g.group))

"`design_sqp_fnn!` on every device (BASELINE configs[4]); `P` n x n or n x n x batch"
function group_design_sqp_fnn!(g::HipGroup, W_in::Matrix{Float64}, W_h::Union{Array{Float64,3},Vector{Matrix{Float64}}}, b_h::Matrix{Float64}, W_out::Matrix{Float64},
                               activation::Integer, Q::Matrix{Float64}, R::Matrix{Float64}, S::Matrix{Float64}, P::Array{Float64},
                               umin::Vector{Float64}, umax::Vector{Float64}; x_ref::Matrix{Float64}, u_ref::Matrix{Float64}, net::Symbol = :fnn,
                               structured_qp::Bool = false)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_set_structured, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, structured_qp ? 1 : 0))
    if net === :densenet
        gcheck(g.group, ccall((:almpc_group_sqp_densenet_setup, libalmpc), Cint,
                       (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                        Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                       g.group, size(W_in, 1), length(W_h), activation, W_in, densenet_pack(W_h), b_h, W_out, x_ref, u_ref, Q, R, S, P,
                       ndims(P) == 3 ? 1 : 0, umin, umax, g.opts.rho, g.opts.sigma))
        return g
    end
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_setup, libalmpc), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble),
                   g.group, size(W_in, 1), size(W_h, 3), net_code(net, activation), W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, ndims(P) == 3 ? 1 : 0,
                   umin, umax, g.opts.rho, g.opts.sigma))
    return g
end
function group_sqp_start!(g::HipGroup, x0::Matrix{Float64}; u_guess::Union{Nothing,Array{Float64,3}} = nothing)
    length(x0) == g.n * g.batch || throw(DimensionMismatch("x0 must hold n x batch values"))
    pg = u_guess === nothing ? Ptr{Float64}(C_NULL) : pointer(u_guess)
    GC.@preserve u_guess gcheck(g.group, ccall((:almpc_group_sqp_fnn_start, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), g.group, x0, pg))
end
function group_sqp_iterate!(g::HipGroup, iters::Integer; step::Float64 = 1.0, merit_safeguard::Bool = true)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_set_step_rule, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, merit_safeguard ? 1 : 0))
    st, de = zeros(iters), zeros(iters)
    o = Ref(g.opts)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_iterate, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{AlmpcOpts}, Ptr{Float64}, Ptr{Float64}),
                          g.group, iters, step, o, st, de))
    return st, de
end
group_set_sqp_hessian!(g::HipGroup, mode::Symbol) =
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_set_hessian, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, mode === :exact ? 1 : 0))
group_set_sqp_row_multipliers!(g::HipGroup, on::Bool = true) =
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_set_row_multipliers, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, on ? 1 : 0))
function group_state_multipliers(g::HipGroup)
    mu = Array{Float64,3}(undef, g.n, g.N, g.batch)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_state_multipliers, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Float64}), g.group, mu))
    return mu
end
function group_sqp_solve!(g::HipGroup, max_iters::Integer, tol::Float64; merit_safeguard::Bool = true)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_set_step_rule, libalmpc), Cint, (Ptr{Cvoid}, Cint), g.group, merit_safeguard ? 1 : 0))
    st, it, kk = Vector{Int32}(undef, g.batch), Vector{Int32}(undef, g.batch), Vector{Float64}(undef, g.batch)
    o = Ref(g.opts)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_solve, libalmpc), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{AlmpcOpts}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                          g.group, max_iters, tol, o, st, it, kk))
    return st, it, kk
end
function group_sqp_skipped(g::HipGroup)
    sk = Vector{Int32}(undef, g.batch)
    gcheck(g.group, ccall((:almpc_group_sqp_fnn_skipped, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Int32}), g.group, sk))
    return sk
end

"zero-copy input: the handles' pinned x0 slots (n x count_i matrices over library memory); write the states, then `group_update_initialization_staged!`"
function group_x0_staging(g::HipGroup)
    k = ccall((:almpc_group_size, libalmpc), Cint, (Ptr{Cvoid},), g.group)
    slots = Vector{Ptr{Float64}}(undef, k)
    gcheck(g.group, ccall((:almpc_group_x0_staging, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), g.group, slots))
    return slots, [unsafe_wrap(Array, slots[i], (g.n, group_shard(g, i)[2])) for i in 1:k]
end
group_update_initialization_staged!(g::HipGroup, slots::Vector{Ptr{Float64}}) =
    gcheck(g.group, ccall((:almpc_group_update_initialization_staged, libalmpc), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), g.group, slots))

"request the results of the last enqueued step of every device (`want`: mask of ALMPC_WANT_*); returns the group's ticket"
function group_results_async(g::HipGroup, want::Integer)
    # `group_results_wait!` always reads the status (solution or throw, src/main/computation_mpc.jl:41-53): it is part of every request
    t = ccall((:almpc_group_get_results_async, libalmpc), Cint, (Ptr{Cvoid}, UInt32), g.group, UInt32(want) | WANT_STATUS)
    t < 0 && gcheck(g.group, t)
    return t
end
"wait for a ticket of `group_results_async` and gather into the caller's arrays (any may be `nothing`); returns the status vector"
function group_results_wait!(g::HipGroup, ticket::Integer; x = nothing, e_x = nothing, u = nothing, e_u = nothing, u0 = nothing)
    nx, nu = g.n * (g.N + 1) * g.batch, g.m * g.N * g.batch
    for (name, a, want) in (("x", x, nx), ("e_x", e_x, nx), ("u", u, nu), ("e_u", e_u, nu), ("u0", u0, g.m * g.batch))
        a === nothing || length(a) == want || throw(DimensionMismatch("$name holds $(length(a)) values, the group writes $want"))
    end
    status = Vector{Int32}(undef, g.batch)
    pf(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve x e_x u e_u u0 gcheck(g.group, ccall((:almpc_group_get_results_wait, libalmpc), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        g.group, ticket, pf(x), pf(e_x), pf(u), pf(e_u), pf(u0), status, C_NULL, C_NULL))
    return throw_on_status(status; strict = g.opts.polish != 0)
end

# the name BASELINE.json uses; absent from the reference (SURVEY.md section 0): one batched step, host in / host out
function _model_predictive_control_computation(mod::HipModeler, X0::Matrix{Float64}, x, e_x, u, e_u; first_move_only::Bool = false)
    check_result_sizes(mod, x, e_x, u, e_u)
    if mod.mode === :sqp
        update_initialization!(mod, X0)      # the SQP loop restarts from mod.x0 (almpc_sqp_fnn_start), which only this method stores
    else
        update_initialization_async!(mod, X0)
    end
    calculate!(mod, x, e_x, u, e_u; first_move_only = first_move_only)
end
function _model_predictive_control_computation(g::HipGroup, X0::Matrix{Float64}, x, e_x, u, e_u)
    group_update_initialization!(g, X0)
    group_calculate!(g)
    group_read_results!(g; x = x, e_x = e_x, u = u, e_u = e_u)
end

end # module
