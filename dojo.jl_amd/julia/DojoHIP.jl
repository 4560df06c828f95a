# DojoHIP.jl -- thin Julia shim over libdojo_hip.so (include/dojo_hip.h).
#
# NOT EXECUTED IN THE BUILD CONTAINER (no Julia toolchain there); kept deliberately thin: it only
# (a) walks a live Dojo `Mechanism` and fills the C-POD topology, (b) owns a handle, (c) forwards
# step! / simulate! / get_maximal_gradients! for a batch, and (d) installs, on enable!(mechanism), a
# Dojo.mehrotra! method that round-trips that Mechanism through the library (B = 1, body impulses
# JF2/Jτ2 in, solution + μ out) and writes everything mehrotra! mutates back, so that DojoEnvironments
# works unmodified.  The exact call sequence of (d) is replayed from C by tests/c_driver/shim_driver.c.  The same calls are exercised from
# Python by dojo.jl_amd/host/dojo_amd/api.py, which the parity tests drive.
module DojoHIP

using Dojo
using StaticArrays
using Libdl

# The library is opened when the module is LOADED (not when it is precompiled): __init__ puts GPU_MAX_HW_QUEUES into the
# environment before the HIP runtime starts (one hardware queue per environment group of dojo_step_dev / dojo_rollout,
# INTEGRATION.md "Streams and hardware queues"), resolves DOJO_HIP_LIB and dlopens it; every @ccall below goes through a
# dlsym'ed function pointer.
const LIBH = Ref{Ptr{Cvoid}}(C_NULL)
const SYMS = Dict{Symbol,Ptr{Cvoid}}()
function __init__()
    get!(ENV, "GPU_MAX_HW_QUEUES", "24")
    LIBH[] = Libdl.dlopen(get(ENV, "DOJO_HIP_LIB", joinpath(@__DIR__, "..", "csrc", "libdojo_hip.so")))
    empty!(SYMS)
end
fn(name::Symbol) = get!(() -> Libdl.dlsym(LIBH[], name), SYMS, name)

# ---- C PODs (layout identical to include/dojo_hip.h) -------------------------------------------
struct CBody;      mass::Cdouble; inertia::NTuple{9,Cdouble}; end
struct CJointHalf
    nl::Int32; nlim::Int32
    cmask::NTuple{9,Cdouble}; amask::NTuple{9,Cdouble}
    spring::Cdouble; damper::Cdouble
    spring_offset::NTuple{3,Cdouble}; limit_lo::NTuple{3,Cdouble}; limit_hi::NTuple{3,Cdouble}
end
struct CJoint
    parent::Int32; child::Int32; spring_on::Int32; damper_on::Int32
    vertex_parent::NTuple{3,Cdouble}; vertex_child::NTuple{3,Cdouble}; orientation_offset::NTuple{4,Cdouble}
    tra::CJointHalf; rot::CJointHalf
end
struct CContact
    body::Int32; model::Int32; friction_coefficient::Cdouble
    normal::NTuple{3,Cdouble}; tangent::NTuple{6,Cdouble}; origin::NTuple{3,Cdouble}; radius::Cdouble; offset::NTuple{3,Cdouble}
    collision::Int32; child_body::Int32; child_origin::NTuple{3,Cdouble}; child_radius::Cdouble      # SphereSphereCollision (collision = 1)
end
struct CTopology
    n_bodies::Int32; n_joints::Int32; n_contacts::Int32; reserved::Int32
    timestep::Cdouble; input_scaling::Cdouble; gravity::NTuple{3,Cdouble}
    bodies::Ptr{CBody}; joints::Ptr{CJoint}; contacts::Ptr{CContact}
end
struct CSolverOptions
    rtol::Cdouble; btol::Cdouble; undercut::Cdouble; no_progress_undercut::Cdouble
    max_iter::Int32; max_ls::Int32; no_progress_max::Int32; reserved::Int32
end

pad(v, n) = ntuple(i -> i <= length(v) ? Float64(v[i]) : 0.0, n)
rowmajor(M) = pad(vec(permutedims(Matrix(M))), 9)          # k x 3 mask -> 9 doubles, row-major, zero padded

function half(j::Dojo.Joint{T,Nλ,Nb,N,Nb½}) where {T,Nλ,Nb,N,Nb½}
    lo = Nb½ > 0 ? j.joint_limits[1] : Float64[]
    hi = Nb½ > 0 ? j.joint_limits[2] : Float64[]
    CJointHalf(Nλ, Nb½, rowmajor(Dojo.constraint_mask(j)), rowmajor(Dojo.nullspace_mask(j)),
               j.spring, j.damper, pad(j.spring_offset, 3), pad(lo, 3), pad(hi, 3))
end

"walk a Mechanism (bodies / joints / contacts in their live order) -> C arrays"
function export_topology(m::Dojo.Mechanism{T,Nn,Ne,Nb,Ni}) where {T,Nn,Ne,Nb,Ni}
    bidx(id) = id == 0 ? Int32(-1) : Int32(id - Ne - 1)      # node id -> 0-based index into mechanism.bodies
    bodies = [CBody(b.mass, pad(vec(permutedims(Matrix(b.inertia))), 9)) for b in m.bodies]
    joints = [CJoint(bidx(j.parent_id), bidx(j.child_id), Int32(j.spring), Int32(j.damper),
                     pad(j.translational.vertices[1], 3), pad(j.translational.vertices[2], 3),
                     pad(Dojo.vector(j.rotational.orientation_offset), 4), half(j.translational), half(j.rotational)) for j in m.joints]
    contacts = CContact[]
    for c in m.contacts
        (c.model isa Dojo.NonlinearContact || c.model isa Dojo.ImpactContact || c.model isa Dojo.LinearContact) || error("DojoHIP: unknown contact model")
        impact = c.model isa Dojo.ImpactContact
        col = c.model.collision
        if col isa Dojo.SphereSphereCollision
            # body-body contact (src/contacts/collisions/sphere_sphere.jl): forward only.  Where the child body's joint hangs on the parent body the
            # contact is an edge of the tree (the fast quad builds); between any other two bodies the library carries it as a cut element (general
            # lane-mapping builds, at most two per mechanism, NonlinearContact / ImpactContact).  A child body WITHOUT a joint (test/collisions.jl:2-58)
            # gets a Floating joint to the parent here -- the tree-edge form: no rows; its six inputs come last in the library's u and must stay zero
            # (pad u accordingly).
            cb = bidx(c.child_id)
            if !any(j -> j.child == cb, joints)
                free = CJointHalf(0, 0, ntuple(_ -> 0.0, 9), rowmajor([1.0 0 0; 0 1 0; 0 0 1]), 0.0, 0.0, ntuple(_ -> 0.0, 3), ntuple(_ -> 0.0, 3), ntuple(_ -> 0.0, 3))
                push!(joints, CJoint(bidx(c.parent_id), cb, Int32(0), Int32(0), ntuple(_ -> 0.0, 3), ntuple(_ -> 0.0, 3), (1.0, 0.0, 0.0, 0.0), free, free))
            end
            push!(contacts, CContact(bidx(c.parent_id), impact ? 1 : (c.model isa Dojo.LinearContact ? 2 : 0), impact ? 0.0 : c.model.friction_coefficient, ntuple(_ -> 0.0, 3), ntuple(_ -> 0.0, 6),
                                     pad(col.origin_parent, 3), col.radius_parent, ntuple(_ -> 0.0, 3), Int32(1), cb, pad(col.origin_child, 3), col.radius_child))
            continue
        end
        col isa Dojo.SphereHalfSpaceCollision || error("DojoHIP: only SphereHalfSpaceCollision and SphereSphereCollision are supported")
        # (LinearContact: the library has the reference's friction_parameterization [0 1; 0 -1; 1 0; -1 0] built in, src/contacts/linear.jl:33-38)
        push!(contacts, CContact(bidx(c.parent_id), impact ? 1 : (c.model isa Dojo.LinearContact ? 2 : 0), impact ? 0.0 : c.model.friction_coefficient, pad(col.contact_normal', 3),
                                 impact ? ntuple(_ -> 0.0, 6) : pad(vec(permutedims(Matrix(col.contact_tangent))), 6), pad(col.contact_origin, 3),
                                 col.contact_radius, pad(col.contact_offset, 3), Int32(0), Int32(-1), ntuple(_ -> 0.0, 3), 0.0))
    end
    return bodies, joints, contacts
end

mutable struct BatchedMechanism{T}
    handle::Ptr{Cvoid}
    mechanism::Dojo.Mechanism
    batch::Int
    nz::Int; nx::Int; nu::Int
end

check(rc) = rc == 0 || error("libdojo_hip: " * unsafe_string(@ccall $(fn(:dojo_last_error))()::Cstring))
"the text of the last failure on this handle (per handle; dojo_last_error is process-wide)"
last_error(bm) = unsafe_string(@ccall $(fn(:dojo_handle_error))(bm.handle::Ptr{Cvoid})::Cstring)
kernel_build(bm) = (o = zeros(Int32, 3); check(@ccall $(fn(:dojo_get_kernel_build))(bm.handle::Ptr{Cvoid}, o::Ptr{Int32})::Cint); (o[1], o[2], o[3]))   # (family, MAXC, waves) of the build that steps the handle

function BatchedMechanism(m::Dojo.Mechanism, batch::Int; T=Float32, device::Int=0)
    bodies, joints, contacts = export_topology(m)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve bodies joints contacts begin
        topo = CTopology(length(bodies), length(joints), length(contacts), 0, m.timestep, m.input_scaling,
                         pad(m.gravity, 3), pointer(bodies), pointer(joints), pointer(contacts))
        check(@ccall $(fn(:dojo_create))(Ref(topo)::Ref{CTopology}, batch::Int32, (T == Float32 ? 1 : 0)::Int32, device::Int32, h::Ref{Ptr{Cvoid}})::Cint)
    end
    bm = BatchedMechanism{T}(h[], m, batch, 13length(m.bodies), 12length(m.bodies), Dojo.input_dimension(m))
    finalizer(b -> (@ccall $(fn(:dojo_destroy))(b.handle::Ptr{Cvoid})::Cvoid), bm)
    return bm
end

function set_options!(bm::BatchedMechanism, o::Dojo.SolverOptions)
    c = CSolverOptions(o.rtol, o.btol, o.undercut, o.no_progress_undercut, o.max_iter, o.max_ls, o.no_progress_max, 0)
    check(@ccall $(fn(:dojo_set_options))(bm.handle::Ptr{Cvoid}, Ref(c)::Ref{CSolverOptions})::Cint)
end

# z: nz x B and u: nu x B column-major Julia matrices == the row-major [B, nz] / [B, nu] of the ABI
"step!(mechanism, z, u; opts): batched, returns (z_next, status)"
function Dojo.step!(bm::BatchedMechanism{T}, z::Matrix{T}, u::Matrix{T}; opts=Dojo.SolverOptions{Float64}(), with_gradient::Bool=false) where T
    set_options!(bm, opts)
    zn = similar(z); status = Vector{Int32}(undef, bm.batch); iters = Vector{Int32}(undef, bm.batch)
    check(@ccall $(fn(:dojo_step))(bm.handle::Ptr{Cvoid}, z::Ptr{T}, u::Ptr{T}, zn::Ptr{T}, status::Ptr{Int32}, iters::Ptr{Int32}, with_gradient::Int32)::Cint)
    return zn, status
end

"""
The vector `Dojo.step!(mechanism, z, u)` literally returns is `get_next_state` AFTER `update_state!` (src/simulation/step.jl:28),
i.e. the mechanism's next state advanced once more; `step!(bm, ...)` above returns the mechanism's next state itself (what the
next step and `get_state` consume).  `reference_return(bm, zn)` maps the one to the other.
"""
function reference_return(bm::BatchedMechanism{T}, zn::Matrix{T}) where T
    zr = similar(zn)
    check(@ccall $(fn(:dojo_next_state))(bm.handle::Ptr{Cvoid}, zn::Ptr{T}, zr::Ptr{T})::Cint)
    return zr
end

"get_maximal_gradients!(mechanism, z, u; opts): batched -> (jacobian_state[12Nb,12Nb,B], jacobian_control[12Nb,nu,B])"
function Dojo.get_maximal_gradients!(bm::BatchedMechanism{T}, z::Matrix{T}, u::Matrix{T}; opts=Dojo.SolverOptions{Float64}()) where T
    Dojo.step!(bm, z, u; opts, with_gradient=true)
    dz = Array{T}(undef, bm.nx, bm.nx, bm.batch); du = Array{T}(undef, bm.nu, bm.nx, bm.batch)      # ABI is row-major [B,nx,nx]/[B,nx,nu]
    check(@ccall $(fn(:dojo_gradients))(bm.handle::Ptr{Cvoid}, dz::Ptr{T}, du::Ptr{T})::Cint)
    return permutedims(dz, (2, 1, 3)), permutedims(du, (2, 1, 3))
end

"simulate! with pre-sampled controls U[nu, B, H] -> Z[nz, B, H], status[B, H]"
function Dojo.simulate!(bm::BatchedMechanism{T}, z0::Matrix{T}, U::Array{T,3}; opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(U, 3)
    Z = Array{T}(undef, bm.nz, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    check(@ccall $(fn(:dojo_rollout))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, U::Ptr{T}, H::Int32, Z::Ptr{T}, status::Ptr{Int32})::Cint)
    return Z, status
end

"""
reverse-mode rollout (no counterpart in Dojo.jl): the rollout of `simulate!` and the gradient of a trajectory loss from the recorded IFT
Jacobians, which stay on the device.  G is the cotangent of the loss w.r.t. the state after every step: [nx, B, H] in the coordinates of
dz (`cot_space = :tangent`) or [nz, B, H] w.r.t. the state vector (`:state`).  -> Z[nz, B, H], status[B, H], gU[nu, B, H], gz0[nx, B]
(tangent coordinates).  `set_gradient_mode!(bm, 1)` is the mode whose chain is the derivative of the rollout.
"""
function rollout_gradients(bm::BatchedMechanism{T}, z0::Matrix{T}, U::Array{T,3}, G::Array{T,3}; cot_space::Symbol=:tangent, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(G, 3)
    Z = Array{T}(undef, bm.nz, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    gU = zeros(T, bm.nu, bm.batch, H); gz = Matrix{T}(undef, bm.nx, bm.batch)
    check(@ccall $(fn(:dojo_rollout_gradients))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, (bm.nu > 0 ? pointer(U) : C_NULL)::Ptr{T}, H::Int32, G::Ptr{T},
                                                Int32(cot_space === :state ? 1 : 0)::Int32, Z::Ptr{T}, status::Ptr{Int32}, gU::Ptr{T}, gz::Ptr{T})::Cint)
    return Z, status, gU, gz
end

"""
set_data!(mechanism.contacts, θ) on the live handle (examples/system_identification/utilities.jl:52): θ[5, Nc] =
[friction_coefficient; contact_radius; contact_origin(3)] per contact, shared by all environments.  The handle then steps as one created with θ.
"""
function set_contact_data!(bm::BatchedMechanism, θ::Matrix{Float64})
    check(@ccall $(fn(:dojo_set_contact_data))(bm.handle::Ptr{Cvoid}, θ::Ptr{Float64})::Cint)
    return bm
end

"""
reverse-mode rollout w.r.t. the contact data: get_contact_gradients (src/gradients/contact.jl:1-55) of every step chained as in
examples/system_identification/utilities.jl:42-90, transposed, on the device.  G as in `rollout_gradients`.
-> Z[nz, B, H], status[B, H], gθ[5, Nc] (summed over the batch), gθ_env[5, Nc, B], gU[nu, B, H], gz0[nx, B] (tangent coordinates).
"""
function rollout_data_gradients(bm::BatchedMechanism{T}, z0::Matrix{T}, U::Array{T,3}, G::Array{T,3}; cot_space::Symbol=:tangent, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(G, 3); Nc = length(bm.mechanism.contacts)
    Z = Array{T}(undef, bm.nz, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    gθ = zeros(T, 5, Nc); gθ_env = zeros(T, 5, Nc, bm.batch)
    gU = zeros(T, bm.nu, bm.batch, H); gz = Matrix{T}(undef, bm.nx, bm.batch)
    check(@ccall $(fn(:dojo_rollout_data_gradients))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, (bm.nu > 0 ? pointer(U) : C_NULL)::Ptr{T}, H::Int32, G::Ptr{T},
                                                     Int32(cot_space === :state ? 1 : 0)::Int32, Z::Ptr{T}, status::Ptr{Int32},
                                                     (Nc > 0 ? pointer(gθ) : C_NULL)::Ptr{T}, (Nc > 0 ? pointer(gθ_env) : C_NULL)::Ptr{T}, gU::Ptr{T}, gz::Ptr{T})::Cint)
    return Z, status, gθ, gθ_env, gU, gz
end

"""
forward-mode rollout: `rollout` plus T tangent directions pushed through the recorded step Jacobians in one pass over the record (dojo_rollout_tangents) --
the chain of examples/system_identification/utilities.jl:42-90 on the device.  dz0[nx, T, B] (tangent coordinates), dU[nu, T, B, H], dθ[5Nc, T] (shared by the
batch); each may be `nothing` (= zeros), not all three.  -> Z[nz, B, H], status[B, H], dZ[nx, T, B, H] (or [nz, T, B, H] with tan_space = :state: dq = q ⊗ (0, φ)).
Nothing flows through a failed step: the tangent of the state after it is 0.
"""
function rollout_tangents(bm::BatchedMechanism{T}, z0::Matrix{T}, U::Union{Nothing,Array{T,3}}, H::Integer; dz0::Union{Nothing,Array{T,3}}=nothing,
                          dU::Union{Nothing,Array{T,4}}=nothing, dθ::Union{Nothing,Matrix{T}}=nothing, tan_space::Symbol=:tangent, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    given = [(a, d) for (a, d) in ((dz0, 2), (dU, 2), (dθ, 2)) if a !== nothing]
    isempty(given) && error("rollout_tangents needs at least one of dz0, dU, dθ")
    nT = size(given[1][1], given[1][2])
    all(size(a, d) == nT for (a, d) in given) || error("dz0, dU and dθ hold different numbers of tangents")
    ptr(a) = a === nothing ? Ptr{T}(C_NULL) : pointer(a)
    Z = Array{T}(undef, bm.nz, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    dZ = Array{T}(undef, tan_space === :state ? bm.nz : bm.nx, nT, bm.batch, H)
    check(@ccall $(fn(:dojo_rollout_tangents))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, ((U !== nothing && bm.nu > 0) ? pointer(U) : C_NULL)::Ptr{T}, Int32(H)::Int32, Int32(nT)::Int32,
                                               ptr(dz0)::Ptr{T}, ptr(dU)::Ptr{T}, ptr(dθ)::Ptr{T}, Int32(tan_space === :state ? 1 : 0)::Int32,
                                               Z::Ptr{T}, status::Ptr{Int32}, dZ::Ptr{T})::Cint)
    return Z, status, dZ
end

"mirror of `DojoPolicy` (include/dojo_hip.h): five pointers, six Int32"
struct DojoPolicy
    W::Ptr{Cvoid}; bias::Ptr{Cvoid}; mean::Ptr{Cvoid}; scale::Ptr{Cvoid}; U_ff::Ptr{Cvoid}
    per_env::Int32; act_off::Int32; na::Int32; contact_forces::Int32; contact_init::Int32; reserved::Int32
end

"""
closed-loop rollout: simulate!(mechanism, steps, storage, control!) with the affine feedback policy
u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale)) evaluated on the device between the steps, o_k = get_state of the state step k starts from
(minimal state, then the clamped contact impulses with `contact_forces`).  W[nobs, na] (one policy for all environments) or W[nobs, na, B] (one
per environment; the transposes of the policy matrices: the ABI is row-major), bias[na] / [na, B], mean, scale[nobs], U_ff[nu, B, H]; the policy
drives the inputs act_off + 1 : act_off + na.  -> Z[nz, B, H], OBS[nobs, B, H + 1], U[nu, B, H], status[B, H].
"""
function rollout_policy(bm::BatchedMechanism{T}, z0::Matrix{T}, W::Array{T}, H::Integer; bias::Union{Nothing,Array{T}}=nothing, mean::Union{Nothing,Vector{T}}=nothing,
                        scale::Union{Nothing,Vector{T}}=nothing, U_ff::Union{Nothing,Array{T,3}}=nothing, act_off::Integer=0, contact_forces::Bool=false,
                        contact_init::Integer=0, n_contacts::Integer=0, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    nobs = 2 * bm.nu + (contact_forces ? n_contacts : 0)
    size(W, 1) == nobs || error("W must have nobs = $nobs rows (pass n_contacts with contact_forces)")
    na = size(W, 2)
    Z = Array{T}(undef, bm.nz, bm.batch, H); OBS = Array{T}(undef, nobs, bm.batch, H + 1)
    U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve W bias mean scale U_ff begin
        pol = Ref(DojoPolicy(p(W), p(bias), p(mean), p(scale), p(U_ff), Int32(ndims(W) == 3), Int32(act_off), Int32(na), Int32(contact_forces), Int32(contact_init), Int32(0)))
        check(@ccall $(fn(:dojo_rollout_policy))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, pol::Ptr{DojoPolicy}, Int32(H)::Int32, Z::Ptr{T}, OBS::Ptr{T}, U::Ptr{T}, status::Ptr{Int32})::Cint)
    end
    return Z, OBS, U, status
end

"mirror of `DojoRiccati` (include/dojo_hip.h): fifteen pointers, two Int32"
struct DojoRiccati
    A::Ptr{Cvoid}; Bm::Ptr{Cvoid}; status::Ptr{Cvoid}; lx::Ptr{Cvoid}; lu::Ptr{Cvoid}; lxx::Ptr{Cvoid}; luu::Ptr{Cvoid}; lux::Ptr{Cvoid}; mu::Ptr{Cvoid}
    K::Ptr{Cvoid}; kff::Ptr{Cvoid}; fail::Ptr{Cvoid}; dV::Ptr{Cvoid}; Vx::Ptr{Cvoid}; Vxx::Ptr{Cvoid}
    act_off::Int32; na::Int32
end

"""
the backward pass of iLQR in minimal coordinates (IterativeLQR's backward pass over get_minimal_gradients!, examples/trajectory_optimization) for the whole
batch on the device: dojo_riccati.  n = 2nu; the ABI is row-major, so every matrix is passed TRANSPOSED: A[n, n, B, H] holds jx' and Bm[nu, n, B, H] holds ju' of
every step, lx[n, B, H + 1], lu[na, B, H], lxx[n, n, B, H + 1], luu[na, na, B, H], lux[n, na, B, H] (or `nothing`), mu[B] (or `nothing`), status[B, H] (or `nothing`).
The policy drives the inputs act_off + 1 : act_off + na.
-> K[n, na, B, H] (K_k'), kff[na, B, H], dV[2, B], fail[B] (0, or 1 + the zero-based step whose Cholesky failed), Vx[n, B], Vxx[n, n, B].
"""
function riccati(bm::BatchedMechanism{T}, A::Array{T,4}, Bm::Array{T,4}, lx::Array{T,3}, lu::Array{T,3}, lxx::Array{T,4}, luu::Array{T,4};
                 lux::Union{Nothing,Array{T,4}}=nothing, mu::Union{Nothing,Vector{T}}=nothing, status::Union{Nothing,Matrix{Int32}}=nothing, act_off::Integer=0) where T
    H = size(A, 4); n = 2 * bm.nu; na = size(lu, 1)
    K = Array{T}(undef, n, na, bm.batch, H); kff = Array{T}(undef, na, bm.batch, H); fail = Vector{Int32}(undef, bm.batch)
    dV = Matrix{T}(undef, 2, bm.batch); Vx = Matrix{T}(undef, n, bm.batch); Vxx = Array{T}(undef, n, n, bm.batch)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve A Bm status lx lu lxx luu lux mu K kff fail dV Vx Vxx begin
        r = Ref(DojoRiccati(p(A), p(Bm), p(status), p(lx), p(lu), p(lxx), p(luu), p(lux), p(mu), p(K), p(kff), p(fail), p(dV), p(Vx), p(Vxx), Int32(act_off), Int32(na)))
        check(@ccall $(fn(:dojo_riccati))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, r::Ptr{DojoRiccati})::Cint)
    end
    return K, kff, dV, fail, Vx, Vxx
end

"mirror of `DojoTracking` (include/dojo_hip_trajopt.h): eleven pointers, two Int32"
struct DojoTracking
    x0::Ptr{Cvoid}; Ubar::Ptr{Cvoid}; Xbar::Ptr{Cvoid}; K::Ptr{Cvoid}; kff::Ptr{Cvoid}; alpha::Ptr{Cvoid}
    X::Ptr{Cvoid}; U_out::Ptr{Cvoid}; status::Ptr{Cvoid}; A::Ptr{Cvoid}; Bm::Ptr{Cvoid}
    act_off::Int32; na::Int32
end

"""
simulate! through DojoEnvironments.step! (minimal state in, minimal state out) under the tracking controller u_k = Ubar_k + E (alpha kff_k + K_k (x_k - Xbar_k)),
evaluated on the device between the steps: dojo_rollout_minimal -- the forward pass of iLQR and, with `jacobians`, its linearization, one call each.  n = 2nu;
x0[n, B], Ubar[nu, B, H], Xbar[n, B, H + 1], K[n, na, B, H] (K_k', as `riccati` returns it), kff[na, B, H], alpha[B]; each but x0 and Ubar may be `nothing`
(zeros; alpha: ones).  The controller drives the inputs act_off + 1 : act_off + na.
-> X[n, B, H + 1], U[nu, B, H], status[B, H] and, with `jacobians`, A[n, n, B, H] (jx' of every step), Bm[nu, n, B, H] (ju'), in the handle's gradient mode.
"""
function rollout_minimal(bm::BatchedMechanism{T}, x0::Matrix{T}, Ubar::Array{T,3}; Xbar::Union{Nothing,Array{T,3}}=nothing, K::Union{Nothing,Array{T,4}}=nothing,
                         kff::Union{Nothing,Array{T,3}}=nothing, alpha::Union{Nothing,Vector{T}}=nothing, act_off::Integer=0, na::Integer=bm.nu - act_off,
                         jacobians::Bool=false) where T
    H = size(Ubar, 3); n = 2 * bm.nu
    X = Array{T}(undef, n, bm.batch, H + 1); U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    A = jacobians ? Array{T}(undef, n, n, bm.batch, H) : nothing; Bm = jacobians ? Array{T}(undef, bm.nu, n, bm.batch, H) : nothing
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve x0 Ubar Xbar K kff alpha X U status A Bm begin
        t = Ref(DojoTracking(p(x0), p(Ubar), p(Xbar), p(K), p(kff), p(alpha), p(X), p(U), p(status), p(A), p(Bm), Int32(act_off), Int32(na)))
        check(@ccall $(fn(:dojo_rollout_minimal))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, t::Ptr{DojoTracking})::Cint)
    end
    return jacobians ? (X, U, status, A, Bm) : (X, U, status)
end

"mirror of `DojoControlLimits` (include/dojo_hip_limits.h): the limits lo, hi [na, B] of the driven inputs; either may be NULL"
struct DojoControlLimits
    lo::Ptr{Cvoid}; hi::Ptr{Cvoid}
end

"""
`riccati` under control limits (control-limited DDP, include/dojo_hip_limits.h): dojo_riccati_box.  U[nu, B, H] are the controls the pass is taken around,
lo[na, B] and hi[na, B] the limits of the driven inputs (+-Inf allowed, either may be `nothing`): lo <= U[act, b, k] + kff[:, b, k] <= hi, the rows of K_k of
clamped inputs are zero.  Other arguments and array conventions as in `riccati`.
-> K, kff, dV, fail[B] (0; 1 + k: the Cholesky of step k failed; -(1 + k): the QP of step k failed or its box is empty), active[B, H] (Int64, bit i: input
act_off + i + 1 clamped), qp_iters[B, H], Vx, Vxx.
"""
function riccati_box(bm::BatchedMechanism{T}, A::Array{T,4}, Bm::Array{T,4}, lx::Array{T,3}, lu::Array{T,3}, lxx::Array{T,4}, luu::Array{T,4}, U::Array{T,3};
                     lo::Union{Nothing,Matrix{T}}=nothing, hi::Union{Nothing,Matrix{T}}=nothing, lux::Union{Nothing,Array{T,4}}=nothing,
                     mu::Union{Nothing,Vector{T}}=nothing, status::Union{Nothing,Matrix{Int32}}=nothing, act_off::Integer=0) where T
    H = size(A, 4); n = 2 * bm.nu; na = size(lu, 1)
    K = Array{T}(undef, n, na, bm.batch, H); kff = Array{T}(undef, na, bm.batch, H); fail = Vector{Int32}(undef, bm.batch)
    dV = Matrix{T}(undef, 2, bm.batch); Vx = Matrix{T}(undef, n, bm.batch); Vxx = Array{T}(undef, n, n, bm.batch)
    active = Matrix{Int64}(undef, bm.batch, H); qp_iters = Matrix{Int32}(undef, bm.batch, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve A Bm status lx lu lxx luu lux mu K kff fail dV Vx Vxx U lo hi active qp_iters begin
        r = Ref(DojoRiccati(p(A), p(Bm), p(status), p(lx), p(lu), p(lxx), p(luu), p(lux), p(mu), p(K), p(kff), p(fail), p(dV), p(Vx), p(Vxx), Int32(act_off), Int32(na)))
        lim = Ref(DojoControlLimits(p(lo), p(hi)))
        check(@ccall $(fn(:dojo_riccati_box))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, r::Ptr{DojoRiccati}, lim::Ptr{DojoControlLimits}, U::Ptr{T}, active::Ptr{Int64},
                                              qp_iters::Ptr{Int32})::Cint)
    end
    return K, kff, dV, fail, active, qp_iters, Vx, Vxx
end

"mirror of `DojoStageConstraints` (include/dojo_hip_constraints.h): four pointers, two Int32"
struct DojoStageConstraints
    Cx::Ptr{Cvoid}; Cu::Ptr{Cvoid}; w::Ptr{Cvoid}; y::Ptr{Cvoid}
    nc::Int32; shared::Int32
end

"""
`riccati_box` with the augmented-Lagrangian terms of nc linearized constraint rows per stage added to the step's model inside the kernel
(include/dojo_hip_constraints.h): dojo_riccati_al.  With G = [Cx Cu] the stage gains G' diag(w) G in its Hessian and G' y in its gradient.
Cx[n, nc, B, H + 1] and Cu[na, nc, B, H] (row i of the Jacobian is column i: the C layout [H][B][nc][n] read column-major), or Cx[n, nc], Cu[na, nc] with
`shared`; Cu may be `nothing` (zeros).  w[nc, B, H + 1]: the weight of a row (0: inactive or absent), y[nc, B, H + 1]: its multiplier estimate lambda + w c.
A row with w = y = 0 is not read.  lo, hi `nothing`: no control limits, and U may be `nothing` too.  Other arguments and outputs as in `riccati_box`.
"""
function riccati_al(bm::BatchedMechanism{T}, A::Array{T,4}, Bm::Array{T,4}, lx::Array{T,3}, lu::Array{T,3}, lxx::Array{T,4}, luu::Array{T,4},
                    Cx::Array{T}, w::Array{T,3}, y::Array{T,3}; Cu::Union{Nothing,Array{T}}=nothing, shared::Bool=false, U::Union{Nothing,Array{T,3}}=nothing,
                    lo::Union{Nothing,Matrix{T}}=nothing, hi::Union{Nothing,Matrix{T}}=nothing, lux::Union{Nothing,Array{T,4}}=nothing,
                    mu::Union{Nothing,Vector{T}}=nothing, status::Union{Nothing,Matrix{Int32}}=nothing, act_off::Integer=0) where T
    H = size(A, 4); n = 2 * bm.nu; na = size(lu, 1); nc = size(w, 1)
    K = Array{T}(undef, n, na, bm.batch, H); kff = Array{T}(undef, na, bm.batch, H); fail = Vector{Int32}(undef, bm.batch)
    dV = Matrix{T}(undef, 2, bm.batch); Vx = Matrix{T}(undef, n, bm.batch); Vxx = Array{T}(undef, n, n, bm.batch)
    active = Matrix{Int64}(undef, bm.batch, H); qp_iters = Matrix{Int32}(undef, bm.batch, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    limited = lo !== nothing || hi !== nothing
    GC.@preserve A Bm status lx lu lxx luu lux mu K kff fail dV Vx Vxx U lo hi active qp_iters Cx Cu w y begin
        r = Ref(DojoRiccati(p(A), p(Bm), p(status), p(lx), p(lu), p(lxx), p(luu), p(lux), p(mu), p(K), p(kff), p(fail), p(dV), p(Vx), p(Vxx), Int32(act_off), Int32(na)))
        lim = Ref(DojoControlLimits(p(lo), p(hi)))
        con = Ref(DojoStageConstraints(p(Cx), p(Cu), p(w), p(y), Int32(nc), Int32(shared)))
        GC.@preserve lim begin
            limp = limited ? Base.unsafe_convert(Ptr{DojoControlLimits}, lim) : Ptr{DojoControlLimits}(C_NULL)
            check(@ccall $(fn(:dojo_riccati_al))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, r::Ptr{DojoRiccati}, limp::Ptr{DojoControlLimits},
                                                 p(U)::Ptr{Cvoid}, con::Ptr{DojoStageConstraints}, active::Ptr{Int64}, qp_iters::Ptr{Int32})::Cint)
        end
    end
    return K, kff, dV, fail, active, qp_iters, Vx, Vxx
end

"""
`rollout_minimal` with the driven inputs clamped into [lo, hi] (lo[na, B], hi[na, B]; either may be `nothing`) before they are rounded and stepped:
dojo_rollout_minimal_box, the forward pass of control-limited iLQR.  Everything else as in `rollout_minimal`.
"""
function rollout_minimal_box(bm::BatchedMechanism{T}, x0::Matrix{T}, Ubar::Array{T,3}; lo::Union{Nothing,Matrix{T}}=nothing, hi::Union{Nothing,Matrix{T}}=nothing,
                             Xbar::Union{Nothing,Array{T,3}}=nothing, K::Union{Nothing,Array{T,4}}=nothing, kff::Union{Nothing,Array{T,3}}=nothing,
                             alpha::Union{Nothing,Vector{T}}=nothing, act_off::Integer=0, na::Integer=bm.nu - act_off, jacobians::Bool=false) where T
    H = size(Ubar, 3); n = 2 * bm.nu
    X = Array{T}(undef, n, bm.batch, H + 1); U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    A = jacobians ? Array{T}(undef, n, n, bm.batch, H) : nothing; Bm = jacobians ? Array{T}(undef, bm.nu, n, bm.batch, H) : nothing
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve x0 Ubar Xbar K kff alpha X U status A Bm lo hi begin
        t = Ref(DojoTracking(p(x0), p(Ubar), p(Xbar), p(K), p(kff), p(alpha), p(X), p(U), p(status), p(A), p(Bm), Int32(act_off), Int32(na)))
        lim = Ref(DojoControlLimits(p(lo), p(hi)))
        check(@ccall $(fn(:dojo_rollout_minimal_box))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, t::Ptr{DojoTracking}, lim::Ptr{DojoControlLimits})::Cint)
    end
    return jacobians ? (X, U, status, A, Bm) : (X, U, status)
end

"mirror of `DojoQuadraticCost` (include/dojo_hip_linesearch.h): four pointers, one Int32"
struct DojoQuadraticCost
    Q::Ptr{Cvoid}; R::Ptr{Cvoid}; Qf::Ptr{Cvoid}; goal::Ptr{Cvoid}
    goal_per_problem::Int32
end

"mirror of `DojoLineSearch` (include/dojo_hip_linesearch.h): sixteen pointers, one Float64, two Int32"
struct DojoLineSearch
    X::Ptr{Cvoid}; U::Ptr{Cvoid}; status::Ptr{Cvoid}; alpha::Ptr{Cvoid}; dV::Ptr{Cvoid}; ok::Ptr{Cvoid}; Xcur::Ptr{Cvoid}; Ucur::Ptr{Cvoid}
    J0::Ptr{Cvoid}; J_trial::Ptr{Cvoid}; J_cur::Ptr{Cvoid}; J_acc::Ptr{Cvoid}; choice::Ptr{Cvoid}; alpha_acc::Ptr{Cvoid}; X_new::Ptr{Cvoid}; U_new::Ptr{Cvoid}
    c1::Float64; act_off::Int32; na::Int32
end

"""
The step lengths of a line search side by side (include/dojo_hip_linesearch.h): dojo_rollout_minimal_fan.  The handle has batch B = T P; environment
(tr - 1) P + p is trial tr of problem p.  x0[n, P], Ubar[nu, P, H], Xbar[n, P, H + 1], K[n, na, P, H], kff[na, P, H], lo[na, P], hi[na, P] are per problem,
alpha[P, T] per environment.  lo and hi `nothing`: no limits.  -> X[n, B, H + 1], U[nu, B, H], status[B, H]: `rollout_minimal_box`'s (`rollout_minimal`'s
without limits) on the inputs repeated T times, bit for bit.
"""
function rollout_minimal_fan(bm::BatchedMechanism{T}, trials::Integer, x0::Matrix{T}, Ubar::Array{T,3}; lo::Union{Nothing,Matrix{T}}=nothing,
                             hi::Union{Nothing,Matrix{T}}=nothing, Xbar::Union{Nothing,Array{T,3}}=nothing, K::Union{Nothing,Array{T,4}}=nothing,
                             kff::Union{Nothing,Array{T,3}}=nothing, alpha::Union{Nothing,Matrix{T}}=nothing, act_off::Integer=0, na::Integer=bm.nu - act_off) where T
    H = size(Ubar, 3); n = 2 * bm.nu
    X = Array{T}(undef, n, bm.batch, H + 1); U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    limited = lo !== nothing || hi !== nothing
    GC.@preserve x0 Ubar Xbar K kff alpha X U status lo hi begin
        t = Ref(DojoTracking(p(x0), p(Ubar), p(Xbar), p(K), p(kff), p(alpha), p(X), p(U), p(status), Ptr{Cvoid}(C_NULL), Ptr{Cvoid}(C_NULL), Int32(act_off), Int32(na)))
        lim = Ref(DojoControlLimits(p(lo), p(hi)))
        GC.@preserve lim begin
            limp = limited ? Base.unsafe_convert(Ptr{DojoControlLimits}, lim) : Ptr{DojoControlLimits}(C_NULL)
            check(@ccall $(fn(:dojo_rollout_minimal_fan))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, Int32(trials)::Int32, t::Ptr{DojoTracking}, limp::Ptr{DojoControlLimits})::Cint)
        end
    end
    return X, U, status
end

"""
The selection of a side-by-side line search (include/dojo_hip_linesearch.h): dojo_linesearch_select on the trials X[n, B, H + 1], U[nu, B, H], status[B, H] of
`rollout_minimal_fan`.  alpha[P, T], dV[2, P] (`riccati`'s), Xcur[n, P, H + 1], Ucur[nu, P, H]: the trajectory the pass was taken around.  `cost` = (Q, R, Qf, goal)
(Q and Qf [n, n] and R [na, na], transposed as every matrix here; goal[n] or goal[n, P]): the costs are evaluated on the device in Float64; `nothing`: J_trial[P, T]
and J0[P] are the caller's.  ok[P] (Int32, 0: the problem accepts nothing) and status may be `nothing`.
-> choice[P] (Int32, 0-based trial or -1), alpha_acc[P], J_trial[P, T], J_cur[P], J_acc[P], X_new[n, P, H + 1], U_new[nu, P, H].
"""
function linesearch_select(bm::BatchedMechanism{T}, trials::Integer, X::Array{T,3}, U::Array{T,3}, alpha::Matrix{T}, dV::Matrix{T}, Xcur::Array{T,3}, Ucur::Array{T,3};
                           cost=nothing, status::Union{Nothing,Matrix{Int32}}=nothing, ok::Union{Nothing,Vector{Int32}}=nothing,
                           J0::Union{Nothing,Vector{Float64}}=nothing, J_trial::Union{Nothing,Matrix{Float64}}=nothing, c1::Real=1e-4, act_off::Integer=0,
                           na::Integer=bm.nu - act_off) where T
    H = size(U, 3); n = 2 * bm.nu; P = div(bm.batch, trials)
    Jt = cost === nothing ? J_trial : Matrix{Float64}(undef, P, trials)
    J_cur = Vector{Float64}(undef, P); J_acc = Vector{Float64}(undef, P); choice = Vector{Int32}(undef, P); alpha_acc = Vector{T}(undef, P)
    X_new = Array{T}(undef, n, P, H + 1); U_new = Array{T}(undef, bm.nu, P, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve X U status alpha dV ok Xcur Ucur J0 Jt J_cur J_acc choice alpha_acc X_new U_new cost begin
        ls = Ref(DojoLineSearch(p(X), p(U), p(status), p(alpha), p(dV), p(ok), p(Xcur), p(Ucur), p(J0), p(Jt), p(J_cur), p(J_acc), p(choice), p(alpha_acc), p(X_new), p(U_new),
                                Float64(c1), Int32(act_off), Int32(na)))
        qc = Ref(cost === nothing ? DojoQuadraticCost(C_NULL, C_NULL, C_NULL, C_NULL, Int32(0)) :
                 DojoQuadraticCost(p(cost[1]), p(cost[2]), p(cost[3]), p(cost[4]), Int32(ndims(cost[4]) == 2)))
        GC.@preserve qc begin
            qcp = cost === nothing ? Ptr{DojoQuadraticCost}(C_NULL) : Base.unsafe_convert(Ptr{DojoQuadraticCost}, qc)
            check(@ccall $(fn(:dojo_linesearch_select))(bm.handle::Ptr{Cvoid}, Int32(H)::Int32, Int32(trials)::Int32, qcp::Ptr{DojoQuadraticCost}, ls::Ptr{DojoLineSearch})::Cint)
        end
    end
    return choice, alpha_acc, Jt, J_cur, J_acc, X_new, U_new
end

"""
reverse mode through a closed-loop rollout (no counterpart in Dojo.jl): the rollout of `rollout_policy` (without contact observations) and the
gradient of a trajectory loss w.r.t. the policy, the feed-forward term and the initial state; the recorded Jacobians stay on the device.
G[nx | nz, B, H] is the cotangent w.r.t. the state after every step (`cot_space = :tangent | :state`), G_u[nu, B, H] and G_obs[nobs, B, H + 1]
(optional) those w.r.t. the applied controls and the observations.  Array conventions as in `rollout_policy`.
-> Z, OBS, U, status, gW (the shape of W), gbias ([na] / [na, B]), gU[nu, B, H], gz0[nx, B] (tangent coordinates).
"""
function rollout_policy_gradients(bm::BatchedMechanism{T}, z0::Matrix{T}, W::Array{T}, G::Array{T,3}; bias::Union{Nothing,Array{T}}=nothing,
                                  mean::Union{Nothing,Vector{T}}=nothing, scale::Union{Nothing,Vector{T}}=nothing, U_ff::Union{Nothing,Array{T,3}}=nothing,
                                  act_off::Integer=0, G_u::Union{Nothing,Array{T,3}}=nothing, G_obs::Union{Nothing,Array{T,3}}=nothing,
                                  cot_space::Symbol=:tangent, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(G, 3); nobs = 2 * bm.nu
    size(W, 1) == nobs || error("W must have nobs = $nobs rows")
    na = size(W, 2); per_env = ndims(W) == 3
    Z = Array{T}(undef, bm.nz, bm.batch, H); OBS = Array{T}(undef, nobs, bm.batch, H + 1)
    U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    gW = similar(W); gbias = per_env ? Matrix{T}(undef, na, bm.batch) : Vector{T}(undef, na)
    gU = Array{T}(undef, bm.nu, bm.batch, H); gz = Matrix{T}(undef, bm.nx, bm.batch)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve W bias mean scale U_ff G_u G_obs begin
        pol = Ref(DojoPolicy(p(W), p(bias), p(mean), p(scale), p(U_ff), Int32(per_env), Int32(act_off), Int32(na), Int32(0), Int32(0), Int32(0)))
        check(@ccall $(fn(:dojo_rollout_policy_gradients))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, pol::Ptr{DojoPolicy}, Int32(H)::Int32, G::Ptr{T},
                                                           Int32(cot_space === :state ? 1 : 0)::Int32, p(G_u)::Ptr{Cvoid}, p(G_obs)::Ptr{Cvoid}, Z::Ptr{T}, OBS::Ptr{T},
                                                           U::Ptr{T}, status::Ptr{Int32}, gW::Ptr{T}, gbias::Ptr{T}, gU::Ptr{T}, gz::Ptr{T})::Cint)
    end
    return Z, OBS, U, status, gW, gbias, gU, gz
end

"mirror of `DojoMlpPolicy` (include/dojo_hip.h): four pointers, three Int32, the five widths, three Int32"
struct DojoMlpPolicy
    theta::Ptr{Cvoid}; mean::Ptr{Cvoid}; scale::Ptr{Cvoid}; U_ff::Ptr{Cvoid}
    per_env::Int32; act_off::Int32; n_layers::Int32; width::NTuple{5,Int32}
    contact_forces::Int32; contact_init::Int32; reserved::Int32
end
mlp_widths(widths) = (1 <= length(widths) - 1 <= 4 || error("widths must be [n_0, .., n_L] with 1 <= L <= 4");
                      ntuple(i -> Int32(i <= length(widths) ? widths[i] : 0), 5))
mlp_parameters(widths) = sum(widths[l + 1] * (widths[l] + 1) for l in 1:length(widths) - 1)

"""
closed-loop rollout with a tanh network policy: `rollout_policy` with h_l = tanh.(b_l + W_l h_{l-1}), h_0 = (o_k - mean) .* scale,
u_k = U_ff[k] + E (b_L + W_L h_{L-1}) evaluated on the device between the steps.  theta[P] (shared) or theta[P, B] (one policy per environment) is the
flat parameter vector of the ABI: layer after layer W_l ROW-major [n_l][n_{l-1}] (i.e. `vec(W_l')`), then b_l; widths = [n_0 = nobs, .., n_L = na].
-> Z[nz, B, H], OBS[nobs, B, H + 1], U[nu, B, H], status[B, H].
"""
function rollout_mlp(bm::BatchedMechanism{T}, z0::Matrix{T}, theta::Array{T}, widths::Vector{<:Integer}, H::Integer; mean::Union{Nothing,Vector{T}}=nothing,
                     scale::Union{Nothing,Vector{T}}=nothing, U_ff::Union{Nothing,Array{T,3}}=nothing, act_off::Integer=0, contact_forces::Bool=false,
                     contact_init::Integer=0, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    nobs = widths[1]
    size(theta, 1) == mlp_parameters(widths) || error("theta must have $(mlp_parameters(widths)) rows")
    Z = Array{T}(undef, bm.nz, bm.batch, H); OBS = Array{T}(undef, nobs, bm.batch, H + 1)
    U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve theta mean scale U_ff begin
        pol = Ref(DojoMlpPolicy(p(theta), p(mean), p(scale), p(U_ff), Int32(ndims(theta) == 2), Int32(act_off), Int32(length(widths) - 1), mlp_widths(widths),
                                Int32(contact_forces), Int32(contact_init), Int32(0)))
        check(@ccall $(fn(:dojo_rollout_mlp))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, pol::Ptr{DojoMlpPolicy}, Int32(H)::Int32, Z::Ptr{T}, OBS::Ptr{T}, U::Ptr{T}, status::Ptr{Int32})::Cint)
    end
    return Z, OBS, U, status
end

"""
reverse mode through `rollout_mlp` (without contact observations): the rollout and the gradient of a trajectory loss w.r.t. the network's parameters,
the feed-forward term and the initial state; the record, the observation Jacobians and the activations stay on the device.  Cotangents as in
`rollout_policy_gradients`.  -> Z, OBS, U, status, gtheta (the shape of theta; summed over the batch for a shared policy), gU[nu, B, H], gz0[nx, B].
"""
function rollout_mlp_gradients(bm::BatchedMechanism{T}, z0::Matrix{T}, theta::Array{T}, widths::Vector{<:Integer}, G::Array{T,3};
                               mean::Union{Nothing,Vector{T}}=nothing, scale::Union{Nothing,Vector{T}}=nothing, U_ff::Union{Nothing,Array{T,3}}=nothing,
                               act_off::Integer=0, G_u::Union{Nothing,Array{T,3}}=nothing, G_obs::Union{Nothing,Array{T,3}}=nothing,
                               cot_space::Symbol=:tangent, opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(G, 3); nobs = 2 * bm.nu
    widths[1] == nobs || error("widths[1] must be nobs = $nobs")
    size(theta, 1) == mlp_parameters(widths) || error("theta must have $(mlp_parameters(widths)) rows")
    Z = Array{T}(undef, bm.nz, bm.batch, H); OBS = Array{T}(undef, nobs, bm.batch, H + 1)
    U = Array{T}(undef, bm.nu, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    gtheta = similar(theta); gU = Array{T}(undef, bm.nu, bm.batch, H); gz = Matrix{T}(undef, bm.nx, bm.batch)
    p(a) = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve theta mean scale U_ff G_u G_obs begin
        pol = Ref(DojoMlpPolicy(p(theta), p(mean), p(scale), p(U_ff), Int32(ndims(theta) == 2), Int32(act_off), Int32(length(widths) - 1), mlp_widths(widths),
                                Int32(0), Int32(0), Int32(0)))
        check(@ccall $(fn(:dojo_rollout_mlp_gradients))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, pol::Ptr{DojoMlpPolicy}, Int32(H)::Int32, G::Ptr{T},
                                                        Int32(cot_space === :state ? 1 : 0)::Int32, p(G_u)::Ptr{Cvoid}, p(G_obs)::Ptr{Cvoid}, Z::Ptr{T}, OBS::Ptr{T},
                                                        U::Ptr{T}, status::Ptr{Int32}, gtheta::Ptr{T}, gU::Ptr{T}, gz::Ptr{T})::Cint)
    end
    return Z, OBS, U, status, gtheta, gU, gz
end

"which states the IFT data blocks are evaluated at: 0 = as the reference does after step! (post-update_state!), 1 = at the solved step (consistent)"
set_gradient_mode!(bm::BatchedMechanism, mode::Integer) = check(@ccall $(fn(:dojo_set_gradient_mode))(bm.handle::Ptr{Cvoid}, Int32(mode)::Int32)::Cint)

"external forces for every body of every environment: fext[6, Nb, B] = [state.Fext (world); state.τext (body frame)]; `nothing` removes them"
function set_external_force!(bm::BatchedMechanism{T}, fext::Union{Nothing,Array{T,3}}) where T
    check(@ccall $(fn(:dojo_set_external_force))(bm.handle::Ptr{Cvoid}, (fext === nothing ? C_NULL : pointer(fext))::Ptr{T})::Cint)
end

"simulate!(...; record=true): as above plus the Storage rows [25, Nb, B, H] (x q v ω px pq vl ωl, storage.jl:50-67)"
function simulate_storage!(bm::BatchedMechanism{T}, z0::Matrix{T}, U::Array{T,3}; opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    H = size(U, 3); Nb = length(bm.mechanism.bodies)
    Z = Array{T}(undef, bm.nz, bm.batch, H); S = Array{T}(undef, 25, Nb, bm.batch, H); status = Matrix{Int32}(undef, bm.batch, H)
    check(@ccall $(fn(:dojo_simulate))(bm.handle::Ptr{Cvoid}, z0::Ptr{T}, U::Ptr{T}, H::Int32, Z::Ptr{T}, S::Ptr{T}, status::Ptr{Int32})::Cint)
    return Z, S, status
end

"get_state(environment): minimal state (+ clamped contact normal impulses, as get_state(::AntARS)) of the last step, [2nu (+Nc), B]"
function get_state(bm::BatchedMechanism{T}; contact_forces::Bool=false) where T
    n = 2 * bm.nu + (contact_forces ? length(bm.mechanism.contacts) : 0)
    obs = Matrix{T}(undef, n, bm.batch)
    check(@ccall $(fn(:dojo_observe))(bm.handle::Ptr{Cvoid}, obs::Ptr{T}, Int32(contact_forces)::Int32)::Cint)
    return obs
end

"get_contact_gradients(mechanism) at the solution of the last get_maximal_gradients!: jacobian_contact[12Nb, 5Nc, B]"
function get_contact_gradients!(bm::BatchedMechanism{T}, ncontacts::Int) where T
    dc = Array{T}(undef, 5 * ncontacts, bm.nx, bm.batch)                      # ABI is row-major [B, nx, 5Nc]
    check(@ccall $(fn(:dojo_contact_gradients))(bm.handle::Ptr{Cvoid}, dc::Ptr{T})::Cint)
    return permutedims(dc, (2, 1, 3))
end

"minimal_to_maximal(mechanism, x): batched, x is 2nu x B (per joint [Δx; Δθ; Δv; Δω]) -> z (13Nb x B)"
function Dojo.minimal_to_maximal(bm::BatchedMechanism{T}, x::Matrix{T}) where T
    z = Matrix{T}(undef, bm.nz, bm.batch)
    check(@ccall $(fn(:dojo_minimal_to_maximal))(bm.handle::Ptr{Cvoid}, x::Ptr{T}, z::Ptr{T})::Cint)
    return z
end

"maximal_to_minimal(mechanism, z): batched"
function Dojo.maximal_to_minimal(bm::BatchedMechanism{T}, z::Matrix{T}) where T
    x = Matrix{T}(undef, 2 * bm.nu, bm.batch)
    check(@ccall $(fn(:dojo_maximal_to_minimal))(bm.handle::Ptr{Cvoid}, z::Ptr{T}, x::Ptr{T})::Cint)
    return x
end

"step_minimal_coordinates!(mechanism, x, u; opts): batched, returns (x_next, status)"
function Dojo.step_minimal_coordinates!(bm::BatchedMechanism{T}, x::Matrix{T}, u::Matrix{T}; opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    xn = similar(x); status = Vector{Int32}(undef, bm.batch); iters = Vector{Int32}(undef, bm.batch)
    check(@ccall $(fn(:dojo_step_minimal))(bm.handle::Ptr{Cvoid}, x::Ptr{T}, u::Ptr{T}, xn::Ptr{T}, status::Ptr{Int32}, iters::Ptr{Int32})::Cint)
    return xn, status
end

"get_minimal_gradients!(mechanism, x, u; opts): batched -> (jacobian_state[2nu, 2nu, B], jacobian_control[2nu, nu, B]); also returns x_next"
function Dojo.get_minimal_gradients!(bm::BatchedMechanism{T}, x::Matrix{T}, u::Matrix{T}; opts=Dojo.SolverOptions{Float64}()) where T
    set_options!(bm, opts)
    nm = 2 * bm.nu
    xn = similar(x); status = Vector{Int32}(undef, bm.batch); iters = Vector{Int32}(undef, bm.batch)
    jx = Array{T}(undef, nm, nm, bm.batch); ju = Array{T}(undef, bm.nu, nm, bm.batch)         # ABI is row-major [B, 2nu, 2nu] / [B, 2nu, nu]
    check(@ccall $(fn(:dojo_minimal_gradients))(bm.handle::Ptr{Cvoid}, x::Ptr{T}, u::Ptr{T}, xn::Ptr{T}, status::Ptr{Int32}, iters::Ptr{Int32}, jx::Ptr{T}, ju::Ptr{T})::Cint)
    return permutedims(jx, (2, 1, 3)), permutedims(ju, (2, 1, 3)), xn, status
end

# ---- device-resident batches, scheduling, multi-GPU ------------------------------------------------
# Everything below takes raw device pointers (Ptr{Cvoid}: `pointer(::ROCArray)` of AMDGPU.jl, or whatever allocator owns
# the handle's GPU) and a hipStream_t as Ptr{Cvoid} (C_NULL = the null stream); nothing is synchronized (dojo_hip.h,
# "device-pointer variants").  A training loop keeps z, u, dz, du on the device and calls step_dev! per step.
const DevPtr = Ptr{Cvoid}

"number of GPUs the library sees"
device_count() = Int(@ccall $(fn(:dojo_device_count))()::Cint)

"one differentiable step on device buffers: z [nz, B], u [nu, B] -> z_next, status [B], iters [B], dz [nx, nx, B], du [nx, nu, B] (dz = du = C_NULL: forward only)"
function step_dev!(bm::BatchedMechanism, z::DevPtr, u::DevPtr, z_next::DevPtr, status::DevPtr, iters::DevPtr,
                   dz::DevPtr=C_NULL, du::DevPtr=C_NULL; stream::DevPtr=C_NULL)
    check(@ccall $(fn(:dojo_step_dev))(bm.handle::Ptr{Cvoid}, z::Ptr{Cvoid}, u::Ptr{Cvoid}, z_next::Ptr{Cvoid}, status::Ptr{Cvoid}, iters::Ptr{Cvoid},
                                       dz::Ptr{Cvoid}, du::Ptr{Cvoid}, stream::Ptr{Cvoid})::Cint)
end

"environment groups of step_dev! (0: the library's choice, 1: one launch on the caller's stream); needs GPU_MAX_HW_QUEUES >= groups + 1"
set_groups!(bm::BatchedMechanism, n::Integer) = check(@ccall $(fn(:dojo_set_groups))(bm.handle::Ptr{Cvoid}, n::Int32)::Cint)
"iteration cap of the step kernel: solves unfinished after `cap` Newton iterations go on in the continuation kernel (line-search trials side by side) in joined steps; 0 / < 0: off (the default); include/dojo_hip.h has the measurements"
set_iteration_cap!(bm::BatchedMechanism, cap::Integer) = check(@ccall $(fn(:dojo_set_iteration_cap))(bm.handle::Ptr{Cvoid}, cap::Int32)::Cint)
set_dispatch_order!(bm::BatchedMechanism, mode::Integer) = check(@ccall $(fn(:dojo_set_dispatch_order))(bm.handle::Ptr{Cvoid}, mode::Int32)::Cint)
"asynchronous environment groups: consecutive step_dev! calls chain per group; join!(bm; stream) orders `stream` behind everything in flight"
set_async!(bm::BatchedMechanism, on::Bool) = check(@ccall $(fn(:dojo_set_async))(bm.handle::Ptr{Cvoid}, on::Int32)::Cint)
set_async!(bm::BatchedMechanism, mode::Integer) = check(@ccall $(fn(:dojo_set_async))(bm.handle::Ptr{Cvoid}, Int32(mode)::Int32)::Cint)      # 2: pipelined groups (dojo_hip.h)
join!(bm::BatchedMechanism; stream::DevPtr=C_NULL) = check(@ccall $(fn(:dojo_join))(bm.handle::Ptr{Cvoid}, stream::Ptr{Cvoid})::Cint)

"""
    set_refinement!(bm, stiffness)

Iterative refinement of the linear solves (Newton directions and IFT columns) of every environment whose cones reach
max γ/s > `stiffness` (Inf: never, 0: always).  Default: 1e4 when `opts.rtol <= 1e-7` or `opts.btol <= 1e-6`, never at the
reference's default tolerances (DESIGN.md §4.5).
"""
set_refinement!(bm::BatchedMechanism, stiffness::Real) = check(@ccall $(fn(:dojo_set_refinement))(bm.handle::Ptr{Cvoid}, Float64(stiffness)::Cdouble)::Cint)

# Multi-GPU: one Julia process per GPU (Distributed / MPI.jl), each with ONE BatchedMechanism for its contiguous slice of
# the batch.  Rank 0 creates the 128-byte id, the host carries it to the other ranks, every rank joins; allgather! then
# moves per-rank device buffers over RCCL / xGMI in rank (= batch) order -- once per rollout chunk, not per step.
#   id = myrank == 0 ? DojoHIP.comm_unique_id() : nothing
#   id = MPI.bcast(id, 0, comm)                        # or Distributed.remotecall_fetch
#   DojoHIP.comm_init!(bm, myrank, nranks, id)
#   DojoHIP.allgather!(bm, pointer(z_local), pointer(z_all), length(z_local))
"128 opaque bytes identifying a new RCCL communicator (call on rank 0 only)"
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    check(@ccall $(fn(:dojo_comm_unique_id))(id::Ptr{UInt8})::Cint)
    return id
end
comm_init!(bm::BatchedMechanism, rank::Integer, world::Integer, id::Vector{UInt8}) =
    check(@ccall $(fn(:dojo_comm_init))(bm.handle::Ptr{Cvoid}, rank::Int32, world::Int32, id::Ptr{UInt8})::Cint)
"recv[count, world] <- send[count] of every rank; elements of the handle's dtype, or Int32 with `as_int32` (status / iteration buffers)"
allgather!(bm::BatchedMechanism, send::DevPtr, recv::DevPtr, count::Integer; as_int32::Bool=false, stream::DevPtr=C_NULL) =
    check(@ccall $(fn(:dojo_allgather_dev))(bm.handle::Ptr{Cvoid}, send::Ptr{Cvoid}, recv::Ptr{Cvoid}, count::Int64, as_int32::Int32, stream::Ptr{Cvoid})::Cint)
"(rank, world) of the handle's communicator, (0, 1) before comm_init!"
function comm_info(bm::BatchedMechanism)
    r = Ref{Int32}(0); w = Ref{Int32}(1)
    check(@ccall $(fn(:dojo_comm_info))(bm.handle::Ptr{Cvoid}, r::Ref{Int32}, w::Ref{Int32})::Cint)
    return Int(r[]), Int(w[])
end

# ---- opt-in single-Mechanism drop-in ------------------------------------------------------------
# DojoHIP.enable!(mechanism) makes Dojo.mehrotra!(mechanism) (src/solver/mehrotra.jl:9) round-trip through the library
# (B = 1, fp64) and write the solution back -- body.state.vsol/ωsol, joint.impulses, contact.impulses(_dual), mechanism.μ,
# and mechanism.system re-assembled at the solution -- so that step!, simulate!, get_maximal_gradients! and the
# DojoEnvironments built on them (DojoEnvironments/src/environments.jl:77-84) keep working unchanged.
# Mechanisms that were not enabled keep the reference's own mehrotra!.
const HANDLES = IdDict{Dojo.Mechanism,BatchedMechanism{Float64}}()
const OVERRIDE_WORLD = Ref{UInt}(0)

"""
install the Dojo.mehrotra! method that dispatches enabled mechanisms to the library (done once, by the first enable!).
UNVERIFIED (no Julia where this was written): the method is `@eval`ed at run time, so call `enable!` at top level before the first
`step!` (a caller compiled earlier keeps dispatching to Dojo's own method until it returns to top level), and never while precompiling.
"""
function install_override!()
    ccall(:jl_generating_output, Cint, ()) == 1 && error("DojoHIP.enable! must not run during precompilation")
    OVERRIDE_WORLD[] != 0 && return
    OVERRIDE_WORLD[] = Base.get_world_counter()           # the world in which Dojo's own method is still the one that runs
    @eval function Dojo.mehrotra!(mechanism::Dojo.Mechanism{T}; opts=Dojo.SolverOptions{T}()) where T
        bm = get(HANDLES, mechanism, nothing)
        bm === nothing && return Base.invoke_in_world(OVERRIDE_WORLD[], Dojo.mehrotra!, mechanism; opts=opts)
        return hip_mehrotra!(mechanism, bm; opts=opts)
    end
    return
end

function enable!(m::Dojo.Mechanism)
    HANDLES[m] = BatchedMechanism(m, 1; T=Float64)
    install_override!()
    return m
end
disable!(m::Dojo.Mechanism) = (delete!(HANDLES, m); m)

"""
    hip_mehrotra!(mechanism, bm; opts)

What `mehrotra!` finds when `step!` calls it (src/simulation/step.jl:11-30): `set_maximal_state!` has set x2, q2, v15, ω15 and
`set_input!` / `input_impulse!` (src/mechanism/set.jl:40-53) have folded the controls into every body's `state.JF2`,
`state.Jτ2` and CLEARED the joints' inputs -- so the controls cross the boundary as body impulses (`dojo_step_impulses`),
next to `state.Fext`, `state.τext`.
"""
function hip_mehrotra!(m::Dojo.Mechanism, bm::BatchedMechanism{Float64}; opts=Dojo.SolverOptions{Float64}())
    set_options!(bm, opts)
    Nb = length(m.bodies)
    z = reshape(Dojo.get_maximal_state(m), :, 1)
    jf = Matrix{Float64}(undef, 6Nb, 1); fext = Array{Float64,3}(undef, 6, Nb, 1)
    for (i, b) in enumerate(m.bodies)
        jf[6i-5:6i-3, 1] = b.state.JF2; jf[6i-2:6i, 1] = b.state.Jτ2
        fext[1:3, i, 1] = b.state.Fext; fext[4:6, i, 1] = b.state.τext
    end
    set_external_force!(bm, fext)
    zn = similar(z); status = Vector{Int32}(undef, 1); iters = Vector{Int32}(undef, 1)
    check(@ccall $(fn(:dojo_step_impulses))(bm.handle::Ptr{Cvoid}, z::Ptr{Float64}, jf::Ptr{Float64}, zn::Ptr{Float64}, status::Ptr{Int32}, iters::Ptr{Int32})::Cint)
    # ---- write-back (what mehrotra! mutates, SURVEY.md §8b) ----
    per = any(c -> c.model isa Dojo.LinearContact, m.contacts) ? 12 : 8      # exported [s; γ] scalars per contact (dojo_hip.h, dojo_get_solution)
    vel = Vector{Float64}(undef, 6Nb); ji = Vector{Float64}(undef, max(1, sum(length.(m.joints)))); cs = Vector{Float64}(undef, max(1, per * length(m.contacts)))
    check(@ccall $(fn(:dojo_get_solution))(bm.handle::Ptr{Cvoid}, vel::Ptr{Float64}, ji::Ptr{Float64}, cs::Ptr{Float64})::Cint)
    for (i, b) in enumerate(m.bodies)
        b.state.vsol[2] = SVector{3}(vel[6i-5:6i-3]); b.state.ωsol[2] = SVector{3}(vel[6i-2:6i])
        b.state.vsol[1] = b.state.vsol[2]; b.state.ωsol[1] = b.state.ωsol[2]        # update! (src/solver/linear_system.jl:32-45)
    end
    off = 0
    for j in m.joints
        n = length(j); j.impulses[2] = SVector{n}(ji[off+1:off+n]); j.impulses[1] = j.impulses[2]; off += n
    end
    for (i, c) in enumerate(m.contacts)
        nh = length(c.impulses[2])            # N½: 4 for NonlinearContact, 1 for ImpactContact (the device exports [s(4); γ(4)] for both), 6 for LinearContact ([s(6); γ(6)])
        o = per * (i - 1); h = per ÷ 2
        c.impulses_dual[2] = SVector{nh}(cs[o+1:o+nh]); c.impulses[2] = SVector{nh}(cs[o+h+1:o+h+nh])
        c.impulses_dual[1] = c.impulses_dual[2]; c.impulses[1] = c.impulses[2]
    end
    mu = Vector{Float64}(undef, 1)
    check(@ccall $(fn(:dojo_get_mu))(bm.handle::Ptr{Cvoid}, mu::Ptr{Float64})::Cint)
    m.μ = mu[1]
    Dojo.set_entries!(m)                      # mechanism.system: the un-factored Jacobian and residual at the solution (mehrotra.jl:69)
    status[1] == 2 && error("Excessive angular velocity.")       # src/solver/line_search.jl:18-20
    return status[1] == 0 ? :success : :failed
end

end # module
