# MMCHip.jl -- the reference's hot-path methods served by libmmc_hip.so (MI355X / gfx950).
#
# HOW IT TAKES EFFECT.  The reference is a script: `Ewald/main.jl` `include`s energy.jl, ewalds.jl,
# auxillary.jl, structs.jl into `Main`, so `LJ_poly_ΔU`, `EwaldReal`, ... are generic functions OWNED
# BY `Main`.  A module that exports functions of the same names cannot replace them (`using` of a
# name Main already owns is a conflict and Main's CPU methods keep being called), and a method with
# a looser signature loses dispatch to the reference's typed one.  Therefore this file is
# `include`d INTO `Main`, AFTER the reference's own includes, and
#   * keeps its session state and ccall helpers inside `module MMCHipCore` (no name clashes), and
#   * defines, at top level, one method per reference method WITH THE REFERENCE'S EXACT TYPE
#     SIGNATURE (each is quoted with its file:line): Julia then overwrites the CPU method in place
#     -- same function object, same signature, new body -- and every existing caller (`Loop()`,
#     `potential`, the tests) runs the GPU path without being edited.
#
#     include("energy.jl"); include("ewalds.jl"); ...            # the reference, unchanged
#     include("/path/to/metropolismontecarlo_amd/julia/MMCHip.jl")
#     MMCHipCore.attach!(moa, soa, vdwTable, box)     # once, after MakeAtomArrays / MakeTables
#       (legacy API: MMCHipCore.attach!(system::Requirements, qq_q))
#
# Overwritten (current moa/soa API)                                     reference
#   LJ_poly_ΔU(i, moa::StructArray, soa::StructArray, vdwTable, r_cut, box)   Ewald/energy.jl:209-210
#   EwaldReal(chosenOne::Int64, moa::StructArray, soa::StructArray, ewald::EWALD,
#             r_cut::Float64, box::Float64)                                   Ewald/ewalds.jl:293-299
#   EwaldShort(i::Int64, moa::StructArray, soa::StructArray, sim_props::Properties2,
#              ewald::EWALD, box::Float64)                                    Ewald/ewalds.jl:892-899
#   PrepareEwaldVariables(ewald::EWALD, boxSize::Real where {T})              Ewald/ewalds.jl:45
#   RecipLong(ewald::EWALD, r::Vector{SVector{3,Float64}}, qq_q::Vector{Float64},
#             box::Float64)                                                   Ewald/ewalds.jl:538-543
#   RecipMove(box::Float64, ewalds::EWALD, r_old::Vector, r_new::Vector, qq_q::Vector)
#                                                                             Ewald/ewalds.jl:718-724
#   EwaldSelf(ewald::EWALD, qq_q::Vector)                                     Ewald/ewalds.jl:829
#   potential(moa::StructArray, soa::StructArray, tot::Properties, ewalds::EWALD, vdwTable::Tables,
#             sim_props::Properties2, coulomb_style::String)                  Ewald/energy.jl:946-954
#   potential(moa::StructArray, soa::StructArray, tot::Properties, ewald::EWALD, vdwTable::Tables,
#             sim_props::Properties2)                       (Wolf)            Ewald/energy.jl:864-871
# Overwritten (legacy `Requirements` API)
#   LJ_poly_ΔU(i::Int, system::Requirements)                                  Ewald/energy.jl:126
#   EwaldReal(qq_r::Vector{SVector{3,Float64}}, qq_q::Vector{Float64}, kappa::Real, box::Float64,
#             thisMol_thisAtom::Vector{SVector{2,Int64}}, chosenOne::Int64,
#             system::Requirements)                                           Ewald/ewalds.jl:205-213
#   EwaldShort(i::Int64, system::Requirements, ewald::EWALD, box::Float64,
#              qq_r::Vector{SVector{3,Float64}}, qq_q::Vector{Float64}, tinfoil = false)
#                                                                             Ewald/ewalds.jl:848-856
#   RecipLong(system::Requirements, ewald::EWALD, r::Vector{SVector{3,Float64}},
#             qq_q::Vector{Float64})                                          Ewald/ewalds.jl:465-470
#   CoulombReal(qq_r::Vector{SVector{3,Float64}}, qq_q::Vector{Float64}, box::Float64,
#               chosenOne::Int64, system::Requirements)                       Ewald/energy.jl:618-624
# Return values are the reference's: (pot, vir), (pot, overlap::Bool), (e, v, overlap),
# (energy, ewald), ΔE, energy, tot.  Host arrays are borrowed for the duration of each ccall
# (GC.@preserve); nothing is cached by pointer (Loop() rebinds ewald.sumQExpOld/New on every move,
# main.jl:621,628).
#
# ONE ccall PER REFERENCE CALL.  The per-molecule methods hand the library the caller's own arrays
# (mmc_call_lj_poly_du / mmc_call_ewald_short / mmc_call_ewald_real / mmc_call_recip_move,
# include/mmc_hip.h): the library compares molecule i and the molecule of the previous call with its
# mirror, evaluates LJ and real-space Coulomb together on the context's persistent kernel, answers
# the second of LJ_poly_ΔU(i) / EwaldShort(i) from that evaluation, computes RecipMove with the
# evaluation of the moved molecule, and finds out by content which of its buffers
# ewald.sumQExpOld / sumQExpNew are.  Measured through the Python mirror of this file (api.py, the
# same library calls): 33 us for the five calls of one Loop() iteration at 750 molecules, against
# 100 us for a C port of the reference on one core (bench.py, `call_surface`).
#
# BEYOND THE REFERENCE'S SURFACE (module MMCHipCore, nothing of Main is touched):
#   MMCHipCore.trial_move / accept_move! / reject_move!   the five calls of one Loop() iteration as
#       ONE evaluation (mmc_trial_move, mmc_accept_move, mmc_reject_move)
#   MMCHipCore.Batch                                      R independent replicas of the system on
#       one GPU (mmc_batch_*): north_star's "many independent NVT replicas fill the device" with
#       accept/reject on the Julia host (eval! / settle!) or in the library's native driver
#       (run! / run_chains!); see INTEGRATION.md.
# tests/test_julia_binding.py parses include/mmc_hip.h and every ccall below and compares symbol,
# arity and the C-to-Julia type of every argument, and the field layouts of the structs.
#
# NOT RUN.  The build image has no `julia` (and no network to fetch one), so this file has never
# been executed; it is written against the reference's source and the C header it binds
# (include/mmc_hip.h), and tests/test_julia_binding.py checks by text that every method above is
# present here with the reference's signature line.  The same C ABI is exercised on the GPU by the
# Python mirror (metropolismontecarlo_amd/api.py).

for needed in (:EWALD, :Requirements, :Properties, :Properties2, :Tables, :StructArray, :SVector)
    isdefined(@__MODULE__, needed) ||
        error("MMCHip.jl must be included AFTER the reference's structs.jl, auxillary.jl, " *
              "energy.jl and ewalds.jl (and their `using StaticArrays, StructArrays`): " *
              "$needed is not defined in $(@__MODULE__)")
end

module MMCHipCore

using StaticArrays

const libmmc = get(ENV, "MMC_HIP_LIB", joinpath(@__DIR__, "..", "libmmc_hip.so"))

# mirrors of the structs of include/mmc_hip.h (field order, types and padding are checked by
# tests/test_julia_binding.py against the header)
struct MMCTotals
    energy::Float64; virial::Float64; coulomb::Float64
    lj::Float64; real::Float64; recip::Float64; self::Float64
    n_overlap::Int32; _pad::Int32
end

struct MMCMove
    mol::Int32; accept_prev::Int32
    com_new::NTuple{3,Float64}
    atoms_new::NTuple{9,Float64}
end

struct MMCMoveResult
    d_lj::Float64; d_real::Float64; d_recip::Float64; d_vir::Float64
    overlap::Int32; _pad::Int32
end

struct MMCRunParams
    temperature::Float64; dr_max::Float64; dphi_max::Float64
    seed::UInt64; n_steps::Int64
    n_groups::Int32; n_parts::Int32; time_kernels::Int32; n_threads::Int32; n_streams::Int32; _pad::Int32
    replica0::UInt64
end

struct MMCRunStats
    moves::Int64; launches::Int64
    trans_attempt::Int64; trans_accept::Int64; rot_attempt::Int64; rot_accept::Int64; overlaps::Int64
    wall_ms::Float64; kernel_ms::Float64; energy_sum::Float64
    timed_launches::Int64; torn_records::Int64; server_steps::Int64; device_decisions::Int64
end

struct MMCNptParams
    pressure::Float64; vmax::Float64; alpha::Float64
    n_sweeps::Int64; moves_per_sweep::Int64
end

struct MMCNptStats
    vol_attempt::Int64; vol_accept::Int64
    box::Float64; volume_sum::Float64; volume_ms::Float64
end

struct MMCChain
    dr_max::Float64; dphi_max::Float64
    energy::Float64; virial::Float64
    avg_energy::Float64; avg_virial::Float64
    steps_taken::Int64; overlaps::Int64
    trans_naccepp::Int64; trans_attempp::Int64; trans_naccept::Int64; trans_attempt::Int64
    rot_naccepp::Int64; rot_attempp::Int64; rot_naccept::Int64; rot_attempt::Int64
    trans_set_value::Float64; rot_set_value::Float64
end

# mmc_state_info ("Save and resume"): 8-byte fields only; passed as a Ref where the C prototypes say void *
struct MMCStateInfo
    magic::UInt64; version::Int64
    R::Int64; n_mol::Int64; nkvecs::Int64; half_k::Int64
    lj_rcut::Float64; qq_rcut::Float64
    topology::UInt64
    nk::Int64; k_sq_max::Int64
    factor::Float64
    coulomb_style::Int64; s_stale::Int64; per_box::Int64
    alpha::Float64
    temps_on::Int64; quat_mode::Int64
    db::NTuple{9, Float64}
    box::Float64; kappa::Float64
    steps_done::Int64
    r_mol_max::Float64
    rigid_only::Int64
    solute_on::Int64
    solute_hash::UInt64
    reserved::NTuple{8, Int64}
end

"Address of the first Float64 of a Vector of bits types (SVector{3,Float64}, ComplexF64, Float64)."
fptr(x) = Ptr{Float64}(pointer(x))

mutable struct Session
    ctx::Ptr{Cvoid}
    box::Float64
    ewald_key::Tuple
end

const SESSION = Ref{Union{Nothing,Session}}(nothing)

function check(status::Int32)
    status == 0 && return
    msg = unsafe_string(ccall((:mmc_last_error, libmmc), Cstring, ()))
    status == 2 && throw(AssertionError(msg))      # a reference @assert
    error("libmmc_hip: status $status: $msg")
end

function upload!(com, fa, la, coords, atype, charge, eps, sig, box::Float64, device::Integer)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mmc_ctx_create, libmmc), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                device, C_NULL, ctx))
    GC.@preserve com fa la coords atype charge eps sig begin
        check(ccall((:mmc_upload_system, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                     Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Float64),
                    ctx[], length(com), length(coords), fptr(com), pointer(fa), pointer(la),
                    fptr(coords), pointer(atype), pointer(charge), size(eps, 1), pointer(eps),
                    pointer(sig), box))
    end
    SESSION[] = Session(ctx[], box, ())
    return SESSION[]
end

"Upload moa/soa/vdwTable once (mmc_upload_system): the current API of Loop()."
attach!(moa, soa, vdwTable, box::Float64; device::Integer = 0) =
    upload!(moa.COM, moa.firstAtom, moa.lastAtom, soa.coords, soa.atype, soa.charge,
            vdwTable.ϵᵢⱼ, vdwTable.σᵢⱼ, box, device)

"Upload a legacy `Requirements` system (auxillary.jl:59-75) and its charges."
function attach!(system, qq_q::Vector{Float64}; device::Integer = 0)
    fa = Int64[t[1] for t in system.thisMol_theseAtoms]
    la = Int64[t[2] for t in system.thisMol_theseAtoms]
    atype = Vector{Int64}(system.atomTypes)
    return upload!(system.rm, fa, la, system.ra, atype, qq_q, system.table.ϵᵢⱼ, system.table.σᵢⱼ,
                   system.box, device)
end

function detach!()
    s = SESSION[]
    s === nothing && return
    ccall((:mmc_ctx_destroy, libmmc), Int32, (Ptr{Cvoid},), s.ctx)
    SESSION[] = nothing
end

session() = (s = SESSION[]; s === nothing ? error("MMCHipCore.attach!(...) first") : s)

"Re-send every centre of mass and atom (after host edits that are not Loop()'s one-molecule pattern)."
function sync_all!(s::Session, com, coords)
    GC.@preserve com coords begin
        check(ccall((:mmc_update_system, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                    s.ctx, com === nothing ? Ptr{Float64}(C_NULL) : fptr(com), fptr(coords)))
    end
end

function bind_ewald!(s::Session, kappa, nk, k_sq_max, factor, box)
    key = (kappa, nk, k_sq_max, factor, box)
    if s.ewald_key != key
        n = Ref{Int64}(0)
        check(ccall((:mmc_prepare_ewald, libmmc), Int32,
                    (Ptr{Cvoid}, Float64, Int64, Int64, Float64, Float64, Ptr{Int64}),
                    s.ctx, kappa, nk, k_sq_max, box, factor, n))
        s.ewald_key = key
    end
end
bind_ewald!(s::Session, ewald, box) =
    bind_ewald!(s, ewald.kappa, ewald.nk, ewald.k_sq_max, ewald.factor, box)

"ewald.sumQExpOld / sumQExpNew <- the device's (RecipLong and potential write both, ewalds.jl:600-601)."
function pull_s!(s::Session, ewald; old::Bool = false)
    so, sn = ewald.sumQExpOld, ewald.sumQExpNew
    GC.@preserve so sn begin
        check(ccall((:mmc_get_sumqexp, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                    s.ctx, old ? fptr(so) : Ptr{Float64}(C_NULL), fptr(sn)))
    end
end

# ---- the per-molecule calls with the caller's own arrays: one ccall each ----
function call_lj_poly_du(s::Session, i::Int64, com, coords, r_cut::Float64)
    pot = Ref{Float64}(0.0); vir = Ref{Float64}(0.0)
    GC.@preserve com coords begin
        check(ccall((:mmc_call_lj_poly_du, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
                    s.ctx, i, fptr(com), fptr(coords), r_cut, pot, vir))
    end
    return pot[], vir[]
end

function call_ewald_real(s::Session, i::Int64, com, coords, r_cut::Float64, ovr::Float64)
    pot = Ref{Float64}(0.0); ov = Ref{Int32}(0)
    GC.@preserve com coords begin
        check(ccall((:mmc_call_ewald_real, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Int32}),
                    s.ctx, i, fptr(com), fptr(coords), r_cut, ovr, pot, ov))
    end
    return pot[], ov[] != 0
end

function call_ewald_short(s::Session, i::Int64, com, coords, qq_rcut::Float64)
    e = Ref{Float64}(0.0); v = Ref{Float64}(0.0); ov = Ref{Int32}(0)
    GC.@preserve com coords begin
        check(ccall((:mmc_call_ewald_short, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    s.ctx, i, fptr(com), fptr(coords), qq_rcut, e, v, ov))
    end
    return e[], v[], ov[] != 0
end

function recip_long(s::Session, ewald)
    energy = Ref{Float64}(0.0)
    check(ccall((:mmc_recip_long, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), s.ctx, energy))
    pull_s!(s, ewald; old = true)              # both arrays are written (ewalds.jl:600-601)
    return energy[]
end

function totals(s::Session, sym::Symbol, lj_rcut::Float64, qq_rcut::Float64)
    t = Ref{MMCTotals}()
    if sym === :ewald
        check(ccall((:mmc_potential_ewald, libmmc), Int32,
                    (Ptr{Cvoid}, Float64, Float64, Ptr{MMCTotals}), s.ctx, lj_rcut, qq_rcut, t))
    else
        check(ccall((:mmc_potential_wolf, libmmc), Int32,
                    (Ptr{Cvoid}, Float64, Float64, Ptr{MMCTotals}), s.ctx, lj_rcut, qq_rcut, t))
    end
    return t[]
end

# ---- one Loop() iteration as ONE evaluation (main.jl:491-593) ----
"""
    d, overlap = trial_move(i, com_new, atoms_new, lj_rcut, qq_rcut)

The five hot-path calls of one Loop() iteration for molecule `i` moved to `com_new` /
`atoms_new` (3 atoms): d = (ΔLJ, Δreal, ΔRecip, Δvirial) as `partial_new - partial_old` builds
them (main.jl:593,600-601).  The device keeps the OLD state: follow with `accept_move!()`
(main.jl:598-621) or `reject_move!()` (:622-629).  The host arrays are the caller's business.
"""
function trial_move(i::Int64, com_new::SVector{3,Float64}, atoms_new::Vector{SVector{3,Float64}},
                    lj_rcut::Float64, qq_rcut::Float64)
    s = session()
    d = zeros(Float64, 4); ov = Ref{Int32}(0); cn = [com_new]
    GC.@preserve cn atoms_new d begin
        check(ccall((:mmc_trial_move, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Int32}),
                    s.ctx, i, fptr(cn), fptr(atoms_new), lj_rcut, qq_rcut, pointer(d), ov))
    end
    return (d[1], d[2], d[3], d[4]), ov[] != 0
end
accept_move!() = check(ccall((:mmc_accept_move, libmmc), Int32, (Ptr{Cvoid},), session().ctx))
reject_move!() = check(ccall((:mmc_reject_move, libmmc), Int32, (Ptr{Cvoid},), session().ctx))

"Counters of the context (mmc_ctx_stats): commands served, launches, retries, cache hits, ..."
function stats()
    out = zeros(Int64, 10)
    check(ccall((:mmc_ctx_stats, libmmc), Int32, (Ptr{Cvoid}, Ptr{Int64}), session().ctx, out))
    return out
end

# =================================================================================================
# The replica batch: R independent NVT chains of the attached kind of system on one GPU
# (include/mmc_hip.h, "replica batch").  Molecules must have 3 atoms (RecipMove, ewalds.jl:740).
# =================================================================================================
mutable struct Batch
    h::Ptr{Cvoid}
    n_replicas::Int64
    n_mol::Int64
end

"""
    b = Batch(n_replicas, moa, soa, vdwTable, ewald, box, lj_rcut, qq_rcut; device = 0)

Every replica starts from (moa, soa); `ewald` supplies kappa, nk, k_sq_max and factor
(main.jl:285-303).  Call `potential_ewald(b)` (or `recip_long!(b)`) once before the first move: it
fills the structure factors.
"""
function Batch(n_replicas::Integer, moa, soa, vdwTable, ewald, box::Float64, lj_rcut::Float64,
               qq_rcut::Float64; device::Integer = 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    com, coords, atype, charge = moa.COM, soa.coords, soa.atype, soa.charge
    eps, sig = vdwTable.ϵᵢⱼ, vdwTable.σᵢⱼ
    GC.@preserve com coords atype charge eps sig begin
        check(ccall((:mmc_batch_create, libmmc), Int32,
                    (Int32, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64},
                     Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Int64, Int64,
                     Float64, Float64, Float64, Ptr{Ptr{Cvoid}}),
                    device, C_NULL, n_replicas, length(com), fptr(com), fptr(coords), pointer(atype),
                    pointer(charge), size(eps, 1), pointer(eps), pointer(sig), box, ewald.kappa,
                    ewald.nk, ewald.k_sq_max, ewald.factor, lj_rcut, qq_rcut, h))
    end
    b = Batch(h[], n_replicas, length(com))
    finalizer(close!, b)
    return b
end

function close!(b::Batch)
    b.h == C_NULL && return
    ccall((:mmc_batch_destroy, libmmc), Int32, (Ptr{Cvoid},), b.h)
    b.h = C_NULL
    return
end

"Tuning switches of include/mmc_hip.h (\"kernel\", \"parts\", \"device_moves\", \"persistent\", ...)."
set_option!(b::Batch, key::String, value::Integer) =
    check(ccall((:mmc_batch_set_option, libmmc), Int32, (Ptr{Cvoid}, Cstring, Int64), b.h, key, value))

"potential(..., \"ewald\") of every replica (energy.jl:946-1032)."
function potential_ewald(b::Batch)
    tot = Vector{MMCTotals}(undef, b.n_replicas)
    check(ccall((:mmc_batch_potential_ewald, libmmc), Int32, (Ptr{Cvoid}, Ptr{MMCTotals}), b.h, tot))
    return tot
end

"""
    set_coulomb_style!(b, :ewald | :wolf)

The reference's global `Wolf` (main.jl:75) for the batch's moves: `:wolf` skips RecipMove
(main.jl:580-590) and leaves S(k) alone.  After switching back to `:ewald` call `recip_long!(b)` (or
`potential_ewald(b)`) before the next move.
"""
function set_coulomb_style!(b::Batch, style::Symbol)
    style in (:ewald, :wolf) || throw(ArgumentError("coulomb style must be :ewald or :wolf"))
    check(ccall((:mmc_batch_set_coulomb_style, libmmc), Int32, (Ptr{Cvoid}, Int32), b.h, style == :wolf ? 1 : 0))
end

function coulomb_style(b::Batch)
    v = Ref{Int32}(0)
    check(ccall((:mmc_batch_get_coulomb_style, libmmc), Int32, (Ptr{Cvoid}, Ptr{Int32}), b.h, v))
    return v[] == 1 ? :wolf : :ewald
end

"potential() of the Wolf overload of every replica (energy.jl:864-943), in either style."
function potential_wolf(b::Batch)
    tot = Vector{MMCTotals}(undef, b.n_replicas)
    check(ccall((:mmc_batch_potential_wolf, libmmc), Int32, (Ptr{Cvoid}, Ptr{MMCTotals}), b.h, tot))
    return tot
end

"RecipLong of every replica; energies WITHOUT factor (ewalds.jl:603)."
function recip_long!(b::Batch)
    e = Vector{Float64}(undef, b.n_replicas)
    check(ccall((:mmc_batch_recip_long, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h, e))
    return e
end

"""
    eval!(b, moves, results)

One trial move per replica in one launch: `moves[r]` (molecule, new COM and atoms;
`accept_prev` settles the replica's previous proposal first, main.jl:598-629) -> `results[r]`
(ΔLJ, Δreal, ΔRecip, Δvirial, overlap).  Accept/reject stays with the caller: this is Loop()'s
body for R chains at once.
"""
function eval!(b::Batch, moves::Vector{MMCMove}, results::Vector{MMCMoveResult})
    length(moves) == b.n_replicas == length(results) || error("one move and one result per replica")
    check(ccall((:mmc_batch_eval, libmmc), Int32, (Ptr{Cvoid}, Ptr{MMCMove}, Ptr{MMCMoveResult}),
                b.h, moves, results))
    return results
end

"Settle the last proposals (accept[r] != 0: commit, main.jl:598-621) without evaluating new ones."
function settle!(b::Batch, accept::Vector{Int32})
    length(accept) == b.n_replicas || error("one flag per replica")
    check(ccall((:mmc_batch_settle, libmmc), Int32, (Ptr{Cvoid}, Ptr{Int32}), b.h, accept))
end

"""
    stats = run!(b, params, energies)

The library's native driver: Loop()'s sequential accept/reject (main.jl:487-644) for every
replica, `params.n_steps` trial moves each; `energies[r]` is the running total.energy (:599).
"""
function run!(b::Batch, params::MMCRunParams, energies::Vector{Float64})
    length(energies) == b.n_replicas || error("one energy per replica")
    p = Ref(params); st = Ref{MMCRunStats}()
    check(ccall((:mmc_batch_run, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{MMCRunParams}, Ptr{Float64}, Ptr{MMCRunStats}), b.h, p, energies, st))
    return st[]
end

"As `run!`, every chain with its own step sizes, block accumulators and Adjust! (adjust.jl:1-83)."
function run_chains!(b::Batch, params::MMCRunParams, chains::Vector{MMCChain}, adjust::Bool)
    length(chains) == b.n_replicas || error("one chain record per replica")
    p = Ref(params); st = Ref{MMCRunStats}()
    check(ccall((:mmc_batch_run_chains, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{MMCRunParams}, Ptr{MMCChain}, Int32, Ptr{MMCRunStats}),
                b.h, p, chains, adjust ? 1 : 0, st))
    return st[]
end

"Coordinates (and sumQExpOld) of replica r (0-based, like the library)."
function get_replica(b::Batch, r::Integer)
    com = Vector{SVector{3,Float64}}(undef, b.n_mol)
    coords = Vector{SVector{3,Float64}}(undef, 3 * b.n_mol)
    s_old = Vector{ComplexF64}(undef, 337)
    GC.@preserve com coords s_old begin
        check(ccall((:mmc_batch_get_replica, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    b.h, r, fptr(com), fptr(coords), fptr(s_old)))
    end
    return com, coords, s_old
end

function set_replica!(b::Batch, r::Integer, com::Vector{SVector{3,Float64}},
                      coords::Vector{SVector{3,Float64}})
    GC.@preserve com coords begin
        check(ccall((:mmc_batch_set_replica, libmmc), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), b.h, r, fptr(com), fptr(coords)))
    end
end

"The device part of an NPT volume move for every replica (volumeChange.jl:59-80)."
volume_change!(b::Batch, new_box::Float64, new_kappa::Float64) =
    check(ccall((:mmc_batch_volume_change, libmmc), Int32, (Ptr{Cvoid}, Float64, Float64),
                b.h, new_box, new_kappa))

"""
    tot = volume_trial!(b, new_box, new_kappa); ...; volume_accept!(b) | volume_reject!(b)

An NPT volume move of a ONE-replica batch without a host round trip (Ewald/volumeChange.jl:59-147):
device-side snapshot, rescale, new tables, total energy at the new volume; a rejection restores
everything bit for bit.
"""
function volume_trial!(b::Batch, new_box::Float64, new_kappa::Float64)
    t = Ref{MMCTotals}()
    check(ccall((:mmc_batch_volume_trial, libmmc), Int32, (Ptr{Cvoid}, Float64, Float64, Ptr{MMCTotals}),
                b.h, new_box, new_kappa, t))
    return t[]
end
volume_accept!(b::Batch) = check(ccall((:mmc_batch_volume_accept, libmmc), Int32, (Ptr{Cvoid},), b.h))
volume_reject!(b::Batch) = check(ccall((:mmc_batch_volume_reject, libmmc), Int32, (Ptr{Cvoid},), b.h))

"""
    (run_stats, npt_stats) = run_npt!(b, params, npt, energy)

An NPT chain of a one-replica batch: `npt.n_sweeps` times { `npt.moves_per_sweep` trial moves
(Loop(), main.jl:487-644), one volume move (volumeChange.jl:59-147) }; `energy[1]` is the running
total.energy of the replica.
"""
function run_npt!(b::Batch, params::MMCRunParams, npt::MMCNptParams, energy::Vector{Float64})
    length(energy) == 1 || error("an NPT chain is a batch of one replica")
    p = Ref(params); q = Ref(npt); st = Ref{MMCRunStats}(); ns = Ref{MMCNptStats}()
    check(ccall((:mmc_batch_run_npt, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{MMCRunParams}, Ptr{MMCNptParams}, Ptr{Float64}, Ptr{MMCRunStats},
                 Ptr{MMCNptStats}), b.h, p, q, energy, st, ns))
    return st[], ns[]
end

"""
    set_boxes!(b, boxes; alpha = 5.6);  boxes = get_boxes(b)

Per-replica boxes (independent NPT replicas in one batch): replica r lives in `boxes[r]` with
kappa = alpha / boxes[r] (main.jl:290-291).  The coordinates are not rescaled; call
`recip_long(b)` afterwards.
"""
function set_boxes!(b::Batch, boxes::Vector{Float64}; alpha::Float64 = 5.6)
    length(boxes) == b.n_replicas || error("one box per replica")
    check(ccall((:mmc_batch_set_boxes, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}, Float64),
                b.h, boxes, alpha))
end
function get_boxes(b::Batch)
    boxes = Vector{Float64}(undef, b.n_replicas)
    check(ccall((:mmc_batch_get_boxes, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h, boxes))
    return boxes
end

"""
    tot = volume_trial_replicas!(b, new_boxes); ...; volume_settle!(b, accept)

One batched volume trial of a batch with per-replica boxes (`new_boxes[r] == 0`: replica r stays),
then the decisions: a rejected or unmoved replica gets its state back bit for bit.
"""
function volume_trial_replicas!(b::Batch, new_boxes::Vector{Float64})
    length(new_boxes) == b.n_replicas || error("one box per replica")
    tot = Vector{MMCTotals}(undef, b.n_replicas)
    check(ccall((:mmc_batch_volume_trial_replicas, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{MMCTotals}), b.h, new_boxes, tot))
    return tot
end
function volume_settle!(b::Batch, accept::Vector{Int32})
    length(accept) == b.n_replicas || error("one decision per replica")
    check(ccall((:mmc_batch_volume_settle, libmmc), Int32, (Ptr{Cvoid}, Ptr{Int32}), b.h, accept))
end

"""
    (run_stats, npt_stats) = run_npt_replicas!(b, params, npt, energies; pressures = nothing)

`run_npt!`'s chain for every replica of a batch with per-replica boxes; `pressures` (one per
replica) overrides `npt.pressure`.  `npt_stats` has one `MMCNptStats` per replica.
"""
function run_npt_replicas!(b::Batch, params::MMCRunParams, npt::MMCNptParams, energies::Vector{Float64};
                           pressures::Union{Nothing,Vector{Float64}} = nothing)
    length(energies) == b.n_replicas || error("one energy per replica")
    p = Ref(params); q = Ref(npt); st = Ref{MMCRunStats}()
    ns = Vector{MMCNptStats}(undef, b.n_replicas)
    pr = pressures === nothing ? Ptr{Float64}(C_NULL) : pointer(pressures)
    GC.@preserve pressures begin
        check(ccall((:mmc_batch_run_npt_replicas, libmmc), Int32,
                    (Ptr{Cvoid}, Ptr{MMCRunParams}, Ptr{MMCNptParams}, Ptr{Float64}, Ptr{Float64},
                     Ptr{MMCRunStats}, Ptr{MMCNptStats}), b.h, p, q, pr, energies, st, ns))
    end
    return st[], ns
end

# ---- Parallel tempering (include/mmc_hip.h, "Parallel tempering") -----------------------------------
"""
    set_temperatures!(b, temps);  set_temperatures!(b, nothing);  temps = temperatures(b)

Replica r's trial moves (`run!`, `run_chains!`, `run_npt_replicas!` and its volume criterion) are
decided at `temps[r]`; `params.temperature` is then ignored.  `nothing` switches the array off.
"""
function set_temperatures!(b::Batch, temps::Union{Nothing,Vector{Float64}})
    temps === nothing || length(temps) == b.n_replicas || error("one temperature per replica")
    tp = temps === nothing ? Ptr{Float64}(C_NULL) : pointer(temps)
    GC.@preserve temps begin
        check(ccall((:mmc_batch_set_temperatures, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h, tp))
    end
end
function temperatures(b::Batch)
    temps = Vector{Float64}(undef, b.n_replicas)
    check(ccall((:mmc_batch_get_temperatures, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h, temps))
    return temps
end

"""
    exchange_round!(n_rungs, parity, seed, replica0, round, pressure, energies, volumes, temps, rung, attempt, accept)

One round of ladder exchanges as a pure host function (no device, no batch): ladder l is replicas
l * n_rungs + 1 : (l + 1) * n_rungs of the arrays, `rung[r]` (0-based values) the rung replica r
holds; `temps` and `rung` swap in place, `attempt` / `accept` (n_rungs - 1) accumulate.  `volumes`
may be `nothing` (NVT).
"""
function exchange_round!(n_rungs::Integer, parity::Integer, seed::UInt64, replica0::Integer, round::Integer,
                         pressure::Float64, energies::Vector{Float64}, volumes::Union{Nothing,Vector{Float64}},
                         temps::Vector{Float64}, rung::Vector{Int32}, attempt::Vector{Int64}, accept::Vector{Int64})
    length(energies) == length(temps) == length(rung) || error("one energy, temperature and rung per replica")
    n_rungs >= 1 && length(rung) % n_rungs == 0 || error("the replicas are not whole ladders")
    length(attempt) == length(accept) == n_rungs - 1 || error("one counter per neighbouring pair of rungs")
    vp = volumes === nothing ? Ptr{Float64}(C_NULL) : pointer(volumes)
    GC.@preserve volumes begin
        check(ccall((:mmc_exchange_round, libmmc), Int32,
                    (Int64, Int32, Int32, UInt64, UInt64, UInt64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Int32}, Ptr{Int64}, Ptr{Int64}),
                    length(rung) ÷ n_rungs, n_rungs, parity, seed, replica0, round, pressure, energies, vp, temps, rung,
                    attempt, accept))
    end
end

"""
    exchange!(b, n_rungs, parity, seed, replica0, round, pressure, energies, rung, attempt, accept)

`exchange_round!` on the batch's own temperatures (volumes = box^3 with per-replica boxes, NVT
otherwise); a swap exchanges temperatures, no replica state moves.
"""
function exchange!(b::Batch, n_rungs::Integer, parity::Integer, seed::UInt64, replica0::Integer, round::Integer,
                   pressure::Float64, energies::Vector{Float64}, rung::Vector{Int32}, attempt::Vector{Int64},
                   accept::Vector{Int64})
    length(energies) == length(rung) == b.n_replicas || error("one energy and rung per replica")
    length(attempt) == length(accept) == n_rungs - 1 || error("one counter per neighbouring pair of rungs")
    check(ccall((:mmc_batch_exchange, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Int32, UInt64, UInt64, UInt64, Float64, Ptr{Float64}, Ptr{Int32}, Ptr{Int64},
                 Ptr{Int64}), b.h, n_rungs, parity, seed, replica0, round, pressure, energies, rung, attempt, accept))
end

"""
    stats = run_exchange!(b, params, n_rounds, n_rungs, round0, energies, rung, attempt, accept)

`n_rounds` times { `params.n_steps` trial moves of every replica at its own temperature, one
exchange with round = round0 + i and parity = round & 1 } on a one-box batch.
"""
function run_exchange!(b::Batch, params::MMCRunParams, n_rounds::Integer, n_rungs::Integer, round0::Integer,
                       energies::Vector{Float64}, rung::Vector{Int32}, attempt::Vector{Int64},
                       accept::Vector{Int64})
    length(energies) == length(rung) == b.n_replicas || error("one energy and rung per replica")
    length(attempt) == length(accept) == n_rungs - 1 || error("one counter per neighbouring pair of rungs")
    p = Ref(params); st = Ref{MMCRunStats}()
    check(ccall((:mmc_batch_run_exchange, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{MMCRunParams}, Int64, Int32, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int64},
                 Ptr{Int64}, Ptr{MMCRunStats}), b.h, p, n_rounds, n_rungs, round0, energies, rung, attempt, accept, st))
    return st[]
end

# ---- Widom test-particle insertion (include/mmc_hip.h, mmc_batch_widom / mmc_batch_widom_at) ------
"""
    widom!(b, n_insert, seed, draw0, offsets, temperature, boltz_sum, n_overlap)
    widom_at!(b, mol_in, n_insert, temperature, boltz_sum, n_overlap)

`n_insert` insertions of a rigid copy of molecule 1 (atoms at COM + R offsets[a], `offsets` 9
Float64, A) into every replica; `boltz_sum[r] += sum exp(-dU / T)` in insertion order and
`n_overlap[r] +=` the insertions of weight 0.  dU is the change of potential(..., "ewald")
(energy.jl:946-1032) when the molecule is appended as molecule N + 1; the reference has no
insertion code.  `widom_at!` evaluates the caller's molecules, `mol_in` = R * n_insert * 12 Float64
(atoms, then COM).  Read-only for the chains.  mu_ex = -T log(boltz_sum / n) in K.
"""
function widom!(b::Batch, n_insert::Integer, seed::Integer, draw0::Integer, offsets::Vector{Float64},
                temperature::Float64, boltz_sum::Vector{Float64}, n_overlap::Vector{Int64})
    length(offsets) == 9 || error("offsets: 3 atoms x 3 components")
    length(boltz_sum) == b.n_replicas && length(n_overlap) == b.n_replicas || error("one sum per replica")
    check(ccall((:mmc_batch_widom, libmmc), Int32,
                (Ptr{Cvoid}, Int64, UInt64, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Int64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, n_insert, UInt64(seed), draw0, offsets, temperature, boltz_sum, n_overlap,
                C_NULL, C_NULL, C_NULL))
    return boltz_sum, n_overlap
end
function widom_at!(b::Batch, mol_in::Vector{Float64}, n_insert::Integer, temperature::Float64,
                   boltz_sum::Vector{Float64}, n_overlap::Vector{Int64})
    length(mol_in) == 12 * n_insert * b.n_replicas || error("mol_in: R x n_insert x 12")
    length(boltz_sum) == b.n_replicas && length(n_overlap) == b.n_replicas || error("one sum per replica")
    check(ccall((:mmc_batch_widom_at, libmmc), Int32,
                (Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, n_insert, mol_in, temperature, boltz_sum, n_overlap, C_NULL, C_NULL))
    return boltz_sum, n_overlap
end

# ---- foreign solutes (include/mmc_hip.h, mmc_batch_widom_solute / mmc_batch_widom_solute_at) --------
"""
    widom_solute!(b, offsets, charge, eps, sig, n_insert, seed, draw0, temperature, boltz_sum, n_overlap)
    widom_solute_at!(b, charge, eps, sig, mol_in, n_insert, temperature, boltz_sum, n_overlap)

`n_insert` insertions into every replica of a rigid solute that is not the batch's molecule: S =
`length(charge)` sites (1..16) at c + R offsets[a] (`offsets` 3 S Float64, A, site by site), with
`eps` / `sig` 3 S Float64 (K, A) against the three atom slots of the batch's molecule, already mixed,
site by site.  The draws are `widom!`'s: for one (seed, draw0) the reference points c are its centres
of mass.  `boltz_sum[r] += sum exp(-dU / T)` in insertion order, `n_overlap[r] +=` the insertions of
weight 0; dU as for `widom!`, with the solute's own types.  A solute without charges has no
Coulomb terms; a net charge gets NO neutralising background (the reference has none).
`widom_solute_at!` evaluates the caller's solutes, `mol_in` = R * n_insert * (S + 1) * 3 Float64 (the
sites, then c).  Read-only for the chains.  mu_ex = -T log(boltz_sum / n) in K.
"""
function widom_solute!(b::Batch, offsets::Vector{Float64}, charge::Vector{Float64}, eps::Vector{Float64},
                       sig::Vector{Float64}, n_insert::Integer, seed::Integer, draw0::Integer,
                       temperature::Float64, boltz_sum::Vector{Float64}, n_overlap::Vector{Int64})
    S = length(charge)
    1 <= S <= 16 || error("a solute has 1..16 sites")
    length(offsets) == 3S && length(eps) == 3S && length(sig) == 3S || error("offsets, eps, sig: S x 3")
    length(boltz_sum) == b.n_replicas && length(n_overlap) == b.n_replicas || error("one sum per replica")
    check(ccall((:mmc_batch_widom_solute, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, UInt64, Int64,
                 Float64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, S, offsets, charge, eps, sig, n_insert, UInt64(seed), draw0, temperature, boltz_sum,
                n_overlap, C_NULL, C_NULL, C_NULL))
    return boltz_sum, n_overlap
end
function widom_solute_at!(b::Batch, charge::Vector{Float64}, eps::Vector{Float64}, sig::Vector{Float64},
                          mol_in::Vector{Float64}, n_insert::Integer, temperature::Float64,
                          boltz_sum::Vector{Float64}, n_overlap::Vector{Int64})
    S = length(charge)
    1 <= S <= 16 || error("a solute has 1..16 sites")
    length(eps) == 3S && length(sig) == 3S || error("eps, sig: S x 3")
    length(mol_in) == 3 * (S + 1) * n_insert * b.n_replicas || error("mol_in: R x n_insert x (S + 1) x 3")
    length(boltz_sum) == b.n_replicas && length(n_overlap) == b.n_replicas || error("one sum per replica")
    check(ccall((:mmc_batch_widom_solute_at, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Float64,
                 Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, S, charge, eps, sig, n_insert, mol_in, temperature, boltz_sum, n_overlap, C_NULL, C_NULL))
    return boltz_sum, n_overlap
end

# ---- a fixed solute (include/mmc_hip.h, "A fixed solute") ---------------------------------------------
"""
    set_solute!(b, mol, charge, eps, sig)      remove_solute!(b)
    get_solute(b) -> (n_sites, mol, charge, eps, sig)
    solute_energy(b) -> (u_lj, u_real, ovl)
    rdf_solute(b, numbins, r_max, per_replica) -> hist

One rigid solute of S = `length(charge)` sites (1..16) held fixed at the same place in every replica:
`mol` = 3 (S + 1) Float64, the sites, then the reference point; `eps` / `sig` 3 S Float64 against the
three atom slots of the batch's molecule.  Every trial move, total and saved state then sees it as
molecule N + 1 of potential(..., "ewald"); the host decides every move.  A charged solute (set or
removed) leaves S(k) stale until `recip_long!` / `potential_ewald`.  `solute_energy`: the water-solute
pair energy of every replica (K) and its overlap flag.  `rdf_solute`: UInt64 counts
[numbins, 3, 1 + S] (column-major: C's [1 + S][3][numbins]), with `per_replica` one such block per
replica: row 1 from the reference point, row 1 + a from site a, against the three water slots.
"""
function set_solute!(b::Batch, mol::Vector{Float64}, charge::Vector{Float64}, eps::Vector{Float64},
                     sig::Vector{Float64})
    S = length(charge)
    1 <= S <= 16 || error("a solute has 1..16 sites")
    length(mol) == 3 * (S + 1) && length(eps) == 3S && length(sig) == 3S || error("mol: (S + 1) x 3; eps, sig: S x 3")
    check(ccall((:mmc_batch_set_solute, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                b.h, S, mol, charge, eps, sig))
    return b
end
function remove_solute!(b::Batch)
    check(ccall((:mmc_batch_set_solute, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                b.h, 0, C_NULL, C_NULL, C_NULL, C_NULL))
    return b
end
function get_solute(b::Batch)
    n = Ref{Int32}(0)
    mol, charge, eps, sig = zeros(51), zeros(16), zeros(48), zeros(48)
    check(ccall((:mmc_batch_get_solute, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                b.h, n, mol, charge, eps, sig))
    S = Int(n[])
    return S, mol[1:(S > 0 ? 3 * (S + 1) : 0)], charge[1:S], eps[1:3S], sig[1:3S]
end
function solute_energy(b::Batch)
    u_lj, u_real, ovl = zeros(b.n_replicas), zeros(b.n_replicas), zeros(UInt8, b.n_replicas)
    check(ccall((:mmc_batch_solute_energy, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}), b.h, u_lj, u_real, ovl))
    return u_lj, u_real, ovl
end
function rdf_solute(b::Batch, numbins::Integer, r_max::Float64 = 0.0, per_replica::Bool = false)
    S = get_solute(b)[1]
    hist = per_replica ? zeros(UInt64, numbins, 3, 1 + S, b.n_replicas) : zeros(UInt64, numbins, 3, 1 + S)
    check(ccall((:mmc_batch_rdf_solute, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Float64, Int32, Ptr{UInt64}), b.h, numbins, r_max, per_replica ? 1 : 0, hist))
    return hist
end

"""
    hydration_map(b, n_half, cell, channel_mask, per_replica) -> maps

The solute-centred maps of the water around the fixed solute (`mmc_batch_hydration_map`): Int64
[cells + 2, n_ch] (column-major: C's [n_ch][cells + 2]) with cells = (2 n_half)^3 and n_ch =
count_ones(channel_mask), with `per_replica` one such block per replica.  Bits 0..2 of the mask: counts
of the three water slots; 3..5: sums of the unit bisector's components in units of 2^-30; 6, 7: sums of
the water-solute LJ and real-space energy in units of 2^-20 K.  The last two entries of a channel: the
deposits outside the cube, and the waters left out.
"""
function hydration_map(b::Batch, n_half::Integer, cell::Float64, channel_mask::Integer = 255,
                       per_replica::Bool = false)
    1 <= n_half <= 12 && 1 <= channel_mask <= 255 || error("n_half: 1..12, channel_mask: 1..255")
    n_ch, len = count_ones(channel_mask), (2 * n_half)^3 + 2
    maps = per_replica ? zeros(Int64, len, n_ch, b.n_replicas) : zeros(Int64, len, n_ch)
    check(ccall((:mmc_batch_hydration_map, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Float64, Int32, Int32, Ptr{Int64}),
                b.h, n_half, cell, channel_mask, per_replica ? 1 : 0, maps))
    return maps
end

"""
    solute_forces(b; details = false) -> (force, torque, flags[, site_lj, field, phi, recip])

What the water does to the fixed solute in every replica (`mmc_batch_solute_forces`): `force`, `torque`
[3, R] (column-major: C's [R][3]) in K / A and K about the reference point, `flags` [R] (bit 0 an overlap,
bit 1 a non-finite output; a flagged replica's rows are zeros).  With `details` also `site_lj`, `field`
[3, S, R], `phi` [S, R] and `recip` [4, S, R]: the Lennard-Jones force on every site, the electric field
and the electrostatic potential there (phi = dU/dq_a), and the reciprocal part of (field, phi) alone.
"""
function solute_forces(b::Batch; details::Bool = false)
    R, S = b.n_replicas, get_solute(b)[1]
    force, torque, flags = zeros(3, R), zeros(3, R), zeros(UInt8, R)
    site_lj, field, phi, recip = zeros(3, S, R), zeros(3, S, R), zeros(S, R), zeros(4, S, R)
    check(ccall((:mmc_batch_solute_forces, libmmc), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{UInt8}),
                b.h, force, torque, details ? site_lj : C_NULL, details ? field : C_NULL, details ? phi : C_NULL,
                details ? recip : C_NULL, flags))
    return details ? (force, torque, flags, site_lj, field, phi, recip) : (force, torque, flags)
end

# ---- solute pairs (include/mmc_hip.h, mmc_batch_widom_pair / mmc_batch_widom_pair_at) -----------------
"""
    widom_pair!(b, A, B, eps_ab, sig_ab, d, n_insert, seed, draw0, temperature, sums)
    widom_pair_at!(b, A, B, eps_ab, sig_ab, n_sep, mol_a_in, mol_b_in, n_insert, temperature, sums)

`n_insert` insertions into every replica of two rigid foreign solutes, B at the `K = length(d)`
separations `d` (A, each below half the box) from A along one random ray per insertion: the sums of
the potential distribution theorem's g_AB(d) = <exp(-dU_AB / T)> / (<exp(-dU_A / T)> <exp(-dU_B / T)>)
at infinite dilution.  `A` and `B` are named tuples `(offsets, charge, eps, sig)` as `widom_solute!`
takes them (S_A + S_B <= 16), `eps_ab` / `sig_ab` are S_A * S_B Float64, A's site by A's site.
`sums` is a named tuple `(boltz_a, n_zero_a, boltz_b, n_zero_b, boltz_ab, n_zero_ab)`: R, R, K * R,
K * R, K * R, K * R entries (separation fastest), added to in insertion order.  A is drawn as
`widom_solute!` draws it.  `widom_pair_at!` evaluates the caller's placements: `mol_a_in` = R *
n_insert * (S_A + 1) * 3 and `mol_b_in` = R * n_insert * K * (S_B + 1) * 3 Float64 (sites, then the
reference point).  Read-only for the chains.  w(d) = -T log g_AB(d) in K.
"""
function widom_pair!(b::Batch, A, B, eps_ab::Vector{Float64}, sig_ab::Vector{Float64}, d::Vector{Float64},
                     n_insert::Integer, seed::Integer, draw0::Integer, temperature::Float64, sums)
    SA, SB, K = length(A.charge), length(B.charge), length(d)
    SA >= 1 && SB >= 1 && SA + SB <= 16 || error("a solute pair has at most 16 sites in all")
    length(eps_ab) == SA * SB && length(sig_ab) == SA * SB || error("eps_ab, sig_ab: S_A x S_B")
    pair_sums_ok(b, sums, K)
    check(ccall((:mmc_batch_widom_pair, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64,
                 UInt64, Int64, Float64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, SA, A.offsets, A.charge, A.eps, A.sig, SB, B.offsets, B.charge, B.eps, B.sig, eps_ab, sig_ab, K,
                d, n_insert, UInt64(seed), draw0, temperature, sums.boltz_a, sums.n_zero_a, sums.boltz_b,
                sums.n_zero_b, sums.boltz_ab, sums.n_zero_ab, C_NULL, C_NULL, C_NULL, C_NULL))
    return sums
end
function widom_pair_at!(b::Batch, A, B, eps_ab::Vector{Float64}, sig_ab::Vector{Float64}, n_sep::Integer,
                        mol_a_in::Vector{Float64}, mol_b_in::Vector{Float64}, n_insert::Integer,
                        temperature::Float64, sums)
    SA, SB, K = length(A.charge), length(B.charge), Int(n_sep)
    SA >= 1 && SB >= 1 && SA + SB <= 16 || error("a solute pair has at most 16 sites in all")
    length(eps_ab) == SA * SB && length(sig_ab) == SA * SB || error("eps_ab, sig_ab: S_A x S_B")
    length(mol_a_in) == 3 * (SA + 1) * n_insert * b.n_replicas || error("mol_a_in: R x n_insert x (S_A + 1) x 3")
    length(mol_b_in) == 3 * (SB + 1) * K * n_insert * b.n_replicas || error("mol_b_in: R x n_insert x K x (S_B + 1) x 3")
    pair_sums_ok(b, sums, K)
    check(ccall((:mmc_batch_widom_pair_at, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Float64,
                 Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, SA, A.charge, A.eps, A.sig, SB, B.charge, B.eps, B.sig, eps_ab, sig_ab, K, n_insert, mol_a_in,
                mol_b_in, temperature, sums.boltz_a, sums.n_zero_a, sums.boltz_b, sums.n_zero_b, sums.boltz_ab,
                sums.n_zero_ab, C_NULL, C_NULL))
    return sums
end
function pair_sums_ok(b::Batch, sums, K::Integer)
    R = b.n_replicas
    length(sums.boltz_a) == R && length(sums.n_zero_a) == R || error("boltz_a, n_zero_a: one per replica")
    all(length(v) == R * K for v in (sums.boltz_b, sums.n_zero_b, sums.boltz_ab, sums.n_zero_ab)) ||
        error("boltz_b, n_zero_b, boltz_ab, n_zero_ab: R x K")
    return nothing
end

# ---- deletion energies (include/mmc_hip.h, mmc_batch_deletion) -------------------------------------
"""
    deletion(b, temperature; sel = nothing, bins = nothing, per_replica = false,
             boltz_sum = zeros(R), n_flagged = zeros(Int64, R))

The deletion (binding) energy dU_i = potential(N) - potential(N without i) (energy.jl:946-1032) of
the molecules `sel` (1-based indices shared by all replicas, duplicates allowed; `nothing` = all)
of every replica, read-only for the chains; the reference has no deletion code.  `bins` =
`(n_bins, u_lo, u_hi)` asks for the histogram of dU: `n_bins + 2` UInt64 counts (slot 1 below
`u_lo`, the last at or above `u_hi`), or an `(n_bins + 2, R)` matrix with `per_replica`.  Returns
`(hist, esum, boltz_sum, n_flagged)`: `esum` a `(4, R)` matrix (sums of d_lj, d_real, d_recip and the
number summed), `boltz_sum[r] += sum exp(+dU / T)` (inverse Widom), `n_flagged[r] +=` the molecules
with an overlap or a non-finite dU, which enter no sum and no bin.
"""
function deletion(b::Batch, temperature::Float64; sel::Union{Nothing,Vector{<:Integer}} = nothing,
                  bins::Union{Nothing,Tuple{Int,Float64,Float64}} = nothing, per_replica::Bool = false,
                  boltz_sum::Vector{Float64} = zeros(Float64, b.n_replicas),
                  n_flagged::Vector{Int64} = zeros(Int64, b.n_replicas))
    length(boltz_sum) == b.n_replicas && length(n_flagged) == b.n_replicas || error("one sum per replica")
    sel0 = sel === nothing ? Int32[] : Int32[i - 1 for i in sel]
    sel === nothing || !isempty(sel0) || error("sel must not be empty")
    n_bins, u_lo, u_hi = bins === nothing ? (0, 0.0, 0.0) : bins
    hist = bins === nothing ? UInt64[] :
           per_replica ? zeros(UInt64, n_bins + 2, b.n_replicas) : zeros(UInt64, n_bins + 2)
    esum = zeros(Float64, 4, b.n_replicas)
    check(ccall((:mmc_batch_deletion, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Int32}, Float64, Int32, Float64, Float64, Int32, Ptr{UInt64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}),
                b.h, length(sel0), sel === nothing ? C_NULL : sel0, temperature, n_bins, u_lo, u_hi,
                per_replica ? 1 : 0, bins === nothing ? C_NULL : hist, esum, boltz_sum, n_flagged,
                C_NULL, C_NULL))
    return hist, esum, boltz_sum, n_flagged
end

# ---- forces and torques (include/mmc_hip.h, mmc_batch_forces) --------------------------------------
"""
    forces(b; sel = nothing, mass = nothing, details = false, n_flagged = zeros(Int64, R))

Minus the gradient of potential(..., "ewald") (energy.jl:946-1032) at fixed neighbour sets on the
atoms of the molecules `sel` (1-based indices shared by all replicas, duplicates allowed; `nothing`
= all) of every replica, read-only for the chains; the reference has no forces.  `mass` (3 values,
one per atom slot) asks for t = tau' I^-1 tau.  Returns `(fsum, n_flagged)`: `fsum` a `(9, R)` matrix
(number summed, sum F.F, sum tau.tau, sum t, sum F_x, sum F_y, sum F_z, sum w_lj, sum w_real);
with `details` also `force`, `torque`, `vir` `(3, n, R)`, `atom` `(3, 3, n, R)` and `ovl` `(n, R)`.
"""
function forces(b::Batch; sel::Union{Nothing,Vector{<:Integer}} = nothing,
                mass::Union{Nothing,Vector{Float64}} = nothing, details::Bool = false,
                n_flagged::Vector{Int64} = zeros(Int64, b.n_replicas))
    length(n_flagged) == b.n_replicas || error("one count per replica")
    mass === nothing || length(mass) == 3 || error("mass: one value per atom slot")
    sel0 = sel === nothing ? Int32[] : Int32[i - 1 for i in sel]
    sel === nothing || !isempty(sel0) || error("sel must not be empty")
    n = sel === nothing ? b.n_mol : length(sel0)
    fsum = zeros(Float64, 9, b.n_replicas)
    force = details ? zeros(Float64, 3, n, b.n_replicas) : Float64[]
    torque = details ? zeros(Float64, 3, n, b.n_replicas) : Float64[]
    vir = details ? zeros(Float64, 3, n, b.n_replicas) : Float64[]
    atom = details ? zeros(Float64, 3, 3, n, b.n_replicas) : Float64[]
    ovl = details ? zeros(UInt8, n, b.n_replicas) : UInt8[]
    check(ccall((:mmc_batch_forces, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt8}),
                b.h, length(sel0), sel === nothing ? C_NULL : sel0, mass === nothing ? C_NULL : mass,
                details ? force : C_NULL, details ? torque : C_NULL, details ? vir : C_NULL,
                details ? atom : C_NULL, fsum, n_flagged, details ? ovl : C_NULL))
    return details ? (fsum, n_flagged, force, torque, vir, atom, ovl) : (fsum, n_flagged)
end

# ---- structure observables (include/mmc_hip.h, mmc_batch_rdf_sites / mmc_batch_dipoles) ----------
"""
    rdf_sites(b, numbins; r_max = 0.0, per_replica = false)
    dipoles(b)

`rdf_sites`: the six site-site pair histograms of gr.jl's pair loop in one pass, slot pairs
(0,0) (0,1) (0,2) (1,1) (1,2) (2,2): a `(numbins + 1, 6)` UInt64 matrix summed over the replicas
(column k = row k of the C layout), or `(numbins + 1, 6, R)` with `per_replica`.  `r_max <= 0`: bins
of (L / 2) / numbins (one shared box only), else of r_max / numbins.  `dipoles`: the total dipole
moment of every replica, a `(3, R)` Float64 matrix in e A.  Both are read-only for the chains.
"""
function rdf_sites(b::Batch, numbins::Integer; r_max::Float64 = 0.0, per_replica::Bool = false)
    numbins >= 1 || error("numbins must be >= 1")
    hist = per_replica ? zeros(UInt64, numbins + 1, 6, b.n_replicas) : zeros(UInt64, numbins + 1, 6)
    check(ccall((:mmc_batch_rdf_sites, libmmc), Int32, (Ptr{Cvoid}, Int32, Float64, Int32, Ptr{UInt64}),
                b.h, numbins, r_max, per_replica ? 1 : 0, hist))
    return hist
end
function dipoles(b::Batch)
    dip = zeros(Float64, 3, b.n_replicas)
    check(ccall((:mmc_batch_dipoles, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h, dip))
    return dip
end

# ---- orientational pair correlations (include/mmc_hip.h, mmc_batch_orient_corr) --------------------
"""
    orient_corr(b, numbins; r_max = 0.0, per_replica = false)

Orientational pair correlations over the slot-1 (O) separation, every pair i < j once, in the bins of
`rdf_sites`' first column plus slot numbins + 1 for every pair beyond r_max: a `(numbins + 2, 4)`
Int64 matrix summed over the replicas (column k = row k of the C layout), or `(numbins + 2, 4, R)`
with `per_replica`.  Column 1 the pair count; columns 2, 3, 4 the sums of u_i.u_j,
3 (u_i.rhat)(u_j.rhat) - u_i.u_j and P2(u_i.u_j) in units of 2^-30, u the unit vector of the
molecule's dipole.  G_K(R) = 1 + 2 cumsum(column 2) / (2^30 N frames); read-only for the chains.
"""
function orient_corr(b::Batch, numbins::Integer; r_max::Float64 = 0.0, per_replica::Bool = false)
    numbins >= 1 || error("numbins must be >= 1")
    hist = per_replica ? zeros(Int64, numbins + 2, 4, b.n_replicas) : zeros(Int64, numbins + 2, 4)
    check(ccall((:mmc_batch_orient_corr, libmmc), Int32, (Ptr{Cvoid}, Int32, Float64, Int32, Ptr{Int64}),
                b.h, numbins, r_max, per_replica ? 1 : 0, hist))
    return hist
end

# ---- spatial distribution functions (include/mmc_hip.h, mmc_batch_sdf) -----------------------------
"""
    sdf(b, n_half, cell; fold = 3, site_mask = 1, per_replica = false)

The counts of the spatial distribution function: the sites selected in `site_mask` (bit a = slot a,
1 = O) of every neighbour per cell of a cube of half-width `n_half * cell` in the centre molecule's
body-fixed frame (z the bisector, x in the molecular plane); `fold` bit 0 / 1 folds x / y onto
|x| / |y|.  Returns `(grid, outside, noframe)`: `grid` a `(g_z, g_y, g_x)` UInt64 array (the C layout
read column-major; g = n_half along a folded axis, 2 n_half otherwise), the deposits outside the cube
and those of centres without a frame.  Summed over the replicas, or with a trailing replica axis with
`per_replica`.  Read-only for the chains.
"""
function sdf(b::Batch, n_half::Integer, cell::Float64; fold::Integer = 3, site_mask::Integer = 1,
             per_replica::Bool = false)
    n_half >= 1 || error("n_half must be >= 1")
    0 <= fold <= 3 || error("fold must be in 0..3")
    gx, gy, gz = (fold & 1) != 0 ? n_half : 2n_half, (fold & 2) != 0 ? n_half : 2n_half, 2n_half
    cells = gx * gy * gz
    cells <= 32768 || error("the grid has more than 32768 cells")
    hist = per_replica ? zeros(UInt64, cells + 2, b.n_replicas) : zeros(UInt64, cells + 2)
    check(ccall((:mmc_batch_sdf, libmmc), Int32, (Ptr{Cvoid}, Int32, Float64, Int32, Int32, Int32, Ptr{UInt64}),
                b.h, n_half, cell, fold, site_mask, per_replica ? 1 : 0, hist))
    if per_replica
        return reshape(hist[1:cells, :], gz, gy, gx, :), hist[cells + 1, :], hist[cells + 2, :]
    end
    return reshape(hist[1:cells], gz, gy, gx), hist[cells + 1], hist[cells + 2]
end

# ---- pair-energy distributions (include/mmc_hip.h, mmc_batch_pair_energy) --------------------------
"""
    pair_energy(b, numbins; r_max = 0.0, ebins = nothing, u_hb = nothing, per_replica = false)

The interaction energy u = u_C + u_LJ (K) of every pair of molecules whose slot-1 (O) separation is in
range, every pair i < j once, over the bins of `orient_corr`.  Returns `(rows, uhist, nhb, flagged)`:
`rows` a `(numbins + 2, 3)` Int64 matrix (column k = row k of the C layout: the pair count and the sums
of u_C and u_LJ in units of 2^-20 K); with `ebins = (n_ebins, u_lo, u_hi)` `uhist`, `n_ebins + 2`
UInt64 counts of the pairs in range binned on u (slot 1 below `u_lo`, the last at or above `u_hi`),
else `nothing`; with `u_hb` `nhb`, 9 UInt64 counts of the molecules with 0..7 and 8 or more partners
below `u_hb`, else `nothing`; `flagged`, the pairs in range whose energy is not finite or beyond
2^20 K.  Summed over the replicas, or with a trailing replica axis with `per_replica`.  Read-only for
the chains.
"""
function pair_energy(b::Batch, numbins::Integer; r_max::Float64 = 0.0,
                     ebins::Union{Nothing,Tuple{Integer,Float64,Float64}} = nothing,
                     u_hb::Union{Nothing,Float64} = nothing, per_replica::Bool = false)
    numbins >= 1 || error("numbins must be >= 1")
    n_ebins, u_lo, u_hi = ebins === nothing ? (0, 0.0, 1.0) : ebins
    ebins === nothing || 1 <= n_ebins <= 4096 || error("n_ebins must be in 1..4096")
    tail = per_replica ? (b.n_replicas,) : ()
    rows = zeros(Int64, numbins + 2, 3, tail...)
    uhist = ebins === nothing ? nothing : zeros(UInt64, n_ebins + 2, tail...)
    nhb = u_hb === nothing ? nothing : zeros(UInt64, 9, tail...)
    flagged = zeros(UInt64, per_replica ? b.n_replicas : 1)
    check(ccall((:mmc_batch_pair_energy, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Float64, Int32, Float64, Float64, Float64, Int32, Ptr{Int64}, Ptr{UInt64},
                 Ptr{UInt64}, Ptr{UInt64}),
                b.h, numbins, r_max, n_ebins, u_lo, u_hi, u_hb === nothing ? 0.0 : u_hb, per_replica ? 1 : 0,
                rows, uhist === nothing ? C_NULL : uhist, nhb === nothing ? C_NULL : nhb, flagged))
    return rows, uhist, nhb, flagged
end

# ---- partial structure factors (include/mmc_hip.h, mmc_batch_structure_factor) --------------------
"""
    structure_factor(b, n_max; per_replica = false)

The products rho_a(n) rho_b(n)* of the three atom-slot densities over the box's own wave vectors
q = 2 pi n / L, 0 < |n|^2 <= n_max^2 (n_max <= 32), summed per shell s = |n|^2 (index s + 1).
Returns `(count, sq)`: `count` the Int32 number of vectors of each shell; `sq` an
`(n_max^2 + 1, 6, R)` Int64 array in units of 2^-24 with `per_replica`, else an `(n_max^2 + 1, 6)`
Float64 matrix summed over the replicas (column k = row k of the C layout: slot pairs (0,0) (0,1)
(0,2) (1,1) (1,2) (2,2), a cross term held once).  S_ab(q) = sq / (count sqrt(N_a N_b) frames);
read-only for the chains.  With per-replica boxes only `per_replica = true`.
"""
function structure_factor(b::Batch, n_max::Integer; per_replica::Bool = false)
    1 <= n_max <= 32 || error("n_max must be in 1..32")
    S = n_max * n_max + 1
    count = zeros(Int32, S)
    if per_replica
        sq = zeros(Int64, S, 6, b.n_replicas)
        check(ccall((:mmc_batch_structure_factor, libmmc), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}),
                    b.h, n_max, 1, count, sq, C_NULL))
        return count, sq
    end
    sq_sum = zeros(Float64, S, 6)
    check(ccall((:mmc_batch_structure_factor, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}),
                b.h, n_max, 0, count, C_NULL, sq_sum))
    return count, sq_sum
end

# ---- local order (include/mmc_hip.h, mmc_batch_local_order) ----------------------------------------
"""
    local_order(b; q_bins = 400, r_hb = 3.5, theta_deg = 30.0, per_replica = false)

Hydrogen bonds (O-O closer than `r_hb`, H-O...O angle within `theta_deg`) and the tetrahedral order
parameter q of every molecule (slot 1 = O, slots 2 and 3 = H) in one read-only pass.  Returns
`(hb_hist, q_hist, q_sum)`: `hb_hist` a `(9, 3)` UInt64 matrix (columns donated, accepted, total;
molecules with n = 0..8 bonds), `q_hist` `q_bins` counts over [-3, 1] -- `(9, 3, R)` and
`(q_bins, R)` with `per_replica` -- and `q_sum` `(2, R)`: the sum of the replica's finite q and their
number.
"""
function local_order(b::Batch; q_bins::Integer = 400, r_hb::Float64 = 3.5, theta_deg::Float64 = 30.0,
                     per_replica::Bool = false)
    1 <= q_bins <= 4096 || error("q_bins must be in 1..4096")
    hb_hist = per_replica ? zeros(UInt64, 9, 3, b.n_replicas) : zeros(UInt64, 9, 3)
    q_hist = per_replica ? zeros(UInt64, q_bins, b.n_replicas) : zeros(UInt64, q_bins)
    q_sum = zeros(Float64, 2, b.n_replicas)
    check(ccall((:mmc_batch_local_order, libmmc), Int32,
                (Ptr{Cvoid}, Float64, Float64, Int32, Int32, Ptr{UInt64}, Ptr{UInt64}, Ptr{Float64},
                 Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}),
                b.h, r_hb, cosd(theta_deg), q_bins, per_replica ? 1 : 0, hb_hist, q_hist, q_sum,
                C_NULL, C_NULL, C_NULL))
    return hb_hist, q_hist, q_sum
end

# ---- shell order (include/mmc_hip.h, mmc_batch_shell_order) ----------------------------------------
"""
    shell_order(b; r_list = 6.0, r_lsi = 3.7, r_ang = 3.3, r_hb = 3.5, theta_deg = 30.0, n_rank = 8,
                r_bins = 300, lsi_bins = 200, lsi_max = 0.4, ang_bins = 180, zeta_bins = 200,
                zeta_lo = -1.5, zeta_hi = 2.5, per_replica = false)

Every molecule's O-O neighbours inside `r_list` sorted by distance (slot 1 = O, slots 2 and 3 = H), and
from that list, in one read-only pass: `rank_hist` `(r_bins + 1, n_rank)` UInt64, column k the distance
to the k-th neighbour in bins of `r_list / r_bins` (last row: fewer than k listed); `lsi_hist`
`lsi_bins + 1` counts of the local structure index over [0, `lsi_max`]; `ang_hist` `ang_bins + 1`
counts of the cosine of the O-O-O angles between neighbours inside `r_ang` over [-1, 1]; `zeta_hist`
`zeta_bins + 1` counts of zeta over [`zeta_lo`, `zeta_hi`] with `local_order`'s bonds; the last entry
of each is "undefined" -- all with a trailing dimension R with `per_replica`.  Returns
`(rank_hist, lsi_hist, ang_hist, zeta_hist, flagged, sums)`: `flagged` the molecules per replica with
more than 64 neighbours inside `r_list` (in no histogram), `sums` `(4, R)`: the sum of the replica's
defined LSI, their number, the sum of its defined zeta, their number.
"""
function shell_order(b::Batch; r_list::Float64 = 6.0, r_lsi::Float64 = 3.7, r_ang::Float64 = 3.3,
                     r_hb::Float64 = 3.5, theta_deg::Float64 = 30.0, n_rank::Integer = 8, r_bins::Integer = 300,
                     lsi_bins::Integer = 200, lsi_max::Float64 = 0.4, ang_bins::Integer = 180,
                     zeta_bins::Integer = 200, zeta_lo::Float64 = -1.5, zeta_hi::Float64 = 2.5,
                     per_replica::Bool = false)
    1 <= n_rank <= 16 || error("n_rank must be in 1..16")
    all(1 <= n <= 1024 for n in (r_bins, lsi_bins, ang_bins, zeta_bins)) || error("bin counts must be in 1..1024")
    tail = per_replica ? (b.n_replicas,) : ()
    rank_hist = zeros(UInt64, r_bins + 1, n_rank, tail...)
    lsi_hist = zeros(UInt64, lsi_bins + 1, tail...)
    ang_hist = zeros(UInt64, ang_bins + 1, tail...)
    zeta_hist = zeros(UInt64, zeta_bins + 1, tail...)
    flagged = zeros(UInt64, b.n_replicas)
    sums = zeros(Float64, 4, b.n_replicas)
    check(ccall((:mmc_batch_shell_order, libmmc), Int32,
                (Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Int32, Int32, Int32, Float64, Int32, Int32,
                 Float64, Float64, Int32, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64},
                 Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                b.h, r_list, r_lsi, r_ang, r_hb, cosd(theta_deg), n_rank, r_bins, lsi_bins, lsi_max, ang_bins,
                zeta_bins, zeta_lo, zeta_hi, per_replica ? 1 : 0, rank_hist, lsi_hist, ang_hist, zeta_hist, flagged,
                sums, C_NULL, C_NULL, C_NULL, C_NULL))
    return rank_hist, lsi_hist, ang_hist, zeta_hist, flagged, sums
end

# ---- Voronoi cells (include/mmc_hip.h, mmc_batch_voronoi) -------------------------------------------
"""
    voronoi(b; r_list = 7.0, area_min = 0.0, v_bins = 200, v_max = 80.0, eta_bins = 200, eta_max = 3.0,
            r_bins = 280, per_replica = false)

The Voronoi cell of every molecule's O (slot 1) from its O-O neighbours inside `r_list` (at most 64, at
most half the smallest box), in one read-only pass: `vol_hist` `v_bins + 1` UInt64 counts of the cell
volume over [0, `v_max`); `eta_hist` `eta_bins + 1` counts of the asphericity S^3 / (36 pi V^2) over
[1, `eta_max`); the last entry of each is "beyond"; `face_hist` 65 counts of molecules by their number
of counted faces (area > `area_min`); `side_hist` 17 counts of counted faces by number of sides;
`nbr_hist` `r_bins + 1` counts of the O-O distance of counted faces over [0, `r_list`) -- all with a
trailing dimension R with `per_replica`.  Returns `(vol_hist, eta_hist, face_hist, side_hist, nbr_hist,
flagged, sums)`: `flagged` `(3, R)` the molecules per replica with more than 64 neighbours in range,
with a cell that is not certified closed, with a polygon beyond 16 vertices (in no histogram and no
sum); `sums` `(8, R)`: the number summed, sum V, sum V^2, sum S, sum eta, sum of counted faces, sum of
their area, 0.
"""
function voronoi(b::Batch; r_list::Float64 = 7.0, area_min::Float64 = 0.0, v_bins::Integer = 200,
                 v_max::Float64 = 80.0, eta_bins::Integer = 200, eta_max::Float64 = 3.0, r_bins::Integer = 280,
                 per_replica::Bool = false)
    all(1 <= n <= 1024 for n in (v_bins, eta_bins, r_bins)) || error("bin counts must be in 1..1024")
    tail = per_replica ? (b.n_replicas,) : ()
    vol_hist = zeros(UInt64, v_bins + 1, tail...)
    eta_hist = zeros(UInt64, eta_bins + 1, tail...)
    face_hist = zeros(UInt64, 65, tail...)
    side_hist = zeros(UInt64, 17, tail...)
    nbr_hist = zeros(UInt64, r_bins + 1, tail...)
    flagged = zeros(UInt64, 3, b.n_replicas)
    sums = zeros(Float64, 8, b.n_replicas)
    check(ccall((:mmc_batch_voronoi, libmmc), Int32,
                (Ptr{Cvoid}, Float64, Float64, Int32, Float64, Int32, Float64, Int32, Int32, Ptr{UInt64}, Ptr{UInt64},
                 Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                b.h, r_list, area_min, v_bins, v_max, eta_bins, eta_max, r_bins, per_replica ? 1 : 0, vol_hist,
                eta_hist, face_hist, side_hist, nbr_hist, flagged, sums, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    return vol_hist, eta_hist, face_hist, side_hist, nbr_hist, flagged, sums
end

# ---- bond order (include/mmc_hip.h, mmc_batch_bond_order) -------------------------------------------
"""
    bond_order(b; l = 3, r_nb = 3.5, n_nb = 4, a = (-Inf, -0.8), b_win = (-0.35, 0.25), min_a = 3,
               min_ab = 4, q_bins = 200, c_bins = 200, per_replica = false)

Steinhardt's q_l of every molecule over its `n_nb` nearest O-O neighbours inside `r_nb` (l = 3, 4 or
6), the neighbour-averaged qbar_l, the bond correlations c_ij, the bonds in the closed windows `a` and
`b_win` (defaults: CHILL+'s staggered and eclipsed bonds), and the clusters of solid-like molecules (at
least `min_a` bonds in `a` and `min_ab` in both), in one read-only pass.  Returns `(q_hist, qbar_hist,
c_hist, ab_hist, size_hist, stats, sums)`: `q_hist`, `qbar_hist` `q_bins + 1` UInt64 over [0, 1] and
`c_hist` `c_bins + 1` over [-1, 1] (last entry: undefined), `ab_hist` `(17, 17)` with the molecules at
`[n_B + 1, n_A + 1]`, `size_hist` `N + 1` clusters by size -- all with a trailing dimension R with
`per_replica` -- `stats` `(8, R)` Int64 (defined, undefined, flagged, truncated, solid-like molecules,
clusters, the largest cluster, the sum of s^2) and `sums` `(4, R)`: the sum of the replica's defined
q_l, their number, the sum of its defined qbar_l, their number.
"""
function bond_order(b::Batch; l::Integer = 3, r_nb::Float64 = 3.5, n_nb::Integer = 4,
                    a::Tuple{Float64,Float64} = (-Inf, -0.8), b_win::Tuple{Float64,Float64} = (-0.35, 0.25),
                    min_a::Integer = 3, min_ab::Integer = 4, q_bins::Integer = 200, c_bins::Integer = 200,
                    per_replica::Bool = false)
    l in (3, 4, 6) || error("l must be 3, 4 or 6")
    1 <= n_nb <= 16 || error("n_nb must be in 1..16")
    all(1 <= n <= 4096 for n in (q_bins, c_bins)) || error("bin counts must be in 1..4096")
    tail = per_replica ? (b.n_replicas,) : ()
    q_hist = zeros(UInt64, q_bins + 1, tail...)
    qbar_hist = zeros(UInt64, q_bins + 1, tail...)
    c_hist = zeros(UInt64, c_bins + 1, tail...)
    ab_hist = zeros(UInt64, 17, 17, tail...)
    size_hist = zeros(UInt64, b.n_mol + 1, tail...)
    stats = zeros(Int64, 8, b.n_replicas)
    sums = zeros(Float64, 4, b.n_replicas)
    check(ccall((:mmc_batch_bond_order, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Float64, Int32, Float64, Float64, Float64, Float64, Int32, Int32, Int32, Int32,
                 Int32, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}),
                b.h, l, r_nb, n_nb, a[1], a[2], b_win[1], b_win[2], min_a, min_ab, q_bins, c_bins,
                per_replica ? 1 : 0, q_hist, qbar_hist, c_hist, ab_hist, size_hist, stats, sums,
                C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    return q_hist, qbar_hist, c_hist, ab_hist, size_hist, stats, sums
end

# ---- hydrogen-bond network (include/mmc_hip.h, mmc_batch_hbond_network) -----------------------------
"""
    hbond_network(b; r_hb = [3.5], theta_deg = [30.0], min_bonds = [0], per_replica = false)

The hydrogen-bond graph of every replica under K = 1..8 criteria at once, read-only: bonds by
`local_order`'s geometry with `(r_hb[k], theta_deg[k])`, sites the molecules with at least
`min_bonds[k]` bonds.  Returns `(size_hist, deg_hist, stats)`: `size_hist` `(N + 1, K)` UInt64
(clusters by number of sites), `deg_hist` `(17, K)` (molecules by number of bonds) -- each with a
trailing dimension R with `per_replica` -- and `stats` `(8, K, R)` Int64: bonds, sites, clusters, the
largest cluster, the sum of s^2, the OR of the wrap masks (x = 1, y = 2, z = 4), the largest wrapping
cluster, flagged.
"""
function hbond_network(b::Batch; r_hb::Vector{Float64} = [3.5], theta_deg::Vector{Float64} = [30.0],
                       min_bonds::Vector{Int32} = Int32[0], per_replica::Bool = false)
    K = length(r_hb)
    1 <= K <= 8 || error("1 to 8 criteria")
    length(theta_deg) == K && length(min_bonds) == K || error("r_hb, theta_deg and min_bonds have one length")
    N = b.n_mol
    size_hist = per_replica ? zeros(UInt64, N + 1, K, b.n_replicas) : zeros(UInt64, N + 1, K)
    deg_hist = per_replica ? zeros(UInt64, 17, K, b.n_replicas) : zeros(UInt64, 17, K)
    stats = zeros(Int64, 8, K, b.n_replicas)
    check(ccall((:mmc_batch_hbond_network, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{UInt64}, Ptr{UInt64},
                 Ptr{Int64}, Ptr{Int32}, Ptr{Int32}),
                b.h, K, r_hb, cosd.(theta_deg), min_bonds, per_replica ? 1 : 0, size_hist, deg_hist, stats,
                C_NULL, C_NULL))
    return size_hist, deg_hist, stats
end

# ---- hydrogen-bond rings (include/mmc_hip.h, mmc_batch_hbond_rings) ---------------------------------
"""
    hbond_rings(b; r_hb = 3.5, theta_deg = 30.0, n_max = 8, per_replica = false)

The shortest-path rings (Franzblau) of 3 to `n_max` <= 8 molecules in the hydrogen-bond graph of every
replica under one criterion (`hbond_network`'s bond), read-only.  Returns `(ring_hist, member_hist,
stats)`: `ring_hist` `(9, 3)` UInt64 (by size: the rings that do not wrap the box, those that do, the
homodromic ones among the first), `member_hist` `(33, 9)` (molecules by the number of n-rings they are
members of; row 0: rings of any size; the last bin 32 or more) -- each with a trailing dimension R with
`per_replica` -- and `stats` `(8, R)` Int64: bonds, rings, wrapping rings, homodromic rings, molecules
in no ring, the most rings one molecule is in, rings dropped from a ring list (0 here), flagged.
"""
function hbond_rings(b::Batch; r_hb::Float64 = 3.5, theta_deg::Float64 = 30.0, n_max::Integer = 8,
                     per_replica::Bool = false)
    3 <= n_max <= 8 || error("n_max is 3 to 8")
    ring_hist = per_replica ? zeros(UInt64, 9, 3, b.n_replicas) : zeros(UInt64, 9, 3)
    member_hist = per_replica ? zeros(UInt64, 33, 9, b.n_replicas) : zeros(UInt64, 33, 9)
    stats = zeros(Int64, 8, b.n_replicas)
    # (the macro form: count_out is the only 16-bit pointer of the interface, NULL here)
    check(@ccall libmmc.mmc_batch_hbond_rings(b.h::Ptr{Cvoid}, r_hb::Float64, cosd(theta_deg)::Float64,
                                              n_max::Int32, (per_replica ? 1 : 0)::Int32,
                                              ring_hist::Ptr{UInt64}, member_hist::Ptr{UInt64},
                                              stats::Ptr{Int64}, C_NULL::Ptr{UInt16}, 0::Int64,
                                              C_NULL::Ptr{Int32})::Int32)
    return ring_hist, member_hist, stats
end

# ---- cavities and occupancy (include/mmc_hip.h, mmc_batch_cavity, mmc_batch_cavity_at) --------------
"""
    cavity(b, n_probe, seed; draw0 = 0, radii = [3.3], site = 0, n_cap = 32, nn_bins = 0, nn_max = 0.0,
           per_replica = false)
    cavity_at(b, points; radii = [3.3], site = 0, n_cap = 32, nn_bins = 0, nn_max = 0.0, per_replica = false)

Occupancy statistics of probe spheres in one read-only pass: for each of the 1 to 8 ascending `radii`
the number n of sites (atom slot `site` = 0, 1, 2 of every molecule, C numbering; -1 = the centres of
mass) closer than it to each of `n_probe` random points per replica -- bit for bit the COMs `widom!`
draws for the same `seed` and `draw0` -- or to the caller's `points` `(3, n_probe, R)`.  Returns
`(occ_hist, occ_mom, nn_hist)`: `occ_hist` `(n_cap + 1, K)` UInt64 (points with n = 0..n_cap, the last
row n_cap or more), `occ_mom` `(2, K)` (the sums of n and n^2) and, with `nn_bins > 0`, `nn_hist`
`nn_bins + 1` counts of the distance to the nearest site in bins of `nn_max / nn_bins` (else
`nothing`); each with a trailing dimension R with `per_replica`.
"""
function cavity(b::Batch, n_probe::Integer, seed::Integer; draw0::Integer = 0, radii::Vector{Float64} = [3.3],
                site::Integer = 0, n_cap::Integer = 32, nn_bins::Integer = 0, nn_max::Float64 = 0.0,
                per_replica::Bool = false)
    occ_hist, occ_mom, nn_hist = cavity_outputs(b, radii, n_cap, nn_bins, per_replica)
    check(ccall((:mmc_batch_cavity, libmmc), Int32,
                (Ptr{Cvoid}, Int64, UInt64, Int64, Int32, Int32, Ptr{Float64}, Int32, Int32, Float64, Int32,
                 Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                b.h, n_probe, seed % UInt64, draw0, site, length(radii), radii, n_cap, nn_bins, nn_max,
                per_replica ? 1 : 0, occ_hist, occ_mom, nn_hist === nothing ? C_NULL : nn_hist,
                C_NULL, C_NULL, C_NULL, C_NULL))
    return occ_hist, occ_mom, nn_hist
end
function cavity_at(b::Batch, points::Array{Float64,3}; radii::Vector{Float64} = [3.3], site::Integer = 0,
                   n_cap::Integer = 32, nn_bins::Integer = 0, nn_max::Float64 = 0.0, per_replica::Bool = false)
    size(points, 1) == 3 && size(points, 3) == b.n_replicas || error("points are (3, n_probe, R)")
    occ_hist, occ_mom, nn_hist = cavity_outputs(b, radii, n_cap, nn_bins, per_replica)
    check(ccall((:mmc_batch_cavity_at, libmmc), Int32,
                (Ptr{Cvoid}, Int64, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Float64, Int32,
                 Ptr{UInt64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                b.h, size(points, 2), points, site, length(radii), radii, n_cap, nn_bins, nn_max,
                per_replica ? 1 : 0, occ_hist, occ_mom, nn_hist === nothing ? C_NULL : nn_hist,
                C_NULL, C_NULL, C_NULL))
    return occ_hist, occ_mom, nn_hist
end
function cavity_outputs(b::Batch, radii::Vector{Float64}, n_cap::Integer, nn_bins::Integer, per_replica::Bool)
    K = length(radii)
    1 <= K <= 8 || error("1 to 8 radii")
    1 <= n_cap <= 255 || error("n_cap must be in 1..255")
    0 <= nn_bins <= 4096 || error("nn_bins must be in 0..4096")
    tail = per_replica ? (b.n_replicas,) : ()
    return zeros(UInt64, n_cap + 1, K, tail...), zeros(UInt64, 2, K, tail...),
           nn_bins > 0 ? zeros(UInt64, nn_bins + 1, tail...) : nothing
end

# ---- virtual volume moves (include/mmc_hip.h, mmc_batch_volume_perturb) ---------------------------
"""
    volume_perturb!(b, scales, temperature, boltz_sum, n_overlap)

Virtual volume moves of every replica, read-only: for each test box `L_k = scales[k] L` (1 to 8 of
them; `kappa_k = alpha / L_k`) the change dU of potential(..., "ewald") (energy.jl:946-1032) under
the NPT move's own rescale (volumeChange.jl:62-80), `boltz_sum[k, r] += exp(-dU / T + N log(scale^3))`
and `n_overlap[k, r] +=` the weights forced to 0; both are `(K, R)` matrices (column r = row r of
the C layout).  beta P = log(mean w) / dV.
"""
function volume_perturb!(b::Batch, scales::Vector{Float64}, temperature::Float64,
                         boltz_sum::Matrix{Float64}, n_overlap::Matrix{Int64})
    K = length(scales)
    1 <= K <= 8 || error("1 to 8 scales")
    size(boltz_sum) == (K, b.n_replicas) && size(n_overlap) == (K, b.n_replicas) || error("sums are (K, R)")
    check(ccall((:mmc_batch_volume_perturb, libmmc), Int32,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                b.h, K, scales, temperature, boltz_sum, n_overlap, C_NULL, C_NULL))
    return boltz_sum, n_overlap
end

# ---- save and resume: bulk state records (include/mmc_hip.h, "Save and resume") ----
"""
    info = state_info(b)                        # the batch as it is configured now
    offsets, record_bytes = state_record_layout(info)
    records = get_state(b, r0, nr)              # Matrix{UInt8} (record_bytes, nr): column k = replica r0 + k
    set_state!(b, info, r0, records)            # into a batch of the same system, configured the same way

The records carry what the chains keep from call to call (box, temperature, centres of mass,
coordinates, S(k) in device order bit for bit, orientations), `info` the batch-level rest (the
position of the random streams among it).  `set_state!` configures nothing: bring a fresh batch into
the saved mode first (`set_coulomb_style!`, `set_boxes!`, `set_temperatures!`), then chains resume
bit for bit under the same options.  The file format of the Python side (checkpoint.py) is a prefix,
a JSON header with these fields and the raw records: `write(io, records)` gives the same bytes.
"""
function state_info(b::Batch)
    info = Ref{MMCStateInfo}()
    check(ccall((:mmc_batch_state_info, libmmc), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), b.h, info))
    return info[]
end
function state_record_layout(info::MMCStateInfo)
    offsets = Vector{Int64}(undef, 8)
    bytes = Ref{Int64}(0)
    check(ccall((:mmc_state_record_layout, libmmc), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}),
                Ref(info), offsets, bytes))
    return offsets, bytes[]
end
function get_state(b::Batch, r0::Integer, nr::Integer)
    _, bytes = state_record_layout(state_info(b))
    records = Matrix{UInt8}(undef, bytes, nr)
    check(ccall((:mmc_batch_get_state, libmmc), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                b.h, r0, nr, records))
    return records
end
function set_state!(b::Batch, info::MMCStateInfo, r0::Integer, records::Matrix{UInt8})
    _, bytes = state_record_layout(info)
    size(records, 1) == bytes || error("a record of this state has $bytes bytes")
    check(ccall((:mmc_batch_set_state, libmmc), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                b.h, Ref(info), r0, size(records, 2), records))
end

# ---- the one collective of a sharded run: RCCL behind the C ABI (include/mmc_hip.h, mmc_dist_*) ----
"""
    id = dist_unique_id()                       # rank 0; send the 128 bytes to the other ranks
    d  = dist_init(rank, world, id; device = rank)
    dist_reduce!(d, sums, maxima)               # in place over all ranks: sum / max, Float64
    dist_destroy(d)

One process per GPU; replicas shard over ranks with no data-path collective, and this is the
reduction of a block's observables (energy sums, acceptance counters; the longest elapsed time).
"""
function dist_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:mmc_dist_unique_id, libmmc), Int32, (Ptr{UInt8},), id))
    return id
end
function dist_init(rank::Integer, world::Integer, id::Vector{UInt8}; device::Integer = 0)
    length(id) == 128 || error("the unique id has 128 bytes")
    d = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mmc_dist_init, libmmc), Int32, (Int32, Int32, Ptr{UInt8}, Int32, Ptr{Ptr{Cvoid}}),
                rank, world, id, device, d))
    return d[]
end
dist_reduce!(d::Ptr{Cvoid}, sums::Vector{Float64}, maxima::Vector{Float64}) =
    check(ccall((:mmc_dist_reduce, libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                d, sums, length(sums), maxima, length(maxima)))
dist_destroy(d::Ptr{Cvoid}) = check(ccall((:mmc_dist_destroy, libmmc), Int32, (Ptr{Cvoid},), d))

"Status line of one block as Loop() prints it (main.jl:667-679) from one chain record."
function block_line(chain::MMCChain, block::Integer, n_mol::Integer, box::Float64;
                    ideal_term::Float64 = 4.60453)
    buf = Vector{UInt8}(undef, 512); c = Ref(chain)
    check(ccall((:mmc_chain_block_line, libmmc), Int32,
                (Ptr{MMCChain}, Int64, Int64, Float64, Float64, Ptr{UInt8}, Int64),
                c, block, n_mol, box, ideal_term, buf, length(buf)))
    return unsafe_string(pointer(buf))
end

end # module MMCHipCore

# =================================================================================================
# The reference's methods, redefined in the including module (Main) with their exact signatures.
# =================================================================================================

# ---- Ewald/ewalds.jl:45 ---------------------------------------------------------------------------
function PrepareEwaldVariables(ewald::EWALD, boxSize::Real where {T})
    C = MMCHipCore
    box = Float64(min(boxSize...))                       # ewalds.jl:50
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    C.check(ccall((:mmc_ctx_create, C.libmmc), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), 0, C_NULL, ctx))
    n = Ref{Int64}(0)
    st = ccall((:mmc_prepare_ewald, C.libmmc), Int32,
               (Ptr{Cvoid}, Float64, Int64, Int64, Float64, Float64, Ptr{Int64}),
               ctx[], ewald.kappa, ewald.nk, ewald.k_sq_max, box, ewald.factor, n)
    st != 0 && (ccall((:mmc_ctx_destroy, C.libmmc), Int32, (Ptr{Cvoid},), ctx[]); C.check(st))
    kxyz = Vector{SVector{3,Int32}}(undef, n[])
    cfac = Vector{Float64}(undef, n[])
    GC.@preserve kxyz cfac begin
        C.check(ccall((:mmc_get_kvectors, C.libmmc), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}),
                      ctx[], Ptr{Int32}(pointer(kxyz)), pointer(cfac)))
    end
    ccall((:mmc_ctx_destroy, C.libmmc), Int32, (Ptr{Cvoid},), ctx[])
    return EWALD(ewald.kappa, ewald.nk, ewald.k_sq_max, oftype(ewald.nk, n[]), kxyz, cfac,
                 zeros(ComplexF64, n[]), zeros(ComplexF64, n[]), ewald.factor)   # ewalds.jl:91-101
end

# ---- Ewald/energy.jl:209-210 ----------------------------------------------------------------------
function LJ_poly_ΔU(i, moa::StructArray, soa::StructArray,
                            vdwTable, r_cut, box)
    return MMCHipCore.call_lj_poly_du(MMCHipCore.session(), Int64(i), moa.COM, soa.coords, Float64(r_cut))
end

# ---- Ewald/energy.jl:126 (legacy) -----------------------------------------------------------------
function LJ_poly_ΔU(i::Int, system::Requirements)
    return MMCHipCore.call_lj_poly_du(MMCHipCore.session(), Int64(i), system.rm, system.ra, system.r_cut)
end

# ---- Ewald/ewalds.jl:293-299 ----------------------------------------------------------------------
function EwaldReal(chosenOne::Int64,
                    moa::StructArray,
                    soa::StructArray,
                    ewald::EWALD,
                    r_cut::Float64,
                    box::Float64
    )
    s = MMCHipCore.session(); MMCHipCore.bind_ewald!(s, ewald, box)
    return MMCHipCore.call_ewald_real(s, chosenOne, moa.COM, soa.coords, r_cut, 0.5)  # ovr = 0.5 (ewalds.jl:327)
end

# ---- Ewald/ewalds.jl:205-213 (legacy: ovr = 1.0, cutoff from system.r_cut) --------------------------
function EwaldReal(
    qq_r::Vector{SVector{3,Float64}},
    qq_q::Vector{Float64},
    kappa::Real,
    box::Float64,
    thisMol_thisAtom::Vector{SVector{2,Int64}},
    chosenOne::Int64,
    system::Requirements,
)
    s = MMCHipCore.session()
    MMCHipCore.bind_ewald!(s, Float64(kappa), 5, 27, factor, box)  # `factor`: constants.jl:28
    return MMCHipCore.call_ewald_real(s, chosenOne, system.rm, qq_r, system.r_cut, 1.0)  # ovr = 1.0 (ewalds.jl:240)
end

# ---- Ewald/ewalds.jl:892-899 ----------------------------------------------------------------------
function EwaldShort(
    i::Int64,
    moa::StructArray,
    soa::StructArray,
    sim_props::Properties2,
    ewald::EWALD,
    box::Float64,
)
    s = MMCHipCore.session(); MMCHipCore.bind_ewald!(s, ewald, box)
    return MMCHipCore.call_ewald_short(s, i, moa.COM, soa.coords, sim_props.qq_rcut)
end

# ---- Ewald/ewalds.jl:848-856 (legacy) -------------------------------------------------------------
function EwaldShort(
    i::Int64,
    system::Requirements,
    ewald::EWALD,
    box::Float64,
    qq_r::Vector{SVector{3,Float64}},
    qq_q::Vector{Float64},
    tinfoil = false,
)
    realEwald, overlap = EwaldReal(qq_r, qq_q, ewald.kappa, box, system.thisMol_theseAtoms, i, system)
    realEwald *= ewald.factor                                      # ewalds.jl:870
    return realEwald, realEwald / 3, overlap                       # :871-872, :887
end

# ---- Ewald/ewalds.jl:538-543 ----------------------------------------------------------------------
function RecipLong(
    ewald::EWALD,
    r::Vector{SVector{3,Float64}},
    qq_q::Vector{Float64},
    box::Float64
)
    s = MMCHipCore.session(); MMCHipCore.bind_ewald!(s, ewald, box)
    MMCHipCore.sync_all!(s, nothing, r)        # every atom matters here: re-send `r` (COM = NULL)
    return MMCHipCore.recip_long(s, ewald), ewald
end

# ---- Ewald/ewalds.jl:465-470 (legacy: the box is system.box, :478) ---------------------------------
function RecipLong(
    system::Requirements,
    ewald::EWALD,
    r::Vector{SVector{3,Float64}},
    qq_q::Vector{Float64},
)
    s = MMCHipCore.session(); MMCHipCore.bind_ewald!(s, ewald, system.box)
    MMCHipCore.sync_all!(s, nothing, r)
    return MMCHipCore.recip_long(s, ewald), ewald
end

# ---- Ewald/ewalds.jl:718-724 ----------------------------------------------------------------------
function RecipMove(
    box::Float64,
    ewalds::EWALD,
    r_old::Vector,
    r_new::Vector,
    qq_q::Vector,
)
    C = MMCHipCore
    s = C.session(); C.bind_ewald!(s, ewalds, box)
    ro = Vector{SVector{3,Float64}}(r_old); rn = Vector{SVector{3,Float64}}(r_new)
    q = Vector{Float64}(qq_q)
    so, sn = ewalds.sumQExpOld, ewalds.sumQExpNew   # as they are NOW: Loop rebinds them (main.jl:621,628)
    de = Ref{Float64}(0.0)
    GC.@preserve ro rn q so sn begin
        C.check(ccall((:mmc_call_recip_move, C.libmmc), Int32,
                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                       Ptr{Float64}, Ptr{Float64}),
                      s.ctx, C.fptr(ro), C.fptr(rn), pointer(q), length(q), C.fptr(so), C.fptr(sn), de))
    end
    return de[], ewalds                         # sumQExpNew was updated in place (:805-814)
end

# ---- Ewald/ewalds.jl:829 --------------------------------------------------------------------------
function EwaldSelf(ewald::EWALD, qq_q::Vector)
    s = MMCHipCore.session()
    e = Ref{Float64}(0.0)
    MMCHipCore.check(ccall((:mmc_ewald_self, MMCHipCore.libmmc), Int32, (Ptr{Cvoid}, Ptr{Float64}),
                           s.ctx, e))
    return e[]
end

# ---- Ewald/energy.jl:618-624 (bare Coulomb, legacy API only) ---------------------------------------
function CoulombReal(
    qq_r::Vector{SVector{3,Float64}},
    qq_q::Vector{Float64},
    box::Float64,
    chosenOne::Int64,
    system::Requirements
)
    C = MMCHipCore
    s = C.session(); C.sync_all!(s, system.rm, qq_r)
    pot = Ref{Float64}(0.0); ov = Ref{Int32}(0)
    # `@assert r_cut == 10.0` (energy.jl:648) comes back as status 2 -> AssertionError
    C.check(ccall((:mmc_coulomb_real, C.libmmc), Int32,
                  (Ptr{Cvoid}, Int64, Float64, Ptr{Float64}, Ptr{Int32}),
                  s.ctx, chosenOne, system.r_cut, pot, ov))
    return pot[], ov[] != 0
end

# ---- Ewald/energy.jl:946-954 ----------------------------------------------------------------------
function potential(
    moa::StructArray,
    soa::StructArray,
    tot::Properties,
    ewalds::EWALD,
    vdwTable::Tables,
    sim_props::Properties2,
    coulomb_style::String #triggers wolf summations using double strings
)
    C = MMCHipCore
    s = C.session(); C.bind_ewald!(s, ewalds, sim_props.box); C.sync_all!(s, moa.COM, soa.coords)
    t = C.totals(s, :ewald, sim_props.LJ_rcut, sim_props.qq_rcut)
    C.pull_s!(s, ewalds; old = true)           # RecipLong inside wrote both arrays (energy.jl:1008)
    # the reference adds onto `tot` and halves what it holds after the LJ loop (energy.jl:964-969)
    tot.energy = tot.energy / 2 + t.energy; tot.virial = tot.virial / 2 + t.virial
    tot.coulomb += t.coulomb
    return tot
end

# ---- Ewald/energy.jl:864-871 (Wolf) ---------------------------------------------------------------
function potential(
    moa::StructArray,
    soa::StructArray,
    tot::Properties,
    ewald::EWALD,
    vdwTable::Tables,
    sim_props::Properties2#triggers wolf summations using double strings
)
    C = MMCHipCore
    s = C.session(); C.bind_ewald!(s, ewald, sim_props.box); C.sync_all!(s, moa.COM, soa.coords)
    t = C.totals(s, :wolf, sim_props.LJ_rcut, sim_props.qq_rcut)
    tot.energy = tot.energy / 2 + t.energy; tot.virial = tot.virial / 2 + t.virial   # energy.jl:882-887
    tot.coulomb += t.coulomb
    return tot
end
