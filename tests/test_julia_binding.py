"""The Julia binding (metropolismontecarlo_amd/julia/MMCHip.jl) cannot be executed here: the
image has no `julia`.  What can be checked by text is the property that makes it take effect --
every hot-path method of the reference is redefined at TOP LEVEL (outside any module, so in the
module that includes the file: Main) with exactly the reference's type signature, so that Julia
overwrites the CPU method instead of adding a less specific one beside it.

The expected signatures below are the reference's, normalised (whitespace and comments removed);
each cites where it stands in the reference's Ewald/ directory."""
import hashlib
import json
import os
import re

from boundary import ccall_mismatches, header_code, header_text, julia_ccalls, julia_text

HERE = os.path.dirname(os.path.abspath(__file__))

SIGNATURES = {
    # current moa / soa API
    "energy.jl:209-210": "LJ_poly_ΔU(i,moa::StructArray,soa::StructArray,vdwTable,r_cut,box)",
    "ewalds.jl:293-299": "EwaldReal(chosenOne::Int64,moa::StructArray,soa::StructArray,ewald::EWALD,"
                         "r_cut::Float64,box::Float64)",
    "ewalds.jl:892-899": "EwaldShort(i::Int64,moa::StructArray,soa::StructArray,sim_props::Properties2,"
                         "ewald::EWALD,box::Float64,)",
    "ewalds.jl:45": "PrepareEwaldVariables(ewald::EWALD,boxSize::Realwhere{T})",
    "ewalds.jl:538-543": "RecipLong(ewald::EWALD,r::Vector{SVector{3,Float64}},qq_q::Vector{Float64},"
                         "box::Float64)",
    "ewalds.jl:718-724": "RecipMove(box::Float64,ewalds::EWALD,r_old::Vector,r_new::Vector,qq_q::Vector,)",
    "ewalds.jl:829": "EwaldSelf(ewald::EWALD,qq_q::Vector)",
    "energy.jl:946-954": "potential(moa::StructArray,soa::StructArray,tot::Properties,ewalds::EWALD,"
                         "vdwTable::Tables,sim_props::Properties2,coulomb_style::String)",
    "energy.jl:864-871": "potential(moa::StructArray,soa::StructArray,tot::Properties,ewald::EWALD,"
                         "vdwTable::Tables,sim_props::Properties2)",
    # legacy Requirements API
    "energy.jl:126": "LJ_poly_ΔU(i::Int,system::Requirements)",
    "ewalds.jl:205-213": "EwaldReal(qq_r::Vector{SVector{3,Float64}},qq_q::Vector{Float64},kappa::Real,"
                         "box::Float64,thisMol_thisAtom::Vector{SVector{2,Int64}},chosenOne::Int64,"
                         "system::Requirements,)",
    "ewalds.jl:848-856": "EwaldShort(i::Int64,system::Requirements,ewald::EWALD,box::Float64,"
                         "qq_r::Vector{SVector{3,Float64}},qq_q::Vector{Float64},tinfoil=false,)",
    "ewalds.jl:465-470": "RecipLong(system::Requirements,ewald::EWALD,r::Vector{SVector{3,Float64}},"
                         "qq_q::Vector{Float64},)",
    "energy.jl:618-624": "CoulombReal(qq_r::Vector{SVector{3,Float64}},qq_q::Vector{Float64},box::Float64,"
                         "chosenOne::Int64,system::Requirements)",
}


def top_level_signatures(text):
    """`function name(args)` headers that are not nested inside a `module ... end` block,
    normalised like SIGNATURES."""
    # drop the core module (its body is indented code between `module MMCHipCore` and its `end`)
    text = re.sub(r"(?ms)^module MMCHipCore\b.*?^end # module MMCHipCore\s*$", "", text)
    assert "module " not in re.sub(r"(?m)^\s*#.*$", "", text), "methods must not live in a module"
    out = []
    for m in re.finditer(r"(?ms)^function\s+(\S+?)\((.*?)\n?\s*\)\s*$", text):
        args = re.sub(r"#[^\n]*", "", m.group(2))          # the reference's trailing comments
        out.append(re.sub(r"\s+", "", f"{m.group(1)}({args})"))
    return out


def test_every_reference_method_is_overwritten_with_its_exact_signature():
    got = top_level_signatures(julia_text())
    assert len(got) == len(set(got)), "a signature is defined twice"
    want = {re.sub(r"\s+", "", v): k for k, v in SIGNATURES.items()}
    missing = [f"{want[w]}: {w}" for w in want if w not in got]
    assert not missing, "not redefined with the reference's signature:\n" + "\n".join(missing)
    extra = [g for g in got if g not in want]
    assert not extra, f"top-level methods the reference does not have: {extra}"


def test_signatures_are_the_references_own():
    """The expected signatures above are compared with the reference's source text itself:
    tests/golden/reference_signatures.json holds the SHA-256 of the reference's header at every
    cited location, comments and whitespace removed (written by tests/golden/make_fixtures.py)."""
    with open(os.path.join(HERE, "golden", "reference_signatures.json"), encoding="utf-8") as fh:
        digests = json.load(fh)
    assert set(digests) == set(SIGNATURES), "the fixture and SIGNATURES cite different locations"
    for where, sig in SIGNATURES.items():
        norm = "function" + re.sub(r"\s+", "", sig)
        assert hashlib.sha256(norm.encode("utf-8")).hexdigest() == digests[where], (where, sig)


def test_binding_says_how_it_takes_effect_and_that_it_was_not_run():
    text = julia_text()
    assert "include" in text and "AFTER" in text and "overwrites" in text
    assert "NOT RUN" in text and "no `julia`" in text
    integ = open(os.path.join(os.path.dirname(HERE), "INTEGRATION.md"), encoding="utf-8").read()
    assert "using .MMCHip" not in integ                     # the recipe that silently did nothing
    assert "MMCHipCore.attach!" in integ and "has not been run" in integ


# ---- every ccall against the prototypes of include/mmc_hip.h (boundary.ccall_mismatches) ----------------
C_STRUCT_OF = {"MMCTotals": "mmc_totals", "MMCMove": "mmc_move", "MMCMoveResult": "mmc_move_result",
               "MMCRunParams": "mmc_run_params", "MMCRunStats": "mmc_run_stats", "MMCChain": "mmc_chain",
               "MMCNptParams": "mmc_npt_params", "MMCNptStats": "mmc_npt_stats"}
FIELD_C2J = {"double": "Float64", "int32_t": "Int32", "int64_t": "Int64", "uint64_t": "UInt64",
             "uint32_t": "UInt32"}
SIZEOF = {"Float64": 8, "Int64": 8, "UInt64": 8, "Int32": 4, "UInt32": 4}


def test_every_ccall_matches_its_prototype():
    text = julia_text()
    calls = julia_ccalls(text)
    assert len(calls) >= 35
    assert not ccall_mismatches(text), "\n".join(ccall_mismatches(text))
    bound = {c[0] for c in calls}
    # the replica batch and the fused move are bound, not only the per-call surface
    for sym in ("mmc_batch_create", "mmc_batch_destroy", "mmc_batch_eval", "mmc_batch_settle",
                "mmc_batch_run", "mmc_batch_run_chains", "mmc_batch_potential_ewald",
                "mmc_batch_recip_long", "mmc_batch_set_option", "mmc_batch_get_replica",
                "mmc_batch_volume_trial", "mmc_batch_volume_accept", "mmc_batch_volume_reject",
                "mmc_batch_run_npt",
                "mmc_trial_move", "mmc_accept_move", "mmc_reject_move", "mmc_call_lj_poly_du",
                "mmc_call_ewald_short", "mmc_call_ewald_real", "mmc_call_recip_move"):
        assert sym in bound, f"{sym} is not bound in MMCHip.jl"


def test_the_checker_catches_abi_slips():
    text = julia_text()
    good = ("(Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, "
            "Ptr{Int32})")
    assert text.count(good) == 1                        # mmc_call_ewald_short
    swapped = text.replace(good, "(Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Float64}, "
                                 "Ptr{Float64}, Ptr{Float64}, Ptr{Int32})")
    bad = ccall_mismatches(swapped)
    assert any("mmc_call_ewald_short: parameter 4" in b for b in bad), bad
    short = text.replace(good, "(Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, "
                               "Ptr{Float64}, Ptr{Int32})")
    assert any("mmc_call_ewald_short: 8 parameters in the header, 7" in b
               for b in ccall_mismatches(short))
    renamed = text.replace(":mmc_batch_settle", ":mmc_batch_setle")
    assert any("mmc_batch_setle: not declared" in b for b in ccall_mismatches(renamed))
    # ... and a header that changes under the binding
    hdr = header_text().replace("int32_t mmc_batch_settle(mmc_batch *b, const int32_t *accept);",
                                      "int32_t mmc_batch_settle(mmc_batch *b, const int64_t *accept);")
    assert any("mmc_batch_settle: parameter 2" in b for b in ccall_mismatches(text, hdr))


def _c_structs():
    src = header_code()
    out = {}
    for m in re.finditer(r"typedef struct \{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                n = n.strip()
                arr = re.match(r"(\w+)\[(\d+)\]", n)
                fields.append((arr.group(1), ctype, int(arr.group(2))) if arr else (n, ctype, 1))
        out[m.group(2)] = fields
    return out


def _julia_structs(text):
    out = {}
    for m in re.finditer(r"(?ms)^struct (\w+)\n(.*?)^end", text):
        fields = []
        for decl in re.split(r"[;\n]", re.sub(r"#[^\n]*", "", m.group(2))):
            decl = decl.strip()
            if not decl:
                continue
            name, jt = decl.split("::")
            tup = re.match(r"NTuple\{(\d+),\s*(\w+)\}", jt)
            fields.append((name, tup.group(2), int(tup.group(1))) if tup else (name, jt, 1))
        out[m.group(1)] = fields
    return out


def _layout(fields):
    """Offsets of bits-type fields under natural alignment (C and Julia agree on this rule)."""
    off, offs, align = 0, {}, 1
    for name, jt, n in fields:
        sz = SIZEOF[jt]
        off = (off + sz - 1) // sz * sz
        offs[name] = off
        off += sz * n
        align = max(align, sz)
    return offs, (off + align - 1) // align * align


def test_julia_structs_mirror_the_header_and_the_ctypes_mirrors():
    import ctypes as C
    from metropolismontecarlo_amd import _lib
    cs, js = _c_structs(), _julia_structs(julia_text())
    for jname, cname in C_STRUCT_OF.items():
        assert jname in js, f"struct {jname} missing in MMCHip.jl"
        want = [(n, FIELD_C2J[t], k) for n, t, k in cs[cname]]
        assert js[jname] == want, f"{jname} differs from {cname}:\n{js[jname]}\n{want}"
    # sizes and a few offsets against the structures test_abi.py checks against gcc's layout
    for jname, ct in (("MMCTotals", _lib.Totals), ("MMCMove", _lib.Move),
                      ("MMCMoveResult", _lib.MoveResult), ("MMCRunParams", _lib.RunParams),
                      ("MMCRunStats", _lib.RunStats), ("MMCNptParams", _lib.NptParams),
                      ("MMCNptStats", _lib.NptStats)):
        offs, size = _layout(js[jname])
        assert size == C.sizeof(ct), jname
        for fname, _ in ct._fields_:
            assert offs[fname] == getattr(ct, fname).offset, (jname, fname)
    offs, size = _layout(js["MMCChain"])
    assert size == _lib.CHAIN_DTYPE.itemsize == 144
    for fname in _lib.CHAIN_DTYPE.names:
        assert offs[fname] == _lib.CHAIN_DTYPE.fields[fname][1], fname
