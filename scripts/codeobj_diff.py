#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmmc_hip.so, kernel by kernel.

    scripts/codeobj_diff.py BASE.so NEW.so [--json OUT]

For every kernel symbol: .vgpr_count, .sgpr_count, .private_segment_fixed_size and
.group_segment_fixed_size from the code object's metadata note, and the size of the symbol's
.text.  A kernel of BASE is looked up in NEW by its demangled name; where a function template has
gained trailing parameters with defaults, or a kernel a trailing argument, the BASE name is matched with those appended
(RENAMES below: the only difference is the mangled name).  Prints every kernel of BASE that
differs or is missing, lists the kernels only NEW has, and exits 1 if a BASE kernel differs.

Needs llvm-objcopy, clang-offload-bundler and llvm-readelf (ROCm's LLVM; $LLVM_BIN).
"""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")

# BASE demangled name (regex) -> NEW demangled name: template parameters added with a default
RENAMES = [
    # k_move_eval_wave<SUBST, IMG, MULTI> gained WOLF = false
    (re.compile(r"^void k_move_eval_wave<(\w+), (\w+), (\w+)>\("), r"void k_move_eval_wave<\1, \2, \3, false>("),
    # ... and then LADDER = false
    (re.compile(r"^void k_move_eval_wave<(\w+), (\w+), (\w+), (\w+)>\("),
     r"void k_move_eval_wave<\1, \2, \3, \4, false>("),
    # k_move_eval_fast<PerBox...> gained a leading WOLF (false for every form that existed)
    (re.compile(r"^void k_move_eval_fast<>\("), r"void k_move_eval_fast<false>("),
    (re.compile(r"^void k_move_eval_fast<(?!false|true)([^>]+)>\("), r"void k_move_eval_fast<false, \1>("),
    # k_move_eval_wave and k_settle_rec gained a trailing CandView argument (the candidate lists, mmc_cand.hpp)
    (re.compile(r"^(void k_move_eval_wave<\w+, \w+, \w+, \w+, \w+>\(.*unsigned int\*, unsigned int)\)$"), r"\1, CandView)"),
    (re.compile(r"^(k_settle_rec\(.*int, int)\)$"), r"\1, CandView)"),
    # k_move_eval became a template <bool WOLF = false>
    (re.compile(r"^k_move_eval\("), r"void k_move_eval<false>("),
]


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def kernels(lib):
    """{demangled kernel name: {key: value, 'text_size': n}} of the gfx950 code object in `lib`."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "co.elf")
        tool("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "rest"))
        tool("clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}",
             "--unbundle")
        notes = tool("llvm-readelf", "--notes", co)
        syms = tool("llvm-readelf", "--symbols", "--wide", co)
        syms_dem = tool("llvm-readelf", "--symbols", "--wide", "--demangle", co)
    size, demangled = {}, {}
    for line, dline in zip(syms.splitlines(), syms_dem.splitlines()):  # the same rows, names demangled
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
            demangled[f[7]] = dline.split(None, 7)[7]
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'\"")
        if k in (".agpr_count", ".args") and line.lstrip().startswith("- "):
            cur = {}                      # first key of a kernel's record
        if cur is None:
            continue
        if k == ".name":
            cur["name"] = v
        elif k == ".symbol":
            cur["symbol"] = v
        elif k in KEYS:
            cur[k] = int(v)
        if k == ".wavefront_size":        # last key of a kernel's record (keys are sorted)
            if "name" in cur:
                cur["text_size"] = size.get(cur["name"], -1)
                out[cur["name"]] = cur
            cur = None
    return {demangled.get(n, n): {k: v for k, v in rec.items() if k not in ("name", "symbol")}
            for n, rec in out.items()}


def renamed(name):
    for rx, to in RENAMES:
        if rx.search(name):
            return rx.sub(to, name, count=1)
    return name


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    base, new = kernels(argv[1]), kernels(argv[2])
    matched, diffs, missing = {}, [], []
    for name, rec in sorted(base.items()):
        to = name if name in new else renamed(name)
        if to not in new:
            missing.append(name)
            continue
        matched[to] = name
        if new[to] != rec:
            diffs.append((name, rec, new[to]))
    added = sorted(n for n in new if n not in matched)
    print(f"{len(base)} kernels in BASE, {len(new)} in NEW, {len(matched)} matched "
          f"({sum(1 for a, b in matched.items() if a != b)} under a new template signature)")
    for name, a, b in diffs:
        print("DIFFERS", name)
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                print(f"    {k}: {a.get(k)} -> {b.get(k)}")
    for name in missing:
        print("MISSING in NEW", name)
    print(f"{len(added)} kernels only in NEW:")
    for name in added:
        r = new[name]
        print(f"    {name.split('(')[0]}  vgpr {r.get('.vgpr_count')} sgpr {r.get('.sgpr_count')} "
              f"scratch {r.get('.private_segment_fixed_size')} lds {r.get('.group_segment_fixed_size')} "
              f"text {r.get('text_size')}")
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            json.dump({"base_kernels": len(base), "new_kernels": len(new), "matched": len(matched),
                       "differs": [{"kernel": n, "base": a, "new": b} for n, a, b in diffs],
                       "missing": missing,
                       "only_in_new": {n: new[n] for n in added}}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if diffs or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
