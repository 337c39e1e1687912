"""Per-kernel comparison of two `hipcc -S --cuda-device-only` outputs of one translation unit (tests/test_abi_cpu.py has
the command line): is a kernel's body -- label to s_endpgm, the __hip_cuid_ symbol aside -- byte-equal, and what do the
two builds' metadata say about registers, spills, LDS and the waves per SIMD that follow from them.
    python tools/kernel_asm_table.py PARENT.s BRANCH.s [--csv FILE] [--loop SUBSTRING ...]
A kernel is matched by its demangled name, and its body is compared with the symbol and the function's number in the
local labels (BB<n>_) and the comments taken out, so that kernels added to the unit do not make every later body differ.  --drop-last ARG:
a branch kernel `name<.., ARG>` that the parent lacks is compared with the parent's `name<..>` (a template parameter added
with ARG as the value that keeps the old kernel); branch kernels without a parent kernel are listed with empty parent columns.
--loop: for the kernels whose demangled name contains SUBSTRING, also count the instructions of the steady-state stage
loop of the fused item scan: the innermost loop that holds both MFMAs and a barrier, from its head to its last s_barrier.
Exit status 1 when a kernel that is not byte-equal loses waves per SIMD, spills, or differs in LDS (or a --loop grows)."""
import argparse
import csv
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def kernels(path):
    """{symbol: (body, {field: int})}"""
    text = open(path).read()
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", text)
    meta, cur = {}, None
    for line in text.splitlines():
        if re.match(r"\s+- \.agpr_count:", line):
            cur = {}
        if cur is not None:
            f = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", line)
            if f:
                cur[f.group(1)] = f.group(2)
                if f.group(1) == "wavefront_size":
                    meta[cur["name"]] = {k: int(cur[k]) for k in FIELDS}
                    cur = None
    out = {}
    for sym, m in meta.items():
        at = re.search(r"^" + re.escape(sym) + r":", text, re.M).start()
        body = text[at:text.index("s_endpgm", at)].replace(sym, "KERNEL")
        out[demangle(sym)] = (re.sub(r"[ \t]*;.*", "", re.sub(r"BB\d+_", "BB_", body)), m)
    return out


def demangle(sym):
    """name<template arguments> of a kernel symbol (integer, bool, float and double arguments: all this unit has)"""
    m = re.match(r"_Z(\d+)", sym)
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while not rest.startswith("E"):
            lit = re.match(r"L([ib])(n?\d+)E", rest)
            if lit:
                args.append(lit.group(2).replace("n", "-") if lit.group(1) == "i" else ("false", "true")[int(lit.group(2))])
                rest = rest[lit.end():]
            else:
                args.append({"f": "float", "d": "double"}[rest[0]])
                rest = rest[1:]
    return name + ("<" + ", ".join(args) + ">" if args else "")


def waves(m):
    return min(8, 512 // ((m["vgpr_count"] + m["agpr_count"] + 7) // 8 * 8))


def instructions(lines):
    return [l for l in lines if re.match(r"\s+[a-z]\w+", l) and not l.lstrip().startswith((";", "."))]


def stage_loop(body):
    """instruction count of the innermost loop with MFMAs and a barrier, head label .. last s_barrier"""
    lines = body.splitlines()
    label = {m.group(1): n for n, l in enumerate(lines) if (m := re.match(r"(\.LBB\w+):", l))}
    best = None
    for n, l in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+ (\.LBB\w+)", l) or re.match(r"\s+s_branch (\.LBB\w+)", l)
        if m and label.get(m.group(1), n) < n:
            span = lines[label[m.group(1)]:n + 1]
            if any("v_mfma" in s for s in span) and any("s_barrier" in s for s in span) and (best is None or len(span) < len(best)):
                best = span
    if best is None:
        return -1
    last = max(n for n, s in enumerate(best) if "s_barrier" in s)
    return len(instructions(best[:last + 1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--csv")
    ap.add_argument("--loop", action="append", default=[])
    ap.add_argument("--drop-last")
    args = ap.parse_args()
    a, b = kernels(args.parent), kernels(args.branch)
    twin = {}
    for name in b:
        old = name
        if name not in a and args.drop_last and name.endswith(", " + args.drop_last + ">"):
            old = name[:-len(", " + args.drop_last + ">")] + ">"
        if old in a:
            twin[name] = old
    assert set(twin.values()) == set(a), sorted(set(a) - set(twin.values()))
    rows, bad, equal = [], [], 0
    for name in sorted(b):
        bb, mb = b[name]
        if name not in twin:   # new in the branch
            row = {"kernel": name, "body_equal": "", "waves_parent": "", "waves_branch": waves(mb)}
            for f in FIELDS:
                row[f + "_parent"], row[f + "_branch"] = "", mb[f]
            row["instructions_parent"], row["instructions_branch"] = "", len(instructions(bb.splitlines()))
            row["stage_loop_parent"], row["stage_loop_branch"] = "", stage_loop(bb) if any(s in name for s in args.loop) else ""
            if mb["vgpr_spill_count"] or mb["private_segment_fixed_size"]:
                bad.append((name, "spill / scratch", mb["vgpr_spill_count"], mb["private_segment_fixed_size"]))
            print(f"new: {name}: vgpr {mb['vgpr_count']}, sgpr spills {mb['sgpr_spill_count']}, waves {waves(mb)}, "
                  f"instructions {row['instructions_branch']}, stage loop {row['stage_loop_branch']}")
            rows.append(row)
            continue
        ba, ma = a[twin[name]]
        same = ba == bb
        equal += same
        row = {"kernel": name, "body_equal": int(same), "waves_parent": waves(ma), "waves_branch": waves(mb)}
        for f in FIELDS:
            row[f + "_parent"], row[f + "_branch"] = ma[f], mb[f]
        row["instructions_parent"], row["instructions_branch"] = len(instructions(ba.splitlines())), len(instructions(bb.splitlines()))
        row["stage_loop_parent"] = row["stage_loop_branch"] = ""
        if any(s in name for s in args.loop):
            row["stage_loop_parent"], row["stage_loop_branch"] = stage_loop(ba), stage_loop(bb)
            if row["stage_loop_branch"] > row["stage_loop_parent"] or row["stage_loop_branch"] < 0:
                bad.append((name, "stage loop", row["stage_loop_parent"], row["stage_loop_branch"]))
        if not same:
            if waves(mb) != waves(ma):
                bad.append((name, "waves per SIMD", waves(ma), waves(mb)))
            if mb["vgpr_spill_count"] or mb["private_segment_fixed_size"]:
                bad.append((name, "spill / scratch", mb["vgpr_spill_count"], mb["private_segment_fixed_size"]))
            if mb["sgpr_spill_count"] > ma["sgpr_spill_count"]:
                bad.append((name, "sgpr spills", ma["sgpr_spill_count"], mb["sgpr_spill_count"]))
            if mb["group_segment_fixed_size"] != ma["group_segment_fixed_size"]:
                bad.append((name, "LDS", ma["group_segment_fixed_size"], mb["group_segment_fixed_size"]))
            print(f"differs: {name}: vgpr {ma['vgpr_count']} -> {mb['vgpr_count']}, sgpr spills {ma['sgpr_spill_count']} -> "
                  f"{mb['sgpr_spill_count']}, waves {waves(ma)} -> {waves(mb)}, instructions {row['instructions_parent']} -> "
                  f"{row['instructions_branch']}, stage loop {row['stage_loop_parent']} -> {row['stage_loop_branch']}")
        rows.append(row)
    print(f"{equal} of {len(twin)} kernel bodies byte-equal, {len(rows) - len(twin)} new kernels")
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)
    for x in bad:
        print("FAIL", *x)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
