#!/usr/bin/env python3
"""Per-kernel resource table of two `hipcc -S --cuda-device-only` outputs of one source (before / after a change; no GPU needed).

    python tools/static_diff.py before.s after.s [--md out.md] [--all]

Reads the kernel descriptors only (next_free_vgpr, next_free_sgpr, private_segment_fixed_size, group_segment_fixed_size) and counts the
instructions of every kernel body.  Kernels are matched by demangled name; a kernel that lost ONE template argument is matched to the
old instantiation whose remaining arguments agree.  Exit status 1 if a kernel crosses an occupancy step (512 VGPRs per SIMD lane, in
granules of 8, at most 8 waves), gains scratch, or changes its static LDS -- or if the sets of kernels do not match.
"""
import argparse
import re
import subprocess
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels_of(path):
    """{demangled name: {'vgpr', 'sgpr', 'scratch', 'lds', 'insts'}}"""
    text = open(path).read().split("\n")
    desc, cur = {}, None
    for ln in text:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            cur = s.split()[1]
            desc[cur] = {}
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None:
            m = re.match(r"^\.amdhsa_(\w+)\s+(\d+)", s)
            if m and m.group(1) in FIELDS:
                desc[cur][m.group(1)] = int(m.group(2))
    insts, cur = {}, None
    for ln in text:
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in desc:
            cur = m.group(1)
            insts[cur] = 0
            continue
        if cur is None:
            continue
        s = ln.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
            insts[cur] += 1
    symbols = sorted(desc)
    names = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, name in zip(symbols, names):
        name = name.replace("(anonymous namespace)::", "").replace("void ", "", 1)
        d = desc[sym]
        out[short(name)] = {"vgpr": d["next_free_vgpr"], "sgpr": d["next_free_sgpr"], "scratch": d["private_segment_fixed_size"],
                            "lds": d["group_segment_fixed_size"], "insts": insts.get(sym, 0)}
    return out


def short(name):
    """kernel<template arguments> without the parameter list"""
    depth = 0
    for i, c in enumerate(name):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return name[:i]
    return name


def template_args(name):
    if "<" not in name:
        return name, []
    head, rest = name.split("<", 1)
    rest = rest[: rest.rindex(">")]
    args, depth, cur = [], 0, ""
    for c in rest:
        if c == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
            continue
        depth += c == "<"
        depth -= c == ">"
        cur += c
    args.append(cur.strip())
    return head, args


def match(old, new):
    """[(old name, new name)], unmatched old, unmatched new"""
    pairs = [(n, n) for n in old if n in new]
    left_old = [n for n in old if n not in new]
    left_new = set(n for n in new if n not in old)
    for n in list(left_old):
        head, args = template_args(n)
        hits = set()
        for i in range(len(args)):
            cand = head + "<" + ", ".join(args[:i] + args[i + 1:]) + ">"
            if cand in left_new:
                hits.add(cand)
        if len(hits) == 1:
            pairs.append((n, hits.pop()))
            left_old.remove(n)
            left_new.discard(pairs[-1][1])
    return pairs, left_old, sorted(left_new)


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--md", help="write the table here as markdown")
    ap.add_argument("--all", action="store_true", help="list the unchanged kernels too")
    a = ap.parse_args()
    old, new = kernels_of(a.before), kernels_of(a.after)
    pairs, lost, gained = match(old, new)
    rows, bad, changed = [], [], 0
    for o, n in sorted(pairs, key=lambda p: p[1]):
        x, y = old[o], new[n]
        same = x == y
        changed += not same
        why = []
        if waves(x["vgpr"]) != waves(y["vgpr"]):
            why.append("occupancy step")
        if y["scratch"] > x["scratch"]:
            why.append("scratch")
        if y["lds"] != x["lds"]:
            why.append("static LDS")
        if why:
            bad.append((n, why))
        if a.all or not same:
            pct = 100.0 * (y["insts"] - x["insts"]) / max(x["insts"], 1)
            rows.append(f"| `{n}` | {x['vgpr']} -> {y['vgpr']} | {waves(x['vgpr'])} -> {waves(y['vgpr'])} | {x['sgpr']} -> {y['sgpr']} | "
                        f"{x['scratch']} -> {y['scratch']} | {x['lds']} -> {y['lds']} | {x['insts']} -> {y['insts']} | {pct:+.1f} % |"
                        + (" " + ", ".join(why) if why else ""))
    head = [f"{len(old)} kernels before, {len(new)} after; {len(pairs)} matched, {changed} of them differ in a figure below.",
            f"Unmatched before: {lost or 'none'}.  Unmatched after: {gained or 'none'}.",
            f"Violations (occupancy step, new scratch, static LDS): {bad or 'none'}.", "",
            "| kernel | VGPRs | waves / SIMD | SGPRs | scratch bytes | static LDS bytes | instructions | change |",
            "|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n"
    if a.md:
        open(a.md, "w").write(text)
    print(text)
    return 1 if bad or lost or gained else 0


if __name__ == "__main__":
    sys.exit(main())
