#!/usr/bin/env python3
"""Exact counterfactual regret minimisation on an enumerated tree: the NashConv curves CFR, CFR+, linear CFR and DCFR reach
(learn/tabular.py TabularCFR, csrc/cfr.hip) -- no sampled games, no net; all variants in lockstep, one sweep pair per iteration.

    python tools/tabular_cfr.py --tree TREE.tar --variants cfr cfr+ linear --iterations 1000 --every 50 [--against RUN_DIR ...]

TREE.tar is a tree file as Tree.save writes it.  A variant is cfr, cfr+, linear or dcfr:ALPHA:BETA:GAMMA.  Prints one JSON line per
variant: variant, alternating, iterations (the recorded ones), average_nashconv and nashconv (of the average and of the current policy
at those iterations).  With --against, every RUN_DIR (learn/checkpoint.RunStore) enters with the target net of its latest checkpoint and
the line also carries names and payoff: util.metric.cross_play of the final average policy (player 0) against those nets.

    python tools/tabular_cfr.py --bench [--runs 30] [--out profiles/cfr.md]

times one rnad_cfr_iterate at n = 1, 8, 32 on the BASELINE.json configs[1] tree and on the configs[3]-shaped native tree: the median of
`runs` warm calls after 10, one device event pair around each, next to rnad_reg_evaluate on the same tree and n in the same process; then
runs 1000 CFR+ iterations on the configs[1] tree next to TabularRNaD's 32 updates at eta = 0.2, and writes the report with the kernels'
resource use as the built library records it.  Needs the GPU.
"""
import argparse
import importlib.util
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "r-nad_amd"))
import torch  # noqa: E402

import rnad_hip  # noqa: E402
from environment.tree import Tree  # noqa: E402
from learn import tabular  # noqa: E402
from util import metric  # noqa: E402


def _cross_play_tool():
    spec = importlib.util.spec_from_file_location("cross_play_tool", os.path.join(ROOT, "tools", "cross_play.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def parse_variant(text):
    if text.startswith("dcfr:"):
        parts = text.split(":")
        if len(parts) != 4:
            raise SystemExit(f"--variants: {text!r}: expected dcfr:ALPHA:BETA:GAMMA")
        return ("dcfr",) + tuple(float(p) for p in parts[1:])
    return text


def median_ms(fn, runs, warm=10):
    """Median ms of `runs` warm calls of fn after `warm` calls, one device event pair per call."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def kernel_resources():
    """[(kernel, A, vgpr, sgpr, lds, scratch)] of the k_cfr_* kernels from the built library's metadata (rnad_hip.kernel_notes); None
    where the ROCm LLVM tools are not installed."""
    notes = rnad_hip.kernel_notes("k_cfr_update")
    if notes is None:
        return None
    out = []
    for k in notes:
        m = re.search(r"k_cfr_(reach|update)ILi(\d+)EE", k.get(".name", ""))
        if m:
            out.append((m.group(1), int(m.group(2)), int(k[".vgpr_count"]), int(k[".sgpr_count"]), int(k.get(".group_segment_fixed_size", 0)),
                        int(k[".private_segment_fixed_size"])))
    return sorted(out)


def first_below(iterations, curve, level):
    """The first recorded iteration whose NashConv is at or below `level`, or None."""
    return next((t for t, v in zip(iterations, curve) if v <= level), None)


def bench(runs, out_path, device, ns=(1, 8, 32), eta=0.2, iterations=1000, every=10, updates=32):
    tool = _cross_play_tool()
    rows, curves = [], None
    for label, kw, gen in tool.BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        mask = tabular.legal_mask(tree)
        magnet = tabular.uniform_log_reg(tree)
        for n in ns:
            cfr = tabular.TabularCFR(tree, ["cfr"] * n)
            for _ in range(4):  # regrets of a few iterations: regret matching is off the uniform branch
                cfr.step()
            cfr.set_iteration(5)
            outs = (cfr.policy, cfr.values, cfr.reach)
            policies = cfr.average_policy.contiguous()
            log_reg = magnet[:, None, :].expand(S, n, 2 * A).contiguous()
            ev = rnad_hip.reg_evaluate(handle, eta, policies, log_reg)
            rows.append(dict(tree=label, S=S, A=A, C=C, levels=int(handle.max_depth), n=n, runs=runs,
                             cfr_iterate_ms=median_ms(lambda: rnad_hip.cfr_iterate(handle, cfr.regret, cfr.strategy_sum, cfr.discount, cfr.sides, *outs), runs),
                             reg_evaluate_ms=median_ms(lambda: rnad_hip.reg_evaluate(handle, eta, policies, log_reg, *ev), runs),
                             bytes=dict(records=S * A * A * C * 12, tables=S * n * 2 * A * 4, columns=S * n * 4)))
            del cfr, outs, policies, log_reg, ev
        if curves is None:  # the configs[1] tree: CFR+ next to the exact R-NaD schedule
            cfr = tabular.TabularCFR(tree, "cfr+")
            cfr.run(iterations, every=every)
            solver = tabular.TabularRNaD(tree, eta)
            solver.run(updates)
            curves = dict(tree=label, eta=eta, iterations=list(cfr.recorded), cfr_plus_average=list(cfr.average_nashconv_history[0]),
                          cfr_plus_current=list(cfr.nashconv_history[0]), rnad=list(solver.nashconv_history))
        del tree, handle, mask, magnet
    for r in rows:
        r["ratio"] = r["cfr_iterate_ms"] / r["reg_evaluate_ms"]
    name = torch.cuda.get_device_name(device)
    lines = ["# Exact CFR: one rnad_cfr_iterate", "",
             f"`python tools/tabular_cfr.py --bench --runs {runs}` on {name} ({torch.cuda.get_device_properties(device).gcnArchName}), library "
             f"{rnad_hip.source_hash()}: the median of {runs} warm calls after 10, one device event pair around each; n members of plain CFR after",
             "four iterations.  `rnad_reg_evaluate` ran on the same tree and n in the same process (the members' average policies against the",
             "uniform magnet).  No time is gated.  `MB` is what an iteration must move at least: every record once per sweep, a read and a write",
             "of the regret and strategy-sum tables, a write and a read of sigma, and the value and reach columns written and read.", "",
             "| tree | S | A | C | levels | n | MB | rnad_cfr_iterate ms | rnad_reg_evaluate ms | ratio |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['levels']} | {r['n']} | {(2 * b['records'] + 6 * b['tables'] + 8 * b['columns']) / 1e6:.1f} | "
                     f"{r['cfr_iterate_ms']:.3f} | {r['reg_evaluate_ms']:.3f} | {r['ratio']:.2f} |")
    c = curves
    final_rnad, final_cfr = c["rnad"][-1], c["cfr_plus_average"][-1]
    cross = first_below(c["iterations"], c["cfr_plus_average"], final_rnad)
    lines += ["", f"## CFR+ next to the exact R-NaD schedule on the {c['tree']} tree", "",
              f"NashConv of the average policy of {iterations} CFR+ iterations (alternating, linear average; recorded every {every}) and of",
              f"`TabularRNaD`'s {updates} updates at eta = {eta} from the uniform magnet.", "",
              "| CFR+ iteration | NashConv of the average | of the current policy |", "|---|---|---|"]
    shown = [i for i, t in enumerate(c["iterations"]) if t in (10, 20, 50, 100, 200, 500, 1000) or i == len(c["iterations"]) - 1]
    for i in sorted(set(shown)):
        lines.append(f"| {c['iterations'][i]} | {c['cfr_plus_average'][i]:.6g} | {c['cfr_plus_current'][i]:.6g} |")
    lines += ["", "| R-NaD update | NashConv |", "|---|---|"]
    for m in sorted({1, 2, 4, 8, 16, updates}):
        if m <= len(c["rnad"]):
            lines.append(f"| {m} | {c['rnad'][m - 1]:.6g} |")
    reached = f"is at or below that from iteration {cross} on" if cross is not None else f"does not get there in {iterations} iterations"
    lines += ["", f"After {updates} updates the R-NaD schedule stands at {final_rnad:.6g}; the CFR+ average {reached} and ends at {final_cfr:.6g}."]
    for m, v in enumerate(c["rnad"], 1):
        t = first_below(c["iterations"], c["cfr_plus_average"], v)
        if m in (1, 2, 4, 8, 16, updates):
            lines.append(f"R-NaD update {m} ({v:.6g}) is matched by the CFR+ average at iteration {t if t is not None else '> ' + str(iterations)}.")
    res = kernel_resources()
    lines += ["", "## Resources", ""]
    if res is None:
        lines.append("Not read: ROCm's llvm-objcopy, clang-offload-bundler and llvm-readobj were not found on the machine that ran this.")
    else:
        lines += ["From the built library's kernel metadata (gfx950); 256 threads per block, a wave per state.", "",
                  "| kernel | A | VGPRs | SGPRs | LDS bytes | scratch bytes |", "|---|---|---|---|---|---|"]
        for kernel, A, vgpr, sgpr, lds, scratch in res:
            lines.append(f"| k_cfr_{kernel} | {A} | {vgpr} | {sgpr} | {lds} | {scratch} |")
    lines.append("")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, curves=curves, crossing=cross, out=out_path, library=rnad_hip.source_hash())))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", help="tree.tar of the tree to sweep")
    ap.add_argument("--variants", nargs="+", default=["cfr", "cfr+", "linear"], help="cfr, cfr+, linear or dcfr:ALPHA:BETA:GAMMA (up to 32)")
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--every", type=int, default=50, help="record NashConv after every this many iterations (and after the last)")
    ap.add_argument("--against", nargs="*", default=[], metavar="RUN_DIR", help="saved runs whose target nets play the final average policy")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bench", action="store_true", help="time one iteration instead (see the module docstring)")
    ap.add_argument("--runs", type=int, default=30, help="--bench: timed calls (at least 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfr.md"), help="--bench: the report to write ('' for none)")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("tabular_cfr needs the GPU: there is no CPU path")
    torch.cuda.set_device(device)
    if args.bench:
        if args.runs < 20:
            raise SystemExit("--runs: a median of fewer than 20 calls is not reported")
        return bench(args.runs, args.out, device)
    if not args.tree:
        ap.error("--tree is required")
    tool = _cross_play_tool()
    tree = tool.load_tree(args.tree, device)
    names, nets = [], []
    for directory in args.against:
        name, net, _ = tool.load_player(directory, None, tree, device)
        names.append(name)
        nets.append(net)
    try:
        cfr = tabular.TabularCFR(tree, [parse_variant(v) for v in args.variants])
    except ValueError as e:
        raise SystemExit(str(e))
    cfr.run(args.iterations, every=args.every)
    average = cfr.average_policy
    results = []
    for k, text in enumerate(args.variants):
        out = dict(variant=text, alternating=cfr.alternating[k], iterations=list(cfr.recorded), average_nashconv=cfr.average_nashconv_history[k],
                   nashconv=cfr.nashconv_history[k])
        if nets:
            res = metric.cross_play(tree, [average[:, k].contiguous()] + nets)
            out.update(names=[f"{text}@T={cfr.t}"] + names, payoff=res.payoff.tolist())
        print(json.dumps(out))
        results.append(out)
    return results


if __name__ == "__main__":
    main()
