#!/usr/bin/env python3
"""Exact tabular R-NaD on an enumerated tree: the NashConv curve the regularisation schedule itself reaches (learn/tabular.py,
csrc/reg_solve.hip) -- no sampled games, no net.

    python tools/tabular_rnad.py --tree TREE.tar --eta 0.2 0.5 1 --updates 32 [--tol 1e-5] [--max-iters 4096] [--against RUN_DIR ...]

TREE.tar is a tree file as Tree.save writes it.  Prints one JSON line per eta: eta, nashconv (after update 1 .. updates, from the uniform
magnet), unconverged (states per update that did not reach tol).  With --against, every RUN_DIR (learn/checkpoint.RunStore) enters with the
target net of its latest checkpoint and the line also carries names and payoff: util.metric.cross_play of the final table (player 0)
against those nets, payoff[i][j] the row player's expected payoff when player i plays the rows and player j the columns.

    python tools/tabular_rnad.py --bench [--eta 0.2] [--runs 30] [--out profiles/tabular_rnad.md]

times one rnad_reg_solve from the uniform magnet on the BASELINE.json configs[1] tree and on the configs[3]-shaped native tree: a device
event pair around each of `runs` warm calls, the median reported, next to the histogram of iterations per state.  Needs the GPU.
"""
import argparse
import importlib.util
import json
import os
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


def solve_times(tree, eta, tol, max_iters, runs):
    """(per-call ms list, the outputs) of `runs` warm rnad_reg_solve calls from the uniform magnet, one event pair per call."""
    handle = tree.handle()
    log_reg = tabular.uniform_log_reg(tree)
    outs = rnad_hip.reg_solve(handle, eta, log_reg, tol=tol, max_iters=max_iters)
    for _ in range(3):
        rnad_hip.reg_solve(handle, eta, log_reg, tol, max_iters, *outs)
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rnad_hip.reg_solve(handle, eta, log_reg, tol, max_iters, *outs)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times, outs


def bench(eta, tol, max_iters, runs, out_path, device):
    tool = _cross_play_tool()
    rows = []
    edges = (0, 1, 8, 16, 32, 64, 128, 256, 512, 1024, 4096)
    for label, kw, gen in tool.BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        times, (_, policy, _, residual, iters) = solve_times(tree, eta, tol, max_iters, runs)
        reached = policy.sum(1) > 0  # rows the sweep never reaches hold zeros
        it = iters[reached].cpu()
        hist = {f"{lo}..{hi - 1}": int(((it >= lo) & (it < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])}
        hist[f">={edges[-1]}"] = int((it >= edges[-1]).sum())
        times = sorted(times)
        rows.append(dict(tree=label, S=handle.S, A=handle.A, C=handle.C, levels=int(handle.max_depth), eta=eta, tol=tol, runs=runs,
                         median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], iters_max=int(it.max()),
                         iters_mean=float(it.float().mean()), iters_sum=int(it.sum()),
                         unconverged=int(((iters >= max_iters) & ~(residual <= tol))[reached].sum()), histogram=hist))
        del tree, handle
    name = torch.cuda.get_device_name(device)
    lines = ["# Exact tabular R-NaD: one rnad_reg_solve", "",
             f"`python tools/tabular_rnad.py --bench --eta {eta} --runs {runs}` on {name} ({torch.cuda.get_device_properties(device).gcnArchName}), library "
             f"{rnad_hip.source_hash()}: one device event pair around each of {runs} warm calls from the uniform magnet, tol = {tol}; "
             "the median, with the fastest and slowest call next to it.", "",
             "| tree | S | A | C | median ms | min | max | iterations: max | mean | sum over states | unconverged |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} | {r['max_ms']:.3f} | {r['iters_max']} | "
                     f"{r['iters_mean']:.1f} | {r['iters_sum']} | {r['unconverged']} |")
    lines += ["", "Iterations per reached state:", "", "| tree | " + " | ".join(rows[0]["histogram"]) + " |", "|---|" + "---|" * len(rows[0]["histogram"])]
    for r in rows:
        lines.append(f"| {r['tree']} | " + " | ".join(str(v) for v in r["histogram"].values()) + " |")
    lines.append("")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, out=out_path, library=rnad_hip.source_hash(), so=os.path.basename(os.path.realpath(rnad_hip.SO_PATH)))))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", help="tree.tar of the tree to sweep")
    ap.add_argument("--eta", type=float, nargs="+", default=None, help="regularisation strengths, each > 0")
    ap.add_argument("--updates", type=int, default=32, help="regularisation updates per eta")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--max-iters", type=int, default=4096)
    ap.add_argument("--against", nargs="*", default=[], metavar="RUN_DIR", help="saved runs whose target nets play the final table")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bench", action="store_true", help="time one solve instead (see the module docstring)")
    ap.add_argument("--runs", type=int, default=30, help="--bench: timed calls (at least 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabular_rnad.md"), help="--bench: the report to write ('' for none)")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("tabular_rnad needs the GPU: there is no CPU path")
    torch.cuda.set_device(device)
    etas = args.eta if args.eta else ([0.2] if args.bench else [0.2, 0.5, 1.0])
    if any(not e > 0 for e in etas):
        raise SystemExit("--eta must be positive: the unregularised game has no unique fixed point to sweep to")
    if args.bench:
        if args.runs < 20:
            raise SystemExit("--runs: a median of fewer than 20 calls is not reported")
        return bench(etas[0], args.tol, args.max_iters, args.runs, args.out, device)
    if not args.tree:
        ap.error("--tree is required")
    tool = _cross_play_tool()
    tree = tool.load_tree(args.tree, device)
    names, nets = [], []
    for directory in args.against:
        name, net, _ = tool.load_player(directory, None, tree, device)
        names.append(name)
        nets.append(net)
    results = []
    for eta in etas:
        solver = tabular.TabularRNaD(tree, eta, tol=args.tol, max_iters=args.max_iters)
        solver.run(args.updates)
        out = dict(eta=eta, nashconv=list(solver.nashconv_history), unconverged=list(solver.unconverged_history))
        if nets:
            res = metric.cross_play(tree, [solver.policy] + nets)
            out.update(names=[f"tabular@eta={eta}"] + names, payoff=res.payoff.tolist())
        print(json.dumps(out))
        results.append(out)
    return results


if __name__ == "__main__":
    main()
