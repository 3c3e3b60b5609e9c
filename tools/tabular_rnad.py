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
event pair around each of `runs` warm calls, the median reported, next to the histogram of iterations per state.  It then times
rnad_reg_evaluate at n = 1, 8, 32 on the same trees, with rnad_cross_play and rnad_best_response on the same tables in the same process as
context, and writes profiles/reg_evaluate.md (--evaluate-out).  Needs the GPU.

    python tools/tabular_rnad.py --tree TREE.tar --evaluate RUN_DIR [RUN_DIR ...] [--alpha ALPHA] [--eta ETA]

measures a saved run's inner loop: for every checkpoint (m, n) of every RUN_DIR one JSON line with run, m, n, alpha, eta and, for the net and
the target net of the checkpoint, distance and max_residual to the fixed point of the magnet alpha * log pi_reg + (1 - alpha) * log pi_reg_
(the four nets are in the checkpoint) and the root value there (learn.tabular.evaluate_regularized).  alpha is the schedule's for (m, n)
(RNaD.alpha_of with the run's bounds and delta_m) unless --alpha overrides it; eta is the run's unless --eta does.
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


def median_ms(fn, runs):
    """Median ms of `runs` warm calls of fn, one device event pair per call (3 warm-up calls first)."""
    for _ in range(3):
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


def bench_evaluate(eta, runs, out_path, device, ns=(1, 8, 32)):
    """rnad_reg_evaluate at each n on the two bench trees, next to rnad_cross_play and rnad_best_response on the same tables."""
    tool = _cross_play_tool()
    rows = []
    for label, kw, gen in tool.BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        mask = tabular.legal_mask(tree)
        magnet = tabular.uniform_log_reg(tree)
        for n in ns:
            torch.manual_seed(n)
            z = torch.where(mask[:, None, :], torch.randn((S, n, 2 * A), device=device), torch.full((), float("-inf"), device=device))
            policies = torch.stack([tabular.softmax_support(z[:, k]) for k in range(n)], dim=1).contiguous()
            log_reg = magnet[:, None, :].expand(S, n, 2 * A).contiguous()
            outs = rnad_hip.reg_evaluate(handle, eta, policies, log_reg)
            br = rnad_hip.best_response(handle, policies)
            cp = rnad_hip.cross_play(handle, policies)
            rows.append(dict(tree=label, S=S, A=A, C=C, n=n, eta=eta, runs=runs,
                             reg_evaluate_ms=median_ms(lambda: rnad_hip.reg_evaluate(handle, eta, policies, log_reg, *outs), runs),
                             cross_play_ms=median_ms(lambda: rnad_hip.cross_play(handle, policies, cp), runs),
                             best_response_ms=median_ms(lambda: rnad_hip.best_response(handle, policies, *br), runs),
                             bytes=dict(records=S * A * A * C * 12, tables=2 * S * n * 2 * A * 4, q=S * n * 2 * A * 4, columns=5 * S * n * 4)))
            del policies, log_reg, outs, br, cp, z
        del tree, handle
    name = torch.cuda.get_device_name(device)
    lines = ["# Exact evaluation in the regularised game: one rnad_reg_evaluate", "",
             f"`python tools/tabular_rnad.py --bench --eta {eta} --runs {runs}` on {name} ({torch.cuda.get_device_properties(device).gcnArchName}), library "
             f"{rnad_hip.source_hash()}: the median of {runs} warm calls, one device event pair around each; policies are seeded masked softmax",
             "tables, the magnet is uniform.  `rnad_cross_play` (n * n values per state, one sweep) and `rnad_best_response` (two sweeps, the same",
             "lane layout) ran on the same tables in the same process and are context, not baselines.  No time is gated.  `MB` is what a call must",
             "move at least: every record once per sweep (`2 * S*A*A*C*12`), the two input tables, q, and a read and a write of the columns.", "",
             "| tree | S | A | C | n | MB | rnad_reg_evaluate ms | rnad_cross_play ms | rnad_best_response ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['n']} | {(2 * b['records'] + b['tables'] + b['q'] + b['columns']) / 1e6:.1f} | "
                     f"{r['reg_evaluate_ms']:.3f} | {r['cross_play_ms']:.3f} | {r['best_response_ms']:.3f} |")
    lines.append("")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(dict(bench_evaluate=rows, out=out_path, library=rnad_hip.source_hash())))
    return rows


def evaluate_runs(tree, directories, alpha, eta, device):
    """One JSON line per checkpoint of every run directory (see the module docstring)."""
    from learn.checkpoint import RunStore
    from learn.rnad import RNaD

    tool = _cross_play_tool()
    results = []
    for directory in directories:
        store = RunStore(directory)
        params = store.read_params()
        if "tree_hash" in params and params["tree_hash"] != tree.hash:
            raise SystemExit(f"{directory}: trained on another tree (hash {params['tree_hash']} != {tree.hash})")
        run_eta = float(params["eta"]) if eta is None else eta
        if not run_eta > 0:
            raise SystemExit(f"{directory}: eta = {run_eta}: the unregularised game has no fixed point to measure against (pass --eta)")
        for m in store.updates():
            delta_m = next((steps for bound, steps in zip(params["bounds"], params["delta_m"]) if m < bound), params["delta_m"][-1])
            for n in store.steps(m):
                saved = store.read(m, n, map_location=device)
                nets = {}
                for key in ("net", "net_target", "net_reg", "net_reg_"):
                    nets[key] = tool.new_net(saved["net_params"], device)
                    nets[key].load_state_dict(saved[key])
                a = float(RNaD.alpha_of(n, delta_m)) if alpha is None else alpha
                terms = [(w, tabular.log_reg_of(tree, nets[key])) for w, key in ((a, "net_reg"), (1 - a, "net_reg_")) if w != 0]
                magnet = terms[0][1] if len(terms) == 1 else terms[0][0] * terms[0][1] + terms[1][0] * terms[1][1]  # (a zero weight is skipped)
                ev = tabular.evaluate_regularized(tree, [nets["net"], nets["net_target"]], run_eta, log_reg=magnet)
                out = dict(run=os.path.basename(os.path.normpath(directory)), m=m, n=n, alpha=a, eta=run_eta, players=["net", "net_target"],
                           distance=ev.distance.tolist(), max_residual=ev.max_residual.tolist(), root_value=ev.values[1].tolist())
                print(json.dumps(out))
                results.append(out)
    return results


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
    ap.add_argument("--evaluate-out", default=os.path.join(ROOT, "profiles", "reg_evaluate.md"),
                    help="--bench: the report of the rnad_reg_evaluate timing ('' for none)")
    ap.add_argument("--evaluate", nargs="+", default=None, metavar="RUN_DIR", help="measure the inner loop of saved runs instead")
    ap.add_argument("--alpha", type=float, default=None, help="--evaluate: the magnet's alpha (default: the schedule's for each checkpoint)")
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
        rows = bench(etas[0], args.tol, args.max_iters, args.runs, args.out, device)
        bench_evaluate(etas[0], args.runs, args.evaluate_out, device)
        return rows
    if not args.tree:
        ap.error("--tree is required")
    tool = _cross_play_tool()
    tree = tool.load_tree(args.tree, device)
    if args.evaluate:
        if args.alpha is not None and not 0 <= args.alpha <= 1:
            raise SystemExit("--alpha must lie in [0, 1]")
        return evaluate_runs(tree, args.evaluate, args.alpha, args.eta[0] if args.eta else None, device)
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
