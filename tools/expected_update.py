"""The learner's update with the sampling taken out, for the checkpoints of saved runs.

    python tools/expected_update.py --tree TREE.tar RUN_DIR [RUN_DIR ...] [--alpha A] [--rho R ...] [--c C ...] [--lambda L ...]

prints one JSON line per checkpoint and setting: the run's four nets and hyperparameters (the actor's policy -- the net's raw pi -- as the
behaviour) go through learn.vtrace.expected_update (rnad_vtrace_expect), which gives what the V-trace targets, the action
values and the two heads' row gradients ARE in expectation over complete episodes.  Reported: the expected episode length, target_bias
(sum_s reach |target - v_target| per player: how far clips, lambda and the bootstrap push the target away from the value it stands for),
the reach-weighted |v - target| the value head still has to close, the norms of the two expected gradient tables, and the share of the
reached rows on which the NeuRD direction is the exact expectation.  --rho, --c, --lambda replace the run's values; several values give
one line each, so a clip setting can be compared on the very same nets.  --noise goes through learn.vtrace.update_noise instead
(rnad_vtrace_moments) and adds, per player and for one episode, target_noise (sum_s reach Var[v_target]: to be read next to
target_bias), dv_noise (the summed variance of the value head's row gradients) and episodes_for_unit_snr (the batch at which that
gradient's signal equals its noise).

    python tools/expected_update.py --bench [--runs 30]

times rnad_vtrace_expect at n = 1, 8, 32 on the configs[1] tree and the configs[3]-shaped tree, next to rnad_reg_evaluate at the same n on
the same trees in the same process, and writes profiles/vtrace_expect.md (--out).  --bench --noise times rnad_vtrace_moments next to
rnad_vtrace_expect instead, the same way, and writes profiles/vtrace_moments.md.  Needs the GPU."""
import argparse
import importlib.util
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "r-nad_amd"))
import torch  # noqa: E402

import rnad_hip  # noqa: E402
from environment.tree import Tree  # noqa: E402
from learn import tabular, vtrace  # noqa: E402


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def learn_params(params, alpha, rho=None, c=None, lambda_=None):
    """The LearnParams of a saved run's `params` (RNaD's attribute names), with the three V-trace settings replaced where given."""
    get = params.get
    return rnad_hip.make_learn_params(
        alpha=alpha, eta=float(get("eta", 0.2)), lambda_=1.0 if lambda_ is None else lambda_, c=float(get("c_bar", 1)) if c is None else c,
        rho=float(get("roh_bar", 1)) if rho is None else rho, gamma=float(get("vtrace_gamma", 1)), clip=float(get("neurd_clip", 1e3)),
        threshold=float(get("beta", 2)), w_v=float(get("value_weight", 1)), w_n=float(get("neurd_weight", 1)),
        eps_threshold=float(get("epsilon_threshold", 0.03)), n_disc=int(get("n_discrete", 32)))


def summarise(ev, v_rows):
    S = ev.reach.shape[0]
    reach2 = torch.cat([ev.reach, ev.reach]).double()
    gap = reach2 * (v_rows.double() - ev.target.double()).abs()
    seen = reach2 > 0
    return dict(length=ev.length, target_bias=ev.target_bias.tolist(), value_gap=[float(gap[:S].sum()), float(gap[S:].sum())],
                dv_norm=float(ev.dv_tab.double().norm()), dlogit_norm=float(ev.dlogit_tab.double().norm()),
                linear_share=float((ev.linear & seen).sum()) / max(int(seen.sum()), 1), root_target=[float(ev.target[1]), float(ev.target[S + 1])])


def summarise_noise(noise):
    S = noise.expected.reach.shape[0]
    return dict(target_noise=noise.target_noise.tolist(), dv_noise=[float(noise.dv_var_tab[:S].sum()), float(noise.dv_var_tab[S:].sum())],
                episodes_for_unit_snr=noise.episodes_for_unit_snr.tolist())


def expected_updates(tree, directories, alpha, rhos, cs, lambdas, device, noise=False):
    """One JSON line per checkpoint of every run directory and per (rho, c, lambda) setting."""
    from learn.checkpoint import RunStore
    from learn.rnad import RNaD

    tool = _tool("cross_play")
    results = []
    for directory in directories:
        store = RunStore(directory)
        params = store.read_params()
        if "tree_hash" in params and params["tree_hash"] != tree.hash:
            raise SystemExit(f"{directory}: trained on another tree (hash {params['tree_hash']} != {tree.hash})")
        for m in store.updates():
            delta_m = next((steps for bound, steps in zip(params["bounds"], params["delta_m"]) if m < bound), params["delta_m"][-1])
            for n in store.steps(m):
                saved = store.read(m, n, map_location=device)
                nets = {}
                for key in ("net", "net_target", "net_reg", "net_reg_"):
                    nets[key] = tool.new_net(saved["net_params"], device)
                    nets[key].load_state_dict(saved[key])
                a = float(RNaD.alpha_of(n, delta_m)) if alpha is None else alpha
                v_rows = vtrace._net_rows(tree, nets["net"])[1]
                for rho, c, lambda_ in itertools.product(rhos, cs, lambdas):
                    hp = learn_params(params, a, rho, c, lambda_)
                    call = vtrace.update_noise if noise else vtrace.expected_update
                    ev = call(tree, nets["net"], nets["net"], None, nets["net_target"], nets["net_reg"], nets["net_reg_"], hp)
                    extra = summarise_noise(ev) if noise else {}
                    ev = ev.expected if noise else ev
                    out = dict(run=os.path.basename(os.path.normpath(directory)), m=m, n=n, alpha=a, eta=hp.eta, gamma=hp.gamma,
                               rho=hp.rho, c=hp.c, **{"lambda": hp.lambda_}, **summarise(ev, v_rows), **extra)
                    print(json.dumps(out))
                    results.append(out)
    return results


def bench(runs, out_path, device, ns=(1, 8, 32)):
    """rnad_vtrace_expect at each n on the two bench trees, next to rnad_reg_evaluate at the same n in the same process."""
    timing = _tool("tabular_rnad")
    rows = []
    for label, kw, gen in _tool("cross_play").BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        mask = tabular.legal_mask(tree)
        magnet = tabular.uniform_log_reg(tree)
        for n in ns:
            torch.manual_seed(n)
            minus = torch.full((), float("-inf"), device=device)
            draw = lambda: torch.stack([tabular.softmax_support(torch.where(mask, torch.randn((S, 2 * A), device=device), minus))  # noqa: E731
                                        for _ in range(n)], dim=1).contiguous()
            mu, pip = draw(), draw()
            lpol = torch.where(mask[:, None, :], torch.randn((S, n, 2 * A), device=device), torch.zeros((), device=device)).contiguous()
            vv = (0.5 * torch.randn((S, n, 2), device=device)).contiguous()
            hyper = [(0.2, 1.0, 0.9, 1.0, 1.0)] * n
            log_reg = magnet[:, None, :].expand(S, n, 2 * A).contiguous()
            ws = torch.empty((int(rnad_hip.lib().rnad_vtrace_expect_workspace(S, A, n)),), device=device)
            outs = rnad_hip.vtrace_expect(handle, hyper, mu, pip, lpol, vv, workspace=ws)
            ev = rnad_hip.reg_evaluate(handle, 0.2, pip, log_reg)
            rows.append(dict(tree=label, S=S, A=A, C=C, n=n, runs=runs,
                             vtrace_expect_ms=timing.median_ms(lambda: rnad_hip.vtrace_expect(handle, hyper, mu, pip, lpol, vv, *outs, ws), runs),
                             reg_evaluate_ms=timing.median_ms(lambda: rnad_hip.reg_evaluate(handle, 0.2, pip, log_reg, *ev), runs),
                             bytes=dict(records=S * A * A * C * 12, tables=3 * S * n * 2 * A * 4, q=S * n * 2 * A * 4,
                                        export=2 * S * n * (3 * A + 5) * 4, columns=(2 + 2 + A + 2) * S * n * 4)))
            del mu, pip, lpol, vv, log_reg, ws, outs, ev
        del tree, handle
    name = torch.cuda.get_device_name(device)
    lines = ["# The exact expected learner update: one rnad_vtrace_expect", "",
             f"`python tools/expected_update.py --bench --runs {runs}` on {name} ({torch.cuda.get_device_properties(device).gcnArchName}), library "
             f"{rnad_hip.source_hash()}: the median of {runs} warm calls, one device event pair around each; mu and pip are seeded masked",
             "softmax tables, lpol and vv seeded normals, (eta, gamma, lambda, rho, c) = (0.2, 1, 0.9, 1, 1).  `rnad_reg_evaluate` ran at the same",
             "n on the same trees in the same process (pip as its policy, the uniform magnet) and is context, not a baseline.  No time is gated.",
             "`MB` is what a call must move at least: every record once per sweep, the three input tables, q, one write and one read of every",
             "export record, and the columns (vv, target, target_given_row, reach twice).", "",
             "| tree | S | A | C | n | MB | rnad_vtrace_expect ms | rnad_reg_evaluate ms | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['n']} | "
                     f"{(2 * b['records'] + b['tables'] + b['q'] + b['export'] + b['columns']) / 1e6:.1f} | {r['vtrace_expect_ms']:.3f} | "
                     f"{r['reg_evaluate_ms']:.3f} | {r['vtrace_expect_ms'] / r['reg_evaluate_ms']:.2f} |")
    lines.append("")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, out=out_path, library=rnad_hip.source_hash())))
    return rows


def bench_noise(runs, out_path, device, ns=(1, 8, 32)):
    """rnad_vtrace_moments at each n on the two bench trees, next to rnad_vtrace_expect on the same inputs in the same process."""
    timing = _tool("tabular_rnad")
    rows = []
    for label, kw, gen in _tool("cross_play").BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        mask = tabular.legal_mask(tree)
        for n in ns:
            torch.manual_seed(n)
            minus = torch.full((), float("-inf"), device=device)
            draw = lambda: torch.stack([tabular.softmax_support(torch.where(mask, torch.randn((S, 2 * A), device=device), minus))  # noqa: E731
                                        for _ in range(n)], dim=1).contiguous()
            mu, pip = draw(), draw()
            lpol = torch.where(mask[:, None, :], torch.randn((S, n, 2 * A), device=device), torch.zeros((), device=device)).contiguous()
            vv = (0.5 * torch.randn((S, n, 2), device=device)).contiguous()
            hyper = [(0.2, 1.0, 0.9, 1.0, 1.0)] * n
            ws = torch.empty((int(rnad_hip.lib().rnad_vtrace_expect_workspace(S, A, n)),), device=device)
            ws2 = torch.empty((int(rnad_hip.lib().rnad_vtrace_moments_workspace(S, A, n)),), device=device)
            outs = rnad_hip.vtrace_expect(handle, hyper, mu, pip, lpol, vv, workspace=ws)
            mom = rnad_hip.vtrace_moments(handle, hyper, mu, pip, lpol, vv, ws, *outs[:3], workspace=ws2)
            rows.append(dict(tree=label, S=S, A=A, C=C, n=n, runs=runs,
                             vtrace_expect_ms=timing.median_ms(lambda: rnad_hip.vtrace_expect(handle, hyper, mu, pip, lpol, vv, *outs, ws), runs),
                             vtrace_moments_ms=timing.median_ms(
                                 lambda: rnad_hip.vtrace_moments(handle, hyper, mu, pip, lpol, vv, ws, *outs[:3], *mom, ws2), runs),
                             bytes=dict(records=S * A * A * C * 12, tables=3 * S * n * 2 * A * 4, q=2 * S * n * 2 * A * 4,
                                        export=S * n * (3 * A + 5) * 4 + 2 * S * n * (A + 1) * 4, columns=(2 + 2 + A + 2 + A) * S * n * 4)))
            del mu, pip, lpol, vv, ws, ws2, outs, mom
        del tree, handle
    name = torch.cuda.get_device_name(device)
    lines = ["# The exact variance of the learner update: one rnad_vtrace_moments", "",
             f"`python tools/expected_update.py --bench --noise --runs {runs}` on {name} ({torch.cuda.get_device_properties(device).gcnArchName}), "
             f"library {rnad_hip.source_hash()}: the median of {runs} warm calls, one device event pair around each, on the inputs of",
             "profiles/vtrace_expect.md (seeded masked softmax tables mu and pip, seeded normal lpol and vv, (eta, gamma, lambda, rho, c) =",
             "(0.2, 1, 0.9, 1, 1)).  `rnad_vtrace_expect` ran on the same inputs in the same process; its outputs and export records are this",
             "sweep's first moments.  No time is gated.  `MB` is what a call must move at least: every record once, the three input tables,",
             "q and q_var, one read of every first-moment export record, one write and one read of every second-moment record, and the",
             "columns (vv, target, target_given_row, target_var, target_given_row_var).", "",
             "| tree | S | A | C | n | MB | rnad_vtrace_moments ms | rnad_vtrace_expect ms | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['n']} | "
                     f"{(b['records'] + b['tables'] + b['q'] + b['export'] + b['columns']) / 1e6:.1f} | {r['vtrace_moments_ms']:.3f} | "
                     f"{r['vtrace_expect_ms']:.3f} | {r['vtrace_moments_ms'] / r['vtrace_expect_ms']:.2f} |")
    lines.append("")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, out=out_path, library=rnad_hip.source_hash())))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("runs_dirs", nargs="*", metavar="RUN_DIR", help="saved runs whose checkpoints to evaluate")
    ap.add_argument("--tree", help="tree.tar of the tree the runs were trained on")
    ap.add_argument("--alpha", type=float, default=None, help="the magnet's alpha (default: the schedule's for each checkpoint)")
    ap.add_argument("--rho", type=float, nargs="+", default=[None], help="V-trace clip rho (default: the run's)")
    ap.add_argument("--c", type=float, nargs="+", default=[None], help="V-trace clip c (default: the run's)")
    ap.add_argument("--lambda", dest="lambda_", type=float, nargs="+", default=[None], help="V-trace lambda (default: 1, the learner's)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--noise", action="store_true", help="add the exact variance of the update (learn.vtrace.update_noise) to each line")
    ap.add_argument("--bench", action="store_true", help="time the sweep instead (see the module docstring)")
    ap.add_argument("--runs", type=int, default=30, help="--bench: timed calls (at least 20)")
    ap.add_argument("--out", default=None,
                    help="--bench: the report to write ('' for none; default profiles/vtrace_expect.md, with --noise profiles/vtrace_moments.md)")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("expected_update needs the GPU: there is no CPU path")
    torch.cuda.set_device(device)
    if args.bench:
        if args.runs < 20:
            raise SystemExit("--runs: a median of fewer than 20 calls is not reported")
        default = os.path.join(ROOT, "profiles", "vtrace_moments.md" if args.noise else "vtrace_expect.md")
        return (bench_noise if args.noise else bench)(args.runs, default if args.out is None else args.out, device)
    if not args.tree or not args.runs_dirs:
        ap.error("--tree and at least one RUN_DIR are required")
    if args.alpha is not None and not 0 <= args.alpha <= 1:
        raise SystemExit("--alpha must lie in [0, 1]")
    if any(x is not None and x < 0 for x in args.rho + args.c):
        raise SystemExit("--rho and --c must not be negative")
    tree = _tool("cross_play").load_tree(args.tree, device)
    return expected_updates(tree, args.runs_dirs, args.alpha, args.rho, args.c, args.lambda_, device, noise=args.noise)


if __name__ == "__main__":
    main()
