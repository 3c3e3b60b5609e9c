#!/usr/bin/env python3
"""Saved runs judged as a population: the meta-Nash and the uniform mixture of their nets (util.metric.population, csrc/mixture.hip).

    python tools/population.py --tree TREE.tar RUN_DIR [RUN_DIR ...] [--last K] [--fresh] [--seed 0]

TREE.tar and RUN_DIR as for tools/cross_play.py, whose loaders this tool imports.  Every run enters with the TARGET nets of its last K
checkpoints (default 1: its latest); --fresh adds an untrained net of the first run's shape (an MLP of width 256 when there is no run).
At most 32 players in total.  Prints one JSON line: names, payoff and nashconv per player as tools/cross_play.py prints them; row and col,
the meta-Nash weights of the payoff matrix, with its value and gap (util.metric.meta_nash); nash_nashconv and uniform_nashconv, the
NashConv of the Nash mixture and of the uniform mixture of the players -- for the checkpoints of one run, of its average iterate.

    python tools/population.py --bench [--players 8] [--out profiles/mixture.md]

times one rnad_mixture of `players` untrained nets with uniform weights on the two trees of tools/cross_play.py --bench, and next to it
one rnad_cross_play of the same tables -- context only: the two answer different questions and nothing is gated on either time.  Times are
device events around a window of back-to-back calls after a warm-up.  Needs the GPU: there is no CPU path.
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
from learn.checkpoint import RunStore  # noqa: E402
from nn import net as nets  # noqa: E402
from util import metric  # noqa: E402

_spec = importlib.util.spec_from_file_location("cross_play_tool", os.path.join(ROOT, "tools", "cross_play.py"))
cross_play_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cross_play_tool)


def last_checkpoints(directory, k):
    """The last k checkpoints (m, n) of a run directory, oldest first."""
    store = RunStore(directory)
    every = [(m, n) for m in store.updates() for n in store.steps(m)]
    if not every:
        raise SystemExit(f"{directory}: no checkpoint")
    return every[-k:]


def sweep_bytes(S, A, C, n):
    """What one sweep must move: every Trans record once, a write and a read of every reach row, the policy tables, the mixture."""
    return dict(records=S * A * A * C * 12, reach=2 * S * 2 * n * 4, policies=S * n * 2 * A * 4, mix=S * 2 * A * 4)


def bench(n, out_path, device):
    rows = []
    for label, kw, gen in cross_play_tool.BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        torch.manual_seed(0)
        policies = torch.zeros((S, n, 2 * A), device=device)
        for k in range(n):
            metric.joint_policy_of(tree, nets.MLP(A, 256, device=device), out=policies[:, k])
        weights = torch.full((2, n), 1.0 / n, device=device)
        mix, reach = torch.empty((S, 2 * A), device=device), torch.empty((S, 2, n), device=device)
        values = torch.empty((S, n, n), device=device)
        mix_ms, mix_reps = cross_play_tool.timeit(lambda: rnad_hip.mixture(handle, policies, weights, mix, reach))
        cross_ms, cross_reps = cross_play_tool.timeit(lambda: rnad_hip.cross_play(handle, policies, values))
        rows.append(dict(tree=label, S=S, A=A, C=C, n=n,
                         mix_ms=mix_ms, mix_reps=mix_reps, cross_ms=cross_ms, cross_reps=cross_reps, bytes=sweep_bytes(S, A, C, n)))
        del tree, handle, policies, weights, mix, reach, values
    lines = ["# Mixture sweep: one rnad_mixture, with rnad_cross_play of the same tables beside it", "",
             f"`python tools/population.py --bench --players {n}` on {torch.cuda.get_device_name(device)} "
             f"({torch.cuda.get_device_properties(device).gcnArchName}): device events around a window of",
             f"back-to-back calls (about {cross_play_tool.WINDOW_MS:.0f} ms) after a warm-up; players are untrained MLPs of width 256, weights "
             "uniform.  The sweep must move",
             "every Trans record once (`S*A*A*C*12` bytes), write and read every reach row (`2*S*2n*4`), read the policy tables (`S*n*2A*4`) and",
             "write the mixture (`S*2A*4`); `GB/s` is those bytes over the measured time, not a counter.  The `rnad_cross_play` column is",
             "context, not a baseline: it answers another question, bottom-up, with n*n values per state.  No time is gated anywhere.", "",
             "| tree | S | A | C | n | records MB | reach MB | policies MB | rnad_mixture ms | GB/s | rnad_cross_play ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        total = sum(b.values())
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['n']} | {b['records'] / 1e6:.1f} | {b['reach'] / 1e6:.1f} | "
                     f"{b['policies'] / 1e6:.1f} | {r['mix_ms']:.3f} ({r['mix_reps']} calls) | {total / r['mix_ms'] / 1e6:.0f} | "
                     f"{r['cross_ms']:.3f} ({r['cross_reps']} calls) |")
    lines += ["", "A call is one launch per level of the tree plus the one that writes the rows no path reaches; a wave holds one state, so with n = 8 a\nquarter of its lanes carry a member.  Variants that were measured and not kept: `profiles/mixture_variants.md`.", ""]
    with open(out_path, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, out=out_path)))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("runs", nargs="*", help="run directories (params + <m>/<n> checkpoints)")
    ap.add_argument("--tree", help="tree.tar of the tree the runs were trained on")
    ap.add_argument("--last", type=int, default=1, metavar="K", help="checkpoints to take from every run, counted from its latest")
    ap.add_argument("--fresh", action="store_true", help="add an untrained net")
    ap.add_argument("--seed", type=int, default=0, help="seed of the untrained net")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bench", action="store_true", help="time the sweep instead (see the module docstring)")
    ap.add_argument("--players", type=int, default=8, help="--bench: number of policies")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture.md"), help="--bench: the report to write")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("population needs the GPU: there is no CPU path")
    torch.cuda.set_device(device)
    if args.bench:
        return bench(args.players, args.out, device)
    if not args.tree or not (args.runs or args.fresh):
        ap.error("--tree and at least one run directory (or --fresh) are required")
    if args.last < 1:
        ap.error("--last takes a positive count")
    if len(args.runs) + int(args.fresh) > rnad_hip.CROSS_PLAY_MAX:
        raise SystemExit(f"population takes at most {rnad_hip.CROSS_PLAY_MAX} players, got {len(args.runs)} runs"
                         + (" and a fresh net" if args.fresh else ""))
    tree = cross_play_tool.load_tree(args.tree, device)
    names, players, net_params = [], [], None
    for directory in args.runs:
        for at in last_checkpoints(directory, args.last):
            name, net, params = cross_play_tool.load_player(directory, at, tree, device)
            names.append(name)
            players.append(net)
            net_params = net_params or params
    if args.fresh:
        torch.manual_seed(args.seed)
        names.append("fresh")
        players.append(cross_play_tool.new_net(net_params or {"type": "MLP", "max_actions": tree.max_actions, "width": 256}, device))
    if len(players) > rnad_hip.CROSS_PLAY_MAX:
        raise SystemExit(f"population takes at most {rnad_hip.CROSS_PLAY_MAX} players, got {len(players)}")
    pop = metric.population(tree, players)
    out = dict(names=names, payoff=pop.cross.payoff.tolist(), nashconv=pop.cross.nashconv.tolist(), row=pop.meta.row.tolist(),
               col=pop.meta.col.tolist(), value=pop.meta.value, gap=pop.meta.gap, nash_nashconv=pop.nash_nashconv,
               uniform_nashconv=pop.uniform_nashconv)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
