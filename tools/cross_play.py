#!/usr/bin/env python3
"""Exact cross-play of saved runs: which net beats which on the enumerated tree (util.metric.cross_play, csrc/cross_play.hip).

    python tools/cross_play.py --tree TREE.tar RUN_DIR [RUN_DIR ...] [--checkpoint M N] [--fresh] [--seed 0]

TREE.tar is a tree file as Tree.save writes it; every RUN_DIR is a run directory (learn/checkpoint.RunStore: `params` and `<m>/<n>`
checkpoints).  A run enters with the TARGET net of its latest checkpoint, or of checkpoint M/N with --checkpoint; --fresh adds an
untrained net of the first run's shape (an MLP of width 256 when there is no run).  A run trained on another tree is refused, by the hash
in its `params`.  Prints one JSON line: names, payoff (payoff[i][j]: the row player's expected payoff when player i plays the rows and
player j the columns), nashconv and exploitability per player.

    python tools/cross_play.py --bench [--players 8] [--out profiles/cross_play.md]

times one rnad_cross_play of `players` untrained nets on the BASELINE.json configs[1] tree (depth-6 ternary, 66 431 states) and on the
configs[3]-shaped native tree (5 x 5 actions, 4 chance outcomes, depth 8, pruned 7/8), and next to it `players` calls of rnad_nashconv on the
same tables -- context only: the two answer different questions and nothing is gated on the ratio.  Times are device events around a window
of back-to-back calls after a warm-up.  Needs the GPU: there is no CPU path.
"""
import argparse
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

WINDOW_MS = 500.0  # a timed window lasts about this long: well above clock and scheduler noise


def load_tree(path, device):
    """A Tree from a tree.tar file (the dict Tree.save writes, environment/tree.py) on `device`."""
    tree = Tree()
    for key, value in torch.load(path, map_location="cpu", weights_only=False).items():
        tree.__dict__[key] = value
    tree.to(device)
    return tree


def new_net(net_params, device):
    types = {"MLP": nets.MLP}
    if hasattr(nets, "ConvNet"):
        types["ConvNet"] = nets.ConvNet
    kw = {k: v for k, v in net_params.items() if k != "type"}
    net = types[net_params["type"]](**kw, device=device)
    net.eval()
    return net


def load_player(directory, checkpoint, tree, device):
    """(name, target net, net_params) of a run directory at `checkpoint` = (m, n), or at its latest checkpoint."""
    store = RunStore(directory)
    params = store.read_params()
    if "tree_hash" in params and params["tree_hash"] != tree.hash:
        raise SystemExit(f"{directory}: trained on another tree (hash {params['tree_hash']} != {tree.hash})")
    at = tuple(checkpoint) if checkpoint is not None else store.latest()
    if at is None or at[1] not in store.steps(at[0]):
        raise SystemExit(f"{directory}: no checkpoint" + (f" {at[0]}/{at[1]}" if at else ""))
    saved = store.read(*at, map_location=device)
    net = new_net(saved["net_params"], device)
    net.load_state_dict(saved["net_target"])
    return f"{os.path.basename(os.path.normpath(directory))}@{at[0]}/{at[1]}", net, saved["net_params"]


def timeit(fn, max_reps=2000):
    """ms per call over one window of back-to-back calls: 3 warm-up calls, one calibration call, then as many calls as fill WINDOW_MS."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = int(max(3, min(max_reps, WINDOW_MS / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def sweep_bytes(S, A, C, n):
    """What one sweep must move: every Trans record once, and about a read and a write of every value (plus the policy tables)."""
    P = n * n
    return dict(records=S * A * A * C * 12, values=2 * S * P * 4, policies=S * n * 2 * A * 4)


BENCH_TREES = (
    ("configs[1]", dict(max_actions=3, max_transitions=1, depth_bound=6, transition_threshold=0.0), dict(seed=0, prune=(0, 0))),
    ("configs[3]-shaped", dict(max_actions=5, max_transitions=4, depth_bound=8, transition_threshold=0.1), dict(seed=0, prune=(7, 8))),
)


def bench(n, out_path, device):
    rows = []
    for label, kw, gen in BENCH_TREES:
        tree = Tree(device=device, **kw)
        tree.generate_native(**gen)
        handle = tree.handle()
        S, A, C = handle.S, handle.A, handle.C
        torch.manual_seed(0)
        policies = torch.zeros((S, n, 2 * A), device=device)
        for k in range(n):
            metric.joint_policy_of(tree, nets.MLP(A, 256, device=device), out=policies[:, k])
        values = torch.empty((S, n, n), device=device)
        cross_ms, cross_reps = timeit(lambda: rnad_hip.cross_play(handle, policies, values))
        tables = [policies[:, k].contiguous() for k in range(n)]
        data = metric.NashConvData(tree)

        def nashconvs():
            for t in tables:
                rnad_hip.nashconv(handle, t, t[1], 1, 1.0, data.row_best, data.col_best, data.reach_probability, data.depth)

        nash_ms, nash_reps = timeit(nashconvs)
        rows.append(dict(tree=label, S=S, A=A, C=C, n=n, cross_ms=cross_ms, cross_reps=cross_reps, nash_ms=nash_ms, nash_reps=nash_reps,
                         bytes=sweep_bytes(S, A, C, n)))
        del tree, handle, policies, values, tables, data
    lines = ["# Cross-play sweep: one rnad_cross_play against n calls of rnad_nashconv", "",
             f"`python tools/cross_play.py --bench --players {n}` on {torch.cuda.get_device_name(device)} "
             f"({torch.cuda.get_device_properties(device).gcnArchName}): device events around a window of",
             f"back-to-back calls (about {WINDOW_MS:.0f} ms) after a warm-up; players are untrained MLPs of width 256.  The sweep must move every",
             "Trans record once (`S*A*A*C*12` bytes) and read and write every value about once (`2*S*P*4`, P = n*n), next to the policy tables",
             "(`S*n*2A*4`); `GB/s` is those bytes over the measured time, not a counter.  The `rnad_nashconv` column is context, not a baseline:",
             "it answers another question (best responses to one joint policy) with two sweeps per call.", "",
             "| tree | S | A | C | n | records MB | values MB | policies MB | rnad_cross_play ms | GB/s | n x rnad_nashconv ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = r["bytes"]
        total = b["records"] + b["values"] + b["policies"]
        lines.append(f"| {r['tree']} | {r['S']} | {r['A']} | {r['C']} | {r['n']} | {b['records'] / 1e6:.1f} | {b['values'] / 1e6:.1f} | "
                     f"{b['policies'] / 1e6:.1f} | {r['cross_ms']:.3f} ({r['cross_reps']} calls) | {total / r['cross_ms'] / 1e6:.0f} | "
                     f"{r['nash_ms']:.3f} ({r['nash_reps']} rounds) |")
    lines += ["", "Built one pair at a time, the sweep would read the records n*n times; here a wave reads them once for 64 pairs.", ""]
    with open(out_path, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(dict(bench=rows, out=out_path)))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("runs", nargs="*", help="run directories (params + <m>/<n> checkpoints)")
    ap.add_argument("--tree", help="tree.tar of the tree the runs were trained on")
    ap.add_argument("--checkpoint", type=int, nargs=2, metavar=("M", "N"), help="checkpoint to take from every run (default: its latest)")
    ap.add_argument("--fresh", action="store_true", help="add an untrained net")
    ap.add_argument("--seed", type=int, default=0, help="seed of the untrained net")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bench", action="store_true", help="time the sweep instead (see the module docstring)")
    ap.add_argument("--players", type=int, default=8, help="--bench: number of policies")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_play.md"), help="--bench: the report to write")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("cross_play needs the GPU: there is no CPU path")
    torch.cuda.set_device(device)
    if args.bench:
        return bench(args.players, args.out, device)
    if not args.tree or not (args.runs or args.fresh):
        ap.error("--tree and at least one run directory (or --fresh) are required")
    tree = load_tree(args.tree, device)
    names, players, net_params = [], [], None
    for directory in args.runs:
        name, net, params = load_player(directory, args.checkpoint, tree, device)
        names.append(name)
        players.append(net)
        net_params = net_params or params
    if args.fresh:
        torch.manual_seed(args.seed)
        names.append("fresh")
        players.append(new_net(net_params or {"type": "MLP", "max_actions": tree.max_actions, "width": 256}, device))
    result = metric.cross_play(tree, players)
    out = dict(names=names, payoff=result.payoff.tolist(), nashconv=result.nashconv.tolist(), exploitability=result.exploitability.tolist())
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
