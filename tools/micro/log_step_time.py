"""Time of a LOGGED training step, RNaD.train_step(buf, alpha, log={}), next to the replayed step -- BASELINE.json configs[1] (A = 3, C = 1,
depth 6, width 256) at 2^20 lanes by default -- with RNaD.compact_log off and on.

A logged step runs eagerly between replays and ends in a device -> host copy, so its cost to the user is wall time: a host clock around the
call, which returns only after that copy (the stream is idle before it: synchronised).  The device events around the same call are printed
beside it (what the GPU was busy for).  Warm-up first (the capture, both logged variants once), then `--reps` logged steps per variant,
the variants alternating, two replays in between as in a run with log_mod > 1; medians.  The replayed step: `--replays` replays between two
events, `--reps` times; median.

    python tools/micro/log_step_time.py [--batch-log2 20] [--reps 15] [--flags off on]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "..", "r-nad_amd"))
import torch  # noqa: E402

from environment.episode import Buffer  # noqa: E402
from environment.tree import Tree  # noqa: E402
from learn.rnad import RNaD  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-log2", type=int, default=20)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--flags", nargs="+", choices=("off", "on"), default=["off", "on"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("log_step_time.py needs the GPU: there is nothing to time without it")
    if "on" in args.flags and not hasattr(RNaD, "compact_log"):
        raise SystemExit("this tree has no RNaD.compact_log: run with --flags off")
    dev = torch.device("cuda:0")
    tree = Tree(device=dev, max_actions=3, max_transitions=1, depth_bound=args.depth, transition_threshold=0.0)
    tree.generate_native(seed=0)
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_logtime_")
    torch.manual_seed(0)
    rn = RNaD(tree=tree, device=dev, directory_name="logtime", batch_size=1 << args.batch_log2, eta=0.2, b1_adam=0.0,
              net_params={"type": "MLP", "max_actions": 3, "width": args.width})
    rn.initialize()
    with torch.no_grad():
        for p in rn.net_reg_.parameters():  # (two distinct regularisation nets, as bench.py)
            p.mul_(1.001)
    buf = Buffer(1)
    alpha = 0.3

    def plain(n=1):
        for _ in range(n):
            rn.train_step(buf, alpha)
            rn.total_steps += 1

    def logged(flag):
        if hasattr(RNaD, "compact_log"):
            rn.compact_log = flag == "on"
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        log = {}
        rn.train_step(buf, alpha, log=log)
        end.record()
        wall = time.perf_counter() - t0  # (the step's last act was the copy of its scalars to the host)
        rn.total_steps += 1
        end.synchronize()
        assert len(log) == 9, sorted(log)
        return 1e3 * wall, start.elapsed_time(end)

    plain(10)
    for flag in args.flags:
        logged(flag)
        plain(2)
    torch.cuda.synchronize()
    replayed = bool(getattr(rn, "_graph", None) and rn._graph.get("graph") is not None)
    times = {flag: [] for flag in args.flags}
    for _ in range(args.reps):
        for flag in args.flags:
            times[flag].append(logged(flag))
            plain(2)
    step = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        plain(args.replays)
        end.record()
        end.synchronize()
        step.append(start.elapsed_time(end) / args.replays)
    out = {"lanes_log2": args.batch_log2, "depth": args.depth, "width": args.width, "reps": args.reps, "graph_replay": replayed,
           "replayed_step_ms": round(statistics.median(step), 4), "replayed_step_ms_min_max": [round(min(step), 4), round(max(step), 4)]}
    for flag, ts in times.items():
        wall, events = [w for w, _ in ts], [e for _, e in ts]
        out[f"logged_step_wall_ms_compact_log_{flag}"] = round(statistics.median(wall), 3)
        out[f"logged_step_wall_ms_min_max_compact_log_{flag}"] = [round(min(wall), 3), round(max(wall), 3)]
        out[f"logged_step_events_ms_compact_log_{flag}"] = round(statistics.median(events), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
