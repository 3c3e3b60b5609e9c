#!/usr/bin/env python3
"""What a replay buffer costs per training step, and what RNaD.compact_replay makes of it: RNaD.train_step on the BASELINE configs[1]
tree (A = 3, one outcome, depth 6: 132 862 rows) at 2^20 lanes, in seven legs --

  (a)  the default on-policy step (a one-batch buffer refilled every step; captured as a hipGraph);
  (b)  environment.episode.Buffer with n_batches_per_buffer = 4: the off-policy path as it stands (dense batches, Buffer.sample /
       Episodes.collate, the per-slot kernels);
  (c)  compact_replay at the same settings (CompactBuffer, one stored batch per update);
  (d)  (c) with buffer_mod = 4: a rollout every fourth step;
  (b4) (b) with buffer_mod = 4, the counterpart of (d);
  (e)  compact_replay with replay_lanes: 2^20 lanes drawn across the 4 stored batches per step (Buffer's own draw, compacted on the
       GPU: rnad_bucket_draw_lanes), one learner launch per contributing batch;
  (e4) (e) with buffer_mod = 4 --

and the bytes one stored batch holds in (b) and in (c).  Every step is timed with a pair of device events; a leg's figure is the median
of --steps warm steps after --warmup (min and max beside it), and the whole round of legs is repeated so that the run-to-run spread
is visible next to the differences.  Writes a markdown report (default profiles/compact_replay.md).  Needs the MI355X.

    python tools/replay_bench.py [--batch-log2 20] [--depth 6] [--steps 30] [--warmup 10] [--rounds 2] [--out profiles/compact_replay.md]
                                 [--kernels kernel_stats.csv]

--kernels: the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/replay_bench.py --legs e ...`, a
run of its own; the report then lists the three draw launches beside the learner and the behaviour records of that run.
"""
import argparse
import os
import random
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "r-nad_amd"))
import numpy  # noqa: E402
import torch  # noqa: E402

from environment.episode import Buffer, CompactBuffer  # noqa: E402
from environment.tree import Tree  # noqa: E402
from learn.rnad import RNaD  # noqa: E402

LEGS = {
    "a": dict(title="default on-policy step", n_batches=1, buffer_mod=1, compact=False),
    "b": dict(title="Buffer, 4 batches", n_batches=4, buffer_mod=1, compact=False),
    "c": dict(title="compact_replay, 4 batches", n_batches=4, buffer_mod=1, compact=True),
    "d": dict(title="compact_replay, 4 batches, buffer_mod = 4", n_batches=4, buffer_mod=4, compact=True),
    "b4": dict(title="Buffer, 4 batches, buffer_mod = 4", n_batches=4, buffer_mod=4, compact=False),
    "e": dict(title="compact_replay + replay_lanes, 4 batches", n_batches=4, buffer_mod=1, compact=True, lanes=True),
    "e4": dict(title="compact_replay + replay_lanes, 4 batches, buffer_mod = 4", n_batches=4, buffer_mod=4, compact=True, lanes=True),
}


def tensors_of(obj, seen):
    """Bytes of the distinct storages behind the tensors `obj` holds directly (attributes, tuples / lists of them, tensor attributes)."""
    total = 0
    stack = [obj]
    while stack:
        x = stack.pop()
        if torch.is_tensor(x):
            st = x.untyped_storage()
            if st.data_ptr() not in seen:
                seen.add(st.data_ptr())
                total += st.nbytes()
            stack.extend(v for v in getattr(x, "__dict__", {}).values() if torch.is_tensor(v))
        elif isinstance(x, (tuple, list)):
            stack.extend(x)
        elif isinstance(x, dict):
            stack.extend(x.values())
    return total


def dense_batch_bytes(ep):
    """What one batch in a Buffer keeps alive: its own fields (whatever has been materialised by now), its trajectory's buffers, the
    records it was played with (and their policy rows) and the work list."""
    seen = set()
    total = tensors_of(dict(ep.__dict__), seen)
    for name in ("_traj", "buckets", "states"):
        o = ep.__dict__.get(name)
        if o is not None:
            total += tensors_of(dict(getattr(o, "__dict__", {})), seen)
    if ep.__dict__.get("_compact") is not None:
        total += tensors_of(list(ep._compact[1:]), seen)
    return total


def make(leg, tree, dev, batch):
    cfg = LEGS[leg]
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_replay_bench_")
    torch.manual_seed(0)
    numpy.random.seed(0)
    random.seed(0)
    rn = RNaD(tree=tree, device=dev, directory_name=f"leg_{leg}", batch_size=batch, eta=0.2, b1_adam=0.0,
              n_batches_per_buffer=cfg["n_batches"], buffer_mod=cfg["buffer_mod"],
              net_params={"type": "MLP", "max_actions": tree.max_actions, "width": 256})
    rn.initialize()
    rn.compact_replay = cfg["compact"]
    rn.replay_lanes = cfg.get("lanes", False)
    with torch.no_grad():
        for p in rn.net_reg_.parameters():
            p.mul_(1.001)
    buf = rn.make_buffer()
    assert isinstance(buf, CompactBuffer) == cfg["compact"], f"leg {leg}: compact_replay refused"
    return rn, buf


def run(rn, buf, steps, timed):
    times = []
    for _ in range(steps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rn.train_step(buf, 0.3)
        end.record()
        rn.total_steps += 1
        end.synchronize()
        times.append(start.elapsed_time(end))
    return times if timed else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-log2", type=int, default=20)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", nargs="*", default=list(LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_replay.md"))
    ap.add_argument("--kernels", default=None, help="kernel_stats.csv of a rocprofv3 run of leg (e) alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench: no GPU: nothing here can be measured without the MI355X")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    tree = Tree(device=dev, max_actions=3, max_transitions=1, depth_bound=args.depth, transition_threshold=0.0)
    tree.generate_native(seed=0)
    batch = 1 << args.batch_log2
    S = tree.handle().S
    trainers = {}
    for leg in args.legs:
        trainers[leg] = make(leg, tree, dev, batch)
        run(*trainers[leg], args.warmup, False)
        torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({leg: run(*trainers[leg], args.steps, True) for leg in args.legs})
    stored = {}
    if "b" in trainers:
        stored["b"] = dense_batch_bytes(trainers["b"][1].episodes_buffer[-1])
    if "c" in trainers:
        stored["c"] = trainers["c"][1].slot_bytes()
    graph = {leg: bool(getattr(rn, "_graph", None) and rn._graph.get("graph") is not None) for leg, (rn, _) in trainers.items()}

    lines = ["# Replay buffer: cost per training step, Buffer against compact_replay", "",
             f"`tools/replay_bench.py` on an MI355X: configs[1] shape (A = 3, one outcome, depth {args.depth}: S = {S}, {2 * S} rows), "
             f"2^{args.batch_log2} lanes, MLP of width 256.  Every step is timed with a pair of device events around `RNaD.train_step` "
             f"(rollout when due, sample, learner, backward, optimiser); a figure is the median of {args.steps} warm steps after "
             f"{args.warmup}, with the fastest and the slowest step beside it; the legs run one after the other and the whole round is "
             f"repeated {args.rounds} times (the spread between rounds is the noise to read the differences against).  Host-inclusive: "
             "an eager step's Python is part of it.", "",
             "| leg | step | " + " | ".join(f"round {k + 1}: median (min .. max) ms" for k in range(args.rounds)) + " | hipGraph |",
             "|---|---|" + "---|" * args.rounds + "---|"]
    for leg in args.legs:
        cells = [f"{statistics.median(r[leg]):.3f} ({min(r[leg]):.3f} .. {max(r[leg]):.3f})" for r in rounds]
        lines.append(f"| ({leg}) | {LEGS[leg]['title']} | " + " | ".join(cells) + f" | {'replayed' if graph[leg] else 'eager'} |")
    lines.append("")
    med = {leg: statistics.median([statistics.median(r[leg]) for r in rounds]) for leg in args.legs}
    if "b" in med and "c" in med:
        lines.append(f"(c) against (b): {med['b'] / med['c']:.2f} times {'faster' if med['c'] < med['b'] else 'SLOWER'} "
                     f"({med['b']:.3f} -> {med['c']:.3f} ms per step).")
    if "b4" in med and "d" in med:
        lines.append(f"(d) against (b4): {med['b4'] / med['d']:.2f} times {'faster' if med['d'] < med['b4'] else 'SLOWER'} "
                     f"({med['b4']:.3f} -> {med['d']:.3f} ms per step).")
    if "a" in med and "c" in med:
        lines.append(f"(c) against (a), the on-policy step: {med['c'] / med['a']:.2f} times its time ({med['a']:.3f} -> {med['c']:.3f} ms).")
    def against(x, y, what):
        """Ratio of leg x to leg y: of the medians over the rounds, and round by round (the between-round spread)."""
        per_round = [statistics.median(r[x]) / statistics.median(r[y]) for r in rounds]
        return (f"({x}) against ({y}), {what}: {med[x] / med[y]:.2f} times its time ({med[y]:.3f} -> {med[x]:.3f} ms); round by round "
                + ", ".join(f"{q:.3f}" for q in per_round) + f" (spread {max(per_round) - min(per_round):.3f}).")

    if "e" in med and "b" in med:
        lines.append(f"(e) against (b), the only other path with the reference's draw: {med['b'] / med['e']:.2f} times "
                     f"{'faster' if med['e'] < med['b'] else 'SLOWER'} ({med['b']:.3f} -> {med['e']:.3f} ms per step).")
    if "e" in med and "c" in med:
        lines.append(against("e", "c", "whole batches"))
    if "e" in med and "a" in med:
        lines.append(against("e", "a", "the on-policy step"))
    if "e4" in med and "d" in med:
        lines.append(against("e4", "d", "whole batches at buffer_mod = 4"))
    if "e4" in med and "b4" in med:
        lines.append(f"(e4) against (b4): {med['b4'] / med['e4']:.2f} times {'faster' if med['e4'] < med['b4'] else 'SLOWER'} "
                     f"({med['b4']:.3f} -> {med['e4']:.3f} ms per step).")
    if args.kernels:
        import csv
        import re

        lines += ["", "## The launches of a lane-draw step", "",
                  "`rocprofv3 --kernel-trace --stats` over a run of leg (e) alone (a run of its own: the step times above are not from it).", "",
                  "| kernel | launches | average us | share of the run's kernel time |", "|---|---|---|---|"]
        per_kernel = {}
        for row in csv.DictReader(open(args.kernels)):
            name = re.sub(r"\(anonymous namespace\)::", "", row["Name"])
            if re.search(r"k_draw_|k_bucket_learn_c|k_behaviour_records|k_bucket_finish", name):
                short = re.sub(r"\(.*", "", re.sub(r"^void ", "", name))
                lines.append(f"| `{short}` | {row['Calls']} | {float(row['AverageNs']) / 1e3:.1f} | {float(row['Percentage']):.1f} % |")
                per_kernel[short.split("<")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e3)
        if "k_draw_scan" in per_kernel and "k_bucket_learn_c" in per_kernel:
            steps = per_kernel["k_draw_scan"][0]  # (one scan launch per draw call, one draw call per step with <= 8 stored batches)
            draw = {k: v[1] / steps for k, v in per_kernel.items() if k.startswith("k_draw_")}
            learn = per_kernel["k_bucket_learn_c"][1] / steps
            worst = max(draw, key=draw.get)
            lines += ["", f"Per step: the three draw launches {sum(draw.values()):.1f} us ("
                      + ", ".join(f"`{k}` {v:.1f}" for k, v in sorted(draw.items())) + f"), the learner launches {learn:.1f} us "
                      f"({per_kernel['k_bucket_learn_c'][0] / steps:.2f} per step).  "
                      + (f"The draw costs more than the learner it feeds; `{worst}` is the largest part of it."
                         if sum(draw.values()) > learn else "The draw costs less than the learner it feeds.")]
    lines.append("")
    lines.append("## Bytes held per stored batch")
    lines.append("")
    if "b" in stored:
        lines.append(f"- (b) a batch in `Buffer` (every tensor it keeps alive after the timed steps: the rollout's buffers, the dense fields "
                     f"materialised for `sample` / `collate`, the records it was played with): {stored['b']} B = {stored['b'] / batch:.1f} B per lane.")
    if "c" in stored:
        lines.append(f"- (c) a slot of `CompactBuffer` (relative states, packed actions, one reward, lane ids, work list, counts, and the "
                     f"behaviour's policy rows [2S, 4]): {stored['c']} B = {stored['c'] / batch:.1f} B per lane, of which the policy table is "
                     f"{2 * S * 16} B.")
    lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
