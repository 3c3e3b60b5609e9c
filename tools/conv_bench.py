#!/usr/bin/env python3
"""Benchmark of the fused ConvNet kernels (csrc/conv_tower.hip) on the BASELINE.json configs[1] tree (depth-6 ternary, 66 431 states):

  (a) rnad_conv_forward (learner + target net) and rnad_conv_backward on all 2S = 132 862 observation rows and on the distinct ones,
      with the share of the fp32-MFMA peak the executed matrix instructions reach;
  (b) the same net as plain torch modules (nn.Conv2d / nn.Linear, autograd) on the same rows, in the same process -- the baseline;
  (c) one default RNaD.train_step at 2^20 lanes for the ConvNet and for the MLP.

    python tools/conv_bench.py [--channels 16] [--depth 2] [--reps 2000] [--rounds 3] [--lanes-log2 20] [--out FILE.md]

--lazy runs another leg instead (default --out profiles/convnet_lazy_rows.md): one default ConvNet train_step with RNaD.lazy_rows off (the
all-rows step) and on (staged actor, target and backward on the visited rows), on the pruned 5x5, 4-outcome configs[3]-shaped tree and on
the configs[1] tree, with the rows each step ran on.  The two trainers of a tree start from the same seed; their windows alternate.

--tail runs a third leg instead (default --out profiles/convnet_tail.md): one default ConvNet train_step with the one-launch optimiser tail
(RNaD.fused_optimizer = True: rnad_conv_optimizer_step, which also keeps the packed images current) off and on -- on the configs[1] tree, and
with lazy rows on the configs[3]-shaped A = 5 tree of --lazy -- each with the kernel launches of one step.

--obs-half runs a fourth leg instead (default --out profiles/convnet_half.md): the forward of net + target and the backward on the
configs[1] tree, all rows and distinct observations, on the fp32 and on the fp16 observation table (the same kernels instantiated on the
element type of the table: rnad_conv_forward_obs / rnad_conv_backward_obs), and one default ConvNet train_step with RNaD.obs_half off
and on.  The windows of the two tables alternate; nothing gates the ratio.

Times are device events around `reps` back-to-back calls after a warm-up of the same shapes; fused and torch windows alternate.  Needs the GPU: there is no CPU path.
"""
import argparse
import copy
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "r-nad_amd"))
import torch  # noqa: E402

import rnad_hip  # noqa: E402
from environment.episode import Buffer  # noqa: E402
from environment.tree import Tree  # noqa: E402
from learn.rnad import RNaD  # noqa: E402
from nn.net import ConvNet  # noqa: E402

PEAK_F32_MFMA = 157.3e12  # MI355X fp32 matrix peak, FLOP/s


WINDOW_MS = 500.0  # a timed window lasts about this long: well above clock and scheduler noise


def timeit(fn, max_reps):
    """ms per call over one window of back-to-back calls: 3 warm-up calls, one calibration call, then as many calls as fill
    WINDOW_MS (at least 3, at most max_reps) between two device events."""
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
    return a.elapsed_time(b) / reps


def mfma_flops(A, Ch, depth):
    """Executed MFMA flops per row: (forward, backward).  A 16x16x4 instruction is 2048 flops over 16 rows."""
    Mt, KS, KS0 = Ch * A // 16, Ch * A // 4, (2 * A + 3) // 4
    conv = 2 * A * Mt * KS * 128.0
    pre = 2 * A * Mt * KS0 * 128.0
    fwd = pre + 2 * depth * conv
    wgrad = 2 * Mt * Mt * 4 * A * 128.0
    wgrad_pre = 2 * Mt * 1 * 4 * A * 128.0
    return fwd, fwd + 2 * depth * (conv + wgrad) + wgrad_pre


def lazy_leg(args, dev):
    """One default ConvNet train_step with lazy_rows off and on, per tree: ms per step (mean and spread over alternating windows) and the
    rows the actor / the target and the backward ran on."""
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_conv_lazy_")
    B = 1 << args.lanes_log2
    out = args.out or os.path.join(ROOT, "profiles", "convnet_lazy_rows.md")
    lines = [f"# ConvNet train_step with lazy rows off / on, channels = {args.channels}, depth = {args.depth}, 2^{args.lanes_log2} lanes", "",
             f"Device events around back-to-back steps; every window lasts about {WINDOW_MS / 1000:g} s after 8 priming steps of its trainer (eager warm-up "
             f"and the graph capture); the windows of the two trainers alternate, {args.rounds} rounds; a figure is the mean over the rounds, with the "
             "smallest and the largest round beside it.", "",
             "| tree | 2S rows | lazy_rows | ms per step (min .. max) | actor rows (staged_rows) | target + backward rows (last_rows) | hipGraph replay |",
             "|---|---|---|---|---|---|---|"]
    trees = (("configs[3] shape: 5x5, 4 outcomes, depth 8, threshold 0.1, pruned 7/8", dict(max_actions=5, max_transitions=4, depth_bound=8, transition_threshold=0.1), (7, 8)),
             ("configs[1]: 3x3, depth 6", dict(max_actions=3, max_transitions=1, depth_bound=6, transition_threshold=0.0), (0, 0)))
    ratios = []
    for what, kw, prune in trees:
        tree = Tree(device=dev, **kw)
        tree.generate_native(seed=0, prune=prune)
        handle = tree.handle()
        A, S2 = tree.max_actions, 2 * handle.S
        legs = {}
        for lazy in (False, True):
            torch.manual_seed(0)
            rn = RNaD(tree=tree, device=dev, directory_name=f"lazy_{A}_{lazy}", batch_size=B, eta=0.2, b1_adam=0.0, lr=5e-5,
                      net_params={"type": "ConvNet", "max_actions": A, "channels": args.channels, "depth": args.depth, "batch_norm": False})
            rn.initialize()
            rn.lazy_rows = lazy
            buf = Buffer(1)

            def step(rn=rn, buf=buf):
                rn.train_step(buf, alpha=0.5)
                rn.total_steps += 1

            for _ in range(8):
                step()
            torch.cuda.synchronize()
            legs[lazy] = (rn, step, [])
        for _ in range(args.rounds):
            for lazy in (False, True):
                legs[lazy][2].append(timeit(legs[lazy][1], args.steps))
        for lazy in (False, True):
            rn, _, ms = legs[lazy]
            staged = getattr(rn.last_episodes, "staged_rows", None) if lazy else None
            took = staged is not None
            actor = "+".join(str(int(r.count.item())) for r in staged) if took else str(S2)
            visited = int(rn.last_rows.count.item()) if (took and rn.last_rows is not None) else S2
            replay = bool(getattr(rn, "_graph", None) and rn._graph.get("graph") is not None)
            mean = sum(ms) / len(ms)
            lines.append(f"| {what} | {S2} | {'on' if lazy else 'off'}{'' if took == lazy else ' (NOT TAKEN)'} | {mean:.3f} ({min(ms):.3f} .. {max(ms):.3f}) | "
                         f"{actor} | {visited} | {replay} |")
            print(lines[-1], flush=True)
        off, on = (sum(legs[k][2]) / len(legs[k][2]) for k in (False, True))
        ratios.append(f"- {what}: all-rows step / lazy step = {off / on:.2f}x ({off:.3f} ms / {on:.3f} ms).")
        legs.clear()
        del tree, handle
        torch.cuda.empty_cache()
    lines += ["", "`lazy_rows` off is the step of the commit before this leg existed (every net on all 2S rows); the ratio against it:", ""] + ratios
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


def launches_of(step):
    """Device kernels of one EAGER call of `step`, counted by torch's profiler (None where it cannot trace the device)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as err:  # the count is a by-product of the leg
        print(f"launch count not taken: {err}", flush=True)
        return None


def tail_leg(args, dev):
    """One default ConvNet train_step with the one-launch optimiser tail off and on, per tree: ms per step (mean and spread over
    alternating windows) and the kernel launches of one eager step."""
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_conv_tail_")
    B = 1 << args.lanes_log2
    out = args.out or os.path.join(ROOT, "profiles", "convnet_tail.md")
    lines = [f"# ConvNet train_step with the one-launch optimiser tail off / on, channels = {args.channels}, depth = {args.depth}, 2^{args.lanes_log2} lanes", "",
             f"Build {rnad_hip.source_hash()}.  Device events around back-to-back steps; every window lasts about {WINDOW_MS / 1000:g} s after 8 priming steps of "
             f"its trainer (eager warm-up and the graph capture); the windows of the two trainers alternate, {args.rounds} rounds; a figure is the mean over "
             "the rounds, with the smallest and the largest round beside it.  Launches: device kernels of one eager step of the same trainer after the "
             "timed windows, counted by torch's profiler.", "",
             "| tree | lazy_rows | fused tail | ms per step (min .. max) | launches per eager step | tail in use | hipGraph replay |",
             "|---|---|---|---|---|---|---|"]
    trees = (("configs[1]: 3x3, depth 6", dict(max_actions=3, max_transitions=1, depth_bound=6, transition_threshold=0.0), (0, 0), None),
             ("configs[3] shape: 5x5, 4 outcomes, depth 8, threshold 0.1, pruned 7/8",
              dict(max_actions=5, max_transitions=4, depth_bound=8, transition_threshold=0.1), (7, 8), True))
    ratios = []
    for what, kw, prune, lazy in trees:
        tree = Tree(device=dev, **kw)
        tree.generate_native(seed=0, prune=prune)
        A = tree.max_actions
        legs = {}
        for fused in (False, True):
            torch.manual_seed(0)
            rn = RNaD(tree=tree, device=dev, directory_name=f"tail_{A}_{fused}", batch_size=B, eta=0.2, b1_adam=0.0, lr=5e-5,
                      net_params={"type": "ConvNet", "max_actions": A, "channels": args.channels, "depth": args.depth, "batch_norm": False})
            rn.initialize()
            rn.lazy_rows, rn.fused_optimizer = lazy, fused
            buf = Buffer(1)

            def step(rn=rn, buf=buf):
                rn.train_step(buf, alpha=0.5)
                rn.total_steps += 1

            for _ in range(8):
                step()
            torch.cuda.synchronize()
            legs[fused] = (rn, step, [])
        for _ in range(args.rounds):
            for fused in (False, True):
                legs[fused][2].append(timeit(legs[fused][1], args.steps))
        for fused in (False, True):
            rn, step, ms = legs[fused]
            replay = bool(getattr(rn, "_graph", None) and rn._graph.get("graph") is not None)
            in_use = rn._fused_tail() is not None
            rn.use_graph = False  # (one eager step, for the launch count)
            launches = launches_of(step)
            mean = sum(ms) / len(ms)
            lines.append(f"| {what} | {'on' if lazy else 'off'} | {'on' if fused else 'off'} | {mean:.3f} ({min(ms):.3f} .. {max(ms):.3f}) | "
                         f"{'not counted' if launches is None else launches} | {in_use} | {replay} |")
            print(lines[-1], flush=True)
        off, on = (sum(legs[k][2]) / len(legs[k][2]) for k in (False, True))
        ratios.append(f"- {what}: tail off / tail on = {off / on:.3f}x ({off:.3f} ms / {on:.3f} ms).")
        legs.clear()
        del tree
        torch.cuda.empty_cache()
    lines += ["", "Tail off is the step of the same build with RNaD.fused_optimizer unset (rnad_clip_grad_norm, torch's fused Adam, two _foreach EMA "
              "launches and two rnad_conv_pack launches on the next step); the ratio against it:", ""] + ratios
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


def spread(ms):
    return f"{sum(ms) / len(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f})"


def half_leg(args, dev):
    """The tower kernels and one default ConvNet train_step on the fp32 and on the fp16 observation table: ms (mean and spread over
    alternating windows) per side, and the fp16 / fp32 ratio."""
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_conv_half_")
    out = args.out or os.path.join(ROOT, "profiles", "convnet_half.md")
    torch.manual_seed(0)
    A = 3
    tree = Tree(device=dev, max_actions=A, max_transitions=1, depth_bound=6, transition_threshold=0.0)
    tree.generate_native(seed=0)
    handle = tree.handle()
    tables = {False: handle.observations_table(False), True: handle.observations_table(True)}
    dedups = {False: handle.obs_dedup(False), True: handle.obs_dedup(True)}
    N = tables[False].shape[0]
    shape = (A, args.channels, args.depth)
    net = ConvNet(*shape, batch_norm=False, device=dev)
    target = copy.deepcopy(net)
    assert net._fusable(), "this shape is declined by rnad_conv_supported: nothing to time"
    packed, packed_t = net.pack(), target.pack()
    dl, dv = torch.randn((N, A), device=dev), torch.randn((N, 1), device=dev)
    lines = [f"# ConvNet tower kernels on an fp32 and on an fp16 observation table, A = {A}, channels = {args.channels}, depth = {args.depth}, "
             f"configs[1] tree ({N} rows)", "",
             f"Build {rnad_hip.source_hash()}.  Device events around back-to-back calls; every window lasts about {WINDOW_MS / 1000:g} s after a warm-up of "
             f"the same shapes; the windows of the two tables alternate, {args.rounds} rounds; a figure is the mean over the rounds, with the smallest "
             "and the largest round beside it.  The fp16 kernels load the table as `__half2` pairs, converted with `__half22float2` as the "
             "tile is staged; the activations and all arithmetic are fp32 on both sides.", "",
             "| what | rows (fp32 / fp16 table) | fp32 table ms (min .. max) | fp16 table ms (min .. max) | fp16 / fp32 |", "|---|---|---|---|---|"]
    notes = []

    def row(what, rows, ms):
        ratio = (sum(ms[True]) / len(ms[True])) / (sum(ms[False]) / len(ms[False]))
        lines.append(f"| {what} | {rows} | {spread(ms[False])} | {spread(ms[True])} | {ratio:.3f} |")
        print(lines[-1], flush=True)
        # slower by more than the rounds of either side differ among themselves
        noise = max(max(ms[k]) - min(ms[k]) for k in (False, True))
        if sum(ms[True]) / len(ms[True]) - sum(ms[False]) / len(ms[False]) > noise:
            notes.append(f"- {what}: the fp16 table is SLOWER by more than the spread between rounds ({ratio:.3f}x).")

    for what, distinct in (("all rows", False), ("distinct observations", True)):
        lives = {h: (dedups[h].uniq if distinct else None) for h in (False, True)}
        counts = {h: (dedups[h].n_unique if distinct else N) for h in (False, True)}

        def forward(h):
            for p in (packed, packed_t):
                rnad_hip.conv_forward(p, *shape, tables[h], live=lives[h], zero_rest=False)

        def backward(h):
            rnad_hip.conv_backward(packed, net._weights(), *shape, tables[h], dl, dv, live=lives[h], capacity=counts[h] if distinct else None)

        for kind, fn in (("forward, net + target", forward), ("backward", backward)):
            ms = {False: [], True: []}
            for _ in range(args.rounds):
                for h in (False, True):
                    ms[h].append(timeit(lambda: fn(h), args.reps))
            row(f"{kind}, {what}", f"{counts[False]} / {counts[True]}", ms)
    B = 1 << args.lanes_log2
    legs = {}
    for h in (False, True):
        torch.manual_seed(0)
        rn = RNaD(tree=tree, device=dev, directory_name=f"half_{h}", batch_size=B, eta=0.2, b1_adam=0.0, lr=5e-5,
                  net_params={"type": "ConvNet", "max_actions": A, "channels": args.channels, "depth": args.depth, "batch_norm": False})
        rn.initialize()
        rn.obs_half = h
        buf = Buffer(1)

        def step(rn=rn, buf=buf):
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1

        for _ in range(8):  # eager warm-up and the graph capture
            step()
        torch.cuda.synchronize()
        legs[h] = (rn, step, [])
    for _ in range(args.rounds):
        for h in (False, True):
            legs[h][2].append(timeit(legs[h][1], args.steps))
    replay = all(bool(getattr(legs[h][0], "_graph", None) and legs[h][0]._graph.get("graph") is not None) for h in (False, True))
    row(f"one default train_step, 2^{args.lanes_log2} lanes (hipGraph replay on both sides: {replay})", f"{N} / {N}", {h: legs[h][2] for h in (False, True)})
    lines += ["", "Nothing gates the ratio: the tower is bound by LDS traffic, and the table is read once per tile.  The fp16 table is half the "
              f"bytes of the fp32 one ({tables[True].numel() * 2} against {tables[False].numel() * 4})."]
    lines += [""] + (notes or ["On no line is the fp16 table slower than the fp32 table by more than the spread between rounds."])
    text = "\n".join(lines) + "\n"
    # the registers / scratch of the instantiations are read from the code object's metadata, not measured here: that section is kept
    marker, kept = "## Code object resources", ""
    if os.path.exists(out):
        old = open(out).read()
        kept = old[old.index(marker):] if marker in old else ""
    with open(out, "w") as f:
        f.write(text + ("\n" + kept if kept else ""))
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2000, help="most back-to-back calls per timed window (a window lasts about 0.5 s)")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of a fused window and a torch window")
    ap.add_argument("--lanes-log2", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--torch-chunk", type=int, default=32768, help="rows per call of the torch modules' backward (gradients accumulate)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch-module baseline out")
    ap.add_argument("--lazy", action="store_true", help="only the lazy-rows leg: a ConvNet train_step with lazy_rows off and on, on two trees")
    ap.add_argument("--obs-half", action="store_true", help="only the fp16-table leg: the tower kernels and a ConvNet train_step on the fp32 and the fp16 observation table")
    ap.add_argument("--tail", action="store_true", help="only the optimiser-tail leg: a ConvNet train_step with RNaD.fused_optimizer off and on, on two trees")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "conv_bench needs the MI355X"
    dev = torch.device("cuda:0")
    if args.lazy:
        return lazy_leg(args, dev)
    if args.tail:
        return tail_leg(args, dev)
    if args.obs_half:
        return half_leg(args, dev)
    torch.manual_seed(0)
    A = 3
    tree = Tree(device=dev, max_actions=A, max_transitions=1, depth_bound=6, transition_threshold=0.0)
    tree.generate_native(seed=0)
    handle = tree.handle()
    table = handle.observations_table(False)
    dedup = handle.obs_dedup(False)
    N = table.shape[0]
    shape = (A, args.channels, args.depth)
    net = ConvNet(*shape, batch_norm=False, device=dev)
    target = copy.deepcopy(net)
    assert net._fusable(), "this shape is declined by rnad_conv_supported: nothing to time"
    packed, packed_t = net.pack(), target.pack()
    dl, dv = torch.randn((N, A), device=dev), torch.randn((N, 1), device=dev)
    fwd_flop, bwd_flop = mfma_flops(*shape)
    title = f"# ConvNet tower kernels, A = {A}, channels = {args.channels}, depth = {args.depth}, configs[1] tree ({N} rows, {dedup.n_unique} distinct)"
    report = {"fused": {}, "torch": {}, "steps": []}

    def say(msg):
        print(msg, flush=True)

    def write_out():
        """The report so far (rewritten after every section, so that a run that is cut short leaves what it measured)."""
        lines = [title, "", "| what | rows | fused kernels ms | torch modules ms | speed-up | fp32-MFMA share of peak |", "|---|---|---|---|---|---|"]
        slow = False
        for key, (n_rows, ms, flop) in report["fused"].items():
            base = report["torch"].get(key)
            share = flop * n_rows / (ms * 1e-3) / PEAK_F32_MFMA
            slow = slow or (base is not None and ms > base)
            lines.append(f"| {key} | {n_rows} | {ms:.4f} | {'not measured' if base is None else f'{base:.4f}'} | "
                         f"{'-' if base is None else f'{base / ms:.1f}x'} | {100 * share:.1f} % |")
        lines += ["", f"The torch backward runs in chunks of {args.torch_chunk} rows with accumulated gradients (the convolution library's first-call "
                  "search of backward algorithms grows with the batch: 17 s at 4 096 rows, 107 s at 32 768); its forward runs on all rows at once."]
        lines += ["", f"| one default train_step, 2^{args.lanes_log2} lanes | ms per step | per-row step taken | hipGraph replay |", "|---|---|---|---|"]
        lines += report["steps"]
        if report["torch"]:
            lines += ["", ("A fused figure above is SLOWER than the torch modules: that shape must be sent to the fallback (ConvNet._fusable / "
                           "rnad_conv_supported)." if slow else
                           "The fused kernels are faster than the torch modules on every line, so rnad_conv_supported keeps this shape on the fused path.")]
        text = "\n".join(lines) + "\n"
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return text

    def torch_forward(obs):
        with torch.no_grad():
            for n in (net, target):
                h = n._tower(obs)
                n.policy(h), n.value(h)

    def torch_backward(obs, gl, gv):
        # in chunks of --torch-chunk rows, gradients accumulated: the convolution library searches its backward algorithms on the first
        # call of every batch size, and that search grows with the batch (measured here: 17 s at 4 096 rows, 107 s at 32 768)
        net.zero_grad(set_to_none=True)
        for r0 in range(0, obs.shape[0], args.torch_chunk):
            h = net._tower(obs[r0:r0 + args.torch_chunk])
            torch.autograd.backward([net.policy(h), net.value(h)], [gl[r0:r0 + args.torch_chunk], gv[r0:r0 + args.torch_chunk]])

    cases = (("all rows", None, N), ("distinct observations", dedup.uniq, dedup.n_unique))
    # (a) the fused kernels and (b) the same net as torch modules on the same rows, ALTERNATING in rounds of `reps` calls each (the first,
    # untimed, torch call of every shape includes the convolution library's search); the figure of a side is the mean over its rounds
    for what, live, n_rows in cases:
        sel = slice(None) if live is None else live.rows[:n_rows].long()
        obs_sel, dl_sel, dv_sel = table[sel].contiguous(), dl[sel].contiguous(), dv[sel].contiguous()

        def fused_forward():
            for p in (packed, packed_t):
                rnad_hip.conv_forward(p, *shape, table, live=live, zero_rest=False)

        def fused_backward():
            rnad_hip.conv_backward(packed, net._weights(), *shape, table, dl, dv, live=live, capacity=None if live is None else n_rows)

        for kind, fused, base, flop in (("forward, net + target", fused_forward, lambda: torch_forward(obs_sel), 2 * fwd_flop),
                                        ("backward", fused_backward, lambda: torch_backward(obs_sel, dl_sel, dv_sel), bwd_flop)):
            key = f"{kind}, {what}"
            ms_f, ms_t = [], []
            for _ in range(args.rounds):
                ms_f.append(timeit(fused, args.reps))
                if not args.skip_torch:
                    ms_t.append(timeit(base, args.reps))
            report["fused"][key] = (n_rows, sum(ms_f) / len(ms_f), flop)
            say(f"fused {key} ({n_rows} rows): {report['fused'][key][1]:.4f} ms  rounds {['%.4f' % x for x in ms_f]}")
            if ms_t:
                report["torch"][key] = sum(ms_t) / len(ms_t)
                say(f"torch {key} ({n_rows} rows): {report['torch'][key]:.4f} ms  rounds {['%.4f' % x for x in ms_t]}")
            write_out()
    # (c) one default train_step
    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_conv_bench_")
    B = 1 << args.lanes_log2
    for name, params in (("ConvNet", {"type": "ConvNet", "max_actions": A, "channels": args.channels, "depth": args.depth, "batch_norm": False}),
                         ("MLP", {"type": "MLP", "max_actions": A, "width": 256})):
        rn = RNaD(tree=tree, device=dev, directory_name=f"bench_{name}", batch_size=B, eta=0.2, b1_adam=0.0, lr=5e-5, net_params=params)
        rn.initialize()
        buf = Buffer(1)

        def step():
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1

        for _ in range(5):  # eager warm-up and the graph capture
            step()
        ms = timeit(step, args.steps)
        mode = rn._tabular_mode(2 * handle.max_depth, B) is True
        replay = bool(getattr(rn, "_graph", None) and rn._graph.get("graph") is not None)
        report["steps"].append(f"| {name} | {ms:.4f} | {mode} | {replay} |")
        say(f"train_step {name}: {ms:.4f} ms (per-row step {mode}, graph replay {replay})")
        del rn, buf
    print(write_out())


if __name__ == "__main__":
    main()
