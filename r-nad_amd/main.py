"""Minimal driver, the counterpart of the reference's main.py:9-81: generate a small 3x3 stochastic tree, save it, then run
R-NaD for a few values of eta on the MI355X.  Lives next to the `environment / learn / nn / util` packages, exactly like the
reference's script lives next to its own, and uses only their reference-compatible API.

    python r-nad_amd/main.py [--updates 8] [--steps 100] [--batch 512] [--compact-log] [--obs-half] [--net convnet --channels 16 --depth 2 [--lazy-rows] [--fused-tail]]
                             [--compact-replay [--replay-batches K]]
"""
import argparse
import logging
from random import random
from time import time

import torch

from environment.tree import Tree
from learn.rnad import RNaD

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=64, help="regularisation updates m (reference: bounds=[64])")
    ap.add_argument("--steps", type=int, default=100, help="learner steps per update (reference: delta_m=[100])")
    ap.add_argument("--batch", type=int, default=2**9)
    ap.add_argument("--etas", type=float, nargs="*", default=[0, 0.2, 0.5, 1])
    ap.add_argument("--compact-log", action="store_true",
                    help="logged steps: statistics from per-row quantities and visit counts, one host sync (RNaD.compact_log)")
    ap.add_argument("--obs-half", action="store_true",
                    help="RNaD.obs_half = True: observations stored as fp16, arithmetic in fp32 (BASELINE.json configs[4]); either net family")
    ap.add_argument("--net", choices=("mlp", "convnet"), default="mlp", help="the reference's MLP line or its ConvNet line (main.py:72)")
    ap.add_argument("--channels", type=int, default=16, help="ConvNet: channels of the CrossConv tower")
    ap.add_argument("--depth", type=int, default=2, help="ConvNet: residual blocks")
    ap.add_argument("--lazy-rows", action="store_true",
                    help="RNaD.lazy_rows = True: the nets run on the rows the batch stages and visits (a ConvNet's opt-in; automatic for the MLP)")
    ap.add_argument("--fused-tail", action="store_true",
                    help="RNaD.fused_optimizer = True: clip + Adam + EMA in one launch that keeps the packed images current (a ConvNet's opt-in; "
                         "the MLP's default)")
    ap.add_argument("--compact-replay", action="store_true",
                    help="RNaD.compact_replay = True: a replay buffer of compact batches with their behaviour's policy rows, learned from "
                         "off-policy by the compact learner (environment.episode.CompactBuffer)")
    ap.add_argument("--replay-batches", type=int, default=1, metavar="K",
                    help="with --compact-replay: stored batches per update (RNaD.replay_batches; the buffer holds at least K)")
    ap.add_argument("--replay-lanes", action="store_true",
                    help="with --compact-replay: RNaD.replay_lanes = True -- every update draws batch_size lanes across ALL stored batches, the "
                         "reference's Buffer.sample, compacted on the GPU; --replay-batches is then ignored")
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO)
    if not torch.cuda.is_available():
        raise SystemExit("this build runs the R-NaD hot path on an MI355X only (no CPU fallback)")

    tree = Tree(
        device=torch.device("cuda"),
        max_actions=3,
        max_transitions=2,
        transition_threshold=0.3,
        depth_bound=4,
        depth_bound_lambda=lambda tree: tree.depth_bound - 1 - 2 * (random() < 0.5),
        desc="3x3 stochastic tree, with depth up to 4",
    )
    tree.generate()
    tree.assert_index_is_tree()
    tree.save("small_tree")
    # tree.load("small_tree")  # instead of generate(), to reuse a tree

    if args.net == "convnet":  # batch_norm=False: the fused tower and the per-row step (a BatchNorm net runs the torch modules per slot)
        net_params = {"type": "ConvNet", "max_actions": tree.max_actions, "channels": args.channels, "depth": args.depth, "batch_norm": False}
    else:
        net_params = {"type": "MLP", "max_actions": tree.max_actions, "width": 2**8}
    timestamp = str(int(time()))
    for idx, eta in enumerate(args.etas):
        same_init_net = None if idx == 0 else f"{timestamp}-eta={args.etas[0]}"  # compare etas from one initial net
        trial = RNaD(
            use_same_init_net_as=same_init_net,
            tree=tree,
            directory_name=f"{timestamp}-eta={eta}",
            device=tree.device,
            wandb=False,
            eta=eta,
            bounds=[args.updates],
            delta_m=[args.steps],
            lr=1 * 10**-3,
            gamma_averaging=0.01,
            batch_size=args.batch,
            logit_clip=2,
            net_params=net_params,
        )
        trial.compact_log = args.compact_log
        trial.obs_half = args.obs_half
        if args.lazy_rows:
            trial.lazy_rows = True
        if args.fused_tail:
            trial.fused_optimizer = True
        if args.compact_replay:
            trial.compact_replay, trial.replay_batches = True, args.replay_batches
            trial.n_batches_per_buffer = max(trial.n_batches_per_buffer, args.replay_batches)
            trial.replay_lanes = args.replay_lanes
        trial.run(log_mod=10, expl_mod=1, checkpoint_mod=args.steps)
        print(f"eta={eta}: NashConv by update:", [round(v, 3) for _, _, v in trial.nashconv_history])
