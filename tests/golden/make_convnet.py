#!/usr/bin/env python3
"""ConvNet fixtures from the REFERENCE (baskuit/R-NaD nn/net.py:88-269) on the golden trees.

Runs only in the build container (imports the reference like make_golden.py); writes data only:

  convnet_{small,a5,c1}.npz   a batch_norm=False ConvNet with random non-zero biases: state-dict arrays (w_<key>) and key order, the 2S
                              observation rows of the tree (row player rows, then column player rows: States.observations), the
                              reference's logits / policy / value on them in fp32, a seeded dlogits / dv and every parameter's
                              gradient (g_<key>) from the reference net under autograd in fp64.  `small` also carries the same data for a
                              batch_norm=True net in eval mode with non-trivial running statistics (bn_ prefix) and
                              NashConvData.get_nashconv_from_net of the batch_norm=False net.
  curve_convnet_small.npz     NashConv after each update of the reference's RNaD with the `small` ConvNet, 3 seeds
                              (`python make_convnet.py curve`; asserts that every seed falls by at least 0.30).
"""
import os
import sys

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets up the reference import, stubs and seeding helpers)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
torch.multinomial = mg._orig_multinomial  # plain reference sampling here: no recording needed

SHAPES = {"small": dict(channels=16, depth=2, seed=31), "a5": dict(channels=16, depth=1, seed=32), "c1": dict(channels=32, depth=3, seed=33)}
TREE_KW = {"small": dict(max_actions=3, max_transitions=2, depth_bound=4), "a5": dict(max_actions=5, max_transitions=2, depth_bound=2),
           "c1": dict(max_actions=2, max_transitions=1, depth_bound=3)}


def load_tree(name):
    g = np.load(os.path.join(HERE, f"tree_{name}.npz"))
    tree = mg.ref_tree.Tree(**TREE_KW[name])
    for key, attr in (("index", "index_tensor"), ("value", "value_tensor"), ("chance", "chance_tensor"),
                      ("expected_value", "expected_value_tensor"), ("legal", "legal_tensor"), ("root_value", "root_value_tensor"),
                      ("solution", "solution_tensor")):
        setattr(tree, attr, torch.tensor(g[key]))
    tree.hash = 1234
    return tree


def observation_rows(tree):
    S = tree.expected_value_tensor.shape[0]
    states = mg.ref_episode.States(tree, S)
    states.indices = torch.arange(S, dtype=torch.int32)
    rows = []
    for player in (0, 1):
        states.player_to_move = torch.full((S,), player, dtype=torch.long)
        rows.append(states.observations())
    return torch.cat(rows, 0).contiguous()


def randomise(net, bn):
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
        if bn:
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.copy_(torch.randn_like(m.running_mean) * 0.2)
                    m.running_var.copy_(torch.rand_like(m.running_var) + 0.5)
                    m.weight.copy_(torch.rand_like(m.weight) + 0.5)


def net_data(A, channels, depth, bn, obs, dlogits, dv, prefix):
    net = mg.ref_net.ConvNet(A, channels, depth=depth, batch_norm=bn)
    randomise(net, bn)
    net.eval()
    with torch.no_grad():
        logits, policy, value, _ = net.forward(obs.clone())
    out = {prefix + "keys": np.array(list(net.state_dict().keys()))}
    for k, v in net.state_dict().items():
        out[prefix + "w_" + k.replace(".", "_")] = v.detach().numpy().copy()
    out.update({prefix + "logits": logits.numpy(), prefix + "policy": policy.numpy(), prefix + "value": value.numpy()})
    net64 = mg.ref_net.ConvNet(A, channels, depth=depth, batch_norm=bn, dtype=torch.float64)
    net64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in net.state_dict().items()})
    net64.eval()
    l64, _, v64, _ = net64.forward(obs.double())
    ((l64 * dlogits.double()).sum() + (v64 * dv.double()).sum()).backward()
    for k, p in net64.named_parameters():
        out[prefix + "g_" + k.replace(".", "_")] = p.grad.numpy().copy()
    return net, out


def make_nets():
    for name, spec in SHAPES.items():
        tree = load_tree(name)
        A = tree.max_actions
        mg.seed_all(spec["seed"])
        obs = observation_rows(tree)
        N = obs.shape[0]
        dlogits, dv = torch.randn(N, A), torch.randn(N, 1)
        net, arrays = net_data(A, spec["channels"], spec["depth"], False, obs, dlogits, dv, "")
        arrays.update(obs=obs.numpy(), dlogits=dlogits.numpy(), dv=dv.numpy(), max_actions=A, channels=spec["channels"], depth=spec["depth"])
        if name == "small":
            _, bn = net_data(A, spec["channels"], spec["depth"], True, obs, dlogits, dv, "bn_")
            arrays.update(bn)
            net.device = torch.device("cpu")
            data = mg.ref_metric.NashConvData(tree)
            data.get_nashconv_from_net(tree, net)
            arrays["nashconv"] = (data.row_best[1] + data.col_best[1]).item()
        mg.save("convnet_" + name, **arrays)


M, DELTA, B, SEEDS = 12, 100, 512, (0, 1, 2)


def make_curve():
    tree = load_tree("small")
    curves = []
    for seed in SEEDS:
        mg.seed_all(2000 + seed)
        rn = mg.ref_rnad.RNaD(tree=tree, device=torch.device("cpu"), directory_name=f"curve_conv{seed}", wandb=False, eta=0.2, bounds=[M],
                              delta_m=[DELTA], lr=1e-3, gamma_averaging=0.01, batch_size=B, logit_clip=2, b1_adam=0.0,
                              net_params={"type": "ConvNet", "max_actions": 3, "channels": 16, "depth": 2, "batch_norm": False})
        ncs = []
        orig = rn._RNaD__nashconv

        def rec():
            v = orig()
            ncs.append(v)
            return v

        rn._RNaD__nashconv = rec
        rn._RNaD__initialize()
        rn._RNaD__nashconv()  # untrained net (the reference logs from m = 1 on)
        rn._RNaD__resume(checkpoint_mod=10**9, expl_mod=1, log_mod=10**9)
        rn._RNaD__nashconv()
        curves.append(list(ncs))
        print(seed, [round(x, 3) for x in ncs], flush=True)
        assert len(ncs) == M + 1
        assert ncs[-1] <= ncs[0] - 0.30, f"seed {seed}: NashConv fell from {ncs[0]:.3f} to {ncs[-1]:.3f} only: lengthen the run"
    np.savez_compressed(os.path.join(HERE, "curve_convnet_small.npz"), nashconv=np.array(curves), M=M, delta_m=DELTA, batch=B, eta=0.2,
                        lr=1e-3, gamma_averaging=0.01, seeds=np.array(SEEDS))


if __name__ == "__main__":
    if "curve" in sys.argv[1:]:
        make_curve()
    else:
        make_nets()
