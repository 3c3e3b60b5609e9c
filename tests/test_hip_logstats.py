"""Logged statistics from the compact trajectory (rnad_bucket_log_stats, RNaD.compact_log): per-row statistics weighted with the visits
per row are the reference's per-slot statistics (rnad.py:427-452), at every cut of the tree, and a logged step with the flag on is the
logged step with it off -- same gradients, same parameters, nothing dense built."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("entropy", "entropy_target", "traj_len", "logit_mean", "logit_max")
NINE = {"loss_v", "loss_nerd", "traj_len", "gradient_norm", "logit_mean", "logit_max", "entropy", "entropy_target", "actor_learner_kld"}


@functools.lru_cache(maxsize=None)
def _setup(name):
    """Tree, records of four nets (learner = nets[0], target logits from ANOTHER net) and the per-row statistics in fp64, once per tree."""
    import rnad_hip
    from test_hip_bucket import TREES, _four_nets, _native_tree, _tables

    tree = _native_tree(**TREES[name])
    h = tree.handle()
    A, S = tree.max_actions, h.S
    nets = _four_nets(A, 64, seed=3)
    logit, v, vt, lr, lr_ = _tables(tree, nets, A)
    logit_target = rnad_hip.mlp_forward(nets[1].pack(), 64, h.observations_table(), A, want_value=False)[0].contiguous()
    assert not torch.equal(logit_target, logit)
    hp = rnad_hip.make_learn_params(alpha=0.3, eta=0.2)
    rec, fast = rnad_hip.bucket_records(h, logit, v, vt, lr, lr_, hp, fast=True)
    legal = tree.legal_tensor.cpu().numpy()[:, 0] != 0  # [S, A, A]
    masks = np.concatenate([legal[:, :, 0], legal[:, 0, :]])  # the mover's legal actions per row p * S + s (episode.py:208)
    rows = dict(masks=masks, logit=logit.cpu().numpy().astype(np.float64))
    sums = logit.cpu().numpy()[:, 0].copy()  # sum_r is a per-row fp32 quantity: A - 1 fp32 additions in the order of the actions
    for a in range(1, A):
        sums = (sums + logit.cpu().numpy()[:, a]).astype(np.float32)
    rows["sum"] = sums.astype(np.float64)
    rows["e"] = _row_entropy(rows["logit"], masks)
    return tree, nets, rec, fast, logit_target, rows


def _row_entropy(logit64, masks):
    """e_r = sum_legal pi (log pi - log q), q = 1 / n_r, pi = softmax over the legal actions: fp64 from the fp32 logits."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = np.where(masks, np.exp(logit64), 0.0)
        pi = ex / ex.sum(1, keepdims=True)
        log_q = np.log(1.0 / masks.sum(1))[:, None]
        return np.where(masks, pi * (np.log(pi) - log_q), 0.0).sum(1)


def _expected(rows, e_target, idx, alive, T, B, S):
    """The contract's results from ep.indices / ep.alive and the per-row statistics, fp64."""
    A = rows["logit"].shape[1]
    idx = idx[:T].astype(np.int64)
    slot_rows = idx + (np.arange(T) & 1)[:, None] * S
    c = np.bincount(slot_rows[idx != 0], minlength=2 * S).astype(np.float64)
    N = c.sum()
    used = c > 0
    z = [float(sum(B - int(alive[t]) for t in range(p, T, 2))) for p in (0, 1)]
    sums = rows["sum"]
    total = (c * sums).sum() + z[0] * sums[0] + z[1] * sums[S]
    mean = total / (T * B * A)
    seen = used.copy()
    seen[0] |= z[0] > 0
    seen[S] |= z[1] > 0
    want = {"entropy": (c[used] * rows["e"][used]).sum() / N, "entropy_target": (c[used] * e_target[used]).sum() / N, "traj_len": N / B,
            "logit_mean": mean, "logit_max": np.abs(rows["logit"][seen] - mean).max()}
    return want, N, total, (c * np.abs(sums)).sum() + z[0] * abs(sums[0]) + z[1] * abs(sums[S])


def _play(name, monkeypatch, cut, B=6000, seed=11):
    import rnad_hip
    from environment.episode import Episodes

    tree, nets, rec, fast, logit_target, rows = _setup(name)
    h = tree.handle()
    if cut is None:
        monkeypatch.delenv("RNAD_BUCKET_ROWS", raising=False)
    else:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(cut))
        if rnad_hip.bucket_plan(h, B) is None:
            pytest.skip(f"a table of {cut} rows does not fit this tree")
    ep = Episodes(tree, B, seed=seed, lane_offset=5)
    ep.generate(nets[0], tabular=True, bucketed=True, trim=False, store_values=False, compact=True,
                policy_table=(rec, rnad_hip.policy_column(tree.max_actions)))
    assert ep._compact is not None
    return ep


def _check(got, want, key):
    print(f"{key}: got {got!r} want {want!r} |diff| {abs(got - want):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * max(1.0, abs(want)), err_msg=key)


def _against_fp64(name, ep, T, fresh=True):
    import rnad_hip

    tree, nets, rec, fast, logit_target, rows = _setup(name)
    h = tree.handle()
    A, S, B = tree.max_actions, h.S, ep.batch_size
    out = rnad_hip.bucket_log_stats(h, ep.buckets, ep._compact[0], T, rec, logit_target)
    if fresh:  # (a batch nothing has asked for the dense views of)
        assert ep.__dict__.get("_indices") is None and ep._compact[0].policy is None, "the statistics must not build anything dense"
    host = out.cpu().numpy()
    got = rnad_hip.log_stats_to_dict(host.tolist(), T, B, A)
    e_target = _row_entropy(logit_target.cpu().numpy().astype(np.float64), rows["masks"])
    alive = ep.alive.cpu().numpy()
    want, N, total, scale = _expected(rows, e_target, ep.indices.cpu().numpy(), alive, T, B, S)
    assert host[3] == float(alive[:T].sum()) == N, "the slot count is an integer sum: exact"
    np.testing.assert_allclose(host[4], total, rtol=0, atol=1e-11 * scale, err_msg="sum of the logits over all T * B slots (fp64 sums)")
    for key in KEYS:
        _check(got[key], want[key], key)
    print(f"actor_learner_kld: got {got['actor_learner_kld']!r}")
    np.testing.assert_allclose(got["actor_learner_kld"], 0.0, rtol=0, atol=1e-6, err_msg="actor_learner_kld")
    return got


@pytest.mark.parametrize("cut", (None, 40, 8, 2))
@pytest.mark.parametrize("name", ("ternary4", "pruned", "a5c4", "binary"))
def test_statistics_are_the_per_slot_ones_in_fp64(name, cut, monkeypatch):
    """Every cut: upper-state buckets, runs of several sibling subtrees, terminal buckets and (where a cut reaches them) two-byte states."""
    ep = _play(name, monkeypatch, cut)
    _against_fp64(name, ep, ep.t_eff + 1)


def test_shorter_window(monkeypatch):
    """T = T_cap - 2: the absorbed slots' share and the denominators follow T."""
    ep = _play("pruned", monkeypatch, None)
    full = _against_fp64("pruned", ep, ep.t_eff + 1)
    short = _against_fp64("pruned", ep, ep.t_eff - 1, fresh=False)
    assert short["traj_len"] < full["traj_len"]


def test_nan_is_the_reference_nan(monkeypatch):
    """A target policy with an exact zero on a legal action: 0 * (log 0 - log q) is NaN in the reference (util/metric.kld has no special
    case), so entropy_target is NaN -- and nothing else moves."""
    import rnad_hip

    tree, nets, rec, fast, logit_target, rows = _setup("ternary4")
    h = tree.handle()
    ep = _play("ternary4", monkeypatch, None)
    T, B, A = ep.t_eff + 1, ep.batch_size, tree.max_actions
    clean = rnad_hip.log_stats_to_dict(rnad_hip.bucket_log_stats(h, ep.buckets, ep._compact[0], T, rec, logit_target).tolist(), T, B, A)
    poisoned = logit_target.clone()
    poisoned[1] = torch.tensor([0.0, -200.0, 0.0], device=DEV)  # the root (state 1), player 0: expf(-200) == 0 in fp32
    assert rows["masks"][1].all()
    got = rnad_hip.log_stats_to_dict(rnad_hip.bucket_log_stats(h, ep.buckets, ep._compact[0], T, rec, poisoned).tolist(), T, B, A)
    assert np.isnan(got["entropy_target"]) and not np.isnan(clean["entropy_target"])
    for key in ("entropy", "traj_len", "logit_mean", "logit_max", "actor_learner_kld"):
        np.testing.assert_allclose(got[key], clean[key], rtol=1e-12, atol=0, err_msg=key)  # (fp64 sums whose order may vary)


def _trainer(tree, tag, B):
    from learn.rnad import RNaD

    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_test_")
    torch.manual_seed(9)
    rn = RNaD(tree=tree, device=DEV, directory_name=tag, batch_size=B, eta=0.2, b1_adam=0.0,
              net_params={"type": "MLP", "max_actions": tree.max_actions, "width": 64})
    rn.initialize()
    return rn


@pytest.mark.parametrize("ragged", (False, True))
def test_logged_step_with_the_flag_is_the_logged_step_without(ragged):
    """train_step(buf, alpha, log={}) on the batch the trainer's own nets played, compact_log off and on from the same weights and seed:
    the same nine keys, the same gradients, and with the flag on nothing dense was materialised."""
    from environment.episode import Buffer
    from environment.tree import Tree
    from test_hip_ragged import _ragged_tree

    if ragged:
        tree = _ragged_tree()
    else:
        tree = Tree(device=DEV, max_actions=3, max_transitions=1, depth_bound=4)
        tree.generate_native(seed=2)
    B = 1 << 13
    logs, grads = {}, {}
    for flag in (False, True):
        rn = _trainer(tree, f"clog{int(ragged)}{int(flag)}", B)
        with torch.no_grad():
            for i, m in enumerate((rn.net_target, rn.net_reg, rn.net_reg_)):
                for p_ in m.parameters():
                    p_.add_(0.05 * (i + 1) * torch.randn_like(p_))
        rn.compact_log = flag
        seen = []
        rn.tabular_gate = 0
        # (the step's last use of .grad is the optimiser's zero_grad: keep a copy instead)
        rn.optimizer.zero_grad = lambda *a, rn=rn, **k: seen.append([p_.grad.detach().clone() for p_ in rn.net.parameters() if p_.grad is not None])
        logs[flag] = {}
        rn.train_step(Buffer(1), 0.4, log=logs[flag])
        torch.cuda.synchronize()
        grads[flag] = seen[-1]
        ep = rn.last_episodes
        assert ep._compact is not None and ep.buckets is not None, "the step must have played the compact bucketed batch"
        if flag:
            assert ep.__dict__["_indices"] is None and ep._compact[0].policy is None
        else:
            assert ep.__dict__["_indices"] is not None and ep._compact[0].policy is not None
    assert set(logs[False]) == set(logs[True]) == NINE
    for key, want in logs[False].items():
        got = logs[True][key]
        print(f"{key}: off {want!r} on {got!r}")
        if key.startswith("loss"):
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=key)
        elif key == "gradient_norm":
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=key)
        elif key == "actor_learner_kld":
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=key)
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * max(1.0, abs(want)), err_msg=key)
    assert len(grads[False]) == len(grads[True]) == len(list(rn.net.parameters())) and all(torch.equal(a, b) for a, b in zip(grads[False], grads[True]))


def test_logged_step_between_replays(monkeypatch):
    """Eight steps, the 5th logged (past the warm-up: replays surround it): the parameters are those of a trainer that logged the same
    step with the flag off, and the steps around the logged one were replays of one captured graph."""
    from environment.episode import Buffer
    from test_hip_bucket import TREES, _native_tree

    tree = _native_tree(**TREES["ternary4"])
    replays = []
    real = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real(self))[1])
    finals, logged, counts = [], [], []
    for flag in (False, True):
        rn = _trainer(tree, f"creplay{int(flag)}", 1 << 13)
        rn.compact_log = flag
        buf = Buffer(1)
        replays.clear()
        per_step = []
        for i in range(8):
            log = {} if i == 4 else None
            before = len(replays)
            rn.train_step(buf, alpha=min(1.0, 0.15 * i), log=log)
            rn.total_steps += 1
            per_step.append(len(replays) - before)
            if log is not None:
                logged.append(log)
        torch.cuda.synchronize()
        assert rn._graph["graph"] is not None and not rn._graph["failed"]
        assert len(set(replays)) == 1, "one capture: the logged step must not re-capture"
        counts.append(per_step)
        finals.append([p_.detach().clone() for n in (rn.net, rn.net_target) for p_ in n.parameters()])
    assert counts[0] == counts[1] == [0] * RNaD_warmup() + [1, 0, 1, 1, 1], counts
    assert set(logged[0]) == set(logged[1]) == NINE
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def RNaD_warmup():
    from learn.rnad import RNaD

    assert RNaD._GRAPH_WARMUP == 3, "the logged step of this test must come after the capture"
    return RNaD._GRAPH_WARMUP
