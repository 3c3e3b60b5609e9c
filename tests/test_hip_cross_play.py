"""rnad_cross_play on the MI355X against the fp64 sweep of tests/_crossref.py, within its derived gate at EVERY state:

  a. values: the four golden trees, the native A = 3, C = 2, depth_bound = 5 tree (27 670 states) and the pruned A = 5, C = 4 one, each with
     n = 1, 2, 3, 8, 9 and 32 policies -- 1, 4 and 9 pairs in a wave, exactly one tile of 64, one tile and a partial second, 16 tiles.
     `values` is pre-filled with NaN: afterwards every row is finite and row 0 zero;
  b. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed twice, gives the eager bits;
  c. the API: util.metric.cross_play (diagonal between -col_best[1] and row_best[1] of get_nashconv, exploitability summing to nashconv),
     RNaD.cross_play for two trainers and its refusal of a foreign tree, the binding's refusals;
  d. tools/cross_play.py in-process on the reference-written run and tree files of tests/golden.

The worst share of the gate per case goes to cross_play_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/cross_play_errors.json holds the figures of an MI355X."""
import functools
import gc
import importlib.util
import json
import os
import shutil
import tempfile
import zlib

import numpy as np
import pytest
import torch

import _crossref as cr
from _util import GOLDEN, TREES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
ALL_TREES = TREES + ("native_a3", "native_a5")
NS = (1, 2, 3, 8, 9, 32)
SHARES = {}


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    SHARES.clear()
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if SHARES and os.path.isdir(out):
        with open(os.path.join(out, "cross_play_errors.json"), "w") as f:
            json.dump(SHARES, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def product_tree(name):
    from _gpu import tree_from_arrays

    arrs = cr.tree_arrays(name)
    tree = tree_from_arrays(arrs, depth_bound=arrs["meta"]["kw"]["depth_bound"])
    tree.hash = arrs["meta"].get("hash", zlib.crc32(name.encode()))
    return tree


def run(name, n, values=None):
    import rnad_hip

    tree, J, V, g = cr.case(name, n)
    policies = torch.tensor(J, device=DEV)  # (a copy: the case's arrays are read-only)
    return rnad_hip.cross_play(product_tree(name).handle(), policies, values), policies


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ALL_TREES)
def test_values_within_the_gate_at_every_state(name, n):
    tree, J, V, g = cr.case(name, n)
    S = V.shape[0]
    assert S < 10**5
    values = torch.full((S, n, n), float("nan"), device=DEV)
    out, _ = run(name, n, values)
    assert out is values
    got = values.cpu().numpy()
    assert np.isfinite(got).all(), "a row was left unwritten"
    assert (got[0] == 0).all()
    worst = cr.share(got, V, g)
    SHARES[f"{name}/n{n}"] = dict(S=int(S), pairs=n * n, gate_share=worst, root_gate_share=cr.share(got[1], V[1], g[1]))
    print(f"{name} n={n}: {worst:.3f} of the gate (root {SHARES[f'{name}/n{n}']['root_gate_share']:.3f})")
    assert worst <= 1.0


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 9), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n):
    import rnad_hip

    first, policies = run(name, n)
    second, _ = run(name, n)
    assert torch.equal(first, second)
    handle = product_tree(name).handle()
    values = torch.full_like(first, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.cross_play(handle, policies, values)
    finally:
        if gc_was_on:
            gc.enable()
    for _ in range(2):
        values.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(values, first)


def _nashconv_of(tree, table):
    from util.metric import NashConvData

    data = NashConvData(tree)
    data.joint_policy.copy_(table)
    data.get_nashconv(tree, data.joint_policy)
    return data.row_best[1].item(), data.col_best[1].item()


@pytest.mark.parametrize("name", ("small", "ragged"))
def test_metric_cross_play_against_get_nashconv(name):
    from nn.net import MLP
    from util import metric

    arrs, J, V, g = cr.case(name, 4)
    tree = product_tree(name)
    torch.manual_seed(5)
    net = MLP(tree.max_actions, 64, device=DEV)
    net.train()
    tables = [torch.tensor(J[:, k], device=DEV) for k in range(4)]
    res = metric.cross_play(tree, tables + [net])
    assert net.training, "the net is left in the mode it came in"
    assert res.payoff.shape == (5, 5) and res.values.shape == (V.shape[0], 5, 5) and res.nashconv.shape == (5,) and res.exploitability.shape == (5, 2)
    assert torch.equal(res.payoff, res.values[1])
    # the tables' block is the case of the sweep; the net's table is joint_policy_of, which get_nashconv_from_net fills bit for bit
    assert cr.share(res.values[:, :4, :4].cpu().numpy(), V, g) <= 1.0
    data = metric.NashConvData(tree)
    data.get_nashconv_from_net(tree, net)
    assert torch.equal(data.joint_policy, metric.joint_policy_of(tree, net))
    full = np.concatenate([J, data.joint_policy.cpu().numpy()[:, None]], axis=1)
    V5, B5, h5 = cr.reference(arrs, full)
    g5 = cr.gate(arrs, B5, h5)
    assert cr.share(res.values.cpu().numpy(), V5, g5) <= 1.0
    payoff, nash, expl = (t.cpu().numpy().astype(np.float64) for t in (res.payoff, res.nashconv, res.exploitability))
    for k, table in enumerate(tables + [data.joint_policy]):
        row_best, col_best = _nashconv_of(tree, table)
        # "up to rounding": the payoff is within its gate, and a best-response sweep rounds as often per level as the cross-play sweep
        # (A * A * C products and their sums, then a maximum, which rounds nothing) on values that are no larger, so it gets the same
        slack = 2 * g5[1, k, k]
        assert -col_best - slack <= payoff[k, k] <= row_best + slack
        assert abs(nash[k] - (row_best + col_best)) <= 1e-6
        assert abs(expl[k].sum() - nash[k]) <= 1e-6
        assert (expl[k] >= -slack).all()
    assert abs(nash[0]) <= 1e-5, "player 0 is the tree's solution"


def _trainer(tree, name, seed):
    from learn.rnad import RNaD

    os.environ["RNAD_SAVE_DIR"] = tempfile.mkdtemp(prefix="rnad_cross_play_")
    torch.manual_seed(seed)
    rn = RNaD(tree=tree, device=DEV, directory_name=name, batch_size=256, eta=0.2, b1_adam=0.0, lr=1e-3,
              net_params={"type": "MLP", "max_actions": tree.max_actions, "width": 64})
    rn.initialize()
    return rn


def test_rnad_cross_play_two_trainers_and_a_foreign_tree():
    from util import metric

    tree = product_tree("small")
    a, b = _trainer(tree, "a", 1), _trainer(tree, "b", 2)
    res = a.cross_play(b)
    assert res.payoff.shape == (2, 2) and torch.isfinite(res.payoff).all() and torch.isfinite(res.nashconv).all()
    arrs = cr.tree_arrays("small")
    J = np.stack([metric.joint_policy_of(tree, rn.net_target).cpu().numpy() for rn in (a, b)], axis=1)
    V, B, h = cr.reference(arrs, J)
    assert cr.share(res.values.cpu().numpy(), V, cr.gate(arrs, B, h)) <= 1.0
    assert a.cross_play().payoff.shape == (1, 1)
    foreign = _trainer(product_tree("ragged"), "c", 3)
    assert foreign.tree.hash != tree.hash
    with pytest.raises(ValueError, match="another tree"):
        a.cross_play(b, foreign)


def test_binding_refusals():
    import rnad_hip

    handle = product_tree("small").handle()
    S, A = handle.S, handle.A
    good = torch.zeros((S, 2, 2 * A), device=DEV)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="GPU"):
        rnad_hip.cross_play(handle, good.cpu())
    with pytest.raises(err, match="dtype"):
        rnad_hip.cross_play(handle, good.double())
    with pytest.raises(err, match="contiguous"):
        rnad_hip.cross_play(handle, torch.zeros((2, S, 2 * A), device=DEV).transpose(0, 1))
    with pytest.raises(err, match="do not fit"):
        rnad_hip.cross_play(handle, torch.zeros((S + 1, 2, 2 * A), device=DEV))
    with pytest.raises(err, match="do not fit"):
        rnad_hip.cross_play(handle, torch.zeros((S, 2, 2 * A + 2), device=DEV))
    with pytest.raises(err, match="outside"):
        rnad_hip.cross_play(handle, torch.zeros((S, 33, 2 * A), device=DEV))
    with pytest.raises(err, match=r"\[S, n, 2A\]"):
        rnad_hip.cross_play(handle, torch.zeros((S, 2 * A), device=DEV))
    with pytest.raises(err, match="values"):
        rnad_hip.cross_play(handle, good, torch.zeros((S, 2, 3), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.cross_play(handle, good, torch.zeros((S, 2, 2), device=DEV, dtype=torch.float64))
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.cross_play(product_tree("small"), good)
    # the C entry point itself: n out of range and null pointers, nothing launched
    lib = rnad_hip.lib()
    assert lib.rnad_cross_play(handle.ptr, 0, good.data_ptr(), good.data_ptr(), None) != 0
    assert b"outside" in lib.rnad_last_error()
    assert lib.rnad_cross_play(handle.ptr, 2, None, good.data_ptr(), None) != 0
    assert b"null" in lib.rnad_last_error()


def test_tool_on_a_reference_written_run(tmp_path, capsys):
    from util import metric

    spec = importlib.util.spec_from_file_location("cross_play_tool", os.path.join(ROOT, "tools", "cross_play.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run_dir = tmp_path / "from_reference"
    os.makedirs(run_dir / "1")
    shutil.copy(os.path.join(GOLDEN, "ref_run_params"), run_dir / "params")
    shutil.copy(os.path.join(GOLDEN, "ref_run_ckpt_1_0"), run_dir / "1" / "0")
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, str(run_dir), "--fresh"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == out and out["names"] == ["from_reference@1/0", "fresh"]
    payoff = np.asarray(out["payoff"])
    assert payoff.shape == (2, 2) and np.isfinite(payoff).all()
    assert len(out["nashconv"]) == 2 and np.asarray(out["exploitability"]).shape == (2, 2)
    # the same two nets through the API
    tree = tool.load_tree(tar, DEV)
    _, net, params = tool.load_player(str(run_dir), (1, 0), tree, DEV)
    torch.manual_seed(0)
    res = metric.cross_play(tree, [net, tool.new_net(params, DEV)])
    np.testing.assert_allclose(np.diagonal(payoff), torch.diagonal(res.payoff).cpu().numpy(), rtol=0, atol=1e-6)
    with pytest.raises(SystemExit, match="no checkpoint"):
        tool.main(["--tree", tar, str(run_dir), "--checkpoint", "7", "0"])
