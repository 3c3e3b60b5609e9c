"""rnad_best_response on the MI355X against the fp64 sweep of tests/_brref.py, within its derived gates at EVERY state:

  a. values, gain, reach and best: the four golden trees, the native A = 3, C = 2, depth_bound = 5 tree and the pruned A = 5, C = 4 one,
     each with n = 1, 2, 3, 31 and 32 tables -- one lane per side, partial half-waves, a full wave.  All four outputs are pre-filled with
     NaN: afterwards every row is written, the rows of state 0 and of unreached states are zero, every reached row of best is one-hot
     on a legal action, and the exact response of that action lies within twice the gate of the exact maximum;
  b. bits: values[:, 0, k] and values[:, 1, k] are rnad_nashconv's row_best and col_best for table k, bit for bit, at every reached state;
  c. the performance-difference identity on the device: the fp64 host sum of reach * gain against util.metric.cross_play's exploitability;
  d. the table is a policy: rnad_cross_play over the members and their best-response tables returns values[1] on both sides;
  e. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed twice, gives the eager bits;
  f. the API: util.metric.best_response, RNaD.best_response, the refusals of the binding, of the C entry and of a tree that is none, and
     tools/exploit.py in-process on the reference-written run and tree files of tests/golden.

The worst share of each gate per case goes to best_response_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/best_response_errors.json holds the figures of an MI355X."""
import gc
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

import _brref as br
import _crossref as cr
from _util import GOLDEN, TREES, assert_bits_equal
from rnad_hip import best_response as _the_symbol_this_file_is_about  # noqa: F401  (without it nothing below can run)
from test_hip_cross_play import _trainer, product_tree

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
ALL_TREES = TREES + ("native_a3", "native_a5")
NS = (1, 2, 3, 31, 32)
SHARES = {}


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    SHARES.clear()
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if SHARES and os.path.isdir(out):
        with open(os.path.join(out, "best_response_errors.json"), "w") as f:
            json.dump(SHARES, f, indent=1, sort_keys=True)


def run(name, n, outs=(None, None, None, None)):
    import rnad_hip

    policies = torch.tensor(br.case(name, n).J, device=DEV)  # (a copy: the case's arrays are read-only)
    return rnad_hip.best_response(product_tree(name).handle(), policies, *outs) + (policies,)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ALL_TREES)
def test_every_output_within_its_gate_at_every_state(name, n):
    c = br.case(name, n)
    ref, reached = c.ref, c.reached
    S, _, A2 = c.J.shape
    A = A2 // 2
    assert S < 10**5
    outs = tuple(torch.full(shape, float("nan"), device=DEV) for shape in ((S, n, A2), (S, 2, n), (S, 2, n), (S, n)))
    got = run(name, n, outs)
    assert all(a is b for a, b in zip(got, outs))
    best, values, gain, reach = (t.cpu().numpy() for t in outs)
    for a in (best, values, gain, reach):
        assert np.isfinite(a).all(), "a row was left unwritten"
        assert (a[~reached] == 0).all(), "state 0 and the states no path reaches are zero"
    assert (reach[1] == 1).all()
    shares = dict(values=cr.share(values, ref.V, c.gV), gain=cr.share(gain, ref.G, c.gG), reach=cr.share(reach, ref.R, c.gR))
    hot = best.reshape(S, n, 2, A).transpose(0, 2, 1, 3)                      # [S, 2, n, A]
    assert set(np.unique(hot)) <= {0.0, 1.0}
    assert (hot[reached].sum(axis=3) == 1).all(), "one action per reached state, side and member"
    assert not (hot != 0)[np.broadcast_to(~ref.legal[:, :, None, :], hot.shape)].any(), "an illegal action was picked"
    regret = br.picked_regret(ref, best)
    with np.errstate(divide="ignore", invalid="ignore"):
        shares["picked_action_below_maximum"] = float(np.where(regret == 0, 0.0, regret / (2 * c.gV)).max())
    SHARES[f"{name}/n{n}"] = dict(S=int(S), **shares)
    print(f"{name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the gates")
    assert max(shares.values()) <= 1.0


@pytest.mark.parametrize("name", ("small", "ragged", "native_a5"))
def test_values_carry_the_bits_of_rnad_nashconv(name):
    import rnad_hip

    n = 3
    c = br.case(name, n)
    _, values, _, _, policies = run(name, n)
    handle = product_tree(name).handle()
    S = c.J.shape[0]
    reached = c.reached
    for k in range(n):
        table = policies[:, k].contiguous()
        row_best, col_best, reach = (torch.zeros((S,), device=DEV) for _ in range(3))
        depth = torch.zeros((S,), dtype=torch.int32, device=DEV)
        rnad_hip.nashconv(handle, table, table[1].contiguous(), 1, 1.0, row_best, col_best, reach, depth)
        assert_bits_equal(values[:, 0, k].cpu().numpy()[reached], row_best.cpu().numpy()[reached], f"{name} table {k} row_best")
        assert_bits_equal(values[:, 1, k].cpu().numpy()[reached], col_best.cpu().numpy()[reached], f"{name} table {k} col_best")


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a3", 2), ("native_a5", 8)])
def test_performance_difference_identity_on_the_device(name, n):
    from util import metric

    c = br.case(name, n)
    ref = c.ref
    _, values, gain, reach, policies = run(name, n)
    got = (reach.cpu().numpy().astype(np.float64)[:, None, :] * gain.cpu().numpy().astype(np.float64)).sum(axis=0).T       # [n, 2]
    cross = metric.cross_play(product_tree(name), [policies[:, k] for k in range(n)])
    want = cross.exploitability.cpu().numpy().astype(np.float64)
    # the exact identity holds to 1e-15 (tests/test_best_response.py).  Left of it every factor is within its gate; right of it
    # row_best / col_best are the bits of values[1] (gate of V), the payoff is within the cross-play gate, and the fp32 difference of the
    # two rounds once
    V, B, h = cr.reference(c.tree, c.J)
    g = np.diagonal(cr.gate(c.tree, B, h)[1])
    R, G = np.asarray(ref.R, np.float64)[:, None, :], np.abs(np.asarray(ref.G, np.float64))
    left = (c.gR[:, None, :] * G + R * c.gG + c.gR[:, None, :] * c.gG).sum(axis=0).T
    right = c.gV[1].T + g[:, None] + 2 * br.U * (np.abs(ref.V[1]).T + np.abs(np.diagonal(V[1]))[:, None])
    tol = left + right + 1e-12 * ref.B[1].T
    print(f"{name} n={n}: {(np.abs(got - want) / tol).max():.3f} of the tolerance; exploitability up to {want.max():.3g}")
    assert (np.abs(got - want) <= tol).all()


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 16), ("native_a5", 8)])
def test_the_best_response_table_plays_like_a_policy(name, n):
    import rnad_hip

    c = br.case(name, n)
    best, values, _, _, policies = run(name, n)
    everyone = torch.cat([policies, best], dim=1).contiguous()
    payoff = rnad_hip.cross_play(product_tree(name).handle(), everyone)[1].cpu().numpy().astype(np.float64)
    V, B, h = cr.reference(c.tree, everyone.cpu().numpy())
    g = cr.gate(c.tree, B, h)[1]
    v = values[1].cpu().numpy().astype(np.float64)
    k = np.arange(n)
    rows, cols = np.abs(payoff[n + k, k] - v[0]), np.abs(-payoff[k, n + k] - v[1])
    print(f"{name} n={n}: {max((rows / (2 * g[n + k, k])).max(), (cols / (2 * g[k, n + k])).max()):.3f} of two cross-play gates")
    assert (rows <= 2 * g[n + k, k]).all() and (cols <= 2 * g[k, n + k]).all()


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n):
    import rnad_hip

    first = run(name, n)
    second = run(name, n)
    policies = first[4]
    assert all(torch.equal(a, b) for a, b in zip(first[:4], second[:4]))
    handle = product_tree(name).handle()
    outs = tuple(torch.full_like(t, float("nan")) for t in first[:4])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.best_response(handle, policies, *outs)
    finally:
        if gc_was_on:
            gc.enable()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, first[:4]))


# ---------------------------------------------------------------------------------------------------- the API
def test_metric_best_response_with_tables_and_a_net():
    from nn.net import MLP
    from util import metric

    name = "small"
    arrs = cr.tree_arrays(name)
    tree = product_tree(name)
    J = cr.players(arrs, 3, 0, cr.fixture_policy(name))
    torch.manual_seed(5)
    net = MLP(tree.max_actions, 64, device=DEV)
    net.train()
    tables = [torch.tensor(J[:, k], device=DEV) for k in range(3)]
    res = metric.best_response(tree, tables + [net])
    assert net.training, "the net is left in the mode it came in"
    S, A = J.shape[0], tree.max_actions
    assert res.policy.shape == (S, 4, 2 * A) and res.values.shape == (S, 2, 4) and res.gain.shape == (S, 2, 4) and res.reach.shape == (S, 4)
    assert res.attribution.shape == (S, 2, 4) and res.exploitability.shape == (4, 2)
    assert res.exploitability.dtype == torch.float64 and res.exploitability.device.type == "cpu"
    assert torch.equal(res.attribution, res.reach[:, None, :] * res.gain)
    assert torch.equal(res.exploitability, res.attribution.double().sum(dim=0).t().cpu())
    full = np.concatenate([J, metric.joint_policy_of(tree, net).cpu().numpy()[:, None]], axis=1)
    ref = br.reference(arrs, full)
    gV, gQ, gG, gR = br.gates(arrs, ref, full)
    assert cr.share(res.values.cpu().numpy(), ref.V, gV) <= 1.0 and cr.share(res.gain.cpu().numpy(), ref.G, gG) <= 1.0
    assert cr.share(res.reach.cpu().numpy(), ref.R, gR) <= 1.0
    # policy[:, k] is an ordinary table: cross_play, mixture, population and the tabular solver take it as a player
    exploiter = res.policy[:, 3]
    cross = metric.cross_play(tree, tables + [exploiter])
    assert torch.isfinite(cross.payoff).all()
    assert metric.mixture(tree, [tables[0], exploiter]).policy.shape == (S, 2 * A)
    assert np.isfinite(metric.population(tree, [tables[1], exploiter]).nash_nashconv)
    from learn.tabular import solve_regularized

    assert torch.isfinite(solve_regularized(tree, 0.2, reg=exploiter).policy).all()


def test_rnad_best_response_two_trainers_and_a_foreign_tree():
    from util import metric

    tree = product_tree("small")
    a, b = _trainer(tree, "a", 1), _trainer(tree, "b", 2)
    res = a.best_response(b)
    want = metric.best_response(tree, [a.net_target, b.net_target])
    assert res.policy.shape[1] == 2 and all(torch.equal(x, y) for x, y in zip(res, want))
    assert a.best_response().exploitability.shape == (1, 2)
    foreign = _trainer(product_tree("ragged"), "c", 3)
    with pytest.raises(ValueError, match="another tree"):
        a.best_response(b, foreign)


# ---------------------------------------------------------------------------------------------------- refusals
def test_binding_refusals():
    import rnad_hip

    handle = product_tree("small").handle()
    S, A = handle.S, handle.A
    good = torch.zeros((S, 2, 2 * A), device=DEV)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="GPU"):
        rnad_hip.best_response(handle, good.cpu())
    with pytest.raises(err, match="dtype"):
        rnad_hip.best_response(handle, good.double())
    with pytest.raises(err, match="contiguous"):
        rnad_hip.best_response(handle, torch.zeros((2, S, 2 * A), device=DEV).transpose(0, 1))
    with pytest.raises(err, match="do not fit"):
        rnad_hip.best_response(handle, torch.zeros((S + 1, 2, 2 * A), device=DEV))
    with pytest.raises(err, match="do not fit"):
        rnad_hip.best_response(handle, torch.zeros((S, 2, 2 * A + 2), device=DEV))
    with pytest.raises(err, match="outside"):
        rnad_hip.best_response(handle, torch.zeros((S, 33, 2 * A), device=DEV))
    with pytest.raises(err, match=r"\[S, n, 2A\]"):
        rnad_hip.best_response(handle, torch.zeros((S, 2 * A), device=DEV))
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.best_response(product_tree("small"), good)
    with pytest.raises(err, match="best"):
        rnad_hip.best_response(handle, good, torch.zeros((S, 2, 2 * A + 1), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.best_response(handle, good, None, torch.zeros((S, 2, 2), device=DEV, dtype=torch.float64))
    with pytest.raises(err, match="gain"):
        rnad_hip.best_response(handle, good, None, None, torch.zeros((S, 2, 3), device=DEV))
    with pytest.raises(err, match="reach"):
        rnad_hip.best_response(handle, good, None, None, None, torch.zeros((S, 3), device=DEV))
    with pytest.raises(err, match="values aliases policies"):
        rnad_hip.best_response(handle, good, None, good.view(-1)[: S * 4].view(S, 2, 2))
    with pytest.raises(err, match="reach aliases policies"):
        rnad_hip.best_response(handle, good, None, None, None, good.view(-1)[S * 2 * A:][: S * 2].view(S, 2))
    # the C entry point itself: n out of range and null pointers, nothing launched
    lib = rnad_hip.lib()
    p = good.data_ptr()
    assert lib.rnad_best_response(handle.ptr, 0, p, p, p, p, p, None) != 0
    assert b"outside" in lib.rnad_last_error()
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert lib.rnad_best_response(handle.ptr, 2, *args, None) != 0
        assert b"null" in lib.rnad_last_error()
    torch.cuda.synchronize()
    assert (good == 0).all(), "nothing was launched"


def test_a_state_with_two_parents_is_refused_before_any_sweep(monkeypatch):
    import rnad_hip
    from _gpu import tree_from_arrays
    from util import metric

    arrs = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in cr.tree_arrays("small").items()}
    index, chance = arrs["index"], arrs["chance"]
    live = (index != 0) & (chance > 0)
    levels = cr.level_order(index, chance)
    assert len(levels) >= 3
    # the first live link of the root now leads to a grandchild, which keeps the parent it has
    s, t, r, c = 1, *[int(v[0]) for v in np.nonzero(live[1])]
    index[s, t, r, c] = levels[2][0]
    tree = tree_from_arrays(arrs, depth_bound=arrs["meta"]["kw"]["depth_bound"])
    table = torch.tensor(cr.players(cr.tree_arrays("small"), 1)[:, 0], device=DEV)

    def no_sweep(*args, **kwargs):
        raise AssertionError("a sweep ran")

    monkeypatch.setattr(rnad_hip, "best_response", no_sweep)
    for _ in range(2):  # the second answer comes from the tree object
        with pytest.raises(ValueError, match="not a tree: joint reach is undefined"):
            metric.best_response(tree, [table, table])


# ---------------------------------------------------------------------------------------------------- the tool
def test_tool_on_a_reference_written_run(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("exploit_tool", os.path.join(ROOT, "tools", "exploit.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run_dir = tmp_path / "from_reference"
    os.makedirs(run_dir / "1")
    shutil.copy(os.path.join(GOLDEN, "ref_run_params"), run_dir / "params")
    shutil.copy(os.path.join(GOLDEN, "ref_run_ckpt_1_0"), run_dir / "1" / "0")
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, str(run_dir), "--fresh", "--top", "3"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == out and out["names"] == ["from_reference@1/0", "fresh"]
    assert set(out) == {"names", "exploitability", "nashconv", "by_depth", "top", "exploiter_payoff"}
    expl, by_depth = np.asarray(out["exploitability"]), np.asarray(out["by_depth"])
    assert expl.shape == (2, 2) and np.isfinite(expl).all() and by_depth.shape[:2] == (2, 2) and by_depth.shape[2] >= 2
    np.testing.assert_allclose(by_depth.sum(axis=2), expl, rtol=0, atol=1e-12)
    np.testing.assert_allclose(expl.sum(axis=1), out["nashconv"], rtol=0, atol=1e-5)
    for k in range(2):
        for side in range(2):
            listed = out["top"][k][side]
            assert len(listed) == 3 and all(set(e) == {"state", "depth", "reach", "gain", "share"} for e in listed)
            shares = [e["share"] for e in listed]
            assert shares == sorted(shares, reverse=True) and sum(shares) <= 1 + 1e-6
            assert all(abs(e["reach"] * e["gain"] - e["share"] * expl[k, side]) <= 1e-6 for e in listed)
    # each player against its own exploiter: what the best response earns
    cross = tool.cross_play_tool
    tree = cross.load_tree(tar, DEV)
    _, net, params = cross.load_player(str(run_dir), (1, 0), tree, DEV)
    from util import metric

    torch.manual_seed(0)
    res = metric.best_response(tree, [net, cross.new_net(params, DEV)])
    np.testing.assert_allclose(expl, res.exploitability.numpy(), rtol=0, atol=1e-6)
    payoff = np.asarray(out["exploiter_payoff"])
    np.testing.assert_allclose(payoff[:, 0], res.values[1, 0].cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(payoff[:, 1], -res.values[1, 1].cpu().numpy(), rtol=0, atol=1e-5)
    with pytest.raises(SystemExit, match="at most 32"):
        tool.main(["--tree", tar] + [str(run_dir)] * 33)
