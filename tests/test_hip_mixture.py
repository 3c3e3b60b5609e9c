"""rnad_mixture on the MI355X against the fp64 sweep of tests/_mixref.py, within its derived gates at EVERY state:

  a. mix and reach: the four golden trees, the native A = 3, C = 2, depth_bound = 5 tree and the pruned A = 5, C = 4 one, each with
     n = 1, 2, 3, 31 and 32 policies -- one lane per side, partial half-waves, a full wave -- and the four weight sets of _mixref
     (uniform, a seeded Dirichlet per side, one with zero entries, one-hot on the tree's solution: the D == 0 rows).  Both outputs are
     pre-filled with NaN: afterwards every row is finite and row 0 zero;
  b. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed twice, gives the eager bits;
  c. the Kuhn identity on the device: rnad_cross_play over the members and the mixture gives the mixture the weighted sums of the
     members' payoffs;
  d. the API: util.metric.mixture, meta_nash and population, RNaD.population, TabularRNaD(average=True), the refusals of the binding,
     of the C entry and of a tree that is none;
  e. tools/population.py in-process on the reference-written run and tree files of tests/golden.

The worst share of the gates per case goes to mixture_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/mixture_errors.json holds the figures of an MI355X."""
import gc
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

import _crossref as cr
import _mixref as mr
from _util import GOLDEN, TREES
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
        with open(os.path.join(out, "mixture_errors.json"), "w") as f:
            json.dump(SHARES, f, indent=1, sort_keys=True)


def run(name, n, kind, mix=None, reach=None):
    import rnad_hip

    tree, J, w = mr.case(name, n, kind)[:3]
    policies, weights = torch.tensor(J, device=DEV), torch.tensor(w, device=DEV)  # (copies: the case's arrays are read-only)
    return rnad_hip.mixture(product_tree(name).handle(), policies, weights, mix, reach) + (policies, weights)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ALL_TREES)
def test_mix_and_reach_within_their_gates_at_every_state(name, n):
    zero_d = 0
    for kind in mr.WEIGHTS:
        tree, J, w, M, R, depth, gM, gR = mr.case(name, n, kind)
        S, A2 = M.shape
        assert S < 10**5
        mix = torch.full((S, A2), float("nan"), device=DEV)
        reach = torch.full((S, 2, n), float("nan"), device=DEV)
        out = run(name, n, kind, mix, reach)
        assert out[0] is mix and out[1] is reach
        got_m, got_r = mix.cpu().numpy(), reach.cpu().numpy()
        assert np.isfinite(got_m).all() and np.isfinite(got_r).all(), "a row was left unwritten"
        assert (got_m[0] == 0).all() and (got_r[0] == 0).all() and (got_r[1] == 1).all()
        assert (got_m[depth < 0] == 0).all() and (got_r[depth < 0] == 0).all()
        worst_m, worst_r = cr.share(got_m, M, gM), cr.share(got_r, R, gR)
        never = int(mr.never_reached_by_the_mixture(w, R, depth).sum())
        zero_d += never
        SHARES[f"{name}/n{n}/{kind}"] = dict(S=int(S), mix_gate_share=worst_m, reach_gate_share=worst_r, rows_with_D_zero=never)
        print(f"{name} n={n} {kind}: mix {worst_m:.3f} of its gate, reach {worst_r:.3f} of its gate, {never} rows with D == 0")
        assert worst_m <= 1.0 and worst_r <= 1.0
    assert zero_d > 0, "one-hot weights on the solution leave reached states that the mixture never comes to: the D == 0 rows"


@pytest.mark.parametrize("name,n,kind", [("small", 3, "dirichlet"), ("ragged", 31, "zeros"), ("native_a5", 32, "onehot")])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n, kind):
    import rnad_hip

    first_m, first_r, policies, weights = run(name, n, kind)
    second_m, second_r, _, _ = run(name, n, kind)
    assert torch.equal(first_m, second_m) and torch.equal(first_r, second_r)
    handle = product_tree(name).handle()
    mix, reach = torch.full_like(first_m, float("nan")), torch.full_like(first_r, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.mixture(handle, policies, weights, mix, reach)
    finally:
        if gc_was_on:
            gc.enable()
    for _ in range(2):
        mix.fill_(float("nan"))
        reach.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mix, first_m) and torch.equal(reach, first_r)


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a3", 2), ("native_a5", 8)])
def test_kuhn_identity_on_the_device(name, n, kind):
    import rnad_hip

    tree, J, w, M, R, depth, gM, gR = mr.case(name, n, kind)
    mix, _, policies, _ = run(name, n, kind)
    everyone = torch.cat([policies, mix[:, None]], dim=1).contiguous()
    got = rnad_hip.cross_play(product_tree(name).handle(), everyone)[1].cpu().numpy().astype(np.float64)
    # what the two gates give: each cross-play value is within its gate g of the exact value of the tables it was given, the mixture's
    # side of the identity and the members' side (a convex combination of values with the same bound) -- 2 g; and the table it was
    # given is the exact mixture times (1 + delta), |delta| <= eps, at the h[1] states of a path, in a value that is linear in each
    V, B, h = cr.reference(tree, everyone.cpu().numpy())
    g = cr.gate(tree, B, h)
    tol = 2 * g[1] + ((1 + mr.eps(depth, n)) ** int(h[1]) - 1) * B[1]
    x, y = mr.exact_weights(w)
    P = got[:n, :n]
    rows, cols, both = np.abs(got[n, :n] - x @ P), np.abs(got[:n, n] - P @ y), abs(got[n, n] - x @ P @ y)
    print(f"{name} n={n} {kind}: {max((rows / tol[n, :n]).max(), (cols / tol[:n, n]).max(), both / tol[n, n]):.3f} of the tolerance")
    assert (rows <= tol[n, :n]).all() and (cols <= tol[:n, n]).all() and both <= tol[n, n]


# ---------------------------------------------------------------------------------------------------- the API
def test_metric_mixture_with_tables_and_a_net():
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
    res = metric.mixture(tree, tables + [net], [3, 0, 1, 4], col_weights=[1, 1, 1, 1])
    assert net.training, "the net is left in the mode it came in"
    S, A = J.shape[0], tree.max_actions
    assert res.policy.shape == (S, 2 * A) and res.reach.shape == (S, 2, 4) and res.weights.shape == (2, 4)
    want_w = np.array([[0.375, 0.0, 0.125, 0.5], [0.25, 0.25, 0.25, 0.25]], np.float32)
    assert np.array_equal(res.weights.cpu().numpy(), want_w)
    full = np.concatenate([J, metric.joint_policy_of(tree, net).cpu().numpy()[:, None]], axis=1)
    M, R, depth = mr.reference(arrs, full, want_w)
    gM, gR = mr.gates(M, R, depth, 4)
    assert cr.share(res.policy.cpu().numpy(), M, gM) <= 1.0 and cr.share(res.reach.cpu().numpy(), R, gR) <= 1.0
    uniform = metric.mixture(tree, tables)
    assert np.array_equal(uniform.weights.cpu().numpy(), np.full((2, 3), np.float32(1.0 / 3)))
    # the result is an ordinary table: cross_play takes it as a player
    assert torch.isfinite(metric.cross_play(tree, tables + [uniform.policy]).payoff).all()


@pytest.mark.parametrize("name", ("small", "ragged"))
def test_metric_population(name):
    import rnad_hip
    from util import metric

    arrs = cr.tree_arrays(name)
    tree = product_tree(name)
    n = 5
    J = cr.players(arrs, n, 0, cr.fixture_policy(name))
    tables = [torch.tensor(J[:, k], device=DEV) for k in range(n)]
    pop = metric.population(tree, tables)
    assert pop.cross.payoff.shape == (n, n) and pop.meta.row.shape == (n,) and pop.meta.col.shape == (n,)
    P = pop.cross.payoff.cpu().numpy().astype(np.float64)
    assert pop.meta.gap <= 1e-9 * max(1.0, np.abs(P).max())
    # the Nash mixture against every member, through the sweep itself
    everyone = torch.stack(tables + [pop.nash_policy], dim=1).contiguous()
    V, B, h = cr.reference(arrs, everyone.cpu().numpy())
    g = cr.gate(arrs, B, h)
    depth = mr.reference(arrs, J, np.full((2, n), 1.0 / n))[2]
    # the device identity's tolerance, the certificate's bound, and n weights rounded to fp32 on payoffs of at most max B
    slack = float((2 * g[1] + ((1 + mr.eps(depth, n)) ** int(h[1]) - 1) * B[1]).max()) + 1e-9 * max(1.0, np.abs(P).max()) + n * mr.U * B[1].max()
    got = rnad_hip.cross_play(tree.handle(), everyone)[1].cpu().numpy().astype(np.float64)
    assert (got[n, :n] >= pop.meta.value - slack).all(), "no member's column side gains on the Nash mixture's row side"
    assert (got[:n, n] <= pop.meta.value + slack).all(), "no member's row side gains on the Nash mixture's column side"
    for nc in (pop.nash_nashconv, pop.uniform_nashconv):
        assert np.isfinite(nc) and nc >= -slack
    uniform = metric.mixture(tree, tables).policy
    assert torch.equal(pop.uniform_policy, uniform)
    nash = metric.mixture(tree, tables, pop.meta.row, pop.meta.col).policy
    assert torch.equal(pop.nash_policy, nash)


def test_a_population_of_the_solution_alone_is_the_solution():
    from util import metric

    tree = product_tree("small")
    pop = metric.population(tree, [tree.solution_tensor])
    assert pop.meta.row.tolist() == [1.0] and pop.meta.col.tolist() == [1.0]
    assert abs(pop.nash_nashconv) <= 1e-5 and abs(pop.uniform_nashconv) <= 1e-5


def test_rnad_population_two_trainers_and_a_foreign_tree():
    from util import metric

    tree = product_tree("small")
    a, b = _trainer(tree, "a", 1), _trainer(tree, "b", 2)
    pop = a.population(b)
    assert pop.cross.payoff.shape == (2, 2) and np.isfinite(pop.nash_nashconv) and np.isfinite(pop.uniform_nashconv)
    want = metric.population(tree, [a.net_target, b.net_target])
    assert torch.equal(pop.nash_policy, want.nash_policy) and torch.equal(pop.uniform_policy, want.uniform_policy)
    assert a.population().cross.payoff.shape == (1, 1)
    foreign = _trainer(product_tree("ragged"), "c", 3)
    with pytest.raises(ValueError, match="another tree"):
        a.population(b, foreign)


def test_tabular_rnad_average():
    from learn.tabular import TabularRNaD
    from util import metric

    name = "small"
    arrs = cr.tree_arrays(name)
    tree = product_tree(name)
    plain, averaged = TabularRNaD(tree, eta=0.2), TabularRNaD(tree, eta=0.2, average=True)
    iterates = []
    for _ in range(3):
        plain.update()
        averaged.update()
        iterates.append(averaged.policy.clone())
    assert plain.average_policy is None and plain.average_nashconv_history == []
    assert plain.nashconv_history == averaged.nashconv_history and torch.equal(plain.policy, averaged.policy)
    assert len(averaged.average_nashconv_history) == 3 and averaged.average_nashconv_history[0] == averaged.nashconv_history[0]
    direct = metric.mixture(tree, iterates)
    J = torch.stack(iterates, dim=1).cpu().numpy()
    M, R, depth = mr.reference(arrs, J, direct.weights.cpu().numpy())
    gM, _ = mr.gates(M, R, depth, 3)
    # folding took two sweeps of two members, the direct mixture one of three: each within a gate of the exact table of its inputs
    comes = np.repeat((depth >= 0)[:, None] & ((direct.weights.cpu().numpy().astype(np.float64)[None] * R).sum(axis=2) > 0), M.shape[1] // 2, axis=1)
    err = np.abs(averaged.average_policy.cpu().numpy().astype(np.float64) - direct.policy.cpu().numpy())
    assert comes[1].all() and (err[comes] <= 3 * gM[comes]).all()


# ---------------------------------------------------------------------------------------------------- refusals
def test_binding_refusals():
    import rnad_hip

    handle = product_tree("small").handle()
    S, A = handle.S, handle.A
    good, w = torch.zeros((S, 2, 2 * A), device=DEV), torch.full((2, 2), 0.5, device=DEV)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="GPU"):
        rnad_hip.mixture(handle, good.cpu(), w)
    with pytest.raises(err, match="dtype"):
        rnad_hip.mixture(handle, good.double(), w)
    with pytest.raises(err, match="contiguous"):
        rnad_hip.mixture(handle, torch.zeros((2, S, 2 * A), device=DEV).transpose(0, 1), w)
    with pytest.raises(err, match="do not fit"):
        rnad_hip.mixture(handle, torch.zeros((S + 1, 2, 2 * A), device=DEV), w)
    with pytest.raises(err, match="do not fit"):
        rnad_hip.mixture(handle, torch.zeros((S, 2, 2 * A + 2), device=DEV), w)
    with pytest.raises(err, match="outside"):
        rnad_hip.mixture(handle, torch.zeros((S, 33, 2 * A), device=DEV), torch.zeros((2, 33), device=DEV))
    with pytest.raises(err, match=r"\[S, n, 2A\]"):
        rnad_hip.mixture(handle, torch.zeros((S, 2 * A), device=DEV), w)
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.mixture(product_tree("small"), good, w)
    with pytest.raises(err, match="weights"):
        rnad_hip.mixture(handle, good, torch.zeros((2, 3), device=DEV))
    with pytest.raises(err, match="GPU"):
        rnad_hip.mixture(handle, good, w.cpu())
    with pytest.raises(err, match="weights"):
        rnad_hip.mixture(handle, good, None)
    with pytest.raises(err, match="mix"):
        rnad_hip.mixture(handle, good, w, torch.zeros((S, 2 * A + 1), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.mixture(handle, good, w, torch.zeros((S, 2 * A), device=DEV, dtype=torch.float64))
    with pytest.raises(err, match="reach"):
        rnad_hip.mixture(handle, good, w, None, torch.zeros((S, 2, 3), device=DEV))
    with pytest.raises(err, match="mix aliases policies"):
        rnad_hip.mixture(handle, good, w, good.view(-1)[: S * 2 * A].view(S, 2 * A))
    with pytest.raises(err, match="reach aliases policies"):
        rnad_hip.mixture(handle, good, w, None, good.view(-1)[S * 2 * A:][: S * 4].view(S, 2, 2))
    # the C entry point itself: n out of range and null pointers, nothing launched
    lib = rnad_hip.lib()
    p = good.data_ptr()
    assert lib.rnad_mixture(handle.ptr, 0, p, p, p, p, None) != 0
    assert b"outside" in lib.rnad_last_error()
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.rnad_mixture(handle.ptr, 2, *args, None) != 0
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

    monkeypatch.setattr(rnad_hip, "mixture", no_sweep)
    for _ in range(2):  # the second answer comes from the tree object
        with pytest.raises(ValueError, match="not a tree: own-action reach is undefined"):
            metric.mixture(tree, [table, table])
    assert metric.index_is_tree(product_tree("small")) and not metric.index_is_tree(tree)


# ---------------------------------------------------------------------------------------------------- the tool
def test_tool_on_a_reference_written_run(tmp_path, capsys):
    from util import metric

    spec = importlib.util.spec_from_file_location("population_tool", os.path.join(ROOT, "tools", "population.py"))
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
    assert set(out) == {"names", "payoff", "nashconv", "row", "col", "value", "gap", "nash_nashconv", "uniform_nashconv"}
    payoff = np.asarray(out["payoff"])
    assert payoff.shape == (2, 2) and np.isfinite(payoff).all() and len(out["nashconv"]) == 2
    for side in (out["row"], out["col"]):
        assert len(side) == 2 and min(side) >= 0 and abs(sum(side) - 1) <= 1e-12
    assert 0 <= out["gap"] + 1e-15 and out["gap"] <= 1e-9 * max(1.0, np.abs(payoff).max())
    assert np.isfinite([out["value"], out["nash_nashconv"], out["uniform_nashconv"]]).all()
    # the same two nets through the API
    cross = tool.cross_play_tool
    tree = cross.load_tree(tar, DEV)
    _, net, params = cross.load_player(str(run_dir), (1, 0), tree, DEV)
    torch.manual_seed(0)
    res = metric.cross_play(tree, [net, cross.new_net(params, DEV)])
    np.testing.assert_allclose(np.diagonal(payoff), torch.diagonal(res.payoff).cpu().numpy(), rtol=0, atol=1e-6)
    with pytest.raises(SystemExit, match="at most 32"):
        tool.main(["--tree", tar] + [str(run_dir)] * 33)
