"""rnad_reg_solve on the MI355X against tests/_regref.py, at EVERY reached state of every case (trees x eta x magnets of _regref.cases()):

  a. residual, recomputed in fp64 from the outputs and their own children values, <= 2 * tol; b. value within its derived gate;
  c. policy and value within gate (c) of the fp64 fixed point, as profiles/reg_solve_errors.json records it (tests/test_reg_solve.py
     holds that file to what _regref.gate_c() computes); e. anchor: mu = solution answers in 0 iterations with pi = mu and
     V = root_value within _regref.anchor_bound on every tree (golden trees: within gate (b) too).  Outputs are pre-filled with NaN
     (iters with -1): afterwards everything is finite except -inf in log_policy, the rows of state 0 and of unreachable states are
     as specified, and no state is unconverged;
  - max_iters = 3 at eta = 0.05 reports iters == 3 with a residual above tol somewhere, and still passes (b);
  - two runs and a replayed torch.cuda.graph give identical bits;
  - TabularRNaD, RNaD.tabular_baseline and tools/tabular_rnad.py.

The worst shares go to reg_solve_errors.json (key "mi355x") in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/reg_solve_errors.json holds the figures of an MI355X."""
import functools
import gc
import importlib.util
import json
import os
import zlib

import numpy as np
import pytest
import torch

import _crossref as cr
import _regref as rr
from _util import GOLDEN, TREES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
SHARES = {}
KEYS = ("log_policy", "policy", "values", "residual", "iters")


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    SHARES.clear()
    yield
    if SHARES:
        gp, gv = rr.committed_gate_c()
        rr.update_errors_file("mi355x", dict(policy_gate=gp, value_gate=gv, cases=dict(SHARES)))


@functools.lru_cache(maxsize=None)
def product_tree(name):
    from _gpu import tree_from_arrays

    arrs = rr.tree_arrays(name)
    tree = tree_from_arrays(arrs, depth_bound=arrs["meta"]["kw"]["depth_bound"])
    tree.hash = arrs["meta"].get("hash", zlib.crc32(name.encode()))
    return tree


def buffers(name):
    S, A2 = rr.legal_mask(rr.tree_arrays(name)).shape
    nan = float("nan")
    return dict(log_policy=torch.full((S, A2), nan, device=DEV), policy=torch.full((S, A2), nan, device=DEV), values=torch.full((S,), nan, device=DEV),
                residual=torch.full((S,), nan, device=DEV), iters=torch.full((S,), -1, device=DEV, dtype=torch.int32))


def run(name, reg, eta, tol=rr.TOL, max_iters=rr.MAX_ITERS, out=None):
    import rnad_hip

    out = buffers(name) if out is None else out
    got = rnad_hip.reg_solve(product_tree(name).handle(), eta, reg, tol, max_iters, **out)
    assert all(g is out[k] for g, k in zip(got, KEYS))
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_rows(name, got):
    """Everything finite except -inf in log_policy; state 0 and unreachable rows zero with log_policy -inf."""
    S = got["values"].shape[0]
    st = np.concatenate(rr.levels_of(name))
    rest = np.setdiff1d(np.arange(S), st)
    assert 0 in rest
    for k in ("policy", "values", "residual"):
        assert np.isfinite(got[k]).all(), f"{k}: a row was left unwritten"
        assert (got[k][rest] == 0).all(), k
    assert (got["iters"] >= 0).all() and (got["iters"][rest] == 0).all()
    assert not np.isnan(got["log_policy"]).any() and not (got["log_policy"] == np.inf).any()
    assert (got["log_policy"][rest] == -np.inf).all()
    assert ((got["log_policy"] == -np.inf) <= (got["policy"] == 0)).all()
    return st


@pytest.mark.parametrize("eta", rr.ETAS)
@pytest.mark.parametrize("name", rr.ALL_TREES)
def test_gates_at_every_reached_state(name, eta):
    gp, gv = rr.committed_gate_c()
    tree = rr.tree_arrays(name)
    assert tree["index"].shape[0] < 10**5
    for kind in rr.MAGNETS:
        reg, star = rr.magnet(name, kind, eta), rr.star(name, kind, eta)
        got = host(run(name, torch.tensor(reg, device=DEV), eta))
        st = check_rows(name, got)
        unconverged = int(((got["iters"][st] >= rr.MAX_ITERS) & ~(got["residual"][st] <= rr.TOL)).sum())
        a, b = rr.shares(name, reg, eta, got)
        dp, dv = rr.distance(name, got, star)
        SHARES[f"{name}/eta{eta}/{kind}"] = dict(residual_over_tol=a, gate_b_share=b, policy_distance_share=dp / gp, value_distance_share=dv / gv,
                                                 max_iters=int(got["iters"][st].max()))
        print(f"{name} eta={eta} {kind}: residual {a:.3f} tol, value {b:.3f} of gate (b), distance {dp / gp:.3f} / {dv / gv:.3f} of gate (c), "
              f"at most {got['iters'][st].max()} iterations")
        assert unconverged == 0
        assert a <= 2.0
        assert b <= 1.0
        assert dp <= gp and dv <= gv
        if kind == "solution":
            c = rr.check(name, reg, eta, got)
            assert (got["iters"][st] == 0).all()
            assert np.abs(got["policy"][st].astype(np.float64) - np.asarray(tree["solution"], np.float64)[st]).max() <= 8 * rr.U
            dv = np.abs(got["values"][st].astype(np.float64) - np.asarray(tree["root_value"], np.float64)[st, 0])
            assert (dv <= rr.anchor_bound(name, eta, got)[st]).all()
            if name in TREES:
                assert (dv <= c["gate_b"][st]).all()


@pytest.mark.parametrize("name", ("small", "native_a5", "gen_a8c1"))
def test_three_iterations_are_reported_and_the_value_still_fits_its_policy(name):
    eta = 0.05
    reg = rr.magnet(name, "uniform", eta)
    got = host(run(name, torch.tensor(reg, device=DEV), eta, max_iters=3))
    st = check_rows(name, got)
    assert got["iters"][st].max() == 3
    cut = got["iters"][st] == 3
    assert (got["residual"][st][cut] > rr.TOL).any()
    assert (got["residual"][st][~cut] <= rr.TOL).all()
    _, b = rr.shares(name, reg, eta, got)
    assert b <= 1.0


@pytest.mark.parametrize("name,eta,kind", [("small", 0.2, "uniform"), ("ragged", 0.05, "softmax"), ("native_a5", 1.0, "after4")])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, eta, kind):
    reg = torch.tensor(rr.magnet(name, kind, eta), device=DEV)
    first, second = run(name, reg, eta), run(name, reg, eta)
    for k in KEYS:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
    out = buffers(name)
    product_tree(name).handle()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            run(name, reg, eta, out=out)
    finally:
        if gc_was_on:
            gc.enable()
    for _ in range(2):
        for k in KEYS:
            out[k].fill_(-1 if k == "iters" else float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(out[k].view(torch.int32), first[k].view(torch.int32)), k


@pytest.mark.parametrize("name", ("small", "ragged"))
def test_tabular_rnad_against_the_fp64_chain(name):
    from learn.tabular import TabularRNaD, solve_regularized
    from util import metric

    eta = 0.2
    tree = product_tree(name)
    solver = TabularRNaD(tree, eta)
    assert solver.run(4) is solver.nashconv_history and len(solver.nashconv_history) == 4
    assert solver.unconverged_history == [0, 0, 0, 0]
    gp, _ = rr.committed_gate_c()
    depth = len(rr.levels_of(name))
    want = [rr.nashconv64(name, sol["policy"]) for sol in rr.chain(name, eta)]
    print(f"{name}: NashConv {solver.nashconv_history} against fp64 {want}")
    for got, ref in zip(solver.nashconv_history, want):
        assert abs(got - ref) <= gp * 2 * depth
    assert torch.equal(solver.policy, solver.solution.policy) and solver.values.shape == (tree.value_tensor.shape[0],)
    # the first update is solve_regularized from the uniform magnet, bit for bit
    once = solve_regularized(tree, eta)
    again = TabularRNaD(tree, eta)
    again.update()
    assert torch.equal(once.policy, again.policy) and once.unconverged == 0
    # the saddle inequality of the tree's solution against the table, within the cross-play sweep's own gate
    arrs = rr.tree_arrays(name)
    tables = [solver.policy, torch.tensor(np.asarray(arrs["solution"], np.float32), device=DEV)]
    res = metric.cross_play(tree, tables)
    V, B, h = cr.reference(arrs, np.stack([t.cpu().numpy() for t in tables], axis=1))
    g = cr.gate(arrs, B, h)
    assert cr.share(res.values.cpu().numpy(), V, g) <= 1.0
    payoff = res.payoff.cpu().numpy().astype(np.float64)
    slack = 2 * g[1].max()
    assert payoff[1, 0] + slack >= payoff[1, 1] >= payoff[0, 1] - slack
    with pytest.raises(ValueError, match="no unique fixed point"):
        TabularRNaD(tree, 0.0)


def test_rnad_tabular_baseline(monkeypatch, tmp_path):
    from learn.rnad import RNaD
    from learn.tabular import TabularRNaD

    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    tree = product_tree("small")
    rn = RNaD(tree=tree, device=DEV, directory_name="t", batch_size=256, eta=0.5)
    assert rn.tabular_baseline(3) == TabularRNaD(tree, 0.5).run(3)
    with pytest.raises(ValueError, match="no unique fixed point"):
        RNaD(tree=tree, device=DEV, directory_name="t0", batch_size=256, eta=0).tabular_baseline(3)


def test_binding_refusals():
    import rnad_hip

    handle = product_tree("small").handle()
    S, A = handle.S, handle.A
    good = torch.zeros((S, 2 * A), device=DEV)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="GPU"):
        rnad_hip.reg_solve(handle, 0.2, good.cpu())
    with pytest.raises(err, match="dtype"):
        rnad_hip.reg_solve(handle, 0.2, good.double())
    with pytest.raises(err, match="does not fit"):
        rnad_hip.reg_solve(handle, 0.2, torch.zeros((S + 1, 2 * A), device=DEV))
    with pytest.raises(err, match="eta"):
        rnad_hip.reg_solve(handle, 0.0, good)
    with pytest.raises(err, match="tol"):
        rnad_hip.reg_solve(handle, 0.2, good, tol=0.0)
    with pytest.raises(err, match="max_iters"):
        rnad_hip.reg_solve(handle, 0.2, good, max_iters=0)
    with pytest.raises(err, match="values"):
        rnad_hip.reg_solve(handle, 0.2, good, values=torch.zeros((S, 2), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.reg_solve(handle, 0.2, good, iters=torch.zeros((S,), device=DEV))
    with pytest.raises(err, match="aliases"):
        rnad_hip.reg_solve(handle, 0.2, good, policy=good)
    # overlap anywhere, not only at the first byte, and between two outputs
    big = torch.zeros((2 * S * 2 * A,), device=DEV)
    with pytest.raises(err, match="aliases log_reg"):
        rnad_hip.reg_solve(handle, 0.2, big[: S * 2 * A].view(S, 2 * A), policy=big[2 * A: 2 * A + S * 2 * A].view(S, 2 * A))
    shared = torch.zeros((S, 2 * A), device=DEV)
    with pytest.raises(err, match="aliases log_policy"):
        rnad_hip.reg_solve(handle, 0.2, good, log_policy=shared, policy=shared)
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.reg_solve(product_tree("small"), 0.2, good)
    lib = rnad_hip.lib()
    columns = [torch.zeros((S,), device=DEV) for _ in range(3)]
    col = [t.data_ptr() for t in columns]
    assert lib.rnad_reg_solve(handle.ptr, 0.2, 1e-5, 10, good.data_ptr(), big.data_ptr(), big.data_ptr() + 8 * A, *col, None) != 0
    assert b"two outputs overlap" in lib.rnad_last_error()
    assert lib.rnad_reg_solve(handle.ptr, 0.2, 1e-5, 10, big.data_ptr() + 8 * A, big.data_ptr() + 4 * S * 2 * A + 8 * A, shared.data_ptr(),
                              big.data_ptr(), *col[:2], None) != 0
    assert b"aliases log_reg" in lib.rnad_last_error()
    p = good.data_ptr()
    assert lib.rnad_reg_solve(handle.ptr, 0.0, 1e-5, 10, p, p, p, p, p, p, None) != 0
    assert b"eta" in lib.rnad_last_error()
    assert lib.rnad_reg_solve(handle.ptr, 0.2, 1e-5, 10, p, p, p, p, p, p, None) != 0
    assert b"aliases" in lib.rnad_last_error()


def test_tool_on_a_reference_written_tree(capsys):
    spec = importlib.util.spec_from_file_location("tabular_rnad_tool", os.path.join(ROOT, "tools", "tabular_rnad.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, "--eta", "0.2", "1", "--updates", "5"])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert lines == out and [x["eta"] for x in out] == [0.2, 1.0]
    for x in out:
        assert len(x["nashconv"]) == 5 and np.isfinite(x["nashconv"]).all() and x["unconverged"] == [0] * 5
        assert x["nashconv"][-1] < x["nashconv"][0], "five updates bring the table closer to equilibrium"
    assert out[0]["nashconv"][0] < out[1]["nashconv"][0], "the weaker regularisation starts closer to equilibrium"
    with pytest.raises(SystemExit, match="positive"):
        tool.main(["--tree", tar, "--eta", "0"])
