"""rnad_reg_evaluate on the MI355X against the fp64 sweep of tests/_regevalref.py, within its derived gates at EVERY state:

  a. values, q, residual and reach: every tree of _regref.ALL_TREES (A = 1 .. 8, C = 1 .. 4) with n = 1, 2, 3, 31 and 32 members that cycle
     through three etas, four magnets and five policies (one-hot tables with zeros inside the support and fp64 fixed points rounded to fp32
     among them).  All four outputs are pre-filled with NaN: afterwards every row is written and the rows of state 0 and of unreached states
     are exactly zero;
  b. bits: reach is rnad_hip.best_response's reach for the same tables;
  c. agreement with rnad_hip.reg_solve on its own output: the residual at most 2 * tol where it reports convergence, values within the sum
     of the two value gates;
  d. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed, gives the eager bits;
  e. the refusals of the binding and of learn.tabular.evaluate_regularized, none of which touches an output;
  f. RNaD.inner_progress, learn.tabular.TabularNeuRD against its fp64 restatement, and swap() against TabularRNaD's second update.

The worst share of each gate per case and the NeuRD figures go to reg_evaluate_errors.json in the directory that RNAD_ERRORS_DIR names, when
it is set; profiles/reg_evaluate_errors.json holds the figures of an MI355X."""
import gc
import types

import numpy as np
import pytest
import torch

import _regevalref as rv
import _regref as rr
from rnad_hip import reg_evaluate as _the_symbol_this_file_is_about  # noqa: F401  (without it nothing below can run)
from test_hip_cross_play import _trainer
from test_hip_reg_solve import product_tree

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NS = (1, 2, 3, 31, 32)
SHARES = {}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    SHARES.clear()
    yield
    if SHARES:
        rv.update_errors_file("mi355x", dict(SHARES))


def outputs(S, n, A2):
    return tuple(torch.full(shape, NAN, device=DEV) for shape in ((S, n), (S, n, A2), (S, n), (S, n)))


def run(name, n, outs=(None, None, None, None)):
    import rnad_hip

    J, L, etas = rv.inputs(name)
    policies = torch.tensor(np.ascontiguousarray(J[:, :n]), device=DEV)
    log_reg = torch.tensor(np.ascontiguousarray(L[:, :n]), device=DEV)
    return rnad_hip.reg_evaluate(product_tree(name).handle(), etas[:n].tolist(), policies, log_reg, *outs) + (policies, log_reg)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", rv.ALL_TREES)
def test_every_output_within_its_gate_at_every_state(name, n):
    c = rv.case(name)
    S, _, A2 = c.J.shape
    assert S < 10**5
    outs = outputs(S, n, A2)
    got = run(name, n, outs)
    assert all(a is b for a, b in zip(got, outs))
    values, q, residual, reach = (t.cpu().numpy() for t in outs)
    for a in (values, q, residual, reach):
        assert np.isfinite(a).all(), "a row was left unwritten, or an infinity arose from pi = 0 inside the support"
        assert (a[~c.reached] == 0).all(), "state 0 and the states no path reaches are zero"
    assert (reach[1] == 1).all()
    shares = rv.shares(c, types.SimpleNamespace(V=values, Q=q, RES=residual, R=reach), n)
    SHARES[f"{name}/n{n}"] = dict(S=int(S), **shares)
    print(f"{name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the gates")
    assert max(shares.values()) <= 1.0


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32), ("gen_a8c1", 2)])
def test_reach_carries_the_bits_of_best_response(name, n):
    import rnad_hip

    _, _, _, reach, policies, _ = run(name, n)
    want = rnad_hip.best_response(product_tree(name).handle(), policies)[3]
    assert torch.equal(reach.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("eta", rr.ETAS)
@pytest.mark.parametrize("name", ("small", "ragged", "native_a5", "gen_a7c4"))
def test_agrees_with_reg_solve_on_its_own_output(name, eta):
    import rnad_hip

    handle = product_tree(name).handle()
    tree = rr.tree_arrays(name)
    lm = rr.magnet(name, "uniform", eta)
    log_reg = torch.tensor(lm, device=DEV)
    log_policy, policy, v_solve, r_solve, iters = rnad_hip.reg_solve(handle, eta, log_reg, rr.TOL, rr.MAX_ITERS)
    values, _, residual, _ = rnad_hip.reg_evaluate(handle, eta, policy[:, None, :].contiguous(), log_reg[:, None, :].contiguous())
    solved = dict(policy=policy.cpu().numpy(), log_policy=log_policy.cpu().numpy(), values=v_solve.cpu().numpy())
    audit = rr.check(name, lm, eta, solved)
    ref = rv.reference(tree, solved["policy"][:, None, :], lm[:, None, :], [eta])
    gV = rv.gates(tree, ref, [eta])[0][:, 0]
    st = audit["reached"]
    converged = (r_solve.cpu().numpy() <= rr.TOL)[st]
    res = residual.cpu().numpy()[st, 0]
    diff = np.abs(values.cpu().numpy()[st, 0].astype(np.float64) - solved["values"][st].astype(np.float64))
    bound = gV[st] + audit["gate_b"][st]
    print(f"{name} eta={eta}: residual up to {res[converged].max() / rr.TOL:.3f} tol at {converged.sum()} converged states; values "
          f"{(diff / bound).max():.3f} of the two gates")
    SHARES[f"reg_solve/{name}/eta{eta}"] = dict(residual_over_tol=float(res[converged].max() / rr.TOL), values=float((diff / bound).max()))
    assert converged.any() and (res[converged] <= 2 * rr.TOL).all()
    assert (diff <= bound).all()


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n):
    import rnad_hip

    first = run(name, n)
    second = run(name, n)
    policies, log_reg = first[4], first[5]
    assert all(torch.equal(a, b) for a, b in zip(first[:4], second[:4]))
    handle = product_tree(name).handle()
    etas = rv.inputs(name)[2][:n].tolist()
    outs = tuple(torch.full_like(t, NAN) for t in first[:4])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.reg_evaluate(handle, etas, policies, log_reg, *outs)
    finally:
        if gc_was_on:
            gc.enable()
    for t in outs:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, first[:4]))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_no_output():
    import rnad_hip
    from learn import tabular

    tree = product_tree("small")
    handle = tree.handle()
    S, A = handle.S, handle.A
    J, L, _ = rv.inputs("small")
    policies, log_reg = torch.tensor(np.ascontiguousarray(J[:, :2]), device=DEV), torch.tensor(np.ascontiguousarray(L[:, :2]), device=DEV)
    outs = outputs(S, 2, 2 * A)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="outside"):
        rnad_hip.reg_evaluate(handle, 0.2, policies[:, :0].contiguous(), log_reg[:, :0].contiguous())
    with pytest.raises(err, match="outside"):
        rnad_hip.reg_evaluate(handle, 0.2, torch.zeros((S, 33, 2 * A), device=DEV), torch.zeros((S, 33, 2 * A), device=DEV))
    for bad in (0.0, [0.2, 0.0], [0.2, -1.0], [0.2, float("nan")], [0.2, float("inf")]):
        with pytest.raises(err, match="not positive"):
            rnad_hip.reg_evaluate(handle, bad, policies, log_reg, *outs)
    with pytest.raises(err, match="3 values of eta"):
        rnad_hip.reg_evaluate(handle, [0.2, 0.2, 0.2], policies, log_reg, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.reg_evaluate(handle, 0.2, policies.cpu(), log_reg, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg.cpu(), *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg, outs[0].cpu())
    with pytest.raises(err, match="do not fit"):
        rnad_hip.reg_evaluate(handle, 0.2, torch.zeros((S + 1, 2, 2 * A), device=DEV), log_reg, *outs)
    with pytest.raises(err, match="log_reg must be"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg[:, :1].contiguous(), *outs)
    with pytest.raises(err, match="q must be"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg, outs[0], torch.zeros((S, 2, 2 * A + 1), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.reg_evaluate(handle, 0.2, policies.double(), log_reg, *outs)
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.reg_evaluate(tree, 0.2, policies, log_reg, *outs)
    with pytest.raises(err, match="values aliases policies"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg, policies.view(-1)[: S * 2].view(S, 2))
    with pytest.raises(err, match="q aliases log_reg"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg, outs[0], log_reg)
    with pytest.raises(err, match="reach aliases values"):
        rnad_hip.reg_evaluate(handle, 0.2, policies, log_reg, outs[0], outs[1], outs[2], outs[0])
    # the C entry point itself: n and eta out of range, an overlap, null pointers -- nothing launched
    import ctypes as C

    lib = rnad_hip.lib()
    eta2 = (C.c_float * 2)(0.2, 0.2)
    ep = C.cast(eta2, C.c_void_p)
    p, r = policies.data_ptr(), log_reg.data_ptr()
    o = [t.data_ptr() for t in outs]
    assert lib.rnad_reg_evaluate(handle.ptr, 0, ep, p, r, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert lib.rnad_reg_evaluate(handle.ptr, 33, ep, p, r, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    zero = (C.c_float * 2)(0.2, 0.0)
    assert lib.rnad_reg_evaluate(handle.ptr, 2, C.cast(zero, C.c_void_p), p, r, *o, None) != 0 and b"eta[1]" in lib.rnad_last_error()
    assert lib.rnad_reg_evaluate(handle.ptr, 2, ep, p, r, o[0], p, o[2], o[3], None) != 0 and b"overlaps an input" in lib.rnad_last_error()
    assert lib.rnad_reg_evaluate(handle.ptr, 2, ep, p, r, o[0], o[1], o[0], o[3], None) != 0 and b"two outputs" in lib.rnad_last_error()
    for k in range(7):
        args = [ep, p, r] + o
        args[k] = None
        assert lib.rnad_reg_evaluate(handle.ptr, 2, *args, None) != 0 and b"null" in lib.rnad_last_error()
    # mass outside the magnet's support, through the public interface
    magnet = torch.tensor(np.exp(rr.magnet("small", "solution", 0.2).astype(np.float64)).astype(np.float32), device=DEV)
    uniform = torch.exp(tabular.uniform_log_reg(tree))
    assert bool(((uniform > 0) & (magnet == 0))[1:].any()), "the solution has zeros at legal actions"
    with pytest.raises(ValueError, match="outside its magnet's support"):
        tabular.evaluate_regularized(tree, [uniform], 0.2, reg=magnet)
    with pytest.raises(ValueError, match="no unique fixed point"):
        tabular.evaluate_regularized(tree, [uniform], 0.0)
    with pytest.raises(ValueError, match="1 to 32"):
        tabular.evaluate_regularized(tree, [], 0.2)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"
    assert torch.equal(policies.cpu(), torch.tensor(np.ascontiguousarray(J[:, :2]))) and torch.equal(log_reg.cpu(), torch.tensor(np.ascontiguousarray(L[:, :2])))


def test_a_state_with_two_parents_is_refused_before_any_sweep(monkeypatch):
    import rnad_hip
    from _gpu import tree_from_arrays
    from learn import tabular

    import _crossref as cr

    arrs = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in cr.tree_arrays("small").items()}
    index, chance = arrs["index"], arrs["chance"]
    live = (index != 0) & (chance > 0)
    levels = cr.level_order(index, chance)
    s, t, r, c = 1, *[int(v[0]) for v in np.nonzero(live[1])]
    index[s, t, r, c] = levels[2][0]
    tree = tree_from_arrays(arrs, depth_bound=arrs["meta"]["kw"]["depth_bound"])
    table = torch.exp(tabular.uniform_log_reg(tree))

    def no_sweep(*args, **kwargs):
        raise AssertionError("a sweep ran")

    monkeypatch.setattr(rnad_hip, "reg_evaluate", no_sweep)
    with pytest.raises(ValueError, match="not a tree"):
        tabular.evaluate_regularized(tree, [table], 0.2)


# ---------------------------------------------------------------------------------------------------- the public interface
def test_evaluate_regularized_with_tables_a_net_and_every_form_of_magnet():
    from learn import tabular
    from nn.net import MLP

    name = "small"
    tree = product_tree(name)
    c = rv.case(name)
    S, A = c.J.shape[0], tree.max_actions
    members = (0, 5, 10)  # (any table may meet the uniform magnet: every legal action is in its support)
    tables = [torch.tensor(c.J[:, k], device=DEV) for k in members]
    torch.manual_seed(3)
    net = MLP(A, 64, device=DEV)
    ev = tabular.evaluate_regularized(tree, tables + [net], [1.0, 0.05, 0.2, 0.2])
    assert ev.policy.shape == (S, 4, 2 * A) and ev.values.shape == (S, 4) and ev.q.shape == (S, 4, 2 * A) and ev.advantage.shape == (S, 4, 2 * A)
    assert ev.distance.shape == (4,) and ev.distance.dtype == torch.float64 and ev.distance.device.type == "cpu" and ev.max_residual.shape == (4,)
    want = (ev.reach.double() * ev.residual.double()).sum(dim=0).cpu()
    assert torch.allclose(ev.distance, want, rtol=1e-12, atol=0)
    assert torch.equal(ev.max_residual, torch.where(ev.reach > 0, ev.residual, torch.zeros_like(ev.residual)).max(dim=0).values.double().cpu())
    # against the reference: the uniform magnet for all four
    J = ev.policy.cpu().numpy()
    L = np.repeat(rr.magnet(name, "uniform", 0.2)[:, None, :], 4, axis=1)
    etas = [1.0, 0.05, 0.2, 0.2]
    ref = rv.reference(c.tree, J, L, etas)
    gV, gQ, gRES, gR = rv.gates(c.tree, ref, etas)
    R = ref.depth >= 0
    assert rv.share(ev.values.cpu().numpy()[R], ref.V[R], gV[R]) <= 1 and rv.share(ev.residual.cpu().numpy()[R], ref.RES[R], gRES[R]) <= 1
    # the advantage: zero where pi = 0 or outside the support; elsewhere q - eta (log pi - log mu) minus its pi-weighted mean per side,
    # recomputed in fp64 from the returned q.  Every fp32 step (the log: 1 ulp, the difference, two products, at most A sums, the centring)
    # is relative to |q|, eta |log pi|, eta |log mu| or their pi-weighted sum: at most A + 8 roundings of their total
    adv = ev.advantage.cpu().numpy().astype(np.float64)
    on = ref.on & (J > 0)
    assert (adv[~on] == 0).all()
    eta64 = np.asarray(etas, np.float32).astype(np.float64)[None, :, None]
    logJ, lm = np.log(np.where(on, J, 1.0).astype(np.float64)), np.where(on, L, 0.0).astype(np.float64)
    qd = ev.q.cpu().numpy().astype(np.float64)
    raw = np.where(on, qd - eta64 * (logJ - lm), 0.0)
    size = np.where(on, np.abs(qd) + eta64 * (np.abs(logJ) + np.abs(lm)), 0.0)
    per_side = lambda x: np.repeat((J * x).reshape(S, 4, 2, A).sum(axis=3), A, axis=2)  # noqa: E731
    want_adv = np.where(on, raw - per_side(raw), 0.0)
    tol = (A + 8) * rv.U * (size + per_side(size))
    print(f"advantage: {float(np.where(tol > 0, np.abs(adv - want_adv) / np.where(tol > 0, tol, 1), 0)[R].max()):.3f} of its tolerance")
    assert (np.abs(adv - want_adv)[R] <= tol[R]).all()
    # one magnet for all, one per player, a ready log table: the same numbers
    one = tabular.evaluate_regularized(tree, tables, 0.2)
    table = tabular.evaluate_regularized(tree, tables, 0.2, reg=torch.exp(tabular.uniform_log_reg(tree)))
    assert torch.allclose(table.values, one.values, atol=1e-5) and torch.allclose(table.residual, one.residual, atol=1e-5)
    per = tabular.evaluate_regularized(tree, tables, 0.2, reg=[None, None, None])
    log = tabular.evaluate_regularized(tree, tables, 0.2, log_reg=tabular.uniform_log_reg(tree))
    log3 = tabular.evaluate_regularized(tree, tables, 0.2, log_reg=tabular.uniform_log_reg(tree)[:, None, :].expand(S, 3, 2 * A))
    for other in (per, log, log3):
        assert torch.equal(one.values, other.values) and torch.equal(one.residual, other.residual) and torch.equal(one.advantage, other.advantage)
    # an unnormalised magnet: the softmax and the fixed point do not care, the values shift by eta * log of the factor per side, which cancels
    shifted = tabular.evaluate_regularized(tree, tables, 0.2, log_reg=tabular.uniform_log_reg(tree) + 0.5)
    assert torch.allclose(shifted.residual, one.residual, atol=64 * rv.U) and torch.allclose(shifted.q, one.q, atol=1e-4)


def test_rnad_inner_progress():
    tree = product_tree("small")
    rn = _trainer(tree, "inner", 7)
    S, A = tree.value_tensor.shape[0], tree.max_actions
    ev = rn.inner_progress()
    assert ev.policy.shape == (S, 2, 2 * A) and ev.values.shape == (S, 2) and ev.distance.shape == (2,)
    want = (ev.reach.cpu().numpy().astype(np.float64) * ev.residual.cpu().numpy().astype(np.float64)).sum(axis=0)
    assert np.allclose(ev.distance.numpy(), want, rtol=1e-12, atol=0)
    assert torch.isfinite(ev.values).all() and torch.isfinite(ev.advantage).all() and (ev.distance > 0).all()
    for alpha in (0.0, 0.5, 1.0):  # all four nets start equal: every alpha names the same magnet
        again = rn.inner_progress(alpha)
        assert torch.equal(again.residual, ev.residual) and torch.equal(again.values, ev.values)
    with torch.no_grad():  # two different regularisation nets: the mixed magnet is no log of a distribution, and no 0 * -inf arises
        for p in rn.net_reg_.parameters():
            p.add_(0.05 * torch.randn_like(p))
    mixed = rn.inner_progress(0.5)
    assert torch.isfinite(mixed.values).all() and torch.isfinite(mixed.residual).all() and not torch.equal(mixed.residual, ev.residual)
    with pytest.raises(ValueError, match="alpha"):
        rn.inner_progress(1.5)
    rn.eta = 0.0
    with pytest.raises(ValueError, match="eta = 0"):
        rn.inner_progress()
    from learn.rnad import RNaD

    fresh = RNaD(tree=tree, device=DEV, directory_name="inner_fresh", batch_size=256, eta=0.2,
                 net_params={"type": "MLP", "max_actions": A, "width": 64})
    with pytest.raises(ValueError, match="not initialised"):
        fresh.inner_progress()


def test_tabular_neurd_against_its_fp64_restatement():
    from learn import tabular

    cfg = rv.NEURD
    want, floor, first = rv.neurd_loop()
    tree = product_tree(cfg["tree"])
    loop = tabular.TabularNeuRD(tree, cfg["eta"], cfg["lr"])
    start = float(loop.evaluate().max_residual[0])
    loop.run(cfg["steps"])
    got = loop.residual_history
    print(f"max residual {start:.4g} -> {got[-1]:.4g} after {len(got)} steps; fp64: {first:.4g} -> {want[-1]:.4g}; gate {floor:.3g}")
    SHARES["neurd"] = dict(tree=cfg["tree"], eta=cfg["eta"], lr=cfg["lr"], steps=cfg["steps"], start=start, max_residual=got[-1],
                           fp64_max_residual=want[-1], residual_gate=floor, distance=loop.distance_history[-1])
    assert len(got) == cfg["steps"] and len(loop.distance_history) == cfg["steps"]
    assert abs(start - first) <= floor
    # each state's game is strongly monotone: roundings are damped, not accumulated -- a factor of two over the fp64 figure, and the gate
    # of the residual itself as the floor
    assert got[-1] <= 2 * want[-1] + floor
    assert (loop.logits[~tabular.legal_mask(tree)] == float("-inf")).all(), "entries outside the support never move"
    with pytest.raises(ValueError, match="lr \\* eta below 1"):
        tabular.TabularNeuRD(tree, 0.5, 2.0)
    with pytest.raises(ValueError, match="eta = 0"):
        tabular.TabularNeuRD(tree, 0.0, 0.1)


def test_swap_composes_outer_iterations():
    from learn import tabular

    name, eta = "small", 0.2
    tree = product_tree(name)
    gp, gv = rr.committed_gate_c()
    exact = tabular.TabularRNaD(tree, eta)
    exact.update()
    loop = tabular.TabularNeuRD(tree, eta, 0.2)
    loop.logits.copy_(exact.solution.log_policy)  # the inner loop has arrived at the fixed point of the uniform magnet
    at_fixed_point = loop.evaluate()
    assert float(at_fixed_point.max_residual[0]) <= 2 * rr.TOL
    loop.swap()
    assert torch.equal(loop.logits, loop.log_reg) and float(loop.evaluate().residual.max()) > 10 * rr.TOL
    second = tabular._solve(tree, eta, loop.log_reg, rr.TOL, rr.MAX_ITERS)
    exact.update()
    dp = float((second.policy - exact.solution.policy).abs().max())
    dv = float((second.values - exact.solution.values).abs().max())
    print(f"after swap() the exact solve lies {dp:.3g} / {dv:.3g} from TabularRNaD's second update (gates {gp:.3g} / {gv:.3g})")
    SHARES["swap"] = dict(policy=dp / gp, values=dv / gv)
    assert second.unconverged == 0 and dp <= gp and dv <= gv


# ---------------------------------------------------------------------------------------------------- the tool
def test_tool_evaluates_a_reference_written_run(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import shutil

    from _util import GOLDEN

    root = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    spec = importlib.util.spec_from_file_location("tabular_rnad_tool", os.path.join(root, "tools", "tabular_rnad.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run_dir = tmp_path / "from_reference"
    os.makedirs(run_dir / "1")
    shutil.copy(os.path.join(GOLDEN, "ref_run_params"), run_dir / "params")
    shutil.copy(os.path.join(GOLDEN, "ref_run_ckpt_1_0"), run_dir / "1" / "0")
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, "--evaluate", str(run_dir)])
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert lines == out and len(out) == 1
    rec = out[0]
    assert set(rec) == {"run", "m", "n", "alpha", "eta", "players", "distance", "max_residual", "root_value"}
    assert (rec["run"], rec["m"], rec["n"], rec["alpha"], rec["players"]) == ("from_reference", 1, 0, 0.0, ["net", "net_target"])
    assert abs(rec["eta"] - 0.2) < 1e-12 and len(rec["distance"]) == len(rec["max_residual"]) == len(rec["root_value"]) == 2
    assert all(np.isfinite(v) and v >= 0 for v in rec["distance"] + rec["max_residual"]) and all(np.isfinite(v) for v in rec["root_value"])
    assert all(d >= m * (1 - 1e-6) for d, m in zip(rec["distance"], rec["max_residual"])), "the root has reach 1: distance >= its residual"
    other = tool.main(["--tree", tar, "--evaluate", str(run_dir), "--alpha", "1", "--eta", "0.5"])
    capsys.readouterr()
    assert other[0]["alpha"] == 1.0 and other[0]["eta"] == 0.5 and other[0]["distance"] != rec["distance"]
