"""rnad_vtrace_expect on the MI355X against the fp64 sweep of tests/_vtexpref.py (which tests/test_vtrace_expect.py ties to the enumeration
of every episode), within its derived gates at EVERY state:

  a. target, target_given_row, q and reach: every tree of _regref.ALL_TREES (A = 1 .. 8, C = 1 .. 4) with n = 1, 2, 3, 31 and 32 members
     that cycle through the four hyperparameter sets of _learnref.HP and three behaviours (on-policy, a seeded softmax, one with zeros).
     All outputs and the workspace are pre-filled with NaN: afterwards every output row is written and the rows of state 0 and of
     unreached states are exactly zero;
  b. bits: reach is rnad_hip.best_response's reach for the table mu;
  c. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed, gives the eager bits;
  d. the refusals of the binding, the C entry point and learn.vtrace.expected_update, none of which touches an output;
  e. learn.vtrace.expected_update on row tables and RNaD.expected_update on a trainer's nets against the reference fed the same rows;
  f. no instantiation uses scratch (the built library's metadata).

The worst share of each gate per case goes to vtrace_expect_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/vtrace_expect_errors.json holds the figures of an MI355X."""
import gc
import os

import numpy as np
import pytest
import torch

import _learnref as lr
import _vtexpref as vx
from rnad_hip import vtrace_expect as _the_symbol_this_file_is_about  # noqa: F401  (without it nothing below can run)
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
        vx.update_errors_file("mi355x", dict(SHARES))


def outputs(S, n, A):
    shapes = ((S, n, 2), (S, n, A), (S, n, 2 * A), (S, n), (vx.workspace(S, A, n),))
    return tuple(torch.full(shape, NAN, device=DEV) for shape in shapes)


def run(name, n, outs=(None,) * 5):
    import rnad_hip

    MU, PIP, LPOL, VV, hyper = vx.inputs(name)
    tens = tuple(torch.tensor(np.ascontiguousarray(x[:, :n]), device=DEV) for x in (MU, PIP, LPOL, VV))
    return rnad_hip.vtrace_expect(product_tree(name).handle(), hyper[:n].tolist(), *tens, *outs) + tens


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", vx.ALL_TREES)
def test_every_output_within_its_gate_at_every_state(name, n):
    c = vx.case(name)
    S, _, A2 = c.MU.shape
    assert S < 10**5
    outs = outputs(S, n, A2 // 2)
    got = run(name, n, outs)
    assert all(a is b for a, b in zip(got[:4], outs))
    arrays = dict(zip(vx.OUTPUTS, (t.cpu().numpy() for t in outs[:4])))
    for a in arrays.values():
        assert np.isfinite(a).all(), "a row was left unwritten"
        assert (a[~c.reached] == 0).all(), "state 0 and the states no path reaches are zero"
    assert (arrays["reach"][1] == 1).all()
    shares = vx.shares(c, arrays, n)
    SHARES[f"{name}/n{n}"] = dict(S=int(S), **shares)
    print(f"{name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the gates")
    assert max(shares.values()) <= 1.0


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32), ("gen_a8c1", 2)])
def test_reach_carries_the_bits_of_best_response(name, n):
    import rnad_hip

    got = run(name, n)
    want = rnad_hip.best_response(product_tree(name).handle(), got[4])[3]
    assert torch.equal(got[3].view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n):
    import rnad_hip

    first = run(name, n)
    second = run(name, n)
    assert all(torch.equal(a, b) for a, b in zip(first[:4], second[:4]))
    handle = product_tree(name).handle()
    hyper = vx.inputs(name)[4][:n].tolist()
    S, A = handle.S, handle.A
    outs = outputs(S, n, A)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.vtrace_expect(handle, hyper, *first[4:], *outs)
    finally:
        if gc_was_on:
            gc.enable()
    for t in outs:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs[:4], first[:4]))


def test_refusals_touch_no_output():
    import ctypes as C

    import rnad_hip

    tree = product_tree("small")
    handle = tree.handle()
    S, A = handle.S, handle.A
    MU, PIP, LPOL, VV, hyper = vx.inputs("small")
    mu, pip, lpol, vv = (torch.tensor(np.ascontiguousarray(x[:, :2]), device=DEV) for x in (MU, PIP, LPOL, VV))
    hy = hyper[:2].tolist()
    outs = outputs(S, 2, A)
    err = rnad_hip.RnadHipError
    big = torch.zeros((S, 33, 2 * A), device=DEV)
    with pytest.raises(err, match="outside"):
        rnad_hip.vtrace_expect(handle, [], mu[:, :0].contiguous(), pip[:, :0].contiguous(), lpol[:, :0].contiguous(), vv[:, :0].contiguous())
    with pytest.raises(err, match="outside"):
        rnad_hip.vtrace_expect(handle, [hy[0]] * 33, big, big.clone(), big.clone(), torch.zeros((S, 33, 2), device=DEV))
    for bad, what in (((0.2, 0.0, 1.0, 1.0, 1.0), "gamma"), ((0.2, -1.0, 1.0, 1.0, 1.0), "gamma"), ((0.2, float("nan"), 1.0, 1.0, 1.0), "gamma"),
                      ((0.2, 1.0, 1.0, -0.5, 1.0), "clips"), ((0.2, 1.0, 1.0, 1.0, -1e-3), "clips"), ((float("inf"), 1.0, 1.0, 1.0, 1.0), "finite")):
        with pytest.raises(err, match=what):
            rnad_hip.vtrace_expect(handle, [hy[0], bad], mu, pip, lpol, vv, *outs)
    with pytest.raises(err, match="2 rows"):
        rnad_hip.vtrace_expect(handle, [hy[0]] * 3, mu, pip, lpol, vv, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.vtrace_expect(handle, hy, mu.cpu(), pip, lpol, vv, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol.cpu(), vv, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv, outs[0].cpu())
    with pytest.raises(err, match="does not fit"):
        rnad_hip.vtrace_expect(handle, hy, torch.zeros((S + 1, 2, 2 * A), device=DEV), pip, lpol, vv, *outs)
    with pytest.raises(err, match="vv must be"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv[:, :1].contiguous(), *outs)
    with pytest.raises(err, match="q must be"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv, outs[0], outs[1], torch.zeros((S, 2, 2 * A + 1), device=DEV))
    with pytest.raises(err, match="workspace must be"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv, *outs[:4], torch.zeros((7,), device=DEV))
    with pytest.raises(err, match="dtype"):
        rnad_hip.vtrace_expect(handle, hy, mu.double(), pip, lpol, vv, *outs)
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.vtrace_expect(tree, hy, mu, pip, lpol, vv, *outs)
    with pytest.raises(err, match="q aliases pip"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv, outs[0], outs[1], pip)
    with pytest.raises(err, match="reach aliases target"):
        rnad_hip.vtrace_expect(handle, hy, mu, pip, lpol, vv, outs[0], outs[1], outs[2], outs[0].view(-1)[: S * 2].view(S, 2))
    # the C entry point itself: nothing launched
    lib = rnad_hip.lib()
    flat = lambda rows: C.cast((C.c_float * (5 * len(rows)))(*[x for r in rows for x in r]), C.c_void_p)  # noqa: E731
    keep = [(C.c_float * 10)(*[x for r in hy for x in r])]
    hp = C.cast(keep[0], C.c_void_p)
    i = [t.data_ptr() for t in (mu, pip, lpol, vv)]
    o = [t.data_ptr() for t in outs]
    assert lib.rnad_vtrace_expect(handle.ptr, 0, hp, *i, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert lib.rnad_vtrace_expect(handle.ptr, 33, hp, *i, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert lib.rnad_vtrace_expect(handle.ptr, 2, flat([hy[0], (0.2, 0.0, 1.0, 1.0, 1.0)]), *i, *o, None) != 0 and b"gamma[1]" in lib.rnad_last_error()
    assert lib.rnad_vtrace_expect(handle.ptr, 2, flat([hy[0], (0.2, 1.0, 1.0, -1.0, 1.0)]), *i, *o, None) != 0 and b"clips" in lib.rnad_last_error()
    assert lib.rnad_vtrace_expect(handle.ptr, 2, hp, *i, o[0], o[1], i[1], o[3], o[4], None) != 0 and b"overlaps an input" in lib.rnad_last_error()
    assert lib.rnad_vtrace_expect(handle.ptr, 2, hp, *i, o[0], o[1], o[2], o[2], o[4], None) != 0 and b"two outputs" in lib.rnad_last_error()
    for k in range(10):
        args = [hp] + i + o
        args[k] = None
        assert lib.rnad_vtrace_expect(handle.ptr, 2, *args, None) != 0 and b"null" in lib.rnad_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"
    assert torch.equal(mu.cpu(), torch.tensor(np.ascontiguousarray(MU[:, :2])))


# ---------------------------------------------------------------------------------------------------- the public interface
def _reference_for_rows(name, mu_rows, pip_rows, lpol_rows, vv_rows, hp):
    """(ref, gates) of the single member whose row tables [2S, (A)] are given, with the learner's hyperparameters."""
    tree = vx.rr.tree_arrays(name)
    S = np.asarray(tree["index"]).shape[0]
    ref = vx.reference(np.float64, tree, *(vx.to_sides(x, S)[:, None] for x in (mu_rows, pip_rows, lpol_rows, vv_rows)), [vx.hyper_of(hp)])
    return tree, ref, vx.gates(tree, ref)


def _shares_of(ev, ref, g, S):
    R = ref.depth >= 0
    A = ev.q.shape[1]
    tg = ev.target.cpu().numpy()
    q = ev.q.cpu().numpy()
    got = dict(target=np.stack([tg[:S], tg[S:]], 1)[:, None], target_given_row=ev.target_given_row.cpu().numpy()[:, None],
               q=np.concatenate([q[:S], q[S:]], 1)[:, None], reach=ev.reach.cpu().numpy()[:, None])
    want = vx.values_of(ref)
    assert A == want["target_given_row"].shape[2]
    return {k: vx.share(got[k][R], want[k][R], g[k][R]) for k in vx.OUTPUTS}


@pytest.mark.parametrize("hp_name", ("H0", "H1"))
def test_expected_update_on_row_tables(hp_name):
    import rnad_hip
    from learn import vtrace

    name = "small"
    tree = product_tree(name)
    arrs = vx.rr.tree_arrays(name)
    S, A = tree.value_tensor.shape[0], tree.max_actions
    hp = lr.HP[hp_name]
    rng = np.random.default_rng(17)
    legal_tab = lr.legal_table(np.asarray(arrs["legal"]))
    tables = lr.draw_tables(rng, legal_tab, hp)
    _, pip64, lpol64 = vx.row_inputs(np.float64, tables, legal_tab, hp)
    mu = vx.behaviour_table("zeros", rng, legal_tab, pip64).astype(np.float32)
    dev = lambda x: torch.tensor(np.asarray(x, np.float32), device=DEV)  # noqa: E731
    params = rnad_hip.make_learn_params(**lr.hp_kwargs(hp))
    ev = vtrace.expected_update(tree, dev(mu), dev(tables["logit"]), dev(tables["v"]), dev(tables["v_target"]), dev(tables["logit_reg"]),
                                dev(tables["logit_reg_"]), params)
    assert np.array_equal(ev.pi_processed.cpu().numpy(), pip64.astype(np.float32)), "process_policy: every row has its decision margin"
    _, ref, g = _reference_for_rows(name, mu, pip64.astype(np.float32), lpol64.astype(np.float32), tables["v_target"], hp)
    shares = _shares_of(ev, ref, g, S)
    SHARES[f"expected_update/{hp_name}"] = shares
    print(f"expected_update {hp_name}: {shares} of the gates")
    assert max(shares.values()) <= 1.0
    # the host side: the formulas of _vtexpref.expected_tables on the sweep's own outputs
    want = vx.expected_tables(arrs, tables, legal_tab, mu, pip64, lpol64, hp, ev.target.cpu().numpy().astype(np.float64),
                              ev.q.cpu().numpy().astype(np.float64), ev.reach.cpu().numpy().astype(np.float64))
    assert abs(ev.length - want["length"]) <= 1e-12 * want["length"]
    assert ev.dv_tab.shape == (2 * S, 1) and ev.dlogit_tab.shape == (2 * S, A) and ev.linear.shape == (2 * S,)
    assert np.allclose(ev.dv_tab.cpu().numpy()[:, 0], want["dv_tab"], rtol=1e-6, atol=1e-9)
    assert np.allclose(ev.dlogit_tab.cpu().numpy(), want["dlogit_tab"], rtol=1e-5, atol=1e-7)
    assert np.array_equal(ev.linear.cpu().numpy(), want["linear"])
    assert ev.target_bias.dtype == torch.float64 and ev.target_bias.device.type == "cpu"
    assert np.allclose(ev.target_bias.numpy(), want["target_bias"], rtol=1e-6)
    # a behaviour that never draws what the policy plays at a reached state
    starved = mu.copy()
    played = int(np.flatnonzero(pip64[S + 1] > 0)[0])  # the column player at the root
    others = [b for b in np.flatnonzero(legal_tab[S + 1] > 0) if b != played]
    if others:
        starved[S + 1] = 0
        starved[S + 1, others[0]] = 1
        with pytest.raises(ValueError, match="never draws"):
            vtrace.expected_update(tree, dev(starved), dev(tables["logit"]), dev(tables["v"]), dev(tables["v_target"]), dev(tables["logit_reg"]),
                                   dev(tables["logit_reg_"]), params)
    with pytest.raises(ValueError, match="logit must be"):
        vtrace.expected_update(tree, dev(mu), dev(tables["logit"])[:-1], dev(tables["v"]), dev(tables["v_target"]), dev(tables["logit_reg"]),
                               dev(tables["logit_reg_"]), params)


def test_rnad_expected_update():
    import rnad_hip
    from learn import vtrace

    name = "small"
    tree = product_tree(name)
    rn = _trainer(tree, "expected", 7)
    with torch.no_grad():  # four different nets, as in the middle of a run
        for k, module in enumerate((rn.net_target, rn.net_reg, rn.net_reg_)):
            for p in module.parameters():
                p.add_(0.05 * (k + 1) * torch.randn_like(p))
    S, A = tree.value_tensor.shape[0], tree.max_actions
    alpha = 0.3
    ev = rn.expected_update(alpha)
    assert ev.target.shape == (2 * S,) and ev.q.shape == (2 * S, A) and ev.target_given_row.shape == (S, A) and ev.reach.shape == (S,)
    for t in (ev.target, ev.q, ev.target_given_row, ev.reach, ev.dv_tab, ev.dlogit_tab):
        assert torch.isfinite(t).all()
    assert ev.length >= 1 and (ev.target_bias >= 0).all()
    # the reference fed the same rows: the nets' tables as the kernels computed them
    arrs = vx.rr.tree_arrays(name)
    legal_tab = lr.legal_table(np.asarray(arrs["legal"]))
    legal = torch.tensor(legal_tab, device=DEV)
    logit, _ = vtrace._net_rows(tree, rn.net)
    vv = vtrace._net_rows(tree, rn.net_target)[1].cpu().numpy()
    mu = rnad_hip.policy_head(logit, mask=legal).cpu().numpy()
    hp = lr._hp(alpha=alpha, eta=rn.eta, lambda_=1.0, c=rn.c_bar, rho=rn.roh_bar, gamma=rn.vtrace_gamma, clip=rn.neurd_clip,
                threshold=rn.beta, w_v=rn.value_weight, w_n=rn.neurd_weight, eps=rn.epsilon_threshold, n_disc=rn.n_discrete)
    tables = dict(logit=logit.cpu().numpy(), logit_reg=vtrace._net_rows(tree, rn.net_reg)[0].cpu().numpy(),
                  logit_reg_=vtrace._net_rows(tree, rn.net_reg_)[0].cpu().numpy())
    _, _, lpol64 = vx.row_inputs(np.float64, tables, legal_tab, hp)
    pip = ev.pi_processed.cpu().numpy()  # (a net's rows have no decision margin: the kernel's own pi_processed)
    _, ref, g = _reference_for_rows(name, mu, pip, lpol64.astype(np.float32), vv, hp)
    shares = _shares_of(ev, ref, g, S)
    SHARES["rnad_expected_update"] = shares
    print(f"RNaD.expected_update: {shares} of the gates")
    assert max(shares.values()) <= 1.0
    again = rn.expected_update(alpha)
    assert torch.equal(again.target, ev.target) and torch.equal(again.q, ev.q)
    with pytest.raises(ValueError, match="alpha"):
        rn.expected_update(1.5)
    from learn.rnad import RNaD

    fresh = RNaD(tree=tree, device=DEV, directory_name="expected_fresh", batch_size=256, eta=0.2,
                 net_params={"type": "MLP", "max_actions": A, "width": 64})
    with pytest.raises(ValueError, match="not initialised"):
        fresh.expected_update()


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = vx.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    SHARES["kernels"] = {str(A): table[A] for A in sorted(table)}
    assert sorted(table) == list(range(1, 9)) and all(k["scratch"] == 0 for k in table.values())


# ---------------------------------------------------------------------------------------------------- the tool
def test_tool_reports_a_reference_written_run(tmp_path, capsys):
    import importlib.util
    import json
    import shutil

    from _util import GOLDEN

    root = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    spec = importlib.util.spec_from_file_location("expected_update_tool", os.path.join(root, "tools", "expected_update.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run_dir = tmp_path / "from_reference"
    os.makedirs(run_dir / "1")
    shutil.copy(os.path.join(GOLDEN, "ref_run_params"), run_dir / "params")
    shutil.copy(os.path.join(GOLDEN, "ref_run_ckpt_1_0"), run_dir / "1" / "0")
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, str(run_dir)])
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert lines == out and len(out) == 1
    rec = out[0]
    assert set(rec) == {"run", "m", "n", "alpha", "eta", "gamma", "rho", "c", "lambda", "length", "target_bias", "value_gap", "dv_norm",
                        "dlogit_norm", "linear_share", "root_target"}
    assert (rec["run"], rec["m"], rec["n"], rec["lambda"]) == ("from_reference", 1, 0, 1.0) and rec["length"] >= 1
    assert all(np.isfinite(x) and x >= 0 for x in rec["target_bias"] + rec["value_gap"] + [rec["dv_norm"], rec["dlogit_norm"]])
    swept = tool.main(["--tree", tar, str(run_dir), "--rho", "0.25", "1", "--lambda", "0.5"])
    capsys.readouterr()
    assert [(r["rho"], r["lambda"]) for r in swept] == [(0.25, 0.5), (1.0, 0.5)] and swept[0]["target_bias"] != swept[1]["target_bias"]
