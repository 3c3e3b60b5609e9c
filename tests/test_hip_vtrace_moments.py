"""rnad_vtrace_moments on the MI355X against the fp64 sweep of tests/_vtmomref.py (which tests/test_vtrace_moments.py ties to the
enumeration of every episode), within its derived gates at EVERY state:

  a. target_var, target_given_row_var and q_var: every tree of _regref.ALL_TREES (A = 1 .. 8, C = 1 .. 4) with n = 1, 2, 3, 31 and 32
     members that cycle through the four hyperparameter sets of _learnref.HP and three behaviours, as `_vtexpref.member` has them.  The
     reference takes the first moments the DEVICE wrote (rnad_vtrace_expect's outputs and export record, up-converted) as input data, so
     the gate counts this kernel's roundings only.  All outputs and the workspace are pre-filled with NaN: afterwards every output row is
     written, nothing is negative and the rows of state 0 and of unreached states are exactly zero;
  b. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed, gives the eager bits;
  c. rnad_vtrace_expect's four outputs and its export record carry the same bits before and after;
  d. the refusals of the binding and the C entry point, none of which touches an output;
  e. learn.vtrace.update_noise on row tables and RNaD.update_noise on a trainer's nets against the all-fp64 pipeline fed the same rows,
     within the end-to-end gate (the kernel's plus the first-order term of the fp32 first moments);
  f. no instantiation uses scratch (the built library's metadata).

The worst share of each gate per case goes to vtrace_moments_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/vtrace_moments_errors.json holds the figures of an MI355X."""
import functools
import gc
import os
import types

import numpy as np
import pytest
import torch

import _learnref as lr
import _vtexpref as vx
import _vtmomref as vm
from rnad_hip import vtrace_moments as _the_symbol_this_file_is_about  # noqa: F401  (without it nothing below can run)
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
        vm.update_errors_file("mi355x", dict(SHARES))


def outputs(S, n, A):
    shapes = ((S, n, 2), (S, n, A), (S, n, 2 * A), (vm.workspace(S, A, n),))
    return tuple(torch.full(shape, NAN, device=DEV) for shape in shapes)


def expect(name, n):
    """rnad_vtrace_expect on the first n members: (inputs as tensors, hyper rows, (target, target_given_row, q, reach), workspace)."""
    import rnad_hip

    MU, PIP, LPOL, VV, hyper = vx.inputs(name)
    tens = tuple(torch.tensor(np.ascontiguousarray(x[:, :n]), device=DEV) for x in (MU, PIP, LPOL, VV))
    handle = product_tree(name).handle()
    ws = torch.full((vx.workspace(handle.S, handle.A, n),), NAN, device=DEV)
    outs = rnad_hip.vtrace_expect(handle, hyper[:n].tolist(), *tens, workspace=ws)
    return tens, hyper[:n].tolist(), outs, ws


def run(name, n, outs=(None,) * 4):
    import rnad_hip

    tens, hyper, first, ws = expect(name, n)
    return rnad_hip.vtrace_moments(product_tree(name).handle(), hyper, *tens, ws, *first[:3], *outs), (tens, hyper, first, ws)


def _first_of_device(first, ws, S, A, n):
    return types.SimpleNamespace(target=first[0].cpu().numpy(), W1=first[1].cpu().numpy(), q=first[2].cpu().numpy(),
                                 rec=ws.cpu().numpy().reshape(S, 3 * A + 5, n))


@functools.lru_cache(maxsize=None)
def device_case(name):
    """The reference of all 32 members on the first moments the device wrote, computed once: (first, ref, gates)."""
    c = vx.case(name)
    S, _, A2 = c.MU.shape
    _, _, first, ws = expect(name, vx.N_MAX)
    dev_first = _first_of_device(first, ws, S, A2 // 2, vx.N_MAX)
    ref = vm.reference(np.float64, c.tree, c.MU, c.PIP, c.LPOL, c.VV, c.hyper, dev_first)
    return dev_first, ref, vm.gates(c.tree, ref)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", vx.ALL_TREES)
def test_every_output_within_its_gate_at_every_state(name, n):
    dev_first, ref, g = device_case(name)
    c = vx.case(name)
    S, _, A2 = c.MU.shape
    A = A2 // 2
    assert S < 10**5
    outs = outputs(S, n, A)
    got, (_, _, first, ws) = run(name, n, outs)
    assert all(a is b for a, b in zip(got, outs))
    mine = _first_of_device(first, ws, S, A, n)
    assert np.array_equal(mine.target, dev_first.target[:, :n]) and np.array_equal(mine.W1, dev_first.W1[:, :n]) and \
        np.array_equal(mine.q, dev_first.q[:, :n]) and np.array_equal(mine.rec, dev_first.rec[:, :, :n]), \
        "the first moments of n members are the first n of 32: the reference is shared"
    arrays = dict(zip(vm.OUTPUTS, (t.cpu().numpy() for t in outs[:3])))
    for a in arrays.values():
        assert np.isfinite(a).all(), "a row was left unwritten"
        assert (a >= 0).all(), "every summand is a square"
        assert (a[~ref.reached] == 0).all(), "state 0 and the states no path reaches are zero"
    assert np.array_equal(ref.reached, c.reached)
    assert torch.isfinite(outs[3]).all(), "every export record is written"
    shares = vm.shares(ref, g, arrays, n)
    SHARES[f"{name}/n{n}"] = dict(S=int(S), **shares)
    print(f"{name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the gates")
    assert max(shares.values()) <= 1.0


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_give_the_same_bits(name, n):
    import rnad_hip

    one, (tens, hyper, first, ws) = run(name, n)
    two, _ = run(name, n)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    handle = product_tree(name).handle()
    outs = outputs(handle.S, n, handle.A)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.vtrace_moments(handle, hyper, *tens, ws, *first[:3], *outs)
    finally:
        if gc_was_on:
            gc.enable()
    for t in outs:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs[:3], one))


@pytest.mark.parametrize("name,n", [("ragged", 31), ("gen_a8c1", 2)])
def test_the_first_moments_are_left_as_they_were(name, n):
    import rnad_hip

    tens, hyper, first, ws = expect(name, n)
    before = [t.clone() for t in first + (ws,) + tens]
    rnad_hip.vtrace_moments(product_tree(name).handle(), hyper, *tens, ws, *first[:3])
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, first + (ws,) + tens))
    again = expect(name, n)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before[:4], again[2]))


def test_refusals_touch_no_output():
    import ctypes as C

    import rnad_hip

    tree = product_tree("small")
    handle = tree.handle()
    S, A = handle.S, handle.A
    (mu, pip, lpol, vv), hy, first, ws = expect("small", 2)
    f = (ws,) + first[:3]
    outs = outputs(S, 2, A)
    err = rnad_hip.RnadHipError
    for bad, what in (((0.2, 0.0, 1.0, 1.0, 1.0), "gamma"), ((0.2, float("nan"), 1.0, 1.0, 1.0), "gamma"), ((0.2, 1.0, 1.0, -0.5, 1.0), "clips"),
                      ((0.2, 1.0, 1.0, 1.0, -1e-3), "clips"), ((float("inf"), 1.0, 1.0, 1.0, 1.0), "finite")):
        with pytest.raises(err, match=what):
            rnad_hip.vtrace_moments(handle, [hy[0], bad], mu, pip, lpol, vv, *f, *outs)
    with pytest.raises(err, match="2 rows"):
        rnad_hip.vtrace_moments(handle, [hy[0]] * 3, mu, pip, lpol, vv, *f, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, ws.cpu(), *first[:3], *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, outs[0].cpu())
    with pytest.raises(err, match="does not fit"):
        rnad_hip.vtrace_moments(handle, hy, torch.zeros((S + 1, 2, 2 * A), device=DEV), pip, lpol, vv, *f, *outs)
    with pytest.raises(err, match="expect_workspace must be"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, ws[:-1], *first[:3], *outs)
    with pytest.raises(err, match="target_given_row must be"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, ws, first[0], first[0], first[2], *outs)
    with pytest.raises(err, match="q_var must be"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, outs[0], outs[1], torch.zeros((S, 2, 2 * A + 1), device=DEV))
    with pytest.raises(err, match="workspace must be"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, *outs[:3], torch.zeros((7,), device=DEV))
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.vtrace_moments(tree, hy, mu, pip, lpol, vv, *f, *outs)
    with pytest.raises(err, match="q_var aliases q"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, outs[0], outs[1], first[2])
    with pytest.raises(err, match="workspace aliases expect_workspace"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, *outs[:3], ws[: vm.workspace(S, A, 2)])
    with pytest.raises(err, match="workspace aliases q_var"):
        rnad_hip.vtrace_moments(handle, hy, mu, pip, lpol, vv, *f, *outs[:3], outs[2].view(-1)[: vm.workspace(S, A, 2)])
    # the C entry point itself: nothing launched
    lib = rnad_hip.lib()
    flat = lambda rows: C.cast((C.c_float * (5 * len(rows)))(*[x for r in rows for x in r]), C.c_void_p)  # noqa: E731
    keep = [(C.c_float * 10)(*[x for r in hy for x in r])]
    hp = C.cast(keep[0], C.c_void_p)
    i = [t.data_ptr() for t in (mu, pip, lpol, vv) + f]
    o = [t.data_ptr() for t in outs]
    call = lib.rnad_vtrace_moments
    assert call(handle.ptr, 0, hp, *i, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert call(handle.ptr, 33, hp, *i, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert call(handle.ptr, 2, flat([hy[0], (0.2, 0.0, 1.0, 1.0, 1.0)]), *i, *o, None) != 0 and b"gamma[1]" in lib.rnad_last_error()
    assert call(handle.ptr, 2, flat([hy[0], (0.2, 1.0, 1.0, -1.0, 1.0)]), *i, *o, None) != 0 and b"clips" in lib.rnad_last_error()
    assert call(handle.ptr, 2, hp, *i, o[0], o[1], i[1], o[3], None) != 0 and b"overlaps an input" in lib.rnad_last_error()
    assert call(handle.ptr, 2, hp, *i, o[0], o[1], o[2], o[2], None) != 0 and b"two outputs" in lib.rnad_last_error()
    assert call(handle.ptr, 2, hp, *i, o[0], o[1], o[2], i[4], None) != 0 and b"expect_workspace overlaps" in lib.rnad_last_error()
    assert call(handle.ptr, 2, hp, *i, o[0], o[1], o[2], i[4] + 4 * (ws.numel() - 1), None) != 0 and b"expect_workspace overlaps" in lib.rnad_last_error()
    for k in range(13):
        args = [hp] + i + o
        args[k] = None
        assert call(handle.ptr, 2, *args, None) != 0 and b"null" in lib.rnad_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"


# ---------------------------------------------------------------------------------------------------- the public interface
def _end_to_end(name, mu_rows, pip_rows, lpol_rows, vv_rows, hp):
    """(ref, gates) of the all-fp64 pipeline for the single member whose row tables [2S, (A)] are given: the fp64 first moments, the
    fp64 sweep on them, and the end-to-end gates (`_vtmomref`: the kernel's plus the first-order term of the first moments' own gates)."""
    tree = vx.rr.tree_arrays(name)
    S = np.asarray(tree["index"]).shape[0]
    a = tuple(vx.to_sides(x, S)[:, None] for x in (mu_rows, pip_rows, lpol_rows, vv_rows))
    exp = vx.reference(np.float64, tree, *a, [vx.hyper_of(hp)])
    ref = vm.reference(np.float64, tree, *a, [vx.hyper_of(hp)], vm.first_of(np.float64, *a, exp), first_gates=vx.gates(tree, exp))
    return exp, ref, vm.gates(tree, ref, first_order=True)


def _shares_of(noise, ref, g, S):
    tv, qv = noise.target_var.cpu().numpy(), noise.q_var.cpu().numpy()
    got = dict(target_var=np.stack([tv[:S], tv[S:]], 1)[:, None], target_given_row_var=noise.target_given_row_var.cpu().numpy()[:, None],
               q_var=np.concatenate([qv[:S], qv[S:]], 1)[:, None])
    return vm.shares(ref, g, got)


def _check_host_tables(noise, hp, v_rows, S):
    ev = noise.expected
    want = vm.noise_tables(hp, v_rows, ev.target.cpu().numpy().astype(np.float64), noise.target_var.cpu().numpy().astype(np.float64),
                           ev.reach.cpu().numpy().astype(np.float64))
    assert noise.dv_var_tab.shape == (2 * S,) and noise.dv_var_tab.dtype == torch.float64
    assert np.allclose(noise.dv_var_tab.cpu().numpy(), want["dv_var_tab"], rtol=1e-9, atol=0)
    for got, key in ((noise.target_noise, "target_noise"), (noise.episodes_for_unit_snr, "episodes_for_unit_snr")):
        assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (2,)
        assert np.allclose(got.numpy(), want[key], rtol=1e-9)
    assert (noise.dv_var_tab >= 0).all() and (noise.target_noise > 0).all() and (noise.episodes_for_unit_snr > 0).all()


@pytest.mark.parametrize("hp_name", ("H0", "H1"))
def test_update_noise_on_row_tables(hp_name):
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
    args = (tree, dev(mu), dev(tables["logit"]), dev(tables["v"]), dev(tables["v_target"]), dev(tables["logit_reg"]), dev(tables["logit_reg_"]),
            params)
    noise = vtrace.update_noise(*args)
    ev = vtrace.expected_update(*args)
    assert all(torch.equal(a, b) for a, b in zip((noise.expected.target, noise.expected.q, noise.expected.reach, noise.expected.dv_tab),
                                                 (ev.target, ev.q, ev.reach, ev.dv_tab))), "expected is the ExpectedUpdate of the same call"
    assert noise.target_var.shape == (2 * S,) and noise.q_var.shape == (2 * S, A) and noise.target_given_row_var.shape == (S, A)
    _, ref, g = _end_to_end(name, mu, pip64.astype(np.float32), lpol64.astype(np.float32), tables["v_target"], hp)
    shares = _shares_of(noise, ref, g, S)
    SHARES[f"update_noise/{hp_name}"] = shares
    print(f"update_noise {hp_name}: {shares} of the end-to-end gates")
    assert max(shares.values()) <= 1.0
    _check_host_tables(noise, hp, tables["v"], S)
    with pytest.raises(ValueError, match="logit must be"):
        vtrace.update_noise(tree, dev(mu), dev(tables["logit"])[:-1], *args[3:])


def test_rnad_update_noise():
    import rnad_hip
    from learn import vtrace

    name = "small"
    tree = product_tree(name)
    rn = _trainer(tree, "noise", 7)
    with torch.no_grad():  # four different nets, as in the middle of a run
        for k, module in enumerate((rn.net_target, rn.net_reg, rn.net_reg_)):
            for p in module.parameters():
                p.add_(0.05 * (k + 1) * torch.randn_like(p))
    S, A = tree.value_tensor.shape[0], tree.max_actions
    alpha = 0.3
    noise = rn.update_noise(alpha)
    ev = rn.expected_update(alpha)
    assert torch.equal(noise.expected.target, ev.target) and torch.equal(noise.expected.q, ev.q)
    for t in (noise.target_var, noise.q_var, noise.target_given_row_var, noise.dv_var_tab):
        assert torch.isfinite(t).all() and (t >= 0).all()
    # the reference fed the same rows: the nets' tables as the kernels computed them
    arrs = vx.rr.tree_arrays(name)
    legal_tab = lr.legal_table(np.asarray(arrs["legal"]))
    legal = torch.tensor(legal_tab, device=DEV)
    logit, v_rows = vtrace._net_rows(tree, rn.net)
    vv = vtrace._net_rows(tree, rn.net_target)[1].cpu().numpy()
    mu = rnad_hip.policy_head(logit, mask=legal).cpu().numpy()
    hp = lr._hp(alpha=alpha, eta=rn.eta, lambda_=1.0, c=rn.c_bar, rho=rn.roh_bar, gamma=rn.vtrace_gamma, clip=rn.neurd_clip,
                threshold=rn.beta, w_v=rn.value_weight, w_n=rn.neurd_weight, eps=rn.epsilon_threshold, n_disc=rn.n_discrete)
    tables = dict(logit=logit.cpu().numpy(), logit_reg=vtrace._net_rows(tree, rn.net_reg)[0].cpu().numpy(),
                  logit_reg_=vtrace._net_rows(tree, rn.net_reg_)[0].cpu().numpy())
    _, _, lpol64 = vx.row_inputs(np.float64, tables, legal_tab, hp)
    pip = ev.pi_processed.cpu().numpy()  # (a net's rows have no decision margin: the kernel's own pi_processed)
    _, ref, g = _end_to_end(name, mu, pip, lpol64.astype(np.float32), vv, hp)
    shares = _shares_of(noise, ref, g, S)
    SHARES["rnad_update_noise"] = shares
    print(f"RNaD.update_noise: {shares} of the end-to-end gates")
    assert max(shares.values()) <= 1.0
    _check_host_tables(noise, hp, v_rows.cpu().numpy(), S)
    again = rn.update_noise(alpha)
    assert torch.equal(again.target_var, noise.target_var) and torch.equal(again.q_var, noise.q_var)
    with pytest.raises(ValueError, match="alpha"):
        rn.update_noise(1.5)


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = vm.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    SHARES["kernels"] = {str(A): table[A] for A in sorted(table)}
    assert sorted(table) == list(range(1, 9)) and all(k["scratch"] == 0 for k in table.values())


# ---------------------------------------------------------------------------------------------------- the tool
def test_tool_adds_the_noise_of_a_reference_written_run(tmp_path, capsys):
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
    plain = tool.main(["--tree", tar, str(run_dir)])
    out = tool.main(["--tree", tar, str(run_dir), "--noise"])
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert lines == plain + out and len(out) == 1
    rec = out[0]
    assert set(rec) - set(plain[0]) == {"target_noise", "dv_noise", "episodes_for_unit_snr"}
    assert {k: rec[k] for k in plain[0]} == plain[0], "the expectation's figures are the same call's"
    for key in ("target_noise", "dv_noise", "episodes_for_unit_snr"):
        assert len(rec[key]) == 2 and all(np.isfinite(x) and x > 0 for x in rec[key])
