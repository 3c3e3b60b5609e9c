"""rnad_cfr_iterate on the MI355X against the fp64 iteration of tests/_cfrref.py, within its derived bounds -- half of
_cfrref's one-ulp gates, K * 2^-24 * the absolute terms (cf.DEVICE_SHARE) -- at EVERY state:

  a. one iteration: every tree of _regref.ALL_TREES (A = 1 .. 8, C = 1 .. 4) with n = 1, 2, 3, 31 and 32 members that cycle through four
     variants, three sides values and 0 .. 7 earlier iterations.  policy, values and reach are pre-filled with NaN: afterwards every row
     is written and the rows of state 0 and of unreached states are exactly zero; untouched rows, illegal entries and a cleared side's
     rows of regret and strategy_sum carry their input bits;
  b. eight iterations in a row on the device: iteration t against the fp64 reference fed the tables the device held after t - 1;
  c. reproducibility: two runs give identical bits, and one captured torch.cuda.graph, replayed after discount and sides were rewritten,
     gives the bits of an eager call with the new values;
  d. the sibling sweeps: the product of the three reach factors against rnad_best_response's reach of sigma_t, values against
     rnad_cross_play's diagonal, the average policy of four plain iterations against util.metric.mixture of the four iterates;
  e. the regret bound on the device's own tables after 256 iterations;
  f. the refusals of the binding, of the C entry point and of learn.tabular.TabularCFR, none of which touches a table;
  g. RNaD.cfr_baseline, tools/tabular_cfr.py, and the sibling sweeps' bits before and after a CFR call.

The worst share of each gate per case goes to cfr_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/cfr_errors.json holds the figures of an MI355X."""
import gc
import types

import numpy as np
import pytest
import torch

import _brref as br
import _cfrref as cf
import _crossref as cr
import _mixref as mx
import _regref as rr
from rnad_hip import cfr_iterate as _the_symbol_this_file_is_about  # noqa: F401  (without it nothing below can run)
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
        cf.update_errors_file("mi355x", dict(SHARES))


def outputs(S, n, A2):
    return tuple(torch.full(shape, NAN, device=DEV) for shape in ((S, n, A2), (S, n), (S, 3, n)))


def device_inputs(name, n):
    """(regret, strategy_sum, discount, sides) of the first n members of a tree's case, fresh copies on the device."""
    R, S, disc, sides = cf.inputs(name)
    return (torch.tensor(np.ascontiguousarray(R[:, :n]), device=DEV), torch.tensor(np.ascontiguousarray(S[:, :n]), device=DEV),
            torch.tensor(np.ascontiguousarray(disc[:n]), device=DEV), torch.tensor(np.ascontiguousarray(sides[:n]), device=DEV))


def run(name, n, outs=(None, None, None)):
    import rnad_hip

    regret, strategy_sum, discount, sides = device_inputs(name, n)
    got = rnad_hip.cfr_iterate(product_tree(name).handle(), regret, strategy_sum, discount, sides, *outs)
    return got, (regret, strategy_sum, discount, sides)


def host(regret, strategy_sum, policy, values, reach):
    return types.SimpleNamespace(RG=regret.cpu().numpy(), SS=strategy_sum.cpu().numpy(), P=policy.cpu().numpy(), V=values.cpu().numpy(),
                                 reach=reach.cpu().numpy())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", cf.ALL_TREES)
def test_every_output_within_its_gate_at_every_state(name, n):
    c = cf.case(name)
    S, _, A2 = c.R.shape
    assert S < 10**5
    outs = outputs(S, n, A2)
    got, (regret, strategy_sum, _, _) = run(name, n, outs)
    assert all(a is b for a, b in zip(got, outs))
    g = host(regret, strategy_sum, *outs)
    for a in (g.P, g.V, g.reach):
        assert np.isfinite(a).all(), "a row was left unwritten"
        assert (a[~c.reached] == 0).all(), "state 0 and the states no path reaches are zero"
    assert (g.reach[1] == 1).all()
    assert (g.P[:, :, ~np.zeros(A2, bool)][~c.ref.mask[:, None, :].repeat(n, 1)] == 0).all(), "illegal actions get 0"
    # rows no gate covers -- unreached states, state 0, illegal actions, a cleared side -- carry their input bits
    for out, table, gate in ((g.RG, c.R, c.g.RG), (g.SS, c.S, c.g.SS)):
        kept = gate[:, :n] == 0
        assert kept[~c.reached].all() and kept[:, :, ~np.zeros(A2, bool)][~c.ref.mask[:, None, :].repeat(n, 1)].all()
        for k in range(n):
            for side in (0, 1):
                if not (int(c.sides[k]) >> side) & 1:
                    assert kept[:, k, side * (A2 // 2):(side + 1) * (A2 // 2)].all()
        assert np.array_equal(out.view(np.uint32)[kept], np.ascontiguousarray(table[:, :n]).view(np.uint32)[kept])
    shares = cf.shares(c.ref, c.g, g, n)
    SHARES[f"{name}/n{n}"] = dict(S=int(S), **shares)
    print(f"{name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the gates")
    assert max(shares.values()) <= cf.DEVICE_SHARE


@pytest.mark.parametrize("name", ("small", "ragged", "a5", "gen_a3c4", "gen_a8c1"))
def test_eight_iterations_in_a_row(name):
    """Iteration t is compared with the fp64 reference fed the tables the device held after t - 1, up-converted: the gates count this
    kernel's roundings only, and no divergence of trajectories enters."""
    import rnad_hip

    n = 32
    tree = rr.tree_arrays(name)
    handle = product_tree(name).handle()
    regret, strategy_sum, discount, sides = device_inputs(name, n)
    outs = outputs(*regret.shape)
    worst = {}
    for step in range(8):
        ts = [cf.member(k)[1] + 1 + step for k in range(n)]
        disc = cf.discounts([cf.member(k)[0] for k in range(n)], ts)
        turn = np.asarray([cf.turn(cf.member(k)[2], t) for k, t in enumerate(ts)], np.int32)
        before_R, before_S = regret.cpu().numpy(), strategy_sum.cpu().numpy()
        discount.copy_(torch.tensor(disc))
        sides.copy_(torch.tensor(turn))
        for t in outs:
            t.fill_(NAN)
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides, *outs)
        ref = cf.iterate(tree, before_R, before_S, disc, turn)
        gates = cf.gates(tree, ref, before_R, before_S, disc, turn)
        shares = cf.shares(ref, gates, host(regret, strategy_sum, *outs))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in shares.items()}
        assert max(shares.values()) <= cf.DEVICE_SHARE, (step, shares)
    SHARES[f"eight/{name}"] = worst
    print(f"{name}: eight iterations use up to " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of the gates")
    assert (regret.cpu().numpy() < 0).any() and (strategy_sum.cpu().numpy() > 0).any()


@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 31), ("native_a5", 32)])
def test_two_runs_and_a_replayed_graph_that_follows_its_tensors(name, n):
    import rnad_hip

    first, (r1, s1, _, _) = run(name, n)
    second, (r2, s2, _, _) = run(name, n)
    assert all(torch.equal(a, b) for a, b in zip(first + (r1, s1), second + (r2, s2)))
    handle = product_tree(name).handle()
    regret, strategy_sum, discount, sides = device_inputs(name, n)
    start_R, start_S = regret.clone(), strategy_sum.clone()
    outs = outputs(*regret.shape)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc_was_on = gc.isenabled()
    gc.disable()  # (a collection inside the capture could free device memory, which invalidates it)
    try:
        with torch.cuda.graph(graph):
            rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides, *outs)
    finally:
        if gc_was_on:
            gc.enable()
    # the captured values, then new ones written into the same tensors: the replay follows them
    for new in (False, True):
        regret.copy_(start_R)
        strategy_sum.copy_(start_S)
        if new:
            discount.copy_(torch.tensor(cf.discounts([cf.member(k)[0] for k in range(n)], [cf.member(k)[1] + 9 for k in range(n)])))
            sides.copy_(torch.tensor([(3, 1, 2)[k % 3] for k in range(n)], dtype=torch.int32))
        for t in outs:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        eager_R, eager_S = start_R.clone(), start_S.clone()
        eager = rnad_hip.cfr_iterate(handle, eager_R, eager_S, discount.clone(), sides.clone())
        assert all(torch.equal(a, b) for a, b in zip(outs + (regret, strategy_sum), eager + (eager_R, eager_S)))
        if new:
            assert not torch.equal(regret, r1) and not torch.equal(strategy_sum, s1), "the new discounts and sides changed the update"
        else:
            assert torch.equal(regret, r1) and torch.equal(strategy_sum, s1)


# ---------------------------------------------------------------------------------------------------- the sibling sweeps
@pytest.mark.parametrize("name,n", [("small", 3), ("ragged", 5), ("gen_a7c4", 4)])
def test_reach_and_values_against_best_response_and_cross_play(name, n):
    """Both siblings are handed the device's own sigma_t; their fp64 references on that table are exact for it, this kernel's reach and
    values are computed from the same table (its gates count sigma's rounding on top), so the two devices differ by at most the sum."""
    import rnad_hip

    c = cf.case(name)
    handle = product_tree(name).handle()
    (policy, values, reach), _ = run(name, n)
    J = policy.cpu().numpy()
    R = c.reached
    joint = reach.cpu().numpy().astype(np.float64).prod(axis=1)
    want = rnad_hip.best_response(handle, policy)[3].cpu().numpy()
    bref = br.reference(c.tree, J)
    g_br = br.gates(c.tree, bref, J)[3]
    rel = cf.DEVICE_SHARE * sum(c.g.reach[:, i, :n] / np.where(c.ref.reach[:, i, :n] > 0, c.ref.reach[:, i, :n], 1.0) for i in range(3))
    g_joint = rel * np.asarray(bref.R, np.float64) + 3 * 2 * cf.TINY
    share_reach = cf.share(joint[R], want[R], (g_br + g_joint)[R])
    diag = np.arange(n)
    cross = rnad_hip.cross_play(handle, policy).cpu().numpy()[:, diag, diag]
    V, B, h = cr.reference(c.tree, J)
    g_cross = cr.gate(c.tree, B, h)[:, diag, diag]
    share_values = cf.share(values.cpu().numpy()[R], cross[R], (g_cross + cf.DEVICE_SHARE * c.g.V[:, :n])[R])
    SHARES[f"siblings/{name}/n{n}"] = dict(reach=share_reach, values=share_values)
    print(f"{name} n={n}: joint reach {share_reach:.3f}, values {share_values:.3f} of the summed gates")
    assert share_reach <= 1.0 and share_values <= 1.0
    assert (joint[R] > 0).any() and (np.abs(cross[R]) > 0).any()


@pytest.mark.parametrize("name", ("small", "ragged"))
def test_average_policy_against_the_mixture_of_the_iterates(name):
    """Four plain iterations.  An entry of the strategy sum is a sum of four products own * sigma: with e = d (A + 2) + A + 6 roundings on
    a term (the reach's d (A + 2) + 1, sigma's A + 1, the product, three sums), all terms nonnegative, the normalised entry carries the
    numerator's e, the denominator's e + A - 1 and the division: (2 e + A + 1) * 2^-24 of itself, + 1 for second order.  The mixture's gate is
    _mixref's for n = 4."""
    from learn import tabular
    from util import metric

    tree = product_tree(name)
    arrs = rr.tree_arrays(name)
    A = tree.max_actions
    loop = tabular.TabularCFR(tree, "cfr")
    iterates = []
    for _ in range(4):
        loop.step()
        iterates.append(loop.policy[:, 0].clone())
    assert loop.sides.tolist() == [3] and loop.discount.tolist() == [[1.0, 1.0, 1.0]]
    avg = loop.average_policy[:, 0].cpu().numpy()
    got = metric.mixture(tree, iterates, [1, 1, 1, 1]).policy.cpu().numpy()
    M, _, depth = mx.reference(arrs, np.stack([p.cpu().numpy() for p in iterates], axis=1), np.full((2, 4), 0.25, np.float32))
    d = np.maximum(depth, 0).astype(np.float64)
    g_avg = ((2 * (d * (A + 2) + A + 6) + A + 1) * cf.U)[:, None] * M
    g_mix = mx.gates(M, np.zeros((M.shape[0], 2, 4)), depth, 4)[0]
    R = depth >= 0
    share = cf.share(avg[R], got[R], (g_avg + g_mix)[R])
    SHARES[f"average/{name}"] = dict(average=share)
    print(f"{name}: average policy against metric.mixture {share:.3f} of the summed gates")
    assert share <= 1.0 and R.sum() > 1


@pytest.mark.parametrize("name", ("small", "ragged"))
def test_regret_bound_on_the_device(name):
    """NashConv(average) <= (sum_s max_a R+_row + sum_s max_b R+_col) / T on the device's own tables.  The device's regrets differ from the
    exact regrets of the strategies it played by at most one regret gate per iteration and entry; the gates of an iteration from the
    final tables (the largest regrets, so the largest gates) stand for all T.  In fp64 the two sides are 0.154 <= 0.328 and
    0.071 <= 0.133 at T = 256: the slack does not decide the test."""
    from learn import tabular

    T = 256
    tree = product_tree(name)
    arrs = rr.tree_arrays(name)
    mask = cf.legal_mask(arrs)
    loop = tabular.TabularCFR(tree, "cfr")
    loop.run(T, every=T)
    assert loop.t == T and loop.recorded == [T] and loop.alternating == [False]
    R, S = loop.regret.cpu().numpy(), loop.strategy_sum.cpu().numpy()
    disc, sides = cf.discounts(["cfr"], [T + 1]), [3]
    slack = T * cf.DEVICE_SHARE * cf.gates(arrs, cf.iterate(arrs, R, S, disc, sides), R, S, disc, sides).regret_gate_sum[0].sum()
    nc = loop.average_nashconv_history[0][-1]
    bound = cf.positive_regret(mask, R)[0].sum()
    print(f"{name} T={T}: NashConv(average) {nc:.6g} <= ({bound:.6g} + {slack:.3g}) / {T} = {(bound + slack) / T:.6g}")
    SHARES[f"bound/{name}"] = dict(nashconv=nc, bound=(bound + slack) / T, slack=slack / T)
    assert nc <= (bound + slack) / T
    # T iterations of a few hundred ulps each: per cent of the bound, an order of magnitude under the factor of two the bound leaves
    assert slack < 0.1 * bound
    assert abs(nc - rr.nashconv64(name, cf.average_policy(mask, S)[:, 0])) <= 1e-4


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_no_table():
    import ctypes as C

    import rnad_hip

    name, n = "small", 2
    tree = product_tree(name)
    handle = tree.handle()
    S, A = handle.S, handle.A
    regret, strategy_sum, discount, sides = device_inputs(name, n)
    keep = (regret.clone(), strategy_sum.clone())
    outs = outputs(S, n, 2 * A)
    err = rnad_hip.RnadHipError
    with pytest.raises(err, match="outside"):
        rnad_hip.cfr_iterate(handle, regret[:, :0].contiguous(), strategy_sum[:, :0].contiguous(), discount[:0], sides[:0])
    with pytest.raises(err, match="outside"):
        rnad_hip.cfr_iterate(handle, torch.zeros((S, 33, 2 * A), device=DEV), torch.zeros((S, 33, 2 * A), device=DEV),
                             torch.ones((33, 3), device=DEV), torch.ones((33,), dtype=torch.int32, device=DEV))
    with pytest.raises(err, match="GPU"):
        rnad_hip.cfr_iterate(handle, regret.cpu(), strategy_sum, discount, sides, *outs)
    with pytest.raises(err, match="GPU"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount.cpu(), sides, *outs)
    with pytest.raises(err, match="do not fit|does not fit"):
        rnad_hip.cfr_iterate(handle, torch.zeros((S + 1, n, 2 * A), device=DEV), strategy_sum, discount, sides, *outs)
    with pytest.raises(err, match="strategy_sum must be"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum[:, :1].contiguous(), discount, sides, *outs)
    with pytest.raises(err, match="discount must be"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount[:, :2].contiguous(), sides, *outs)
    with pytest.raises(err, match="dtype"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides.float(), *outs)
    with pytest.raises(err, match="must be a tensor"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, [1.0, 1.0, 1.0], sides, *outs)
    with pytest.raises(err, match="reach must be"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides, outs[0], outs[1], torch.zeros((S, n, 3), device=DEV))
    with pytest.raises(err, match="TreeHandle"):
        rnad_hip.cfr_iterate(tree, regret, strategy_sum, discount, sides, *outs)
    with pytest.raises(err, match="strategy_sum aliases regret"):
        rnad_hip.cfr_iterate(handle, regret, regret, discount, sides, *outs)
    with pytest.raises(err, match="policy aliases strategy_sum"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides, strategy_sum)
    with pytest.raises(err, match="values aliases regret"):
        rnad_hip.cfr_iterate(handle, regret, strategy_sum, discount, sides, outs[0], regret.view(-1)[: S * n].view(S, n))
    # the C entry point itself: n out of range, overlaps, null pointers -- nothing launched
    lib = rnad_hip.lib()
    d, i, r, s = discount.data_ptr(), sides.data_ptr(), regret.data_ptr(), strategy_sum.data_ptr()
    o = [t.data_ptr() for t in outs]
    assert lib.rnad_cfr_iterate(handle.ptr, 0, d, i, r, s, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(handle.ptr, 33, d, i, r, s, *o, None) != 0 and b"outside" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(handle.ptr, n, d, i, r, r, *o, None) != 0 and b"overlap" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(handle.ptr, n, d, i, r, s, o[0], o[1], o[0], None) != 0 and b"overlap" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(handle.ptr, n, d, i, r, s, r + 4, o[1], o[2], None) != 0 and b"overlap" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(handle.ptr, n, d, i, r, s, o[0], d, o[2], None) != 0 and b"overlaps discount or sides" in lib.rnad_last_error()
    for k in range(7):
        args = [d, i, r, s] + o
        args[k] = None
        assert lib.rnad_cfr_iterate(handle.ptr, n, *args, None) != 0 and b"null" in lib.rnad_last_error()
    assert lib.rnad_cfr_iterate(None, n, d, i, r, s, *o, None) != 0 and b"null" in lib.rnad_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"
    assert torch.equal(regret, keep[0]) and torch.equal(strategy_sum, keep[1])
    assert isinstance(C.c_void_p(d).value, int)


def test_tabular_cfr_refusals(monkeypatch):
    import rnad_hip
    from _gpu import tree_from_arrays
    from learn import tabular

    tree = product_tree("small")
    with pytest.raises(ValueError, match="unknown variant"):
        tabular.TabularCFR(tree, "cfr++")
    with pytest.raises(ValueError, match="unknown variant"):
        tabular.TabularCFR(tree, ["cfr", ("dcfr", 1.5, 0.0)])
    with pytest.raises(ValueError, match="33 variants"):
        tabular.TabularCFR(tree, ["cfr"] * 33)
    with pytest.raises(ValueError, match="0 variants"):
        tabular.TabularCFR(tree, [])
    with pytest.raises(ValueError, match="values of alternating"):
        tabular.TabularCFR(tree, ["cfr", "cfr+"], alternating=[True])
    fresh = tabular.TabularCFR(tree, ["cfr", "cfr+", "linear", ("dcfr", 1.5, 0, 2)])
    assert fresh.alternating == [False, True, False, False] and fresh.n == 4
    with pytest.raises(ValueError, match="no iteration has run"):
        fresh.policy
    assert tabular.TabularCFR(tree, ("dcfr", 1.5, 0.0, 2.0)).variants == [("dcfr", 1.5, 0.0, 2.0)]
    assert tabular.TabularCFR(tree, ["cfr", "cfr"], alternating=True).alternating == [True, True]
    # a state with two parents: refused before any sweep
    arrs = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in cr.tree_arrays("small").items()}
    index, chance = arrs["index"], arrs["chance"]
    live = (index != 0) & (chance > 0)
    levels = cr.level_order(index, chance)
    s, t, r, c = 1, *[int(v[0]) for v in np.nonzero(live[1])]
    index[s, t, r, c] = levels[2][0]
    knot = tree_from_arrays(arrs, depth_bound=arrs["meta"]["kw"]["depth_bound"])

    def no_sweep(*args, **kwargs):
        raise AssertionError("a sweep ran")

    monkeypatch.setattr(rnad_hip, "cfr_iterate", no_sweep)
    with pytest.raises(ValueError, match="not a tree"):
        tabular.TabularCFR(knot, "cfr")


# ---------------------------------------------------------------------------------------------------- the public interface
def test_tabular_cfr_runs_every_variant_and_hands_out_ordinary_tables():
    from learn import tabular
    from util import metric

    name = "small"
    tree = product_tree(name)
    arrs = rr.tree_arrays(name)
    mask = cf.legal_mask(arrs)
    S, A = mask.shape[0], mask.shape[1] // 2
    variants = ["cfr", "cfr+", "linear", ("dcfr", 1.5, 0.0, 2.0)]
    loop = tabular.TabularCFR(tree, variants, alternating=[False, True, False, True])
    curves = loop.run(60, every=25)
    assert loop.recorded == [25, 50, 60] and curves is loop.average_nashconv_history and len(curves) == 4 and all(len(c) == 3 for c in curves)
    assert loop.sides.tolist() == [3, 2, 3, 2], "iteration 60 is even: the alternating members updated the column side"
    want = cf.discounts(variants, [60] * 4)
    assert np.array_equal(loop.discount.cpu().numpy(), want), "fp64 on the host, rounded to fp32"
    avg = loop.average_policy
    assert avg.shape == (S, 4, 2 * A) and loop.policy.shape == (S, 4, 2 * A) and loop.values.shape == (S, 4) and loop.reach.shape == (S, 3, 4)
    assert np.array_equal(avg.cpu().numpy() > 0, (avg.cpu().numpy() > 0) & mask[:, None, :])
    sums = avg.cpu().numpy().reshape(S, 4, 2, A).sum(axis=3)
    assert np.abs(sums[1:] - 1).max() <= 4 * A * cf.U, "every side of every state but 0 is a distribution (uniform where the sum is 0)"
    for k in range(4):
        fp64 = rr.nashconv64(name, avg[:, k].cpu().numpy())
        assert abs(curves[k][-1] - fp64) <= 1e-4 and abs(loop.nashconv_history[k][-1] - rr.nashconv64(name, loop.policy[:, k].cpu().numpy())) <= 1e-4
        assert curves[k][-1] < 0.5 * rr.nashconv64(name, cf.average_policy(mask, np.zeros((S, 1, 2 * A)))[:, 0]), "far below the uniform policy"
    # the first iteration against fp64 CFR+: the row side's turn, from the uniform strategy.  Only the first: regret matching has kinks
    # (a state whose regrets are all exactly 0 in fp64 and +-1e-9 on the device plays uniform in one and a pure action in the other), so
    # trajectories part for good reasons; test_eight_iterations_in_a_row compares every step from the device's own tables instead
    one = tabular.TabularCFR(tree, "cfr+")
    one.run(1)
    R64, S64, _ = cf.run(name, "cfr+", 1, alternating=True)
    assert np.abs(one.regret.cpu().numpy() - R64).max() <= 1e-5 and np.abs(one.strategy_sum.cpu().numpy() - S64).max() <= 1e-5
    assert (one.regret[:, 0, A:] == 0).all() and (one.regret[:, 0, :A] != 0).any(), "row first"
    # ordinary tables for the sibling entry points
    tables = [avg[:, k].contiguous() for k in range(4)]
    payoff = metric.cross_play(tree, tables).payoff
    assert payoff.shape == (4, 4) and torch.isfinite(payoff).all()
    assert metric.best_response(tree, tables).policy.shape == (S, 4, 2 * A)
    assert metric.mixture(tree, tables, [1, 2, 3, 4]).policy.shape == (S, 2 * A)
    ev = tabular.evaluate_regularized(tree, tables, 0.2)
    assert torch.isfinite(ev.values).all() and ev.residual.shape == (S, 4)
    magnet = tabular.TabularRNaD(tree, 0.2, reg=tables[1])
    magnet.update()
    assert np.isfinite(magnet.nashconv_history[0])


def test_rnad_cfr_baseline():
    tree = product_tree("small")
    rn = _trainer(tree, "cfr_baseline", 7)
    iterations, curve = rn.cfr_baseline(40, every=10)
    assert iterations == [10, 20, 30, 40] and len(curve) == 4 and all(np.isfinite(curve)) and curve[-1] < curve[0]
    other_iterations, other = rn.cfr_baseline(5, variant="cfr")
    assert other_iterations == [1, 2, 3, 4, 5] and len(other) == 5
    exact = rn.tabular_baseline(2)
    assert len(exact) == 2 and np.isfinite(exact).all(), "its twin still answers"


def test_tool_on_the_reference_written_tree(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import shutil

    from _util import GOLDEN

    root = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    spec = importlib.util.spec_from_file_location("tabular_cfr_tool", os.path.join(root, "tools", "tabular_cfr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run_dir = tmp_path / "from_reference"
    os.makedirs(run_dir / "1")
    shutil.copy(os.path.join(GOLDEN, "ref_run_params"), run_dir / "params")
    shutil.copy(os.path.join(GOLDEN, "ref_run_ckpt_1_0"), run_dir / "1" / "0")
    tar = os.path.join(GOLDEN, "ref_tree_c1.tar")
    out = tool.main(["--tree", tar, "--variants", "cfr", "cfr+", "linear", "dcfr:1.5:0:2", "--iterations", "40", "--every", "15",
                     "--against", str(run_dir)])
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert lines == out and [rec["variant"] for rec in out] == ["cfr", "cfr+", "linear", "dcfr:1.5:0:2"]
    for rec in out:
        assert set(rec) == {"variant", "alternating", "iterations", "average_nashconv", "nashconv", "names", "payoff"}
        assert rec["iterations"] == [15, 30, 40] and len(rec["average_nashconv"]) == len(rec["nashconv"]) == 3
        assert all(np.isfinite(v) and v >= -1e-6 for v in rec["average_nashconv"] + rec["nashconv"])
        assert rec["alternating"] == (rec["variant"] == "cfr+") and len(rec["names"]) == 2 and np.asarray(rec["payoff"]).shape == (2, 2)
        assert rec["average_nashconv"][-1] < rec["average_nashconv"][0]
    with pytest.raises(SystemExit, match="unknown variant"):
        tool.main(["--tree", tar, "--variants", "cfr2"])


# ---------------------------------------------------------------------------------------------------- isolation
def test_the_sibling_sweeps_keep_their_bits_around_a_cfr_call():
    import _regevalref as rv
    import rnad_hip

    name, n = "ragged", 5
    handle = product_tree(name).handle()
    J, L, etas = rv.inputs(name)
    policies = torch.tensor(np.ascontiguousarray(J[:, :n]), device=DEV)
    log_reg = torch.tensor(np.ascontiguousarray(L[:, :n]), device=DEV)
    weights = torch.tensor(mx.weights("dirichlet", n), device=DEV)

    def siblings():
        return (rnad_hip.reg_evaluate(handle, etas[:n].tolist(), policies, log_reg) + rnad_hip.best_response(handle, policies)
                + rnad_hip.mixture(handle, policies, weights))

    before = siblings()
    run(name, 32)
    after = siblings()
    assert len(before) == 10 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))
