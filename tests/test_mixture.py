"""Mixtures without a GPU: the reference and gates of tests/_mixref.py are pinned by what a mixture must do, not by a measurement --

  - the Kuhn identity: played through the fp64 cross-play recursion of tests/_crossref.py, the mixture table earns exactly the weighted
    sum of what its members earn, on either side and on both;
  - composition: a mixture of mixtures is the mixture of the members;
  - one-hot weights give the member's own table wherever it comes to;
  - an fp32 restatement stays within half of the gates, and three natural mistakes exceed twice the gate;
  - the D == 0 rule is exercised by the case list;

and util.metric.meta_nash (host code) and the host half of the C ABI are checked.
"""
import numpy as np
import pytest

import _crossref as cr
import _mixref as mr
from _util import TREES

CPU_TREES = TREES + ("native_a5",)
N = 6  # solution, uniform, (fixture,) and seeded softmax tables
MIXED = tuple(k for k in mr.WEIGHTS if k != "onehot")


def _with_mixture(J, M):
    return np.ascontiguousarray(np.concatenate([J, M[:, None].astype(J.dtype)], axis=1))


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("name", CPU_TREES)
def test_kuhn_identity(name, kind):
    tree, J, w, M, R, depth, gM, gR = mr.case(name, N, kind)
    V, B, h = cr.reference(tree, _with_mixture(J.astype(np.float64), M))
    x, y = mr.exact_weights(w)
    P, tol = V[1, :N, :N], 1e-12 * B[1]
    assert (np.abs(V[1, N, :N] - x @ P) <= tol[N, :N]).all(), "the row side of the mixture against every member"
    assert (np.abs(V[1, :N, N] - P @ y) <= tol[:N, N]).all(), "every member against the column side of the mixture"
    assert abs(V[1, N, N] - x @ P @ y) <= tol[N, N]


@pytest.mark.parametrize("name", CPU_TREES)
def test_a_mixture_of_mixtures_is_the_mixture_of_the_members(name):
    tree = cr.tree_arrays(name)
    J = cr.players(tree, 4, 0, cr.fixture_policy(name)).astype(np.float64)
    a_b_c = J[:, [0, 1, 3]]
    third = np.full((2, 3), 1.0 / 3)
    M3, R3, depth = mr.reference(tree, a_b_c, third)
    M2, _, _ = mr.reference(tree, a_b_c[:, :2], np.full((2, 2), 0.5))
    Mc, _, _ = mr.reference(tree, np.stack([M2, a_b_c[:, 2]], axis=1), np.array([[2.0, 1.0], [2.0, 1.0]]) / 3)
    A = M3.shape[1] // 2
    comes = np.repeat((depth >= 0)[:, None] & ((third[None] * R3).sum(axis=2) > 0), A, axis=1)   # [S, 2A]
    assert comes[1].all() and comes.sum() > 2 * A
    assert (np.abs(Mc - M3)[comes] <= 1e-12 * M3[comes]).all()


@pytest.mark.parametrize("name", CPU_TREES)
def test_one_hot_weights_give_the_members_table(name):
    tree, J, w, M, R, depth, gM, gR = mr.case(name, N, "onehot")
    A = M.shape[1] // 2
    comes = np.repeat(R[:, :, 0] > 0, A, axis=1)
    assert comes[1].all()
    want = J[:, 0].astype(np.float64)
    assert (np.abs(M - want)[comes] <= 1e-14 * want[comes]).all()


@pytest.mark.parametrize("kind", mr.WEIGHTS)
@pytest.mark.parametrize("name,n", [(t, N) for t in CPU_TREES] + [("native_a5", 32), ("small", 1)])
def test_fp32_restatement_stays_within_half_the_gates(name, n, kind):
    tree, J, w, M, R, depth, gM, gR = mr.case(name, n, kind)
    got_m, got_r, _ = mr.reference(tree, J, w, dtype=np.float32)
    assert got_m.dtype == np.float32 and got_r.dtype == np.float32
    worst_m, worst_r = cr.share(got_m, M, gM), cr.share(got_r, R, gR)
    print(f"{name} n={n} {kind}: fp32 restatement uses {worst_m:.3f} of the mixture's gate, {worst_r:.3f} of the reach's")
    assert worst_m <= 0.5 and worst_r <= 0.5


# one-hot weights are left out: the mixture of one policy is that policy's table, which the reach-free average gives as well
@pytest.mark.parametrize("variant", mr.VARIANTS)
@pytest.mark.parametrize("kind", MIXED)
@pytest.mark.parametrize("name", CPU_TREES)
def test_mutations_exceed_twice_the_gate(name, kind, variant):
    tree, J, w, M, R, depth, gM, gR = mr.case(name, N, kind)
    got, _, _ = mr.reference(tree, J, w, variant=variant)
    reached = depth >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        gates_off = np.where(got == M, 0.0, np.abs(got - M) / gM)[reached]
    print(f"{name} {kind} {variant}: {gates_off.max():.3g} gates at the worst reached state")
    assert gates_off.max() > 2.0
    if variant == "average":
        V, B, h = cr.reference(tree, _with_mixture(J.astype(np.float64), got))
        g = cr.gate(tree, B, h)
        x, y = mr.exact_weights(w)
        P = V[1, :N, :N]
        off = max(float((np.abs(V[1, N, :N] - x @ P) / g[1, N, :N]).max()), float((np.abs(V[1, :N, N] - P @ y) / g[1, :N, N]).max()))
        print(f"{name} {kind}: the table average misses the Kuhn identity by {off:.3g} cross-play gates at the root")
        assert off > 2.0


def test_the_cases_exercise_the_d_equals_zero_rule():
    count = {}
    for name in CPU_TREES:
        for kind in mr.WEIGHTS:
            tree, J, w, M, R, depth, gM, gR = mr.case(name, N, kind)
            never = mr.never_reached_by_the_mixture(w, R, depth)
            count[name, kind] = int(never.sum())
            A = M.shape[1] // 2
            flat = np.einsum("ck,skca->sca", w.astype(np.float64), J.astype(np.float64).reshape(J.shape[0], N, 2, A))
            assert np.array_equal(M.reshape(-1, 2, A)[never], flat[never]), "a D == 0 row is the weighted average of the tables"
    print(count)
    assert sum(count.values()) > 0
    assert any(v > 0 for (name, kind), v in count.items() if kind == "onehot")


# ---------------------------------------------------------------------------------------------------- meta_nash
def _check_equilibrium(P, res):
    P = np.asarray(P, np.float64)
    row, col = res.row.numpy(), res.col.numpy()
    assert row.dtype == np.float64 and row.shape == (P.shape[0],) and col.shape == (P.shape[1],)
    for side in (row, col):
        assert (side >= 0).all() and abs(side.sum() - 1) <= 1e-12
    bound = 1e-9 * max(1.0, float(np.abs(P).max()))
    assert 0 <= res.gap + 1e-15 and res.gap <= bound
    assert abs(res.gap - ((P @ col).max() - (row @ P).min())) <= 1e-15 * max(1.0, float(np.abs(P).max()))
    assert (row @ P).min() - 1e-15 <= res.value <= (P @ col).max() + 1e-15
    return bound


def _linprog_value(P):
    from scipy.optimize import linprog

    P = np.asarray(P, np.float64)
    m, k = P.shape
    # max v  s.t.  (x^T P)_j >= v,  sum x = 1,  x >= 0
    res = linprog(c=np.r_[np.zeros(m), -1.0], A_ub=np.c_[-P.T, np.ones(k)], b_ub=np.zeros(k), A_eq=np.r_[np.ones(m), 0.0][None], b_eq=[1.0],
                  bounds=[(0, None)] * m + [(None, None)], method="highs")
    assert res.status == 0
    return -res.fun


def test_meta_nash_small_games():
    from util import metric

    rps = metric.meta_nash([[0, -1, 1], [1, 0, -1], [-1, 1, 0]])
    _check_equilibrium([[0, -1, 1], [1, 0, -1], [-1, 1, 0]], rps)
    assert np.allclose(rps.row.numpy(), 1 / 3, rtol=0, atol=1e-12) and np.allclose(rps.col.numpy(), 1 / 3, rtol=0, atol=1e-12)
    assert abs(rps.value) <= 1e-12
    saddle = [[3.0, 1.0, 4.0], [5.0, 2.0, 6.0], [0.0, -1.0, 9.0]]  # row 1 and column 1: 2 is the smallest of its row, the largest of its column
    res = metric.meta_nash(saddle)
    _check_equilibrium(saddle, res)
    assert res.row.tolist() == [0.0, 1.0, 0.0] and res.col.tolist() == [0.0, 1.0, 0.0] and res.value == 2.0
    one = metric.meta_nash([[-2.5]])
    assert one.row.tolist() == [1.0] and one.col.tolist() == [1.0] and one.value == -2.5 and one.gap == 0.0
    twice = [[0, -1, 1], [0, -1, 1], [1, 0, -1], [-1, 1, 0], [-1, 1, 0]]  # rock and scissors twice
    res = metric.meta_nash(twice)
    _check_equilibrium(twice, res)
    assert abs(res.value) <= 1e-12
    flat = np.full((4, 7), 0.25)
    res = metric.meta_nash(flat)
    _check_equilibrium(flat, res)
    assert res.value == 0.25 and res.gap == 0.0
    assert metric.meta_nash(twice).row.tolist() == metric.meta_nash(twice).row.tolist(), "deterministic"


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_meta_nash_seeded_games_against_linear_programming(seed):
    import torch

    from util import metric

    rng = np.random.default_rng(seed)
    full = rng.standard_normal((32, 32)) * (1.0 + 9.0 * seed)
    anti = full - full.T                                  # a symmetric game: value 0
    wide = rng.uniform(-1.0, 1.0, (5, 32))
    padded = np.concatenate([wide, np.full((27, 32), wide.min() - 1.0)])   # 27 rows the row side never plays
    for P in (full, anti, wide, padded):
        res = metric.meta_nash(torch.tensor(P))
        bound = _check_equilibrium(P, res)
        assert abs(res.value - _linprog_value(P)) <= bound + 1e-9
        assert metric.meta_nash(P).row.tolist() == res.row.tolist(), "deterministic, and an array is taken like a tensor"
    assert abs(metric.meta_nash(anti).value) <= 1e-9 * max(1.0, float(np.abs(anti).max()))
    assert abs(metric.meta_nash(padded).value - metric.meta_nash(wide).value) <= 1e-9
    assert float(metric.meta_nash(padded).row[5:].sum()) == 0.0


def test_meta_nash_refusals():
    from util import metric

    for bad in (np.zeros((33, 2)), np.zeros((0, 3)), np.zeros(4), [[float("nan")]]):
        with pytest.raises(ValueError, match="meta_nash"):
            metric.meta_nash(bad)


def test_weights_are_checked_before_anything_runs():
    import torch

    from util import metric

    class NoTree:  # two states, one action: nothing of it is touched before the weights are refused
        value_tensor = torch.zeros((2, 1, 1, 1))
        max_actions = 1

    table = torch.ones((2, 2))
    for bad in ([1.0, -1.0], [0.0, 0.0], [float("inf"), 1.0], [float("nan"), 1.0], [1.0]):
        with pytest.raises(ValueError, match="weights"):
            metric.mixture(NoTree(), [table, table], bad)
    with pytest.raises(ValueError, match="col_weights"):
        metric.mixture(NoTree(), [table, table], [1.0, 1.0], [1.0, -1.0])
    with pytest.raises(ValueError, match="1 to 32"):
        metric.mixture(NoTree(), [])


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_size_export():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_mixture_size(2, 1) == 4
    assert lib.rnad_mixture_size(283, 8) == 2 * 283 * 8
    assert lib.rnad_mixture_size(2**33, 32) == 2**33 * 64
    for S, n in ((283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_mixture_size(S, n) == -1, (S, n)


def test_binding_refuses_a_cpu_tensor():
    import torch

    import rnad_hip

    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.mixture(None, torch.zeros(22, 2, 4), torch.full((2, 2), 0.5))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.mixture(None, torch.zeros(22, 4), torch.full((2, 2), 0.5))


def test_null_arguments_are_refused_on_the_host():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_mixture(None, 2, None, None, None, None, None) != 0
    assert b"rnad_mixture" in lib.rnad_last_error()
