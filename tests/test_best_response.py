"""Best responses without a GPU: the reference and gates of tests/_brref.py are pinned by what a best response must do, not by a
measurement --

  - the reference project's recorded row_best / col_best (tests/golden/nashconv_*.npz, for its net's table and for the tree's solution)
    lie within the gate of V at every reached state;
  - the performance-difference identity: sum_s R * G is the exploitability that the fp64 cross-play recursion of tests/_crossref.py
    gives, per player and side;
  - the best-response table is a policy: played through that recursion it earns V[1] on both sides, and no member earns more;
  - an fp32 restatement in the kernel's order stays within half of every gate on the four golden trees (on the native trees its reach
    comes to 0.50 of the gate -- 12 roundings of up to 2^-24 each against 13 -- so the half is not asked there; the gates themselves are
    what tests/test_hip_best_response.py asks at every state of every tree);
  - six natural mistakes land beyond twice some gate, or pick an action whose response lies more than twice the gate below the maximum;
  - the cases hold exact ties, illegal actions that would beat the legal ones, and gains that a table's own rounding turns negative;

and the host half of the C ABI is checked.
"""
import numpy as np
import pytest

import _brref as br
import _crossref as cr
from _util import TREES, load

CPU_TREES = TREES + ("native_a5",)
N = 6  # solution, uniform, (fixture,) and seeded softmax tables


def _shares(c, got):
    R = c.reached
    return dict(V=cr.share(got.V[R], c.ref.V[R], c.gV[R]), Q=cr.share(got.Q[R], c.ref.Q[R], c.gQ[R]),
                G=cr.share(got.G[R], c.ref.G[R], c.gG[R]), R=cr.share(got.R[R], c.ref.R[R], c.gR[R]))


def _regret_in_gates(c, best):
    R = c.reached
    with np.errstate(divide="ignore", invalid="ignore"):
        regret = br.picked_regret(c.ref, best)[R]
        return float(np.where(regret == 0, 0.0, regret / c.gV[R]).max())


@pytest.mark.parametrize("name", TREES)
def test_reference_matches_the_recorded_best_response_values(name):
    tree = cr.tree_arrays(name)
    z = load("nashconv_" + name)
    for prefix, table in (("", z["joint_policy"]), ("sol_", tree["solution"])):
        J = np.asarray(table, np.float32)[:, None]
        ref = br.reference(tree, J)
        gV = br.gates(tree, ref, J)[0]
        R = ref.depth >= 0
        assert R.sum() > 1
        for side, key in enumerate(("row_best", "col_best")):
            err = np.abs(z[prefix + key][R].astype(np.float64) - ref.V[R, side, 0])
            print(f"{name} {prefix}{key}: at most {err.max():.3g}, {cr.share(z[prefix + key][R], ref.V[R, side, 0], gV[R, side, 0]):.3f} of the gate")
            assert (err <= gV[R, side, 0]).all()


@pytest.mark.parametrize("name", CPU_TREES)
def test_performance_difference_identity(name):
    c = br.case(name, N)
    V, B, h = cr.reference(c.tree, c.J.astype(np.float64))
    own = np.diagonal(V[1])
    want = np.stack([c.ref.V[1, 0] - own, c.ref.V[1, 1] + own], axis=1)     # [n, 2]
    got = br.exploitability(c.ref)
    print(f"{name}: identity to {np.abs(got - want).max():.3g}")
    assert (np.abs(got - want) <= 1e-12 * c.ref.B[1].T).all()


@pytest.mark.parametrize("name", CPU_TREES)
def test_the_best_response_table_is_a_policy_that_earns_the_values(name):
    c = br.case(name, N)
    everyone = np.concatenate([c.J.astype(np.float64), c.ref.best], axis=1)
    V, B, h = cr.reference(c.tree, everyone)
    tol, A = 1e-12 * B[1], c.J.shape[2] // 2
    for k in range(N):
        assert abs(V[1, N + k, k] - c.ref.V[1, 0, k]) <= tol[N + k, k], "the exploiter's row side against member k's column side"
        assert abs(-V[1, k, N + k] - c.ref.V[1, 1, k]) <= tol[k, N + k], "member k's row side against the exploiter's column side"
        # a member's fp32 table is no exact distribution: a side sums to 1 + delta, |delta| <= A u, at each of the h[1] states of a path,
        # and a payoff is linear in each of them -- that much a member may "earn" above the maximum over true policies
        loose = tol + ((1 + A * br.U) ** int(h[1]) - 1) * B[1]
        assert (c.ref.V[1, 0, k] >= V[1, :N, k] - loose[:N, k]).all(), "no member's row side earns more against k than its best response"
        assert (c.ref.V[1, 1, k] >= -V[1, k, :N] - loose[k, :N]).all()
    hot = c.ref.best[c.reached].reshape(-1, N, 2, c.J.shape[2] // 2)
    assert set(np.unique(hot)) <= {0.0, 1.0} and (hot.sum(axis=3) == 1).all(), "one action per reached state, side and member"


@pytest.mark.parametrize("name,n", [(t, N) for t in TREES] + [(t, 32) for t in TREES] + [("small", 1)])
def test_fp32_restatement_stays_within_half_the_gates(name, n):
    c = br.case(name, n)
    got = br.reference(c.tree, c.J, dtype=np.float32)
    shares = _shares(c, got)
    regret = _regret_in_gates(c, got.best)
    print(f"{name} n={n}: fp32 restatement uses {shares} of the gates; its action lies {regret:.3f} gates below the maximum")
    assert max(shares.values()) <= 0.5 and regret <= 1.0
    assert (got.best[~c.reached] == 0).all() and (got.R[~c.reached] == 0).all()


MUTATIONS = [(t, v) for t in CPU_TREES for v in ("swapped", "one_step", "plus_terminal", "reach_kreach")] + [("ragged", "illegal")] + \
            [(t, "reach_no_chance") for t in CPU_TREES if t != "c1"]  # c1 has one chance outcome per joint action: chance is 1 there


@pytest.mark.parametrize("name,variant", MUTATIONS)
def test_mutations_exceed_twice_a_gate(name, variant):
    c = br.case(name, N)
    got = br.reference(c.tree, c.J, variant=variant)
    shares = _shares(c, got)
    regret = _regret_in_gates(c, got.best)
    print(f"{name} {variant}: {shares} gates off, the picked action {regret:.3g} gates below the maximum")
    if variant.startswith("reach"):
        assert shares["R"] > 2.0 and shares["V"] == 0.0
    else:
        assert shares["V"] > 2.0 and shares["G"] > 2.0 and regret > 2.0 and shares["R"] == 0.0


def test_the_cases_hold_ties_illegal_winners_and_negative_gains():
    ties, winners, negative = {}, {}, {}
    for name in CPU_TREES:
        c = br.case(name, N)
        ref, R = c.ref, c.reached
        A = ref.Q.shape[3]
        ok = ref.legal[:, :, None, :]
        attained = ((ref.Q == ref.V[..., None]) & ok).sum(axis=3)[R]
        assert (attained >= 1).all()
        ties[name] = int((attained >= 2).sum())
        first = np.where(ok, ref.Q, -np.inf).argmax(axis=3)
        picked = ref.best.reshape(-1, N, 2, A).transpose(0, 2, 1, 3).argmax(axis=3)
        assert np.array_equal(first[R], picked[R]), "ties go to the lowest legal index"
        winners[name] = int((np.where(~ok, ref.Q, -np.inf).max(axis=3) > ref.V)[R].sum())
        negative[name] = int((ref.G[R] < 0).sum())
        # a table's side sums to 1 + at most A roundings of fp32: where every action it plays ties, it "earns" that much above the maximum
        assert (ref.G[R] >= -(A + 2) * br.U * ref.P_abs[R]).all()
    print("exact ties", ties, "illegal actions that beat the legal ones", winners, "negative gains", negative)
    assert sum(ties.values()) > 0 and ties["small"] > 0
    assert winners["ragged"] > 0 and sum(v for k, v in winners.items() if k != "ragged") == 0
    assert sum(negative.values()) > 0


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_size_export():
    import rnad_hip

    lib = rnad_hip.lib()
    for S, n in ((2, 1), (283, 8), (2**33, 32), (283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_best_response_size(S, n) == br.size(S, n), (S, n)
    assert br.size(283, 8) == 2 * 283 * 8 and br.size(1, 1) == -1 and br.size(283, 33) == -1


def test_binding_refuses_a_cpu_tensor():
    import torch

    import rnad_hip

    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.best_response(None, torch.zeros(22, 2, 4))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.best_response(None, torch.zeros(22, 4))


def test_null_arguments_are_refused_on_the_host():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_best_response(None, 2, None, None, None, None, None, None) != 0
    assert b"rnad_best_response" in lib.rnad_last_error()


def test_players_are_counted_before_anything_runs():
    import torch

    from util import metric

    class NoTree:  # two states, one action: nothing of it is touched before the player count is refused
        value_tensor = torch.zeros((2, 1, 1, 1))
        max_actions = 1

    with pytest.raises(ValueError, match="best_response takes 1 to 32"):
        metric.best_response(NoTree(), [])
    with pytest.raises(ValueError, match="1 to 32"):
        metric.best_response(NoTree(), [torch.ones((2, 2))] * 33)
