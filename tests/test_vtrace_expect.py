"""The exact expected learner update without a GPU.  The sweep of tests/_vtexpref.py (the kernel's recursion, csrc/vtrace_expect.hip) is
pinned by its definition, not by a measurement --

  - in fp64 it equals the ENUMERATION: `_learnref.learner(np.float64, ...)` run on every complete episode of a hand-sized ragged tree,
    each lane weighted by its probability: reach, target, q where the behaviour draws, the value-head sums on every row, and the NeuRD
    sums at threshold 50 and clip 2^30 (every gate open: the linear case);
  - on rows with a closed gate `linear` is false and the direction is the gated one at the expected q; where `linear` is true under the
    set's own threshold and clip, the enumeration's NeuRD sum is the direction at the expected q;
  - with eta = 0, mu = pip, rho, c >= 1 and lambda = gamma = 1 the target is the fp64 cross-play value of pip with itself, whatever the
    bootstrap vv;
  - the fp32 restatement stays within half of every derived gate on the GPU sweep's inputs;
  - eight natural mistakes land beyond twice a gate;

and the host half of the C ABI is checked: the header, the exports, the refusals, the scratch of the eight instantiations."""
import os
import types

import numpy as np
import pytest

import _crossref as cr
import _vtexpref as vx
from _util import TREES

HAND = tuple(vx.HAND_TREES)
HAND_CASES = [(t, h, b) for t in HAND for h in vx.SETS for b in vx.BEHAVIOURS]
CPU_TREES = TREES
SWEEP_TREES = tuple(t for t in vx.ALL_TREES if not t.startswith("native"))  # A = 1 .. 8, C = 1 .. 4; the two large ones run on the GPU


def open_gates(hp):
    """The set with threshold 50 and clip 2^30: no gate closes, no clip binds; nothing else of the program depends on the two."""
    return types.SimpleNamespace(**{**vars(hp), "threshold": 50.0, "clip": 2.0 ** 30})


def test_the_hand_trees_hold_what_the_enumeration_must_meet():
    assert {vx.HAND_TREES[t]["A"] for t in HAND} >= {2, 3} and any(vx.HAND_TREES[t]["C"] == 1 for t in HAND)
    for t in HAND:
        tree = vx.hand_tree(t)
        index, chance, legal = tree["index"], tree["chance"], tree["legal"][:, 0]
        levels = cr.level_order(index, chance)
        reached = np.concatenate(levels)
        assert (legal[reached].reshape(len(reached), -1) == 0).any(), "illegal actions"
        if vx.HAND_TREES[t]["C"] > 1:
            assert ((chance[reached] <= 0) & (legal[reached][:, None] > 0)).any(), "zero-chance records of legal joint actions"
        exits = [((index[lv] == 0) & (chance[lv] > 0)).any() for lv in levels]
        assert len(levels) >= 2 and exits[-1] and (any(exits[:-1]) or len(levels) == 2), "episodes that leave the tree early"
    zeros = 0
    for t, h, b in HAND_CASES:
        c = vx.hand_case(t, h, b)
        en = vx.enumeration(c.tree, c.mu_tab, c.tables, c.hp)
        rows = np.concatenate([en.reach > 0] * 2)
        assert en.episodes <= 4000
        assert not ((c.pip > 0) & (c.mu_tab == 0))[rows].any(), "pip > 0 where mu = 0 on a reached row"
        zeros += int(((c.mu_tab == 0) & (c.legal_tab > 0))[rows].sum())
    assert zeros > 0, "mu zeros where pip is zero"


@pytest.mark.parametrize("hp_name", vx.SETS)
def test_the_inputs_reach_both_clips_binding_and_not(hp_name):
    """On the reference alone: off-policy weights fall on both sides of rho and of c for every hyperparameter set."""
    for t in HAND:
        c = vx.hand_case(t, hp_name, "softmax")
        cov = vx.clip_coverage(vx.sweep_of(c), [vx.hyper_of(c.hp)])
        assert min(cov.values()) > 0.05, (t, cov)


@pytest.mark.parametrize("tree,hp_name,kind", HAND_CASES)
def test_fp64_reference_equals_the_enumeration(tree, hp_name, kind):
    c = vx.hand_case(tree, hp_name, kind)
    hp = open_gates(c.hp)
    en = vx.enumeration(c.tree, c.mu_tab, c.tables, hp)
    ref = vx.sweep_of(c, hp)
    S = c.S
    seen = np.concatenate([en.reach > 0] * 2)
    assert np.array_equal(en.reach > 0, ref.R[:, 0] > 0) and en.episodes <= 4000
    tol = 1e-12
    assert (np.abs(ref.R[:, 0] - en.reach) <= tol * en.reach).all()
    tg, tg_m = vx.to_rows(ref.target.v[:, 0], True), vx.to_rows(ref.target.m[:, 0], True)
    q, q_m = vx.to_rows(ref.q.v[:, 0]), vx.to_rows(ref.q.m[:, 0])
    err_t = np.abs(tg - en.target)[seen]
    assert (err_t <= tol * tg_m[seen]).all()
    drawn = (c.mu_tab > 0) & (c.legal_tab > 0) & seen[:, None]
    err_q = np.abs(q - en.q)
    assert (err_q[drawn] <= tol * q_m[drawn]).all()
    # what the program leaves where the behaviour never draws: vv - eta lpol (an illegal action: vv)
    assert (err_q[seen] <= tol * q_m[seen]).all()
    ex = vx.expected_tables(c.tree, c.tables, c.legal_tab, c.mu_tab, c.pip, c.lpol, hp, tg, q, ref.R[:, 0])
    reach2, L = np.concatenate([ref.R[:, 0]] * 2), ex["length"]
    v = np.asarray(c.tables["v"], np.float64)
    err_dv = np.abs(ex["dv_tab"] * L - en.dv_sum)
    assert (err_dv <= tol * 2 * hp.w_v * reach2 * (np.abs(v) + tg_m)).all(), "the value head's sums on every row"
    assert ex["linear"][seen].all() and not ex["linear"][~seen].any()
    mag_dl = hp.w_n * reach2 * 2 * (q_m.max(-1) + (c.pip * q_m).sum(-1))
    err_dl = np.abs(ex["dlogit_tab"] * L - en.dlogit_sum)
    assert (err_dl <= tol * mag_dl[:, None]).all(), "the NeuRD sums with every gate open"
    print(f"{tree} {hp_name} {kind}: {en.episodes} episodes, S = {S}; reach {np.abs(ref.R[:, 0] - en.reach).max():.2g}, target "
          f"{err_t.max():.2g}, q {err_q[seen].max():.2g}, dv {err_dv.max():.2g}, dlogit {err_dl.max():.2g}")


@pytest.mark.parametrize("tree,hp_name", [(t, h) for t in HAND for h in vx.SETS])
def test_closed_gates_are_not_linear_and_linear_rows_are_the_expectation(tree, hp_name):
    c = vx.hand_case(tree, hp_name, "softmax")
    hp = c.hp
    en = vx.enumeration(c.tree, c.mu_tab, c.tables, hp)
    ref = vx.sweep_of(c)
    tg, q = vx.to_rows(ref.target.v[:, 0], True), vx.to_rows(ref.q.v[:, 0])
    ex = vx.expected_tables(c.tree, c.tables, c.legal_tab, c.mu_tab, c.pip, c.lpol, hp, tg, q, ref.R[:, 0])
    reach2, L = np.concatenate([ref.R[:, 0]] * 2), ex["length"]
    logit = np.asarray(c.tables["logit"], np.float64)
    A = logit.shape[1]
    closed = 0
    for row in np.flatnonzero(reach2 > 0):  # the gated direction at the expected q, element by element
        l = logit[row] - (logit[row] * c.legal_tab[row]).sum() / A
        adv = np.clip(q[row] - (c.pip[row] * q[row]).sum(), -hp.clip, hp.clip)
        f = np.zeros(A)
        shut = False
        for a in range(A):
            if c.legal_tab[row, a] == 0:
                continue
            lo, hi = l[a] > -hp.threshold, l[a] < hp.threshold
            shut |= not (lo and hi)
            f[a] = (min(adv[a], 0) if lo else 0) + (max(adv[a], 0) if hi else 0)
        want = -hp.w_n * (f - c.legal_tab[row] * f.sum() / A) * reach2[row] / L
        assert np.allclose(ex["dlogit_tab"][row], want, rtol=1e-12, atol=1e-15)
        if shut:
            closed += 1
            assert not ex["linear"][row]
    if hp_name in ("H1", "H2", "H3"):
        assert closed > 0, "no row with a closed gate"
    lin = ex["linear"]
    mag = hp.w_n * reach2 * 4 * np.abs(en.q).max(-1)
    assert (np.abs(ex["dlogit_tab"] * L - en.dlogit_sum)[lin] <= 1e-11 * (1 + mag[lin, None])).all(), "a row marked linear is not"
    print(f"{tree} {hp_name}: {int(lin.sum())} linear rows of {int((reach2 > 0).sum())} reached, {closed} with a closed gate")


@pytest.mark.parametrize("name", CPU_TREES)
def test_on_policy_without_regularisation_the_target_is_the_cross_play_value(name):
    tree = dict(cr.tree_arrays(name))
    J = cr.players(tree, 4, 0, cr.fixture_policy(name)).astype(np.float64)
    S, n, A2 = J.shape
    live = np.asarray(tree["chance"], np.float64) * (np.asarray(tree["chance"]) > 0)
    tree["chance"] = live / np.where(live.sum(1, keepdims=True) > 0, live.sum(1, keepdims=True), 1)  # the column side's vv (1 - sum p) likewise
    for side in (slice(0, A2 // 2), slice(A2 // 2, A2)):  # distributions to 1e-16: vv (1 - sum mu0 mu1) is what does not telescope
        tot = J[:, :, side].sum(-1, keepdims=True)
        J[:, :, side] /= np.where(tot > 0, tot, 1)
    rng = np.random.default_rng(5)
    VV = rng.standard_normal((S, n, 2))  # the bootstrap telescopes away: any value will do
    hyper = [(0.0, 1.0, 1.0, 1.0, 1.0), (0.0, 1.0, 1.0, 1.5, 1.0), (0.0, 1.0, 1.0, 1.0, 2.0), (0.0, 1.0, 1.0, 4.0, 3.0)]
    ref = vx.reference(np.float64, tree, J, J, rng.standard_normal(J.shape), VV, hyper)
    V, B, h = cr.reference(tree, J)
    R = ref.depth >= 0
    k = np.arange(n)
    bound = 1e-12 * np.maximum(B[R][:, k, k], ref.target.m[R].max(-1))
    assert (np.abs(ref.target.v[R][:, :, 0] - V[R][:, k, k]) <= bound).all()
    assert (np.abs(ref.target.v[R][:, :, 1] + V[R][:, k, k]) <= bound).all()
    # the column player's target is conditioned on the row action: its mean under the row policy is the unconditioned one
    mean = (J[:, :, :A2 // 2] * ref.W1.v).sum(-1)
    assert (np.abs(mean[R] + V[R][:, k, k]) <= bound).all()


@pytest.mark.parametrize("name", SWEEP_TREES)
def test_fp32_restatement_stays_within_half_the_gates(name):
    c = vx.case(name)
    got = vx.values_of(vx.reference(np.float32, c.tree, c.MU, c.PIP, c.LPOL, c.VV, c.hyper))
    shares = vx.shares(c, got)
    print(f"{name}: fp32 restatement uses {shares} of the gates")
    assert max(shares["target"], shares["target_given_row"], shares["q"]) <= 0.5
    assert shares["reach"] <= (0.5 if name in TREES else 1.0)  # (tests/test_best_response.py: 0.50 of the gate on the generated trees)
    for a in got.values():
        assert (a[~c.reached] == 0).all()
    few = vx.values_of(vx.reference(np.float32, c.tree, c.MU[:, :3], c.PIP[:, :3], c.LPOL[:, :3], c.VV[:, :3], c.hyper[:3]))
    assert all(np.array_equal(few[k], got[k][:, :3]) for k in vx.OUTPUTS), "the members do not see each other"


BEYOND = dict(rho_c=("target",), no_lambda=("target",), opp_entropy_sign=("target", "q"), w1_mean=("target_given_row",),
              gamma_child=("target", "q"), q0_no_cs=("q",), reward_sign=("target", "q"), no_chance=("target", "q"))
MUTATIONS = [(t, v) for t in CPU_TREES for v in vx.VARIANTS if not (t == "c1" and v == "no_chance")]  # (c1: one outcome, chance 1)


@pytest.mark.parametrize("name,variant", MUTATIONS)
def test_mutations_exceed_twice_a_gate(name, variant):
    c = vx.case(name)
    n = 12  # every hyperparameter set with every behaviour
    got = vx.values_of(vx.reference(np.float64, c.tree, c.MU[:, :n], c.PIP[:, :n], c.LPOL[:, :n], c.VV[:, :n], c.hyper[:n], variant=variant))
    shares = vx.shares(c, got, n)
    print(f"{name} {variant}: {shares} gates off")
    for key in BEYOND[variant]:
        assert shares[key] > 2.0
    assert shares["reach"] == 0.0


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_the_header_declares_the_three_entry_points():
    import ctypes as C

    import rnad_hip

    protos = rnad_hip.header_prototypes()
    assert protos["rnad_vtrace_expect_size"] == (C.c_int64, [C.c_int64, C.c_int])
    assert protos["rnad_vtrace_expect_workspace"] == (C.c_int64, [C.c_int64, C.c_int, C.c_int])
    assert protos["rnad_vtrace_expect"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 11)


def test_the_library_exports_them_and_the_size_companions_answer():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_vtrace_expect is not None
    for S, n in ((2, 1), (283, 8), (2**33, 32), (283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_vtrace_expect_size(S, n) == vx.size(S, n), (S, n)
        for A in (0, 1, 3, 8, 9):
            assert lib.rnad_vtrace_expect_workspace(S, A, n) == vx.workspace(S, A, n), (S, A, n)
    assert vx.workspace(283, 3, 8) == 283 * 8 * 14 and vx.size(1, 1) == -1


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = vx.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    print({A: table[A] for A in sorted(table)})
    assert sorted(table) == list(range(1, 9)), "one k_vtrace_expect per A = 1 .. 8"
    assert all(k["scratch"] == 0 for k in table.values())
    assert all(k["lds"] == 4 * A * A * 8 * 3 * 4 for A, k in table.items()), "four waves' record slices, nothing else"


def test_null_arguments_and_a_cpu_tensor_are_refused_on_the_host():
    import torch

    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_vtrace_expect(None, 2, *([None] * 11)) != 0
    assert b"rnad_vtrace_expect" in lib.rnad_last_error()
    z = torch.zeros(22, 2, 4)
    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.vtrace_expect(None, [(0.2, 1.0, 1.0, 1.0, 1.0)] * 2, z, z, z, torch.zeros(22, 2, 2))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.vtrace_expect(None, [(0.2, 1.0, 1.0, 1.0, 1.0)], torch.zeros(22, 4), torch.zeros(22, 4), torch.zeros(22, 4), torch.zeros(22, 2))
