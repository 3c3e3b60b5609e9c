"""The exact variance of the learner update without a GPU.  The sweep of tests/_vtmomref.py (the kernel's recursion,
csrc/vtrace_moments.hip) is pinned by its definition, not by a measurement --

  - in fp64 it equals the ENUMERATION: the second central moments of `_learnref.learner(np.float64, ...)`'s per-slot v_target and q over
    every complete episode of a hand-sized ragged tree, each lane weighted by its probability, the column slots also grouped by the row
    action taken: target_var, target_given_row_var and q_var at every action, on the 48 cases of tests/test_vtrace_expect.py;
  - the inputs put importance weights on both sides of rho and of c, and some reached row has a q_var that the 1 / mu term dominates;
  - with C = 1 and a one-hot behaviour nothing is random: the enumeration's variances are exactly 0 and the sweep's are squares of the
    rounding residue of the first moments' round trip W = vv + (W - vv), below (8 eps)^2 of their magnitude;
  - with eta = 0, mu = pip, rho, c >= 1 and lambda = gamma = 1 both players' target_var is the variance of the game's payoff from the
    state under the policy, whatever the bootstrap vv (an independent recursion on E[r] and E[r^2]);
  - dv_var_tab, target_noise and episodes_for_unit_snr equal their definitions computed from the enumeration's per-lane sums;
  - the fp32 restatement stays within half of every derived gate for A = 1 .. 8 and C = 1 .. 4;
  - eight natural mistakes land beyond twice a gate;

and the host half of the C ABI is checked: the header, the exports, the size helper, the refusals, the scratch of the eight
instantiations."""
import os
import types

import numpy as np
import pytest

import _crossref as cr
import _learnref as lr
import _vtexpref as vx
import _vtmomref as vm
from _util import TREES

HAND = tuple(vx.HAND_TREES)
HAND_CASES = [(t, h, b) for t in HAND for h in vx.SETS for b in vx.BEHAVIOURS]
SWEEP_TREES = tuple(t for t in vx.ALL_TREES if not t.startswith("native"))  # A = 1 .. 8, C = 1 .. 4; the two large ones run on the GPU


def _rows(ref, S):
    """(target_var [2S], target_given_row_var [S, A], q_var [2S, A]) values and magnitudes of the single member of a hand case."""
    pick = lambda x: (vx.to_rows(x.v[:, 0], scalar=x.v.shape[-1] == 2), vx.to_rows(x.m[:, 0], scalar=x.v.shape[-1] == 2))  # noqa: E731
    return pick(ref.tvar), (ref.V1.v[:, 0], ref.V1.m[:, 0]), pick(ref.qvar)


@pytest.mark.parametrize("tree_name,hp_name,kind", HAND_CASES)
def test_the_fp64_sweep_is_the_enumeration(tree_name, hp_name, kind):
    c = vx.hand_case(tree_name, hp_name, kind)
    en = vm.enumeration(c.tree, c.mu_tab, c.tables, c.hp)
    ref = vm.sweep_of(c)
    S = c.S
    seen = en.reach > 0
    assert seen[1] and ref.reached[seen].all()
    (tv, tm), (gv, gm), (qv, qm) = _rows(ref, S)
    seen2 = np.concatenate([seen, seen])
    drawn = c.mu_tab > 0
    assert (np.abs(tv - en.target_var)[seen2] <= 1e-12 * tm[seen2]).all()
    assert (np.abs(qv - en.q_var)[seen2][drawn[seen2]] <= 1e-12 * qm[seen2][drawn[seen2]]).all(), "q_var at every action drawn"
    # an action never drawn has a constant q: exactly 0 in the sweep, the square of the mean's rounding residue in the enumeration
    assert (qv[seen2][~drawn[seen2]] == 0).all() and (en.q_var[seen2][~drawn[seen2]] <= 1e-24 * (1 + en.q[seen2][~drawn[seen2]] ** 2)).all()
    assert (np.abs(gv - en.given_row_var)[seen] <= 1e-12 * gm[seen]).all()
    assert (gv[seen][~drawn[:S][seen]] == 0).all(), "a row action never drawn conditions on nothing"
    if en.episodes > 1:  # (a2c1d5 under H2's coarse pip and the behaviour with zeros plays one episode: nothing is random)
        assert en.target_var[seen2].max() > 0 and en.q_var[seen2].max() > 0 and en.given_row_var[seen].max() > 0
    # the first moments the sweep stands on are the enumeration's too
    exp = vx.sweep_of(c)
    assert np.allclose(exp.W1.v[:, 0][seen][drawn[:S][seen]], en.given_row[seen][drawn[:S][seen]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("hp_name", vx.SETS)
def test_the_inputs_reach_both_clips_and_a_row_the_inverse_mu_term_dominates(hp_name):
    below = above = 0.0
    dominated = 0
    for t in HAND:
        for b in vx.BEHAVIOURS:
            c = vx.hand_case(t, hp_name, b)
            exp = vx.sweep_of(c)
            cov = vx.clip_coverage(exp, [vx.hyper_of(c.hp)])
            below, above = below + cov["rho_below"] + cov["c_below"], above + cov["rho_above"] + cov["c_above"]
            if b == "on_policy":
                continue
            assert min(cov["rho_below"], cov["rho_above"], cov["c_below"], cov["c_above"]) > 0, (t, b, cov)
            ref = vm.sweep_of(c)
            S = c.S
            qv = vx.to_rows(ref.qvar.v[:, 0])
            tbar = vx.to_rows(exp.q.v[:, 0]) - (np.asarray(c.tables["v_target"], np.float64).reshape(-1, 1) - c.hp.eta * c.lpol)
            mu = c.mu_tab
            seen = np.concatenate([exp.depth >= 0] * 2)[:, None] & (mu > 0) & (mu < 0.1)
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(seen, (1 - mu) * tbar ** 2 / mu / qv, 0.0)
            dominated += int((share > 0.5).sum())
    assert below > 0 and above > 0
    assert dominated > 0, "some q_var with mu < 0.1 is mostly (1 - mu) tbar^2 / mu"


def test_a_deterministic_behaviour_on_a_tree_without_chance_has_no_variance():
    c = vx.hand_case("a2c1d5", "H1", "softmax")
    assert c.tree["index"].shape[1] == 1
    one_hot = np.zeros_like(c.mu_tab)
    first_legal = np.argmax(c.legal_tab > 0, axis=-1)
    one_hot[np.arange(one_hot.shape[0]), first_legal] = (c.legal_tab.sum(-1) > 0)
    d = types.SimpleNamespace(**{**vars(c), "mu_tab": one_hot})
    ref = vm.sweep_of(d)
    R = ref.reached
    eps = np.finfo(np.float64).eps
    for x in (ref.tvar, ref.V1, ref.qvar):  # a deviation is a few roundings of its magnitude, a variance's magnitude is that squared
        assert (x.v[R] <= (8 * eps) ** 2 * x.m[R]).all()
    en = vm.enumeration(d.tree, one_hot, d.tables, d.hp)
    assert en.episodes == 1 and en.target_var.max() == 0 and en.q_var.max() == 0


@pytest.mark.parametrize("tree_name", HAND)
def test_on_policy_without_clips_target_var_is_the_variance_of_the_payoff(tree_name):
    c = vx.hand_case(tree_name, "H0", "on_policy")
    hp = lr._hp(alpha=0.5, eta=0.0, lambda_=1.0, c=2.0, rho=3.0, gamma=1.0)
    tree, S = c.tree, c.S
    rng = np.random.default_rng(5)
    d = types.SimpleNamespace(**{**vars(c), "mu_tab": c.pip, "tables": {**c.tables, "v_target": rng.standard_normal(2 * S)}})
    ref = vm.sweep_of(d, hp)
    # the independent recursion: E[r] and E[r^2] from a state under the policy
    index, chance, value = (np.asarray(tree[k]) for k in ("index", "chance", "value"))
    A = index.shape[2]
    E1, E2 = np.zeros(S), np.zeros(S)
    for level in reversed(cr.level_order(index, chance)):
        for s in level:
            w = c.pip[s][None, :, None] * c.pip[S + s][None, None, :] * np.where(chance[s] > 0, chance[s], 0.0)
            u = np.where(chance[s] > 0, index[s], 0)
            E1[s] = (w * np.where(u == 0, value[s], E1[u])).sum()
            E2[s] = (w * np.where(u == 0, value[s] ** 2, E2[u])).sum()
    var = E2 - E1 ** 2
    R = ref.reached & (vx.sweep_of(d, hp).R[:, 0] > 0)
    assert R.sum() > 3 and var[R].max() > 0.01 and A >= 2
    for P in range(2):
        assert (np.abs(ref.tvar.v[R, 0, P] - var[R]) <= 1e-12 * np.maximum(ref.tvar.m[R, 0, P], E2[R])).all(), P


@pytest.mark.parametrize("tree_name,hp_name,kind", [(t, h, b) for t, h, b in HAND_CASES if b != "on_policy"][::3])
def test_the_host_tables_are_their_definitions_on_the_enumeration(tree_name, hp_name, kind):
    c = vx.hand_case(tree_name, hp_name, kind)
    en = vm.enumeration(c.tree, c.mu_tab, c.tables, c.hp)
    ref, exp = vm.sweep_of(c), vx.sweep_of(c)
    S = c.S
    got = vm.noise_tables(c.hp, c.tables["v"], vx.to_rows(exp.target.v[:, 0], scalar=True), vx.to_rows(ref.tvar.v[:, 0], scalar=True), exp.R[:, 0])
    L = en.reach.sum()
    scale = (2 * c.hp.w_v / L) ** 2
    dv_var = scale * (en.dv2 - en.dv1 ** 2)  # one episode's entry of dv_tab is 2 w_v (v - v_target) / L at the row's slot, 0 if not visited
    assert np.allclose(got["dv_var_tab"], dv_var, rtol=1e-9, atol=1e-14 * scale)
    reach2 = np.concatenate([en.reach, en.reach])
    noise = reach2 * en.target_var
    assert np.allclose(got["target_noise"], [noise[:S].sum(), noise[S:].sum()], rtol=1e-10)
    signal = scale * en.dv1 ** 2
    want = [dv_var[:S].sum() / signal[:S].sum(), dv_var[S:].sum() / signal[S:].sum()]
    assert np.allclose(got["episodes_for_unit_snr"], want, rtol=1e-8, atol=1e-20) and (min(want) > 0 or en.episodes == 1)
    flat = vm.noise_tables(c.hp, vx.to_rows(exp.target.v[:, 0], scalar=True), vx.to_rows(exp.target.v[:, 0], scalar=True),
                           vx.to_rows(ref.tvar.v[:, 0], scalar=True), exp.R[:, 0])
    assert np.isinf(flat["episodes_for_unit_snr"]).all(), "no signal: v already is the target"


def _sweep_case(name, n=None):
    """(arguments, first moments rounded to fp32, fp64 reference, gates) of the first n members of a `_vtexpref.case`."""
    c = vx.case(name)
    n = c.n if n is None else n
    a = (c.MU[:, :n], c.PIP[:, :n], c.LPOL[:, :n], c.VV[:, :n])
    exp = c.ref if n == c.n else vx.reference(np.float64, c.tree, *a, c.hyper[:n])
    first = vm.first_of(np.float32, *a, exp)
    ref = vm.reference(np.float64, c.tree, *a, c.hyper[:n], first)
    return c, a, first, ref, vm.gates(c.tree, ref)


@pytest.mark.parametrize("name", SWEEP_TREES)
def test_fp32_restatement_stays_within_half_the_gates(name):
    c, a, first, ref, g = _sweep_case(name)
    got = vm.values_of(vm.reference(np.float32, c.tree, *a, c.hyper, first))
    shares = vm.shares(ref, g, got)
    print(f"{name}: fp32 restatement uses {shares} of the gates")
    assert max(shares.values()) <= 0.5
    assert np.array_equal(ref.reached, c.reached)
    for x in got.values():
        assert (x[~ref.reached] == 0).all() and (x >= 0).all()
    few = vm.values_of(vm.reference(np.float32, c.tree, *(x[:, :3] for x in a), c.hyper[:3],
                                    types.SimpleNamespace(target=first.target[:, :3], W1=first.W1[:, :3], q=first.q[:, :3],
                                                          rec=first.rec[:, :, :3])))
    assert all(np.array_equal(few[k], got[k][:, :3]) for k in vm.OUTPUTS), "the members do not see each other"


def test_the_gate_constant():
    assert [vm.K_of(A, C) for A, C in ((1, 1), (3, 2), (8, 4))] == [36, 47, 74]


BEYOND = dict(c_not_squared=("target_var", "target_given_row_var"), v1_mean=("target_given_row_var", "q_var"), no_between=("target_var",),
              no_tbar=("q_var",), mu_squared=("q_var",), rho_c=("target_var", "target_given_row_var", "q_var"),
              no_chance=("target_var", "target_given_row_var", "q_var"), reward_sign=("target_var", "target_given_row_var", "q_var"))
MUTATIONS = [(t, v) for t in TREES for v in vm.VARIANTS if not (t == "c1" and v == "no_chance")]  # (c1: one outcome, chance 1)


@pytest.mark.parametrize("name,variant", MUTATIONS)
def test_mutations_exceed_twice_a_gate(name, variant):
    n = 12  # every hyperparameter set with every behaviour
    c, a, first, ref, g = _sweep_case(name, n)
    got = vm.values_of(vm.reference(np.float64, c.tree, *a, c.hyper[:n], first, variant=variant))
    shares = vm.shares(ref, g, got)
    print(f"{name} {variant}: {shares} gates off")
    for key in BEYOND[variant]:
        assert shares[key] > 2.0


def test_the_first_order_channel_covers_fp32_first_moments():
    """The end-to-end gate: the fp64 sweep on fp32-rounded first moments against the all-fp64 pipeline."""
    for name in ("small", "ragged"):
        c = vx.case(name)
        n = 12
        a = (c.MU[:, :n], c.PIP[:, :n], c.LPOL[:, :n], c.VV[:, :n])
        exp64 = vx.reference(np.float64, c.tree, *a, c.hyper[:n])
        exp32 = vx.reference(np.float32, c.tree, *a, c.hyper[:n])
        ref = vm.reference(np.float64, c.tree, *a, c.hyper[:n], vm.first_of(np.float64, *a, exp64), first_gates=vx.gates(c.tree, exp64))
        got = vm.values_of(vm.reference(np.float64, c.tree, *a, c.hyper[:n], vm.first_of(np.float32, *a, exp32)))
        g = vm.gates(c.tree, ref, first_order=True)
        shares = vm.shares(ref, g, got)
        print(f"{name}: fp32 first moments use {shares} of the end-to-end gates")
        assert max(shares.values()) <= 0.5
        assert max(vm.shares(ref, vm.gates(c.tree, ref), got).values()) > max(shares.values()), "the channel is what admits them"


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_the_header_declares_the_two_entry_points():
    import ctypes as C

    import rnad_hip

    protos = rnad_hip.header_prototypes()
    assert protos["rnad_vtrace_moments_workspace"] == (C.c_int64, [C.c_int64, C.c_int, C.c_int])
    assert protos["rnad_vtrace_moments"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 14)


def test_the_library_exports_them_and_the_workspace_helper_answers():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_vtrace_moments is not None
    for S, n in ((2, 1), (283, 8), (2**33, 32), (283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        for A in (0, 1, 3, 8, 9):
            assert lib.rnad_vtrace_moments_workspace(S, A, n) == vm.workspace(S, A, n), (S, A, n)
    assert vm.workspace(283, 3, 8) == 283 * 8 * 4 and vm.workspace(1, 1, 1) == -1 and vm.workspace(5, 9, 1) == -1


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = vm.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    print({A: table[A] for A in sorted(table)})
    assert sorted(table) == list(range(1, 9)), "one k_vtrace_moments per A = 1 .. 8"
    assert all(k["scratch"] == 0 for k in table.values())
    assert all(k["lds"] == 4 * A * A * 8 * 3 * 4 for A, k in table.items()), "four waves' record slices, nothing else"


def test_null_arguments_and_a_cpu_tensor_are_refused_on_the_host():
    import torch

    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_vtrace_moments(None, 2, *([None] * 14)) != 0
    assert b"rnad_vtrace_moments" in lib.rnad_last_error()
    z = torch.zeros(22, 2, 4)
    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.vtrace_moments(None, [(0.2, 1.0, 1.0, 1.0, 1.0)] * 2, z, z, z, torch.zeros(22, 2, 2), torch.zeros(22 * 2 * 11),
                                torch.zeros(22, 2, 2), torch.zeros(22, 2, 2), z)
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.vtrace_moments(None, [(0.2, 1.0, 1.0, 1.0, 1.0)], torch.zeros(22, 4), torch.zeros(22, 4), torch.zeros(22, 4),
                                torch.zeros(22, 2), None, None, None, None)
