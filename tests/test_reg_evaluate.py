"""Exact evaluation in the regularised game without a GPU: the reference and gates of tests/_regevalref.py are pinned by what the
quantities must satisfy, not by a measurement --

  - every input of the GPU sweep is absolutely continuous with respect to its magnet (a condition, asserted at every state);
  - with log_reg = log pi both KL terms vanish and values[:, k] is the fp64 cross-play recursion's V[s, k, k];
  - at _regref.solve's fp64 fixed point the residual is at most 1e-10, values equals its V and the advantage vanishes on the support;
  - the telescoping identity values[1, k] = sum_s reach[s, k] * (imm[s, k] - eta KL_row + eta KL_col);
  - reach is _brref.reference's, bit for bit, in fp64 and in the fp32 restatement;
  - the fp32 restatement in the kernel's order stays within half of every gate on every input (the reach on the generated trees comes to
    0.50 of its gate, as tests/test_best_response.py records for the same sweep, so there the gate itself is asked);
  - eight natural mistakes land beyond twice some gate;

and the host half of the C ABI is checked: the header, the exports, the scratch of the eight instantiations.
"""
import os

import numpy as np
import pytest

import _crossref as cr
import _regevalref as rv
import _regref as rr
from _util import TREES

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CPU_TREES = TREES + ("native_a5",)


@pytest.mark.parametrize("name", rv.ALL_TREES)
def test_every_input_is_absolutely_continuous(name):
    J, L, etas = rv.inputs(name)
    tree = rr.tree_arrays(name)
    support = rv.legal_mask(tree)[:, None, :] & (L > -np.inf)
    assert not ((J > 0) & ~support).any(), "a policy puts mass where its magnet has none"
    assert (etas > 0).all() and J.shape[1] == 32 and np.isfinite(J).all() and not np.isnan(L).any() and (L < np.inf).all()
    reached = np.concatenate(rv.levels_of(name))
    A = J.shape[2] // 2
    sides = J[reached].reshape(len(reached), 32, 2, A).sum(axis=3)
    has = support[reached].reshape(len(reached), 32, 2, A).any(axis=3)
    assert (np.abs(sides - 1)[has] <= 4 * A * rv.U).all(), "every side with a support is a distribution"
    one_hot = J[reached][:, 3]  # member 3 plays the one-hot table: zeros inside the support, the select's case
    assert ((one_hot == 0) & support[reached][:, 3]).any() or A == 1


@pytest.mark.parametrize("name", CPU_TREES)
def test_without_kl_the_value_is_cross_play_of_the_policy_with_itself(name):
    tree = cr.tree_arrays(name)
    J = cr.players(tree, 4, 0, cr.fixture_policy(name)).astype(np.float64)
    with np.errstate(divide="ignore"):
        L = np.where(J > 0, np.log(np.where(J > 0, J, 1.0)), -np.inf)
    ref = rv.reference(tree, J, L, [1.0, 0.2, 0.05, 0.2])
    assert (ref.KL == 0).all()
    V, B, h = cr.reference(tree, J)
    R = ref.depth >= 0
    k = np.arange(4)
    err = np.abs(ref.V[R] - V[R][:, k, k])
    print(f"{name}: values against V[s, k, k] to {err.max():.3g}")
    assert (err <= 1e-12 * np.maximum(B[R][:, k, k], ref.Bv[R])).all()
    assert (err <= 1e-12 * B[R][:, k, k]).all()


FIXED_POINTS = [("small", "uniform", 0.2), ("small", "after4", 0.05), ("ragged", "solution", 1.0), ("c1", "softmax", 0.2),
                ("a5", "after4", 1.0), ("native_a5", "softmax", 0.05), ("gen_a8c1", "uniform", 0.05)]


@pytest.mark.parametrize("name,kind,eta", FIXED_POINTS)
def test_at_the_fp64_fixed_point(name, kind, eta):
    tree, lm, star = rr.tree_arrays(name), rr.magnet(name, kind, eta), rr.star(name, kind, eta)
    ref = rv.reference(tree, star["policy"][:, None, :], lm[:, None, :], [eta], round_eta=False)
    R = ref.depth >= 0
    sup, pi = ref.on[:, 0] & R[:, None], star["policy"]  # (rows the sweep never reaches hold log_policy = -inf)
    A = sup.shape[1] // 2
    assert ref.RES[R].max() <= 1e-10
    assert (np.abs(ref.V[R, 0] - star["values"][R]) <= 1e-10 * ref.Bv[R, 0]).all()
    # the advantage, with the solver's own log-policy.  The solver stops on a residual in probability space, so an action of probability
    # e^-40 is converged to 1e-12 in probability and to nothing in its logarithm: the statement that holds is the pi-weighted one
    lp = np.where(sup, star["log_policy"], 0.0)
    raw = np.where(sup, ref.Q[:, 0] - eta * (lp - np.where(sup, lm, 0.0)), 0.0)
    mean = np.concatenate([np.repeat((pi[:, :A] * raw[:, :A]).sum(1, keepdims=True), A, 1),
                           np.repeat((pi[:, A:] * raw[:, A:]).sum(1, keepdims=True), A, 1)], axis=1)
    adv = np.where(sup, raw - mean, 0.0)
    print(f"{name} {kind} eta={eta}: residual {ref.RES[R].max():.3g}, pi * advantage {np.abs(pi * adv)[R].max():.3g}")
    assert (np.abs(pi * adv)[R] <= 1e-10).all()
    assert (np.abs(adv)[R][pi[R] >= 1e-3] <= 1e-7).all()


@pytest.mark.parametrize("name", CPU_TREES)
def test_telescoping_identity(name):
    c = rv.case(name)
    ref = c.ref
    eta = c.etas.astype(np.float64)[None, :]
    local = ref.imm - eta * ref.KL[:, :, 0] + eta * ref.KL[:, :, 1]
    total = (np.asarray(ref.R, np.float64) * local).sum(axis=0)
    print(f"{name}: root value against the sum over states to {(np.abs(total - ref.V[1]) / ref.Bv[1]).max():.3g} of B[1]")
    assert (np.abs(total - ref.V[1]) <= 1e-12 * ref.Bv[1]).all()


@pytest.mark.parametrize("name", CPU_TREES)
def test_reach_is_the_best_response_sweeps(name):
    c = rv.case(name)
    assert np.array_equal(c.ref.R, rv.br.reference(c.tree, c.J).R)
    n = 5
    got = rv.reference(c.tree, c.J[:, :n], c.L[:, :n], c.etas[:n], dtype=np.float32)
    assert np.array_equal(got.R, rv.br.reference(c.tree, c.J[:, :n], dtype=np.float32).R)


@pytest.mark.parametrize("name", rv.ALL_TREES)
def test_fp32_restatement_stays_within_half_the_gates(name):
    c = rv.case(name)
    got = rv.reference(c.tree, c.J, c.L, c.etas, dtype=np.float32)
    shares = rv.shares(c, got)
    print(f"{name}: fp32 restatement uses {shares} of the gates")
    assert max(shares["values"], shares["q"], shares["residual"]) <= 0.5
    assert shares["reach"] <= (0.5 if name in TREES else 1.0)
    for a in (got.V, got.Q, got.RES, got.R):
        assert (a[~c.reached] == 0).all()
    # a slice of the members is the case of fewer members: they do not see each other
    few = rv.reference(c.tree, c.J[:, :3], c.L[:, :3], c.etas[:3], dtype=np.float32)
    assert np.array_equal(few.V, got.V[:, :3]) and np.array_equal(few.RES, got.RES[:, :3]) and np.array_equal(few.R, got.R[:, :3])


BEYOND = dict(col_kl_sign=("values",), reverse_kl=("values",), no_opp_kl=("values",), q_own_side=("q", "values"), no_chance_q=("q", "values"),
              reach_no_chance=("reach",), log_residual=("residual",), log_underflow=("values",))
MUTATIONS = [(t, v) for t in CPU_TREES for v in rv.VARIANTS if not (t == "c1" and v in ("no_chance_q", "reach_no_chance"))]
# (c1 has one chance outcome per joint action: chance is 1 there)


@pytest.mark.parametrize("name,variant", MUTATIONS)
def test_mutations_exceed_twice_a_gate(name, variant):
    c = rv.case(name)
    got = rv.reference(c.tree, c.J, c.L, c.etas, variant=variant)
    shares = rv.shares(c, got)
    print(f"{name} {variant}: {shares} gates off")
    for key in BEYOND[variant]:
        assert shares[key] > 2.0
    if variant == "reach_no_chance":
        assert shares["values"] == 0.0
    else:
        assert shares["reach"] == 0.0


def test_the_neurd_loop_contracts_in_fp64():
    hist, floor, first = rv.neurd_loop()
    print(f"max residual {first:.3g} -> {hist[-1]:.3g} after {len(hist)} steps; the residual gate there is {floor:.3g}")
    assert len(hist) == rv.NEURD["steps"] and rv.NEURD["lr"] * rv.NEURD["eta"] < 1 and floor < hist[-1]


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_the_header_declares_both_entry_points():
    import ctypes as C

    import rnad_hip

    protos = rnad_hip.header_prototypes()
    assert protos["rnad_reg_evaluate_size"] == (C.c_int64, [C.c_int64, C.c_int])
    assert protos["rnad_reg_evaluate"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8)


def test_the_library_exports_both_and_the_size_companion_answers():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_reg_evaluate is not None
    for S, n in ((2, 1), (283, 8), (2**33, 32), (283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_reg_evaluate_size(S, n) == rv.size(S, n), (S, n)
    assert rv.size(283, 8) == 283 * 8 and rv.size(1, 1) == -1 and rv.size(283, 33) == -1


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = rv.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    print({A: table[A] for A in sorted(table)})
    assert sorted(table) == list(range(1, 9)), "one k_reg_evaluate per A = 1 .. 8"
    assert all(k["scratch"] == 0 for k in table.values())
    assert all(k["lds"] == 4 * A * A * 8 * 3 * 4 for A, k in table.items()), "four waves' record slices, nothing else"


def test_null_arguments_and_a_cpu_tensor_are_refused_on_the_host():
    import torch

    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_reg_evaluate(None, 2, None, None, None, None, None, None, None, None) != 0
    assert b"rnad_reg_evaluate" in lib.rnad_last_error()
    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.reg_evaluate(None, 0.2, torch.zeros(22, 2, 4), torch.zeros(22, 2, 4))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.reg_evaluate(None, 0.2, torch.zeros(22, 4), torch.zeros(22, 4))
