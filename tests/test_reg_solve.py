"""The regularised-game solver without a GPU: the gates of tests/_regref.py are fixed here and the reference alone is shown to stay
inside them; four deliberately wrong programs are shown to leave them; the host half of the C ABI and the built kernels are checked.

  a. residual gate 2 * tol: the fp32 restatement of the shipped iteration stays <= 1.25 * tol (fp64 recomputation from its own outputs)
     with no unconverged state;
  b. value gate (A*A*C + 2A + 8) * 2^-24 * B[s]: the restatement stays within half of it;
  c. distance to the fp64 fixed point: the gate is twice the worst the restatement shows, computed here and written to
     reg_solve_errors.json in the directory RNAD_ERRORS_DIR names (profiles/reg_solve_errors.json holds a copy);
  d. the column player's sign not flipped, the magnet ignored, the opponent's KL term dropped from V, chance ignored: each exceeds
     twice gate (a) or (b) at the root or one level below;
  e. anchor: with mu = the tree's solution every state answers in 0 iterations with pi = mu and V = root_value, on every tree within
     the bound _regref.anchor_bound accumulates over the state's height, on the golden trees within the one-level gate (b) as well;
  f. refusals of the C entry point and of the binding; g. zero scratch in all eight instantiations of the built library.
"""
import ctypes
import os

import numpy as np
import pytest

import _regref as rr
from _util import TREES

MUTATION_TREES = TREES + ("native_a5",)


@pytest.mark.parametrize("eta", rr.ETAS)
@pytest.mark.parametrize("name", rr.ALL_TREES)
def test_fp32_restatement_stays_inside_gates_a_and_b(name, eta):
    for kind in rr.MAGNETS:
        reg, star, rest = rr.case(name, kind, eta)
        st = np.concatenate(rr.levels_of(name))
        assert rest["policy"].dtype == np.float32 and rest["values"].dtype == np.float32
        assert star["residual"][st].max() <= 1e-12, "the fp64 reference did not reach 1e-12"
        unconverged = int(((rest["iters"][st] >= rr.MAX_ITERS) & (rest["residual"][st] > rr.TOL)).sum())
        a, b = rr.shares(name, reg, eta, rest)
        print(f"{name} eta={eta} {kind}: residual {a:.3f} tol, value {b:.3f} of gate (b), at most {rest['iters'][st].max()} iterations")
        assert unconverged == 0
        assert a <= 1.25
        assert b <= 0.5


def test_gate_c_is_twice_the_restatements_worst_distance():
    gp, gv, at = rr.gate_c()
    print(f"gate (c): policy {gp:.3e} (worst at {at[0]}), value {gv:.3e} (worst at {at[1]})")
    assert 0 < gp < 1e-3 and 0 < gv < 1e-3, "the restatement itself is far from the fixed point"
    # the GPU tests read the gate from profiles/reg_solve_errors.json: the file says what is computed here (numpy's exp and log may
    # differ in the last bit between builds, which moves a state's last iteration, not the worst case by 2 %)
    fp, fv = rr.committed_gate_c()
    assert abs(fp - gp) <= 0.02 * gp and abs(fv - gv) <= 0.02 * gv, (fp, gp, fv, gv)
    figures = dict(policy_gate=gp, value_gate=gv, worst_policy_case=list(at[0]), worst_value_case=list(at[1]), cases={})
    for n, k, e in rr.cases():
        reg, star, rest = rr.case(n, k, e)
        a, b = rr.shares(n, reg, e, rest)
        dp, dv = rr.distance(n, rest, star)
        st = np.concatenate(rr.levels_of(n))
        figures["cases"][f"{n}/eta{e}/{k}"] = dict(residual_over_tol=a, gate_b_share=b, policy_distance=dp, value_distance=dv,
                                                  max_iters=int(rest["iters"][st].max()))
    rr.update_errors_file("fp32_restatement", figures)


# c1 has one outcome per joint action (C = 1, chance = 1): there is no chance factor to drop
@pytest.mark.parametrize("name,variant", [(t, v) for t in MUTATION_TREES for v in rr.VARIANTS if not (t == "c1" and v == "no_chance")])
def test_wrong_programs_leave_the_gates_near_the_root(name, variant):
    eta = 0.2
    reg = rr.magnet(name, "softmax", eta)
    out = rr.solve(name, reg, eta, np.float32, max_iters=512, variant=variant)
    c = rr.check(name, reg, eta, out)
    top = np.concatenate(rr.levels_of(name)[:2])
    a = float(c["res64"][top].max() / (2 * rr.TOL))
    b = float((np.abs(out["values"][top].astype(np.float64) - c["v64"][top]) / c["gate_b"][top]).max())
    print(f"{name} {variant}: {a:.1f} gates (a), {b:.1f} gates (b) at the root or one level below")
    assert max(a, b) > 2.0


@pytest.mark.parametrize("name", rr.ALL_TREES)
def test_anchor_the_solution_is_its_own_fixed_point(name):
    tree = rr.tree_arrays(name)
    st = np.concatenate(rr.levels_of(name))
    for eta in rr.ETAS:
        reg, star, rest = rr.case(name, "solution", eta)
        c = rr.check(name, reg, eta, rest)
        assert (rest["iters"][st] == 0).all()
        dp = float(np.abs(rest["policy"][st].astype(np.float64) - np.asarray(tree["solution"], np.float64)[st]).max())
        dv = np.abs(rest["values"][st].astype(np.float64) - np.asarray(tree["root_value"], np.float64)[st, 0])
        print(f"{name} eta={eta}: |pi - mu| {dp:.1e}, |V - root_value| {dv.max():.1e}")
        assert dp <= 8 * rr.U  # exp(log mu - logsumexp): an absolute error of a few 2^-24 |log pi| in the exponent, pi |log pi| <= 1 / e
        # on every tree within the bound accumulated over the state's height (rr.anchor_bound); on the golden trees within the one-level
        # gate (b) as well
        bound = rr.anchor_bound(name, eta, rest)
        print(f"{name} eta={eta}: at most {float((dv / bound[st]).max()):.3f} of the anchor bound (root: {bound[1]:.1e})")
        assert (dv <= bound[st]).all()
        if name in TREES:
            assert (dv <= c["gate_b"][st]).all()


def test_host_refusals():
    import rnad_hip

    lib = rnad_hip.lib()
    bufs = [np.zeros(64, np.float32) for _ in range(7)]
    tree, reg, lp, pol, val, res, it = (ctypes.c_void_p(b.ctypes.data) for b in bufs)  # never dereferenced: every call is refused first
    for eta, tol, iters, word in ((0.0, 1e-5, 10, b"eta"), (-0.2, 1e-5, 10, b"eta"), (0.2, 0.0, 10, b"tol"), (0.2, -1e-5, 10, b"tol"),
                                  (0.2, 1e-5, 0, b"max_iters")):
        assert lib.rnad_reg_solve(tree, eta, tol, iters, reg, lp, pol, val, res, it, None) != 0
        assert word in lib.rnad_last_error(), lib.rnad_last_error()
    for k in range(7):
        args = [tree, reg, lp, pol, val, res, it]
        args[k] = None
        assert lib.rnad_reg_solve(args[0], 0.2, 1e-5, 10, *args[1:], None) != 0
        assert b"null" in lib.rnad_last_error()
    for k in range(2, 7):
        args = [tree, reg, lp, pol, val, res, it]
        args[k] = reg
        assert lib.rnad_reg_solve(args[0], 0.2, 1e-5, 10, *args[1:], None) != 0
        assert b"aliases" in lib.rnad_last_error()


def test_binding_refuses_a_cpu_tensor():
    import torch

    import rnad_hip

    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.reg_solve(None, 0.2, torch.zeros(22, 4))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, 2A\]"):
        rnad_hip.reg_solve(None, 0.2, torch.zeros(22, 2, 4))


def test_every_instantiation_is_free_of_scratch():
    import rnad_hip

    meta = rr.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    assert sorted(meta) == list(range(1, 9)), f"k_reg_solve instantiations found: {sorted(meta)}"
    for A, m in sorted(meta.items()):
        print(f"A={A}: {m}")
    assert all(m["scratch"] == 0 for m in meta.values()), meta
