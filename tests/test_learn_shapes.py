"""What the GPU sweep of the learner kernels (tests/test_hip_learn_shapes.py) stands on, checked without a GPU.

1. Anchor.  tests/_learnref.learner in fp64 on the five recorded learner batches of the reference (tests/golden/learn_*.npz) reproduces
   their pi_processed exactly and their v_target, q, dlogit, dv and losses at the tolerances tests/test_oracle_golden.py holds the oracle
   to: the reference of the sweep is tied to the reference project's numbers before it judges a kernel.
2. Gate.  On every case of the sweep -- the dense batches at A = 1 .. 8 under the four hyperparameter sets, and the tree batches -- two
   fp32 programs stay within HALF of K 2^-24 mag per output family: learner(np.float32) and the composition of the oracle's C
   restatements.  K (tests/_learnref.K) is the smallest power of two that is at least twice their worst share; their shares go to
   learn_errors_cpu.json in RNAD_ERRORS_DIR.  No row is redrawn or rejected at comparison time: every decision margin is >= MARGIN.
3. Mutants.  Nine wrong fp32 programs each exceed TWICE the gate on at least one case of these inputs.
4. Coverage.  The fp64 reference alone shows that the inputs reach what the sweep is for: importance weights on both sides of rho and c,
   a clip that binds, closed gates, actions dropped below eps, the all-below-eps branch, an exhausted leftover, a zero normaliser,
   illegal actions.  At A = 1 pi = mu = 1 and l = 0 in every row, so the conditions on w and on the gates are stated for A >= 2; they
   hold in every case with T >= 7, the one-lane batches included (tests/_learnref.dense_case draws those until they do).
5. The fixed-point units of the two row-sum paths, restated in tests/_learnref.py, are 2^(40 - e) units per 1.0."""
import functools
import json
import os

import numpy as np
import pytest

import _learnref as lr
from _util import load, load_tree, mlp_weights

CPU = {}  # case -> {program/output: share of 2^-24 mag}
OUTPUTS = ("pi", "v_target", "q", "dlogit", "dv", "losses")


@pytest.fixture(scope="module", autouse=True)
def _log_cpu_figures():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if CPU and os.path.isdir(out):
        with open(os.path.join(out, "learn_errors_cpu.json"), "w") as f:
            json.dump(CPU, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def native_tree(A):
    import rnad_hip  # (the generator is host code: the library loads without a device)

    kw = dict(lr.TREES[A])
    out = rnad_hip.tree_generate(kw.pop("A"), kw.pop("C"), kw.pop("depth_bound"), **kw)
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def tree_case(key):
    """(batch, tables) of a tree case; key = (A, set) or ("ragged", set): the golden tree with ragged legality."""
    A, s = key
    if A == "ragged":
        tree, B, seed = load_tree("ragged"), 3000, 99
    else:
        tree, B, seed = native_tree(A), lr.TREE_B[A], A
    return lr.tree_batch(np.random.default_rng([seed, lr.SETS.index(s)]), tree, B, lr.HP[s])


@functools.lru_cache(maxsize=None)
def tree_reference(key):
    batch, tables = tree_case(key)
    return lr.learner(np.float64, batch, tables, lr.HP[key[1]])


TREE_CASES = lr.tree_cases() + [("ragged", s) for s in lr.SETS]
ALL = [("dense", k) for k in lr.dense_cases()] + [("tree", k) for k in TREE_CASES]


def _id(c):
    return lr.case_id(c[1]) if c[0] == "dense" else f"tree_A{c[1][0]}_{c[1][1]}"


def _case(c):
    kind, key = c
    batch, slots = lr.dense_case(key) if kind == "dense" else tree_case(key)
    ref = lr.dense_reference(key) if kind == "dense" else tree_reference(key)
    return batch, slots, ref, lr.HP[key[1]]


def oracle_program(batch, slots, hp):
    """The oracle's fp32 C restatement composed as tests/test_hip_parity.py composes the single kernels:
    policy_head -> process_policy -> vtrace x 2 -> loss_v / loss_nerd."""
    from oracle import oracle

    idx = batch["indices"]
    T, B = idx.shape
    A = batch["mu"].shape[-1]
    turn = np.broadcast_to((np.arange(T) & 1)[:, None], (T, B)).astype(np.int64)
    if "S" in batch:
        rows = turn * batch["S"] + idx
        slots = {k: np.asarray(v)[rows] for k, v in slots.items()}
    legal = batch["legal"]
    pi, logp = oracle.policy_head(slots["logit"], legal)
    _, logr = oracle.policy_head(slots["logit_reg"], legal)
    _, logr_ = oracle.policy_head(slots["logit_reg_"], legal)
    lpol = logp - (np.float32(hp.alpha) * logr + np.float32(hp.one_minus_alpha) * logr_)
    pip = oracle.process_policy(pi, legal, hp.n_disc, hp.eps)
    valid = (idx != 0).astype(np.float32)
    a_oh = np.eye(A, dtype=np.float32)[batch["actions"]]
    vtn = slots["v_target"].reshape(T, B, 1)
    vt, q, has = [], [], []
    for p in range(2):
        rew = batch["rewards"] if p == 0 else -batch["rewards"]
        a, h, b = oracle.vtrace(vtn, valid, turn, batch["mu"], pip, lpol, a_oh, rew, p, eta=hp.eta, lambda_=hp.lambda_, c=hp.c, rho=hp.rho,
                                gamma=hp.gamma)
        vt.append(a.reshape(T, B)), q.append(b), has.append(h)
    v = slots["v"].reshape(T, B)
    lv, dv = oracle.loss_v(v, vt[0], vt[1], has[0], has[1], scale=hp.w_v)
    ln, dl = oracle.loss_nerd(slots["logit"], pip, q[0], q[1], valid, turn, legal, hp.clip, hp.threshold, scale=hp.w_n)
    return dict(pi=pi, pi_processed=pip, v_target=np.stack(vt), q=np.stack(q), dlogit=dl, dv=dv, losses=np.array([lv, ln]))


def _tables_of(ref, batch, dlogit, dv):
    """Per-row sums of per-slot gradients, added in fp64 (tests/_learnref.learner does the same for its own)."""
    S, A = batch["S"], dlogit.shape[-1]
    rows = ref.turn * S + batch["indices"]
    tl, tv = np.zeros((2 * S, A)), np.zeros(2 * S)
    np.add.at(tl, rows[ref.valid], np.asarray(dlogit, np.float64)[ref.valid])
    np.add.at(tv, rows[ref.valid], np.asarray(dv, np.float64).reshape(rows.shape)[ref.valid])
    return tl, tv


def _shares(ref, got, batch):
    s = {n: lr.share(got[n], getattr(ref, n)) for n in OUTPUTS}
    if "S" in batch:
        tl, tv = got["tables"] if "tables" in got else _tables_of(ref, batch, got["dlogit"], got["dv"])
        s["tables"] = max(lr.share(tl, ref.dlogit_tab), lr.share(tv, ref.dv_tab))
    return s


def _family(name):
    return name if name in lr.K else "tables"


# ------------------------------------------------------------------------------------------------ 1. anchor
LEARN = ("c1_eta0.2", "small_eta0", "small_eta0.2", "ragged_eta0.5", "a5_eta0.2")
TOL = 1e-5


def _net(g, tag, obs, A):
    """The MLP of nn/net.py:71-73 in fp64 -> logits."""
    w = [x.astype(np.float64) for x in mlp_weights(g, f"w_{tag}_")]
    x = obs.reshape(-1, 2 * A * A).astype(np.float64)
    return (np.maximum(x @ w[4].T + w[5], 0) @ w[6].T + w[7]).reshape(obs.shape[:2] + (A,))


@pytest.mark.parametrize("name", LEARN)
def test_the_reference_reproduces_the_recorded_learner_batches(name):
    g = load("learn_" + name)
    ro = load("rollout_" + name.split("_")[0])
    A = ro["policy"].shape[-1]
    T, B = g["valid"].shape
    hp = lr._hp(alpha=float(g["alpha"]), eta=float(g["eta"]), lambda_=1.0, c=float(g.get("hp_c_bar", 1.0)), rho=float(g.get("hp_roh_bar", 1.0)),
                gamma=float(g.get("hp_vtrace_gamma", 1.0)), clip=float(g.get("hp_neurd_clip", 1e3)), threshold=float(g.get("hp_beta", 2.0)))
    batch = dict(indices=ro["indices"], legal=ro["masks"], actions=ro["actions"].argmax(-1), rewards=ro["rewards"], mu=ro["policy"])
    slots = dict(logit=g["logit"], v=g["v"].reshape(T, B), v_target=g["v_target_net"].reshape(T, B), logit_reg=_net(g, "reg", ro["observations"], A),
                 logit_reg_=_net(g, "reg_", ro["observations"], A))
    assert np.array_equal(g["valid"], ro["indices"] != 0) and np.array_equal(ro["turns"], np.broadcast_to((np.arange(T) & 1)[:, None], (T, B)))
    ref = lr.learner(np.float64, batch, slots, hp)
    assert np.array_equal(ref.pi_processed.v, g["pi_processed"].astype(np.float64)), "pi_processed is exact"
    np.testing.assert_allclose(ref.pi.v, g["pi"], rtol=TOL, atol=1e-7)
    for p in range(2):
        np.testing.assert_array_equal(ref.valid & (ref.turn == p), g[f"has_played_p{p}"] != 0)
        np.testing.assert_allclose(ref.v_target.v[p], g[f"v_target_p{p}"][..., 0], rtol=TOL, atol=TOL)
        np.testing.assert_allclose(ref.q.v[p], g[f"q_p{p}"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(ref.losses.v[0], g["loss_v"], rtol=TOL)
    np.testing.assert_allclose(ref.losses.v[1], g["loss_nerd"], rtol=TOL, atol=1e-7)
    np.testing.assert_allclose(ref.dv.v, g["dv"][..., 0], rtol=TOL, atol=1e-8)
    np.testing.assert_allclose(ref.dlogit.v, g["dlogit"], rtol=TOL, atol=1e-8)


# ------------------------------------------------------------------------------------------------ 2. the gate
def test_the_case_lists_are_what_the_sweep_says():
    dense = lr.dense_cases()
    assert len(dense) == 8 * 4 * 16 and {k[0] for k in dense} == set(range(1, 9)) and {k[1] for k in dense} == {"H0", "H1", "H2", "H3"}
    assert {(k[2], k[3]) for k in dense} == {(T, B) for T in (1, 2, 7, 32) for B in (1, 255, 257, 1023)}, "the whole cross"
    for k in dense:  # no empty batch: the first lane has all T steps, so both players move whenever T >= 2
        v = lr.dense_case(k)[0]["indices"] != 0
        assert v[0::2].any() and (k[2] < 2 or v[1::2].any()), k
    assert any(k[3] > 256 for k in dense), "more than one 256-thread workgroup"
    assert sorted(lr.TREES) == list(range(1, 9)) and set(lr.TREE_B.values()) == {3000, 4096}
    for A in lr.TREES:
        t = native_tree(A)
        assert t["index"].shape[-1] == A and 2 <= t["index"].shape[0] <= lr.MAX_STATES
    assert any(lr.TREES[A]["C"] == 4 for A in lr.TREES)
    h0 = lr.HP["H0"]  # learn/rnad.py:41-71 and lambda_ = 1.0 (:397)
    assert (h0.eta, h0.lambda_, h0.c, h0.rho, h0.gamma, h0.clip, h0.threshold, h0.eps, h0.n_disc) == (np.float32(0.2), 1, 1, 1, 1, 1e3, 2, np.float32(0.03), 32)
    assert lr.HP["H2"].c > lr.HP["H2"].rho and lr.HP["H3"].clip == 2.0 ** 30


@functools.lru_cache(maxsize=None)
def _figures(case):
    """program/output -> the worst share of 2^-24 mag on one case, for both fp32 programs (kept: the K test below reads every case's)."""
    batch, slots, ref, hp = _case(case)
    assert (ref.margin >= lr.MARGIN).all(), "a row below the decision margin: nothing is redrawn at comparison time"
    f32 = lr.learner(np.float32, batch, slots, hp)
    got = {n: getattr(f32, n).v for n in OUTPUTS + ("pi_processed",)}
    if "S" in batch:
        got["tables"] = (f32.dlogit_tab.v, f32.dv_tab.v)
    figures = {}
    for program, out in (("numpy", got), ("oracle", oracle_program(batch, slots, hp))):
        assert np.array_equal(np.asarray(out["pi_processed"], np.float64).reshape(ref.pi_processed.v.shape), ref.pi_processed.v), \
            f"{program}: pi_processed is not the reference's"
        for name, s in _shares(ref, out, batch).items():
            figures[f"{program}/{name}"] = round(s, 3)
    CPU[_id(case)] = figures
    return figures


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_two_fp32_programs_use_at_most_half_of_the_gate(case):
    figures = _figures(case)
    print(_id(case), figures)
    over = {k: v for k, v in figures.items() if not v <= lr.K[_family(k.split("/")[1])] / 2}
    assert not over, f"an fp32 program beyond half of the gate (units of 2^-24 mag): {over}"


def test_K_is_the_smallest_power_of_two_at_twice_the_worst_share():
    """K is neither looser nor tighter than the rule, over the figures of EVERY case (computed here where the sweep above has not)."""
    every = [_figures(c) for c in ALL]
    for fam in lr.FAMILIES:
        worst = max(v for f in every for k, v in f.items() if _family(k.split("/")[1]) == fam)
        assert lr.K[fam] / 2 >= worst > lr.K[fam] / 4, (fam, worst, lr.K[fam])


# ------------------------------------------------------------------------------------------------ 3. mutants
@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_a_wrong_program_exceeds_twice_the_gate(mutant):
    cases = [c for c in ALL if c[0] == "tree"] if mutant == "row_slot" else ALL
    order = sorted(cases, key=lambda c: (c[1][1] != "H1", c[0] == "dense" and c[1][2] != 7))  # the off-unit set first
    for case in order:
        batch, slots, ref, hp = _case(case)
        m = lr.learner(np.float32, batch, slots, hp, mutate=mutant)
        got = {n: getattr(m, n).v for n in OUTPUTS}
        if "S" in batch:
            got["tables"] = (m.dlogit_tab.v, m.dv_tab.v)
        worst = max(s / lr.K[_family(n)] for n, s in _shares(ref, got, batch).items())
        if worst > 2:
            print(mutant, _id(case), "->", round(worst, 1), "gates")
            return
    pytest.fail(f"{mutant}: within twice the gate on every case -- the inputs are too tame")


# ------------------------------------------------------------------------------------------------ 4. coverage
@pytest.mark.parametrize("key", [k for k in lr.dense_cases() if k[2] >= 7 and k[0] >= 2], ids=lr.case_id)
def test_weights_straddle_rho_and_c_and_under_H1_the_clip_binds_and_each_gate_closes(key):
    """Every case with T >= 7, a single lane included: at least 5 % of the mover's slots have w on each side of rho and of c; under H1
    the clip binds on at least 5 % of the legal actions and each gate is closed on at least 5 %."""
    batch, slots = lr.dense_case(key)
    cov = lr.coverage(batch, slots, lr.HP[key[1]], lr.dense_reference(key))
    assert lr.covered(key, cov), (key, cov)


def test_process_policy_takes_every_branch():
    dropped = rows = 0
    exhausted = False
    below = {A: 0 for A in range(6, 9)}
    illegal = {A: False for A in range(2, 9)}
    for key in lr.dense_cases():
        A, s = key[0], key[1]
        batch, _ = lr.dense_case(key)
        ref, hp = lr.dense_reference(key), lr.HP[s]
        pi, pip, on = ref.pi.v.reshape(-1, A), ref.pi_processed.v.reshape(-1, A), batch["legal"].reshape(-1, A) > 0
        all_below = (pi.max(-1) < hp.eps)
        if A >= 2:
            rows += len(pi)
            dropped += int(((on & (pi < hp.eps)).any(-1) & ~all_below).sum())
        if s == "H2" and A >= 6:
            below[A] += int(all_below.sum())
        # an action that survives the threshold and still gets nothing: the leftover ran out before its rank
        survives = on & ((pi >= hp.eps) | all_below[:, None])
        exhausted |= bool((survives & (pip == 0)).any())
        assert (batch["legal"].sum(-1) >= 1).all()
        if A >= 2 and len(pi) > 100:
            illegal[A] |= bool((batch["legal"] == 0).any(-1).mean() >= 0.05)
    assert dropped >= 0.05 * rows, (dropped, rows)
    assert all(n >= 1 for n in below.values()), below
    assert exhausted
    assert all(illegal.values()), "every A >= 2 has rows with an illegal action"


def test_one_step_batches_give_player_1_a_zero_normaliser():
    for key in (k for k in lr.dense_cases() if k[2] == 1):
        ref = lr.dense_reference(key)
        assert not (ref.valid & (ref.turn == 1)).any() and ref.norm[1] == 1 and ref.norm[0] == max(1, ref.valid.sum())
    lengths = {int(n) for k in lr.dense_cases() if k[2] == 7 for n in (lr.dense_case(k)[0]["indices"] != 0).sum(0)}
    assert lengths >= set(range(0, 8)), "lanes of every length 0 .. T"
    b, _ = lr.dense_case((3, "H1", 32, 257))
    v = b["indices"] != 0
    assert (v[2:] & ~v[1:-1] & v[:-2].any(0)).any(), "a lane with an invalid slot in the middle"


# ------------------------------------------------------------------------------------------------ 5. fixed-point units
def test_the_fixed_point_units_are_the_sources():
    """csrc/bucket.hip fixed_point_for: 2^(40 - e_l) units of dL/dlogit per 1.0 with 2^e_l the first power of two above 2 clip (at most
    2^30), 2^(40 - 11) of dL/dv; csrc/learn.hip k_row_sums: 2^40 units per column maximum rounded up to a power of two."""
    want = {"H0": (11, False), "H1": (1, False), "H2": (11, False), "H3": (30, True)}  # 2 * 1e3 < 2^11; 2 * 0.5 = 1 < 2^1; 2 * 2^30 does not fit
    for s, (e_l, check) in want.items():
        assert lr.bucketed_exponents(lr.HP[s]) == (e_l, 11, check), s
        ul, uv = lr.bucketed_units(lr.HP[s])
        assert 1 / ul == 2.0 ** (40 - e_l) and 1 / uv == 2.0 ** (40 - 11)
    assert lr.bucketed_units(lr.HP["H3"])[0] == 2.0 ** -10, "one unit of dL/dlogit under the check_l instantiation"
    for mx, e in ((1.0, 1), (0.75, 0), (1.5, 1), (2.0 ** -20, -19), (3e-4, -11)):
        assert lr.row_sums_unit(mx) == 2.0 ** (e - 40) and mx < 2.0 ** e
    assert lr.row_sums_unit(0.0) == 1.0
