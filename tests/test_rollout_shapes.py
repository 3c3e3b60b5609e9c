"""What the GPU sweep of the rollout kernels (tests/test_hip_rollout_shapes.py) stands on, checked without a GPU.

1. The reference is right.  tests/_rolloutref.replay agrees exactly, on every case, with the C oracle's step functions
   (oracle.uniforms, oracle.pick, oracle.transition with a 1-D uniform) chained the same way: two independent restatements of the seeded
   rollout.  Every spine tree is what it promises: an increasing index, one parent per state, every subtree an id range, chance rows that
   sum to 1, exact zeros among them that the replay never takes.
2. The inputs reach the edges: assertions on the reference alone (caps, not measurements) at B = 4096, seed 21, lane0 77 -- lanes alive
   after 10 transitions and at step 30, action 7 and outcome 7 (and other values) before and after step 10 above the bottom cut, lanes
   leaving the tree at every level, -0.0 rewards, negative payoffs, every action and outcome, ragged legality, a relative state above 255.
3. A wrong program would show: eight mutants of the replay each change a compared output on at least one case.
4. The library's constants are the ones the cases were sized for.

RNAD_ERRORS_DIR, when set, receives rollout_shapes_cpu.json: per case S, depth and the edge counts (profiles/rollout_shapes.md)."""
import json
import os

import numpy as np
import pytest

import _learnref as lr
import _rolloutref as rr

B, SEED, LANE0 = rr.B_MAIN, rr.SEED, rr.LANE0
COUNTS = {}


@pytest.fixture(scope="module", autouse=True)
def _log_counts():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if COUNTS and os.path.isdir(out):
        with open(os.path.join(out, "rollout_shapes_cpu.json"), "w") as f:
            json.dump(COUNTS, f, indent=1, sort_keys=True)


def _id(case):
    return f"{case[0]}_T{case[1]}"


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the reference is right
@pytest.mark.parametrize("case", rr.cases() + [("s88_d11", 22, rr.LANE0_WIDE), ("n3", 8, rr.LANE0_WIDE)], ids=lambda c: _id(c) + ("_wide" if len(c) > 2 else ""))
def test_replay_is_the_chain_of_the_oracle_step_functions(case):
    from oracle import oracle

    name, T_cap = case[:2]
    lane0 = case[2] if len(case) > 2 else LANE0
    t = rr.tree(name)
    table = rr.policy_table(name)
    S = t["index"].shape[0]
    ref = rr.reference(name, T_cap, lane0=lane0)
    state = np.ones(B, np.int64)
    row_a = u = None
    for step in range(T_cap):
        if step % 2 == 0:
            u = oracle.uniforms(B, SEED, lane0, step)
        np.testing.assert_array_equal(ref["indices"][step], state, err_msg=f"state, step {step}")
        a = oracle.pick(table[(step & 1) * S + state], np.ascontiguousarray(u[:, step & 1]))
        np.testing.assert_array_equal(ref["actions"][step], a, err_msg=f"action, step {step}")
        if step & 1:
            state, rew = oracle.transition(t["index"], t["chance"], t["value"], state, row_a, a, np.ascontiguousarray(u[:, 2]))
            np.testing.assert_array_equal(_bits(ref["rewards"][step]), _bits(rew), err_msg=f"reward bits, step {step}")
        else:
            row_a = a
            assert (_bits(ref["rewards"][step]) == 0).all(), "a row step pays +0.0"
    np.testing.assert_array_equal(ref["indices"][T_cap], state)


@pytest.mark.parametrize("kind", ("spine", "adversarial"))
@pytest.mark.parametrize("name", rr.TREES)
def test_policy_tables_are_zero_on_illegal_actions_and_not_normalised(name, kind):
    p = rr.policy_table(name, kind)
    legal = rr.legal_rows(rr.tree(name))
    assert p.dtype == np.float32 and p.shape == legal.shape
    assert (p[legal == 0] == 0).all() and (p.sum(-1) > 0).all() and np.isfinite(p).all()
    assert (np.abs(p.sum(-1) - 1) > 1e-3).any()
    S = len(p) // 2
    assert not np.array_equal(p[:S], p[S:]) or p.shape[1] == 1, "the two players' rows of a state differ"


@pytest.mark.parametrize("name", sorted(rr.SPINE))
def test_spine_trees_keep_their_promises(name):
    t = rr.tree(name)
    index, chance, value = t["index"], t["chance"], t["value"]
    S, C, A, _ = index.shape
    m = t["meta"]
    assert rr.tree_depth(t) == m["D"] == m["depth"] and S <= 5000
    kids_of = [np.sort(index[s][(index[s] != 0) & (chance[s] > 0)]) for s in range(S)]
    assert not (index[(chance == 0)] != 0).any(), "an entry without chance leads nowhere"
    parents = np.zeros(S, np.int64)
    for s in range(1, S):
        assert (kids_of[s] > s).all(), "increasing index"
        np.add.at(parents, kids_of[s], 1)
    assert (parents[2:] == 1).all() and parents[1] == 0 and len(kids_of[0]) == 0, "one parent per state, the root has none"
    size = np.ones(S, np.int64)
    for s in range(S - 1, 0, -1):
        size[s] += size[kids_of[s]].sum()
        hi = max([s + 1] + [int(k + size[k]) for k in kids_of[s]])
        assert hi - s == size[s], "every subtree is an id range"
    np.testing.assert_allclose(chance[1:].astype(np.float64).sum(1), 1.0, atol=2e-7)
    if C >= 3 and name != rr.WIDE:
        assert ((chance[1:] == 0).sum(1) >= 1).all(), "every joint action has an outcome of probability 0"
    spine = t["spine"]
    np.testing.assert_array_equal(index[spine, C - 1, A - 1, A - 1], np.concatenate([spine[1:], [0]]))
    twig = np.setdiff1d(np.arange(1, S), spine)
    assert (index[twig] == 0).all(), "a twig's transitions are terminal"
    for s in spine[:-1]:
        np.testing.assert_array_equal(kids_of[s], np.arange(s + 1, s + 2 + m["twigs"]), err_msg="twigs first, as consecutive ids, then the spine")
    live = chance > 0
    assert (value[live & (index == 0)] > 0).any() and (value[live & (index == 0)] < 0).any()
    assert (value[live & (index != 0)] < 0).any(), "negative entries on non-terminal transitions"
    # the replay never takes an outcome of probability 0
    for T_cap in rr.windows(name):
        ref = rr.reference(name, T_cap)
        odd = np.arange(1, T_cap, 2)
        st, c, a0, a1 = ref["indices"][odd], ref["outcomes"][odd], ref["actions"][odd - 1], ref["actions"][odd]
        on = st != 0
        assert (chance[st[on], c[on], a0[on], a1[on]] > 0).all()


# ------------------------------------------------------------------------------------------------ 2. the inputs reach the edges
def _level_exits(ref, T_cap):
    idx = ref["indices"]
    return [int(((idx[2 * d + 1] != 0) & (idx[2 * d + 2] == 0)).sum()) for d in range(T_cap // 2)]


@pytest.mark.parametrize("case", rr.cases(), ids=_id)
def test_every_case_draws_every_action_and_outcome_and_both_zeros(case):
    name, T_cap = case
    t = rr.tree(name)
    S, C, A, _ = t["index"].shape
    ref = rr.reference(name, T_cap)
    live = ref["live"]
    acts = np.bincount(ref["actions"][live], minlength=A)
    odd = np.arange(1, T_cap, 2)
    outs = np.bincount(ref["outcomes"][odd][live[odd]], minlength=C)
    assert (acts > 0).all(), f"actions drawn: {acts}"
    assert (outs > 0).all(), f"outcomes drawn: {outs}"
    exits = _level_exits(ref, T_cap)
    depth = t["meta"]["depth"]
    rew = ref["rewards"][live]
    minus_zero = int(((rew == 0) & np.signbit(rew)).sum())
    negative = int((ref["final_reward"] < 0).sum())
    COUNTS[_id(case)] = dict(S=int(S), A=int(A), C=int(C), depth=depth, alive=[int(x) for x in ref["alive"]], exits_per_level=exits,
                             minus_zero_rewards=minus_zero, negative_payoffs=negative, min_action_count=int(acts.min()),
                             min_outcome_count=int(outs.min()))
    if T_cap >= 2 * depth:
        assert ref["alive"][T_cap] == 0
    if name in rr.SPINE:
        assert all(n > 0 for n in exits[: min(depth, T_cap // 2)]), f"lanes leave the tree at every level: {exits}"
        assert minus_zero > 0, "a non-terminal transition with a negative value: its dense reward is -0.0"
        assert negative > 0 and (ref["final_reward"] > 0).any()
        # every lane's one non-zero reward is its final one
        assert ((ref["rewards"] != 0).sum(0) <= 1).all()


def test_lanes_are_alive_after_ten_transitions_and_at_step_thirty():
    for name in rr.DEEP:
        ref = rr.reference(name, 2 * rr.tree(name)["meta"]["depth"])
        assert ref["alive"][20] >= 64, f"{name}: {ref['alive'][20]} lanes after transition 10"
    assert rr.reference("s88_d11", 21)["alive"][21] >= 64, "a compact window of 21 steps cuts live lanes off"
    assert rr.reference("s75_d10", 21)["alive"][19] >= 64 and rr.reference("s75_d10", 21)["alive"][20] == 0, "D = 10: 20 live steps in a window of 21"
    assert rr.reference("s28_d15", 30)["alive"][29] >= 32, "lanes alive at the last step of the 30-step window"
    COUNTS["alive_after_10_transitions"] = {n: int(rr.reference(n, 2 * rr.tree(n)["meta"]["depth"])["alive"][20]) for n in rr.DEEP}
    COUNTS["alive_at_step_29_d15"] = int(rr.reference("s28_d15", 30)["alive"][29])


def test_the_top_bit_of_both_fields_of_the_decision_word_is_drawn_and_not_drawn():
    """A = 8, C = 8: action 7 and outcome 7, and other values, at a step < 10 and at a step >= 10 while the lane is in a state above the
    bottom cut (a spine state that has a spine state below it: its subtree is larger than any table of 2 or 4 rows)."""
    t = rr.tree("s88_d11")
    ref = rr.reference("s88_d11", 22)
    upper = np.isin(ref["indices"][:22], t["spine"][:-1])
    counts = {}
    for lo, hi, tag in ((0, 10, "packed"), (10, 22, "redrawn")):
        steps = np.arange(lo, hi)
        odd = steps[steps % 2 == 1]
        a, c = ref["actions"][steps][upper[steps]], ref["outcomes"][odd][upper[odd]]
        counts[tag] = dict(action_7=int((a == 7).sum()), action_other=int((a != 7).sum()), outcome_7=int((c == 7).sum()),
                           outcome_other=int((c != 7).sum()))
        assert all(v > 0 for v in counts[tag].values()), (tag, counts[tag])
        for bit in range(3):  # every bit of both fields is seen set and clear
            assert ((a >> bit) & 1).any() and (~(a >> bit) & 1).any() and ((c >> bit) & 1).any() and (~(c >> bit) & 1).any()
    # the compact word: an action with its top bit set at step 20 (bits 60 .. 62)
    ref21 = rr.reference("s88_d11", 21)
    step20 = ref21["actions"][20][ref21["live"][20]]
    assert (step20 == 7).any() and (step20 != 7).any() and (ref21["acts"] >> np.uint64(62)).any()
    counts["step_20"] = dict(action_7=int((step20 == 7).sum()), action_other=int((step20 != 7).sum()))
    COUNTS["decision_word_s88_d11"] = counts


def test_ragged_legality_is_respected_and_its_edge_rows_are_visited():
    name = "s33r_d8"
    t = rr.tree(name)
    legal = rr.legal_rows(t)
    S, A = len(legal) // 2, legal.shape[1]
    ref = rr.reference(name, 16)
    live = ref["live"]
    rows = ((np.arange(16) & 1)[:, None] * S + ref["indices"][:16])
    assert (legal[rows[live], ref["actions"][live]] == 1).all(), "no illegal action is drawn"
    seen = legal[np.unique(rows[live])]
    only_last = (seen[:, A - 1] == 1) & (seen.sum(1) == 1)
    only_first = (seen[:, 0] == 1) & (seen.sum(1) == 1)
    assert only_last.any() and only_first.any()
    assert len(np.unique(lr.mask_bits(seen))) >= 4, "several different masks are visited"
    COUNTS["ragged_rows_visited"] = dict(only_last=int(only_last.sum()), only_first=int(only_first.sum()))


def test_the_wide_run_of_twigs_is_visited_beyond_one_byte():
    t = rr.tree(rr.WIDE)
    ref = rr.reference(rr.WIDE, 8)
    first_twig = t["spine"][0] + 1  # the run below the root: 280 one-state subtrees with consecutive ids
    rel = ref["indices"][2] - first_twig + 1  # the relative state k_bucket_rollout_items stores: state - lo + 1
    in_run = (ref["indices"][2] >= first_twig) & (ref["indices"][2] < t["spine"][1])
    assert t["meta"]["twigs"] == 280 and (rel[in_run] > 255).sum() >= 8 and (rel[in_run] <= 255).sum() >= 8
    COUNTS["wide_relative_states"] = dict(above_255=int((rel[in_run] > 255).sum()), up_to_255=int((rel[in_run] <= 255).sum()))


# ------------------------------------------------------------------------------------------------ 3. a wrong program would show
@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_every_mutant_of_the_replay_changes_a_compared_output(mutant):
    found = {}
    for name, T_cap in rr.cases():
        bad = rr.replay(rr.tree(name), rr.policy_table(name), B, T_cap, SEED, LANE0, mutate=mutant)
        d = rr.differs(rr.reference(name, T_cap), bad)
        if d:
            found[f"{name}_T{T_cap}"] = d
    COUNTS.setdefault("mutants", {})[mutant] = sorted(found)
    assert found, f"{mutant}: no case of the sweep tells this program from the right one"
    if mutant == "outcome_2bits":
        assert any(rr.tree(n.rsplit("_T", 1)[0])["meta"]["C"] >= 5 for n in found)
    if mutant in ("shift32", "no_lone_step"):
        assert all(n.endswith("_T21") for n in found), "only a window of 21 steps reaches step 20 / ends on a lone row step"
    if mutant == "plus_zero":
        assert all(d == ["rewards"] for d in found.values()), "only the dense rewards carry the sign of a zero"


# ------------------------------------------------------------------------------------------------ 4. the library's constants
def test_the_library_constants_are_the_ones_the_cases_were_sized_for():
    import re

    import rnad_hip  # (host side only: the library loads without a device)

    assert rnad_hip.MAX_ACTIONS == 8 and rnad_hip.MAX_TRANSITIONS == 8 and rnad_hip.COMPACT_MAX_STEPS == rr.COMPACT_MAX == 21
    root = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    header = open(os.path.join(root, "include", "rnad_hip.h")).read()
    assert re.search(r"#define\s+RNAD_MAX_ACTIONS\s+8\b", header) and re.search(r"#define\s+RNAD_MAX_TRANSITIONS\s+8\b", header)
    bucket = open(os.path.join(root, "r-nad_amd", "csrc", "bucket.hip")).read()
    for name, want in (("kPackedSteps", 10), ("kCompactSteps", 21), ("kMaxPath", 32)):
        assert re.search(rf"constexpr int {name} = {want};", bucket), name
    assert max(A for A in (rr.tree(n)["meta"]["A"] for n in rr.TREES)) == 8 and max(rr.tree(n)["meta"]["C"] for n in rr.TREES) == 8
    assert {rr.tree(n)["meta"]["A"] for n in rr.TREES} == set(range(1, 9)) and {rr.tree(n)["meta"]["C"] for n in rr.TREES} == set(range(1, 9))
    assert all(T <= 21 or n in ("s88_d11", "s28_d15") for n, T in rr.cases())
