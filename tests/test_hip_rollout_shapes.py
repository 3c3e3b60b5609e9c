"""The seeded rollout kernels -- k_sample, k_transition, k_act (csrc/rollout.hip), pick / pick_n / transition_lane (csrc/rollout_math.hpp),
the keys walks with their decision word, k_bucket_rollout, rollout_items_body with its compact action word, k_bucket_indices,
k_bucket_expand, the staged sort and the one-launch rollout + learner (csrc/bucket.hip) -- against the plain numpy replay of
tests/_rolloutref.py on the same table, seed and lane0: at every A, C = 1 .. 8, on trees deep enough that lanes spend more than 10 env
steps above a cut and that windows of 20, 21, 22 and 30 steps are played.

Everything is compared BIT FOR BIT (floats as int32 views): under the randomness contract a decision is made of
integer operations and single fp32 operations, so there is no tolerance, and nothing is rejected at comparison time.  What the reference
stands on -- the replay against the C oracle, the edges the inputs reach, the mutants a comparison would catch -- is checked without a
GPU in tests/test_rollout_shapes.py.

  a. rnad_sample / rnad_transition seeded (n, C = 1 .. 8); rollout_begin -> rollout_step(policy=...) -> rollout_end and
     rollout_run_tabular (logits table: the policy head first) on every case;
  b. rollout_bucketed (dense): policy rows in three strides, a logits table, with and without a value table;
  c. rollout_bucketed_compact at T_cap = 2 * depth, 20 and 21: rnad_bucket_indices, acts, final_reward, alive, visited, deferred alive
     counts, rnad_bucket_expand;
  d. (b) and (c) under the switches that change which kernel or branch runs: RNAD_BUCKET_ROWS (bottom, middle, 300 on the wide tree:
     two-byte relative states), RNAD_KEYS_GLOBAL, the hybrid walk, RNAD_SORT_TILE, RNAD_BUCKET_CHUNK;
  e. bucket_sort + bucket_play, the second staging level, rollout_learn_bucketed_compact plain and distinct;
  f. the planner's refusals are pinned (none), a compact window of 22 steps is refused with the library's message.

RNAD_ERRORS_DIR, when set, receives rollout_shapes_gpu.json: the cut of every (case, batch, forced table) the sweep planned
(profiles/rollout_shapes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _learnref as lr
import _rolloutref as rr

pytestmark = pytest.mark.gpu

I32 = torch.int32
SEED, LANE0 = rr.SEED, rr.LANE0
TREE_KEYS = ("index", "value", "chance", "expected_value", "legal", "root_value", "solution")
SWITCHES = ("RNAD_BUCKET_ROWS", "RNAD_BUCKET_CHUNK", "RNAD_SORT_TILE", "RNAD_KEYS_GLOBAL", "RNAD_KEYS_LDS", "RNAD_KEYS_STAGE_BYTES", "RNAD_KEYS_HYBRID",
            "RNAD_FUSED_CHUNK", "RNAD_FUSED_DISTINCT")
BOTTOM = 2  # a table of two rows: every spine state with a spine state below it is an upper state
# (case, forced rows) that rnad_bucket_plan refuses at the sweep's batch sizes, with the reason: none.  Every forced table here has at
# most 300 rows and the trees have fewer than 5 000 states: the limits of cut_fits (12 288 buckets, 8 192 upper states, 32 path steps)
# and rows_max are not reached.
REFUSED = frozenset()
# (case, forced rows) whose relative states take two bytes: the forced table of 300 rows on the wide tree -- and the planner's OWN choice on
# three trees whose levels do not give a cut of single subtrees (choose_rows falls through to halving the LDS budget and stops above
# 255 rows): the default plan is not one byte everywhere.  Everywhere else: one byte.  The rule itself (rows > 255) is asserted too.
# (The planner's choice depends on the batch: the pin holds for the batch each tree is played at, _batch(name).)
TWO_BYTES = frozenset({(rr.WIDE, rr.WIDE_ROWS), (rr.WIDE, None), ("n3", None), ("n6", None)})
PLANNED = set()  # (case, rows) whose plan a test of this run asked for; test_the_planner_refuses_nothing_but_the_pinned_cases asks again


PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def _log_plans():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if PLANS and os.path.isdir(out):
        with open(os.path.join(out, "rollout_shapes_gpu.json"), "w") as f:
            json.dump(PLANS, f, indent=1, sort_keys=True)


def _hip():
    import rnad_hip

    return rnad_hip


def _new_tree(name):
    import _gpu as G

    t = rr.tree(name)
    return G.tree_from_arrays({k: t[k] for k in TREE_KEYS}, depth_bound=t["meta"]["depth"])


_tree = functools.lru_cache(maxsize=None)(_new_tree)


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(got, want, what):
    """Bit for bit; the message names the first differing (step, column)."""
    got, want = _bits(_np(got) if torch.is_tensor(got) else got), _bits(np.asarray(want))
    if got.dtype != want.dtype:
        got, want = got.astype(np.int64), want.astype(np.int64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want):
        at = tuple(int(i) for i in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} differ, first at {at}: got {got[at]}, want {want[at]}")


def _ref(name, T_cap, B, kind="spine", lane0=LANE0):
    full = rr.reference(name, T_cap, kind, rr.B_MAIN, lane0)
    return full if B == rr.B_MAIN else rr.prefix(full, B)


def _batch(name):
    return 3000 if rr.TREES.index(name) & 1 else 4096  # 3000: a ragged last workgroup


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _plan(name, h, B, rows, tag=""):
    """The plan of (tree, B) under the switches set; a refusal must be one of the pinned ones, and is then skipped by name."""
    plan = _hip().bucket_plan(h, B)
    PLANNED.add((name, rows))
    assert (plan is None) == ((name, rows) in REFUSED), f"{name}, rows {rows}: the planner's refusals are the pinned ones"
    if plan is None:
        pytest.skip(f"pinned refusal: {name} at a forced table of {rows} rows")
    assert plan.rel_bytes == (2 if plan.rows > 255 else 1) == (2 if (name, rows) in TWO_BYTES else 1), f"{name}, rows {rows}: {plan.rows} rows, {plan.rel_bytes} bytes"
    assert rows is None or plan.rows == rows
    PLANS[f"{name} B={B} forced={rows}" + (f" {tag}" if tag else "")] = dict(rows=plan.rows, groups=plan.n_groups, upper=plan.n_upper, buckets=plan.n_buckets,
                                                                            rel_bytes=plan.rel_bytes, sort_tile=plan.sort_tile, chunk=plan.chunk)
    return plan


def _record_shape(A):
    hip = _hip()
    return int(hip.lib().rnad_bucket_record_stride(A)), hip.policy_column(A)


def _dev(a, dtype=None):
    import _gpu as G

    return G.gpu(a, dtype)


# ------------------------------------------------------------------------------------------------ a. per-slot entry points
@pytest.mark.parametrize("n", range(1, 9))
def test_seeded_sample_on_adversarial_rows(n):
    import _numpy_rng as R

    hip = _hip()
    for B, lane0 in ((3000, LANE0), (257, rr.LANE0_WIDE)):
        p = R.adversarial_weights(np.random.default_rng([n, B]), B, n)
        probs = _dev(p)
        for step in (0, 1, 20, 31):
            for stream_id in (0, 1):
                got = hip.sample(probs, seed=SEED, lane0=lane0, step=step, stream_id=stream_id)
                _same(got, R.pick(p, R.slot_uniform(B, SEED, lane0, step, stream_id)), f"n={n} B={B} step={step} stream={stream_id}")


TREE_OF_C = {1: "s41_d6", 2: "n1", 3: "s33r_d8", 4: "n5", 5: "s75_d10", 6: "s26_d3", 7: "s27_d3", 8: "s88_d11"}


@pytest.mark.parametrize("C", range(1, 9))
def test_seeded_transition_at_every_outcome_count(C):
    import _numpy_rng as R

    hip = _hip()
    name = TREE_OF_C[C]
    t = rr.tree(name)
    S, Cc, A, _ = t["index"].shape
    assert Cc == C
    h = _tree(name).handle()
    for B, lane0 in ((3000, LANE0), (257, rr.LANE0_WIDE)):
        rng = np.random.default_rng([C, B])
        state, a0, a1 = rng.integers(0, S, B), rng.integers(0, A, B), rng.integers(0, A, B)
        if "spine" in t:  # half of the lanes in a spine state, most of them with the joint action that leads down
            state[: B // 2] = t["spine"][rng.integers(0, len(t["spine"]), B // 2)]
            a0[: B // 3], a1[: B // 3] = A - 1, A - 1
        alive = torch.zeros((1,), dtype=I32, device="cuda:0")
        nxt, rew = hip.transition(h, _dev(state, I32), _dev(a0, I32), _dev(a1, I32), seed=SEED, lane0=lane0, step=7, alive=alive)
        _, want_next, want_rew = rr.transition(t, state, a0, a1, R.decision_uniforms(B, SEED, lane0, 7)[:, 2])
        _same(nxt, want_next, f"C={C} next")
        _same(rew, want_rew, f"C={C} reward bits")
        assert int(alive.item()) == int((want_next != 0).sum())


def _check_lane_ordered(traj, ref, what):
    _same(traj.indices, ref["indices"], f"{what}: indices")
    _same(traj.actions, ref["actions"], f"{what}: actions")
    _same(traj.rewards, ref["rewards"], f"{what}: rewards (bits)")
    _same(traj.mask_bits, ref["mask_bits"], f"{what}: mask_bits")
    _same(traj.alive, ref["alive"], f"{what}: alive")
    _same(traj.policy, ref["policy"], f"{what}: policy")


@pytest.mark.parametrize("case", rr.cases(), ids=lambda c: f"{c[0]}_T{c[1]}")
def test_step_loop_with_policy_rows(case):
    """rollout_begin -> rollout_step(policy = the rows of the lanes' states, mode 1) -> rollout_end."""
    hip = _hip()
    name, T_cap = case
    B = _batch(name)
    h = _tree(name).handle()
    table = _dev(rr.policy_table(name))
    ref = _ref(name, T_cap, B)
    traj = hip.Trajectory(h, B, T_cap, "cuda:0")
    zeros = torch.zeros((B,), device="cuda:0")
    hip.rollout_begin(h, traj)
    for t in range(T_cap):
        rows = (t & 1) * h.S + traj.indices[t].long()
        hip.rollout_step(h, traj, t, zeros, policy=table[rows].contiguous(), seed=SEED, lane0=LANE0)
    hip.rollout_end(h, traj)
    _check_lane_ordered(traj, ref, f"{name} T={T_cap}")


def _logits_and_head(name):
    """A logits table and what rnad_policy_head gives for it under the rows' legal bits (device tensors, and the head on the host)."""
    hip = _hip()
    t = rr.tree(name)
    legal = rr.legal_rows(t)
    rng = np.random.default_rng([rr.TREES.index(name), 5])
    logits = (rng.standard_normal(legal.shape) * 1.5).astype(np.float32)
    if "spine" in t:  # the spine's action well ahead, so that lanes go deep
        S = len(legal) // 2
        logits[np.concatenate([t["spine"], S + t["spine"]]), -1] += np.float32(4.0)
    dev = _dev(logits)
    head = hip.policy_head(dev, mask_bits=_dev(lr.mask_bits(legal)))
    return dev, head, _np(head)


@pytest.mark.parametrize("name", rr.TREES)
def test_run_tabular_with_a_logits_table(name):
    hip = _hip()
    B = _batch(name)
    T_cap = 2 * rr.tree(name)["meta"]["depth"]
    h = _tree(name).handle()
    logits, head, table = _logits_and_head(name)
    ref = rr.replay(rr.tree(name), table, B, T_cap, SEED, LANE0)
    value = torch.arange(2 * h.S, device="cuda:0", dtype=torch.float32).view(-1, 1) * 0.5
    traj = hip.Trajectory(h, B, T_cap, "cuda:0")
    hip.rollout_run_tabular(h, traj, logits, value, seed=SEED, lane0=LANE0)
    rows = ((np.arange(T_cap) & 1)[:, None] * h.S + ref["indices"][:T_cap])
    _same(traj.policy, table[rows], f"{name}: the recorded policy is the head of the lane's row")
    _check_lane_ordered(traj, ref, name)
    _same(traj.values, rows.astype(np.float32) * np.float32(0.5), f"{name}: values")


# ------------------------------------------------------------------------------------------------ b. the dense bucketed rollout
def _check_order(name, tree, bk, ref, B, chunk=256):
    """lane_ids = the stable argsort of the restated keys; the work list tiles the sorted lanes bucket by bucket."""
    key, want_ids, n_groups = rr.order(tree, B, ref["indices"])
    assert n_groups == bk.plan.n_groups and key.max() < bk.plan.n_buckets
    _same(bk.lane_ids, want_ids, f"{name}: lane_ids")
    items = _np(bk.items)[: int(bk.n_items.item())]
    rr.check_work_items(items, key, want_ids, chunk)
    T = len(ref["alive"]) - 1
    _same(bk.norm, np.array([ref["alive"][0:T:2].sum(), ref["alive"][1:T:2].sum()], np.float64), f"{name}: norm")
    return key, want_ids, n_groups


def _dense(name, T_cap, B, rows, tree=None, forms=("A", "vec4", "record", "logits"), chunk=256, lane0=LANE0, kind="spine", tag=""):
    hip = _hip()
    tree = tree or _tree(name)
    h = tree.handle()
    _plan(name, h, B, rows, tag)
    A, S = h.A, h.S
    spine_ref = _ref(name, T_cap, B, kind, lane0)
    strides = dict(zip(("A", "vec4", "record"), rr.stride_variants(A, *_record_shape(A))))
    value = torch.arange(2 * S, device="cuda:0", dtype=torch.float32).view(-1, 1) * 0.25
    for n, form in enumerate(forms):
        what = f"{name} T={T_cap} B={B} rows={rows} {kind} {form}"
        traj = hip.Trajectory(h, B, T_cap, "cuda:0", with_observations=False)
        with_value = n % 2 == 0
        if form == "logits":
            logits, _, table = _logits_and_head(name)
            ref = rr.replay(rr.tree(name), table, B, T_cap, SEED, lane0)
            bk = hip.rollout_bucketed(h, traj, logits, value if with_value else None, seed=SEED, lane0=lane0)
        else:
            stride, column = strides[form]
            ref = spine_ref
            phys = _dev(rr.strided(rr.policy_table(name, kind), stride, column))
            bk = hip.rollout_bucketed(h, traj, phys, value if with_value else None, seed=SEED, lane0=lane0, table_is_policy=True, column=column)
        _, ids, _ = _check_order(what, tree, bk, ref, B, chunk)
        _same(traj.indices, ref["indices"][:, ids], f"{what}: indices")  # (row T_cap included)
        for k in ("actions", "mask_bits", "policy"):
            _same(getattr(traj, k), ref[k][:, ids], f"{what}: {k}")
        _same(traj.rewards, ref["rewards"][:, ids], f"{what}: rewards (bits)")
        _same(traj.alive, ref["alive"], f"{what}: alive")
        rows_of = ((np.arange(T_cap) & 1)[:, None] * S + ref["indices"][:T_cap, ids]).astype(np.float32)
        _same(traj.values, rows_of * np.float32(0.25) if with_value else np.zeros_like(rows_of), f"{what}: values")


@pytest.mark.parametrize("rows", (None, BOTTOM))
@pytest.mark.parametrize("name", rr.TREES)
def test_dense_bucketed_rollout_is_the_replay_in_bucket_order(name, rows, monkeypatch):
    _clear(monkeypatch)
    if rows is not None:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
    _dense(name, 2 * rr.tree(name)["meta"]["depth"], _batch(name), rows)


@pytest.mark.parametrize("B,lane0", ((1, LANE0), (257, LANE0), (3000, rr.LANE0_WIDE)))
def test_dense_bucketed_rollout_small_batches_and_a_lane_above_2_32(B, lane0, monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv("RNAD_BUCKET_ROWS", str(BOTTOM))
    _dense("s88_d11", 22, B, BOTTOM, forms=("vec4", "logits"), lane0=lane0)


def test_thirty_steps_above_a_cut_of_one_row(monkeypatch):
    """D = 15 under a table of ONE row: every group is a single subtree, its lanes share 30 env steps (28 above the cut and the group's
    root): inside kMaxPath = 32, three times the decision word."""
    _clear(monkeypatch)
    monkeypatch.setenv("RNAD_BUCKET_ROWS", "1")
    _dense("s28_d15", 30, 4096, 1, forms=("A", "vec4"))


# ------------------------------------------------------------------------------------------------ c. the compact rollout
def _records_like(name, kind="spine"):
    """A records-shaped table whose pi columns are the policy table (what rnad_bucket_expand reads), 3.0 everywhere else."""
    A = rr.tree(name)["meta"]["A"]
    stride, column = _record_shape(A)
    return _dev(rr.strided(rr.policy_table(name, kind), stride, column)), column


def _check_compact(what, tree, traj, bk, ref, B, chunk=256, visited=None):
    key, ids, n_groups = _check_order(what, tree, bk, ref, B, chunk)
    _same(traj.indices, ref["indices"][:, ids], f"{what}: rnad_bucket_indices")
    _same(traj.acts, ref["acts"][ids].view(np.int64), f"{what}: acts")
    _same(traj.final_reward, ref["final_reward"][ids], f"{what}: final_reward (bits)")
    _same(traj.alive, ref["alive"], f"{what}: alive")
    if visited is not None:
        _same(visited, ref["visited"], f"{what}: visited")
    return key, ids, n_groups


def _compact(name, T_cap, B, rows, tree=None, chunk=256, full=True, lane0=LANE0, kind="spine", tag=""):
    hip = _hip()
    tree = tree or _tree(name)
    h = tree.handle()
    _plan(name, h, B, rows, tag)
    A, S = h.A, h.S
    ref = _ref(name, T_cap, B, kind, lane0)
    rec, column = _records_like(name, kind)
    what = f"{name} T={T_cap} B={B} rows={rows} {kind}"
    traj = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    vis = torch.full((2 * S,), 7, dtype=I32, device="cuda:0")
    bk = hip.rollout_bucketed_compact(h, traj, rec, seed=SEED, lane0=lane0, table_is_policy=True, column=column, visited=vis)
    _, ids, _ = _check_compact(what, tree, traj, bk, ref, B, chunk, vis)
    # the dense buffers on demand
    hip.bucket_expand(h, traj, rec)
    live = ref["live"][:, ids]
    _same(traj.mask_bits, ref["mask_bits"][:, ids], f"{what}: expanded mask_bits")
    _same(traj.policy, ref["policy"][:, ids], f"{what}: expanded policy")
    _same(traj.actions, np.where(live, ref["actions"][:, ids], 0), f"{what}: expanded actions (0 on absorbed slots)")
    got_rew = _bits(_np(traj.rewards))
    assert np.array_equal(got_rew[live], _bits(ref["rewards"][:, ids])[live]), f"{what}: expanded rewards (bits) on live slots"
    assert (got_rew[~live] == 0).all(), f"{what}: +0.0 on absorbed slots"
    if not full:
        return
    # the alive counts left to a later launch
    late = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    late.alive.fill_(-1)
    bk2 = hip.rollout_bucketed_compact(h, late, rec, seed=SEED, lane0=lane0, table_is_policy=True, column=column, defer_alive=True)
    assert bk2.alive_pending is late
    hip.bucket_alive(h, bk2)
    assert bk2.alive_pending is None
    _same(late.alive, ref["alive"], f"{what}: deferred alive")
    assert torch.equal(bk2.norm, bk.norm) and torch.equal(late.acts, traj.acts) and torch.equal(bk2.lane_ids, bk.lane_ids)
    # the other two forms of the actor's table: rows of A floats, rows of a multiple of 4 floats (16-byte loads)
    for stride, col in rr.stride_variants(A, *_record_shape(A))[:2]:
        other = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
        bk3 = hip.rollout_bucketed_compact(h, other, _dev(rr.strided(rr.policy_table(name, kind), stride, col)), seed=SEED, lane0=lane0,
                                           table_is_policy=True, column=col)
        _check_compact(f"{what} stride {stride}", tree, other, bk3, ref, B, chunk)
    # ... and a logits table
    logits, _, table = _logits_and_head(name)
    ref_l = rr.replay(rr.tree(name), table, B, T_cap, SEED, lane0)
    other = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    bk4 = hip.rollout_bucketed_compact(h, other, logits, seed=SEED, lane0=lane0, table_is_policy=False)
    _check_compact(f"{what} logits", tree, other, bk4, ref_l, B, chunk)


COMPACT_CASES = [(n, T) for n, T in rr.cases() if T <= rr.COMPACT_MAX]


@pytest.mark.parametrize("rows", (None, BOTTOM))
@pytest.mark.parametrize("case", COMPACT_CASES, ids=lambda c: f"{c[0]}_T{c[1]}")
def test_compact_rollout_is_the_replay_in_bucket_order(case, rows, monkeypatch):
    _clear(monkeypatch)
    if rows is not None:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
    name, T_cap = case
    _compact(name, T_cap, _batch(name), rows)


@pytest.mark.parametrize("rows", (None, BOTTOM))
@pytest.mark.parametrize("name", rr.TREES)
def test_rollouts_on_adversarial_policy_rows(name, rows, monkeypatch):
    """pick<A> inside the rollouts on the rows rnad_sample is held to: exact zeros anywhere, sums near 1e-30 and 1e30, exact ties of a
    running sum with u * total, all mass on the last legal action -- dense (16-byte rows and rows of A floats) and compact."""
    _clear(monkeypatch)
    if rows is not None:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
    T_cap = 2 * rr.tree(name)["meta"]["depth"]
    B = _batch(name)
    _dense(name, T_cap, B, rows, forms=("vec4", "A"), kind="adversarial")
    if T_cap <= rr.COMPACT_MAX:
        _compact(name, T_cap, B, rows, full=False, kind="adversarial")


def test_compact_rollout_small_batches_and_a_lane_above_2_32(monkeypatch):
    """(T_cap = 20 and 21 on D = 10 are in COMPACT_CASES.)  The (8, 8) tree at 21 steps with B = 1, 257 and a lane offset above 2^32."""
    _clear(monkeypatch)
    monkeypatch.setenv("RNAD_BUCKET_ROWS", str(BOTTOM))
    for B, lane0 in ((1, LANE0), (257, LANE0), (3000, rr.LANE0_WIDE)):
        _compact("s88_d11", 21, B, BOTTOM, full=False, lane0=lane0)


# ------------------------------------------------------------------------------------------------ d. the switches
def _middle(name):
    """A table size between the bottom and the whole tree: the subtree of the spine's middle state / 8 rows on a native tree."""
    t = rr.tree(name)
    return int(t["index"].shape[0] - t["spine"][len(t["spine"]) // 2]) if "spine" in t else 8


def _hybrid(name, n_levels):
    """(budget, n_hot, n_upper) of the hybrid keys walk under the bottom cut with the top n_levels levels of upper states staged in LDS
    (None: half of the levels), restated on the host (tests/_rolloutref.hybrid_staging)."""
    t = rr.tree(name)
    if n_levels is None:
        n_levels = max(1, len(np.unique(rr.tree_levels(t)[rr.upper_states(t, BOTTOM)])) // 2)
    return rr.hybrid_staging(t, BOTTOM, n_levels)


VARIANTS = {
    "middle": lambda name: {"RNAD_BUCKET_ROWS": str(_middle(name))},
    "keys_global": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_KEYS_GLOBAL": "1"},
    "hybrid_top": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_KEYS_LDS": "0", "RNAD_KEYS_STAGE_BYTES": str(_hybrid(name, 1)[0])},
    "hybrid_half": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_KEYS_LDS": "0", "RNAD_KEYS_STAGE_BYTES": str(_hybrid(name, None)[0])},
    "tile_1024": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_SORT_TILE": "1024"},
    "tile_4096": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_SORT_TILE": "4096"},
    "chunk_64": lambda name: {"RNAD_BUCKET_ROWS": str(BOTTOM), "RNAD_BUCKET_CHUNK": "64"},
    "middle_keys_global": lambda name: {"RNAD_BUCKET_ROWS": str(_middle(name)), "RNAD_KEYS_GLOBAL": "1"},
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ("s88_d11", "n5", "s33r_d8"))
def test_kernel_and_branch_variants_play_the_replay(name, variant, monkeypatch):
    """Every switch meets the (8, 8) spine tree (10 upper states under the bottom cut, spine[0 .. 9]: 20 env steps above it, 22 shared
    by the lanes of the lone group of spine[10] -- the decision word holds 10), a native tree with ragged episode lengths and the tree
    with ragged legality; dense at 2 * depth, compact at min(2 * depth, 21).
    The hybrid walk runs only while 0 < n_hot < n_upper (choose_keys_walk): its LDS budget is sized per tree so that the top level
    (hybrid_top) or half of the levels (hybrid_half: the walk changes from the LDS tables to the global ones in the middle of the path,
    at A = 8, C = 8 after step 10) are staged and the next level does not fit; n_hot is restated on the host and asserted."""
    _clear(monkeypatch)
    env = VARIANTS[variant](name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rows = int(env["RNAD_BUCKET_ROWS"])
    tree = None
    if variant.startswith("hybrid"):
        budget, n_hot, n_upper = _hybrid(name, 1 if variant == "hybrid_top" else None)
        assert 0 < n_hot < n_upper and budget == int(env["RNAD_KEYS_STAGE_BYTES"]), f"{name}: {n_hot} of {n_upper} upper states staged: not the hybrid walk"
        assert variant == "hybrid_top" or name == "n5" or n_hot > 1
        tree = _new_tree(name)  # (the staged levels are chosen when the cut is built, and kept with it)
        bucket_of, n_groups = _hip().bucket_map(tree.handle(), 4096)
        np.testing.assert_array_equal(np.flatnonzero(bucket_of.numpy() >= n_groups), rr.upper_states(rr.tree(name), BOTTOM),
                                      err_msg="the upper states of the cut are the restated ones")
    chunk = int(env.get("RNAD_BUCKET_CHUNK", 256))
    depth = rr.tree(name)["meta"]["depth"]
    B = 3000 if variant in ("tile_1024", "keys_global") else 4096
    _dense(name, 2 * depth, B, rows, tree=tree, forms=("record", "logits"), chunk=chunk, tag=variant)
    _compact(name, min(2 * depth, 21), B, rows, tree=tree, chunk=chunk, full=False, tag=variant)


def test_two_byte_relative_states_on_the_wide_run(monkeypatch):
    """A forced table of 300 rows on the tree whose spine states have 280 one-state twigs: the run of siblings is ONE group (not one
    subtree: every lane keeps its own decision word), its relative states go beyond 255."""
    _clear(monkeypatch)
    monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rr.WIDE_ROWS))
    hip = _hip()
    h = _tree(rr.WIDE).handle()
    plan = hip.bucket_plan(h, 4096)
    assert plan is not None and plan.rel_bytes == 2 and plan.rows == rr.WIDE_ROWS
    traj = hip.Trajectory(h, 4096, 8, "cuda:0", compact=True)
    assert traj.states.dtype == torch.int16
    _compact(rr.WIDE, 8, 4096, rr.WIDE_ROWS)
    _dense(rr.WIDE, 8, 4096, rr.WIDE_ROWS, forms=("record",))
    monkeypatch.setenv("RNAD_KEYS_GLOBAL", "1")
    _compact(rr.WIDE, 8, 3000, rr.WIDE_ROWS, full=False)


# ------------------------------------------------------------------------------------------------ e. two calls, one launch
def _records(name):
    """bucket_records of a logits table whose head is sharp on the spine; the actor of the replay is the pi columns read back."""
    hip = _hip()
    h = _tree(name).handle()
    logits, _, _ = _logits_and_head(name)
    rng = np.random.default_rng([rr.TREES.index(name), 9])
    other = lambda cols: _dev((rng.standard_normal((2 * h.S, cols)) * 0.7).astype(np.float32))  # noqa: E731
    hp = hip.make_learn_params(alpha=0.3, eta=0.2, w_v=0.7, w_n=1.3)
    rec, fast = hip.bucket_records(h, logits, other(1), other(1), other(h.A), other(h.A), hp, fast=True)
    col = hip.policy_column(h.A)
    table = _np(rec[:, col: col + h.A]).copy()
    pol = rec._policy_rows
    _same(pol[:, : h.A], table, f"{name}: the policy rows are the pi columns of the records")
    return rec, fast, hp, table


TWO_CALL = (("s88_d11", 21), ("s75_d10", 20), ("s33r_d8", 16))


@pytest.mark.parametrize("rows", (None, BOTTOM, "middle"))
@pytest.mark.parametrize("case", TWO_CALL, ids=lambda c: f"{c[0]}_T{c[1]}")
def test_sort_then_play_and_the_staged_row_lists(case, rows, monkeypatch):
    _clear(monkeypatch)
    hip = _hip()
    name, T_cap = case
    rows = _middle(name) if rows == "middle" else rows
    if rows is not None:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
    B = _batch(name)
    tree = _tree(name)
    h = tree.handle()
    S, A = h.S, h.A
    _plan(name, h, B, rows)
    rec, fast, hp, table = _records(name)
    pol = rec._policy_rows
    ref = rr.replay(rr.tree(name), table, B, T_cap, SEED, LANE0)
    what = f"{name} T={T_cap} rows={rows}"
    # one call, for reference (c)
    one = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    bk1 = hip.rollout_bucketed_compact(h, one, rec, seed=SEED, lane0=LANE0)
    key, ids, n_groups = _check_compact(what + " one call", tree, one, bk1, ref, B)
    # sort, then play
    traj = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    vis = torch.full((2 * S,), 7, dtype=I32, device="cuda:0")
    bk, listed, flags = hip.bucket_sort(h, traj, pol, seed=SEED, lane0=LANE0, table_is_policy=True, want_flags=True, visited=vis)
    bucket_of = hip.bucket_map(h, B)[0].numpy()
    entered = np.isin(bucket_of, np.unique(key[key < n_groups])) & (bucket_of >= 0)
    want_flags = np.concatenate([entered, entered]).astype(np.int32)
    _same(flags, want_flags, f"{what}: group_flags")
    n = int(listed.count.item())
    assert set(_np(listed.rows[:n]).tolist()) == set(np.flatnonzero(want_flags).tolist()), f"{what}: staged_rows"
    hip.bucket_play(h, traj, bk, pol, seed=SEED, lane0=LANE0, table_is_policy=True, visited=vis, visited_is_clear=True)
    _check_compact(what + " sort + play", tree, traj, bk, ref, B, visited=vis)
    # the second staging level: the roots of the group subtrees the lanes enter, then the subtrees below the states they land in
    stage = hip.bucket_stage(h, B)
    assert stage is not None
    st = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
    bk_s, _, _ = hip.bucket_sort(h, st, pol, seed=SEED, lane0=LANE0, table_is_policy=True, want_rows=False, stage=stage)
    roots = hip.bucket_stage_rows(h, B, stage, 0, seed=SEED)
    n0 = int(roots.count.item())
    hip.bucket_stage_walk(h, st, bk_s, stage, pol, seed=SEED, lane0=LANE0)
    below = hip.bucket_stage_rows(h, B, stage, 1, seed=SEED)
    n1 = int(below.count.item())
    staged = set(_np(roots.rows[:n0]).tolist()) | set(_np(below.rows[:n1]).tolist())
    in_group = (bucket_of >= 0) & (bucket_of < n_groups)
    need = set(np.flatnonzero(ref["visited"] & np.concatenate([in_group, in_group])).tolist())
    assert need <= staged, f"{what}: {len(need - staged)} rows the replay visits below the cut are in neither staged list"
    hip.bucket_play(h, st, bk_s, pol, seed=SEED, lane0=LANE0, table_is_policy=True)
    _check_compact(what + " staged", tree, st, bk_s, ref, B)


@pytest.mark.parametrize("rows", (None, BOTTOM))
@pytest.mark.parametrize("case", TWO_CALL, ids=lambda c: f"{c[0]}_T{c[1]}")
def test_one_launch_rollout_and_learner_plays_the_replay(case, rows, monkeypatch):
    _clear(monkeypatch)
    hip = _hip()
    name, T_cap = case
    if rows is not None:
        monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
    B = _batch(name)
    tree = _tree(name)
    h = tree.handle()
    _plan(name, h, B, rows)
    rec, fast, hp, table = _records(name)
    ref = rr.replay(rr.tree(name), table, B, T_cap, SEED, LANE0)
    for distinct in (False, True):
        if distinct:
            monkeypatch.setenv("RNAD_FUSED_CHUNK", "512" if B == 3000 else "1024")
        what = f"{name} T={T_cap} rows={rows} distinct={distinct}"
        runs = []
        for _ in range(2):
            traj = hip.Trajectory(h, B, T_cap, "cuda:0", compact=True)
            bk, dlogit, dv = hip.rollout_learn_bucketed_compact(h, traj, rec, fast, hp, seed=SEED, lane0=LANE0, distinct=distinct)
            runs.append((traj, bk, dlogit, dv))
        traj, bk, dlogit, dv = runs[0]
        key, ids, _ = rr.order(tree, B, ref["indices"])
        _same(bk.lane_ids, ids, f"{what}: lane_ids")
        _same(traj.indices, ref["indices"][:, ids], f"{what}: states")
        _same(traj.acts, ref["acts"][ids].view(np.int64), f"{what}: acts")
        _same(traj.final_reward, ref["final_reward"][ids], f"{what}: final_reward (bits)")
        _same(traj.alive, ref["alive"], f"{what}: alive")
        _same(bk.norm, np.array([ref["alive"][0:T_cap:2].sum(), ref["alive"][1:T_cap:2].sum()], np.float64), f"{what}: norm")
        items = _np(bk.items)[: int(bk.n_items.item())]
        assert items[:, 1].sum() == B and np.array_equal(np.bincount(items[:, 2], weights=items[:, 1], minlength=bk.plan.n_buckets),
                                                         np.bincount(key, minlength=bk.plan.n_buckets))
        assert torch.isfinite(dlogit).all() and float(dlogit.abs().sum()) > 0
        assert torch.equal(dlogit.view(I32), runs[1][2].view(I32)) and torch.equal(dv.view(I32), runs[1][3].view(I32)), f"{what}: two runs differ"


# ------------------------------------------------------------------------------------------------ f. refusals
def test_a_compact_window_of_22_steps_is_refused_with_the_library_message(monkeypatch):
    """The four compact entry points of include/rnad_hip.h at T_cap = 22, called through the C ABI with the buffers of a valid 21-step
    batch (each refuses before it reads one of them), then through the binding: rnad_hip's own guards on three of them, the library's
    message on bucket_play, which has none."""
    import ctypes as C

    _clear(monkeypatch)
    hip = _hip()
    name = "s88_d11"
    h = _tree(name).handle()
    B = 256
    plan = _plan(name, h, B, None)
    rec, fast, hp, _ = _records(name)
    pol = rec._policy_rows
    traj = hip.Trajectory(h, B, 21, "cuda:0", compact=True)
    bk = hip.rollout_bucketed_compact(h, traj, rec, seed=SEED, lane0=LANE0)
    before = (traj.acts.clone(), traj.states.clone(), bk.lane_ids.clone())
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dlogit = torch.zeros((2 * h.S, h.A), device="cuda:0")
    dv = torch.zeros((2 * h.S, 1), device="cuda:0")
    actor = (ptr(pol), pol.shape[1])
    sort_out = (ptr(plan.scratch), ptr(bk.lane_ids), ptr(bk.items), ptr(bk.n_items), ptr(bk.norm))
    traj_out = (ptr(traj.states), ptr(traj.alive), ptr(traj.acts), ptr(traj.final_reward))
    lib = hip.lib()
    calls = {
        "rnad_rollout_bucketed_compact": lambda T: lib.rnad_rollout_bucketed_compact(h.ptr, T, B, *actor, 1, SEED, LANE0, None, *sort_out, *traj_out, None, stream),
        "rnad_bucket_sort": lambda T: lib.rnad_bucket_sort(h.ptr, T, B, *actor, 1, SEED, LANE0, None, *sort_out, None, None, None, None, None, None, stream),
        "rnad_bucket_play": lambda T: lib.rnad_bucket_play(h.ptr, T, B, *actor, 1, None, None, SEED, LANE0, None, *sort_out, *traj_out, None, 0, stream),
        "rnad_rollout_learn_bucketed_compact": lambda T: lib.rnad_rollout_learn_bucketed_compact(
            h.ptr, T, B, *actor, SEED, LANE0, None, *sort_out, *traj_out, None, 0, None, None, ptr(fast), C.byref(hp), ptr(plan.accumulators),
            hip.PLAY_LEARN_FINISH, None, ptr(dlogit), ptr(dv), None, None, None, None, stream),
    }
    for fn, call in calls.items():
        assert call(22) != 0, f"{fn} accepts a window of 22 steps"
        message = lib.rnad_last_error().decode()
        assert message.startswith(f"{fn}: 1 <= T_cap <= 21") and message.endswith("got 22"), message
    torch.cuda.synchronize()
    for x, y in zip(before, (traj.acts, traj.states, bk.lane_ids)):
        assert torch.equal(x, y), "a refused call leaves the batch as it was"
    # the binding
    long = hip.Trajectory(h, B, 22, "cuda:0", compact=True)
    with pytest.raises(AssertionError):
        hip.rollout_bucketed_compact(h, long, rec, seed=SEED, lane0=LANE0)
    with pytest.raises(AssertionError):
        hip.bucket_sort(h, long, pol, seed=SEED, lane0=LANE0, table_is_policy=True)
    with pytest.raises(AssertionError):
        hip.rollout_learn_bucketed_compact(h, long, rec, fast, hp, seed=SEED, lane0=LANE0)
    with pytest.raises(hip.RnadHipError, match=r"rnad_bucket_play: 1 <= T_cap <= 21, got 22"):
        hip.bucket_play(h, long, bk, pol, seed=SEED, lane0=LANE0, table_is_policy=True)


def test_the_planner_refuses_nothing_but_the_pinned_cases(monkeypatch):
    """Every (tree, forced table) of the sweep, asked again: the set of refusals is REFUSED (empty), so no comparison above was skipped.
    (REFUSED holding a case that alone carries an edge -- the (8, 8) tree under the bottom cut, the wide tree at 300 rows, the D = 15
    tree -- would take the edge out of the sweep: it must stay empty for those.)"""
    hip = _hip()
    _clear(monkeypatch)
    asked = {(n, r) for n in rr.TREES for r in (None, BOTTOM)} | {(n, _middle(n)) for n in ("s88_d11", "n5", "s33r_d8", "s75_d10")}
    asked |= {(rr.WIDE, rr.WIDE_ROWS), ("s28_d15", 1)} | PLANNED
    refused = set()
    for name, rows in sorted(asked, key=str):
        if rows is None:
            monkeypatch.delenv("RNAD_BUCKET_ROWS", raising=False)
        else:
            monkeypatch.setenv("RNAD_BUCKET_ROWS", str(rows))
        for B in (4096, 3000):
            if hip.bucket_plan(_tree(name).handle(), B) is None:
                refused.add((name, rows))
    assert refused == set(REFUSED)
    assert not {n for n, _ in REFUSED} & {"s88_d11", rr.WIDE, "s28_d15", "s75_d10", "s33r_d8"}
