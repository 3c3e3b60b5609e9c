"""Trees, policy tables and the exact replay of the rollout sweep (csrc/rollout.hip, csrc/rollout_math.hpp, the rollout half of
csrc/bucket.hip) -- tests/test_rollout_shapes.py on the CPU, tests/test_hip_rollout_shapes.py on the GPU.  numpy only; nothing here calls
a project kernel (`native_tree` runs the host-side generator, `order` asks the library for the cut it chose).

Under the randomness contract every decision of a seeded rollout is a function of (seed, global lane, env step) and
the actor's policy row, made of integer operations and single fp32 operations.  `replay` restates environment/episode.py:96-125 with
those draws in plain numpy, so every state, action, outcome and reward of a kernel can be compared bit for bit: there is no tolerance
anywhere in the sweep.

`spine_tree` builds by hand what the native generator cannot: a thin DEEP tree (one spine state per level, twigs beside it) at any
A, C <= 8, so that lanes spend more than 10 env steps above a cut (the decision word of the keys walk holds 10), windows of 20 / 21 / 22 /
30 steps exist, action 7 and outcome 7 are drawn, chance rows have exact zeros and fewer than 8 entries, `value` is negative on
non-terminal transitions (their dense reward is -0.0) and a run of sibling one-state subtrees is longer than 255 states."""
import functools

import numpy as np

import _learnref as lr
import _numpy_rng as rng_ref

SEED, LANE0, B_MAIN = 21, 77, 4096
LANE0_WIDE = (1 << 32) + 12345  # a global lane above 2^32: the counter's second word is not zero
P_SPINE = 0.93  # weight of action A - 1 in a spine row of the "spine" policy
P_DOWN = 0.9  # chance of outcome C - 1 (C > 1)


# ------------------------------------------------------------------------------------------------ trees
def _chance_rows(rng, n, C, k_min=1, p_last=P_DOWN):
    """[n, C] fp32: p_last on outcome C - 1, the rest spread over a random subset of k_min .. C - 2 other outcomes, so that with
    C >= 3 at least one outcome of every row has probability exactly 0 (k_min = C - 1: every outcome is used).  Rows sum to 1 up to
    the rounding of their entries to fp32."""
    if C == 1:
        return np.ones((n, 1), np.float32)
    out = np.zeros((n, C), np.float64)
    for i in range(n):
        k = C - 1 if k_min >= C - 1 else rng.integers(k_min, max(C - 2, 1) + 1)
        used = rng.choice(np.arange(C - 1), size=k, replace=False)
        out[i, used] = rng.dirichlet(np.ones(k)) * (1.0 - p_last)
        out[i, C - 1] = p_last
    return out.astype(np.float32)


def spine_tree(A, C, D, twigs, seed, ragged=False):
    """The seven reference-layout arrays (index int64, value / chance fp32 [S, C, A, A], expected_value / legal fp32 [S, 1, A, A],
    root_value [S, 1], solution [S, 2A]) of a spine tree, plus "spine" (the ids of the spine states) and "meta".

    State 0 absorbs, the spine state of level d = 0 .. D - 1 is followed by its twigs (consecutive ids, DFS pre-order), then by the next
    spine state.  Joint action (A - 1, A - 1) with outcome C - 1 leads down the spine, from the last spine state out of the tree.
    `twigs` other (outcome, a0, a1) entries with positive chance of every spine state but the last lead to twig states, whose entries
    are all terminal; the rest are terminal.  (The last spine state has no twigs, so that the depth of the tree is D.)
    value: uniform in [-1, 1] on every entry with positive chance, non-terminal ones included; the entry down the spine is negative
    at even levels.  ragged: legal masks that differ per player and state, among them twig rows with only the last action legal and
    with only the first; the spine's rows keep action A - 1 legal.
    expected_value / root_value / solution are consistent with each other under the uniform policy over the legal actions (not an
    equilibrium: nothing in the rollout reads them beyond the observation table)."""
    rng = np.random.default_rng([A, C, D, twigs, seed])
    assert twigs <= A * A * C - 2, "a spine state needs the entry down the spine and a terminal one"
    S = 1 + D + (D - 1) * twigs
    index = np.zeros((S, C, A, A), np.int64)
    value = np.zeros((S, C, A, A), np.float32)
    chance = np.zeros((S, C, A, A), np.float32)
    legal = np.zeros((S, 1, A, A), np.float32)
    chance[0, 0] = 1.0  # the absorbing state: one outcome, back to itself, value 0
    legal[0, 0, 0, 0] = 1.0
    spine = np.array([1 + d * (1 + twigs) for d in range(D)], np.int64)
    is_spine = np.zeros(S, bool)
    is_spine[spine] = True
    k_min = -(-(twigs + 1) // (A * A))  # other outcomes per joint action that the twigs and one terminal entry need
    for s in range(1, S):
        chance[s] = _chance_rows(rng, A * A, C, k_min if is_spine[s] else 1).T.reshape(C, A, A)
    on = chance[1:] > 0
    value[1:][on] = rng.uniform(-1.0, 1.0, int(on.sum())).astype(np.float32)
    for d, s in enumerate(spine):
        nxt = spine[d + 1] if d + 1 < D else 0
        index[s, C - 1, A - 1, A - 1] = nxt
        if nxt and d % 2 == 0:
            value[s, C - 1, A - 1, A - 1] = -np.abs(value[s, C - 1, A - 1, A - 1]) - np.float32(0.125)
        if d + 1 < D:
            cand = np.argwhere(chance[s] > 0)
            cand = cand[~((cand[:, 0] == C - 1) & (cand[:, 1] == A - 1) & (cand[:, 2] == A - 1))]
            assert len(cand) > twigs, "not enough entries with positive chance for the twigs and a terminal one"
            # in random order: the entries the batch takes often (an action A - 1 in them) lie all along the run of twig ids
            for k, (c, a0, a1) in enumerate(cand[rng.permutation(len(cand))[:twigs]]):
                index[s, c, a0, a1] = s + 1 + k
    # legality: the row player's mask is legal[s, 0, :, 0], the column player's legal[s, 0, 0, :] (episode.py:62-68): they share [0, 0]
    row_ok = np.ones((S, A), bool)
    col_ok = np.ones((S, A), bool)
    if ragged:
        assert A >= 2
        for s in range(1, S):
            kind = rng.integers(0, 5) if not is_spine[s] else 4
            if kind == 0:  # only the last action, both players
                row_ok[s] = col_ok[s] = np.arange(A) == A - 1
            elif kind == 1:  # only the first
                row_ok[s] = col_ok[s] = np.arange(A) == 0
            elif kind == 4:  # a random subset that keeps A - 1 (the spine) -- action 0 is shared by the two masks
                first = rng.random() < 0.5
                row_ok[s] = rng.random(A) < 0.6
                col_ok[s] = rng.random(A) < 0.6
                row_ok[s, 0] = col_ok[s, 0] = first
                row_ok[s, A - 1] = col_ok[s, A - 1] = True
    row_ok[0] = col_ok[0] = np.arange(A) == 0
    legal[:, 0] = (row_ok[:, :, None] & col_ok[:, None, :]).astype(np.float32)
    legal[:, 0, :, 0] = row_ok
    legal[:, 0, 0, :] = col_ok
    # values under the uniform policy over the legal actions, children first (ids are increasing)
    root_value = np.zeros((S, 1), np.float32)
    ev = np.zeros((S, 1, A, A), np.float32)
    solution = np.zeros((S, 2 * A), np.float32)
    solution[:, :A] = row_ok / row_ok.sum(1, keepdims=True)
    solution[:, A:] = col_ok / col_ok.sum(1, keepdims=True)
    for s in range(S - 1, 0, -1):
        below = np.where(index[s] == 0, value[s].astype(np.float64), root_value[index[s], 0].astype(np.float64))
        ev[s, 0] = (chance[s].astype(np.float64) * below).sum(0).astype(np.float32)
        root_value[s, 0] = np.float32(solution[s, :A].astype(np.float64) @ ev[s, 0].astype(np.float64) @ solution[s, A:].astype(np.float64))
    return dict(index=index, value=value, chance=chance, expected_value=ev, legal=legal, root_value=root_value, solution=solution,
                spine=spine, meta=dict(A=A, C=C, D=D, twigs=twigs, ragged=ragged, depth=D))


# name -> spine_tree arguments.  Between them: (A, C) = (8, 8), (7, 5), (1, 8), (4, 1), (2, 8), (3, 3 ragged); every C = 1 .. 8;
# D = 10 (windows of 20 and 21 steps fit the compact word), D = 11 (a compact window of 21 steps cuts live lanes off after a lone row
# step; dense at 22), D = 15 (dense only: 30 steps), and "wide": runs of 280 one-state sibling twigs.  (A run of 300 siblings does not
# exist: a table of more than 255 rows needs A <= 6 -- the LDS of a learner workgroup, rows_max in csrc/bucket.hip make_plan -- and a
# state has at most A * A * C - 1 = 287 children then.  280 siblings under a forced table of 300 rows take the second byte all the same.)
SPINE = {
    "s88_d11": dict(A=8, C=8, D=11, twigs=6, seed=1),
    "s75_d10": dict(A=7, C=5, D=10, twigs=5, seed=2),
    "s18_d10": dict(A=1, C=8, D=10, twigs=3, seed=3),
    "s41_d6": dict(A=4, C=1, D=6, twigs=5, seed=4),
    "s28_d15": dict(A=2, C=8, D=15, twigs=4, seed=5),
    "s33r_d8": dict(A=3, C=3, D=8, twigs=4, seed=6, ragged=True),
    "s26_d3": dict(A=2, C=6, D=3, twigs=3, seed=7),
    "s27_d3": dict(A=2, C=7, D=3, twigs=3, seed=8),
    "wide_d4": dict(A=6, C=8, D=4, twigs=280, seed=9),
}
NATIVE = tuple(f"n{A}" for A in lr.TREES)  # the eight native trees of tests/_learnref.py: bushy and shallow, A = 1 .. 8
TREES = NATIVE + tuple(SPINE)
WIDE, WIDE_ROWS = "wide_d4", 300
DEEP = ("s88_d11", "s28_d15")  # D >= 11
COMPACT_MAX = 21  # rnad_hip.COMPACT_MAX_STEPS, pinned by tests/test_rollout_shapes.py


@functools.lru_cache(maxsize=None)
def native_tree(A):
    import rnad_hip  # (the generator is host code: the library loads without a device)

    kw = dict(lr.TREES[A])
    out = rnad_hip.tree_generate(kw.pop("A"), kw.pop("C"), kw.pop("depth_bound"), **kw)
    return {k: v.numpy() for k, v in out.items()}


def tree_levels(tree):
    """int [S]: the level of every state below the root (state 1: level 0; -1: not reachable).  Children are the entries with positive
    chance, and have larger ids."""
    index, chance = tree["index"], tree["chance"]
    level = np.full(index.shape[0], -1)
    level[1] = 0
    for s in range(1, index.shape[0]):
        if level[s] >= 0:
            kids = index[s][(index[s] != 0) & (chance[s] > 0)]
            assert (kids > s).all()
            level[kids] = level[s] + 1
    return level


def tree_depth(tree):
    """Levels of the tree: the longest episode has 2 * depth env steps."""
    return int(tree_levels(tree).max()) + 1


def upper_states(tree, rows):
    """The states above the cut of a table of `rows` rows, restated from build_cut (csrc/bucket.hip): the reachable states whose subtree
    has more than `rows` states."""
    index, chance = tree["index"], tree["chance"]
    level = tree_levels(tree)
    size = (level >= 0).astype(np.int64)
    for s in range(index.shape[0] - 1, 0, -1):
        if level[s] >= 0:
            size[s] += size[index[s][(index[s] != 0) & (chance[s] > 0)]].sum()
    return np.flatnonzero(size > rows)


def hybrid_staging(tree, rows, n_levels):
    """(budget, n_hot, n_upper): an RNAD_KEYS_STAGE_BYTES under which the hybrid keys walk stages exactly the top `n_levels` levels of
    the upper states of the cut in LDS, restated from get_cut (csrc/bucket.hip): whole levels, top down, while
    n_upper * 4 + 16 + n * per_state <= budget, per_state = A * A * C * 12 (an UpperWalk: two int32 and a float) + 2 * ((A + 3) & ~3) * 4
    (both players' policy rows).  The budget lies half a state above what those levels need: the next level does not fit."""
    S, C, A, _ = tree["index"].shape
    upper = upper_states(tree, rows)
    per_level = np.bincount(tree_levels(tree)[upper])
    n_hot = int(per_level[:n_levels].sum())
    per_state = A * A * C * 12 + 2 * ((A + 3) & ~3) * 4
    return len(upper) * 4 + 16 + n_hot * per_state + per_state // 2, n_hot, len(upper)


@functools.lru_cache(maxsize=None)
def tree(name):
    if name in SPINE:
        return spine_tree(**SPINE[name])
    t = dict(native_tree(int(name[1:])))
    t["meta"] = dict(A=t["index"].shape[-1], C=t["index"].shape[1], depth=tree_depth(t), ragged=False)
    return t


def legal_rows(t):
    """[2S, A] 0 / 1: the mover's legal mask of every (player, state) row."""
    return lr.legal_table(t["legal"])


def windows(name):
    """The T_cap values a case is replayed (and played) at: 2 * depth, and the edges of the compact word."""
    d = tree(name)["meta"]["depth"]
    w = [2 * d]
    if name == "s75_d10":
        w += [21]
    if name == "s88_d11":
        w += [21]
    return tuple(w)


# ------------------------------------------------------------------------------------------------ policy tables
@functools.lru_cache(maxsize=None)
def policy_table(name, kind="spine", seed=0):
    """fp32 [2S, A] rows for table_is_policy = 1: zero on illegal actions, NOT normalised (the kernels compare running sums with
    u * sum(p)).  "spine": P_SPINE on action A - 1 in the rows of spine states (native trees have none), random weights elsewhere, every
    row scaled by a factor of its own; "adversarial": tests/_numpy_rng.adversarial_weights per row, masked, with a legal positive entry."""
    t = tree(name)
    legal = legal_rows(t)
    n, A = legal.shape
    S = n // 2
    rng = np.random.default_rng([TREES.index(name), seed, ("spine", "adversarial").index(kind)])
    if kind == "adversarial":
        p = rng_ref.adversarial_weights(rng, n, A) * legal
        dead = p.sum(-1) <= 0
        p[dead, legal[dead].argmax(-1)] = np.float32(1e-3)
    else:
        p = (rng.random((n, A)) + 0.05) * legal
        p = p / p.sum(-1, keepdims=True)
        if "spine" in t and A > 1:
            rows = np.concatenate([t["spine"], S + t["spine"]])
            rest = p[rows].copy()
            rest[:, A - 1] = 0
            tot = rest.sum(-1, keepdims=True)
            rest = np.where(tot > 0, rest / np.maximum(tot, 1e-30) * (1 - P_SPINE), 0)
            rest[:, A - 1] = P_SPINE
            p[rows] = rest
        p = p * rng.uniform(0.5, 2.0, (n, 1))
    p = p.astype(np.float32)
    assert ((p > 0) <= (legal > 0)).all() and (p.sum(-1) > 0).all()
    p.setflags(write=False)
    return p


def strided(table, stride, column=0, fill=3.0):
    """The rows of `table` inside a wider one: A floats from `column` on in rows of `stride` floats, `fill` everywhere else (a kernel
    that reads a float too many draws differently)."""
    n, A = table.shape
    assert stride >= column + A
    out = np.full((n, stride), fill, np.float32)
    out[:, column: column + A] = table
    return out


def stride_variants(A, record_stride, record_column):
    """(stride, column): rows of A floats; of a multiple of 4 floats (the 16-byte loads of load_policy_row); a record-like row with
    the policy at a column offset."""
    return ((A, 0), ((A + 3) & ~3, 0), (record_stride, record_column))


# ------------------------------------------------------------------------------------------------ the replay
MUTANTS = ("outcome_2bits", "stale_uniforms", "shift32", "no_padding", "plus_zero", "local_lane", "no_lone_step", "column_row")


def transition(t, state, a0, a1, u, no_padding=False):
    """episode.py:106-121 for lanes in `state` with joint action (a0, a1) and the chance uniform u -> (outcome, next, reward)."""
    index, chance, value = t["index"], t["chance"], t["value"]
    S, C, A, _ = index.shape
    if no_padding:  # mutant: eight chance entries from the lane's record on, whatever C is (the device layout: [s][a0][a1][c])
        flat = lambda x: np.concatenate([np.ascontiguousarray(x.transpose(0, 2, 3, 1)).ravel(), np.zeros(8, x.dtype)])  # noqa: E731
        base = ((state * A + a0) * A + a1) * C
        at = base[:, None] + np.arange(8)
        c = rng_ref.pick(flat(chance)[at], u) if C > 1 else np.zeros(len(state), np.int64)
        return c, flat(index)[base + c], flat(value)[base + c] * (flat(index)[base + c] == 0).astype(np.float32)
    c = rng_ref.pick(chance[state, :, a0, a1], u) if C > 1 else np.zeros(len(state), np.int64)
    nxt = index[state, c, a0, a1]
    return c, nxt, (value[state, c, a0, a1] * (nxt == 0).astype(np.float32)).astype(np.float32)


def replay(t, table, B, T_cap, seed=SEED, lane0=LANE0, mutate=None):
    """Episodes.generate (episode.py:96-125, :194-212) with the seeded draws, for lanes lane0 .. lane0 + B - 1 and the tabular actor
    `table` [2S, A].  Every lane plays all T_cap env steps: an absorbed lane sits in state 0 and goes on drawing from that state's rows,
    as the dense kernels do.  An odd T_cap ends with a row step and no transition.
    -> dict: indices int64 [T_cap + 1, B], actions / outcomes int64 [T_cap, B] (outcomes: -1 on row steps), rewards fp32 [T_cap, B],
    policy fp32 [T_cap, B, A], mask_bits uint8 [T_cap, B], alive int64 [T_cap + 1]; and the compact view: acts uint64 [B] (3 bits per
    LIVE step; None beyond 21 steps), final_reward fp32 [B] (the reward of the transition that leaves the tree), visited int32 [2S] (the rows live slots sit
    in, and the two rows of state 0)."""
    assert mutate is None or mutate in MUTANTS
    S = t["index"].shape[0]
    A = table.shape[1]
    bits = lr.mask_bits(legal_rows(t))
    state = np.ones(B, np.int64)
    out = dict(indices=np.zeros((T_cap + 1, B), np.int64), actions=np.zeros((T_cap, B), np.int64), outcomes=np.full((T_cap, B), -1, np.int64),
               rewards=np.zeros((T_cap, B), np.float32), policy=np.zeros((T_cap, B, A), np.float32), mask_bits=np.zeros((T_cap, B), np.uint8))
    u = a0 = None
    for step in range(T_cap):
        if step % 2 == 0:
            t_u = step - 2 if (mutate == "stale_uniforms" and step >= 10) else step
            u = rng_ref.decision_uniforms(B, seed, 0 if mutate == "local_lane" else lane0, t_u)
        row = (step & 1) * S + state
        pol = table[state if mutate == "column_row" else row]
        a = rng_ref.pick(pol, u[:, step & 1])
        if mutate == "no_lone_step" and step == T_cap - 1 and step % 2 == 0:
            a = np.zeros(B, np.int64)
        out["indices"][step], out["actions"][step], out["policy"][step], out["mask_bits"][step] = state, a, table[row], bits[row]
        if step & 1:
            c, nxt, rew = transition(t, state, a0, a, u[:, 2], no_padding=mutate == "no_padding")
            if mutate == "outcome_2bits" and step < 10:
                c = c & 3
                nxt = t["index"][state, c, a0, a]
                rew = (t["value"][state, c, a0, a] * (nxt == 0).astype(np.float32)).astype(np.float32)
            if mutate == "plus_zero":
                rew = rew + np.float32(0.0)
            out["outcomes"][step], out["rewards"][step] = c, rew
            state = nxt
        else:
            a0 = a
    out["indices"][T_cap] = state
    return _summaries(out, S, mutate)


def _summaries(out, S, mutate=None):
    """alive and the compact view of the per-slot arrays of a replay."""
    T_cap, B = out["actions"].shape
    live = out["indices"][:T_cap] != 0
    out["alive"] = (out["indices"] != 0).sum(1)
    acts = np.zeros(B, np.uint64) if T_cap <= COMPACT_MAX else None  # (a longer window has no compact form)
    for step in range(T_cap if acts is not None else 0):
        if mutate == "shift32" and step == 20:
            continue
        acts |= np.where(live[step], out["actions"][step], 0).astype(np.uint64) << np.uint64(3 * step)
    leaves = live & (out["indices"][1:] == 0)  # the transition into state 0: at most one per lane
    assert mutate is not None or (leaves.sum(0) <= 1).all()  # (a wrong program may walk back into the tree: its first exit counts)
    final = np.zeros(B, np.float32)
    at = leaves.argmax(0)
    final[leaves.any(0)] = out["rewards"][at, np.arange(B)][leaves.any(0)]
    visited = np.zeros(2 * S, np.int32)
    rows = ((np.arange(T_cap) & 1)[:, None] * S + out["indices"][:T_cap])[live]
    visited[rows] = 1
    visited[0] = visited[S] = 1
    out.update(acts=acts, final_reward=final, visited=visited, live=live)
    return out


def prefix(ref, B):
    """The replay of the first B lanes of a replay: a lane's episode depends on its global lane alone."""
    S = len(ref["visited"]) // 2
    return _summaries({k: ref[k][:, :B] for k in ("indices", "actions", "outcomes", "rewards", "policy", "mask_bits")}, S)


@functools.lru_cache(maxsize=None)
def reference(name, T_cap, kind="spine", B=B_MAIN, lane0=LANE0):
    """The replay of a case, computed once and shared by the tests (which leave it unchanged)."""
    return replay(tree(name), policy_table(name, kind), B, T_cap, SEED, lane0)


def cases():
    return [(name, T_cap) for name in TREES for T_cap in windows(name)]


COMPARED = ("indices", "actions", "rewards", "policy", "mask_bits", "alive", "acts", "final_reward", "visited")


def differs(a, b):
    """The compared outputs of two replays that differ, floats as bit patterns."""
    view = lambda x: x.view(np.int32) if x.dtype == np.float32 else x  # noqa: E731
    return [k for k in COMPARED if a[k] is not None and not np.array_equal(view(a[k]), view(b[k]))]


# ------------------------------------------------------------------------------------------------ the bucket order, restated
def order(tree_obj, B, indices):
    """(key [B], lane_ids [B], n_groups): the bucket of every lane under the cut the LIBRARY chose for (tree, B) (rnad_bucket_map --
    the cut is its choice, the key of a lane is restated on the host by tests/_gpu.bucket_keys) and the stable argsort by it.
    indices int [T_cap + 1, B]: the replay's states."""
    import _gpu

    key, n_groups = _gpu.bucket_keys(tree_obj, B, np.asarray(indices[:-1]), np.asarray(indices[-1]))
    return key, np.argsort(key, kind="stable"), n_groups


def check_work_items(items, key, lane_ids, chunk=256):
    """The work list [n, 4] (begin, count, bucket, single) tiles the sorted lanes bucket by bucket, at most `chunk` lanes per item (the
    checks of tests/test_hip_bucket.py::test_bucketed_rollout_is_the_lane_ordered_rollout)."""
    sk = key[lane_ids]
    assert items[:, 1].sum() == len(key) and (items[:, 1] > 0).all() and (items[:, 1] <= chunk).all()
    np.testing.assert_array_equal(items[:, 0], np.concatenate([[0], np.cumsum(items[:, 1])[:-1]]))
    for begin, count, bucket, single in items:
        assert (sk[begin: begin + count] == bucket).all()
        assert bool(single) == ((sk == bucket).sum() <= chunk)
