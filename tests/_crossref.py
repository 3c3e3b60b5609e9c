"""fp64 reference, error gate and player tables for the cross-play sweep (csrc/cross_play.hip, util.metric.cross_play).

    V[0, i, j] = 0
    V[s, i, j] = sum_{r,c} J_i[s, r] * J_j[s, A + c] * sum_t chance[s,t,r,c] * (index[s,t,r,c] == 0 ? value[s,t,r,c] : V[index, i, j])

Entries with chance <= 0 are skipped.  `reference` walks the levels it builds from `index` bottom-up, vectorised per level: the
terminal entries of a state collapse to one A x A matrix, the others are a list of (parent, r, c, child) links whose contributions
are summed per parent.

The gate is derived, not measured.  In fp32 a state's value is a sum of A * A * C products; written term by term, each term meets
at most A * A * C + 2 roundings on its way into the state's value (its products, then every partial sum it is part of), each at
most 2^-24 of the partial sum, which the sum of the absolute terms bounds.  That sum, with the children's own bounds in place of
their values, is B[s, i, j]: the same recursion on |value|.  The children's errors enter through a convex combination (the policy
and chance weights are >= 0 and sum to at most 1 up to rounding), so the bound grows by one such term per level of height:

    |got - V| <= h[s] * (A * A * C + 4) * 2^-24 * B[s, i, j]

with h[s] = 1 where every child is terminal; the + 4 instead of + 2 pays for the second-order terms and for weights that sum to
1 + a few 2^-24.
"""
import functools

import numpy as np

from _util import TREES, load, load_tree

U = 2.0 ** -24
VARIANTS = ("swapped", "no_chance", "no_terminal", "transposed")
NATIVE_SPECS = {
    "native_a3": dict(A=3, C=2, depth_bound=5, transition_threshold=0.2, seed=1, prune=(0, 0)),
    "native_a5": dict(A=5, C=4, depth_bound=4, transition_threshold=0.2, seed=11, prune=(1, 2)),
}


def level_order(index, chance):
    """States grouped by depth below the root (state 1), from the links with index != 0 and chance > 0."""
    index = np.asarray(index)
    live = (index != 0) & (np.asarray(chance) > 0)
    levels = [np.array([1], np.int64)]
    while True:
        cur = levels[-1]
        nxt = index[cur][live[cur]]
        if nxt.size == 0:
            break
        nxt = np.unique(nxt)
        assert nxt.min() > 0 and nxt.size == index[cur][live[cur]].size, "the index tensor is not a tree"
        levels.append(nxt.astype(np.int64))
    return levels


def reference(tree_arrays, policies, dtype=np.float64, variant=None):
    """(V, B, h): V, B [S, n, n] in `dtype`, h int [S].  policies [S, n, 2A].  variant: None, or one of VARIANTS -- a deliberately
    wrong restatement (the mutations of tests/test_cross_play.py)."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    S, C, A, _ = index.shape
    J = np.asarray(policies).astype(dtype)
    n = J.shape[1]
    assert J.shape == (S, n, 2 * A)
    rows, cols = (J[:, :, A:], J[:, :, :A]) if variant == "swapped" else (J[:, :, :A], J[:, :, A:])
    live = chance > 0
    w = np.where(live, 1.0 if variant == "no_chance" else chance, 0.0).astype(dtype)
    V = np.zeros((S, n, n), dtype)
    B = np.zeros((S, n, n), dtype)
    h = np.zeros((S,), np.int64)
    for states in reversed(level_order(index, chance)):
        idx = index[states]                                   # [m, C, A, A]
        wl = w[states]
        term = (idx == 0)
        pay = np.zeros_like(value[states]) if variant == "no_terminal" else value[states]
        pr, pc = rows[states], cols[states]                   # [m, n, A]
        # terminal entries: one A x A matrix per state
        for out, x in ((V, pay), (B, np.abs(value[states]))):
            T = np.where(term, wl * x, 0.0).astype(dtype).sum(axis=1)   # [m, A, A]
            out[states] = np.matmul(np.matmul(pr, T), pc.transpose(0, 2, 1))   # sum_{r,c} pr[m,i,r] T[m,r,c] pc[m,j,c]
        h[states] = 1
        # links to children: (parent position, r, c) -> child, summed per parent
        m_pos, t_, r_, c_ = np.nonzero((~term) & live[states])
        if m_pos.size:
            child = idx[m_pos, t_, r_, c_]
            weight = (wl[m_pos, t_, r_, c_][:, None, None] * pr[m_pos, :, r_][:, :, None]) * pc[m_pos, :, c_][:, None, :]   # [links, n, n]
            starts = np.flatnonzero(np.r_[True, m_pos[1:] != m_pos[:-1]])
            parents = states[m_pos[starts]]
            for out in (V, B):
                out[parents] += np.add.reduceat(weight * out[child], starts, axis=0)
            h[parents] = 1 + np.maximum.reduceat(h[child], starts)
    if variant == "transposed":
        V = np.ascontiguousarray(V.transpose(0, 2, 1))
    return V, B, h


def gate(tree_arrays, B, h):
    """[S, n, n]: the bound on |got - V| of the module docstring."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    return h[:, None, None] * ((A * A * C + 4) * U) * np.asarray(B, np.float64)


def share(got, V, g):
    """Largest |got - V| / gate over the elements (0 where both are 0; inf where the gate is 0 and the values differ)."""
    err = np.abs(np.asarray(got, np.float64) - V)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / g)
    return float(s.max())


# ---------------------------------------------------------------------------------------------------- trees
@functools.lru_cache(maxsize=None)
def tree_arrays(name):
    """The reference-layout arrays of a golden tree (tests/golden/tree_<name>.npz) or of a NATIVE_SPECS tree (host generator)."""
    if name in TREES:
        return load_tree(name)
    import rnad_hip

    k = NATIVE_SPECS[name]
    out = rnad_hip.tree_generate(k["A"], k["C"], k["depth_bound"], float(k["transition_threshold"]), (-1.0, 1.0), k["prune"], k["seed"])
    arrs = {key: out[key].numpy() for key in ("index", "value", "chance", "expected_value", "legal", "root_value", "solution")}
    arrs["meta"] = dict(kw=dict(depth_bound=k["depth_bound"]), spec=k)
    return arrs


def fixture_policy(name):
    """joint_policy of tests/golden/nashconv_<name>.npz for a golden tree, else None."""
    return load("nashconv_" + name)["joint_policy"] if name in TREES else None


def players(tree, n, seed=0, fixture=None):
    """[S, n, 2A] fp32: the tree's solution, uniform over the legal actions, the fixture's joint_policy where there is one, then seeded
    masked softmax tables.  The rows of a state without legal actions (state 0) are zero in the tables built here."""
    legal = np.asarray(tree["legal"])[:, 0]                               # [S, A, A]
    S, A, _ = legal.shape
    mask = np.concatenate([legal[:, :, 0], legal[:, 0, :]], axis=1) != 0  # row player's actions | column player's
    count = np.concatenate([np.repeat(mask[:, :A].sum(1, keepdims=True), A, 1), np.repeat(mask[:, A:].sum(1, keepdims=True), A, 1)], axis=1)
    tables = [np.asarray(tree["solution"], np.float32), (mask / np.maximum(count, 1)).astype(np.float32)]
    if fixture is not None:
        tables.append(np.asarray(fixture, np.float32))
    rng = np.random.default_rng(seed)
    while len(tables) < n:
        e = np.where(mask, np.exp(2.0 * rng.standard_normal((S, 2 * A))), 0.0)
        tot = np.concatenate([np.repeat(e[:, :A].sum(1, keepdims=True), A, 1), np.repeat(e[:, A:].sum(1, keepdims=True), A, 1)], axis=1)
        tables.append((e / np.maximum(tot, 1e-300)).astype(np.float32))
    return np.ascontiguousarray(np.stack(tables[:n], axis=1))


@functools.lru_cache(maxsize=None)
def case(name, n, seed=0):
    """(tree arrays, policies [S, n, 2A], V, gate) of one test case, computed once."""
    tree = tree_arrays(name)
    J = players(tree, n, seed, fixture_policy(name))
    V, B, h = reference(tree, J)
    for a in (J, V):
        a.setflags(write=False)
    g = gate(tree, B, h)
    g.setflags(write=False)
    return tree, J, V, g
