"""fp64 reference, error gates and cases for the best-response sweep (csrc/best_response.hip, util.metric.best_response).

For table k of J [S, n, 2A], side 0 is the row player responding to k's column side and side 1 the column player responding to k's row
side.  A record (s, t, r, c) counts when chance > 0; it is a live link when moreover index != 0.

    m[s, side, k, r, c] = sum_t chance * (index == 0 ? (side ? -value : value) : V[index, side, k])
    q[s, 0, k, r]       = sum_c m[s, 0, k, r, c] * J[s, k, A + c]          q[s, 1, k, c] = sum_r J[s, k, r] * m[s, 1, k, r, c]
    V[s, side, k]       = max over the side's legal a of q[s, side, k, a]   (-inf without a legal action)
    best[s, k, side*A+a] = 1 at the first legal a that attains V
    G[s, side, k]       = V[s, side, k] - sum over legal a of J[s, k, side*A + a] * q[s, side, k, a]
    R[1, k] = 1,   R[u, k] = R[s, k] * (J[s, k, r] * J[s, k, A + c]) * chance           for every live link (s, t, r, c) -> u

`reference` walks the levels of `_crossref.level_order`, bottom-up for q, V, best, G and top-down for R, in the operation order of the
kernel (t ascending inside a joint action, then the other side's action ascending; legal actions ascending in the maximum and in the
played sum), so that `reference(..., dtype=np.float32)` is a restatement of the kernel.  State 0 and states no live path reaches keep
zero rows.

The gates are derived, not measured; u = 2^-24.

q and V.  Written term by term, q[s, side, k, a] is a sum of A * C terms x * chance * J, x a payoff or a child's V.  In the kernel's
order a term meets its product with chance, at most C - 1 sums over t (the first is 0 + term, exact), its product with J and at most
A - 1 sums over the other side's action: at most A + C roundings, each at most u times a partial sum that the sum of the absolute
terms bounds.  With the children's own bounds in place of their values that sum is Bq[s, side, k, a]: the same recursion on |value|,
and B[s, side, k] = max over the legal a of Bq >= |V|.  A child's error enters with the weight chance * J of its term, so by induction
over the height h[s] (1 where no record leads to a child)

    |got q - q| <= h[s] * (A + C + 2) * u * Bq[s, side, k, a]          |got V - V| <= h[s] * (A + C + 2) * u * B[s, side, k]

the second because a maximum is 1-Lipschitz in the sup norm; the + 2 pays for the second-order terms, (1 + u)^k - 1 <= 1.01 k u for
every k that occurs.  No convexity is needed: the weights stand inside Bq as they are.  This is tighter than the count A * C + 4 of a
sum taken in one go: the kernel's two-stage order never puts more than A + C roundings on a term.
The action the kernel picks maximises its own q over the legal actions, so its exact q is within gate(q of it) + gate(q of the exact
maximiser) <= 2 * gate(V) of the exact maximum.

G.  The played sum P = sum over legal a of J * q adds a product and at most A - 1 sums per term, the difference V - P one more rounding
on |V| + |P|, and q enters P with the weights J:

    |got G - G| <= gate(V) + sum_a J[a] * gate(q[a]) + (A + 2) * u * sum_a J[a] * |q[a]| + 2 * u * |V|

R.  Every factor is nonnegative: no cancellation, the error is relative.  A level multiplies three times (J * J, R *, * chance):

    |got R - R| <= (3 * depth[s] + 1) * u * R[s, k]

Players: `_crossref.players` -- player 0 is the tree's solution, player 1 uniform over the legal actions, then the fixture's joint
policy where there is one, then seeded masked softmax tables.
"""
import functools
import types

import numpy as np

import _crossref as cr

U = cr.U
VARIANTS = ("swapped", "illegal", "one_step", "plus_terminal", "reach_kreach", "reach_no_chance")
CHUNK = 4096  # states of a level taken at a time: bounds the [chunk, A, A, n] temporaries


def size(S, n):
    """rnad_best_response_size restated: floats of `values` (and of `gain`)."""
    return 2 * S * n if S >= 2 and 1 <= n <= 32 else -1


def reference(tree_arrays, J, dtype=np.float64, variant=None):
    """A namespace of Q, Bq [S, 2, n, A]; V, G, B, P_abs [S, 2, n] (P_abs = sum over legal a of J * |q|); best [S, n, 2A]; R [S, n];
    h, depth int [S] (depth -1: not reached); legal bool [S, 2, A]; all floats in `dtype`.  variant: None, or one of VARIANTS -- a
    deliberately wrong restatement: "swapped" responds to the table's other side, "illegal" maximises over every action, "one_step" puts
    the table's own play below the state instead of the best response, "plus_terminal" gives the column side +value at a terminal,
    "reach_kreach" takes the reach in the J[A + r] * J[c] orientation of nashconv.hip's k_reach, "reach_no_chance" leaves chance out of
    the reach."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    lg = np.asarray(tree_arrays["legal"])[:, 0] != 0                      # [S, A, A]
    S, C, A, _ = index.shape
    J = np.asarray(J).astype(dtype)
    n = J.shape[1]
    assert J.shape == (S, n, 2 * A)
    legal = np.stack([lg[:, :, 0], lg[:, 0, :]], axis=1)                  # row player's actions, column player's (metric.py:167-168)
    if variant == "illegal":
        legal = np.ones_like(legal)
    rows, cols = J[:, :, :A], J[:, :, A:]
    zero, ninf = dtype(0), dtype(-np.inf)
    out = types.SimpleNamespace(
        Q=np.zeros((S, 2, n, A), dtype), Bq=np.zeros((S, 2, n, A), np.float64), V=np.zeros((S, 2, n), dtype), G=np.zeros((S, 2, n), dtype),
        B=np.zeros((S, 2, n), np.float64), P_abs=np.zeros((S, 2, n), np.float64), best=np.zeros((S, n, 2 * A), dtype), R=np.zeros((S, n), dtype),
        h=np.zeros((S,), np.int64), depth=np.full((S,), -1, np.int64), legal=legal)
    W = np.zeros((S, 2, n), dtype)                                        # what a parent reads: V, or the table's own play ("one_step")
    levels = cr.level_order(index, chance)
    for d, states in enumerate(levels):
        out.depth[states] = d
    with np.errstate(invalid="ignore", over="ignore"):
        for level in reversed(levels):
            for lo in range(0, level.size, CHUNK):
                states = level[lo:lo + CHUNK]
                idx, live, val = index[states], chance[states] > 0, value[states]      # [m, C, A, A]
                w, term = chance[states], index[states] == 0
                m_count = states.size
                link = live & ~term
                deepest = np.where(link, out.h[idx], 0).reshape(m_count, -1).max(axis=1)
                out.h[states] = 1 + deepest
                for side in (0, 1):
                    sign = dtype(-1) if side == 1 and variant != "plus_terminal" else dtype(1)
                    M = np.zeros((m_count, A, A, n), dtype)
                    BM = np.zeros((m_count, A, A, n), np.float64)
                    for t in range(C):
                        x = np.where(term[:, t, :, :, None], (sign * val[:, t])[..., None], W[idx[:, t], side])
                        M = M + np.where(live[:, t, :, :, None], (x * w[:, t, :, :, None]).astype(dtype), zero)
                        bx = np.where(term[:, t, :, :, None], np.abs(val[:, t]).astype(np.float64)[..., None], out.B[idx[:, t], side])
                        BM = BM + np.where(live[:, t, :, :, None], bx * w[:, t, :, :, None].astype(np.float64), 0.0)
                    responds_to_cols = (side == 0) != (variant == "swapped")
                    opp = (cols if responds_to_cols else rows)[states]                 # [m, n, A]
                    own = (rows if responds_to_cols else cols)[states]
                    q = np.zeros((m_count, n, A), dtype)
                    bq = np.zeros((m_count, n, A), np.float64)
                    for j in range(A):  # the other side's action, ascending
                        Mj, BMj = (M[:, :, j, :], BM[:, :, j, :]) if side == 0 else (M[:, j, :, :], BM[:, j, :, :])   # [m, own action, n]
                        q = q + (Mj.transpose(0, 2, 1) * opp[:, :, j, None]).astype(dtype)
                        bq = bq + BMj.transpose(0, 2, 1) * opp[:, :, j, None].astype(np.float64)
                    ok = legal[states, side][:, None, :]                                # [m, 1, A]
                    qm = np.where(ok, q, ninf)
                    v = qm.max(axis=2)
                    arg = qm.argmax(axis=2)                                             # the first maximum: ties go to the lowest index
                    one_hot = (np.arange(A)[None, None, :] == arg[:, :, None]) & ok.any(axis=2, keepdims=True)
                    played = np.zeros((m_count, n), dtype)
                    for a in range(A):
                        played = played + np.where(ok[:, :, a], (own[:, :, a] * q[:, :, a]).astype(dtype), zero)
                    out.Q[states, side], out.Bq[states, side] = q, bq
                    out.V[states, side], out.G[states, side] = v, (v - played).astype(dtype)
                    out.B[states, side] = np.where(ok, bq, 0.0).max(axis=2)
                    out.P_abs[states, side] = np.where(ok, own.astype(np.float64) * np.abs(q.astype(np.float64)), 0.0).sum(axis=2)
                    out.best[states, :, side * A:(side + 1) * A] = one_hot.astype(dtype)
                    W[states, side] = played if variant == "one_step" else v
    out.R[1] = 1
    for level in levels:
        idx, link = index[level], (index[level] != 0) & (chance[level] > 0)
        m_pos, t_, r_, c_ = np.nonzero(link)
        if m_pos.size == 0:
            continue
        s_ = level[m_pos]
        child = idx[m_pos, t_, r_, c_]
        joint = (cols[s_, :, r_] * rows[s_, :, c_]) if variant == "reach_kreach" else (rows[s_, :, r_] * cols[s_, :, c_])   # [links, n]
        through = (out.R[s_] * joint.astype(dtype)).astype(dtype)
        out.R[child] = through if variant == "reach_no_chance" else (through * chance[s_, t_, r_, c_][:, None]).astype(dtype)
    for a in (out.Q, out.V, out.G, out.best, out.R):
        assert a.dtype == dtype
    return out


def gates(tree_arrays, ref, J):
    """(gate of V [S, 2, n], gate of q [S, 2, n, A], gate of G [S, 2, n], gate of R [S, n]): the bounds of the module docstring, from an
    fp64 `ref`."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    n = ref.R.shape[1]
    k = ref.h.astype(np.float64) * ((A + C + 2) * U)
    gV, gQ = k[:, None, None] * ref.B, k[:, None, None, None] * ref.Bq
    own = np.asarray(J, np.float64).reshape(-1, n, 2, A).transpose(0, 2, 1, 3)              # [S, 2, n, A]
    ok = ref.legal[:, :, None, :]
    gG = gV + np.where(ok, own * gQ, 0.0).sum(axis=3) + (A + 2) * U * ref.P_abs + 2 * U * np.abs(np.where(np.isfinite(ref.V), ref.V, 0.0))
    gR = ((3 * np.maximum(ref.depth, 0) + 1) * U)[:, None] * np.asarray(ref.R, np.float64)
    return gV, gQ, gG, gR


def exploitability(ref):
    """[n, 2] fp64: sum over the states of R * G, the right-hand side of the performance-difference identity."""
    return (np.asarray(ref.R, np.float64)[:, None, :] * np.asarray(ref.G, np.float64)).sum(axis=0).T


def picked_regret(ref, best):
    """[S, 2, n] fp64: how far the exact q of the action that the one-hot table `best` [S, n, 2A] names lies below the exact maximum
    (0 where the row of `best` is zero)."""
    S, n, A2 = best.shape
    A = A2 // 2
    hot = np.asarray(best, np.float64).reshape(S, n, 2, A).transpose(0, 2, 1, 3)            # [S, 2, n, A]
    q = np.where(hot != 0, np.asarray(ref.Q, np.float64), 0.0).sum(axis=3)
    return np.where(hot.any(axis=3), np.where(np.isfinite(ref.V), ref.V, 0.0) - q, 0.0)


@functools.lru_cache(maxsize=None)
def case(name, n, seed=0):
    """A namespace of one test case, computed once and read-only: tree (arrays), J [S, n, 2A] fp32, ref (fp64 reference), gV, gQ, gG,
    gR, reached bool [S]."""
    tree = cr.tree_arrays(name)
    J = cr.players(tree, n, seed, cr.fixture_policy(name))
    ref = reference(tree, J)
    gV, gQ, gG, gR = gates(tree, ref, J)
    for a in (J, gV, gQ, gG, gR) + tuple(v for v in vars(ref).values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return types.SimpleNamespace(tree=tree, J=J, ref=ref, gV=gV, gQ=gQ, gG=gG, gR=gR, reached=ref.depth >= 0)
