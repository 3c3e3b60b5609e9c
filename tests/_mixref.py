"""fp64 reference, error gates, weight sets and cases for the mixture sweep (csrc/mixture.hip, util.metric.mixture).

A link (s, r, c, t) -> u is live when chance[s,t,r,c] > 0 and index[s,t,r,c] = u != 0.  With J [S, n, 2A] and w [2, n]:

    R[1, side, k] = 1
    R[u, 0, k]    = R[s, 0, k] * J[s, k, r]              R[u, 1, k] = R[s, 1, k] * J[s, k, A + c]
    D[s, side]    = sum_k w[side, k] * R[s, side, k]
    M[s, side*A+a] = sum_k w[side, k] * R[s, side, k] * J[s, k, side*A + a] / D[s, side]      where D > 0
                   = sum_k w[side, k] * J[s, k, side*A + a]                                    where D == 0

`reference` walks the levels of `_crossref.level_order` top-down, vectorised per level.  State 0 and states no live path reaches keep
zero rows.

The gates are derived, not measured.  Every term is nonnegative, so there is no cancellation and every error is relative.  In fp32
R at depth d is a product of d factors: d roundings.  A term w * R * J of a numerator carries those d and its two products, a term
w * R of D those d and one product; a sum of n terms puts at most n - 1 roundings on each term, whatever the order (the half-wave
butterfly of the kernel puts ceil(log2 n) <= 5 on it: adding a spare lane's 0 rounds nothing); the quotient adds one.  Numerator and
denominator together: at most (d + 2 + n) + (d + 1 + n) + 1 = 2d + 2n + 4 factors (1 + delta), |delta| <= 2^-24; the + 8 instead of
+ 4 pays for the second-order terms ((1 + u)^k - 1 <= 1.01 k u for k <= 10^4) and for the factors of D standing in a denominator.
The D == 0 row is one product and a sum, well inside.  Hence

    |got - M| <= (2 * depth[s] + 2 * n + 8) * 2^-24 * M[s]          |got - R| <= (depth[s] + 1) * 2^-24 * R[s]

(the + 1 on R again for the second order).  The weights are the fp32 numbers the device reads: the reference takes them as they are.
"""
import functools

import numpy as np

import _crossref as cr

U = cr.U
VARIANTS = ("average", "joint", "swapped")
WEIGHTS = ("uniform", "dirichlet", "zeros", "onehot")


def reference(tree_arrays, J, w, dtype=np.float64, variant=None):
    """(M [S, 2A], R [S, 2, n]) in `dtype` and depth int [S] (-1: not reached).  variant: None, or one of VARIANTS -- a deliberately
    wrong restatement: "average" forgets the reach (the state-wise weighted average of the tables), "joint" multiplies the member's
    opponent-side factor into its reach as well, "swapped" gives the row side's reach the column action and the other way round."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    chance = np.asarray(tree_arrays["chance"])
    S, C, A, _ = index.shape
    J = np.asarray(J).astype(dtype)
    n = J.shape[1]
    w = np.asarray(w).astype(dtype)
    assert J.shape == (S, n, 2 * A) and w.shape == (2, n)
    live = (index != 0) & (chance > 0)
    M = np.zeros((S, 2 * A), dtype)
    R = np.zeros((S, 2, n), dtype)
    depth = np.full((S,), -1, np.int64)
    R[1] = 1
    for d, states in enumerate(cr.level_order(index, chance)):
        depth[states] = d
        Rs = R[states]                                                        # [m, 2, n]
        Js = J[states].reshape(-1, n, 2, A).transpose(0, 2, 1, 3)             # [m, 2, n, A]
        wr = (w[None] * (np.ones_like(Rs) if variant == "average" else Rs)).astype(dtype)
        num = (wr[..., None] * Js).astype(dtype).sum(axis=2, dtype=dtype)     # [m, 2, A]
        D = wr.sum(axis=2, dtype=dtype)                                       # [m, 2]
        flat = (w[None, :, :, None] * Js).astype(dtype).sum(axis=2, dtype=dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            M[states] = np.where(D[..., None] > 0, num / D[..., None], flat).astype(dtype).reshape(-1, 2 * A)
        m_pos, t_, r_, c_ = np.nonzero(live[states])
        if m_pos.size:
            child = index[states][m_pos, t_, r_, c_]
            own_row, own_col = Js[m_pos, 0, :, r_], Js[m_pos, 1, :, c_]       # [links, n]
            if variant == "swapped":
                own_row, own_col = own_col, own_row
            if variant == "joint":
                own_row = own_col = (own_row * own_col).astype(dtype)
            R[child, 0] = (Rs[m_pos, 0] * own_row).astype(dtype)
            R[child, 1] = (Rs[m_pos, 1] * own_col).astype(dtype)
    assert M.dtype == dtype and R.dtype == dtype
    return M, R, depth


def gates(M, R, depth, n):
    """(gate of the mixture [S, 2A], gate of the reach [S, 2, n]): the bounds of the module docstring."""
    d = np.maximum(depth, 0).astype(np.float64)
    return ((2 * d + 2 * n + 8) * U)[:, None] * np.asarray(M, np.float64), ((d + 1) * U)[:, None, None] * np.asarray(R, np.float64)


def eps(depth, n):
    """The largest relative error the mixture's gate allows anywhere on the tree."""
    return float((2 * depth.max() + 2 * n + 8) * U)


def weights(kind, n, seed=0):
    """[2, n] fp32 (row side, column side), normalised in fp64 first as util.metric.mixture does."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "uniform":
        w = np.ones((2, n))
    elif kind == "dirichlet":
        w = rng.dirichlet(np.ones(n), size=2)          # the two sides differ
    elif kind == "zeros":
        w = rng.dirichlet(np.ones(n), size=2)
        w[0, 1::2] = 0.0                                # n = 1: nothing to drop, the set degenerates to one-hot
        if n > 1:
            w[1, 0] = 0.0
    else:
        assert kind == "onehot"
        w = np.zeros((2, n))
        w[:, 0] = 1.0                                   # player 0 of _crossref.players is the tree's solution
    w = w / w.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(w.astype(np.float32))


def exact_weights(w):
    """(x, y) in fp64, each summing to 1: the mixture that fp32 weights describe.  Scaling a side's weights leaves the mixture as it is
    (D scales with the numerators), so weights that sum to 1 + a few 2^-24 stand for their normalised selves."""
    w = np.asarray(w, np.float64)
    return w[0] / w[0].sum(), w[1] / w[1].sum()


@functools.lru_cache(maxsize=None)
def case(name, n, kind, seed=0):
    """(tree arrays, J [S, n, 2A], w [2, n], M, R, depth, gate of M, gate of R) of one test case, computed once and read-only."""
    tree = cr.tree_arrays(name)
    J = cr.players(tree, n, seed, cr.fixture_policy(name))
    w = weights(kind, n, seed)
    M, R, depth = reference(tree, J, w)
    gM, gR = gates(M, R, depth, n)
    for a in (J, w, M, R, depth, gM, gR):
        a.setflags(write=False)
    return tree, J, w, M, R, depth, gM, gR


def never_reached_by_the_mixture(w, R, depth):
    """bool [S, 2]: reached states with D == 0 on a side."""
    D = (np.asarray(w, np.float64)[None] * R).sum(axis=2)
    return (depth >= 0)[:, None] & (D == 0)
