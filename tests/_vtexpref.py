"""The exact expected learner update (csrc/vtrace_expect.hip, rnad_hip.vtrace_expect, learn.vtrace.expected_update): its definition by
enumeration, the sweep in the kernel's order of operations, derived gates, inputs and deliberately wrong variants.  numpy only.

DEFINITION.  `enumerate_batch` builds the batch that holds every complete episode of a tree exactly once (actions with mu = 0 and records
with chance <= 0 are never drawn) with the probability of each under the behaviour table mu and the tree's chance; `enumeration` runs
`_learnref.learner(np.float64, ...)` on it and reduces, with row = P * S + s:

    reach[s]       = sum_lanes prob [lane visits s]
    target[P, s]   = sum_lanes prob v_target_P at the slot / reach[s]              q[P, s, a] likewise
    dv_sum[row]    = sum_lanes prob N_P dv at the slot                             dlogit_sum[row, a] likewise        (N_P: the program's norm)

SWEEP.  `reference(dtype, ...)` is the bottom-up recursion of include/rnad_hip.h (rnad_vtrace_expect) operation by operation as the kernel
performs it: the chance outcomes t ascending inside a joint action, the child's row actions a' ascending inside an outcome, b ascending
inside a, every skipped term (mu = 0, chance <= 0) skipped by a select.  np.float64 is the reference, np.float32 the stand-in for a correct
kernel.  The reach is `_brref.reference`'s for the table mu (the kernel launches rnad_best_response's top-down kernel).

GATES.  Every value is a `_learnref.VM`: it carries the sum of its absolute terms m (mag(x +- y) = mag x + mag y, mag(x y) = mag x mag y,
mag(x / y) = mag x / |y|, a select or min takes the magnitude of the operand taken).  u = 2^-24, h[s] the height of s.  Counting the
roundings that one term of the longest chain -- the column side's target -- meets at its own level:
    cs1 = pip / mu and the child's cs0 (2 divisions), w' = cs1 cs0 (1), X: g eta, its product with e0[n], e0[n]'s own A products and sums
    (at most A + 1), the three sums and the product g g vv1 -- the term of X that meets most: A + 5 --, min * X (1), lgg = (lambda g) g and
    its two products (4, on the other summand, not more than X's), the sum of the two summands (1), the product with mu0[n][a'] (1), the
    A-fold child sum (A), the product with chance (1), the sum over C outcomes (C), the product with mu1[b] (1), the sum over b (A), the sum
    with vv1 (1), and for target[1] the product with mu0[a] and the sum over a (A + 1):        4A + C + 16, + 2 for second order.
Every other output meets fewer.  A child's error enters with the weight of its term and the child's magnitude enters m with the same
weight, min(w, .) is 1-Lipschitz in w, so by induction over the height
    |got - want| <= h[s] K u m,      K = 4A + C + 18,
for target, target_given_row and q alike.  reach: DESIGN.md 1.4's bound with the subnormal term of _regevalref,
(3 depth[s] + 1) (u R + 2^-126).

DIRECTION.  `direction` is the NeuRD row gradient of the sampled program (learn/vtrace.py:362-431 in closed form, as `_learnref.learner`)
evaluated at the EXPECTED q; `linear` marks the rows on which that is the expectation of the sampled gradient: both threshold gates open
on every legal action and a clip that no sample can reach (`sample_bound`)."""
import functools
import json
import os
import re
import types

import numpy as np

import _brref as br
import _crossref as cr
import _learnref as lr
import _regref as rr
from _learnref import HP, SETS, VM, minimum, where  # noqa: F401
from _regref import ALL_TREES  # noqa: F401

U = 2.0 ** -24
N_MAX = 32
CHUNK = 4096
BEHAVIOURS = ("on_policy", "softmax", "zeros")
VARIANTS = ("rho_c", "no_lambda", "opp_entropy_sign", "w1_mean", "gamma_child", "q0_no_cs", "reward_sign", "no_chance")
OUTPUTS = ("target", "target_given_row", "q", "reach")


def size(S, n):
    return S * n if S >= 2 and 1 <= n <= 32 else -1


def workspace(S, A, n):
    return S * n * (3 * A + 5) if S >= 2 and 1 <= n <= 32 and 1 <= A <= 8 else -1


def hyper_of(hp):
    """(eta, gamma, lambda, rho, c) of a hyperparameter set, the row of the kernel's `hyper`."""
    return (hp.eta, hp.gamma, hp.lambda_, hp.rho, hp.c)


def to_sides(x, S):
    """A learner-layout row table [2S, ...] as the sweeps' [S, 2 ...]: the row player's entries, then the column player's."""
    x = np.asarray(x)
    return np.concatenate([x[:S], x[S:]], axis=1) if x.ndim == 2 else np.stack([x[:S], x[S:]], axis=1)


def to_rows(x, scalar=False):
    """The inverse: [S, 2A] -> [2S, A]; scalar: [S, 2] -> [2S]."""
    x = np.asarray(x)
    A = x.shape[1] // 2
    out = np.concatenate([x[:, :A], x[:, A:]], axis=0)
    return out[:, 0] if scalar else out


def row_inputs(dtype, tables, legal_tab, hp):
    """(pi, pip, lpol) [2S, A] of the learner's five row tables, by the very functions `_learnref.learner` calls (rnad.py:373-382)."""
    legal = np.asarray(legal_tab).astype(dtype)
    pi, log_pi = lr.policy_head(dtype, np.asarray(tables["logit"]), legal)
    _, log_reg = lr.policy_head(dtype, np.asarray(tables["logit_reg"]), legal)
    _, log_reg_ = lr.policy_head(dtype, np.asarray(tables["logit_reg_"]), legal)
    pp, _, _ = lr.process_policy(dtype, pi.v, legal, hp.n_disc, hp.eps)
    pp = np.where(legal.sum(-1, keepdims=True) > 0, pp, dtype(0))  # (a row without a legal action, state 0's: 0 / 0 there)
    lpol = log_pi - (dtype(hp.alpha) * log_reg + dtype(hp.one_minus_alpha) * log_reg_)
    return pi.v, pp, lpol.v


# ---------------------------------------------------------------------------------------------------- the definition
def enumerate_batch(tree, mu_tab, limit=20000):
    """(batch for `_learnref.learner`, prob [B]): every complete episode of the tree once.  mu_tab [2S, A]."""
    index, chance, value = (np.asarray(tree[k]) for k in ("index", "chance", "value"))
    S, C, A, _ = index.shape
    mu_tab = np.asarray(mu_tab)
    episodes = []

    def walk(s, prob, path):
        assert len(episodes) <= limit, "too many episodes for an enumeration"
        for a in range(A):
            if not mu_tab[s, a] > 0:
                continue
            for b in range(A):
                if not mu_tab[S + s, b] > 0:
                    continue
                for t in range(C):
                    p = float(chance[s, t, a, b])
                    if not p > 0:
                        continue
                    nxt = int(index[s, t, a, b])
                    q = prob * float(mu_tab[s, a]) * float(mu_tab[S + s, b]) * p
                    if nxt == 0:
                        episodes.append((q, path + [(s, a, b, float(value[s, t, a, b]))]))
                    else:
                        walk(nxt, q, path + [(s, a, b, 0.0)])

    walk(1, 1.0, [])
    B, T = len(episodes), 2 * max(len(p) for _, p in episodes)
    prob = np.array([q for q, _ in episodes])
    assert abs(prob.sum() - 1) < 1e-12, "mu or the chance is not a distribution (to fp64) somewhere on the way"
    indices, actions, rewards = np.zeros((T, B), np.int32), np.zeros((T, B), np.int32), np.zeros((T, B))
    for lane, (_, path) in enumerate(episodes):
        for j, (s, a, b, r) in enumerate(path):
            indices[2 * j, lane] = indices[2 * j + 1, lane] = s
            actions[2 * j, lane], actions[2 * j + 1, lane] = a, b
            rewards[2 * j + 1, lane] = r  # the column step makes the transition and is paid
    legal_tab = lr.legal_table(np.asarray(tree["legal"]))
    rows = (np.arange(T) & 1)[:, None] * S + indices
    batch = dict(indices=indices, legal=np.where((indices != 0)[..., None], legal_tab[rows], 0.0), actions=actions, rewards=rewards,
                 mu=np.where((indices != 0)[..., None], mu_tab[rows], 0.0).astype(np.float64), S=S)
    return batch, prob


def enumeration(tree, mu_tab, tables, hp):
    """The definition: a namespace of reach [S], target [2S], q [2S, A], dv_sum [2S], dlogit_sum [2S, A], episodes."""
    batch, prob = enumerate_batch(tree, mu_tab)
    out = lr.learner(np.float64, batch, tables, hp)
    idx = batch["indices"]
    T, B = idx.shape
    S = batch["S"]
    A = batch["mu"].shape[-1]
    valid = idx != 0
    rows = ((np.arange(T) & 1)[:, None] * S + idx)[valid]
    w = np.broadcast_to(prob[None, :], (T, B))[valid]
    visits = np.zeros(2 * S)
    np.add.at(visits, rows, w)
    assert np.array_equal(visits[:S] > 0, visits[S:] > 0) and np.allclose(visits[:S], visits[S:], rtol=1e-13, atol=0)
    turn = out.turn
    vt = np.where(turn == 0, out.v_target.v[0], out.v_target.v[1])[valid]
    qq = np.where((turn == 0)[..., None], out.q.v[0], out.q.v[1])[valid]
    norm = out.norm[turn][valid]
    target, q, dv, dl = np.zeros(2 * S), np.zeros((2 * S, A)), np.zeros(2 * S), np.zeros((2 * S, A))
    np.add.at(target, rows, w * vt)
    np.add.at(q, rows, w[:, None] * qq)
    np.add.at(dv, rows, w * norm * out.dv.v[valid])
    np.add.at(dl, rows, (w * norm)[:, None] * out.dlogit.v[valid])
    seen = visits > 0
    target[seen] /= visits[seen]
    q[seen] /= visits[seen][:, None]
    return types.SimpleNamespace(reach=visits[:S], target=target, q=q, dv_sum=dv, dlogit_sum=dl, episodes=B)


# ---------------------------------------------------------------------------------------------------- the sweep
class _Store:
    """VM arrays addressed by state."""

    def __init__(self, shape, dtype):
        self.v, self.m = np.zeros(shape, dtype), np.zeros(shape, dtype)

    def __getitem__(self, i):
        return VM(self.v[i], self.m[i])

    def __setitem__(self, i, x):
        self.v[i], self.m[i] = x.v, x.m


def _stack(xs, axis=-1):
    return VM(np.stack([x.v for x in xs], axis), np.stack([x.m for x in xs], axis))


def reference(dtype, tree_arrays, MU, PIP, LPOL, VV, hyper, variant=None):
    """A namespace of VM target [S, n, 2], W1 [S, n, A] (target_given_row), q [S, n, 2A] and R [S, n] in `dtype`; h, depth int [S]
    (depth -1: not reached); w [list of fp64 arrays]: the importance weights cs0 cs1 met on the way (the clips' coverage).
    MU, PIP, LPOL [S, n, 2A], VV [S, n, 2], hyper [n, 5] = (eta, gamma, lambda, rho, c), rounded to fp32 as the kernel's arguments are.
    variant: None or one of VARIANTS, a deliberately wrong program."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    S, C, A, _ = index.shape
    MU, PIP, LPOL, VV = (np.asarray(x).astype(dtype) for x in (MU, PIP, LPOL, VV))
    n = MU.shape[1]
    assert MU.shape == PIP.shape == LPOL.shape == (S, n, 2 * A) and VV.shape == (S, n, 2)
    hy = np.asarray(hyper, np.float32).astype(dtype).reshape(n, 5)
    eta, g, lam, rho, cb = (VM(hy[None, :, i]) for i in range(5))
    if variant == "rho_c":
        rho, cb = cb, rho
    if variant == "no_lambda":
        lam = VM(np.ones_like(lam.v))
    ge, gg, lgg = g * eta, g * g, (lam * g) * g
    g_child = VM(np.ones_like(g.v)) if variant == "gamma_child" else g
    gg_child = g if variant == "gamma_child" else gg
    ge_opp = -ge if variant == "opp_entropy_sign" else ge
    zero = dtype(0)
    W0, P1, E0 = _Store((S, n), dtype), _Store((S, n), dtype), _Store((S, n), dtype)
    WA, CS0, W1, Q = _Store((S, n, A), dtype), _Store((S, n, A), dtype), _Store((S, n, A), dtype), _Store((S, n, 2 * A), dtype)
    TG = _Store((S, n, 2), dtype)
    h, depth, ws = np.zeros((S,), np.int64), np.full((S,), -1, np.int64), []
    levels = cr.level_order(index, chance)
    for d, states in enumerate(levels):
        depth[states] = d
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for level in reversed(levels):
            for lo in range(0, level.size, CHUNK):
                st = level[lo:lo + CHUNK]
                m = st.size
                idx, live_all = index[st], chance[st] > 0
                nxt_all = np.where(live_all, idx, 0)
                h[st] = 1 + np.where(nxt_all != 0, h[nxt_all], 0).reshape(m, -1).max(axis=1)
                side = lambda X, k: [VM(X[st][:, :, k * A + a]) for a in range(A)]  # noqa: E731
                mu0, mu1, pip0, pip1, lp0, lp1 = side(MU, 0), side(MU, 1), side(PIP, 0), side(PIP, 1), side(LPOL, 0), side(LPOL, 1)
                vv0, vv1 = VM(VV[st][:, :, 0]), VM(VV[st][:, :, 1])
                blank = VM(np.zeros((m, n), dtype))
                e0 = e1 = blank
                cs0, cs1 = [], []
                for a in range(A):
                    e0 = where(pip0[a].v > 0, e0 + pip0[a] * lp0[a], e0)
                    e1 = where(pip1[a].v > 0, e1 + pip1[a] * lp1[a], e1)
                    cs0.append(where(mu0[a].v > 0, pip0[a] / VM(np.where(mu0[a].v > 0, mu0[a].v, 1)), zero))
                    cs1.append(where(mu1[a].v > 0, pip1[a] / VM(np.where(mu1[a].v > 0, mu1[a].v, 1)), zero))
                base0 = (ge_opp * e1 - eta * e0) - vv0
                acc, qa0, qa1, wa = blank, [blank] * A, [blank] * A, [blank] * A
                for a in range(A):
                    for b in range(A):
                        leave_clip = minimum(cs1[b], rho)
                        xr = yr = zr = xc = zc = blank
                        for t in range(C):
                            live, nxt = live_all[:, t, a, b][:, None], nxt_all[:, t, a, b]
                            leaves = (nxt == 0)[:, None]
                            p = VM(np.where(live, 1, chance[st, t, a, b][:, None]).astype(dtype)) if variant == "no_chance" else \
                                VM(chance[st, t, a, b][:, None])
                            r = VM(value[st, t, a, b][:, None])
                            f_vv0, f_w0 = VM(VV[nxt][:, :, 0]), W0[nxt]
                            tx = where(leaves, r, g_child * f_vv0)
                            ux = where(leaves, zero, f_w0 - f_vv0)
                            zx = where(leaves, r, g_child * f_w0)
                            xr, yr, zr = where(live, xr + p * tx, xr), where(live, yr + p * ux, yr), where(live, zr + p * zx, zr)
                            f_vv1, e0n, p1n = VM(VV[nxt][:, :, 1]), E0[nxt], P1[nxt]
                            X = ((ge_opp * e0n - eta * e1) + gg_child * f_vv1) - vv1
                            inner = blank
                            wan, cs0n = WA[nxt], CS0[nxt]
                            if variant == "w1_mean":
                                mean = TG[nxt][..., 1] - f_vv1
                            for i in range(A):
                                mi, c0 = VM(MU[nxt][:, :, i]), cs0n[..., i]
                                dd = mean if variant == "w1_mean" else wan[..., i]
                                w = cs1[b] * c0
                                term = minimum(w, rho) * X + lgg * minimum(w, cb) * dd
                                inner = where(mi.v > 0, inner + mi * term, inner)
                            rr_ = r if variant == "reward_sign" else -r
                            tl = leave_clip * ((rr_ - eta * e1) - vv1)
                            tx = where(leaves, tl, inner)
                            zx = where(leaves, rr_, ge_opp * e0n + gg_child * p1n)
                            xc, zc = where(live, xc + p * tx, xc), where(live, zc + p * zx, zc)
                        w = cs0[a] * cs1[b]
                        both = (mu0[a].v > 0) & (mu1[b].v > 0)
                        ws.append(np.where(both, w.v, np.nan).astype(np.float64))
                        term = minimum(w, rho) * (base0 + g * xr) + lgg * minimum(w, cb) * yr
                        acc = where(both, acc + (mu0[a] * mu1[b]) * term, acc)
                        tail_w = mu1[b] if variant == "q0_no_cs" else pip1[b]
                        qa0[a] = where(mu1[b].v > 0, qa0[a] + tail_w * zr, qa0[a])
                        qa1[b] = where(mu0[a].v > 0, qa1[b] + mu0[a] * zc, qa1[b])
                        wa[a] = where(mu1[b].v > 0, wa[a] + mu1[b] * xc, wa[a])
                tgt1 = p1 = blank
                w1, q0, q1 = [], [], []
                for a in range(A):
                    w1.append(vv1 + wa[a])
                    tgt1 = where(mu0[a].v > 0, tgt1 + mu0[a] * w1[a], tgt1)
                    p1 = where(mu0[a].v > 0, p1 + pip0[a] * w1[a], p1)
                    q0.append(where(mu0[a].v > 0, (ge_opp * e1 - eta * lp0[a]) + g * qa0[a], vv0 - eta * lp0[a]))
                    q1.append(where(mu1[a].v > 0, (-(eta * lp1[a])) + qa1[a], vv1 - eta * lp1[a]))
                W0[st], P1[st], E0[st] = vv0 + acc, p1, e0
                WA[st], CS0[st], W1[st] = _stack(wa), _stack(cs0), _stack(w1)
                Q[st] = _stack(q0 + q1)
                TG[st] = _stack([W0[st], tgt1])
    R = br.reference(tree_arrays, MU, dtype=dtype).R
    for a in (TG.v, W1.v, Q.v, R):
        assert a.dtype == dtype
    return types.SimpleNamespace(target=VM(TG.v, TG.m), W1=VM(W1.v, W1.m), q=VM(Q.v, Q.m), R=R, h=h, depth=depth, w=ws)


def gates(tree_arrays, ref):
    """dict of the gates of target [S, n, 2], target_given_row [S, n, A], q [S, n, 2A], reach [S, n] from an fp64 `ref` (module docstring)."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    K = 4 * A + C + 18
    hk = ref.h.astype(np.float64)[:, None, None] * K * U
    gR = (3 * np.maximum(ref.depth, 0) + 1)[:, None] * (U * np.asarray(ref.R, np.float64) + np.where(ref.depth >= 0, 2.0 ** -126, 0.0)[:, None])
    return dict(target=hk * ref.target.m, target_given_row=hk * ref.W1.m, q=hk * ref.q.m, reach=gR)


def share(got, want, g):
    """Largest |got - want| / gate over the elements: 0 where both agree, inf where either is NaN or where the gate is 0 and they differ."""
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        s = np.where(err == 0, 0.0, err / g)
    return float(np.nan_to_num(s, nan=np.inf, posinf=np.inf).max()) if s.size else 0.0


def values_of(ref):
    """dict of the four outputs' plain arrays of a `reference` namespace."""
    return dict(target=ref.target.v, target_given_row=ref.W1.v, q=ref.q.v, reach=ref.R)


def shares(c, got, n=None):
    """dict of the worst share of each gate over the reached states for outputs `got` (a dict keyed as OUTPUTS) against case c restricted
    to its first n members."""
    n = c.n if n is None else n
    R, want = c.reached, values_of(c.ref)
    return {k: share(np.asarray(got[k])[R], want[k][R][:, :n], c.gates[k][R][:, :n]) for k in OUTPUTS}


def clip_coverage(ref, hyper):
    """From the reference alone: the shares of the importance weights met (mu > 0 on both sides) strictly below and above rho and c."""
    hy = np.asarray(hyper, np.float64).reshape(-1, 5)
    w = np.concatenate([x.reshape(-1, x.shape[-1]) for x in ref.w], axis=0)
    ok = ~np.isnan(w)
    out = {}
    for name, col in (("rho", 3), ("c", 4)):
        out[name + "_below"] = float(((w < hy[None, :, col]) & ok).sum() / max(ok.sum(), 1))
        out[name + "_above"] = float(((w > hy[None, :, col]) & ok).sum() / max(ok.sum(), 1))
    return out


# ---------------------------------------------------------------------------------------------------- the row gradients
def sample_bound(tree_arrays, mu_tab, pip, lpol, vv, hp, reached):
    """An upper bound on |q| of any SAMPLED slot of the program, from global maxima over the reached rows: with D the longest episode in
    states, cs <= K = max pip / mu, |e| <= E, |vv| <= V, |r| <= R, a sampled target obeys
        |vt| <= V + rho (eta E (1 + g) + g R + g g V + V) + lambda c g g (|vt below| + V),   D times from |vt| = 0,
    a tail |dr + g is nvt - vv| <= g (eta E + K R) + g g K |vt| + V, and |q| <= V + eta max|lpol| + tail / min mu."""
    S = np.asarray(tree_arrays["index"]).shape[0]
    rows = np.concatenate([reached, reached])
    mu, pip, lpol, vv = (np.asarray(x, np.float64)[rows] for x in (mu_tab, pip, lpol, vv))
    drawn = mu > 0
    if not drawn.any():
        return 0.0
    Kc = float((pip[drawn] / mu[drawn]).max())
    E = float(np.abs((pip * np.where(pip > 0, lpol, 0.0)).sum(-1)).max())
    V, Rm = float(np.abs(vv).max()), float(np.abs(np.asarray(tree_arrays["value"])).max())
    D = len(cr.level_order(tree_arrays["index"], tree_arrays["chance"]))
    g = hp.gamma
    vt = 0.0
    for _ in range(D):
        vt = V + hp.rho * (hp.eta * E * (1 + g) + g * Rm + g * g * V + V) + abs(hp.lambda_) * hp.c * g * g * (vt + V)
    tail = g * (hp.eta * E + Kc * Rm) + g * g * Kc * vt + V
    return V + hp.eta * float(np.abs(np.where(drawn, lpol, 0.0)).max()) + tail / float(mu[drawn].min())


def direction(logit, legal_tab, pip, q, hp):
    """(dlogit [2S, A], gates_open bool [2S]): -w_n times the NeuRD gradient of one slot of a row at the action values q, fp64, and
    whether both threshold gates are open on every legal action of the row."""
    logit, legal, pip, q = (np.asarray(x, np.float64) for x in (logit, legal_tab, pip, q))
    A = logit.shape[-1]
    adv = q - (pip * q).sum(-1, keepdims=True)
    adv = np.clip(adv, -hp.clip, hp.clip)
    l = logit - (logit * legal).sum(-1, keepdims=True) / A
    lo, hi = l > -hp.threshold, l < hp.threshold
    f = np.where(lo, np.minimum(adv, 0), 0) + np.where(hi, np.maximum(adv, 0), 0)
    wgt = legal * f
    grad = wgt - legal * wgt.sum(-1, keepdims=True) / A
    return -hp.w_n * grad, ((lo & hi) | (legal == 0)).all(-1)


def expected_tables(tree_arrays, tables, legal_tab, mu_tab, pip, lpol, hp, target, q, reach):
    """What learn.vtrace.expected_update derives on the host side of the sweep, in fp64: dict of dv_tab [2S] = 2 w_v reach (v - target) / L,
    dlogit_tab [2S, A] = reach direction / L, linear bool [2S], length L, target_bias [2]."""
    S = reach.shape[0]
    reach2 = np.concatenate([reach, reach]).astype(np.float64)
    L = float(reach.astype(np.float64).sum())
    v = np.asarray(tables["v"], np.float64).reshape(2 * S)
    dv = 2 * hp.w_v * reach2 * (v - target) / L
    dl, open_ = direction(tables["logit"], legal_tab, pip, q, hp)
    bound = sample_bound(tree_arrays, mu_tab, pip, lpol, tables["v_target"], hp, reach > 0)
    linear = open_ & (reach2 > 0) & (2 * bound <= hp.clip)
    bias = np.abs(target - np.asarray(tables["v_target"], np.float64).reshape(2 * S)) * reach2
    return dict(dv_tab=dv, dlogit_tab=reach2[:, None] * dl / L, linear=linear, length=L, target_bias=np.array([bias[:S].sum(), bias[S:].sum()]))


# ---------------------------------------------------------------------------------------------------- hand-sized trees for the enumeration
def make_tree(A, C, depth, seed, stop=0.35):
    """A ragged tree in the reference layout (index, chance, value [S, C, A, A], legal [S, 1, A, A]; state 0 absorbing, the root is 1) with
    illegal actions, zero-chance records and episodes that leave the tree at every depth."""
    rng = np.random.default_rng(seed)
    states = [None, 0]  # depth of each state; state 0 is the absorbing one
    recs = {}
    s = 1
    while s < len(states):
        d = states[s]
        rows = rng.random(A) < 0.75
        cols = rng.random(A) < 0.75
        rows[0] = cols[0] = True  # the layout reads a side's legal actions off the other side's action 0 (episode.py:62-68)
        for a in np.flatnonzero(rows):
            for b in np.flatnonzero(cols):
                p = rng.random(C) * (rng.random(C) < 0.7)
                p[rng.integers(C)] += 0.1
                p /= p.sum()
                for t in np.flatnonzero(p > 0):
                    if d + 1 < depth and rng.random() > stop:
                        states.append(d + 1)
                        recs[(s, t, a, b)] = (len(states) - 1, p[t], 0.0)
                    else:
                        recs[(s, t, a, b)] = (0, p[t], rng.uniform(-1, 1))
        recs[("legal", s)] = (rows, cols)
        s += 1
    S = len(states)
    index, chance, value = np.zeros((S, C, A, A), np.int64), np.zeros((S, C, A, A)), np.zeros((S, C, A, A))  # fp64: distributions to 1e-16
    legal = np.zeros((S, 1, A, A), np.float32)
    for key, x in recs.items():
        if key[0] == "legal":
            legal[key[1], 0] = np.outer(x[0], x[1])
        else:
            index[key], chance[key], value[key] = x
    return dict(index=index, chance=chance, value=value, legal=legal)


HAND_TREES = {"a2c2d3": dict(A=2, C=2, depth=3, seed=3, stop=0.2), "a3c2d3": dict(A=3, C=2, depth=3, seed=5, stop=0.55),
              "a2c1d5": dict(A=2, C=1, depth=5, seed=7, stop=0.15), "a4c3d2": dict(A=4, C=3, depth=2, seed=9, stop=0.3)}
# (24, 14, 44 and a handful of states; about a hundred episodes each under a full-support behaviour)


@functools.lru_cache(maxsize=None)
def hand_tree(name):
    return make_tree(**HAND_TREES[name])


def _softmax_rows(rng, legal):
    e = np.where(legal > 0, np.exp(rng.standard_normal(legal.shape)), 0.0)
    return e / np.maximum(e.sum(-1, keepdims=True), 1e-300)


def behaviour_table(kind, rng, legal_tab, pip, dtype=np.float32):
    """mu [2S, A] rounded to `dtype`: `on_policy` = pip; `softmax` a seeded table unrelated to the policy; `zeros` that table with every
    legal action zeroed at which pip is zero, as long as one action stays (so pip > 0 implies mu > 0 everywhere)."""
    if kind == "on_policy":
        return np.asarray(pip, dtype).astype(np.float64)
    mu = _softmax_rows(rng, legal_tab)
    if kind == "zeros":
        keep = np.where((np.asarray(pip) > 0) | (np.asarray(pip).sum(-1, keepdims=True) == 0), mu, 0.0)
        mu = keep / np.maximum(keep.sum(-1, keepdims=True), 1e-300)
    return mu.astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def hand_case(name, hp_name, kind):
    """One member on a hand-sized tree: tree, hp, tables (fp64 row tables), legal_tab, mu_tab, pip, lpol [2S, A] fp64, S."""
    tree, hp = hand_tree(name), HP[hp_name]
    S = tree["index"].shape[0]
    rng = np.random.default_rng([sorted(HAND_TREES).index(name), SETS.index(hp_name), BEHAVIOURS.index(kind)])
    legal_tab = lr.legal_table(tree["legal"])
    tables = {k: np.asarray(v, np.float64) for k, v in lr.draw_tables(rng, legal_tab, hp).items()}
    _, pip, lpol = row_inputs(np.float64, tables, legal_tab, hp)
    mu_tab = behaviour_table(kind, rng, legal_tab, pip, np.float64)  # a distribution to 1e-16, as the enumeration needs
    return types.SimpleNamespace(tree=tree, hp=hp, tables=tables, legal_tab=legal_tab, mu_tab=mu_tab, pip=pip, lpol=lpol, S=S)


def sweep_of(c, hp=None, dtype=np.float64, variant=None):
    """`reference` for the single member of a hand case."""
    hp = c.hp if hp is None else hp
    S = c.S
    return reference(dtype, c.tree, to_sides(c.mu_tab, S)[:, None], to_sides(c.pip, S)[:, None], to_sides(c.lpol, S)[:, None],
                     to_sides(c.tables["v_target"], S)[:, None], [hyper_of(hp)], variant=variant)


# ---------------------------------------------------------------------------------------------------- inputs of the GPU sweep
def member(k):
    """(hyperparameter set, behaviour) of member k."""
    return SETS[k % len(SETS)], BEHAVIOURS[k % len(BEHAVIOURS)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(MU, PIP, LPOL [S, 32, 2A], VV [S, 32, 2], hyper [32, 5]) fp32 of a tree of _regref.ALL_TREES, read-only.  Member k draws its own
    five row tables; pip and lpol are computed from them in fp64 and rounded (pip is a multiple of 1 / n_disc: exact)."""
    tree = rr.tree_arrays(name)
    S = np.asarray(tree["index"]).shape[0]
    legal_tab = lr.legal_table(np.asarray(tree["legal"]))
    cols = [[], [], [], []]
    for k in range(N_MAX):
        hp_name, kind = member(k)
        hp = HP[hp_name]
        rng = np.random.default_rng([ALL_TREES.index(name), k])
        tables = lr.draw_tables(rng, legal_tab, hp)
        _, pip, lpol = row_inputs(np.float64, tables, legal_tab, hp)
        mu = behaviour_table(kind, rng, legal_tab, pip)
        for col, x in zip(cols, (mu, pip, lpol, tables["v_target"])):
            col.append(to_sides(x, S).astype(np.float32))
    MU, PIP, LPOL, VV = (np.ascontiguousarray(np.stack(c, axis=1)) for c in cols)
    hyper = np.asarray([hyper_of(HP[member(k)[0]]) for k in range(N_MAX)], np.float32)
    for a in (MU, PIP, LPOL, VV, hyper):
        a.setflags(write=False)
    return MU, PIP, LPOL, VV, hyper


@functools.lru_cache(maxsize=None)
def case(name):
    """A namespace of one tree's case for all 32 members, computed once and read-only: tree, MU, PIP, LPOL, VV, hyper, ref (fp64), gates,
    reached bool [S], n = 32.  The case of n members is the slice [:, :n] of everything."""
    tree = rr.tree_arrays(name)
    MU, PIP, LPOL, VV, hyper = inputs(name)
    ref = reference(np.float64, tree, MU, PIP, LPOL, VV, hyper)
    g = gates(tree, ref)
    for a in tuple(g.values()) + (ref.target.v, ref.W1.v, ref.q.v, ref.R):
        a.setflags(write=False)
    return types.SimpleNamespace(tree=tree, MU=MU, PIP=PIP, LPOL=LPOL, VV=VV, hyper=hyper, ref=ref, gates=g, reached=ref.depth >= 0, n=N_MAX)


# ---------------------------------------------------------------------------------------------------- figures and the built kernels
COMMITTED_ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "profiles", "vtrace_expect_errors.json")
_KERNEL = re.compile(r"k_vtrace_expectILi(\d+)EE")


def update_errors_file(key, figures):
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "vtrace_expect_errors.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def kernel_metadata(so_path):
    """{A: dict(scratch, vgpr, sgpr, lds)} of every k_vtrace_expect instantiation in the built library, read as
    _regevalref.kernel_metadata reads k_reg_evaluate's: .hip_fatbin -> its offload bundles -> the gfx950 code object -> the
    amdhsa.kernels note."""
    import subprocess
    import tempfile

    tools = {t: os.path.join(rr.LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    kernels = []
    with tempfile.TemporaryDirectory(prefix="vtexp_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(rr._BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_vtrace_expect" not in part:
                continue
            bundle, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(bundle, "wb").write(part)
            subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={bundle}", f"--output={co}"])
            cur = None
            for line in subprocess.check_output([tools["llvm-readobj"], "--notes", co], text=True).splitlines():
                m = re.match(r"^\s{2}(?:- |\s{2})(\.\w+):\s*(.*)$", line)
                if not m:
                    continue
                if line.lstrip().startswith("- "):
                    cur = {}
                    kernels.append(cur)
                if cur is not None:
                    cur[m.group(1)] = m.group(2).strip().strip("'\"")
    table = {}
    for k in kernels:
        m = _KERNEL.search(k.get(".name", ""))
        if m:
            table[int(m.group(1))] = dict(scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"]), sgpr=int(k[".sgpr_count"]),
                                          lds=int(k.get(".group_segment_fixed_size", 0)))
    return table
