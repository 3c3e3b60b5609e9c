"""fp64 reference, derived gates and inputs for exact evaluation in the regularised game (csrc/reg_evaluate.hip, rnad_hip.reg_evaluate,
learn.tabular.evaluate_regularized, learn.tabular.TabularNeuRD).

For member k (policy pi = J[:, k], log magnet lm = L[:, k], eta_k > 0), bottom-up over `_crossref.level_order`, V[0] = 0:

    Qm[s,r,c]   = sum_t chance[s,t,r,c] * (index == 0 ? value[s,t,r,c] : V[index, k])          records with chance <= 0 skipped
    q[s,k,r]    = sum_c Qm[s,r,c] * pi[s, A + c]                 q[s,k,A + c] = - sum_r pi[s, r] * Qm[s,r,c]
    KL_side     = sum over a with pi > 0 of pi[a] * (log pi[a] - lm[a])
    V[s,k]      = sum_r pi[s,r] * q[s,k,r] - eta_k * KL_row + eta_k * KL_col
    RES[s,k]    = max over both sides and the side's support (legal, lm > -inf) of |pi(a) - softmax(lm + q / eta_k)(a)|
    R[1,k] = 1,  R[u,k] = R[s,k] * (pi[s,r] * pi[s,A+c]) * chance                              for every live link (s,t,r,c) -> u

`reference` keeps the kernel's order of operations (t ascending inside a joint action, the other side's action ascending, actions ascending
in every sum over a side, (game - eta KL_row) + eta KL_col), so `reference(..., dtype=np.float32)` restates the kernel (numpy's exp and
log stand in for the device's).

The gates are derived, not measured; u = 2^-24, h[s] the height of s (1 where no record leads to a child).

q.  As in _brref.py a term of q meets at most A + C roundings at its own level, each at most u of a partial sum that the sum of the
absolute terms Bq[s,k,a] bounds (the same recursion on |value|, with Bv below in place of a child's value); + 2 pays for second order.
V.  A term of the game part sum_r pi q meets those A + C, its product with pi, at most A - 1 sums and the two final sums: 2A + C + 2.
A term of a KL sum meets the logarithm (accurate to 1 ulp = 2u), the difference, the product with pi, at most A - 1 sums, the product
with eta and the two final sums: A + 6.  The logarithm's error and the rounding of the difference are relative to |log pi| and |lm| each,
NOT to their difference -- at pi = mu the difference cancels and the errors do not --, so the absolute-term sum of a KL side is
K = sum_a pi (|log pi| + |lm|) >= sum_a pi |log pi - lm|, and
    Bv[s,k] = sum_r pi[r] Bq[r] + eta (K_row + K_col) >= |V[s,k]|.
With KV = max(2A + C + 4, A + 8) (+ 2 for second order in both counts) one level adds at most KV u Bv.  A child's error enters with the
weight chance * pi * pi of its term and Bv[child] enters Bv[s] with the same weight, so by induction over the height
    |got V - V| <= h[s] KV u Bv[s,k]                  |got q - q| <= ((A + C + 2) + (h[s] - 1) KV) u Bq[s,k,a].
RES.  The exponent t = lm + q / eta carries the error of q divided by eta, and its own roundings (1 / eta, the product, the sum, the
subtraction of the maximum: at most 5u of T = max_a (|lm| + Bq / eta), the last being relative to |t - max| <= 2T).  A softmax is
1-Lipschitz in the sup norm, so that is an error of at most delta = max_a gate(q[a]) / eta + 5 u T in a probability; the softmax itself
adds exp (1 ulp = 2u), at most A - 1 sums, the division and the difference from pi, all relative to numbers <= 1, + 2 for second order:
    |got RES - RES| <= max over the two sides of delta + (A + 6) u.
R.  _brref's: every factor is nonnegative, three products per level: |got R - R| <= (3 depth[s] + 1) u R[s,k].  That bound is relative and
holds for normal numbers only.  The fixed-point policies below hold probabilities of e^-40 and less, and their reach falls under the
smallest normal fp32 number, 2^-126: there a product is rounded to a multiple of 2^-149, or flushed to zero where a device does that --
an absolute error of at most 2^-126 per product, which is added: (3 depth[s] + 1) (u R[s,k] + 2^-126).

Inputs (`case`): member k takes eta = ETAS[k % 3], the magnet MAGNETS[k % 4] of _regref at that eta and policy POLICIES[k % 5], built ON
THE MAGNET'S SUPPORT (legal and lm > -inf; for three of the four magnets that is every legal action, the "solution" magnet has zeros):
uniform over it, a seeded softmax, the tree's solution mixed 0.99 / 0.01 with that uniform, a one-hot table (zeros inside the support), and
the fp64 fixed point of the magnet rounded to fp32.  So pi = 0 wherever lm = -inf at every state: the absolute-continuity condition,
asserted in tests/test_reg_evaluate.py.  The 32 members are independent: the case of n members is the first n of the 32.
"""
import functools
import json
import os
import re
import types

import numpy as np

import _brref as br  # noqa: F401  (tests compare the reach with br.reference through this module)
import _crossref as cr
import _regref as rr
from _regref import ALL_TREES, ETAS, MAGNETS, legal_mask, levels_of, magnet, solve  # noqa: F401  (what the tests import from here)

U = 2.0 ** -24
POLICIES = ("uniform", "softmax", "solution_mix", "one_hot", "fixed_point")
VARIANTS = ("col_kl_sign", "reverse_kl", "no_opp_kl", "q_own_side", "no_chance_q", "reach_no_chance", "log_residual", "log_underflow")
N_MAX = 32
CHUNK = 4096


def size(S, n):
    """rnad_reg_evaluate_size restated: floats of `values` (and of residual, reach)."""
    return S * n if S >= 2 and 1 <= n <= 32 else -1


def _seq(x, axis=-1):
    """sum in index order along `axis` (what an unrolled loop does)."""
    x = np.moveaxis(x, axis, 0)
    s = np.zeros_like(x[0])
    for a in range(x.shape[0]):
        s = s + x[a]
    return s


def _side_softmax_residual(p, lm, q, on, inv_eta, dtype, log_space=False):
    """[m, n]: max over the support of |p - softmax(lm + q * inv_eta)|, in reg_solve.hip's residual_of order."""
    t = (np.where(on, lm, 0).astype(dtype) + (q * inv_eta).astype(dtype)).astype(dtype)
    top = np.where(on, t, -np.inf).max(axis=-1, keepdims=True)
    top = np.where(np.isfinite(top), top, 0).astype(dtype)
    e = np.where(on, np.exp(np.where(on, t - top, 0).astype(dtype)), 0).astype(dtype)
    tot = _seq(e)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = (e / tot).astype(dtype)
        if log_space:
            d = np.where(on & (p > 0), np.abs(np.log(np.where(p > 0, p, 1)) - np.log(np.where(sm > 0, sm, 1))), 0)
        else:
            d = np.where(on, np.abs(p - sm), 0)
    return d.max(axis=-1).astype(dtype)


def reference(tree_arrays, J, L, etas, dtype=np.float64, variant=None, round_eta=True):
    """A namespace of V, RES, R [S, n]; Q [S, n, 2A] in `dtype`; fp64 bounds Bq [S, n, 2A], Bv, K (both sides' KL absolute-term sums,
    [S, n, 2]), KL [S, n, 2], T [S, n, 2], imm [S, n] (the expected terminal payoff collected at s); h, depth int [S] (depth -1: not
    reached); on bool [S, n, 2A].  variant: None or one of VARIANTS, a deliberately wrong program.  round_eta: eta goes through fp32 first, as
    the kernel's arguments do (False: an fp64 computation that has nothing to do with the kernel, such as _regref.solve's)."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    S, C, A, _ = index.shape
    J = np.asarray(J).astype(dtype)
    L = np.asarray(L).astype(dtype)
    n = J.shape[1]
    assert J.shape == (S, n, 2 * A) and L.shape == J.shape
    eta = (np.asarray(etas, np.float32) if round_eta else np.asarray(etas, np.float64)).astype(dtype)
    assert eta.shape == (n,)
    inv_eta = (dtype(1) / eta).astype(dtype)
    on = legal_mask(tree_arrays)[:, None, :] & (L > -np.inf)
    out = types.SimpleNamespace(
        V=np.zeros((S, n), dtype), RES=np.zeros((S, n), dtype), R=np.zeros((S, n), dtype), Q=np.zeros((S, n, 2 * A), dtype),
        Bq=np.zeros((S, n, 2 * A)), Bv=np.zeros((S, n)), K=np.zeros((S, n, 2)), KL=np.zeros((S, n, 2)), T=np.zeros((S, n, 2)),
        imm=np.zeros((S, n)), h=np.zeros((S,), np.int64), depth=np.full((S,), -1, np.int64), on=on)
    levels = cr.level_order(index, chance)
    for d, states in enumerate(levels):
        out.depth[states] = d
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for level in reversed(levels):
            for lo in range(0, level.size, CHUNK):
                st = level[lo:lo + CHUNK]
                m = st.size
                idx, live, val, w = index[st], chance[st] > 0, value[st], chance[st]
                nxt = np.where(live, idx, 0)
                term = nxt == 0
                out.h[st] = 1 + np.where(live & ~term, out.h[idx], 0).reshape(m, -1).max(axis=1)
                wq = np.where(live, dtype(1), w) if variant == "no_chance_q" else w
                Qm = np.zeros((m, A, A, n), dtype)
                BQ = np.zeros((m, A, A, n))
                Tm = np.zeros((m, A, A))
                for t in range(C):
                    x = np.where(term[:, t, :, :, None], val[:, t][..., None], out.V[nxt[:, t]])
                    Qm = np.where(live[:, t, :, :, None], Qm + (x * wq[:, t, :, :, None]).astype(dtype), Qm)
                    bx = np.where(term[:, t, :, :, None], np.abs(val[:, t]).astype(np.float64)[..., None], out.Bv[nxt[:, t]])
                    BQ = BQ + np.where(live[:, t, :, :, None], bx * w[:, t, :, :, None].astype(np.float64), 0.0)
                    Tm = Tm + np.where(live[:, t] & term[:, t], val[:, t].astype(np.float64) * w[:, t].astype(np.float64), 0.0)
                pr, pc = J[st, :, :A], J[st, :, A:]                                    # [m, n, A]
                opp_r, opp_c = (pr, pc) if variant == "q_own_side" else (pc, pr)       # what the row / column player answers
                qr, qc = np.zeros((m, n, A), dtype), np.zeros((m, n, A), dtype)
                bqr, bqc = np.zeros((m, n, A)), np.zeros((m, n, A))
                for j in range(A):  # the other side's action, ascending
                    qr = qr + (Qm[:, :, j, :].transpose(0, 2, 1) * opp_r[:, :, j, None]).astype(dtype)
                    qc = qc + (Qm[:, j, :, :].transpose(0, 2, 1) * opp_c[:, :, j, None]).astype(dtype)
                    bqr = bqr + BQ[:, :, j, :].transpose(0, 2, 1) * pc[:, :, j, None].astype(np.float64)
                    bqc = bqc + BQ[:, j, :, :].transpose(0, 2, 1) * pr[:, :, j, None].astype(np.float64)
                qc = -qc
                game = _seq((pr * qr).astype(dtype))
                kl, kabs = [], []
                for p, lm in ((pr, L[st, :, :A]), (pc, L[st, :, A:])):
                    played = p > 0
                    if variant == "log_underflow":
                        terms = (p * (np.log(p) - lm).astype(dtype)).astype(dtype)        # 0 * (-inf - lm): NaN where pi = 0
                        played = np.ones_like(played)
                    elif variant == "reverse_kl":
                        mu = np.where(lm > -np.inf, np.exp(lm), 0).astype(dtype)
                        terms = (mu * (np.where(played, lm, 0) - np.log(np.where(played, p, 1))).astype(dtype)).astype(dtype)
                    else:
                        terms = (p * (np.log(np.where(played, p, 1)).astype(dtype) - lm).astype(dtype)).astype(dtype)
                    acc = np.zeros((m, n), dtype)
                    for a in range(A):
                        acc = np.where(played[:, :, a], acc + terms[:, :, a], acc)
                    kl.append(acc)
                    p64, lm64 = p.astype(np.float64), lm.astype(np.float64)
                    kabs.append(np.where(p > 0, p64 * (np.abs(np.log(np.where(p > 0, p64, 1.0))) + np.abs(np.where(p > 0, lm64, 0.0))), 0.0).sum(axis=2))
                e = eta[None, :]
                if variant == "col_kl_sign":
                    v = ((game - (e * kl[0]).astype(dtype)).astype(dtype) - (e * kl[1]).astype(dtype)).astype(dtype)
                elif variant == "no_opp_kl":
                    v = (game - (e * kl[0]).astype(dtype)).astype(dtype)
                else:
                    v = ((game - (e * kl[0]).astype(dtype)).astype(dtype) + (e * kl[1]).astype(dtype)).astype(dtype)
                log_space = variant == "log_residual"
                res = np.maximum(_side_softmax_residual(pr, L[st, :, :A], qr, on[st, :, :A], inv_eta[None, :, None], dtype, log_space),
                                 _side_softmax_residual(pc, L[st, :, A:], qc, on[st, :, A:], inv_eta[None, :, None], dtype, log_space))
                out.V[st], out.RES[st] = v, res
                out.Q[st] = np.concatenate([qr, qc], axis=2)
                out.Bq[st] = np.concatenate([bqr, bqc], axis=2)
                out.K[st] = np.stack(kabs, axis=2)
                out.KL[st] = np.stack(kl, axis=2).astype(np.float64)
                eta64 = eta.astype(np.float64)[None, :]
                out.Bv[st] = (pr.astype(np.float64) * bqr).sum(axis=2) + eta64 * (kabs[0] + kabs[1])
                lm_abs = np.where(on[st], np.abs(np.where(on[st], L[st], 0)).astype(np.float64), 0.0) + out.Bq[st] / eta64[..., None]
                lm_abs = np.where(on[st], lm_abs, 0.0)
                out.T[st] = np.stack([lm_abs[:, :, :A].max(axis=2), lm_abs[:, :, A:].max(axis=2)], axis=2)
                out.imm[st] = np.einsum("mnr,mrc,mnc->mn", pr.astype(np.float64), Tm, pc.astype(np.float64))
    out.R[1] = 1
    rows, cols = J[:, :, :A], J[:, :, A:]
    for level in levels:  # _brref.reference's top-down loop, operation by operation
        idx, link = index[level], (index[level] != 0) & (chance[level] > 0)
        m_pos, t_, r_, c_ = np.nonzero(link)
        if m_pos.size == 0:
            continue
        s_ = level[m_pos]
        child = idx[m_pos, t_, r_, c_]
        joint = rows[s_, :, r_] * cols[s_, :, c_]
        through = (out.R[s_] * joint.astype(dtype)).astype(dtype)
        out.R[child] = through if variant == "reach_no_chance" else (through * chance[s_, t_, r_, c_][:, None]).astype(dtype)
    for a in (out.V, out.RES, out.R, out.Q):
        assert a.dtype == dtype
    return out


def gates(tree_arrays, ref, etas):
    """(gate of V [S, n], of q [S, n, 2A], of RES [S, n], of R [S, n]): the bounds of the module docstring, from an fp64 `ref`."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    eta = np.asarray(etas, np.float32).astype(np.float64)[None, :]
    KV = max(2 * A + C + 4, A + 8)
    h = ref.h.astype(np.float64)
    gV = (h * KV * U)[:, None] * ref.Bv
    gQ = (((A + C + 2) + (h - 1) * KV) * U)[:, None, None] * ref.Bq
    worst = np.where(ref.on, gQ, 0.0)
    delta = np.stack([worst[:, :, :A].max(axis=2), worst[:, :, A:].max(axis=2)], axis=2) / eta[..., None] + 5 * U * ref.T
    gRES = delta.max(axis=2) + (A + 6) * U
    gR = (3 * np.maximum(ref.depth, 0) + 1)[:, None] * (U * np.asarray(ref.R, np.float64) + np.where(ref.depth >= 0, 2.0 ** -126, 0.0)[:, None])
    return gV, gQ, gRES, gR


def share(got, want, g):
    """Largest |got - want| / gate over the elements: 0 where both agree, inf where either is NaN or where the gate is 0 and they differ."""
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        s = np.where(err == 0, 0.0, err / g)
    return float(np.nan_to_num(s, nan=np.inf, posinf=np.inf).max())


def shares(c, got, n=None):
    """dict of the worst share of each gate over the reached states for outputs `got` (a namespace of V, Q, RES, R, or arrays keyed the
    same) against case c restricted to its first n members."""
    n = c.n if n is None else n
    R = c.reached
    return dict(values=share(got.V[R], c.ref.V[R, :n], c.gV[R, :n]), q=share(got.Q[R], c.ref.Q[R, :n], c.gQ[R, :n]),
                residual=share(got.RES[R], c.ref.RES[R, :n], c.gRES[R, :n]), reach=share(got.R[R], c.ref.R[R, :n], c.gR[R, :n]))


# ---------------------------------------------------------------------------------------------------- inputs
def member(k):
    """(eta, magnet kind, policy kind) of member k."""
    return ETAS[k % len(ETAS)], MAGNETS[k % len(MAGNETS)], POLICIES[k % len(POLICIES)]


def _per_side(x, A, fn):
    return np.concatenate([fn(x[:, :A]), fn(x[:, A:])], axis=1)


def policy_table(name, k):
    """fp32 [S, 2A]: member k's policy, on the support of member k's magnet."""
    eta, kind, pol = member(k)
    tree = rr.tree_arrays(name)
    lm = magnet(name, kind, eta)
    sup = legal_mask(tree) & (lm > -np.inf)
    S, A2 = sup.shape
    A = A2 // 2
    count = _per_side(sup, A, lambda h: np.repeat(h.sum(1, keepdims=True), A, 1))
    uniform = sup / np.maximum(count, 1)
    if pol == "uniform":
        out = uniform
    elif pol == "softmax":
        z = np.where(sup, np.exp(2.0 * np.random.default_rng(100 + k).standard_normal((S, A2))), 0.0)
        out = z / np.maximum(_per_side(z, A, lambda h: np.repeat(h.sum(1, keepdims=True), A, 1)), 1e-300)
    elif pol == "solution_mix":
        sol = np.where(sup, np.asarray(tree["solution"], np.float64), 0.0)
        tot = _per_side(sol, A, lambda h: np.repeat(h.sum(1, keepdims=True), A, 1))
        sol = np.where(tot > 0, sol / np.where(tot > 0, tot, 1), uniform)  # (a side whose solution lies outside the support: uniform)
        out = 0.99 * sol + 0.01 * uniform
    elif pol == "one_hot":
        first = _per_side(sup, A, lambda h: (np.cumsum(h, axis=1) == 1) & h)
        out = first.astype(np.float64)
    else:
        out = np.where(sup, rr.star(name, kind, eta)["policy"], 0.0)
    return np.where(sup, out, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(J [S, 32, 2A] fp32, L [S, 32, 2A] fp32, etas [32] fp32) of a tree, read-only."""
    J = np.ascontiguousarray(np.stack([policy_table(name, k) for k in range(N_MAX)], axis=1))
    L = np.ascontiguousarray(np.stack([magnet(name, member(k)[1], member(k)[0]) for k in range(N_MAX)], axis=1)).astype(np.float32)
    etas = np.asarray([member(k)[0] for k in range(N_MAX)], np.float32)
    for a in (J, L, etas):
        a.setflags(write=False)
    return J, L, etas


@functools.lru_cache(maxsize=None)
def case(name):
    """A namespace of one tree's case for all 32 members, computed once and read-only: tree, J, L, etas, ref (fp64), gV, gQ, gRES, gR,
    reached bool [S], n = 32.  The case of n members is the slice [:, :n] of everything."""
    tree = rr.tree_arrays(name)
    J, L, etas = inputs(name)
    ref = reference(tree, J, L, etas)
    gV, gQ, gRES, gR = gates(tree, ref, etas)
    for a in (gV, gQ, gRES, gR) + tuple(v for v in vars(ref).values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return types.SimpleNamespace(tree=tree, J=J, L=L, etas=etas, ref=ref, gV=gV, gQ=gQ, gRES=gRES, gR=gR, reached=ref.depth >= 0, n=N_MAX)


# ---------------------------------------------------------------------------------------------------- the exact NeuRD loop, restated
# lr * eta = 0.04 < 1.  A state's q moves with its opponent and with the values below it, so the step must be small against eta; in fp64
# lr = 0.5 never settles, 0.3 reaches 0.016 after 300 steps and 0.2 reaches 0.0026 (from 0.667 at the uniform magnet), not monotonically.
NEURD = dict(tree="small", eta=0.2, lr=0.2, steps=300)


def _log_softmax_sides(l, A):
    def one(h):
        with np.errstate(invalid="ignore", divide="ignore"):
            top = np.where(np.isfinite(h), h, -np.inf).max(axis=1, keepdims=True)
            top = np.where(np.isfinite(top), top, 0.0)
            return h - (top + np.log(np.maximum(np.exp(h - top).sum(axis=1, keepdims=True), 1e-300)))
    return np.concatenate([one(l[:, :A]), one(l[:, A:])], axis=1)


@functools.lru_cache(maxsize=None)
def neurd_loop(name=NEURD["tree"], eta=NEURD["eta"], lr=NEURD["lr"], steps=NEURD["steps"]):
    """learn.tabular.TabularNeuRD restated in fp64 from the uniform magnet: (max_residual after each step [steps], the residual gate at the
    reached states of the last evaluation (its largest value: the floor of the comparison), max_residual before the first step).  Asserts
    that the loop contracts: the last figure is below a hundredth of the first, and below the figure at half time."""
    tree = rr.tree_arrays(name)
    lm = np.asarray(magnet(name, "uniform", eta), np.float64)
    sup = legal_mask(tree) & (lm > -np.inf)
    A = sup.shape[1] // 2
    l = np.where(sup, lm, -np.inf)
    hist, ref = [], None

    def evaluate(l):
        lp = _log_softmax_sides(l, A)
        pi = np.where(sup, np.exp(np.where(sup, lp, 0.0)), 0.0)
        ref = reference(tree, pi[:, None, :], np.where(sup, lm, -np.inf)[:, None, :], [eta])
        reached = np.asarray(ref.R[:, 0]) > 0
        return lp, pi, ref, float(ref.RES[reached, 0].max())

    lp, pi, ref, first = evaluate(l)
    for _ in range(steps):
        raw = np.where(sup, ref.Q[:, 0] - eta * (np.where(sup, lp, 0.0) - np.where(sup, lm, 0.0)), 0.0)
        mean = np.concatenate([np.repeat((pi[:, :A] * raw[:, :A]).sum(1, keepdims=True), A, 1),
                               np.repeat((pi[:, A:] * raw[:, A:]).sum(1, keepdims=True), A, 1)], axis=1)
        l = np.where(sup, l + lr * np.where(sup, raw - mean, 0.0), -np.inf)
        lp, pi, ref, res = evaluate(l)
        hist.append(res)
    gRES = gates(tree, ref, [eta])[2]
    floor = float(gRES[np.asarray(ref.R[:, 0]) > 0, 0].max())
    assert hist[-1] < 0.01 * first and hist[-1] < hist[len(hist) // 2], (first, hist)
    return tuple(hist), floor, first


# ---------------------------------------------------------------------------------------------------- figures and the built kernels
COMMITTED_ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "profiles", "reg_evaluate_errors.json")
_KERNEL = re.compile(r"k_reg_evaluateILi(\d+)EE")


def update_errors_file(key, figures):
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "reg_evaluate_errors.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def kernel_metadata(so_path):
    """{A: dict(scratch, vgpr, sgpr, lds)} of every k_reg_evaluate instantiation in the built library, read as _regref.kernel_metadata
    reads k_reg_solve's: .hip_fatbin -> its offload bundles -> the gfx950 code object -> the amdhsa.kernels note."""
    import subprocess
    import tempfile

    tools = {t: os.path.join(rr.LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    kernels = []
    with tempfile.TemporaryDirectory(prefix="regeval_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(rr._BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_reg_evaluate" not in part:
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
