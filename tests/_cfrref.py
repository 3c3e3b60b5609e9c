"""fp64 reference, derived gates and inputs for exact CFR on the enumerated tree (csrc/cfr.hip, rnad_hip.cfr_iterate,
learn.tabular.TabularCFR).

One iteration for member k with regrets R = RG[:, k], strategy sums SS[:, k], discounts (dp, dn, da) = discount[k] and side bits
sides[k] (bit 0: the row side updates, bit 1: the column side); every state is its own information set for both players:

    sigma[s,side,a] = R+(a) / sum R+ over the side's legal actions where the sum is > 0, else 1 / (number of legal actions); R+ = max(R, 0)
    reach[1] = (1, 1, 1);  for every live link (s,t,r,c) -> u (chance > 0, index != 0):
        row[u] = row[s] * sigma[s, r]          col[u] = col[s] * sigma[s, A + c]          chn[u] = chn[s] * chance[s,t,r,c]
    Qm[s,r,c] = sum_t chance[s,t,r,c] * (index == 0 ? value[s,t,r,c] : V[index, k])          records with chance <= 0 skipped
    q0[r] = sum_c Qm[r,c] * sigma[A + c]         q1[c] = -(sum_r Qm[r,c] * sigma[r])         V[s,k] = v = sum_r sigma[r] * q0[r]
    for a side whose bit is set, on its legal actions, cf_row = col * chn, cf_col = row * chn, v_row = v, v_col = -v:
        R[a] <- (R[a] > 0 ? dp : dn) * R[a] + cf_side * (q_side[a] - v_side)         SS[a] <- da * SS[a] + own_side * sigma_side[a]

`iterate` keeps the kernel's order of operations (a ascending in sigma's sum, t ascending inside a joint action, the other side's action
ascending in q, r ascending in v, (disc * R) + (cf * (q - v)), (da * SS) + (own * sigma)), so `iterate(..., dtype=np.float32)` restates the
kernel; `iterate(..., np.float64)` is the reference.  `schedule(variant, t)` gives the discounts of iteration t (1-based):

    "cfr"  (1, 1, 1)      "cfr+"  (1, 0, (t-1)/t): CFR+ regrets with the linear average its authors pair them with      "linear"  (1, 1, (t-1)/t)
    ("dcfr", alpha, beta, gamma)  (x^alpha / (x^alpha + 1), x^beta / (x^beta + 1), (x / (x + 1))^gamma) at x = t - 1, the previous t

The gates are derived, not measured; d[s] the depth of s, h[s] its height (1 where no record leads to a child).  Both programs read the
same fp32 regrets, sums, discounts, chances and payoffs, so inputs carry no error and every select (legal, R > 0, sum R+ > 0, the side
bits) falls the same way in both.  Every rounding is budgeted at one ulp, u = 2 * 2^-24, not at the half ulp of round-to-nearest: a
device whose division is faithful but not correctly rounded is still inside, and a correctly rounded program -- the fp32 restatement --
must then stay within HALF of every gate, which tests/test_cfr.py asserts as the check of the counts below.  Half of a gate is K * 2^-24
times the sum of the absolute terms with K counted from the chains, the bound a correctly rounded device must meet, and that half --
DEVICE_SHARE -- is what tests/test_hip_cfr.py asks of the MI355X at every state, and what its slacks are built from.  A result below the normal
range (2^-126) is rounded to a multiple of 2^-149 or flushed to zero; the floor f = 2 * 2^-126 added to the reach, regret and sum gates
pays for that.

sigma.  R+ is exact; the sum over at most A nonnegative terms puts at most A - 1 roundings on each, the division one more: a relative
error of at most A u, gate (A + 1) u sigma with + 1 for second order.  The uniform branch is one division.
reach.  Every factor is nonnegative.  row[s] is a product of d sigmas, each within (A + 1) u relative, and d products:
|got - row| <= (d (A + 2) + 1) u row, col alike; chn has exact factors and d products: (d + 1) u chn.  Those bounds are relative and hold
for normal numbers; below them the floor is added per product: (d (A + 2) + 1) (u row + f), as _regevalref does for its reach.
V.  A term sigma[r] Qm-term sigma[c] of v meets the product with chance and at most C sums (C + 1), the product with sigma[c] and at most
A sums (A + 1), the product with sigma[r] and at most A sums (A + 1), and the two sigmas' own errors (2 (A + 1)): 4A + C + 5 roundings, each
at most u of a partial sum that the sum of the absolute terms bounds, Bv[s,k] = sum sigma sigma chance (|value| or Bv[child]); + 2 pays for
second order: KV = 4A + C + 7.  A child's error enters with the weight of its term and Bv[child] enters Bv[s] with the same weight, so
    |got V - V| <= h[s] KV u Bv[s,k].
q (not an output; it feeds the regret gate).  The same chain without the last product, sums and sigma: KQ = 2A + C + 5 at its own level,
the children's h - 1 levels of KV below: |got q - q| <= (KQ + (h[s] - 1) KV) u Bq[s,k,a], Bq the absolute-term sum of q.
regret.  kept = disc * R is one rounding of an exact product.  cf = opp * chn carries both reach gates and one product:
E_cf = g_opp chn + opp g_chn + u cf.  The difference q - v carries gq + gV and one rounding relative to |q - v| <= Bq + Bv; its product
with cf one more, the final sum one relative to |kept| + cf (Bq + Bv); one more u on the second term for second order:
    |got R - R| <= 2 u |kept| + (E_cf + 4 u cf) (Bq + Bv) + cf (gq + gV) + f.
Where the side's bit is clear or the action is illegal the gate is 0: the entry keeps its bits.
strategy sum.  da * SS is one rounding of an exact product; own * sigma carries the reach gate, sigma's gate and one product; the final
sum one more, + 1 for second order:
    |got SS - SS| <= 2 u |da SS| + g_own sigma + own g_sigma + 3 u own sigma + f.
`regret_gate_sum` is the regret gate summed over the states and a side's actions: what one iteration can move sum_s max_a R+ by.

Inputs (`case`): member k runs variant MEMBERS[k % 4]; its tables are those after PRIOR[k] = (k // 4) % 8 fp64 iterations of that variant
from zero tables, rounded to fp32, so every variant meets 0 .. 7 earlier iterations: after 0 every side has sum R+ = 0, later ones hold
negative regrets, sides that regret matching has driven to a pure action, and states those actions cut off (zero counterfactual reach).
During the earlier iterations the members with ((k // 4) + k) % 2 = 1 alternate (row side on odd t, column side on even t), the others
update both sides.  The compared iteration is t = PRIOR[k] + 1 with sides[k] = (1, 2, 3)[k % 3].  A regret whose magnitude is below 2^-60
after the rounding is set to 0: nonzero R+ stays far above the fp32 denormal range (2^-126), where the relative bounds above would not
hold.  The 32 members are independent: the case of n members is the first n of the 32.
"""
import functools
import json
import os
import re
import types

import numpy as np

import _crossref as cr
import _regref as rr
from _regref import ALL_TREES, legal_mask  # noqa: F401  (what the tests import from here)

U = 2.0 ** -24
ULP = 2 * U
DEVICE_SHARE = 0.5  # of a one-ulp gate: K * 2^-24 * the absolute terms, what the device is held to (the module docstring)
TINY = 2.0 ** -126
MEMBERS = ("cfr", "cfr+", "linear", ("dcfr", 1.5, 0.0, 2.0))
VARIANTS = ("no_chance_cf", "joint_cf", "own_reach_regret", "opp_reach_average", "col_sign", "dp_dn_swapped", "uniform_all_actions",
            "cleared_side_updated")
N_MAX = 32
CHUNK = 4096


def size(S, n):
    """rnad_cfr_size restated: floats of `reach`."""
    return 3 * S * n if S >= 2 and 1 <= n <= 32 else -1


def _ratio(x, e):
    """x^e / (x^e + 1) for an integer x >= 0, with the limits at x = 0 and e = -inf."""
    if x == 0:
        return 0.0 if e > 0 else (0.5 if e == 0 else 1.0)
    p = float(x) ** e
    return p / (p + 1.0)


def schedule(variant, t):
    """(dp, dn, da) of iteration t >= 1 in fp64."""
    t = int(t)
    assert t >= 1
    if variant == "cfr":
        return 1.0, 1.0, 1.0
    if variant == "cfr+":
        return 1.0, 0.0, (t - 1) / t
    if variant == "linear":
        return 1.0, 1.0, (t - 1) / t
    kind, alpha, beta, gamma = variant
    assert kind == "dcfr"
    return _ratio(t - 1, alpha), _ratio(t - 1, beta), ((t - 1) / t) ** gamma


def _seq(x, axis=-1):
    """sum in index order along `axis` (what an unrolled loop does)."""
    x = np.moveaxis(x, axis, 0)
    s = np.zeros_like(x[0])
    for a in range(x.shape[0]):
        s = s + x[a]
    return s


def sigma_of(mask, R, dtype=np.float64, all_actions=False):
    """[S, n, 2A]: regret matching on R [S, n, 2A] per side over the legal actions mask [S, 2A]."""
    A = mask.shape[1] // 2
    R = np.asarray(R).astype(dtype)
    out = np.zeros_like(R)
    for lo in (0, A):
        on = mask[:, None, lo:lo + A]
        plus = np.where(on & (R[:, :, lo:lo + A] > 0), R[:, :, lo:lo + A], dtype(0))
        tot = _seq(plus)[..., None]
        cnt = np.full(on.sum(axis=2, keepdims=True).shape, A) if all_actions else on.sum(axis=2, keepdims=True)
        uniform = (dtype(1) / np.maximum(cnt, 1).astype(dtype)).astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, :, lo:lo + A] = np.where(on, np.where(tot > 0, (plus / np.where(tot > 0, tot, 1)).astype(dtype), uniform), dtype(0))
    return out


def iterate(tree_arrays, R, S, discount, sides, dtype=np.float64, variant=None):
    """One iteration.  R, S [S, n, 2A] (not modified), discount [n, 3], sides [n].  A namespace of RG, SS [S, n, 2A] (the updated tables),
    P [S, n, 2A] (sigma_t), V [S, n], reach [S, 3, n], Q [S, n, 2A] (both sides' q) in `dtype`; fp64 bounds Bv [S, n], Bq [S, n, 2A];
    h, depth int [S] (depth -1: not reached); mask bool [S, 2A].  variant: None or one of VARIANTS, a deliberately wrong program."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    Sn, C, A, _ = index.shape
    R = np.asarray(R).astype(dtype)
    S = np.asarray(S).astype(dtype)
    n = R.shape[1]
    assert R.shape == (Sn, n, 2 * A) and S.shape == R.shape
    disc = np.asarray(discount, np.float32).astype(dtype)
    sides = np.asarray(sides).astype(np.int64)
    assert disc.shape == (n, 3) and sides.shape == (n,)
    dp, dn, da = disc[None, :, 0, None], disc[None, :, 1, None], disc[None, :, 2, None]
    if variant == "dp_dn_swapped":
        dp, dn = dn, dp
    mask = legal_mask(tree_arrays)
    levels = cr.level_order(index, chance)
    out = types.SimpleNamespace(RG=R.copy(), SS=S.copy(), P=np.zeros_like(R), V=np.zeros((Sn, n), dtype), reach=np.zeros((Sn, 3, n), dtype),
                                Q=np.zeros_like(R), Bv=np.zeros((Sn, n)), Bq=np.zeros((Sn, n, 2 * A)), h=np.zeros((Sn,), np.int64),
                                depth=np.full((Sn,), -1, np.int64), mask=mask)
    for d, states in enumerate(levels):
        out.depth[states] = d
    reached = out.depth >= 0
    P = np.where(reached[:, None, None], sigma_of(mask, R, dtype, all_actions=variant == "uniform_all_actions"), dtype(0)).astype(dtype)
    out.P = P
    out.reach[1] = 1
    for level in levels:
        idx, link = index[level], (index[level] != 0) & (chance[level] > 0)
        m_pos, t_, r_, c_ = np.nonzero(link)
        if m_pos.size == 0:
            continue
        s_ = level[m_pos]
        child = idx[m_pos, t_, r_, c_]
        out.reach[child, 0] = (out.reach[s_, 0] * P[s_, :, r_]).astype(dtype)
        out.reach[child, 1] = (out.reach[s_, 1] * P[s_, :, A + c_]).astype(dtype)
        out.reach[child, 2] = (out.reach[s_, 2] * chance[s_, t_, r_, c_][:, None]).astype(dtype)
    for level in reversed(levels):
        for lo in range(0, level.size, CHUNK):
            st = level[lo:lo + CHUNK]
            m = st.size
            idx, live, val, w = index[st], chance[st] > 0, value[st], chance[st]
            nxt = np.where(live, idx, 0)
            term = nxt == 0
            out.h[st] = 1 + np.where(live & ~term, out.h[idx], 0).reshape(m, -1).max(axis=1)
            Qm = np.zeros((m, A, A, n), dtype)
            BQ = np.zeros((m, A, A, n))
            for t in range(C):
                x = np.where(term[:, t, :, :, None], val[:, t][..., None], out.V[nxt[:, t]])
                Qm = np.where(live[:, t, :, :, None], Qm + (x * w[:, t, :, :, None]).astype(dtype), Qm)
                bx = np.where(term[:, t, :, :, None], np.abs(val[:, t]).astype(np.float64)[..., None], out.Bv[nxt[:, t]])
                BQ = BQ + np.where(live[:, t, :, :, None], bx * w[:, t, :, :, None].astype(np.float64), 0.0)
            pr, pc = P[st, :, :A], P[st, :, A:]                                    # [m, n, A]
            qr, qc = np.zeros((m, n, A), dtype), np.zeros((m, n, A), dtype)
            bqr, bqc = np.zeros((m, n, A)), np.zeros((m, n, A))
            for j in range(A):  # the other side's action, ascending
                qr = qr + (Qm[:, :, j, :].transpose(0, 2, 1) * pc[:, :, j, None]).astype(dtype)
                qc = qc + (Qm[:, j, :, :].transpose(0, 2, 1) * pr[:, :, j, None]).astype(dtype)
                bqr = bqr + BQ[:, :, j, :].transpose(0, 2, 1) * pc[:, :, j, None].astype(np.float64)
                bqc = bqc + BQ[:, j, :, :].transpose(0, 2, 1) * pr[:, :, j, None].astype(np.float64)
            if variant != "col_sign":
                qc = -qc
            v = _seq((pr * qr).astype(dtype))                                       # [m, n]
            out.V[st] = v
            out.Q[st] = np.concatenate([qr, qc], axis=2)
            out.Bq[st] = np.concatenate([bqr, bqc], axis=2)
            out.Bv[st] = (pr.astype(np.float64) * bqr).sum(axis=2)
            row, col, chn = out.reach[st, 0], out.reach[st, 1], out.reach[st, 2]   # [m, n]
            for side, (own, opp, q, vs, sig) in enumerate(((row, col, qr, v, pr), (col, row, qc, -v, pc))):
                sl = slice(side * A, side * A + A)
                if variant == "no_chance_cf":
                    cf = opp
                elif variant == "joint_cf":
                    cf = ((own * opp).astype(dtype) * chn).astype(dtype)
                elif variant == "own_reach_regret":
                    cf = (own * chn).astype(dtype)
                else:
                    cf = (opp * chn).astype(dtype)
                weight = opp if variant == "opp_reach_average" else own
                r_in, s_in = R[st][:, :, sl], S[st][:, :, sl]
                kept = (np.where(r_in > 0, dp, dn) * r_in).astype(dtype)
                gain = (cf[..., None] * (q - vs[..., None]).astype(dtype)).astype(dtype)
                updates = np.ones((n,), bool) if variant == "cleared_side_updated" else ((sides >> side) & 1) != 0
                write = updates[None, :, None] & mask[st][:, None, sl]
                out.RG[st, :, sl] = np.where(write, (kept + gain).astype(dtype), r_in)
                out.SS[st, :, sl] = np.where(write, ((da * s_in).astype(dtype) + (weight[..., None] * sig).astype(dtype)).astype(dtype), s_in)
    for a in (out.RG, out.SS, out.P, out.V, out.reach, out.Q):
        assert a.dtype == dtype
    return out


def gates(tree_arrays, ref, R, S, discount, sides):
    """A namespace of the gates of the module docstring from an fp64 `ref` = iterate(tree_arrays, R, S, discount, sides): P, RG, SS
    [S, n, 2A], V [S, n], reach [S, 3, n], and regret_gate_sum [n, 2] (the regret gate summed over the states and a side's actions)."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    R, S = np.asarray(R, np.float64), np.asarray(S, np.float64)
    disc = np.asarray(discount, np.float32).astype(np.float64)
    sides = np.asarray(sides).astype(np.int64)
    reached = ref.depth >= 0
    d = np.maximum(ref.depth, 0).astype(np.float64)
    h = ref.h.astype(np.float64)
    U = ULP  # one ulp per rounding (the module docstring)
    floor = np.where(reached, 2 * TINY, 0.0)
    P, reach = np.asarray(ref.P, np.float64), np.asarray(ref.reach, np.float64)
    gP = (A + 1) * U * P
    g_reach = np.empty_like(reach)
    for side in (0, 1):
        g_reach[:, side] = (d * (A + 2) + 1)[:, None] * (U * reach[:, side] + floor[:, None])
    g_reach[:, 2] = (d + 1)[:, None] * (U * reach[:, 2] + floor[:, None])
    KV, KQ = 4 * A + C + 7, 2 * A + C + 5
    gV = (h * KV * U)[:, None] * ref.Bv
    gQ = ((KQ + (h - 1) * KV) * U)[:, None, None] * ref.Bq
    gR, gS = np.zeros_like(R), np.zeros_like(S)
    for side in (0, 1):
        sl = slice(side * A, side * A + A)
        own, opp, chn = reach[:, side], reach[:, 1 - side], reach[:, 2]
        g_own, g_opp, g_chn = g_reach[:, side], g_reach[:, 1 - side], g_reach[:, 2]
        cf = opp * chn
        e_cf = g_opp * chn + opp * g_chn + U * cf
        kept = np.abs(np.where(R[:, :, sl] > 0, disc[None, :, 0, None], disc[None, :, 1, None]) * R[:, :, sl])
        span = ref.Bq[:, :, sl] + ref.Bv[:, :, None]
        write = (((sides >> side) & 1) != 0)[None, :, None] & ref.mask[:, None, sl] & reached[:, None, None]
        gR[:, :, sl] = np.where(write, 2 * U * kept + (e_cf + 4 * U * cf)[..., None] * span + cf[..., None] * (gQ[:, :, sl] + gV[:, :, None]) + 2 * TINY, 0.0)
        gS[:, :, sl] = np.where(write, 2 * U * np.abs(disc[None, :, 2, None] * S[:, :, sl]) + g_own[..., None] * P[:, :, sl]
                                + own[..., None] * gP[:, :, sl] + 3 * U * own[..., None] * P[:, :, sl] + 2 * TINY, 0.0)
    total = np.stack([gR[:, :, :A].sum(axis=(0, 2)), gR[:, :, A:].sum(axis=(0, 2))], axis=1)
    return types.SimpleNamespace(P=gP, V=gV, reach=g_reach, RG=gR, SS=gS, Q=gQ, regret_gate_sum=total)


def share(got, want, g):
    """Largest |got - want| / gate over the elements: 0 where both agree, inf where either is NaN or where the gate is 0 and they differ."""
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        s = np.where(err == 0, 0.0, err / g)
    s = np.nan_to_num(s, nan=np.inf, posinf=np.inf)
    return float(s.max()) if s.size else 0.0


OUTPUTS = ("RG", "SS", "P", "V", "reach")


def shares(ref, g, got, n=None):
    """dict of the worst share of each gate, over every state, of outputs `got` (a namespace of RG, SS, P, V, reach for the first n
    members) against the fp64 `ref` and its gates `g`.  Rows no gate covers (unreached, illegal, a cleared side) have gate 0: they must agree
    exactly -- for RG and SS that is the input, bit for bit."""
    n = ref.V.shape[1] if n is None else n
    cut = dict(RG=lambda x: x[:, :n], SS=lambda x: x[:, :n], P=lambda x: x[:, :n], V=lambda x: x[:, :n], reach=lambda x: x[:, :, :n])
    return {name: share(getattr(got, name), cut[name](getattr(ref, name)), cut[name](getattr(g, name))) for name in OUTPUTS}


# ---------------------------------------------------------------------------------------------------- inputs
def member(k):
    """(variant, earlier iterations, alternating during them, sides of the compared iteration) of member k."""
    return MEMBERS[k % len(MEMBERS)], (k // 4) % 8, ((k // 4) + k) % 2 == 1, (1, 2, 3)[k % 3]


def turn(alternating, t):
    """sides value of iteration t >= 1: both sides, or row on odd t and column on even t."""
    return (1 if t % 2 == 1 else 2) if alternating else 3


def discounts(variants, ts):
    """fp32 [n, 3]: schedule(variant, t) per member, rounded as the host layer rounds them."""
    return np.asarray([schedule(v, t) for v, t in zip(variants, ts)], np.float64).astype(np.float32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(R, S fp32 [S, 32, 2A], discount fp32 [32, 3], sides int32 [32]) of a tree, read-only."""
    tree = rr.tree_arrays(name)
    mask = legal_mask(tree)
    Sn, A2 = mask.shape
    variants = [member(k)[0] for k in range(N_MAX)]
    prior = np.asarray([member(k)[1] for k in range(N_MAX)])
    R64, S64 = np.zeros((Sn, N_MAX, A2)), np.zeros((Sn, N_MAX, A2))
    R, S = np.zeros((Sn, N_MAX, A2), np.float32), np.zeros((Sn, N_MAX, A2), np.float32)
    for t in range(1, 8):
        ref = iterate(tree, R64, S64, discounts(variants, [t] * N_MAX), [turn(member(k)[2], t) for k in range(N_MAX)])
        R64, S64 = ref.RG, ref.SS
        take = prior == t
        R[:, take], S[:, take] = R64[:, take].astype(np.float32), S64[:, take].astype(np.float32)
    R[np.abs(R) < 2.0 ** -60] = 0.0
    disc = discounts(variants, prior + 1)
    sides = np.asarray([member(k)[3] for k in range(N_MAX)], np.int32)
    for a in (R, S, disc, sides):
        a.setflags(write=False)
    return R, S, disc, sides


@functools.lru_cache(maxsize=None)
def case(name):
    """A namespace of one tree's case for all 32 members, computed once and read-only: tree, R, S, discount, sides, ref (fp64), g (gates),
    reached bool [S], n = 32.  The case of n members is the slice of the first n of everything."""
    tree = rr.tree_arrays(name)
    R, S, disc, sides = inputs(name)
    ref = iterate(tree, R, S, disc, sides)
    g = gates(tree, ref, R, S, disc, sides)
    for a in tuple(v for ns in (ref, g) for v in vars(ns).values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return types.SimpleNamespace(tree=tree, R=R, S=S, discount=disc, sides=sides, ref=ref, g=g, reached=ref.depth >= 0, n=N_MAX)


def average_policy(mask, SS):
    """[S, n, 2A] fp64: SS normalised per side over the legal actions, uniform over them where the sum is 0."""
    A = mask.shape[1] // 2
    SS = np.asarray(SS, np.float64)
    out = np.zeros_like(SS)
    for lo in (0, A):
        on = mask[:, None, lo:lo + A]
        x = np.where(on, SS[:, :, lo:lo + A], 0.0)
        tot = x.sum(axis=2, keepdims=True)
        cnt = np.maximum(on.sum(axis=2, keepdims=True), 1)
        out[:, :, lo:lo + A] = np.where(on, np.where(tot > 0, x / np.where(tot > 0, tot, 1.0), 1.0 / cnt), 0.0)
    return out


def run(name, variant, iterations, alternating=False, keep=False):
    """fp64 CFR from zero tables on tree `name`, one member: (R, S, list of sigma_t if keep) after `iterations` iterations."""
    tree = rr.tree_arrays(name)
    mask = legal_mask(tree)
    R, S, kept = np.zeros((mask.shape[0], 1, mask.shape[1])), np.zeros((mask.shape[0], 1, mask.shape[1])), []
    for t in range(1, iterations + 1):
        ref = iterate(tree, R, S, discounts([variant], [t]), [turn(alternating, t)])
        R, S = ref.RG, ref.SS
        if keep:
            kept.append(ref.P[:, 0].copy())
    return R, S, kept


def positive_regret(mask, R):
    """[n, 2] fp64: sum over the states of max over the side's legal actions of R+."""
    A = mask.shape[1] // 2
    plus = np.where(mask[:, None, :], np.maximum(np.asarray(R, np.float64), 0.0), 0.0)
    return np.stack([plus[:, :, :A].max(axis=2).sum(axis=0), plus[:, :, A:].max(axis=2).sum(axis=0)], axis=1)


# ---------------------------------------------------------------------------------------------------- figures and the built kernels
COMMITTED_ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "profiles", "cfr_errors.json")
_KERNEL = re.compile(r"k_cfr_(reach|update)ILi(\d+)EE")


def update_errors_file(key, figures):
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "cfr_errors.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def kernel_metadata(so_path):
    """{(kernel, A): dict(scratch, vgpr, sgpr, lds)} of every k_cfr_reach / k_cfr_update instantiation in the built library, from its
    kernel metadata (rnad_hip.kernel_notes, which tools/tabular_cfr.py --bench reports from as well)."""
    import rnad_hip

    kernels = rnad_hip.kernel_notes("k_cfr_update", so_path)
    assert kernels is not None, "ROCm's LLVM tools are not installed: the scratch invariant cannot be checked"
    table = {}
    for k in kernels:
        m = _KERNEL.search(k.get(".name", ""))
        if m:
            table[(m.group(1), int(m.group(2)))] = dict(scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"]),
                                                        sgpr=int(k[".sgpr_count"]), lds=int(k.get(".group_segment_fixed_size", 0)))
    return table
