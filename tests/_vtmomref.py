"""The exact variance of the learner update (csrc/vtrace_moments.hip, rnad_hip.vtrace_moments, learn.vtrace.update_noise): its definition
by enumeration, the sweep in the kernel's order of operations, derived gates and deliberately wrong variants.  numpy only.

DEFINITION.  `enumeration` runs `_learnref.learner(np.float64, ...)` on `_vtexpref.enumerate_batch` (every complete episode once, with
its probability under the behaviour mu and the tree's chance) and takes, over the lanes that visit s weighted by prob / reach[s],
    target_var[P, s]           = E[(v_target_P at the slot - target[P, s])^2]
    target_given_row_var[s, a] = the same for the column slot over the lanes whose row action at s was a, about their own mean
    q_var[P, s, a]             = E[(q_P[a] at the slot - q[P, s, a])^2]          (every action, drawn or not)
and the per-lane sums of (v - v_target) and its square by row, from which the variance of a row's entry of dv_tab follows.

SWEEP.  `reference(dtype, ...)` is the bottom-up recursion of include/rnad_hip.h (rnad_vtrace_moments) as the kernel performs it: t
ascending inside a joint action, the child's row actions a' ascending inside an outcome, b ascending inside a, every skipped term skipped
by a select.  The first moments are INPUT: `first` holds rnad_vtrace_expect's outputs target, target_given_row, q and its export record
[S, 3A + 5, n].  np.float64 is the reference, np.float32 the stand-in for a correct kernel.

GATES.  Every value is a `_learnref.VM` (value and the sum of its absolute terms m; a square's magnitude is the square of the magnitude).
u = 2^-24, h[s] the height of s.  The longest chain is the column side's V1 through dev' and the square; its roundings at its own level:
    dev': cs1 = pip / mu (1), w' = cs1 cs0 (1), X's longest path runs through e1: pip lpol and the A sums (A + 1), eta e1 (1), the three
    sums of X (3), min X (1), the sum with the lambda summand (1, whose own lgg min d meets 5 < A + 6), the difference with dW1[s][a] (1):
    A + 10; the square doubles them and adds one: 2A + 21;
    the sum with the child's variance term (1; that term meets 12: cs1, w', lgg (2), the product with min, the square, the product with
    V1), the product with mu0[u][a'] (1), the A-fold child sum (A), the product with chance (1), the sum over C outcomes (C), the product
    with mu1[b] (1), the sum over b (A): 4A + C + 26;
    target_var[1] adds the sum with the between-action square (1), the product with mu0[a] (1) and the sum over a (A): 5A + C + 28.
q_var meets fewer: tm (at most 9) squared (19), the same sums (2A + C + 5), the sum with (1 - mu) tbar^2 and the division (2).  With + 2
for second order, a child's error entering with the weight its magnitude enters m with, by induction over the height
    |got - want| <= h[s] K u m,      K(A, C) = 5A + C + 30,
for target_var, target_given_row_var and q_var alike.

END TO END.  learn.vtrace.update_noise feeds the kernel fp32 first moments; the all-fp64 pipeline differs from the fp64 sweep on those by
the first moments' own errors, each within its gate of `_vtexpref` (target, target_given_row, q: h K' u m; the record's e0[u]: (A + 1) u
mag, cs0[u]: u cs0).  A squared deviation moves by d(dev^2) = 2 dev d(dev) + d(dev)^2, so with G(dev) the sum of |coefficient| * gate over
the first moments dev reads (min(w, .) is 1-Lipschitz in w), the first-order term of a summand is 2 |dev| G(dev) (+ G(dev)^2, kept), a
weight (lgg min(w', c))^2 moves by 2 (lgg min) lgg cs1 gate(cs0), and the terms add with the weights of the recursion: `first_gates`
switches this third channel on (fp64 only), `gates(..., first_order=True)` adds it."""
import json
import os
import re
import types

import numpy as np

import _crossref as cr
import _learnref as lr
import _regref as rr
import _vtexpref as vx
from _learnref import HP, SETS, VM, minimum, where  # noqa: F401
from _regref import ALL_TREES  # noqa: F401
from _vtexpref import BEHAVIOURS, HAND_TREES, N_MAX, U, hand_case, share, to_rows, to_sides  # noqa: F401

CHUNK = 4096
VARIANTS = ("c_not_squared", "v1_mean", "no_between", "no_tbar", "mu_squared", "rho_c", "no_chance", "reward_sign")
OUTPUTS = ("target_var", "target_given_row_var", "q_var")


def workspace(S, A, n):
    return S * n * (A + 1) if S >= 2 and 1 <= n <= 32 and 1 <= A <= 8 else -1


def K_of(A, C):
    return 5 * A + C + 30


# ---------------------------------------------------------------------------------------------------- the definition
def enumeration(tree, mu_tab, tables, hp):
    """The definition: a namespace of reach [S], target, target_var [2S], given_row, given_row_var [S, A], q, q_var [2S, A], and the per-lane
    sums dv1, dv2 [2S] = sum_lanes prob (v - v_target at the row's slot) and its square (0 for a lane that does not visit the row)."""
    batch, prob = vx.enumerate_batch(tree, mu_tab)
    out = lr.learner(np.float64, batch, tables, hp)
    idx, act = batch["indices"], batch["actions"]
    T, B = idx.shape
    S, A = batch["S"], batch["mu"].shape[-1]
    valid = idx != 0
    turn = out.turn
    rows = ((np.arange(T) & 1)[:, None] * S + idx)[valid]
    w = np.broadcast_to(prob[None, :], (T, B))[valid]
    vt = np.where(turn == 0, out.v_target.v[0], out.v_target.v[1])[valid]
    qq = np.where((turn == 0)[..., None], out.q.v[0], out.q.v[1])[valid]
    visits, target, q = np.zeros(2 * S), np.zeros(2 * S), np.zeros((2 * S, A))
    np.add.at(visits, rows, w)
    np.add.at(target, rows, w * vt)
    np.add.at(q, rows, w[:, None] * qq)
    seen = visits > 0
    target[seen] /= visits[seen]
    q[seen] /= visits[seen][:, None]
    tvar, qvar = np.zeros(2 * S), np.zeros((2 * S, A))
    np.add.at(tvar, rows, w * (vt - target[rows]) ** 2)
    np.add.at(qvar, rows, w[:, None] * (qq - q[rows]) ** 2)
    tvar[seen] /= visits[seen]
    qvar[seen] /= visits[seen][:, None]
    # the column slots grouped by the row action taken at the same state one step earlier
    col = valid & (turn == 1)
    row_act = np.zeros_like(act)
    row_act[1:] = act[:-1]
    key = (idx * A + row_act)[col]
    wc = np.broadcast_to(prob[None, :], (T, B))[col]
    vc = out.v_target.v[1][col]
    cnt, g, gvar = np.zeros(S * A), np.zeros(S * A), np.zeros(S * A)
    np.add.at(cnt, key, wc)
    np.add.at(g, key, wc * vc)
    on = cnt > 0
    g[on] /= cnt[on]
    np.add.at(gvar, key, wc * (vc - g[key]) ** 2)
    gvar[on] /= cnt[on]
    v = np.asarray(tables["v"], np.float64).reshape(2 * S)
    d = v[rows] - vt
    dv1, dv2 = np.zeros(2 * S), np.zeros(2 * S)
    np.add.at(dv1, rows, w * d)
    np.add.at(dv2, rows, w * d * d)
    return types.SimpleNamespace(reach=visits[:S], target=target, target_var=tvar, given_row=g.reshape(S, A), given_row_var=gvar.reshape(S, A),
                                 q=q, q_var=qvar, dv1=dv1, dv2=dv2, episodes=B)


def noise_tables(hp, v, target, target_var, reach):
    """What learn.vtrace.update_noise derives on the host, fp64: dict of dv_var_tab [2S], target_noise [2], episodes_for_unit_snr [2]."""
    S = reach.shape[0]
    reach2 = np.concatenate([reach, reach]).astype(np.float64)
    L = float(reach.astype(np.float64).sum())
    d = np.asarray(v, np.float64).reshape(2 * S) - np.asarray(target, np.float64)
    var = np.asarray(target_var, np.float64)
    scale = (2 * hp.w_v / L) ** 2
    dv_var = scale * (reach2 * (var + d * d) - reach2 * reach2 * d * d)
    dv = 2 * hp.w_v * reach2 * d / L
    noise = reach2 * var
    snr = []
    for P in range(2):
        sig = float((dv[P * S:(P + 1) * S] ** 2).sum())
        snr.append(float(dv_var[P * S:(P + 1) * S].sum()) / sig if sig > 0 else np.inf)
    return dict(dv_var_tab=dv_var, target_noise=np.array([noise[:S].sum(), noise[S:].sum()]), episodes_for_unit_snr=np.array(snr))


# ---------------------------------------------------------------------------------------------------- the sweep
def first_of(dtype, MU, PIP, LPOL, VV, exp):
    """rnad_vtrace_expect's outputs and export record [S, 3A + 5, n] in `dtype` from a `_vtexpref.reference` namespace `exp`."""
    MU, PIP, LPOL, VV = (np.asarray(x).astype(dtype) for x in (MU, PIP, LPOL, VV))
    S, n, A2 = MU.shape
    A = A2 // 2
    rec = np.zeros((S, 3 * A + 5, n), dtype)
    tg, W1, q = (np.asarray(x).astype(dtype) for x in (exp.target.v, exp.W1.v, exp.q.v))
    rec[:, 0], rec[:, 1], rec[:, 3] = VV[:, :, 0], tg[:, :, 0], VV[:, :, 1]
    e0 = np.zeros((S, n), dtype)
    p1 = np.zeros((S, n), dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(A):
            e0 = np.where(PIP[:, :, a] > 0, e0 + PIP[:, :, a] * LPOL[:, :, a], e0)
            p1 = np.where(MU[:, :, a] > 0, p1 + PIP[:, :, a] * W1[:, :, a], p1)
            rec[:, 5 + a] = MU[:, :, a]
            rec[:, 5 + A + a] = np.where(MU[:, :, a] > 0, PIP[:, :, a] / np.where(MU[:, :, a] > 0, MU[:, :, a], 1), 0)
            rec[:, 5 + 2 * A + a] = W1[:, :, a] - VV[:, :, 1]
    rec[:, 2], rec[:, 4] = e0, p1
    dead = np.asarray(exp.depth) < 0
    rec[dead] = 0
    return types.SimpleNamespace(target=tg, W1=W1, q=q, rec=rec)


_Store = vx._Store


def reference(dtype, tree_arrays, MU, PIP, LPOL, VV, hyper, first, variant=None, first_gates=None):
    """A namespace of VM tvar [S, n, 2], V1 [S, n, A] (target_given_row_var), qvar [S, n, 2A] in `dtype`; h int [S]; reached bool [S]; with
    `first_gates` (fp64 only) also f_tvar, f_V1, f_qvar: the first-order channel of the module docstring.  `first`: see `first_of`."""
    assert variant is None or variant in VARIANTS
    index = np.asarray(tree_arrays["index"]).astype(np.int64)
    value = np.asarray(tree_arrays["value"]).astype(dtype)
    chance = np.asarray(tree_arrays["chance"]).astype(dtype)
    S, C, A, _ = index.shape
    MU, PIP, LPOL, VV = (np.asarray(x).astype(dtype) for x in (MU, PIP, LPOL, VV))
    n = MU.shape[1]
    rec, TGf, W1f, Qf = (np.asarray(x).astype(dtype) for x in (first.rec, first.target, first.W1, first.q))
    assert rec.shape == (S, 3 * A + 5, n) and TGf.shape == (S, n, 2) and W1f.shape == (S, n, A) and Qf.shape == (S, n, 2 * A)
    hy = np.asarray(hyper, np.float32).astype(dtype).reshape(n, 5)
    eta, g, lam, rho, cb = (VM(hy[None, :, i]) for i in range(5))
    if variant == "rho_c":
        rho, cb = cb, rho
    ge, gg, lgg = g * eta, g * g, (lam * g) * g
    zero = dtype(0)
    FO = first_gates is not None
    if FO:
        assert dtype is np.float64
        gT, gW, gQ = (np.asarray(first_gates[k], np.float64) for k in ("target", "target_given_row", "q"))
        absv = np.abs
    M0, M1, M1mean = _Store((S, n), dtype), _Store((S, n, A), dtype), _Store((S, n), dtype)
    TV, QV = _Store((S, n, 2), dtype), _Store((S, n, 2 * A), dtype)
    F0, F1, FT, FQ = np.zeros((S, n)), np.zeros((S, n, A)), np.zeros((S, n, 2)), np.zeros((S, n, 2 * A))
    E0M = np.zeros((S, n))
    h = np.zeros((S,), np.int64)
    reached = np.zeros((S,), bool)
    levels = cr.level_order(index, chance)
    sq = lambda x: x * x  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for level in reversed(levels):
            for lo in range(0, level.size, CHUNK):
                st = level[lo:lo + CHUNK]
                m = st.size
                reached[st] = True
                idx, live_all = index[st], chance[st] > 0
                nxt_all = np.where(live_all, idx, 0)
                h[st] = 1 + np.where(nxt_all != 0, h[nxt_all], 0).reshape(m, -1).max(axis=1)
                side = lambda X, k: [VM(X[st][:, :, k * A + a]) for a in range(A)]  # noqa: E731
                mu0, mu1, pip0, pip1, lp0, lp1 = side(MU, 0), side(MU, 1), side(PIP, 0), side(PIP, 1), side(LPOL, 0), side(LPOL, 1)
                vv0, vv1 = VM(VV[st][:, :, 0]), VM(VV[st][:, :, 1])
                blank = VM(np.zeros((m, n), dtype))
                fz = np.zeros((m, n))
                e0 = e1 = blank
                cs0, cs1 = [], []
                for a in range(A):
                    e0 = where(pip0[a].v > 0, e0 + pip0[a] * lp0[a], e0)
                    e1 = where(pip1[a].v > 0, e1 + pip1[a] * lp1[a], e1)
                    cs0.append(where(mu0[a].v > 0, pip0[a] / VM(np.where(mu0[a].v > 0, mu0[a].v, 1)), zero))
                    cs1.append(where(mu1[a].v > 0, pip1[a] / VM(np.where(mu1[a].v > 0, mu1[a].v, 1)), zero))
                base0 = (ge * e1 - eta * e0) - vv0
                d0s = VM(TGf[st][:, :, 0]) - vv0
                tgt1 = VM(TGf[st][:, :, 1])
                dW1s = [VM(rec[st, 5 + 2 * A + a, :]) for a in range(A)]
                W1s = [VM(W1f[st][:, :, a]) for a in range(A)]
                tbar0 = [VM(Qf[st][:, :, a]) - (vv0 - eta * lp0[a]) for a in range(A)]
                tbar1 = [VM(Qf[st][:, :, A + a]) - (vv1 - eta * lp1[a]) for a in range(A)]
                v0acc, qv0, v1acc, qv1 = blank, [blank] * A, [blank] * A, [blank] * A
                f0acc, fq0, f1acc, fq1 = fz, [fz] * A, [fz] * A, [fz] * A
                for a in range(A):
                    for b in range(A):
                        leave_clip = minimum(cs1[b], rho)
                        w = cs0[a] * cs1[b]
                        cr_, cc = minimum(w, rho), lgg * minimum(w, cb)
                        cc2 = cc if variant == "c_not_squared" else cc * cc
                        gc = g * cs1[b]
                        ggc = gg * cs1[b]
                        ggc2 = ggc * ggc
                        xr = zr = xc = zc = blank
                        fxr = fzr = fxc = fzc = fz
                        for t in range(C):
                            live, nxt = live_all[:, t, a, b][:, None], nxt_all[:, t, a, b]
                            leaves = (nxt == 0)[:, None]
                            p = VM(np.where(live, 1, chance[st, t, a, b][:, None]).astype(dtype)) if variant == "no_chance" else \
                                VM(chance[st, t, a, b][:, None])
                            r = VM(value[st, t, a, b][:, None])
                            # the row side
                            vv0u, W0u, V0u = VM(rec[nxt, 0, :]), VM(rec[nxt, 1, :]), M0[nxt]
                            d0u = W0u - vv0u
                            delta0 = base0 + g * where(leaves, r, g * vv0u)
                            dev = (cr_ * delta0 + where(leaves, zero, cc * d0u)) - d0s
                            term = dev * dev + where(leaves, zero, cc2 * V0u)
                            xr = where(live, xr + p * term, xr)
                            tm = (ge * e1 + gc * where(leaves, r, g * W0u)) - vv0
                            dq = tm - tbar0[a]
                            qt = dq * dq + where(leaves, zero, ggc2 * V0u)
                            zr = where(live, zr + p * qt, zr)
                            if FO:
                                gdev = np.where(leaves, 0.0, absv(cc.v) * gT[nxt][:, :, 0]) + gT[st][:, :, 0]
                                ft = 2 * absv(dev.v) * gdev + sq(gdev) + np.where(leaves, 0.0, cc2.v * F0[nxt])
                                fxr = np.where(live, fxr + p.v * ft, fxr)
                                gdq = np.where(leaves, 0.0, absv(ggc.v) * gT[nxt][:, :, 0]) + gQ[st][:, :, a]
                                fq = 2 * absv(dq.v) * gdq + sq(gdq) + np.where(leaves, 0.0, ggc2.v * F0[nxt])
                                fzr = np.where(live, fzr + p.v * fq, fzr)
                            # the column side
                            vv1u, e0u = VM(rec[nxt, 3, :]), VM(rec[nxt, 2, :])
                            X = ((ge * e0u - eta * e1) + gg * vv1u) - vv1
                            lead = ge * e0u
                            inner = innerq = blank
                            finner = finnerq = fz
                            v1mean = M1mean[nxt]
                            if FO:
                                ge0u = (A + 1) * U * E0M[nxt]  # e0[u]'s own gate: A products and sums
                            for i in range(A):
                                mi, c0, dd = VM(rec[nxt, 5 + i, :]), VM(rec[nxt, 5 + A + i, :]), VM(rec[nxt, 5 + 2 * A + i, :])
                                Vc = v1mean if variant == "v1_mean" else M1[nxt][..., i]
                                wp = cs1[b] * c0
                                crp, ccp = minimum(wp, rho), lgg * minimum(wp, cb)
                                ccp2 = ccp if variant == "c_not_squared" else ccp * ccp
                                devp = (crp * X + ccp * dd) - dW1s[a]
                                tt = devp * devp + ccp2 * Vc
                                inner = where(mi.v > 0, inner + mi * tt, inner)
                                gcc = gg * c0
                                tmq = (lead + gcc * (vv1u + dd)) - vv1
                                dqq = tmq - tbar1[b]
                                tq = dqq * dqq + (gcc * gcc) * Vc
                                innerq = where(mi.v > 0, innerq + mi * tq, innerq)
                                if FO:
                                    gc0 = U * absv(c0.v)
                                    gw = absv(cs1[b].v) * gc0
                                    gdev = absv(crp.v) * absv(ge.v) * ge0u + gw * (absv(X.v) + absv(lgg.v) * absv(dd.v)) + \
                                        absv(ccp.v) * gW[nxt][:, :, i] + gW[st][:, :, a]
                                    f = 2 * absv(devp.v) * gdev + sq(gdev) + ccp2.v * F1[nxt][:, :, i] + \
                                        (2 * absv(ccp.v) * absv(lgg.v) * gw + sq(absv(lgg.v) * gw)) * Vc.v
                                    finner = np.where(mi.v > 0, finner + mi.v * f, finner)
                                    ggcc = absv(gg.v) * gc0
                                    gdq = absv(ge.v) * ge0u + ggcc * absv((vv1u + dd).v) + absv(gcc.v) * gW[nxt][:, :, i] + gQ[st][:, :, A + b]
                                    f = 2 * absv(dqq.v) * gdq + sq(gdq) + sq(gcc.v) * F1[nxt][:, :, i] + (2 * absv(gcc.v) * ggcc + sq(ggcc)) * Vc.v
                                    finnerq = np.where(mi.v > 0, finnerq + mi.v * f, finnerq)
                            rr_ = r if variant == "reward_sign" else -r
                            devl = leave_clip * ((rr_ - eta * e1) - vv1) - dW1s[a]
                            dql = (rr_ - vv1) - tbar1[b]
                            tx = where(leaves, devl * devl, inner)
                            zx = where(leaves, dql * dql, innerq)
                            xc, zc = where(live, xc + p * tx, xc), where(live, zc + p * zx, zc)
                            if FO:
                                fl = 2 * absv(devl.v) * gW[st][:, :, a] + sq(gW[st][:, :, a])
                                fql = 2 * absv(dql.v) * gQ[st][:, :, A + b] + sq(gQ[st][:, :, A + b])
                                fxc = np.where(live, fxc + p.v * np.where(leaves, fl, finner), fxc)
                                fzc = np.where(live, fzc + p.v * np.where(leaves, fql, finnerq), fzc)
                        both = (mu0[a].v > 0) & (mu1[b].v > 0)
                        v0acc = where(both, v0acc + (mu0[a] * mu1[b]) * xr, v0acc)
                        qv0[a] = where(mu1[b].v > 0, qv0[a] + mu1[b] * zr, qv0[a])
                        v1acc[a] = where(mu1[b].v > 0, v1acc[a] + mu1[b] * xc, v1acc[a])
                        qv1[b] = where(mu0[a].v > 0, qv1[b] + mu0[a] * zc, qv1[b])
                        if FO:
                            f0acc = np.where(both, f0acc + mu0[a].v * mu1[b].v * fxr, f0acc)
                            fq0[a] = np.where(mu1[b].v > 0, fq0[a] + mu1[b].v * fzr, fq0[a])
                            f1acc[a] = np.where(mu1[b].v > 0, f1acc[a] + mu1[b].v * fxc, f1acc[a])
                            fq1[b] = np.where(mu0[a].v > 0, fq1[b] + mu0[a].v * fzc, fq1[b])
                tv1 = mean1 = blank
                ftv1 = fz
                q0, q1, fq0o, fq1o = [], [], [], []
                one = dtype(1)
                for a in range(A):
                    btw = W1s[a] - tgt1
                    part = v1acc[a] if variant == "no_between" else v1acc[a] + btw * btw
                    tv1 = where(mu0[a].v > 0, tv1 + mu0[a] * part, tv1)
                    mean1 = where(mu0[a].v > 0, mean1 + mu0[a] * v1acc[a], mean1)
                    for (muP, tb, acc, dst) in ((mu0, tbar0, qv0, q0), (mu1, tbar1, qv1, q1)):
                        safe = VM(np.where(muP[a].v > 0, muP[a].v, 1))
                        num = acc[a] if variant == "no_tbar" else acc[a] + (one - muP[a]) * (tb[a] * tb[a])
                        quo = (num / safe) / safe if variant == "mu_squared" else num / safe
                        dst.append(where(muP[a].v > 0, quo, zero))
                    if FO:
                        gb = gW[st][:, :, a] + gT[st][:, :, 1]
                        ftv1 = np.where(mu0[a].v > 0, ftv1 + mu0[a].v * (f1acc[a] + 2 * absv(btw.v) * gb + sq(gb)), ftv1)
                        for (muP, tb, facc, dst, col) in ((mu0, tbar0, fq0, fq0o, a), (mu1, tbar1, fq1, fq1o, A + a)):
                            gq = gQ[st][:, :, col]
                            safe = np.where(muP[a].v > 0, muP[a].v, 1)
                            dst.append(np.where(muP[a].v > 0, (facc[a] + (1 - muP[a].v) * (2 * absv(tb[a].v) * gq + sq(gq))) / safe, 0.0))
                v1acc = [where(mu0[a].v > 0, v1acc[a], zero) for a in range(A)]  # a row action never drawn conditions on nothing
                M0[st], M1[st], M1mean[st] = v0acc, vx._stack(v1acc), mean1
                TV[st] = vx._stack([v0acc, tv1])
                QV[st] = vx._stack(q0 + q1)
                if FO:
                    F0[st], F1[st] = f0acc, np.stack(f1acc, -1)
                    FT[st], FQ[st] = np.stack([f0acc, ftv1], -1), np.stack(fq0o + fq1o, -1)
                E0M[st] = e0.m
    out = types.SimpleNamespace(tvar=VM(TV.v, TV.m), V1=VM(M1.v, M1.m), qvar=VM(QV.v, QV.m), h=h, reached=reached)
    if FO:
        out.f_tvar, out.f_V1, out.f_qvar = FT, F1, FQ
    for a in (TV.v, M1.v, QV.v):
        assert a.dtype == dtype
    return out


def gates(tree_arrays, ref, first_order=False):
    """dict of the gates of target_var [S, n, 2], target_given_row_var [S, n, A], q_var [S, n, 2A] from an fp64 `ref`: h K u m (module
    docstring); first_order: plus the first-order channel of a `ref` computed with `first_gates` (the end-to-end gate)."""
    _, C, A, _ = np.asarray(tree_arrays["index"]).shape
    hk = ref.h.astype(np.float64)[:, None, None] * K_of(A, C) * U
    g = dict(target_var=hk * ref.tvar.m, target_given_row_var=hk * ref.V1.m, q_var=hk * ref.qvar.m)
    if first_order:
        g = {k: g[k] + f for k, f in zip(OUTPUTS, (ref.f_tvar, ref.f_V1, ref.f_qvar))}
    return g


def values_of(ref):
    return dict(target_var=ref.tvar.v, target_given_row_var=ref.V1.v, q_var=ref.qvar.v)


def shares(ref, g, got, n=None):
    """dict of the worst share of each gate over the reached states for outputs `got` (keyed as OUTPUTS) against the first n members."""
    R, want = ref.reached, values_of(ref)
    n = want["q_var"].shape[1] if n is None else n
    return {k: share(np.asarray(got[k])[R], want[k][R][:, :n], g[k][R][:, :n]) for k in OUTPUTS}


def sweep_of(c, hp=None, dtype=np.float64, variant=None, first_dtype=np.float64, first_order=False):
    """`reference` for the single member of a `_vtexpref.hand_case`, the first moments from `_vtexpref.sweep_of` in `first_dtype`."""
    hp = c.hp if hp is None else hp
    S = c.S
    args = (to_sides(c.mu_tab, S)[:, None], to_sides(c.pip, S)[:, None], to_sides(c.lpol, S)[:, None], to_sides(c.tables["v_target"], S)[:, None])
    exp = vx.sweep_of(c, hp)
    first = first_of(first_dtype, *args, exp)
    return reference(dtype, c.tree, *args, [vx.hyper_of(hp)], first, variant=variant,
                     first_gates=vx.gates(c.tree, exp) if first_order else None)


# ---------------------------------------------------------------------------------------------------- figures and the built kernels
COMMITTED_ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "profiles", "vtrace_moments_errors.json")
_KERNEL = re.compile(r"k_vtrace_momentsILi(\d+)EE")


def update_errors_file(key, figures):
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "vtrace_moments_errors.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def kernel_metadata(so_path):
    """{A: dict(scratch, vgpr, sgpr, lds)} of every k_vtrace_moments instantiation in the built library, read as
    _vtexpref.kernel_metadata reads k_vtrace_expect's: .hip_fatbin -> its offload bundles -> the gfx950 code object -> the
    amdhsa.kernels note."""
    import subprocess
    import tempfile

    tools = {t: os.path.join(rr.LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    kernels = []
    with tempfile.TemporaryDirectory(prefix="vtmom_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(rr._BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_vtrace_moments" not in part:
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
