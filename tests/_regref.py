"""References, gates and inputs for the regularised-game solver (csrc/reg_solve.hip, rnad_hip.reg_solve, learn/tabular.py).

What is solved, at every state s reachable from the root (state 1), bottom-up:

    Q[s,r,c] = sum_t chance[s,t,r,c] * (index == 0 ? value[s,t,r,c] : V[index])          entries with chance <= 0 skipped
    pi_row ~ mu_row * exp((Q pi_col) / eta)         pi_col ~ mu_col * exp(-(Q^T pi_row) / eta)
    V[s] = pi_row^T Q pi_col - eta * KL(pi_row || mu_row) + eta * KL(pi_col || mu_col)   V[0] = 0

`solve(..., np.float64)` is the reference: every level to residual 1e-12 (the shipped extragradient iteration, polished with Newton steps
on pi - softmax(log mu + q / eta) = 0, which only ever replace an iterate by one with a smaller residual).  `solve(..., np.float32)` is the
restatement of the iteration the kernel runs, operation by operation (numpy's exp and log stand in for the device's).

Gates, at every reached state, on a solver's OUTPUTS (`check`):
  (a) residual: max_a |pi(a) - softmax(log mu + q / eta)(a)| recomputed in fp64 from the policy it returned and the values it returned for
      the children, <= 2 * tol.
  (b) value: |V[s] - V64| <= (A*A*C + 2A + 8) * 2^-24 * B[s], V64 the formula above in fp64 on the returned policy, log-policy and
      children values.  Derived as in _crossref.py, for one level: a term of pi_row^T Q pi_col meets at most A*A*C + A roundings of
      partial sums and its own products, a KL term A more, the final two sums and the log-difference the rest; every rounding is at
      most 2^-24 of the partial sum, which B[s], the sum of the absolute terms (eta * |pi log(pi / mu)| included), bounds.
  (c) distance to the fp64 fixed point, max |pi - pi*| and max |V - V*|: not derivable (it is the residual times the conditioning of the
      state).  `gate_c()` is twice the worst the fp32 restatement shows over all inputs below.
"""
import functools
import json
import os
import re
import subprocess
import tempfile

import numpy as np

import _crossref as cr
from _util import TREES

U = 2.0 ** -24
ETAS = (1.0, 0.2, 0.05)
TOL = 1e-5
MAX_ITERS = 4096
# fp64 reference: a Newton polish is tried after every so many extragradient steps.  Every 10 or 5 is not faster: at eta = 0.05 the polish
# then throws states of native_a3 and native_a5 far out in log space again and again and they never reach 1e-12; with 20 every case does
# (asserted in tests/test_reg_solve.py).
POLISH_EVERY = 20
MAGNETS = ("uniform", "solution", "softmax", "after4")
VARIANTS = ("col_sign", "no_magnet", "no_opp_kl", "no_chance")
# small generated trees so that every A = 1 .. 8 and C = 1 .. 4 occurs: (A, C, depth_bound)
GEN_SPECS = {f"gen_a{A}c{C}": dict(A=A, C=C, depth_bound=d, transition_threshold=0.1, seed=20 + A, prune=(0, 0))
             for A, C, d in ((1, 2, 4), (2, 3, 4), (3, 4, 3), (4, 1, 3), (5, 2, 2), (6, 3, 2), (7, 4, 2), (8, 1, 2))}
ALL_TREES = TREES + ("native_a3", "native_a5") + tuple(GEN_SPECS)


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def tree_arrays(name):
    if name not in GEN_SPECS:
        return cr.tree_arrays(name)
    import rnad_hip

    k = GEN_SPECS[name]
    out = rnad_hip.tree_generate(k["A"], k["C"], k["depth_bound"], float(k["transition_threshold"]), (-1.0, 1.0), k["prune"], k["seed"])
    arrs = {key: out[key].numpy() for key in ("index", "value", "chance", "expected_value", "legal", "root_value", "solution")}
    arrs["meta"] = dict(kw=dict(depth_bound=k["depth_bound"]), spec=k)
    return arrs


def legal_mask(tree):
    legal = np.asarray(tree["legal"])[:, 0]
    return np.concatenate([legal[:, :, 0], legal[:, 0, :]], axis=1) != 0


def log_table(table, mask):
    """fp32 log of a probability table; zeros and illegal actions become -inf."""
    t = np.asarray(table, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mask & (t > 0), np.log(np.where(t > 0, t, 1.0)), -np.inf).astype(np.float32)


@functools.lru_cache(maxsize=None)
def levels_of(name):
    t = tree_arrays(name)
    return tuple(cr.level_order(t["index"], t["chance"]))


@functools.lru_cache(maxsize=None)
def magnet(name, kind, eta):
    """fp32 [S, 2A] log mu.  after4 depends on eta: the table after 4 fp64 updates from uniform, rounded to fp32."""
    tree = tree_arrays(name)
    mask = legal_mask(tree)
    S, A2 = mask.shape
    A = A2 // 2
    if kind == "uniform":
        n = np.concatenate([np.repeat(mask[:, :A].sum(1, keepdims=True), A, 1), np.repeat(mask[:, A:].sum(1, keepdims=True), A, 1)], axis=1)
        out = log_table(mask / np.maximum(n, 1), mask)
    elif kind == "solution":
        out = log_table(tree["solution"], mask)
    elif kind == "softmax":
        rng = np.random.default_rng(7)
        z = 2.0 * rng.standard_normal((S, A2))
        lse = np.concatenate([np.repeat(_lse(z[:, :A], mask[:, :A]), A, 1), np.repeat(_lse(z[:, A:], mask[:, A:]), A, 1)], axis=1)
        out = np.where(mask, z - lse, -np.inf).astype(np.float32)
    else:
        assert kind == "after4"
        out = chain(name, eta)[3]["log_policy"].astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chain(name, eta, updates=4):
    """The fp64 solutions of `updates` regularisation updates from the uniform magnet; the log table handed from one update to the
    next is rounded to fp32, which is what the product hands on."""
    reg, outs = magnet(name, "uniform", eta), []
    for _ in range(updates):
        outs.append(solve(name, reg, eta, np.float64))
        reg = outs[-1]["log_policy"].astype(np.float32)
    return tuple(outs)


def nashconv64(name, policy):
    """row_best[1] + col_best[1] of util/metric.py:134-175 for a [S, 2A] table, fp64, level by level."""
    tree = tree_arrays(name)
    idx, ch = np.asarray(tree["index"]), np.asarray(tree["chance"], np.float64)
    val = np.asarray(tree["value"], np.float64)
    mask = legal_mask(tree)
    S, A2 = mask.shape
    A = A2 // 2
    pi = np.asarray(policy, np.float64)
    rb, cb = np.zeros(S), np.zeros(S)
    for st in reversed(levels_of(name)):
        live = ch[st] > 0
        nxt = np.where(live, idx[st], 0)
        Mr = np.where(live, ch[st] * np.where(nxt == 0, val[st], rb[nxt]), 0.0).sum(axis=1)
        Mc = np.where(live, ch[st] * np.where(nxt == 0, -val[st], cb[nxt]), 0.0).sum(axis=1)
        rowr = np.einsum("mrc,mc->mr", Mr, pi[st, A:])
        colr = np.einsum("mr,mrc->mc", pi[st, :A], Mc)
        rb[st] = np.where(mask[st, :A], rowr, -np.inf).max(axis=1)
        cb[st] = np.where(mask[st, A:], colr, -np.inf).max(axis=1)
    return float(rb[1] + cb[1])


def _lse(x, on):
    with np.errstate(invalid="ignore"):
        m = np.where(on, x, -np.inf).max(axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return m + np.log(np.maximum(np.where(on, np.exp(np.where(on, x, 0.0) - m), 0.0).sum(axis=1, keepdims=True), 1e-300))


# ---------------------------------------------------------------------------------------------------- the iteration
def _q_matrix(tree, st, V, dtype, no_chance=False):
    """Q [m, A, A] of the states `st` from the children's V: the chance outcomes in order, one accumulator."""
    idx = np.asarray(tree["index"])[st]
    ch = np.asarray(tree["chance"])[st].astype(dtype)
    val = np.asarray(tree["value"])[st].astype(dtype)
    live = ch > 0
    nxt = np.where(live, idx, 0)
    v = np.where(nxt == 0, val, V[nxt])
    w = np.where(live, dtype(1), ch) if no_chance else ch
    Q = np.zeros(idx.shape[:1] + idx.shape[2:], dtype)
    for t in range(idx.shape[1]):
        Q = np.where(live[:, t], Q + w[:, t] * v[:, t], Q)
    return Q


def _normalise(x, on):
    m = np.where(on, x, -np.inf).max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    e = np.where(on, np.exp(np.where(on, x - m, 0)), 0).astype(x.dtype)
    s = _seqsum(e)
    with np.errstate(divide="ignore"):
        lse = m + np.log(s)
    return np.where(on, x - lse, 0).astype(x.dtype)


def _seqsum(x):
    """sum over axis 1 in index order (what an unrolled loop does), keepdims."""
    s = np.zeros_like(x[:, :1])
    for a in range(x.shape[1]):
        s = s + x[:, a:a + 1]
    return s


def _responses(Q, pr, pc, col_sign=1.0):
    """qr = Q pc, qc = -(Q^T pr), accumulated c inside r."""
    m, A, _ = Q.shape
    if Q.dtype == np.float64:  # the reference: the order of a sum is not its subject
        qr, qc = np.einsum("mrc,mc->mr", Q, pc), -np.einsum("mrc,mr->mc", Q, pr)
        return qr, (qc if col_sign > 0 else -qc)
    qr = np.zeros_like(pr)
    qc = np.zeros_like(pc)
    for r in range(A):
        for c in range(A):
            qr[:, r] = qr[:, r] + Q[:, r, c] * pc[:, c]
            qc[:, c] = qc[:, c] - pr[:, r] * Q[:, r, c]
    return qr, (qc if col_sign > 0 else -qc)


def _softmax(t, on):
    m = np.where(on, t, -np.inf).max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0).astype(t.dtype)
    e = np.where(on, np.exp(np.where(on, t - m, 0)), 0).astype(t.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(on, e / _seqsum(e), 0).astype(t.dtype)


def _residual(p, lm, q, on, inv_eta):
    d = np.where(on, np.abs(p - _softmax(lm + q * inv_eta, on)), 0)
    return d.max(axis=1)


def _newton(Q, lmr, lmc, onr, onc, lr, lc, inv_eta):
    """One Newton step on G(p) = p - softmax(lm + q(p) / eta) = 0 for both players, then one application of the fixed-point map so
    that the result is again a pair of log-policies (fp64 only).  Rows outside the support are identity rows of the Jacobian."""
    m, A, _ = Q.shape
    pr, pc = np.where(onr, np.exp(lr), 0.0), np.where(onc, np.exp(lc), 0.0)
    qr, qc = _responses(Q, pr, pc)
    sr, sc = _softmax(lmr + qr * inv_eta, onr), _softmax(lmc + qc * inv_eta, onc)
    G = np.concatenate([pr - sr, pc - sc], axis=1)
    Jr = sr[:, :, None] * np.eye(A)[None] - sr[:, :, None] * sr[:, None, :]
    Jc = sc[:, :, None] * np.eye(A)[None] - sc[:, :, None] * sc[:, None, :]
    J = np.zeros((m, 2 * A, 2 * A))
    J[:, :A, :A] = np.eye(A)
    J[:, A:, A:] = np.eye(A)
    J[:, :A, A:] = -np.matmul(Jr, Q) * inv_eta                       # d softmax_r / d pc
    J[:, A:, :A] = np.matmul(Jc, Q.transpose(0, 2, 1)) * inv_eta    # d softmax_c / d pr  (qc = -Q^T pr)
    try:
        step = np.linalg.solve(J, G[:, :, None])[:, :, 0]
    except np.linalg.LinAlgError:
        return lr, lc
    step = np.where(np.abs(step).max(axis=1, keepdims=True) < 0.05, step, 0.0)  # a Newton step is only trusted close to the solution
    p = np.concatenate([pr, pc], axis=1) - step
    qr, qc = _responses(Q, p[:, :A], p[:, A:])
    return _normalise(lmr + qr * inv_eta, onr), _normalise(lmc + qc * inv_eta, onc)


def _solve_level(Q, lmr, lmc, onr, onc, eta, tol, max_iters, dtype, col_sign=1.0, polish=False):
    """The extragradient iteration of csrc/reg_solve.hip on the states of one level; a state leaves when its residual is <= tol."""
    m, A, _ = Q.shape
    eta, tol = dtype(eta), dtype(tol)
    inv_eta = dtype(1) / eta
    tau = (dtype(0.5) / np.maximum(np.abs(Q).reshape(m, -1).max(axis=1), dtype(1e-6))).astype(dtype)[:, None]
    tau_eta = tau * eta
    inv_1p = dtype(1) / (dtype(1) + tau_eta)
    lr, lc = _normalise(lmr, onr), _normalise(lmc, onc)
    out = dict(lr=lr.copy(), lc=lc.copy(), pr=np.zeros_like(lr), pc=np.zeros_like(lc), qr=np.zeros_like(lr), qc=np.zeros_like(lc),
               res=np.zeros((m,), dtype), it=np.zeros((m,), np.int32))
    act = np.arange(m)
    it = 0
    while act.size:
        pr, pc = np.where(onr[act], np.exp(lr), 0).astype(dtype), np.where(onc[act], np.exp(lc), 0).astype(dtype)
        qr, qc = _responses(Q[act], pr, pc, col_sign)
        res = np.maximum(_residual(pr, lmr[act], qr, onr[act], inv_eta), _residual(pc, lmc[act], qc, onc[act], inv_eta))
        if polish and it % POLISH_EVERY == POLISH_EVERY - 1:
            nr, nc = _newton(Q[act], lmr[act], lmc[act], onr[act], onc[act], lr, lc, inv_eta)
            npr, npc = np.where(onr[act], np.exp(nr), 0.0), np.where(onc[act], np.exp(nc), 0.0)
            nqr, nqc = _responses(Q[act], npr, npc)
            nres = np.maximum(_residual(npr, lmr[act], nqr, onr[act], inv_eta), _residual(npc, lmc[act], nqc, onc[act], inv_eta))
            better = (nres < 0.5 * res)[:, None]
            lr, lc, pr, pc, qr, qc = (np.where(better, a, b) for a, b in ((nr, lr), (nc, lc), (npr, pr), (npc, pc), (nqr, qr), (nqc, qc)))
            res = np.where(better[:, 0], nres, res)
        done = (res <= tol) if it < max_iters else np.ones(act.size, bool)
        if done.any():
            d = act[done]
            for key, a in (("lr", lr), ("lc", lc), ("pr", pr), ("pc", pc), ("qr", qr), ("qc", qc), ("res", res)):
                out[key][d] = a[done]
            out["it"][d] = it
            keep = ~done
            act, lr, lc, qr, qc = act[keep], lr[keep], lc[keep], qr[keep], qc[keep]
            if not act.size:
                break
        te, tt, ip = tau_eta[act], tau[act], inv_1p[act]
        hr = _normalise((lr + te * lmr[act] + tt * qr) * ip, onr[act])
        hc = _normalise((lc + te * lmc[act] + tt * qc) * ip, onc[act])
        qhr, qhc = _responses(Q[act], np.where(onr[act], np.exp(hr), 0).astype(dtype), np.where(onc[act], np.exp(hc), 0).astype(dtype), col_sign)
        lr = _normalise((lr + te * lmr[act] + tt * qhr) * ip, onr[act])
        lc = _normalise((lc + te * lmc[act] + tt * qhc) * ip, onc[act])
        it += 1
    return out


def solve(name, log_reg, eta, dtype=np.float64, tol=None, max_iters=None, variant=None, only_levels=None):
    """dict(policy, log_policy [S, 2A], values, residual [S] in `dtype`, iters int32 [S]).  dtype fp64: tol 1e-12 with Newton polish,
    the reference; fp32: the restatement of the kernel at tol / max_iters.  variant: one of VARIANTS, a deliberately wrong program."""
    assert variant is None or variant in VARIANTS
    tree = tree_arrays(name)
    mask = legal_mask(tree)
    S, A2 = mask.shape
    A = A2 // 2
    ref = dtype == np.float64 and variant is None and tol is None
    tol = (1e-12 if dtype == np.float64 else TOL) if tol is None else tol
    max_iters = (100000 if ref else MAX_ITERS) if max_iters is None else max_iters
    reg = np.asarray(log_reg)
    on = mask & (reg > -np.inf)
    if variant == "no_magnet":
        lm = np.zeros((S, A2), dtype)
    else:
        lm = np.where(on, np.where(on, reg, 0), 0).astype(dtype)
    policy = np.zeros((S, A2), dtype)
    log_policy = np.full((S, A2), -np.inf, dtype)
    V, residual, iters = np.zeros((S,), dtype), np.zeros((S,), dtype), np.zeros((S,), np.int32)
    e = dtype(eta)
    for st in reversed(levels_of(name)):
        Q = _q_matrix(tree, st, V, dtype, no_chance=variant == "no_chance")
        o = _solve_level(Q, lm[st, :A], lm[st, A:], on[st, :A], on[st, A:], eta, tol, max_iters, dtype,
                         col_sign=-1.0 if variant == "col_sign" else 1.0, polish=ref)
        game = _seqsum(o["pr"] * (o["qr"]))[:, 0]
        kl_r = _seqsum(o["pr"] * (o["lr"] - lm[st, :A]))[:, 0]
        kl_c = _seqsum(o["pc"] * (o["lc"] - lm[st, A:]))[:, 0]
        V[st] = game - e * kl_r + (dtype(0) if variant == "no_opp_kl" else e * kl_c)
        policy[st] = np.concatenate([o["pr"], o["pc"]], axis=1)
        log_policy[st] = np.where(on[st], np.concatenate([o["lr"], o["lc"]], axis=1), -np.inf)
        residual[st], iters[st] = o["res"], o["it"]
    return dict(policy=policy, log_policy=log_policy, values=V, residual=residual, iters=iters)


# ---------------------------------------------------------------------------------------------------- gates
def check(name, log_reg, eta, out):
    """fp64 audit of a solver's outputs: dict(res64 [S], v64 [S], gate_b [S], reached [n]) -- res64 and v64 from the returned policy,
    log-policy and the returned values of the state's own children."""
    tree = tree_arrays(name)
    mask = legal_mask(tree)
    S, A2 = mask.shape
    A, C = A2 // 2, np.asarray(tree["index"]).shape[1]
    reg = np.asarray(log_reg, np.float64)
    on = mask & (reg > -np.inf)
    lm = np.where(on, np.where(on, reg, 0), 0)
    pi = np.asarray(out["policy"], np.float64)
    with np.errstate(invalid="ignore"):
        lp = np.where(on, np.asarray(out["log_policy"], np.float64), 0.0)
    V = np.asarray(out["values"], np.float64)
    reached = np.concatenate(levels_of(name))
    res64, v64, B = np.zeros(S), np.zeros(S), np.zeros(S)
    st = reached
    Q = _q_matrix(tree, st, V, np.float64)
    idx = np.asarray(tree["index"])[st]
    ch = np.asarray(tree["chance"], np.float64)[st]
    live = ch > 0
    nxt = np.where(live, idx, 0)
    absQ = np.where(live, ch * np.abs(np.where(nxt == 0, np.asarray(tree["value"], np.float64)[st], V[nxt])), 0.0).sum(axis=1)
    pr, pc = pi[st, :A], pi[st, A:]
    qr, qc = np.einsum("mrc,mc->mr", Q, pc), -np.einsum("mrc,mr->mc", Q, pr)
    res64[st] = np.maximum(_residual(pr, lm[st, :A], qr, on[st, :A], 1.0 / eta), _residual(pc, lm[st, A:], qc, on[st, A:], 1.0 / eta))
    klr, klc = pr * (lp[st, :A] - lm[st, :A]), pc * (lp[st, A:] - lm[st, A:])
    v64[st] = np.einsum("mr,mrc,mc->m", pr, Q, pc) - eta * klr.sum(1) + eta * klc.sum(1)
    B[st] = np.einsum("mr,mrc,mc->m", pr, absQ, pc) + eta * np.abs(klr).sum(1) + eta * np.abs(klc).sum(1)
    q_max = np.zeros(S)
    q_max[st] = absQ.reshape(len(st), -1).max(axis=1)
    return dict(res64=res64, v64=v64, gate_b=(A * A * C + 2 * A + 8) * U * B, reached=reached, q_max=q_max)


def anchor_bound(name, eta, out):
    """[S]: bound on |V[s] - root_value[s]| when mu = the tree's solution and the solver answered pi = mu within 8 * 2^-24 per entry
    (asserted next to it).  root_value is the tree builder's own bottom-up fp32 sweep (tree.py:280-300): evm = sum_t value * chance with
    the children's root_value in the value slots, root_value = (p1 @ evm) @ p2 on the fp32 solution.  V is the same bilinear form on Q,
    so the two differ, per state, by
      - the roundings of the two fp32 evaluations: gate (b) once for each, the builder's having no more operations than ours;
      - the policy: |pi - solution| <= 8 * 2^-24 per entry moves a bilinear form by at most 2 * A * 8 * 2^-24 * max|Q|;
      - the two KL terms, which root_value does not have.  With pi = mu, log pi - log mu = -logsumexp(log mu) plus the roundings of
        the normalisation: at most (2A + 4 + 2 |log pi(a)|) * 2^-24 for action a, and sum_a pi(a) |log pi(a)| <= log A < 2.5, so each
        KL term is at most (2A + 9) * 2^-24 in size and enters V times eta;
      - the children: their differences enter Q through the chance weights of one joint action, and the value of a bilinear form on
        two distributions moves by at most the largest entry's change: max over (r, c) of sum_t chance * bound[child].
    The last item makes the bound grow with the height of the state; the others are its own level's."""
    tree = tree_arrays(name)
    S, C, A, _ = np.asarray(tree["index"]).shape
    c = check(name, magnet(name, "solution", eta), eta, out)
    own = 2 * c["gate_b"] + 16 * A * U * c["q_max"] + 2 * eta * (2 * A + 9) * U
    idx, ch = np.asarray(tree["index"]), np.asarray(tree["chance"], np.float64)
    bound = np.zeros(S)
    for st in reversed(levels_of(name)):
        live = ch[st] > 0
        nxt = np.where(live, idx[st], 0)
        below = np.where(live, ch[st] * bound[nxt], 0.0).sum(axis=1).reshape(len(st), -1).max(axis=1)  # (bound[0] = 0: terminal)
        bound[st] = own[st] + below
    return bound


def shares(name, log_reg, eta, out, tol=TOL):
    """(worst res64 / tol, worst |V - V64| / gate (b)) over the reached states."""
    c = check(name, log_reg, eta, out)
    st = c["reached"]
    err = np.abs(np.asarray(out["values"], np.float64)[st] - c["v64"][st])
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(err == 0, 0.0, err / c["gate_b"][st])
    return float(c["res64"][st].max() / tol), float(b.max())


@functools.lru_cache(maxsize=None)
def star(name, kind, eta):
    """The fp64 fixed point of one input, computed once and read-only."""
    out = solve(name, magnet(name, kind, eta), eta, np.float64)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name, kind, eta):
    """(log_reg fp32, fp64 fixed point, fp32 restatement) of one input, computed once and read-only."""
    reg = magnet(name, kind, eta)
    rest = solve(name, reg, eta, np.float32)
    for a in rest.values():
        a.setflags(write=False)
    return reg, star(name, kind, eta), rest


def distance(name, out, star):
    st = np.concatenate(levels_of(name))
    dp = float(np.abs(np.asarray(out["policy"], np.float64)[st] - star["policy"][st]).max())
    dv = float(np.abs(np.asarray(out["values"], np.float64)[st] - star["values"][st]).max())
    return dp, dv


def cases():
    return [(n, k, e) for n in ALL_TREES for e in ETAS for k in MAGNETS]


@functools.lru_cache(maxsize=None)
def gate_c():
    """(policy gate, value gate, worst case ids): twice the worst distance of the fp32 restatement to the fp64 fixed point over cases()."""
    worst_p, worst_v, at_p, at_v = 0.0, 0.0, None, None
    for n, k, e in cases():
        _, star, rest = case(n, k, e)
        dp, dv = distance(n, rest, star)
        if dp > worst_p:
            worst_p, at_p = dp, (n, k, e)
        if dv > worst_v:
            worst_v, at_v = dv, (n, k, e)
    return 2 * worst_p, 2 * worst_v, (at_p, at_v)


COMMITTED_ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "profiles", "reg_solve_errors.json")


def committed_gate_c():
    """(policy gate, value gate) as profiles/reg_solve_errors.json records them for the fp32 restatement.  gate_c() needs every case's
    restatement and reference; a GPU test needs its own cases only, and reads the gate here.  tests/test_reg_solve.py holds the file
    to what gate_c() computes."""
    with open(COMMITTED_ERRORS) as f:
        rec = json.load(f)["fp32_restatement"]
    return float(rec["policy_gate"]), float(rec["value_gate"])


def update_errors_file(key, figures):
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "reg_solve_errors.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------- the built kernels
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
_KERNEL = re.compile(r"k_reg_solveILi(\d+)EE")
_BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def kernel_metadata(so_path, arch="gfx950"):
    """{A: dict(scratch, vgpr, sgpr)} of every k_reg_solve instantiation in the built library, read as tests/_rowsref.py reads the rows
    kernels': .hip_fatbin -> its offload bundles -> the gfx950 code object -> the amdhsa.kernels note.  A missing tool is an error."""
    tools = {t: os.path.join(LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    kernels = []
    with tempfile.TemporaryDirectory(prefix="reg_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(_BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_reg_solve" not in part:
                continue
            bundle, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(bundle, "wb").write(part)
            subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}",
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
            table[int(m.group(1))] = dict(scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"]), sgpr=int(k[".sgpr_count"]))
    return table
