"""Inputs, the reference and the error bound of the learner sweep (csrc/learn_math.hpp, k_learn_fused, k_row_sums, the bucketed learners of
csrc/bucket.hip) -- tests/test_learn_shapes.py on the CPU, tests/test_hip_learn_shapes.py on the GPU.  numpy only; nothing here calls a
project kernel or imports the package.

`learner(dtype, batch, slots, hp)` is the per-slot program of the reference's RNaD.__learn (learn/rnad.py:365-425, learn/vtrace.py, the
policy head of nn/net.py:74-77), written from that Python and generic in the number format: with np.float64 it is the reference, with
np.float32 the stand-in for a correct kernel.  The five net outputs (logit, v, v_target, logit_reg, logit_reg_) are synthetic inputs, per
slot [T, B, (A)] or, where the batch carries S, per (player, state) row [2S, (A)] with row = player * S + state.

Every value carries a MAGNITUDE (class VM): mag(x +- y) = mag x + mag y, mag(x y) = mag x mag y, mag(x / y) = mag x / |y|, mag(c) = |c|,
mag(exp x) = exp(x) (1 + |x|), mag(log x) = |log x| + mag x / |x|; min / max / select take the magnitude of the operand taken;
pi_processed is exact (multiples of 1 / n_disc) and carries its value.  The gate of an output is K 2^-24 mag(output); the constants K per
output family are measured in tests/test_learn_shapes.py from two fp32 programs on these very inputs, never from a kernel.  A row table
(sums over the slots of a row) has K 2^-24 (sum of the slots' magnitudes) plus the fixed-point term: slots * half a unit (`row_sums_unit`,
`bucketed_units`, restated from csrc/learn.hip and csrc/bucket.hip).

The program has two kinds of discontinuity, both functions of a row's logits and legal mask alone: the decisions of process_policy
(pi >= eps, the rank order of p, ceil(n_disc p)) and the two threshold gates of apply_force_with_threshold.  `row_margin` is the smallest
distance of any of them from its boundary; `draw_logits` redraws every row below MARGIN until none is left, so that no comparison needs to
reject a row.  Decisions on operands that are exact in both formats (p = 0 or 1, an illegal action) have no boundary."""
import functools
import types

import numpy as np

U = 2.0 ** -24
MARGIN = 1e-4
FAMILIES = ("pi", "v_target", "q", "dlogit", "dv", "losses", "tables")
# the smallest power of two >= twice the worst share of 2^-24 mag that the two fp32 programs of tests/test_learn_shapes.py use on the
# sweep's inputs (profiles/learn_errors.json, section "cpu")
K = {"pi": 16, "v_target": 8, "q": 16, "dlogit": 16, "dv": 8, "losses": 4, "tables": 8}

SHARES = {}  # case -> {output: worst share of the gate}; the test modules log it


# ------------------------------------------------------------------------------------------------ hyperparameter sets
def _hp(alpha, eta, lambda_=1.0, c=1.0, rho=1.0, gamma=1.0, clip=1e3, threshold=2.0, w_v=1.0, w_n=1.0, eps=0.03, n_disc=32):
    """The values as the kernels receive them: every float rounded to fp32, 1 - alpha taken in double first (rnad.py:382)."""
    f = lambda x: float(np.float32(x))  # noqa: E731
    return types.SimpleNamespace(alpha=f(alpha), one_minus_alpha=f(1.0 - float(alpha)), eta=f(eta), lambda_=f(lambda_), c=f(c), rho=f(rho),
                                 gamma=f(gamma), clip=f(clip), threshold=f(threshold), w_v=f(w_v), w_n=f(w_n), eps=f(eps), n_disc=int(n_disc))


HP = {
    "H0": _hp(alpha=0.5, eta=0.2),  # RNaD's own defaults (learn/rnad.py:41-71; lambda_ = 1.0 at :397)
    "H1": _hp(alpha=0.3, eta=0.5, lambda_=0.8, c=0.7, rho=1.4, gamma=0.9, clip=0.5, threshold=1.0, w_v=0.7, w_n=1.3, eps=0.03, n_disc=32),
    "H2": _hp(alpha=1.0, eta=0.0, lambda_=0.9, c=1.5, rho=0.6, gamma=0.95, threshold=0.5, eps=0.2, n_disc=16),
    "H3": _hp(alpha=0.3, eta=0.5, lambda_=0.8, c=0.7, rho=1.4, gamma=0.9, clip=2.0 ** 30, threshold=1.0, w_v=0.7, w_n=1.3, eps=0.03, n_disc=32),
}
SETS = tuple(HP)


def hp_kwargs(hp):
    """Arguments of rnad_hip.make_learn_params."""
    return dict(alpha=hp.alpha, eta=hp.eta, lambda_=hp.lambda_, c=hp.c, rho=hp.rho, gamma=hp.gamma, clip=hp.clip, threshold=hp.threshold,
                w_v=hp.w_v, w_n=hp.w_n, eps_threshold=hp.eps, n_disc=hp.n_disc)


# ------------------------------------------------------------------------------------------------ fixed-point units, restated
FIXED_BITS = 40  # csrc/learn.hip kFixedBits; csrc/bucket.hip 62 - kLaneBits


def row_sums_unit(col_max):
    """k_row_sums (csrc/learn.hip): one unit of a column whose largest |addend| is col_max: 2^(e - 40), e the exponent with max < 2^e."""
    if col_max == 0:
        return 1.0
    e = int(np.floor(np.log2(float(np.float32(col_max))))) + 1
    return 2.0 ** (e - FIXED_BITS)


def bucketed_exponents(hp):
    """fixed_point_for (csrc/bucket.hip): e_l is the smallest e in 1 .. 30 with 2^e > 2 clip, e_v = 11; check_l: 2 clip does not fit."""
    e_l = 1
    while 2.0 ** e_l <= 2.0 * abs(hp.clip) and e_l < 30:
        e_l += 1
    return e_l, 11, not (2.0 * abs(hp.clip) < 2.0 ** e_l)


def bucketed_units(hp):
    """One unit of an addend of dL/dlogit and of dL/dv BEFORE the scaling by w / N_P: 2^-(40 - e)."""
    e_l, e_v, _ = bucketed_exponents(hp)
    return 2.0 ** -(FIXED_BITS - e_l), 2.0 ** -(FIXED_BITS - e_v)


# ------------------------------------------------------------------------------------------------ values with magnitudes
class VM:
    """A value and its magnitude (module docstring).  Arrays of one dtype; plain numbers and arrays are constants (mag = |c|)."""
    __slots__ = ("v", "m")
    __array_ufunc__ = None  # ndarray op VM goes to VM's reflected operator

    def __init__(self, v, m=None):
        self.v = v
        self.m = np.abs(v) if m is None else m

    @staticmethod
    def of(x):
        return x if isinstance(x, VM) else VM(x)

    def __add__(self, o):
        o = VM.of(o)
        return VM(self.v + o.v, self.m + o.m)

    __radd__ = __add__

    def __sub__(self, o):
        o = VM.of(o)
        return VM(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return VM.of(o) - self

    def __mul__(self, o):
        o = VM.of(o)
        return VM(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = VM.of(o)
        return VM(self.v / o.v, self.m / np.abs(o.v))

    def __neg__(self):
        return VM(-self.v, self.m)

    def __getitem__(self, i):
        return VM(self.v[i], self.m[i])

    def exp(self):
        e = np.exp(self.v)
        return VM(e, e * (1 + np.abs(self.v)))

    def log(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return VM(np.log(self.v), np.abs(np.log(self.v)) + self.m / np.abs(self.v))

    def sum_last(self):
        """Sum over the last axis in index order."""
        out = self[..., 0]
        for a in range(1, self.v.shape[-1]):
            out = out + self[..., a]
        return out

    def take(self, idx):
        i = idx[..., None]
        return VM(np.take_along_axis(self.v, i, -1)[..., 0], np.take_along_axis(self.m, i, -1)[..., 0])

    def expand(self):
        return VM(self.v[..., None], self.m[..., None])


def where(c, a, b):
    a, b = VM.of(a), VM.of(b)
    return VM(np.where(c, a.v, b.v), np.where(c, a.m, b.m))


def minimum(a, b):
    a, b = VM.of(a), VM.of(b)
    return where(a.v <= b.v, a, b)


def maximum(a, b):
    a, b = VM.of(a), VM.of(b)
    return where(a.v >= b.v, a, b)


# ------------------------------------------------------------------------------------------------ the program
def policy_head(dtype, logit, legal):
    """nn/net.py:74-77 -> (pi, log_pi) as VM."""
    lg = VM(logit.astype(dtype))
    on = legal > 0
    ex = where(on, lg.exp(), dtype(0))
    s = ex.sum_last()  # the L1 norm of F.normalize and the plain sum are the same number: every term is >= 0
    pi = ex / maximum(s, dtype(1e-12)).expand()
    log_pi = where(on, lg - s.log().expand(), dtype(0))
    return pi, log_pi


def process_policy(dtype, pi, legal, n_disc, eps):
    """learn/vtrace.py:24-55 on rows [N, A] of plain values -> (result, p, survivors mask)."""
    N, A = pi.shape
    eps, n = dtype(eps), dtype(n_disc)
    legal = legal.astype(dtype)
    mask = legal * ((pi >= eps) | (pi.max(-1, keepdims=True) < eps))
    mp = mask * pi
    s = mp[:, 0].copy()
    for a in range(1, A):
        s = s + mp[:, a]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = mp / s[:, None]
    blocks = np.ceil(n * p)
    order = np.argsort(-p, axis=-1, kind="stable")
    rows = np.arange(N)
    result = np.zeros_like(p)
    leftover = np.full(N, n, dtype)
    for i in range(A):
        x = np.minimum(leftover, blocks[rows, order[:, i]])
        leftover = leftover - x
        result[rows, order[:, i]] += x
    return result / n, p, mask


def row_margin(logit, legal, hp):
    """fp64: the smallest distance of a decision of the rows [N, A] from its boundary (module docstring)."""
    A = logit.shape[-1]
    on = legal > 0
    pi, _ = policy_head(np.float64, logit, legal)
    pi = pi.v
    big = np.float64(1e9)
    m = np.where(on, np.abs(pi - hp.eps), big).min(-1)  # pi >= eps, max < eps (the maximum is one of them)
    _, p, mask = process_policy(np.float64, pi, legal, hp.n_disc, hp.eps)
    live = mask > 0
    several = live.sum(-1, keepdims=True) > 1  # a single survivor has p == 1 exactly in both formats
    x = hp.n_disc * p
    m = np.minimum(m, np.where(live & several, np.abs(x - np.round(x)), big).min(-1))  # ceil(n_disc p)
    ps = np.sort(np.where(live, p, -np.arange(1, A + 1, dtype=np.float64)), -1)  # the dead ones apart from each other and from the live
    if A > 1:
        gap = np.diff(ps, axis=-1)
        m = np.minimum(m, np.where(ps[:, :-1] > 0, gap, big).min(-1))  # the rank order of p
    mean = (logit.astype(np.float64) * legal).sum(-1, keepdims=True) / A
    l = logit - mean
    m = np.minimum(m, np.where(on, np.abs(np.abs(l) - hp.threshold), big).min(-1))  # l > -thr, l < thr
    return m


MUTANTS = ("gamma_nv", "lambda", "rho_c", "inv_mu", "mean_legal", "reward_sign", "others_sign", "alpha", "row_slot")


def learner(dtype, batch, slots, hp, mutate=None):
    """The module docstring's program.  batch: indices [T, B] (0: invalid), legal [T, B, A] 0 / 1, actions [T, B], rewards [T, B],
    mu [T, B, A], and S where `slots` are row tables.  slots: logit, v, v_target, logit_reg, logit_reg_.  The player to move at step t is
    t & 1.  -> namespace of VM outputs (value .v, magnitude .m): pi, pi_processed, v_target [2, T, B], q [2, T, B, A], dlogit, dv, losses
    [2] (loss_v, loss_nerd, unweighted), with S also dlogit_tab [2S, A], dv_tab [2S], row_slots [2S]; margin [T, B]; norm [2]."""
    assert mutate is None or mutate in MUTANTS
    idx = np.asarray(batch["indices"])
    T, B = idx.shape
    A = batch["mu"].shape[-1]
    S = batch.get("S")
    valid = idx != 0
    turn = (np.arange(T) & 1)[:, None] + np.zeros((1, B), np.int64)
    if S is None:
        g = lambda x: np.asarray(x)  # noqa: E731
    else:
        rows = turn * S + idx
        g = lambda x: np.asarray(x)[rows]  # noqa: E731
    logit, v, vtn, lreg, lreg_ = (g(slots[k]).astype(dtype) for k in ("logit", "v", "v_target", "logit_reg", "logit_reg_"))
    v, vtn = v.reshape(T, B), vtn.reshape(T, B)
    legal = np.asarray(batch["legal"]).astype(dtype)
    mu = VM(np.asarray(batch["mu"]).astype(dtype))
    act = np.asarray(batch["actions"]).astype(np.int64)
    rew = np.asarray(batch["rewards"]).astype(dtype)
    oh = (np.arange(A) == act[..., None])
    one, zero = dtype(1), dtype(0)

    pi, log_pi = policy_head(dtype, logit, legal)  # rnad.py:373
    _, log_reg = policy_head(dtype, lreg, legal)  # :379
    _, log_reg_ = policy_head(dtype, lreg_, legal)  # :380
    pp, _, _ = process_policy(dtype, pi.v.reshape(T * B, A), legal.reshape(T * B, A), hp.n_disc, hp.eps)  # :374
    pip = VM(pp.reshape(T, B, A))
    a0, a1 = dtype(hp.alpha), dtype(hp.one_minus_alpha)
    if mutate == "alpha":
        a1 = a0
    lpol = log_pi - (a0 * log_reg + a1 * log_reg_)  # :382

    gamma, lam, eta = dtype(hp.gamma), dtype(hp.lambda_), dtype(hp.eta)
    rho, cbar = (dtype(hp.c), dtype(hp.rho)) if mutate == "rho_c" else (dtype(hp.rho), dtype(hp.c))
    if mutate == "lambda":
        lam = one
    vf = valid.astype(dtype)
    ent = (pip * lpol).sum_last()
    # _policy_ratio (vtrace.py:199-204)
    sel = lambda x: x.take(act) * vf + (one - vf)  # noqa: E731
    sel_mu = sel(mu)
    cs = sel(pip) / sel_mu
    inv_mu = VM(np.ones((T, B), dtype)) if mutate == "inv_mu" else (VM(np.ones((T, B), dtype)) * vf + (one - vf)) / sel_mu
    vts, qs = [], []
    for player in range(2):
        r_p = rew if player == 0 or mutate == "reward_sign" else -rew  # rnad.py:368
        ours_t = turn == player
        po = (2 * ours_t - 1).astype(dtype) * vf  # _player_others (:83-87)
        if mutate == "others_sign":
            po = vf
        ere = (-eta) * ent * po  # :234-238
        elp = (-eta) * lpol * po[..., None]  # :239
        z = VM(np.zeros(B, dtype))
        c_r, c_ru, c_nv, c_nvt, c_is = z, z, z, z, VM(np.ones(B, dtype))
        vt_out, q_out = [None] * T, [None] * T
        for t in range(T - 1, -1, -1):
            vv, rw = VM(vtn[t]), VM(r_p[t])
            ru = rw + gamma * c_ru + ere[t]  # :262
            dr = rw + gamma * c_r  # :263
            w = cs[t] * c_is
            our_vt = vv + minimum(w, rho) * (ru + gamma * c_nv - vv) + lam * minimum(w, cbar) * gamma * (c_nvt - c_nv)  # :266-282
            tail = dr + gamma * c_is * c_nvt - vv
            our_q = vv.expand() + elp[t] + where(oh[t], (inv_mu[t] * tail).expand(), zero)  # :288-300
            ours = valid[t] & ours_t[t]
            opp = valid[t] & ~ours_t[t]
            vt_out[t] = where(ours, our_vt, zero)
            q_out[t] = where(ours[:, None], our_q, zero)
            opp_nv = c_nv if mutate == "gamma_nv" else gamma * c_nv
            c_r = where(ours, zero, where(opp, ere[t] + cs[t] * dr, zero))  # :306-320
            c_ru = where(ours, zero, where(opp, ru, zero))
            c_nv, c_nvt = where(ours, vv, where(opp, opp_nv, zero)), where(ours, our_vt, where(opp, gamma * c_nvt, zero))
            c_is = where(ours, one, where(opp, w, one))
        vts.append(VM(np.stack([x.v for x in vt_out]), np.stack([x.m for x in vt_out])))
        qs.append(VM(np.stack([x.v for x in q_out]), np.stack([x.m for x in q_out])))

    # losses (vtrace.py:377-431) and the closed-form gradients: the force is detached, d/dlogit sum_a legal l f = w - legal sum(w) / A
    mover = valid[None] & (turn[None] == np.arange(2)[:, None, None])  # has_played_P = valid && turn == P
    count = mover.sum((1, 2))
    norm = (count + (count == 0)).astype(dtype)
    nslot = VM(norm[turn])
    vt_p = where(turn == 0, vts[0], vts[1])
    q_p = where((turn == 0)[..., None], qs[0], qs[1])
    d = VM(v) - vt_p
    sq = where(valid, d * d / nslot, zero)
    dv = where(valid, dtype(hp.w_v) * (dtype(2) * d / nslot), zero)
    base = (pip * q_p).sum_last()
    adv = q_p - base.expand()
    clip = dtype(hp.clip)
    adv = maximum(minimum(adv, clip), -clip)  # :417
    lgv = VM(logit)
    mean = (lgv * legal).sum_last() / (np.maximum(legal.sum(-1), 1).astype(dtype) if mutate == "mean_legal" else dtype(A))  # :420
    l = lgv - mean.expand()
    thr = dtype(hp.threshold)
    f = where(l.v > -thr, minimum(adv, zero), zero) + where(l.v < thr, maximum(adv, zero), zero)  # :362-366
    nerd = (legal * (l * f)).sum_last()
    wgt = legal * f
    grad = wgt - legal * wgt.sum_last().expand() / dtype(A)
    dlogit = where(valid[..., None], dtype(hp.w_n) * (-grad / nslot.expand()), zero)
    nl = where(valid, -nerd / nslot, zero)
    # the sum of a loss over the slots: the per-slot terms in the format of the program, added in fp64 as one running sum over [T, B] in
    # storage order (a fixed order, whatever the numpy build; the kernels and the oracle add their fp32 terms in fp64 too)
    total = lambda x: VM(np.cumsum(x.v.ravel(), dtype=np.float64)[-1:], np.cumsum(x.m.ravel(), dtype=np.float64)[-1:])  # noqa: E731
    lv, ln = total(sq), total(nl)
    out = types.SimpleNamespace(pi=pi, pi_processed=pip, v_target=VM(np.stack([x.v for x in vts]), np.stack([x.m for x in vts])),
                                q=VM(np.stack([x.v for x in qs]), np.stack([x.m for x in qs])), dlogit=dlogit, dv=dv,
                                losses=VM(np.concatenate([lv.v, ln.v]), np.concatenate([lv.m, ln.m])), norm=norm, valid=valid, turn=turn)
    if S is not None:
        keep = valid.copy()
        if mutate == "row_slot":
            keep[np.unravel_index(np.flatnonzero(valid)[-1], valid.shape)] = False  # one slot left out of its row's sum
        r = rows[keep]

        def tab(x, shape):  # both kernels add a row's slots in fixed point: the sum is exact up to that term, whatever the format of the slots
            z = np.zeros(shape, np.float64)
            np.add.at(z, r, x[keep].astype(np.float64))
            return z

        out.dlogit_tab = VM(tab(dlogit.v, (2 * S, A)), tab(dlogit.m, (2 * S, A)))
        out.dv_tab = VM(tab(dv.v, (2 * S,)), tab(dv.m, (2 * S,)))
        out.row_slots = np.bincount(rows[valid], minlength=2 * S)
    if dtype is np.float64:
        out.margin = row_margin(logit.reshape(T * B, A), legal.reshape(T * B, A), hp).reshape(T, B)
    return out


# ------------------------------------------------------------------------------------------------ gates and shares
def share(got, want):
    """The worst |got - want.v| / (2^-24 want.m) over all elements; an element of magnitude zero must be exact."""
    got = np.asarray(got, np.float64).reshape(want.v.shape)
    err = np.abs(got - want.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(want.m > 0, err / (U * want.m), np.where(err == 0, 0.0, np.inf))
    return float(s.max()) if s.size else 0.0


def table_share(got, want, fixed):
    """The same for a row table whose gate has the additive fixed-point term `fixed` (an array like want.v): the share of
    K 2^-24 mag + fixed that the error uses, expressed as err / (2^-24 mag + fixed / K['tables'])."""
    got = np.asarray(got, np.float64).reshape(want.v.shape)
    err = np.abs(got - want.v)
    den = U * want.m + np.broadcast_to(fixed, err.shape) / K["tables"]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    return float(s.max()) if s.size else 0.0


def log_share(case, name, value):
    SHARES.setdefault(case, {})[name] = round(float(value), 3)


# ------------------------------------------------------------------------------------------------ inputs
def draw_logits(rng, legal, hp, scale):
    """Logits [N, A] ~ scale[row] N(0, 1), every row redrawn until its fp64 decision margin is at least MARGIN."""
    N, A = legal.shape
    logit = (rng.standard_normal((N, A)) * scale[:, None]).astype(np.float32)
    for _ in range(200):
        bad = np.flatnonzero(~(row_margin(logit, legal, hp) >= MARGIN))
        if bad.size == 0:
            return logit
        logit[bad] = (rng.standard_normal((bad.size, A)) * scale[bad, None]).astype(np.float32)
    raise AssertionError("rows below the decision margin remain")


def draw_legal(rng, N, A):
    legal = (rng.random((N, A)) < 0.8).astype(np.float32)
    legal[np.arange(N), rng.integers(0, A, N)] = 1.0
    return legal


def draw_scale(rng, N):
    """Most rows have logits of scale 1.5; one in five is nearly uniform (the all-below-eps branch, an exhausted leftover)."""
    return np.where(rng.random(N) < 0.2, 0.1, 1.5)


def draw_tables(rng, legal, hp):
    """The five net outputs for rows with the given legal masks [N, A]."""
    N, A = legal.shape
    return dict(logit=draw_logits(rng, legal, hp, draw_scale(rng, N)), v=(0.6 * rng.standard_normal(N)).astype(np.float32),
                v_target=(0.6 * rng.standard_normal(N)).astype(np.float32), logit_reg=(1.5 * rng.standard_normal((N, A))).astype(np.float32),
                logit_reg_=(1.5 * rng.standard_normal((N, A))).astype(np.float32))


def behaviour(rng, legal):
    """mu [.., A] float32, independent of the learner's policy, and actions drawn from it (a row without a legal action: zeros, action 0)."""
    z = rng.standard_normal(legal.shape)
    e = np.where(legal > 0, np.exp(z), 0.0)
    mu = (e / np.maximum(e.sum(-1, keepdims=True), 1e-300)).astype(np.float32)
    cdf = np.cumsum(mu.astype(np.float64), -1)
    u = rng.random(legal.shape[:-1] + (1,)) * cdf[..., -1:]
    act = np.minimum((u >= cdf).sum(-1), legal.shape[-1] - 1)
    act = np.where(np.take_along_axis(legal, act[..., None], -1)[..., 0] > 0, act, legal.argmax(-1))  # (u at the very end of the cdf)
    return mu, act.astype(np.int32)


# native trees (rnad_hip.tree_generate; none has more than 5 000 states) and the batch played on each
TREES = {
    1: dict(A=1, C=2, depth_bound=6, transition_threshold=0.1, seed=11),
    2: dict(A=2, C=1, depth_bound=4, seed=12),
    3: dict(A=3, C=2, depth_bound=4, transition_threshold=0.25, prune=(1, 3), seed=13),  # ragged episode lengths
    4: dict(A=4, C=1, depth_bound=3, seed=14),
    5: dict(A=5, C=4, depth_bound=3, transition_threshold=0.1, prune=(1, 2), seed=15),
    6: dict(A=6, C=1, depth_bound=3, seed=16),
    7: dict(A=7, C=1, depth_bound=3, seed=17),
    8: dict(A=8, C=1, depth_bound=2, seed=18),
}
TREE_B = {A: (3000 if A & 1 else 4096) for A in TREES}
MAX_STATES = 5000


def tree_cases():
    return [(A, s) for A in TREES for s in SETS]


DENSE_T, DENSE_B = (1, 2, 7, 32), (1, 255, 257, 1023)
DENSE_SHAPES = tuple((T, B) for T in DENSE_T for B in DENSE_B)  # the whole cross
A_RANGE = tuple(range(1, 9))


def dense_cases():
    return [(A, s, T, B) for A in A_RANGE for s in SETS for T, B in DENSE_SHAPES]


def case_id(key):
    A, s, T, B = key
    return f"A{A}_{s}_T{T}_B{B}"


def coverage(batch, slots, hp, ref):
    """From the fp64 reference alone: the shares of the mover's valid slots whose importance weight w = cs * is lies below / above rho and
    c, and the shares of the legal actions of valid slots on which the clip binds and on which each threshold gate is closed."""
    idx = batch["indices"]
    T, B = idx.shape
    A = batch["mu"].shape[-1]
    act = np.asarray(batch["actions"]).astype(np.int64)[..., None]
    take = lambda x: np.take_along_axis(x, act, -1)[..., 0]  # noqa: E731
    cs = np.where(ref.valid, take(ref.pi_processed.v) / np.where(ref.valid, take(batch["mu"].astype(np.float64)), 1), 1)
    w = np.zeros((T, B))
    for p in range(2):
        carry = np.ones(B)
        for t in range(T - 1, -1, -1):
            ours = ref.valid[t] & (t & 1 == p)
            w[t] = np.where(ours, cs[t] * carry, w[t])
            carry = np.where(ours, 1.0, np.where(ref.valid[t], cs[t] * carry, 1.0))
    w = w[ref.valid]
    on = (batch["legal"] > 0) & ref.valid[..., None]
    q = np.where((ref.turn == 0)[..., None], ref.q.v[0], ref.q.v[1])
    adv = q - (ref.pi_processed.v * q).sum(-1, keepdims=True)
    logit = np.asarray(slots["logit"], np.float64)
    l = logit - (logit * batch["legal"]).sum(-1, keepdims=True) / A
    mean = lambda x: float(x.mean()) if x.size else 0.0  # noqa: E731
    return dict(w_below_rho=mean(w < hp.rho), w_above_rho=mean(w > hp.rho), w_below_c=mean(w < hp.c), w_above_c=mean(w > hp.c),
                clip=mean(np.abs(adv[on]) > hp.clip), gate_lo=mean(l[on] <= -hp.threshold), gate_hi=mean(l[on] >= hp.threshold))


def covered(key, cov):
    """The conditions of tests/test_learn_shapes.py on a dense case with T >= 7 and A >= 2 (at A = 1 pi = mu = 1 and l = 0 in every row)."""
    names = ("w_below_rho", "w_above_rho", "w_below_c", "w_above_c") + (("clip", "gate_lo", "gate_hi") if key[1] == "H1" else ())
    return all(cov[n] >= 0.05 for n in names)


def _draw_dense(key, attempt):
    A, s, T, B = key
    hp = HP[s]
    rng = np.random.default_rng([A, SETS.index(s), T, B, attempt])
    length = (T - np.arange(B)) % (T + 1)  # lane 0 has all T steps; with B > T every length 0 .. T occurs
    length[1:] = rng.permutation(length[1:])
    valid = np.arange(T)[:, None] < length[None]
    hole = (rng.random(B) < 0.1) & (length >= 3)
    valid[np.minimum(length // 2, T - 1)[hole], np.flatnonzero(hole)] = False
    indices = np.where(valid, rng.integers(1, 100, (T, B)), 0).astype(np.int32)
    legal = draw_legal(rng, T * B, A)
    slots = {k: x.reshape((T, B) + x.shape[1:]) for k, x in draw_tables(rng, legal, hp).items()}
    legal = legal.reshape(T, B, A)
    mu, act = behaviour(rng, legal)
    rewards = np.where(rng.random((T, B)) < 1 / 3, rng.uniform(-1, 1, (T, B)), 0.0).astype(np.float32)
    return dict(indices=indices, legal=legal, actions=act, rewards=rewards, mu=mu), slots


@functools.lru_cache(maxsize=None)
def dense_case(key):
    """(batch, slots) of a dense case: lanes of every length 0 .. T (a single lane: T), a few with an invalid slot in the middle (the
    carry reset), illegal actions at A >= 2, mu independent of the learner, rewards on about a third of the slots.  A batch of ONE lane
    with T >= 7 has too few slots for the coverage conditions to hold by numbers alone: it is drawn again, from the next seed, until the
    fp64 reference shows them (`covered`); nothing of a kernel's or an fp32 program's output enters that choice."""
    A, s, T, B = key
    for attempt in range(1000):
        batch, slots = _draw_dense(key, attempt)
        if B > 1 or T < 7 or A < 2 or covered(key, coverage(batch, slots, HP[s], learner(np.float64, batch, slots, HP[s]))):
            return batch, slots
    raise AssertionError(f"{case_id(key)}: no draw meets the coverage conditions")


@functools.lru_cache(maxsize=None)
def dense_reference(key):
    batch, slots = dense_case(key)
    return learner(np.float64, batch, slots, HP[key[1]])


def mask_bits(legal):
    A = legal.shape[-1]
    return (legal.astype(np.int64) << np.arange(A)).sum(-1).astype(np.uint8)


def legal_table(legal):
    """The legal masks of the (player, state) rows [2S, A] from a tree's legal tensor [S, (1,) A, A] (episode.py:62-68, :208: the row player
    sees legal[s, :, 0], the column player legal[s, 0, :])."""
    legal = np.asarray(legal)
    legal = legal.reshape(legal.shape[0], legal.shape[-1], legal.shape[-1])
    return np.concatenate([legal[:, :, 0], legal[:, 0, :]], 0).astype(np.float32)


def _pick(rng, p):
    """One draw per row of p [N, n] (rows of zeros: 0)."""
    cdf = np.cumsum(p.astype(np.float64), -1)
    u = rng.random((p.shape[0], 1)) * cdf[:, -1:]
    k = np.minimum((u >= cdf).sum(-1), p.shape[1] - 1)
    return np.where(np.take_along_axis(p, k[:, None], -1)[:, 0] > 0, k, p.argmax(-1))


def tree_batch(rng, tree, B, hp):
    """B episodes of a tree (index / chance / value [S, C, A, A], legal [S, A, A]; the root is state 1, the players move in turn, the
    column player's step makes the transition and is paid value * (next == 0)) played OFF-policy: the actor's policy is a row table of its
    own, the learner's five row tables are drawn independently of it.  -> (batch with S, tables)."""
    index, chance, value = (np.asarray(tree[k]) for k in ("index", "chance", "value"))
    S, C, A, _ = index.shape
    legal_tab = legal_table(np.asarray(tree["legal"]))
    mu_tab, _ = behaviour(rng, legal_tab)
    state = np.ones(B, np.int64)
    steps = []
    for t in range(64):
        if not state.any():
            break
        live = state != 0
        mu = np.where(live[:, None], mu_tab[(t & 1) * S + state], np.float32(0))
        act = _pick(rng, mu)
        rew = np.zeros(B, np.float32)
        steps.append((state.copy(), mu, act, rew))
        if t & 1 == 0:
            row_act = act
        else:
            c = _pick(rng, chance[state, :, row_act, act])
            nxt = np.where(live, index[state, c, row_act, act], 0)
            rew[:] = np.where(live & (nxt == 0), value[state, c, row_act, act], 0)
            state = nxt
    assert not state.any(), "episodes longer than 64 steps"
    indices, mu, act, rew = (np.stack(x) for x in zip(*steps))
    batch = dict(indices=indices.astype(np.int32), legal=legal_tab[(np.arange(len(steps)) & 1)[:, None] * S + indices], actions=act.astype(np.int32),
                 rewards=rew, mu=mu, S=S)
    return batch, draw_tables(rng, legal_tab, hp)


def compare(case, ref, got):
    """Assert every output of `got` (name -> array) within K 2^-24 mag of the reference and log the shares of the gate."""
    worst = {}
    for name, arr in got.items():
        s = share(arr, getattr(ref, name)) / K[name]
        worst[name] = s
        log_share(case, name, s)
    bad = {n: round(s, 3) for n, s in worst.items() if not s <= 1.0}
    assert not bad, f"{case}: outside the gate (shares of K 2^-24 mag): {bad}"
    return worst
