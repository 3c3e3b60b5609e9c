"""V-trace / NeuRD functions -- drop-in for reference learn/vtrace.py, each backed by one HIP kernel.

Same free functions, argument order and return values as the reference (which is itself an adaptation of
OpenSpiel's R-NaD): `process_policy`, `_player_others`, `v_trace`, `get_loss_v`, `get_loss_nerd`.  Inputs may be any
GPU tensors of the reference's shapes; they are made contiguous fp32/int32 for the kernels.  `RNaD.__learn` does not
go through these one by one -- it calls the fused kernel (rnad_hip.learn_fused) -- but they compute the same
expressions in the same order and are what tests compare against the reference's fixtures.
"""
from typing import Any, NamedTuple, Sequence, Tuple

import torch

import rnad_hip


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def process_policy(policy: torch.Tensor, mask: torch.Tensor, n_disc, epsilon_threshold=0.03):
    """Threshold (eps) + discretise (n_disc) the learner policy.  reference learn/vtrace.py:24-55."""
    t_eff, batch_size, n_actions = policy.shape
    out = rnad_hip.process_policy(_f32(policy).view(-1, n_actions), _f32(mask).view(-1, n_actions), n_disc, epsilon_threshold)
    return out.view(t_eff, batch_size, n_actions)


def _player_others(player_ids: torch.Tensor, valid: torch.Tensor, player: int) -> torch.Tensor:
    """1 for the current player, -1 for others, 0 on invalid steps, shape [..., 1].  reference learn/vtrace.py:70-87."""
    res = 2 * (player_ids == player) - 1
    res = res * valid
    return torch.unsqueeze(res, dim=-1)


def v_trace(
    v: torch.Tensor,
    valid: torch.Tensor,
    player_id: torch.Tensor,
    acting_policy: torch.Tensor,
    merged_policy: torch.Tensor,
    merged_log_policy: torch.Tensor,
    player_others: torch.Tensor,
    actions_oh: torch.Tensor,
    reward: torch.Tensor,
    player: int,
    # Scalars below.
    eta: float,
    lambda_: float,
    c: float,
    rho: float,
    gamma=1.0,
) -> Tuple[Any, Any, Any]:
    """Two-player V-trace for `player`.  reference learn/vtrace.py:207-352.

    Returns (v_target [T,B,1], has_played [T,B] int64, learning_output [T,B,A]).  `player_others` must be
    `_player_others(player_id, valid, player)` as at the reference's only call site (learn/rnad.py:393); the kernel
    recomputes it.  `actions_oh` may also be an int32 `[T,B]` tensor of action ids.
    """
    T, B, A = acting_policy.shape
    acts = actions_oh.contiguous() if actions_oh.dtype == torch.int32 else _f32(actions_oh)
    vt, has_played, q = rnad_hip.vtrace(
        _f32(v).view(T, B), _f32(valid), player_id.to(torch.int32).contiguous(), _f32(acting_policy), _f32(merged_policy),
        _f32(merged_log_policy), acts, _f32(reward), player, eta, lambda_, c, rho, gamma)
    return vt.view(T, B, 1), has_played.to(torch.int64), q


class _LossV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, v_targets, masks):
        vv = _f32(v)
        dv = torch.empty_like(vv)
        loss = torch.zeros((1,), dtype=torch.float64, device=v.device)
        for k, (vt, m) in enumerate(zip(v_targets, masks)):
            mf = _f32(m).view(-1)
            rnad_hip.loss_v(vv.view(-1), _f32(vt).view(-1), mf, rnad_hip.mask_sum(mf), 1.0, loss, dv.view(-1), k > 0)
        ctx.save_for_backward(dv)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad):
        (dv,) = ctx.saved_tensors
        return grad * dv, None, None


def get_loss_v(v_list: Sequence[torch.Tensor], v_target_list: Sequence[torch.Tensor], mask_list: Sequence[torch.Tensor]) -> torch.Tensor:
    """Critic loss sum_k sum(mask_k (v_k - target_k)^2) / max(sum(mask_k), 1).  reference learn/vtrace.py:377-393.
    Differentiable w.r.t. every entry of `v_list` (closed-form gradient).  At the reference's call site (learn/rnad.py:407) every entry
    is the same tensor: one pass of the kernel per player over it, one gradient buffer; distinct tensors (r06: the full signature) take
    one call per entry and the losses are added as the reference adds them (:393)."""
    if all(v is v_list[0] for v in v_list):
        return _LossV.apply(v_list[0], list(v_target_list), list(mask_list))
    return sum(_LossV.apply(v, [vt], [m]) for v, vt, m in zip(v_list, v_target_list, mask_list))


class _LossNerd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, pis, qs, masks, legal, clip, threshold):
        lg = _f32(logit)
        A = lg.shape[-1]
        dl = torch.empty_like(lg)
        loss = torch.zeros((1,), dtype=torch.float64, device=logit.device)
        legal_f = _f32(legal).view(-1, A)
        for k, (pi, q, m) in enumerate(zip(pis, qs, masks)):
            mf = _f32(m).view(-1)
            rnad_hip.loss_nerd(lg.view(-1, A), _f32(pi).view(-1, A), _f32(q).view(-1, A), mf, legal_f, rnad_hip.mask_sum(mf),
                               clip, threshold, 1.0, loss, dl.view(-1, A), k > 0)
        ctx.save_for_backward(dl)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad):
        (dl,) = ctx.saved_tensors
        return grad * dl, None, None, None, None, None, None


def get_loss_nerd(
    logit_list: Sequence[torch.Tensor],
    policy_list: Sequence[torch.Tensor],
    q_vr_list: Sequence[torch.Tensor],
    valid: torch.Tensor,
    player_ids: Sequence[torch.Tensor],
    legal_actions: torch.Tensor,
    importance_sampling_correction: Sequence[torch.Tensor],
    clip: float = 100,
    threshold: float = 2,
) -> torch.Tensor:
    """NeuRD loss.  reference learn/vtrace.py:396-431.  Differentiable w.r.t. `logit` (the force is detached there too).
    The importance weights multiply the advantage before clipping (:416); a weight per ROW (a scalar, or a last dimension of 1, as the
    reference passes: learn/rnad.py:409-410) commutes with the advantage -- adv is linear in q -- and is folded into q (`is_c * q`); a
    weight per ACTION does not commute and is refused.  At the reference's call site every entry of logit_list is the same tensor: one
    kernel pass per player over it; distinct tensors (r06: the full signature) take one call per entry, the losses added as at :431."""
    assert isinstance(importance_sampling_correction, list)
    for is_c in importance_sampling_correction:
        assert not torch.is_tensor(is_c) or is_c.dim() == 0 or is_c.shape[-1] == 1, \
            "get_loss_nerd: importance weights per action are not supported (one weight per row, shape [..., 1], or a scalar)"
    qs = [q * is_c for q, is_c in zip(q_vr_list, importance_sampling_correction)]
    masks = [valid * (player_ids == k) for k in range(len(logit_list))]
    if all(l is logit_list[0] for l in logit_list):
        return _LossNerd.apply(logit_list[0], list(policy_list), qs, masks, legal_actions, float(clip), float(threshold))
    return sum(_LossNerd.apply(lg, [pi], [q], [m], legal_actions, float(clip), float(threshold))
               for lg, pi, q, m in zip(logit_list, policy_list, qs, masks))


# ---------------------------------------------------------------------------------------------------- the exact expected update
class ExpectedUpdate(NamedTuple):
    """expected_update's result: what the learner's estimates are in expectation over complete episodes played by the behaviour; tensors
    on the tree's device unless said otherwise, rows in the learner's layout (row = player * S + state).
    pi_processed [2S, A]: the policy the targets evaluate; target [2S]: E[v_target at the slot | the row is visited]; target_given_row
    [S, A]: the column player's target given the row action taken at the state; q [2S, A]: E[q at the slot | visited] (an action the
    behaviour never draws keeps vv - eta lpol, as the sampled program leaves it); reach [S]: the probability that an episode visits the
    state; length: sum_s reach, the expected number of slots per player and episode, E[N_P] / B; dv_tab [2S, 1], dlogit_tab [2S, A]: the
    expectation of rnad_learn_fused_tabular's outputs with the batch normaliser replaced by its expectation, 2 w_v reach (v - target) / L
    and reach * direction / L; linear bool [2S]: where dlogit_tab IS that expectation (both threshold gates open on every legal action,
    a clip no sample can reach) -- elsewhere it is the gated, clipped direction at the expected q; target_bias [2]: the fp64 host sum of
    reach * |target - v_target| per player."""

    pi_processed: torch.Tensor
    target: torch.Tensor
    target_given_row: torch.Tensor
    q: torch.Tensor
    reach: torch.Tensor
    length: float
    dv_tab: torch.Tensor
    dlogit_tab: torch.Tensor
    linear: torch.Tensor
    target_bias: torch.Tensor


def _net_rows(tree, net):
    """(logit [2S, A], v [2S]) of a net on the tree's 2S observations (the row player's S rows, then the column player's)."""
    obs_row, obs_col = rnad_hip.observe_all(tree.handle(), tree.value_tensor.device)
    was_training = net.training
    net.eval()
    with torch.no_grad():
        halves = [net.forward_logits(obs) for obs in (obs_row, obs_col)]
    net.train(was_training)
    return (torch.cat([h[0] for h in halves], dim=0).float().contiguous(), torch.cat([h[1].reshape(-1) for h in halves], dim=0).float().contiguous())


def _rows(tree, x, what, value=False):
    """A row table [2S, A] (value: [2S]) on the tree's device from a tensor or a net."""
    S, A = tree.value_tensor.shape[0], tree.max_actions
    if not torch.is_tensor(x):
        return _net_rows(tree, x)[1 if value else 0]
    t = x.detach().to(device=tree.value_tensor.device, dtype=torch.float)
    if value:
        t = t.reshape(-1)
    if tuple(t.shape) != ((2 * S,) if value else (2 * S, A)):
        raise ValueError(f"expected_update: {what} must be a net or a row table {[2 * S] if value else [2 * S, A]}, got {tuple(x.shape)}")
    return t.contiguous()


def _sides(x, S):
    """A row table [2S, k] as one member of the sweeps' layout, [S, 1, 2k]."""
    x = x.reshape(2 * S, -1)
    return torch.cat([x[:S], x[S:]], dim=1)[:, None, :].contiguous()


def _sample_bound(tree, mu, pip, lpol, vv, hp, seen) -> float:
    """An upper bound on |q| of any sampled slot, from maxima over the visited rows: with D the longest episode in states, cs <= K,
    |e| <= E, |vv| <= V, |r| <= R a sampled target obeys |vt| <= V + rho (eta E (1 + g) + g R + g g V + V) + lambda c g g (|vt below| + V),
    D times from 0; a tail is at most g (eta E + K R) + g g K |vt| + V, and |q| <= V + eta max|lpol| + tail / min mu."""
    rows = torch.cat([seen, seen])
    mu, pip, lpol, vv = (t.double()[rows] for t in (mu, pip, lpol, vv))
    drawn = mu > 0
    if not bool(drawn.any()):
        return 0.0
    K = float((pip[drawn] / mu[drawn]).max())
    E = float((pip * torch.where(pip > 0, lpol, torch.zeros_like(lpol))).sum(-1).abs().max())
    V, R = float(vv.abs().max()), float(tree.value_tensor.abs().max())
    index, chance = tree.index_tensor, tree.chance_tensor
    live = (index != 0) & (chance > 0)
    frontier, D = torch.ones((1,), dtype=torch.long, device=index.device), 0
    while frontier.numel() > 0:
        D += 1
        frontier = index[frontier][live[frontier]].to(torch.long)
    g, vt = hp.gamma, 0.0
    for _ in range(D):
        vt = V + hp.rho * (hp.eta * E * (1 + g) + g * R + g * g * V + V) + abs(hp.lambda_) * hp.c * g * g * (vt + V)
    tail = g * (hp.eta * E + K * R) + g * g * K * vt + V
    return V + hp.eta * float(torch.where(drawn, lpol, torch.zeros_like(lpol)).abs().max()) + tail / float(mu[drawn].min())


def expected_update(tree, behaviour, logit, v, v_target, logit_reg, logit_reg_, hp) -> ExpectedUpdate:
    """The learner's update with the sampling taken out (rnad_vtrace_expect, csrc/vtrace_expect.hip): the expectation, over complete
    episodes played by `behaviour` and the tree's chance, of the two-player V-trace targets and action values that RNaD's learner
    computes from sampled trajectories, and of the row gradients it hands to the nets.  Every input is a net or a row table in the
    learner's layout: behaviour a net (its raw policy) or a probability table [2S, A]; logit [2S, A] and v [2S] (a net given as `logit`
    serves both when v is None); v_target [2S] (the target net's value head); logit_reg, logit_reg_ [2S, A].  hp: an
    rnad_hip.LearnParams (make_learn_params).  pi, pi_processed and the log policies come from the learner's own policy-head and
    process_policy kernels.  Refuses a behaviour that never draws an action the evaluated policy plays at a state it reaches: the
    importance ratio there is infinite."""
    return _expected(tree, behaviour, logit, v, v_target, logit_reg, logit_reg_, hp)[0]


def _expected(tree, behaviour, logit, v, v_target, logit_reg, logit_reg_, hp):
    """expected_update's result and what update_noise needs of the sweep behind it: (hyper, the four inputs in the sweep's layout, the
    export workspace, the sweep's raw outputs, v as a row table)."""
    from learn import tabular
    from util import metric

    if not metric.index_is_tree(tree):
        raise ValueError("expected_update: the index tensor is not a tree: a state with two parents has no single expectation")
    S, A = tree.value_tensor.shape[0], tree.max_actions
    if v is None and not torch.is_tensor(logit):
        logit_tab, v_tab = _net_rows(tree, logit)
    else:
        logit_tab, v_tab = _rows(tree, logit, "logit"), _rows(tree, v, "v", value=True)
    vv = _rows(tree, v_target, "v_target", value=True)
    on = tabular.legal_mask(tree)
    legal = torch.cat([on[:, :A], on[:, A:]], dim=0).float().contiguous()
    zero = torch.zeros_like(logit_tab)
    pi, log_pi = rnad_hip.policy_head(logit_tab, mask=legal, want_log=True)
    pip = rnad_hip.process_policy(pi, legal, hp.n_disc, hp.eps_threshold)
    magnet = zero
    for weight, reg in ((hp.alpha, logit_reg), (hp.one_minus_alpha, logit_reg_)):
        if weight != 0:  # a term whose weight is exactly zero is skipped, as train_step skips it
            log_reg = rnad_hip.policy_head(_rows(tree, reg, "logit_reg"), mask=legal, want_log=True)[1]
            magnet = magnet + weight * torch.where(legal > 0, log_reg, zero)
    lpol = torch.where(legal > 0, torch.where(legal > 0, log_pi, zero) - magnet, zero)
    if torch.is_tensor(behaviour):
        mu = _rows(tree, behaviour, "behaviour")
    else:
        mu = rnad_hip.policy_head(_net_rows(tree, behaviour)[0], mask=legal)
    if not bool(torch.isfinite(mu).all()) or bool((mu < 0).any()):
        raise ValueError("expected_update: the behaviour table must be finite and nonnegative")
    hyper = [(hp.eta, hp.gamma, hp.lambda_, hp.rho, hp.c)]
    sides = tuple(_sides(t, S) for t in (mu, pip, lpol, vv))
    workspace = torch.empty((rnad_hip.lib().rnad_vtrace_expect_workspace(S, A, 1),), dtype=torch.float, device=mu.device)
    first = rnad_hip.vtrace_expect(tree.handle(), hyper, *sides, workspace=workspace)
    target, given_row, q, reach = first
    reach = reach[:, 0]
    reach2 = torch.cat([reach, reach])
    never = (pip > 0) & (mu == 0) & (reach2 > 0)[:, None]
    if bool(never.any().item()):
        row, a = (int(x) for x in never.nonzero()[0])
        raise ValueError(f"expected_update: the behaviour never draws action {a} of player {row // S} at state {row % S}, which the "
                         f"evaluated policy plays with probability {pip[row, a].item():.3g}: the importance ratio is infinite")
    target = torch.cat([target[:, 0, 0], target[:, 0, 1]])
    q = torch.cat([q[:, 0, :A], q[:, 0, A:]], dim=0)
    L = float(reach.double().sum())
    dv_tab = (2 * hp.w_v * reach2.double() * (v_tab.double() - target.double()) / L).float()[:, None]
    # the row gradient of one slot at the expected q (vtrace.py:396-431 in closed form): gates and clip applied to it
    adv = (q - (pip * q).sum(-1, keepdim=True)).clamp(-hp.clip, hp.clip)
    l = logit_tab - (logit_tab * legal).sum(-1, keepdim=True) / A
    lo, hi = l > -hp.threshold, l < hp.threshold
    force = legal * (torch.where(lo, adv.clamp(max=0), zero) + torch.where(hi, adv.clamp(min=0), zero))
    grad = force - legal * force.sum(-1, keepdim=True) / A
    dlogit_tab = (reach2.double()[:, None] * (-hp.w_n * grad.double()) / L).float()
    gates_open = ((lo & hi) | (legal == 0)).all(dim=-1)
    bound = _sample_bound(tree, mu, pip, lpol, vv, hp, reach > 0)
    linear = gates_open & (reach2 > 0) & bool(2 * bound <= hp.clip)
    bias = reach2.double() * (target.double() - vv.double()).abs()
    target_bias = torch.stack([bias[:S].sum(), bias[S:].sum()]).cpu()
    return ExpectedUpdate(pip, target, given_row[:, 0], q, reach, L, dv_tab, dlogit_tab, linear, target_bias), (hyper, sides, workspace, first, v_tab)


# ---------------------------------------------------------------------------------------------------- the exact variance of the update
class UpdateNoise(NamedTuple):
    """update_noise's result: the variance, over complete episodes played by the behaviour, of what ExpectedUpdate gives in expectation;
    rows in the learner's layout (row = player * S + state), tensors on the tree's device unless said otherwise.
    expected: the ExpectedUpdate of the same call; target_var [2S]: Var[v_target at the slot | the row is visited]; target_given_row_var
    [S, A]: the column player's given the row action taken (0 where the behaviour never draws it); q_var [2S, A]: the variance of every
    entry of the sampled q, drawn or not (0 where mu = 0) -- the input to the variance of dlogit, which is not derived where the threshold
    gates or the NeuRD clip are non-linear.  For ONE episode (a batch of B divides by B), fp64 on the host: dv_var_tab [2S]: the variance
    of the row's entry of dv_tab, (2 w_v / L)^2 (reach (var + d^2) - reach^2 d^2) with d = v - target and the normaliser at its
    expectation L; target_noise [2]: sum_s reach target_var per player, to be read next to target_bias; episodes_for_unit_snr [2]:
    sum_rows dv_var_tab / sum_rows dv_tab^2, the batch at which the value head's gradient has signal equal to noise (inf where the
    signal is 0)."""

    expected: ExpectedUpdate
    target_var: torch.Tensor
    target_given_row_var: torch.Tensor
    q_var: torch.Tensor
    dv_var_tab: torch.Tensor
    target_noise: torch.Tensor
    episodes_for_unit_snr: torch.Tensor


def update_noise(tree, behaviour, logit, v, v_target, logit_reg, logit_reg_, hp) -> UpdateNoise:
    """The noise of the learner's update next to its expectation (rnad_vtrace_moments, csrc/vtrace_moments.hip): the exact second central
    moments of the sampled V-trace targets and action values, by a second bottom-up sweep over the first moments expected_update's sweep
    left.  Arguments and refusals are expected_update's."""
    expected, (hyper, sides, workspace, first, v_tab) = _expected(tree, behaviour, logit, v, v_target, logit_reg, logit_reg_, hp)
    S, A = tree.value_tensor.shape[0], tree.max_actions
    target_var, given_row_var, q_var = rnad_hip.vtrace_moments(tree.handle(), hyper, *sides, workspace, *first[:3])
    target_var = torch.cat([target_var[:, 0, 0], target_var[:, 0, 1]])
    q_var = torch.cat([q_var[:, 0, :A], q_var[:, 0, A:]], dim=0)
    reach2 = torch.cat([expected.reach, expected.reach]).double()
    L = expected.length
    d = v_tab.double() - expected.target.double()
    var = target_var.double()
    dv_var_tab = (2 * hp.w_v / L) ** 2 * (reach2 * (var + d * d) - reach2 * reach2 * d * d)
    noise = reach2 * var
    target_noise = torch.stack([noise[:S].sum(), noise[S:].sum()]).cpu()
    signal = (2 * hp.w_v * reach2 * d / L) ** 2
    inf = torch.full((), float("inf"), dtype=torch.double, device=signal.device)
    snr = [torch.where(signal[r].sum() > 0, dv_var_tab[r].sum() / signal[r].sum(), inf) for r in (slice(0, S), slice(S, 2 * S))]
    return UpdateNoise(expected, target_var, given_row_var[:, 0], q_var, dv_var_tab, target_noise, torch.stack(snr).cpu())
