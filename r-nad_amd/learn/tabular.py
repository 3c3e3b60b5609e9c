"""Exact tabular R-NaD on the enumerated tree -- an addition without a counterpart in the reference.

For a regularisation policy mu and eta > 0 the fixed point of one R-NaD regularisation update is, at every state, the unique equilibrium of
the state's matrix game (payoffs: the values of its children) with the KL terms of learn/vtrace.py:234-239 added.  `solve_regularized`
computes it for the whole tree in one bottom-up sweep (rnad_reg_solve, csrc/reg_solve.hip); `TabularRNaD` feeds the result back as the next
regularisation policy (learn/rnad.py:530-531) and records NashConv after every update: the curve the algorithm itself would reach with
sampling noise, off-policy correction and function approximation taken out.  The tables have the layout of NashConvData.joint_policy, so
`util.metric.cross_play` plays them against trained nets as they are.

`evaluate_regularized` answers the question in between: how far is an ARBITRARY policy from the fixed point its magnet defines, and what
is it worth there (rnad_reg_evaluate, csrc/reg_evaluate.hip) -- the quantities the learner estimates by sampling.  `TabularNeuRD` is the
exact inner loop built on it: NeuRD steps on a logit table, between `TabularRNaD` (no inner loop) and the sampled trainer.

`TabularCFR` runs the algorithm the field puts beside R-NaD on the same tree: counterfactual regret minimisation, exact because every
state is its own information set for both players (rnad_cfr_iterate, csrc/cfr.hip) -- plain CFR, CFR+, linear averaging and DCFR, up to
32 variants in lockstep, judged by the same NashConv.
"""
from typing import List, NamedTuple

import torch

import rnad_hip
from util import metric


class RegSolution(NamedTuple):
    """solve_regularized's result, tensors on the tree's device.  policy, log_policy [S, 2A] (log_policy is -inf where policy is 0 by
    construction: illegal actions and actions outside the magnet's support; it stays finite where exp underflows); values [S]: the row
    player's regularised value; residual [S]: max_a |pi(a) - softmax(log mu + q / eta)(a)| as the state last evaluated it; iters int32 [S];
    unconverged: the number of states that spent max_iters steps and still have residual > tol."""

    policy: torch.Tensor
    log_policy: torch.Tensor
    values: torch.Tensor
    residual: torch.Tensor
    iters: torch.Tensor
    unconverged: int


def legal_mask(tree) -> torch.Tensor:
    """bool [S, 2A]: the row player's legal actions (legal_tensor[s, 0, :, 0]) | the column player's (legal_tensor[s, 0, 0, :])."""
    legal = tree.legal_tensor[:, 0]
    return torch.cat([legal[:, :, 0], legal[:, 0, :]], dim=1) != 0


def uniform_log_reg(tree) -> torch.Tensor:
    """log of the uniform policy over the legal actions, -inf elsewhere (all of state 0's row)."""
    mask = legal_mask(tree)
    A = tree.max_actions
    count = torch.cat([mask[:, :A].sum(1, keepdim=True).expand(-1, A), mask[:, A:].sum(1, keepdim=True).expand(-1, A)], dim=1)
    minus_inf = torch.full(mask.shape, float("-inf"), device=mask.device)
    return torch.where(mask, -torch.log(count.clamp(min=1).float()), minus_inf).contiguous()


def log_reg_of(tree, reg) -> torch.Tensor:
    """The magnet as the log table rnad_reg_solve reads: None -> uniform over the legal actions; a net -> its policy at every state
    (util.metric.joint_policy_of); a [S, 2A] probability table -> its log, zeros becoming -inf."""
    S, A = tree.value_tensor.shape[0], tree.max_actions
    dev = tree.value_tensor.device
    if reg is None:
        return uniform_log_reg(tree)
    if torch.is_tensor(reg):
        if tuple(reg.shape) != (S, 2 * A):
            raise ValueError(f"reg: a policy table must be [{S}, {2 * A}], got {tuple(reg.shape)}")
        table = reg.detach().to(device=dev, dtype=torch.float)
    else:
        table = metric.joint_policy_of(tree, reg)
    if bool((table < 0).any().item()):
        raise ValueError("reg: a policy table holds probabilities, got negative entries")
    return torch.log(table).contiguous()  # log 0 = -inf: outside the support


def _solve(tree, eta, log_reg, tol, max_iters) -> RegSolution:
    log_policy, policy, values, residual, iters = rnad_hip.reg_solve(tree.handle(), eta, log_reg, tol=tol, max_iters=max_iters)
    unconverged = int(((iters >= max_iters) & ~(residual <= tol)).sum().item())
    return RegSolution(policy, log_policy, values, residual, iters, unconverged)


def solve_regularized(tree, eta, reg=None, tol=1e-5, max_iters=4096) -> RegSolution:
    """The fixed point of one regularisation update with magnet `reg` (None, a net or a [S, 2A] probability table: log_reg_of)."""
    if not float(eta) > 0:
        raise ValueError(f"solve_regularized: eta = {eta}: the unregularised game has no unique fixed point to sweep to")
    return _solve(tree, float(eta), log_reg_of(tree, reg), float(tol), int(max_iters))


class TabularRNaD:
    """R-NaD's outer loop with every inner loop replaced by its exact fixed point.  update(): solve for the current magnet, then mu <- pi
    (the log table is handed on, so a magnet far below e^-500 survives).  nashconv_history[m]: NashConv of the policy after update m + 1
    (NashConvData.get_nashconv); unconverged_history[m]: the states of that solve that did not reach tol.  average=True also keeps
    average_policy, the exact uniform mixture of the policies of all updates so far (util.metric.mixture: update m + 1 folds in as the
    mixture of the average and the new policy with weights m and 1), and its NashConv in average_nashconv_history."""

    def __init__(self, tree, eta, tol=1e-5, max_iters=4096, reg=None, average=False):
        if not float(eta) > 0:
            raise ValueError(f"TabularRNaD: eta = {eta}: the unregularised game has no unique fixed point to sweep to")
        self.tree, self.eta, self.tol, self.max_iters = tree, float(eta), float(tol), int(max_iters)
        self.log_reg = log_reg_of(tree, reg)
        self.solution = None
        self.nashconv_history: List[float] = []
        self.unconverged_history: List[int] = []
        self._data = metric.NashConvData(tree)
        self.average = bool(average)
        self.average_policy = None
        self.average_nashconv_history: List[float] = []

    @property
    def policy(self) -> torch.Tensor:
        """[S, 2A]: the policy of the last update (before the first: the magnet)."""
        return self.solution.policy if self.solution is not None else torch.exp(self.log_reg)

    @property
    def values(self) -> torch.Tensor:
        if self.solution is None:
            raise ValueError("TabularRNaD.values: no update has run yet")
        return self.solution.values

    def update(self) -> float:
        self.solution = _solve(self.tree, self.eta, self.log_reg, self.tol, self.max_iters)
        self.log_reg = self.solution.log_policy
        self._data.joint_policy.copy_(self.solution.policy)
        self._data.get_nashconv(self.tree, self._data.joint_policy)
        self.nashconv_history.append((self._data.row_best[1] + self._data.col_best[1]).item())
        self.unconverged_history.append(self.solution.unconverged)
        if self.average:
            m = len(self.average_nashconv_history)
            self.average_policy = (self.solution.policy.clone() if m == 0 else
                                   metric.mixture(self.tree, [self.average_policy, self.solution.policy], [m, 1]).policy)
            self._data.joint_policy.copy_(self.average_policy)
            self._data.get_nashconv(self.tree, self._data.joint_policy)
            self.average_nashconv_history.append((self._data.row_best[1] + self._data.col_best[1]).item())
        return self.nashconv_history[-1]

    def run(self, updates: int) -> List[float]:
        for _ in range(int(updates)):
            self.update()
        return self.nashconv_history


# ---------------------------------------------------------------------------------------------------- exact evaluation
class RegEvaluation(NamedTuple):
    """evaluate_regularized's result for n (policy, magnet, eta) triples; tensors on the tree's device unless said otherwise.
    policy [S, n, 2A]: the tables as evaluated; values [S, n]: the row player's regularised value (solve_regularized's values for that
    policy); q [S, n, 2A]: each side's unregularised action values against the other side, in its own payoff; residual [S, n]:
    max_a |pi(a) - softmax(log mu + q / eta)(a)| over both sides, reg_solve's stopping quantity; reach [S, n]: the policy's joint reach,
    chance included (best_response's); advantage [S, n, 2A] = q - eta * (log pi - log mu), centred by its pi-weighted mean per side, zero
    outside the support and where pi = 0: the exact NeuRD direction, zero on the support at the fixed point; distance [n]: the fp64 sum
    over the states of reach * residual, on the host; max_residual [n]: the largest residual over the states with reach > 0, on the host."""

    policy: torch.Tensor
    values: torch.Tensor
    q: torch.Tensor
    residual: torch.Tensor
    reach: torch.Tensor
    advantage: torch.Tensor
    distance: torch.Tensor
    max_residual: torch.Tensor


def swept_states(tree) -> torch.Tensor:
    """bool [S]: the states a sweep from the root visits (live links: chance > 0, index != 0).  Kept on the tree object for the tensors it
    was computed from."""
    index, chance = tree.index_tensor, tree.chance_tensor
    key = (index.data_ptr(), chance.data_ptr(), index._version, chance._version)
    cached = tree.__dict__.get("_swept_states")
    if cached is not None and cached[0] == key:
        return cached[1]
    live = (index != 0) & (chance > 0)
    swept = torch.zeros((index.shape[0],), dtype=torch.bool, device=index.device)
    frontier = torch.ones((1,), dtype=torch.long, device=index.device)
    while frontier.numel() > 0:
        swept[frontier] = True
        frontier = index[frontier][live[frontier]].to(torch.long)
    tree.__dict__["_swept_states"] = (key, swept)
    return swept


def _per_member(tree, tables, n, what) -> torch.Tensor:
    """[S, n, 2A] fp32 on the tree's device from one [S, 2A] table for all members or a ready [S, n, 2A] one."""
    S, A = tree.value_tensor.shape[0], tree.max_actions
    t = tables.detach().to(device=tree.value_tensor.device, dtype=torch.float)
    if tuple(t.shape) == (S, 2 * A):
        t = t[:, None, :].expand(S, n, 2 * A)
    if tuple(t.shape) != (S, n, 2 * A):
        raise ValueError(f"{what}: a log table must be [{S}, {2 * A}] or [{S}, {n}, {2 * A}], got {tuple(tables.shape)}")
    return t.contiguous()


def neurd_advantage(tree, policies, log_policy, log_reg, q, eta, on) -> torch.Tensor:
    """[S, n, 2A]: q - eta * (log pi - log mu), minus its pi-weighted mean per side, where `on`; zero elsewhere.  eta: [n] on the device.
    log_policy: log pi as the caller holds it (finite where exp underflows)."""
    A = tree.max_actions
    zero = torch.zeros_like(q)
    raw = torch.where(on, q - eta[None, :, None] * (torch.where(on, log_policy, zero) - torch.where(on, log_reg, zero)), zero)
    mean = torch.cat([(policies[..., :A] * raw[..., :A]).sum(-1, keepdim=True).expand(-1, -1, A),
                      (policies[..., A:] * raw[..., A:]).sum(-1, keepdim=True).expand(-1, -1, A)], dim=-1)
    return torch.where(on, raw - mean, zero)


def _evaluate(tree, policies, log_reg, etas, log_policy=None) -> RegEvaluation:
    """policies, log_reg [S, n, 2A] on the device, etas: n positive floats.  Refuses mass outside the magnet's support at a swept state:
    the KL there is infinite, and one such state poisons every value above it."""
    if not metric.index_is_tree(tree):
        raise ValueError("evaluate_regularized: the index tensor is not a tree: joint reach is undefined (a state with two parents has "
                         "no perfect recall, and its two reach values would race)")
    support = legal_mask(tree)[:, None, :] & (log_reg > float("-inf"))
    outside = (policies > 0) & ~support & swept_states(tree)[:, None, None]
    if bool(outside.any().item()):
        s, k, a = (int(v) for v in outside.nonzero()[0])
        raise ValueError(f"evaluate_regularized: player {k} puts probability {policies[s, k, a].item():.3g} on action {a} of state {s}, "
                         "outside its magnet's support (illegal or mu = 0): the KL term is infinite")
    values, q, residual, reach = rnad_hip.reg_evaluate(tree.handle(), etas, policies, log_reg)
    eta_dev = torch.tensor(etas, dtype=torch.float, device=policies.device)
    if log_policy is None:  # a table: where pi = 0 there is no log to take and no direction to report
        advantage = neurd_advantage(tree, policies, torch.log(torch.where(policies > 0, policies, torch.ones_like(policies))), log_reg, q,
                                    eta_dev, support & (policies > 0))
    else:  # logits: an action whose probability underflowed still has its log and can come back
        advantage = neurd_advantage(tree, policies, log_policy, log_reg, q, eta_dev, support)
    distance = (reach.to(torch.float64) * residual.to(torch.float64)).sum(dim=0).cpu()
    max_residual = torch.where(reach > 0, residual, torch.zeros_like(residual)).max(dim=0).values.to(torch.float64).cpu()
    return RegEvaluation(policies, values, q, residual, reach, advantage, distance, max_residual)


def evaluate_regularized(tree, players, eta, reg=None, log_reg=None) -> RegEvaluation:
    """Exact evaluation of `players` (nets or [S, 2A] tables, as util.metric.cross_play takes them) in the game regularised towards a
    magnet: their values, action values, distance to the magnet's fixed point and reach, in one sweep pair for up to 32 players.
    eta: one positive number or one per player.  reg: None (the uniform magnet), one magnet for all players or a list of one per player,
    each as log_reg_of takes it (a net or a probability table).  log_reg=: instead of reg, ready log tables [S, 2A] or [S, n, 2A] taken as
    they are -- they need not be normalised (the trainer's alpha * log mu + (1 - alpha) * log mu_ is not)."""
    policies = metric._policy_tables(tree, players, "evaluate_regularized")
    n = policies.shape[1]
    etas = [float(e) for e in eta] if hasattr(eta, "__len__") else [float(eta)] * n
    if len(etas) != n:
        raise ValueError(f"evaluate_regularized: {len(etas)} values of eta for {n} players")
    if not all(e > 0 and e != float("inf") for e in etas):
        raise ValueError(f"evaluate_regularized: eta = {etas}: the unregularised game has no unique fixed point to measure against")
    if log_reg is not None:
        if reg is not None:
            raise ValueError("evaluate_regularized: give reg or log_reg, not both")
        logs = _per_member(tree, log_reg, n, "log_reg")
    elif isinstance(reg, (list, tuple)):
        if len(reg) != n:
            raise ValueError(f"evaluate_regularized: {len(reg)} magnets for {n} players")
        logs = torch.stack([log_reg_of(tree, r) for r in reg], dim=1).contiguous()
    else:
        logs = _per_member(tree, log_reg_of(tree, reg), n, "reg")
    return _evaluate(tree, policies, logs, etas)


def softmax_support(logits) -> torch.Tensor:
    """[S, 2A] policy of a logit table whose entries outside the support are -inf: a softmax per side, zero rows where a side has none."""
    A = logits.shape[-1] // 2
    halves = [torch.softmax(h, dim=-1) for h in (logits[..., :A], logits[..., A:])]
    return torch.nan_to_num(torch.cat(halves, dim=-1), nan=0.0)


def _log_softmax_support(logits) -> torch.Tensor:
    A = logits.shape[-1] // 2
    return torch.cat([torch.log_softmax(h, dim=-1) for h in (logits[..., :A], logits[..., A:])], dim=-1)


class TabularNeuRD:
    """R-NaD's inner loop made exact: NeuRD on a logit table l [S, 2A] with the advantage computed by a tree sweep instead of V-trace on
    sampled games.  l starts at the magnet; entries outside the support (illegal, mu = 0) are -inf and never move.  step():
    pi = softmax_support(l), evaluate pi (one rnad_reg_evaluate), l += lr * advantage with log pi taken as log_softmax(l) -- log(pi) of an
    underflowed pi would be -inf.  At the fixed point of the magnet the advantage vanishes on the support.  run(steps) records distance and
    max_residual (RegEvaluation) after every step in distance_history / residual_history (the evaluation of the new policy is kept and
    serves the next step: one sweep pair per step); swap() makes the current policy the magnet, as
    TabularRNaD.update does, so outer iterations compose.  lr * eta must stay below 1: the step multiplies log pi - log mu by 1 - lr * eta.
    Not modelled: the logit-threshold gate and the gradient clip of get_loss_nerd (learn/vtrace.py), which act on a net's logits, and
    everything sampling brings (importance weights, the thresholded acting policy)."""

    def __init__(self, tree, eta, lr, reg=None):
        if not float(eta) > 0:
            raise ValueError(f"TabularNeuRD: eta = {eta}: the unregularised game has no unique fixed point to descend to")
        if not float(lr) > 0 or float(lr) * float(eta) >= 1:
            raise ValueError(f"TabularNeuRD: lr = {lr} with eta = {eta}: lr must be positive and lr * eta below 1")
        self.tree, self.eta, self.lr = tree, float(eta), float(lr)
        mask = legal_mask(tree)
        log_reg = log_reg_of(tree, reg)
        self.log_reg = torch.where(mask, log_reg, torch.full_like(log_reg, float("-inf"))).contiguous()
        self.logits = self.log_reg.clone()
        self.evaluation = None
        self.distance_history: List[float] = []
        self.residual_history: List[float] = []

    @property
    def policy(self) -> torch.Tensor:
        """[S, 2A]: the policy of the current logits."""
        return softmax_support(self.logits)

    def evaluate(self) -> RegEvaluation:
        """The current policy against the current magnet (no step)."""
        return _evaluate(self.tree, self.policy[:, None, :].contiguous(), self.log_reg[:, None, :].contiguous(), [self.eta],
                         log_policy=torch.nan_to_num(_log_softmax_support(self.logits), nan=0.0)[:, None, :])

    def step(self) -> RegEvaluation:
        """One NeuRD step; returns the evaluation of the policy the step started from."""
        ev = self.evaluation if self.evaluation is not None else self.evaluate()
        self.logits += self.lr * ev.advantage[:, 0]  # (-inf + 0 outside the support)
        self.evaluation = None
        return ev

    def run(self, steps: int) -> List[float]:
        for _ in range(int(steps)):
            self.step()
            self.evaluation = self.evaluate()
            self.distance_history.append(float(self.evaluation.distance[0]))
            self.residual_history.append(float(self.evaluation.max_residual[0]))
        return self.residual_history

    def swap(self) -> None:
        """mu <- pi (learn/rnad.py:530-531): the log table is handed on, so a magnet far below e^-500 survives."""
        self.log_reg = torch.where(self.logits > float("-inf"), _log_softmax_support(self.logits), self.logits).contiguous()
        self.logits = self.log_reg.clone()
        self.evaluation = None


# ---------------------------------------------------------------------------------------------------- exact CFR
CFR_VARIANTS = ("cfr", "cfr+", "linear")


def _ratio(x: int, e: float) -> float:
    """x^e / (x^e + 1) for an integer x >= 0, with the limits at x = 0 and e = -inf."""
    if x == 0:
        return 0.0 if e > 0 else (0.5 if e == 0 else 1.0)
    p = float(x) ** e
    return p / (p + 1.0)


def cfr_discounts(variant, t: int):
    """(dp, dn, da) of iteration t >= 1 in fp64 (rnad_cfr_iterate): what the accumulated regrets (positive, negative) and the strategy sum
    are multiplied by before iteration t's terms are added.  "cfr": (1, 1, 1).  "cfr+": (1, 0, (t - 1) / t) -- the negatives are zeroed
    before the add, which leaves the same R+ as clamping after it, and the average weighs iteration t by t as its authors do.
    "linear": (1, 1, (t - 1) / t).  ("dcfr", alpha, beta, gamma): (x^alpha / (x^alpha + 1), x^beta / (x^beta + 1), (x / (x + 1))^gamma) at
    x = t - 1."""
    t = int(t)
    if variant == "cfr":
        return 1.0, 1.0, 1.0
    if variant == "cfr+":
        return 1.0, 0.0, (t - 1) / t
    if variant == "linear":
        return 1.0, 1.0, (t - 1) / t
    _, alpha, beta, gamma = variant
    return _ratio(t - 1, alpha), _ratio(t - 1, beta), ((t - 1) / t) ** gamma


def _cfr_variant(v):
    if isinstance(v, str) and v in CFR_VARIANTS:
        return v
    if isinstance(v, (tuple, list)) and len(v) == 4 and v[0] == "dcfr":
        try:
            alpha, beta, gamma = (float(x) for x in v[1:])
        except (TypeError, ValueError):
            alpha = beta = gamma = float("nan")
        if alpha == alpha and beta == beta and gamma == gamma:
            return ("dcfr", alpha, beta, gamma)
    raise ValueError(f"TabularCFR: unknown variant {v!r}: expected one of {CFR_VARIANTS} or ('dcfr', alpha, beta, gamma)")


def normalised_per_side(tree, table) -> torch.Tensor:
    """[S, n, 2A]: a nonnegative table normalised per side over the legal actions, uniform over them where the side's sum is 0, zero on
    illegal actions."""
    A = tree.max_actions
    mask = legal_mask(tree)[:, None, :]
    x = torch.where(mask, table, torch.zeros_like(table))
    halves = []
    for lo in (0, A):
        h, on = x[..., lo:lo + A], mask[..., lo:lo + A]
        tot = h.sum(-1, keepdim=True)
        cnt = on.sum(-1, keepdim=True).clamp(min=1).to(h.dtype)
        halves.append(torch.where(on, torch.where(tot > 0, h / torch.where(tot > 0, tot, torch.ones_like(tot)), 1.0 / cnt), torch.zeros_like(h)))
    return torch.cat(halves, dim=-1)


class TabularCFR:
    """Counterfactual regret minimisation on the enumerated tree, exactly: every state is its own information set for both players, so
    one iteration is one top-down and one bottom-up sweep (rnad_cfr_iterate, csrc/cfr.hip), and up to 32 variants run in lockstep on one
    read of the transition tables.  variants: one name or a list; each "cfr", "cfr+", "linear" or ("dcfr", alpha, beta, gamma)
    (cfr_discounts).  alternating: one bool or one per member, default True for "cfr+" and False otherwise; an alternating member updates
    the row side on odd iterations and the column side on even ones.  The discounts are computed in fp64 on the host per iteration,
    rounded to fp32 and written to the device tensors the kernels read.  step() runs one iteration; run(iterations, every) records
    nashconv_history[k] (the current policy sigma_t) and average_nashconv_history[k] at the iterations in `recorded`.  regret,
    strategy_sum [S, n, 2A]; policy (sigma of the last iteration), values [S, n], reach [S, 3, n] after the first step; average_policy
    [S, n, 2A]: strategy_sum normalised per side, uniform over the legal actions where the sum is 0 -- average_policy[:, k] is an ordinary
    policy table for util.metric.cross_play, best_response, mixture, evaluate_regularized and TabularRNaD(reg=...)."""

    def __init__(self, tree, variants="cfr+", alternating=None):
        if not metric.index_is_tree(tree):
            raise ValueError("TabularCFR: the index tensor is not a tree: own-action reach is undefined (a state with two parents has no "
                             "perfect recall, and its reach values would race)")
        many = isinstance(variants, list) or (isinstance(variants, tuple) and not (len(variants) == 4 and variants[0] == "dcfr"))
        self.variants = [_cfr_variant(v) for v in (variants if many else [variants])]
        n = len(self.variants)
        if not 1 <= n <= rnad_hip.CROSS_PLAY_MAX:
            raise ValueError(f"TabularCFR: {n} variants outside [1, {rnad_hip.CROSS_PLAY_MAX}]")
        if alternating is None:
            self.alternating = [v == "cfr+" for v in self.variants]
        elif isinstance(alternating, (list, tuple)):
            if len(alternating) != n:
                raise ValueError(f"TabularCFR: {len(alternating)} values of alternating for {n} variants")
            self.alternating = [bool(a) for a in alternating]
        else:
            self.alternating = [bool(alternating)] * n
        self.tree, self.n, self.t = tree, n, 0
        S, A, dev = tree.value_tensor.shape[0], tree.max_actions, tree.value_tensor.device
        self.regret = torch.zeros((S, n, 2 * A), dtype=torch.float, device=dev)
        self.strategy_sum = torch.zeros((S, n, 2 * A), dtype=torch.float, device=dev)
        # the per-iteration parameters share one device buffer of 4n words, so that an iteration costs one host-to-device copy
        self._step_words = torch.empty((4 * n,), dtype=torch.int32, device=dev)
        self.discount = self._step_words[:3 * n].view(torch.float).view(n, 3)
        self.sides = self._step_words[3 * n:]
        self.discount.fill_(1.0)
        self.sides.fill_(3)
        self._policy = torch.empty((S, n, 2 * A), dtype=torch.float, device=dev)
        self._values = torch.empty((S, n), dtype=torch.float, device=dev)
        self._reach = torch.empty((S, 3, n), dtype=torch.float, device=dev)
        self._data = metric.NashConvData(tree)
        self.recorded: List[int] = []
        self.nashconv_history: List[List[float]] = [[] for _ in range(n)]
        self.average_nashconv_history: List[List[float]] = [[] for _ in range(n)]

    def _ran(self, what):
        if self.t == 0:
            raise ValueError(f"TabularCFR.{what}: no iteration has run yet")

    @property
    def policy(self) -> torch.Tensor:
        """[S, n, 2A]: sigma of the last iteration."""
        self._ran("policy")
        return self._policy

    @property
    def values(self) -> torch.Tensor:
        self._ran("values")
        return self._values

    @property
    def reach(self) -> torch.Tensor:
        self._ran("reach")
        return self._reach

    @property
    def average_policy(self) -> torch.Tensor:
        return normalised_per_side(self.tree, self.strategy_sum)

    def set_iteration(self, t: int) -> None:
        """Write iteration t's discounts and side bits to the device tensors."""
        disc = torch.tensor([cfr_discounts(v, t) for v in self.variants], dtype=torch.float64).to(torch.float)
        turn = torch.tensor([(1 if t % 2 == 1 else 2) if a else 3 for a in self.alternating], dtype=torch.int32)
        self._step_words.copy_(torch.cat([disc.reshape(-1).view(torch.int32), turn]))

    def step(self) -> None:
        self.set_iteration(self.t + 1)
        rnad_hip.cfr_iterate(self.tree.handle(), self.regret, self.strategy_sum, self.discount, self.sides, self._policy, self._values,
                             self._reach)
        self.t += 1

    def _nashconv(self, table) -> float:
        self._data.joint_policy.copy_(table)
        self._data.get_nashconv(self.tree, self._data.joint_policy)
        return (self._data.row_best[1] + self._data.col_best[1]).item()

    def record(self) -> None:
        """NashConv of every member's current and average policy at this iteration."""
        self._ran("record")
        average = self.average_policy
        self.recorded.append(self.t)
        for k in range(self.n):
            self.nashconv_history[k].append(self._nashconv(self._policy[:, k]))
            self.average_nashconv_history[k].append(self._nashconv(average[:, k]))

    def run(self, iterations: int, every: int = 1) -> List[List[float]]:
        """`iterations` more iterations, recording after every `every`-th of them and after the last; returns average_nashconv_history."""
        every = max(1, int(every))
        for i in range(1, int(iterations) + 1):
            self.step()
            if i % every == 0 or i == int(iterations):
                self.record()
        return self.average_nashconv_history
