"""NashConv evaluation -- drop-in for reference util/metric.py, level-batched on the GPU.

`NashConvData(tree)` keeps the reference's attributes (`joint_policy, row_best, col_best, reach_probability, depth`)
and methods (`get_nashconv_from_net`, `get_nashconv`, `mean_nashconv_by_depth`).  The reference moves the tree to the
CPU and recurses in Python with ~20 tiny tensor ops per state (metric.py:84-175); here the whole tree is inferenced
with two `forward_policy` calls per slice and the best-response values come from rnad_nashconv's two level sweeps.

`cross_play(tree, players)` is an addition without a counterpart in the reference: the exact payoff matrix of n nets or policy
tables against each other (rnad_cross_play, one bottom-up sweep for all n * n pairs), with each player's NashConv next to it.

`mixture(tree, players, weights)`, `meta_nash(payoff)` and `population(tree, players)` judge mixtures of whole policies, again
without a counterpart: the behaviour policy that plays like the mixture (rnad_mixture, one top-down sweep of every member's
own-action reach), the equilibrium weights of a payoff matrix, and the two together for a population.

`best_response(tree, players)` gives what get_nashconv drops: the best response to each player as a policy table of its own, and the
states at which the player loses its exploitability (rnad_best_response, one bottom-up and one top-down sweep for all players).
"""
from typing import Dict, NamedTuple

import numpy as np
import torch

import rnad_hip


class NashConvData:
    def __init__(self, tree):
        self.size = tree.value_tensor.shape[0]
        dev = tree.device
        self.joint_policy = torch.zeros((self.size, 2 * tree.max_actions), device=dev, dtype=torch.float)
        self.row_best = torch.zeros((self.size,), device=dev, dtype=torch.float)
        self.col_best = torch.zeros((self.size,), device=dev, dtype=torch.float)
        self.reach_probability = torch.zeros((self.size,), device=dev, dtype=torch.float)
        self.depth = torch.zeros((self.size,), device=dev, dtype=torch.int)

    def to(self, device):
        for key, value in self.__dict__.items():
            if torch.is_tensor(value):
                self.__dict__[key] = value.to(device)

    # ---------------------------------------------------------------- metric.py:51-90
    def get_nashconv_from_net(self, tree, net, inference_batch_size: int = 10**5) -> None:
        """Inference every state for both players, then evaluate.  Observations of all states come from K1 with
        idx = 0..S-1 (rnad_observe_all) instead of cat / negate / swapaxes per slice (metric.py:66-81)."""
        joint_policy_of(tree, net, out=self.joint_policy, inference_batch_size=inference_batch_size)
        self.get_nashconv(tree, self.joint_policy)
        net.train()

    # ---------------------------------------------------------------- metric.py:93-175
    def get_nashconv(self, tree, joint_policy: torch.Tensor, state_index: int = 1, reach_probablity: float = 1, depth: int = 0) -> None:
        """Best-response values of both players against `joint_policy` for the sub-tree below `state_index`.

        Like the reference, the state the call starts from uses `joint_policy[state_index]` while every descendant uses
        `self.joint_policy` (the recursion at metric.py:148-151 passes `self.joint_policy`); `get_nashconv_from_net`
        makes the two coincide.  `depth` is accepted for signature compatibility (the reference never reads it)."""
        dev = self.joint_policy.device
        root_policy = joint_policy[state_index].detach().to(device=dev, dtype=torch.float).contiguous()
        rnad_hip.nashconv(tree.handle(), self.joint_policy.contiguous(), root_policy, int(state_index), float(reach_probablity),
                          self.row_best, self.col_best, self.reach_probability, self.depth)

    # ---------------------------------------------------------------- metric.py:178-190
    def mean_nashconv_by_depth(self) -> Dict[int, float]:
        max_depth = int(self.depth[1].item())
        nashconv = self.row_best + self.col_best
        means: Dict[int, float] = {}
        for depth in range(1, max_depth + 1):
            idx = self.depth == depth
            means[depth] = torch.mean(nashconv[idx]).item()
        return means


def joint_policy_of(tree, net, out: torch.Tensor = None, inference_batch_size: int = 10**5) -> torch.Tensor:
    """The net's policy at every state for both players, [S, 2A]: row player's in [:A], column player's in [A:] (the inference half of
    get_nashconv_from_net, metric.py:60-82).  out: an existing [S, 2A] fp32 table (or a view of one) on the tree's device to fill.
    The net is evaluated in eval mode and left in the mode it came in."""
    S, A = tree.value_tensor.shape[0], tree.max_actions
    if out is None:
        out = torch.zeros((S, 2 * A), device=tree.device, dtype=torch.float)
    assert tuple(out.shape) == (S, 2 * A) and out.dtype == torch.float
    obs_row, obs_col = rnad_hip.observe_all(tree.handle(), out.device)
    was_training = net.training
    net.eval()
    with torch.no_grad():
        for lo in range(0, S, inference_batch_size):
            hi = min(lo + inference_batch_size, S)
            out[lo:hi, :A] = net.forward_policy(obs_row[lo:hi])  # row player
            out[lo:hi, A:] = net.forward_policy(obs_col[lo:hi])  # column player
    net.train(was_training)
    return out


class CrossPlay(NamedTuple):
    """cross_play's result, tensors on the tree's device.  payoff[i, j]: expected payoff of the row player at the root when player i
    plays the rows and player j the columns (the column player's is its negative); values [S, n, n]: the same at every state;
    nashconv [n]: row_best[1] + col_best[1] of get_nashconv per player; exploitability [n, 2]: what a best response gains over the
    player's self-play value against its column side (row_best[1] - payoff[k, k]) and against its row side (col_best[1] + payoff[k, k]).
    The two are >= 0 up to rounding and sum to nashconv[k]."""

    payoff: torch.Tensor
    values: torch.Tensor
    nashconv: torch.Tensor
    exploitability: torch.Tensor


def cross_play(tree, players) -> CrossPlay:
    """Exact cross-play of `players` on the enumerated tree: each is a net (forward_policy) or a ready [S, 2A] policy table in the
    layout of NashConvData.joint_policy.  No games are sampled: rnad_cross_play sweeps the tree once for all pairs."""
    policies = _policy_tables(tree, players, "cross_play")
    n = policies.shape[1]
    values = rnad_hip.cross_play(tree.handle(), policies)
    payoff = values[1].clone()
    data = NashConvData(tree)
    best = []
    for k in range(n):
        data.joint_policy.copy_(policies[:, k])
        data.get_nashconv(tree, data.joint_policy)
        best.append(torch.stack([data.row_best[1], data.col_best[1]]))
    best = torch.stack(best)  # [n, 2]
    diag = torch.diagonal(payoff)
    exploitability = torch.stack([best[:, 0] - diag, best[:, 1] + diag], dim=1)
    return CrossPlay(payoff=payoff, values=values, nashconv=best[:, 0] + best[:, 1], exploitability=exploitability)


class Mixture(NamedTuple):
    """mixture's result, tensors on the tree's device.  policy [S, 2A]: the behaviour policy that plays like the mixture, an ordinary
    joint_policy table; reach [S, 2, n]: every member's own-action reach (reach[s, 0, k]: the product of member k's row-player
    probabilities on the path to s; [s, 1, k]: of its column player's); weights [2, n]: the normalised row and column weights, fp32."""

    policy: torch.Tensor
    reach: torch.Tensor
    weights: torch.Tensor


class MetaNash(NamedTuple):
    """meta_nash's result, on the host in fp64.  row [m], col [k]: the equilibrium of the matrix game (the row side maximises);
    value = row^T P col; gap = max_i (P col)_i - min_j (row^T P)_j >= 0: what best responses still gain, the solver's own certificate."""

    row: torch.Tensor
    col: torch.Tensor
    value: float
    gap: float


class Population(NamedTuple):
    """population's result.  cross: cross_play of the players; meta: meta_nash(cross.payoff); nash_policy, uniform_policy [S, 2A]: the
    mixture with the row side weighted by meta.row and the column side by meta.col, and the uniform mixture; *_nashconv: their NashConv."""

    cross: CrossPlay
    meta: MetaNash
    nash_policy: torch.Tensor
    nash_nashconv: float
    uniform_policy: torch.Tensor
    uniform_nashconv: float


def _policy_tables(tree, players, what) -> torch.Tensor:
    """[S, n, 2A] fp32 on the tree's device: nets through joint_policy_of, [S, 2A] tables as they are."""
    players = list(players)
    n = len(players)
    if not 1 <= n <= rnad_hip.CROSS_PLAY_MAX:
        raise ValueError(f"{what} takes 1 to {rnad_hip.CROSS_PLAY_MAX} players, got {n}")
    S, A = tree.value_tensor.shape[0], tree.max_actions
    dev = tree.value_tensor.device
    policies = torch.zeros((S, n, 2 * A), device=dev, dtype=torch.float)
    for k, player in enumerate(players):
        if torch.is_tensor(player):
            if tuple(player.shape) != (S, 2 * A):
                raise ValueError(f"player {k}: a policy table must be [{S}, {2 * A}], got {tuple(player.shape)}")
            policies[:, k] = player.detach().to(device=dev, dtype=torch.float)
        else:
            joint_policy_of(tree, player, out=policies[:, k])
    return policies


def _normalised(weights, n, what) -> torch.Tensor:
    """fp64 [n] on the host, summing to 1.  None: uniform."""
    if weights is None:
        return torch.full((n,), 1.0 / n, dtype=torch.float64)
    w = torch.as_tensor(weights).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if w.numel() != n:
        raise ValueError(f"mixture: {what} holds {w.numel()} entries for {n} players")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not float(w.sum()) > 0:
        raise ValueError(f"mixture: {what} must be finite, nonnegative and positive in sum, got {w.tolist()}")
    return w / w.sum()


def index_is_tree(tree) -> bool:
    """True when the live links (chance > 0, index != 0) that leave the states reachable from the root name distinct children, none of
    them the root: every reached state then has one parent and one path to it.  Walked level by level on the tree's device; the answer is
    kept on the tree object for the tensors it was computed from."""
    index, chance = tree.index_tensor, tree.chance_tensor
    key = (index.data_ptr(), chance.data_ptr(), index._version, chance._version)
    cached = tree.__dict__.get("_index_is_tree")
    if cached is not None and cached[0] == key:
        return cached[1]
    S = index.shape[0]
    live = (index != 0) & (chance > 0)
    frontier = torch.ones((1,), dtype=torch.long, device=index.device)
    seen = [frontier]
    ok, total = True, 1
    while ok and frontier.numel() > 0:
        children = index[frontier][live[frontier]].to(torch.long)
        total += children.numel()
        ok = total <= S and (children.numel() == 0 or (int(children.min()) > 1 and int(children.max()) < S))
        frontier = children
        seen.append(children)
    if ok:
        every = torch.cat(seen)
        ok = torch.unique(every).numel() == every.numel()
    tree.__dict__["_index_is_tree"] = (key, ok)
    return ok


def mixture(tree, players, weights=None, col_weights=None) -> Mixture:
    """The behaviour policy that plays like "draw player k with probability weights[k], then play it to the end" (Kuhn's theorem): at a
    state each member counts with the probability that its own actions lead there, which rnad_mixture sweeps top-down -- not the
    state-wise average of the tables.  players as in cross_play; weights: None (uniform) or n nonnegative numbers, normalised here in
    fp64; col_weights: the column side's, None to reuse `weights`.  The result is an ordinary [S, 2A] table for get_nashconv, cross_play
    and solve_regularized(reg=...).  A mixture of mixtures is the mixture of their members, so more than 32 policies fold in steps."""
    policies = _policy_tables(tree, players, "mixture")
    n = policies.shape[1]
    row = _normalised(weights, n, "weights")
    col = row if col_weights is None else _normalised(col_weights, n, "col_weights")
    if not index_is_tree(tree):
        raise ValueError("mixture: the index tensor is not a tree: own-action reach is undefined (a state with two parents has no "
                         "perfect recall, and no behaviour policy plays like the mixture)")
    w = torch.stack([row, col]).to(dtype=torch.float).to(policies.device)
    mix, reach = rnad_hip.mixture(tree.handle(), policies, w)
    return Mixture(policy=mix, reach=reach, weights=w)


class BestResponse(NamedTuple):
    """best_response's result.  policy [S, n, 2A]: policy[:, k] is the exploiter of player k, an ordinary one-hot joint_policy table --
    its row half the row player's best response to k's column side, its column half the column player's to k's row side; values
    [S, 2, n]: the best-response values (row_best / col_best of get_nashconv for player k); gain [S, 2, n]: what the best action gains at
    the state over k's own play of that side, with the best response below; reach [S, n]: player k's joint reach of the state, chance
    included; attribution [S, 2, n] = reach[:, None] * gain: the share of k's exploitability the state accounts for.  These live on the
    tree's device.  exploitability [n, 2]: the fp64 sum of attribution over the states, on the host -- by the performance-difference
    identity what cross_play reports as exploitability, now as a sum over states."""

    policy: torch.Tensor
    values: torch.Tensor
    gain: torch.Tensor
    reach: torch.Tensor
    attribution: torch.Tensor
    exploitability: torch.Tensor


def best_response(tree, players) -> BestResponse:
    """The exact best response to each of `players` (nets or tables, as in cross_play) as a policy table, and where on the tree each
    player is exploited: one bottom-up and one top-down sweep for all of them (rnad_best_response).  policy[:, k] plays like any other
    table: cross_play, mixture, population and solve_regularized(reg=...) take it as a player."""
    policies = _policy_tables(tree, players, "best_response")
    if not index_is_tree(tree):
        raise ValueError("best_response: the index tensor is not a tree: joint reach is undefined (a state with two parents has no "
                         "perfect recall, and its two reach values would race)")
    best, values, gain, reach = rnad_hip.best_response(tree.handle(), policies)
    attribution = reach[:, None, :] * gain
    exploitability = attribution.to(torch.float64).sum(dim=0).t().contiguous().cpu()
    return BestResponse(policy=best, values=values, gain=gain, reach=reach, attribution=attribution, exploitability=exploitability)


def _simplex_max(T, basis, max_pivots):
    """Bland's rule on a tableau whose last row holds the reduced costs and whose last column the right-hand sides, in place."""
    m = T.shape[0] - 1
    for _ in range(max_pivots):
        entering = np.flatnonzero(T[-1, :-1] < -1e-12)
        if entering.size == 0:
            return
        e = int(entering[0])
        col = T[:m, e]
        rows = np.flatnonzero(col > 1e-12)
        if rows.size == 0:
            raise ArithmeticError("meta_nash: the linear programme is unbounded")
        ratio = T[rows, -1] / col[rows]
        tied = rows[ratio <= ratio.min() * (1 + 1e-12) + 1e-300]
        r = int(tied[np.argmin(basis[tied])])  # ties: the basic variable of lowest index leaves
        T[r] /= T[r, e]
        for i in range(m + 1):
            if i != r and T[i, e] != 0.0:
                T[i] -= T[i, e] * T[r]
        basis[r] = e
    raise ArithmeticError(f"meta_nash: no optimum after {max_pivots} pivots")


def meta_nash(payoff) -> MetaNash:
    """The equilibrium of the zero-sum matrix game payoff[i, j] (the row side maximises), e.g. cross_play(...).payoff: the Nash
    averaging weights of a population.  Solved on the host in fp64: the matrix is moved into [1, 2], the column side's linear programme
    max sum z, P' z <= 1, z >= 0 runs through a simplex with Bland's rule from the slack basis, and the row side is read off the duals.
    Deterministic; sides of up to 32 (rnad_solve_matrix enumerates supports and is meant for the A x A games of a state)."""
    P = torch.as_tensor(payoff).detach().to(device="cpu", dtype=torch.float64).numpy()
    if P.ndim != 2 or min(P.shape) < 1 or max(P.shape) > rnad_hip.CROSS_PLAY_MAX or not np.isfinite(P).all():
        raise ValueError(f"meta_nash: a finite payoff matrix with sides of 1 to {rnad_hip.CROSS_PLAY_MAX}, got shape {tuple(P.shape)}")
    m, k = P.shape
    lo, span = float(P.min()), float(P.max() - P.min())
    Q = 1.0 + (P - lo) / span if span > 0 else np.ones_like(P)
    T = np.zeros((m + 1, k + m + 1))
    T[:m, :k], T[:m, k:k + m], T[:m, -1] = Q, np.eye(m), 1.0
    T[-1, :k] = -1.0
    basis = np.arange(k, k + m)
    _simplex_max(T, basis, max_pivots=200 * (m + k))
    z = np.zeros(k + m)
    z[basis] = T[:m, -1]
    col, row = np.maximum(z[:k], 0.0), np.maximum(T[-1, k:k + m], 0.0)
    col, row = col / col.sum(), row / row.sum()
    value = float(row @ P @ col)
    gap = float((P @ col).max() - (row @ P).min())
    return MetaNash(row=torch.from_numpy(row), col=torch.from_numpy(col), value=value, gap=gap)


def _nashconv_of_table(tree, data, table) -> float:
    data.joint_policy.copy_(table)
    data.get_nashconv(tree, data.joint_policy)
    return (data.row_best[1] + data.col_best[1]).item()


def population(tree, players) -> Population:
    """A population of nets or tables judged as mixtures: cross_play, the meta-Nash of its payoff matrix, then the Nash mixture (the row
    side mixed with meta.row, the column side with meta.col) and the uniform mixture as policy tables, each with its NashConv."""
    policies = _policy_tables(tree, players, "population")
    tables = [policies[:, k] for k in range(policies.shape[1])]
    cross = cross_play(tree, tables)
    meta = meta_nash(cross.payoff)
    nash = mixture(tree, tables, meta.row, meta.col).policy
    uniform = mixture(tree, tables).policy
    data = NashConvData(tree)
    return Population(cross=cross, meta=meta, nash_policy=nash, nash_nashconv=_nashconv_of_table(tree, data, nash),
                      uniform_policy=uniform, uniform_nashconv=_nashconv_of_table(tree, data, uniform))


def kld(p: torch.Tensor, q: torch.Tensor, valid: torch.Tensor, legal_actions: torch.Tensor, valid_count: int = None):
    """Masked KL(p || q) averaged over valid steps -- logging only (reference util/metric.py:193-211)."""
    if valid_count is None:
        valid_count = valid.sum().item()
    mask = (valid.unsqueeze(-1) * legal_actions).to(torch.bool)
    return torch.where(mask, p * (torch.log(p) - torch.log(q)), 0).sum().item() / valid_count
