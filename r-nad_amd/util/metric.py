"""NashConv evaluation -- drop-in for reference util/metric.py, level-batched on the GPU.

`NashConvData(tree)` keeps the reference's attributes (`joint_policy, row_best, col_best, reach_probability, depth`)
and methods (`get_nashconv_from_net`, `get_nashconv`, `mean_nashconv_by_depth`).  The reference moves the tree to the
CPU and recurses in Python with ~20 tiny tensor ops per state (metric.py:84-175); here the whole tree is inferenced
with two `forward_policy` calls per slice and the best-response values come from rnad_nashconv's two level sweeps.

`cross_play(tree, players)` is an addition without a counterpart in the reference: the exact payoff matrix of n nets or policy
tables against each other (rnad_cross_play, one bottom-up sweep for all n * n pairs), with each player's NashConv next to it.
"""
from typing import Dict, NamedTuple

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
    players = list(players)
    n = len(players)
    if not 1 <= n <= rnad_hip.CROSS_PLAY_MAX:
        raise ValueError(f"cross_play takes 1 to {rnad_hip.CROSS_PLAY_MAX} players, got {n}")
    S, A = tree.value_tensor.shape[0], tree.max_actions
    handle = tree.handle()
    dev = tree.value_tensor.device
    policies = torch.zeros((S, n, 2 * A), device=dev, dtype=torch.float)
    for k, player in enumerate(players):
        if torch.is_tensor(player):
            if tuple(player.shape) != (S, 2 * A):
                raise ValueError(f"player {k}: a policy table must be [{S}, {2 * A}], got {tuple(player.shape)}")
            policies[:, k] = player.detach().to(device=dev, dtype=torch.float)
        else:
            joint_policy_of(tree, player, out=policies[:, k])
    values = rnad_hip.cross_play(handle, policies)
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


def kld(p: torch.Tensor, q: torch.Tensor, valid: torch.Tensor, legal_actions: torch.Tensor, valid_count: int = None):
    """Masked KL(p || q) averaged over valid steps -- logging only (reference util/metric.py:193-211)."""
    if valid_count is None:
        valid_count = valid.sum().item()
    mask = (valid.unsqueeze(-1) * legal_actions).to(torch.bool)
    return torch.where(mask, p * (torch.log(p) - torch.log(q)), 0).sum().item() / valid_count
