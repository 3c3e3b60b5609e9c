"""Exact tabular R-NaD on the enumerated tree -- an addition without a counterpart in the reference.

For a regularisation policy mu and eta > 0 the fixed point of one R-NaD regularisation update is, at every state, the unique equilibrium of
the state's matrix game (payoffs: the values of its children) with the KL terms of learn/vtrace.py:234-239 added.  `solve_regularized`
computes it for the whole tree in one bottom-up sweep (rnad_reg_solve, csrc/reg_solve.hip); `TabularRNaD` feeds the result back as the next
regularisation policy (learn/rnad.py:530-531) and records NashConv after every update: the curve the algorithm itself would reach with
sampling noise, off-policy correction and function approximation taken out.  The tables have the layout of NashConvData.joint_policy, so
`util.metric.cross_play` plays them against trained nets as they are.
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
