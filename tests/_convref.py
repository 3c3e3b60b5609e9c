"""Inputs and the fp64 reference for the shape sweep of the ConvNet tower kernels (tests/test_convnet_shapes.py on the CPU,
tests/test_hip_convnet_shapes.py on the GPU).

The reference is the torch modules of nn/net.py in double precision on the CPU: tests/test_convnet.py pins them to the original
implementation (forward and fp64 gradients), so at any shape they are a plain high-precision statement of what csrc/conv_tower.hip
computes.

The ReLU kink.  A gradient is discontinuous where a ReLU input crosses zero: a sample whose pre-activation lies within fp32 rounding
of zero can take the other branch in a CORRECT fp32 implementation, and its whole contribution then differs from the fp64 gradient.
That is a property of the inputs, not of a kernel, so `case` draws 2N candidate samples and keeps the first N whose smallest
|pre-activation| over every tower[d].conv0 / conv1 (fp64) is at least KINK = 1e-5, the project's fp32 forward bound.  At most half of
the candidates may be rejected -- a condition of the builder, asserted, not a measurement; tests/test_convnet_shapes.py holds the
rejected share under 10 % and shows that plain fp32 torch on these inputs uses at most half of each gate, which is what licenses the
gates on the GPU.
"""
import copy
import types

import numpy as np
import torch

KINK = 1e-5      # smallest |ReLU input| a kept sample may have: the fp32 forward bound (README.md)
FWD_ATOL = 1e-5  # forward gate, absolute (tests/test_hip_convnet.py)
GRAD_RTOL, GRAD_ATOL = 1e-3, 2e-5  # gradient gate: rtol, atol as a share of max|g| of the tensor (tests/test_hip_convnet.py)

# (A, channels, depth) -> (sample tiles NT of k_conv_forward, variant of k_conv_backward) at this commit, from ConvShape::fwd_lds /
# bwd_lds / bwd_lds_lean against 160 KiB (`paths` restates them; tests/test_convnet_shapes.py holds the table to it).
SHAPES = {
    (1, 16, 1): (4, "plain"),  # A = 1: one tap, 1 x 1 board; pre-layer K = 2 padded to 4
    (2, 8, 1): (4, "plain"),   # Mt = 1
    (2, 24, 8): (4, "lean"),   # depth 8, the declared maximum
    (2, 56, 3): (2, "lean"),   # Mt = 7
    (3, 32, 1): (2, "plain"),  # Mt = 6
    (3, 48, 1): (1, "lean"),   # NT = 1; lean at depth 1; Mt = 9
    (4, 4, 2): (4, "plain"),   # Ch = 4; pre-layer K = 8 exact
    (4, 20, 2): (2, "lean"),   # Mt = 5
    (4, 28, 1): (1, "lean"),   # NT = 1; lean at depth 1; Mt = 7
    (6, 8, 1): (2, "plain"),   # A = 6
    (6, 8, 3): (2, "lean"),
    (8, 2, 1): (4, "plain"),   # Ch = 2: bias_grad on 32 lanes; pre-layer ncols = 16 exact
    (8, 2, 8): (4, "lean"),
    (8, 6, 1): (2, "plain"),
    (8, 4, 3): (2, "lean"),    # Mt = 2
}
N_SWEEP = 203  # = 3*64 + 11 = 6*32 + 11 = 12*16 + 11: every NT ends on a partial tile
# the backward gives a workgroup a second 16-sample tile past 256 * 16 rows: 4149 = 256*16 + 53, workgroups 0-3 take one, the last holds 5 rows
BWD_LOOP = {(2, 8, 1): 4149, (2, 24, 8): 4149}
# the forward gives a workgroup a second tile past 1024 * 16 NT rows: each case is one (partial) tile past that
FWD_LOOP = {(2, 8, 1): 65536 + 11, (4, 16, 1): 32768 + 11, (4, 28, 1): 16384 + 11}
FWD_LOOP_NT = {(2, 8, 1): 4, (4, 16, 1): 2, (4, 28, 1): 1}
SEEDS = {}  # shape -> seed where the default 0 does not satisfy tests/test_convnet_shapes.py (change the seed, never a gate)


def seed_of(shape):
    return SEEDS.get(tuple(shape), 0)


def sweep_rows(N=N_SWEEP):
    """The row list of the sweep: a stride pattern and a hole that spans more than two 16-sample tiles."""
    return np.array([r for r in range(N) if r % 5 != 2 and not 40 <= r < 75], np.int32)


def paths(A, Ch, D, lds=160 * 1024):
    """(NT, "plain" | "lean" | None) of a shape: a host restatement of ConvShape::fwd_lds / bwd_lds / bwd_lds_lean and fwd_tiles."""
    F = Ch * A * A
    P, XP = F | 1, (2 * A * A) | 1
    nt = next((n for n in (4, 2, 1) if 3 * n * 16 * P * 4 <= lds), 0)
    plain = 16 * ((3 * D + 3) * P + XP + A + 1) * 4
    lean = 16 * ((D + 4) * P + XP + A + 1) * 4
    return nt, ("plain" if plain <= lds else "lean" if lean <= lds else None)


def _preacts(ref, obs64):
    """Smallest |ReLU input| of every sample over the tower of the fp64 net."""
    seen = []
    hooks = [conv.register_forward_hook(lambda m, i, out: seen.append(out.detach().abs().flatten(1).min(1).values))
             for block in ref.tower for conv in (block.conv0, block.conv1)]
    try:
        with torch.no_grad():
            ref.forward_logits(obs64)
    finally:
        for h in hooks:
            h.remove()
    assert len(seen) == 2 * len(ref.tower)
    return torch.stack(seen).min(0).values


def _draw(n, A, g):
    obs = torch.empty((n, 2, A, A))
    obs[:, 0] = torch.rand((n, A, A), generator=g) * 2 - 1
    obs[:, 1] = (torch.rand((n, A, A), generator=g) < 0.75).float()
    return obs


def case(A, Ch, depth, N, seed, kink=True, device=None):
    """The fp32 net (on `device`), its fp64 CPU copy, obs [N, 2, A, A], dlogits [N, A] and dv [N, 1] (fp32, CPU).
    kink=False: the first N candidates as they come (forward-only cases: the forward is continuous)."""
    from nn.net import ConvNet

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ConvNet(A, Ch, depth=depth, batch_norm=False)
        with torch.no_grad():
            for k, p in net.named_parameters():
                if k.endswith("bias"):
                    p.copy_(torch.randn_like(p) * 0.3)  # as tests/golden/make_convnet.py: the default biases are nearly zero
    ref = copy.deepcopy(net).double()
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    rejected = 0.0
    if kink:
        cand = _draw(2 * N, A, g)
        keep = _preacts(ref, cand.double()) >= KINK
        assert int(keep.sum()) >= N, f"({A},{Ch},{depth}) seed {seed}: more than half of the candidates sit on a ReLU kink"
        rejected = 1.0 - float(keep.float().mean())
        obs = cand[keep][:N].contiguous()
    else:
        obs = _draw(N, A, g)
    dlogits, dv = torch.randn((N, A), generator=g), torch.randn((N, 1), generator=g)
    if device is not None:
        net = net.to(device)
        net.device = device
    return types.SimpleNamespace(shape=(A, Ch, depth), N=N, seed=seed, net=net, ref=ref, obs=obs, dlogits=dlogits, dv=dv, rejected=rejected)


def reference(c, rows=None, grads=True):
    """fp64: logits [N, A] and value [N, 1] of every row, and the autograd gradients of every parameter (parameters() order) of
    sum(logits * dlogits) + sum(value * dv) over `rows` (None: all).  numpy arrays, read-only."""
    ref = c.ref
    obs64 = c.obs.double()
    with torch.no_grad():
        logits, value = ref.forward_logits(obs64)
    out = [logits.numpy(), value.numpy()]
    if grads:
        sel = torch.arange(c.N) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
        ref.zero_grad()
        l64, v64 = ref.forward_logits(obs64[sel])
        torch.autograd.backward([l64, v64], [c.dlogits.double()[sel], c.dv.double()[sel]])
        out.append([p.grad.numpy().copy() for p in ref.parameters()])
        ref.zero_grad()
    else:
        out.append(None)
    for a in [out[0], out[1]] + (out[2] or []):
        a.setflags(write=False)
    return tuple(out)


def gate(got, want, what=""):
    """The gradient gate of tests/test_hip_convnet.py."""
    want = np.asarray(want)
    np.testing.assert_allclose(np.asarray(got), want, rtol=GRAD_RTOL, atol=GRAD_ATOL * np.abs(want).max(), err_msg=what)
