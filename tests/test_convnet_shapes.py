"""What the GPU sweep of the ConvNet tower kernels (tests/test_hip_convnet_shapes.py) stands on, checked without a GPU.

1. The inputs of tests/_convref.py keep the reference honest: on every case of the sweep plain fp32 torch on the CPU stays within HALF
   of each gate against the fp64 reference (forward 1e-5 absolute; gradients rtol 1e-3, atol 2e-5 * max|g| per tensor -- the gates of
   tests/test_hip_convnet.py), and the ReLU-kink filter rejects at most 10 % of its candidates.  A correct fp32 kernel therefore has
   the other half of the gate for its own summation order; if a seed fails here, the seed changes (SEEDS in _convref.py), not the gate.
2. The host-side shape functions of csrc/conv_tower.hip (the library loads without a device, as tests/test_abi.py relies on):
   rnad_conv_supported, rnad_conv_param_count, rnad_conv_packed_size and rnad_conv_backward_workspace on the shapes of the sweep and
   on their declined neighbours."""
import functools

import numpy as np
import pytest
import torch

import _convref as cr

SWEEP = sorted(cr.SHAPES)
DECLINED = {
    (7, 16, 1): "does not fit the LDS",
    (6, 16, 1): "does not fit the LDS",
    (3, 8, 1): "channels * A is not a multiple of 16",
    (4, 4, 9): "the depth is too large",
    (9, 16, 1): "A is too large",
}


def _id(shape):
    return "-".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def _case(shape, N, kink=True):
    return cr.case(*shape, N, cr.seed_of(shape), kink=kink)


def _fp32(c, rows=None, grads=True):
    """Plain fp32 torch on the CPU: logits and value of every row, gradients over `rows`."""
    net = c.net
    with torch.no_grad():
        logits, value = net.forward_logits(c.obs)
    g = None
    if grads:
        sel = torch.arange(c.N) if rows is None else torch.as_tensor(rows, dtype=torch.long)
        net.zero_grad()
        l, v = net.forward_logits(c.obs[sel])
        torch.autograd.backward([l, v], [c.dlogits[sel], c.dv[sel]])
        g = [p.grad.numpy().copy() for p in net.parameters()]
        net.zero_grad()
    return logits.numpy(), value.numpy(), g


def _half_gates(c, rows=None, grads=True):
    want_l, want_v, want_g = cr.reference(c, rows, grads)
    got_l, got_v, got_g = _fp32(c, rows, grads)
    print(c.shape, "N", c.N, "fp32 torch forward error", float(max(np.abs(got_l - want_l).max(), np.abs(got_v - want_v).max())))
    np.testing.assert_allclose(got_l, want_l, rtol=0, atol=cr.FWD_ATOL / 2, err_msg="logits")
    np.testing.assert_allclose(got_v, want_v, rtol=0, atol=cr.FWD_ATOL / 2, err_msg="value")
    if not grads:
        return
    worst = 0.0
    for (k, _), g, w in zip(c.net.named_parameters(), got_g, want_g):
        tol = cr.GRAD_ATOL * np.abs(w).max() + cr.GRAD_RTOL * np.abs(w)
        worst = max(worst, float((np.abs(g - w) / tol).max()))
        np.testing.assert_allclose(g, w, rtol=cr.GRAD_RTOL / 2, atol=cr.GRAD_ATOL / 2 * np.abs(w).max(), err_msg=k)
    print(c.shape, "N", c.N, "rows", "all" if rows is None else len(rows), "share of the gradient gate used by fp32 torch", round(worst, 4))


# ------------------------------------------------------------------------------------------------ the builder
def test_shape_table_names_the_paths_the_kernels_take():
    """The table's (NT, plain | lean) against the LDS arithmetic of ConvShape: if the kernel's layout changes, the sweep's shapes have
    to be chosen again so that every variant still runs."""
    for shape, want in cr.SHAPES.items():
        assert cr.paths(*shape) == want, shape
    for shape, nt in cr.FWD_LOOP_NT.items():
        assert cr.paths(*shape)[0] == nt, shape
    assert {nt for nt, _ in cr.SHAPES.values()} == {4, 2, 1} and {b for _, b in cr.SHAPES.values()} == {"plain", "lean"}
    assert not any(nt == 1 and b == "plain" for nt, b in (cr.paths(A, Ch, D) for A in range(1, 9) for Ch in range(2, 257) for D in range(1, 9)
                                                           if (Ch * A) % 16 == 0) if b), "no supported shape has NT = 1 with the plain backward"
    for shape, N in cr.FWD_LOOP.items():
        ns = 16 * cr.FWD_LOOP_NT[shape]
        assert 1024 * ns < N <= 1025 * ns, "one tile past 1024 workgroups"
    for N in cr.BWD_LOOP.values():
        assert 256 * 16 < N < 257 * 16 + 64 and N % 16 != 0


@pytest.mark.parametrize("shape", SWEEP, ids=_id)
def test_fp32_torch_uses_at_most_half_of_each_gate_on_the_sweep(shape):
    c = _case(shape, cr.N_SWEEP)
    assert c.obs.shape == (cr.N_SWEEP, 2, shape[0], shape[0]) and c.dlogits.shape == (cr.N_SWEEP, shape[0]) and c.dv.shape == (cr.N_SWEEP, 1)
    assert c.rejected <= 0.10, f"the kink filter rejected {c.rejected:.1%} of its candidates"
    assert set(np.unique(c.obs[:, 1].numpy())) <= {0.0, 1.0} and 0.6 < float(c.obs[:, 1].mean()) < 0.9
    assert float(c.obs[:, 0].min()) >= -1 and float(c.obs[:, 0].max()) <= 1
    _half_gates(c)
    _half_gates(c, cr.sweep_rows())


@pytest.mark.parametrize("shape", sorted(cr.BWD_LOOP), ids=_id)
def test_fp32_torch_uses_at_most_half_of_each_gate_at_the_backward_tile_loop(shape):
    c = _case(shape, cr.BWD_LOOP[shape])
    assert c.rejected <= 0.10, f"the kink filter rejected {c.rejected:.1%} of its candidates"
    _half_gates(c)


@pytest.mark.parametrize("shape", sorted(cr.FWD_LOOP), ids=_id)
def test_fp32_torch_uses_at_most_half_of_the_forward_gate_at_the_forward_tile_loop(shape):
    _half_gates(_case(shape, cr.FWD_LOOP[shape], False), grads=False)


def test_the_kink_filter_keeps_samples_off_the_kink_and_is_deterministic():
    shape = (4, 4, 2)
    c = _case(shape, cr.N_SWEEP)
    assert float(cr._preacts(c.ref, c.obs.double()).min()) >= cr.KINK
    again = cr.case(*shape, cr.N_SWEEP, cr.seed_of(shape))
    assert torch.equal(again.obs, c.obs) and torch.equal(again.dlogits, c.dlogits) and torch.equal(again.dv, c.dv)
    for p, q in zip(again.net.parameters(), c.net.parameters()):
        assert torch.equal(p, q)
    for p, q in zip(c.ref.parameters(), c.net.parameters()):
        assert p.dtype == torch.float64 and torch.equal(p.float(), q)
    raw = cr.case(*shape, cr.N_SWEEP, cr.seed_of(shape), kink=False)
    assert raw.rejected == 0.0 and raw.obs.shape == c.obs.shape


# ------------------------------------------------------------------------------------------------ host-side shape functions
def _lib():
    import rnad_hip

    return rnad_hip.lib()


def _part_total(A, Ch, D):
    """Floats of one workgroup's partial slice (ConvShape::part_total): per layer both Toeplitz-shaped products and the bias, then the heads."""
    M, F = Ch * A, Ch * A * A
    return (2 * M * 2 * A + Ch) + 2 * D * (2 * M * M + Ch) + A * F + F + A + 1


@pytest.mark.parametrize("shape", SWEEP + sorted(cr.FWD_LOOP), ids=_id)
def test_supported_shapes_and_their_parameter_count(shape):
    from nn.net import ConvNet

    lib = _lib()
    assert lib.rnad_conv_supported(*shape) == 1
    net = ConvNet(*shape[:2], depth=shape[2], batch_norm=False)
    assert lib.rnad_conv_param_count(*shape) == sum(p.numel() for p in net.parameters())
    assert lib.rnad_conv_packed_size(*shape) > 0 and lib.rnad_conv_packed_size(*shape) % 4 == 0


@pytest.mark.parametrize("shape", SWEEP, ids=_id)
def test_backward_workspace_grows_with_the_workgroups(shape):
    lib = _lib()
    one = lib.rnad_conv_backward_workspace(0, *shape)
    assert one == 4 * _part_total(*shape)
    for N, slices in ((0, 1), (16, 1), (17, 2), (4096, 256), (4097, 256), (10**6, 256)):
        assert lib.rnad_conv_backward_workspace(N, *shape) == slices * one, N
    assert lib.rnad_conv_backward_workspace(-1, *shape) == -1


@pytest.mark.parametrize("shape", sorted(DECLINED), ids=_id)
def test_declined_neighbours(shape):
    lib = _lib()
    assert lib.rnad_conv_supported(*shape) == 0, DECLINED[shape]
    assert lib.rnad_conv_param_count(*shape) == -1 and lib.rnad_conv_packed_size(*shape) == -1
    assert lib.rnad_conv_backward_workspace(16, *shape) == -1
