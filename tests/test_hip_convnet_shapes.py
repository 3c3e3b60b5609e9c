"""csrc/conv_tower.hip against the fp64 torch modules over every kernel variant and the tile loops.

tests/test_hip_convnet.py compares the tower kernels with the reference's recorded nets at four shapes and a few hundred rows.  The file
picks its code by shape and by row count; this sweep runs what those fixtures do not reach, each against tests/_convref.py (the torch
modules of nn/net.py in double precision on the CPU, pinned to the original by tests/test_convnet.py):

  k_conv_forward<NT>      NT = 4, 2 and 1 sample tiles per workgroup, each ending on a partial tile (N = 203); the loop that gives a
                          workgroup a second tile (N > 1024 * 16 NT) at every NT
  k_conv_backward<LEAN>   plain and lean, lean at depth 1 (one H buffer, H_D in Gz from the first block on, G on Rs), 3 and 8; the loop that
                          gives a workgroup a second tile (N > 4096), where everything accumulates into the workgroup's partial slice
  shapes                  A in 1 .. 8 (the pre-layer's K padded or exact), Mt = channels * A / 16 in {1, 2, 5, 6, 7, 9}, channels = 2
                          (bias_grad on half a wave), depth 8
  FwdActor<A>             A = 2, 4, 8 and NT = 1, its policy rows against the CPU oracle

The path of every shape is the table SHAPES of _convref.py (held to the LDS arithmetic by tests/test_convnet_shapes.py).  Gates: forward
1e-5 absolute, gradients rtol 1e-3 / atol 2e-5 * max|g| (tests/test_hip_convnet.py), policy rows rtol 1e-5 / atol 1e-7
(tests/test_hip_parity.py::test_policy_head); tests/test_convnet_shapes.py shows that fp32 torch itself uses at most half of the first
two on these inputs.  Every comparison goes through np.testing.assert_allclose: profiles/convnet_shapes_errors.json is the record of a
run on an MI355X."""
import functools

import numpy as np
import pytest
import torch

import _convref as cr

pytestmark = pytest.mark.gpu

SWEEP = sorted(cr.SHAPES)
NAN = float("nan")
SENTINEL = 7.0


def _id(shape):
    return "-".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def _case(shape, N, kink=True):
    """The case on the device, built once: net, packed image, inputs, and the fp64 reference (read-only) of all rows."""
    from _gpu import DEV

    c = cr.case(*shape, N, cr.seed_of(shape), kink=kink, device=DEV)
    c.obs_d, c.dl_d, c.dv_d = c.obs.to(DEV), c.dlogits.to(DEV), c.dv.to(DEV)
    c.packed = c.net.pack()
    c.want_l, c.want_v, c.want_g = cr.reference(c, None, grads=kink)
    return c


def _backward(c, obs, dl, dv, **kw):
    import rnad_hip

    return rnad_hip.conv_backward(c.packed, c.net._weights(), *c.net._shape(), obs, dl, dv, **kw)


def _gate_all(c, got, want, what):
    from _gpu import cpu

    assert len(got) == len(want) == 8 + 8 * c.shape[2]
    for (k, _), g, w in zip(c.net.named_parameters(), got, want):
        cr.gate(cpu(g), w, f"{c.shape} {what} {k}")


def _with_nan_elsewhere(listed, *tensors):
    """Copies of the tensors with NaN in every row that is not listed: a kernel that reads such a row poisons its output."""
    out = []
    for t in tensors:
        t = t.clone()
        t[~listed] = NAN
        out.append(t)
    return out


@pytest.mark.parametrize("shape", SWEEP, ids=_id)
def test_sweep_forward_and_backward(shape):
    from _gpu import cpu

    c = _case(shape, cr.N_SWEEP)
    net = c.net
    assert net._fusable(), "every shape of the sweep must take the tower kernels"
    with torch.no_grad():
        logits, value = net.forward_logits(c.obs_d, packed=c.packed)
        only_l, none_v = net.forward_logits(c.obs_d, want_value=False, packed=c.packed)
        none_l, only_v = net.forward_logits(c.obs_d, want_logits=False, packed=c.packed)
    np.testing.assert_allclose(cpu(logits), c.want_l, rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} logits")
    np.testing.assert_allclose(cpu(value), c.want_v, rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} value")
    assert none_v is None and none_l is None and torch.equal(only_l, logits) and torch.equal(only_v, value)
    got = _backward(c, c.obs_d, c.dl_d, c.dv_d)
    again = _backward(c, c.obs_d, c.dl_d, c.dv_d)
    _gate_all(c, got, c.want_g, "all rows")
    for x, y in zip(got, again):
        assert torch.equal(x, y), "two backward calls on the same inputs must give identical bits"


@pytest.mark.parametrize("shape", SWEEP, ids=_id)
def test_sweep_row_lists(shape):
    import rnad_hip
    from _gpu import DEV, cpu

    c = _case(shape, cr.N_SWEEP)
    N, A = c.N, shape[0]
    rows = cr.sweep_rows(N)
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
    obs, dl, dv = _with_nan_elsewhere(listed, c.obs_d, c.dl_d, c.dv_d)
    live = rnad_hip.RowList(rows, N, DEV)
    out_l, out_v = torch.full((N, A), SENTINEL, device=DEV), torch.full((N, 1), SENTINEL, device=DEV)
    rnad_hip.conv_forward(c.packed, *c.net._shape(), obs, live=live, out=(out_l, out_v))
    np.testing.assert_allclose(cpu(out_l[listed]), c.want_l[rows], rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} logits of the listed rows")
    np.testing.assert_allclose(cpu(out_v[listed]), c.want_v[rows], rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} value of the listed rows")
    assert (out_l[~listed] == SENTINEL).all() and (out_v[~listed] == SENTINEL).all(), "rows that are not listed are left alone"
    _, _, want_g = cr.reference(c, rows)
    got = _backward(c, obs, dl, dv, live=live)
    for g in got:
        assert torch.isfinite(g).all(), "a row that is not listed was read"
    _gate_all(c, got, want_g, "row list")
    # a fixed list: a buffer of N entries whose first `count` are the rows (the others name NaN rows), launched for its capacity
    rest = np.array(sorted(set(range(N)) - set(rows.tolist())), np.int32)
    fixed = rnad_hip.RowList(np.concatenate([rows, rest]), N, DEV)
    fixed.count.fill_(len(rows))
    cap = _backward(c, obs, dl, dv, live=fixed, capacity=N)
    for x, y in zip(got, cap):
        assert torch.equal(x, y), "the same rows in a list of larger capacity must give identical bits"


@pytest.mark.parametrize("shape", sorted(cr.BWD_LOOP), ids=_id)
def test_backward_tile_loop(shape):
    """More than 256 16-sample tiles: workgroups 0 - 3 take a second one and add to the partials of their first.  (Not larger: at 32 777
    rows plain fp32 torch itself used 17 times the gradient gate.)"""
    import rnad_hip
    from _gpu import DEV

    c = _case(shape, cr.BWD_LOOP[shape])
    N = c.N
    assert rnad_hip.lib().rnad_conv_backward_workspace(N, *shape) == rnad_hip.lib().rnad_conv_backward_workspace(4096, *shape) and N > 4096
    _gate_all(c, _backward(c, c.obs_d, c.dl_d, c.dv_d), c.want_g, f"all {N} rows")
    # the same samples as the even rows of a table twice as long, NaN in its odd rows
    rows = np.arange(0, 2 * N, 2, dtype=np.int32)
    table = []
    for t in (c.obs_d, c.dl_d, c.dv_d):
        wide = torch.full((2 * N,) + tuple(t.shape[1:]), NAN, device=DEV)
        wide[::2] = t
        table.append(wide)
    got = _backward(c, *table, live=rnad_hip.RowList(rows, 2 * N, DEV))
    for g in got:
        assert torch.isfinite(g).all(), "a row that is not listed was read"
    _gate_all(c, got, c.want_g, f"{N} even rows of {2 * N}")


@pytest.mark.parametrize("shape", sorted(cr.FWD_LOOP), ids=_id)
def test_forward_tile_loop(shape):
    """One tile past 1024 workgroups, at NT = 4, 2 and 1: workgroup 0 walks the loop twice and reuses its LDS."""
    from _gpu import cpu

    c = _case(shape, cr.FWD_LOOP[shape], False)
    assert c.net._fusable()
    with torch.no_grad():
        logits, value = c.net.forward_logits(c.obs_d, packed=c.packed)
    np.testing.assert_allclose(cpu(logits), c.want_l, rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} logits N={c.N}")
    np.testing.assert_allclose(cpu(value), c.want_v, rtol=0, atol=cr.FWD_ATOL, err_msg=f"{shape} value N={c.N}")


ACTOR_CASES = {  # tree -> (channels, depth) of the net on it, NT of its forward
    "a4": (dict(A=4, C=1, depth=2, seed=7), (28, 1), 1),
    "a8": (dict(A=8, C=1, depth=2, seed=7), (2, 1), 4),
    "binary": (None, (56, 3), 2),                        # TREES["binary"] of tests/test_hip_bucket.py: A = 2, two pad columns
    # the two trees above with fewer than 90 rows, deeper: the 87-row list of tests/test_hip_convnet_lazy.py fits these as it stands
    "a4_deeper": (dict(A=4, C=1, depth=3, seed=7), (28, 1), 1),
    "binary_deeper": (dict(A=2, C=1, depth=5, seed=1), (56, 3), 2),
}


def _odd_rows(S):
    """The "odd" list of tests/test_hip_convnet_lazy.py (87 rows from row 3 on: whole 16-sample tiles and 7 rows more).  On a tree with
    fewer rows than that list reaches, the same list cut to the tree: from row 3 on, as many whole 16-sample tiles as fit, and 7 rows."""
    from test_hip_convnet_lazy import _row_lists

    N = 2 * S
    if N >= 90:
        return _row_lists(S)["odd"]
    odd = np.arange(3, 3 + (N - 10) // 16 * 16 + 7, dtype=np.int32)
    assert len(odd) > 16 and len(odd) % 16 == 7 and odd[-1] < N
    return odd


@pytest.mark.parametrize("name", sorted(ACTOR_CASES))
def test_actor_epilogue_other_shapes(name):
    """rnad_conv_forward_actor where tests/test_hip_convnet_lazy.py does not take it (A = 3 and 5, NT >= 2 there): logits and value carry
    the bits of rnad_conv_forward, the policy rows are the CPU oracle's policy head of the launch's own logits under each row's legal
    mask, pad columns are zeros, rows that are not listed keep what they held."""
    import rnad_hip
    from _gpu import DEV, cpu
    from nn.net import ConvNet
    from oracle import oracle
    from test_hip_bucket import TREES, _native_tree

    kw, (Ch, depth), nt = ACTOR_CASES[name]
    tree = _native_tree(**(kw or TREES[name]))
    h = tree.handle()
    A, S = tree.max_actions, h.S
    N = 2 * S
    assert cr.paths(A, Ch, depth)[0] == nt
    torch.manual_seed(5)
    net = ConvNet(A, Ch, depth=depth, batch_norm=False, device=DEV)
    assert net._fusable() and net.lazy_rows_ready()
    packed, table = net.pack(), h.observations_table()
    stride = int(rnad_hip.lib().rnad_bucket_policy_row_stride(A))
    mask = cpu(table[:, 1, :, 0].float().contiguous())  # the mover's legal actions: legal[a][0] of its view of the state
    for rows in (None, _odd_rows(S)):
        live = None if rows is None else rnad_hip.RowList(rows, N, DEV)
        logits = torch.full((N, A), SENTINEL, device=DEV)
        value = torch.full((N, 1), SENTINEL, device=DEV)
        pol = torch.full((N, stride), SENTINEL, device=DEV)
        rnad_hip.conv_forward_actor(h, packed, *net._shape(), table, logits, value, pol, rows=live)
        want_l, want_v = rnad_hip.conv_forward(packed, *net._shape(), table, live=live)
        listed = torch.ones(N, dtype=torch.bool, device=DEV)
        if rows is not None:
            listed[:] = False
            listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
        assert torch.equal(logits[listed], want_l[listed]) and torch.equal(value[listed], want_v[listed])
        sel = cpu(listed)
        want_pol, _ = oracle.policy_head(cpu(logits)[sel], mask[sel], want_log=False)
        np.testing.assert_allclose(cpu(pol)[sel][:, :A], want_pol, rtol=1e-5, atol=1e-7, err_msg=f"{name} policy rows")
        assert ((cpu(pol)[sel][:, :A] == 0) == (mask[sel] == 0)).all()
        assert (pol[listed][:, A:] == 0).all(), "pad columns are zeros"
        for out in (logits, value, pol):
            assert (out[~listed] == SENTINEL).all(), "rows that are not listed are left alone"
