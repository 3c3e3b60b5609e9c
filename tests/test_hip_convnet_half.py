"""fp16 observation tables through the CrossConv tower kernels (csrc/conv_tower.hip instantiated on `__half` observations:
rnad_conv_forward_obs / rnad_conv_forward_actor_obs / rnad_conv_backward_obs).

The yardstick needs no tolerance.  An fp16 table holds values fp32 represents exactly and the kernels differ only in the load of a tile,
so every output on an fp16 table `t` must equal, BIT FOR BIT, the output of the fp32 path of the same build on `t.float()` -- and the fp32
path is pinned against fp64 over every variant by tests/test_hip_convnet_shapes.py.  Every comparison below is of int32 views (so -0.0
and NaN count as what they are)."""
import ctypes as C
import functools

import pytest
import torch

import _convref as cr

pytestmark = pytest.mark.gpu

SWEEP = sorted(cr.SHAPES)
NAMES = ("pruned", "a5c4")
SENTINEL = 7.0
# -0.0, the smallest fp16 subnormal, another subnormal, the smallest normal (negative) and the largest finite value
SPECIALS = (-0.0, 2.0 ** -24, 2.0 ** -15, -(2.0 ** -14), 65504.0)
SPECIAL_ROWS = (0, 1, 3, 4, 5)  # rows of cr.sweep_rows(): the list reads them too


def _id(shape):
    return "-".join(map(str, shape))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, what=""):
    assert got.dtype == torch.float32 and want.dtype == torch.float32 and got.shape == want.shape, what
    assert torch.equal(_bits(got), _bits(want)), f"{what}: the fp16 table must give the bits of the up-converted table"


@functools.lru_cache(maxsize=None)
def _case(shape, N):
    """Net, packed image and inputs of one shape on the device, built once: the fp16 table (the case's observations rounded, a few
    elements overwritten with SPECIALS) and its exact fp32 image."""
    from _gpu import DEV

    c = cr.case(*shape, N, cr.seed_of(shape), kink=False, device=DEV)
    assert c.net._fusable(), "every shape here must take the tower kernels"
    OBS = 2 * shape[0] ** 2
    half = c.obs.half().reshape(N, OBS)
    for k, (row, x) in enumerate(zip(SPECIAL_ROWS, SPECIALS)):
        half[row, k % OBS] = x
    want = torch.tensor(SPECIALS, dtype=torch.float64)
    got = torch.stack([half[row, k % OBS] for k, row in enumerate(SPECIAL_ROWS)]).double()
    assert torch.equal(got, want) and torch.signbit(got[0]), "fp16 holds the special values exactly"
    c.half = half.reshape(N, 2, shape[0], shape[0]).to(DEV)
    c.up = c.half.float()
    c.dl_d, c.dv_d = c.dlogits.to(DEV), c.dv.to(DEV)
    c.packed = c.net.pack()
    return c


def _forward(c, obs, **kw):
    import rnad_hip

    return rnad_hip.conv_forward(c.packed, *c.net._shape(), obs, **kw)


def _backward(c, obs, dl, dv, **kw):
    import rnad_hip

    return rnad_hip.conv_backward(c.packed, c.net._weights(), *c.net._shape(), obs, dl, dv, **kw)


def _same_grads(c, got, want, what):
    assert len(got) == len(want) == 8 + 8 * c.shape[2]
    for (k, _), g, w in zip(c.net.named_parameters(), got, want):
        _same(g, w, f"{c.shape} {what} {k}")


def _poisoned(listed, *tensors):
    """Copies with NaN in every row that is not listed: a kernel that reads such a row poisons its output."""
    out = []
    for t in tensors:
        t = t.clone()
        t[~listed] = float("nan")
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. sweep
@pytest.mark.parametrize("shape", SWEEP, ids=_id)
def test_sweep(shape):
    import rnad_hip
    from _gpu import DEV

    c = _case(shape, cr.N_SWEEP)
    N, A = c.N, shape[0]
    # forward, all rows: both heads, each head alone
    want_l, want_v = _forward(c, c.up)
    got_l, got_v = _forward(c, c.half)
    _same(got_l, want_l, f"{shape} logits")
    _same(got_v, want_v, f"{shape} value")
    only_l, none_v = _forward(c, c.half, want_value=False)
    none_l, only_v = _forward(c, c.half, want_logits=False)
    assert none_v is None and none_l is None
    _same(only_l, want_l, f"{shape} logits alone")
    _same(only_v, want_v, f"{shape} value alone")
    # forward, row list: rows that are not listed hold fp16 NaN and keep the sentinel in the outputs
    rows = cr.sweep_rows(N)
    assert set(SPECIAL_ROWS) <= set(rows.tolist())
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
    half, dl, dv = _poisoned(listed, c.half, c.dl_d, c.dv_d)
    assert half.dtype == torch.float16 and torch.isnan(half[~listed]).all()
    live = rnad_hip.RowList(rows, N, DEV)
    outs = {}
    for key, obs in (("half", half), ("up", half.float())):
        out_l, out_v = torch.full((N, A), SENTINEL, device=DEV), torch.full((N, 1), SENTINEL, device=DEV)
        _forward(c, obs, live=live, out=(out_l, out_v))
        outs[key] = (out_l, out_v)
    _same(outs["half"][0], outs["up"][0], f"{shape} logits of the list")
    _same(outs["half"][1], outs["up"][1], f"{shape} value of the list")
    assert (outs["half"][0][~listed] == SENTINEL).all() and (outs["half"][1][~listed] == SENTINEL).all(), "rows that are not listed are left alone"
    # backward, all rows and the row list: every gradient tensor, and a second call
    for what, args, kw in (("all rows", (c.dl_d, c.dv_d), {}), ("row list", (dl, dv), dict(live=live))):
        obs = c.half if not kw else half
        want = _backward(c, obs.float(), *args, **kw)
        got = _backward(c, obs, *args, **kw)
        again = _backward(c, obs, *args, **kw)
        if kw:
            for g in got:
                assert not torch.isnan(g).any(), f"{shape} {what}: a row that is not listed was read"
        _same_grads(c, got, want, what)
        _same_grads(c, again, got, what + ", second call")


# ------------------------------------------------------------------------------------------------------------------ 2. tile loops
@pytest.mark.parametrize("shape", sorted(cr.FWD_LOOP), ids=_id)
def test_forward_tile_loop(shape):
    """One tile past 1024 workgroups at NT = 4, 2 and 1: workgroup 0 stages a second fp16 tile over its first."""
    c = _case(shape, cr.FWD_LOOP[shape])
    assert cr.paths(*shape)[0] == cr.FWD_LOOP_NT[shape]
    want_l, want_v = _forward(c, c.up)
    got_l, got_v = _forward(c, c.half)
    _same(got_l, want_l, f"{shape} logits N={c.N}")
    _same(got_v, want_v, f"{shape} value N={c.N}")


@pytest.mark.parametrize("shape", sorted(cr.BWD_LOOP), ids=_id)
def test_backward_tile_loop(shape):
    """More than 256 16-sample tiles, plain and lean: workgroups 0 - 3 take a second tile."""
    c = _case(shape, cr.BWD_LOOP[shape])
    assert cr.SHAPES[shape][1] == {(2, 8, 1): "plain", (2, 24, 8): "lean"}[shape] and c.N > 4096
    _same_grads(c, _backward(c, c.half, c.dl_d, c.dv_d), _backward(c, c.up, c.dl_d, c.dv_d), f"all {c.N} rows")


# ------------------------------------------------------------------------------------------------------------------ 3. actor
@functools.lru_cache(maxsize=None)
def _tree_case(name):
    import rnad_hip
    from test_hip_bucket import TREES, _native_tree
    from test_hip_convnet_lazy import _net

    tree = _native_tree(**TREES[name])
    h = tree.handle()
    net = _net(tree.max_actions)
    half = h.observations_table(True)
    assert half.dtype == torch.float16
    return dict(tree=tree, h=h, A=tree.max_actions, S=h.S, net=net, packed=net.pack(), half=half, up=half.float(),
                stride=int(rnad_hip.lib().rnad_bucket_policy_row_stride(tree.max_actions)))


@pytest.mark.parametrize("which", ("none", "holes", "empty", "all", "odd"))
@pytest.mark.parametrize("name", NAMES)
def test_actor(name, which):
    import rnad_hip
    from _gpu import DEV
    from test_hip_convnet_lazy import _row_lists

    c = _tree_case(name)
    h, A, S, net = c["h"], c["A"], c["S"], c["net"]
    N = 2 * S
    rows = None if which == "none" else _row_lists(S)[which]
    live = None if rows is None else rnad_hip.RowList(rows, N, DEV)
    listed = torch.ones(N, dtype=torch.bool, device=DEV)
    if rows is not None:
        listed[:] = False
        listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
    outs = {}
    for key in ("half", "up"):
        logits, value = torch.full((N, A), SENTINEL, device=DEV), torch.full((N, 1), SENTINEL, device=DEV)
        pol = torch.full((N, c["stride"]), SENTINEL, device=DEV)
        rnad_hip.conv_forward_actor(h, c["packed"], *net._shape(), c[key], logits, value, pol, rows=live)
        outs[key] = (logits, value, pol)
    for what, got, want in zip(("logits", "value", "policy rows"), outs["half"], outs["up"]):
        _same(got, want, f"{name} {which} {what}")
        assert (got[~listed] == SENTINEL).all(), "rows that are not listed are left alone"
        assert not (got[listed] == SENTINEL).all() or not listed.any()
    if which in ("none", "all"):
        want_l, want_v = rnad_hip.conv_forward(c["packed"], *net._shape(), c["half"])
        _same(outs["half"][0], want_l, "the actor launch carries the bits of conv_forward")
        _same(outs["half"][1], want_v, "the actor launch carries the bits of conv_forward")


# ------------------------------------------------------------------------------------------------------------------ 4. no hidden copy
def test_no_fp32_copy_of_the_table():
    """65 547 rows at (2, 8, 1): the fp16 table is 1.05 MB, an fp32 copy of it would be 2.1 MB, the outputs are 0.8 MB.  The peak of the
    allocator over the call stays below that copy; and the C entry point, called directly with the fp16 pointer, gives the binding's bits."""
    import rnad_hip
    from _gpu import DEV

    shape = (2, 8, 1)
    c = _case(shape, cr.FWD_LOOP[shape])
    N, A = c.N, shape[0]
    assert N == 65547
    copy_bytes = N * 2 * A * A * 4
    _forward(c, c.half)  # (the first call of a kernel may allocate on the runtime's side; not torch's allocator, but be fair)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got_l, got_v = _forward(c, c.half)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"allocator peak over the call: {grew} bytes (outputs {got_l.numel() * 4 + got_v.numel() * 4}, an fp32 copy would add {copy_bytes})")
    assert grew < copy_bytes, "conv_forward made an fp32 copy of an fp16 table"
    logits, value = torch.full((N, A), SENTINEL, device=DEV), torch.full((N, 1), SENTINEL, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = rnad_hip.lib().rnad_conv_forward_obs(C.c_int64(N), None, None, *shape, ptr(c.packed), ptr(c.half), 1, ptr(logits), ptr(value),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rnad_hip.lib().rnad_last_error()
    torch.cuda.synchronize()
    _same(logits, got_l, "rnad_conv_forward_obs(obs_half = 1) against the binding")
    _same(value, got_v, "rnad_conv_forward_obs(obs_half = 1) against the binding")


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("dtype", (torch.float64, torch.bfloat16), ids=str)
def test_other_dtypes_are_refused(dtype):
    import rnad_hip
    from _gpu import DEV

    c = _tree_case("pruned")
    h, A, net = c["h"], c["A"], c["net"]
    N = 2 * c["S"]
    obs = c["up"].to(dtype)
    logits, value = torch.empty((N, A), device=DEV), torch.empty((N, 1), device=DEV)
    pol = torch.empty((N, c["stride"]), device=DEV)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_forward(c["packed"], *net._shape(), obs)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_forward_actor(h, c["packed"], *net._shape(), obs, logits, value, pol)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_backward(c["packed"], net._weights(), *net._shape(), obs, torch.zeros_like(logits), torch.zeros_like(value))


def test_a_half_table_off_its_pairs_is_refused():
    """The kernels read an fp16 table as __half2 pairs: a table that starts 2 bytes past a 4-byte boundary is refused, not read."""
    import rnad_hip
    from _gpu import DEV

    c = _tree_case("pruned")
    h, A, net = c["h"], c["A"], c["net"]
    N = 2 * c["S"]
    off = torch.zeros((c["half"].numel() + 1,), dtype=torch.float16, device=DEV)[1:].view(c["half"].shape)
    assert off.is_contiguous() and off.data_ptr() % 4 == 2
    logits, value = torch.empty((N, A), device=DEV), torch.empty((N, 1), device=DEV)
    pol = torch.empty((N, c["stride"]), device=DEV)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_forward(c["packed"], *net._shape(), off)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_forward_actor(h, c["packed"], *net._shape(), off, logits, value, pol)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_backward(c["packed"], net._weights(), *net._shape(), off, torch.zeros_like(logits), torch.zeros_like(value))


# ------------------------------------------------------------------------------------------------------------------ 6. net entry points
def _no_torch_modules(monkeypatch):
    from nn.net import ConvNet

    def tower(self, x):
        raise AssertionError("the torch modules ran: fp16 observations must take the fused kernels")

    monkeypatch.setattr(ConvNet, "_tower", tower)


def _grads_of(net, logits, value, dl, dv):
    net.zero_grad(set_to_none=True)
    torch.autograd.backward([logits, value], [dl, dv])
    out = [p.grad.detach().clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    return out


def test_forward_logits_takes_the_fused_kernels(monkeypatch):
    _no_torch_modules(monkeypatch)
    c = _case((3, 32, 1), cr.N_SWEEP)
    net = c.net
    with torch.no_grad():
        got_l, got_v = net.forward_logits(c.half)
        want_l, want_v = net.forward_logits(c.up)
    _same(got_l, want_l, "forward_logits, no grad: logits")
    _same(got_v, want_v, "forward_logits, no grad: value")
    assert not got_l.requires_grad
    # under autograd: FusedConv, whose backward reads the same fp16 tensor
    got_l, got_v = net.forward_logits(c.half)
    assert got_l.requires_grad and got_v.requires_grad
    got_g = _grads_of(net, got_l, got_v, c.dl_d, c.dv_d)
    up_l, up_v = net.forward_logits(c.up)
    want_g = _grads_of(net, up_l, up_v, c.dl_d, c.dv_d)
    _same(got_l.detach(), want_l, "forward_logits, autograd: logits")
    _same(got_v.detach(), want_v, "forward_logits, autograd: value")
    _same_grads(c, got_g, want_g, "forward_logits, autograd")


@pytest.mark.parametrize("name", NAMES)
def test_forward_batch_takes_the_half_table(name, monkeypatch):
    import rnad_hip
    from _gpu import DEV
    from environment.episode import Episodes
    from nn.net import ConvNet

    c = _tree_case(name)
    tree, h, A, net = c["tree"], c["h"], c["A"], c["net"]
    B = 8192
    ep = Episodes(tree, B, seed=17, obs_half=True)
    ep.generate(net)
    T = ep.t_eff + 1
    assert 8 * h.S <= T * B and ep.indices.dtype == torch.int32, "a batch small enough for the table route"
    _no_torch_modules(monkeypatch)

    def per_slot(self, *a, **k):
        raise AssertionError("forward_batch left the table route on an fp16 batch")

    monkeypatch.setattr(ConvNet, "forward_logits", per_slot)
    seen = []
    real = rnad_hip.conv_forward
    monkeypatch.setattr(rnad_hip, "conv_forward", lambda packed, A_, Ch, depth, obs, *a, **k: (seen.append(obs.dtype), real(packed, A_, Ch, depth, obs, *a, **k))[1])
    idx = ep.indices[:T].contiguous()
    g = torch.Generator(device="cpu").manual_seed(4)
    dl, dv = torch.randn((T * B, A), generator=g).to(DEV), torch.randn((T * B, 1), generator=g).to(DEV)
    with torch.no_grad():
        ng_l, _, _, ng_v = net.forward_batch(ep)
    got_l, _, _, got_v = net.forward_batch(ep)
    assert seen == [torch.float16, torch.float16]
    got_g = _grads_of(net, got_l.reshape(-1, A), got_v.reshape(-1, 1), dl, dv)
    want_l, want_v = rnad_hip.TabularConv.apply(c["up"], idx, h, net._shape(), net.pack(), *net._weights())
    want_g = _grads_of(net, want_l, want_v, dl, dv)
    for what, got in (("no grad", (ng_l, ng_v)), ("autograd", (got_l.detach(), got_v.detach()))):
        _same(got[0].reshape(-1, A), want_l.detach(), f"forward_batch {what}: logits")
        _same(got[1].reshape(-1, 1), want_v.detach(), f"forward_batch {what}: value")
    for (k, _), g_, w_ in zip(net.named_parameters(), got_g, want_g):
        _same(g_, w_, f"forward_batch gradient {k}")


# ------------------------------------------------------------------------------------------------------------------ 7. episodes
@pytest.mark.parametrize("name", NAMES)
def test_episodes_on_the_half_table(name):
    import rnad_hip
    from environment.episode import Episodes

    c = _tree_case(name)
    tree, net = c["tree"], c["net"]
    B = 4096
    lt, vt = rnad_hip.conv_forward(c["packed"], *net._shape(), c["up"])
    ref = Episodes(tree, B, seed=29)
    ref.generate(net, tabular=True, logits_table=lt, value_table=vt)
    ep = Episodes(tree, B, seed=29, obs_half=True)
    ep.generate(net, tabular=True)
    assert ep.t_eff == ref.t_eff
    T = ep.t_eff + 1
    for what in ("indices", "action_idx", "rewards", "policy"):
        a, b = getattr(ep, what)[:T], getattr(ref, what)[:T]
        assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                                   b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b), what
    assert ep.observations.dtype == torch.float16


# ------------------------------------------------------------------------------------------------------------------ 8. trainer
def _trainer(name, tag, half, control, monkeypatch, tmp_path, seed, **attrs):
    """A trainer on a tree object of its own.  control: obs_half stays False and the handle's fp32 table IS the up-converted fp16 table
    (set before anything else touches the handle, so obs_dedup groups the same rows)."""
    from test_hip_bucket import TREES, _native_tree
    from test_hip_convnet_lazy import BATCH, _rnad

    tree = _native_tree(**TREES[name])
    if control:
        h = tree.handle()
        h._obs_table = h.observations_table(True).float()
        assert h.observations_table(False) is h._obs_table
    torch.manual_seed(seed)
    return _rnad(tree, tag, BATCH[name], monkeypatch, tmp_path, obs_half=half, tabular_gate=0, **attrs)


def _steps(rn, n, watch=True):
    from environment.episode import Buffer

    buf, seen = Buffer(1), []
    for _ in range(n):
        rn.train_step(buf, alpha=0.5)
        rn.total_steps += 1
        if watch:
            ep = rn.last_episodes
            seen.append((ep.indices.clone(), ep.rewards.clone()))
    torch.cuda.synchronize()
    return seen


def _params(rn):
    return [(k, p.detach()) for net in (rn.net, rn.net_target) for k, p in net.named_parameters()]


@pytest.mark.parametrize("mode", ("default", "lazy", "fused"))
@pytest.mark.parametrize("name", NAMES)
def test_trainer_on_the_half_table_is_the_trainer_on_its_fp32_image(name, mode, tmp_path, monkeypatch):
    """Three eager steps with obs_half against three with the up-converted table as the fp32 table: every launch reads equal values in
    equal order, so the batches and, after the third step, net and target are bit-equal."""
    attrs = {"default": {}, "lazy": dict(lazy_rows=True), "fused": dict(fused_optimizer=True)}[mode]
    runs = {}
    for half in (True, False):
        rn = _trainer(name, f"h{int(half)}", half, not half, monkeypatch, tmp_path, 11, use_graph=False, **attrs)
        seen = _steps(rn, 3)
        assert rn.last_episodes.buckets is not None, "the bucketed per-row step"
        if mode == "lazy":
            assert getattr(rn.last_episodes, "staged_rows", None) is not None, "the lazy branch must have run"
        if mode == "fused":
            assert rn._fused_tail() is not None, "the one-launch tail must be in use"
        if half:
            assert getattr(rn.tree.handle(), "_obs_table_half", None) is not None, "the step must have read the fp16 table"
        runs[half] = (seen, _params(rn))
    for t, ((i_h, r_h), (i_f, r_f)) in enumerate(zip(runs[True][0], runs[False][0])):
        assert torch.equal(i_h, i_f), f"step {t}: indices"
        assert torch.equal(_bits(r_h), _bits(r_f)), f"step {t}: rewards"
    for (k, a), (_, b) in zip(runs[True][1], runs[False][1]):
        _same(a, b, f"{name} {mode} {k} after three steps")


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_with_the_half_table(name, tmp_path, monkeypatch):
    finals = {}
    for use_graph in (True, False):
        rn = _trainer(name, f"g{int(use_graph)}", True, False, monkeypatch, tmp_path, 7, use_graph=use_graph)
        _steps(rn, 5, watch=False)
        if use_graph:
            assert rn._graph["graph"] is not None and not rn._graph["failed"], "the obs_half step must have been captured and replayed"
        finals[use_graph] = _params(rn)
    for (k, a), (_, b) in zip(finals[True], finals[False]):
        _same(a, b, f"{name} {k}: replayed against eager")
