"""Lazy rows for the ConvNet family: the staged actor launch (rnad_conv_forward_actor, csrc/conv_tower.hip) and RNaD's lazy-rows step on it.

The actor launch is the forward kernel with one more epilogue, so logits and values are compared bit for bit with rnad_conv_forward, the
policy rows bit for bit with the pi columns rnad_bucket_records makes from those logits, and a batch played from staged rows with the batch
played from a records table.  The trainer's first lazy step differs from the all-rows step only in which rows the backward sums over, i.e.
in fp32 summation order: the gradient gate of tests/test_hip_convnet.py (rtol 1e-3, atol 2e-5 * max|g|); every such comparison goes
through np.testing.assert_allclose, so tests/conftest.py records the achieved errors."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("pruned", "a5c4")
BATCH = {"pruned": 4096, "a5c4": 4096}  # lanes of the trainer tests: a batch that leaves rows of the tree unvisited
SENTINEL = 7.0


def _gate(got, want, what=""):
    want = np.asarray(want)
    np.testing.assert_allclose(np.asarray(got), want, rtol=1e-3, atol=2e-5 * np.abs(want).max(), err_msg=what)


def _net(A, seed=5):
    from _gpu import DEV
    from nn.net import ConvNet

    torch.manual_seed(seed)
    net = ConvNet(A, 16, depth=2, batch_norm=False, device=DEV)
    assert net._fusable() and net.lazy_rows_ready()
    return net


@functools.lru_cache(maxsize=None)
def _case(name):
    """Tree, net and the all-rows reference of one tree, computed once: conv_forward on all 2S rows and the records made from it."""
    import rnad_hip
    from test_hip_bucket import TREES, _native_tree

    tree = _native_tree(**TREES[name])
    h = tree.handle()
    A = tree.max_actions
    net = _net(A)
    packed, table = net.pack(), h.observations_table()
    full_l, full_v = rnad_hip.conv_forward(packed, *net._shape(), table)
    hp = rnad_hip.make_learn_params(alpha=0.3, eta=0.2)
    rec, _ = rnad_hip.bucket_records(h, full_l, full_v, full_v, full_l, full_l, hp, fast=True)
    return dict(tree=tree, h=h, A=A, S=h.S, net=net, packed=packed, table=table, full_l=full_l, full_v=full_v, rec=rec,
                stride=int(rnad_hip.lib().rnad_bucket_policy_row_stride(A)))


def _row_lists(S):
    N = 2 * S
    holes = np.array([r for r in range(N) if r in (0, S) or (r % 3 != 1 and not (40 <= r < 75))], np.int32)
    odd = np.arange(3, 3 + 16 * 5 + 7, dtype=np.int32)  # 87 rows: not a multiple of a 16-sample tile
    assert len(odd) % 16 != 0 and odd[-1] < N and 0 in holes and S in holes and len(holes) < N
    return {"holes": holes, "empty": np.zeros((0,), np.int32), "all": np.arange(N, dtype=np.int32), "odd": odd}


@pytest.mark.parametrize("which", ("holes", "empty", "all", "odd"))
@pytest.mark.parametrize("name", NAMES)
def test_actor_launch_is_the_forward_plus_the_policy_rows(name, which):
    import rnad_hip
    from _gpu import DEV

    c = _case(name)
    h, A, S, net = c["h"], c["A"], c["S"], c["net"]
    N = 2 * S
    rows = _row_lists(S)[which]
    live = rnad_hip.RowList(rows, N, DEV)
    logits = torch.full((N, A), SENTINEL, device=DEV)
    value = torch.full((N, 1), SENTINEL, device=DEV)
    pol = torch.full((N, c["stride"]), SENTINEL, device=DEV)
    rnad_hip.conv_forward_actor(h, c["packed"], *net._shape(), c["table"], logits, value, pol, rows=live)
    want_l, want_v = rnad_hip.conv_forward(c["packed"], *net._shape(), c["table"], live=live)
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
    assert int(listed.sum()) == len(rows)
    assert torch.equal(logits[listed], want_l[listed]) and torch.equal(value[listed], want_v[listed])
    # the pi columns of the records made from those logits: the same function, the same bits
    hp = rnad_hip.make_learn_params(alpha=0.3, eta=0.2)
    rec = rnad_hip.bucket_records(h, want_l, want_v, want_v, want_l, want_l, hp)
    col = rnad_hip.policy_column(A)
    assert torch.equal(pol[listed][:, :A].contiguous().view(torch.int32), rec[listed][:, col:col + A].contiguous().view(torch.int32))
    assert (pol[listed][:, A:] == 0).all(), "pad columns are zeros"
    for out in (logits, value, pol):
        assert (out[~listed] == SENTINEL).all(), "rows that are not listed are left alone"
    if which == "all":  # rows = None is the list of all rows
        l2, v2, p2 = torch.empty_like(logits), torch.empty_like(value), torch.empty_like(pol)
        rnad_hip.conv_forward_actor(h, c["packed"], *net._shape(), c["table"], l2, v2, p2)
        assert torch.equal(l2, logits) and torch.equal(v2, value) and torch.equal(p2.view(torch.int32), pol.view(torch.int32))
        assert torch.equal(l2, c["full_l"]) and torch.equal(v2, c["full_v"])


def test_misaligned_policy_rows_are_refused():
    import rnad_hip
    from _gpu import DEV

    c = _case("pruned")
    N, A, net = 2 * c["S"], c["A"], c["net"]
    logits, value = torch.empty((N, A), device=DEV), torch.empty((N, 1), device=DEV)
    off = torch.empty((N * c["stride"] + 1,), device=DEV)[1:].view(N, c["stride"])  # contiguous, 4 bytes past a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_forward_actor(c["h"], c["packed"], *net._shape(), c["table"], logits, value, off)


def test_backward_of_the_a5_net_matches_fp64_autograd():
    """A = 5, channels = 16, depth = 2: the saved activations of rnad_conv_backward do not fit the LDS, so it recomputes relu(conv0) and
    relu(conv1) of a block when the walk back reaches it (the LEAN instantiation).  Against fp64 autograd of the same torch modules, all
    rows of a sample and a row list, at the gradient gate of tests/test_hip_convnet.py."""
    import copy

    import rnad_hip
    from _gpu import DEV, cpu

    c = _case("a5c4")
    net, A = c["net"], c["A"]
    N = 200
    obs = c["table"][:N].contiguous()
    g = torch.Generator(device="cpu").manual_seed(9)
    dl, dv = torch.randn(N, A, generator=g), torch.randn(N, 1, generator=g)
    ref = copy.deepcopy(net).double().cpu()
    for rows in (None, np.array([r for r in range(N) if r % 5 != 2], np.int32)):
        ref.zero_grad()
        sel = torch.arange(N) if rows is None else torch.as_tensor(rows, dtype=torch.long)
        l64, v64 = ref.forward_logits(obs.cpu().double()[sel])
        torch.autograd.backward([l64, v64], [dl.double()[sel], dv.double()[sel]])
        got = rnad_hip.conv_backward(c["packed"], net._weights(), *net._shape(), obs, dl.to(DEV), dv.to(DEV),
                                     live=None if rows is None else rnad_hip.RowList(rows, N, DEV))
        again = rnad_hip.conv_backward(c["packed"], net._weights(), *net._shape(), obs, dl.to(DEV), dv.to(DEV),
                                       live=None if rows is None else rnad_hip.RowList(rows, N, DEV))
        for (k, p_), g_, h_ in zip(ref.named_parameters(), got, again):
            _gate(cpu(g_), p_.grad.numpy(), f"{k} rows={'all' if rows is None else len(rows)}")
            assert torch.equal(g_, h_), "two backward calls on the same inputs must give identical bits"


@pytest.mark.parametrize("levels", ("1", "2"))
@pytest.mark.parametrize("name", NAMES)
def test_staged_convnet_actor_plays_the_same_batch(name, levels, monkeypatch):
    """The net's own closure behind NaN-filled tables against the batch played from the records of the all-rows forward: the same
    episodes, and every visited row was staged -- logits, value and policy row."""
    import rnad_hip
    from _gpu import DEV
    from environment.episode import Episodes

    c = _case(name)
    tree, h, A, S, net = c["tree"], c["h"], c["A"], c["S"], c["net"]
    B = 4096
    kw = dict(tabular=True, bucketed=True, trim=False, store_values=False, compact=True)
    full = Episodes(tree, B, seed=23, lane_offset=5)
    vis_full = torch.empty((2 * S,), dtype=torch.int32, device=DEV)
    full.generate(net, policy_table=(c["rec"], rnad_hip.policy_column(A)), visited=vis_full, **kw)

    monkeypatch.setenv("RNAD_STAGE_LEVELS", levels)
    nan = float("nan")
    logit = torch.full((2 * S, A), nan, device=DEV)  # a row that was not evaluated would poison the rollout
    v = torch.full((2 * S, 1), nan, device=DEV)
    logit._policy_rows = torch.full((2 * S, c["stride"]), nan, device=DEV)
    actor = net.staged_actor(h, c["packed"], c["table"], logit, v, logit._policy_rows)
    ep = Episodes(tree, B, seed=23, lane_offset=5)
    vis = torch.empty((2 * S,), dtype=torch.int32, device=DEV)
    ep.generate(net, logits_table=logit, visited=vis, staged_actor=actor, **kw)
    assert len(ep.staged_rows) == (3 if levels == "2" else 2)
    assert torch.equal(ep.indices, full.indices) and torch.equal(ep.lane_ids, full.lane_ids)
    assert torch.equal(ep._compact[0].acts, full._compact[0].acts) and torch.equal(ep._compact[0].final_reward, full._compact[0].final_reward)
    ep._compact = (ep._compact[0], c["rec"])  # (the dense views expand from a records table: a staged batch gets it attached afterwards)
    assert torch.equal(ep.action_idx, full.action_idx) and torch.equal(ep.rewards, full.rewards)
    assert torch.equal(vis, vis_full)
    seen = vis.bool()
    assert seen[0] and seen[S], "the rows of the absorbing state come with the upper rows"
    for what, t in (("logit", logit), ("v", v), ("policy_rows", logit._policy_rows)):
        assert not torch.isnan(t[seen]).any(), f"{what}: every visited row must have been staged"
    assert torch.equal(logit[seen], c["full_l"][seen]) and torch.equal(v[seen], c["full_v"][seen])


def _rnad(tree, name, B, monkeypatch, tmp_path, net_params=None, **attrs):
    from _gpu import DEV
    from learn.rnad import RNaD

    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    A = tree.max_actions
    rn = RNaD(tree=tree, device=DEV, directory_name=name, batch_size=B, eta=0.2, b1_adam=0.0, lr=1e-3,
              net_params=net_params or {"type": "ConvNet", "max_actions": A, "channels": 16, "depth": 2, "batch_norm": False})
    rn.initialize()
    for k, val in attrs.items():
        setattr(rn, k, val)
    return rn


@pytest.mark.parametrize("name", NAMES)
def test_first_lazy_step_is_the_all_rows_step(name, tmp_path, monkeypatch):
    """Two trainers from the same seed and weights, one step each: the lazy one stages the actor, evaluates the target and back-propagates
    on the visited rows only, and arrives at the batch, the records (on those rows) and -- up to fp32 summation order -- the gradients of
    the step on all rows."""
    import rnad_hip
    from environment.episode import Buffer
    from test_hip_bucket import TREES, _native_tree

    tree = _native_tree(**TREES[name])
    S, B = tree.handle().S, BATCH[name]
    out = {}
    for lazy in (True, False):
        torch.manual_seed(11)
        rn = _rnad(tree, f"l{lazy}", B, monkeypatch, tmp_path, lazy_rows=lazy, tabular_gate=0, use_graph=False)
        with torch.no_grad():
            for p in rn.net_reg_.parameters():
                p.mul_(1.01)
        seen = {}

        def spy(real, seen=seen):
            def wrapped(*a, **k):
                tables = real(*a, **k)
                seen["tables"] = tables
                return tables
            return wrapped

        rn._table_outputs, rn._value_tables = spy(rn._table_outputs), spy(rn._value_tables)
        captured, real = {}, rn.optimizer.step
        rn.optimizer.step = lambda: (captured.update(g=[p.grad.detach().clone() for p in rn.net.parameters()]), real())[1]
        rn.train_step(Buffer(1), alpha=0.4)
        ep = rn.last_episodes
        assert ep.buckets is not None, "the bucketed per-row step"
        rnad_hip.complete_records(seen["tables"]["records"])
        out[lazy] = dict(g=captured["g"], indices=ep.indices.clone(), rewards=ep.rewards.clone(), records=seen["tables"]["records"],
                         fast=seen["tables"]["fast_records"], staged=getattr(ep, "staged_rows", None), rows=rn.last_rows)
    lz, al = out[True], out[False]
    # the lazy branch really ran, on a batch that leaves rows out
    assert lz["staged"] is not None and al["staged"] is None and al["rows"] is None
    n = int(lz["rows"].count.item())
    print(f"{name}: B={B} 2S={2 * S} visited rows={n} staged={[int(r.count.item()) for r in lz['staged']]}")
    assert 0 < n < 2 * S
    assert torch.equal(lz["indices"], al["indices"]) and torch.equal(lz["rewards"], al["rewards"])
    listed = lz["rows"].rows[:n].long()
    for key in ("records", "fast"):
        assert torch.equal(lz[key][listed].view(torch.int32), al[key][listed].view(torch.int32)), key
    for (k, _), a, b in zip(rn.net.named_parameters(), al["g"], lz["g"]):
        _gate(b.cpu().numpy(), a.cpu().numpy(), k)


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_ends_where_eager_steps_end(name, tmp_path, monkeypatch):
    from environment.episode import Buffer
    from test_hip_bucket import TREES, _native_tree

    tree = _native_tree(**TREES[name])
    finals = {}
    for use_graph in (True, False):
        torch.manual_seed(7)
        rn = _rnad(tree, f"g{use_graph}", BATCH[name], monkeypatch, tmp_path, lazy_rows=True, tabular_gate=0, use_graph=use_graph)
        buf = Buffer(1)
        for _ in range(5):
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1
        torch.cuda.synchronize()
        assert getattr(rn.last_episodes, "staged_rows", None) is not None, "the lazy branch must have run"
        if use_graph:
            assert rn._graph["graph"] is not None and not rn._graph["failed"], "the lazy step must have been captured and replayed"
        finals[use_graph] = [p.detach().clone() for p in list(rn.net.parameters()) + list(rn.net_target.parameters())]
    for a, b in zip(finals[True], finals[False]):
        assert torch.equal(a, b)


def test_gates(tmp_path, monkeypatch):
    from environment.episode import Buffer
    from test_hip_bucket import TREES, _native_tree

    tree = _native_tree(**TREES["a5c4"])
    h, A = tree.handle(), tree.max_actions
    B, T_cap = (4096 if 2 * h.S > 4096 else 1024), 2 * h.max_depth
    assert 2 * h.S > B, "a tree with more rows than the batch has lanes"
    buf = Buffer(1)
    conv = _rnad(tree, "conv", B, monkeypatch, tmp_path, tabular_gate=0)
    assert conv.lazy_rows is None and conv._tabular_mode(T_cap, B) is True
    assert conv._use_lazy_rows(h, B, T_cap, None, buf) is False, "a ConvNet's lazy rows are opt-in"
    assert conv._row_extras() is False
    conv.lazy_rows = True
    assert conv._use_lazy_rows(h, B, T_cap, None, buf) is True
    assert conv._use_lazy_rows(h, B, T_cap, {}, buf) is False, "a logged step falls back to all rows"
    bn = _rnad(tree, "bn", B, monkeypatch, tmp_path, lazy_rows=True, tabular_gate=0,
               net_params={"type": "ConvNet", "max_actions": A, "channels": 16, "depth": 2, "batch_norm": True})
    assert bn._tabular_mode(T_cap, B) is False
    mlp = _rnad(tree, "mlp", B, monkeypatch, tmp_path, tabular_gate=0, net_params={"type": "MLP", "max_actions": A, "width": 64})
    assert mlp.lazy_rows is None and mlp._use_lazy_rows(h, B, T_cap, None, buf) is True, "the MLP's automatic rule: 2S > lanes"
    assert mlp._use_lazy_rows(h, B, T_cap, {}, buf) is False
    mlp.lazy_rows = False
    assert mlp._use_lazy_rows(h, B, T_cap, None, buf) is False
    big_B = 1 << (2 * h.S).bit_length()  # at least as many lanes as rows: the automatic rule says no
    big = _rnad(tree, "mlpbig", big_B, monkeypatch, tmp_path, tabular_gate=0, net_params={"type": "MLP", "max_actions": A, "width": 64})
    assert big._use_lazy_rows(h, big_B, T_cap, None, buf) is False
