"""The fused ConvNet (csrc/conv_tower.hip) on the GPU against the reference's recorded nets (tests/golden/convnet_*.npz): forward,
row lists, backward against fp64 autograd gradients, reproducibility, the torch fallback, forward_batch's table route, RNaD's per-row step,
NashConv, the training curve and checkpoints.

Tolerances: forward 1e-5 absolute (the project's fp32 bound, README.md); gradients rtol 1e-3, atol 2e-5 * max|g| (the project's gradient
gate).  Every comparison goes through np.testing.assert_allclose, so tests/conftest.py records the achieved errors of a run;
profiles/convnet_parity_errors.json is a copy of that record from a run of this file on an MI355X."""
import numpy as np
import pytest
import torch

from _util import load

pytestmark = pytest.mark.gpu

SHAPES = ("small", "a5", "c1")
FWD_ATOL = 1e-5


def _gate(got, want, what=""):
    want = np.asarray(want)
    np.testing.assert_allclose(np.asarray(got), want, rtol=1e-3, atol=2e-5 * np.abs(want).max(), err_msg=what)


def _fixture(name):
    return load("convnet_" + name)


def _net(fx, prefix="", batch_norm=False, channels=None):
    from _gpu import DEV
    from nn.net import ConvNet

    net = ConvNet(int(fx["max_actions"]), int(fx["channels"]) if channels is None else channels, depth=int(fx["depth"]), batch_norm=batch_norm,
                  device=DEV)
    if channels is None:
        sd = {str(k): torch.as_tensor(fx[prefix + "w_" + str(k).replace(".", "_")]) for k in fx[prefix + "keys"]}
        net.load_state_dict(sd, strict=True)
    return net


def _flat_grads(fx, net):
    return [fx["g_" + k.replace(".", "_")] for k, _ in net.named_parameters()]


@pytest.mark.parametrize("name", SHAPES)
def test_forward_matches_the_reference(name):
    from _gpu import cpu, gpu

    fx = _fixture(name)
    net = _net(fx)
    assert net._fusable(), "the shapes of the fixtures must take the tower kernels"
    obs = gpu(fx["obs"])
    packed = net.pack()
    for N in (1, 33, obs.shape[0]):
        with torch.no_grad():
            logits, value = net.forward_logits(obs[:N], packed=packed)
        np.testing.assert_allclose(cpu(logits), fx["logits"][:N], rtol=0, atol=FWD_ATOL, err_msg=f"logits N={N}")
        np.testing.assert_allclose(cpu(value), fx["value"][:N], rtol=0, atol=FWD_ATOL, err_msg=f"value N={N}")
        with torch.no_grad():
            only_l, none_v = net.forward_logits(obs[:N], want_value=False, packed=packed)
            none_l, only_v = net.forward_logits(obs[:N], want_logits=False, packed=packed)
        assert none_v is None and none_l is None and torch.equal(only_l, logits) and torch.equal(only_v, value)
    np.testing.assert_allclose(cpu(net.forward_policy(obs)), fx["policy"], rtol=0, atol=FWD_ATOL)


@pytest.mark.parametrize("name", ("small", "a5"))
def test_row_list_outputs_are_those_of_the_full_launch(name):
    import rnad_hip
    from _gpu import DEV, gpu

    fx = _fixture(name)
    net = _net(fx)
    obs = gpu(fx["obs"])
    N = obs.shape[0]
    packed = net.pack()
    with torch.no_grad():
        full_l, full_v = net.forward_logits(obs, packed=packed)
    holes = np.array([r for r in range(N) if r % 3 != 1 and not (40 <= r < 75)], np.int32)
    for rows in (holes, np.zeros((0,), np.int32), np.arange(N, dtype=np.int32)):
        live = rnad_hip.RowList(rows, N, DEV)
        with torch.no_grad():
            l, v = net.forward_logits(obs, packed=packed, live=live)
        listed = torch.zeros(N, dtype=torch.bool, device=DEV)
        listed[torch.as_tensor(rows, dtype=torch.long, device=DEV)] = True
        assert torch.equal(l[listed], full_l[listed]) and torch.equal(v[listed], full_v[listed])
        assert (l[~listed] == 0).all() and (v[~listed] == 0).all(), "rows that are not listed come back as zeros"
        # out= / zero_rest=False: rows that are not listed are left alone
        out_l, out_v = torch.full((N, net.max_actions), 7.0, device=DEV), torch.full((N, 1), 7.0, device=DEV)
        rnad_hip.conv_forward(packed, *net._shape(), obs, live=live, out=(out_l, out_v))
        assert torch.equal(out_l[listed], full_l[listed]) and (out_l[~listed] == 7.0).all() and (out_v[~listed] == 7.0).all()


@pytest.mark.parametrize("name", SHAPES)
def test_backward_matches_the_fp64_gradients(name):
    import rnad_hip
    from _gpu import DEV, cpu, gpu

    fx = _fixture(name)
    net = _net(fx)
    obs, dl, dv = gpu(fx["obs"]), gpu(fx["dlogits"]), gpu(fx["dv"])
    N = obs.shape[0]
    logits, value = net.forward_logits(obs)  # under autograd: rnad_conv_backward is the node's backward
    torch.autograd.backward([logits, value], [dl, dv])
    for (k, p), want in zip(net.named_parameters(), _flat_grads(fx, net)):
        _gate(cpu(p.grad), want, f"{k} N={N}")
    # one row, and a row list: against fp64 autograd of the same torch modules on those rows
    import copy

    ref = copy.deepcopy(net).double().cpu()
    for rows in (np.array([0], np.int32), np.array([r for r in range(N) if r % 5 != 2], np.int32)):
        ref.zero_grad()
        sel = torch.as_tensor(rows, dtype=torch.long)
        l64, v64 = ref.forward_logits(torch.as_tensor(fx["obs"]).double()[sel])
        torch.autograd.backward([l64, v64], [torch.as_tensor(fx["dlogits"]).double()[sel], torch.as_tensor(fx["dv"]).double()[sel]])
        if len(rows) == 1:
            got = rnad_hip.conv_backward(net.pack(), net._weights(), *net._shape(), obs[:1].contiguous(), dl[:1].contiguous(), dv[:1].contiguous())
        else:
            got = rnad_hip.conv_backward(net.pack(), net._weights(), *net._shape(), obs, dl, dv, live=rnad_hip.RowList(rows, N, DEV))
        for (k, p), g in zip(ref.named_parameters(), got):
            _gate(cpu(g), p.grad.numpy(), f"{k} rows={len(rows)}")


def test_backward_is_reproducible_and_pack_follows_the_weights():
    import rnad_hip
    from _gpu import gpu

    fx = _fixture("small")
    net = _net(fx)
    obs, dl, dv = gpu(fx["obs"]), gpu(fx["dlogits"]), gpu(fx["dv"])
    packed = net.pack()
    a = rnad_hip.conv_backward(packed, net._weights(), *net._shape(), obs, dl, dv)
    b = rnad_hip.conv_backward(packed, net._weights(), *net._shape(), obs, dl, dv)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two backward calls on the same inputs must give identical bits"
    with torch.no_grad():
        before, _ = net.forward_logits(obs, packed=packed)
        net.tower[1].conv0.col_conv.weight.mul_(1.5)
        stale, _ = net.forward_logits(obs, packed=packed)
        after, _ = net.forward_logits(obs, packed=net.pack())
    assert torch.equal(stale, before) and not torch.equal(after, before)


def test_unsupported_shapes_and_batch_norm_take_the_torch_modules(tmp_path, monkeypatch):
    import rnad_hip
    from _gpu import DEV, cpu, gpu, golden_tree
    from learn.rnad import RNaD

    fx = _fixture("small")
    assert not rnad_hip.conv_supported(3, 12, 2)
    obs = gpu(fx["obs"])
    odd = _net(fx, channels=12)
    assert not odd._fusable() and odd.pack() is None
    import copy

    host = copy.deepcopy(odd).cpu()  # the same torch modules, evaluated by the CPU
    with torch.no_grad():
        logits, value = odd.forward_logits(obs)
        want_l, want_v = host.forward_logits(torch.as_tensor(fx["obs"]))
    np.testing.assert_allclose(cpu(logits), want_l.numpy(), rtol=0, atol=FWD_ATOL)
    np.testing.assert_allclose(cpu(value), want_v.numpy(), rtol=0, atol=FWD_ATOL)
    bn = _net(fx, "bn_", True).eval()
    assert not bn._fusable()
    with torch.no_grad():
        logits, value = bn.forward_logits(obs)
    np.testing.assert_allclose(cpu(logits), fx["bn_logits"], rtol=0, atol=FWD_ATOL)
    np.testing.assert_allclose(cpu(value), fx["bn_value"], rtol=0, atol=FWD_ATOL)
    np.testing.assert_allclose(cpu(bn.forward_policy(obs)), fx["bn_policy"], rtol=0, atol=FWD_ATOL)
    # a BatchNorm net never takes the per-row table step
    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    tree, _ = golden_tree("small")
    rn = RNaD(tree=tree, device=DEV, directory_name="bn", batch_size=512, eta=0.2,
              net_params={"type": "ConvNet", "max_actions": 3, "channels": 16, "depth": 2, "batch_norm": True})
    rn.initialize()
    rn.tabular_gate = 0
    assert rn._tabular_mode(8, 512) is False


def _episodes_on_recorded_states(tree, indices):
    """An Episodes object over the reference's recorded states (onpolicy_*.npz keeps the trajectory's states, not its observations:
    those are a function of the state and the player to move, and K1 makes them here)."""
    import rnad_hip
    from _gpu import DEV, gpu
    from environment.episode import Episodes

    T, B = indices.shape
    ep = Episodes(tree, B, seed=0)
    ep.t_eff, ep.finished = T - 1, True
    ep.indices = gpu(indices, torch.int32)
    obs, bits = [], []
    for t in range(T):
        mb = torch.empty((B,), dtype=torch.uint8, device=DEV)
        obs.append(rnad_hip.observe(tree.handle(), ep.indices[t].contiguous(), t & 1, mask_bits=mb))
        bits.append(mb)
    ep.observations, ep.mask_bits = torch.stack(obs), torch.stack(bits)
    return ep


def test_forward_batch_table_route_is_the_per_slot_route():
    from _gpu import cpu, golden_tree

    fx = _fixture("small")
    tree, _ = golden_tree("small")
    ep = _episodes_on_recorded_states(tree, load("onpolicy_small")["indices"])
    ep.tree = tree
    T, B, A = ep.t_eff + 1, ep.batch_size, 3
    assert 8 * tree.handle().S <= T * B, "the fixture must take the table route"
    net_a, net_b = _net(fx), _net(fx)
    with torch.no_grad():
        table_out = net_a.forward_batch(ep)
        slot_l, slot_v = net_b.forward_logits(ep.observations[:T].reshape(-1, 2, A, A))
    assert torch.equal(table_out[0].reshape(-1, A), slot_l) and torch.equal(table_out[3].reshape(-1, 1), slot_v)
    g = torch.Generator(device="cpu").manual_seed(5)
    dl = torch.randn(T * B, A, generator=g).to(slot_l.device)
    dv = torch.randn(T * B, 1, generator=g).to(slot_l.device)
    valid = (ep.indices[:T] != 0).reshape(-1, 1).float()  # absorbed slots carry no gradient for any consumer; the row sums skip them
    dl, dv = dl * valid, dv * valid
    out = net_a.forward_batch(ep)
    torch.autograd.backward([out[0].reshape(-1, A), out[3].reshape(-1, 1)], [dl, dv])
    l, v = net_b.forward_logits(ep.observations[:T].reshape(-1, 2, A, A))
    torch.autograd.backward([l, v], [dl, dv])
    for (k, p), q in zip(net_a.named_parameters(), net_b.parameters()):
        _gate(cpu(p.grad), cpu(q.grad), k)


def _rnad(tree, name, B, monkeypatch, tmp_path, **kw):
    from _gpu import DEV
    from learn.rnad import RNaD

    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    return RNaD(tree=tree, device=DEV, directory_name=name, batch_size=B, eta=0.2, b1_adam=0.0, lr=1e-3,
                net_params={"type": "ConvNet", "max_actions": 3, "channels": 16, "depth": 2, "batch_norm": False}, **kw)


def test_train_step_modes_agree(tmp_path, monkeypatch):
    """One update on the `small` tree from the same weights and seed: dense and "forward" give identical gradients, the default per-row
    step gives them up to fp32 summation order -- and really is the bucketed per-row step."""
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    grads = {}
    for mode in (False, "forward", True):
        torch.manual_seed(11)
        rn = _rnad(tree, f"m{mode}", 512, monkeypatch, tmp_path)
        rn.initialize()
        rn.tabular, rn.tabular_gate = mode, 0
        with torch.no_grad():
            for p in rn.net_reg_.parameters():
                p.mul_(1.01)
        captured = {}
        real = rn.optimizer.step
        rn.optimizer.step = lambda: (captured.update(g=[p.grad.detach().clone() for p in rn.net.parameters()]), real())[1]
        assert rn._tabular_mode(2 * tree.handle().max_depth, 512) == mode
        rn.train_step(Buffer(1), alpha=0.4)
        grads[mode] = captured["g"]
        assert (rn.last_episodes.buckets is not None) == (mode is True), "mode True must be the bucketed per-row step"
    for a, b in zip(grads[False], grads["forward"]):
        assert torch.equal(a, b)
    for a, b in zip(grads[False], grads[True]):
        _gate(b.cpu().numpy(), a.cpu().numpy())


def test_distinct_observation_step_gives_the_all_rows_gradients(tmp_path, monkeypatch):
    """A tree whose rows share observations (the depth-4 ternary tree of tests/test_hip_dedup.py): the default step evaluates the nets on
    one representative per distinct observation, copies the records to the groups and back-propagates the groups' summed gradients on
    the representatives -- the gradients of the step on all rows (dedup_rows=False) up to fp32 summation order."""
    from _gpu import DEV
    from environment.episode import Buffer
    from learn.rnad import RNaD
    from test_hip_bucket import _native_tree

    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    tree = _native_tree(A=3, C=1, depth=4, seed=0)
    d = tree.handle().obs_dedup(False)
    assert 5 * d.n_unique <= 4 * d.n_rows, "the tree must be one on which distinct observations pay"
    grads, used = {}, {}
    for dedup in (False, True):
        torch.manual_seed(11)
        rn = RNaD(tree=tree, device=DEV, directory_name=f"d{dedup}", batch_size=1 << 14, eta=0.2, b1_adam=0.0, lr=1e-3,
                  net_params={"type": "ConvNet", "max_actions": 3, "channels": 16, "depth": 2, "batch_norm": False})
        rn.initialize()
        rn.dedup_rows, rn.use_graph = dedup, False
        with torch.no_grad():
            for p in rn.net_reg_.parameters():
                p.mul_(1.01)
        seen, real_tables = {}, rn._table_outputs

        def spy(*a, real=real_tables, seen=seen, **k):
            tables = real(*a, **k)
            seen["dedup"] = tables.get("dedup") is not None
            return tables

        rn._table_outputs = spy
        captured, real = {}, rn.optimizer.step
        rn.optimizer.step = lambda: (captured.update(g=[p.grad.detach().clone() for p in rn.net.parameters()]), real())[1]
        rn.train_step(Buffer(1), alpha=0.4)
        assert rn.last_episodes.buckets is not None, "the bucketed per-row step"
        grads[dedup], used[dedup] = captured["g"], seen["dedup"]
    assert used == {False: False, True: True}, "the distinct-observation branch must really have run"
    for a, b in zip(grads[False], grads[True]):
        _gate(b.cpu().numpy(), a.cpu().numpy())


def test_nashconv_of_the_reference_net():
    from _gpu import golden_tree
    from util.metric import NashConvData

    fx = _fixture("small")
    tree, _ = golden_tree("small")
    net = _net(fx)
    data = NashConvData(tree)
    data.get_nashconv_from_net(tree, net)
    np.testing.assert_allclose((data.row_best[1] + data.col_best[1]).item(), float(fx["nashconv"]), rtol=0, atol=1e-5)


def test_nashconv_curve_matches_reference_band(tmp_path, monkeypatch):
    """As tests/test_hip_curve.py, for the ConvNet in the default mode against the reference's ConvNet curves."""
    from _gpu import golden_tree

    ref = load("curve_convnet_small")
    curves = ref["nashconv"]
    M, delta, B = int(ref["M"]), int(ref["delta_m"]), int(ref["batch"])
    lo, hi = curves.min(0), curves.max(0)
    tree, _ = golden_tree("small")
    torch.manual_seed(2000)
    rn = _rnad(tree, "curve", B, monkeypatch, tmp_path, bounds=[M], delta_m=[delta], gamma_averaging=float(ref["gamma_averaging"]), logit_clip=2)
    rn.initialize()
    assert rn._tabular_mode(2 * tree.handle().max_depth, B) is True, "the default mode must be the per-row step"
    nc0 = rn._evaluate_nashconv()
    rn._RNaD__resume(checkpoint_mod=10**9, expl_mod=1, log_mod=10**9)
    nc = np.array([nc0] + [v for _, _, v in rn.nashconv_history] + [rn._evaluate_nashconv()])
    assert len(nc) == M + 1
    print("reference band lo", np.round(lo, 3), "\nreference band hi", np.round(hi, 3), "\nthis build        ", np.round(nc, 3))
    tol = 0.15
    assert (nc >= lo - tol).all() and (nc <= hi + tol).all(), (nc, lo, hi)
    assert nc[-1] <= nc[0] - 0.30


def test_graph_replay_ends_where_eager_steps_end(tmp_path, monkeypatch):
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    finals = {}
    for use_graph in (True, False):
        torch.manual_seed(7)
        rn = _rnad(tree, f"g{use_graph}", 512, monkeypatch, tmp_path)
        rn.initialize()
        rn.use_graph = use_graph
        buf = Buffer(1)
        for _ in range(7):
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1
        torch.cuda.synchronize()
        if use_graph:
            assert rn._graph.get("graph") is not None, "the step must have been captured and replayed"
        finals[use_graph] = [p.detach().clone() for p in list(rn.net.parameters()) + list(rn.net_target.parameters())]
    for a, b in zip(finals[True], finals[False]):
        assert torch.equal(a, b)


def test_checkpoint_round_trip(tmp_path, monkeypatch):
    """`run` for one update (checkpoints before every step), then a fresh RNaD on the same directory resumes the last checkpoint:
    net_params and the four state dicts are those of the moment it was written."""
    from _gpu import golden_tree

    fx = _fixture("small")
    tree, _ = golden_tree("small")
    torch.manual_seed(3)
    rn = _rnad(tree, "ckpt", 512, monkeypatch, tmp_path, bounds=[1], delta_m=[2])
    written = []
    step = rn.train_step

    def spy(buffer, alpha, log=None):  # __resume saves right before each step
        written.append((rn.m, rn.n, {name: {k: v.detach().clone() for k, v in getattr(rn, name).state_dict().items()}
                                     for name in ("net", "net_target", "net_reg", "net_reg_")}))
        step(buffer, alpha, log=log)

    rn.train_step = spy
    rn.run(max_updates=1, checkpoint_mod=1, expl_mod=10**9, log_mod=10**9)
    assert [(m, n) for m, n, _ in written] == [(0, 0), (0, 1)]
    again = _rnad(tree, "ckpt", 512, monkeypatch, tmp_path, bounds=[1], delta_m=[2])
    again.initialize()
    assert (again.m, again.n) == (0, 1) and again.total_steps == 1
    assert again.net_params == rn.net_params and again.net_params["type"] == "ConvNet"
    assert type(again.net).__name__ == "ConvNet" and again.net._fusable()
    for name, want in written[-1][2].items():
        got = getattr(again, name).state_dict()
        assert list(got.keys()) == list(want.keys())
        for k in want:
            assert torch.equal(got[k], want[k]), (name, k)
    assert any(not torch.equal(a, b) for a, b in zip(written[0][2]["net"].values(), written[1][2]["net"].values())), "the step must have trained"
    sd = {str(k): torch.as_tensor(fx["w_" + str(k).replace(".", "_")]) for k in fx["keys"]}
    again.net.load_state_dict(sd, strict=True)
