"""rnad_conv_optimizer_step on the GPU: the bits of rnad_optimizer_step on the same bucket and state, the two packed images kept equal
to a fresh rnad_conv_pack of the updated tensors, and the tail inside RNaD (opt-in for a ConvNet: RNaD.fused_optimizer = True).

Gates: the kernels share their arithmetic, so tensors-as-72-views against one flat tensor is compared bit for bit; against torch's
clip_grad_norm_ / fused Adam / _foreach EMA the gate is the one tests/test_hip_graph.py::test_fused_optimizer_tail_is_clip_adam_ema
already holds this arithmetic to (rtol 2e-5, atol 1e-8)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (A, channels, depth): see tests/test_conv_tail.py
SHAPES = [(1, 16, 1), (2, 8, 1), (3, 16, 2), (5, 16, 2), (8, 2, 8)]
IDS = ["A%d_Ch%d_D%d" % s for s in SHAPES]
RTOL, ATOL = 2e-5, 1e-8
SENTINEL, MARGIN = -1234.5, 64  # floats around an image in its buffer


def _sizes(A, Ch, depth):
    taps, F = 2 * A - 1, Ch * A * A
    return [Ch * 2 * taps, Ch] * 2 + [Ch * Ch * taps, Ch] * (4 * depth) + [A * F, A, F, 1]


def _views(flat, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(flat[at:at + n])
        at += n
    assert at == flat.numel()
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _state(shape, seed, fresh=False):
    """param / exp_avg / exp_avg_sq / target as four flat buffers in net.parameters() order (fresh: Adam's state before its first step)."""
    from _gpu import DEV

    n = sum(_sizes(*shape))
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.1
    m = torch.zeros(n) if fresh else torch.randn(n, generator=g) * 1e-2
    v = torch.zeros(n) if fresh else torch.rand(n, generator=g) * 1e-3
    t = p.clone() if fresh else torch.randn(n, generator=g) * 0.1
    return [x.to(DEV) for x in (p, m, v, t)]


def _buckets(shape, seed):
    """Three gradient buckets: norm ~ 10 (max_norm = 1 clips), ~ 0.1 (it does not), ~ 3."""
    from _gpu import DEV

    n = sum(_sizes(*shape))
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    out = []
    for norm in (10.0, 0.1, 3.0):
        b = torch.randn(n, generator=g)
        out.append((b * (norm / float(b.norm()))).to(DEV))
    return out


def _image_buffers(shape, tensors):
    """An image of `tensors` in the middle of a sentinel-filled buffer -> (buffer, image view)."""
    import rnad_hip
    from _gpu import DEV

    size = int(rnad_hip.lib().rnad_conv_packed_size(*shape))
    buf = torch.full((size + 2 * MARGIN,), SENTINEL, dtype=torch.float32, device=DEV)
    image = buf[MARGIN:MARGIN + size]
    rnad_hip.conv_pack(tensors, *shape, out=image)
    return buf, image


def _margins_untouched(buf):
    return bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())


def _conv_run(shape, beta1, images="both", steps=3, seed=0, fresh=False):
    """`steps` launches of the ConvNet tail on 8 + 8 depth views -> dict of the final state."""
    import rnad_hip
    from _gpu import DEV

    sizes = _sizes(*shape)
    p, m, v, t = _state(shape, seed, fresh)
    counters = [torch.zeros((), dtype=torch.float32, device=DEV) for _ in sizes]
    bufs = imgs = (None, None)
    if images != "none":
        pairs = [_image_buffers(shape, _views(x, sizes)) for x in (p, t)]
        bufs, imgs = [b for b, _ in pairs], [i for _, i in pairs]
    before = [None if b is None else b.clone() for b in bufs]
    packed = {"both": tuple(imgs), "param": (imgs[0], None), "none": None}[images]
    tail = rnad_hip.ConvOptimizerStep(shape, _views(p, sizes), _views(m, sizes), _views(v, sizes), counters, _views(t, sizes),
                                      1e-3, beta1, 0.999, 1e-8, 1.0, 0.01, packed=packed)
    norms = torch.zeros((steps,), dtype=torch.float32, device=DEV)
    for i, bucket in enumerate(_buckets(shape, seed)[:steps]):
        kept = bucket.clone()
        tail(bucket, total_norm=norms[i:i + 1])
        assert torch.equal(_bits(bucket), _bits(kept)), "the gradient bucket is read only"
    torch.cuda.synchronize()
    assert int(tail.ticket.item()) == 0, "the last workgroup hands the ticket word back"
    return dict(p=p, m=m, v=v, t=t, counters=counters, norms=norms, bufs=bufs, imgs=imgs, before=before, sizes=sizes)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_same_bits_as_the_existing_tail(shape):
    """8 + 8 depth views of four flat buffers through rnad_conv_optimizer_step == the buffers as ONE tensor through rnad_optimizer_step."""
    import rnad_hip
    from _gpu import DEV

    n = sum(_sizes(*shape))
    for beta1 in (0.0, 0.9):  # (at::lerp takes its other branch below beta1 = 0.5)
        got = _conv_run(shape, beta1, images="none")
        p, m, v, t = _state(shape, 0)
        counter = torch.zeros((), dtype=torch.float32, device=DEV)
        ref = rnad_hip.OptimizerStep([p], [m], [v], [counter], [t], 1e-3, beta1, 0.999, 1e-8, 1.0, 0.01)
        norms = torch.zeros((3,), dtype=torch.float32, device=DEV)
        for i, bucket in enumerate(_buckets(shape, 0)):
            ref(bucket, total_norm=norms[i:i + 1])
        torch.cuda.synchronize()
        assert p.numel() == n
        for name, want in (("p", p), ("m", m), ("v", v), ("t", t), ("norms", norms)):
            assert torch.equal(_bits(got[name]), _bits(want)), (name, beta1)
        np.testing.assert_allclose(norms.cpu().numpy(), [10.0, 0.1, 3.0], rtol=1e-5)
        assert float(counter) == 3.0 and [float(c) for c in got["counters"]] == [3.0] * (8 + 8 * shape[2])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_step_is_torchs_clip_adam_ema(shape):
    sizes = _sizes(*shape)
    for beta1 in (0.0, 0.9):
        got = _conv_run(shape, beta1, images="none", steps=1, fresh=True)
        p, _, _, t = _state(shape, 0, fresh=True)
        params = [torch.nn.Parameter(x) for x in _views(p, sizes)]
        for q, g in zip(params, _views(_buckets(shape, 0)[0].clone(), sizes)):
            q.grad = g
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt = torch.optim.Adam(params, lr=1e-3, betas=(beta1, 0.999), eps=1e-8, fused=True, capturable=True)
        opt.step()
        targets = _views(t, sizes)
        with torch.no_grad():
            torch._foreach_mul_(targets, 1 - 0.01)
            torch._foreach_add_(targets, [q.detach() for q in params], alpha=0.01)
        torch.cuda.synchronize()
        v = torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params])
        assert all(float(opt.state[q]["step"]) == 1.0 for q in params) and [float(c) for c in got["counters"]] == [1.0] * len(sizes)
        for name, want in (("p", p), ("t", t), ("v", v)):
            np.testing.assert_allclose(got[name].cpu().numpy(), want.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=f"{name} beta1={beta1}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_images_follow_the_weights(shape):
    """After three steps each image is a fresh rnad_conv_pack of the updated tensors, bit for bit (padding slots included: never written,
    they keep the zeros of the first pack), and nothing around an image -- or a NULL image's buffer -- is written."""
    import rnad_hip

    both = _conv_run(shape, 0.0, images="both")
    sizes = both["sizes"]
    for key, buf, image in (("p", both["bufs"][0], both["imgs"][0]), ("t", both["bufs"][1], both["imgs"][1])):
        fresh = rnad_hip.conv_pack(_views(both[key], sizes), *shape)
        assert torch.equal(_bits(image), _bits(fresh)), key
        assert _margins_untouched(buf), key
        assert not torch.equal(buf, both["before"][0 if key == "p" else 1]), "the image must have moved with the weights"
    # packed_target = NULL: the learner's image follows, the target's buffer is left as it was
    half = _conv_run(shape, 0.0, images="param")
    assert torch.equal(_bits(half["imgs"][0]), _bits(both["imgs"][0])) and _margins_untouched(half["bufs"][0])
    assert torch.equal(_bits(half["bufs"][1]), _bits(half["before"][1]))
    # both NULL: the tensors alone
    none = _conv_run(shape, 0.0, images="none")
    for run in (half, none):
        for key in ("p", "m", "v", "t", "norms"):
            assert torch.equal(_bits(run[key]), _bits(both[key])), key


# ---------------------------------------------------------------------------------------------------- in RNaD
def _rnad(tree, name, B, monkeypatch, tmp_path, net="ConvNet", **kw):
    from _gpu import DEV
    from learn.rnad import RNaD

    monkeypatch.setenv("RNAD_SAVE_DIR", str(tmp_path))
    A = tree.max_actions
    net_params = ({"type": "ConvNet", "max_actions": A, "channels": 16, "depth": 2, "batch_norm": False} if net == "ConvNet"
                  else {"type": "MLP", "max_actions": A, "width": 64})
    return RNaD(tree=tree, device=DEV, directory_name=name, batch_size=B, eta=0.2, b1_adam=0.0, lr=1e-3, net_params=net_params, **kw)


def _count_torch_steps(rn):
    calls, real = [], rn.optimizer.step
    rn.optimizer.step = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    return calls


def _held_images(rn):
    """The two images the trainer holds, WITHOUT asking _packed_images (which would re-pack stale ones)."""
    cache = rn._packed_cache
    assert cache["maintained"] is False, "a ConvNet's maintained layout is the plain one"
    return cache["layouts"][False]["images"]


def _assert_images_current(rn):
    import rnad_hip

    torch.cuda.synchronize()
    for image, net in zip(_held_images(rn), (rn.net, rn.net_target)):
        assert torch.equal(_bits(image), _bits(rnad_hip.conv_pack(net._weights(), *net._shape())))


def test_the_tail_is_opt_in_for_a_convnet(tmp_path, monkeypatch):
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    torch.manual_seed(5)
    conv = _rnad(tree, "conv", 512, monkeypatch, tmp_path)
    conv.initialize()
    assert conv.fused_optimizer is None
    calls = _count_torch_steps(conv)
    buf = Buffer(1)
    for _ in range(2):
        conv.train_step(buf, alpha=0.5)
        conv.total_steps += 1
    assert conv._fused_tail() is None and len(calls) == 2 and conv._fused_optimizer_on() is False
    mlp = _rnad(tree, "mlp", 512, monkeypatch, tmp_path, net="MLP")
    mlp.initialize()
    assert mlp.fused_optimizer is None and mlp._fused_optimizer_on() is True
    mlp.train_step(Buffer(1), alpha=0.5)
    assert mlp._fused_tail() is not None
    mlp.fused_optimizer = False
    assert mlp._fused_tail() is None

    on = _rnad(tree, "on", 512, monkeypatch, tmp_path)
    on.initialize()
    on.fused_optimizer, on.use_graph = True, False
    calls = _count_torch_steps(on)
    buf = Buffer(1)
    assert on._fused_tail() is None, "Adam's state does not exist before torch's first step"
    on.train_step(buf, alpha=0.5)
    assert len(calls) == 1 and on._fused_tail() is not None
    for _ in range(2):
        on.train_step(buf, alpha=0.5)
        on.total_steps += 1
    assert len(calls) == 1, "once the tail exists torch's optimizer.step is not called"
    assert [float(st["step"]) for st in on.optimizer.state.values()] == [3.0] * 24
    _assert_images_current(on)


def test_images_stay_current_eager_and_replayed(tmp_path, monkeypatch):
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    finals = {}
    for use_graph in (False, True):
        torch.manual_seed(7)
        rn = _rnad(tree, f"g{use_graph}", 512, monkeypatch, tmp_path)
        rn.initialize()
        rn.use_graph, rn.fused_optimizer = use_graph, True
        calls = _count_torch_steps(rn)
        buf = Buffer(1)
        ptrs = None
        for i in range(7):
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1
            if i == 1:
                ptrs = [t.data_ptr() for t in _held_images(rn)]
        _assert_images_current(rn)
        assert [t.data_ptr() for t in _held_images(rn)] == ptrs, "the images keep their addresses"
        assert len(calls) == 1
        if use_graph:
            assert rn._graph.get("graph") is not None and not rn._graph["failed"], "the step must have been captured and replayed"
            assert rn._graph["advances"], "the captured step ends in the tail, which moves the step queue on"
        assert [float(st["step"]) for st in rn.optimizer.state.values()] == [7.0] * 24
        finals[use_graph] = [p.detach().clone() for p in list(rn.net.parameters()) + list(rn.net_target.parameters())]
    for a, b in zip(finals[True], finals[False]):
        assert torch.equal(a, b)


def test_images_stay_current_with_lazy_rows_at_a5(tmp_path, monkeypatch):
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("a5")
    torch.manual_seed(9)
    rn = _rnad(tree, "lazy", 512, monkeypatch, tmp_path)
    rn.initialize()
    rn.lazy_rows, rn.fused_optimizer, rn.tabular_gate, rn.use_graph = True, True, 0, False
    calls = _count_torch_steps(rn)
    buf = Buffer(1)
    for _ in range(4):
        rn.train_step(buf, alpha=0.5)
        rn.total_steps += 1
    print("lazy step applied:", rn.last_rows is not None)
    assert len(calls) == 1 and rn._fused_tail() is not None
    _assert_images_current(rn)


def test_one_tail_step_against_torchs(tmp_path, monkeypatch):
    """Two runs from one seed: step 1 is torch's in both (identical states), step 2 the tail's in one and torch's in the other."""
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    runs = {}
    for fused in (False, True):
        torch.manual_seed(13)
        rn = _rnad(tree, f"t{fused}", 512, monkeypatch, tmp_path, grad_clip=0.05, gamma_averaging=0.01)
        rn.initialize()
        rn.use_graph, rn.fused_optimizer = False, fused
        calls = _count_torch_steps(rn)
        buf = Buffer(1)
        for _ in range(2):
            rn.train_step(buf, alpha=0.5)
            rn.total_steps += 1
        torch.cuda.synchronize()
        assert len(calls) == (1 if fused else 2)
        runs[fused] = ([p.detach().clone() for n in (rn.net, rn.net_target) for p in n.parameters()]
                       + [rn.optimizer.state[p]["exp_avg_sq"].clone() for p in rn.net.parameters()])
    assert any(not torch.equal(a, b) for a, b in zip(runs[False][:24], runs[False][24:48])), "the nets must have trained"
    for a, b in zip(runs[False], runs[True]):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_checkpoint_written_with_the_tail_resumes(tmp_path, monkeypatch):
    from _gpu import golden_tree
    from environment.episode import Buffer

    tree, _ = golden_tree("small")
    torch.manual_seed(3)
    rn = _rnad(tree, "ckpt", 512, monkeypatch, tmp_path, bounds=[1], delta_m=[3])
    rn.fused_optimizer, rn.use_graph = True, False
    rn.run(max_updates=1, checkpoint_mod=1, expl_mod=10**9, log_mod=10**9)
    assert rn._fused_tail() is not None
    again = _rnad(tree, "ckpt", 512, monkeypatch, tmp_path, bounds=[1], delta_m=[3])
    again.fused_optimizer, again.use_graph = True, False
    again.initialize()
    assert (again.m, again.n) == (0, 2) and again.total_steps == 2
    assert [float(st["step"]) for st in again.optimizer.state.values()] == [2.0] * 24, "step 2 was the tail's: its counters are in the checkpoint"
    calls = _count_torch_steps(again)
    again.train_step(Buffer(1), alpha=0.5)
    assert len(calls) == 0 and again._fused_tail() is not None, "the resumed run uses the tail from its first step"
    assert [float(st["step"]) for st in again.optimizer.state.values()] == [3.0] * 24
    _assert_images_current(again)
