"""ConvNet family (nn/net.py) on the CPU against the reference's recorded nets (tests/golden/convnet_*.npz, written by
tests/golden/make_convnet.py from the imported reference): state-dict layout, strict checkpoint loading and the torch fallback's outputs.

Tolerance 1e-6 absolute: INTEGRATION.md's figure for "the same function in another summation order" -- the modules are the reference's
torch ops (expected error 0); the policy differs from the reference's softmax * mask renormalised by rounding only."""
import numpy as np
import pytest
import torch

from _util import load

SHAPES = ("small", "a5", "c1")
TOL = 1e-6


def _net(fx, prefix="", batch_norm=False):
    from nn.net import ConvNet

    net = ConvNet(int(fx["max_actions"]), int(fx["channels"]), depth=int(fx["depth"]), batch_norm=batch_norm)
    sd = {str(k): torch.as_tensor(fx[prefix + "w_" + str(k).replace(".", "_")]) for k in fx[prefix + "keys"]}
    net.load_state_dict(sd, strict=True)
    return net


@pytest.mark.parametrize("name", SHAPES)
def test_state_dict_keys_and_shapes_are_the_references(name):
    from nn.net import ConvNet

    fx = load("convnet_" + name)
    cases = [("", False)] + ([("bn_", True)] if name == "small" else [])
    for prefix, bn in cases:
        net = ConvNet(int(fx["max_actions"]), int(fx["channels"]), depth=int(fx["depth"]), batch_norm=bn)
        sd = net.state_dict()
        assert list(sd.keys()) == [str(k) for k in fx[prefix + "keys"]]
        for k, v in sd.items():
            assert tuple(v.shape) == fx[prefix + "w_" + k.replace(".", "_")].shape, k
        A, Ch = int(fx["max_actions"]), int(fx["channels"])
        assert tuple(sd["pre.row_conv.weight"].shape) == (Ch, 2, 1, 2 * A - 1) and tuple(sd["pre.col_conv.weight"].shape) == (Ch, 2, 2 * A - 1, 1)
        assert tuple(sd["policy.weight"].shape) == (A, Ch * A * A) and tuple(sd["value.weight"].shape) == (1, Ch * A * A)
        assert ("tower.0.batch_norm0.weight" in sd) == bn


@pytest.mark.parametrize("name", SHAPES)
def test_reference_checkpoint_loads_strictly_and_reproduces_its_outputs(name):
    fx = load("convnet_" + name)
    net = _net(fx).eval()
    obs = torch.as_tensor(fx["obs"])
    with torch.no_grad():
        logits, value = net.forward_logits(obs)
    policy = net.forward_policy(obs)
    for what, got, want in (("logits", logits, fx["logits"]), ("value", value, fx["value"]), ("policy", policy, fx["policy"])):
        print(name, what, "max abs err", float(np.abs(got.numpy() - want).max()))
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=TOL, err_msg=what)
    logits2, policy2, value2, actions = net.forward(obs)
    np.testing.assert_allclose(policy2.numpy(), fx["policy"], rtol=0, atol=TOL)
    legal = obs[:, 1, :, 0] != 0
    assert legal[torch.arange(obs.shape[0]), actions].all(), "a sampled action must be legal"


def test_batch_norm_eval_reproduces_the_reference():
    fx = load("convnet_small")
    net = _net(fx, "bn_", True).eval()
    obs = torch.as_tensor(fx["obs"])
    with torch.no_grad():
        logits, value = net.forward_logits(obs)
    policy = net.forward_policy(obs)
    for what, got, want in (("logits", logits, fx["bn_logits"]), ("value", value, fx["bn_value"]), ("policy", policy, fx["bn_policy"])):
        print("bn eval", what, "max abs err", float(np.abs(got.numpy() - want).max()))
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=TOL, err_msg=what)


def test_batch_norm_train_uses_the_statistics_of_the_batch_it_is_given():
    """Training-mode BatchNorm against freshly computed torch modules: conv -> relu -> batch statistics, as the reference's block."""
    import torch.nn.functional as F

    fx = load("convnet_small")
    net = _net(fx, "bn_", True).train()
    A = net.max_actions
    obs = torch.as_tensor(fx["obs"])[:97]
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        logits, value = net.forward_logits(obs)

    def cross(x, p):
        r = F.conv2d(F.pad(x, (A - 1, A - 1, 0, 0)), sd[p + ".row_conv.weight"], sd[p + ".row_conv.bias"])
        return r + F.conv2d(F.pad(x, (0, 0, A - 1, A - 1)), sd[p + ".col_conv.weight"], sd[p + ".col_conv.bias"])

    def bn(x, p):
        return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], training=True, eps=1e-5)

    x = cross(obs, "pre")
    for d in range(net.depth):
        t = f"tower.{d}"
        x = x + bn(torch.relu(cross(bn(torch.relu(cross(x, t + ".conv0")), t + ".batch_norm0"), t + ".conv1")), t + ".batch_norm1")
    x = x.reshape(obs.shape[0], -1)
    want_l, want_v = x @ sd["policy.weight"].T + sd["policy.bias"], x @ sd["value.weight"].T + sd["value.bias"]
    print("bn train max abs err", float((logits - want_l).abs().max()), float((value - want_v).abs().max()))
    np.testing.assert_allclose(logits.numpy(), want_l.numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(value.numpy(), want_v.numpy(), rtol=0, atol=TOL)
    with torch.no_grad():
        other, _ = net.forward_logits(obs[:31])
    assert not torch.allclose(other, logits[:31], atol=1e-4), "training-mode statistics must depend on the batch"


def test_cpu_and_batch_norm_nets_are_never_fused():
    fx = load("convnet_small")
    assert _net(fx)._fusable() is False  # CPU tensors
    assert _net(fx, "bn_", True)._fusable() is False
    assert _net(fx).pack() is None and _net(fx).per_row_ready() is False


def test_autograd_through_the_fallback_matches_the_fp64_gradients():
    fx = load("convnet_small")
    net = _net(fx)
    obs = torch.as_tensor(fx["obs"])
    logits, value = net.forward_logits(obs)
    torch.autograd.backward([logits, value], [torch.as_tensor(fx["dlogits"]), torch.as_tensor(fx["dv"])])
    for k, p in net.named_parameters():
        want = fx["g_" + k.replace(".", "_")]
        np.testing.assert_allclose(p.grad.numpy(), want, rtol=1e-3, atol=2e-5 * np.abs(want).max(), err_msg=k)
