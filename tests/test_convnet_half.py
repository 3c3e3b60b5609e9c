"""fp16 observation tables for the ConvNet family, the part that needs no GPU: the three *_obs entry points exist (header and built
library), the binding's dtype check lets float16 through, and an fp16 table MEANS rounded values with fp32 arithmetic -- the statement
tests/test_hip_convnet_half.py holds the kernels to bit for bit."""
import pytest
import torch

NEW = ("rnad_conv_forward_obs", "rnad_conv_forward_actor_obs", "rnad_conv_backward_obs")


def test_header_declares_and_library_exports_the_obs_entry_points():
    import ctypes as C

    import rnad_hip

    protos = rnad_hip.header_prototypes()
    for name in NEW:
        assert name in protos, f"include/rnad_hip.h does not declare {name}"
        twin = name[: -len("_obs")]
        ret, args = protos[name]
        tret, targs = protos[twin]
        # the twin's argument list with (const void *obs, int obs_half) in place of (const float *obs)
        assert ret is tret and len(args) == len(targs) + 1
        at = next(i for i, (a, b) in enumerate(zip(args, targs)) if a is not b)
        assert args[at] is C.c_int and args[at - 1] is C.c_void_p, f"{name}: `int obs_half` follows `const void *obs`"
        assert args[:at] == targs[:at] and args[at + 1:] == targs[at:], f"{name}: every other argument is its twin's"
        assert hasattr(rnad_hip.lib(), name), f"librnad_hip.so does not export {name}"


@pytest.mark.parametrize("dtype", (torch.float16, torch.float32, torch.float64, torch.bfloat16))
def test_binding_dtype_check(dtype):
    """The check alone, on CPU tensors: fp32 and fp16 observations pass it (and are then refused for not being on a GPU -- there is no CPU
    path), any other dtype is refused for what it is."""
    import rnad_hip

    A, Ch, depth = 2, 8, 1
    obs = torch.zeros((4, 2, A, A), dtype=dtype)
    packed = torch.zeros((int(rnad_hip.lib().rnad_conv_packed_size(A, Ch, depth)),))
    with pytest.raises(rnad_hip.RnadHipError) as err:
        rnad_hip.conv_forward(packed, A, Ch, depth, obs)
    refused_for_dtype = "observations only" in str(err.value)
    assert refused_for_dtype == (dtype not in (torch.float16, torch.float32)), str(err.value)
    if not refused_for_dtype:
        assert "GPU tensor" in str(err.value)


def test_half_observations_are_rounded_values_with_fp32_arithmetic():
    from nn.net import ConvNet

    torch.manual_seed(3)
    net = ConvNet(3, 16, depth=2, batch_norm=False)
    obs = torch.rand((37, 2, 3, 3)) * 2 - 1
    obs[0, 0, 0, 0], obs[1, 0, 0, 0], obs[2, 0, 0, 0] = 2.0 ** -24, -(2.0 ** -14), 65504.0  # an fp16 subnormal and the two ends of the normals
    half = obs.half()
    assert not torch.equal(half.float(), obs), "the rounding must be visible in the inputs"
    with torch.no_grad():
        got_l, got_v = net.forward_logits(half)
        want_l, want_v = net.forward_logits(half.float())
    assert got_l.dtype == torch.float32 and got_v.dtype == torch.float32
    assert torch.equal(got_l, want_l) and torch.equal(got_v, want_v)
