"""The ConvNet optimiser tail without a GPU: the two symbols it adds to the C-ABI, and the map from a parameter element to its slots of
the packed image (rnad_conv_image_slots -- the function k_conv_optimizer_step scatters by) against a numpy restatement of k_conv_pack's
gather, written from the layout of ConvShape (csrc/conv_shape.hpp) and DESIGN.md section 5.6:

    per layer l (0 = pre, then conv0, conv1 of every block):  [row operand][column operand][Ch summed biases]
    then per tower layer:                                     [transposed row operand][transposed column operand]
    then policy.weight [A, F] | value.weight [F] | policy.bias [A] | value.bias | padding to a multiple of 4 floats

An operand is Mt x KS tiles of 64 floats, tile (mt, ks) at (mt * KS + ks) * 64, lane (k & 3) * 16 + (m & 15) of it holding entry
(m, k) = (16 mt + (lane & 15), 4 ks + (lane >> 4)); M = Ch A rows, K = Cin A columns (the pre-layer's 2 A padded to a multiple of 4).
Forward entry ((o, y), (c, x)) = W[o, c, x - y + A - 1]; transposed entry ((c, x), (o, y)) = the same weight.
"""
import ctypes as C

import pytest

import rnad_hip

# (A, channels, depth): one tap per conv | no K padding in the pre-layer | K padded 6 -> 8, the product shape | 10 -> 12, the lean
# backward's shape | 72 tensors, the limit of the pointer tables
SHAPES = [(1, 16, 1), (2, 8, 1), (3, 16, 2), (5, 16, 2), (8, 2, 8)]


def tensor_sizes(A, Ch, depth):
    taps, F = 2 * A - 1, Ch * A * A
    return [Ch * 2 * taps, Ch] * 2 + [Ch * Ch * taps, Ch] * (4 * depth) + [A * F, A, F, 1]


def gather_map(A, Ch, depth):
    """packed index -> the (tensor, element) pairs k_conv_pack reads for it; () for a padding slot.  Returns (list, kinds) with
    kinds[i] in 'weight' | 'bias' | 'head' | 'pad'."""
    L, taps, F = 2 * depth + 1, 2 * A - 1, Ch * A * A
    M, Mt = Ch * A, Ch * A // 16
    src, kinds = [], []

    def operand(l, dir_, transposed):
        cin = 2 if l == 0 else Ch
        K = cin * A
        KS = (K + 3) // 4
        for q in range(Mt * KS * 64):
            mt, ks, lane = q // (KS * 64), (q // 64) % KS, q % 64
            m, k = 16 * mt + (lane & 15), 4 * ks + (lane >> 4)
            if k >= K:
                src.append(()), kinds.append("pad")
                continue
            (o, y), (c, x) = (divmod(k, A), divmod(m, A)) if transposed else (divmod(m, A), divmod(k, A))
            src.append(((4 * l + 2 * dir_, (o * cin + c) * taps + x - y + A - 1),)), kinds.append("weight")

    for l in range(L):
        operand(l, 0, False)
        operand(l, 1, False)
        for o in range(Ch):
            src.append(((4 * l + 1, o), (4 * l + 3, o))), kinds.append("bias")
    for l in range(1, L):
        assert M == Ch * A  # (a tower operand is square: the transposed one has the same tiling)
        operand(l, 0, True)
        operand(l, 1, True)
    for tensor, n in ((4 * L, A * F), (4 * L + 2, F), (4 * L + 1, A), (4 * L + 3, 1)):
        for e in range(n):
            src.append(((tensor, e),)), kinds.append("head")
    while len(src) % 4:
        src.append(()), kinds.append("pad")
    return src, kinds


def test_declarations():
    protos = rnad_hip.header_prototypes()
    i32, i64, ptr = C.c_int, C.c_int64, C.c_void_p
    assert protos["rnad_conv_optimizer_step"] == (i32, [i32, i32, i32] + [ptr] * 13)
    assert protos["rnad_conv_image_slots"] == (i32, [i32, i32, i32, i32, i64, ptr, i32])
    lib = rnad_hip.lib()
    for name in ("rnad_conv_optimizer_step", "rnad_conv_image_slots"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == protos[name]
    # the entry point declines before it touches a device: a shape the tower kernels do not cover, and a null gradient bucket
    n = 8 + 8 * 2
    fake = (C.c_void_p * n)(*[0x1000] * n)  # (never dereferenced: both calls fail their argument checks)
    hp = rnad_hip.AdamParams(1e-3, 0.0, 0.999, 1e-8, 1.0, 0.001)
    word = C.c_uint32(0)
    assert not rnad_hip.conv_supported(3, 10, 1)
    rc = lib.rnad_conv_optimizer_step(3, 10, 1, fake, C.addressof(word), fake, fake, fake, fake, C.byref(hp), None, None, None, None,
                                      C.addressof(word), None)
    assert rc != 0 and b"unsupported shape" in lib.rnad_last_error()
    rc = lib.rnad_conv_optimizer_step(3, 16, 2, fake, None, fake, fake, fake, fake, C.byref(hp), None, None, None, None, C.addressof(word), None)
    assert rc != 0 and b"null argument" in lib.rnad_last_error()
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_image_slots(3, 10, 1, 0, 0)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.conv_image_slots(3, 16, 2, 1, 16)  # a bias has Ch = 16 elements


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "A%d_Ch%d_D%d" % s)
def test_slot_map_is_the_inverse_of_the_pack(shape):
    A, Ch, depth = shape
    assert rnad_hip.conv_supported(*shape)
    sizes = tensor_sizes(*shape)
    assert len(sizes) == 8 + 8 * depth and sum(sizes) == rnad_hip.conv_param_count(*shape)
    src, kinds = gather_map(*shape)
    total = int(rnad_hip.lib().rnad_conv_packed_size(*shape))
    assert len(src) == total

    named = [[] for _ in range(total)]  # slot -> the elements that name it, from the export
    lib, buf = rnad_hip.lib(), (C.c_int32 * (2 * A))()
    taps = 2 * A - 1
    for tensor, size in enumerate(sizes):
        conv_weight = tensor < 4 * (2 * depth + 1) and tensor % 2 == 0
        for e in range(size):
            n = lib.rnad_conv_image_slots(A, Ch, depth, tensor, e, buf, len(buf))
            slots = list(buf[:n])
            assert 0 < n <= len(buf) and len(set(slots)) == n and all(0 <= s < total for s in slots)
            if conv_weight:
                want = A - abs(e % taps - (A - 1))
                assert n == (want if tensor < 4 else 2 * want), (tensor, e)
            else:
                assert n == 1
            for s in slots:
                named[s].append((tensor, e))
    # a short buffer: the count is still the whole answer, only `capacity` indices are written
    small = (C.c_int32 * 2)(-7, -7)
    first_tower = 4
    mid = (A - 1)  # the centre tap of W[0, 0, :]: 2 A slots
    assert lib.rnad_conv_image_slots(A, Ch, depth, first_tower, mid, small, 1) == 2 * A and small[1] == -7

    for i in range(total):
        got = tuple(sorted(named[i]))
        assert got == tuple(sorted(src[i])), (i, kinds[i], got, src[i])
        assert len(got) == {"weight": 1, "head": 1, "bias": 2, "pad": 0}[kinds[i]]
        if kinds[i] == "bias":
            (t0, e0), (t1, e1) = got
            assert t1 == t0 + 2 and t0 % 4 == 1 and e0 == e1
    # padding: the pre-layer's K rounded up to a multiple of 4 in both of its operands, and fewer than four floats at the very end
    K0 = 2 * A
    pre_pads = 2 * (Ch * A) * ((K0 + 3) // 4 * 4 - K0)
    tail_pads = kinds.count("pad") - pre_pads
    assert 0 <= tail_pads < 4 and kinds[: 2 * (Ch * A) * ((K0 + 3) // 4 * 4)].count("pad") == pre_pads
    assert all(k == "pad" for k in kinds[total - tail_pads:])
    if shape == (2, 8, 1):
        assert "pad" not in kinds[: kinds.index("bias")]  # K = 4: the pre-layer's operands have no padding
    if shape == (3, 16, 2):
        assert kinds[: 2 * 48 * 8].count("pad") == 2 * 48 * 2  # K padded 6 -> 8
