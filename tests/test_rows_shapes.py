"""What the GPU sweep of the fused rows kernel (tests/test_hip_rows_shapes.py on csrc/mlp_rows.hip) stands on, checked without a GPU.

1. G.  The gate of the sweep is |got - want| <= G * 2^-24 * B against the fp64 reference of tests/_rowsref.py (B: the sum of the
   absolute terms of a row's output).  On every case of the sweep plain fp32 torch on the CPU stays within HALF of it; a correct fp32
   kernel has the other half for its own summation order.  G is fixed here, from these numbers (fp32 torch used 0.07 - 0.50 units on
   the "init" family, up to 2.66 on "wide", where the sums along the sign-aligned path do not cancel: profiles/mlp_rows_errors.json),
   and nowhere else; it is never adjusted from a kernel's output.  If a seed fails here, the seed changes.
2. The gate sees the split first layer: h + m + l == x bit for bit; the emulated six-product chain stays within half of the gate, and
   with any one of the small products W_l x_h, W_h x_l, W_m x_m left out its largest error is more than TWICE the gate at A = 2 .. 5
   (measured 28 - 48 units against 2 G = 16).
3. The sizes of the sweep keep the properties they were chosen for (the kernel's partition of rows over workgroups, restated).
4. The host functions that select an instantiation -- rnad_mlp_rows_records_supported, rnad_mlp_rows_actor_supported,
   rnad_mlp_rows_uses_split -- on the shapes of the sweep and on their declined neighbours.
5. No instantiation that those functions can select uses scratch memory: read from the kernel metadata of the BUILT library (a build
   with scratch wrote wrong records once)."""
import os

import numpy as np
import pytest
import torch

import _rowsref as rr

G = 8.0  # the smallest power of two with fp32 torch inside G / 2 (worst 2.66) -- and 2 G stays below what a dropped product costs (28.4)


def _id(c):
    return "-".join(str(x) for x in c)


def _lib():
    import rnad_hip

    return rnad_hip.lib()


# ------------------------------------------------------------------------------------------------ 1. the inputs and G
@pytest.mark.parametrize("c", rr.sweep_cases(), ids=_id)
def test_fp32_torch_uses_at_most_half_of_the_gate(c):
    case = rr.case(*c)
    kind, A = c[0], c[1]
    assert case.N == (rr.SMALL_ROWS if kind == "small" else rr.CHUNK_ROWS)[A] <= rr.MAX_ROWS
    assert case.obs.dtype == (torch.float16 if case.half else torch.float32)
    legal = case.obs[:, 1].reshape(case.N, -1).float()
    e0 = torch.zeros(A * A)
    e0[0] = 1.0
    absorbing = (legal == e0).all(1) & torch.tensor(A > 1)
    assert ((legal == 1).all(1) | absorbing).all(), "every tree of the sweep is foldable"
    assert A == 1 or int(absorbing.sum()) == 2, "the two rows of the absorbing state"
    ref = case.ref
    logits, v, vt = rr.fp32_torch(case.nets[0], case.nets[1], case.obs)
    used = [rr.gate(got, want, B, G / 2, f"{c} {what}") for what, got, want, B in
            (("logits", logits, ref.logits, ref.B_logits), ("v", v, ref.v, ref.B_v), ("v_target", vt, ref.v_target, ref.B_v_target))]
    print(c, "fp32 torch, units of 2^-24 B (logits, v, v_target):", [round(u, 3) for u in used])


def test_the_cases_are_deterministic_and_the_wide_family_is_what_it_says():
    a, b = rr.nets(3, 256, "wide"), rr.nets(3, 256, "wide")
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x._weights(), y._weights()))
    assert torch.equal(rr.wide_ev(100, 3), rr.wide_ev(100, 3))
    init = rr.nets(3, 256, "init")
    for i in (2, 3):  # the regularisation nets, and everything but the first-layer matrices (and the value signs), stay the default init
        assert all(torch.equal(p, q) for p, q in zip(a[i]._weights(), init[i]._weights()))
    for i in (0, 1):
        wa, wi = a[i]._weights(), init[i]._weights()
        assert all(torch.equal(wa[j], wi[j]) for j in (1, 3, 5, 6, 7)) and torch.equal(wa[2].abs(), wi[2].abs())
        for j in (0, 4):
            w = wa[j].detach().abs()
            assert float(w[:, :9].min()) >= 2.0**-6 and float(w[:, :9].max()) < 2 and float(w[2:, 9:].min()) >= 2.0**-12 and float(w[2:, 9:].max()) < 2.0**-4  # (before: hand-placed values)
    ev = rr.wide_ev(4096, 5).abs()
    assert float(ev.min()) >= 2.0**-8 and float(ev.max()) < 2
    flat = rr.wide((64,), -6, 1, torch.Generator().manual_seed(0)).numpy()
    assert flat[0] == np.float32(2) - np.float32(2.0**-23) and flat[4] == np.float32(1 + 2.0**-8), "the hand-placed values lead"


# ------------------------------------------------------------------------------------------------ 2. the split first layer
def _wide_values(A):
    n = rr.nets(A, 256, "wide")
    obs = rr.observations(rr.tree_observations("small", A), "wide")
    vals = [rr.fold(w[0].detach(), w[1].detach(), A)[0].flatten() for w in (n[0]._weights()[0:2], n[0]._weights()[4:6], n[1]._weights()[0:2])]
    return torch.cat(vals + [obs[:, 0].flatten(), obs[:, 0].half().float().flatten()])


@pytest.mark.parametrize("A", (2, 3, 4, 5))
def test_split_identity(A):
    """x = h + m + l exactly on every value the split kernels see on the "wide" family: folded weights, ev in fp32 and rounded to fp16."""
    x = _wide_values(A)
    h, m, l = rr.split3(x)
    assert h.dtype == m.dtype == l.dtype == torch.bfloat16
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert float((m != 0).float().mean()) > 0.9 and float((l.float()[:x.numel() // 2] != 0).float().mean()) > 0.5, "all three pieces carry weight"


@pytest.mark.parametrize("A", (2, 3, 4, 5))
def test_the_gate_sees_a_dropped_product(A):
    case = rr.case("small", A, 256, "wide", False)
    ref = case.ref
    heads = ((case.nets[0]._weights()[4:8], ref.logits, ref.B_logits), (case.nets[0]._weights()[0:4], ref.v[:, None], ref.B_v[:, None]),
             (case.nets[1]._weights()[0:4], ref.v_target[:, None], ref.B_v_target[:, None]))
    worst = {}
    for drop in (None, "lh", "hl", "mm"):
        worst[drop] = max(float(rr.normalised(rr.split_chain(w, case.obs, drop), want, B).max()) for w, want, B in heads)
    print("A", A, "emulated split chain, largest error in units of 2^-24 B:", {str(k): round(v, 2) for k, v in worst.items()})
    assert worst[None] <= G / 2, "the six-product chain is the same function to fp32 accuracy"
    for drop in ("lh", "hl", "mm"):
        assert worst[drop] >= 2 * G, f"dropping W_{drop[0]} x_{drop[1]} must not pass the gate"


# ------------------------------------------------------------------------------------------------ 3. the partition
CUS = 256  # an MI355X


def test_partition_restates_the_kernel():
    assert rr.partition(44, CUS) == [(2, 1, 1)]
    assert rr.partition(22, CUS) == [(1, 1, 1)]                           # A = 1: one partial half step
    assert rr.partition(0, CUS, 1642) == [(0, 0, 0)] * 26                 # an empty list on the 52-tile table
    assert rr.partition(257, CUS, 1642) == [(1, 1, 1)] * 9 + [(0, 0, 0)] * 17
    p = rr.partition(132862, CUS)
    assert len(p) == CUS and p[:56] == [(17, 9, 3)] * 56 and p[56:] == [(16, 8, 2)] * 200
    assert rr.partition(1195744, CUS)[0] == (146, 73, 19)


@pytest.mark.parametrize("A", sorted(rr.CHUNK))
def test_chunk_cases_walk_the_chunk_loop(A):
    N = rr.CHUNK_ROWS[A]
    n = rr.chunk_list_length(N)
    assert 0 < N - n < 64 and n % 32 != 0 and N <= rr.MAX_ROWS
    for rows, table in ((N, None), (n, N)):
        got = rr.partition_properties(rows, CUS, table)
        assert got["three_chunks"] and got["short_last_chunk"] and got["half_step"] and got["partial_tile"], (A, rows, got)


def test_short_lists_leave_most_workgroups_empty_and_every_wave_count_runs():
    for A in (3, 4):
        N = rr.SMALL_ROWS[A]
        for n in rr.LIST_LENGTHS:
            assert n < N
            if A == 3 or n < 100:  # (257 rows are nine of the eighteen tiles of the A = 4 tree: one per workgroup)
                assert rr.partition_properties(n, CUS, N)["empty"] > 0.5, (A, n)
    assert rr.SMALL_ROWS[1] < 32
    assert {W // 32 for W in (256,) + rr.WIDTHS_EXTRA} == {1, 3, 5, 7, 8}
    assert {n % 32 for n in rr.LIST_LENGTHS} >= {0, 1, 31} and {n % 64 for n in rr.LIST_LENGTHS} >= {0, 1, 31, 32, 33, 63}


# ------------------------------------------------------------------------------------------------ 4. host shape functions
# (A, fold, mode, split) at width 256: mode 0 = both nets and the records, 1 = logits from the table, 2 = the staged actor
LAUNCHABLE_256 = {(1, False, m, False) for m in (0, 1, 2)} \
    | {(A, f, m, False) for A in (2, 3) for f in (False, True) for m in (0, 1, 2)} | {(A, True, m, True) for A in (2, 3) for m in (0, 1, 2)} \
    | {(4, False, 1, False), (4, True, 1, False), (4, True, 1, True), (4, True, 2, False), (4, True, 2, True)} \
    | {(5, True, 1, False), (5, True, 1, True), (5, True, 2, False)}  # (the staged rows of the A = 5 actor do not fit the LDS: no split)


def test_supported_shapes_of_the_sweep():
    lib = _lib()
    assert set(rr.launchable(lib, 256)) == LAUNCHABLE_256
    for W in rr.WIDTHS_EXTRA:  # the split first layer is a width-256 kernel
        assert set(rr.launchable(lib, W)) == {k for k in LAUNCHABLE_256 if not k[3]}, W
    # 2 = the default, 1 = on request only
    assert [lib.rnad_mlp_rows_uses_split(A, 256, 1, 1) for A in (1, 2, 3, 4, 5, 6)] == [0, 1, 1, 2, 2, 0]
    assert [lib.rnad_mlp_rows_uses_split(A, 256, 1, 2) for A in (2, 3, 4, 5)] == [1, 1, 2, 0]
    assert lib.rnad_mlp_rows_uses_split(3, 256, 0, 0) == 0 and lib.rnad_mlp_rows_uses_split(3, 224, 1, 0) == 0
    assert lib.rnad_mlp_rows_uses_split(3, 256, 1, 3) == 0 and lib.rnad_mlp_rows_uses_split(3, 256, 1, -1) == 0


@pytest.mark.parametrize("A,W,fold,why", (
    (0, 256, 0, "A = 0"), (9, 256, 0, "A = 9"), (3, 16, 0, "width 16"), (3, 48, 0, "width 48"), (3, 288, 0, "width 288"),
    (3, 16, 1, "width 16"), (3, 48, 1, "width 48"), (3, 288, 1, "width 288"), (1, 256, 1, "fold at A = 1"), (6, 256, 1, "fold at A = 6")))
def test_declined_neighbours(A, W, fold, why):
    lib = _lib()
    for mode in (0, 1):
        assert lib.rnad_mlp_rows_records_supported(A, W, fold, mode) == 0, why
    assert lib.rnad_mlp_rows_actor_supported(A, W, fold) == 0, why
    for mode in (0, 1, 2):
        assert lib.rnad_mlp_rows_uses_split(A, W, fold, mode) == 0, why


def test_declined_modes():
    lib = _lib()
    for fold in (0, 1):
        assert lib.rnad_mlp_rows_records_supported(4, 256, fold, 0) == 0, "MODE 0 at A = 4"
        assert lib.rnad_mlp_rows_uses_split(4, 256, fold, 0) in (0, 2), "(the split rule does not know the modes' limits: rows_launch asks both)"
    assert lib.rnad_mlp_rows_records_supported(5, 256, 0, 1) == 0, "MODE 1 without the fold at A = 5"
    assert lib.rnad_mlp_rows_records_supported(5, 256, 1, 1) == 1 and lib.rnad_mlp_rows_records_supported(4, 256, 0, 1) == 1
    assert lib.rnad_mlp_rows_actor_supported(4, 256, 0) == 0 and lib.rnad_mlp_rows_actor_supported(3, 256, 0) == 1


# ------------------------------------------------------------------------------------------------ 5. scratch
def test_no_launchable_instantiation_uses_scratch():
    import rnad_hip

    lib = _lib()
    meta = rr.rows_kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    assert len(meta) >= 2 * len(LAUNCHABLE_256), f"only {len(meta)} k_rows_forward_records instantiations found in the library"
    keys = {k for W in (256,) + rr.WIDTHS_EXTRA for k in rr.launchable(lib, W)}
    assert keys == LAUNCHABLE_256
    bad = {}
    for A, fold, mode, split in sorted(keys):
        for half in (False, True):
            m = meta.get((A, half, fold, mode, split))
            assert m is not None, f"k_rows_forward_records<{A}, {'__half' if half else 'float'}, {fold}, {mode}, {split}> is not in the library"
            print(f"A={A} half={half} fold={fold} mode={mode} split={split}: {m}")
            if m["scratch"] != 0:
                bad[(A, half, fold, mode, split)] = m
    assert not bad, f"instantiations that can be launched use scratch memory: {bad}"
