"""What the GPU sweep of the MLP backward (tests/test_hip_mlp_bwd_shapes.py on csrc/mlp_bwd_t.hip, csrc/mlp_bwd.hip) stands on, checked
without a GPU.

1. G.  The gate of the sweep is |got - want| <= G * 2^-24 * B on every element of the eight gradient tensors against the fp64 reference of
   tests/_mlpbwdref.py (B: the sum of the absolute terms of the entry).  On every case of the sweep -- the tile-loop cases at the sizes an
   MI355X's 256 CUs give them -- plain fp32 torch.autograd on the CPU stays within HALF of it; a correct fp32 kernel has the other half for
   its own summation order.  G is fixed here from these numbers (profiles/mlp_bwd_errors.json, "fp32_torch") and nowhere else; it is never
   adjusted from a kernel's output.  If a seed fails here, the seed changes (_mlpbwdref.SEEDS).
2. The ReLU kink: fewer than 10 % of the draws of every case are rejected.
3. The inputs are what they say: deterministic, fold tables all-ones or e0 in every row, fp16 tables equal to their own rounding.
4. The kernels' shape tables, restated in Python, and the host's launch plan (rnad_mlp_backward_plan answers without a device).
5. The gate sees what it is there for, by emulation in fp64: a dropped left-over feature column, `rest = db0` in the fold's reduction, one
   sample of 203 left out, an fp16 table read without its rounding -- each costs more than 2 G in the tensor it touches."""
import json
import os

import numpy as np
import pytest
import torch

import _mlpbwdref as mr

# The smallest power of two with plain fp32 torch inside G / 2 on every tensor of every case: the worst is 5.76 units of 2^-24 B
# (value_fc0.weight of the cancelling fold at A = 7, width 64, 203 rows; 3.94 without the cancelling cases: the fold at A = 4), so G / 2 = 4
# is too small; the tile-loop cases (10 251 - 81 931 rows) use at most 0.27 - 0.70.
G = 16.0

ALL_CASES = mr.sweep_cases() + mr.width_cases() + mr.size_cases() + mr.row_list_cases() + mr.loop_cases()
FP32_TORCH = {}


@pytest.fixture(scope="module", autouse=True)
def _log_fp32_torch_figures():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")  # the directory the figures of a run are kept in, if any
    if FP32_TORCH and os.path.isdir(out):
        with open(os.path.join(out, "mlp_bwd_errors_fp32_torch.json"), "w") as f:
            json.dump(FP32_TORCH, f, indent=1, sort_keys=True)


def worst_shares(got, c, grads=None, bounds=None):
    """{tensor: largest |got - want| in units of 2^-24 B} against the case's reference (no assertion)."""
    grads, bounds = grads or c.grads, bounds or c.bounds
    return {k: float(mr.share(g, want, B).max()) for k, g, want, B in zip(mr.KEYS, got, grads, bounds)}


# ------------------------------------------------------------------------------------------------ 1 - 3. the inputs and G
def test_the_case_lists_are_what_the_sweep_says():
    assert len(mr.sweep_cases()) == 30 + 3 and len(set(ALL_CASES)) == len(ALL_CASES)
    assert {(v, A) for v, A, *_ in mr.sweep_cases()} == {("plain", A) for A in range(1, 9)} | {("fold", A) for A in range(2, 9)} \
        | {("cancel", A) for A in (2, 4, 7)}
    assert mr.N_SWEEP == 6 * 32 + 11 and (mr.N_SWEEP + 31) // 32 == 7 < 16
    assert [min(256, (n + 31) // 32) for n in mr.SIZES] == [1, 1, 1, 2, 16, 16, 17, 33], "partial rows of the size cases: 1, 15 .. 17, 33 slices' worth"
    assert {n % 32 for n in mr.LIST_LENGTHS} >= {0, 1, 31} and max(mr.LIST_LENGTHS) < mr.TABLE_ROWS
    for key in mr.loop_cases():
        v, A, W, N, half = key
        p = mr.loop_properties(N, mr.LOOP_GRID_256[(v, A, W)])
        assert p == dict(rounds=3, partial_round=True, partial_tile=True) and N <= mr.MAX_LOOP_ROWS, key
        assert mr.loop_list_length(N) % 32 != 0


@pytest.mark.parametrize("key", ALL_CASES, ids=mr.case_id)
def test_fp32_torch_uses_at_most_half_of_the_gate(key):
    c = mr.case(*key)
    v, A, W, N, half = key
    assert c.rejected < 0.10, f"{key}: {c.rejected:.1%} of the draws sit on a ReLU kink: change the seed (_mlpbwdref.SEEDS)"
    assert c.obs.shape == (N, 2, A, A) and c.obs.dtype == (torch.float16 if half else torch.float32)
    assert c.dlogits.shape == (N, A) and c.dvalue.shape == (N, 1) and [tuple(w.shape) for w in c.weights] == \
        [(W, 2 * A * A), (W,), (1, W), (1,), (W, 2 * A * A), (W,), (A, W), (A,)]
    legal = c.obs[:, 1].reshape(N, -1).float()
    assert ((legal == 0) | (legal == 1)).all() and (legal[:, 0] == 1).all()
    ev = c.obs[:, 0].float()
    assert float(ev.abs().max()) <= 1 and (not half or torch.equal(c.obs, c.obs.float().half())), "fp16 tables equal their own rounding"
    if half:
        assert not torch.equal(ev.reshape(N, -1), c.ev_unrounded), "the rounding to fp16 changes the ev plane"
    if c.fold:
        e0 = torch.zeros(A * A)
        e0[0] = 1.0
        assert ((legal == 1).all(1) ^ (legal == e0).all(1)).all(), "every row of a fold table is all ones or e0"
        assert torch.equal((legal == e0).all(1), c.absorbing)
        rows = c.absorbing
        if N >= mr.N_SWEEP:
            share = float(rows.float().mean())
            assert (0.01 < share < 0.12) if v == "fold" else (0.4 < share < 0.6), share
        assert (c.dvalue[rows] != 0).all() and (c.dlogits[rows] != 0).all() and (ev[rows] != 0).all(), "absorbing rows keep their gradients"
    else:
        assert c.absorbing is None and 0.3 < float(legal[:, 1:].mean()) < 0.7 if A > 1 and N >= mr.N_SWEEP else True
    if N >= mr.N_SWEEP:  # about 30 % of the rows that are not absorbing carry no policy gradient
        others = ~c.absorbing if c.fold else torch.ones(N, dtype=torch.bool)
        assert 0.15 < float((c.dlogits[others] == 0).all(1).float().mean()) < 0.45 and (c.dvalue != 0).all()
    used = mr.gate_all(mr.fp32_torch(c), c.grads, c.bounds, G / 2, f"fp32 torch {mr.case_id(key)}")
    FP32_TORCH[mr.case_id(key)] = dict(rejected=round(c.rejected, 5), **{k: round(u, 4) for k, u in used.items()})
    print(mr.case_id(key), "rejected %.3f %%" % (100 * c.rejected), "fp32 torch, units of 2^-24 B:", {k: round(u, 2) for k, u in used.items()})


def test_the_cases_are_deterministic():
    for key in (("plain", 3, 64, 203, False), ("fold", 4, 64, 203, True), ("cancel", 7, 64, 203, False)):
        a = mr.case(*key)
        mr.case.cache_clear()
        b = mr.case(*key)
        assert a is not b
        assert all(torch.equal(x, y) for x, y in zip(a.weights, b.weights))
        assert torch.equal(a.obs, b.obs) and torch.equal(a.dlogits, b.dlogits) and torch.equal(a.dvalue, b.dvalue)
        assert all(np.array_equal(x, y) for x, y in zip(a.grads + a.bounds, b.grads + b.bounds))
    assert torch.equal(mr.shuffled(600, 3), mr.shuffled(600, 3)) and not torch.equal(mr.shuffled(600, 3), torch.arange(600, dtype=torch.int32))


def test_the_reference_of_a_row_list_is_the_reference_of_those_rows():
    c = mr.case("fold", 4, 64, mr.TABLE_ROWS, True)
    order = mr.shuffled(c.N, 1).long()
    g_all, b_all = mr.reference(c, order)
    for a, b in zip(g_all + b_all, c.grads + c.bounds):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)  # every row, another order: fp64 rounding only
    g0, b0 = mr.reference(c, order[:0])
    assert all((a == 0).all() for a in g0 + b0), "an empty list has zero gradients and zero bounds: the gate then asks for exact zeros"
    g33, _ = mr.reference(c, order[:33])
    poisoned = c.obs.clone()
    listed = torch.zeros(c.N, dtype=torch.bool)
    listed[order[:33]] = True
    poisoned[~listed] = mr.POISON[torch.float16]
    assert all(np.array_equal(a, b) for a, b in zip(g33, mr.reference(c, order[:33], obs=poisoned)[0])), "rows that are not listed are not read"


# ------------------------------------------------------------------------------------------------ 4. shape tables and the launch plan
def test_shape_tables_restate_the_kernels():
    assert [(s.N16, s.LO) for s in (mr.shape(A, False) for A in range(1, 9))] == [(0, 3), (1, 0), (1, 3), (2, 1), (3, 3), (5, 0), (6, 3), (8, 1)]
    assert [(s.N16, s.LO) for s in (mr.shape(A, True) for A in range(2, 9))] == [(1, 0), (1, 0), (1, 3), (2, 0), (3, 0), (3, 3), (4, 3)]
    assert [mr.shape(A, False).K for A in range(1, 9)] == [2, 8, 18, 32, 50, 72, 98, 128]
    assert [mr.shape(A, True).K for A in range(2, 9)] == [6, 10, 18, 26, 38, 50, 66]
    assert [mr.shape(A, False).KQ for A in range(1, 9)] == [1, 2, 5, 8, 13, 18, 25, 32]
    assert [mr.shape(A, True).KQ for A in range(2, 9)] == [2, 3, 5, 7, 10, 13, 17]
    assert [mr.shape(A, False).XS for A in range(1, 9)] == [5, 17, 21, 37, 53, 81, 101, 133]   # bwd_stage_stride
    assert [mr.shape(A, True).XS for A in range(2, 9)] == [17, 17, 21, 33, 49, 53, 69]
    assert [mr.shape(A, False).FW for A in range(1, 9)] == [4, 12, 20, 64, 64, 96, 128, 160]   # bwd_feature_stride
    assert [mr.shape(A, True).FW for A in range(2, 9)] == [8, 12, 20, 28, 64, 64, 96]
    for fold in (False, True):
        for A in range(2 if fold else 1, 9):
            s = mr.shape(A, fold)
            assert s.XS % 2 == 1 and s.XS >= 4 * s.KQ and s.XS >= s.K + 1 and s.FW >= s.K + 1 and s.FW % 4 == 0
            assert 16 * s.N16 + s.LO >= s.K + 1 > 16 * s.N16 + s.LO - (16 if s.LO == 0 else 1), "the feature tiles cover x and the bias column exactly"
    assert [mr.resident_launch(W) for W in (32, 64, 96, 128, 160, 192, 256, 512)] == \
        [(1, 1), (2, 1), (1, 3), (4, 1), (1, 5), (2, 3), (4, 2), (4, 4)]
    assert {mr.resident_launch(W)[0] for W in mr.WIDTHS} == {1, 2, 4} and {mr.resident_launch(W)[1] for W in mr.WIDTHS} == {1, 2, 3, 5}


def test_the_plan_export_answers_without_a_device():
    """rnad_mlp_backward_plan is host code: without a device it assumes 256 CUs and, the occupancy query failing, one resident workgroup
    per CU; with one it reports that device's launch.  Either way the grid covers the tiles or fills the device, and the workspace holds
    one row of partials (2 W FW + W + A W + 1 + A floats, rounded up to four) per workgroup."""
    import rnad_hip

    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    for fold in (False, True):
        for A in range(2 if fold else 1, 9):
            for W in (32, 64, 96, 128, 160, 192, 256, 512):
                for N in (1, 203, 10**6):
                    p = rnad_hip.mlp_backward_plan(N, A, W, fold)
                    assert p.waves * p.groups == W // 32 and 1 <= p.grid_x <= (N + 31) // 32, (A, W, N, fold, vars(p))
                    if p.resident:
                        assert (p.waves, p.groups) == mr.resident_launch(W)
                    assert fold <= p.resident, "the fold exists in the register-resident kernel only"
                    total = 2 * W * mr.shape(A, fold).FW + W + A * W + 1 + A
                    assert rnad_hip.lib().rnad_mlp_backward_workspace(N, A, W) >= 4 * ((total + 3) & ~3) * p.grid_x, \
                        "the workspace holds a row of partials per workgroup"
                    tiles = (N + 31) // 32
                    assert p.grid_x == tiles or (p.grid_x < tiles and p.grid_x * p.groups >= cus - p.groups), "fewer workgroups than tiles only on a full device"
    for A, W, fold in ((0, 64, False), (9, 64, False), (1, 64, True), (3, 48, False), (3, 16, False), (3, 0, True)):
        with pytest.raises(rnad_hip.RnadHipError, match="rnad_mlp_backward_plan"):
            rnad_hip.mlp_backward_plan(203, A, W, fold)
    with pytest.raises(rnad_hip.RnadHipError, match="rnad_mlp_backward_plan"):
        rnad_hip.mlp_backward_plan(0, 3, 64)


# ------------------------------------------------------------------------------------------------ 5. the gate sees a wrong kernel
def fold_reduce(dW0_ev, d_abs, db0, A, rest_is_db0=False):
    """k_mlp_reduce<A, true> in fp64: the gradient of the [W, 2 A^2] first-layer matrix from the folded columns ev | indicator | bias."""
    rest = db0 if rest_is_db0 else db0 - d_abs
    return np.concatenate([dW0_ev, db0[:, None], np.repeat(rest[:, None], A * A - 1, 1)], 1)


def _folded_columns(c):
    """Per head: (dW0 of the ev columns, d_abs, db0) in fp64 -- d_abs, the indicator column, is db0 over the absorbing rows alone."""
    g_abs, _ = mr.reference(c, torch.nonzero(c.absorbing)[:, 0])
    return [(c.grads[4 * hd][:, :c.A * c.A], g_abs[4 * hd + 1], c.grads[4 * hd + 1]) for hd in (0, 1)]


@pytest.mark.parametrize("key", [k for k in mr.sweep_cases() if k[0] != "plain" and not k[4]], ids=mr.case_id)
def test_the_folded_reduction_and_its_rest_term(key):
    """dW_legal[h][0] = db0, dW_legal[h][j >= 1] = db0 - d_abs is exact; `rest = db0` costs more than 2 G in every legal column j >= 1."""
    c = mr.case(*key)
    assert int(c.absorbing.sum()) >= 3
    A = c.A
    for hd, (ev_cols, d_abs, db0) in enumerate(_folded_columns(c)):
        want, B = c.grads[4 * hd], c.bounds[4 * hd]
        np.testing.assert_allclose(fold_reduce(ev_cols, d_abs, db0, A), want, rtol=0, atol=1e-6 * mr.U * B.max())  # fp64 rounding: a millionth of a unit
        s = mr.share(fold_reduce(ev_cols, d_abs, db0, A, rest_is_db0=True), want, B)
        assert s[:, :A * A + 1].max() < 1e-6
        live = c.bounds[4 * hd + 1] > 0  # (a hidden unit that no row switches on has no gradient to get wrong)
        assert live.mean() > 0.5 and s[live][:, A * A + 1:].max() > 2 * G
        print(mr.case_id(key), mr.KEYS[4 * hd], "rest = db0: median %.3g, largest %.3g units" % (np.median(s[live][:, A * A + 1:]), s.max()))
        if key[0] == "cancel":  # db0 - d_abs cancels: the absorbing rows carry most of db0's terms
            assert np.median(np.abs(d_abs[live]) / (np.abs(db0[live] - d_abs[live]) + 1e-300)) > 1


@pytest.mark.parametrize("key", [("plain", 3, 64, 203, False), ("fold", 4, 64, 203, False)], ids=mr.case_id)
def test_the_gate_sees_a_dropped_leftover_column(key):
    """LO = 3 in both: the last left-over feature column (the one a store condition of LO - 1 would lose) is the bias column."""
    c = mr.case(*key)
    s = mr.shape(c.A, c.fold)
    assert s.LO == 3 and 16 * s.N16 + s.LO - 1 == s.K
    got = [g.copy() for g in c.grads]
    for hd in (0, 1):
        got[4 * hd + 1][:] = 0.0
        if c.fold:
            ev_cols, d_abs, _ = _folded_columns(c)[hd]
            got[4 * hd] = fold_reduce(ev_cols, d_abs, got[4 * hd + 1], c.A)
    used = worst_shares(got, c)
    print(mr.case_id(key), {k: "%.3g" % u for k, u in used.items()})
    assert used["value_fc0.bias"] > 2 * G and used["policy_fc0.bias"] > 2 * G
    assert all(used[k] == 0 for k in mr.KEYS if "fc1" in k) and (used["value_fc0.weight"] > 2 * G) == c.fold


@pytest.mark.parametrize("key", [("plain", 3, 64, 203, False), ("fold", 4, 64, 203, True), ("plain", 8, 64, 203, False)], ids=mr.case_id)
def test_the_gate_sees_one_sample_of_203_left_out(key):
    c = mr.case(*key)
    n = int(torch.nonzero((c.dlogits != 0).all(1))[-1])  # the last row that carries a policy gradient
    rows = [r for r in range(c.N) if r != n]
    used = worst_shares(mr.reference(c, rows)[0], c)
    print(mr.case_id(key), "row", n, "left out:", {k: "%.3g" % u for k, u in used.items()})
    assert all(u > 2 * G for u in used.values()), used


@pytest.mark.parametrize("key", [k for k in mr.sweep_cases() if k[4]], ids=mr.case_id)
def test_the_gate_sees_an_fp16_table_read_without_its_rounding(key):
    c = mr.case(*key)
    table = torch.cat([c.ev_unrounded, c.obs[:, 1].reshape(c.N, -1).float()], 1).reshape(c.N, 2, c.A, c.A)
    used = worst_shares(mr.reference(c, obs=table)[0], c)
    print(mr.case_id(key), "unrounded ev:", {k: "%.3g" % u for k, u in used.items()})
    assert used["value_fc0.weight"] > 2 * G and used["policy_fc0.weight"] > 2 * G
