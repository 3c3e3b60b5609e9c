"""What the GPU sweep of the MLP forward (tests/test_hip_mlp_fwd_shapes.py on csrc/mlp_fwd.hip) stands on, checked without a GPU.

1. G.  The gate of the sweep is |got - want| <= G * 2^-24 * B per row and output against the fp64 reference of tests/_rowsref.py (B: the sum
   of the absolute terms, the legal plane counted as ones).  On every case of every list -- the span-loop cases at the sizes an MI355X's
   256 CUs give them -- plain fp32 torch on the CPU stays within HALF of it; a correct fp32 kernel has the other half for its own summation
   order.  G is fixed here from these numbers and nowhere else; it is never adjusted from a kernel's output.
2. The inputs are what they say: deterministic, fold tables all ones or e0 in every row, fp16 tables equal to their own rounding.
3. The gate sees a wrong kernel, by emulation in fp64: the last input feature's product dropped from the first layer, the fold's indicator
   column ignored, an fp16 table read without its rounding, another net's outputs in a 4-net set -- each costs more than 2 G.
4. The launch arithmetic (_mlpfwdref.plan) and the weight image (_mlpfwdref.image), restated in Python, against the library's host exports
   rnad_mlp_forward_plan, rnad_mlp_packed_size and rnad_mlp_fold_packed_size (the library loads without a device), and the sizes of the
   sweep keep the properties they were chosen for."""
import json
import os

import numpy as np
import pytest
import torch

import _mlpfwdref as mf

# The smallest power of two with plain fp32 torch inside G / 2 on both outputs of every case: the worst is 2.75 units of 2^-24 B (v of the
# span-loop case plain, A = 3, width 512, 163 851 rows, "wide"; the other span-loop cases 1.97 - 2.64, all on v, where the sums along the
# sign-aligned path do not cancel), so G / 2 = 2 is too small.  The 203-row "wide" cases use up to 1.72, the "init" family at most 0.34
# (profiles/mlp_fwd_errors.json, "fp32_torch").  The same G as the rows sweep has for the same function (tests/test_rows_shapes.py).
G = 8.0

CUS = 256  # an MI355X
LOOP_256, LOOP_OVER_256 = mf.loop_cases(CUS)
ALL_CASES = mf.sweep_cases() + mf.width_cases() + mf.largest_cases() + mf.size_cases() + mf.row_list_cases() + LOOP_256
FP32_TORCH = {}


@pytest.fixture(scope="module", autouse=True)
def _log_fp32_torch_figures():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")  # the directory the figures of a run are kept in, if any
    if FP32_TORCH and os.path.isdir(out):
        with open(os.path.join(out, "mlp_fwd_errors_fp32_torch.json"), "w") as f:
            json.dump(FP32_TORCH, f, indent=1, sort_keys=True)


def _hip():
    import rnad_hip

    return rnad_hip


def _worst(mutant, ref, rows=None):
    """Largest share of 2^-24 B by which a mutant's (logits, v) miss the reference, over `rows`."""
    sel = slice(None) if rows is None else rows
    return max(float(mf.normalised(mutant.logits[sel], ref.logits[sel], ref.B_logits[sel]).max()),
               float(mf.normalised(mutant.v[sel], ref.v[sel], ref.B_v[sel]).max()))


# ------------------------------------------------------------------------------------------------ 1 - 2. the inputs and G
def test_the_case_lists_are_what_the_sweep_says():
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    sweep = mf.sweep_cases()
    assert len(sweep) == (8 + 7) * 2 * 2
    assert {(v, A) for v, A, *_ in sweep} == {("plain", A) for A in range(1, 9)} | {("fold", A) for A in range(2, 9)}
    assert {(k[4], k[5]) for k in sweep} == {(h, f) for h in (False, True) for f in mf.FAMILIES}
    assert [k[2] for k in mf.width_cases() if k[0] == "plain"] == list(mf.WIDTHS) and [k[2] for k in mf.width_cases() if k[0] == "fold"] == list(mf.WIDTHS)
    assert mf.N_SWEEP == 3 * 64 + 11
    assert {n % 32 for n in mf.LIST_LENGTHS} >= {0, 1, 31} and max(mf.LIST_LENGTHS) < mf.TABLE_ROWS
    # size cases: one workgroup (up to 256 samples) and more than one; partial and empty sample tiles; a lone span
    per_net = [mf.plan(k[3], k[1], k[2], k[0] == "fold", 1, CUS).per_net for k in mf.size_cases() if k[0] == "plain"]
    assert per_net == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3]
    assert {mf.plan(k[3], k[1], k[2], k[0] == "fold", 1, CUS).lds_bytes > 64 * 1024 for k in ALL_CASES} == {False, True}, \
        "images on both sides of 64 KiB, where the launch raises the kernel's dynamic LDS limit"


def test_the_loop_cases_walk_the_span_loop_and_respect_the_row_limits():
    assert not LOOP_OVER_256 and len(LOOP_256) == len(mf.LOOP_SHAPES) == 6
    assert [k[3] for k in LOOP_256] == [294923, 294923, 163851, 163851, 163851, 163851]
    assert [mf.plan(k[3], k[1], k[2], k[0] == "fold", 1, CUS).blocks_per_cu for k in LOOP_256] == [3, 3, 1, 1, 1, 1]
    for cus in (64, 104, 228, 256, 304):
        cases, over = mf.loop_cases(cus)
        assert len(cases) + len(over) == 6
        for v, A, W, N, half, family in cases:
            assert N <= (300_000 if A == 3 else 180_000), "DESIGN.md: known and not diagnosed"
            for n_nets in (1, 2):
                for count in (None, mf.loop_list_length(N)):
                    p = mf.plan_properties(N, A, W, v == "fold", n_nets, cus, count)
                    assert p["rounds"] >= 2 and p["uneven"] and p["partial_span"], (cus, v, A, W, N, count, p)
            assert mf.loop_list_length(N) % 32 != 0 and N % 64 == 11
        for (v, A, W, half), N in over:
            assert N > (300_000 if A == 3 else 180_000)
    # a device of 304 CUs pushes all but one shape over its limit (350 219 rows at A = 3, width 256; 194 571 at A >= 4): the GPU file skips those
    assert [k[:3] for k in mf.loop_cases(304)[0]] == [("plain", 3, 512)] and len(mf.loop_cases(228)[0]) == 6


@pytest.mark.parametrize("key", ALL_CASES, ids=mf.case_id)
def test_fp32_torch_uses_at_most_half_of_the_gate(key):
    c = mf.case(*key)
    v, A, W, N, half, family = key
    assert N <= mf.max_rows(A)
    assert c.obs.shape == (N, 2, A, A) and c.obs.dtype == (torch.float16 if half else torch.float32)
    assert [tuple(w.shape) for w in c.weights[0]] == [(W, 2 * A * A), (W,), (1, W), (1,), (W, 2 * A * A), (W,), (A, W), (A,)]
    legal = c.obs[:, 1].reshape(N, -1).float()
    ev = c.obs[:, 0].reshape(N, -1).float()
    assert ((legal == 0) | (legal == 1)).all() and (legal[:, 0] == 1).all()
    assert float(ev.abs().max()) <= 2 and (ev != 0).all() and (not half or torch.equal(c.obs, c.obs.float().half()))
    if half:
        assert not torch.equal(ev, c.ev_unrounded), "the rounding to fp16 changes the ev plane"
    if c.fold:
        e0 = torch.zeros(A * A)
        e0[0] = 1.0
        assert ((legal == 1).all(1) ^ (legal == e0).all(1)).all(), "every row of a fold table is all ones or e0"
        assert torch.equal((legal == e0).all(1), c.absorbing)
        if N >= mf.N_SWEEP:
            assert 0.01 < float(c.absorbing.float().mean()) < 0.12
    elif A > 1 and N >= mf.N_SWEEP:
        assert c.absorbing is None and 0.3 < float(legal[:, 1:].mean()) < 0.7
    ref = c.ref(0)
    logits, value, _ = mf.fp32_torch(c.nets[0], c.nets[0], c.obs)
    used = mf.gate_outputs(logits, value, ref, G / 2, f"fp32 torch {mf.case_id(key)}")
    mf.SHARES.clear()  # (the GPU file's log; this file keeps its own)
    FP32_TORCH[mf.case_id(key)] = {k: round(u, 4) for k, u in used.items()}
    print(mf.case_id(key), "fp32 torch, units of 2^-24 B:", {k: round(u, 3) for k, u in used.items()})


def test_every_net_of_a_net_set_is_inside_half_of_the_gate():
    for key in mf.net_set_cases() + [k for k in mf.row_list_cases() if mf.row_list_nets(k) == 4]:
        c = mf.case(*key)
        for i in range(4):
            logits, value, _ = mf.fp32_torch(c.nets[i], c.nets[i], c.obs)
            mf.gate_outputs(logits, value, c.ref(i), G / 2, f"fp32 torch {mf.case_id(key)} net {i}")
    mf.SHARES.clear()


def test_the_cases_are_deterministic():
    for key in (("plain", 3, 64, 203, False, "init"), ("fold", 4, 64, 203, True, "wide"), ("fold", 8, 64, 203, False, "init")):
        a = mf.case(*key)
        ra = a.ref(1)
        mf.case.cache_clear()
        b = mf.case(*key)
        assert a is not b and torch.equal(a.obs, b.obs)
        assert all(torch.equal(x, y) for wa, wb in zip(a.weights, b.weights) for x, y in zip(wa, wb))
        rb = b.ref(1)
        assert all(np.array_equal(getattr(ra, k), getattr(rb, k)) for k in ("logits", "v", "B_logits", "B_v"))
    c = mf.case("plain", 3, 64, 203, False, "init")
    assert len({float(w[0].sum()) for w in c.weights}) == 4, "four nets of distinct weights"
    assert torch.equal(mf.shuffled(600, 3), mf.shuffled(600, 3)) and not torch.equal(mf.shuffled(600, 3), torch.arange(600, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the gate sees a wrong kernel
@pytest.mark.parametrize("key", [k for k in mf.sweep_cases() if k[5] == "init"], ids=mf.case_id)
def test_the_gate_sees_a_dropped_input_feature(key):
    """(i) The product of the last feature of the row (legal[A - 1][A - 1]) left out of the first layer, on the rows where it is set."""
    c = mf.case(*key)
    rows = (c.obs.reshape(c.N, -1)[:, -1] == 1).numpy()
    assert rows.sum() >= 50
    table = c.obs.clone()
    table.reshape(c.N, -1)[:, -1] = 0
    mutant = mf.net_reference(c, 0, obs=table)
    ref = c.ref(0)
    per_row = np.maximum(mf.normalised(mutant.logits, ref.logits, ref.B_logits).max(1), mf.normalised(mutant.v, ref.v, ref.B_v))
    print(mf.case_id(key), "last feature dropped: median %.3g, largest %.3g units" % (np.median(per_row[rows]), per_row[rows].max()))
    assert np.median(per_row[rows]) > 2 * G and (per_row[~rows] == 0).all()


@pytest.mark.parametrize("key", [k for k in mf.sweep_cases() if k[0] == "fold"], ids=mf.case_id)
def test_the_gate_sees_an_ignored_indicator_column(key):
    """(ii) The fold without its indicator column evaluates the absorbing rows as if their legal plane were all ones."""
    c = mf.case(*key)
    assert int(c.absorbing.sum()) >= 3
    table = c.obs.clone()
    table[:, 1] = 1
    mutant, ref = mf.net_reference(c, 0, obs=table), c.ref(0)
    rows = c.absorbing.numpy()
    worst = [_worst(mutant, ref, np.array([r])) for r in np.nonzero(rows)[0]]
    print(mf.case_id(key), "indicator ignored: smallest %.3g, largest %.3g units over %d absorbing rows" % (min(worst), max(worst), len(worst)))
    assert min(worst) > 2 * G and _worst(mutant, ref, ~rows) == 0


@pytest.mark.parametrize("key", [k for k in mf.sweep_cases() if k[4]], ids=mf.case_id)
def test_the_gate_sees_an_fp16_table_read_without_its_rounding(key):
    """(iii)"""
    c = mf.case(*key)
    table = torch.cat([c.ev_unrounded, c.obs[:, 1].reshape(c.N, -1).float()], 1).reshape(c.N, 2, c.A, c.A)
    worst = _worst(mf.net_reference(c, 0, obs=table), c.ref(0))
    print(mf.case_id(key), "unrounded ev: %.3g units" % worst)
    assert worst > 2 * G


@pytest.mark.parametrize("key", mf.net_set_cases() + [k for k in mf.row_list_cases() if mf.row_list_nets(k) == 4], ids=mf.case_id)
def test_the_gate_sees_another_nets_outputs(key):
    """(iv) In a 4-net set, net j's logits or value handed out as net i's: more than 2 G for every pair and either output."""
    c = mf.case(*key)
    refs = [c.ref(i) for i in range(4)]
    for i in range(4):
        for j in range(4):
            if i != j:
                assert mf.normalised(refs[j].logits, refs[i].logits, refs[i].B_logits).max() > 2 * G
                assert mf.normalised(refs[j].v, refs[i].v, refs[i].B_v).max() > 2 * G


# ------------------------------------------------------------------------------------------------ 4. restatements and bookkeeping
def _export(N, A, W, fold, n_nets, cus):
    hip = _hip()
    try:
        return hip.mlp_forward_plan(N, A, W, fold, n_nets, cus)
    except hip.RnadHipError:
        return None


def _same_plan(N, A, W, fold, n_nets, cus):
    want, got = mf.plan(N, A, W, fold, n_nets, cus), _export(N, A, W, fold, n_nets, cus)
    assert (want is None) == (got is None), (N, A, W, fold, n_nets, cus)
    if want is not None:
        assert (got.lds_bytes, got.blocks_per_cu, got.per_net, got.rounds) == (want.lds_bytes, want.blocks_per_cu, want.per_net, max(want.spans)), \
            (N, A, W, fold, n_nets, cus, vars(got))
    return got


def test_the_plan_restates_the_export():
    for key in ALL_CASES:
        for n_nets in (1, 4):
            for cus in (64, 256, 304):
                assert _same_plan(key[3], key[1], key[2], key[0] == "fold", n_nets, cus) is not None
    refused = set()
    for A in range(1, 9):
        for W in range(32, 513, 32):
            for fold in (False, True):
                for n_nets in range(1, 5):
                    for cus in (64, 256, 304):
                        for N in (0, 1, 203, 64 * 4 * cus + 1, 163851, 10**6):
                            if _same_plan(N, A, W, fold, n_nets, cus) is None:
                                refused.add((A, W, fold))
    assert {(A, W, f) for (A, W) in mf.TOO_LARGE for f in (False, True)} <= refused and all((1, W, True) in refused for W in (32, 512))
    assert not any((A, W, f) in refused for (A, W) in mf.LARGEST + ((3, 512), (4, 512), (5, 256)) for f in (False, True))


def test_the_refusals_agree_with_the_export():
    hip = _hip()
    for (A, W, fold), reason in ((((6, 288, False), "do not fit"), ((7, 224, False), "do not fit"), ((8, 160, False), "do not fit"),
                                  ((6, 288, True), "do not fit"), ((7, 224, True), "do not fit"), ((8, 160, True), "do not fit"),
                                  ((1, 64, True), "at least two actions"), ((3, 48, False), "multiple of 32"), ((3, 0, False), "multiple of 32"),
                                  ((0, 64, False), "out of range"), ((9, 64, False), "out of range"))):
        assert mf.plan(203, A, W, fold, 1, CUS) is None
        with pytest.raises(hip.RnadHipError, match=reason):
            hip.mlp_forward_plan(203, A, W, fold, 1, CUS)
    for n_nets in (0, 5):
        assert mf.plan(203, 3, 64, False, n_nets, CUS) is None and _export(203, 3, 64, False, n_nets, CUS) is None
    assert mf.plan(-1, 3, 64, False, 1, CUS) is None and _export(-1, 3, 64, False, 1, CUS) is None


def test_the_largest_widths_fit_and_their_neighbours_do_not():
    lib = _hip().lib()
    for (A, W), (plain, fold) in mf.LARGEST_FLOATS.items():
        assert (mf.image_floats(A, W, False), mf.image_floats(A, W, True)) == (plain, fold) and fold <= mf.LDS_FLOATS == 40960
        assert (lib.rnad_mlp_packed_size(A, W), lib.rnad_mlp_fold_packed_size(A, W)) == (plain, fold)
        assert _export(203, A, W, False, 1, CUS).lds_bytes == 4 * plain and _export(203, A, W, True, 1, CUS).lds_bytes == 4 * fold
        assert _export(203, A, W, True, 1, CUS).blocks_per_cu == 1
        assert mf.image_floats(A, W + 32, False) > mf.LDS_FLOATS and mf.image_floats(A, W + 32, True) > mf.LDS_FLOATS
    assert [(A, W + 32) for A, W in mf.LARGEST] == list(mf.TOO_LARGE)
    # blocks_per_cu 3, 2 and 1
    assert [_export(203, A, 256, f, 1, CUS).blocks_per_cu for A, f in ((3, False), (3, True), (4, False), (4, True), (5, False), (5, True))] == \
        [3, 3, 2, 2, 1, 1]


@pytest.mark.parametrize("fold", (False, True), ids=("plain", "fold"))
def test_the_image_holds_every_weight_element_exactly_once(fold):
    lib = _hip().lib()
    for A in range(2 if fold else 1, 9):
        for W in (32, 96, 256):
            if mf.image_floats(A, W, fold) > mf.LDS_FLOATS:
                continue
            weights = mf.integer_weights(A, W)
            n = sum(w.numel() for w in weights)
            img = mf.image(weights, A, fold)
            assert img.dtype == np.float32 and img.size == (lib.rnad_mlp_fold_packed_size if fold else lib.rnad_mlp_packed_size)(A, W) == mf.image_floats(A, W, fold)
            filled = np.sort(img[img != 0])
            assert np.array_equal(filled, np.arange(1, n + 1, dtype=np.float32)), "every element in exactly one slot, the other slots zero"
            # spot checks from the header's own words: W0[hidden][k] of tile 1, k-step 1, half 1, col 5; the biases; the legal columns
            K = ((A * A + 2) & ~1) if fold else 2 * A * A
            vw0, vb0, vw1, vb1, pw0, pb0, pw1, pb1 = [w.numpy() for w in weights]
            if W >= 64 and K >= 4 and A * A > 3:
                assert img[((1 * (K // 2) + 1) * 2 + 1) * 32 + 5] == vw0[32 + 5, 3]
            T = W // 32
            assert img[((T * (K // 2) + 0) * 2 + 0) * 32 + 7] == pw0[7, 0], "tile T is the policy head's first"
            b0 = 2 * W * K
            assert img[b0 + 3] == vb0[3] and img[b0 + W + 3] == pb0[3] and img[b0 + 2 * W + 9] == vw1[0, 9]
            assert img[b0 + 3 * W + (A - 1) * W + 2] == pw1[A - 1, 2]
            b1 = b0 + 3 * W + A * W
            assert img[b1] == vb1[0] and img[b1 + A] == pb1[A - 1] and (img[b1 + 1 + A:b1 + 12] == 0).all()
            if fold:
                assert (img[[((t * (K // 2) + (A * A) // 2) * 2 + (A * A) % 2) * 32 + c for t in range(2 * T) for c in range(32)]] == 0).all(), \
                    "the indicator slot is zero"
                legal = b1 + 12
                assert img[legal + 2 * (2 * W) + 4] == vw0[4, A * A + 2] and img[legal + 1 * (2 * W) + W + 4] == pw0[4, A * A + 1]

