"""The MLP forward (csrc/mlp_fwd.hip: k_mlp_forward<A, ObsT, HEADS, FOLD>, k_mlp_pack and the host's launch plan) against an fp64 evaluation of
the net, over every instantiation, net sets, row lists and through the span loop.

tests/test_hip_parity.py compares five plain shapes with the fp32 C oracle under atol = rtol = 1e-5; tests/test_hip_ragged.py, test_hip_fold.py
and test_hip_rows.py compare this kernel with itself or with a sibling that shares its packing, weight image and fold.  Here the reference is
tests/_mlpfwdref.py (the unfolded net in double precision), and the gate is |got - want| <= G 2^-24 B per row and output (B: the sum of the
absolute terms; G from tests/test_mlp_fwd_shapes.py, where plain fp32 torch uses at most half of it).  Every output table starts as the
sentinel 7.0; under a row list the observations of the rows that are not listed hold a large finite poison (mlp_fwd.o is built with
-fno-honor-nans).

  a. every instantiation at 203 rows: A = 1 .. 8 plain and A = 2 .. 8 folded, fp32 and fp16 tables, value only / logits only / both
     (HEADS = 1, 2, 3) -- all 90 that exist -- in both input families; widths 32 .. 512 and the largest widths that fit the 160 KiB LDS
     (images beyond 64 KiB raise the kernel's dynamic LDS limit);
  b. 1 .. 513 rows at width 32: partial and empty sample tiles, a lone span, one and several workgroups; N = 0 writes nothing;
  c. net sets: 1 .. 4 nets of distinct weights in one launch, heads wanted in patterns whose union is 1, 2 and 3 and in which nets skip a
     head the launch is instantiated for; one and three workgroups per net; a net that wants nothing is refused;
  d. shuffled row lists of 0 .. 257 rows and the whole table of 600, one net and four: the other rows of every output keep the sentinel;
  e. the span loop: 1.5 or 2.5 rounds of spans over the grid THIS machine is given (rnad_mlp_forward_plan with its CU count), a last span of
     11 samples, the whole table and a shuffled list, at A = 3 also a 2-net set; each launch twice with identical bits.  No case has more
     than 180 000 rows at A >= 4 or 300 000 at A = 3 (DESIGN.md "Known and not diagnosed");
  f. the actor epilogue of k_mlp_forward itself (RNAD_ROWS_ACTOR=0) on small trees, A = 1 .. 5 and 8: logits inside the gate, policy rows
     the policy head of the kernel's own logits bit for bit, pad columns zero, rows that are not listed untouched;
  g. k_mlp_pack, plain and fold, 1 and 4 nets, against the layout as tests/_mlpfwdref.image states it, bit for bit;
  h. the refusals, on real device tensors: nothing is written.

The worst share of the gate per case and output goes to mlp_fwd_errors.json in the directory that RNAD_ERRORS_DIR names, when it is set;
profiles/mlp_fwd_errors.json holds the figures of an MI355X."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import _mlpfwdref as mf
from test_mlp_fwd_shapes import G

pytestmark = pytest.mark.gpu

SENTINEL = mf.SENTINEL
I32 = torch.int32
HEADS = {1: (False, True), 2: (True, False), 3: (True, True)}  # HEADS of the instantiation -> (logits, value) wanted


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    mf.SHARES.clear()
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if mf.SHARES and os.path.isdir(out):
        with open(os.path.join(out, "mlp_fwd_errors.json"), "w") as f:
            json.dump(mf.SHARES, f, indent=1, sort_keys=True)


def _hip():
    import rnad_hip

    return rnad_hip


def _cus():
    from _gpu import DEV

    return torch.cuda.get_device_properties(DEV).multi_processor_count


@functools.lru_cache(maxsize=None)
def _device(key, n_nets=1):
    """A case of tests/_mlpfwdref.py on the device, with the weight images of its first n_nets nets."""
    from _gpu import DEV

    hip = _hip()
    c = mf.case(*key)
    w = [[t.to(DEV).contiguous() for t in ws] for ws in c.weights[:n_nets]]
    if c.fold and n_nets == 1:
        packed = [mf.pack_fold(hip, w[0], c.A)]
    else:
        packed = hip.mlp_pack_many(w, c.A, fold=c.fold)
    assert all(p.numel() == hip.mlp_packed_size(c.A, c.W, fold=c.fold) == mf.image_floats(c.A, c.W, c.fold) for p in packed)
    return types.SimpleNamespace(c=c, packed=packed, obs=c.obs.to(DEV))


def _outputs(N, A, wants):
    """Sentinel-filled tables for the heads that are wanted, None for the others."""
    from _gpu import DEV

    return [(torch.full((N, A), SENTINEL, device=DEV) if wl else None, torch.full((N, 1), SENTINEL, device=DEV) if wv else None) for wl, wv in wants]


def _launch(d, wants, live=None, obs=None, capacity=None):
    """One launch of the first len(wants) nets into sentinel-filled tables -> [(logits or None, value or None)].  Plain cases go through
    rnad_mlp_forward (one net), rnad_mlp_forward_rows (one net, a row list) or rnad_mlp_forward_multi; fold cases through
    rnad_mlp_forward_fold."""
    hip, c = _hip(), d.c
    obs = d.obs if obs is None else obs
    outs = _outputs(c.N, c.A, wants)
    packed = d.packed[:len(wants)]
    assert len(packed) == len(wants)
    if c.fold:
        mf.forward_fold(hip, packed, obs, c.A, c.W, outs, live=live, capacity=capacity)
    elif len(wants) == 1:
        assert capacity is None
        got = hip.mlp_forward(packed[0], c.W, obs, c.A, live=live, out=outs[0])
        assert got[0] is outs[0][0] and got[1] is outs[0][1], "out= tables are the ones written"
    else:
        assert live is None and capacity is None
        got = hip.mlp_forward_multi(packed, c.W, obs, c.A, None, out=outs)
        assert all(g[0] is o[0] and g[1] is o[1] for g, o in zip(got, outs)), "out= tables are the ones written"
    return outs


def _check(d, outs, what, detail, listed=None):
    """Every table that was handed in is inside the gate on the listed rows (None: all) and keeps the sentinel elsewhere."""
    c = d.c
    sel = None if listed is None else listed.cpu().numpy()
    used = {}
    for i, (logits, value) in enumerate(outs):
        for t in (logits, value):
            if t is not None and listed is not None:
                assert (t[~listed] == SENTINEL).all(), f"{what} {detail}: net {i} wrote a row that is not listed"
        u = mf.gate_outputs(None if logits is None else logits.cpu().numpy(), None if value is None else value.cpu().numpy(), c.ref(i), G, what,
                            rows=sel, detail=f"{detail} net {i}")
        used.update({f"{k}{i}": round(v, 2) for k, v in u.items()})
    print(what, detail, "-> units of 2^-24 B:", used)
    return used


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for name, s, t in zip(("logits", "value"), x, y):
            assert (s is None) == (t is None)
            assert s is None or torch.equal(s.view(I32), t.view(I32)), f"{what}: two launches differ in the {name} of net {i}"


def _row_list(N, order, n):
    """The first n entries of `order` as a row list in the shape of a LiveRows (all N entries in the buffer, the count in device memory)
    -> (list, bool mask of the listed rows)."""
    from _gpu import DEV

    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[order[:n].to(DEV).long()] = True
    assert order.numel() == N and int(listed.sum()) == n, "a row list names every row once"
    live = _hip().RowList(order, N, DEV)
    live.count.fill_(n)
    return live, listed


def _poisoned(obs, listed):
    table = obs.clone()
    table[~listed] = mf.POISON[table.dtype]
    return table


# ------------------------------------------------------------------------------------------------ a. every instantiation
@pytest.mark.parametrize("key", mf.sweep_cases() + mf.width_cases() + mf.largest_cases(), ids=mf.case_id)
def test_every_instantiation(key):
    d = _device(key)
    p = _hip().mlp_forward_plan(key[3], key[1], key[2], d.c.fold, 1, _cus())
    assert (p.per_net, p.rounds) == (1, 1), "203 rows: four spans, one workgroup"
    for heads, wants in HEADS.items():
        outs = _launch(d, [wants])
        assert [t is not None for t in outs[0]] == list(wants), "a head that is not wanted has no table"
        _check(d, outs, f"a {mf.case_id(key)}", f"HEADS={heads}")


# ------------------------------------------------------------------------------------------------ b. sizes
@pytest.mark.parametrize("key", mf.size_cases(), ids=mf.case_id)
def test_sizes(key):
    d = _device(key)
    N = key[3]
    assert _hip().mlp_forward_plan(N, key[1], key[2], d.c.fold, 1, _cus()).per_net == (N + 255) // 256
    _check(d, _launch(d, [(True, True)]), f"b {mf.case_id(key)}", "both heads")


@pytest.mark.parametrize("key", [k for k in mf.size_cases() if k[3] == 65], ids=mf.case_id)
def test_no_rows_write_nothing(key):
    hip, d = _hip(), _device(key)
    c = d.c
    (logits, value), = _outputs(c.N, c.A, [(True, True)])
    stream = torch.cuda.current_stream().cuda_stream
    if c.fold:
        P, L, V = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in (d.packed[0], logits, value)]
        rc = hip.lib().rnad_mlp_forward_fold(1, 0, None, None, c.A, c.W, P, d.obs.data_ptr(), 0, L, V, stream)
    else:
        rc = hip.lib().rnad_mlp_forward(0, c.A, c.W, d.packed[0].data_ptr(), d.obs.data_ptr(), 0, logits.data_ptr(), value.data_ptr(), stream)
    assert rc == 0, hip.lib().rnad_last_error().decode()
    torch.cuda.synchronize()
    assert (logits == SENTINEL).all() and (value == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ c. net sets
T, F = True, False
WANT_PATTERNS = (  # per net (logits, value)
    [(T, T)], [(F, T)], [(T, F)],
    [(T, T), (F, T)], [(F, T), (F, T)], [(T, F), (T, F)], [(T, F), (F, T)],
    [(T, T), (F, T), (T, F)], [(F, T), (T, F), (T, T)],
    [(T, T), (F, T), (T, F), (T, F)], [(F, T), (F, T), (F, T), (F, T)], [(T, F), (T, F), (T, F), (T, F)], [(F, T), (T, F), (F, T), (T, F)],
)
NET_SET_TABLES = mf.net_set_cases() + [k for k in mf.size_cases() if k[3] == 513]  # 203 rows: one workgroup per net; 513: three


def test_the_want_patterns_cover_what_they_should():
    union = lambda p: (1 if any(v for _, v in p) else 0) | (2 if any(lg for lg, _ in p) else 0)  # noqa: E731
    skips = lambda p: any((union(p) & 2 and not lg) or (union(p) & 1 and not v) for lg, v in p)  # noqa: E731
    assert {(len(p), union(p)) for p in WANT_PATTERNS} >= {(n, u) for n in (1, 2, 4) for u in (1, 2, 3)} | {(3, 3)}
    assert all(any(len(p) == n and skips(p) for p in WANT_PATTERNS) for n in (2, 3, 4))
    assert [(T, T), (F, T), (T, F), (T, F)] in WANT_PATTERNS


@pytest.mark.parametrize("key", NET_SET_TABLES, ids=mf.case_id)
def test_net_sets(key):
    hip, d = _hip(), _device(key, 4)
    c = d.c
    assert hip.mlp_forward_plan(c.N, c.A, c.W, c.fold, 4, _cus()).per_net == (1 if c.N == 203 else 3)
    for wants in WANT_PATTERNS:
        outs = _launch(d, wants)
        assert [(lg is not None, v is not None) for lg, v in outs] == list(wants)
        _check(d, outs, f"c {mf.case_id(key)}", "wants " + " ".join(("L" if lg else "") + ("V" if v else "") for lg, v in wants))
    # every net's output is that net's function: the gate above rejects any other net's (tests/test_mlp_fwd_shapes.py, mutation iv)
    for wants in ([(T, T), (F, F)], [(F, F)], [(T, F), (F, T), (F, F), (T, T)]):
        with pytest.raises(hip.RnadHipError, match="wants no output|null argument"):
            if c.fold:
                _launch(d, wants)
            else:
                hip.mlp_forward_multi(d.packed[:len(wants)], c.W, d.obs, c.A, None, out=_outputs(c.N, c.A, wants))


# ------------------------------------------------------------------------------------------------ d. row lists
@pytest.mark.parametrize("key", mf.row_list_cases(), ids=mf.case_id)
def test_row_lists(key):
    n_nets = mf.row_list_nets(key)
    d = _device(key, n_nets)
    c = d.c
    assert c.N == mf.TABLE_ROWS and (n_nets == 1 or c.fold)
    order = mf.shuffled(c.N, 100 * c.A)
    assert not torch.equal(order, torch.sort(order).values)
    wants = [(T, T)] if n_nets == 1 else [(T, T), (F, T), (T, F), (T, F)]
    for n in mf.LIST_LENGTHS + (c.N,):
        live, listed = _row_list(c.N, order, n)
        table = _poisoned(d.obs, listed)
        first = _launch(d, wants, live=live, obs=table)
        if n == 0:
            assert all((t == SENTINEL).all() for o in first for t in o if t is not None), "an empty list writes nothing"
        _check(d, first, f"d {mf.case_id(key)}", f"{n_nets} nets, {n} rows", listed)
        _same_bits(first, _launch(d, wants, live=live, obs=table), f"{mf.case_id(key)} {n} rows")


# ------------------------------------------------------------------------------------------------ e. the span loop
def _loop_id(shape):
    v, A, W, half = shape
    return f"{v}_A{A}_W{W}_{'fp16' if half else 'fp32'}"


@pytest.mark.parametrize("shape", mf.LOOP_SHAPES, ids=_loop_id)
def test_span_loop(shape):
    hip, cus = _hip(), _cus()
    cases, over = mf.loop_cases(cus)
    left_out = dict(over)
    if shape in left_out:
        pytest.skip(f"{cus} CUs ask for {left_out[shape]} rows, above the limit of {mf.max_rows(shape[1])} at A = {shape[1]}")
    key = next(k for k in cases if (k[0], k[1], k[2], k[4]) == shape)
    v, A, W, N, half, _ = key
    fold = v == "fold"
    n = mf.loop_list_length(N)
    sets = [[(T, T)]] + ([[(T, T), (F, T)]] if A == 3 else [])
    for wants in sets:
        for count in (None, n):
            p = mf.plan_properties(N, A, W, fold, len(wants), cus, count)
            assert p["rounds"] >= 2 and p["uneven"] and p["partial_span"], (key, cus, count, p)
        assert hip.mlp_forward_plan(N, A, W, fold, len(wants), cus).rounds == mf.plan(N, A, W, fold, len(wants), cus).rounds >= 2
    d = _device(key, len(sets[-1]))
    live, listed = _row_list(N, mf.shuffled(N, 7 * A), n)
    table = _poisoned(d.obs, listed)
    for wants in sets:
        what = f"e {mf.case_id(key)}"
        first = _launch(d, wants)
        _same_bits(first, _launch(d, wants), f"{what} {len(wants)} nets")
        _check(d, first, what, f"{len(wants)} nets, all rows")
        if fold or len(wants) == 1:  # (the plain multi-net entry point takes no row list)
            first = _launch(d, wants, live=live, obs=table)
            _same_bits(first, _launch(d, wants, live=live, obs=table), f"{what} {len(wants)} nets, {n} rows")
            _check(d, first, what, f"{len(wants)} nets, {n} rows", listed)


# ------------------------------------------------------------------------------------------------ f. the actor epilogue
@functools.lru_cache(maxsize=None)
def _tree(A):
    from test_hip_bucket import _native_tree

    tree = _native_tree(**mf.ACTOR_TREES[A])
    h = tree.handle()
    assert h.legal_foldable == (A >= 2), "every tree of the sweep is foldable"
    return tree, h


@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("A", sorted(mf.ACTOR_TREES))
def test_actor_epilogue(A, half, monkeypatch):
    from _gpu import DEV

    monkeypatch.setenv("RNAD_ROWS_ACTOR", "0")  # k_mlp_forward's own epilogue, not csrc/mlp_rows.hip's
    hip = _hip()
    case = mf.actor_case(A, half)
    _, h = _tree(A)
    N, W = case.N, case.W
    assert N == 2 * h.S < 2000
    table = h.observations_table(half)
    own = table.clone()
    assert torch.equal(own.cpu(), case.obs), "the host's observation table is the device's"
    weights = [w.detach().to(DEV).contiguous() for w in case.net._weights()]
    stride = int(hip.lib().rnad_bucket_policy_row_stride(A))
    assert stride == (A + 3) // 4 * 4
    mask = case.mask.to(DEV)
    order = mf.shuffled(N, 11 * A)
    try:
        for fold in ((False, True) if A >= 2 else (False,)):
            packed = hip.mlp_pack_many([weights], A, fold=fold)[0]
            for n in (None, 0, 1, min(33, N - 5), N - 3):
                live, listed = (None, None) if n is None else _row_list(N, order, n)
                table.copy_(own if listed is None else _poisoned(own, listed))
                logits, rows = torch.full((N, A), SENTINEL, device=DEV), torch.full((N, stride), SENTINEL, device=DEV)
                hip.mlp_forward_actor(h, packed, W, table, logits, rows, rows=live, fold=h if fold else False)
                what = f"f actor_A{A}_W{W}_N{N}_{'fp16' if half else 'fp32'}"
                detail = f"fold={fold} rows={'all' if n is None else n}"
                L = slice(None) if listed is None else listed
                if listed is not None:
                    assert (logits[~listed] == SENTINEL).all() and (rows[~listed] == SENTINEL).all(), f"{what} {detail}: a row that is not listed was written"
                used = mf.gate_outputs(logits.cpu().numpy(), None, case.ref, G, what, rows=None if listed is None else listed.cpu().numpy(), detail=detail)
                want = hip.policy_head(logits, mask=mask)
                assert torch.equal(rows[L][:, :A].view(I32), want[L].view(I32)), f"{what} {detail}: policy rows are the policy head of the kernel's own logits"
                assert (rows[L][:, A:] == 0).all(), f"{what} {detail}: pad columns are zeros"
                print(what, detail, "-> units of 2^-24 B:", used)
    finally:
        table.copy_(own)


# ------------------------------------------------------------------------------------------------ g. pack
@pytest.mark.parametrize("fold", (False, True), ids=("plain", "fold"))
@pytest.mark.parametrize("n_nets", (1, 4))
def test_pack_writes_the_layout_the_header_describes(n_nets, fold):
    from _gpu import DEV

    hip = _hip()
    for A in range(2 if fold else 1, 9):
        for W in (32, 96, 256):
            if mf.image_floats(A, W, fold) > mf.LDS_FLOATS:
                continue
            per_net = sum(w.numel() for w in mf.integer_weights(A, W))
            host = [mf.integer_weights(A, W, base=i * per_net) for i in range(n_nets)]
            outs = [torch.full((hip.mlp_packed_size(A, W, fold=fold),), SENTINEL, device=DEV) for _ in range(n_nets)]
            got = hip.mlp_pack_many([[w.to(DEV) for w in ws] for ws in host], A, out=outs, fold=fold)
            for i in range(n_nets):
                want = mf.image(host[i], A, fold)
                assert np.array_equal(got[i].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"A={A} W={W} fold={fold}: image of net {i} of {n_nets}"


# ------------------------------------------------------------------------------------------------ h. refusals
@pytest.mark.parametrize("A,W,fold,reason", [(A, W, f, "do not fit") for A, W in mf.TOO_LARGE for f in (False, True)]
                         + [(3, 48, False, "multiple of 32"), (4, 48, True, "multiple of 32"), (1, 64, True, "at least two actions")])
def test_refusals_write_nothing(A, W, fold, reason):
    from _gpu import DEV

    hip = _hip()
    N = 65
    assert mf.plan(N, A, W, fold, 1, _cus()) is None
    obs = torch.zeros((N, 2, A, A), device=DEV)
    packed = torch.zeros((mf.image_floats(A, W, fold),), device=DEV)
    (logits, value), = outs = _outputs(N, A, [(T, T)])
    with pytest.raises(hip.RnadHipError, match=reason):
        if fold:
            mf.forward_fold(hip, [packed], obs, A, W, outs)
        else:
            hip.mlp_forward(packed, W, obs, A, out=outs[0])
    live, _ = _row_list(N, mf.shuffled(N, 1), 33)
    with pytest.raises(hip.RnadHipError, match=reason):
        if fold:
            mf.forward_fold(hip, [packed], obs, A, W, outs, live=live)
        else:
            hip.mlp_forward(packed, W, obs, A, live=live, out=outs[0])
    torch.cuda.synchronize()
    assert (logits == SENTINEL).all() and (value == SENTINEL).all()
