"""csrc/mlp_rows.hip (k_rows_forward_records<A, ObsT, FOLD, MODE, SPLIT>) against an fp64 evaluation of the net, over every instantiation
that can be launched and through the chunk loop.

tests/test_hip_rows.py compares the kernel with k_mlp_forward, which shares its packing, weight image and legal fold, at A in {2, 3, 5},
widths 32 / 64 / 256 and -- but for one case -- one chunk per workgroup.  Here the reference is tests/_rowsref.py: the unfolded net in
double precision, with the gate |got - want| <= G 2^-24 B per row and output (B: the sum of the absolute terms; G from
tests/test_rows_shapes.py, where plain fp32 torch uses at most half of it and a dropped product of the split first layer more than twice).

  a. every instantiation rnad_mlp_rows_records_supported / rnad_mlp_rows_actor_supported / rnad_mlp_rows_uses_split can select: A = 1 .. 5,
     with and without the fold, fp32 and fp16 tables, MODE 0 / 1 / 2, the split first layer off and -- where it can be launched -- on, both
     input families, width 256 and T = 1, 3, 5, 7 compute waves (widths 32, 96, 160, 224) at A = 3 and 5;
  b. row lists of 0 .. 257 rows and the whole table, shuffled, in every MODE: every output table starts as a sentinel and keeps it in the
     rows that are not listed, whose observations carry a large finite poison (mlp_rows.o is built with -fno-honor-nans);
  c. the chunk loop at width 256 on 132 862 - 174 764 rows: both partial-sum / staged-row buffers used again, a short last chunk, a half
     step, a partial last tile -- the properties are asserted for the device's CU count -- each variant twice with identical bits.

Everywhere the records, fast records and policy rows are rnad_bucket_records / rnad_policy_head of the kernel's OWN outputs bit for bit,
and MODE 1 leaves the logit table it is given unchanged.  No case has more than 180 000 rows and none calls rnad_mlp_forward_multi
(DESIGN.md section 7)."""
import functools
import types

import pytest
import torch

import _rowsref as rr
from test_rows_shapes import G

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
I32 = torch.int32
MODES = {0: "records", 1: "records, logits from the table", 2: "actor"}


@functools.lru_cache(maxsize=None)
def _handle(kind, A):
    """The tree of SMALL[A] / CHUNK[A] on the device: kept for the module; its observation tables are overwritten in place by _install."""
    from test_hip_bucket import _native_tree

    tree = _native_tree(**(rr.SMALL if kind == "small" else rr.CHUNK)[A])
    h = tree.handle()
    assert 2 * h.S == (rr.SMALL_ROWS if kind == "small" else rr.CHUNK_ROWS)[A] <= rr.MAX_ROWS
    assert h.legal_foldable == (A >= 2), "every tree of the sweep is foldable"
    assert torch.equal(cpu_t(h.observations_table()), rr.tree_observations(kind, A)), "the host's observation table is the device's"
    return tree, h


def cpu_t(t):
    return t.detach().cpu()


@functools.lru_cache(maxsize=None)
def _device(kind, A, W, family, half):
    """A case of tests/_rowsref.py on the device: packed images, regularisation logits, the logit table of MODE 1, the legal masks."""
    import rnad_hip as hip
    from _gpu import DEV

    case = rr.case(kind, A, W, family, half)
    _, h = _handle(kind, A)
    lib = hip.lib()
    weights = [[w.detach().to(DEV).contiguous() for w in n._weights()] for n in case.nets[:2]]
    g = torch.Generator().manual_seed(9 + A)
    d = types.SimpleNamespace(case=case, h=h, A=A, W=W, N=case.N, obs=case.obs.to(DEV))
    d.packs = {fold: hip.mlp_pack_many(weights, A, fold=fold) for fold in ((False, True) if A >= 2 else (False,))}
    d.lr, d.lr2 = (torch.randn((case.N, A), generator=g).to(DEV) for _ in range(2))
    d.logit_tab = torch.tensor(case.ref.logits, dtype=torch.float32).to(DEV)  # MODE 1: "a staged actor wrote the logits"
    d.mask = case.obs[:, 1, :, 0].float().contiguous().to(DEV)  # the mover's legal actions
    d.hp = hip.make_learn_params(alpha=0.3, eta=0.2, clip=1e3, threshold=2.0, eps_threshold=0.03, n_disc=16)
    d.strides = dict(records=int(lib.rnad_bucket_record_stride(A)), fast_records=int(lib.rnad_bucket_fast_record_stride(A)),
                     policy_rows=int(lib.rnad_bucket_policy_row_stride(A)))
    return d


def _install(d, listed=None):
    """The case's observations into the handle's own table (the only object the fold accepts); the rows that are not listed poisoned."""
    table = d.h.observations_table(d.case.half)
    assert table.shape == d.obs.shape and table.dtype == d.obs.dtype
    table.copy_(d.obs)
    if listed is not None:
        table[~listed] = rr.POISON[table.dtype]
    return table


def _row_list(d, order, n):
    """The first n entries of `order` as a row list in the shape of a LiveRows: a buffer of all 2S entries (the others name rows that are
    not listed) and the count in device memory.  -> (list, bool mask of the listed rows)"""
    import rnad_hip as hip
    from _gpu import DEV

    listed = torch.zeros(d.N, dtype=torch.bool, device=DEV)
    listed[order[:n].to(DEV).long()] = True
    assert order.numel() == d.N and int(listed.sum()) == n, "a row list names every row once"
    live = hip.RowList(order, d.N, DEV)
    live.count.fill_(n)
    return live, listed


def _launch(d, table, fold, mode, rows):
    """One launch into sentinel-filled tables -> dict of the tables it may write."""
    import rnad_hip as hip
    from _gpu import DEV

    new = lambda cols: torch.full((d.N, cols), SENTINEL, device=DEV)  # noqa: E731
    f = d.h if fold else False
    if mode == 2:
        out = dict(logit=new(d.A), policy_rows=new(d.strides["policy_rows"]))
        hip.mlp_forward_actor(d.h, d.packs[fold][0], d.W, table, out["logit"], out["policy_rows"], rows=rows, fold=f)
        return out
    out = dict(v=new(1), v_target=new(1), records=new(d.strides["records"]), fast_records=new(d.strides["fast_records"]))
    logit_tab = None
    if mode == 0:
        out.update(logit=new(d.A), policy_rows=new(d.strides["policy_rows"]))
    else:
        logit_tab = d.logit_tab.clone()
    got = hip.mlp_rows_records(d.h, d.packs[fold][0], d.packs[fold][1], d.W, table, d.lr, d.lr2, d.hp, fold=f, rows=rows, logit_tab=logit_tab,
                               out=dict(out))
    assert all(got[k] is t for k, t in out.items()), "out= tables are the ones written"
    if mode == 1:
        assert got["logit"] is logit_tab and got["policy_rows"] is None
        assert torch.equal(logit_tab.view(I32), d.logit_tab.view(I32)), "MODE 1 must not write the logit table it reads"
        out["logit_given"] = logit_tab
    return out


def _verify(d, out, mode, listed, what):
    import rnad_hip as hip

    ref, A = d.case.ref, d.A
    sel = None if listed is None else cpu_t(listed).numpy()
    used = []
    if mode != 1:
        used.append(rr.gate(cpu_t(out["logit"]).numpy(), ref.logits, ref.B_logits, G, f"{what}: logits", sel))
    if mode != 2:
        used.append(rr.gate(cpu_t(out["v"]).numpy()[:, 0], ref.v, ref.B_v, G, f"{what}: v", sel))
        used.append(rr.gate(cpu_t(out["v_target"]).numpy()[:, 0], ref.v_target, ref.B_v_target, G, f"{what}: v_target", sel))
    if listed is not None:
        for k, t in out.items():
            if k != "logit_given":
                assert (t[~listed] == SENTINEL).all(), f"{what}: {k} was written in a row that is not listed"
    L = slice(None) if listed is None else listed
    if mode == 2:
        want = hip.policy_head(out["logit"].contiguous(), mask=d.mask)
        assert torch.equal(out["policy_rows"][L][:, :A].view(I32), want[L].view(I32)), f"{what}: policy rows are the policy head of the kernel's own logits"
        assert (out["policy_rows"][L][:, A:] == 0).all(), f"{what}: pad columns are zeros"
    else:  # rnad_bucket_records of the kernel's own tables (its rows that are not listed hold the sentinel: compared where listed)
        logit = out["logit_given"] if mode == 1 else out["logit"]
        rec, fast = hip.bucket_records(d.h, logit, out["v"], out["v_target"], d.lr, d.lr2, d.hp, fast=True)
        assert torch.equal(out["records"][L].view(I32), rec[L].view(I32)), f"{what}: records differ from rnad_bucket_records"
        assert torch.equal(out["fast_records"][L].view(I32), fast[L].view(I32)), f"{what}: fast records differ"
        if mode == 0:
            assert torch.equal(out["policy_rows"][L].view(I32), rec._policy_rows[L].view(I32)), f"{what}: policy rows differ"
    return max(used) if used else 0.0


def _variants(A, W):
    import rnad_hip as hip

    return rr.launchable(hip.lib(), W, (A,))


def _env(monkeypatch, mode, split):
    monkeypatch.setenv("RNAD_MLP_SPLIT", "1" if split else "0")
    monkeypatch.setenv("RNAD_FUSED_ROWS", "1")
    monkeypatch.setenv("RNAD_POLICY_ROWS", "1")
    monkeypatch.setenv("RNAD_ROWS_ACTOR", "1" if mode == 2 else "0")


# ------------------------------------------------------------------------------------------------ a. every instantiation, small
@pytest.mark.parametrize("family", rr.FAMILIES)
@pytest.mark.parametrize("A", sorted(rr.SMALL))
def test_every_instantiation_on_a_small_tree(A, family, monkeypatch):
    ran = set()
    for W in (256,) + (rr.WIDTHS_EXTRA if A in (3, 5) else ()):
        variants = _variants(A, W)
        assert variants, (A, W)
        for half in (False, True):
            d = _device("small", A, W, family, half)
            table = _install(d)
            for _, fold, mode, split in variants:
                _env(monkeypatch, mode, split)
                what = f"A={A} W={W} {family} half={half} fold={fold} {MODES[mode]} split={split}"
                used = _verify(d, _launch(d, table, fold, mode, None), mode, None, what)
                print(what, "-> largest error %.3f of 2^-24 B" % used)
                ran.add((W // 32, half, fold, mode, split))
    from test_rows_shapes import LAUNCHABLE_256

    assert {(fold, mode, split) for T, _, fold, mode, split in ran if T == 8} == {k[1:] for k in LAUNCHABLE_256 if k[0] == A}
    assert {T for T, *_ in ran} == ({1, 3, 5, 7, 8} if A in (3, 5) else {8}) and {h for _, h, *_ in ran} == {False, True}


# ------------------------------------------------------------------------------------------------ b. row lists
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("A", (3, 4))  # A = 3: every MODE, dedicated record waves; A = 4: the 8-wave build whose compute waves write the records
def test_row_lists_leave_the_other_rows_alone(A, mode, half, monkeypatch):
    variants = [v for v in _variants(A, 256) if v[2] == mode]
    if not variants:
        assert (A, mode) == (4, 0), "only MODE 0 at A = 4 has no launch"
        return
    d = _device("small", A, 256, "wide", half)
    order = rr.shuffled(d.N, 100 * A + mode)
    assert not torch.equal(order, torch.sort(order).values)
    for n in rr.LIST_LENGTHS + (d.N,):
        live, listed = _row_list(d, order, n)
        table = _install(d, listed)
        for _, fold, _, split in variants:
            _env(monkeypatch, mode, split)
            what = f"A={A} {n} of {d.N} rows half={half} fold={fold} {MODES[mode]} split={split}"
            out = _launch(d, table, fold, mode, live)
            if n == 0:
                assert all((t == SENTINEL).all() for k, t in out.items() if k != "logit_given"), f"{what}: an empty list writes nothing"
            _verify(d, out, mode, listed, what)
    _install(d)


# ------------------------------------------------------------------------------------------------ c. the chunk loop
def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(I32), b[k].view(I32)), f"{what}: two launches differ in {k}"


@pytest.mark.parametrize("A", sorted(rr.CHUNK))
def test_chunk_loop(A, monkeypatch):
    from _gpu import DEV

    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    N = rr.CHUNK_ROWS[A]
    n = rr.chunk_list_length(N)
    for count, rows_of_table in ((N, None), (n, N)):
        p = rr.partition_properties(count, cus, rows_of_table)
        assert p["three_chunks"] and p["short_last_chunk"] and p["half_step"] and p["partial_tile"], \
            f"{count} rows on {cus} CUs do not walk the chunk loop as the case was chosen to: {p}"
    variants = _variants(A, 256)
    fp16 = {next(v for v in variants if v[3]), next(v for v in variants if not v[3] and v[1] and v[2] == 2)}  # one split, one not
    for half in (False, True):
        d = _device("chunk", A, 256, "wide", half)
        live, listed = _row_list(d, rr.shuffled(N, 7 * A), n)
        for _, fold, mode, split in variants:
            if half and (A, fold, mode, split) not in fp16:
                continue
            _env(monkeypatch, mode, split)
            on_list = mode != 0
            table = _install(d, listed if on_list else None)
            what = f"A={A} {n if on_list else N} of {N} rows half={half} fold={fold} {MODES[mode]} split={split}"
            first = _launch(d, table, fold, mode, live if on_list else None)
            again = _launch(d, table, fold, mode, live if on_list else None)
            _same_bits(first, again, what)
            used = _verify(d, first, mode, listed if on_list else None, what)
            print(what, "-> largest error %.3f of 2^-24 B" % used)
    _install(d)
