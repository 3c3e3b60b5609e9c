"""The MLP backward (csrc/mlp_bwd_t.hip: k_mlp_backward_t<A, ObsT, WAVES, FOLD>; csrc/mlp_bwd.hip: k_mlp_backward, k_mlp_reduce<A, FOLD>) against
fp64 autograd through the unfolded net, over every instantiation and through the tile loop.

tests/test_hip_parity.py compares the plain backward with autograd at twelve shapes under a per-tensor tolerance with the hidden units near a
ReLU kink left out; tests/test_hip_fold.py and tests/test_hip_ragged.py compare the fold and the row lists with the plain kernel on trees'
own tables.  Here the reference is tests/_mlpbwdref.py, and the gate is |got - want| <= G 2^-24 B on EVERY element of all eight tensors (B:
the sum of the absolute terms of the entry; G from tests/test_mlp_bwd_shapes.py, where plain fp32 torch uses at most half of it).  Every
output tensor starts as 1e30 (finite: the objects are built with -fno-honor-nans), and so does the workspace of per-workgroup partials.

  a. every variant at 203 rows, width 64: A = 1 .. 8 plain and A = 2 .. 8 folded, fp32 and fp16 observations -- (N16, LO) from (0, 3) to
     (8, 1), the folded left-over columns (A = 4, 7, 8) among them -- and the fold with half of the rows absorbing, where db0 - d_abs cancels;
  b. widths 32 .. 256: 1, 2, 4 waves and 1, 2, 3, 5 groups of hidden tiles, the plan held to the restated table;
  c. 1 .. 1055 rows at width 32: 1, 15, 16, 17 and 33 rows of partials for the 16 slices of the reduction;
  d. shuffled row lists of 0 .. 257 rows over a table of 600 whose other rows (observations, dlogits, dvalue) hold a large finite poison:
     an empty list gives exact zeros; the fold entry point also with the list's own length as the capacity;
  e. the tile loop: 2.5 tiles per workgroup of the launch this machine plans (rnad_mlp_backward_plan), so some workgroups walk three tiles,
     some two, and the last tile is partial; each case twice with identical bits; one of them also through a shuffled row list;
  f. the LDS-transpose kernel (RNAD_MLP_BWD=lds, chosen once per process) on the plain cases of a. and two of e., in a child process.

The worst share of the gate per case and tensor goes to mlp_bwd_errors.json (the child process: mlp_bwd_errors_lds.json) in the directory
that RNAD_ERRORS_DIR names, when it is set; profiles/mlp_bwd_errors.json holds the figures of an MI355X."""
import functools
import json
import os
import subprocess
import sys
import time
import types

import pytest
import torch

import _mlpbwdref as mr
from test_mlp_bwd_shapes import G

pytestmark = pytest.mark.gpu

LDS = os.environ.get("RNAD_MLP_BWD", "")[:1] == "l"  # use_resident_backward (csrc/mlp_bwd.hip)
CHILD_START_UP = 120.0  # seconds allowed on top for the child's interpreter, imports and device initialisation
_TIMES = {}             # (group, case id) -> seconds this process took for the case: sizes the child's time limit


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if mr.SHARES and os.path.isdir(out):
        with open(os.path.join(out, "mlp_bwd_errors_lds.json" if LDS else "mlp_bwd_errors.json"), "w") as f:
            json.dump(mr.SHARES, f, indent=1, sort_keys=True)


def _hip():
    import rnad_hip

    return rnad_hip


@functools.lru_cache(maxsize=None)
def _device(key):
    """A case of tests/_mlpbwdref.py on the device, with its weight image."""
    from _gpu import DEV

    hip = _hip()
    c = mr.case(*key)
    w = [t.to(DEV).contiguous() for t in c.weights]
    packed = mr.pack_fold(hip, w, c.A) if c.fold else hip.mlp_pack(w, c.A)
    assert packed.numel() == hip.mlp_packed_size(c.A, c.W, fold=c.fold)
    return types.SimpleNamespace(c=c, w=w, packed=packed, obs=c.obs.to(DEV), dlogits=c.dlogits.to(DEV), dvalue=c.dvalue.to(DEV))


def _plan(key, N=None):
    v, A, W, n, _ = key
    return _hip().mlp_backward_plan(n if N is None else N, A, W, v != "plain")


def _backward(d, tables=None, live=None, capacity=None):
    """One backward into tensors that start as the poison -> the eight gradients on the host."""
    hip, c = _hip(), d.c
    obs, dl, dv = tables or (d.obs, d.dlogits, d.dvalue)
    out = [torch.full_like(w, mr.POISON[torch.float32]) for w in d.w]
    if c.fold:
        mr.backward_fold(hip, d.packed, obs, c.A, c.W, dl, dv, out, live=live, capacity=capacity)
    else:
        assert capacity is None
        ws = torch.full((hip.lib().rnad_mlp_backward_workspace(c.N, c.A, c.W) // 4,), mr.POISON[torch.float32], device=obs.device)
        hip.mlp_backward(d.packed, d.w, obs, c.A, dl, dv, live=live, out=out, workspace=ws)
    return [g.cpu() for g in out]


def _gate(got, grads, bounds, what):
    used = mr.gate_all([g.double().numpy() for g in got], grads, bounds, G, what)
    print(what, "-> units of 2^-24 B:", {k.replace("_fc", "").replace(".weight", ".w").replace(".bias", ".b"): round(u, 2) for k, u in used.items()})
    return used


def _run_whole(key, group):
    """The case on all its rows, gated; -> the gradients."""
    t0 = time.perf_counter()
    try:
        d = _device(key)
        assert _plan(key).resident == (d.c.fold or not LDS)
        got = _backward(d)
        _gate(got, d.c.grads, d.c.bounds, f"{group} {mr.case_id(key)}")
    finally:  # (also when the case fails: the child's time limit is sized from the time taken, whatever the outcome)
        _TIMES[(group, mr.case_id(key))] = time.perf_counter() - t0
    return got


# ------------------------------------------------------------------------------------------------ a. every variant
@pytest.mark.parametrize("key", mr.sweep_cases(), ids=mr.case_id)
def test_variant_sweep(key):
    _run_whole(key, "a")
    p = _plan(key)
    assert p.grid_x == 7 and p.waves * p.groups == 2, "203 rows: seven workgroups, seven rows of partials"


# ------------------------------------------------------------------------------------------------ b. widths
@pytest.mark.parametrize("key", mr.width_cases(), ids=mr.case_id)
def test_widths(key):
    p = _plan(key)
    assert p.resident == (key[0] != "plain" or not LDS)
    if not LDS:
        assert (p.waves, p.groups) == mr.resident_launch(key[2]), "the launch is not the one the case was chosen for"
    assert p.waves * p.groups == key[2] // 32
    _run_whole(key, "b")


# ------------------------------------------------------------------------------------------------ c. sizes
@pytest.mark.parametrize("key", mr.size_cases(), ids=mr.case_id)
def test_sizes(key):
    p = _plan(key)
    assert p.grid_x == (key[3] + 31) // 32, "one workgroup, and one row of partials, per tile"
    _run_whole(key, "c")


# ------------------------------------------------------------------------------------------------ d. row lists
@functools.lru_cache(maxsize=None)
def _listed(key, n, seed):
    """The first n rows of a shuffled order of the case's table: the list (all rows, count n, as a LiveRows), the tables with the other
    rows poisoned, the fp64 reference of the listed rows."""
    from _gpu import DEV

    hip, d = _hip(), _device(key)
    order = mr.shuffled(d.c.N, seed)
    assert not torch.equal(order, torch.sort(order).values)
    live = hip.RowList(order, d.c.N, DEV)
    live.count.fill_(n)
    listed = torch.zeros(d.c.N, dtype=torch.bool, device=DEV)
    listed[order[:n].to(DEV).long()] = True
    assert int(listed.sum()) == n
    tables = [d.obs.clone(), d.dlogits.clone(), d.dvalue.clone()]
    for t in tables:
        t[~listed] = mr.POISON[t.dtype]
    return live, tables, mr.reference(d.c, order[:n].long())


@pytest.mark.parametrize("n", mr.LIST_LENGTHS)
@pytest.mark.parametrize("key", mr.row_list_cases(), ids=mr.case_id)
def test_row_lists(key, n):
    d = _device(key)
    live, tables, (grads, bounds) = _listed(key, n, 100 * key[1])
    got = _backward(d, tables, live=live)
    if n == 0:
        assert all((g == 0).all() for g in got), "an empty list gives exact zeros in all eight tensors"
    _gate(got, grads, bounds, f"d {mr.case_id(key)} rows {n}")


def test_fold_row_list_capacity():
    """The fold entry point sizes its launch from the list's capacity: the table's 600 rows, or exactly the 33 that are listed."""
    key = next(k for k in mr.row_list_cases() if k[0] != "plain")
    d = _device(key)
    live, tables, (grads, bounds) = _listed(key, 33, 100 * key[1])
    assert _plan(key, 600).grid_x == 19 and _plan(key, 33).grid_x == 2
    for capacity in (600, 33):
        _gate(_backward(d, tables, live=live, capacity=capacity), grads, bounds, f"d {mr.case_id(key)} rows 33 capacity {capacity}")


# ------------------------------------------------------------------------------------------------ e. the tile loop
def _loop_key(shape):
    """The case of a tile-loop shape on THIS machine: 2.5 tiles per persistent workgroup of the launch the host plans for 10^6 rows."""
    v, A, W, half = shape
    g = _hip().mlp_backward_plan(10**6, A, W, v != "plain").grid_x
    key = (v, A, W, mr.loop_rows(g), half)
    N = key[3]
    assert N <= mr.MAX_LOOP_ROWS, f"{shape}: {g} persistent workgroups ask for {N} rows"
    p = mr.loop_properties(N, _plan(key).grid_x)
    assert _plan(key).grid_x == g and p["rounds"] >= 3 and p["partial_round"] and p["partial_tile"], (shape, g, N, p)
    return key


def _loop_id(shape):
    v, A, W, half = shape
    return f"{v}_A{A}_W{W}_{'fp16' if half else 'fp32'}"


def _same_bits(a, b, what):
    for k, x, y in zip(mr.KEYS, a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: two launches differ in {k}"


@pytest.mark.parametrize("shape", mr.LOOP_SHAPES, ids=_loop_id)
def test_tile_loop(shape):
    key = _loop_key(shape)
    t0 = time.perf_counter()
    try:
        first = _run_whole(key, "e")
        _same_bits(first, _backward(_device(key)), mr.case_id(key))  # the partials are summed in a fixed order
    finally:
        _TIMES[("e", _loop_id(shape))] = time.perf_counter() - t0


def test_row_list_through_the_tile_loop():
    shape = mr.LOOP_SHAPES[0]
    assert shape[:3] == ("fold", 3, 256)
    key = _loop_key(shape)
    d = _device(key)
    n = mr.loop_list_length(d.c.N)
    g = _plan(key).grid_x
    p = mr.loop_properties(n, g)
    assert p["rounds"] >= 3 and p["partial_round"] and p["partial_tile"], (n, g, p)
    live, tables, (grads, bounds) = _listed(key, n, 7)
    first = _backward(d, tables, live=live)
    _gate(first, grads, bounds, f"e {mr.case_id(key)} rows {n}")
    _same_bits(first, _backward(d, tables, live=live), f"{mr.case_id(key)} rows {n}")


# ------------------------------------------------------------------------------------------------ f. the LDS-transpose kernel
LDS_LOOP_SHAPES = [s for s in mr.LOOP_SHAPES if s[:3] in (("plain", 3, 256), ("plain", 8, 32))]
LDS_SELECT = "(test_variant_sweep and plain_) or (test_tile_loop and (" + " or ".join(_loop_id(s) for s in LDS_LOOP_SHAPES) + "))"


def test_lds_transpose_kernel_in_a_child_process():
    """csrc/mlp_bwd.hip's own kernel (RNAD_MLP_BWD=lds) is chosen once per process: one child runs the plain cases of a. and two of e. under
    the same gate.  Its time limit is ten times what this process took for those cases, plus the child's start-up."""
    assert not LDS, "the child must not start a child"
    assert len(LDS_LOOP_SHAPES) == 2
    for key in mr.sweep_cases():
        if key[0] == "plain" and ("a", mr.case_id(key)) not in _TIMES:
            test_variant_sweep(key)
    for shape in LDS_LOOP_SHAPES:
        if ("e", _loop_id(shape)) not in _TIMES:
            test_tile_loop(shape)
    took = sum(_TIMES[("a", mr.case_id(k))] for k in mr.sweep_cases() if k[0] == "plain") + sum(_TIMES[("e", _loop_id(s))] for s in LDS_LOOP_SHAPES)
    env = dict(os.environ, RNAD_MLP_BWD="lds")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.realpath(__file__), "-q", "-x", "-s", "-k", LDS_SELECT], env=env,
                       capture_output=True, text=True, timeout=10 * took + CHILD_START_UP)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "18 passed" in r.stdout, r.stdout[-2000:]
