"""Inputs, the fp64 reference, the error bound and the restated host arithmetic for the shape sweep of the MLP forward (csrc/mlp_fwd.hip:
k_mlp_forward<A, ObsT, HEADS, FOLD>, k_mlp_pack, mlp_forward_plan) -- tests/test_mlp_fwd_shapes.py on the CPU,
tests/test_hip_mlp_fwd_shapes.py on the GPU.  Nothing here needs a GPU or calls a project kernel, but for the launch helpers at the end.

The reference is tests/_rowsref.py's: the net of nn/net.py in double precision on the UNFOLDED observation [ev | legal] (2 A^2 features);
for an fp16 table it takes the fp16-rounded values.  It shares nothing with the packing, the weight image or the legal fold.  The gate is
|got - want| <= G 2^-24 B per row and output, B the sum of the absolute terms with the legal plane counted as ones (_rowsref.py); G is fixed
in tests/test_mlp_fwd_shapes.py from plain fp32 torch on these very inputs, never from a kernel's output.  A case holds FOUR nets of distinct
weights (_rowsref.nets: learner, target and two regularisation nets); `reference` is applied pairwise, net i with itself, so that every
net of a net set has its own logits, v and bounds.

Inputs are synthetic, not tied to a tree.  Family "init": the default MLP init, ev uniform in (-1, 1).  Family "wide": _rowsref's wide
first-layer matrices (nets 0 and 1) and wide_ev.  "plain" rows carry a random 0 / 1 legal plane with legal[0] = 1; "fold" rows an all-ones
plane, but for about 5 % absorbing rows whose plane is exactly e0 = [1, 0, ..., 0] and which keep their non-zero ev.

A case key is (variant, A, W, N, half, family)."""
import ctypes
import functools
import types

import numpy as np
import torch

from _mlpbwdref import pack_fold  # noqa: F401  (the FOLD weight image of one net)
from _rowsref import (LIST_LENGTHS, POISON, SMALL, fp32_torch, gate, host_observations, host_tree, nets, normalised, reference, shuffled,  # noqa: F401
                      wide_ev)

U = 2.0 ** -24
VARIANTS = ("plain", "fold")
FAMILIES = ("init", "wide")
SENTINEL = 7.0
ABSORBING = 0.05

N_SWEEP = 203  # = 3 * 64 + 11: four spans -- one workgroup -- the last with a partial first tile and an empty second tile
SWEEP_W = 64
WIDTHS = (32, 96, 160, 256, 512)
LARGEST = ((6, 256), (7, 192), (8, 128))  # the largest widths whose image fits 160 KiB, plain and fold
LARGEST_FLOATS = {(6, 256): (39180, 40204), (7, 192): (39564, 39948), (8, 128): (34188, 34700)}  # plain, fold -- of 40 960
TOO_LARGE = ((6, 288), (7, 224), (8, 160))  # their neighbours: refused
LDS_FLOATS = 160 * 1024 // 4
SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)  # sample tiles of 32, wave spans of 64, workgroups of 256 samples
TABLE_ROWS = 600
ROW_LIST_CASES = (("plain", 3, False, 1), ("fold", 4, True, 1), ("plain", 8, False, 1), ("fold", 5, False, 4))  # variant, A, fp16, nets
LOOP_SHAPES = (("fold", 3, 256, False), ("plain", 3, 256, True), ("fold", 5, 256, False), ("plain", 5, 256, True), ("plain", 3, 512, False),
               ("fold", 8, 128, True))  # variant, A, W, fp16; no blocks_per_cu = 2 shape (A = 4, width 256: 196 619 rows at 256 CUs)
MAX_ROWS = {3: 300_000}  # A = 3; every A >= 4 case: MAX_ROWS_A4 (DESIGN.md "Known and not diagnosed")
MAX_ROWS_A4 = 180_000
WAVES = 4  # waves of a forward workgroup (kFwdThreads / 64)
SPAN = 64  # samples of a wave iteration


def max_rows(A):
    return MAX_ROWS.get(A, MAX_ROWS_A4) if A >= 3 else MAX_ROWS_A4


# ------------------------------------------------------------------------------------------------ the launch arithmetic, restated
def image_floats(A, W, fold):
    if not fold:
        return 2 * W * 2 * A * A + 3 * W + A * W + 12
    K_f = (A * A + 2) & ~1
    return 2 * W * K_f + 3 * W + A * W + 12 + 2 * W * A * A


def plan(N, A, W, fold, n_nets, cus, count=None):
    """mlp_forward_plan of csrc/mlp_fwd.hip: None where the launch is refused, else lds_bytes, blocks_per_cu, per_net, rounds and
    `spans`, the number of 64-sample spans each of the 4 per_net waves of a net walks.  count: the rows of a row list of capacity N (the
    grid is sized from N on the host, the spans come from the count in device memory)."""
    if W < 32 or W % 32 or not 1 <= A <= 8 or N < 0 or not 1 <= n_nets <= 4 or (fold and A < 2):
        return None
    floats = image_floats(A, W, fold)
    if floats > LDS_FLOATS:
        return None
    blocks_per_cu = max(1, min(3, LDS_FLOATS // floats))
    host_spans = -(-N // SPAN)
    per_net = max(1, min(-(-host_spans // WAVES), cus * blocks_per_cu))
    waves = per_net * WAVES
    n_spans = -(-(N if count is None else count) // SPAN)
    spans = [max(0, -(-(n_spans - w) // waves)) for w in range(waves)]
    assert sum(spans) == n_spans
    return types.SimpleNamespace(lds_bytes=4 * floats, blocks_per_cu=blocks_per_cu, per_net=per_net, rounds=-(-host_spans // waves), spans=spans)


def plan_properties(N, A, W, fold, n_nets, cus, count=None):
    p = plan(N, A, W, fold, n_nets, cus, count)
    n = N if count is None else count
    return dict(rounds=max(p.spans), uneven=max(p.spans) - min(p.spans) == 1, partial_span=n % SPAN != 0)


def loop_rows(A, W, fold, cus):
    """Rows of a span-loop case: R = 4 cus blocks_per_cu spans to a round; 1.5 rounds (three resident workgroups per CU) or 2.5 (one), and
    11 samples in the last span."""
    b = plan(1, A, W, fold, 1, cus).blocks_per_cu
    assert b in (1, 3), "no blocks_per_cu = 2 shape: it would pass the row limit of A >= 4"
    R = WAVES * cus * b
    return SPAN * ((R if b == 3 else 2 * R) + R // 2) + 11


def loop_list_length(N):
    """Rows of the shuffled list of a span-loop case: nearly all N, not a multiple of 32."""
    n = N - 45
    return n - 5 if n % 32 == 0 else n


# ------------------------------------------------------------------------------------------------ the weight image, restated
def image(weights, A, fold):
    """The packed image of one net (numpy fp32) from its eight tensors, as the header of csrc/mlp_common.hpp describes it:
         w0t [2T][K/2][2][32]  element ((tile K/2 + ks) 2 + half) 32 + col = W0[hidden 32 tile + col][k = 2 ks + half], the value head's hidden
                               units first, then the policy head's;  b0 [2W];  w1v [W];  w1p [A][W];  b1 [1 + A] in 12 floats;
       fold: K = (A^2 + 2) & ~1 -- the ev columns, the indicator slot and the padding (both zero) -- and behind b1 the raw legal columns
       [A^2][2W], column major."""
    vw0, vb0, vw1, vb1, pw0, pb0, pw1, pb1 = [np.asarray(w, np.float32) for w in weights]
    W, AA = vw0.shape[0], A * A
    assert vw0.shape == pw0.shape == (W, 2 * AA) and vw1.shape == (1, W) and pw1.shape == (A, W) and W % 32 == 0
    W0 = np.concatenate([vw0, pw0])  # [2W, 2 A^2]
    K = ((AA + 2) & ~1) if fold else 2 * AA
    first = np.zeros((2 * W, K), np.float32)
    first[:, :AA if fold else K] = W0[:, :AA if fold else K]
    w0t = first.reshape(2 * W // 32, 32, K // 2, 2).transpose(0, 2, 3, 1)  # [tile][col][ks][half] -> [tile][ks][half][col]
    b1 = np.zeros(12, np.float32)
    b1[0], b1[1:1 + A] = vb1[0], pb1
    parts = [w0t.ravel(), vb0, pb0, vw1.ravel(), pw1.ravel(), b1]
    if fold:
        parts.append(W0[:, AA:].T.ravel())
    return np.concatenate(parts)


def integer_weights(A, W, base=0):
    """The eight tensors filled with the distinct integers base + 1, base + 2, ... (exact in fp32)."""
    shapes = [(W, 2 * A * A), (W,), (1, W), (1,), (W, 2 * A * A), (W,), (A, W), (A,)]
    out, n = [], base
    for s in shapes:
        k = int(np.prod(s))
        out.append(torch.arange(n + 1, n + 1 + k, dtype=torch.float32).reshape(s))
        n += k
    assert n < 2**24
    return out


# ------------------------------------------------------------------------------------------------ the cases
def sweep_cases():
    """a. every A plain and every A >= 2 folded, fp32 and fp16 tables, both families."""
    return [(v, A, SWEEP_W, N_SWEEP, half, family) for v, lo in (("plain", 1), ("fold", 2)) for A in range(lo, 9) for half in (False, True)
            for family in FAMILIES]


def width_cases():
    return [(v, A, W, N_SWEEP, False, "init") for v, A in (("plain", 3), ("fold", 4)) for W in WIDTHS
            if image_floats(A, W, v == "fold") <= LDS_FLOATS]


def largest_cases():
    return [(v, A, W, N_SWEEP, False, "init") for A, W in LARGEST for v in VARIANTS]


def size_cases():
    return [(v, A, 32, N, False, "init") for v, A in (("plain", 3), ("fold", 4)) for N in SIZES]


def row_list_cases():
    return [(v, A, SWEEP_W, TABLE_ROWS, half, "init") for v, A, half, _ in ROW_LIST_CASES]


def row_list_nets(key):
    return next(n for v, A, half, n in ROW_LIST_CASES if (v, A, half) == (key[0], key[1], key[4]))


def net_set_cases():
    """c. the tables of the net sets: plain A = 3, fold A = 5 and A = 4."""
    return [("plain", 3, SWEEP_W, N_SWEEP, False, "init"), ("fold", 5, SWEEP_W, N_SWEEP, False, "init"), ("fold", 4, SWEEP_W, N_SWEEP, True, "init")]


def loop_cases(cus):
    """e. the span-loop cases on a device of `cus` compute units that stay inside the row limits -> (cases, [(shape, rows) left out])."""
    out, over = [], []
    for v, A, W, half in LOOP_SHAPES:
        N = loop_rows(A, W, v == "fold", cus)
        if N <= max_rows(A):
            out.append((v, A, W, N, half, "wide"))
        else:
            over.append(((v, A, W, half), N))
    for key in out:
        assert key[3] <= max_rows(key[1]), key
    return out, over


def case_id(key):
    v, A, W, N, half, family = key
    return f"{v}_A{A}_W{W}_N{N}_{'fp16' if half else 'fp32'}_{family}"


def _draw(N, A, variant, family, seed):
    g = torch.Generator().manual_seed(31337 + 100 * A + seed)
    ev = wide_ev(N, A, seed).reshape(N, A * A) if family == "wide" else torch.rand((N, A * A), generator=g) * 2 - 1
    if variant == "plain":
        absorbing = None
        legal = (torch.rand((N, A * A), generator=g) < 0.5).float()
        legal[:, 0] = 1.0
    else:
        absorbing = torch.rand((N,), generator=g) < ABSORBING
        legal = torch.ones((N, A * A))
        legal[absorbing, 1:] = 0.0
    return ev, legal, absorbing


@functools.lru_cache(maxsize=None)
def case(variant, A, W, N, half, family):
    """Four nets, the observation table [N, 2, A, A] (fp32 or fp16) and -- lazily, per net -- the fp64 reference: built once, left unchanged."""
    assert variant in VARIANTS and family in FAMILIES and (variant == "plain" or A >= 2)
    ev, legal, absorbing = _draw(N, A, variant, family, 0)
    obs = torch.cat([ev, legal], 1).reshape(N, 2, A, A)
    obs = obs.half() if half else obs
    c = types.SimpleNamespace(key=(variant, A, W, N, half, family), variant=variant, fold=variant == "fold", A=A, W=W, N=N, half=half,
                              family=family, obs=obs, ev_unrounded=ev, absorbing=absorbing, nets=nets(A, W, family), _refs={})
    c.weights = [[w.detach().clone() for w in n._weights()] for n in c.nets]
    c.ref = lambda i=0: net_reference(c, i)
    return c


def net_reference(c, i, obs=None):
    """logits [N, A], v [N] and their bounds of net i of the case (obs: another table in place of the case's, not cached)."""
    if obs is not None:
        return reference(c.nets[i], c.nets[i], obs)
    if i not in c._refs:
        c._refs[i] = reference(c.nets[i], c.nets[i], c.obs)
    return c._refs[i]


SHARES = {}  # what -> {output: largest share of 2^-24 B}: every gate_outputs() of the run, for the logged figures


def gate_outputs(logits, value, ref, G, what, rows=None, detail=""):
    """The gate on the outputs that are not None (numpy [N, A] / [N] or [N, 1]) over `rows` (None: all) -> {output: largest share}; both are
    compared before the first failure is raised.  The figures are kept under `what` (the case); detail: the launch, for the message."""
    used, failures = {}, []
    for name, got, want, B in (("logits", logits, ref.logits, ref.B_logits), ("v", value, ref.v, ref.B_v)):
        if got is None:
            continue
        got = np.asarray(got, np.float64).reshape(want.shape)
        try:
            used[name] = gate(got, want, B, G, f"{what} {detail}: {name}", rows)
        except AssertionError as e:
            failures.append(str(e))
            sel = slice(None) if rows is None else rows
            used[name] = float(np.nan_to_num(normalised(got[sel], want[sel], B[sel]), nan=1e300).max())
        rec = SHARES.setdefault(what, {})
        rec[name] = max(rec.get(name, 0.0), used[name])
    assert not failures, "\n".join(failures)
    return used


# ------------------------------------------------------------------------------------------------ the trees of the actor epilogue
ACTOR_TREES = {**SMALL, 8: dict(A=8, C=1, depth=2, seed=0)}  # _rowsref's small trees (A = 1 .. 5) and one of 132 rows at A = 8
ACTOR_W = 64


@functools.lru_cache(maxsize=None)
def actor_case(A, half):
    """The tree's own observation table (built on the host; fp16: rounded), a net of the default init and the fp64 reference of its logits."""
    obs = host_observations(host_tree(**ACTOR_TREES[A]))
    obs = obs.half() if half else obs
    n = nets(A, ACTOR_W, "init")
    return types.SimpleNamespace(A=A, W=ACTOR_W, half=half, N=obs.shape[0], obs=obs, net=n[0], ref=reference(n[0], n[0], obs),
                                 mask=obs[:, 1, :, 0].float().contiguous())  # the mover's legal actions


# ------------------------------------------------------------------------------------------------ launches (GPU)
def forward_fold(hip, packed_list, obs, A, W, outs, live=None, capacity=None):
    """rnad_mlp_forward_fold itself on arbitrary tables.  The Python wrappers rightly accept only a tree's own table; the C contract is "the
    caller guarantees the premise" (every legal plane all ones or e0), which the fold cases satisfy.  packed_list: 1 .. 4 FOLD images;
    outs: per net (logits [N, A] or None, value [N, 1] or None), written in place; live: a row list (capacity: N unless given)."""
    lib = hip.lib()
    n = len(packed_list)
    tensors = list(packed_list) + [obs] + [t for o in outs for t in o if t is not None]
    assert len(outs) == n and all(t.is_cuda and t.is_contiguous() for t in tensors)
    assert obs.dtype in POISON and all(t.dtype == torch.float32 for t in tensors if t is not obs)
    N = obs.shape[0]
    assert all((lg is None or lg.shape == (N, A)) and (v is None or v.shape == (N, 1)) for lg, v in outs)
    cap = N if capacity is None else int(capacity)
    assert live is not None or cap == N
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    P = (ctypes.c_void_p * n)(*[p.data_ptr() for p in packed_list])
    L = (ctypes.c_void_p * n)(*[ptr(o[0]) for o in outs])
    V = (ctypes.c_void_p * n)(*[ptr(o[1]) for o in outs])
    rows, count = (None, None) if live is None else (live.rows.data_ptr(), live.count.data_ptr())
    rc = lib.rnad_mlp_forward_fold(n, cap, rows, count, A, W, P, obs.data_ptr(), int(obs.dtype == torch.float16), L, V,
                                   torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise hip.RnadHipError(lib.rnad_last_error().decode())
    return outs
