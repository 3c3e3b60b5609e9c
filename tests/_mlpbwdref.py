"""Inputs, the fp64 reference and the error bound for the shape sweep of the MLP backward (csrc/mlp_bwd_t.hip: k_mlp_backward_t<A, ObsT,
WAVES, FOLD>, csrc/mlp_bwd.hip: k_mlp_backward and k_mlp_reduce<A, FOLD>) -- tests/test_mlp_bwd_shapes.py on the CPU,
tests/test_hip_mlp_bwd_shapes.py on the GPU.  Nothing here needs a GPU or calls a project kernel, but for the two launch helpers at the end.

The reference is the net of nn/net.py in double precision on the UNFOLDED observation [ev | legal] (2 A^2 features), differentiated by
torch.autograd: the gradients of the eight Linear tensors for given dL/dlogits [N, A] and dL/dvalue [N, 1].  It shares nothing with the
packing, the legal fold or the per-workgroup partial layout.  For an fp16 table it takes the fp16-rounded values (exact in fp64); for a row
list exactly the listed rows.

The gate is relative to what the arithmetic can lose.  With gate = [z64 > 0], Bz[n, h] = sum_k |W0[h, k]| |x[n, k]| + |b0[h]| and
UP[n, h] = sum_o |W1[o, h]| |dout[n, o]|, the sum of the absolute terms of an entry is
    dW0[h, k]  sum_n gate UP |x[n, k]|        db0[h]  sum_n gate UP
    dW1[o, h]  sum_n |dout[n, o]| gate Bz      db1[o]  sum_n |dout[n, o]|
and on a fold case the legal columns j >= 1 of dW0, which k_mlp_reduce<A, true> derives as db0 - d_abs, take B(db0) + B(d_abs), d_abs being
the same sum over the absorbing rows only.  |got - want| <= G 2^-24 B on EVERY element of all eight tensors; G is fixed in
tests/test_mlp_bwd_shapes.py from plain fp32 torch on these very inputs, never from a kernel's output.

The ReLU kink.  A gradient is discontinuous where a pre-activation crosses zero: a correct fp32 implementation may take the other branch
there, and the sample's whole contribution then differs.  That is a property of the inputs, so a sample is kept only if every hidden unit of
both heads has |z64| >= 2 (K + 1) 2^-24 Bz with K = 2 A^2 -- twice the worst-case error of an fp32 sum of K + 1 terms in any order -- and
a rejected sample is redrawn, so N stays exact.  Fewer than 10 % of the draws may be rejected (tests/test_mlp_bwd_shapes.py); a case that
violates it gets another seed in SEEDS, never another threshold.

Inputs: the default MLP(A, W) init; ev uniform in (-1, 1); dlogits normal with about 30 % of the rows zeroed; dvalue normal.  "plain" cases
have a random 0 / 1 legal plane with legal[0] = 1.  "fold" cases have it all ones but for about 5 % absorbing rows whose plane is exactly e0;
"cancel" has 50 % absorbing rows whose dlogits and dvalue are five times larger, so that db0 - d_abs cancels.  Absorbing rows keep non-zero
ev, dlogits and dvalue."""
import ctypes
import functools
import types

import numpy as np
import torch

from _rowsref import shuffled  # noqa: F401  (the row lists: shuffled prefixes of a permutation)

U = 2.0 ** -24
KEYS = ("value_fc0.weight", "value_fc0.bias", "value_fc1.weight", "value_fc1.bias",
        "policy_fc0.weight", "policy_fc0.bias", "policy_fc1.weight", "policy_fc1.bias")
VARIANTS = ("plain", "fold", "cancel")
ABSORBING = {"fold": 0.05, "cancel": 0.5}
POISON = {torch.float32: 1e30, torch.float16: 6e4}  # finite: the MLP objects are built with -fno-honor-nans

N_SWEEP = 203  # = 6 * 32 + 11: 7 partial rows, fewer than the 16 slices of k_mlp_reduce
SWEEP_W = 64
WIDTHS = (32, 96, 128, 160, 192, 256)
SIZES = (1, 31, 32, 33, 481, 512, 513, 1055)  # at width 32: 1, 1, 1, 2, 16, 16, 17, 33 workgroups, i.e. partial rows
TABLE_ROWS = 600
LIST_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 257)
ROW_LIST_CASES = (("plain", 3, False), ("fold", 4, True), ("plain", 8, False))  # variant, A, fp16
LOOP_SHAPES = (("fold", 3, 256, False), ("plain", 3, 256, True), ("fold", 4, 128, True), ("plain", 5, 256, False), ("plain", 8, 32, False),
               ("fold", 7, 64, False))  # variant, A, W, fp16
MAX_LOOP_ROWS = 700_000
# persistent workgroups (grid x) of the resident kernel for 10^6 rows on an MI355X (256 CUs), as rnad_mlp_backward_plan reports them
# there: the CPU file fixes G at the sizes they give; the GPU file asks the machine it runs on
LOOP_GRID_256 = {("fold", 3, 256): 256, ("plain", 3, 256): 256, ("fold", 4, 128): 512, ("plain", 5, 256): 128, ("plain", 8, 32): 1024,
                 ("fold", 7, 64): 512}
SEEDS = {}  # case key -> seed where the default 0 does not satisfy tests/test_mlp_bwd_shapes.py (change the seed, never a gate)


# ------------------------------------------------------------------------------------------------ the kernels' shape tables, restated
def shape(A, fold):
    """K, N16, LO, KQ, XS, FW of MlpShape<A, FOLD> / k_mlp_backward_t / bwd_stage_stride / bwd_feature_stride."""
    K = ((A * A + 2) & ~1) if fold else 2 * A * A
    rem = (K + 1) % 16
    N16, LO = (K + 1) // 16 + (1 if rem > 4 else 0), (0 if rem > 4 else rem)
    XS = (N16 * 16 + (4 if LO > 0 else 0)) | 1
    FW = ((K + 1 + 3) & ~3) if K + 1 <= 32 else ((K + 1 + 31) // 32) * 32
    return types.SimpleNamespace(K=K, N16=N16, LO=LO, KQ=(K + 3) // 4, XS=XS, FW=FW)


def resident_launch(W):
    """(waves per workgroup, groups of hidden tiles) of the register-resident kernel at width W (mlp_backward_plan)."""
    T, waves = W // 32, 4
    while waves > 1 and T % waves:
        waves >>= 1
    return waves, T // waves


def loop_rows(grid_x):
    """Rows of a tile-loop case: with g persistent workgroups, g / 2 of them walk three 32-row tiles, the others two, the last tile holds 11."""
    return 32 * (2 * grid_x + grid_x // 2) + 11


def loop_properties(N, grid_x):
    n_tiles = (N + 31) // 32
    return dict(rounds=(n_tiles + grid_x - 1) // grid_x, partial_round=n_tiles % grid_x != 0, partial_tile=N % 32 != 0)


def loop_list_length(N):
    return N - 45


# ------------------------------------------------------------------------------------------------ the cases
def sweep_cases():
    """a. every A plain and every A >= 2 folded, fp32 and fp16 observations, and the cancelling fold at A = 2, 4, 7."""
    out = [(v, A, SWEEP_W, N_SWEEP, half) for v, lo in (("plain", 1), ("fold", 2)) for A in range(lo, 9) for half in (False, True)]
    return out + [("cancel", A, SWEEP_W, N_SWEEP, False) for A in (2, 4, 7)]


def width_cases():
    return [(v, A, W, N_SWEEP, False) for v, A in (("plain", 3), ("fold", 4)) for W in WIDTHS]


def size_cases():
    return [(v, A, 32, N, False) for v, A in (("plain", 3), ("fold", 4)) for N in SIZES]


def row_list_cases():
    return [(v, A, SWEEP_W, TABLE_ROWS, half) for v, A, half in ROW_LIST_CASES]


def loop_cases(grid_of=None):
    """The tile-loop cases for the grids `grid_of(variant, A, W)` (default: an MI355X's, LOOP_GRID_256)."""
    grid_of = grid_of or (lambda v, A, W: LOOP_GRID_256[(v, A, W)])
    return [(v, A, W, loop_rows(grid_of(v, A, W)), half) for v, A, W, half in LOOP_SHAPES]


def case_id(key):
    v, A, W, N, half = key
    return f"{v}_A{A}_W{W}_N{N}_{'fp16' if half else 'fp32'}"


def _net(A, W, seed):
    from nn.net import MLP

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * A + W + seed)
        net = MLP(A, W)
    return [w.detach().clone() for w in net._weights()]


def _kink_free(x, w64, A):
    """[n] bool: every hidden unit of both heads has |z64| >= 2 (K + 1) 2^-24 Bz on these rows (x: fp64 [n, 2 A^2])."""
    K = 2 * A * A
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for h in (0, 4):
        z = x @ w64[h].T + w64[h + 1]
        Bz = x.abs() @ w64[h].abs().T + w64[h + 1].abs()
        ok &= (z.abs() >= 2 * (K + 1) * U * Bz).all(1)
    return ok


def _draw(n, A, variant, half, g):
    ev = torch.rand((n, A * A), generator=g) * 2 - 1
    absorbing = None
    if variant == "plain":
        legal = (torch.rand((n, A * A), generator=g) < 0.5).float()
        legal[:, 0] = 1.0
    else:
        absorbing = torch.rand((n,), generator=g) < ABSORBING[variant]
        legal = torch.ones((n, A * A))
        legal[absorbing, 1:] = 0.0
    obs = torch.cat([ev, legal], 1)
    dl = torch.randn((n, A), generator=g)
    keep = torch.rand((n, 1), generator=g) < 0.7
    dv = torch.randn((n, 1), generator=g)
    if absorbing is not None:
        keep |= absorbing[:, None]
        if variant == "cancel":
            dl[absorbing] *= 5.0
            dv[absorbing] *= 5.0
    dl = dl * keep
    return (obs.half() if half else obs), ev, dl, dv, absorbing


@functools.lru_cache(maxsize=None)
def case(variant, A, W, N, half):
    """Weights (the eight fp32 CPU tensors, KEYS order), obs [N, 2, A, A] (fp32 or fp16), dlogits [N, A], dvalue [N, 1], the absorbing rows
    (fold variants) and the fp64 reference of all rows: built once, left unchanged."""
    assert variant in VARIANTS and (variant == "plain" or A >= 2)
    key = (variant, A, W, N, half)
    seed = SEEDS.get(key, 0)
    weights = _net(A, W, seed)
    w64 = [w.double() for w in weights]
    g = torch.Generator().manual_seed(4242 + 100 * A + seed)
    kept, draws, have = [], 0, 0
    while have < N:
        n = (N - have) + (N - have) // 8 + 32
        parts = _draw(n, A, variant, half, g)
        ok = _kink_free(parts[0].double(), w64, A)
        draws += n
        kept.append([None if p is None else p[ok] for p in parts])
        have += int(ok.sum())
        assert draws <= 2 * N + 64, f"{key}: more than half of the draws sit on a ReLU kink"
    # the rejection share counts every draw that was looked at, the surplus of the last round included
    rejected = 1.0 - have / draws
    obs, ev, dl, dv, absorbing = [None if kept[0][i] is None else torch.cat([k[i] for k in kept])[:N].contiguous() for i in range(5)]
    c = types.SimpleNamespace(key=key, variant=variant, fold=variant != "plain", A=A, W=W, N=N, half=half, seed=seed, weights=weights,
                              obs=obs.reshape(N, 2, A, A), ev_unrounded=ev, dlogits=dl, dvalue=dv, absorbing=absorbing, rejected=rejected)
    c.grads, c.bounds = reference(c)
    return c


# ------------------------------------------------------------------------------------------------ fp64 reference and bound
def reference(c, rows=None, obs=None, block=1 << 15):
    """(grads, bounds): the fp64 autograd gradients of the eight tensors over `rows` of the case (None: all, in order) and the sums of
    absolute terms B of every entry, as read-only numpy arrays in KEYS order.  obs: another table in place of the case's."""
    A = c.A
    obs = c.obs if obs is None else obs
    sel = torch.arange(c.N) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
    ws = [w.double().clone().requires_grad_(True) for w in c.weights]
    wa = [w.double().abs() for w in c.weights]
    B = [torch.zeros_like(w) for w in wa]
    B_abs = [torch.zeros(c.W, dtype=torch.float64) for _ in range(2)]
    for r0 in range(0, sel.numel(), block):
        s = sel[r0:r0 + block]
        x = obs[s].reshape(s.numel(), -1).double()
        douts = (c.dvalue[s].double(), c.dlogits[s].double())
        outs = []
        for hd, d in enumerate(douts):
            w0, b0, w1, b1 = ws[4 * hd:4 * hd + 4]
            z = x @ w0.T + b0
            outs.append(torch.relu(z) @ w1.T + b1)
            with torch.no_grad():
                gate = (z > 0).double()
                Bz = x.abs() @ wa[4 * hd].T + wa[4 * hd + 1]
                GU = gate * (d.abs() @ wa[4 * hd + 2])
                B[4 * hd] += GU.T @ x.abs()
                B[4 * hd + 1] += GU.sum(0)
                B[4 * hd + 2] += d.abs().T @ (gate * Bz)
                B[4 * hd + 3] += d.abs().sum(0)
                if c.fold:
                    B_abs[hd] += GU[c.absorbing[s]].sum(0)
        torch.autograd.backward(outs, list(douts))
    if c.fold:
        for hd in (0, 1):
            B[4 * hd][:, A * A + 1:] = (B[4 * hd + 1] + B_abs[hd])[:, None]
    grads = [(torch.zeros_like(w) if w.grad is None else w.grad).numpy().copy() for w in ws]
    bounds = [b.numpy() for b in B]
    for a in grads + bounds:
        a.setflags(write=False)
    return grads, bounds


def fp32_torch(c):
    """Plain fp32 torch.autograd on the CPU: the eight gradients."""
    ws = [w.clone().requires_grad_(True) for w in c.weights]
    x = c.obs.reshape(c.N, -1).float()
    value = torch.relu(x @ ws[0].T + ws[1]) @ ws[2].T + ws[3]
    logits = torch.relu(x @ ws[4].T + ws[5]) @ ws[6].T + ws[7]
    torch.autograd.backward([logits, value], [c.dlogits, c.dvalue])
    return [w.grad.numpy() for w in ws]


def share(got, want, B):
    """|got - want| in units of 2^-24 B, elementwise (0 where both the error and B are zero)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / (U * B))


SHARES = {}  # what -> {tensor: largest share of 2^-24 B}: every gate() of the run, for the logged figures


def gate(got, want, B, G, what, tensor=""):
    """|got - want| <= G 2^-24 B on every element, through np.testing.assert_allclose so that tests/conftest.py records the share of the
    tolerance that was used.  -> the largest error in units of 2^-24 B."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, f"{what} {tensor}: shape {got.shape}, expected {want.shape}"
    assert np.isfinite(got).all(), f"{what} {tensor}: not finite"
    s = share(got, want, B)
    worst = float(s.max()) if s.size else 0.0
    if tensor:
        rec = SHARES.setdefault(what, {})
        rec[tensor] = max(rec.get(tensor, 0.0), worst if np.isfinite(worst) else 1e300)
    at = np.unravel_index(int(np.argmax(s)), s.shape) if s.size else ()
    np.testing.assert_allclose(s, np.zeros_like(s), rtol=0, atol=G, err_msg=(  # (in units of 2^-24 B: atol must be a scalar)
        f"{what}: {tensor} uses {worst:.3g} units of 2^-24 B at {tuple(int(i) for i in at)}"
        + (f" (got {got[at]!r}, want {want[at]!r}, B {B[at]!r})" if s.size else "")))
    return worst


def gate_all(got, grads, bounds, G, what):
    """The gate on all eight tensors -> {tensor: largest share}; every tensor is compared before the first failure is raised."""
    used, failures = {}, []
    for name, g, want, B in zip(KEYS, got, grads, bounds):
        try:
            used[name] = gate(g, want, B, G, what, name)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    return used


# ------------------------------------------------------------------------------------------------ launches (GPU)
def pack_fold(hip, weights, A):
    """The FOLD weight image of one net: rnad_mlp_pack_fold_multi."""
    W = weights[0].shape[0]
    lib = hip.lib()
    packed = torch.empty((int(lib.rnad_mlp_fold_packed_size(A, W)),), dtype=torch.float32, device=weights[0].device)
    wp = (ctypes.c_void_p * 8)(*[w.data_ptr() for w in weights])
    op = (ctypes.c_void_p * 1)(packed.data_ptr())
    rc = lib.rnad_mlp_pack_fold_multi(1, A, W, wp, op, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rnad_last_error().decode()
    return packed


def backward_fold(hip, packed, obs, A, W, dlogits, dvalue, out, live=None, capacity=None):
    """rnad_mlp_backward_fold itself.  The Python wrapper rightly accepts only a tree's own table; the C contract is "the caller
    guarantees the premise" (every legal plane all ones or e0), which the fold cases satisfy.  The workspace starts as the poison."""
    lib = hip.lib()
    assert all(t.is_cuda and t.is_contiguous() for t in [packed, obs, dlogits, dvalue] + list(out))
    assert obs.dtype in POISON and dlogits.dtype == dvalue.dtype == torch.float32 and all(g.dtype == torch.float32 for g in out)
    N = obs.shape[0]
    cap = N if capacity is None else int(capacity)
    assert live is not None or cap == N
    nbytes = int(lib.rnad_mlp_backward_workspace(cap, A, W))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), POISON[torch.float32], dtype=torch.float32, device=obs.device)
    rows, count = (None, None) if live is None else (live.rows.data_ptr(), live.count.data_ptr())
    rc = lib.rnad_mlp_backward_fold(cap, rows, count, A, W, packed.data_ptr(), obs.data_ptr(), int(obs.dtype == torch.float16),
                                    dlogits.data_ptr(), dvalue.data_ptr(), *[g.data_ptr() for g in out], ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise hip.RnadHipError(lib.rnad_last_error().decode())
    return out
