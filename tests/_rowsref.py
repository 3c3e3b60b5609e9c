"""Inputs, the fp64 reference and the error bound for the shape sweep of the fused rows kernel (csrc/mlp_rows.hip:
k_rows_forward_records<A, ObsT, FOLD, MODE, SPLIT>) -- tests/test_rows_shapes.py on the CPU, tests/test_hip_rows_shapes.py on the GPU.

The reference is the net of nn/net.py written out in double precision on the UNFOLDED observation [ev | legal] (2 A^2 features):
z = W0 x + b0, ReLU, both heads -- logits and v from the learner's weights, v_target from the target's.  Nothing of the kernels'
packing, weight-image layout or legal fold is shared with it, so the fold is held to the unfolded function, the two rows of the
absorbing state included.  For an fp16 table the reference takes the fp16-rounded values (exact in fp64).

The gate is relative to what the arithmetic can lose: per row and output
    B = sum_h |w1[o, h]| (sum_k |W0[h, k]| |x~_k| + |b0[h]|) + |b1[o]|,      |got - want| <= G * 2^-24 * B
with x~ = |ev| and the legal plane taken as all ones in EVERY row: the fold's indicator weight w_ind = W_legal[0] - sum_k W_legal[k]
is rounded at the size of the whole sum also where it cancels (the absorbing rows).  G is fixed in tests/test_rows_shapes.py from plain
fp32 torch on these very inputs, never from a kernel's output.

Two input families.  "init": the default MLP init on the tree's own observations.  "wide": the first-layer matrices of the learner and
the target and the ev plane are random sign x random 23-bit mantissa x 2^e (e uniform in [-6, 1) for the ev columns of the weights,
[-12, -5) for their legal columns, [-8, 1) for ev; normal numbers only) with a few hand-placed values -- all-ones mantissas and exact
bf16 ties.  On "init" inputs a dropped W_l x_h, W_h x_l or W_m x_m product of the split first layer (chain_split) stays inside any
usable gate, and with independent signs everywhere it still averages out over the K inputs and W hidden units to a few 2^-24 B, no more
than plain fp32 summation loses.  So "wide" also lines signs up along one path: the m and l pieces of every value carry the value's
sign (`wide(aligned=True)`), the ev weights of a hidden unit share one sign, every fourth row has a positive ev plane, and the value
heads' second-layer weights are positive on the units such a row switches on -- a relative error of 2^-17 in the first layer then
reaches v and v_target of those rows undiminished (28 - 48 units of 2^-24 B, tests/test_rows_shapes.py), while three rows in four, the
policy head and the "init" family keep independent signs."""
import functools
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import torch

U = 2.0 ** -24
FAMILIES = ("init", "wide")
WIDTHS_EXTRA = (32, 96, 160, 224)  # T = 1, 3, 5, 7 compute waves (width 256: T = 8)

# the small trees of the sweep, one per A (2S rows: 22, 684, 1642, 548, 1304 -- tests/test_rows_shapes.py holds the counts)
SMALL = {
    1: dict(A=1, C=1, depth=10, seed=0),  # fewer than 32 rows: a single partial half step
    2: dict(A=2, C=1, depth=5, seed=1),
    3: dict(A=3, C=1, depth=4, seed=0),
    4: dict(A=4, C=1, depth=3, seed=2),
    5: dict(A=5, C=1, depth=3, seed=3),
}
SMALL_ROWS = {1: 22, 2: 684, 3: 1642, 4: 548, 5: 1304}
# the trees of the chunk loop: at 256 CUs some workgroup walks three chunks, ends on a short chunk and on a half step
CHUNK = {
    2: dict(A=2, C=1, depth=9, seed=0),
    3: dict(A=3, C=1, depth=6, seed=0),
    4: dict(A=4, C=1, depth=5, seed=0),
    5: dict(A=5, C=1, depth=5, seed=1, prune=(1, 3)),
}
CHUNK_ROWS = {2: 174764, 3: 132862, 4: 139812, 5: 162546}
MAX_ROWS = 180000  # no case of the sweep is larger
LIST_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 257)
POISON = {torch.float32: 1e30, torch.float16: 6e4}  # finite: mlp_rows.o is built with -fno-honor-nans


# ------------------------------------------------------------------------------------------------ trees and observations on the host
def host_tree(A, C, depth, seed, prune=(0, 0), threshold=None):
    """The arrays of tests/test_hip_bucket.py::_native_tree(...) from the host generator (no device)."""
    import rnad_hip

    thr = threshold if threshold is not None else (0.0 if C == 1 else 0.5 / C)
    return rnad_hip.tree_generate(A, C, depth, float(thr), (-1.0, 1.0), prune, seed)


def host_observations(arrs):
    """[2S, 2, A, A] fp32: row = player * S + state, as TreeHandle.observations_table() (the CPU oracle's observe)."""
    from oracle import oracle

    ev, legal = arrs["expected_value"].numpy(), arrs["legal"].numpy()
    S = ev.shape[0]
    idx = np.arange(S, dtype=np.int64)
    return torch.from_numpy(np.concatenate([oracle.observe(ev, legal, idx, np.full(S, p, np.int64))[0] for p in (0, 1)]))


def chunk_list_length(N):
    """Rows of the shuffled list of a chunk-loop case: nearly all N, not a multiple of 32."""
    n = N - 45
    return n - 5 if n % 32 == 0 else n


def shuffled(N, seed):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ the two input families
SPECIAL_BITS = (0x3FFFFFFF, 0xBFFFFFFF, 0x3F7FFFFF, 0x3EFFFFFF)  # all-ones mantissas (1.9999999, its negative, 0.99999994, 0.49999997)
SPECIAL = (1 + 2.0**-8, 1 + 2.0**-8 + 2.0**-16, -(1 + 2.0**-8), 1 + 2.0**-7 + 2.0**-8, 0.5 + 2.0**-9 + 2.0**-17, 1 + 2.0**-8 + 2.0**-16 + 2.0**-23)


def wide(shape, lo, hi, g, aligned=False):
    """fp32 tensor: random sign, random 23-bit mantissa, exponent uniform in [lo, hi); the hand-placed values in its first entries.
    aligned: mantissa bits 8 and 17 (from the top) cleared, 9 and 18 set -- both bf16 roundings of split8 then go DOWN, so the m and l
    pieces are non-zero and carry the sign of the value (19 of the 23 bits stay random)."""
    n = int(np.prod(shape))
    mant = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64).numpy()
    if aligned:
        mant = (mant & ~((1 << 15) | (1 << 6))) | (1 << 14) | (1 << 5)
    exp = torch.randint(lo, hi, (n,), generator=g, dtype=torch.int64).numpy() + 127
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64).numpy()
    x = ((sign << 31) | (exp << 23) | mant).astype(np.uint32).view(np.float32).copy()
    hand = np.concatenate([np.array(SPECIAL_BITS, np.uint32).view(np.float32), np.array(SPECIAL, np.float32)])
    k = min(n, hand.size)
    x[:k] = hand[:k]
    assert np.isfinite(x).all() and (np.abs(x) >= 2.0**-126).all()
    return torch.from_numpy(x).reshape(shape)


def nets(A, W, family, seed=0):
    """Learner, target and the two regularisation nets (CPU, fp32), default init; "wide": the first-layer matrices of the learner and
    the target replaced."""
    from nn.net import MLP

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * A + W + seed)
        out = [MLP(A, W) for _ in range(4)]
    if family == "wide":
        g = torch.Generator().manual_seed(77 + 1000 * A + W + seed)
        with torch.no_grad():
            for net in out[:2]:
                for fc, fc1 in ((net.value_fc0, net.value_fc1), (net.policy_fc0, net.policy_fc1)):
                    w = wide(fc.weight.shape, -6, 1, g, aligned=True)
                    sign = torch.where(torch.rand((W, 1), generator=g) < 0.5, -1.0, 1.0)
                    w[:, :A * A] = sign * w[:, :A * A].abs()       # one sign per hidden unit (see the module docstring)
                    w[:, A * A:] = wide((W, A * A), -12, -5, g)    # legal columns: wide too, but small next to the ev part
                    fc.weight.copy_(w)
                    if fc1 is net.value_fc1:                       # the units a positive row switches on: their value weights positive
                        up = sign[:, 0] > 0
                        fc1.weight[:, up] = fc1.weight[:, up].abs()
    else:
        assert family == "init"
    return out


def wide_ev(N, A, seed=0):
    """[N, A, A] fp32: the ev plane of the "wide" family; every fourth row is positive throughout."""
    ev = wide((N, A, A), -8, 1, torch.Generator().manual_seed(555 + 10 * A + seed), aligned=True)
    ev[::4] = ev[::4].abs()
    return ev


def observations(obs, family, half=False, seed=0):
    """The observation table of a case from the tree's own [2S, 2, A, A] fp32 table: "wide" replaces the ev plane; half rounds to fp16."""
    obs = obs.clone()
    if family == "wide":
        obs[:, 0] = wide_ev(obs.shape[0], obs.shape[-1], seed)
    return obs.half() if half else obs


# ------------------------------------------------------------------------------------------------ fp64 reference, bound, gate
def _weights64(net):
    return [w.detach().cpu().double() for w in net._weights()]


def reference(learner, target, obs, block=1 << 14):
    """fp64 logits [N, A], v [N], v_target [N] and their bounds B (same shapes) on obs [N, 2, A, A] (fp32 or fp16): read-only numpy."""
    N, A = obs.shape[0], obs.shape[-1]
    wl, wt = _weights64(learner), _weights64(target)
    heads = ((wl[4:8], A), (wl[0:4], 1), (wt[0:4], 1))  # logits, v, v_target
    outs = [np.empty((N, n)) for _, n in heads]
    bounds = [np.empty((N, n)) for _, n in heads]
    for r0 in range(0, N, block):
        x = obs[r0:r0 + block].reshape(-1, 2 * A * A).double()
        xt = x.abs()
        xt[:, A * A:] = 1.0
        for i, ((W0, b0, W1, b1), _) in enumerate(heads):
            outs[i][r0:r0 + block] = (torch.relu(x @ W0.T + b0) @ W1.T + b1).numpy()
            bounds[i][r0:r0 + block] = ((xt @ W0.abs().T + b0.abs()) @ W1.abs().T + b1.abs()).numpy()
    for a in outs + bounds:
        a.setflags(write=False)
    return types.SimpleNamespace(logits=outs[0], v=outs[1][:, 0], v_target=outs[2][:, 0], B_logits=bounds[0], B_v=bounds[1][:, 0],
                                 B_v_target=bounds[2][:, 0])


def fp32_torch(learner, target, obs):
    """Plain fp32 torch on the CPU: logits, v, v_target."""
    x = obs.reshape(obs.shape[0], -1).float()
    with torch.no_grad():
        logits = learner.policy_fc1(torch.relu(learner.policy_fc0(x)))
        v = learner.value_fc1(torch.relu(learner.value_fc0(x)))
        vt = target.value_fc1(torch.relu(target.value_fc0(x)))
    return logits.numpy(), v.numpy()[:, 0], vt.numpy()[:, 0]


def normalised(got, want, B):
    """|got - want| in units of 2^-24 B."""
    return np.abs(np.asarray(got, np.float64) - want) / (U * B)


def gate(got, want, B, G, what="", rows=None):
    """|got - want| <= G 2^-24 B on `rows` (None: all), through np.testing.assert_allclose so that tests/conftest.py records the share
    of the gate that was used."""
    got = np.asarray(got, np.float64)
    if rows is not None:
        got, want, B = got[rows], want[rows], B[rows]
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = normalised(got, want, B)
    np.testing.assert_allclose(err, np.zeros_like(err), rtol=0, atol=G, err_msg=f"{what} (|error| / (2^-24 B))")
    return float(err.max()) if err.size else 0.0


# ------------------------------------------------------------------------------------------------ the cases of the sweep
def sweep_cases():
    """(kind, A, width, family, half) of every reference the GPU sweep compares with."""
    small = [("small", A, W, family, half) for A in SMALL for W in (256,) + (WIDTHS_EXTRA if A in (3, 5) else ())
             for family in FAMILIES for half in (False, True)]
    return small + [("chunk", A, 256, "wide", half) for A in CHUNK for half in (False, True)]


@functools.lru_cache(maxsize=None)
def tree_observations(kind, A):
    """The fp32 observation table of SMALL[A] / CHUNK[A], built on the host."""
    return host_observations(host_tree(**(SMALL if kind == "small" else CHUNK)[A]))


@functools.lru_cache(maxsize=None)
def case(kind, A, W, family, half):
    """Nets, observation table and fp64 reference of one case, built once and left unchanged."""
    obs = observations(tree_observations(kind, A), family, half)
    n = nets(A, W, family)
    return types.SimpleNamespace(kind=kind, A=A, W=W, family=family, half=half, N=obs.shape[0], obs=obs, nets=n, ref=reference(n[0], n[1], obs))


# ------------------------------------------------------------------------------------------------ the kernel's partition, restated
def partition(N, cus, table_rows=None):
    """[(my_tiles, steps, chunks)] per workgroup: N rows (the list's count, or the table's) over the grid the host sizes from the
    TABLE's rows (2S: a list's count lives in device memory) -- 32-row tiles, 64-row steps, 4 steps to a chunk."""
    host_tiles = ((N if table_rows is None else table_rows) + 31) // 32
    grid = max(1, min((host_tiles + 1) // 2, cus))
    n_tiles = (N + 31) // 32
    base, rem = divmod(n_tiles, grid)
    out = []
    for b in range(grid):
        my_tiles = base + (1 if b < rem else 0)
        steps = (my_tiles + 1) // 2
        out.append((my_tiles, steps, (steps + 3) // 4))
    assert sum(p[0] for p in out) == n_tiles
    return out


def partition_properties(N, cus, table_rows=None):
    p = partition(N, cus, table_rows)
    return dict(three_chunks=any(c >= 3 for _, _, c in p),                      # both partial-sum / staged buffers used again
                short_last_chunk=any(c >= 2 and s % 4 != 0 for _, s, c in p),    # a last chunk of fewer than 4 steps behind a full one
                half_step=any(t % 2 == 1 for t, _, _ in p),
                partial_tile=N % 32 != 0,
                empty=sum(1 for t, _, _ in p if t == 0) / len(p))


# ------------------------------------------------------------------------------------------------ the split first layer, emulated
def split3(x):
    """x fp32 -> (h, m, l) in torch bf16 with h + m + l == x: round to nearest each time, as split8 of csrc/mlp_rows.hip."""
    x = x.float()
    h = x.bfloat16()
    r = x - h.float()
    m = r.bfloat16()
    q = r - m.float()
    return h, m, q.bfloat16()


PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")  # weight piece, input piece; the kernel's order, small terms first


def fold(W0, b0, A):
    """fp32 [W, 2 A^2], [W] -> the folded first layer [W, A^2 + 1], [W] as fold_hidden_unit computes it (s summed in ascending k)."""
    s = torch.zeros_like(b0)
    for k in range(A * A):
        s = s + W0[:, A * A + k]
    return torch.cat([W0[:, :A * A], (W0[:, A * A] - s)[:, None]], 1), b0 + s


def fold_obs(obs):
    """[N, 2, A, A] -> [N, A^2 + 1] fp32: ev | 1 - legal[0][1] (obs_feature)."""
    N, A = obs.shape[0], obs.shape[-1]
    flat = obs.reshape(N, -1).float()
    return torch.cat([flat[:, :A * A], (1.0 - flat[:, A * A + 1])[:, None]], 1)


def split_chain(net_head, obs, drop=None):
    """One head (W0, b0, W1, b1: fp32) on foldable obs with the split first layer emulated: the products of the bf16 pieces in fp64
    (each is exact in fp32), z rounded to fp32, the second layer in fp64.  drop: one of PRODUCTS left out."""
    W0, b0, W1, b1 = [w.detach().float() for w in net_head]
    A = obs.shape[-1]
    Wf, bf = fold(W0, b0, A)
    x = fold_obs(obs)
    wp = dict(zip("hml", (p.double() for p in split3(Wf))))
    xp = dict(zip("hml", (p.double() for p in split3(x))))
    z = bf.double().expand(x.shape[0], -1).clone()
    for name in PRODUCTS:
        if name != drop:
            z = z + xp[name[1]] @ wp[name[0]].T
    return (torch.relu(z.float()).double() @ W1.double().T + b1.double()).numpy()


# ------------------------------------------------------------------------------------------------ what can be launched
def launchable(lib, W=256, A_range=range(0, 10)):
    """Every (A, fold, mode, split) the host functions of csrc/mlp_rows.hip let rows_launch select at width W: mode 0 / 1 by
    rnad_mlp_rows_records_supported, 2 by rnad_mlp_rows_actor_supported, split by rnad_mlp_rows_uses_split (non-zero: launchable)."""
    out = []
    for A in A_range:
        for fold_ in (False, True):
            for mode in (0, 1, 2):
                ok = lib.rnad_mlp_rows_actor_supported(A, W, int(fold_)) if mode == 2 else lib.rnad_mlp_rows_records_supported(A, W, int(fold_), mode)
                if not ok:
                    continue
                out.append((A, fold_, mode, False))
                if lib.rnad_mlp_rows_uses_split(A, W, int(fold_), mode):
                    out.append((A, fold_, mode, True))
    return out


# ------------------------------------------------------------------------------------------------ kernel metadata of the built library
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
_KERNEL = re.compile(r"k_rows_forward_recordsILi(\d+)E(f|6__half)Lb([01])ELi(\d+)ELb([01])EEE")
_BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


@functools.lru_cache(maxsize=None)
def rows_kernel_metadata(so_path, arch="gfx950"):
    """{(A, half, fold, mode, split): dict(scratch, vgpr, agpr, sgpr, lds)} of every k_rows_forward_records instantiation in the built
    library: .hip_fatbin (llvm-objcopy) -> its offload bundles -> the gfx950 code objects (clang-offload-bundler) -> the
    amdhsa.kernels note (llvm-readobj).  A missing tool is an error."""
    tools = {t: os.path.join(LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    out = {}
    with tempfile.TemporaryDirectory(prefix="rows_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(_BUNDLE), blob)]  # one bundle per translation unit
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_rows_forward_records" not in part:
                continue
            bundle, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(bundle, "wb").write(part)
            subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}",
                                   f"--input={bundle}", f"--output={co}"])
            notes = subprocess.check_output([tools["llvm-readobj"], "--notes", co], text=True)
            cur = None
            for line in notes.splitlines():
                m = re.match(r"^\s{2}(?:- |\s{2})(\.\w+):\s*(.*)$", line)  # keys of a kernel's own map (its arguments sit deeper)
                if not m:
                    continue
                if line.lstrip().startswith("- "):
                    cur = {}
                    out.setdefault("_all", []).append(cur)
                if cur is not None:
                    cur[m.group(1)] = m.group(2).strip().strip("'\"")
    table = {}
    for k in out.get("_all", []):
        m = _KERNEL.search(k.get(".name", ""))
        if not m:
            continue
        key = (int(m.group(1)), m.group(2) != "f", m.group(3) == "1", int(m.group(4)), m.group(5) == "1")
        table[key] = dict(scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"]), agpr=int(k.get(".agpr_count", 0)),
                          sgpr=int(k[".sgpr_count"]), lds=int(k[".group_segment_fixed_size"]))
    return table
