"""What the compact-replay tests share (tests/test_compact_replay.py on the CPU, tests/test_hip_compact_replay.py on the GPU): the numpy
restatement of rnad_bucket_behaviour_records (include/rnad_hip.h), synthetic fast-record / policy-row tables, and the kernel metadata of
k_behaviour_records in the built library.  numpy only; nothing here calls a project kernel."""
import os
import re

import numpy as np

import _learnref as lr
import _regref as rr


def fast_stride(A):
    return 4 + 4 * A


def policy_stride(A):
    return (A + 3) & ~3


def behaviour_records(fast, mu, A):
    """out = fast with floats 4 + 2A .. rebuilt: out[r][4 + 2A + a] = fast[r][4 + a] / mu[r][a], out[r][4 + 3A + a] = 1 / mu[r][a], in fp32
    (IEEE division; numpy's float32 division is correctly rounded)."""
    fast, mu = np.asarray(fast, np.float32), np.asarray(mu, np.float32)
    assert fast.shape[1] == fast_stride(A) and mu.shape[1] == policy_stride(A)
    out = fast.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 4 + 2 * A: 4 + 3 * A] = fast[:, 4: 4 + A] / mu[:, :A]
        out[:, 4 + 3 * A: 4 + 4 * A] = np.float32(1) / mu[:, :A]
    return out


def draw_mu(rng, legal):
    """Policy rows [N, policy_stride(A)] by _learnref.behaviour: at least 1e-3 on legal actions (so that no denormal decides a bit), exact
    zeros on illegal ones and in the pad columns.  Rows are redrawn until they meet the floor."""
    N, A = legal.shape
    mu, _ = lr.behaviour(rng, legal)
    for _ in range(200):
        bad = np.flatnonzero(((legal > 0) & (mu < 1e-3)).any(-1))
        if bad.size == 0:
            break
        mu[bad] = lr.behaviour(rng, legal[bad])[0]
    else:
        raise AssertionError("rows below the floor remain")
    assert (mu[legal == 0] == 0).all()
    out = np.zeros((N, policy_stride(A)), np.float32)
    out[:, :A] = mu
    return out


def draw_fast(rng, legal):
    """A synthetic fast-record table [N, 4 + 4A]: arbitrary bits in the columns that only travel, a processed policy (multiples of 1 / 32
    on the legal actions) in columns 4 .. 4 + A, and the on-policy ratios of an unrelated pi in the last 2A (they must be replaced)."""
    N, A = legal.shape
    fast = rng.standard_normal((N, fast_stride(A))).astype(np.float32)
    fast[:, 3] = rng.integers(0, 2 ** 24, N).astype(np.uint32).view(np.float32)
    fast[:, 4: 4 + A] = (rng.integers(0, 33, (N, A)) / 32.0).astype(np.float32) * legal
    return fast


_KERNEL = re.compile(r"k_behaviour_recordsILi(\d+)EE")


def kernel_metadata(so_path):
    """{A: dict(scratch, vgpr, sgpr, lds)} of every k_behaviour_records instantiation in the built library, read as _regref.kernel_metadata
    reads k_reg_solve's: .hip_fatbin -> its offload bundles -> the gfx950 code object -> the amdhsa.kernels note."""
    import subprocess
    import tempfile

    tools = {t: os.path.join(rr.LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    kernels = []
    with tempfile.TemporaryDirectory(prefix="replay_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(rr._BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_behaviour_records" not in part:
                continue
            bundle, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(bundle, "wb").write(part)
            subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={bundle}", f"--output={co}"])
            cur = None
            for line in subprocess.check_output([tools["llvm-readobj"], "--notes", co], text=True).splitlines():
                m = re.match(r"^\s{2}(?:- |\s{2})(\.\w+):\s*(.*)$", line)
                if not m:
                    continue
                if line.lstrip().startswith("- "):
                    cur = {}
                    kernels.append(cur)
                if cur is not None:
                    cur[m.group(1)] = m.group(2).strip().strip("'\"")
    table = {}
    for k in kernels:
        m = _KERNEL.search(k.get(".name", ""))
        if m:
            table[int(m.group(1))] = dict(scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"]), sgpr=int(k[".sgpr_count"]),
                                          lds=int(k.get(".group_segment_fixed_size", 0)))
    return table
