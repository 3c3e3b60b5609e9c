"""numpy restatement of the lane draw of the compact replay (include/rnad_rng.h "THE LANE DRAW", csrc/replay.hip): the keyed bijection,
the drawn columns of a source and the rebuilt work lists.  Nothing here calls the library."""
import numpy as np

ROUNDS = 6  # RNAD_DRAW_ROUNDS
U32, U64 = np.uint32, np.uint64
_M32 = U64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, seed):
    """rnad_philox4x32_10 on arrays of counters (uint32 each), key = the two halves of `seed`; returns the four output words."""
    c = [np.asarray(x, U64) & _M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = U64(0xD2511F53) * c[0]
        p1 = U64(0xCD9E8D57) * c[2]
        c = [((p1 >> U64(32)) ^ c[1] ^ U64(k0)) & _M32, p1 & _M32, ((p0 >> U64(32)) ^ c[3] ^ U64(k1)) & _M32, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def half_bits(B):
    h = 1
    while (1 << (2 * h)) < B:
        h += 1
    return h


def _round(seed, source, B, r, x, mask):
    return philox4x32_10(x, source, r | (3 << 24), B & 0xFFFFFFFF, seed)[0] & U64(mask)


def _walk(seed, source, B, y, rounds, step):
    """Cycle walking: apply `step` to the entries of y until each lands in [0, B)."""
    h = half_bits(B)
    mask = (1 << h) - 1
    y = np.array(y, U64, ndmin=1)
    todo = np.ones(y.shape, bool)
    while todo.any():
        L, R = y[todo] >> U64(h), y[todo] & U64(mask)
        for r in rounds:
            L, R = step(L, R, _round, (seed, source, B, r), mask)
        y[todo] = (L << U64(h)) | R
        todo &= y >= U64(B)
    return y.astype(np.int64)


def sigma(seed, source, B, i):
    """sigma(i): ROUNDS rounds (L, R) -> (R, L ^ F_r(R)), walked into [0, B)."""
    return _walk(seed, source, B, i, range(ROUNDS), lambda L, R, F, key, m: (R, L ^ F(*key, R, m)))


def sigma_inv(seed, source, B, j):
    """sigma^-1(j): the rounds in reverse, (L, R) -> (R ^ F_r(L), L)."""
    return _walk(seed, source, B, j, range(ROUNDS - 1, -1, -1), lambda L, R, F, key, m: (R ^ F(*key, L, m), L))


def selected(seed, source, B, b, cols):
    """Membership of the columns `cols` in the draw of b out of B."""
    cols = np.asarray(cols, np.int64)
    if b <= 0:
        return np.zeros(cols.shape, bool)
    if b >= B:
        return np.ones(cols.shape, bool)
    return sigma_inv(seed, source, B, cols) < b


def draw_columns(seed, source, B, b):
    """The drawn columns, ascending (rnad_draw_columns)."""
    return np.flatnonzero(selected(seed, source, B, b, np.arange(B))).astype(np.int32)


def source_items(counts, chunk):
    """The work list a rollout leaves for a batch whose bucket b holds counts[b] lanes: items of at most `chunk` lanes, bucket by bucket
    ({begin, count, bucket, single}, csrc/bucket.hip items_phase)."""
    items, begin = [], 0
    for b, n in enumerate(counts):
        k = -(-n // chunk)
        for c in range(k):
            items.append((begin + c * chunk, min(chunk, n - c * chunk), b, int(k == 1)))
        begin += n
    return np.array(items, np.int32).reshape(-1, 4)


def rebuild_items(items, drawn, chunk, off, sole):
    """The work list of one source's stretch of a draw.  items: the source's work list; drawn: bool per source column; off: the first
    destination column of the stretch; sole: this source contributes every lane of the draw.  The drawn lanes of a bucket are
    repacked into items of at most `chunk` lanes, a bucket without drawn lanes gets none, `single` only when the bucket ends up
    with one item AND no other source adds into the same accumulators before the finish."""
    out, begin = [], off
    per_bucket = {}
    for b0, n, bucket, _ in items:
        per_bucket[int(bucket)] = per_bucket.get(int(bucket), 0) + int(np.count_nonzero(drawn[b0: b0 + n]))
    for bucket in sorted(per_bucket):  # (a source's columns are sorted by bucket)
        n = per_bucket[bucket]
        k = -(-n // chunk)
        for c in range(k):
            out.append((begin + c * chunk, min(chunk, n - c * chunk), bucket, int(sole and k == 1)))
        begin += n
    return np.array(out, np.int32).reshape(-1, 4)


def flush(acc, item, value):
    """csrc/bucket.hip learn_epilogue on a toy accumulator (one word per bucket): a `single` item flushes its bucket's table with a
    plain store, any other item adds."""
    _, _, bucket, single = (int(x) for x in item)
    acc[bucket] = value if single else acc[bucket] + value


def draw_kernel_scratch(so_path):
    """{kernel name: scratch bytes per lane} of every k_draw_* kernel in the built library, read as tests/_replayref.kernel_metadata reads
    k_behaviour_records': .hip_fatbin -> its offload bundles -> the gfx950 code object -> the amdhsa.kernels note."""
    import os
    import re
    import subprocess
    import tempfile

    import _regref as rr

    tools = {t: os.path.join(rr.LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    for t, p in tools.items():
        assert os.path.exists(p), f"{t} not found at {p}: the scratch invariant cannot be checked"
    out = {}
    with tempfile.TemporaryDirectory(prefix="draw_meta_") as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fat}", so_path, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(rr._BUNDLE), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        for i, s in enumerate(starts):
            part = blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            if b"k_draw_" not in part:
                continue
            bundle, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(bundle, "wb").write(part)
            subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={bundle}", f"--output={co}"])
            name = None
            for line in subprocess.check_output([tools["llvm-readobj"], "--notes", co], text=True).splitlines():
                m = re.match(r"^\s{2}(?:- |\s{2})(\.\w+):\s*(.*)$", line)
                if not m:
                    continue
                if line.lstrip().startswith("- "):
                    name = None
                value = m.group(2).strip().strip("'\"")
                if m.group(1) == ".name":
                    name = value
                    out.setdefault(name, None)
                elif m.group(1) == ".private_segment_fixed_size" and name is not None:
                    out[name] = int(value)
    return {k: v for k, v in out.items() if "k_draw_" in k}
