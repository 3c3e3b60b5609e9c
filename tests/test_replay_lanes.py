"""The lane draw of the compact replay, CPU half: the keyed bijection of include/rnad_rng.h (rnad_draw_columns against the numpy
restatement of tests/_drawref.py), its uniformity, and the rebuilt work lists restated in numpy and held to hand-built lists.
tests/test_hip_replay_lanes.py holds the GPU half (rnad_bucket_draw_lanes, the learner on a draw, the trainer)."""
import itertools
import random

import numpy as np
import pytest

import _drawref as dr


def _hip():
    import rnad_hip

    return rnad_hip


# ------------------------------------------------------------------------------------------------ the draw contract
def test_sigma_is_a_bijection_and_sigma_inv_its_inverse():
    for B in (1, 2, 3, 5, 16, 17, 64, 100, 257):
        cols = np.arange(B)
        fwd = dr.sigma(77, 3, B, cols)
        assert np.array_equal(np.sort(fwd), cols), f"B={B}: sigma is not a permutation"
        assert np.array_equal(dr.sigma_inv(77, 3, B, fwd), cols), f"B={B}: sigma_inv is not its inverse"


@pytest.mark.parametrize("B", [1, 2, 3, 64, 100, 4096])
def test_draw_columns_equals_the_restatement(B):
    hip = _hip()
    for b in sorted({0, 1, B - 1, B}):
        got = hip.draw_columns(1234, 2, B, b)
        assert got.dtype == np.int32 and got.shape == (b,)
        assert np.array_equal(got, dr.draw_columns(1234, 2, B, b)), f"B={B} b={b}"
        assert (np.diff(got) > 0).all() and (b == 0 or (got[0] >= 0 and got[-1] < B)), "exactly b distinct ascending columns"
        assert np.array_equal(got, hip.draw_columns(1234, 2, B, b)), "two calls agree"
        # the drawn set is { sigma(i) : i < b }
        assert np.array_equal(got, np.sort(dr.sigma(1234, 2, B, np.arange(b)))) if 0 < b < B else True
    if B >= 64:
        b = B // 4
        base = hip.draw_columns(1234, 2, B, b)
        assert not np.array_equal(base, hip.draw_columns(1235, 2, B, b)), "another seed, another set"
        assert not np.array_equal(base, hip.draw_columns(1234, 3, B, b)), "another source, another set"
        assert not np.array_equal(base, hip.draw_columns(1234 + (1 << 32), 2, B, b)), "the high half of the seed counts"


def test_draw_columns_at_2_to_20_sampled():
    hip = _hip()
    B = 1 << 20
    rng = np.random.default_rng(20)
    cols = np.unique(np.concatenate([rng.integers(0, B, 4096), [0, 1, B - 2, B - 1]]))
    for b in (0, 1, B - 1, B, B // 3):
        got = hip.draw_columns(99, 5, B, b)
        assert got.shape == (b,) and (np.diff(got) > 0).all()
        member = np.zeros(B, bool)
        member[got] = True
        assert np.array_equal(member[cols], dr.selected(99, 5, B, b, cols)), f"b={b}: the sampled columns' membership"


def test_draw_columns_refuses():
    hip = _hip()
    for args in ((0, 0, 0, 0), (0, 0, 8, 9), (0, 0, 8, -1), (0, -1, 8, 1), (0, 0, (1 << 30) + 1, 1)):
        with pytest.raises(hip.RnadHipError, match="outside|negative"):
            hip.draw_columns(*args)


# ------------------------------------------------------------------------------------------------ uniformity
# B = 64, b = 16 over M seeds.  A uniform 16-subset holds a given column with p1 = 1/4 and a given pair with p2 = 16 * 15 / (64 * 63)
# (hypergeometric), so over M independent draws the counts are Binomial(M, p): the condition is |count - M p| <= 6 sqrt(M p (1 - p)) for
# each of the 64 columns and the 2016 pairs.  M = 4000: the pair counts have mean 238 and sigma 15, large enough for the normal tail
# (2 * 1e-9 per count, 4e-6 over all 2080), and the reference generator itself (python's random.sample, what Buffer.sample draws the
# subsets with) stays inside with room, which the test shows first.
UNI_B, UNI_b, UNI_M = 64, 16, 4000


def _worst_deviations(sets):
    """(max over columns, max over pairs) of |count - mean| / sigma for M drawn subsets."""
    M = len(sets)
    member = np.zeros((M, UNI_B), np.float64)
    for m, s in enumerate(sets):
        member[m, s] = 1
    single = member.sum(0)
    joint = member.T @ member
    p1 = UNI_b / UNI_B
    p2 = UNI_b * (UNI_b - 1) / (UNI_B * (UNI_B - 1))
    dev1 = np.abs(single - M * p1) / np.sqrt(M * p1 * (1 - p1))
    iu = np.triu_indices(UNI_B, 1)
    dev2 = np.abs(joint[iu] - M * p2) / np.sqrt(M * p2 * (1 - p2))
    return dev1.max(), dev2.max()


def test_uniformity_of_columns_and_pairs():
    hip = _hip()
    gen = random.Random(2024)
    ref = _worst_deviations([gen.sample(range(UNI_B), UNI_b) for _ in range(UNI_M)])
    print(f"random.sample: worst column {ref[0]:.2f} sigma, worst pair {ref[1]:.2f} sigma")
    assert ref[0] <= 6 and ref[1] <= 6, "the bound holds for the reference generator at this M"
    for source in (0, 3):
        got = _worst_deviations([hip.draw_columns(seed, source, UNI_B, UNI_b) for seed in range(UNI_M)])
        print(f"lane draw, source {source}: worst column {got[0]:.2f} sigma, worst pair {got[1]:.2f} sigma")
        assert got[0] <= 6 and got[1] <= 6, f"source {source}: inclusion counts outside 6 sigma ({got[0]:.2f}, {got[1]:.2f})"
    # across sources under ONE seed the subsets are independent draws too
    got = _worst_deviations([hip.draw_columns(7, source, UNI_B, UNI_b) for source in range(UNI_M)])
    assert got[0] <= 6 and got[1] <= 6


# ------------------------------------------------------------------------------------------------ the item rebuild
CHUNK = 4


def _drawn(B, cols):
    d = np.zeros(B, bool)
    d[list(cols)] = True
    return d


def test_source_items_by_hand():
    # buckets of 5, 0, 3 and 1 lanes at 4 lanes per item
    want = [(0, 4, 0, 0), (4, 1, 0, 0), (5, 3, 2, 1), (8, 1, 3, 1)]
    assert dr.source_items([5, 0, 3, 1], CHUNK).tolist() == [list(w) for w in want]


def test_rebuild_repacks_a_bucket_into_full_items():
    # bucket 0 holds 10 lanes in three source items (4, 4, 2); 2 + 3 + 1 = 6 of them are drawn: ONE full item and one of 2, not three
    items = dr.source_items([10, 2], CHUNK)
    assert items.tolist() == [[0, 4, 0, 0], [4, 4, 0, 0], [8, 2, 0, 0], [10, 2, 1, 1]]
    drawn = _drawn(12, [0, 3, 4, 5, 7, 9, 11])
    got = dr.rebuild_items(items, drawn, CHUNK, off=20, sole=False)
    assert got.tolist() == [[20, 4, 0, 0], [24, 2, 0, 0], [26, 1, 1, 0]]
    # a program that keeps one (under-filled) item per source item fails this
    naive = [[20, 2, 0, 0], [22, 3, 0, 0], [25, 1, 0, 0], [26, 1, 1, 0]]
    assert got.tolist() != naive
    # the same draw as the only contributing source: bucket 1 ends up with one item and may flush with a plain store; bucket 0 has two
    assert dr.rebuild_items(items, drawn, CHUNK, off=0, sole=True).tolist() == [[0, 4, 0, 0], [4, 2, 0, 0], [6, 1, 1, 1]]


def test_rebuild_drops_empty_buckets_and_handles_the_edges():
    items = dr.source_items([3, 0, 2, 4], CHUNK)
    assert dr.rebuild_items(items, _drawn(9, []), CHUNK, off=5, sole=False).shape == (0, 4), "nothing drawn: no item"
    got = dr.rebuild_items(items, _drawn(9, [5, 6, 7, 8]), CHUNK, off=5, sole=False)
    assert got.tolist() == [[5, 4, 3, 0]], "buckets 0 and 2 received no lane: no item for them"
    everything = dr.rebuild_items(items, _drawn(9, range(9)), CHUNK, off=0, sole=True)
    assert everything.tolist() == items.tolist(), "every lane of the only source drawn: the source's own work list"
    # an exact multiple of the chunk: no empty trailing item
    full = dr.rebuild_items(dr.source_items([12], CHUNK), _drawn(12, range(4, 12)), CHUNK, off=0, sole=False)
    assert full.tolist() == [[0, 4, 0, 0], [4, 4, 0, 0]]


def test_single_items_of_two_sources_would_lose_a_sum():
    """Two sources each hold bucket 1's only item.  The learner is called once per source before ONE finish, and a `single` item flushes
    its bucket's table with a plain store (csrc/bucket.hip learn_epilogue): marked single, the second call overwrites the first."""
    src = [dr.source_items([2, 3], CHUNK), dr.source_items([1, 2], CHUNK)]
    assert all(s[s[:, 2] == 1][:, 3].tolist() == [1] for s in src), "in each source the bucket's only item"
    drawn = [_drawn(5, [0, 2, 3]), _drawn(3, [1, 2])]
    lists = [dr.rebuild_items(src[0], drawn[0], CHUNK, off=0, sole=False), dr.rebuild_items(src[1], drawn[1], CHUNK, off=3, sole=False)]
    assert lists[0].tolist() == [[0, 1, 0, 0], [1, 2, 1, 0]] and lists[1].tolist() == [[3, 2, 1, 0]]
    sums = [{0: 10, 1: 200}, {1: 3000}]  # what each source's lanes add into a bucket

    def run(work_lists):
        acc = {0: 0, 1: 0}
        for items, s in zip(work_lists, sums):
            for item in items:
                dr.flush(acc, item, s[int(item[2])])
        return acc

    assert run(lists) == {0: 10, 1: 3200}, "single = 0: both sources' sums meet in the accumulators"
    wrong = [np.array(x) for x in lists]
    for w in wrong:
        w[:, 3] = 1  # what the source lists said: each is its bucket's only item
    assert run(wrong) == {0: 10, 1: 3000}, "single = 1 in both: source 0's sum for bucket 1 is lost"
    # one source contributing alone keeps the plain store
    alone = dr.rebuild_items(src[0], drawn[0], CHUNK, off=0, sole=True)
    assert alone[:, 3].tolist() == [1, 1] and run([alone]) == {0: 10, 1: 200}


def test_rebuild_against_a_brute_force_partition():
    """Random lists: the rebuilt items tile [off, off + drawn lanes) in order, never cross a bucket, never exceed the chunk, and only a
    bucket's last item is under-filled."""
    rng = np.random.default_rng(8)
    for trial, sole in itertools.product(range(20), (False, True)):
        counts = rng.integers(0, 14, size=6)
        items = dr.source_items(counts, CHUNK)
        B = int(counts.sum())
        drawn = rng.random(B) < rng.random()
        got = dr.rebuild_items(items, drawn, CHUNK, off=7, sole=sole)
        bucket_of = np.repeat(np.arange(6), counts)
        want_per_bucket = np.bincount(bucket_of[drawn], minlength=6)
        at = 7
        for b in range(6):
            mine = got[got[:, 2] == b]
            assert mine[:, 1].sum() == want_per_bucket[b]
            assert (mine[:-1, 1] == CHUNK).all() and (mine[:, 1] >= 1).all() and (mine[:, 1] <= CHUNK).all()
            assert (mine[:, 3] == int(sole and len(mine) == 1)).all()
            for begin, n, _, _ in mine:
                assert begin == at
                at += n
        assert at == 7 + int(drawn.sum())


def test_no_draw_kernel_uses_scratch():
    table = dr.draw_kernel_scratch(_hip().SO_PATH)
    print(table)
    assert len(table) == 5, "k_draw_count and k_draw_gather for one- and two-byte states, k_draw_scan"
    assert all(v == 0 for v in table.values()), table
