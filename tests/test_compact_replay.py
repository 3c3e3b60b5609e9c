"""Compact replay without a GPU (tests/test_hip_compact_replay.py holds the kernel, the learner and the trainer to the same statements on
an MI355X).

1. Record restatement.  rnad_bucket_behaviour_records precomputes, per (player, state) row and action, the two quantities the learner
   reads of the acting policy: pi_processed[a] / mu[a] and 1 / mu[a].  The reference forms them per SLOT (learn/vtrace.py:199-204):
   sum(onehot * pi) / sum(onehot * mu) and sum(onehot) / sum(onehot * mu) with `* valid + (1 - valid)` on every selected probability.  For
   every legal action with mu > 0, at A = 1 .. 8, the two are the same fp32 bits -- which is what licenses the per-row precomputation.
2. Ring bookkeeping of environment.episode.CompactBuffer on CPU tensors with a stub plan: eviction order, slot reuse without
   reallocation, k distinct slots per draw, uniform draws, every refusal.
3. The entry point: header, export, no scratch in any of the eight instantiations of the built library."""
import random
import types

import numpy as np
import pytest
import torch

import _learnref as lr
import _replayref as rp


# ------------------------------------------------------------------------------------------------ 1. the record transform
def _per_slot_ratios(pi, mu, act):
    """_policy_ratio of learn/vtrace.py:199-204 in fp32 on valid slots, written out: the sums run over the actions in index order."""
    f = np.float32
    A = pi.shape[-1]
    oh = (np.arange(A) == act[:, None]).astype(f)
    valid = np.ones(len(act), f)

    def select(x):
        s = (oh[:, 0] * x[:, 0]).astype(f)
        for a in range(1, A):
            s = (s + (oh[:, a] * x[:, a]).astype(f)).astype(f)
        return (s * valid + (f(1) - valid)).astype(f)

    return (select(pi) / select(mu)).astype(f), (select(np.ones_like(pi)) / select(mu)).astype(f)


@pytest.mark.parametrize("A", lr.A_RANGE)
def test_row_records_hold_the_per_slot_ratios_bit_for_bit(A):
    rng = np.random.default_rng([808, A])
    N = 512
    legal = lr.draw_legal(rng, N, A)
    mu = rp.draw_mu(rng, legal)
    fast = rp.draw_fast(rng, legal)
    out = rp.behaviour_records(fast, mu, A)
    assert np.array_equal(out[:, : 4 + 2 * A].view(np.uint32), fast[:, : 4 + 2 * A].view(np.uint32)), "the first 4 + 2A floats only travel"
    pip = fast[:, 4: 4 + A]
    checked = 0
    for a in range(A):
        rows = np.flatnonzero((legal[:, a] > 0) & (mu[:, a] > 0))
        cs, inv = _per_slot_ratios(pip[rows], mu[rows, :A], np.full(rows.size, a))
        assert np.array_equal(out[rows, 4 + 2 * A + a].view(np.uint32), cs.view(np.uint32)), f"cs, action {a}"
        assert np.array_equal(out[rows, 4 + 3 * A + a].view(np.uint32), inv.view(np.uint32)), f"inv_mu, action {a}"
        checked += rows.size
    assert checked >= N  # every row has a legal action
    # an illegal action (mu = 0) holds inf or NaN, as the on-policy record does; nothing selects it
    off = legal == 0
    assert not np.isfinite(out[:, 4 + 3 * A:][off]).any()


# ------------------------------------------------------------------------------------------------ 2. the ring
A_, S_, B_, T_ = 3, 5, 6, 4


def _stub_tree():
    handle = types.SimpleNamespace(S=S_, A=A_)
    return types.SimpleNamespace(device="cpu", max_actions=A_, handle=lambda: handle)


def _stub_plan(B=B_):
    return types.SimpleNamespace(B=B, max_items=4)


def _batch(tree, plan, tag, with_rows=True):
    """A compact bucket-ordered Episodes on CPU tensors whose every buffer is filled with `tag`."""
    import rnad_hip
    from environment.episode import Episodes

    traj = rnad_hip.Trajectory.__new__(rnad_hip.Trajectory)
    traj.T_cap, traj.B, traj.A, traj.half, traj.compact, traj.device = T_, plan.B, A_, False, True, torch.device("cpu")
    traj._indices = traj._owner = traj.c = None
    traj.observations = traj.mask_bits = traj.policy = traj.actions = traj.rewards = traj.values = None
    traj.states = torch.full((T_ + 1, plan.B), tag, dtype=torch.uint8)
    traj.acts = torch.full((plan.B,), tag, dtype=torch.int64)
    traj.final_reward = torch.full((plan.B,), float(tag))
    traj.alive = torch.full((T_ + 1,), tag, dtype=torch.int32)
    buckets = rnad_hip.Buckets(plan, "cpu")
    for t in (buckets.lane_ids, buckets.items, buckets.n_items, buckets.norm):
        t.fill_(tag)
    records = torch.full((2 * S_, 16), float(tag))
    if with_rows:
        records._policy_rows = torch.full((2 * S_, 4), float(tag))
    ep = Episodes(tree, plan.B, seed=1000 + tag, lane_offset=tag)
    ep.t_eff, ep.finished = T_ - 1, True
    ep._traj, ep.buckets, ep.lane_ids, ep.alive = traj, buckets, buckets.lane_ids, traj.alive
    ep._compact = (traj, records)
    return ep


def _tags(ring):
    return sorted(int(s.view.behaviour_rows[0, 0]) for s in ring._slots[: len(ring)])


def test_ring_evicts_the_oldest_and_reuses_its_slots():
    from environment.episode import CompactBuffer

    tree, plan = _stub_tree(), _stub_plan()
    ring = CompactBuffer(3)
    assert len(ring) == 0
    with pytest.raises(ValueError, match="empty"):
        ring.sample(B_)
    for tag in (1, 2):
        ring.append(_batch(tree, plan, tag))
    assert len(ring) == 2 and _tags(ring) == [1, 2]
    ring.append(_batch(tree, plan, 3))
    ptrs = [[t.data_ptr() for t in s.tensors()] for s in ring._slots]
    views = [s.view for s in ring._slots]
    assert len(ring._slots) == 3 and ring.slot_bytes() == sum(t.numel() * t.element_size() for t in ring._slots[0].tensors())
    for tag, want in ((4, [2, 3, 4]), (5, [3, 4, 5]), (6, [4, 5, 6]), (7, [5, 6, 7])):
        ring.append(_batch(tree, plan, tag))
        assert len(ring) == 3 and _tags(ring) == want, "the oldest batch leaves"
    assert [[t.data_ptr() for t in s.tensors()] for s in ring._slots] == ptrs, "slots are written in place after wrap-around"
    assert [s.view for s in ring._slots] == views
    # a view shows its slot as stored: every buffer of the batch, seed and lane offset, and the behaviour's rows
    slot = ring._slots[0]  # holds batch 7 (appends 1, 4, 7 landed here)
    v = slot.view
    assert v.seed == 1007 and v.lane_offset == 7 and v.t_eff == T_ - 1 and v.batch_size == B_
    assert v.buckets is slot.buckets and v.lane_ids is slot.buckets.lane_ids and v._compact[0] is slot.traj
    for t in slot.tensors():
        assert (t == 7).all()
    assert v.behaviour_rows is slot.mu and tuple(slot.mu.shape) == (2 * S_, 4)
    assert torch.equal(v.alive, slot.traj.alive) and torch.equal(v.valid_counts, slot.buckets.norm)
    ring.clear()
    assert len(ring) == 0
    ring.append(_batch(tree, plan, 9))
    assert len(ring) == 1 and _tags(ring) == [9] and [[t.data_ptr() for t in s.tensors()] for s in ring._slots] == ptrs


def test_rows_without_a_table_of_their_own_come_from_the_pi_columns():
    from environment.episode import CompactBuffer

    tree, plan = _stub_tree(), _stub_plan()
    ep = _batch(tree, plan, 2, with_rows=False)
    ep._compact[1][:, 3 * A_ + 3: 4 * A_ + 3] = torch.arange(2 * S_ * A_, dtype=torch.float32).view(2 * S_, A_)
    ring = CompactBuffer(1)
    ring.append(ep)
    mu = ring.sample(B_)[0].behaviour_rows
    assert torch.equal(mu[:, :A_], ep._compact[1][:, 3 * A_ + 3: 4 * A_ + 3]) and (mu[:, A_:] == 0).all()


def test_draws_are_distinct_and_uniform():
    from environment.episode import CompactBuffer

    tree, plan = _stub_tree(), _stub_plan()
    ring = CompactBuffer(4)
    for tag in range(4):
        ring.append(_batch(tree, plan, tag))
    views = [s.view for s in ring._slots]
    random.seed(20240)
    for k in (1, 2, 3, 4):
        for _ in range(50):
            drawn = ring.sample(B_, k)
            assert len(drawn) == k and len({id(e) for e in drawn}) == k and all(any(e is v for v in views) for e in drawn)
    with pytest.raises(ValueError, match="distinct"):
        ring.sample(B_, 5)
    with pytest.raises(ValueError, match="whole batches"):
        ring.sample(B_ - 1)
    random.seed(7)
    counts = [0, 0, 0, 0]
    for _ in range(10_000):
        counts[views.index(ring.sample(B_)[0])] += 1
    sd = (10_000 * 0.25 * 0.75) ** 0.5
    assert all(abs(c - 2_500) <= 4 * sd for c in counts), counts


def test_every_refusal_says_which():
    from environment.episode import CompactBuffer, Episodes

    tree, plan = _stub_tree(), _stub_plan()
    ring = CompactBuffer(2)
    ring.append(_batch(tree, plan, 1))
    dense = Episodes(tree, B_, seed=1)
    with pytest.raises(ValueError, match="not compact"):
        ring.append(dense)
    with pytest.raises(ValueError, match="BucketPlan differs"):
        ring.append(_batch(tree, _stub_plan(), 2))
    lazy = _batch(tree, plan, 2)
    lazy._compact = (lazy._compact[0], None)
    with pytest.raises(ValueError, match="valid in all 2S rows: no records"):
        ring.append(lazy)
    listed = _batch(tree, plan, 2)
    listed._compact[1]._partial_rows = "a row list"
    with pytest.raises(ValueError, match="valid in all 2S rows: its records were written for a row list"):
        ring.append(listed)
    owed = _batch(tree, plan, 2)
    owed._compact[1]._expand = (object(), [])
    with pytest.raises(ValueError, match="valid in all 2S rows: the copies of its distinct-observation tables"):
        ring.append(owed)
    stale = _batch(tree, plan, 2, with_rows=False)
    stale._compact[1]._expand_job, stale._compact[1]._expand_stale = (object(), []), True
    with pytest.raises(ValueError, match="valid in all 2S rows: the copies of its distinct-observation records"):
        ring.append(stale)
    assert len(ring) == 1 and _tags(ring) == [1], "a refused batch leaves the ring as it was"
    with pytest.raises(ValueError, match="max_size"):
        CompactBuffer(0)


# ------------------------------------------------------------------------------------------------ 3. the entry point
def test_entry_point_is_declared_exported_and_free_of_scratch():
    import rnad_hip

    protos = rnad_hip.header_prototypes()
    assert "rnad_bucket_behaviour_records" in protos and len(protos["rnad_bucket_behaviour_records"][1]) == 8
    assert hasattr(rnad_hip.lib(), "rnad_bucket_behaviour_records")
    table = rp.kernel_metadata(rnad_hip.SO_PATH)
    assert sorted(table) == list(range(1, 9)) and all(k["scratch"] == 0 for k in table.values()), table


def test_the_entry_point_refuses_without_a_launch():
    """n outside 1 .. 8 and null pointers are refused before anything is touched (the checks that need no device memory)."""
    import ctypes as C

    import rnad_hip

    lib = rnad_hip.lib()
    arr = (C.c_void_p * 8)()
    for n in (0, 9, -1):
        assert lib.rnad_bucket_behaviour_records(None, n, None, arr, arr, None, None, None) == 2
        assert b"outside 1 .. 8" in lib.rnad_last_error()
    assert lib.rnad_bucket_behaviour_records(None, 1, None, arr, arr, None, None, None) == 2
    assert b"null argument" in lib.rnad_last_error()
