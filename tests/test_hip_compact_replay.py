"""Compact replay on an MI355X: rnad_bucket_behaviour_records (csrc/replay.hip), the compact learner on its records -- off-policy --, the
ring and the trainer's compact_replay step.  tests/test_compact_replay.py holds the CPU half (the restatement, the ring's bookkeeping).

  a. the kernel at A = 1 .. 8 on the rows of the native trees of tests/_learnref.py: n = 1, 2, 8 behaviours over NaN-filled outputs, the
     bits of the numpy restatement (tests/_replayref.py; an element that is NaN there is NaN here), a shuffled row list that leaves the
     other rows' NaNs alone, two runs with identical bits, refusals that touch nothing, no scratch in the built library;
  b. on-policy consistency: the behaviour records built from the actor's own policy rows are the on-policy fast records bit for bit, and
     the compact learner on them gives the on-policy bits;
  c. off-policy: a compact batch played with one set of tables, learned from with another (tests/_learnref.draw_tables, H0 .. H3): the row
     tables of rnad_learn_bucketed_compact on the behaviour records within tests/_learnref's gates of the fp64 reference fed the played
     slots with the stored rows as mu, and bit-equal to rnad_learn_bucketed on the dense views with mu gathered per slot;
  d. two stored batches with different behaviours and different lengths (tree 3 is ragged): accumulate twice, finish once with the summed
     normalisers -- the fp64 reference on the union of the slots, and the bits of two dense calls and one finish;
  e. the trainer: eight compact_replay steps with a ring of three refilled every other step; a drawn batch shows its behaviour's policy;
     the flag off is the parent bit for bit; a refused condition falls back to Buffer bit for bit."""
import functools
import random

import numpy as np
import pytest
import torch

import _learnref as lr
import _replayref as rp
from test_learn_shapes import native_tree, tree_case

pytestmark = pytest.mark.gpu

I32 = torch.int32
U32 = np.uint32


def _hip():
    import rnad_hip

    return rnad_hip


@functools.lru_cache(maxsize=None)
def _tree(A):
    import _gpu as G

    return G.tree_from_arrays(native_tree(A), depth_bound=lr.TREES[A]["depth_bound"])


def _params(hp):
    return _hip().make_learn_params(**lr.hp_kwargs(hp))


def _tables_on_device(tables):
    import _gpu as G

    return [G.gpu(tables[k]).view(len(tables[k]), -1) for k in ("logit", "v", "v_target", "logit_reg", "logit_reg_")]


def _legal_tab(A):
    import _gpu as G

    return lr.legal_table(G.cpu(_tree(A).legal_tensor))


def _same_bits_or_both_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(((got.view(U32) == want.view(U32)) | (np.isnan(got) & np.isnan(want))).all())


def _nan_tables(n, shape):
    import _gpu as G

    return [torch.full(shape, float("nan"), dtype=torch.float32, device=G.DEV) for _ in range(n)]


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------ a. the kernel
@pytest.mark.parametrize("A", lr.A_RANGE)
def test_kernel_writes_the_restatement_bits(A):
    import _gpu as G

    hip = _hip()
    h = _tree(A).handle()
    N = 2 * h.S
    assert N > 64 and N % 64 != 0, "more than one workgroup of 64 rows, and a partial last tile"
    legal = _legal_tab(A)
    rng = np.random.default_rng([909, A])
    fast = rp.draw_fast(rng, legal)
    mus = [rp.draw_mu(rng, legal) for _ in range(8)]
    want = [rp.behaviour_records(fast, mu, A) for mu in mus]
    d_fast, d_mus = G.gpu(fast), [G.gpu(mu) for mu in mus]
    for n in (1, 2, 8):
        outs = _nan_tables(n, d_fast.shape)
        got = hip.behaviour_records(h, d_fast, d_mus[:n], out=outs)
        again = hip.behaviour_records(h, d_fast, d_mus[:n])
        torch.cuda.synchronize()
        assert all(g is o for g, o in zip(got, outs))
        for k in range(n):
            assert _same_bits_or_both_nan(G.cpu(got[k]), want[k]), f"A={A} n={n}: behaviour {k}"
            assert torch.equal(got[k].view(I32), again[k].view(I32)), f"A={A} n={n}: two runs differ"
    # a shuffled row list: the listed rows hold the restatement, the others keep their NaNs
    listed = rng.permutation(N)[: max(1, (2 * N) // 3)]
    rows = hip.RowList(torch.as_tensor(listed.astype(np.int32)), N, G.DEV)
    outs = hip.behaviour_records(h, d_fast, d_mus[:2], out=_nan_tables(2, d_fast.shape), rows=rows)
    torch.cuda.synchronize()
    rest = np.setdiff1d(np.arange(N), listed)
    for k in range(2):
        o = G.cpu(outs[k])
        assert _same_bits_or_both_nan(o[listed], want[k][listed]) and np.isnan(o[rest]).all(), f"A={A}: row list, behaviour {k}"


def test_refusals_touch_nothing():
    import ctypes as C

    import _gpu as G

    hip = _hip()
    A = 3
    h = _tree(A).handle()
    N, F, P = 2 * h.S, rp.fast_stride(A), rp.policy_stride(A)
    legal = _legal_tab(A)
    rng = np.random.default_rng(5)
    fast, mu = G.gpu(rp.draw_fast(rng, legal)), G.gpu(rp.draw_mu(rng, legal))
    outs = _nan_tables(9, fast.shape)
    with pytest.raises(hip.RnadHipError, match="outside 1 .. 8"):
        hip.behaviour_records(h, fast, [], out=[])
    with pytest.raises(hip.RnadHipError, match="outside 1 .. 8"):
        hip.behaviour_records(h, fast, [mu] * 9, out=outs)
    with pytest.raises(hip.RnadHipError, match="must be"):
        hip.behaviour_records(h, fast[:, :-4].contiguous(), [mu], out=outs[:1])
    with pytest.raises(hip.RnadHipError, match="must be"):
        hip.behaviour_records(h, fast, [mu[:-1]], out=outs[:1])
    with pytest.raises(hip.RnadHipError, match="output tables"):
        hip.behaviour_records(h, fast, [mu, mu], out=outs[:1])
    with pytest.raises(hip.RnadHipError, match="dtype"):
        hip.behaviour_records(h, fast, [mu.double()], out=outs[:1])
    with pytest.raises(hip.RnadHipError, match="GPU tensor"):
        hip.behaviour_records(h, fast, [mu.cpu()], out=outs[:1])
    with pytest.raises(hip.RnadHipError, match=r"out\[0\] overlaps out\[1\]"):
        hip.behaviour_records(h, fast, [mu, mu], out=[outs[0], outs[0]])
    with pytest.raises(hip.RnadHipError, match="overlaps fast_records"):
        hip.behaviour_records(h, fast, [mu], out=[fast])
    # the C entry point itself: a table that is not 16-byte aligned, an output inside a behaviour's rows, rows without n_rows
    lib = hip.lib()
    big = torch.full((N * F + 4,), float("nan"), dtype=torch.float32, device=G.DEV)
    one = lambda p: (C.c_void_p * 1)(p)  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda f, m, o, r=None, nr=None: lib.rnad_bucket_behaviour_records(h.ptr, 1, f, one(m), one(o), r, nr, stream)  # noqa: E731
    assert call(fast.data_ptr(), mu.data_ptr(), big.data_ptr() + 4) == 2 and b"16-byte aligned" in lib.rnad_last_error()
    assert call(fast.data_ptr() + 4, mu.data_ptr(), big.data_ptr()) == 2 and b"16-byte aligned" in lib.rnad_last_error()
    assert call(fast.data_ptr(), mu.data_ptr() + 4, big.data_ptr()) == 2 and b"16-byte aligned" in lib.rnad_last_error()
    assert call(fast.data_ptr(), big.data_ptr() + 16, big.data_ptr()) == 2 and b"overlaps mu_rows" in lib.rnad_last_error()
    assert call(fast.data_ptr(), mu.data_ptr(), None) == 2 and b"null" in lib.rnad_last_error()
    assert call(fast.data_ptr(), mu.data_ptr(), big.data_ptr(), mu.data_ptr(), None) == 2 and b"go together" in lib.rnad_last_error()
    torch.cuda.synchronize()
    assert all(_all_nan(o) for o in outs) and _all_nan(big), "a refused call writes nothing"
    assert P == mu.shape[1]


def test_no_instantiation_uses_scratch():
    hip = _hip()
    table = rp.kernel_metadata(hip.SO_PATH)
    assert sorted(table) == list(range(1, 9)) and all(k["scratch"] == 0 for k in table.values()), table


# ------------------------------------------------------------------------------------------------ b. on-policy consistency
def _play(h, rec, B, seed, lane0=0):
    import _gpu as G

    hip = _hip()
    T = 2 * h.max_depth
    traj = hip.Trajectory(h, B, T, G.DEV, with_observations=False, with_values=False, compact=True)
    return traj, hip.rollout_bucketed_compact(h, traj, rec, seed=seed, lane0=lane0), T


@pytest.mark.parametrize("A", lr.A_RANGE)
def test_the_actors_own_rows_give_the_on_policy_records_and_update(A):
    hip = _hip()
    hp = lr.HP["H1"]
    h = _tree(A).handle()
    params = _params(hp)
    rec, fast = hip.bucket_records(h, *_tables_on_device(tree_case((A, "H1"))[1]), params, fast=True)
    (own,) = hip.behaviour_records(h, fast, [rec._policy_rows])
    assert torch.equal(own.view(I32), fast.view(I32)), "mu = the actor's own pi: the on-policy table, bit for bit"
    traj, bk, T = _play(h, rec, lr.TREE_B[A], seed=31)
    want = hip.learn_bucketed_compact(h, bk, traj, T, rec, fast, bk.norm, params)
    got = hip.learn_bucketed_compact(h, bk, traj, T, rec, own, bk.norm, params)
    assert torch.equal(got[0].view(I32), want[0].view(I32)) and torch.equal(got[1].view(I32), want[1].view(I32))


# ------------------------------------------------------------------------------------------------ c. off-policy
def _case_id(key):
    return f"tree_A{key[0]}_{key[1]}"


def _learner_tables(A, s, legal_tab):
    """The learner's five row tables: a second, independent draw (the behaviour's are tree_case's)."""
    return lr.draw_tables(np.random.default_rng([4242, A, lr.SETS.index(s)]), legal_tab, lr.HP[s])


def _dense_views(h, traj, T, rec_b):
    """The played batch as dense tensors: indices [T, B] and, by rnad_bucket_expand on the BEHAVIOUR's records, mask bits, the policy the
    slots were played with (the stored rows gathered per slot), actions and rewards."""
    hip = _hip()
    idx = traj.indices[:T].contiguous()
    hip.bucket_expand(h, traj, rec_b)
    return idx, traj.actions[:T].contiguous(), traj.rewards[:T].contiguous(), traj.policy[:T].contiguous()


def _compare_tables(case, ref, dl_tab, dv_tab, hp, S, A, tag):
    """tests/test_hip_learn_shapes.py's gate of a bucketed row table: K 2^-24 mag plus slots * half a fixed-point unit, scaled by w / N_P."""
    import _gpu as G

    unit_l, unit_v = lr.bucketed_units(hp)
    n_row = np.repeat(ref.norm, S)
    slots = ref.row_slots.astype(np.float64)
    fixed_l = (slots * 0.5 * unit_l * hp.w_n / n_row)[:, None] * np.ones(A)
    fixed_v = slots * 0.5 * unit_v * hp.w_v / n_row
    sl = lr.table_share(G.cpu(dl_tab), ref.dlogit_tab, fixed_l) / lr.K["tables"]
    sv = lr.table_share(G.cpu(dv_tab), ref.dv_tab, fixed_v) / lr.K["tables"]
    lr.log_share(case, tag + "dlogit_tab", sl)
    lr.log_share(case, tag + "dv_tab", sv)
    print(f"{case} {tag}: shares of the gate: dlogit_tab {sl:.3f}, dv_tab {sv:.3f}")
    assert sl <= 1 and sv <= 1, f"{case} {tag}: row tables outside the gate: dlogit_tab {sl:.3f}, dv_tab {sv:.3f} of it"


@pytest.mark.parametrize("key", lr.tree_cases(), ids=_case_id)
def test_off_policy_learner_on_behaviour_records(key):
    import _gpu as G

    hip = _hip()
    A, s = key
    hp = lr.HP[s]
    case = _case_id(key)
    h = _tree(A).handle()
    B, S = lr.TREE_B[A], h.S
    params = _params(hp)
    legal_tab = _legal_tab(A)
    # the behaviour: records of one set of tables; the batch is played with its policy rows
    rec_b, _ = hip.bucket_records(h, *_tables_on_device(tree_case(key)[1]), params, fast=True)
    mu_rows = rec_b._policy_rows
    traj, bk, T = _play(h, rec_b, B, seed=41, lane0=5)
    # the learner: a second set
    tables = _learner_tables(A, s, legal_tab)
    rec, fast = hip.bucket_records(h, *_tables_on_device(tables), params, fast=True)
    (beh,) = hip.behaviour_records(h, fast, [mu_rows])
    first = hip.learn_bucketed_compact(h, bk, traj, T, rec, beh, bk.norm, params, want_losses=True)
    again = hip.learn_bucketed_compact(h, bk, traj, T, rec, beh, bk.norm, params, want_losses=True)
    assert torch.equal(first[0].view(I32), again[0].view(I32)) and torch.equal(first[1].view(I32), again[1].view(I32)), f"{case}: two runs differ"
    dl_tab, dv_tab, losses = first
    # the inputs are off-policy: importance ratios away from 1
    idx_d, act_d, rew_d, mu_d = _dense_views(h, traj, T, rec_b)
    idx, act, mu = G.cpu(idx_d).astype(np.int32), G.cpu(act_d), G.cpu(mu_d)
    rows = (np.arange(T) & 1)[:, None] * S + idx
    valid = idx != 0
    assert np.array_equal(mu[valid], G.cpu(mu_rows)[rows][valid][:, :A]), "the policy view is the stored rows, gathered per slot"
    pip = G.cpu(fast)[:, 4: 4 + A]
    take = lambda x: np.take_along_axis(x, act.astype(np.int64)[..., None], -1)[..., 0]  # noqa: E731
    ratio = take(pip[rows].astype(np.float64))[valid] / take(mu.astype(np.float64))[valid]
    if A > 1:  # (at A = 1 pi = mu = 1 in every row)
        assert np.abs(ratio - 1).max() > 0.05, f"{case}: the batch is not off-policy"
    assert (take(mu)[valid] > 0).all(), "a taken action has mu > 0"
    # fp64 reference: the played slots with the stored rows as mu
    batch = dict(indices=idx, legal=legal_tab[rows], actions=act, rewards=G.cpu(rew_d), mu=mu, S=S)
    ref = lr.learner(np.float64, batch, tables, hp)
    assert (ref.margin >= lr.MARGIN).all()
    assert np.array_equal(G.cpu(bk.norm), [valid[0::2].sum(), valid[1::2].sum()])
    _compare_tables(case, ref, dl_tab, dv_tab, hp, S, A, "replay_")
    sl = lr.share(G.cpu(losses), ref.losses) / lr.K["losses"]
    lr.log_share(case, "replay_losses", sl)
    assert sl <= 1, f"{case}: losses at {sl:.3f} of the gate"
    # the dense bucketed learner on the same slots, mu per slot: the same operations on the same floats, integer sums
    dense = hip.learn_bucketed(h, bk, idx_d, act_d, rew_d, mu_d, rec, bk.norm, params)
    same_l, same_v = torch.equal(dense[0].view(I32), dl_tab.view(I32)), torch.equal(dense[1].view(I32), dv_tab.view(I32))
    print(f"{case}: bit-equal to the dense bucketed learner: dlogit_tab {same_l}, dv_tab {same_v}")
    assert same_l and same_v, f"{case}: compact-on-behaviour-records and dense learner differ in bits"


# ------------------------------------------------------------------------------------------------ d. two drawn batches, one finish
def _shortest_rows(A):
    """Deterministic policy rows [2S, policy_stride(A)] under which every episode of the tree ends as early as the two players can make it
    (both pick the joint action with the smallest worst-case remaining depth): a behaviour whose batch is shorter than a random one's."""
    t = native_tree(A)
    index, chance, legal = (np.asarray(t[k]) for k in ("index", "chance", "legal"))
    S, C = index.shape[:2]
    legal = legal.reshape(S, A, A)

    @functools.lru_cache(maxsize=None)
    def best(s):
        if s == 0:
            return 0, (0, 0)
        out = (1 << 30, (0, 0))
        for a in range(A):
            for b in range(A):
                if legal[s, a, b] > 0:
                    d = 1 + max([best(int(index[s, c, a, b]))[0] for c in range(C) if chance[s, c, a, b] > 0] or [0])
                    if d < out[0]:
                        out = (d, (a, b))
        return out

    mu = np.zeros((2 * S, rp.policy_stride(A)), np.float32)
    for s in range(1, S):
        if legal[s].any():
            a, b = best(s)[1]
            mu[s, a] = 1.0
            mu[S + s, b] = 1.0
    return mu, 2 * best(1)[0]


def test_two_drawn_batches_accumulate_and_finish_once():
    import _gpu as G

    hip = _hip()
    A, s = 3, "H1"
    hp = lr.HP[s]
    h = _tree(A).handle()
    B, S = lr.TREE_B[A], h.S
    params = _params(hp)
    legal_tab = _legal_tab(A)
    tables = _learner_tables(A, s, legal_tab)
    rec, fast = hip.bucket_records(h, *_tables_on_device(tables), params, fast=True)
    # behaviour 1: a random net's rows; behaviour 2: the shortest deterministic play (a records table that holds its rows as pi)
    rec_1, _ = hip.bucket_records(h, *_tables_on_device(tree_case((A, "H0"))[1]), params, fast=True)
    mu_1 = rec_1._policy_rows
    short, longest = _shortest_rows(A)
    mu_2 = G.gpu(short)
    rec_2 = torch.zeros_like(rec_1)
    rec_2[:, hip.policy_column(A): hip.policy_column(A) + A] = mu_2[:, :A]
    traj_1, bk_1, T_cap = _play(h, rec_1, B, seed=51)
    traj_2, bk_2, _ = _play(h, rec_2, B, seed=52, lane0=B)
    T_1 = int((G.cpu(traj_1.alive)[:T_cap] > 0).sum())
    T_2 = int((G.cpu(traj_2.alive)[:T_cap] > 0).sum())
    assert T_2 <= longest < T_1 == T_cap, f"the two batches have different lengths by construction ({T_1}, {T_2})"
    batches = ((traj_1, bk_1, T_1, rec_1), (traj_2, bk_2, T_2, rec_2))
    beh = hip.behaviour_records(h, fast, [mu_1, mu_2])
    for (traj, bk, T, _), table in zip(batches, beh):
        dl_tab, dv_tab, _ = hip.learn_bucketed_compact(h, bk, traj, T, rec, table, None, params)
    # (bk.norm counts the T_cap steps of the window; the slots at and after a batch's own T are all absorbed)
    norm = bk_1.norm + bk_2.norm
    hip.bucket_finish(h, bk_1, norm, params, dl_tab, dv_tab)
    # the union of the slots for the reference: the shorter batch padded with invalid steps, side by side
    views = [_dense_views(h, traj, T, rec_b) for traj, _, T, rec_b in batches]
    pad = lambda x, T: np.concatenate([x, np.zeros((T_1 - T,) + x.shape[1:], x.dtype)], 0)  # noqa: E731
    idx, act, rew, mu = (np.concatenate([pad(G.cpu(v[k]), b[2]) for v, b in zip(views, batches)], 1) for k in range(4))
    idx = idx.astype(np.int32)
    rows = (np.arange(T_1) & 1)[:, None] * S + idx
    valid = idx != 0
    assert np.array_equal(G.cpu(norm), [valid[0::2].sum(), valid[1::2].sum()]), "the summed normalisers are the union's"
    ref = lr.learner(np.float64, dict(indices=idx, legal=legal_tab[rows], actions=act, rewards=rew, mu=mu, S=S), tables, hp)
    assert (ref.margin >= lr.MARGIN).all()
    _compare_tables("two_batches", ref, dl_tab, dv_tab, hp, S, A, "replay2_")
    # two dense calls with norm = None and one finish: the same bits
    for (traj, bk, T, _), v in zip(batches, views):
        dl_d, dv_d, _ = hip.learn_bucketed(h, bk, v[0], v[1], v[2], v[3], rec, None, params)
    hip.bucket_finish(h, bk_1, norm, params, dl_d, dv_d)
    assert torch.equal(dl_d.view(I32), dl_tab.view(I32)) and torch.equal(dv_d.view(I32), dv_tab.view(I32))
    A1 = A + 1
    assert (bk_1.plan.accumulators[: (2 * S + 128 * max(bk_1.plan.n_upper, 1)) * A1] == 0).all(), "the accumulators are zero again"


# ------------------------------------------------------------------------------------------------ e. the trainer
def _trainer(tree, tmp_path, tag, **attrs):
    import os

    import _gpu as G
    from learn.rnad import RNaD

    os.environ["RNAD_SAVE_DIR"] = str(tmp_path)
    torch.manual_seed(11)
    np.random.seed(11)
    random.seed(11)
    rn = RNaD(tree=tree, device=G.DEV, directory_name=tag, batch_size=1 << 14, eta=0.2, b1_adam=0.0, lr=1e-3, n_batches_per_buffer=3, buffer_mod=2,
              net_params={"type": "MLP", "max_actions": tree.max_actions, "width": 64})
    for name, value in attrs.items():
        if value is _ABSENT:
            del rn.__dict__[name]
        else:
            setattr(rn, name, value)
    rn.initialize()
    with torch.no_grad():
        for p in rn.net_reg_.parameters():
            p.mul_(1.01)
    return rn


_ABSENT = object()


def _steps(rn, buf, n, after=None):
    for i in range(n):
        rn.train_step(buf, alpha=min(1.0, 0.15 * i))
        rn.total_steps += 1
        if after is not None:
            after(i)
    torch.cuda.synchronize()
    return [p.detach().clone() for net in (rn.net, rn.net_target) for p in net.parameters()]


def _ternary4():
    from test_hip_bucket import TREES, _native_tree

    return _native_tree(**TREES["ternary4"])


def test_trainer_steps_on_the_ring(tmp_path):
    from environment.episode import CompactBuffer

    hip = _hip()
    tree = _ternary4()
    rn = _trainer(tree, tmp_path, "ring", compact_replay=True, replay_batches=2)
    before = [p.detach().clone() for p in rn.net.parameters()]
    ring = rn.make_buffer()
    assert isinstance(ring, CompactBuffer) and ring.max_size == 3
    seen = {}

    def after(i):
        if i == 0:
            seen["mu0"] = ring._slots[0].mu.clone()
        if i == 4:  # appends at steps 0, 2, 4: the ring is full
            seen["ptrs"] = [[t.data_ptr() for t in s.tensors()] for s in ring._slots]
            seen["views"] = [s.view for s in ring._slots]
        if i == 3:
            # slot 0 still holds the batch of step 0: its dense policy is THAT step's rows gathered per slot, not a later net's
            view = ring._slots[0].view
            S, T, A = tree.handle().S, view.t_eff + 1, tree.max_actions
            idx = view.indices.long()
            rows = idx + (torch.arange(T, device=idx.device) & 1).view(T, 1) * S
            assert torch.equal(view.behaviour_rows, seen["mu0"])
            assert torch.equal(view.policy, seen["mu0"][rows][..., :A])
            assert not torch.equal(seen["mu0"], ring._slots[1].mu), "the net has moved since"
            assert view.rewards.shape == idx.shape and view.actions.shape == idx.shape + (A,) and view.masks.shape == idx.shape + (A,)

    nets = _steps(rn, ring, 8, after)
    assert len(ring) == 3
    assert [[t.data_ptr() for t in s.tensors()] for s in ring._slots] == seen["ptrs"] and [s.view for s in ring._slots] == seen["views"], \
        "no ring allocation after the first three appends"
    assert all(torch.isfinite(p).all() for p in nets)
    assert any(not torch.equal(a, b) for a, b in zip(before, rn.net.parameters())), "the update moved the net"
    assert getattr(rn, "_graph", None) is None, "the replay step is eager"
    # a logging step goes through the dense route on a drawn batch's views; on an odd step nothing is played, so whichever batch is
    # drawn was played by an older net: the actor-learner divergence is that of an off-policy batch
    rn.total_steps = 9
    log = {}
    rn.train_step(ring, alpha=1.0, log=log)
    assert np.isfinite(log["loss_v"]) and np.isfinite(log["actor_learner_kld"]) and log["actor_learner_kld"] > 0
    # the fixed-point headroom
    rn.replay_batches = hip.BUCKET_MAX_LANES // rn.batch_size + 1
    with pytest.raises(ValueError, match="headroom"):
        rn.train_step(ring, alpha=1.0)


def test_flag_off_is_the_parent_and_a_refusal_falls_back_bit_for_bit(tmp_path, caplog):
    from environment.episode import Buffer, CompactBuffer

    tree = _ternary4()
    absent = _trainer(tree, tmp_path, "absent", compact_replay=_ABSENT, replay_batches=_ABSENT)
    buf = absent.make_buffer()
    assert type(buf) is Buffer
    want = _steps(absent, buf, 8)
    off = _trainer(tree, tmp_path, "off")
    assert off.compact_replay is False and off.replay_batches == 1
    buf = off.make_buffer()
    assert type(buf) is Buffer
    for a, b in zip(want, _steps(off, buf, 8)):
        assert torch.equal(a, b), "compact_replay off: the parent's parameters"
    # a refused condition: lazy rows asked for
    plain = _trainer(tree, tmp_path, "lazy_buffer", lazy_rows=True)
    want = _steps(plain, Buffer(3), 8)
    refused = _trainer(tree, tmp_path, "lazy_ring", lazy_rows=True, compact_replay=True)
    with caplog.at_level("WARNING"):
        assert type(refused.make_buffer()) is Buffer
        got = _steps(refused, CompactBuffer(3), 8)
    assert sum("compact_replay not used" in r.getMessage() for r in caplog.records) == 1, "said once"
    for a, b in zip(want, got):
        assert torch.equal(a, b), "the fallback is the Buffer run"
