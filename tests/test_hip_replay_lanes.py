"""The lane draw of the compact replay on an MI355X: rnad_bucket_draw_lanes (csrc/replay.hip), the compact learner on a draw, the
ring's sample_lanes and the trainer's replay_lanes step.  tests/test_replay_lanes.py holds the CPU half (the draw contract against its
numpy restatement, uniformity, the item rebuild by hand).

  a. gather exactness on the learner sweep's native trees (tests/_learnref.py) at their TREE_B: for 1, 2, 3, 8 and 9 sources played by
     different behaviours, the drawn columns of every source -- rnad_draw_columns on the host -- arrive in order: the rebuilt indices,
     acts, final_reward, lane_ids; the work lists are the numpy rebuild of tests/_drawref.py; norm is the count taken from the indices.
     With two-byte states, the ragged tree, terminal buckets, b_k = 0 beside b_k = B, buckets that receive no lane, a bucket that is a
     single item in two sources at once, source items repacked at 64 lanes per item;
  b. learner bits at A = 1 .. 8 under H0 .. H3: one rnad_learn_bucketed_compact per source on the draw and one finish, bit-equal to
     rnad_learn_bucketed on dense views of the same selected lanes (gathered on the host side of the test from the SOURCES, with work
     lists from the numpy rebuild), both within tests/_learnref's gates of the fp64 learner, accumulators zero again;
  c. the trainer with replay_lanes on a ring of 3: a step's row tables are those of a hand-made sequence of the same calls; with
     replay_lanes off (or absent) the compact_replay step is unchanged bit for bit;
  d. the refusals, which launch nothing."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _drawref as dr
import _learnref as lr
import test_hip_compact_replay as cr
from test_learn_shapes import tree_case

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _hip():
    import rnad_hip

    return rnad_hip


def _behaviour(h, A, k, params, hp_name="H0"):
    """Row records of behaviour k on tree A: an independent draw of the five tables."""
    tables = lr.draw_tables(np.random.default_rng([606, A, k]), cr._legal_tab(A), lr.HP[hp_name])
    rec, _ = _hip().bucket_records(h, *cr._tables_on_device(tables), params, fast=True)
    return rec


def _sources(h, A, n, params, B):
    """n stored batches of tree A, each played by its own behaviour with its own seed and lanes."""
    out = []
    for k in range(n):
        rec = _behaviour(h, A, k, params)
        traj, bk, T_cap = cr._play(h, rec, B, seed=700 + k, lane0=k * B)
        out.append((traj, bk, rec))
    return out, T_cap


def _check_draw(h, sources, sizes, seed, draw, T_cap):
    """Everything (a) says of one draw; returns (per-source selected columns, per-source expected work lists)."""
    import _gpu as G

    hip = _hip()
    plan = sources[0][1].plan
    B = plan.B
    sole = any(b == B for b in sizes)
    norm = np.zeros(2, np.int64)
    sels, lists = [], []
    off = 0
    assert draw.sizes == list(sizes) and draw.offsets == [sum(sizes[:k]) for k in range(len(sizes))] and len(draw.buckets) == len(sizes)
    for k, ((traj, bk, _), b) in enumerate(zip(sources, sizes)):
        sel = hip.draw_columns(seed, k, B, b)
        sels.append(sel)
        sel_d = torch.as_tensor(sel.astype(np.int64), device=G.DEV)
        n_src = int(bk.n_items.item())
        src_items = G.cpu(bk.items[:n_src])
        drawn = np.zeros(B, bool)
        drawn[sel] = True
        want_items = dr.rebuild_items(src_items, drawn, plan.chunk, off, sole)
        lists.append(want_items)
        got_n = int(draw.buckets[k].n_items.item())
        got_items = G.cpu(draw.buckets[k].items[:got_n])
        assert got_n == len(want_items) and np.array_equal(got_items, want_items), f"source {k}: work list\n{got_items}\n{want_items}"
        assert (got_items[:, 1] <= plan.chunk).all()
        if b:
            want_idx = traj.indices[:, sel_d]
            got_idx = hip.bucket_indices(h, draw.buckets[k], draw.traj)[:, off: off + b]
            assert torch.equal(got_idx, want_idx), f"source {k}: the rebuilt indices of the drawn columns"
            assert torch.equal(draw.traj.acts[off: off + b], traj.acts[sel_d]), f"source {k}: acts"
            assert torch.equal(draw.traj.final_reward[off: off + b].view(I32), traj.final_reward[sel_d].view(I32)), f"source {k}: final_reward"
            assert torch.equal(draw.lane_ids[off: off + b], bk.lane_ids[sel_d]), f"source {k}: lane_ids"
            live = G.cpu(want_idx[:T_cap]) != 0
            norm += [live[0::2].sum(), live[1::2].sum()]
        off += b
    assert np.array_equal(G.cpu(draw.norm), norm.astype(np.float64)), f"norm {G.cpu(draw.norm)} against the count {norm}"
    return sels, lists


def _multinomial(rng, B, n):
    return [int(x) for x in rng.multinomial(B, [1 / n] * n)]


# (id, A, sources, sizes(B, rng) or None = multinomial, environment)
GATHER = [
    ("one_source", 2, 1, None, {}),
    ("two_sources", 4, 2, None, {}),
    ("three_sources_ragged", 3, 3, None, {}),
    ("eight_sources", 2, 8, None, {}),
    ("nine_sources_two_calls", 2, 9, None, {}),
    ("two_byte_states", 5, 3, None, {"RNAD_BUCKET_ROWS": "300"}),
    ("zero_beside_all", 3, 3, lambda B, rng: [0, B, 0], {}),
    ("first_call_empty", 2, 9, lambda B, rng: [0] * 8 + [B], {}),
    ("small_draws", 3, 3, lambda B, rng: [7, 9, B - 16], {}),
    ("small_draws_upper_cut", 5, 3, lambda B, rng: [40, 40, B - 80], {"RNAD_BUCKET_ROWS": "8"}),
    ("repacked_at_64", 4, 2, None, {"RNAD_BUCKET_CHUNK": "64"}),
    ("repacked_at_64_ragged", 3, 3, None, {"RNAD_BUCKET_CHUNK": "64", "RNAD_BUCKET_ROWS": "8"}),
]
_seen = {}


@pytest.mark.parametrize("case", GATHER, ids=[c[0] for c in GATHER])
def test_gather_exactness(case, monkeypatch):
    import _gpu as G

    hip = _hip()
    name, A, n, sizes_of, env = case
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    h = cr._tree(A).handle()
    B = lr.TREE_B[A]
    params = cr._params(lr.HP["H0"])
    sources, T_cap = _sources(h, A, n, params, B)
    plan = sources[0][1].plan
    rng = np.random.default_rng([11, len(name), A, n])
    sizes = sizes_of(B, rng) if sizes_of else _multinomial(rng, B, n)
    seed = int(rng.integers(0, 2**63))
    draw = hip.draw_lanes(h, [(t, b) for t, b, _ in sources], sizes, seed)
    # a second draw into the same holder with another seed, then the first again: the holder is rewritten, the result is a function of the inputs
    first = [draw.traj.states.clone(), draw.traj.acts.clone(), draw.lane_ids.clone(), draw.norm.clone()]
    hip.draw_lanes(h, [(t, b) for t, b, _ in sources], sizes, seed + 1, out=draw)
    again = hip.draw_lanes(h, [(t, b) for t, b, _ in sources], sizes, seed, out=draw)
    assert again is draw
    sels, lists = _check_draw(h, sources, sizes, seed, draw, T_cap)
    assert torch.equal(draw.traj.acts, first[1]) and torch.equal(draw.lane_ids, first[2]) and torch.equal(draw.norm, first[3])
    # what the case is there for
    n_buckets, n_groups = plan.n_buckets, plan.n_groups
    per_source = [np.bincount(items[:, 2], weights=items[:, 1], minlength=n_buckets) for items in lists]
    src_buckets = [set(G.cpu(bk.items[: int(bk.n_items.item())])[:, 2].tolist()) for _, bk, _ in sources]
    facts = dict(
        rel_bytes=plan.rel_bytes,
        terminal=any((items[:, 2] >= n_groups).any() for items in lists),
        empty_bucket=any(len(set(items[:, 2].tolist())) < len(sb) for items, sb, b in zip(lists, src_buckets, sizes) if b),
        shared_single=bool(((np.stack([np.bincount(items[:, 2], minlength=n_buckets) for items in lists]) == 1).sum(0) >= 2).any()),
        repacked=any(len(items) < int(bk.n_items.item()) and (np.bincount(items[:, 2], minlength=n_buckets) > 1).any()
                     for items, (_, bk, _) in zip(lists, sources)),
        ragged=bool((G.cpu(sources[0][0].alive)[:T_cap] < B).any()),
    )
    _seen[name] = facts
    print(name, facts, "lanes per source", [int(p.sum()) for p in per_source])
    if name == "two_byte_states":
        assert facts["rel_bytes"] == 2 and draw.traj.states.dtype == torch.int16
    if name == "three_sources_ragged":
        assert facts["ragged"], "tree 3 has ragged episode lengths"
    if name in ("small_draws", "small_draws_upper_cut"):
        assert facts["empty_bucket"], "some bucket of a source receives no lane"
    if name == "small_draws_upper_cut":
        assert facts["shared_single"], "some bucket is a single item in two sources at once"
        assert facts["terminal"], "lanes that leave the tree above the cut: terminal buckets"
    if name.startswith("repacked"):
        assert facts["repacked"], "a bucket's drawn lanes fill fewer items than its source items"


# ------------------------------------------------------------------------------------------------ b. learner bits
@pytest.mark.parametrize("key", lr.tree_cases(), ids=cr._case_id)
def test_learner_bits_on_a_draw(key):
    import _gpu as G

    hip = _hip()
    A, s = key
    hp = lr.HP[s]
    case = "lanes_" + cr._case_id(key)
    h = cr._tree(A).handle()
    B, S = lr.TREE_B[A], h.S
    params = cr._params(hp)
    legal_tab = cr._legal_tab(A)
    n = 3
    sources = []
    for k in range(n):  # the behaviours: tree_case's tables, and two more draws
        tabs = tree_case(key)[1] if k == 0 else lr.draw_tables(np.random.default_rng([808, A, k]), legal_tab, hp)
        rec_b, _ = hip.bucket_records(h, *cr._tables_on_device(tabs), params, fast=True)
        traj, bk, T_cap = cr._play(h, rec_b, B, seed=900 + k, lane0=k * B)
        sources.append((traj, bk, rec_b))
    plan = sources[0][1].plan
    tables = cr._learner_tables(A, s, legal_tab)
    rec, fast = hip.bucket_records(h, *cr._tables_on_device(tables), params, fast=True)
    rng = np.random.default_rng([12, A, lr.SETS.index(s)])
    sizes = _multinomial(rng, B, n)
    seed = int(rng.integers(0, 2**63))
    draw = hip.draw_lanes(h, [(t, b) for t, b, _ in sources], sizes, seed)
    beh = hip.behaviour_records(h, fast, [rec_b._policy_rows for _, _, rec_b in sources])
    for k in draw.contributing():
        dl_tab, dv_tab, _ = hip.learn_bucketed_compact(h, draw.buckets[k], draw.traj, T_cap, rec, beh[k], None, params)
    hip.bucket_finish(h, draw.buckets[0], draw.norm, params, dl_tab, dv_tab)
    # the same selected lanes as dense tensors, gathered from the SOURCES' dense views; work lists from the numpy rebuild
    cols = {name: [] for name in ("idx", "act", "rew", "mu")}
    lists = []
    off = 0
    for k, ((traj, bk, rec_b), b) in enumerate(zip(sources, sizes)):
        sel = hip.draw_columns(seed, k, B, b)
        sel_d = torch.as_tensor(sel.astype(np.int64), device=G.DEV)
        views = cr._dense_views(h, traj, T_cap, rec_b)
        for name, v in zip(cols, views):
            cols[name].append(v[:, sel_d])
        drawn = np.zeros(B, bool)
        drawn[sel] = True
        lists.append(dr.rebuild_items(G.cpu(bk.items[: int(bk.n_items.item())]), drawn, plan.chunk, off, False))
        off += b
    idx_d, act_d, rew_d, mu_d = (torch.cat(cols[name], 1).contiguous() for name in cols)
    assert idx_d.shape == (T_cap, B)
    for k, items in enumerate(lists):
        if len(items):
            dense_bk = G.buckets_of(cr._tree(A), B, np.arange(B), [tuple(int(x) for x in it) for it in items])
            dl_d, dv_d, _ = hip.learn_bucketed(h, dense_bk, idx_d, act_d, rew_d, mu_d, rec, None, params)
    hip.bucket_finish(h, draw.buckets[0], draw.norm, params, dl_d, dv_d)
    same_l, same_v = torch.equal(dl_d.view(I32), dl_tab.view(I32)), torch.equal(dv_d.view(I32), dv_tab.view(I32))
    print(f"{case}: sizes {sizes}; bit-equal to the dense bucketed learner: dlogit_tab {same_l}, dv_tab {same_v}")
    assert same_l and same_v, f"{case}: the learner on the draw and the dense learner on the same lanes differ in bits"
    A1 = A + 1
    assert (plan.accumulators[: (2 * S + 128 * max(plan.n_upper, 1)) * A1] == 0).all(), "the accumulators are zero again"
    # the fp64 learner on those slots
    idx, act, mu = G.cpu(idx_d).astype(np.int32), G.cpu(act_d), G.cpu(mu_d)
    rows = (np.arange(T_cap) & 1)[:, None] * S + idx
    valid = idx != 0
    assert np.array_equal(G.cpu(draw.norm), [valid[0::2].sum(), valid[1::2].sum()])
    ref = lr.learner(np.float64, dict(indices=idx, legal=legal_tab[rows], actions=act, rewards=G.cpu(rew_d), mu=mu, S=S), tables, hp)
    assert (ref.margin >= lr.MARGIN).all()
    cr._compare_tables(case, ref, dl_tab, dv_tab, hp, S, A, "lanes_")
    cr._compare_tables(case, ref, dl_d, dv_d, hp, S, A, "lanes_dense_")


# ------------------------------------------------------------------------------------------------ c. the trainer
def _hand_made_step(rn, ring, alpha):
    """The replay_lanes step's row tables by hand: this step's tables, sample_lanes' two draws, one draw_lanes, behaviour_records, one
    learner call per contributing source, one finish."""
    hip = _hip()
    handle = rn.tree.handle()
    B = rn.batch_size
    with hip.workspace_owner(rn._workspace_token()):
        hp = rn._learn_params(alpha)
        tables = rn._table_outputs(alpha, False, want_target_logits=False, fold=rn._fold(), records_hp=hp)
        slots = ring._slots[: len(ring)]
        sizes = [int(b) for b in np.random.multinomial(B, [1 / len(slots)] * len(slots))]
        seed = random.getrandbits(63)
        draw = hip.draw_lanes(handle, [(s.traj, s.buckets) for s in slots], sizes, seed, T=[s.view.t_eff + 1 for s in slots])
        used = draw.contributing()
        beh = hip.behaviour_records(handle, tables["fast_records"], [slots[k].mu for k in used])
        for k, fast in zip(used, beh):
            dlogit, dv, _ = hip.learn_bucketed_compact(handle, draw.buckets[k], draw.traj, draw.T[k], tables["records"], fast, None, hp)
        hip.bucket_finish(handle, draw.buckets[used[0]], draw.norm, hp, dlogit, dv)
        torch.cuda.synchronize()
        return dlogit.clone(), dv.clone(), sizes, seed


def test_trainer_draws_lanes_on_the_ring(tmp_path, caplog):
    from environment.episode import CompactBuffer

    tree = cr._ternary4()
    rn = cr._trainer(tree, tmp_path, "lanes", compact_replay=True, replay_lanes=True, replay_batches=2)
    before = [p.detach().clone() for p in rn.net.parameters()]
    ring = rn.make_buffer()
    assert isinstance(ring, CompactBuffer) and ring.max_size == 3
    with caplog.at_level("WARNING"):
        nets = cr._steps(rn, ring, 7)  # appends at steps 0, 2, 4, 6
    assert sum("replay_batches = 2 is ignored" in r.getMessage() for r in caplog.records) == 1, "said once"
    assert len(ring) == 3 and all(torch.isfinite(p).all() for p in nets)
    assert any(not torch.equal(a, b) for a, b in zip(before, rn.net.parameters())), "the update moved the net"
    slot = ring._draw
    assert slot is not None and sum(slot.sizes) == rn.batch_size and len(slot.sizes) == 3
    ptrs = [t.data_ptr() for t in (slot.traj.states, slot.traj.acts, slot.traj.final_reward, slot.lane_ids, slot.norm, slot.workspace)]
    # step 7 plays nothing (buffer_mod = 2): the ring is what the hand-made sequence sees
    assert rn.total_steps == 7
    alpha = 0.9
    states = random.getstate(), np.random.get_state()
    want_l, want_v, sizes, seed = _hand_made_step(rn, ring, alpha)
    random.setstate(states[0])
    np.random.set_state(states[1])
    rn.keep_last_tables = True
    rn.train_step(ring, alpha=alpha)
    torch.cuda.synchronize()
    assert ring._draw is slot and ring._draw.sizes == sizes and ring._draw.seed == seed, "the step made the same draw"
    assert min(sizes) > 0 and max(sizes) < rn.batch_size, "lanes of all three stored batches"
    assert [t.data_ptr() for t in (slot.traj.states, slot.traj.acts, slot.traj.final_reward, slot.lane_ids, slot.norm, slot.workspace)] == ptrs, \
        "the draw slot is allocated once"
    got_l, got_v, _ = rn.last_tables
    assert torch.equal(got_l.view(I32), want_l.view(I32)) and torch.equal(got_v.view(I32), want_v.view(I32)), "the step's row tables"
    assert torch.isfinite(got_l).all() and bool((got_l != 0).any())
    # a logging step stays one whole batch through the dense route
    rn.total_steps = 9
    log = {}
    rn.train_step(ring, alpha=1.0, log=log)
    assert np.isfinite(log["loss_v"]) and np.isfinite(log["actor_learner_kld"])


def test_replay_lanes_off_changes_nothing(tmp_path):
    tree = cr._ternary4()
    runs = []
    for tag, attrs in (("absent", dict(replay_lanes=cr._ABSENT)), ("off", dict(replay_lanes=False))):
        rn = cr._trainer(tree, tmp_path, "lanes_" + tag, compact_replay=True, replay_batches=2, keep_last_tables=True, **attrs)
        ring = rn.make_buffer()
        nets = cr._steps(rn, ring, 6)
        assert ring._draw is None, "no draw slot without replay_lanes"
        runs.append((nets, rn.last_tables))
    assert runs[0][1][0].abs().sum() > 0
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1][0].view(I32), runs[1][1][0].view(I32)) and torch.equal(runs[0][1][1].view(I32), runs[1][1][1].view(I32))
    # ... and on, with the same seeds, it is another update
    rn = cr._trainer(tree, tmp_path, "lanes_on", compact_replay=True, replay_batches=2, keep_last_tables=True, replay_lanes=True)
    cr._steps(rn, rn.make_buffer(), 6)
    assert not torch.equal(rn.last_tables[0], runs[0][1][0])


def test_sample_lanes_needs_device_tensors_and_a_filled_ring():
    from environment.episode import CompactBuffer

    ring = CompactBuffer(2)
    with pytest.raises(ValueError, match="empty"):
        ring.sample_lanes(16)
    hip = _hip()
    A = 2
    h = cr._tree(A).handle()
    B = lr.TREE_B[A]
    (src,), _ = _sources(h, A, 1, cr._params(lr.HP["H0"]), B)
    traj, bk, _ = src
    cpu_traj = hip.Trajectory.compact_like(traj)
    for name in ("states", "acts", "final_reward", "alive"):
        setattr(cpu_traj, name, getattr(traj, name).cpu())
    with pytest.raises(ValueError, match="CPU tensors"):
        hip.draw_lanes(h, [(cpu_traj, bk)], [B], 1)


# ------------------------------------------------------------------------------------------------ d. the refusals
def test_refusals_launch_nothing():
    import _gpu as G

    hip = _hip()
    lib = hip.lib()
    A = 2
    h = cr._tree(A).handle()
    B = lr.TREE_B[A]
    sources, T_cap = _sources(h, A, 2, cr._params(lr.HP["H0"]), B)
    pairs = [(t, b) for t, b, _ in sources]
    draw = hip.draw_lanes(h, pairs, [B // 2, B - B // 2], 3)
    torch.cuda.synchronize()
    sentinel = lambda t: t.fill_(-7 if t.dtype != torch.uint8 else 249)  # noqa: E731
    outs = [draw.traj.states, draw.traj.acts, draw.traj.final_reward, draw.lane_ids, draw.norm, draw.buckets[0].items, draw.buckets[0].n_items,
            draw.buckets[1].items, draw.buckets[1].n_items]
    for t in outs:
        sentinel(t)
    kept = [t.clone() for t in outs]
    with pytest.raises(hip.RnadHipError, match="add up"):
        hip.draw_lanes(h, pairs, [B, 1], 3, out=draw)
    with pytest.raises(hip.RnadHipError, match="add up"):
        hip.draw_lanes(h, pairs, [-1, B + 1], 3, out=draw)
    with pytest.raises(hip.RnadHipError, match="sources"):
        hip.draw_lanes(h, [], [], 3)
    # the C entry point itself
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arr = lambda xs: (C.c_void_p * len(xs))(*xs)  # noqa: E731
    dt = draw.traj.states

    def call(n=2, b=(B // 2, B - B // 2), offset=0, states=None, states_out=None, items_out=None, acts=None):
        src_states = states or [t.states.data_ptr() for t, _ in pairs]
        k = max(n, 1)
        rep = lambda xs: arr((list(xs) * 9)[:max(k, len(xs))])  # noqa: E731
        return lib.rnad_bucket_draw_lanes(
            h.ptr, T_cap, B, n, 0, rep(src_states), rep(acts or [t.acts.data_ptr() for t, _ in pairs]),
            rep([t.final_reward.data_ptr() for t, _ in pairs]), rep([s.lane_ids.data_ptr() for _, s in pairs]),
            rep([s.items.data_ptr() for _, s in pairs]), rep([s.n_items.data_ptr() for _, s in pairs]),
            (C.c_int64 * max(k, len(b)))(*((list(b) * 9)[:max(k, len(b))])), 3, offset,
            states_out or dt.data_ptr(), draw.traj.acts.data_ptr(), draw.traj.final_reward.data_ptr(), draw.lane_ids.data_ptr(),
            rep(items_out or [d.items.data_ptr() for d in draw.buckets]), rep([d.n_items.data_ptr() for d in draw.buckets]),
            draw.norm.data_ptr(), draw.workspace.data_ptr(), stream)

    err = lambda: lib.rnad_last_error()  # noqa: E731
    assert call(n=0) == 2 and b"outside 1 .. 8" in err()
    assert call(n=9, b=(0,)) == 2 and b"outside 1 .. 8" in err()
    assert call(states=[pairs[0][0].states.data_ptr(), None]) == 2 and b"null buffer of source 1" in err()
    assert call(states_out=None, states=None, items_out=[draw.buckets[0].items.data_ptr(), None]) == 2 and b"null" in err()
    assert call(b=(-1, B)) == 2 and b"b[0] = -1 outside" in err()
    assert call(b=(B + 1, 0)) == 2 and b"outside 0 .. B" in err()
    assert call(b=(B // 2, B - B // 2), offset=1) == 2 and b"exceeds B" in err()
    assert call(offset=-1) == 2 and b"offset" in err()
    assert call(states_out=pairs[1][0].states.data_ptr()) == 2 and b"destination states_out overlaps states of source 1" in err()
    assert call(items_out=[pairs[0][1].items.data_ptr(), draw.buckets[1].items.data_ptr()]) == 2 and b"overlaps items of source 0" in err()
    assert call(acts=[draw.traj.acts.data_ptr() + 8, pairs[1][0].acts.data_ptr()]) == 2 and b"acts_out overlaps acts of source 0" in err()
    assert call(items_out=[draw.buckets[0].items.data_ptr()] * 2) == 2 and b"destinations" in err()
    torch.cuda.synchronize()
    for t, want in zip(outs, kept):
        assert torch.equal(t, want), "a refused call writes nothing"
    # a tree / batch that cannot be bucketed: more lanes than the pipeline takes
    assert lib.rnad_bucket_draw_workspace(h.ptr, hip.BUCKET_MAX_LANES + 1) == -1
    # and the accepted call still works afterwards
    hip.draw_lanes(h, pairs, [B // 2, B - B // 2], 3, out=draw)
    _check_draw(h, sources, [B // 2, B - B // 2], 3, draw, T_cap)
