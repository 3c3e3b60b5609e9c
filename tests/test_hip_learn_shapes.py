"""The learner kernels -- process_policy, the two-player V-trace scan, the NeuRD loss with its closed-form gradient and the per-row sums
of those gradients (csrc/learn_math.hpp in k_learn_fused<A, TAB> and k_bucket_learn<A>, k_vtrace / k_loss_v / k_loss_nerd, k_row_sums,
fixed_point_for) -- against the fp64 restatement of the reference's RNaD.__learn in tests/_learnref.py, at every A = 1 .. 8, away from the
unit hyperparameters (sets H0 .. H3), off-policy, over more than one workgroup.

Every comparison is |got - want| <= K 2^-24 mag on every slot and every row (mag: the magnitude the reference carries beside each value;
K per output family from tests/test_learn_shapes.py, where two fp32 programs on these very inputs use at most half of it); a row table
adds the fixed-point term of its path, slots * half a unit.  Nothing is rejected at comparison time: the inputs hold no row whose
decisions (process_policy, the threshold gates) are within 1e-4 of a boundary.

  a. rnad_learn_fused on the dense batches (every T of 1, 2, 7, 32 with every B of 1, 255, 257, 1023; lanes of every length, carry resets, illegal
     actions, mu independent of the learner): pi, both v_target, both q, dlogit, dv, losses; and in the same cases the composition
     policy_head -> process_policy -> vtrace x 2 -> loss_v / loss_nerd (accumulate) gives the fused kernel's bits;
  b. rnad_learn_fused_gather and rnad_learn_fused_tabular on tree batches played off-policy on the host (native trees A = 1 .. 8 and the
     golden tree with ragged legality): per-slot gradients, the row tables with k_row_sums' term, two runs with identical bits;
  c. rnad_learn_bucketed (mu per slot) on the same batches, bucketised on the host: row tables and losses with fixed_point_for's term,
     identical bits twice, accumulators zero afterwards; the trees the planner refuses are pinned (none) and would be skipped;
  d. rnad_learn_bucketed_compact (fast_slot on the fast records) on-policy on the batch rnad_rollout_bucketed_compact plays on every
     native tree under every set: the two-launch tables and losses against fp64 on the dense expansion; at A = 1, 4, 6, 7, 8 the one-launch
     rnad_rollout_learn_bucketed_compact, plain and distinct, gives the two-launch bits (under H3 it refuses: clip >= 2^29).

The worst share of the gate per case and output goes to learn_errors.json in the directory RNAD_ERRORS_DIR names, when it is set;
profiles/learn_errors.json holds the figures of an MI355X."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _learnref as lr
from test_learn_shapes import TREE_CASES, native_tree, tree_case, tree_reference

pytestmark = pytest.mark.gpu

I32 = torch.int32


@pytest.fixture(scope="module", autouse=True)
def _log_figures():
    lr.SHARES.clear()
    yield
    out = os.environ.get("RNAD_ERRORS_DIR", "")
    if lr.SHARES and os.path.isdir(out):
        with open(os.path.join(out, "learn_errors.json"), "w") as f:
            json.dump(lr.SHARES, f, indent=1, sort_keys=True)


def _hip():
    import rnad_hip

    return rnad_hip


def _params(hp):
    return _hip().make_learn_params(**lr.hp_kwargs(hp))


def _batch_on_device(batch, perm=None):
    import _gpu as G

    sel = (lambda x: x) if perm is None else (lambda x: x[:, perm])  # noqa: E731
    valid = batch["indices"] != 0
    T = valid.shape[0]
    norm = np.array([valid[0:T:2].sum(), valid[1:T:2].sum()], np.float64)
    return dict(indices=G.gpu(sel(batch["indices"]), I32), mask_bits=G.gpu(sel(lr.mask_bits(batch["legal"]))), actions=G.gpu(sel(batch["actions"]), I32),
                rewards=G.gpu(sel(batch["rewards"])), mu=G.gpu(sel(batch["mu"]))), G.gpu(norm)


def _same_bits(a, b, what):
    """Two runs: the gradients (per slot, or summed per row in fixed point) have identical bits.  The two losses are fp64 block partials
    added with atomics in the order the workgroups arrive: equal up to the rounding of those fp64 additions."""
    (*grads_a, loss_a), (*grads_b, loss_b) = a, b
    for x, y in zip(grads_a, grads_b):
        assert x.dtype == torch.float32 and torch.equal(x.view(I32), y.view(I32)), what
    np.testing.assert_allclose(loss_a.cpu().numpy(), loss_b.cpu().numpy(), rtol=1e-12, atol=1e-300)


# ------------------------------------------------------------------------------------------------ a. the fused kernel, dense batches
@pytest.mark.parametrize("key", lr.dense_cases(), ids=lr.case_id)
def test_learn_fused_and_the_composition_of_the_single_kernels(key):
    import _gpu as G

    hip = _hip()
    A, s, T, B = key
    hp = lr.HP[s]
    batch, slots = lr.dense_case(key)
    ref = lr.dense_reference(key)
    dev, norm = _batch_on_device(batch)
    logit, v, vtn, lreg, lreg_ = (G.gpu(slots[k]) for k in ("logit", "v", "v_target", "logit_reg", "logit_reg_"))
    params = _params(hp)
    dlogit, dv, losses, pi, vt, q = hip.learn_fused(logit=logit, v=v, v_target_net=vtn, logit_reg=lreg, logit_reg_=lreg_, norm=norm, hp=params,
                                                    want_aux=True, **dev)
    torch.cuda.synchronize()
    lr.compare(lr.case_id(key), ref, dict(pi=G.cpu(pi), v_target=G.cpu(vt), q=G.cpu(q), dlogit=G.cpu(dlogit), dv=G.cpu(dv), losses=G.cpu(losses)))
    # the single kernels, composed (tests/test_hip_parity.py on two fixtures): the fused kernel's bits
    bits, acts, idx = dev["mask_bits"].view(-1), dev["actions"], dev["indices"]
    pi2, logp = hip.policy_head(logit.view(-1, A), mask_bits=bits, want_log=True)
    _, logr = hip.policy_head(lreg.view(-1, A), mask_bits=bits, want_log=True)
    _, logr_ = hip.policy_head(lreg_.view(-1, A), mask_bits=bits, want_log=True)
    assert torch.equal(pi.view(-1, A), pi2)
    legal = G.gpu(batch["legal"])
    pip = hip.process_policy(pi2, legal.view(-1, A), hp.n_disc, hp.eps)
    assert np.array_equal(G.cpu(pip).astype(np.float64).reshape(T, B, A), ref.pi_processed.v), "pi_processed is exact"
    # alpha and 1 - alpha as the kernel holds them: fp32 scalars on fp32 tensors, one rounding per operation
    lpol = (logp - (logr * params.alpha + logr_ * params.one_minus_alpha)).view(T, B, A).contiguous()
    valid = (idx != 0).float()
    dl2, dv2 = torch.empty_like(dlogit), torch.empty_like(dv)
    loss2 = torch.zeros((2,), dtype=torch.float64, device=G.DEV)
    turn = (torch.arange(T, device=G.DEV) % 2).view(T, 1).expand(T, B)
    for p in range(2):
        rew = dev["rewards"] if p == 0 else -dev["rewards"]
        vt_p, _, q_p = hip.vtrace(vtn, valid, None, dev["mu"], pip.view(T, B, A), lpol, acts, rew.contiguous(), p, eta=hp.eta, lambda_=hp.lambda_, c=hp.c,
                                  rho=hp.rho, gamma=hp.gamma)
        assert torch.equal(vt_p, vt[p]) and torch.equal(q_p, q[p]), f"k_vtrace, player {p}"
        m = (valid * (turn == p)).contiguous()
        hip.loss_v(v.reshape(-1), vt_p.view(-1), m.view(-1), norm[p:p + 1], hp.w_v, loss2[0:1], dv2.view(-1), p > 0)
        hip.loss_nerd(logit.view(-1, A), pip, q_p.view(-1, A), m.view(-1), legal.view(-1, A), norm[p:p + 1], hp.clip, hp.threshold, hp.w_n, loss2[1:2],
                      dl2.view(-1, A), p > 0)
    assert torch.equal(dv2, dv), "k_loss_v"
    assert torch.equal(dl2, dlogit), "k_loss_nerd"
    np.testing.assert_allclose(G.cpu(loss2), G.cpu(losses), rtol=1e-12, atol=1e-300)


# ------------------------------------------------------------------------------------------------ b, c. tree batches
@functools.lru_cache(maxsize=None)
def _tree(name):
    import _gpu as G

    if name == "ragged":
        return G.golden_tree("ragged")[0]
    arrs = native_tree(name)
    return G.tree_from_arrays(arrs, depth_bound=lr.TREES[name]["depth_bound"])


REFUSED = frozenset()  # the trees (by A, or "ragged") that rnad_bucket_plan refuses at the sweep's batch size: none


def _tree_id(key):
    return f"tree_A{key[0]}_{key[1]}"


def _tables_on_device(tables):
    import _gpu as G

    return [G.gpu(tables[k]).view(len(tables[k]), -1) for k in ("logit", "v", "v_target", "logit_reg", "logit_reg_")]


def _column_units(ref, dlogit, dv):
    """k_row_sums' unit per column of [dlogit[A] | dv], from the largest |addend| of the column over the valid slots.  The kernel takes
    it from its own fp32 addends (dlogit, dv: the gather kernel's, the same bits), the bound from the fp64 reference's: where the two
    maxima straddle a power of two the larger unit holds."""
    A = ref.dlogit.v.shape[-1]
    top = lambda x, y: max(lr.row_sums_unit(np.abs(x[ref.valid]).max(initial=0.0)), lr.row_sums_unit(np.abs(y[ref.valid]).max(initial=0.0)))  # noqa: E731
    return np.array([top(ref.dlogit.v[..., a], dlogit[..., a]) for a in range(A)]), top(ref.dv.v, dv)


def _compare_tables(case, ref, dl_tab, dv_tab, fixed_l, fixed_v, tag):
    import _gpu as G

    sl = lr.table_share(G.cpu(dl_tab), ref.dlogit_tab, fixed_l) / lr.K["tables"]
    sv = lr.table_share(G.cpu(dv_tab), ref.dv_tab, fixed_v) / lr.K["tables"]
    lr.log_share(case, tag + "dlogit_tab", sl)
    lr.log_share(case, tag + "dv_tab", sv)
    assert sl <= 1 and sv <= 1, f"{case} {tag}: row tables outside the gate: dlogit_tab {sl:.3f}, dv_tab {sv:.3f} of it"


@pytest.mark.parametrize("key", TREE_CASES, ids=_tree_id)
def test_gather_and_tabular_on_off_policy_tree_batches(key):
    import _gpu as G

    hip = _hip()
    hp = lr.HP[key[1]]
    batch, tables = tree_case(key)
    ref = tree_reference(key)
    h = _tree(key[0]).handle()
    assert h.S == batch["S"]
    dev, norm = _batch_on_device(batch)
    tabs = _tables_on_device(tables)
    params = _params(hp)
    case = _tree_id(key)
    first = hip.learn_fused_gather(h, *dev.values(), *tabs, norm, params)
    _same_bits(first, hip.learn_fused_gather(h, *dev.values(), *tabs, norm, params), f"{case}: two runs of the gather kernel differ")
    dlogit, dv, losses = first
    lr.compare(case, ref, dict(dlogit=G.cpu(dlogit), dv=G.cpu(dv), losses=G.cpu(losses)))
    first = hip.learn_fused_tabular(h, *dev.values(), *tabs, norm, params)
    _same_bits(first, hip.learn_fused_tabular(h, *dev.values(), *tabs, norm, params), f"{case}: two runs of the tabular kernel differ")
    dl_tab, dv_tab, losses = first
    unit_l, unit_v = _column_units(ref, G.cpu(dlogit), G.cpu(dv))
    slots = ref.row_slots.astype(np.float64)
    _compare_tables(case, ref, dl_tab, dv_tab, slots[:, None] * 0.5 * unit_l[None], slots * 0.5 * unit_v, "tabular_")
    lr.log_share(case, "tabular_losses", lr.share(G.cpu(losses), ref.losses) / lr.K["losses"])
    assert lr.share(G.cpu(losses), ref.losses) <= lr.K["losses"]
    rows = ~np.isin(np.arange(2 * h.S), (np.arange(len(batch["indices"])) & 1)[:, None] * h.S + batch["indices"])
    assert (G.cpu(dl_tab)[rows] == 0).all() and (G.cpu(dv_tab)[rows] == 0).all(), "a row no slot visits has a zero sum"


@pytest.mark.parametrize("key", TREE_CASES, ids=_tree_id)
def test_dense_bucketed_learner_on_off_policy_tree_batches(key):
    import _gpu as G

    hip = _hip()
    hp = lr.HP[key[1]]
    batch, tables = tree_case(key)
    ref = tree_reference(key)
    tree = _tree(key[0])
    h = tree.handle()
    B = batch["indices"].shape[1]
    plan = hip.bucket_plan(h, B)
    assert (plan is None) == (key[0] in REFUSED), f"{_tree_id(key)}: the planner's refusals are the pinned ones"
    if plan is None:
        pytest.skip(f"rnad_bucket_plan refuses this tree at B = {B}: no bucketed update to compare, and no cut is forced")
    perm, items = G.bucket_order(tree, B, batch["indices"].astype(np.int64))
    dev, norm = _batch_on_device(batch, perm)
    buckets = G.buckets_of(tree, B, perm, items)
    params = _params(hp)
    case = _tree_id(key)
    rec = hip.bucket_records(h, *_tables_on_device(tables), params)
    args = (h, buckets, dev["indices"], dev["actions"], dev["rewards"], dev["mu"], rec, norm, params)
    first = hip.learn_bucketed(*args, want_losses=True)
    _same_bits(first, hip.learn_bucketed(*args, want_losses=True), f"{case}: two runs of the bucketed learner differ")
    dl_tab, dv_tab, losses = first
    unit_l, unit_v = lr.bucketed_units(hp)
    A = batch["mu"].shape[-1]
    n_row = np.repeat(ref.norm, h.S)  # N_P of the row's player
    slots = ref.row_slots.astype(np.float64)
    _compare_tables(case, ref, dl_tab, dv_tab, (slots * 0.5 * unit_l * hp.w_n / n_row)[:, None] * np.ones(A), slots * 0.5 * unit_v * hp.w_v / n_row, "bucketed_")
    s = lr.share(G.cpu(losses), ref.losses) / lr.K["losses"]
    lr.log_share(case, "bucketed_losses", s)
    assert s <= 1, f"{case}: losses at {s:.3f} of the gate"
    acc = buckets.plan.accumulators
    assert (acc[: (2 * h.S + 128 * max(buckets.plan.n_upper, 1)) * (A + 1)] == 0).all(), "the accumulators are zero again"


# ------------------------------------------------------------------------------------------------ d. the fast records, on-policy
ONE_LAUNCH_A = (1, 4, 6, 7, 8)  # the action counts tests/test_hip_bucket.py does not take the one-launch kernel to


@pytest.mark.parametrize("key", lr.tree_cases(), ids=_tree_id)
def test_compact_learners_on_the_batch_the_kernels_play(key, monkeypatch):
    """rnad_rollout_bucketed_compact + rnad_learn_bucketed_compact (fast_slot on the records of write_row_records): the batch is played
    by the kernels from the learner's own policy rows; the reference takes the dense expansion (Trajectory.indices, rnad_bucket_expand)
    with mu = the fp64 policy head of the actor's row.  Then rnad_rollout_learn_bucketed_compact, plain and distinct, bit for bit."""
    import _gpu as G

    hip = _hip()
    A, s = key
    hp = lr.HP[s]
    _, tables = tree_case(key)
    tree = _tree(A)
    h = tree.handle()
    B, S = lr.TREE_B[A], h.S
    case = _tree_id(key)
    refused = hip.bucket_plan(h, B) is None
    assert refused == (A in REFUSED), f"{case}: the planner's refusals are the pinned ones"
    if refused:
        pytest.skip(f"rnad_bucket_plan refuses this tree at B = {B}: no bucketed update to compare, and no cut is forced")
    params = _params(hp)
    rec, fast = hip.bucket_records(h, *_tables_on_device(tables), params, fast=True)
    T = 2 * h.max_depth

    def traj():
        return hip.Trajectory(h, B, T, G.DEV, with_observations=False, with_values=False, compact=True)

    two = traj()
    bk2 = hip.rollout_bucketed_compact(h, two, rec, seed=21, lane0=77)
    first = hip.learn_bucketed_compact(h, bk2, two, T, rec, fast, bk2.norm, params, want_losses=True)
    _same_bits(first, hip.learn_bucketed_compact(h, bk2, two, T, rec, fast, bk2.norm, params, want_losses=True), f"{case}: two runs differ")
    dl_tab, dv_tab, losses = first
    # the reference on the dense expansion
    idx = G.cpu(two.indices)[:T].astype(np.int32)
    hip.bucket_expand(h, two, rec)
    legal_tab = lr.legal_table(G.cpu(tree.legal_tensor))
    rows = (np.arange(T) & 1)[:, None] * S + idx
    valid = idx != 0
    assert np.array_equal(G.cpu(two.mask_bits)[valid], lr.mask_bits(legal_tab[rows])[valid])
    pi64 = lr.policy_head(np.float64, tables["logit"], legal_tab)[0].v
    batch = dict(indices=idx, legal=legal_tab[rows], actions=G.cpu(two.actions), rewards=G.cpu(two.rewards), mu=pi64[rows], S=S)
    assert np.abs(G.cpu(two.policy)[valid] - pi64[rows][valid]).max() < 1e-6, "the actor is the learner's policy head"
    ref = lr.learner(np.float64, batch, tables, hp)
    assert (ref.margin >= lr.MARGIN).all()
    assert np.array_equal(G.cpu(bk2.norm), [valid[0::2].sum(), valid[1::2].sum()])
    unit_l, unit_v = lr.bucketed_units(hp)
    n_row = np.repeat(ref.norm, S)
    slots = ref.row_slots.astype(np.float64)
    _compare_tables(case, ref, dl_tab, dv_tab, (slots * 0.5 * unit_l * hp.w_n / n_row)[:, None] * np.ones(A), slots * 0.5 * unit_v * hp.w_v / n_row, "compact_")
    sl = lr.share(G.cpu(losses), ref.losses) / lr.K["losses"]
    lr.log_share(case, "compact_losses", sl)
    assert sl <= 1, f"{case}: losses at {sl:.3f} of the gate"
    # one launch for rollout + learner
    if A not in ONE_LAUNCH_A:
        return
    for distinct in (False, True):
        if distinct:
            monkeypatch.setenv("RNAD_FUSED_CHUNK", "512" if B == 3000 else "1024")
        one = traj()
        if lr.bucketed_exponents(hp)[2]:  # a clip of 2^29 or more takes the two-launch path
            with pytest.raises(hip.RnadHipError, match="two-launch"):
                hip.rollout_learn_bucketed_compact(h, one, rec, fast, params, seed=21, lane0=77, distinct=distinct)
            continue
        bk1, dl1, dv1 = hip.rollout_learn_bucketed_compact(h, one, rec, fast, params, seed=21, lane0=77, distinct=distinct)
        assert torch.equal(bk1.lane_ids, bk2.lane_ids) and torch.equal(bk1.norm, bk2.norm) and torch.equal(one.acts, two.acts)
        assert torch.equal(one.indices, two.indices)
        assert torch.equal(dl1.view(I32), dl_tab.view(I32)) and torch.equal(dv1.view(I32), dv_tab.view(I32)), f"{case}: one launch, distinct={distinct}"
