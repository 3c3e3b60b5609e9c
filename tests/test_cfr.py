"""Exact CFR without a GPU: the reference and gates of tests/_cfrref.py are pinned by what the quantities must satisfy, not by a
measurement --

  - on hand-sized ragged trees the level recursion is a textbook recursive CFR (one Python frame per state, written independently);
  - plain CFR with simultaneous updates satisfies the regret decomposition NashConv(average) <= (sum_s max_a R+_row + sum_s max_b R+_col) / T
    at T = 1, 2, 4, 16, 64, 256 on every tree;
  - the average policy is _mixref.reference's Kuhn mixture of the iterates, uniform weights for plain CFR, weights t for linear averaging;
  - zeroing the negative regrets before the add gives the sigma sequence of textbook CFR+, which clamps after it;
  - the fp32 restatement in the kernel's order stays within half of every gate on all fourteen trees;
  - eight natural mistakes land beyond twice some gate;
  - the inputs reach the edges: a side with sum R+ = 0 at a reached state, a zero-reach state, every sides value;

and the host half of the C ABI is checked: the header, the exports, the refusals, the scratch and registers of the sixteen instantiations.
"""
import os

import numpy as np
import pytest

import _cfrref as cf
import _mixref as mx
import _regref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


# ---------------------------------------------------------------------------------------------------- the textbook recursion
def hand_tree(A, C, seed, depth=3):
    """A small ragged tree as arrays: random legal sets (action 0 always legal, as the legal tensor's layout needs), records without
    chance, records that leave the tree early, states of differing depth."""
    rng = np.random.default_rng(seed)
    index, value, chance, legal = [], [], [], []

    def new_state():
        for arr, shape in ((index, (C, A, A)), (value, (C, A, A)), (chance, (C, A, A)), (legal, (1, A, A))):
            arr.append(np.zeros(shape, np.int64 if arr is index else np.float64))
        return len(index) - 1

    def grow(level):
        s = new_state()
        rows = np.r_[True, rng.random(A - 1) < 0.7]
        cols = np.r_[True, rng.random(A - 1) < 0.7]
        if level == 1:  # below the root one side or the other always lacks its last action
            (rows if s % 2 else cols)[A - 1] = False
        legal[s] = (rows[:, None] & cols[None, :]).astype(np.float64)[None]
        for r in np.flatnonzero(rows):
            for c in np.flatnonzero(cols):
                w = rng.random(C) * (rng.random(C) < 0.75)  # some records carry no chance
                if w.sum() == 0:
                    w[rng.integers(C)] = 1.0
                w = w / w.sum()
                for t in range(C):
                    chance[s][t, r, c] = w[t]
                    first = r == 0 and c == 0 and t == int(np.argmax(w > 0))  # every state above the bound has a child
                    if w[t] > 0 and level < depth and (first or rng.random() < 0.3):
                        index[s][t, r, c] = grow(level + 1)
                    else:
                        value[s][t, r, c] = rng.uniform(-1, 1)  # an early exit (or a payoff no chance ever pays)
                        if w[t] == 0 and rng.random() < 0.5:
                            index[s][t, r, c] = 1  # a dead record may name any state: it is never followed
        return s

    assert new_state() == 0 and grow(0) == 1  # state 0 absorbs, state 1 is the root
    return dict(index=np.stack(index), value=np.stack(value), chance=np.stack(chance), legal=np.stack(legal))


class Textbook:
    """Recursive CFR on a tree of arrays: regrets and strategy sums per state, one frame per state."""

    def __init__(self, tree):
        self.t = tree
        S, C, A, _ = tree["index"].shape
        self.A, self.C = A, C
        self.R = np.zeros((S, 2, A))
        self.T = np.zeros((S, 2, A))
        self.sigma = np.zeros((S, 2, A))

    def legal(self, s, side):
        lg = self.t["legal"][s, 0]
        return [a for a in range(self.A) if (lg[a, 0] if side == 0 else lg[0, a]) != 0]

    def match(self, s, side):
        acts = self.legal(s, side)
        plus = {a: max(self.R[s, side, a], 0.0) for a in acts}
        tot = sum(plus[a] for a in acts)
        sig = np.zeros(self.A)
        for a in acts:
            sig[a] = plus[a] / tot if tot > 0 else 1.0 / len(acts)
        return sig

    def walk(self, s, own, chn, disc, sides):
        """own = (row reach, column reach); returns the row player's value of s under the current strategy."""
        sig = [self.match(s, 0), self.match(s, 1)]
        self.sigma[s] = sig
        Q = np.zeros((self.A, self.A))
        for r in range(self.A):
            for c in range(self.A):
                for t in range(self.C):
                    w, u = self.t["chance"][s, t, r, c], int(self.t["index"][s, t, r, c])
                    if w <= 0:
                        continue
                    x = self.t["value"][s, t, r, c] if u == 0 else self.walk(u, (own[0] * sig[0][r], own[1] * sig[1][c]), chn * w, disc, sides)
                    Q[r, c] += w * x
        q = [Q @ sig[1], -(sig[0] @ Q)]
        v = float(sig[0] @ q[0])
        dp, dn, da = disc
        for side in (0, 1):
            if not (sides >> side) & 1:
                continue
            cfv, u = own[1 - side] * chn, (v if side == 0 else -v)
            for a in self.legal(s, side):
                old = self.R[s, side, a]
                self.R[s, side, a] = (dp if old > 0 else dn) * old + cfv * (q[side][a] - u)
                self.T[s, side, a] = da * self.T[s, side, a] + own[side] * sig[side][a]
        return v

    def tables(self):
        S = self.R.shape[0]
        return self.R.reshape(S, 1, -1).copy(), self.T.reshape(S, 1, -1).copy()


@pytest.mark.parametrize("A,C,seed", [(2, 1, 0), (2, 3, 1), (3, 2, 2), (3, 3, 3), (4, 1, 4), (4, 2, 5), (4, 3, 6)])
@pytest.mark.parametrize("variant,alternating", [("cfr", False), ("cfr+", True), ("linear", False), (("dcfr", 1.5, 0.0, 2.0), True)])
def test_level_recursion_is_the_textbook_recursion(A, C, seed, variant, alternating):
    tree = hand_tree(A, C, seed)
    S = tree["index"].shape[0]
    mask = cf.legal_mask(tree)
    live, playable = tree["chance"] > 0, (mask[:, :A, None] & mask[:, None, A:])[:, None]
    depth = cf.iterate(tree, np.zeros((S, 1, 2 * A)), np.zeros((S, 1, 2 * A)), np.ones((1, 3)), [3]).depth
    assert S >= 4 and (~mask[1:]).any(), "illegal actions"
    assert C == 1 or (~live & playable).any(), "records without chance on a legal joint action"
    assert (live & (tree["index"] == 0))[(depth >= 0) & (depth < depth.max())].any(), "records that leave the tree above the deepest level"
    book = Textbook(tree)
    R, T = np.zeros((S, 1, 2 * A)), np.zeros((S, 1, 2 * A))
    for t in range(1, 7):
        disc, sides = cf.schedule(variant, t), cf.turn(alternating, t)
        ref = cf.iterate(tree, R, T, np.asarray([disc]), [sides])
        # (iterate reads the discounts as fp32, as the kernel does: hand the textbook the same numbers)
        root = book.walk(1, (1.0, 1.0), 1.0, tuple(np.asarray(disc, np.float32).astype(np.float64)), sides)
        R, T = ref.RG, ref.SS
        bR, bT = book.tables()
        reached = ref.depth >= 0
        assert abs(root - ref.V[1, 0]) <= 1e-12
        assert np.abs(bR - R)[reached].max() <= 1e-12 and np.abs(bT - T)[reached].max() <= 1e-12
        assert np.abs(book.sigma.reshape(S, -1)[reached] - ref.P[reached, 0]).max() <= 1e-12
        assert (R[~reached] == 0).all() and (T[~reached] == 0).all() and (R[:, 0][~mask] == 0).all()


# ---------------------------------------------------------------------------------------------------- what CFR must satisfy
@pytest.mark.parametrize("name", cf.ALL_TREES)
def test_regret_bound_of_plain_cfr(name):
    """The regret decomposition: holds for any sequence of strategies."""
    tree = rr.tree_arrays(name)
    mask = cf.legal_mask(tree)
    R, S = np.zeros((mask.shape[0], 1, mask.shape[1])), np.zeros((mask.shape[0], 1, mask.shape[1]))
    disc = cf.discounts(["cfr"], [1])
    for T in range(1, 257):
        ref = cf.iterate(tree, R, S, disc, [3])
        R, S = ref.RG, ref.SS
        if T in (1, 2, 4, 16, 64, 256):
            nc = rr.nashconv64(name, cf.average_policy(mask, S)[:, 0])
            bound = cf.positive_regret(mask, R)[0].sum() / T
            print(f"{name} T={T}: NashConv(average) {nc:.6g} <= {bound:.6g}")
            assert nc <= bound + 1e-12 * max(1.0, bound)


@pytest.mark.parametrize("name", ("small", "ragged", "a5"))
@pytest.mark.parametrize("variant", ("cfr", "linear"))
def test_average_policy_is_the_mixture_of_the_iterates(name, variant):
    T = 6
    tree = rr.tree_arrays(name)
    mask = cf.legal_mask(tree)
    R, S, iterates = cf.run(name, variant, T, keep=True)
    # iteration j enters with the product of the later da: 1 for plain CFR, j / T for linear averaging -- up to the fp32 rounding of each
    # (t - 1) / t, which the device reads and the mixture is therefore given
    da = [float(cf.discounts([variant], [t])[0, 2]) for t in range(1, T + 1)]
    w = np.asarray([np.prod(da[j:]) for j in range(1, T + 1)])
    assert np.abs(w / w.sum() - (np.ones(T) / T if variant == "cfr" else np.arange(1, T + 1) / (T * (T + 1) / 2))).max() <= 4 * T * cf.U
    M, _, depth = mx.reference(tree, np.stack(iterates, axis=1), np.stack([w / w.sum()] * 2))
    avg = cf.average_policy(mask, S)[:, 0]
    # (the first iterate is uniform, so every reached state has a positive strategy sum on both sides: the mixture's reach branch)
    assert (depth >= 0).sum() > 1 and np.abs(avg - M)[depth >= 0].max() <= 1e-12
    assert any(((p == 0) & mask)[depth >= 0].any() for p in iterates), "some iterate has left the interior: a legal action at probability 0"


def test_zero_then_add_is_add_then_clamp():
    """dn = 0 zeroes the negative regrets before the add; textbook CFR+ clamps after it.  The same R+, so the same sigma sequence."""
    name = "ragged"
    tree = rr.tree_arrays(name)
    mask = cf.legal_mask(tree)
    shape = (mask.shape[0], 1, mask.shape[1])
    Rz, Sz, Rc, Sc = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    negatives = 0
    for t in range(1, 13):
        da = (t - 1) / t
        z = cf.iterate(tree, Rz, Sz, np.asarray([[1.0, 0.0, da]]), [cf.turn(True, t)])
        c = cf.iterate(tree, Rc, Sc, np.asarray([[1.0, 1.0, da]]), [cf.turn(True, t)])
        assert np.array_equal(z.P, c.P) and np.array_equal(z.SS, c.SS) and np.array_equal(z.V, c.V)
        assert np.array_equal(np.maximum(z.RG, 0), np.maximum(c.RG, 0))
        negatives += int((z.RG < 0).sum())
        Rz, Sz, Rc, Sc = z.RG, z.SS, np.maximum(c.RG, 0), c.SS
    assert negatives > 0


# ---------------------------------------------------------------------------------------------------- gates
@pytest.mark.parametrize("name", cf.ALL_TREES)
def test_fp32_restatement_stays_within_half_the_gates(name):
    c = cf.case(name)
    got = cf.iterate(c.tree, c.R, c.S, c.discount, c.sides, dtype=np.float32)
    shares = cf.shares(c.ref, c.g, got)
    print(f"{name}: fp32 restatement uses {shares} of the gates")
    assert max(shares.values()) <= 0.5
    for a in (got.P, got.V, got.reach):
        assert (a[~c.reached] == 0).all()
    assert np.array_equal(got.RG[~c.reached], c.R[~c.reached]) and np.array_equal(got.SS[~c.reached], c.S[~c.reached])
    # a slice of the members is the case of fewer members: they do not see each other
    few = cf.iterate(c.tree, c.R[:, :3], c.S[:, :3], c.discount[:3], c.sides[:3], dtype=np.float32)
    assert np.array_equal(few.RG, got.RG[:, :3]) and np.array_equal(few.V, got.V[:, :3]) and np.array_equal(few.reach, got.reach[:, :, :3])


BEYOND = dict(no_chance_cf=("RG",), joint_cf=("RG",), own_reach_regret=("RG",), opp_reach_average=("SS",), col_sign=("RG",),
              dp_dn_swapped=("RG",), uniform_all_actions=("P",), cleared_side_updated=("RG", "SS"))


def _applies(name, variant):
    _, C, A, _ = np.asarray(rr.tree_arrays(name)["index"]).shape
    if variant == "no_chance_cf":
        return A >= 2 and C >= 2  # with one outcome per joint action chance is 1
    if variant == "uniform_all_actions":
        return name == "ragged"  # the tree whose states have illegal actions on a side with sum R+ = 0
    if variant == "col_sign":
        return True
    return A >= 2  # with one action q = v: the regrets stay 0


MUTATIONS = [(t, v) for t in cf.ALL_TREES for v in cf.VARIANTS if _applies(t, v)]


@pytest.mark.parametrize("name,variant", MUTATIONS)
def test_mutations_exceed_twice_a_gate(name, variant):
    c = cf.case(name)
    got = cf.iterate(c.tree, c.R, c.S, c.discount, c.sides, variant=variant)
    shares = cf.shares(c.ref, c.g, got)
    print(f"{name} {variant}: {shares} gates off")
    for key in BEYOND[variant]:
        assert shares[key] > 2.0


@pytest.mark.parametrize("name", cf.ALL_TREES)
def test_the_inputs_reach_the_edges(name):
    c = cf.case(name)
    A = c.R.shape[2] // 2
    mask = c.ref.mask
    plus = np.where(mask[:, None, :], np.maximum(c.R, 0), 0)
    assert sorted(set(c.sides.tolist())) == [1, 2, 3] and c.discount.shape == (32, 3)
    assert {cf.member(k)[0] for k in range(32)} == set(cf.MEMBERS) and {cf.member(k)[1] for k in range(32)} == set(range(8))
    assert {(cf.member(k)[0], cf.member(k)[2]) for k in range(32)} == {(v, a) for v in cf.MEMBERS for a in (False, True)}
    nonzero = np.abs(c.R[c.R != 0])
    assert nonzero.size == 0 or nonzero.min() >= 2.0 ** -60, "nonzero regrets stay far above the denormal range"
    if A == 1:
        return
    row_zero = (plus[:, :, :A].sum(axis=2) == 0) & c.reached[:, None]
    started = np.asarray([cf.member(k)[1] > 0 for k in range(32)])
    assert row_zero[c.reached][:, ~started].all() and not row_zero[c.reached][:, started].all(), \
        "sum R+ = 0 at every reached state of the members that start from zero tables, regret matching proper elsewhere"
    assert (c.R < 0).any() and (c.S > 0).any()
    joint = c.ref.reach[:, 0] * c.ref.reach[:, 1]
    assert ((joint == 0) & c.reached[:, None]).any(), "a reached state with zero reach"
    assert ((c.ref.reach[:, 1] == 0) & c.reached[:, None] & (c.sides[None, :] & 1 != 0)).any(), "zero counterfactual reach on an updating side"


# ---------------------------------------------------------------------------------------------------- host half of the C ABI
def test_the_header_declares_both_entry_points():
    import ctypes as C

    import rnad_hip

    protos = rnad_hip.header_prototypes()
    assert protos["rnad_cfr_size"] == (C.c_int64, [C.c_int64, C.c_int])
    assert protos["rnad_cfr_iterate"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8)


def test_the_library_exports_both_and_the_size_companion_answers():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_cfr_iterate is not None
    for S, n in ((2, 1), (283, 8), (2**33, 32), (283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_cfr_size(S, n) == cf.size(S, n), (S, n)
    assert cf.size(283, 8) == 3 * 283 * 8 and cf.size(1, 1) == -1 and cf.size(283, 33) == -1


def test_no_instantiation_uses_scratch():
    import rnad_hip

    table = cf.kernel_metadata(os.path.realpath(rnad_hip.SO_PATH))
    print({k: table[k] for k in sorted(table)})
    assert sorted(table) == [(kernel, A) for kernel in ("reach", "update") for A in range(1, 9)], "one k_cfr_reach and one k_cfr_update per A"
    assert all(k["scratch"] == 0 for k in table.values())
    assert all(k["lds"] == (4 * A * A * 8 * 3 * 4 if kernel == "update" else 0) for (kernel, A), k in table.items()), \
        "four waves' record slices in the bottom-up kernel, nothing else"
    # registers: the top-down kernel keeps full occupancy (8 waves per SIMD: at most 64), the bottom-up one holds Q[A * A] and four
    # A-vectors and must stay at 4 waves per SIMD or better (at most 128) at A = 8
    assert all(k["vgpr"] <= 64 for (kernel, A), k in table.items() if kernel == "reach")
    assert all(k["vgpr"] <= 128 for (kernel, A), k in table.items() if kernel == "update")


def test_null_arguments_member_counts_and_a_cpu_tensor_are_refused_on_the_host():
    import ctypes as C

    import torch

    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_cfr_iterate(None, 2, None, None, None, None, None, None, None, None) != 0
    assert b"rnad_cfr_iterate: null" in lib.rnad_last_error()
    somewhere = [C.c_void_p(4096 * (i + 1)) for i in range(8)]  # never followed: the member count is refused first
    for position in range(8):
        args = list(somewhere)
        args[position] = None
        assert lib.rnad_cfr_iterate(args[0], 2, *args[1:], None) != 0 and b"null" in lib.rnad_last_error()
    for n in (0, -1, 33):
        assert lib.rnad_cfr_iterate(somewhere[0], n, *somewhere[1:], None) != 0
        assert b"outside [1,32]" in lib.rnad_last_error()
    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.cfr_iterate(None, torch.zeros(22, 2, 4), torch.zeros(22, 2, 4), torch.ones(2, 3), torch.ones(2, dtype=torch.int32))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.cfr_iterate(None, torch.zeros(22, 4), torch.zeros(22, 4), torch.ones(2, 3), torch.ones(2, dtype=torch.int32))


def test_the_schedule_is_the_table_of_the_four_variants():
    assert cf.schedule("cfr", 7) == (1.0, 1.0, 1.0)
    assert cf.schedule("cfr+", 4) == (1.0, 0.0, 0.75) and cf.schedule("linear", 4) == (1.0, 1.0, 0.75)
    dp, dn, da = cf.schedule(("dcfr", 1.5, 0.0, 2.0), 5)
    assert abs(dp - 8.0 / 9.0) <= 1e-15 and dn == 0.5 and abs(da - 0.64) <= 1e-15
    assert cf.schedule(("dcfr", 1.5, float("-inf"), 2.0), 3)[1] == 0.0 and cf.schedule(("dcfr", 1.5, 0.0, 2.0), 1) == (0.0, 0.5, 0.0)
    from learn import tabular

    for v in cf.MEMBERS + (("dcfr", 1.5, float("-inf"), 2.0),):
        for t in (1, 2, 3, 10, 1000):
            assert tabular.cfr_discounts(v, t) == cf.schedule(v, t)
