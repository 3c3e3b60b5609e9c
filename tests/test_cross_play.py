"""Cross-play without a GPU: the reference and gate of tests/_crossref.py are pinned against an fp32 restatement, four deliberate
mistakes and the trees' own anchors, and the host half of the C ABI is checked.

The anchors (fp64, on the golden trees):
  - with the tree's `solution` as both policies the recursion reproduces root_value at every state;
  - with the fixture's joint_policy its root value lies between -col_best[1] and row_best[1] of nashconv_<tree>.npz;
  - with i = solution and j = joint_policy, U[i][j] >= U[i][i] >= U[j][i]: the saddle inequality.
"""
import numpy as np
import pytest

import _crossref as cr
from _util import TREES, load

CPU_TREES = TREES + ("native_a5",)
N = 6  # solution, uniform, (fixture,) and seeded softmax tables


@pytest.mark.parametrize("name", CPU_TREES)
def test_fp32_restatement_stays_within_half_the_gate(name):
    tree, J, V, g = cr.case(name, N)
    got, _, _ = cr.reference(tree, J, dtype=np.float32)
    assert got.dtype == np.float32
    worst = cr.share(got, V, g)
    print(f"{name}: fp32 restatement uses {worst:.3f} of the gate")
    assert worst <= 0.5


# c1 has one outcome per joint action (C = 1, chance = 1): there is no chance factor to drop
@pytest.mark.parametrize("name,variant", [(t, v) for t in CPU_TREES for v in cr.VARIANTS if not (t == "c1" and v == "no_chance")])
def test_mutations_exceed_twice_the_gate_at_the_root(name, variant):
    tree, J, V, g = cr.case(name, N)
    assert variant != "no_chance" or np.asarray(tree["index"]).shape[1] > 1
    got, _, _ = cr.reference(tree, J, variant=variant)
    worst = float((np.abs(got[1] - V[1]) / g[1]).max())
    print(f"{name} {variant}: {worst:.1f} gates at the root")
    assert worst > 2.0


@pytest.mark.parametrize("name", TREES)
def test_anchors(name):
    tree, J, V, g = cr.case(name, N)  # player 0: solution, player 2: the fixture's joint_policy
    reached = np.concatenate(cr.level_order(tree["index"], tree["chance"]))
    root_value = np.asarray(tree["root_value"], np.float64)[:, 0]
    assert (np.abs(V[reached, 0, 0] - root_value[reached]) <= g[reached, 0, 0]).all()
    fx = load("nashconv_" + name)
    assert np.array_equal(J[:, 2], fx["joint_policy"])
    assert -float(fx["col_best"][1]) - g[1, 2, 2] <= V[1, 2, 2] <= float(fx["row_best"][1]) + g[1, 2, 2]
    assert V[1, 0, 2] >= V[1, 0, 0] >= V[1, 2, 0]
    assert (V[0] == 0).all()


def test_size_export():
    import rnad_hip

    lib = rnad_hip.lib()
    assert rnad_hip.CROSS_PLAY_MAX == 32
    assert lib.rnad_cross_play_size(2, 1) == 2
    assert lib.rnad_cross_play_size(283, 8) == 283 * 64
    assert lib.rnad_cross_play_size(2**33, 32) == 2**33 * 1024
    for S, n in ((283, 0), (283, 33), (1, 1), (283, -1), (0, 4)):
        assert lib.rnad_cross_play_size(S, n) == -1, (S, n)


def test_binding_refuses_a_cpu_tensor():
    import torch

    import rnad_hip

    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.cross_play(None, torch.zeros(22, 2, 4))
    with pytest.raises(rnad_hip.RnadHipError, match=r"\[S, n, 2A\]"):
        rnad_hip.cross_play(None, torch.zeros(22, 4))


def test_null_arguments_are_refused_on_the_host():
    import rnad_hip

    lib = rnad_hip.lib()
    assert lib.rnad_cross_play(None, 2, None, None, None) != 0
    assert b"rnad_cross_play" in lib.rnad_last_error()
