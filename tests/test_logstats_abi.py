"""The logged statistics from the compact trajectory (rnad_bucket_log_stats): declared, exported, bound, and off by default."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnad_hip.h")
SO = os.path.join(ROOT, "r-nad_amd", "csrc", "librnad_hip.so")


def test_header_declares_and_library_exports_the_entry():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+rnad_bucket_log_stats\s*\(", src), "include/rnad_hip.h must declare rnad_bucket_log_stats"
    assert os.path.exists(SO), "build it first: make -C r-nad_amd/csrc (or __graft_entry__.build())"
    assert hasattr(ctypes.CDLL(SO), "rnad_bucket_log_stats")


def test_binding_takes_the_prototype_from_the_header():
    import rnad_hip

    ptr, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert list(rnad_hip.lib().rnad_bucket_log_stats.argtypes) == [ptr, i32, i64] + [ptr] * 9
    assert callable(rnad_hip.bucket_log_stats)


def test_compact_log_is_off_by_default():
    from learn.rnad import RNaD

    assert RNaD.compact_log is False


def test_host_side_of_the_statistics():
    """The nine keys' arithmetic on the host copy of the eight sums (section 'Results' of the contract)."""
    import rnad_hip

    T, B, A = 4, 10, 3
    got = rnad_hip.log_stats_to_dict([6.0, 3.0, 0.0, 24.0, 60.0, -2.0, 1.5, 0.0], T, B, A)
    assert got == {"traj_len": 2.4, "logit_mean": 0.5, "logit_max": 2.5, "entropy": 0.25, "entropy_target": 0.125, "actor_learner_kld": 0.0}
    nan = rnad_hip.log_stats_to_dict([6.0, float("nan"), 0.0, 24.0, 60.0, -2.0, 1.5, 0.0], T, B, A)
    assert nan["entropy_target"] != nan["entropy_target"] and nan["entropy"] == 0.25
