"""The C-ABI shared library builds, loads without a GPU and exports every symbol include/rnad_hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnad_hip.h")
SO = os.path.join(ROOT, "r-nad_amd", "csrc", "librnad_hip.so")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(rnad_[a-z_0-9]+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for must in ("rnad_tree_create", "rnad_observe", "rnad_sample", "rnad_transition", "rnad_rollout_begin", "rnad_rollout_step",
                 "rnad_process_policy", "rnad_vtrace", "rnad_loss_v", "rnad_loss_nerd", "rnad_learn_fused", "rnad_nashconv",
                 "rnad_tree_generate", "rnad_solve_matrix", "rnad_last_error"):
        assert must in names


def test_library_loads_and_exports_every_declared_symbol():
    assert os.path.exists(SO), "build it first: make -C r-nad_amd/csrc (or __graft_entry__.build())"
    lib = ctypes.CDLL(SO)
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} is declared in include/rnad_hip.h but not exported"
    assert lib.rnad_version() >= 1


def test_binding_takes_every_prototype_from_the_header():
    """rnad_hip.lib() sets restype AND argtypes of every declared function from include/rnad_hip.h, so a Python int handed to an
    int64_t / uint64_t parameter is converted at full width instead of silently travelling as a C int."""
    import rnad_hip

    lib = rnad_hip.lib()
    protos = rnad_hip.header_prototypes()
    assert sorted(protos) == declared_functions()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype == restype, name
    i64, u64, f32, ptr, i32 = ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    assert list(lib.rnad_sample.argtypes) == [i64, i32, ptr, ptr, u64, i64, i32, i32, ptr, ptr]
    assert list(lib.rnad_clip_grad_norm.argtypes) == [i64, ptr, f32, ptr, ptr]
    assert list(lib.rnad_mlp_backward_plan.argtypes) == [i64, i32, i32, i32, ptr] and lib.rnad_mlp_backward_plan.restype == i32
    assert list(lib.rnad_mlp_forward_plan.argtypes) == [i64, i32, i32, i32, i32, i32, ptr] and lib.rnad_mlp_forward_plan.restype == i32
    assert lib.rnad_tree_info.restype == i64 and lib.rnad_last_error.restype == ctypes.c_char_p and lib.rnad_tree_destroy.restype is None
    # full-width conversion of a bare Python int (no c_int64 wrapper at the call site)
    assert lib.rnad_compact_workspace(2**40) == 2**40 // 2048 + 1


def test_binding_fails_loudly_without_a_gpu_tensor():
    import pytest
    import torch

    import rnad_hip

    with pytest.raises(rnad_hip.RnadHipError, match="GPU"):
        rnad_hip.process_policy(torch.zeros(4, 3), torch.ones(4, 3), 32, 0.03)
    with pytest.raises(rnad_hip.RnadHipError):
        rnad_hip.TreeHandle(torch.zeros(2, 1, 2, 2, dtype=torch.int64), torch.zeros(2, 1, 2, 2), torch.zeros(2, 1, 2, 2),
                            torch.zeros(2, 1, 2, 2), torch.zeros(2, 1, 2, 2), "cpu")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "r-nad_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.lower() or f == "tree_gen.cpp" and "oracle" not in text, (dirpath, f)
