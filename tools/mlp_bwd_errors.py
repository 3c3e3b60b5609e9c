#!/usr/bin/env python
"""profiles/mlp_bwd_errors.json from the figures the MLP-backward sweeps log:
    RNAD_ERRORS_DIR=<dir> python -m pytest tests/test_mlp_bwd_shapes.py tests/test_hip_mlp_bwd_shapes.py
    python tools/mlp_bwd_errors.py <dir> [profiles/mlp_bwd_errors.json]
<dir> then holds mlp_bwd_errors_fp32_torch.json (plain fp32 torch on the CPU: what fixes G), mlp_bwd_errors.json (the kernels, if the run had
a GPU) and mlp_bwd_errors_lds.json (the LDS-transpose kernel, from the child process); they are merged under one key each, with the worst
entry of each beside them.  Every figure is the largest |got - want| of a case and tensor in units of 2^-24 B (tests/_mlpbwdref.py)."""
import json
import os
import sys

PARTS = (("fp32_torch", "mlp_bwd_errors_fp32_torch.json"), ("mi355x", "mlp_bwd_errors.json"), ("mi355x_lds_kernel", "mlp_bwd_errors_lds.json"))


def main(src, dst):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "tests"))
    from test_mlp_bwd_shapes import G

    out = {"_about": "largest |got - want| in units of 2^-24 B per case and tensor (B: the sum of the absolute terms of the entry, "
                     "tests/_mlpbwdref.py); the gate of tests/test_hip_mlp_bwd_shapes.py is G units, fixed in tests/test_mlp_bwd_shapes.py "
                     "from fp32_torch (at most G / 2)", "G": G}
    for key, name in PARTS:
        path = os.path.join(src, name)
        if not os.path.exists(path):
            continue
        part = json.load(open(path))
        out[key] = {c: {t: round(v, 4) for t, v in r.items()} for c, r in part.items()}
        units, case, tensor = max((v, c, t) for c, r in part.items() for t, v in r.items() if t != "rejected")
        out["worst_" + key] = dict(units=round(units, 4), case=case, tensor=tensor)
        print(key, len(part), "cases; worst", round(units, 3), case, tensor)
    assert "fp32_torch" in out, f"{src} holds no mlp_bwd_errors_fp32_torch.json"
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    root = os.path.join(os.path.dirname(os.path.realpath(__file__)), "..")
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "mlp_bwd_errors.json"))
