#!/usr/bin/env python
"""profiles/mlp_fwd_errors.json from the figures the MLP-forward sweeps log:
    RNAD_ERRORS_DIR=<dir> python -m pytest tests/test_mlp_fwd_shapes.py tests/test_hip_mlp_fwd_shapes.py
    python tools/mlp_fwd_errors.py <dir> [profiles/mlp_fwd_errors.json]
<dir> then holds mlp_fwd_errors_fp32_torch.json (plain fp32 torch on the CPU: what fixes G) and mlp_fwd_errors.json (the kernel, if the run had
a GPU); they are merged under one key each, with the worst entry of each beside them.  Every figure is the largest |got - want| of a case and
output in units of 2^-24 B (tests/_mlpfwdref.py); a GPU case's figure covers every launch of the case (heads, nets, row lists)."""
import json
import os
import sys

PARTS = (("fp32_torch", "mlp_fwd_errors_fp32_torch.json"), ("mi355x", "mlp_fwd_errors.json"))


def main(src, dst):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "tests"))
    from test_mlp_fwd_shapes import G

    out = {"_about": "largest |got - want| in units of 2^-24 B per case and output (B: the sum of the absolute terms of the output, "
                     "tests/_rowsref.py); the gate of tests/test_hip_mlp_fwd_shapes.py is G units, fixed in tests/test_mlp_fwd_shapes.py "
                     "from fp32_torch (at most G / 2)", "G": G}
    for key, name in PARTS:
        path = os.path.join(src, name)
        if not os.path.exists(path):
            continue
        part = json.load(open(path))
        out[key] = {c: {t: round(v, 4) for t, v in r.items()} for c, r in part.items()}
        units, case, output = max((v, c, t) for c, r in part.items() for t, v in r.items())
        out["worst_" + key] = dict(units=round(units, 4), case=case, output=output)
        print(key, len(part), "cases; worst", round(units, 3), case, output)
    assert "fp32_torch" in out, f"{src} holds no mlp_fwd_errors_fp32_torch.json"
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    root = os.path.join(os.path.dirname(os.path.realpath(__file__)), "..")
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "mlp_fwd_errors.json"))
