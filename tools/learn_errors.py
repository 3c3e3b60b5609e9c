#!/usr/bin/env python
"""profiles/learn_errors.json from the figures the learner sweeps log:
    RNAD_ERRORS_DIR=<dir> python -m pytest tests/test_learn_shapes.py tests/test_hip_learn_shapes.py
    python tools/learn_errors.py <dir> [profiles/learn_errors.json]
<dir> then holds learn_errors_cpu.json (two fp32 programs on the CPU, "numpy/<output>" and "oracle/<output>", in units of 2^-24 mag: what
fixes K per output family) and learn_errors.json (the kernels, if the run had a GPU, as shares of their gate K 2^-24 mag, the row tables
with the fixed-point term of their path); they are merged under one key each, with the worst entry per output beside them."""
import json
import os
import sys

PARTS = (("cpu", "learn_errors_cpu.json"), ("mi355x", "learn_errors.json"))


def main(src, dst):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "tests"))
    from _learnref import K

    out = {"_about": "cpu: largest |got - want| of two fp32 programs in units of 2^-24 mag per case and output (mag: the magnitude the fp64 "
                     "reference of tests/_learnref.py carries beside the value); K per output family is the smallest power of two that is at "
                     "least twice the worst of them.  mi355x: the largest share of the gate K 2^-24 mag (+ slots * half a fixed-point unit for "
                     "the row tables) a kernel uses, per case and output of tests/test_hip_learn_shapes.py", "K": K}
    for key, name in PARTS:
        path = os.path.join(src, name)
        if not os.path.exists(path):
            continue
        part = json.load(open(path))
        out[key] = {c: {t: round(v, 4) for t, v in r.items()} for c, r in part.items()}
        worst = {}
        for c, r in part.items():
            for t, v in r.items():
                if t not in worst or v > worst[t]["figure"]:
                    worst[t] = dict(figure=round(v, 4), case=c)
        out["worst_" + key] = worst
        print(key, len(part), "cases; worst per output:", {t: w["figure"] for t, w in sorted(worst.items())})
    assert "cpu" in out, f"{src} holds no learn_errors_cpu.json"
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    root = os.path.join(os.path.dirname(os.path.realpath(__file__)), "..")
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "learn_errors.json"))
