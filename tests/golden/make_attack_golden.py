#!/usr/bin/env python
"""Fixtures of the membership-inference estimator: `python tests/golden/make_attack_golden.py REFERENCE_DIR`.

Takes `attack` and `_get_random_subset` from REFERENCE_DIR/mem_inf_attack.py at run time — the file imports packages that are not
installed (coloredlogs, torchvision, sklearn, pytorch_fid), so it is parsed with `ast`, the two function definitions alone are kept and
executed in a namespace holding `np` and `List`; nothing of them is stored — and records what the REFERENCE estimator returns under
`np.random.seed(seed)` for 2000 trials on two small score sets:

  attack_smooth.npz   N = 600 train scores ~ N(0.5, 1), M = 1500 non-train scores ~ N(0, 1): train shifted by half a sigma
  attack_ties.npz     the same scores rounded to the integers of [-2, 2]: five levels, so the tie rule decides many ranks

Each file holds vt, vn (float32), seed, and rates (float64[2000], the reference's per-trial success rates at data_prop 0.1).
tests/test_mem_inf_attack.py compares the host model's mean with the mean of `rates` (two independent Monte-Carlo estimates).
"""
import ast
import os
import sys
from typing import List

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRIALS = 2000
CASES = {"attack_smooth": 20240611, "attack_ties": 20240612}          # np.random.seed of the reference's run


def reference_functions(ref_dir):
    path = os.path.join(ref_dir, "mem_inf_attack.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("attack", "_get_random_subset")]
    assert len(tree.body) == 2, [n.name for n in tree.body]
    ns = {"np": np, "List": List}
    exec(compile(tree, path, "exec"), ns)
    return ns["attack"]


def scores():
    rng = np.random.default_rng(600 + 1500)
    vt = (rng.standard_normal(600) + 0.5).astype(np.float32)
    vn = rng.standard_normal(1500).astype(np.float32)
    return vt, vn


def main(ref_dir):
    attack = reference_functions(ref_dir)
    vt, vn = scores()
    for name, seed in CASES.items():
        a, b = (vt, vn) if name == "attack_smooth" else (np.clip(np.rint(vt), -2, 2).astype(np.float32), np.clip(np.rint(vn), -2, 2).astype(np.float32))
        np.random.seed(seed)
        la, lb = a.tolist(), b.tolist()
        rates = np.array([attack(la, lb, 0.1) for _ in range(TRIALS)], dtype=np.float64)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, vt=a, vn=b, seed=np.int64(seed), rates=rates)
        print("%s: mean %.5f  std %.5f  %d bytes" % (name, rates.mean(), rates.std(ddof=1), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1])
