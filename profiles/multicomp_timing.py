"""Cost of a leapfrog step on the multi-component store (GH_CELL_PRISM_MULTI) on one MI355X, for DESIGN §4.17.

    python profiles/multicomp_timing.py [--out FILE] [--rounds R]

In ONE process, on C2's mesh (100 x 100 x 50 prisms): a 3-component module (gz, gzz, gxx) with N = 3000 stations,
and GravMagModule(component="gzz") with 9000 stations -- the same store size (9000 x 5*10^5, 36 GB), the same
sweep kernel.  Each engine runs R rounds (default 5) of 4 trajectories of 20 fused leapfrog steps, the two engines
alternating; a round gives wall milliseconds per step.  Reported: the median of each, the run-to-run spread of the
single-component engine (max - min over its rounds) and the multi-component store's deficit against it.  The
expectation is equality apart from the epilogue (one more launch: the slab rows' sums per row block).
One JSON line per measurement (also appended to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MRANGE, MSPACING = (0, 5000, 0, 5000, 0, 2500), (50, 50, 50)


def stations(nx, ny):
    x, y = [a.ravel() for a in np.meshgrid(np.linspace(0, 5000, nx), np.linspace(0, 5000, ny))]
    return x, y, np.full_like(x, -1.0)


def prepare(model, rng):
    eng = model._engine
    M = eng.M
    wm = model.Wm.diagonal()
    eng.set_reg("Damping", 1.0, 0.01, None, np.zeros(M))
    eng.chain_init(0.001 * wm, np.zeros(M), wm)
    eng.chain_trajectory(rng.normal(size=M) * 1e-3, 1e-3, 4, 0.5)   # warm-up
    eng.synchronize()


def one_round(model, rng, L=20, traj=4):
    eng = model._engine
    p0 = [rng.normal(size=eng.M) * 1e-3 for _ in range(traj)]
    eng.synchronize()
    t = time.perf_counter()
    for p in p0:
        eng.chain_trajectory(p, 1e-3, L, 0.5)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t) / (traj * (L + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    def emit(d):
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    import gravinv3dhmc_amd as g
    rng = np.random.default_rng(0)
    obs3, obs9 = stations(60, 50), stations(100, 90)
    t = time.perf_counter()
    multi = g.MultiComponentModule([rng.normal(size=3000) for _ in range(3)], MRANGE, MSPACING, obs3,
                                   components=("gz", "gzz", "gxx"), weights=(1.0, 0.02, 0.03), verbose=False)
    emit({"step": "build_multi", "rows": multi._engine.N, "cells": multi._engine.M, "s": time.perf_counter() - t,
          **multi._engine.sweep_layout()})
    t = time.perf_counter()
    single = g.GravMagModule(rng.normal(size=9000), MRANGE, MSPACING, obs9, component="gzz", verbose=False)
    emit({"step": "build_single", "rows": single._engine.N, "cells": single._engine.M, "s": time.perf_counter() - t,
          **single._engine.sweep_layout()})
    prepare(multi, rng)
    prepare(single, rng)
    ms = {"multi": [], "single": []}
    for _ in range(args.rounds):
        ms["single"].append(one_round(single, rng))
        ms["multi"].append(one_round(multi, rng))
    spread = max(ms["single"]) - min(ms["single"])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    emit({"step": "leapfrog_step", "ms_per_step_multi": ms["multi"], "ms_per_step_single": ms["single"],
          "median_multi": med["multi"], "median_single": med["single"], "spread_single": spread,
          "deficit_ms": med["multi"] - med["single"], "allowed_ms": 2 * spread,
          "within": bool(med["multi"] - med["single"] <= 2 * spread)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
