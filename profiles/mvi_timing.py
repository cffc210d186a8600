"""Assembly time of the magnetization-vector store (GH_CELL_PRISM_MVI) on one MI355X, for DESIGN §4.18.

    python profiles/mvi_timing.py [--out FILE] [--rounds R] [--window SECONDS]

In ONE process, at two sizes -- C1's geometry (600 observations x 20x30x10 prisms: 600 x 18000) and the largest the
GPU tests use (6300 observations x 6x12x10 prisms: 6300 x 2160) -- one GH_CELL_PRISM_MVI context (one launch of
prism_mvi_kernel for the three blocks) against THREE GH_CELL_PRISM_TF contexts of the same geometry (three launches of
prism_kernel<PRISM_TF>, a kernel this store leaves untouched).  gh_build_G ends in a stream synchronise, so a host
clock around it times the launch(es) to completion.  After a warm-up build of every context, R rounds (default 9)
alternate the two forms, each round repeating its builds `reps` times so that a timed window of the one-launch form is
about a second (--window) and that of the three launches as many times longer as they take; reported per size:
the medians in milliseconds per assembly, the spread (max - min) of each, and the ratio.
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

MANGLE = (50.0, 30.0)
SIZES = {"C1": ((0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (20, 30)),
         "tests_largest": ((0, 2000, 0, 3000, 0, 900), (150, 250, 200), (90, 70))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()

    def emit(d):
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib, utils
    f = utils.dircos(*MANGLE)
    for name, (mrange, mspacing, (nx, ny)) in SIZES.items():
        cells = g.mesher.PrismMesh(mrange, mspacing).cell_bounds()
        yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, mrange[3], ny), np.linspace(0, mrange[1], nx))]
        zp = np.full(xp.size, -1.0)
        n, m = xp.size, cells.shape[0]
        mvi = g.Engine(n, 3 * m)
        mvi.set_cells_mvi(cells, f)
        mvi.set_obs(xp, yp, zp)
        tfs = []
        for _ in range(3):
            e = g.Engine(n, m)
            e.set_obs(xp, yp, zp)
            e.set_cells(cells, _lib.CELL_PRISM_TF, direction=f)
            tfs.append(e)
        for e in [mvi] + tfs:          # warm-up: allocation, code objects
            e.build_G()
            e.build_G()
        t = time.perf_counter()
        mvi.build_G()
        reps = int(max(1, min(20000, args.window / max(time.perf_counter() - t, 1e-6))))
        ms = {"mvi": [], "tf3": []}
        for _ in range(args.rounds):
            t = time.perf_counter()
            for _ in range(reps):
                for e in tfs:
                    e.build_G()
            ms["tf3"].append(1e3 * (time.perf_counter() - t) / reps)
            t = time.perf_counter()
            for _ in range(reps):
                mvi.build_G()
            ms["mvi"].append(1e3 * (time.perf_counter() - t) / reps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        emit({"step": "assembly", "size": name, "N": n, "cells": m, "M": 3 * m, "reps": reps, "rounds": args.rounds,
              "window_s_mvi": 1e-3 * med["mvi"] * reps, "window_s_tf3": 1e-3 * med["tf3"] * reps,
              "ms_mvi_one_launch": med["mvi"], "ms_three_tf_launches": med["tf3"],
              "spread_mvi": max(ms["mvi"]) - min(ms["mvi"]), "spread_tf3": max(ms["tf3"]) - min(ms["tf3"]),
              "ratio": med["mvi"] / med["tf3"], "not_slower": bool(med["mvi"] <= med["tf3"])})
        for e in [mvi] + tfs:
            e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
