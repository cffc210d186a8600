"""Assembly time of the vector-data magnetization store (GH_CELL_PRISM_MVI_DATA) on one MI355X, for DESIGN §4.18b.

    python profiles/mvi_vecdata_timing.py [--out FILE] [--rounds R] [--window SECONDS]

In ONE process, at two sizes -- C1's geometry (600 observations x 20x30x10 prisms) and the largest the magnetization-
vector GPU tests use (6300 observations x 6x12x10 prisms) -- one GH_CELL_PRISM_MVI context (prism_mvi_kernel: the three
tf blocks, N rows) against one GH_CELL_PRISM_MVI_DATA context of the same mesh and points with data = (bx, by, bz)
(prism_mvi_data_kernel: nine blocks, 3 N rows).  gh_build_G ends in a stream synchronise, so a host clock around it
times the launch to completion.  After a warm-up build of both contexts, R rounds (default 9) alternate the two, each
round repeating its builds `reps` times so that a timed window of the MVI form is about a second (--window); reported
per size: the medians in milliseconds per assembly, the spread (max - min) of each, and the ratio.
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
    from gravinv3dhmc_amd import utils
    f = utils.dircos(*MANGLE)
    for name, (mrange, mspacing, (nx, ny)) in SIZES.items():
        cells = g.mesher.PrismMesh(mrange, mspacing).cell_bounds()
        yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, mrange[3], ny), np.linspace(0, mrange[1], nx))]
        zp = np.full(xp.size, -1.0)
        n, m = xp.size, cells.shape[0]
        mvi = g.Engine(n, 3 * m)
        mvi.set_cells_mvi(cells, f)
        mvi.set_obs(xp, yp, zp)
        vec = g.Engine(3 * n, 3 * m)
        vec.set_cells_mvi_data(cells, None, ("bx", "by", "bz"), (1.0, 1.0, 1.0))
        vec.set_obs(xp, yp, zp)
        for e in (mvi, vec):           # warm-up: allocation, code objects
            e.build_G()
            e.build_G()
        t = time.perf_counter()
        mvi.build_G()
        reps = int(max(1, min(20000, args.window / max(time.perf_counter() - t, 1e-6))))
        ms = {"mvi": [], "vec": []}
        for _ in range(args.rounds):
            for key, e in (("vec", vec), ("mvi", mvi)):
                t = time.perf_counter()
                for _ in range(reps):
                    e.build_G()
                ms[key].append(1e3 * (time.perf_counter() - t) / reps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        emit({"step": "assembly", "size": name, "N": n, "cells": m, "M": 3 * m, "rows_vec": 3 * n, "reps": reps,
              "rounds": args.rounds, "ms_mvi_tf_store": med["mvi"], "ms_bx_by_bz_store": med["vec"],
              "spread_mvi": max(ms["mvi"]) - min(ms["mvi"]), "spread_vec": max(ms["vec"]) - min(ms["vec"]),
              "ratio": med["vec"] / med["mvi"]})
        for e in (mvi, vec):
            e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
