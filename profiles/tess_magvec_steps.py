"""Leapfrog steps per second of the tesseroid magnetization store on the shift-invariant table, on one MI355X, for
DESIGN §4.17c.

    python profiles/tess_magvec_steps.py [--what gz,tensor,magvec] [--out FILE] [--rounds R] [--height H]

On C4's global geometry (3 degree grid: 120 x 60 x 10 tesseroids, 121 x 61 observation points; --height, default
250 km -- satellite height; the table's size and a step's cost do not depend on it) and on the streamed harmonic form
(GRAVHMC_LONSYM_WIDE=2, GRAVHMC_LONSYM_RESIDENT=0 set here, before the library loads):

    gz      GravMagModule(coordinate="spherical", shift_invariant=True): 61 classes, 600 cell rows -- the baseline
    tensor  TesseroidMultiComponentModule(components=("gxx", "gyy", "gzz"), shift_invariant=True): 183 classes, 600 rows
    magvec  TesseroidMagVectorModule(data=("bx", "by", "bz"), shift_invariant=True): 183 classes, 1800 rows (the three
            axis blocks of the columns) -- three times the table of `tensor`, three times the bytes per step

Each engine runs R rounds (default 7) of 8 trajectories of 200 leapfrog steps, the engines alternating inside a round;
a round gives wall milliseconds per step (host clock around work that ends in a device synchronise).  Reported per
engine: the rounds, their median as steps/s, the spread (max - min), and the ratios to gz and to tensor.  One JSON
line per measurement (also appended to --out).  gz and tensor run code this store did not change: on a tree without
the table of the magnetization store they are measured alone."""
import argparse
import json
import os
import sys
import time

os.environ["GRAVHMC_LONSYM_WIDE"] = "2"
os.environ["GRAVHMC_LONSYM_RESIDENT"] = "0"

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MRANGE, MSPACING = (-180, 180, -90, 90, 0, -3000000), (-300000, 3, 3)


def prepare(model, rng):
    eng = model._engine
    M = eng.M
    wm = model.Wm.diagonal()
    eng.set_reg("Damping", 0.05, 0.01, None, np.zeros(M))
    eng.chain_init(0.001 * wm, np.zeros(M), 0.8 * wm)
    eng.chain_trajectory(rng.normal(size=M) * 1e-3, 5e-3, 8, 0.5)   # warm-up
    eng.synchronize()


def one_round(model, rng, L=200, traj=8):
    eng = model._engine
    p0 = [rng.normal(size=eng.M) * 1e-3 for _ in range(traj)]
    eng.synchronize()
    t = time.perf_counter()
    for p in p0:
        eng.chain_trajectory(p, 5e-3, L, 0.5)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t) / (traj * (L + 1))


def has_table(g):
    return getattr(getattr(g, "TesseroidMagVectorModule", None), "_has_table", False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="gz,tensor,magvec")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--height", type=float, default=250000.0)
    args = ap.parse_args()

    def emit(d):
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    import gravinv3dhmc_amd as g
    rng = np.random.default_rng(0)
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 181, 3.0), np.arange(-90, 91, 3.0), indexing="ij")]
    obs = (lon, lat, np.full_like(lon, args.height))
    n = lon.size
    models = {}
    for what in args.what.split(","):
        if what == "magvec" and not has_table(g):
            continue
        t = time.perf_counter()
        if what == "gz":
            m = g.GravMagModule(rng.normal(size=n), MRANGE, MSPACING, obs, coordinate="spherical", verbose=False,
                                shift_invariant=True)
        elif what == "tensor":
            c = ("gxx", "gyy", "gzz")
            m = g.TesseroidMultiComponentModule([rng.normal(size=n) for _ in c], MRANGE, MSPACING, obs, components=c,
                                                weights=(1.0, 1.0, 1.0), shift_invariant=True, verbose=False)
        else:
            c = ("bx", "by", "bz")
            m = g.TesseroidMagVectorModule([rng.normal(size=n) for _ in c], MRANGE, MSPACING, obs, data=c,
                                           weights=(1.0, 1.0, 1.0), shift_invariant=True, verbose=False)
        eng = m._engine
        emit({"step": "build_" + what, "rows": eng.N, "unknowns": eng.M, "s": time.perf_counter() - t,
              **eng.shift_invariant_info(), **eng.shift_invariant_harmonic()})
        prepare(m, rng)
        models[what] = m
    ms = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            ms[k].append(one_round(m, rng))
    for k, v in ms.items():
        med = float(np.median(v))
        emit({"step": "leapfrog_steps", "what": k, "ms_per_step": v, "median_ms": med, "steps_per_s": 1e3 / med,
              "spread_ms": max(v) - min(v)})
    for base in ("gz", "tensor"):
        if base in ms:
            b = float(np.median(ms[base]))
            emit({"step": "ratio_to_" + base, **{k: float(np.median(v)) / b for k, v in ms.items()}})
    return 0


if __name__ == "__main__":
    sys.exit(main())
