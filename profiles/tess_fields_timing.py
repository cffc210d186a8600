"""Timing of the tesseroid gravity fields (GH_CELL_TESSEROID_COMP) on one MI355X, for DESIGN §4.14.

    python profiles/tess_fields_timing.py [--fields gz,gzz,...] [--out FILE]

1. build_G per field on C4's geometry (bench.py's c4_global_tesseroid: 7381 observations at h = 5 km over
   72 000 tesseroids of 3 x 3 degrees x 300 km), each field at its default ratio, against gz; the leaves
   per entry from kernel_stats().
2. tesseroid.gzz(..., return_kernel=False) on the same mesh with the observations at h = 250 km: the
   matrix-free forward, never storing G (build, which includes the statistics pass, and one forward).
Prints one JSON line per measurement (and writes them to --out).
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

FIELDS = ("gz", "potential", "geoid", "gx", "gy", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
RATIO = {"potential": 1, "geoid": 1, "gx": 1.6, "gy": 1.6, "gz": 1.6}


def c4_geometry(h):
    from gravinv3dhmc_amd import mesher
    mesh = mesher.TesseroidMesh((-180, 180, -90, 90, 0, -3000000), (-300000, 3, 3))
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 181, 3.0), np.arange(-90, 91, 3.0), indexing="ij")]
    return mesh, lon, lat, np.full_like(lon, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default=",".join(FIELDS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.engine import Engine
    from gravinv3dhmc_amd.gravmag import tesseroid
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    mesh, lon, lat, h = c4_geometry(5000.0)
    b = mesh.cell_bounds()
    N, M = lon.size, b.shape[0]
    for f in args.fields.split(","):
        eng = Engine(N, M)
        eng.set_obs(lon, lat, h)
        eng.set_cells(b, _lib.CELL_TESSEROID, RATIO.get(f, 8), component=None if f == "gz" else f)
        eng.synchronize()
        t = time.perf_counter()
        eng.build_G()
        eng.synchronize()
        dt = time.perf_counter() - t
        st = eng.kernel_stats()
        eng.close()
        emit({"what": "build_G", "field": f, "ratio": RATIO.get(f, 8), "N": N, "M": M, "seconds": round(dt, 4),
              "leaves_per_entry": round(st["leaves"] / float(N * M), 3), "warn_cells": st["warn_cells"]})
    mesh, lon, lat, h = c4_geometry(250000.0)
    mesh.addprop("density", np.linspace(0.1, 0.5, mesh.size))
    t = time.perf_counter()
    res, _ = tesseroid.gzz(lon, lat, h, mesh, return_kernel=False)
    dt = time.perf_counter() - t
    emit({"what": "gzz_return_kernel_false", "h": 250000.0, "N": lon.size, "M": mesh.size, "seconds": round(dt, 4),
          "max_abs_eotvos": float(np.abs(res).max())})
    if args.out:
        with open(args.out, "w") as fo:
            for d in lines:
                fo.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
