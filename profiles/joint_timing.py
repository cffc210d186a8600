"""Timing of the joint gravity-magnetic store (GH_CELL_PRISM_JOINT) on one MI355X, for DESIGN §4.15.

    python profiles/joint_timing.py [--out FILE]          # every step, each in its own child process
    python profiles/joint_timing.py --step NAME           # one step
    python profiles/joint_timing.py --step joint --crossgrad 1.0   # the joint chains with the cross-gradient coupling on

Steps (C2's geometry: 100 x 100 observations over [0, 5000]^2 at z = -1; C2's mesh is 100 x 100 x 50 prisms):
  assembly  build_G of a joint store over 100 x 100 x 25 prisms (2.5*10^9 pairs, both fields), of a gz and of a
            tf context over the same prisms: joint against gz + tf
  joint     fused leapfrog steps of one chain on the joint store of 100 x 100 x 25 prisms (H: 10^4 x 5*10^5,
            40 GB, C2's bytes): ms per sweep and TB/s
  gz        the same on C2's gz store (10^4 x 5*10^5), and a plain read of it
  small     C1's observations (600, one-wave teams, the two-stage epilogue): fused steps of the joint store of
            20 x 30 x 10 prisms (600 x 12 000) against a gz store of the same bytes (20 x 30 x 20 prisms)
Every child runs under `timeout -k 10 <s>`; the driver stops at the first child that fails.  One JSON line per
measurement (also written to --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"assembly": 900, "joint": 900, "gz": 900, "small": 300}


def geometry(nz):
    from gravinv3dhmc_amd import mesher
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        mesh = mesher.PrismMesh((0, 5000, 0, 5000, 0, 50.0 * nz), (50, 50, 50))
    x, y = [a.ravel() for a in np.meshgrid(np.linspace(0, 5000, 100), np.linspace(0, 5000, 100))]
    return mesh.cell_bounds(), (x, y, np.full_like(x, -1.0))


def engine(kind, bounds, obs):
    from gravinv3dhmc_amd import _lib, utils
    from gravinv3dhmc_amd.engine import Engine
    n, m = obs[0].size, bounds.shape[0]
    d = utils.dircos(60.0, -10.0)
    if kind == "joint":
        eng = Engine(2 * n, 2 * m)
        eng.set_cells(bounds, _lib.CELL_PRISM_JOINT, direction=d)
        eng.set_obs(*obs)
    else:
        eng = Engine(n, m)
        eng.set_obs(*obs)
        if kind == "tf":
            eng.set_cells(bounds, _lib.CELL_PRISM_TF, direction=d)
        else:
            eng.set_cells(bounds, _lib.CELL_PRISM)
    return eng


def timed_build(eng):
    eng.synchronize()
    t = time.perf_counter()
    eng.build_G()
    eng.synchronize()
    return time.perf_counter() - t


def step_assembly(emit):
    bounds, obs = geometry(25)
    out = {"step": "assembly", "obs": obs[0].size, "cells": bounds.shape[0]}
    for kind in ("gz", "tf", "joint"):
        eng = engine(kind, bounds, obs)
        out[kind + "_s"] = timed_build(eng)
        eng.close()
    out["joint_over_sum"] = out["joint_s"] / (out["gz_s"] + out["tf_s"])
    emit(out)


CROSSGRAD = 0.0   # --crossgrad: lambda of the cross-gradient coupling on the joint stores (0: off)


def chain_steps(eng, label, emit, L=20, traj=6, shape=None):
    M = eng.M
    wm = eng.weight(0.5)
    if shape is not None and CROSSGRAD > 0:
        # (unit spacings, normalisers that bring the physical models to O(1))
        m = M // 2
        eng.set_cross_gradient(CROSSGRAD, shape, 1.0, 1.0, np.ones(shape[0] - 1),
                               (1e-3 / np.median(wm[:m]), 1e-3 / np.median(wm[m:])))
        label += "_crossgrad"
    rng = np.random.default_rng(0)
    eng.set_data(rng.normal(size=eng.N))
    eng.set_reg("Damping", 1.0, 0.01, None, np.zeros(M))
    eng.chain_init(0.001 * wm, np.zeros(M), wm)
    eng.chain_trajectory(rng.normal(size=M) * 1e-3, 1e-3, 4, 0.5)   # warm-up
    eng.profile_enable(True)
    eng.synchronize()
    t = time.perf_counter()
    for _ in range(traj):
        eng.chain_trajectory(rng.normal(size=M) * 1e-3, 1e-3, L, 0.5)
    eng.synchronize()
    wall = time.perf_counter() - t
    p = eng.profile_read()
    eng.profile_enable(False)
    steps = traj * (L + 1)
    # (profile_read: the time of the timed sweeps together, and how many there were)
    ms = p["sweep_ms"] / p["sweeps"] if p["sweeps"] else None
    emit({"step": label, "N": eng.N, "M": eng.M, "ms_per_sweep": ms, "bytes_per_sweep": p["bytes_per_sweep"],
          "TBps": p["bytes_per_sweep"] / (ms * 1e-3) / 1e12 if ms else None,
          "wall_ms_per_step": 1e3 * wall / steps, "steps_per_s": steps / wall})


def step_joint(emit):
    bounds, obs = geometry(25)
    eng = engine("joint", bounds, obs)
    eng.build_G()
    chain_steps(eng, "joint", emit, shape=(25, 100, 100))
    eng.close()


def step_gz(emit):
    bounds, obs = geometry(50)
    eng = engine("gz", bounds, obs)
    eng.build_G()
    emit({"step": "plain_read", "GBps": eng.stream_read_gbps(True, 3), "bytes": eng.N * eng.M * 8})
    chain_steps(eng, "gz", emit)
    eng.close()


def step_small(emit):
    import contextlib
    import io
    from gravinv3dhmc_amd import mesher
    x, y = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    obs = (y, x, np.zeros_like(x))
    for kind, depth in (("joint", 1000), ("gz", 2000)):
        with contextlib.redirect_stdout(io.StringIO()):
            bounds = mesher.PrismMesh((0, 2000, 0, 3000, 0, depth), (100, 100, 100)).cell_bounds()
        eng = engine(kind, bounds, obs)
        eng.build_G()
        if kind == "joint":
            emit({"step": "small_layout", **eng.joint_layout()})
        chain_steps(eng, "small_" + kind, emit, L=20, traj=20, shape=(10, 30, 20) if kind == "joint" else None)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--crossgrad", type=float, default=0.0, help="lambda of the cross-gradient coupling (joint stores)")
    args = ap.parse_args()
    global CROSSGRAD
    CROSSGRAD = args.crossgrad

    def emit(d):
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    if args.step:
        {"assembly": step_assembly, "joint": step_joint, "gz": step_gz, "small": step_small}[args.step](emit)
        return 0
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name]
        if args.out:
            cmd += ["--out", args.out]
        if args.crossgrad:
            cmd += ["--crossgrad", str(args.crossgrad)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
