"""The joint gravity-magnetic store on the translation-invariant table against the scalar gz and tf tables of the same
geometry, and against the dense joint store, in one process:
    python profiles/lattice_joint_clocks.py [trajectories] [nodense]
Cells 100 x 100 x 50 of 100 m under the 100 x 100 cell centres.  The joint table's pass does the work of the gz table's
pass and the tf table's pass added -- the same kernel over the layers of both, each on its own observation block --
and no more: each joint pass is expected within 1.05 x the sum of the two scalar passes (this project's +-5 % for
single-run clocks, the margin lattice_mvi_clocks.py reads its ratios with).  Times are HIP events around the launches
of gh_forward / gh_adjoint (gather + pass), one call per reading, the median of 9 readings.  Then the chain's steps per
second through JointModule(translation_invariant=True) and through the dense JointModule of the same geometry (two
blocks of 40 GB: where one GPU holds them; `nodense` leaves it out), and the table alone at 200 x 200 x 60 cells under
200 x 200 stations, where no dense joint store can exist.  One JSON line per measurement; the bar is reported, met or
missed, with the measured values -- nothing is tuned to it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402
from gravinv3dhmc_amd import _lib, utils  # noqa: E402

trajectories = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 40
INC, DEC = 60.0, 25.0
F = tuple(float(v) for v in utils.dircos(INC, DEC))
H = 100.0


def aligned(nx, ny, nz):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * H, np.arange(ny + 1) * H, np.arange(nz + 1) * H
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * H, ye[:-1] + 0.5 * H, indexing="ij")]
    return (xp, yp, np.full(xp.size, -50.0)), np.ascontiguousarray(b6)


def passes(e, wm, N, M):
    """each table pass on its own, the median of 9 readings of one call each"""
    rng = np.random.default_rng(2)
    x, r = rng.uniform(-1, 1, M) * wm, rng.normal(size=N)
    out = {}
    for name, call in (("forward", lambda: e.forward(x)), ("adjoint", lambda: e.adjoint(r))):
        call()
        ms = []
        for _ in range(9):
            e.profile_enable(True)
            call()
            pr = e.profile_read()
            e.profile_enable(False)
            ms.append(pr["sweep_ms"] / max(pr["sweeps"], 1))
        out[name + "_ms"] = round(float(np.median(ms)), 4)
    return out


def scalar_table(obs, b6, field):
    n, m = obs[0].size, b6.shape[0]
    e = g.Engine(n, m)
    e.set_translation_invariant(True)
    e.set_obs(*obs)
    if field == "gz":
        e.set_cells(b6, _lib.CELL_PRISM)
    else:
        e.set_cells(b6, _lib.CELL_PRISM_TF, direction=F)
    e.build_G()
    wm = e.weight(0.5)
    p = passes(e, wm, n, m)
    bytes_ = e.translation_invariant_info()["table_bytes"]
    e.close()
    return p, bytes_


def joint_table(obs, b6):
    n, m = obs[0].size, b6.shape[0]
    e = g.Engine(2 * n, 2 * m)
    e.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=F, translation_invariant=True)
    e.set_obs(*obs)
    t0 = time.perf_counter()
    e.build_G()
    wm = e.weight(0.5)
    e.synchronize()
    t_build = time.perf_counter() - t0
    info = e.translation_invariant_info()
    p = passes(e, wm, 2 * n, 2 * m)
    e.close()
    return p, info, t_build


def compare(cells):
    obs, b6 = aligned(*cells)
    n, m = obs[0].size, b6.shape[0]
    gz, _ = scalar_table(obs, b6, "gz")
    tf, _ = scalar_table(obs, b6, "tf")
    jt, info, t_build = joint_table(obs, b6)
    print(json.dumps({"what": "scalar table passes", "cells": list(cells), "gz": gz, "tf": tf}), flush=True)
    print(json.dumps({"what": "joint table", "cells": list(cells), "points": n, "layers": 2 * info["nz"],
                      "chunks": info["chunks"], "layers_per_chunk": info["layers_per_chunk"],
                      "table_MB": round(info["table_bytes"] / 1e6, 2), "dense_GB": round(2 * 8.0 * n * m / 1e9, 1),
                      "max_dev": info["max_dev"], "build_and_weight_s": round(t_build, 3), "passes": jt}), flush=True)
    out = {"what": "joint pass / (gz pass + tf pass)", "cells": list(cells), "bar": 1.05}
    for k in ("forward", "adjoint"):
        out[k + "_ratio"] = round(jt[k + "_ms"] / (gz[k + "_ms"] + tf[k + "_ms"]), 3)
        out[k + "_bar_met"] = bool(out[k + "_ratio"] <= 1.05)
    print(json.dumps(out), flush=True)
    return obs, b6


def sample(mod, M):
    """Steps per second of the module's chain as HMCSample drives it (Engine.run_chain on the module's engine), over a
    FIXED number of trajectories of L = 10 leapfrog steps: HMCSample itself runs until a number of samples is accepted,
    which is no bounded amount of work on noise data"""
    e, L = mod._engine, 10
    wm = mod.Wm.diagonal()
    mod._use_reg("Damping", 1.0, 0.01, 0.01 * wm)
    e.chain_init(0.01 * wm, -1.0 * wm, 1.0 * wm)
    rng = np.random.default_rng(1)
    trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(trajectories + 1)]
    e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
    e.synchronize()
    t0 = time.perf_counter()
    e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
    e.synchronize()
    el = time.perf_counter() - t0
    steps = trajectories * L
    return {"trajectories": trajectories, "steps": steps, "seconds": round(el, 4), "steps_per_s": round(steps / el, 1),
            "ms_per_step": round(el / steps * 1e3, 4)}


def modules(cells, dense):
    nx, ny, nz = cells
    obs, _ = aligned(*cells)
    n = obs[0].size
    # (the module's mesh: mrange = (xmin, xmax, ymin, ymax, zmin, zmax), mspacing = (dz, dy, dx))
    mrange, mspacing = (0.0, nx * H, 0.0, ny * H, 0.0, nz * H), (H, H, H)
    rng = np.random.default_rng(0)
    dgz, dtf = rng.normal(size=n), 0.1 * rng.normal(size=n)
    for ti in ((True, False) if dense else (True,)):
        what = "chain on the joint table" if ti else "chain on the dense joint store"
        try:
            print(json.dumps({"what": what, "cells": list(cells), "state": "building the module"}), flush=True)
            t0 = time.perf_counter()
            mod = g.JointModule(dgz, dtf, mrange, mspacing, obs, mangle=(INC, DEC), verbose=False,
                                **(dict(translation_invariant=True) if ti else {}))
            t_make = time.perf_counter() - t0
            M = mod._engine.M
            print(json.dumps(dict({"what": what, "cells": list(cells), "module_s": round(t_make, 2)}, **sample(mod, M))), flush=True)
            mod._engine.close()
        except (MemoryError, RuntimeError, NotImplementedError) as err:
            print(json.dumps({"what": what, "not built": str(err)[:200]}), flush=True)


compare((100, 100, 50))
modules((100, 100, 50), "nodense" not in sys.argv[1:])
compare((200, 200, 60))
modules((200, 200, 60), False)
