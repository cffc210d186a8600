"""The magnetization-vector store on the translation-invariant table against the single-block tf table of the same
geometry, in one process:
    python profiles/lattice_mvi_clocks.py [steps] [dense]
Cells 100 x 100 x 50 of 100 m under the 100 x 100 cell centres.  The yardstick is the scalar total-field table
(gh_set_cells_tf with gh_set_translation_invariant(1)): the vector store's passes are the same kernel over axes x nb
times the layers, so a pass is expected within 3 nb times the yardstick's (read with this project's +-5 % for single-run
clocks: ratio <= 1.05 x 3 nb).  For data=("tf",) (nb = 1) and data=("bx", "by", "bz") (nb = 3): the time of each table
pass (HIP events around the launches of gh_forward / gh_adjoint: gather + pass, lattice_clocks.py's method), the ratios,
and the steps per second of a chain.  With `dense`: the chain on the dense store of the first form too (120 GB: where
one GPU holds it).  One JSON line per measurement; nothing is asserted."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402
from gravinv3dhmc_amd import utils  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
L = 10
NX, NY, NZ = 100, 100, 50
F = tuple(float(v) for v in utils.dircos(60.0, 25.0))


def aligned(nx, ny, nz, h=100.0):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * h, np.arange(ny + 1) * h, np.arange(nz + 1) * h
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * h, ye[:-1] + 0.5 * h, indexing="ij")]
    return (xp, yp, np.full(xp.size, -50.0)), np.ascontiguousarray(b6)


def passes(e, wm, N, M):
    """each table pass on its own: the launches of gh_forward (gather x + forward) and gh_adjoint (gather r + adjoint)"""
    rng = np.random.default_rng(2)
    x, r = rng.uniform(-1, 1, M) * wm, rng.normal(size=N)
    out = {}
    for name, call in (("forward", lambda: e.forward(x)), ("adjoint", lambda: e.adjoint(r))):
        call()
        e.profile_enable(True)
        for _ in range(20):
            call()
        pr = e.profile_read()
        e.profile_enable(False)
        out[name + "_ms"] = round(pr["sweep_ms"] / max(pr["sweeps"], 1), 4)
    flops = 2.0 * N * M
    out["forward_tflops"] = round(flops / (out["forward_ms"] * 1e-3) / 1e12, 2)
    out["adjoint_tflops"] = round(flops / (out["adjoint_ms"] * 1e-3) / 1e12, 2)
    return out


def chain(e, wm, M, dobsw):
    e.set_data(dobsw)
    e.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.01 * wm)
    e.chain_init(0.01 * wm, -1.0 * wm, 1.0 * wm)
    rng = np.random.default_rng(1)
    trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(steps // L + 1)]
    e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
    e.synchronize()
    t0 = time.perf_counter()
    e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
    e.synchronize()
    el = time.perf_counter() - t0
    return {"steps": steps, "seconds": round(el, 4), "steps_per_s": round(steps / el, 1), "ms_per_step": round(el / steps * 1e3, 4)}


def data_of(e, wm, N, m):
    truth = np.zeros((3, NZ, NX, NY))
    truth[:, NZ // 5:NZ // 2, NX // 3:NX // 2, NY // 3:NY // 2] = np.array((0.6, -0.9, 0.4))[:, None, None, None]
    d = e.forward(wm * truth.ravel())
    return d + 0.01 * np.abs(d).max() * np.random.default_rng(0).normal(size=N)


obs, b6 = aligned(NX, NY, NZ)
n, m = obs[0].size, b6.shape[0]

# the yardstick: the scalar tf table of the same geometry
e = g.Engine(n, m)
e.set_translation_invariant(True)
e.set_obs(*obs)
e.set_cells(b6, 2, direction=F)
e.build_G()
wm = e.weight(0.5)
yard = passes(e, wm, n, m)
print(json.dumps(dict({"what": "yardstick: single-block tf table passes", "cells": [NX, NY, NZ]}, **yard)), flush=True)
e.close()

for data in (("tf",), ("bx", "by", "bz")):
    nb = len(data)
    e = g.Engine(nb * n, 3 * m)
    e.set_cells_mvi_data(b6, F if "tf" in data else None, data, np.ones(nb), translation_invariant=True)
    e.set_obs(*obs)
    t0 = time.perf_counter()
    e.build_G()
    wm = e.weight(0.5)
    e.synchronize()
    t_build = time.perf_counter() - t0
    info = e.translation_invariant_info()
    print(json.dumps({"what": "magnetization-vector tables", "data": list(data), "rows": nb * n, "M": 3 * m,
                      "layers": 3 * info["nz"], "chunks": info["chunks"], "layers_per_chunk": info["layers_per_chunk"],
                      "table_MB": round(info["table_bytes"] / 1e6, 2), "dense_GB": round(8.0 * nb * n * 3 * m / 1e9, 1),
                      "max_dev": info["max_dev"], "build_and_weight_s": round(t_build, 3)}), flush=True)
    p = passes(e, wm, nb * n, 3 * m)
    print(json.dumps(dict({"what": "magnetization-vector table passes", "data": list(data)}, **p)), flush=True)
    print(json.dumps({"what": "pass / yardstick", "data": list(data), "expected_at_most": round(1.05 * 3 * nb, 2),
                      "forward_ratio": round(p["forward_ms"] / yard["forward_ms"], 3),
                      "adjoint_ratio": round(p["adjoint_ms"] / yard["adjoint_ms"], 3)}), flush=True)
    print(json.dumps(dict({"what": "magnetization-vector table chain", "data": list(data)},
                          **chain(e, wm, 3 * m, data_of(e, wm, nb * n, m)))), flush=True)
    e.close()

if "dense" in sys.argv[2:]:
    # the dense store of the first form: 100 x 100 rows of 3 x 500 000 columns, 120 GB
    try:
        e = g.Engine(n, 3 * m)
        e.set_cells_mvi(b6, F)
        e.set_obs(*obs)
        e.build_G()
        wm = e.weight(0.5)
        print(json.dumps(dict({"what": "dense magnetization-vector chain", "data": ["tf"]},
                              **chain(e, wm, 3 * m, data_of(e, wm, n, m)))), flush=True)
        e.close()
    except (MemoryError, RuntimeError, NotImplementedError) as err:
        print(json.dumps({"what": "dense magnetization-vector store", "not built": str(err)[:200]}), flush=True)
