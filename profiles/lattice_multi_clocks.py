"""The multi-component store on the translation-invariant table against the single-component table engines of its
fields, in one process:
    python profiles/lattice_multi_clocks.py [steps]
Cells 100 x 100 x 50 of 100 m under the 100 x 100 cell centres with gz, gzz, gxx, gyy, gxz, gyz (60 000 stacked rows),
then 200 x 200 x 60 under 200 x 200 with gz, gzz.  The time of each table pass (HIP events around the launches of
gh_forward / gh_adjoint: gather + pass, lattice_clocks.py's method) of the block-aware context and of every
single-component context -- the code path without the blocks --, their sums, and the steps per second of a chain on
the block-aware context.  One JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
L = 10


def aligned(nx, ny, nz, h=100.0):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * h, np.arange(ny + 1) * h, np.arange(nz + 1) * h
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * h, ye[:-1] + 0.5 * h, indexing="ij")]
    return (xp, yp, np.zeros_like(xp)), np.ascontiguousarray(b6)


def passes(e, wm, N, M):
    """each table pass on its own: the launches of gh_forward (gather x + forward) and gh_adjoint (gather r + adjoint)"""
    rng = np.random.default_rng(2)
    x, r = rng.uniform(0, 0.05, M) * wm, rng.normal(size=N)
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
    e.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    e.chain_init(0.001 * wm, 0.0 * wm, 0.05 * wm)
    rng = np.random.default_rng(1)
    trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(steps // L + 1)]
    e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
    e.synchronize()
    t0 = time.perf_counter()
    e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
    e.synchronize()
    el = time.perf_counter() - t0
    return {"steps": steps, "seconds": round(el, 4), "steps_per_s": round(steps / el, 1), "ms_per_step": round(el / steps * 1e3, 4)}


def run(nx, ny, nz, comps):
    obs, b6 = aligned(nx, ny, nz)
    n, M, C = obs[0].size, b6.shape[0], len(comps)
    singles = {}
    for c in comps:
        e = g.Engine(n, M)
        e.set_translation_invariant(True)
        e.set_obs(*obs)
        e.set_cells(b6, 3, component=c)
        e.build_G()
        wm = e.weight(0.5)
        singles[c] = passes(e, wm, n, M)
        print(json.dumps(dict({"what": "single-component table passes", "component": c, "cells": [nx, ny, nz]}, **singles[c])),
              flush=True)
        e.close()
    e = g.Engine(C * n, M)
    e.set_cells_multi(b6, comps, np.ones(C), translation_invariant=True)
    e.set_obs(*obs)
    t0 = time.perf_counter()
    e.build_G()
    wm = e.weight(0.5)
    e.synchronize()
    t_build = time.perf_counter() - t0
    info = e.translation_invariant_info()
    print(json.dumps({"what": "block tables", "cells": [nx, ny, nz], "components": list(comps), "rows": C * n, "M": M,
                      "table_MB": round(info["table_bytes"] / 1e6, 2), "dense_GB": round(8.0 * C * n * M / 1e9, 1),
                      "max_dev": info["max_dev"], "build_and_weight_s": round(t_build, 3)}), flush=True)
    p = passes(e, wm, C * n, M)
    sums = {k: round(sum(s[k] for s in singles.values()), 4) for k in ("forward_ms", "adjoint_ms")}
    print(json.dumps(dict({"what": "block-aware passes"}, **p)), flush=True)
    print(json.dumps({"what": "block-aware / sum of the single-component passes", "sum_forward_ms": sums["forward_ms"],
                      "sum_adjoint_ms": sums["adjoint_ms"], "forward_ratio": round(p["forward_ms"] / sums["forward_ms"], 3),
                      "adjoint_ratio": round(p["adjoint_ms"] / sums["adjoint_ms"], 3)}), flush=True)
    rho = np.zeros((nz, nx, ny))
    rho[nz // 5:nz // 2, nx // 3:nx // 2, ny // 3:ny // 2] = 0.03
    d = e.forward(wm * rho.ravel())
    dobsw = d + 0.01 * np.abs(d).max() * np.random.default_rng(0).normal(size=C * n)
    print(json.dumps(dict({"what": "block-aware chain"}, **chain(e, wm, M, dobsw))), flush=True)
    e.close()


run(100, 100, 50, ("gz", "gzz", "gxx", "gyy", "gxz", "gyz"))
run(200, 200, 60, ("gz", "gzz"))
