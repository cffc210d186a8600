"""The translation-invariant store against the dense store on the SAME aligned geometry, in one process:
    python profiles/lattice_clocks.py [steps] [nx ny nz]
C2-shaped: cells 100 x 100 x 50 of 100 m, observations above the 100 x 100 cell centres at z = 0.  Steps per second of
a chain on the table and on the dense store (same draws), and the time of each table pass (HIP events around the
launches of gh_adjoint / gh_forward / the chain's steps: gather + pass).  Then the table alone at the C5 shape
(200 x 200 x 60 under 200 x 200), where no dense store exists to compare with.  One JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
shape = tuple(int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (100, 100, 50)
L = 10


def aligned(nx, ny, nz, h=100.0):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * h, np.arange(ny + 1) * h, np.arange(nz + 1) * h
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * h, ye[:-1] + 0.5 * h, indexing="ij")]
    return (xp, yp, np.zeros_like(xp)), np.ascontiguousarray(b6)


def chain(e, wm, N, M, dobs, tag):
    e.set_data(dobs)
    e.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    e.chain_init(0.001 * wm, 0.0 * wm, 0.05 * wm)
    rng = np.random.default_rng(1)
    trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(steps // L + 1)]
    e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
    e.synchronize()
    e.profile_enable(True)
    t0 = time.perf_counter()
    e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
    e.synchronize()
    el = time.perf_counter() - t0
    pr = e.profile_read()
    ms, n = pr["sweep_ms"], pr["sweeps"]
    e.profile_enable(False)
    out = {"what": tag + " chain", "steps": steps, "seconds": round(el, 4), "steps_per_s": round(steps / el, 1),
           "ms_per_step": round(el / steps * 1e3, 4), "timed_sweeps": n, "ms_per_timed_sweep": round(ms / max(n, 1), 4),
           "spec_hits": e.chain_stats()["spec_hits"]}
    print(json.dumps(out), flush=True)
    return out


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


def table_engine(obs, b6):
    e = g.Engine(obs[0].size, b6.shape[0])
    e.set_translation_invariant(True)
    e.set_obs(*obs)
    e.set_cells(b6, 0)
    t0 = time.perf_counter()
    e.build_G()
    wm = e.weight(0.5)
    e.synchronize()
    return e, wm, time.perf_counter() - t0


def run(nx, ny, nz, with_dense):
    obs, b6 = aligned(nx, ny, nz)
    N, M = obs[0].size, b6.shape[0]
    e, wm, t_build = table_engine(obs, b6)
    info = e.translation_invariant_info()
    print(json.dumps({"what": "table", "cells": [nx, ny, nz], "N": N, "M": M, "table_MB": round(info["table_bytes"] / 1e6, 2),
                      "dense_GB": round(8.0 * N * M / 1e9, 1), "max_dev": info["max_dev"], "build_and_weight_s": round(t_build, 3)}),
          flush=True)
    rho = np.zeros((nz, nx, ny))
    rho[nz // 5:nz // 2, nx // 3:nx // 2, ny // 3:ny // 2] = 0.03
    d = e.forward(wm * rho.ravel())
    dobs = d + 0.01 * np.abs(d).max() * np.random.default_rng(0).normal(size=N)
    print(json.dumps(dict({"what": "table passes"}, **passes(e, wm, N, M))), flush=True)
    t = chain(e, wm, N, M, dobs, "table")
    e.close()
    if not with_dense:
        return
    e = g.Engine(N, M)
    e.set_obs(*obs)
    e.set_cells(b6, 0)
    t0 = time.perf_counter()
    e.build_G()
    wd = e.weight(0.5)
    e.synchronize()
    print(json.dumps({"what": "dense", "build_and_weight_s": round(time.perf_counter() - t0, 3),
                      "weights_relmax": float(np.abs(wd - wm).max() / wd.max())}), flush=True)
    dn = chain(e, wd, N, M, dobs, "dense")
    print(json.dumps({"what": "dense store's fold", **{k: v for k, v in e.fold_info().items() if k in ("on", "pair_on", "reason")}}),
          flush=True)
    print(json.dumps({"what": "table / dense", "steps_per_s_ratio": round(t["steps_per_s"] / dn["steps_per_s"], 2)}), flush=True)
    e.close()


run(*shape, with_dense=True)
if len(sys.argv) <= 4:
    run(200, 200, 60, with_dense=False)
