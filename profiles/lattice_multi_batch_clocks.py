"""Chain batches on the multi-component translation-invariant table against one chain on the single-chain block passes of
the same geometry, in one process:
    python profiles/lattice_multi_batch_clocks.py [trajectories per chain]
At the README's two multi-component shapes -- gz, gzz, gxx, gyy, gxz, gyz over 100 x 100 x 50 cells of 100 m under the
100 x 100 cell centres, and gz, gzz over 200 x 200 x 60 under 200 x 200:
  (a) chain-steps/s of ONE chain on the single-chain block passes (set_cells_multi(..., translation_invariant=True)): what
      16 chains taking turns would get;
  (b) chain-steps/s of 16 chains on the batch (translation_invariant="chains");
  (c) ms per batch adjoint and forward launch (gather + pass between HIP events) on the block tables, against nb times
      the same launch of the single-block batch (set_translation_invariant("chains"), gz) at the same extents.  A round of
      L = 1 is two adjoint launches and one forward, a round of L = 2 three and two: the two launches' times are solved
      from the medians of the rounds' event times.
(b) is judged against (a) of the same run.  One JSON line per measurement, then the ratios."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3
L = 10
C = 16
REPS = 9


def aligned(nx, ny, nz, h=100.0):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * h, np.arange(ny + 1) * h, np.arange(nz + 1) * h
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * h, ye[:-1] + 0.5 * h, indexing="ij")]
    return (xp, yp, np.zeros_like(xp)), np.ascontiguousarray(b6)


def prepared(e, shape, M):
    """weights, data of a block of anomalous cells plus noise, the regulariser"""
    nx, ny, nz = shape
    wm = e.weight(0.5)
    rho = np.zeros((nz, nx, ny))
    rho[nz // 5:nz // 2, nx // 3:nx // 2, ny // 3:ny // 2] = 0.03
    d = e.forward(wm * rho.ravel())
    e.set_data(d + 0.01 * np.abs(d).max() * np.random.default_rng(0).normal(size=d.size))
    e.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    return wm


def multi(obs, b6, comps, table):
    e = g.Engine(len(comps) * obs[0].size, b6.shape[0])
    e.set_cells_multi(b6, comps, np.ones(len(comps)), translation_invariant=table)
    e.set_obs(*obs)
    e.build_G()
    return e


def single_chain(e, wm, M):
    rng = np.random.default_rng(1)
    e.chain_init(0.001 * wm, 0.0 * wm, 0.05 * wm)
    trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(T * 4 + 1)]
    e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
    e.synchronize()
    t0 = time.perf_counter()
    e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
    e.synchronize()
    el = time.perf_counter() - t0
    steps = L * (len(trajs) - 1)
    return {"chain_steps": steps, "seconds": round(el, 4), "chain_steps_per_s": round(steps / el, 1)}


def batch(e, wm, M):
    rng = np.random.default_rng(1)
    e.batch_init(np.stack([0.001 * wm] * C), 0.0 * wm, 0.05 * wm)

    def lists(n):
        return ([[rng.normal(size=M) * 0.01 for _ in range(n)] for _ in range(C)], np.full((C, n), L), rng.uniform(size=(C, n)))

    p0s, Ls, us = lists(1)
    e.batch_run(p0s, 0.002, Ls, us)  # warm-up
    e.synchronize()
    p0s, Ls, us = lists(T)
    t0 = time.perf_counter()
    acc, _, _ = e.batch_run(p0s, 0.002, Ls, us)
    e.synchronize()
    el = time.perf_counter() - t0
    steps = C * T * L
    return {"chain_steps": steps, "seconds": round(el, 4), "chain_steps_per_s": round(steps / el, 1), "accepted": int(acc.sum())}


def launches(e, wm, M):
    """ms of the batch's adjoint launch and of its forward launch, from lock-step rounds of L = 1 and L = 2"""
    rng = np.random.default_rng(3)
    e.batch_init(np.stack([0.001 * wm] * C), 0.0 * wm, 0.05 * wm)
    ms = {}
    for Lr in (1, 2):
        got = []
        for rep in range(REPS + 1):
            p0s, us = rng.normal(size=(C, M)) * 0.01, rng.uniform(size=C)
            e.profile_enable(True)
            e.batch_trajectory(p0s, 0.002, [Lr] * C, us)
            pr = e.profile_read()
            e.profile_enable(False)
            assert pr["sweeps"] == 2 * Lr + 1, pr
            if rep:  # (the first round warms up)
                got.append(pr["sweep_ms"])
        ms[Lr] = float(np.median(got))
    return {"adjoint_ms": round(2 * ms[1] - ms[2], 4), "forward_ms": round(2 * ms[2] - 3 * ms[1], 4),
            "round_L1_ms": round(ms[1], 4), "round_L2_ms": round(ms[2], 4)}


def run(shape, comps):
    obs, b6 = aligned(*shape)
    n, M, nb = obs[0].size, b6.shape[0], len(comps)
    head = {"cells": list(shape), "components": list(comps)}

    e = multi(obs, b6, comps, True)
    wm = prepared(e, shape, M)
    one = single_chain(e, wm, M)
    print(json.dumps(dict({"what": "one chain on the single-chain block passes"}, **head, **one)), flush=True)
    e.close()

    e = multi(obs, b6, comps, "chains")
    wm = prepared(e, shape, M)
    plan = e.translation_invariant_batch_plan()
    info = e.translation_invariant_info()
    bat = batch(e, wm, M)
    print(json.dumps(dict({"what": "16 chains on the block tables' batch", "table_MB": round(info["table_bytes"] / 1e6, 2),
                           "plan": {k: plan[k] for k in ("blocks", "adj_grid", "fwd_grid", "chunks", "lpc", "adj_lds", "fwd_lds")}},
                          **head, **bat)), flush=True)
    blocks = launches(e, wm, M)
    print(json.dumps(dict({"what": "batch launches on the block tables"}, **head, **blocks)), flush=True)
    e.close()

    e = g.Engine(n, M)
    e.set_translation_invariant("chains")
    e.set_obs(*obs)
    e.set_cells(b6, 0)
    e.build_G()
    wm = prepared(e, shape, M)
    single = launches(e, wm, M)
    print(json.dumps(dict({"what": "batch launches on the single-block table (gz)", "cells": list(shape)}, **single)), flush=True)
    e.close()

    ratio = bat["chain_steps_per_s"] / one["chain_steps_per_s"]
    print(json.dumps({"what": "ratios", "cells": list(shape), "blocks": nb,
                      "batch / single chain (chain-steps/s)": round(ratio, 3),
                      "the batch is slower than 16 single chains": bool(ratio < 1.0),
                      "adjoint / (nb x single-block adjoint)": round(blocks["adjoint_ms"] / (nb * single["adjoint_ms"]), 3),
                      "forward / (nb x single-block forward)": round(blocks["forward_ms"] / (nb * single["forward_ms"]), 3)}),
          flush=True)


run((100, 100, 50), ("gz", "gzz", "gxx", "gyy", "gxz", "gyz"))
run((200, 200, 60), ("gz", "gzz"))
