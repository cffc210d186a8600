"""Chain batches on the translation-invariant store against chains taking turns on the single-chain passes, from the
SAME run:
    python profiles/lattice_batch_clocks.py [trajectories per chain]
At cells 100 x 100 x 50 under 100 x 100 stations and 200 x 200 x 60 under 200 x 200 (observations above the cell
centres at z = 0):
  (a) chain-steps/s of ONE chain on the single-chain table passes (set_translation_invariant(True)): what 16 chains
      taking turns would get;
  (b) chain-steps/s of 16 chains on the batch (set_translation_invariant("chains")), and the time of the batch's launches
      between HIP events (gather r + adjoint pass, gather x + forward pass).
(b) is judged against (a) of the same run: the bar is (b) >= 1.05 (a) at both shapes.  Every measurement is a child
process of its own under its own time limit; after one that fails or runs out of time nothing more is started.  One JSON
line per measurement, then the ratio."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 10
C = 16
SHAPES = ((100, 100, 50), (200, 200, 60))
LIMIT_S = {"single": 240, "batch": 420}


def aligned(nx, ny, nz, h=100.0):
    """cells (layer, x, y) and the observations above their centres"""
    xe, ye, ze = np.arange(nx + 1) * h, np.arange(ny + 1) * h, np.arange(nz + 1) * h
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], ze[k], ze[k + 1]], axis=1)
    xp, yp = [v.ravel() for v in np.meshgrid(xe[:-1] + 0.5 * h, ye[:-1] + 0.5 * h, indexing="ij")]
    return (xp, yp, np.zeros_like(xp)), np.ascontiguousarray(b6)


def table_engine(g, obs, b6, mode, shape):
    nx, ny, nz = shape
    e = g.Engine(obs[0].size, b6.shape[0])
    e.set_translation_invariant(mode)
    e.set_obs(*obs)
    e.set_cells(b6, 0)
    e.build_G()
    wm = e.weight(0.5)
    rho = np.zeros((nz, nx, ny))
    rho[nz // 5:nz // 2, nx // 3:nx // 2, ny // 3:ny // 2] = 0.03
    d = e.forward(wm * rho.ravel())
    dobs = d + 0.01 * np.abs(d).max() * np.random.default_rng(0).normal(size=d.size)
    e.set_data(dobs)
    e.set_reg("Damping", 1.0, 0.01, (1, 1, b6.shape[0]), 0.001 * wm)
    return e, wm


def child(what, shape, T):
    import gravinv3dhmc_amd as g
    obs, b6 = aligned(*shape)
    N, M = obs[0].size, b6.shape[0]
    flop_step = 2 * 2.0 * N * M  # two passes, an FMA per pair and chain
    rng = np.random.default_rng(1)
    if what == "single":
        e, wm = table_engine(g, obs, b6, True, shape)
        e.chain_init(0.001 * wm, 0.0 * wm, 0.05 * wm)
        trajs = [(L, rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(T * 4 + 1)]
        e.run_chain(iter(trajs[:1]), 0.002, lambda *a: None)  # warm-up
        e.synchronize()
        t0 = time.perf_counter()
        e.run_chain(iter(trajs[1:]), 0.002, lambda *a: None)
        e.synchronize()
        el = time.perf_counter() - t0
        steps = L * (len(trajs) - 1)
        out = {"what": "single chain on the table", "cells": list(shape), "chain_steps": steps, "seconds": round(el, 4),
               "chain_steps_per_s": round(steps / el, 1), "tflops": round(flop_step * steps / el / 1e12, 2)}
    else:
        e, wm = table_engine(g, obs, b6, "chains", shape)
        plan = e.translation_invariant_batch_plan()
        e.batch_init(np.stack([0.001 * wm] * C), 0.0 * wm, 0.05 * wm)

        def lists(n):
            return ([[rng.normal(size=M) * 0.01 for _ in range(n)] for _ in range(C)], np.full((C, n), L), rng.uniform(size=(C, n)))

        p0s, Ls, us = lists(1)
        e.batch_run(p0s, 0.002, Ls, us)  # warm-up
        e.synchronize()
        p0s, Ls, us = lists(T)
        e.profile_enable(True)
        t0 = time.perf_counter()
        acc, _, _ = e.batch_run(p0s, 0.002, Ls, us)
        e.synchronize()
        el = time.perf_counter() - t0
        pr = e.profile_read()
        e.profile_enable(False)
        steps = C * T * L
        # (a timed launch is a gather and its pass; a lock-step of the batch is one adjoint and one forward launch)
        ms_launch = pr["sweep_ms"] / max(pr["sweeps"], 1)
        out = {"what": "16 chains on the batch", "cells": list(shape), "chain_steps": steps, "seconds": round(el, 4),
               "chain_steps_per_s": round(steps / el, 1), "tflops": round(flop_step * steps / el / 1e12, 2),
               "timed_launches": pr["sweeps"], "ms_per_timed_launch": round(ms_launch, 4),
               "tflops_in_launches": round(flop_step * C / 2 / (ms_launch * 1e-3) / 1e12, 2) if ms_launch > 0 else None,
               "launch_share_of_wall": round(pr["sweep_ms"] * 1e-3 / el, 3), "accepted": int(acc.sum()),
               "plan": {k: plan[k] for k in ("adj_grid", "fwd_grid", "chunks", "lpc", "adj_lds", "fwd_lds")}}
    e.close()
    print(json.dumps(out), flush=True)


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for shape in SHAPES:
        got = {}
        for what in ("single", "batch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", what] + [str(v) for v in shape] + [str(T)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[what])
            except subprocess.TimeoutExpired:
                print(json.dumps({"what": what, "cells": list(shape), "error": "time limit of %d s" % LIMIT_S[what]}), flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                print(json.dumps({"what": what, "cells": list(shape), "error": "exit status %d" % r.returncode,
                                  "stderr": r.stderr[-2000:]}), flush=True)
                return 1
            print(line[-1], flush=True)
            got[what] = json.loads(line[-1])
        ratio = got["batch"]["chain_steps_per_s"] / got["single"]["chain_steps_per_s"]
        print(json.dumps({"what": "batch / single", "cells": list(shape), "ratio": round(ratio, 3), "bar": 1.05,
                          "met": bool(ratio >= 1.05)}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], tuple(int(v) for v in sys.argv[3:6]), int(sys.argv[6]))
    else:
        sys.exit(main())
