"""The bootstrap batch on the translation-invariant store against the same replicates one at a time on the table and
against the batch on the dense store, from ONE run in one process:
    python profiles/lattice_bscg_clocks.py [reps] [maxk]
At 100 x 100 x 50 cells under 100 x 100 stations (observations above the cell centres at z = 0), samples=16:
  (a) BSCG(batch=16) on the table (BootStrap(translation_invariant=True));
  (b) the 16 replicates through the sequential BootStrap.CG on the table (BSCG());
  (c) BSCG(batch=16) on the dense store -- 40 GB of G and the batch's operand-ordered second copy;
and at 200 x 200 x 60 under 200 x 200, where no dense store exists, (a) alone.  Per form a warm-up, then the median of
`reps` repetitions; ms per lock-step = median / maxk, ms per pass = median / (3 maxk + 1) (a group is 2 maxk + 1
forwards and maxk adjoints); device memory = what the device lost between the constructor's first call and the end of
the warm-up (hipMemGetInfo through torch).  One JSON line per measurement.

The adjoint passes, the new one against the chain batch's:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/lattice_bscg_clocks.py --passes [reps] [maxk]
    python profiles/lattice_bscg_clocks.py --summarise DIR
--passes runs, at the first shape, `reps` groups of 16 on a "replicates" table and as many rounds of 16 chains with
L = maxk on a "chains" table in one process; --summarise reads the trace's kernel rows and prints count, median and
quartiles of the three instantiations of latb_pass_kernel."""
import contextlib
import csv
import glob
import io
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((100, 100, 50), (200, 200, 60))
H = 100.0
FORMS = {"0": "adjoint + leapfrog update (chain batch)", "1": "forward", "2": "adjoint + CG gradient (bootstrap batch)"}


def problem(shape):
    """mrange, mspacing, the observations above the cell centres"""
    nx, ny, nz = shape
    xp, yp = [v.ravel() for v in np.meshgrid((np.arange(nx) + 0.5) * H, (np.arange(ny) + 0.5) * H, indexing="ij")]
    return (0, nx * H, 0, ny * H, 0, nz * H), (H, H, H), (xp, yp, np.zeros_like(xp))


def free_bytes():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def timed(fn, reps):
    with contextlib.redirect_stdout(io.StringIO()):
        fn()  # warm-up (allocations; dense: the operand-ordered copy of G)
        after_warmup = free_bytes()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, after_warmup


def bootstrap(g, shape, maxk, table):
    mrange, mspacing, obs = problem(shape)
    before = free_bytes()
    bs = g.BootStrap(mrange, mspacing, obs, np.zeros(obs[0].size), (0.0, 1.0), samples=16, beta=0.1, maxk=maxk, verbose=False,
                     translation_invariant=table)
    rho = np.zeros(bs.mesh.shape)
    nz, ny, nx = rho.shape
    rho[nz // 5:nz // 2, ny // 3:2 * ny // 3, nx // 3:2 * nx // 3] = 0.8
    bs.dobs = bs._engine.forward(bs.Wm @ rho.ravel()) + 0.05 * np.random.default_rng(7).standard_normal(bs.dsize)
    return bs, before


def report(what, shape, maxk, med, ts, used, extra=None):
    out = {"what": what, "cells": list(shape), "samples": 16, "maxk": maxk, "median_s": round(med, 4),
           "all_s": [round(t, 4) for t in ts], "ms_per_lock_step": round(1e3 * med / maxk, 3),
           "ms_per_pass": round(1e3 * med / (3 * maxk + 1), 3), "device_MB": round(used / 1e6, 1)}
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def clocks(reps, maxk):
    import gravinv3dhmc_amd as g
    for shape in SHAPES:
        bs, before = bootstrap(g, shape, maxk, True)
        m0 = np.full(bs.msize, 0.001)
        info, plan = bs.translation_invariant_info(), bs._engine.translation_invariant_batch_plan()
        med, ts, after = timed(lambda: bs.BSCG(m0, batch=16), reps)
        a = report("BSCG(batch=16) on the table", shape, maxk, med, ts, before - after,
                   {"table_MB": round(info["table_bytes"] / 1e6, 1), "stats": bs._engine.bscg_stats(),
                    "plan": {k: plan[k] for k in ("adj_grid", "fwd_grid", "chunks", "lpc", "adj_lds", "fwd_lds")}})
        if shape != SHAPES[0]:
            bs._engine.close()
            continue
        med, ts, after = timed(lambda: bs.BSCG(m0), max(1, min(reps, 3)))
        b = report("16 x BootStrap.CG on the table, one at a time", shape, maxk, med, ts, before - after)
        bs._engine.close()
        del bs
        bs, before = bootstrap(g, shape, maxk, False)
        med, ts, after = timed(lambda: bs.BSCG(m0, batch=16), reps)
        c = report("BSCG(batch=16) on the dense store", shape, maxk, med, ts, before - after,
                   {"G_MB": round(bs.dsize * bs.msize * 8 / 1e6, 1), "stats": bs._engine.bscg_stats()})
        bs._engine.close()
        del bs
        print(json.dumps({"what": "ratios", "cells": list(shape), "sequential / table batch": round(b["median_s"] / a["median_s"], 2),
                          "dense batch / table batch": round(c["median_s"] / a["median_s"], 3)}), flush=True)


def passes(reps, maxk):
    """What a kernel trace is taken of: the bootstrap batch's and the chain batch's passes at the first shape"""
    import gravinv3dhmc_amd as g
    shape = SHAPES[0]
    bs, _ = bootstrap(g, shape, maxk, True)
    m0 = np.full(bs.msize, 0.001)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(reps):
            bs.BSCG(m0, batch=16)
    dobs, wm = bs.dobs.copy(), bs.Wm.diagonal().copy()
    bounds = bs.mesh.cell_bounds(active_only=True)
    obs = (bs.lonobs, bs.latobs, bs.heightobs)
    bs._engine.close()
    e = g.Engine(obs[0].size, bounds.shape[0])
    e.set_translation_invariant("chains")
    e.set_obs(*obs)
    e.set_cells(bounds, 0)
    e.build_G()
    e.weight(0.5)
    e.set_data(dobs)
    e.set_reg("Damping", 1.0, 0.01, (1, 1, bounds.shape[0]), 0.001 * wm)
    e.batch_init(np.stack([0.001 * wm] * 16), 0.0 * wm, 0.05 * wm)
    rng = np.random.default_rng(1)
    for _ in range(reps):
        e.batch_trajectory(rng.normal(size=(16, bounds.shape[0])) * 0.01, 0.002, [maxk] * 16, rng.uniform(size=16))
    e.synchronize()
    e.close()
    print(json.dumps({"what": "passes run", "cells": list(shape), "groups": reps, "rounds": reps, "maxk": maxk}), flush=True)


def summarise(folder):
    rows = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                m = re.search(r"latb_pass_kernel(?:<|ILi)(\d)", r.get("Kernel_Name", ""))
                if m:
                    rows.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    for form in sorted(rows):
        ms = np.array(rows[form])
        print(json.dumps({"kernel": "latb_pass_kernel<%s>" % form, "form": FORMS.get(form, "?"), "launches": int(ms.size),
                          "median_ms": round(float(np.median(ms)), 4), "q25_ms": round(float(np.percentile(ms, 25)), 4),
                          "q75_ms": round(float(np.percentile(ms, 75)), 4), "min_ms": round(float(ms.min()), 4),
                          "max_ms": round(float(ms.max()), 4)}), flush=True)
    if "0" in rows and "2" in rows:
        print(json.dumps({"what": "CG adjoint / chain adjoint, medians",
                          "ratio": round(float(np.median(rows["2"]) / np.median(rows["0"])), 4)}), flush=True)
    return 0 if rows else 1


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--summarise"]:
        sys.exit(summarise(args[1]))
    mode = passes if args[:1] == ["--passes"] else clocks
    nums = [int(v) for v in args if not v.startswith("--")]
    mode(nums[0] if nums else 5, nums[1] if len(nums) > 1 else 10)
