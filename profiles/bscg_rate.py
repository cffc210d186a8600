"""Bootstrap replicates one at a time against 16 in lock-step (csrc/bscg.hip.h): BSCG() and BSCG(batch=16) on the same
object, samples=16, maxk=10, at C1 (600 x 6000, 27 MiB of G) and at 2500 x 50000 (954 MiB of G: past every cache).
Per run a warm-up, then the median of `reps` repetitions:    python profiles/bscg_rate.py [reps] [c1|large|both]"""
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
which = sys.argv[2] if len(sys.argv) > 2 else "both"
SIZES = {"c1": ((0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (20, 30)),
         "large": ((0, 5000, 0, 5000, 0, 2000), (100, 100, 100), (50, 50))}


def timed(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        fn()  # warm-up (allocations, the operand-ordered copy of G)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, out


for name in (("c1", "large") if which == "both" else (which,)):
    mrange, mspacing, (nx, ny) = SIZES[name]
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(mrange[2], mrange[3], ny), np.linspace(mrange[0], mrange[1], nx))]
    zp = np.zeros_like(xp)
    mesh = g.mesher.PrismMesh(mrange, mspacing)
    rho = np.zeros(mesh.shape)
    rho[3:7, mesh.shape[1] // 3:2 * mesh.shape[1] // 3, mesh.shape[2] // 3:2 * mesh.shape[2] // 3] = 0.8
    bs = g.BootStrap(mrange, mspacing, (xp, yp, zp), np.zeros(xp.size), (0.0, 1.0), samples=16, beta=0.1, maxk=10,
                     verbose=False)
    # the body's field from the resident kernel (Aw (Wm rho) = A rho), plus seeded noise
    bs.dobs = bs._engine.forward(bs.Wm @ rho.ravel()) + 0.05 * np.random.default_rng(7).standard_normal(xp.size)
    m0 = np.full(bs.msize, 0.001)
    t_seq, all_seq, r_seq = timed(lambda: bs.BSCG(m0))
    t_bat, all_bat, r_bat = timed(lambda: bs.BSCG(m0, batch=16))
    dev = max(float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(r_seq, r_bat))
    print("%s: N x M = %d x %d (%.0f MiB of G), samples=16, maxk=10, median of %d" %
          (name, bs.dsize, bs.msize, bs.dsize * bs.msize * 8 / 2 ** 20, reps))
    print("  BSCG()          %.4f s  (%s)" % (t_seq, " ".join("%.4f" % t for t in all_seq)))
    print("  BSCG(batch=16)  %.4f s  (%s)" % (t_bat, " ".join("%.4f" % t for t in all_bat)))
    print("  ratio %.1f; gh_bscg_stats of the group: %r; largest relative difference of the four results %.2e" %
          (t_seq / t_bat, bs._engine.bscg_stats(), dev))
    bs._engine.close()
