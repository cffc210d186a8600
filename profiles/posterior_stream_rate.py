"""What the streaming posterior (csrc/poststream.hip.h) costs a batch of 16 chains, and what it saves: HMCSampleBatch
with sample_sink="none" without and with posterior_stream=True, and with sample_sink="binary" and no stream (what a
user needs today for the same information), at C1 (600 x 6000) and at C2 (10^4 x 5 10^5, matrix-free).  Per run a
warm-up, then the median of `reps` repetitions, in chain-steps/s:
    python profiles/posterior_stream_rate.py [reps] [c1|c2|both] [nsamples]"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gravinv3dhmc_amd as g  # noqa: E402
from gravinv3dhmc_amd.inversion import hmc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
which = sys.argv[2] if len(sys.argv) > 2 else "both"
# name: (nx, ny, nz, dt, accepted samples per chain and run, matrix-free)
SIZES = {"c1": (20, 30, 10, 0.01, 400, False), "c2": (100, 100, 50, 0.002, 6, True)}
CHAINS, BINS = 16, 64


class Steps(object):
    """Leapfrog steps of all chains, counted where the sampler hands the lists to the library."""

    def __init__(self, eng):
        self.eng, self.n, self.inner = eng, 0, eng.batch_run

    def __call__(self, p0s, dt, Ls, us, want_x=False, carry=False, entered=None):
        out = self.inner(p0s, dt, Ls, us, want_x, carry, entered)
        Ls = np.asarray(Ls)
        if carry:
            # (started trajectories; what is still in flight at the end of a run is a fraction of one offer)
            self.n += int(sum(Ls[c, :int(k)].sum() for c, k in enumerate(out[3])))
        else:
            self.n += int(Ls.sum())
        return out


for name in (("c1", "c2") if which == "both" else (which,)):
    nx, ny, nz, dt, nsamp, mf = SIZES[name]
    if len(sys.argv) > 3:
        nsamp = int(sys.argv[3])
    mrange, mspacing = (0, 100.0 * nx, 0, 100.0 * ny, 0, 100.0 * nz), (100, 100, 100)
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * ny, ny), np.linspace(0, 100.0 * nx, nx))]
    zp = np.zeros_like(xp)
    kw = {"matrix_free": True} if mf else {}
    gm = g.GravMagModule(np.zeros(xp.size), mrange, mspacing, (xp, yp, zp), verbose=False, **kw)
    eng = gm._engine
    M, N = eng.M, eng.N
    rho = np.zeros((nz, ny, nx))
    rho[nz // 5:nz // 2, ny // 3:2 * ny // 3, nx // 3:2 * nx // 3] = 1.0
    dobs = eng.forward(gm.Wm.diagonal() * rho.ravel())
    dobs = dobs + 0.02 * np.abs(dobs).max() * np.random.default_rng(0).normal(size=N)
    gm.dobs = dobs
    eng.set_data(dobs)
    counter = Steps(eng)
    eng.batch_run = counter
    tmp = tempfile.mkdtemp(prefix="poststream_rate_")

    def run(sink, stream):
        def once():
            counter.n = 0
            t0 = time.perf_counter()
            hmc.HMCSampleBatch(gm, CHAINS, nsamp, 0, dt, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                               np.c_[np.zeros(M), np.ones(M)], "mandatory", 1000, dobs, "Fixed", 0.8, 1.0, "Damping", 0.001,
                               100, 0.001, save_folder=os.path.join(tmp, "chain"), sample_sink=sink,
                               posterior_stream=True if stream else None)
            eng.synchronize()
            t = time.perf_counter() - t0
            if stream:
                eng.posterior_stream_free()
            return counter.n / t
        with contextlib.redirect_stdout(io.StringIO()):
            once()
            rates = [once() for _ in range(reps)]
        return float(np.median(rates)), rates

    print("%s: N x M = %d x %d, %d chains, %d accepted samples per chain and run, median of %d" %
          (name, N, M, CHAINS, nsamp, reps))
    for label, sink, stream in (("sink none", "none", False), ("sink none + posterior stream", "none", True),
                                ("sink binary", "binary", False)):
        med, rates = run(sink, stream)
        print("  %-30s %12.0f chain-steps/s  (%s)" % (label, med, " ".join("%.0f" % r for r in rates)))
    print("  stream state: (5 x 8 x %d + 4 x %d) x M = %.1f MB" % (CHAINS, BINS, (40 * CHAINS + 4 * BINS) * M / 1e6))
    shutil.rmtree(tmp, ignore_errors=True)
    eng.close()
