"""The dense problem of the trajectory feeder's device tests (tests/test_gpu_chain_feed.py) and what the CPU
oracle does with the reference's random stream on it.  No device.

12 x 10 observations over 12 x 10 x 4 prisms (N = 120, M = 480: with GRAVHMC_RESIDENT=0 the dense fused sweep, several
workgroups, a grid that is not square so nothing folds), Damping, data of a sparse model plus noise, a chain in a
box around its start.  DT is a fifth of the stability limit (helpers.stable_dt): nearly every trajectory of the
stream is accepted.  DT_REJECT and SEED_REJECT were picked on the oracle (rejections() below prints the table): with
them the first 12 trajectories of the stream hold accepted and rejected ones, each decided with a margin."""
import functools

import numpy as np

import fold_oracle_cases as fc
from helpers import stable_dt

OBS, CELLS = (12, 10), (12, 10, 4)
SEED_REJECT, DT_REJECT_FACTOR = 4, 3.2   # the oracle: AArAArAArrrr, closest decision |log u + dH| = 7.1


class Dense(object):
    def __init__(self, orc):
        self.obs, self.b6 = fc.geometry(OBS, CELLS)
        self.N, self.M = self.obs.shape[1], self.b6.shape[0]
        nx, ny, nz = CELLS
        self.shape = (nz, ny, nx)
        self.reg, self.alpha, self.beta = "Damping", 1.0, 0.01
        rng = np.random.default_rng(20250)
        self.Aw, self.wm = orc.col_weight(orc.prism_gz_kernel(self.obs[0], self.obs[1], self.obs[2], self.b6), 0.5)
        rho = np.zeros(self.M)
        rho[rng.choice(self.M, self.M // 10, replace=False)] = 1.0
        clean = self.Aw @ (self.wm * rho)
        self.dobs = clean + 0.01 * np.abs(clean).max() * rng.normal(size=self.N)
        self.mwapr = 0.001 * self.wm
        self.P = orc.Problem(self.Aw, self.dobs, self.mwapr, self.reg, self.alpha, self.beta, wm=self.wm, shape=self.shape)
        xc = self.wm * rng.uniform(0.3, 0.7, size=self.M)
        self.dt = stable_dt(self.P, xc, rng)
        self.dt_reject = DT_REJECT_FACTOR * self.dt
        self.low, self.high = xc - 1.5 * self.dt, xc + 1.5 * self.dt
        self.x0 = xc + self.dt * rng.uniform(-1.0, 1.0, size=self.M)

    def stream(self, seed, n, Lrange=None, plan=None, sigma=1.0):
        """The first n trajectories (L, p0, u) of np.random.RandomState(seed) in the reference's order."""
        rs = np.random.RandomState(seed)
        out = []
        for k in range(n):
            L = plan[k] if plan is not None else rs.randint(Lrange[0], Lrange[1] + 1)
            p0 = rs.randn(self.M) * sigma
            out.append((int(L), p0, float(rs.rand())))
        return out

    def oracle_chain(self, trajs, dt):
        """The oracle's chain over trajs: [(accepted, out5, x after, dH)]."""
        x, out = self.x0, []
        for L, p0, u in trajs:
            x, acc, o, _ = self.P.leapfrog(x, p0, dt, L, self.low, self.high, u)
            out.append((bool(acc), np.array(o), x.copy(), float(o[4] - o[3])))
        return out


@functools.lru_cache(maxsize=1)
def dense():
    from oracle import oracle
    return Dense(oracle)


def rejections(seeds=range(12), factors=(2.0, 2.4, 2.8, 3.2, 3.6, 4.0)):
    """The table DT_REJECT_FACTOR and SEED_REJECT were chosen from: per (factor, seed) the decisions of the first 12
    trajectories with Lrange (5, 20) and the smallest |log u + dH| among them (the margin of the closest decision)."""
    d = dense()
    for f in factors:
        for s in seeds:
            tr = d.stream(s, 12, Lrange=(5, 20))
            ch = d.oracle_chain(tr, f * d.dt)
            margin = min(abs(np.log(t[2]) + c[3]) for t, c in zip(tr, ch))
            print("factor %.1f seed %2d: %s  margin %.3f" % (f, s, "".join("A" if c[0] else "r" for c in ch), margin))


if __name__ == "__main__":
    rejections()
