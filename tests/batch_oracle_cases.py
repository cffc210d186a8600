"""The cases of the stored-kernel chain batch against the CPU oracle (tests/test_gpu_batch_oracle.py on the device,
tests/test_batch_oracle_host.py for the generator itself): the case table, the partitions of batch_alloc and
bteam_plan (csrc/host_batch.h) restated from the CU count, and the generator of inputs and oracle trajectories.

A case is a random Fortran-ordered matrix (column scales over 0.1 .. 3, weighted with 0.5), data with a mean 10^3
times their spread, C chains with their own starts in one box of +-1.5 dt, and T rounds of trajectories whose
lengths are drawn per chain from 1 .. 6 (so that slots idle while others step).  Everything the device is compared
with comes from oracle.Problem.leapfrog, before an engine is touched.  The variate u of a trajectory sits half-way
between the oracle's exp(-dH) and 0 or 1; a rejection is used only where dH > 0.01.

DELTA: the relative change of ONE entry of A that moves the oracle's results by more than 100 TOL_TRAJ (the host
test checks it at two entries per case: last valid row / last column, and first row of the last 16-row patch / first
column of the last tile).  It states how sharp the comparison is: a kernel that misreads one such entry by that
much fails its case."""
import functools

import numpy as np

from helpers import metropolis_u, relmax, shape3, stable_dt

TOL_TRAJ = 1e-10
DELTA = 1e-4          # per case unless the table says otherwise

# csrc/batchteam.hip.h
BT_RC, BT_MINMEM, BT_MAXMEM = 7, 8, 32


def roundup16(n):
    return (n + 15) // 16 * 16


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- the plans, restated

def two_pass_plan(N, M, cus):
    """batch_alloc (stored kernel): the forward's 512-row blocks x column blocks (about four workgroups per CU),
    the adjoint's waves (one per pair of 16-column tiles, at most 16 per CU)."""
    ld = roundup16(N)
    ntiles = cdiv(M, 16)
    rowblocks = cdiv(ld, 512)
    colblocks = max(1, cdiv(cus * 4, rowblocks))
    cpb = roundup16(cdiv(M, colblocks))
    n_colblocks = cdiv(M, cpb)
    npairs = cdiv(ntiles, 2)
    wgs = min(cdiv(npairs, 4), cus * 4)
    return {"ld": ld, "np": ld // 16, "ntiles": ntiles, "rowblocks": rowblocks, "cols_per_block": cpb,
            "n_colblocks": n_colblocks, "last_block": M - (n_colblocks - 1) * cpb, "npairs": npairs,
            "n_waves": wgs * 4}


def team_plan(N, M, cus):
    """bteam_plan: members = row chunks of 448 rows (8 .. 32 of them, at most one per CU), ranges of column tiles
    over the CUs that leaves; members = 0: the two passes stay."""
    ld = roundup16(N)
    ntiles = cdiv(M, 16)
    nrb = cdiv(ld, 64)
    members = cdiv(nrb, BT_RC)
    off = {"members": 0, "ranges": 0, "tpr": 0, "nval": 0, "last_range": 0, "row_chunks": members}
    if members < BT_MINMEM or members > BT_MAXMEM or members > cus:
        return off
    fr = max(1, min(ntiles, cus // members))
    tpr = cdiv(ntiles, fr)
    ranges = cdiv(ntiles, tpr)
    return {"members": members, "ranges": ranges, "tpr": tpr, "nval": cdiv(256, members),
            "last_range": ntiles - (ranges - 1) * tpr, "row_chunks": members}


def _true_3d(M):
    s = shape3(M)
    return s[0] > 1 and s[1] > 1 and s[2] > 1


def column_block_M(N, cus):
    """M at which batch_forward_kernel's column blocks hold 32 columns and the last one 7."""
    rowblocks = cdiv(roundup16(N), 512)
    colblocks = max(1, cdiv(cus * 4, rowblocks))
    k = cdiv(16 * colblocks + 1, 32)
    while not _true_3d(32 * k + 7):
        k += 1
    return 32 * k + 7


def more_pairs_M(cus):
    """Two pairs of tiles more than batch_adjoint_kernel has waves (16 per CU), and a partial last tile."""
    return 32 * 16 * cus + 40


def team_tiles_M(N, cus, tpr):
    """M at which a range of batch_team_kernel holds `tpr` tiles and the last range one: ntiles = tpr fr - (tpr - 1);
    the last tile partial, M a product of three factors > 1."""
    members = cdiv(cdiv(roundup16(N), 64), BT_RC)
    fr = cus // members
    ntiles = tpr * fr - (tpr - 1)
    for short in (9, 7, 11, 5, 13, 3, 1, 15, 6, 10, 4, 12, 2, 14, 8):
        if _true_3d(16 * ntiles - short):
            return 16 * ntiles - short
    raise AssertionError("no 3-D shape with %d tiles" % ntiles)


# ----------------------------------------------------------------------------- the case table

class Spec(object):
    def __init__(self, cid, group, N, M, reg, fix, C, T, team=False, expect=None, colmajor=False, delta=DELTA,
                 shape=None):
        self.id, self.group, self.N, self.M, self.reg, self.fix, self.C, self.T = cid, group, N, M, reg, fix, C, T
        self.team, self.expect, self.colmajor, self.delta, self.shape = team, expect, colmajor, delta, shape

    def size(self, cus):
        """M (from the CU count where the case says so) and its (nz, ny, nx)."""
        M = self.M
        if M == "colblocks":
            M = column_block_M(self.N, cus)
        elif M == "pairs":
            M = more_pairs_M(cus)
        elif isinstance(M, tuple):
            M = team_tiles_M(self.N, cus, M[1])
        shape = self.shape or shape3(M)
        assert shape[0] * shape[1] * shape[2] == M
        return M, shape


# two passes (GRAVHMC_BATCH_TEAM=0).  Regularisers and grav_fix alternate; C runs over 1, 5, 16.
TWO_PASS = [
    # row patches of 16 at M = 33 = 1 x 3 x 11: np = 1, 1, 2, 3, 4, 7 (the adjoint's ring of three).  N = 1: the mean
    # removal leaves no residual, so an entry of A acts through its column's weight only (wm^2 of MS, mwapr)
    Spec("p-n1", "patches", 1, 33, "MS", False, 5, 4, shape=(1, 3, 11)),
    Spec("p-n16", "patches", 16, 33, "Smoothness", True, 16, 4, shape=(1, 3, 11)),
    Spec("p-n17", "patches", 17, 33, "TV", False, 1, 6, shape=(1, 3, 11)),
    Spec("p-n33", "patches", 33, 33, "Damping", True, 5, 4, shape=(1, 3, 11)),
    Spec("p-n49", "patches", 49, 33, "Smoothness", False, 16, 4, shape=(1, 3, 11)),
    Spec("p-n97", "patches", 97, 33, "TV", True, 5, 4, shape=(1, 3, 11)),
    # forward row blocks of 512 and waves of 128 rows; 513, 1025: the last block has waves wholly past ld
    Spec("r-n130", "rowblocks", 130, 105, "TV", True, 5, 4, shape=(3, 5, 7)),
    Spec("r-n496", "rowblocks", 496, 126, "Smoothness", False, 16, 3, shape=(2, 7, 9)),
    Spec("r-n511", "rowblocks", 511, 117, "MS", True, 1, 6, shape=(3, 3, 13)),
    Spec("r-n513", "rowblocks", 513, 110, "Smoothness", True, 5, 4, colmajor=True, shape=(2, 5, 11)),
    Spec("r-n1025", "rowblocks", 1025, 75, "TV", False, 16, 3, shape=(3, 5, 5)),
    # column tiles at N = 49: a single tile, a pair without its second tile, a partial last tile
    Spec("c-m1", "tiles", 49, 1, "Damping", False, 16, 4),
    Spec("c-m15", "tiles", 49, 15, "TV", True, 5, 4),
    Spec("c-m16", "tiles", 49, 16, "MS", False, 5, 4),
    Spec("c-m17", "tiles", 49, 17, "Smoothness", True, 16, 4, colmajor=True),
    Spec("c-m32", "tiles", 49, 32, "Damping", False, 1, 6),
    Spec("c-m33", "tiles", 49, 33, "MS", True, 5, 4),
    Spec("c-m47", "tiles", 49, 47, "TV", False, 16, 4, colmajor=True),
    Spec("c-m48", "tiles", 49, 48, "Smoothness", True, 5, 4),
    # column blocks of the forward: >= 32 columns each, a short last block that is no multiple of 16
    Spec("b-n5003", "colblocks", 5003, "colblocks", "TV", True, 5, 2, delta=1e-3),
    # more pairs of tiles than the adjoint has waves: some waves take a second pair
    Spec("w-n20", "colblocks", 20, "pairs", "Smoothness", False, 5, 2),
]

# teams (GRAVHMC_BATCH_TEAM=1); expect: members (0: bteam_plan refuses, the two passes run)
TEAMS = [
    Spec("t-n3137", "teams", 3137, 273, "Smoothness", True, 16, 3, team=True, expect=8, shape=(3, 7, 13)),
    Spec("t-n3585", "teams", 3585, 330, "TV", False, 5, 3, team=True, expect=9, shape=(5, 6, 11)),
    Spec("t-n14321", "teams", 14321, 252, "MS", True, 5, 2, team=True, expect=32, shape=(4, 7, 9)),
    Spec("t-n14336", "teams", 14336, 306, "Damping", False, 16, 2, team=True, expect=32, shape=(2, 9, 17)),
    Spec("t-n3136-off", "teams", 3136, 285, "TV", True, 5, 3, team=True, expect=0, shape=(3, 5, 19)),
    Spec("t-n14337-off", "teams", 14337, 273, "Smoothness", False, 5, 2, team=True, expect=0, shape=(1, 13, 21)),
    # tiles per range 1 .. 4 (the loop unrolled by three, two tiles of lag), the last range short
    Spec("t-tpr1", "teams", 3137, ("tpr", 1), "Damping", True, 5, 2, team=True, expect=8),
    Spec("t-tpr2", "teams", 3137, ("tpr", 2), "MS", False, 16, 2, team=True, expect=8),
    Spec("t-tpr3", "teams", 3137, ("tpr", 3), "Smoothness", True, 5, 2, team=True, expect=8),
    Spec("t-tpr4", "teams", 3137, ("tpr", 4), "TV", False, 5, 2, team=True, expect=8),
    Spec("t-one-tile", "teams", 3585, 7, "MS", True, 16, 3, team=True, expect=9),
    Spec("t-few-tiles", "teams", 3585, 40, "Smoothness", False, 5, 3, team=True, expect=9, shape=(2, 4, 5)),
]

CASES = TWO_PASS + TEAMS
BY_ID = dict((s.id, s) for s in CASES)


# ----------------------------------------------------------------------------- inputs and oracle trajectories

class Ref(object):
    """What the oracle's chains did: decisions (C, T), out5 (C, T, 5), the states after every trajectory (C, T, M)."""

    def __init__(self, C, T, M):
        self.acc = np.zeros((C, T), dtype=bool)
        self.out5 = np.zeros((C, T, 5))
        self.xs = np.zeros((C, T, M))


def _problem(orc, data, A):
    Aw, wm = orc.col_weight(A, 0.5)
    P = orc.Problem(Aw, data.dobs, 0.001 * wm, data.reg, data.alpha, data.beta, wm=wm, shape=data.shape,
                    grav_fix=data.gfix)
    return P, wm


def replay(P, data):
    """The case's trajectories (its L, p0, u) on the problem P: a Ref."""
    ref = Ref(data.C, data.T, data.M)
    for c in range(data.C):
        x = data.x0s[c]
        for t in range(data.T):
            x, acc, o, _ = P.leapfrog(x, data.p0s[c, t], data.dt, int(data.Ls[c, t]), data.low, data.high,
                                      float(data.us[c, t]))
            ref.acc[c, t], ref.out5[c, t], ref.xs[c, t] = acc, o, x
    return ref


def before(data, ref, c, t):
    return data.x0s[c] if t == 0 else ref.xs[c, t - 1]


def distance(data, ref, other):
    """The largest difference between two results in the quantities the device test compares: decisions, out5, x and
    the displacement of every trajectory, each in relmax."""
    if not np.array_equal(ref.acc, other.acc):
        return np.inf
    worst = 0.0
    for c in range(data.C):
        for t in range(data.T):
            x0 = before(data, ref, c, t)
            worst = max(worst, relmax(other.out5[c, t], ref.out5[c, t]), relmax(other.xs[c, t], ref.xs[c, t]))
            if ref.acc[c, t]:
                worst = max(worst, relmax(other.xs[c, t] - x0, ref.xs[c, t] - x0))
    return worst


class Data(object):
    """Inputs of one case at one CU count and the oracle's trajectories."""

    def __init__(self, orc, spec, cus):
        self.spec, self.cus = spec, cus
        N, C, T = spec.N, spec.C, spec.T
        M, shape = spec.size(cus)
        self.N, self.M, self.C, self.T, self.shape, self.reg = N, M, C, T, shape, spec.reg
        rng = np.random.default_rng(sum(map(ord, spec.id)) * 7919 + N)
        self.A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.1, 3.0, size=M))
        self.dobs = rng.normal(size=N) + 1e3
        self.gfix = rng.normal(size=N) * 5 + 40.0 if spec.fix else None
        self.alpha = 0.05 / N if spec.reg == "MS" else 0.5
        self.beta = 0.01
        self.P, self.wm = _problem(orc, self, self.A)
        P = self.P
        xc = rng.uniform(0.3, 0.7, size=M)
        self.dt = dt = stable_dt(P, xc, rng)
        self.low, self.high = xc - 1.5 * dt, xc + 1.5 * dt
        self.x0s = xc + dt * rng.uniform(-1.0, 1.0, size=(C, M))
        self.Ls = np.zeros((C, T), dtype=np.int32)
        self.p0s = np.zeros((C, T, M))
        self.us = np.zeros((C, T))
        self.ref = ref = Ref(C, T, M)
        n_lo = n_hi = 0
        for c in range(C):
            x = self.x0s[c]
            for t in range(T):
                want = (c + t) % 2 == 0
                for attempt in range(60):
                    L = int(rng.integers(1, 7))
                    scale = 0.7 ** attempt if want else 2.0 + 0.5 * attempt
                    p0 = rng.normal(size=M) * scale
                    o = P.leapfrog(x, p0, dt, L, self.low, self.high, 0.5)[2]
                    dH = o[4] - o[3]
                    if (want and dH < 5.0) or (not want and dH > 0.01):
                        break
                else:
                    raise AssertionError("%s: no trajectory for the decision %r" % (spec.id, want))
                u = metropolis_u(dH, want)
                # the cells the first drift pushes past a bound (clamped, momentum reflected)
                xs = x + dt * (p0 - 0.5 * dt * P.misfit_and_grad(x)[1])
                n_lo += int((xs < self.low).sum())
                n_hi += int((xs > self.high).sum())
                xn, acc, o, _ = P.leapfrog(x, p0, dt, L, self.low, self.high, u)
                assert acc == want
                self.Ls[c, t], self.p0s[c, t], self.us[c, t] = L, p0, u
                ref.acc[c, t], ref.out5[c, t], ref.xs[c, t] = acc, o, xn
                x = xn
        self.clamped = (n_lo, n_hi)
        self.check()

    def check(self):
        """The generator's own conditions."""
        ref = self.ref
        assert ref.acc.any() and not ref.acc.all(), self.spec.id
        if self.C > 1:      # (one chain cannot disagree with itself)
            assert any(ref.acc[:, t].any() and not ref.acc[:, t].all() for t in range(self.T)), self.spec.id
            # slots idle while others step
            assert any(len(set(self.Ls[:, t])) > 1 for t in range(self.T)), self.spec.id
        assert self.clamped[0] > 0 and self.clamped[1] > 0, (self.spec.id, self.clamped)
        for c in range(self.C):
            for t in range(self.T):
                if not ref.acc[c, t]:
                    assert np.array_equal(ref.xs[c, t], before(self, ref, c, t))

    def probes(self):
        """The two entries of A the sensitivity is measured at."""
        ld = roundup16(self.N)
        return ((self.N - 1, self.M - 1), (ld - 16, 16 * (cdiv(self.M, 16) - 1)))

    def perturbed(self, orc, entry, delta):
        """The oracle's results with A[entry] scaled by 1 + delta (weights, mwapr and all)."""
        A = self.A.copy(order="F")
        A[entry] *= 1.0 + delta
        return replay(_problem(orc, self, A)[0], self)


@functools.lru_cache(maxsize=4)
def _cached(cid, cus):
    from oracle import oracle
    return Data(oracle, BY_ID[cid], cus)


def make(cid, cus):
    """The case's Data (generated once; treat it as read-only)."""
    return _cached(cid, cus)
