"""The cases of the bootstrap CG batch (Engine.bscg_run, csrc/bscg.hip.h, csrc/host_bscg.h) against the CPU oracle
(tests/test_gpu_bscg_oracle.py on the device, tests/test_bscg_oracle_host.py for the generator itself): the case
table, the launch arithmetic of bscg_run restated from the CU count (on the plans of tests/batch_oracle_cases.py), and
the generator of inputs and oracle runs.

A case is a random Fortran-ordered matrix (column scales over 0.1 .. 3, weighted with 0.5), data = the forward of a
model drawn uniformly in (0.05, 0.95) plus 0.05 normal noise, B rows of bootstrap draw counts (a multinomial draw of N
out of N: about a third of the rows 0, some >= 3; the probed rows >= 1 in every replicate), the start model 0.5 and
the bounds (0, 1) unless the case says otherwise.  Everything the device is compared with comes from
oracle.cg_port.bootstrap_counts in float64 on the oracle's own col_weight of the matrix, before an engine is touched.

DELTA: the relative change of ONE entry of the weighted matrix that moves the oracle's results by more than
100 TOL_BSCG (the host test checks it at two entries per case: last valid row / last column, and first row of the last
16-row patch / first column of the last tile).  It states how sharp the comparison is: a kernel that misreads one
such entry by that much fails its case."""
import functools

import numpy as np

from batch_oracle_cases import TOL_TRAJ, cdiv, column_block_M, more_pairs_M, roundup16, team_plan, two_pass_plan
from helpers import relmax

TOL_BSCG = TOL_TRAJ   # the project's trajectory bound
DELTA = 1e-4          # per case unless the table says otherwise
NAMES = ("models", "dmis", "mmis", "alpha")
BETA2 = 0.01          # beta = 0.1, squared (BootStrap's MS stabiliser)


def plan(N, M, cus, team):
    """What bscg_run launches: batch_alloc's partition (two_pass_plan; n_waves enlarged to members x ranges, rounded
    up to a multiple of 4, where bteam_plan is on (`team`: GRAVHMC_BATCH_TEAM at its default) -- the adjoint's grid and the rows bscg_mu_kernel sums), nblk
    workgroups of 16 cells for the direction and step kernels and their passes, the passes of the 1024-thread loops
    over N (bscg_kstep_kernel) and ld (bscg_residual_kernel)."""
    p, tp = dict(two_pass_plan(N, M, cus)), team_plan(N, M, cus)
    if not team:
        tp = {"members": 0, "ranges": 0}
    p["members"], p["ranges"] = tp["members"], tp["ranges"]
    p["adjoint_waves"] = max(p["n_waves"], cdiv(tp["members"] * tp["ranges"], 4) * 4)
    p["nblk"] = min(1024, p["ntiles"])
    p["cell_passes"] = cdiv(p["ntiles"], p["nblk"])
    p["n_passes"], p["ld_passes"] = cdiv(N, 1024), cdiv(p["ld"], 1024)
    return p


# ----------------------------------------------------------------------------- the case table

class Spec(object):
    def __init__(self, cid, group, N, M, B, maxk, q, colmajor=False, team=False, delta=DELTA, seed=0, bounds=(0.0, 1.0),
                 stops=False):
        self.id, self.group, self.N, self.M, self.B, self.maxk, self.q = cid, group, N, M, B, maxk, q
        self.colmajor, self.team, self.delta, self.seed, self.bounds = colmajor, team, delta, seed, bounds
        self.stops = stops      # the case means some of its replicates to pass the stop test

    def size(self, cus):
        if self.M == "colblocks":
            return column_block_M(self.N, cus)
        if self.M == "pairs":
            return more_pairs_M(cus)
        return self.M


# B rotates over 1, 5, 15, 16, maxk over 2, 3, 5 and q over 0.9, 0.5
TABLE = [
    # row patches of 16 at M = 33: np = 1, 1, 1, 2, 2, 3, 4, 7 (the adjoint's ring of three, Rt's transposition)
    Spec("p-n1", "patches", 1, 33, 1, 2, 0.9, seed=1),
    Spec("p-n15", "patches", 15, 33, 5, 3, 0.5),
    Spec("p-n16", "patches", 16, 33, 15, 5, 0.9),
    Spec("p-n17", "patches", 17, 33, 16, 2, 0.5),
    Spec("p-n32", "patches", 32, 33, 1, 3, 0.9),
    Spec("p-n33", "patches", 33, 33, 5, 5, 0.5),
    Spec("p-n49", "patches", 49, 33, 15, 2, 0.9),
    Spec("p-n97", "patches", 97, 33, 16, 3, 0.5),
    # column tiles at N = 49: a single tile, a pair without its second tile, partial and full last tiles
    Spec("c-m1", "tiles", 49, 1, 1, 5, 0.9),
    Spec("c-m15", "tiles", 49, 15, 5, 2, 0.5),
    Spec("c-m16", "tiles", 49, 16, 15, 3, 0.9),
    Spec("c-m17", "tiles", 49, 17, 16, 5, 0.5, colmajor=True),
    Spec("c-m32", "tiles", 49, 32, 1, 2, 0.9),
    Spec("c-m33", "tiles", 49, 33, 5, 3, 0.5),
    Spec("c-m47", "tiles", 49, 47, 15, 5, 0.9, colmajor=True),
    Spec("c-m48", "tiles", 49, 48, 16, 2, 0.5),
    # forward row blocks of 512 and the 1024-thread strides of bscg_kstep_kernel / bscg_residual_kernel
    Spec("r-n511", "rowblocks", 511, 117, 1, 3, 0.9),
    Spec("r-n513", "rowblocks", 513, 110, 5, 5, 0.5, colmajor=True, seed=1),
    Spec("r-n1023", "rowblocks", 1023, 75, 15, 2, 0.9),
    Spec("r-n1024", "rowblocks", 1024, 126, 16, 3, 0.5),
    Spec("r-n1025", "rowblocks", 1025, 75, 1, 5, 0.9),
    Spec("r-n2049", "rowblocks", 2049, 90, 5, 2, 0.5),
    # grid-stride of bscg_direction_kernel / bscg_step_kernel: nblk = 1024 exactly, then one cell, one tile, a full
    # second pass and the start of a third
    Spec("s-m16384", "stride", 20, 16384, 15, 3, 0.9, seed=1),
    Spec("s-m16385", "stride", 20, 16385, 16, 5, 0.5),
    Spec("s-m16400", "stride", 20, 16400, 1, 2, 0.9),
    Spec("s-m32790", "stride", 20, 32790, 5, 3, 0.5),
    # column blocks of the forward with a short last block; more pairs of tiles than the adjoint has waves
    Spec("b-n5003", "colblocks", 5003, "colblocks", 5, 2, 0.9),
    Spec("w-n20", "colblocks", 20, "pairs", 1, 3, 0.5, seed=8),
    # bteam_plan on in the context (GRAVHMC_BATCH_TEAM at its default)
    Spec("t-n3585", "teams", 3585, 203, 15, 3, 0.9, team=True, seed=12),
    Spec("t-n14336", "teams", 14336, 198, 5, 2, 0.5, team=True, seed=1),
]
BY_ID = dict((s.id, s) for s in TABLE)

# the recurrence's branches and the slots: one group of 16
BRANCH = Spec("branch", "branches", 49, 47, 16, 6, 0.5, bounds=(0.2, 0.8), stops=True, seed=18)


# ----------------------------------------------------------------------------- inputs and oracle runs

def distance(ref, other):
    """The largest difference between two runs in the quantities the device test compares (models, dmis, mmis,
    alpha, each in relmax), over the replicates whose lengths did not change."""
    same = (ref.n_entries == other.n_entries) & (ref.n_alpha == other.n_alpha)
    if not same.any():
        return 0.0
    return max(relmax(o[same], r[same]) for r, o in zip(ref.results(), other.results()))


def draw_counts(rng, B, N):
    return rng.multinomial(N, np.full(N, 1.0 / N), size=B).astype(np.float64)


class Data(object):
    """Inputs of one case at one CU count and the oracle's run of its group."""

    def __init__(self, orc, cg_port, spec, cus):
        self.spec, self.cus = spec, cus
        N, B = spec.N, spec.B
        M = spec.size(cus)
        self.N, self.M, self.B, self.maxk, self.q = N, M, B, spec.maxk, spec.q
        self.low, self.high = spec.bounds
        rng = np.random.default_rng(sum(map(ord, spec.id)) * 7919 + N + 1000003 * spec.seed)
        self.A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.1, 3.0, size=M))
        self.Aw, self.wm = orc.col_weight(self.A, 0.5)
        self.m_true = rng.uniform(0.05, 0.95, size=M)
        self.dobs = self.Aw @ (self.wm * self.m_true) + 0.05 * rng.normal(size=N)
        self.mw0 = self.wm * np.full(M, 0.5)
        self.counts = self.draw(rng)
        self.adjust(rng)
        self._port = cg_port
        self.ref = self.run(self.Aw, self.counts)

    def draw(self, rng):
        counts = draw_counts(rng, self.B, self.N)
        for row, _ in self.probes():   # (a perturbed entry in a row the draw dropped moves nothing)
            counts[:, row] = np.maximum(counts[:, row], 1.0)
        return counts

    def adjust(self, rng):
        pass

    def run(self, Aw, counts, dtype=np.float64, maxk=None):
        return self._port.bootstrap_counts(Aw, self.wm, counts, self.dobs, self.mw0, (self.low, self.high), BETA2,
                                           self.q, maxk or self.maxk, dtype=dtype)

    def probes(self):
        """The two entries of Aw the sensitivity is measured at."""
        ld = roundup16(self.N)
        return ((self.N - 1, self.M - 1), (ld - 16, 16 * (cdiv(self.M, 16) - 1)))

    def perturbed(self, entry, delta):
        """The oracle's run with Aw[entry] scaled by 1 + delta."""
        Aw = self.Aw.copy(order="F")
        Aw[entry] *= 1.0 + delta
        return self.run(Aw, self.counts)


class BranchData(Data):
    """The branch case.  The reference's step is twice the minimiser's, so a replicate's data term falls slowly and
    passes the stop test only where it is small from the start: the observations of BRANCH_FITTED are the forward of
    the start model plus 0.02 normal noise, and slot 0 counts each of them once and nothing else -- data < 0.05 at
    k = 1, frozen there while the ordinary draws in the other 15 slots run to the end.

    LATE: the one kind of replicate found to freeze at a later k (one observation counted 30 times: the regularised
    steps fit it by k = 3).  Its Iw = I + mu Iw_old cancels to rounding, float64 and longdouble runs of it differ by
    5e-10, so it is no case at TOL_BSCG; it rides in the group of 3 of the slot checks, which compare bits and
    lengths only."""

    def draw(self, rng):
        counts = Data.draw(self, rng)
        counts[0] = 0.0
        counts[0, BRANCH_FITTED] = 1.0
        return counts

    def adjust(self, rng):
        self.dobs[BRANCH_FITTED] = (self.Aw @ self.mw0)[BRANCH_FITTED] + 0.02 * rng.normal(size=BRANCH_FITTED.size)

    def group_of_three(self):
        """Other counts: LATE, the fitted observations counted twice, an ordinary draw."""
        rng = np.random.default_rng(4711)
        counts = Data.draw(self, rng)[:3]
        counts[0] = BRANCH_LATE[1] * (np.arange(self.N) == BRANCH_LATE[0])
        counts[1] = 0.0
        counts[1, BRANCH_FITTED] = 2.0
        return counts


BRANCH_FITTED = np.arange(0, 48, 4)
BRANCH_LATE = (43, 30.0)


@functools.lru_cache(maxsize=4)
def _cached(cid, cus):
    from oracle import cg_port, oracle
    if cid == BRANCH.id:
        return BranchData(oracle, cg_port, BRANCH, cus)
    return Data(oracle, cg_port, BY_ID[cid], cus)


def make(cid, cus):
    """The case's Data (generated once; treat it as read-only)."""
    return _cached(cid, cus)
