"""The cases of the bootstrap batch on the translation-invariant store (Engine.set_translation_invariant("replicates"),
csrc/latbatch.hip.h: latb_pass_kernel<LATB_CG>, csrc/host_bscg.h) against the CPU oracle: test_lattice_bscg_host.py
checks the generator itself, test_gpu_lattice_bscg.py runs the device.  Geometry, the lattice, the restated operator and
the plan come from lattice_batch_cases.py.

A case is one of that module's PASS_CASES (or BIG) with
    m_true ~ U(0.05, 0.95),  dobs = Aw (wm m_true) + 0.02 max|.| N(0, 1),
    counts: B multinomial draws of N out of N (the probed rows >= 1 in every replicate),
    mw0 = 0.5 wm, bounds (0, 1), beta2 = 0.01,
B rotating over 1, 5, 15, 16, maxk over 2, 3, 5 and q over 0.9, 0.5 down the sorted names, seeds SEED0 + i.  Aw is the
restated operator: the oracle's prism_gz_kernel, its table (table_of), expanded again, column-weighted with the
oracle's weights -- what test_gpu_lattice_batch.py::reference builds.  Everything the device is compared with comes from
oracle.cg_port.bootstrap_counts in float64, before an engine is touched.

DELTA: the relative change of ONE entry of Aw at which the oracle's results must move by more than 100 TOL_BSCG (two
entries per case: last row / last column, and the largest entry of the first tile, rows and columns below 16).  BIG is
exempt: one entry among its 16 900 x 800 scaled by 1e-4 moves nothing by that much, and its passes' edges are those of
the small cases."""
import functools

import numpy as np

from helpers import relmax
import lattice_batch_cases as lb
from lattice_cases import geometry

TOL_BSCG = 1e-10      # the project's trajectory bound (bscg_oracle_cases.TOL_BSCG)
DELTA = 1e-4
BETA2 = 0.01
NAMES = ("models", "dmis", "mmis", "alpha")
SEED0 = 100
STOP = 0.1            # the stop test's threshold (data < 0.1)

CASE_NAMES = tuple(sorted(lb.PASS_CASES))
_B, _MAXK, _Q = (1, 5, 15, 16), (2, 3, 5), (0.9, 0.5)
#: name -> (B, maxk, q, seed)
PARAMS = dict((name, (_B[i % 4], _MAXK[i % 3], _Q[i % 2], SEED0 + i)) for i, name in enumerate(CASE_NAMES))
#: 16 900 rows, N not a multiple of 16 (lattice_batch_cases.BIG)
PARAMS["big"] = (5, 2, 0.9, SEED0 + len(CASE_NAMES))
#: the recurrence's branches and the slots, at "beyond": one group of 16
BRANCH = "branch"
PARAMS[BRANCH] = (16, 6, 0.5, SEED0 + len(CASE_NAMES) + 1)
BRANCH_BOUNDS = (0.2, 0.8)


def kwargs_of(name):
    return lb.BIG if name == "big" else lb.PASS_CASES["beyond" if name == BRANCH else name]


def draw_counts(rng, B, N):
    return rng.multinomial(N, np.full(N, 1.0 / N), size=B).astype(np.float64)


def recipe(rng, Aw, wm, B, probe_rows=(), scale=1.0):
    """dobs, counts, mw0 of the module's recipe on a weighted operator (scale: the models' unit, for bounds (0, scale))"""
    N, M = Aw.shape
    m_true = scale * rng.uniform(0.05, 0.95, size=M)
    d0 = Aw @ (wm * m_true)
    dobs = d0 + 0.02 * np.abs(d0).max() * rng.normal(size=N)
    counts = draw_counts(rng, B, N)
    for row in probe_rows:  # (a perturbed entry in a row the draw dropped moves nothing)
        counts[:, row] = np.maximum(counts[:, row], 1.0)
    return dobs, counts, 0.5 * scale * wm


def operator(orc, obs, b6):
    """The restated weighted operator (N x M, Fortran order), the oracle's weights and the lattice's dims"""
    A, wm = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))  # (A: weighted)
    dims, col, ool = lb.lattice(obs, b6)
    T = lb.table_of(A * wm[None, :], dims, col, ool)
    Aw = np.asfortranarray(lb.expanded(T, dims, col, ool) * (1.0 / wm)[None, :])
    return Aw, wm, dims


class Data(object):
    """Inputs of one case and the oracle's run of its group"""

    def __init__(self, orc, cg_port, name):
        self.name = name
        self.B, self.maxk, self.q, self.seed = PARAMS[name]
        self.low, self.high = BRANCH_BOUNDS if name == BRANCH else (0.0, 1.0)
        self.obs, self.b6 = geometry(**kwargs_of(name))
        self.Aw, self.wm, self.dims = operator(orc, self.obs, self.b6)
        self.N, self.M = self.Aw.shape
        rng = np.random.default_rng(self.seed)
        first = np.abs(self.Aw[:16, :16])
        self._first = tuple(int(v) for v in np.unravel_index(int(first.argmax()), first.shape))
        self.dobs, self.counts, self.mw0 = recipe(rng, self.Aw, self.wm, self.B, [r for r, _ in self.probes()])
        if name == BRANCH:
            # slot 0 counts only observations fitted from the start: data < 0.1 at k = 1, frozen there while the ordinary
            # draws of the other 15 slots run to the end (bscg_oracle_cases.BranchData)
            fitted = np.arange(0, self.N, 4)
            self.dobs[fitted] = (self.Aw @ self.mw0)[fitted] + 0.02 * rng.normal(size=fitted.size)
            self.counts[0] = 0.0
            self.counts[0, fitted] = 1.0
        self._port = cg_port
        for a in (self.obs, self.b6, self.Aw, self.wm, self.dobs, self.counts, self.mw0):
            a.setflags(write=False)
        self.ref = self.run(self.Aw, self.counts)

    def run(self, Aw, counts, dtype=np.float64, maxk=None):
        return self._port.bootstrap_counts(Aw, self.wm, counts, self.dobs, self.mw0, (self.low, self.high), BETA2, self.q,
                                           maxk or self.maxk, dtype=dtype)

    def probes(self):
        """The two entries of Aw the sensitivity is measured at: last row / last column, the largest of the first tile"""
        return ((self.N - 1, self.M - 1), self._first)

    def perturbed(self, entry, delta):
        Aw = self.Aw.copy(order="F")
        Aw[entry] *= 1.0 + delta
        return self.run(Aw, self.counts)

    def group_of_three(self):
        """Slots 0, 3 and 7 of the branch group as a group of their own: the frozen replicate and two ordinary draws"""
        return np.ascontiguousarray(self.counts[[0, 3, 7]]), [0, 3, 7]


def distance(ref, other):
    """The largest difference between two runs in the quantities the device test compares, over the replicates whose
    lengths did not change"""
    same = (ref.n_entries == other.n_entries) & (ref.n_alpha == other.n_alpha)
    if not same.any():
        return 0.0
    return max(relmax(o[same], r[same]) for r, o in zip(ref.results(), other.results()))


def conditions(d, sharp=True):
    """What the host test enforces of a case, from the oracle alone: float64 / longdouble spread, the smallest alpha-rule
    margin, the smallest distance of a data value from the stop threshold, whether a clamp acted, and (sharp) how far
    the two probes move the results"""
    ref = d.ref
    ld = d.run(d.Aw, d.counts, dtype=np.longdouble)
    assert np.array_equal(ld.n_entries, ref.n_entries) and np.array_equal(ld.n_alpha, ref.n_alpha)
    spread = max(relmax(v, np.asarray(w, dtype=np.float64)) for v, w in zip(ref.results(), ld.results()))
    margins = [abs(m) for tr in ref.trace for m in tr["margin"].values()]
    stops = [abs(v - STOP) for tr in ref.trace for v in tr["seen"]]
    clamped = sum(lo + hi for tr in ref.trace for lo, hi in tr["clamped"])
    moved = [distance(ref, d.perturbed(e, DELTA)) for e in d.probes()] if sharp else []
    return dict(spread=spread, margin=min(margins) if margins else np.inf, stop=min(stops) if stops else np.inf,
                clamped=clamped, moved=moved)


@functools.lru_cache(maxsize=None)
def make(name):
    """The case's Data (generated once; read-only)"""
    from oracle import cg_port, oracle
    return Data(oracle, cg_port, name)
