"""The cases of a REUSED context against the CPU oracle (tests/test_gpu_context_lifecycle.py on the device,
tests/test_lifecycle_host.py for the generator itself).  No device.

Every other suite creates a context, configures it once in the documented order, runs it and closes it.  Here a
context gets a second kernel, weights after a batch or a stream exists, a second compression.  A context holds
stores DERIVED from its kernel or its weights; four of them once survived a change of what they were made from:

    bt.Gb   the MFMA operand-order copy of G the two-pass batch adjoint (and bscg_run's) contracts
    wv      the wavelet rows (CSR) of the compressed forward and their dense form wv.F of the resident kernel
    cg.sw   the cross-gradient normalisers 1 / (wm scale)
    ps.iw   the posterior stream's 1 / wm

Two problems A and B share (N, M) and differ in geometry and data: gz of prisms, the kernel from
oracle.prism_gz_kernel (what upload_G gets; build_G assembles the same geometry on the device).  Everything the
device is compared with comes from the oracle on the FINAL configuration, before an engine is touched.

Beside the oracle's results the module restates in NumPy what a device with the STALE store would compute, one
restatement per store (stale_*): used only by the host test, which requires every one of them to lie at least SHARP
= 1e-6 (relative) from the oracle's result on B in every quantity the device test compares, under that test's bound
of TOL = 1e-10: a stale store cannot hide.  The variate u of a trajectory sits half-way between the oracle's
exp(-dH) and 0 or 1; a rejection is used only where dH > 0.01 (Metropolis margin |log u + dH| >= MARGIN)."""
import functools

import numpy as np

from crossgrad_host import JointHostProblem, cross_gradient, relative_spacings
from helpers import metropolis_u, relmax, stable_dt
from poststream_host import Stream

TOL = 1e-10
SHARP = 1e-6
MARGIN = 1e-6


# ----------------------------------------------------------------------------- geometry

def prisms(extent, shape):
    """(M, 6) bounds x1, x2, y1, y2, z1, z2 of a regular mesh (nz, ny, nx) on extent, x fastest."""
    x0, x1, y0, y1, z0, z1 = [float(v) for v in extent]
    nz, ny, nx = shape
    xe, ye, ze = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1), np.linspace(z0, z1, nz + 1)
    out = np.empty((nz, ny, nx, 6))
    out[..., 0], out[..., 1] = xe[None, None, :-1], xe[None, None, 1:]
    out[..., 2], out[..., 3] = ye[None, :-1, None], ye[None, 1:, None]
    out[..., 4], out[..., 5] = ze[:-1, None, None], ze[1:, None, None]
    return np.ascontiguousarray(out.reshape(-1, 6))


class Spec(object):
    """One (N, M) with its two geometries: A and B differ in the cells' extent, the points and their height."""

    def __init__(self, cid, N, shape, reg, fix, C=4, T=3):
        self.id, self.N, self.shape, self.reg, self.fix, self.C, self.T = cid, N, tuple(shape), reg, fix, C, T
        self.M = shape[0] * shape[1] * shape[2]


SPECS = [
    # the two-pass MFMA batch: ld = N, three row patches of 16 / padded ld with a ragged last tile of 16 columns
    Spec("two-pass-48x200", 48, (4, 5, 10), "Smoothness", True),
    Spec("two-pass-37x203", 37, (1, 7, 29), "MS", False),
    # the smallest shape of tests/batch_oracle_cases.py that takes batch_team_kernel (t-one-tile: 9 members, one tile)
    Spec("team-3585x7", 3585, (1, 1, 7), "TV", True),
    # the wavelet rows: (4, 6, 8) in 3-D, then 1-D over the same 192 cells
    Spec("wavelet-37x192", 37, (4, 6, 8), "MS", False, C=1, T=6),
    # the posterior stream: M = 120
    Spec("stream-30x120", 30, (3, 5, 8), "Damping", False, C=1, T=8),
    # the folded store: the smallest symmetric grid of tests/fold_oracle_cases.py (U-2x2: 2 x 2 points, 2 x 4 x 2 cells)
    Spec("fold-4x16", 4, (2, 4, 2), "Damping", False, C=1, T=6),
]
BY_ID = dict((s.id, s) for s in SPECS)

GEOMETRY = {
    # cells' extent, the rectangle of the points, their height above z = 0 (z grows downwards)
    "A": ((0.0, 2000.0, 0.0, 3000.0, 0.0, 1000.0), (0.0, 2000.0, 0.0, 3000.0), 0.0),
    "B": ((-300.0, 1500.0, 400.0, 2600.0, 150.0, 1900.0), (-500.0, 1800.0, 200.0, 3100.0), -120.0),
}


class Problem(object):
    """Geometry `which` of a spec: points, cells, the oracle's kernel K and weighted kernel Aw, data of a sparse
    model plus noise on a level of 100, the regulariser's parameters."""

    def __init__(self, orc, spec, which, geometry=None):
        self.spec, self.which = spec, which
        N, M = spec.N, spec.M
        rng = np.random.default_rng(sum(map(ord, spec.id + which)) * 7919 + N)
        if geometry is not None:        # (points (3, N) and cells (M, 6) of the caller's)
            self.obs, self.cells = tuple(np.ascontiguousarray(v) for v in geometry[0]), np.ascontiguousarray(geometry[1])
        else:
            extent, rect, height = GEOMETRY[which]
            self.cells = prisms(extent, spec.shape)
            self.obs = (rng.uniform(rect[0], rect[1], N), rng.uniform(rect[2], rect[3], N),
                        np.full(N, height) - rng.uniform(0.0, 40.0, N))
        self.K = np.asfortranarray(orc.prism_gz_kernel(*self.obs, self.cells))
        self.Aw, self.wm = orc.col_weight(self.K, 0.5)
        m_true = np.where(rng.uniform(size=M) < 0.2, rng.uniform(0.2, 1.0, size=M), 0.0)
        d = self.K @ m_true
        self.dobs = d + 0.05 * np.abs(d).max() * rng.normal(size=N) + 100.0
        self.gfix = (rng.normal(size=N) * 0.2 * np.abs(d).max() + 3.0) if spec.fix else None
        self.reg, self.shape, self.beta = spec.reg, spec.shape, 0.01
        self.alpha = 0.05 / N if spec.reg == "MS" else 0.5
        self.mwapr = 0.001 * self.wm
        self.orc = orc

    def oracle(self, weighted=True, reg=None, mwapr=None, **kw):
        """oracle.Problem of this geometry: on the weighted kernel, or on K itself (no weights: not with MS)."""
        if weighted:
            return self.orc.Problem(self.Aw, self.dobs, self.mwapr if mwapr is None else mwapr, reg or self.reg,
                                    self.alpha, self.beta, wm=self.wm, shape=self.shape, grav_fix=self.gfix, **kw)
        return self.orc.Problem(self.K, self.dobs, self.mwapr if mwapr is None else mwapr, reg or self.reg, self.alpha,
                                self.beta, shape=self.shape, grav_fix=self.gfix, **kw)


# ----------------------------------------------------------------------------- trajectories

class Ref(object):
    """What chains did: decisions (C, T), out5 (C, T, 5), the states after every trajectory (C, T, M)."""

    def __init__(self, C, T, M):
        self.acc = np.zeros((C, T), dtype=bool)
        self.out5 = np.zeros((C, T, 5))
        self.xs = np.zeros((C, T, M))


class Chains(object):
    """C chains with their own starts in one box of +-1.5 dt and T rounds of trajectories on the potential P (anything
    with misfit_and_grad and leapfrog): in every round the chains' lengths differ, decisions alternate over chains
    and rounds.  ref: P's own results; margin: the smallest |log u + dH| met."""

    def __init__(self, P, M, C, T, seed, centre=None):
        rng = np.random.default_rng(seed)
        self.M, self.C, self.T = M, C, T
        xc = rng.uniform(0.3, 0.7, size=M) if centre is None else centre
        self.dt = dt = stable_dt(P, xc, rng)
        self.low, self.high = xc - 1.5 * dt, xc + 1.5 * dt
        self.x0s = xc + dt * rng.uniform(-1.0, 1.0, size=(C, M))
        self.Ls = np.zeros((C, T), dtype=np.int32)
        self.p0s = np.zeros((C, T, M))
        self.us = np.zeros((C, T))
        self.ref = Ref(C, T, M)
        self.margin = np.inf
        for c in range(C):
            x = self.x0s[c]
            for t in range(T):
                want = (c + t) % 2 == 0
                L = 1 + (2 * c + t) % 6
                for attempt in range(60):
                    p0 = rng.normal(size=M) * (0.7 ** attempt if want else 2.0 + 0.5 * attempt)
                    o = P.leapfrog(x, p0, dt, L, self.low, self.high, 0.5)[2]
                    dH = o[4] - o[3]
                    if (want and dH < 5.0) or (not want and dH > 0.01):
                        break
                else:
                    raise AssertionError("no trajectory for the decision %r" % want)
                u = metropolis_u(dH, want)
                self.margin = min(self.margin, abs(np.log(u) + dH))
                self.Ls[c, t], self.p0s[c, t], self.us[c, t] = L, p0, u
                out = P.leapfrog(x, p0, dt, L, self.low, self.high, u)
                assert bool(out[1]) == want
                x = np.array(out[0], dtype=np.float64)
        self.ref = replay(P, self)
        self.check()

    def check(self):
        ref = self.ref
        assert ref.acc.any() and not ref.acc.all()
        assert self.margin >= MARGIN, self.margin
        for c in range(self.C):
            for t in range(self.T):
                assert bool(ref.acc[c, t]) == ((c + t) % 2 == 0)
                if not ref.acc[c, t]:
                    assert np.array_equal(ref.xs[c, t], before(self, ref, c, t))
        if self.C > 1:
            assert all(len(set(self.Ls[:, t])) > 1 for t in range(self.T))


def replay(P, ch):
    """ch's trajectories (its starts, L, p0, u) on the potential P: a Ref."""
    ref = Ref(ch.C, ch.T, ch.M)
    for c in range(ch.C):
        x = ch.x0s[c]
        for t in range(ch.T):
            out = P.leapfrog(x, ch.p0s[c, t], ch.dt, int(ch.Ls[c, t]), ch.low, ch.high, float(ch.us[c, t]))
            x = np.array(out[0], dtype=np.float64)
            ref.acc[c, t], ref.out5[c, t], ref.xs[c, t] = out[1], out[2], x
    return ref


def before(ch, ref, c, t):
    return ch.x0s[c] if t == 0 else ref.xs[c, t - 1]


def distances(ch, ref, other):
    """How far `other` lies from `ref` in each quantity the device test compares: per chain the largest relmax over its
    trajectories, then the SMALLEST of these over the chains (every chain has to see the difference).  A decision that
    differs counts as inf."""
    if not np.array_equal(ref.acc, other.acc):
        return {"out5": np.inf, "x": np.inf, "displacement": np.inf}
    out = {}
    for key in ("out5", "x", "displacement"):
        per_chain = []
        for c in range(ch.C):
            worst = 0.0
            for t in range(ch.T):
                if key == "out5":
                    worst = max(worst, relmax(other.out5[c, t], ref.out5[c, t]))
                elif key == "x":
                    worst = max(worst, relmax(other.xs[c, t], ref.xs[c, t]))
                elif ref.acc[c, t]:
                    x0 = before(ch, ref, c, t)
                    worst = max(worst, relmax(other.xs[c, t] - x0, ref.xs[c, t] - x0))
            per_chain.append(worst)
        out[key] = min(per_chain)
    return out


# ----------------------------------------------------------------------------- the potential with separate operators

class SplitPotential(object):
    """potential.py:812-845 in NumPy with a forward and an adjoint that need not belong together: d = fwd(x),
    r = (d + gfix - mean) - (dobs - mean), U = |r|^2 + alpha R, grad = 2 adj(r) + alpha grad R; the leapfrog of
    hmc.py:85-177 ('mandatory' bounds) on it.  With fwd = Aw @ x and adj = Aw.T @ r: the oracle's potential."""

    def __init__(self, orc, fwd, adj, dobs, gfix, reg, alpha, beta, shape, mwapr, wm=None):
        self.orc, self.fwd, self.adj = orc, fwd, adj
        self.dobs_c = dobs - np.mean(dobs)
        self.gfix, self.reg, self.alpha, self.beta, self.shape, self.mwapr = gfix, reg, alpha, beta, shape, mwapr
        self.wm2 = None if wm is None else wm * wm

    def misfit_and_grad(self, x):
        d = self.fwd(x)
        dinv = d + self.gfix if self.gfix is not None else d
        r = (dinv - np.mean(dinv)) - self.dobs_c
        rv, rg = self.orc.regulariser(self.reg, x, self.mwapr, self.wm2, self.beta, self.shape)
        U_data = float(r @ r)
        return U_data + self.alpha * rv, 2.0 * self.adj(r) + self.alpha * rg, d, U_data, rv

    def leapfrog(self, xcur, p0, dt, L, low, high, u):
        pnew, xnew = p0 * 1.0, xcur * 1.0
        K = np.dot(pnew, pnew) * 0.5
        U, grad, dsyn, U_data, U_model = self.misfit_and_grad(xnew)
        Hcur = K + U
        pnew -= dt * grad * 0.5
        for i in range(L):
            xnew += dt * pnew
            idx1, idx2 = xnew > high, xnew < low
            xnew[idx1], pnew[idx1] = high[idx1], -pnew[idx1]
            xnew[idx2], pnew[idx2] = low[idx2], -pnew[idx2]
            Unew, grad, dsyn_new, Unew_data, Unew_model = self.misfit_and_grad(xnew)
            pnew -= dt * grad if i < L - 1 else dt * grad * 0.5
        Hnew = np.dot(pnew, pnew) * 0.5 + Unew
        if Hnew < Hcur or u < np.exp(-(Hnew - Hcur)):
            return xnew, True, np.array([Unew, Unew_data, Unew_model, Hcur, Hnew]), dsyn_new
        return xcur * 1.0, False, np.array([U, U_data, U_model, Hcur, Hnew]), dsyn


def split(pb, fwd_matrix, adj_matrix, weighted=True, reg=None):
    """pb's potential with the forward of one matrix and the adjoint of another."""
    return SplitPotential(pb.orc, lambda x: fwd_matrix @ x, lambda r: adj_matrix.T @ r, pb.dobs, pb.gfix, reg or pb.reg,
                          pb.alpha, pb.beta, pb.shape, pb.mwapr, pb.wm if weighted else None)


# ----------------------------------------------------------------------------- scenario: kernel A, then kernel B

class TwoKernels(object):
    """The batch (or single chain) scenario: problem A with one round, then problem B with T rounds.
    stale_gb(): the rounds of B with Aw_B in the forward and Aw_A^T in the adjoint (the operand-order copy of A)."""

    def __init__(self, orc, spec):
        self.spec = spec
        self.A, self.B = Problem(orc, spec, "A"), Problem(orc, spec, "B")
        self.PA, self.PB = self.A.oracle(), self.B.oracle()
        self.chA = Chains(self.PA, spec.M, spec.C, 1 if spec.C > 1 else 2, seed=11 + spec.N)
        self.chB = Chains(self.PB, spec.M, spec.C, spec.T, seed=23 + spec.N)

    def stale_gb(self):
        return replay(split(self.B, self.B.Aw, self.A.Aw), self.chB)

    def fresh_split(self):
        """the restatement with nothing stale: must reproduce the oracle"""
        return replay(split(self.B, self.B.Aw, self.B.Aw), self.chB)


class BeforeWeights(object):
    """upload_G, data, reg, batch_init, one round on the UNWEIGHTED kernel; then weight, batch_init, T rounds.
    stale_gb(): the weighted forward with the unweighted adjoint K^T.  (TV: MS needs the weights.)"""

    def __init__(self, orc, spec):
        self.spec = spec
        self.B = Problem(orc, spec, "B")
        self.mwapr = np.full(spec.M, 0.05)       # (given once, before there are weights)
        self.PU = self.B.oracle(weighted=False, reg="TV", mwapr=self.mwapr)
        self.PW = self.B.oracle(weighted=True, reg="TV", mwapr=self.mwapr)
        self.chU = Chains(self.PU, spec.M, spec.C, 1, seed=5 + spec.N)
        self.chW = Chains(self.PW, spec.M, spec.C, spec.T, seed=7 + spec.N)

    def _split(self, adj):
        b = self.B
        return SplitPotential(b.orc, lambda x: b.Aw @ x, lambda r: adj.T @ r, b.dobs, b.gfix, "TV", b.alpha, b.beta,
                              b.shape, self.mwapr, b.wm)

    def stale_gb(self):
        return replay(self._split(self.B.K), self.chW)

    def fresh_split(self):
        return replay(self._split(self.B.Aw), self.chW)


# ----------------------------------------------------------------------------- scenario: bootstrap replicates

BSCG = dict(B=5, maxk=3, q=0.9, beta2=0.01, bounds=(0.0, 1.0))
BSCG_NAMES = ("models", "data misfit", "model misfit", "regularisation factors")


def bscg_split(Afwd, Aadj, wm, counts, dobs, mw0, boundary, beta2, q, maxk):
    """oracle.cg_port.bootstrap_counts in float64 with the products F = Afwd Iw, r = Afwd mw - d of one matrix and the
    adjoint Aadj^T (c o r) of another: what bscg_run computes when its operand-order copy is not the kernel's.
    -> (models, dmis, mmis, alpha) with zeros past the entries a replicate produced."""
    lo, hi = boundary
    N, M = Afwd.shape
    wm2 = wm * wm
    model = lambda mw: np.sum(wm2 * mw * mw / (mw * mw + beta2))                     # noqa: E731
    model_g = lambda mw: 2.0 * wm2 * (mw * beta2) / (mw * mw + beta2) ** 2           # noqa: E731
    B = counts.shape[0]
    out = [np.zeros((B, M)), np.zeros((B, maxk - 1)), np.zeros((B, maxk - 1)), np.zeros((B, maxk))]
    for b, c in enumerate(counts):
        mw = mw0
        r = Afwd @ mw - dobs
        d_cur = np.sum(c * r * r)
        dm, mm, rf = [], [], []
        for k in range(maxk):
            if k == 0:
                alpha = 0.0
            elif k == 1:
                alpha = d_new / model(mw_new)
            elif d_cur - d_new < 0.01 * d_cur:
                alpha = q * alpha
            rf.append(alpha)
            if k > 0:
                I_old, Iw_old = I, Iw
                mw, r, d_cur = mw_new, r_new, d_new
            I = 2.0 * (Aadj.T @ (c * r)) + alpha * model_g(mw)
            Iw = I if k == 0 else I + ((I @ I) / (I_old @ I_old)) * Iw_old
            F = Afwd @ Iw
            kstep = (Iw @ I) / (np.sum(c * F * F) + alpha * (Iw @ Iw))
            m = np.clip((mw - kstep * Iw) / wm, lo, hi)
            mw_new = wm * m
            r_new = Afwd @ mw_new - dobs
            d_new = np.sum(c * r_new * r_new)
            if k > 0:
                if d_new < 0.1:
                    break
                dm.append(d_new / N)
                mm.append(model(mw_new) / M)
        out[0][b] = mw_new / wm
        out[1][b, :len(dm)], out[2][b, :len(mm)], out[3][b, :len(rf)] = dm, mm, rf
    return out


class Bscg(object):
    """bscg_run on kernel A, then on kernel B: B replicates with multinomial draw counts, data of a model inside the
    bounds plus noise (no level: the bootstrap removes no mean).  stale_gb(): the adjoint of A under the forward of B."""

    def __init__(self, orc, cg_port, two):
        self.A, self.B = two.A, two.B
        rng = np.random.default_rng(131)
        N, M = two.spec.N, two.spec.M
        self.runs = []
        for pb in (self.A, self.B):
            dobs = pb.Aw @ (pb.wm * rng.uniform(0.05, 0.95, size=M)) + 0.05 * rng.normal(size=N)
            counts = rng.multinomial(N, np.full(N, 1.0 / N), size=BSCG["B"]).astype(np.float64)
            mw0 = pb.wm * np.full(M, 0.5)
            ref = cg_port.bootstrap_counts(pb.Aw, pb.wm, counts, dobs, mw0, BSCG["bounds"], BSCG["beta2"], BSCG["q"],
                                           BSCG["maxk"])
            self.runs.append({"pb": pb, "dobs": dobs, "counts": counts, "mw0": mw0, "ref": ref})

    def _split(self, Aadj):
        r = self.runs[1]
        return bscg_split(self.B.Aw, Aadj, self.B.wm, r["counts"], r["dobs"], r["mw0"], BSCG["bounds"], BSCG["beta2"],
                          BSCG["q"], BSCG["maxk"])

    def stale_gb(self):
        return self._split(self.A.Aw)

    def fresh_split(self):
        return self._split(self.B.Aw)


# ----------------------------------------------------------------------------- scenario: wavelet rows

WAVELET_THR = 1e-3


class Wavelet(object):
    """Compress A in 3-D; kernel B; compress B in 1-D.  Oracle: B's dense potential in between, B's compressed
    potential (CSR of B in the forward, dense adjoint) afterwards.  stale_*: the CSR of A under the dense adjoint of B."""

    def __init__(self, orc, spec):
        from oracle import wavelet as ow
        self.spec, self.ow = spec, ow
        self.A, self.B = Problem(orc, spec, "A"), Problem(orc, spec, "B")
        rng = np.random.default_rng(41)
        self.xs = [rng.uniform(0.2, 0.8, size=spec.M) for _ in range(2)]
        self.csrA = ow.compress_kernel(self.A.Aw, 3, spec.shape, WAVELET_THR)
        self.csrB = ow.compress_kernel(self.B.Aw, 1, None, WAVELET_THR)
        self.dwtA = lambda v: ow.model_coeffs(v, 3, spec.shape)
        self.dwtB = lambda v: ow.model_coeffs(v, 1)
        self.PB_dense = self.B.oracle()
        self.PB = self.B.oracle(csr=self.csrB, dwt=self.dwtB)
        self.ch = Chains(self.PB, spec.M, 1, spec.T, seed=53)

    def _split(self, csr, dwt):
        b = self.B
        return SplitPotential(b.orc, lambda x: csr @ dwt(x), lambda r: b.Aw.T @ r, b.dobs, b.gfix, b.reg, b.alpha, b.beta,
                              b.shape, b.mwapr, b.wm)

    def stale_potential(self):
        """misfit_and_grad after kernel B with the rows of A still on"""
        return self._split(self.csrA, self.dwtA)

    def stale_chain(self):
        return replay(self._split(self.csrA, self.dwtA), self.ch)

    def fresh_split(self):
        return replay(self._split(self.csrB, self.dwtB), self.ch)


# ----------------------------------------------------------------------------- scenario: cross-gradient normalisers

def joint_weight(A, n, m):
    """gh_weight on a joint store, restated (potential.py:1050-1051, weightKDM): A the stacked 2n x 2m kernel with its
    gz block in [:n, :m] and its tf block in [n:, m:]; wm = the column 2-norms of A, Wb = the tf rows times
    s = std_gz / std_tf (population std of the blocks' entries), Aw = Wb A Wm^-1.
    -> (Aw stacked, wm, (std_gz, std_tf))"""
    gz, tf = A[:n, :m], A[n:, m:]
    std = (float(np.std(gz)), float(np.std(tf)))
    wm = np.concatenate([np.sqrt((gz * gz).sum(axis=0)), np.sqrt((tf * tf).sum(axis=0))])
    Aw = np.zeros_like(A)
    Aw[:n, :m], Aw[n:, m:] = gz / wm[:m], tf * (std[0] / std[1]) / wm[m:]
    return Aw, wm, std


class CrossGrad(object):
    """The joint store of tests/golden/joint_small.npz, geometry a (30 points, 48 cells: the smallest joint mesh of
    the suite) as A.  A joint context keeps its cells (gh_set_cells_joint comes first, once), so B is the same mesh
    under OTHER POINTS: A's points resampled with repetitions -- a kernel the host knows, the rows of A's two blocks
    taken at `idx`, with other block deviations and other column norms.  stale_*: Phi and the chain with sw from A's
    weights."""

    LAM_SHARE = 0.3     # lam Phi as a share of the data term at the chains' centre
    SCALE = (0.5, 2.0)

    def __init__(self, z, mesh):
        m = int(z["a_wm"].size // 2)
        n = int(z["a_xp"].size)
        self.m, self.n = m, n
        self.shape = tuple(int(v) for v in z["a_shape"])
        self.spacing = relative_spacings(mesh)
        rng = np.random.default_rng(77)
        self.A_unweighted = z["a_A"]
        self.AwA, self.wmA, self.stdA = joint_weight(z["a_A"], n, m)
        self.idx = idx = np.sort(rng.integers(0, n, size=n))
        assert len(set(idx.tolist())) < n
        self.obsA = (z["a_xp"], z["a_yp"], z["a_zp"])
        self.obsB = tuple(v[idx] for v in self.obsA)
        self.AwB, self.wmB, self.stdB = joint_weight(z["a_A"][np.concatenate([idx, n + idx])], n, m)
        self.dobswB = z["a_dobsw"][np.concatenate([idx, n + idx])] * 1.1 + 0.01 * np.abs(z["a_dobsw"]).max() * rng.normal(size=2 * n)
        self.reg, self.alpha, self.beta = "Smoothness", 0.8, 0.001
        self.mwaprB = 0.5 * self.wmB
        self.centre = rng.uniform(0.3, 0.7, size=2 * m) * self.wmB
        phi = cross_gradient(self.centre, self.wmB, self.shape, *self.spacing, scale=self.SCALE)[0]
        r = self.AwB @ self.centre - self.dobswB
        self.lam = self.LAM_SHARE * float(r @ r) / phi
        self.mws = [rng.uniform(0.2, 0.8, size=2 * m) * self.wmB for _ in range(2)]
        self.PB = self._problem(self.wmB)
        self.ch = Chains(_Joint4(self.PB), 2 * m, 1, 6, seed=91, centre=self.centre)

    def _problem(self, cg_wm):
        P = _SplitSwJoint(self.AwB, self.dobswB, self.wmB, self.shape, self.reg, self.alpha, self.beta, self.mwaprB,
                          self.lam, self.spacing, self.SCALE)
        P.cg_wm = cg_wm
        return P

    def phi(self, mw, wm):
        return cross_gradient(mw, wm, self.shape, *self.spacing, scale=self.SCALE)

    def stale_chain(self):
        return replay(_Joint4(self._problem(self.wmA)), self.ch)


class _SplitSwJoint(JointHostProblem):
    """JointHostProblem whose coupling takes its normalisers from cg_wm (the regulariser keeps wm)."""
    cg_wm = None

    def misfit_and_grad(self, mw):
        d = self.Aw @ mw
        r = d - self.dobsw
        rv, rg = self.regulariser(mw - self.mwapr)
        U_data = r @ r
        U, grad = U_data + self.alpha * rv, 2 * (self.Aw.T @ r) + self.alpha * rg
        phi, pg, _ = cross_gradient(mw, self.cg_wm, self.shape, *self.spacing, scale=self.scale)
        self.last_phi = phi
        return U + self.lam * phi, grad + self.lam * pg, d, U_data, rv


class _Joint4(object):
    """JointHostProblem behind the (x, accepted, out5, extra) leapfrog of the other potentials."""

    def __init__(self, P):
        self.P = P

    def misfit_and_grad(self, x):
        return self.P.misfit_and_grad(x)

    def leapfrog(self, *a):
        x, acc, out5, phi, _ = self.P.leapfrog(*a)
        return np.array(x, dtype=np.float64), acc, out5, phi


# ----------------------------------------------------------------------------- scenario: the stream's 1 / wm

STREAM_BINS, STREAM_BATCH = 7, 2


class StreamCase(object):
    """One chain of accepted trajectories on B (and, for the stream that outlives its weights, on A before), recorded
    as m = x (1 / wm).  stale_*: the rows recorded as x itself (a stream older than the weights), or with 1 / wm_A."""

    def __init__(self, orc, spec):
        self.spec = spec
        self.A, self.B = Problem(orc, spec, "A"), Problem(orc, spec, "B")
        self.chA = Chains(self.A.oracle(), spec.M, 1, 4, seed=3)
        self.chB = Chains(self.B.oracle(), spec.M, 1, spec.T, seed=4)
        # the histogram's bounds in model units: around the rows of B
        mB = np.array([self.chB.ref.xs[0, t] / self.B.wm for t in range(spec.T)])
        self.lo, self.hi = mB.min(axis=0) - 0.1 * np.ptp(mB, axis=0) - 1e-3, mB.max(axis=0) + 0.1 * np.ptp(mB, axis=0) + 1e-3

    def rows(self, ch):
        """the accepted states of ch's one chain, in order"""
        return [ch.ref.xs[0, t] for t in range(ch.T) if ch.ref.acc[0, t]]

    def stream(self, rows_and_weights):
        st = Stream(1, self.spec.M, STREAM_BINS, STREAM_BATCH, self.lo, self.hi)
        for x, wm in rows_and_weights:
            if wm is None:
                st.add(0, x)
            else:
                st.add_x(0, x, wm)
        return st

    def expected_before_weights(self):
        return self.stream([(x, self.B.wm) for x in self.rows(self.chB)])

    def stale_before_weights(self):
        return self.stream([(x, None) for x in self.rows(self.chB)])

    def expected_outlives(self):
        return self.stream([(x, self.A.wm) for x in self.rows(self.chA)] + [(x, self.B.wm) for x in self.rows(self.chB)])

    def stale_outlives(self):
        return self.stream([(x, self.A.wm) for x in self.rows(self.chA)] + [(x, self.A.wm) for x in self.rows(self.chB)])


def stream_distance(a, b):
    """the smallest relative distance of two streams over mean and std (the histogram decides nothing here)"""
    ra, rb = a.read(), b.read()
    return min(relmax(ra["mean"], rb["mean"]), relmax(ra["std"], rb["std"]))


# ----------------------------------------------------------------------------- scenario: the folded store

class FoldCase(object):
    """Three geometries of one (N, M) in turn, each with build_G and weight: a grid symmetric under both mirrors,
    another symmetric grid (other extent, other layers, other height), and the first grid's points over cells whose
    first column is narrower (no mirror in x).  fold_info: "on", "on", the detector's reason.
    stale_fold(k): stage k's chain on the kernel of stage k - 1 (a folded store that outlived its kernel)."""

    REASONS = ("on", "on", "cells not mirror-symmetric")

    def __init__(self, orc, spec):
        import fold_oracle_cases as fc
        self.spec = spec
        nz, ny, nx = spec.shape
        g1 = fc.geometry((2, 2), (nx, ny, nz))
        g2 = fc.geometry((2, 2), (nx, ny, nz), extent=(1600.0, 2400.0), layers=(0.3, 0.7))
        g2[0][2] = -50.0
        b3 = g1[1].copy()
        edge = b3[:, 1].min()                   # the x edge between the two columns of cells
        b3[b3[:, 1] == edge, 1] = 0.7 * edge
        b3[b3[:, 0] == edge, 0] = 0.7 * edge
        self.stages = [Problem(orc, spec, w, geometry=g) for w, g in (("S1", g1), ("S2", g2), ("AS", (g1[0], b3)))]
        self.P = [pb.oracle() for pb in self.stages]
        self.ch = [Chains(P, spec.M, 1, spec.T, seed=61 + k, centre=pb.wm * np.random.default_rng(k).uniform(0.3, 0.7, spec.M))
                   for k, (P, pb) in enumerate(zip(self.P, self.stages))]
        rng = np.random.default_rng(67)
        self.x, self.r = rng.uniform(0.2, 0.8, spec.M) * self.stages[2].wm, rng.normal(size=spec.N)

    def stale_fold(self, k):
        return replay(split(self.stages[k], self.stages[k - 1].Aw, self.stages[k - 1].Aw), self.ch[k])


# ----------------------------------------------------------------------------- generated once

@functools.lru_cache(maxsize=None)
def fold():
    from oracle import oracle
    return FoldCase(oracle, BY_ID["fold-4x16"])



@functools.lru_cache(maxsize=None)
def two_kernels(cid):
    from oracle import oracle
    return TwoKernels(oracle, BY_ID[cid])


@functools.lru_cache(maxsize=None)
def bscg(cid="two-pass-37x203"):
    from oracle import cg_port, oracle
    return Bscg(oracle, cg_port, two_kernels(cid))


@functools.lru_cache(maxsize=None)
def before_weights(cid="two-pass-37x203"):
    from oracle import oracle
    return BeforeWeights(oracle, BY_ID[cid])


@functools.lru_cache(maxsize=None)
def wavelet():
    from oracle import oracle
    return Wavelet(oracle, BY_ID["wavelet-37x192"])


@functools.lru_cache(maxsize=None)
def stream():
    from oracle import oracle
    return StreamCase(oracle, BY_ID["stream-30x120"])


@functools.lru_cache(maxsize=None)
def crossgrad():
    import contextlib
    import io
    from conftest import gold
    from gravinv3dhmc_amd import mesher
    z = gold("joint_small.npz")
    with contextlib.redirect_stdout(io.StringIO()):
        mesh = mesher.PrismMesh(tuple(z["a_mrange"]), tuple(z["a_mspacing"]))
    return CrossGrad(z, mesh)
