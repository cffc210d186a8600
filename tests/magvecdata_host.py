"""NumPy restatement of the magnetization-vector model under vector data (MagVectorModule(data=...)), for the tests:
the row blocks (tf, bx, by, bz) x the column blocks (x, y, z) stacked from reference columns, the data weighting Wb,
the column norms Wm of Wb A, the data term with one mean per row block, the four regularisers applied to each of the
three properties on its own, the amplitude term, and the leapfrog trajectory and chain with clamp-and-reflect.  The
rows are tests/multicomp_host.py's, the columns tests/magvector_host.py's; nothing here is imported by the product
package."""
import numpy as np

from oracle import oracle

from magvector_host import amplitude_term, regulariser
from multicomp_host import std_weights  # noqa: F401  (re-exported: the "std" rule is MultiComponentModule's)

COMPS = ("tf", "bx", "by", "bz")


def tf_from_b(K, f):
    """The tf blocks (3, n, m) from the b blocks K[comp] = (3, n, m): f . (bx, by, bz) for every axis"""
    return f[0] * np.asarray(K["bx"]) + f[1] * np.asarray(K["by"]) + f[2] * np.asarray(K["bz"])


def stack(K, data, weights, n=None, weightfactor=0.5):
    """(Aw, wm, wb, A) of the store of the data components `data`: K[comp] = (3, n_all, m) holds the unit-axis columns
    of a component (the fixture's), block b = [K_x | K_y | K_z] of data[b] at the first n points; Wb scales block b by
    weights[b], wm holds the column 2-norms of Wb A to the power 2 weightfactor, Aw = Wb A Wm^-1."""
    blocks = []
    for comp in data:
        Kc = np.asarray(K[comp], dtype=np.float64)
        blocks.append(np.hstack([Kc[a][:n] for a in range(3)]))
    A = np.vstack(blocks)
    nb = blocks[0].shape[0]
    wb = np.repeat(np.asarray(weights, dtype=np.float64), nb)
    Aw, wm = oracle.col_weight(A * wb[:, None], weightfactor)
    return Aw, wm, wb, A


def cg_invert(grad, M, iters):
    """Minimiser of a QUADRATIC potential from its gradient alone, by `iters` steps of linear conjugate gradients from
    0: H p = grad(p) - grad(0).  A fixed number of steps in a fixed order: the same arithmetic on whatever evaluates
    the gradient (the restatement, or the device)."""
    g0 = np.array(grad(np.zeros(M)), dtype=np.float64)
    x, r = np.zeros(M), -g0
    p = r.copy()
    for _ in range(iters):
        Hp = np.asarray(grad(p), dtype=np.float64) - g0
        a = (r @ r) / (p @ Hp)
        x = x + a * p
        rn = r - a * Hp
        p = rn + ((rn @ rn) / (r @ r)) * p
        r = rn
    return x


def cos_moment(model, truth):
    """cosine of the angle between the net moments (the sums of the cells' vectors) of two property-major models"""
    a = np.asarray(model).reshape(3, -1).sum(axis=1)
    b = np.asarray(truth).reshape(3, -1).sum(axis=1)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


class VecDataProblem:
    """Potential and trajectory on a weighted stacked store Aw (C n x 3 m) and weighted observations dobsw (C n).
    global_mean=True removes ONE mean over all rows instead of one per block (what the model must not do)."""

    def __init__(self, Aw, dobsw, ncomp, mwapr, regularization="Damping", alpha=1.0, beta=0.01, wm=None, shape=None,
                 lam=0.0, amp_beta=0.01, scale=1.0, global_mean=False):
        self.Aw = np.asarray(Aw, dtype=np.float64)
        self.N, self.M = self.Aw.shape
        assert self.N % ncomp == 0 and self.M % 3 == 0
        self.ncomp, self.n = ncomp, self.N // ncomp
        self.dobsw = np.asarray(dobsw, dtype=np.float64)
        self.mwapr = np.asarray(mwapr, dtype=np.float64)
        self.reg, self.alpha, self.beta = regularization, alpha, beta
        self.wm = np.asarray(wm, dtype=np.float64) if wm is not None else np.ones(self.M)
        self.wm2 = self.wm ** 2
        self.shape = shape
        self.lam, self.amp_beta, self.scale = lam, amp_beta, scale
        self.global_mean = global_mean
        self.phi = 0.0

    def centre(self, v):
        """(v with the mean of every block removed, the means)"""
        if self.global_mean:
            m = np.full(self.ncomp, v.mean())
        else:
            m = v.reshape(self.ncomp, self.n).mean(axis=1)
        return v - np.repeat(m, self.n), m

    def misfit_and_grad(self, x):
        """(misfit, grad, dpre, data_value, model_value) as MagVectorModule.misfit_and_grad; self.phi = Phi,
        self.pred_mean / self.obs_mean the blocks' means"""
        x = np.asarray(x, dtype=np.float64)
        d = self.Aw @ x
        dc, self.pred_mean = self.centre(d)
        oc, self.obs_mean = self.centre(self.dobsw)
        r = dc - oc
        data = float(r @ r)
        R, gR = regulariser(self.reg, x, self.mwapr, self.wm2, self.beta, self.shape)
        U, g = data + self.alpha * R, 2.0 * (self.Aw.T @ r) + self.alpha * gR
        self.phi = 0.0
        if self.lam > 0:
            self.phi, gp, _ = amplitude_term(x, self.wm, self.amp_beta, self.scale)
            U, g = U + self.lam * self.phi, g + self.lam * gp
        return U, g, d, data, R

    def leapfrog(self, x, p0, dt, L, low, high, u):
        """One trajectory (the reference's hmc.py:85-177): (x_new, accepted, out5)"""
        xn, pn = np.array(x, dtype=np.float64), np.array(p0, dtype=np.float64)
        o0 = self.misfit_and_grad(xn)
        Hcur = 0.5 * float(pn @ pn) + o0[0]
        pn -= dt * o0[1] * 0.5
        o1 = o0
        for i in range(L):
            xn += dt * pn
            hi, lo = xn > high, xn < low
            xn[hi], xn[lo] = high[hi], low[lo]
            pn[hi | lo] = -pn[hi | lo]
            o1 = self.misfit_and_grad(xn)
            pn -= dt * o1[1] * (1.0 if i < L - 1 else 0.5)
        Hnew = 0.5 * float(pn @ pn) + o1[0]
        acc = bool(Hnew < Hcur or u < np.exp(-(Hnew - Hcur)))
        o = o1 if acc else o0
        return (xn if acc else np.array(x, dtype=np.float64)), acc, np.array([o[0], o[3], o[4], Hcur, Hnew])

    def chain(self, x0, trajs, dt, low, high):
        """[(accepted, out5, x after the trajectory)] of the trajectories (L, p0, u) from x0"""
        x, out = np.array(x0, dtype=np.float64), []
        for L, p0, u in trajs:
            x, acc, o = self.leapfrog(x, p0, dt, L, low, high, u)
            out.append((acc, o, x.copy()))
        return out


#: the direction case: Damping weight and conjugate-gradient steps
DIR_ALPHA, DIR_ITERS = 1e-6, 40


def direction_case(z, data):
    """The fixture's compact body (2 A/m at (inc, dec) = (-25, 100) under a field at (60, -10)), its noise-free
    reference data plus a base level per block, and the restatement's problem: Damping with a small alpha, mwapr = 0,
    so that the potential is quadratic and cg_invert applies."""
    K = {c: z["K_" + c] for c in COMPS}
    truth = np.ascontiguousarray(z["vec"].T).ravel()
    Aw, wm, wb, A = stack(K, data, np.ones(len(data)))
    base = {"tf": 4.0, "bx": -700.0, "by": 300.0, "bz": 55.0}
    dobs = [z["d_" + c] + base[c] for c in data]
    P = VecDataProblem(Aw, np.concatenate(dobs), len(data), np.zeros(wm.size), "Damping", DIR_ALPHA, 0.01, wm=wm)
    return z, truth, dobs, P, wm
