"""NumPy restatement of the multi-component model (MultiComponentModule), for the tests: C kernels stacked in row
blocks, the data weighting Wb, the column norms Wm of Wb A, the data term with one mean per block, the four
regularisers and the leapfrog trajectory with clamp-and-reflect.  Built on the oracle's public functions where they
apply (col_weight, regulariser); nothing here is imported by the product package."""
import numpy as np

from oracle import oracle


def std_weights(dobs):
    """w_c = std(dobs_0) / std(dobs_c)"""
    sd = np.array([np.std(np.asarray(d, dtype=np.float64)) for d in dobs])
    return sd[0] / sd


def stack(kernels, weights, weightfactor=0.5):
    """(Aw, wm, wb) of the kernels stacked in row blocks: Wb scales block c by weights[c], wm holds the column
    2-norms of Wb A to the power 2 weightfactor, Aw = Wb A Wm^-1."""
    n = kernels[0].shape[0]
    wb = np.repeat(np.asarray(weights, dtype=np.float64), n)
    A = np.vstack([np.asarray(K, dtype=np.float64) for K in kernels]) * wb[:, None]
    Aw, wm = oracle.col_weight(A, weightfactor)
    return Aw, wm, wb


class MultiProblem:
    """Potential and trajectory on a weighted stacked store Aw (C n x M) and weighted observations dobsw (C n).
    global_mean=True removes ONE mean over all rows instead (what the model must not do)."""

    def __init__(self, Aw, dobsw, ncomp, mwapr, regularization="Damping", alpha=1.0, beta=0.01, wm=None, shape=None,
                 global_mean=False):
        self.Aw = np.asarray(Aw, dtype=np.float64)
        self.N, self.M = self.Aw.shape
        assert self.N % ncomp == 0
        self.ncomp, self.n = ncomp, self.N // ncomp
        self.dobsw = np.asarray(dobsw, dtype=np.float64)
        self.mwapr = np.asarray(mwapr, dtype=np.float64)
        self.reg, self.alpha, self.beta = regularization, alpha, beta
        self.wm2 = np.asarray(wm, dtype=np.float64) ** 2 if wm is not None else np.ones(self.M)
        self.shape = shape
        self.global_mean = global_mean

    def centre(self, v):
        """(v with the mean of every block removed, the means)"""
        if self.global_mean:
            m = np.full(self.ncomp, v.mean())
        else:
            m = v.reshape(self.ncomp, self.n).mean(axis=1)
        return v - np.repeat(m, self.n), m

    def potential(self, x):
        d = self.Aw @ x
        r = self.centre(d)[0] - self.centre(self.dobsw)[0]
        R, _ = oracle.regulariser(self.reg, x, self.mwapr, self.wm2, self.beta, self.shape)
        return float(r @ r) + self.alpha * R

    def misfit_and_grad(self, x):
        """(misfit, grad, dpre, data_value, model_value) as GravMagModule.misfit_and_grad"""
        x = np.asarray(x, dtype=np.float64)
        d = self.Aw @ x
        dc, self.pred_mean = self.centre(d)
        oc, self.obs_mean = self.centre(self.dobsw)
        r = dc - oc
        data = float(r @ r)
        R, gR = oracle.regulariser(self.reg, x, self.mwapr, self.wm2, self.beta, self.shape)
        return data + self.alpha * R, 2.0 * (self.Aw.T @ r) + self.alpha * gR, d, data, R

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
