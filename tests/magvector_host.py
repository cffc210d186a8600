"""NumPy restatement of the magnetization-vector model (MagVectorModule), for the tests: the three blocks side by
side, the column norms over all M columns, the data term with its mean removed, the four regularisers applied to each
of the three properties on its own (oracle.regulariser per block), the amplitude term with its gradient, and the
leapfrog trajectory and chain with clamp-and-reflect.  Nothing here is imported by the product package."""
import numpy as np

from oracle import oracle

STENCIL = ("Smoothness", "TV")


def side_by_side(blocks, weightfactor=0.5):
    """(Aw, wm) of A = [A_x | A_y | A_z]: wm the column 2-norms to the power 2 weightfactor, Aw = A Wm^-1"""
    A = np.hstack([np.asarray(B, dtype=np.float64) for B in blocks])
    return oracle.col_weight(A, weightfactor)


def regulariser(kind, x, mwapr, wm2, beta, shape, props=3):
    """(R, grad R) of the stacked model: each of the `props` properties on its own, values summed"""
    m = x.size // props
    val, grad = 0.0, np.empty_like(x)
    for h in range(props):
        s = slice(h * m, (h + 1) * m)
        v, g = oracle.regulariser(kind, x[s], mwapr[s], wm2[s], beta, shape)
        val += v
        grad[s] = g
    return val, grad


def amplitude_term(mw, wm, beta, scale=1.0):
    """(Phi, dPhi/dmw, amp): u = mw / wm / scale (0 where wm is 0), s_c = sum_a u_a[c]^2, Phi = sum s / (s + beta),
    amp = scale sqrt(s)"""
    mw = np.asarray(mw, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sw = np.where(wm == 0.0, 0.0, (1.0 / wm) / scale)
    u = (mw * sw).reshape(3, -1)
    s = (u * u).sum(axis=0)
    den = s + beta
    grad = ((2.0 * beta / (den * den))[None, :] * u).ravel() * sw
    return float(np.sum(s / den)), grad, scale * np.sqrt(s)


class MagVectorProblem:
    """Potential and trajectory on the weighted store Aw (N x M, M = 3 m) and the observations dobs (N)."""

    def __init__(self, Aw, dobs, mwapr, regularization="Damping", alpha=1.0, beta=0.01, wm=None, shape=None,
                 lam=0.0, amp_beta=0.01, scale=1.0):
        self.Aw = np.asarray(Aw, dtype=np.float64)
        self.N, self.M = self.Aw.shape
        assert self.M % 3 == 0
        dobs = np.asarray(dobs, dtype=np.float64)
        self.dobs_c = dobs - dobs.mean()
        self.mwapr = np.asarray(mwapr, dtype=np.float64)
        self.reg, self.alpha, self.beta = regularization, alpha, beta
        self.wm = np.asarray(wm, dtype=np.float64) if wm is not None else np.ones(self.M)
        self.wm2 = self.wm ** 2
        self.shape = shape
        self.lam, self.amp_beta, self.scale = lam, amp_beta, scale
        self.phi = 0.0

    def misfit_and_grad(self, x):
        """(misfit, grad, dpre, data_value, model_value) as MagVectorModule.misfit_and_grad; self.phi = Phi"""
        x = np.asarray(x, dtype=np.float64)
        d = self.Aw @ x
        r = (d - d.mean()) - self.dobs_c
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
