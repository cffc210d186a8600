"""NumPy restatement of the cross-gradient coupling of the joint inversion (include/gravhmc.h,
gh_set_cross_gradient), the host side of tests/test_crossgrad_host.py and tests/test_gpu_crossgrad.py.

Mesh shape (nz, ny, nx), x fastest; the stacked weighted model mw = [mw_rho | mw_kappa]; physical, normalised
models u = mw_rho winv / s_rho, w = mw_kappa winv / s_kappa with winv = 1 / wm (0 where wm == 0); forward
differences over centre distances at the cells with a forward neighbour on every axis; t = Du x Dw,
Phi = sum |t|^2; the gradient through the adjoint of the difference operator."""
import numpy as np


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _diff(f, hx, hy, hz):
    core = f[:-1, :-1, :-1]
    return ((f[:-1, :-1, 1:] - core) / hx, (f[:-1, 1:, :-1] - core) / hy,
            (f[1:, :-1, :-1] - core) / np.asarray(hz, dtype=np.float64)[:, None, None])


def _adjoint(V, shape, hx, hy, hz):
    """Each component of V, divided by its spacing, subtracted at the cell and added at its forward neighbour."""
    g = np.zeros(shape)
    vx, vy, vz = V[0] / hx, V[1] / hy, V[2] / np.asarray(hz, dtype=np.float64)[:, None, None]
    g[:-1, :-1, :-1] -= vx + vy + vz
    g[:-1, :-1, 1:] += vx
    g[:-1, 1:, :-1] += vy
    g[1:, :-1, :-1] += vz
    return g


def cross_gradient(mw, wm, shape, hx, hy, hz, scale=(1.0, 1.0)):
    """(Phi, dPhi/dmw (2m), t (m, 3)) at the stacked weighted model mw (2m)."""
    nz, ny, nx = (int(v) for v in shape)
    m = nz * ny * nx
    mw = np.asarray(mw, dtype=np.float64)
    wm = np.asarray(wm, dtype=np.float64)
    with np.errstate(divide="ignore"):
        winv = np.where(wm == 0, 0.0, 1.0 / wm)
    sw = winv / np.repeat(np.asarray(scale, dtype=np.float64), m)
    u = (mw[:m] * sw[:m]).reshape(nz, ny, nx)
    w = (mw[m:] * sw[m:]).reshape(nz, ny, nx)
    Du, Dw = _diff(u, hx, hy, hz), _diff(w, hx, hy, hz)
    t = _cross(Du, Dw)
    phi = float(sum(np.sum(c * c) for c in t))
    A = [2.0 * c for c in _cross(Dw, t)]
    B = [2.0 * c for c in _cross(t, Du)]
    grad = np.concatenate([_adjoint(A, (nz, ny, nx), hx, hy, hz).ravel(),
                           _adjoint(B, (nz, ny, nx), hx, hy, hz).ravel()]) * sw
    tt = np.zeros((nz, ny, nx, 3))
    for c in range(3):
        tt[:-1, :-1, :-1, c] = t[c]
    return phi, grad, tt.reshape(m, 3)


def relative_spacings(mesh):
    """(hx, hy, hz[nz - 1]) of a PrismMesh as JointModule passes them: centre distances over the smallest one."""
    zc = np.array([0.5 * sum(mesh._layer_z(k)) for k in range(mesh.shape[0])])
    hz = np.diff(zc)
    hmin = min(float(mesh.dims[0]), float(mesh.dims[1]), float(hz.min()))
    return mesh.dims[0] / hmin, mesh.dims[1] / hmin, hz / hmin


class JointHostProblem(object):
    """The joint potential on the host, U = |Aw mw - dobsw|^2 + alpha R + lam Phi (no mean removal), and the
    reference's leapfrog on it (oracle.numpy_port.NumpyProblem.leapfrog, 'mandatory' bounds).  Aw: the stacked
    2n x 2m layout (np.asarray(JointModule.Aw))."""

    def __init__(self, Aw, dobsw, wm, shape, reg, alpha, beta, mwapr, lam, spacing, scale=(1.0, 1.0)):
        import scipy.sparse as sp
        from gravinv3dhmc_amd.inversion.joint import fd3d
        self.Aw, self.dobsw, self.wm, self.shape = np.asarray(Aw), np.asarray(dobsw), np.asarray(wm), tuple(shape)
        self.reg, self.alpha, self.beta, self.mwapr = reg, float(alpha), float(beta), np.asarray(mwapr)
        self.lam, self.spacing, self.scale = float(lam), spacing, scale
        self.R = sp.block_diag([fd3d(self.shape)] * 2, format="csr")
        self.last_phi = 0.0

    def regulariser(self, v):
        """Value and gradient of the regulariser at v = mw - mwapr (potential.py:1690-1778)."""
        if self.reg == "Damping":
            return v @ v, 2 * v
        if self.reg == "MS":
            den = v * v + self.beta
            return np.sum(self.wm ** 2 * v * v / den), 2 * self.beta * self.wm ** 2 * v / den ** 2
        t = self.R @ v
        if self.reg == "Smoothness":
            return t @ t, 2 * (self.R.T @ t)
        u = np.sqrt(t * t + self.beta)
        return np.sum(u), self.R.T @ (t / u)

    def misfit_and_grad(self, mw):
        d = self.Aw @ mw
        r = d - self.dobsw
        rv, rg = self.regulariser(mw - self.mwapr)
        U_data = r @ r
        U, grad = U_data + self.alpha * rv, 2 * (self.Aw.T @ r) + self.alpha * rg
        self.last_phi = 0.0
        if self.lam > 0:
            phi, pg, _ = cross_gradient(mw, self.wm, self.shape, *self.spacing, scale=self.scale)
            U, grad = U + self.lam * phi, grad + self.lam * pg
            self.last_phi = phi
        return U, grad, d, U_data, rv

    def leapfrog(self, xcur, p0, dt, L, low, high, u):
        """-> (x, accepted, out5, Phi of the state returned, cells clamped at a bound during the trajectory)"""
        pnew, xnew = p0 * 1.0, xcur * 1.0
        K = np.dot(pnew, pnew) * 0.5
        U, grad, _, U_data, U_model = self.misfit_and_grad(xnew)
        phi0 = self.last_phi
        Hcur = K + U
        pnew -= dt * grad * 0.5
        clamped = 0
        for i in range(L):
            xnew += dt * pnew
            idx1, idx2 = xnew > high, xnew < low
            clamped += int(idx1.sum() + idx2.sum())
            xnew[idx1], pnew[idx1] = high[idx1], -pnew[idx1]
            xnew[idx2], pnew[idx2] = low[idx2], -pnew[idx2]
            Unew, grad, _, Unew_data, Unew_model = self.misfit_and_grad(xnew)
            pnew -= dt * grad if i < L - 1 else dt * grad * 0.5
        Hnew = np.dot(pnew, pnew) * 0.5 + Unew
        if Hnew < Hcur or u < np.exp(-(Hnew - Hcur)):
            return xnew, True, np.array([Unew, Unew_data, Unew_model, Hcur, Hnew]), self.last_phi, clamped
        return xcur, False, np.array([U, U_data, U_model, Hcur, Hnew]), phi0, clamped


def legacy_draws(seed, n, Lrange, Sigma, count):
    """The reference's draws per trajectory, in its order: randint, randn(n) * Sigma, rand (hmc.py:297,95,164)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        L = rs.randint(Lrange[0], Lrange[1] + 1)
        p0 = rs.randn(n) * Sigma
        out.append((int(L), p0, float(rs.rand())))
    return out
