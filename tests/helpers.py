"""Shared problem builders for the tests (synthetic inputs of BASELINE.json's configs)."""
import numpy as np


def c1_inputs():
    """Config C1: uniformgrid singlecube, 20x30x10 prisms, 600 obs on z=0."""
    from gravinv3dhmc_amd import mesher
    mesh = mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    zp = np.zeros_like(xp)
    return mesh, xp, yp, zp


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def shape3(M):
    """A (nz, ny, nx) with product M for the stencil regularisers."""
    f = [d for d in range(2, int(M ** 0.5) + 1) if M % d == 0]
    if not f:
        return (1, 1, M)
    nz, rest = f[0], M // f[0]
    g = [d for d in range(2, int(rest ** 0.5) + 1) if rest % d == 0]
    ny = g[0] if g else 1
    return (nz, ny, rest // ny)


def stable_dt(P, x0, rng, iters=12):
    """A step a fifth of the stability limit of the stiffest mode: power iteration on differences of the oracle's
    gradient."""
    g0 = P.misfit_and_grad(x0)[1]
    v = rng.normal(size=x0.size)
    lam = 0.0
    for _ in range(iters):
        v = v / np.linalg.norm(v)
        hv = (P.misfit_and_grad(x0 + 1e-6 * v)[1] - g0) / 1e-6
        lam = np.linalg.norm(hv)
        v = hv
    return 0.4 / np.sqrt(lam)


def metropolis_u(dH, want):
    """The variate of a trajectory whose decision is `want`: half-way between exp(-dH) and 0 (accept) or 1 (reject),
    far from the Metropolis edge."""
    return 0.5 * np.exp(-max(dH, 0.0)) if want else 0.5 * (1.0 + np.exp(-dH))
