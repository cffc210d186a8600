"""Host-side checks of the multi-component inversion (MultiComponentModule): exports, argument validation and the
refusals decided before a device is touched, and the NumPy restatement of its model (tests/multicomp_host.py) against
finite differences of its own potential and, with one component, against the oracle."""
import numpy as np
import pytest

from multicomp_host import MultiProblem, stack, std_weights
from oracle import oracle

REGS = ("Damping", "MS", "Smoothness", "TV")


def test_multicomp_exports():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import MultiComponentModule
    assert g.MultiComponentModule is MultiComponentModule
    assert "MultiComponentModule" in g.__all__
    assert _lib.CELL_PRISM_MULTI == 6 and _lib.MULTI_MAX == len(_lib.COMPONENTS)
    assert all(f in _lib.PROTOTYPES for f in ("gh_set_cells_multi", "gh_multi_info"))
    assert MultiComponentModule._props == 1


def _args(n=6, c=2):
    x = np.linspace(0, 2000, n)
    rng = np.random.default_rng(0)
    return ([rng.normal(size=n) for _ in range(c)], (0, 2000, 0, 3000, 0, 900), (300, 750, 500),
            (x, x.copy(), np.full(n, -30.0)))


def test_multicomp_argument_validation():
    from gravinv3dhmc_amd.inversion import MultiComponentModule as MC
    d, mrange, mspacing, obs = _args()
    with pytest.raises(ValueError, match="empty"):
        MC([], mrange, mspacing, obs, components=(), verbose=False)
    with pytest.raises(ValueError, match="gzx"):
        MC(d, mrange, mspacing, obs, components=("gz", "gzx"), verbose=False)
    with pytest.raises(ValueError, match="distinct"):
        MC(d, mrange, mspacing, obs, components=("gzz", "gzz"), verbose=False)
    with pytest.raises(ValueError):
        MC(d[:1], mrange, mspacing, obs, components=("gz", "gzz"), verbose=False)          # one vector, two components
    with pytest.raises(ValueError):
        MC([d[0], d[1][:-1]], mrange, mspacing, obs, components=("gz", "gzz"), verbose=False)   # length mismatch
    with pytest.raises(ValueError):
        MC({"gz": d[0], "gxx": d[1]}, mrange, mspacing, obs, components=("gz", "gzz"), verbose=False)
    for w in ("var", (1.0,), (1.0, -2.0), (1.0, 0.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            MC(d, mrange, mspacing, obs, components=("gz", "gzz"), weights=w, verbose=False)
    with pytest.raises(ValueError):
        MC([d[0], np.zeros(6)], mrange, mspacing, obs, components=("gz", "gzz"), verbose=False)   # std of 0
    with pytest.raises(ValueError):
        MC(d, mrange, mspacing, obs, components=("gz", "gzz"), coordinate="polar", verbose=False)
    with pytest.raises(TypeError):
        MC(d, mrange, mspacing, obs, components=("gz", "gzz"), topo=None, verbose=False)


def test_multicomp_refusals_before_device_work():
    from gravinv3dhmc_amd.inversion import MultiComponentModule as MC
    d, mrange, mspacing, obs = _args()
    for kw in ({"coordinate": "spherical"}, {"wavelet": "1D"}, {"wavelet": "3D"}, {"matrix_free": True},
               {"shift_invariant": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match="multi-component store"):
            MC(d, mrange, mspacing, obs, components=("gz", "gzz"), verbose=False, **kw)
    # more stacked rows than the fused sweep holds: refused with the limit
    n = 8193
    x = np.linspace(0, 2000, n)
    big = [np.arange(n, dtype=float), np.arange(n, dtype=float)]
    with pytest.raises(NotImplementedError, match="16384"):
        MC(big, mrange, mspacing, (x, x, np.zeros(n)), components=("gz", "gzz"), verbose=False)


# ----------------------------------------------------------------------------- the restatement

def _problem(ncomp, n=7, shape=(2, 3, 4), seed=1):
    rng = np.random.default_rng(seed)
    M = int(np.prod(shape))
    # blocks in very different units, as mGal and Eotvos are
    kernels = [rng.normal(size=(n, M)) * 10.0 ** (2 * c) for c in range(ncomp)]
    dobs = [rng.normal(size=n) * 10.0 ** (2 * c) + 3.0 * c for c in range(ncomp)]
    w = std_weights(dobs)
    Aw, wm, wb = stack(kernels, w)
    return kernels, dobs, w, Aw, wm, wb, rng


def test_stack_weights_the_blocks_before_the_norms():
    kernels, dobs, w, Aw, wm, wb, _ = _problem(3)
    n = kernels[0].shape[0]
    assert w[0] == 1.0 and wb.shape == (3 * n,)
    WA = np.vstack([w[c] * kernels[c] for c in range(3)])
    assert np.allclose(wm, np.sqrt((WA ** 2).sum(axis=0)), rtol=1e-13)
    assert np.allclose(Aw * wm[None, :], WA, rtol=1e-13)
    # the norms of the unweighted stack are decided by the block with the largest unit
    A = np.vstack(kernels)
    assert np.abs(np.sqrt((A ** 2).sum(axis=0)) / np.sqrt((kernels[2] ** 2).sum(axis=0)) - 1).max() < 1e-3
    assert np.abs(wm / np.sqrt((A ** 2).sum(axis=0)) - 1).min() > 0.5


@pytest.mark.parametrize("reg", REGS)
def test_restatement_gradient_against_finite_differences(reg):
    shape = (2, 3, 4)
    _, dobs, w, Aw, wm, wb, rng = _problem(3, shape=shape)
    P = MultiProblem(Aw, wb * np.concatenate(dobs), 3, 0.01 * wm, reg, 0.7, 0.05, wm=wm, shape=shape)
    x = rng.uniform(0.1, 1.0, wm.size) * wm
    U, grad, d, data, R = P.misfit_and_grad(x)
    assert abs(U - P.potential(x)) <= 1e-13 * abs(U) and abs(U - (data + 0.7 * R)) <= 1e-13 * abs(U)
    worst = 0.0
    for j in range(wm.size):
        h = 1e-6 * wm[j]
        e = np.zeros(wm.size)
        e[j] = h
        fd = (P.potential(x + e) - P.potential(x - e)) / (2 * h)
        worst = max(worst, abs(fd - grad[j]) / np.abs(grad).max())
    print("%s: finite differences against the gradient, worst %.3e of max |grad|" % (reg, worst))
    assert worst < 1e-6


def test_restatement_removes_one_mean_per_block():
    _, dobs, w, Aw, wm, wb, rng = _problem(3)
    n = dobs[0].size
    x = rng.uniform(0.1, 1.0, wm.size) * wm
    shifted = [d + k for d, k in zip(dobs, (5.0, -700.0, 3.0e4))]
    a = MultiProblem(Aw, wb * np.concatenate(dobs), 3, 0.01 * wm).misfit_and_grad(x)
    b = MultiProblem(Aw, wb * np.concatenate(shifted), 3, 0.01 * wm).misfit_and_grad(x)
    assert abs(a[0] - b[0]) <= 1e-10 * abs(a[0]) and np.abs(a[1] - b[1]).max() <= 1e-10 * np.abs(a[1]).max()
    ga = MultiProblem(Aw, wb * np.concatenate(dobs), 3, 0.01 * wm, global_mean=True).misfit_and_grad(x)
    gb = MultiProblem(Aw, wb * np.concatenate(shifted), 3, 0.01 * wm, global_mean=True).misfit_and_grad(x)
    assert abs(ga[0] - gb[0]) > 1e-3 * abs(ga[0])
    # every block of the residual has zero mean, and so has the residual the gradient is formed from
    P = MultiProblem(Aw, wb * np.concatenate(dobs), 3, 0.01 * wm)
    d = Aw @ x
    r = P.centre(d)[0] - P.centre(P.dobsw)[0]
    assert np.abs(r.reshape(3, n).mean(axis=1)).max() <= 1e-12 * np.abs(r).max()


@pytest.mark.parametrize("reg", REGS)
def test_one_component_is_the_oracle_problem(reg):
    shape = (2, 3, 4)
    kernels, dobs, w, Aw, wm, wb, rng = _problem(1, shape=shape)
    assert w[0] == 1.0
    Ao, wo = oracle.col_weight(kernels[0])
    assert np.array_equal(Ao, Aw) and np.array_equal(wo, wm)
    mwapr = 0.01 * wm
    P = MultiProblem(Aw, dobs[0], 1, mwapr, reg, 0.7, 0.05, wm=wm, shape=shape)
    O = oracle.Problem(Aw, dobs[0], mwapr, reg, 0.7, 0.05, wm=wm, shape=shape)
    x = rng.uniform(0.1, 1.0, wm.size) * wm
    a, b = P.misfit_and_grad(x), O.misfit_and_grad(x)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(b[1]).max()
    assert np.abs(a[2] - b[2]).max() <= 1e-12 * np.abs(b[2]).max()
    assert abs(a[3] - b[3]) <= 1e-12 * abs(b[3]) and abs(a[4] - b[4]) <= 1e-12 * max(abs(b[4]), 1e-300)
    low, high = 0.0 * wm, 0.6 * wm
    x0 = 0.3 * wm
    for k in range(4):
        L, p0, u = int(rng.integers(1, 7)), rng.normal(size=wm.size) * 0.3, float(rng.uniform())
        dt = 0.02 if k < 3 else 0.5   # (the last one overshoots: clamps, and is rejected or accepted alike on both)
        xa, acca, oa = P.leapfrog(x0, p0, dt, L, low, high, u)
        xb, accb, ob, _ = O.leapfrog(x0, p0, dt, L, low, high, u)
        assert acca == accb
        assert np.abs(oa - ob).max() <= 1e-12 * np.abs(ob).max()
        assert np.abs(xa - xb).max() <= 1e-12 * np.abs(xb).max()
        x0 = xb
