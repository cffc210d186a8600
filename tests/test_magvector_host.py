"""Host-side checks of the magnetization-vector inversion (MagVectorModule): exports, argument validation and the
refusals decided before a device is touched, the fixtures' own structure, and the NumPy restatement of the model
(tests/magvector_host.py) against the fixtures and against central differences of its own potential."""
import numpy as np
import pytest

from conftest import gold
from magvector_host import MagVectorProblem, amplitude_term, regulariser, side_by_side
from oracle import oracle

REGS = ("Damping", "MS", "Smoothness", "TV")


def test_magvector_exports():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import MagVectorModule
    assert g.MagVectorModule is MagVectorModule and "MagVectorModule" in g.__all__
    assert _lib.CELL_PRISM_MVI == 7
    assert all(f in _lib.PROTOTYPES for f in ("gh_set_cells_mvi", "gh_set_amplitude", "gh_amplitude_eval",
                                              "gh_amplitude_last"))
    assert MagVectorModule._props == 3
    for name in ("set_cells_mvi", "set_amplitude", "amplitude_eval", "amplitude_last"):
        assert callable(getattr(g.Engine, name))


def _args(n=6):
    x = np.linspace(0, 2000, n)
    return (np.random.default_rng(0).normal(size=n), (0, 2000, 0, 3000, 0, 900), (300, 750, 500),
            (x, x.copy(), np.full(n, -30.0)))


def test_magvector_argument_validation_and_refusals_before_device_work():
    from gravinv3dhmc_amd.inversion import MagVectorModule as MV
    d, mrange, mspacing, obs = _args()
    for kw in ({"coordinate": "spherical"}, {"wavelet": "1D"}, {"wavelet": "3D"}, {"matrix_free": True},
               {"shift_invariant": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match="magnetization-vector"):
            MV(d, mrange, mspacing, obs, verbose=False, **kw)
    with pytest.raises(ValueError):
        MV(d[:-1], mrange, mspacing, obs, verbose=False)
    with pytest.raises(ValueError):
        MV(d, mrange, mspacing, obs, coordinate="polar", verbose=False)
    with pytest.raises(ValueError):
        MV(d, mrange, mspacing, obs, amplitude=-1.0, verbose=False)
    with pytest.raises(ValueError):
        MV(d, mrange, mspacing, obs, amplitude=1.0, amplitude_beta=0.0, verbose=False)
    with pytest.raises(TypeError):
        MV(d, mrange, mspacing, obs, topo=None, verbose=False)
    n = 16385
    x = np.linspace(0, 2000, n)
    with pytest.raises(NotImplementedError, match="16384"):
        MV(np.zeros(n), mrange, mspacing, (x, x, np.zeros(n)), verbose=False)


def test_hmcsamplebatch_refuses_the_store_by_name():
    import gravinv3dhmc_amd as g

    class _E:
        mvi = True

    class _M:
        _engine = _E()

    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        g.HMCSampleBatch(_M(), 2, 1, 0, 0.01, [1, 2], np.zeros((2, 3)), np.zeros(3), np.zeros((3, 2)), "mandatory",
                         1000, np.zeros(2), "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)


def test_vector_helpers_invert_ang2vec():
    """to_vectors / from_vectors, amplitude and direction need no device: run them on a bare instance"""
    from gravinv3dhmc_amd import utils
    from gravinv3dhmc_amd.inversion import MagVectorModule as MV
    mv = MV.__new__(MV)
    mv._cells = 5
    inten = np.array([1.0, 2.5, 0.3, 4.0, 7.0])
    inc = np.array([60.0, -45.0, 0.0, 90.0, 10.0])
    dec = np.array([-10.0, 120.0, 0.0, 0.0, 179.0])
    v = np.stack([utils.ang2vec(float(i), float(a), float(b)) for i, a, b in zip(inten, inc, dec)])
    model = mv.from_vectors(v)
    assert model.shape == (15,) and np.array_equal(model[:5], v[:, 0]) and np.array_equal(model[10:], v[:, 2])
    assert np.array_equal(mv.to_vectors(model), v)
    assert np.allclose(mv.amplitude(model), inten, rtol=1e-14)
    i2, d2 = mv.direction(model)
    assert np.allclose(i2, inc, atol=1e-12)
    assert np.allclose(np.delete(d2, 3), np.delete(dec, 3), atol=1e-10)      # (straight down: no declination)
    with pytest.raises(ValueError):
        mv.to_vectors(np.zeros(14))
    with pytest.raises(ValueError):
        mv.from_vectors(np.zeros((3, 5)))


def test_fixtures_say_what_the_reference_delivers():
    """prism.tf's kernel2d does not depend on pmag (it is always the induced kernel); the blocks are the results.
    With f = e_x block x IS the induced kernel, and for any f the induced kernel is sum_a f_a A_a up to rounding --
    the deviation of the reference's own arrays from that identity is what the GPU test allows the device twice."""
    from gravinv3dhmc_amd import utils
    g, tfc = gold("mvi_cases.npz"), gold("prism_tf_cases.npz")
    worst = 0.0
    for d, (inc, dec) in enumerate(g["dirs"]):
        K = tfc["K%d" % d]
        for a in range(3):
            assert np.array_equal(g["kernel2d%d_%d" % (d, a)], K)
            assert np.isfinite(g["A%d_%d" % (d, a)]).all()
        f = utils.dircos(inc, dec)
        S = sum(f[a] * g["A%d_%d" % (d, a)] for a in range(3))
        dev = np.abs(S - K).max() / np.abs(K).max()
        worst = max(worst, dev)
        print("direction %r: |sum f_a A_a - K| / max|K| = %.3e" % ((inc, dec), dev))
        # a linear combination of the blocks gives the results for per-cell vectors
        for key, mag in (("res_vec%d" % d, g["mag"]), ("res_vec2_%d" % d, g["mag2"])):
            r = sum(g["A%d_%d" % (d, a)] @ mag[:, a] for a in range(3))
            assert np.abs(r - g[key]).max() <= 1e-12 * np.abs(g[key]).max()
    assert worst <= 1e-14
    # f = e_x up to cos(90 deg) = 6e-17: block x is the induced kernel to that
    assert np.abs(g["A1_0"] - tfc["K1"]).max() <= 1e-15 * np.abs(tfc["K1"]).max()


def _small_problem(reg, lam=0.0):
    z = gold("mvi_small.npz")
    Aw, wm = side_by_side(list(z["A"]))
    rng = np.random.default_rng(4)
    M = wm.size
    shape = tuple(int(v) for v in z["shape"])
    dobs = z["res_vec"] + 3.0
    mwapr = rng.normal(size=M) * 0.01 * wm
    P = MagVectorProblem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape, lam=lam, amp_beta=0.05)
    return z, P, wm, rng


def test_restatement_blocks_and_forward_against_the_fixture():
    z, P, wm, _ = _small_problem("Damping")
    m = z["cells"].shape[0]
    assert P.Aw.shape == (42, 3 * m) and int(np.prod(z["shape"])) == m
    model = np.ascontiguousarray(z["vec"].T).ravel()                     # property-major
    d = P.Aw @ (model * wm)
    assert np.abs(d - z["res_vec"]).max() <= 1e-12 * np.abs(z["res_vec"]).max()
    A = P.Aw * wm[None, :]
    for a in range(3):
        assert np.abs(A[:, a * m:(a + 1) * m] - z["A"][a]).max() <= 1e-14 * np.abs(z["A"][a]).max()


def test_regulariser_is_per_property():
    z, P, wm, rng = _small_problem("Smoothness")
    m = z["cells"].shape[0]
    shape = tuple(int(v) for v in z["shape"])
    zero = np.zeros(3 * m)
    # flat within each property, a jump between the blocks: no term crosses the block boundary
    x = np.repeat([1.0, -5.0, 40.0], m)
    for kind in ("Smoothness", "TV"):
        v, g = regulariser(kind, x, zero, wm * wm, 0.0 if kind == "Smoothness" else 1e-300, shape)
        assert abs(v) <= 1e-100 and np.abs(g).max() <= 1e-100
    # ... and the value is the three blocks' summed
    x = rng.normal(size=3 * m)
    for kind in REGS:
        v, g = regulariser(kind, x, zero, wm * wm, 0.01, shape)
        parts = [oracle.regulariser(kind, x[h * m:(h + 1) * m], zero[:m], (wm * wm)[h * m:(h + 1) * m], 0.01, shape)
                 for h in range(3)]
        assert v == sum(p[0] for p in parts) and np.array_equal(g, np.concatenate([p[1] for p in parts]))


def test_amplitude_gradient_against_central_differences():
    rng = np.random.default_rng(9)
    m = 7
    wm = rng.uniform(0.5, 2.0, 3 * m)
    wm[4] = 0.0                                                     # (a column of zeros: u = 0, no gradient)
    mw = rng.normal(size=3 * m)
    for beta, scale in ((0.05, 1.0), (2.0, 0.3)):
        phi, grad, amp = amplitude_term(mw, wm, beta, scale)
        assert 0.0 < phi < m and grad[4] == 0.0
        with np.errstate(divide="ignore"):
            phys = np.where(wm == 0, 0.0, mw / wm).reshape(3, m)
        assert np.allclose(amp, np.sqrt((phys ** 2).sum(axis=0)), rtol=1e-13)
        h = 1e-6
        fd = np.empty_like(mw)
        for j in range(mw.size):
            e = np.zeros_like(mw)
            e[j] = h
            fd[j] = (amplitude_term(mw + e, wm, beta, scale)[0] - amplitude_term(mw - e, wm, beta, scale)[0]) / (2 * h)
        assert np.abs(fd - grad).max() <= 1e-8 * max(np.abs(grad).max(), 1.0)


@pytest.mark.parametrize("reg", REGS)
def test_restatement_gradient_against_central_differences(reg):
    z, P, wm, rng = _small_problem(reg, lam=0.4)
    x = rng.normal(size=P.M) * 0.02 * wm
    U, g, d, data, R = P.misfit_and_grad(x)
    assert P.phi > 0 and abs(U - (data + 0.7 * R + 0.4 * P.phi)) <= 1e-13 * abs(U)
    fd = np.empty(12)
    idx = rng.choice(P.M, 12, replace=False)
    for k, j in enumerate(idx):
        h = 1e-6 * max(abs(x[j]), 1e-3 * wm[j])
        e = np.zeros(P.M)
        e[j] = h
        fd[k] = (P.misfit_and_grad(x + e)[0] - P.misfit_and_grad(x - e)[0]) / (2 * h)
    assert np.abs(fd - g[idx]).max() <= 1e-5 * np.abs(g).max()


def test_restatement_chain_rejects_and_clamps():
    z, P, wm, rng = _small_problem("TV", lam=0.4)
    M = P.M
    low, high = -0.02 * wm, 0.02 * wm
    # (a Metropolis variate of 0 accepts whatever the energy does; one next to 1 rejects an overshoot)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, 0.0) for _ in range(4)]
    trajs += [(8, rng.normal(size=M) * 3.0, 1.0 - 1e-9) for _ in range(3)]
    out = P.chain(P.mwapr, trajs, 0.02, low, high)
    assert any(a for a, _, _ in out) and any(not a for a, _, _ in out)
    for acc, o, x in out:
        assert np.all(x <= high) and np.all(x >= low)
