"""Host-side checks of the magnetization-vector inversion under vector data (prism.bx / by / bz, MagVectorModule(data=),
GH_CELL_PRISM_MVI_DATA): exports and signatures, the C ABI's symbols, argument validation and the refusals decided
before a device is touched, the fixtures' own structure, and the NumPy restatement (tests/magvecdata_host.py) against
the reference's fixtures -- including that it can SEE a global mean in place of the per-block means, and a dropped
block weight."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import gold
from magvecdata_host import (COMPS, DIR_ITERS, VecDataProblem, cg_invert, cos_moment, direction_case, stack,
                             std_weights, tf_from_b)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGS = ("Damping", "MS", "Smoothness", "TV")
BCOMPS = ("bx", "by", "bz")


# ----------------------------------------------------------------------------- exports, signatures, the ABI

def test_public_functions_and_signatures():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd.gravmag import prism
    assert g.prism is prism
    want = ["xp", "yp", "zp", "prisms", "pmag", "njobs", "pool", "return_kernel", "device"]
    for name in BCOMPS:
        fn = getattr(prism, name)
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want, name
        assert [sig.parameters[k].default for k in want[4:]] == [None, 1, None, True, 0]
    sig = inspect.signature(g.MagVectorModule.__init__)
    assert sig.parameters["data"].default == ("tf",) and sig.parameters["weights"].default is None
    assert "component" in inspect.signature(g.MagVectorModule.kernel).parameters
    for name in ("set_cells_mvi_data", "b_result"):
        assert callable(getattr(g.Engine, name))


def test_abi_symbols_and_enum_values():
    from gravinv3dhmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gravhmc.h")).read()
    assert _lib.CELL_PRISM_MVI_DATA == 8 and re.search(r"GH_CELL_PRISM_MVI_DATA = 8 \};", header)
    # (added at the end of the enum: no earlier value moved)
    assert re.search(r"GH_CELL_PRISM_MULTI = 6, GH_CELL_PRISM_MVI = 7, GH_CELL_PRISM_MVI_DATA = 8", header)
    assert (_lib.BCOMP_TF, _lib.BCOMP_BX, _lib.BCOMP_BY, _lib.BCOMP_BZ) == (0, 1, 2, 3)
    assert re.search(r"GH_BCOMP_TF = 0, GH_BCOMP_BX = 1, GH_BCOMP_BY = 2, GH_BCOMP_BZ = 3", header)
    assert _lib.BCOMPONENTS == {"tf": 0, "bx": 1, "by": 2, "bz": 3} and _lib.BCOMP_MAX == 4
    assert re.search(r"#define GH_BCOMP_MAX 4\b", header)
    for sym, nargs in (("gh_set_cells_mvi_data", 8), ("gh_b_result", 4)):
        assert re.search(r"\bint %s\(gh_ctx \*ctx" % sym, header), sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs


# ----------------------------------------------------------------------------- validation before any device work

def _args(n=6, ncomp=3):
    x = np.linspace(0, 2000, n)
    rng = np.random.default_rng(0)
    return ([rng.normal(size=n) for _ in range(ncomp)], (0, 2000, 0, 3000, 0, 900), (300, 750, 500),
            (x, x.copy(), np.full(n, -30.0)))


@pytest.fixture
def no_device(monkeypatch):
    """Engine raises: a constructor that gets as far as the device fails the test with this error"""
    import gravinv3dhmc_amd.inversion.magvector as mvmod
    import gravinv3dhmc_amd.gravmag.prism as prism

    class Touched(AssertionError):
        pass

    def boom(*a, **k):
        raise Touched("device work started")

    monkeypatch.setattr(mvmod, "Engine", boom)
    monkeypatch.setattr(prism, "Engine", boom)
    return Touched


def test_module_value_errors_before_device_work(no_device):
    from gravinv3dhmc_amd.inversion import MagVectorModule as MV
    d, mrange, mspacing, obs = _args()
    ok = ("bx", "by", "bz")
    for data in (("bx", "gz", "bz"), ("bx", "by", "bx"), (), ("b",)):
        with pytest.raises(ValueError):
            MV(d[:len(data)], mrange, mspacing, obs, data=data, verbose=False)
    with pytest.raises(ValueError):                                       # the wrong count
        MV(d[:2], mrange, mspacing, obs, data=ok, verbose=False)
    with pytest.raises(ValueError):                                       # the wrong length
        MV([d[0], d[1][:-1], d[2]], mrange, mspacing, obs, data=ok, verbose=False)
    with pytest.raises(ValueError):                                       # a dict with other keys
        MV({"bx": d[0], "by": d[1], "tf": d[2]}, mrange, mspacing, obs, data=ok, verbose=False)
    for w in ("var", [1.0, 2.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError):
            MV(d, mrange, mspacing, obs, data=ok, weights=w, verbose=False)
    with pytest.raises(ValueError):                                       # "std" of a constant block
        MV([d[0], np.ones(6), d[2]], mrange, mspacing, obs, data=ok, weights="std", verbose=False)
    with pytest.raises(ValueError):
        MV(d, mrange, mspacing, obs, data=ok, amplitude=-1.0, verbose=False)
    # valid arguments do reach the device: the guard itself works
    with pytest.raises(no_device):
        MV(d, mrange, mspacing, obs, data=ok, verbose=False)
    with pytest.raises(no_device):
        MV({"bz": d[0], "tf": d[1]}, mrange, mspacing, obs, data=("tf", "bz"), weights="std", verbose=False)


def test_module_refusals_before_device_work(no_device):
    from gravinv3dhmc_amd.inversion import MagVectorModule as MV
    d, mrange, mspacing, obs = _args()
    for kw in ({"coordinate": "spherical"}, {"wavelet": "1D"}, {"matrix_free": True}, {"shift_invariant": True},
               {"shard": object()}):
        with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
            MV(d, mrange, mspacing, obs, data=("bx", "by", "bz"), verbose=False, **kw)
        # ... and today's module keeps naming its own store
        with pytest.raises(NotImplementedError, match="the magnetization-vector store"):
            MV(d[0], mrange, mspacing, obs, verbose=False, **kw)
    # 16385 stacked rows: 5462 x 3 = 16386 (each block alone is far below the limit)
    n = 5462
    x = np.linspace(0, 2000, n)
    with pytest.raises(NotImplementedError, match="16384.*vector-data magnetization store|vector-data.*16384"):
        MV([np.zeros(n)] * 3, mrange, mspacing, (x, x, np.zeros(n)), data=("bx", "by", "bz"), verbose=False)
    n = 16385
    x = np.linspace(0, 2000, n)
    with pytest.raises(NotImplementedError, match="16384"):
        MV([np.zeros(n)], mrange, mspacing, (x, x, np.zeros(n)), data=("bz",), verbose=False)
    with pytest.raises(TypeError):
        MV(d, mrange, mspacing, obs, data=("bx", "by", "bz"), topo=None, verbose=False)


def test_prism_b_fields_raise_the_references_value_error(no_device):
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd.gravmag import prism
    mesh = g.mesher.PrismMesh((0, 2000, 0, 3000, 0, 900), (450, 1000, 500))
    mesh.addprop("magnetization", np.ones((mesh.size, 3)))
    x = np.linspace(0, 1000, 5)
    for name in BCOMPS:
        with pytest.raises(ValueError, match="Input arrays xp, yp, and zp must have same shape!"):
            getattr(prism, name)(x, x[:-1], x, mesh)
        with pytest.raises(ValueError):                                   # the reference unpacks three values
            getattr(prism, name)(x, x, x, mesh, pmag=2.5)
        with pytest.raises(no_device):
            getattr(prism, name)(x, x, x, mesh)


def test_hmcsamplebatch_refuses_the_store_by_name():
    import gravinv3dhmc_amd as g

    class _E:
        mvi = True
        multi = 3

    class _M:
        _engine = _E()

    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        g.HMCSampleBatch(_M(), 2, 1, 0, 0.01, [1, 2], np.zeros((2, 3)), np.zeros(3), np.zeros((3, 2)), "mandatory",
                         1000, np.zeros(2), "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)


# ----------------------------------------------------------------------------- the fixtures

def test_fixtures_hold_every_component():
    g, tfc = gold("prism_bxyz_cases.npz"), gold("prism_tf_cases.npz")
    # the geometry is prism_tf_cases': the singular points (corners, edges, faces, the x + r = 0 lines) and random ones
    for k in ("xp", "yp", "zp", "cells"):
        assert np.array_equal(g[k], tfc[k]), k
    n, m = g["xp"].size, g["cells"].shape[0]
    assert int(g["n_singular"]) == 112 and n == 232
    for comp in BCOMPS:
        for a in range(3):
            K = g["K_%s_%d" % (comp, a)]
            assert K.shape == (n, m) and np.isfinite(K).all() and np.abs(K).max() > 0
        for key in ("res_vec_", "res_skip_", "res_pmag_"):
            assert g[key + comp].shape == (n,) and np.isfinite(g[key + comp]).all()
    for a in range(3):
        assert g["K_tf_%d" % a].shape == (n, m)
    z = gold("mvi_vecdata_module.npz")
    m = z["cells"].shape[0]
    assert tuple(z["shape"]) == (2, 3, 4) and m == 24 and z["xp"].size == 65
    for comp in COMPS:
        assert z["K_" + comp].shape == (3, 65, m) and z["d_" + comp].shape == (65,)
    assert np.count_nonzero(np.abs(z["vec"]).sum(axis=1)) == 2
    for name in ("prism_bxyz_cases.npz", "mvi_vecdata_module.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 400 * 1024


def test_fixture_identities_of_the_reference():
    """bx of unit e_y equals by of unit e_x (the tensor is symmetric: one second derivative serves both), likewise xz
    and yz; the tf block equals f . (bx, by, bz) to rounding; the results are linear combinations of the columns."""
    g = gold("prism_bxyz_cases.npz")
    assert np.array_equal(g["K_bx_1"], g["K_by_0"])
    assert np.array_equal(g["K_bx_2"], g["K_bz_0"])
    assert np.array_equal(g["K_by_2"], g["K_bz_1"])
    K = {c: np.stack([g["K_%s_%d" % (c, a)] for a in range(3)]) for c in BCOMPS}
    f = g["dircos"]
    T = tf_from_b(K, f)
    worst = 0.0
    for a in range(3):
        ref = g["K_tf_%d" % a]
        dev = np.abs(T[a] - ref).max() / np.abs(ref).max()
        worst = max(worst, dev)
    print("|f.(bx, by, bz) - tf| / max|tf| of the reference's arrays: %.3e" % worst)
    assert worst <= 1e-14
    mag, pvec, skipped = g["mag"], g["pvec"], int(g["skipped"])
    keep = [c for c in range(mag.shape[0]) if c != skipped]
    for comp in BCOMPS:
        r = sum(K[comp][a] @ mag[:, a] for a in range(3))
        assert np.abs(r - g["res_vec_" + comp]).max() <= 1e-12 * np.abs(g["res_vec_" + comp]).max()
        r = sum(K[comp][a][:, keep] @ mag[keep, a] for a in range(3))
        assert np.abs(r - g["res_skip_" + comp]).max() <= 1e-12 * np.abs(g["res_skip_" + comp]).max()
        assert np.abs(r - g["res_vec_" + comp]).max() > 1e-6 * np.abs(r).max()       # (the skipped cell matters)
        # pmag replaces every cell's property, the skipped cell's too (prism.py:768-772)
        r = sum(K[comp][a].sum(axis=1) * pvec[a] for a in range(3))
        assert np.abs(r - g["res_pmag_" + comp]).max() <= 1e-12 * np.abs(g["res_pmag_" + comp]).max()


# ----------------------------------------------------------------------------- the restatement against the fixture

def _module_fixture():
    z = gold("mvi_vecdata_module.npz")
    K = {c: z["K_" + c] for c in COMPS}
    return z, K


def test_restatement_reproduces_the_reference_fixture():
    z, K = _module_fixture()
    model = np.ascontiguousarray(z["vec"].T).ravel()                       # property-major
    from gravinv3dhmc_amd import utils
    f = np.array(utils.dircos(*z["mangle"]))
    T = tf_from_b(K, f)
    assert np.abs(T - K["tf"]).max() <= 1e-14 * np.abs(K["tf"]).max()
    for data, w in ((("bx", "by", "bz"), (1.0, 1.0, 1.0)), (("tf", "bz"), (1.0, 2.5)), (("bz",), (0.5,))):
        Aw, wm, wb, A = stack(K, data, w)
        assert A.shape == (65 * len(data), 72) and Aw.shape == A.shape
        # the unweighted stack times the model: the reference's results, block by block in its own units
        d = A @ model
        for b, comp in enumerate(data):
            ref = z["d_" + comp]
            assert np.abs(d[b * 65:(b + 1) * 65] - ref).max() <= 1e-12 * np.abs(ref).max(), comp
        # Aw = Wb A Wm^-1 with unit columns (weightfactor 0.5: wm the 2-norms of Wb A)
        assert np.allclose(np.sqrt(((A * wb[:, None]) ** 2).sum(axis=0)), wm, rtol=1e-13)
        assert np.allclose((Aw ** 2).sum(axis=0), 1.0, rtol=1e-12)
        assert np.allclose(Aw @ (model * wm), wb * d, rtol=0, atol=1e-12 * np.abs(wb * d).max())
    w = std_weights([z["d_" + c] for c in ("tf", "bz")])
    assert w[0] == 1.0 and abs(w[1] - np.std(z["d_tf"]) / np.std(z["d_bz"])) <= 1e-15 * w[1]


def _problem(reg, data=("tf", "bz"), w=(1.0, 2.5), n=37, lam=0.0, **kw):
    """dobs with clearly different block means: the blocks' base levels are 4, -700, 300, 55 uT"""
    z, K = _module_fixture()
    Aw, wm, wb, A = stack(K, data, w, n=n)
    base = {"tf": 4.0, "bx": -700.0, "by": 300.0, "bz": 55.0}
    dobs = np.concatenate([z["d_" + c][:n] + base[c] for c in data])
    rng = np.random.default_rng(4)
    mwapr = rng.normal(size=wm.size) * 0.01 * wm
    P = VecDataProblem(Aw, wb * dobs, len(data), mwapr, reg, 0.7, 0.001, wm=wm, shape=tuple(int(v) for v in z["shape"]),
                       lam=lam, amp_beta=0.05, **kw)
    return P, wm, rng


@pytest.mark.parametrize("reg", REGS)
def test_restatement_gradient_against_central_differences(reg):
    P, wm, rng = _problem(reg, lam=0.4)
    x = rng.normal(size=P.M) * 0.02 * wm
    U, g, d, data, R = P.misfit_and_grad(x)
    assert P.phi > 0 and abs(U - (data + 0.7 * R + 0.4 * P.phi)) <= 1e-13 * abs(U)
    idx = rng.choice(P.M, 12, replace=False)
    fd = np.empty(12)
    for k, j in enumerate(idx):
        h = 1e-6 * max(abs(x[j]), 1e-3 * wm[j])
        e = np.zeros(P.M)
        e[j] = h
        fd[k] = (P.misfit_and_grad(x + e)[0] - P.misfit_and_grad(x - e)[0]) / (2 * h)
    assert np.abs(fd - g[idx]).max() <= 1e-5 * np.abs(g).max()


def test_restatement_sees_a_global_mean_and_a_dropped_weight():
    """The GPU suite holds the device to 1e-12 of the restatement's values (1e-10 for the means).  The restatement's own
    value moves by many orders more than that when ONE mean over all rows replaces the per-block means, and when a
    block's weight is dropped: the comparison can see both mistakes."""
    for data, w in ((("bx", "by", "bz"), (1.0, 0.4, 2.0)), (("tf", "bz"), (1.0, 2.5))):
        P, wm, rng = _problem("Damping", data, w)
        x = rng.normal(size=P.M) * 0.02 * wm
        U = P.misfit_and_grad(x)[0]
        Pg, _, _ = _problem("Damping", data, w, global_mean=True)
        Ug = Pg.misfit_and_grad(x)[0]
        assert abs(Ug - U) > 1e-3 * abs(U), (data, U, Ug)
        # the last block's weight dropped (1 in its place) in the observations' scaling
        z, K = _module_fixture()
        wd = list(w[:-1]) + [1.0]
        n = P.n
        dobsw = P.dobsw / np.repeat(w, n) * np.repeat(wd, n)
        Pd = VecDataProblem(P.Aw, dobsw, len(data), P.mwapr, "Damping", 0.7, 0.001, wm=wm)
        Ud = Pd.misfit_and_grad(x)[0]
        assert abs(Ud - U) > 1e-3 * abs(U), (data, U, Ud)
        # ... and in the store (the column norms change with it)
        Aw2, wm2, _, _ = stack(K, data, wd, n=n)
        assert np.abs(wm2 - wm).max() > 1e-3 * wm.max()
        print("%r: U = %.6e, one global mean %.6e, weight dropped %.6e" % (data, U, Ug, Ud))


def test_restatement_chain_accepts_rejects_and_clamps():
    P, wm, rng = _problem("TV", ("bx", "by", "bz"), (1.0, 1.0, 1.0), lam=0.4)
    M = P.M
    low, high = -0.02 * wm, 0.02 * wm
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, 0.0) for _ in range(3)]
    trajs += [(8, rng.normal(size=M) * 3.0, 1.0 - 1e-9) for _ in range(2)]
    out = P.chain(P.mwapr, trajs, 0.005, low, high)
    assert any(a for a, _, _ in out) and any(not a for a, _, _ in out)
    for acc, o, x in out:
        assert np.all(x <= high) and np.all(x >= low)


def test_vector_data_fixes_the_direction_on_the_restatement():
    """A compact body magnetized well off the field direction: 40 conjugate-gradient steps on the restatement's
    potential with (bx, by, bz) data give a model whose net moment points along the true one (cosine >= 0.99), and the
    amplitude's centre of mass sits in the body's cells.  What the GPU test asserts of the device's inversion is what
    holds here.  (Deterministic: the fixture's numbers, no noise.)"""
    z, truth, dobs, P, wm = direction_case(gold("mvi_vecdata_module.npz"), ("bx", "by", "bz"))
    got = cg_invert(lambda x: P.misfit_and_grad(x)[1], P.M, DIR_ITERS) / wm
    c = cos_moment(got, truth)
    print("cosine between the recovered and the true net moment: %.6f" % c)
    assert c >= 0.99
    amp, amp_true = np.sqrt((got.reshape(3, -1) ** 2).sum(axis=0)), np.sqrt((truth.reshape(3, -1) ** 2).sum(axis=0))
    assert set(np.argsort(amp)[-2:]) == set(np.flatnonzero(amp_true))
