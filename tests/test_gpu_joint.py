"""GPU suite of the joint gravity-magnetic inversion (GH_CELL_PRISM_JOINT, JointModule): the store's blocks
against single-field contexts bit for bit, the module against the reference's JointModule, forward and
adjoint against host products, whole chains against the reference's HMCSample, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import gold
from helpers import relmax

pytestmark = pytest.mark.gpu

MANGLE = (60.0, -10.0)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _grid(n_y, n_x, x1=2000.0, y1=3000.0, h=0.0):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, y1, n_y), np.linspace(0, x1, n_x))]
    return xp, yp, np.full_like(xp, h)


def _cells(G, mrange, mspacing):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        mesh = G.mesher.PrismMesh(mrange, mspacing)
    return mesh.cell_bounds(active_only=True)


def _joint_engine(G, obs, cells, mangle=MANGLE):
    from gravinv3dhmc_amd import _lib, utils
    n, m = obs[0].size, cells.shape[0]
    eng = G.Engine(2 * n, 2 * m)
    eng.set_cells(cells, _lib.CELL_PRISM_JOINT, direction=utils.dircos(*mangle))
    eng.set_obs(*obs)
    eng.build_G()
    return eng


def _single(G, obs, cells, tf, mangle=MANGLE):
    from gravinv3dhmc_amd import _lib, utils
    eng = G.Engine(obs[0].size, cells.shape[0])
    eng.set_obs(*obs)
    if tf:
        eng.set_cells(cells, _lib.CELL_PRISM_TF, direction=utils.dircos(*mangle))
    else:
        eng.set_cells(cells, _lib.CELL_PRISM)
    eng.build_G()
    return eng


# ----------------------------------------------------------------------------- assembly

@pytest.mark.parametrize("geom", ["small", "odd", "c1"])
def test_joint_store_blocks_bit_identical(G, geom):
    if geom == "small":
        obs, cells = _grid(6, 5), _cells(G, (0, 2000, 0, 3000, 0, 900), (300, 750, 500))
    elif geom == "odd":
        obs, cells = _grid(7, 6, 2100, 2500, -25.0), _cells(G, (0, 2100, 0, 2500, 0, 900), (300, 500, 300))
    else:  # C1: 600 observations x 6000 prisms
        obs, cells = _grid(30, 20), _cells(G, (0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    m = cells.shape[0]
    je = _joint_engine(G, obs, cells)
    H = je.download_G()
    assert H.shape == (obs[0].size, 2 * m)
    gz = _single(G, obs, cells, tf=False)
    tf = _single(G, obs, cells, tf=True)
    assert np.array_equal(H[:, :m], gz.download_G())
    assert np.array_equal(H[:, m:], tf.download_G())
    for e in (je, gz, tf):
        e.close()


# ----------------------------------------------------------------------------- module against the reference

def _module(G, z, g, **kw):
    xp, yp, zp = z[g + "_xp"], z[g + "_yp"], z[g + "_zp"]
    return G.JointModule(z[g + "_dobs_gz"], z[g + "_dobs_tf"], tuple(z[g + "_mrange"]), tuple(z[g + "_mspacing"]),
                         (xp, yp, zp), mangle=tuple(z["mangle"]), verbose=False, **kw)


@pytest.mark.parametrize("geom", ["a", "b"])
def test_joint_module_matches_reference(G, geom):
    z = gold("joint_small.npz")
    g = geom + "_"
    jm = _module(G, z, geom)
    assert relmax(jm.Wm.diagonal(), z[g + "wm"]) <= 1e-11
    std = jm._engine.joint_std()
    assert abs(std[0] - z[g + "std"][0]) <= 1e-13 * z[g + "std"][0]
    assert abs(std[1] - z[g + "std"][1]) <= 1e-13 * z[g + "std"][1]
    s_ref = z[g + "std"][0] / z[g + "std"][1]
    assert abs(jm.Wb.diagonal()[-1] - s_ref) <= 1e-13 * s_ref
    assert relmax(jm.Wb.diagonal(), z[g + "wb"]) <= 1e-13
    assert relmax(np.asarray(jm.Aw), z[g + "Aw"]) <= 1e-10
    assert relmax(jm.dobsw, z[g + "dobsw"]) <= 1e-10
    assert relmax(jm.A, z[g + "A"]) <= 1e-10
    mwapr = z[g + "mwapr"]
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        for k, x in enumerate(z[g + "xs"]):
            mis, grad, dpre, dv, mv = jm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, float(z["alpha"]),
                                                         regulization=reg, beta=float(z["beta"]))
            assert abs(mis - z[g + reg + "_misfit"][k]) <= 1e-10 * abs(z[g + reg + "_misfit"][k]), reg
            assert abs(dv - z[g + reg + "_data"][k]) <= 1e-10 * abs(z[g + reg + "_data"][k]), reg
            assert abs(mv - z[g + reg + "_model"][k]) <= 1e-10 * max(abs(z[g + reg + "_model"][k]), 1e-300), reg
            assert relmax(grad, z[g + reg + "_grad"][k]) <= 1e-10, reg
            assert relmax(dpre, z[g + reg + "_dpre"][k]) <= 1e-10, reg
    for bad in ("MS1", "MStry"):
        with pytest.raises(ValueError):
            jm.misfit_and_grad(z[g + "xs"][0], mwapr, None, None, "mandatory", 1000, 0.7, regulization=bad)
    # the unweighted forward
    model = z[g + "xs"][1] / z[g + "wm"]
    assert relmax(jm.forward(model), z[g + "A"] @ model) <= 1e-10
    jm._engine.close()


# ----------------------------------------------------------------------------- forward / adjoint

def _host_reg(kind, v, wm2, beta, R):
    """Value and gradient of one regulariser at v = mw - mwapr (potential.py:1690-1778; Smoothness and TV with
    the block-diagonal operator R = fd3djoint)."""
    if kind == "Damping":
        return v @ v, 2 * v
    if kind == "MS":
        den = v * v + beta
        return np.sum(wm2 * v * v / den), 2 * beta * wm2 * v / den ** 2
    t = R @ v
    if kind == "Smoothness":
        return t @ t, 2 * (R.T @ t)
    u = np.sqrt(t * t + beta)
    return np.sum(u), R.T @ (t / u)


# n = 600 (< 2048 rows) with 400 cells per block: one epilogue stage (at most 64 slab rows per block); n = 600 with
# 2400 cells per block: two stages (slab rows folded into segments first); n = 2400 (>= 2048 rows): one stage
@pytest.mark.parametrize("n_y,n_x,mspacing,stages", [(30, 20, (250, 300, 200), 1), (30, 20, (250, 100, 100), 2),
                                                     (60, 40, (250, 100, 100), 1)])
def test_joint_forward_adjoint_potential_against_host_products(G, n_y, n_x, mspacing, stages):
    from gravinv3dhmc_amd.inversion.joint import fd3d
    import scipy.sparse as sp
    obs = _grid(n_y, n_x)
    mrange = (0, 2000, 0, 3000, 0, 1000)
    cells = _cells(G, mrange, mspacing)
    shape = (int(round(1000 / mspacing[0])), int(round(3000 / mspacing[1])), int(round(2000 / mspacing[2])))
    n, m = obs[0].size, cells.shape[0]
    assert m == shape[0] * shape[1] * shape[2]
    eng = _joint_engine(G, obs, cells)
    assert eng.joint_layout()["epilogue_stages"] == stages
    wm = eng.weight(0.5)
    H = eng.download_G()
    Hg, Ht = H[:, :m], H[:, m:]
    rng = np.random.default_rng(3)
    x = rng.normal(size=2 * m)
    d = eng.forward(x)
    ref = np.concatenate([Hg @ x[:m], Ht @ x[m:]])
    assert relmax(d, ref) <= 1e-12
    r = rng.normal(size=2 * n)
    g = eng.adjoint(r)
    ref = np.concatenate([Hg.T @ r[:n], Ht.T @ r[n:]])
    assert relmax(g, ref) <= 1e-12
    # the potential through the epilogue of this layout: |H x - dobsw|^2 + alpha R, no mean removal, every
    # regulariser (Smoothness / TV per property, fd3djoint)
    dobsw = rng.normal(size=2 * n)
    eng.set_data(dobsw)
    R = sp.block_diag([fd3d(shape)] * 2, format="csr")
    mwapr = rng.normal(size=2 * m) * 0.1
    res = np.concatenate([Hg @ x[:m], Ht @ x[m:]]) - dobsw
    gdata = 2 * np.concatenate([Hg.T @ res[:n], Ht.T @ res[n:]])
    alpha, beta = 0.5, 0.01
    for kind in ("Damping", "MS", "Smoothness", "TV"):
        eng.set_reg(kind, alpha, beta, shape, mwapr)
        mis, grad, dpre, dv, mv = eng.misfit_and_grad(x)
        rv, rg = _host_reg(kind, x - mwapr, wm * wm, beta, R)
        assert relmax(dpre, res + dobsw) <= 1e-12, kind
        assert abs(dv - res @ res) <= 1e-12 * (res @ res), kind
        assert abs(mv - rv) <= 1e-12 * abs(rv), kind
        assert abs(mis - (res @ res + alpha * rv)) <= 1e-12 * abs(mis), kind
        assert relmax(grad, gdata + alpha * rg) <= 1e-11, kind
    eng.close()


# ----------------------------------------------------------------------------- sampling

@pytest.mark.parametrize("resident", ["1", "0"])
def test_joint_hmcsample_end_to_end(G, tmp_path, capsys, monkeypatch, resident):
    """Whole chains on the joint module against the reference's own runs, on the fused sweep whatever
    GRAVHMC_RESIDENT says (the resident chain kernel never takes a joint context)."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    c = gold("chain_small_joint.npz")
    z = gold("joint_small.npz")
    for tag in ("a", "b"):
        jm = _module(G, z, "a")
        M2 = jm.Wm.shape[0]
        dt, Sigma, lo, hi, n = c[tag + "_cfg"]
        folder = str(tmp_path / ("run_%s_chain" % tag))
        capsys.readouterr()
        G.HMCSample(jm, int(n), 0, float(dt), [5, 20], np.full(M2, 0.001 + lo), np.full(M2, 0.001),
                    np.c_[np.full(M2, lo), np.full(M2, hi)], "mandatory", 1000, jm.dobs,
                    "Fixed", 0.8, 1.0, str(c[tag + "_reg"]), 0.001, 100, float(Sigma), nbest=100,
                    myrank=0, save_folder=folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        assert lines == [str(s) for s in c[tag + "_lines"]]
        np.testing.assert_allclose(np.loadtxt(folder + "0/misfit.dat"), c[tag + "_misfit"], atol=2e-8, rtol=1e-9)
        np.testing.assert_allclose(np.loadtxt(folder + "0/model.dat"), c[tag + "_model"], atol=2e-8)
        st = jm._engine.chain_stats()
        assert st["resident_launches"] == 0 and st["team_launches"] == 0
        jm._engine.close()


# ----------------------------------------------------------------------------- refusals

def test_joint_refusals(G):
    from gravinv3dhmc_amd import _lib, utils
    lib = _lib.load()
    obs, cells = _grid(6, 5), _cells(G, (0, 2000, 0, 3000, 0, 900), (300, 750, 500))
    n, m = obs[0].size, cells.shape[0]
    d = utils.dircos(*MANGLE)
    b = np.ascontiguousarray(cells)
    ptr = _lib.ptr

    def ctx(N, M):
        h = C.c_void_p()
        assert lib.gh_create(C.byref(h), 0, N, M) == _lib.GH_OK
        return h

    # odd N or M
    for N, M in ((2 * n + 1, 2 * m), (2 * n, 2 * m + 1)):
        h = ctx(N, M)
        assert lib.gh_set_cells_joint(h, ptr(b), *d) == _lib.GH_ERR_ARG
        lib.gh_destroy(h)
    # more than 16384 observations per block
    h = ctx(2 * 16400, 2 * m)
    assert lib.gh_set_cells_joint(h, ptr(b), *d) == _lib.GH_ERR_UNSUPPORTED
    lib.gh_destroy(h)
    # matrix-free / shift-invariant asked for first
    for fn in (lib.gh_set_matrix_free, lib.gh_set_shift_invariant):
        h = ctx(2 * n, 2 * m)
        assert fn(h, 1) == _lib.GH_OK
        assert lib.gh_set_cells_joint(h, ptr(b), *d) == _lib.GH_ERR_UNSUPPORTED
        lib.gh_destroy(h)
    # gh_set_cells keeps refusing kind 5
    h = ctx(2 * n, 2 * m)
    big = np.ascontiguousarray(np.vstack([cells, cells]))
    assert lib.gh_set_cells(h, ptr(big), _lib.CELL_PRISM_JOINT, 1.6) == _lib.GH_ERR_ARG
    lib.gh_destroy(h)
    # on a built joint context
    eng = _joint_engine(G, obs, cells)
    h = eng._h
    assert lib.gh_set_matrix_free(h, 1) == _lib.GH_ERR_UNSUPPORTED
    assert lib.gh_set_shift_invariant(h, 1) == _lib.GH_ERR_UNSUPPORTED
    A = np.zeros((2 * n, 2 * m), order="F")
    assert lib.gh_upload_G(h, ptr(A), 2 * n, 1) == _lib.GH_ERR_UNSUPPORTED
    cb = _lib.ALLREDUCE_FN(lambda *a: 0)
    fn = C.cast(cb, C.c_void_p)
    assert lib.gh_shard_init_callback(h, fn, None, 0, 1, 2 * m, 0) == _lib.GH_ERR_UNSUPPORTED
    assert lib.gh_shard_init_rows_callback(h, fn, None, 0, 1, 2 * n, 0) == _lib.GH_ERR_UNSUPPORTED
    eng.weight(0.5)
    eng.set_data(np.zeros(2 * n))
    eng.set_reg("Damping", 1.0, 0.01, None, np.zeros(2 * m))
    nnz, nc = C.c_int64(0), C.c_int64(0)
    shp = (C.c_int * 3)(3, 4, 4)
    assert lib.gh_compress_wavelet(h, 1, shp, 1e-3, 2, C.byref(nnz), C.byref(nc)) == _lib.GH_ERR_UNSUPPORTED
    x0 = np.zeros((2, 2 * m))
    assert lib.gh_batch_init(h, 2, ptr(x0), ptr(x0[0]), ptr(x0[0])) == _lib.GH_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        eng.set_reg("Smoothness", 1.0, 0.01, (3, 4, 8), np.zeros(2 * m))   # prod == M, not M/2
    eng.close()
    z = gold("joint_small.npz")
    jm = _module(G, z, "a")
    M2 = jm.Wm.shape[0]
    with pytest.raises(NotImplementedError):
        G.HMCSampleBatch(jm, 2, 2, 0, 0.01, [5, 20], np.full(M2, 0.001), np.full(M2, 0.001),
                         np.c_[np.zeros(M2), np.ones(M2)], "mandatory", 1000, jm.dobs, "Fixed", 0.8, 1.0,
                         "Damping", 0.001, 100, 0.001)
    jm._engine.close()
