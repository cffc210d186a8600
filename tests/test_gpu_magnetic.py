"""GPU suite of the total-field magnetic field on prisms (GH_CELL_PRISM_TF): entries and results
against the reference's _prism.tf / prism.tf, the magnetic GravMagModule and HMCSample against the
reference's own runs, and the paths that consume a stored or computed kernel against each other.

Tolerances are the gravity suite's (tests/test_gpu_parity.py): entries |dK| <= 1e-10 max|K|;
potential 1e-10 relative; matrix-free against dense 1e-12 (summation order differs)."""
import os

import numpy as np
import pytest

from conftest import gold
from helpers import c1_inputs, relmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _tf_engine(G, xp, yp, zp, cells, inc, dec, matrix_free=False):
    from gravinv3dhmc_amd import _lib, utils
    eng = G.Engine(np.asarray(xp).size, np.asarray(cells).shape[0])
    if matrix_free:
        eng.set_matrix_free(True)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(cells, _lib.CELL_PRISM_TF, direction=utils.dircos(inc, dec))
    return eng


def _module(G, p, **kw):
    return G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]),
                           field="magnetic", mangle=tuple(p["mangle"]), verbose=False, **kw)


# ----------------------------------------------------------------------------- entries / results

def test_tf_entries_and_results_against_the_reference(G):
    from gravinv3dhmc_amd import mesher
    g = gold("prism_tf_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    worst = 0.0
    for d, (inc, dec) in enumerate(g["dirs"]):
        eng = _tf_engine(G, xp, yp, zp, cells, inc, dec)
        eng.build_G()
        K = eng.download_G()
        assert np.isfinite(K).all()
        err = np.abs(K - g["K%d" % d]).max() / np.abs(g["K%d" % d]).max()
        worst = max(worst, err)
        assert err <= 1e-10, (inc, dec, err)
        res = eng.tf_result(g["mag"])                       # gh_tf_result: needs no G, works after it too
        assert np.isfinite(res).all() and relmax(res, g["res_vec%d" % d]) <= 1e-10
        eng.close()
        # prism.tf on a list of prisms: vectors, intensities along the field, a cell without the property, pmag
        mag, scal = g["mag"], g["scal"]
        props = [{"magnetization": float(scal[0])}, {"magnetization": list(mag[1])}, None,
                 {"magnetization": float(scal[3])}]
        prisms = [mesher.Prism(*b, props=p) for b, p in zip(cells, props)]
        r, K3 = G.prism.tf(xp, yp, zp, prisms, inc, dec)
        assert relmax(r, g["res_mixed%d" % d]) <= 1e-10
        assert K3.shape == (xp.size, 3) and K3.flags.f_contiguous
        assert np.abs(K3 - g["K%d" % d][:, [0, 1, 3]]).max() <= 1e-10 * np.abs(g["K%d" % d]).max()
        r, K4 = G.prism.tf(xp, yp, zp, [mesher.Prism(*b) for b in cells], inc, dec, pmag=2.5)
        assert relmax(r, g["res_pmag%d" % d]) <= 1e-10 and K4.shape == (xp.size, 4)
        r, none = G.prism.tf(xp, yp, zp, prisms, inc, dec, pmag=[0.3, -1.2, 0.8], return_kernel=False)
        assert relmax(r, g["res_pvec%d" % d]) <= 1e-10 and none is None
    print("tf entries: max |dK|/max|K| = %.3e" % worst)
    with pytest.raises(ValueError):
        G.prism.tf(xp, yp, zp, [mesher.Prism(*cells[0])], 90.0, 0.0)     # no cell has the property


def test_c1_tf_columns_against_the_reference(G):
    from gravinv3dhmc_amd import utils
    g = gold("c1_tf_columns.npz")
    mesh, xp, yp, zp = c1_inputs()
    inc, dec = g["mangle"]
    mesh.addprop("magnetization", utils.ang2vec(np.zeros(mesh.size), inc, dec))
    res, K = G.prism.tf(xp, yp, zp, mesh, inc, dec)
    assert K.shape == (600, 6000) and np.isfinite(K).all()
    assert np.array_equal(res, np.zeros(600))                # zero magnetization
    err = np.abs(K[:, g["cols"]] - g["K"]).max() / np.abs(g["K"]).max()
    print("C1 tf columns: max |dK|/max|K| = %.3e" % err)
    assert err <= 1e-10


def test_set_cells_keeps_refusing_the_magnetic_kind(G):
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(3, 1)
    with pytest.raises(ValueError):
        eng.set_cells(np.array([[0, 1, 0, 1, 0, 1.0]]), _lib.CELL_PRISM_TF)          # no direction
    with pytest.raises(ValueError):
        eng._chk(eng._lib.gh_set_cells(eng._h, _lib.ptr(np.array([0, 1, 0, 1, 0, 1.0])), 2, 1.0))
    eng.set_cells(np.array([[0, 1, 0, 1, 0, 1.0]]), _lib.CELL_PRISM)
    eng.set_obs(np.zeros(3), np.zeros(3), np.full(3, -1.0))
    with pytest.raises(ValueError):
        eng.tf_result(np.ones((1, 3)))                       # a gravity context
    eng.close()


# ----------------------------------------------------------------------------- the module

def test_magnetic_module_weights_and_potential_golden(G, capsys):
    p = gold("potential_small_tf.npz")
    gm = G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]),
                         field="magnetic", mangle=tuple(p["mangle"]))
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Calculating magnetic field in cartesian coordinate."
    assert not any(l.startswith("kernel.shape") for l in out)           # (potential.py:144-149)
    assert any(l.startswith("End of calculate kernel: ") for l in out)
    assert "magnetization" in gm.mesh.props and "density" not in gm.mesh.props
    assert relmax(gm.Wm.diagonal(), p["wm"]) < 1e-11
    assert relmax(np.asarray(gm.Aw), p["Aw"]) < 1e-10
    worst = 0.0
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        for i, x in enumerate(p["xs"]):
            m, grad, dpre, dv, mv = gm.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000,
                                                       float(p["alpha"]), regulization=reg, beta=float(p["beta"]))
            errs = [abs(m - p[reg + "_misfit"][i]) / abs(m), relmax(grad, p[reg + "_grad"][i]),
                    relmax(dpre, p[reg + "_dpre"][i]), abs(dv - p[reg + "_data"][i]) / abs(dv),
                    abs(mv - p[reg + "_model"][i]) / max(abs(mv), 1e-300)]
            worst = max(worst, max(errs))
            assert max(errs) < 1e-10, (reg, i, errs)
    print("magnetic misfit_and_grad worst rel err %.3e" % worst)
    gm._engine.close()


def _hmc(G, gm, p, c, tag, folder):
    M = p["wm"].size
    dt, Sigma, lo, hi, n = c[tag + "_cfg"]
    G.HMCSample(gm, int(n), 0, float(dt), [5, 20], np.full(M, 0.001 + lo), np.full(M, 0.001),
                np.c_[np.full(M, lo), np.full(M, hi)], "mandatory", 1000, p["dobs"],
                "Fixed", 0.8, 1.0, str(c[tag + "_reg"]), 0.001, 100, float(Sigma), nbest=100,
                myrank=0, save_folder=folder)


@pytest.mark.parametrize("resident", ["1", "0"])
def test_magnetic_hmcsample_end_to_end(G, tmp_path, capsys, monkeypatch, resident):
    """Whole chains on the magnetic module against the reference's own runs; the resident chain
    kernel ("1") and the sweep path ("0") both give the reference's lines."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    c = gold("chain_small_tf.npz")
    p = gold("potential_small_tf.npz")
    for tag in ("a", "b"):
        gm = _module(G, p)
        folder = str(tmp_path / ("run_%s_chain" % tag))
        capsys.readouterr()
        _hmc(G, gm, p, c, tag, folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        assert lines == [str(s) for s in c[tag + "_lines"]]
        np.testing.assert_allclose(np.loadtxt(folder + "0/misfit.dat"), c[tag + "_misfit"], atol=2e-8, rtol=1e-9)
        np.testing.assert_allclose(np.loadtxt(folder + "0/model.dat"), c[tag + "_model"], atol=2e-8)
        gm._engine.close()


def test_magnetic_lockstep_batch_matches_single_chain_engines(G):
    p = gold("potential_small_tf.npz")
    gm = _module(G, p)
    eng = gm._engine
    wm = gm.Wm.diagonal()
    M = wm.size
    eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
    rng = np.random.default_rng(7)
    C, T = 3, 3
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    low, high = 0.0 * wm, 0.02 * wm
    Ls = rng.integers(2, 9, size=(C, T))
    p0s = rng.normal(size=(C, T, M)) * 0.3
    us = rng.uniform(size=(C, T))
    eng.batch_init(x0s, low, high)
    accb, outb, _ = eng.batch_run(p0s, 0.02, Ls, us)
    single = _module(G, p)._engine
    single.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
    for c in range(C):
        x = x0s[c]
        for t in range(T):
            x, acc, o, _ = single.leapfrog(x, p0s[c, t], 0.02, int(Ls[c, t]), low, high, float(us[c, t]))
            assert bool(accb[c, t]) == acc and abs(outb[c, t, 0] - o[0]) <= 1e-10 * abs(o[0])
        assert relmax(eng.batch_get_x(c), x) <= 1e-10
    eng.close()
    single.close()


# ----------------------------------------------------------------------------- matrix-free

@pytest.mark.parametrize("fused", ["1", "0"])
def test_matrix_free_magnetic_matches_dense(G, monkeypatch, fused):
    monkeypatch.setenv("GRAVHMC_MF_FUSED", fused)
    p = gold("potential_small_tf.npz")
    dense = _module(G, p)
    mf = _module(G, p, matrix_free=True)
    assert relmax(mf.Wm.diagonal(), dense.Wm.diagonal()) < 1e-13
    wm = dense.Wm.diagonal()
    M = wm.size
    x = p["xs"][1]
    assert relmax(mf._engine.forward(x), dense._engine.forward(x)) < 1e-12
    r = np.random.default_rng(0).normal(size=p["dobs"].size)
    assert relmax(mf._engine.adjoint(r), dense._engine.adjoint(r)) < 1e-12
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        a = mf.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) < 1e-12 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11
    rng = np.random.default_rng(4)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(8)]
    outs = []
    for m in (mf, dense):
        e = m._engine
        e.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        e.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        res = []
        e.run_chain(iter(trajs), 0.02, lambda L, acc, o, x, res=res: res.append((acc, o.copy(), x)), want_x=True)
        outs.append(res)
    for (a1, o1, x1), (a2, o2, x2) in zip(*outs):
        assert a1 == a2 and relmax(o1, o2) < 1e-12 and (x1 is None or relmax(x1, x2) < 1e-12)
    # the matrix-free batch of chains has no magnetic kernels: refused, never run on gz entries
    with pytest.raises(NotImplementedError, match="magnetic"):
        mf._engine.batch_init(np.stack([0.001 * wm, 0.002 * wm]), 0.0 * wm, 0.02 * wm)
    mf._engine.close()
    dense._engine.close()


def test_wavelet_forward_on_matrix_free_magnetic_model_matches_dense(G):
    p = gold("potential_small_tf.npz")
    dense = _module(G, p, wavelet="3D")
    mf = _module(G, p, wavelet="3D", matrix_free=True)
    cd, cm = dense.Awcp, mf.Awcp
    assert cd.nnz == cm.nnz and np.array_equal(cd.indices, cm.indices) and relmax(cm.data, cd.data) < 1e-12
    x = p["xs"][1]
    assert relmax(mf._engine.forward_wavelet(x), dense._engine.forward_wavelet(x)) < 1e-12
    for reg in ("Damping", "TV"):
        a = mf.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) < 1e-12 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11
    mf._engine.close()
    dense._engine.close()


# ----------------------------------------------------------------------------- refusals / shards

def test_magnetic_refusals(G):
    p = gold("potential_small_tf.npz")
    with pytest.raises(NotImplementedError):
        _module(G, p, shift_invariant=True)
    with pytest.raises(NotImplementedError, match="magnetic"):
        G.GravMagModule(p["dobs"], (0, 10, -5, 5, 0, -10000), (5000, 5, 5), (p["xp"], p["yp"], p["zp"]),
                        coordinate="spherical", field="magnetic", verbose=False)


def test_sharded_engine_rccl_world1_is_bitwise_unsharded_on_the_magnetic_kernel(G, monkeypatch):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    from gravinv3dhmc_amd import _lib, mesher, utils
    from gravinv3dhmc_amd.dist import Ranks, make_sharded_engine
    p = gold("potential_small_tf.npz")
    env = {k: os.environ.pop(k, None) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        ranks = Ranks()
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    bounds = mesher.PrismMesh(tuple(p["mrange"]), tuple(p["mspacing"])).cell_bounds()
    N, M = p["dobs"].size, bounds.shape[0]
    f = utils.dircos(*p["mangle"])

    def setup(eng):
        eng.set_obs(p["xp"], p["yp"], p["zp"])
        eng.set_cells(bounds, _lib.CELL_PRISM_TF, direction=f)
        eng.build_G()
        w = eng.weight(0.5)
        eng.set_data(p["dobs"])
        eng.set_reg("MS", 1.0, 0.001, p["shape"], 0.001 * w)
        eng.chain_init(0.001 * w, 0.0 * w, 0.02 * w)
        return w

    a = make_sharded_engine(N, M, ranks, device=0, backend="rccl")
    b = G.Engine(N, M)
    wa, wb = setup(a), setup(b)
    assert np.array_equal(wa, wb) and relmax(wb, p["wm"]) < 1e-11
    rng = np.random.default_rng(2)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(10)]
    ra, rb = [], []
    a.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: ra.append((acc, o.copy(), x)), want_x=True)
    b.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: rb.append((acc, o.copy(), x)), want_x=True, batch=3)
    for (a1, o1, x1), (a2, o2, x2) in zip(ra, rb):
        assert a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2))
    x = rng.uniform(0, 1, M) * wb
    assert np.array_equal(a.forward(x), b.forward(x))
    ma, mb = a.misfit_and_grad(x), b.misfit_and_grad(x)
    assert ma[0] == mb[0] and np.array_equal(ma[1], mb[1])
    a.close()
    b.close()
