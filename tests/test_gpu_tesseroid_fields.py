"""GPU suite of the tesseroid gravity fields other than gz (GH_CELL_TESSEROID_COMP): entries, results and
warnings against the reference's gravmag.tesseroid.<field> (tests/make_golden_tess.py), the leaf counts
against the oracle's subdivision, and the paths that consume a stored or computed kernel against each other.

Tolerances: entries |dK| <= 1e-10 max|K| and results 1e-10 relative against the reference (the leaf's powers
l**1.5 / l**2.5 are l*sqrt(l) / (l*l)*sqrt(l), not Python's pow: restated in Python on the near-field case that form
moves the entries by 3e-16 of max|K|); matrix-free against dense 1e-12 (the summation order differs); chains 1e-9.
One exception, NEAR_TENSOR: the gradient tensor of the near-field case ("n": observations 0.5 to 5 km from cells a
few km thick, ratio 8) is a sum of leaf terms of ~1/l^3 that cancel by about six orders of magnitude, so the
last-bit differences between the device's sin / cos / acos and the host's at the GLQ nodes reach 1.2e-9 of max|K|
there (measured); those entries are held to 1e-8."""
import os
import warnings

import numpy as np
import pytest

from conftest import gold
from helpers import relmax

pytestmark = pytest.mark.gpu

FIELDS = ("potential", "geoid", "gx", "gy", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
RATIO = {"potential": 1, "geoid": 1, "gx": 1.6, "gy": 1.6}
NEAR_TENSOR = 1e-8


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _case(G, g, case):
    """(lon, lat, h, model, kwargs) of a fixture case, the model rebuilt with this package's mesher."""
    from gravinv3dhmc_amd import mesher
    if case == "g":
        mesh = mesher.TesseroidMesh(tuple(g["g_area"]), tuple(g["g_spacing"]))
        mesh.addprop("density", g["g_rho"])
        assert np.array_equal(mesh.cell_bounds(), g["g_bounds"])
        return g["g_lon"], g["g_lat"], g["g_h"], mesh, {}
    cells = g[case + "_cells"]
    model = [mesher.Tesseroid(*c, props={"density": float(d)}) for c, d in zip(cells, g[case + "_rho"])]
    if case == "d":
        model.insert(int(g["d_none"]), None)
        return g["d_lon"], g["d_lat"], g["d_h"], model, {"dens": float(g["d_dens"])}
    return g[case + "_lon"], g[case + "_lat"], g[case + "_h"], model, {}


def _warnings(fn, *a, **k):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn(*a, **k)
    return out, [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]


@pytest.mark.parametrize("case", ["g", "n", "d"])
@pytest.mark.parametrize("field", FIELDS)
def test_field_entries_results_and_warnings_against_the_reference(G, field, case):
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    lon, lat, h, model, kw = _case(G, g, case)
    K_ref, r_ref, nwarn = g["%s_K_%s" % (case, field)], g["%s_result_%s" % (case, field)], int(g["%s_warn_%s" % (case, field)])
    (res, K), msgs = _warnings(getattr(tesseroid, field), lon, lat, h, model, **kw)
    assert K.shape == K_ref.shape and res.shape == r_ref.shape
    tol = NEAR_TENSOR if (case == "n" and RATIO.get(field, 8) == 8) else 1e-10
    assert relmax(K, K_ref) <= tol, relmax(K, K_ref)
    assert relmax(res, r_ref) <= tol, relmax(res, r_ref)
    # the reference warns once per cell (each message); the frontends warn each message once, as gz does
    small = 1 if case == "d" else 0                        # (the degenerate cell of the "d" case)
    assert sum("Ignoring this tesseroid" in m for m in msgs) == small
    assert any("Stopped dividing" in m for m in msgs) == (nwarn - small > 0)
    # without the kernel: the matrix-free forward, the same warnings
    (res2, K2), msgs2 = _warnings(getattr(tesseroid, field), lon, lat, h, model, return_kernel=False, **kw)
    assert K2 is None and relmax(res2, r_ref) <= tol and relmax(res2, res) <= 1e-12
    assert sorted(set(msgs2)) == sorted(set(msgs))


@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("field", FIELDS)
def test_warn_cells_and_leaves_are_the_references_subdivision(G, field, matrix_free):
    from oracle import oracle
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    ratio = RATIO.get(field, 8)
    for case in ("g", "n"):
        lon, lat, h, model, kw = _case(G, g, case)
        eng, _, ndrop = tesseroid.build_engine(lon, lat, h, model, ratio=ratio, component=field,
                                               matrix_free=matrix_free)
        st = eng.kernel_stats()
        eng.close()
        bounds = np.asarray([c.get_bounds() for c in model]) if case == "n" else model.cell_bounds()
        _, info = oracle.tess_gz_kernel(lon, lat, h, bounds, ratio=ratio, return_info=True)
        assert ndrop == 0 and st["leaves"] == info["leaves"], (case, st, info)
        assert st["warn_cells"] == int(g["%s_warn_%s" % (case, field)]) == info["err_cells"], (case, st, info)


def test_gz_through_the_component_entry_point_is_bitwise_the_tesseroid_kind(G):
    from gravinv3dhmc_amd import _lib
    g = gold("tess_comp_cases.npz")
    lon, lat, h, cells = g["n_lon"], g["n_lat"], g["n_h"], g["n_cells"]
    a = G.Engine(lon.size, cells.shape[0])
    a.set_obs(lon, lat, h)
    a._chk(a._lib.gh_set_cells_tess(a._h, _lib.ptr(np.ascontiguousarray(cells)), _lib.COMP_GZ, 1.6))
    b = G.Engine(lon.size, cells.shape[0])
    b.set_obs(lon, lat, h)
    b.set_cells(cells, _lib.CELL_TESSEROID, 1.6)
    a.build_G()
    b.build_G()
    assert np.array_equal(a.download_G(), b.download_G())
    assert a.kernel_stats() == b.kernel_stats()
    a.close()
    b.close()


def _engine(G, lon, lat, h, bounds, field, matrix_free=False):
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(np.asarray(lon).size, np.asarray(bounds).shape[0])
    if matrix_free:
        eng.set_matrix_free(True)
    eng.set_obs(lon, lat, h)
    eng.set_cells(bounds, _lib.CELL_TESSEROID, RATIO.get(field, 8), component=field)
    eng.build_G()
    return eng


@pytest.mark.parametrize("field", ["gx", "gy", "gxy", "gzz", "potential"])
def test_matrix_free_forward_adjoint_and_column_norms_match_dense(G, field):
    g = gold("tess_comp_cases.npz")
    lon, lat, h, b = g["g_lon"], g["g_lat"], g["g_h"], g["g_bounds"]
    dense, mf = _engine(G, lon, lat, h, b, field), _engine(G, lon, lat, h, b, field, matrix_free=True)
    rng = np.random.default_rng(3)
    x = rng.uniform(0.1, 0.5, b.shape[0])
    assert relmax(mf.forward(x), dense.forward(x)) <= 1e-12
    wd, wf = dense.weight(0.5), mf.weight(0.5)
    assert relmax(wf, wd) <= 1e-12
    assert relmax(mf.forward(x), dense.forward(x)) <= 1e-12
    r = rng.normal(size=lon.size)
    assert relmax(mf.adjoint(r), dense.adjoint(r)) <= 1e-12
    dense.close()
    mf.close()


def test_return_kernel_false_beyond_16384_observations(G):
    """N > 16384: no dense assembly fits one device; the matrix-free forward gives the dense result of the
    same rows assembled in blocks of <= 16384."""
    from gravinv3dhmc_amd import mesher
    from gravinv3dhmc_amd.gravmag import tesseroid
    mesh = mesher.TesseroidMesh((-180, 180, -90, 90, 0, -1e6), (-1e6, 90, 120))
    mesh.addprop("density", np.linspace(0.1, 0.6, mesh.size))
    rng = np.random.default_rng(5)
    N = 16500
    lon, lat, h = rng.uniform(-180, 180, N), rng.uniform(-89, 89, N), np.full(N, 250000.0)
    res, K = tesseroid.gzz(lon, lat, h, mesh, return_kernel=False)
    assert K is None and res.shape == (N,)
    ref = np.concatenate([tesseroid.gzz(lon[i:i + 16384], lat[i:i + 16384], h[i:i + 16384], mesh)[0]
                          for i in range(0, N, 16384)])
    assert relmax(res, ref) <= 1e-12


def _inversion(G, field, matrix_free):
    g = gold("tess_comp_cases.npz")
    lon, lat, h, b = g["g_lon"], g["g_lat"], g["g_h"], g["g_bounds"]
    eng = _engine(G, lon, lat, h, b, field, matrix_free)
    K = None if matrix_free else eng.download_G()
    wm = eng.weight(0.5)
    dobs = np.random.default_rng(11).normal(size=lon.size) * np.abs(eng.forward(0.3 * wm)).max()
    eng.set_data(dobs)
    return eng, K, wm, dobs


@pytest.mark.parametrize("field", ["gzz", "gx"])
def test_stored_kernel_inversion_against_numpy_and_matrix_free(G, field):
    from oracle import oracle
    from oracle.numpy_port import NumpyProblem
    shape = (2, 4, 6)                                      # (the "g" mesh: nr, nlat, nlon)
    eng, K, wm, dobs = _inversion(G, field, False)
    mf, _, wmf, _ = _inversion(G, field, True)
    Aw, wo = oracle.col_weight(K)
    assert relmax(wm, wo) <= 1e-11 and relmax(wmf, wm) <= 1e-12
    assert relmax(eng.download_G(), Aw) <= 1e-11          # (the weighted kernel, in place)
    M = wm.size
    rng = np.random.default_rng(2)
    for reg in ("Damping", "TV"):
        mwapr = 0.001 * wm
        for e in (eng, mf):
            e.set_reg(reg, 0.7, 0.001, shape, mwapr)
        P = oracle.Problem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape)
        for _ in range(2):
            x = rng.uniform(0, 0.5, M) * wm
            a, ref, b = eng.misfit_and_grad(x), P.misfit_and_grad(x), mf.misfit_and_grad(x)
            assert abs(a[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(a[1], ref[1]) <= 1e-10
            assert abs(b[0] - a[0]) <= 1e-12 * abs(a[0]) and relmax(b[1], a[1]) <= 1e-11
            if reg == "Damping":
                n = NumpyProblem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm).misfit_and_grad(x)
                assert abs(a[0] - n[0]) <= 1e-10 * abs(n[0]) and relmax(a[1], n[1]) <= 1e-10
        # chains: the same trajectories on the stored kernel, the matrix-free context and the restatement
        trajs = [(int(rng.integers(2, 8)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(6)]
        low, high, x0 = 0.0 * wm, 0.6 * wm, 0.1 * wm
        outs = []
        for e in (eng, mf):
            e.chain_init(x0, low, high)
            res = []
            e.run_chain(iter(trajs), 0.02, lambda L, acc, o, x, res=res: res.append((acc, o.copy())), batch=3)
            outs.append((res, e.chain_get_x()))
        xo = x0
        for k, (L, p0, u) in enumerate(trajs):
            xo, acco, oo, _ = P.leapfrog(xo, p0, 0.02, L, low, high, u)
            for res, _ in outs:
                assert res[k][0] == acco and abs(res[k][1][0] - oo[0]) <= 1e-9 * abs(oo[0])
        for _, x in outs:
            assert relmax(x, xo) <= 1e-9
    eng.close()
    mf.close()


def test_sharded_engine_world1_is_bitwise_unsharded_on_a_gzz_tesseroid_kernel(G, monkeypatch):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.dist import Ranks, make_sharded_engine
    g = gold("tess_comp_cases.npz")
    lon, lat, h, b = g["g_lon"], g["g_lat"], g["g_h"], g["g_bounds"]
    env = {k: os.environ.pop(k, None) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        ranks = Ranks()
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    N, M = lon.size, b.shape[0]

    def setup(eng):
        eng.set_obs(lon, lat, h)
        eng.set_cells(b, _lib.CELL_TESSEROID, 8, component="gzz")
        eng.build_G()
        w = eng.weight(0.5)
        eng.set_data(np.linspace(-1, 1, N))
        eng.set_reg("Damping", 1.0, 0.001, (2, 4, 6), 0.001 * w)
        eng.chain_init(0.1 * w, 0.0 * w, 0.6 * w)
        return w

    a = make_sharded_engine(N, M, ranks, device=0, backend="rccl")
    c = G.Engine(N, M)
    wa, wc = setup(a), setup(c)
    assert np.array_equal(wa, wc)
    rng = np.random.default_rng(2)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(6)]
    ra, rc = [], []
    a.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: ra.append((acc, o.copy(), x)), want_x=True)
    c.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: rc.append((acc, o.copy(), x)), want_x=True, batch=3)
    for (a1, o1, x1), (a2, o2, x2) in zip(ra, rc):
        assert a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2))
    x = rng.uniform(0, 1, M) * wc
    assert np.array_equal(a.forward(x), c.forward(x))
    a.close()
    c.close()


def test_refusals_name_the_component_and_never_fall_back(G):
    from gravinv3dhmc_amd import _lib
    g = gold("tess_comp_cases.npz")
    lon, lat, h, b = g["g_lon"], g["g_lat"], g["g_h"], g["g_bounds"]
    # the shift-invariant store
    eng = G.Engine(lon.size, b.shape[0])
    eng.set_shift_invariant(True)
    eng.set_obs(lon, lat, h)
    eng.set_cells(b, _lib.CELL_TESSEROID, 8, component="gzz")
    with pytest.raises(NotImplementedError, match="component"):
        eng.build_G()
    eng.close()
    # the matrix-free batch of chains
    mf = _engine(G, lon, lat, h, b, "gxy", matrix_free=True)
    wm = mf.weight(0.5)
    mf.set_data(np.zeros(lon.size))
    mf.set_reg("Damping", 1.0, 0.001, (2, 4, 6), 0.001 * wm)
    with pytest.raises(NotImplementedError, match="component"):
        mf.batch_init(np.stack([0.001 * wm, 0.002 * wm]), 0.0 * wm, 0.02 * wm)
    # the prism result pass; gh_set_cells keeps refusing kind 4; an unknown component
    with pytest.raises(NotImplementedError, match="component"):
        mf.prism_result(np.ones(b.shape[0]))
    with pytest.raises(ValueError):
        mf._chk(mf._lib.gh_set_cells(mf._h, _lib.ptr(np.ascontiguousarray(b)), _lib.CELL_TESSEROID_COMP, 8.0))
    with pytest.raises(ValueError):
        mf._chk(mf._lib.gh_set_cells_tess(mf._h, _lib.ptr(np.ascontiguousarray(b)), 11, 8.0))
    with pytest.raises(ValueError, match="ratio"):
        mf._chk(mf._lib.gh_set_cells_tess(mf._h, _lib.ptr(np.ascontiguousarray(b)), _lib.COMP_GZZ, 0.0))
    bad = np.ascontiguousarray(b.copy())
    bad[3, 4], bad[3, 5] = bad[3, 5], bad[3, 4]                                # top < bottom
    with pytest.raises(ValueError, match="invalid tesseroid dimensions"):
        mf._chk(mf._lib.gh_set_cells_tess(mf._h, _lib.ptr(bad), _lib.COMP_GZZ, 8.0))
    mf.close()


@pytest.mark.parametrize("return_kernel", [True, False])
def test_stack_overflow_raises(G, return_kernel):
    from gravinv3dhmc_amd import mesher
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    model = [mesher.Tesseroid(*c, props={"density": 1.0}) for c in g["o_cells"]]
    with pytest.raises(OverflowError):
        getattr(tesseroid, str(g["o_field"]))(g["o_lon"], g["o_lat"], g["o_h"], model, return_kernel=return_kernel)
