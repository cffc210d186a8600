"""GPU suite of the tesseroid magnetic fields: gravmag.tesseroid.bx / by / bz / tf and TesseroidMagVectorModule on the
GH_CELL_TESS_MVI_DATA store.

1. Entries: [K_N | K_E | K_D] against the composition V Q of the REFERENCE's tensor kernels (tests/golden/
   tess_comp_cases.npz, divided by the tensor's scale), Q written out here from the frames' definitions.  Tolerances
   are tests/test_gpu_tesseroid_fields.py's for these fixtures: 1e-10 max|K|, and NEAR_TENSOR = 1e-8 on the near-field
   case "n" for the reason stated there.  return_kernel=False against the dense result: 1e-12 (summation order).
2. Signs and frames: the point dipole, which shares no code with the engine.  The truncation error of the dipole
   model is of order (cell size / distance)^2 ~ (11 km / 1100 km)^2 = 1e-4: every component to 1e-3 |B|.
3. tf = f_o . (bx, by, bz): 1e-13 of max|tf| (three products and two sums of doubles).
4. The store as a vector-data store against the NumPy restatement tests/magvecdata_host.py on the downloaded
   weighted kernel: potential and gradient 1e-10, one 5-step trajectory 1e-9 (the chains' tolerance of the tesseroid
   suite).
5. Refusals and errors.
6. 17 observations x 5 cells (an odd ld padding, fewer cells than a wave, several workgroups) against the
   composition of tesseroid.gxx .. gzz on the same geometry: 1e-12 max|K| (the same sums; only the 3 x 3
   composition differs)."""
import warnings

import numpy as np
import pytest

from conftest import gold
from helpers import relmax
from magvecdata_host import VecDataProblem

pytestmark = pytest.mark.gpu

NEAR_TENSOR = 1e-8
TENSOR = ("gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
BCOMPS = ("bx", "by", "bz")
D2R = np.pi / 180.0


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


# ----------------------------------------------------------------------------- the definitions, written out

def _frames(lon, lat):
    """n, e, u (ECEF) at the points, (k, 3) each"""
    lam, phi = np.asarray(lon, dtype=float) * D2R, np.asarray(lat, dtype=float) * D2R
    n = np.stack([-np.sin(phi) * np.cos(lam), -np.sin(phi) * np.sin(lam), np.cos(phi)], axis=1)
    e = np.stack([-np.sin(lam), np.cos(lam), np.zeros_like(lam)], axis=1)
    u = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], axis=1)
    return n, e, u


def _Q(lon, lat, bounds):
    """Q[o, c] = [n_o e_o u_o]^T [n_c e_c -u_c], the cells' frames at the midpoints of their lon / lat bounds"""
    no, eo, uo = _frames(lon, lat)
    nc, ec, uc = _frames(0.5 * (bounds[:, 0] + bounds[:, 1]), 0.5 * (bounds[:, 2] + bounds[:, 3]))
    O = np.stack([no, eo, uo], axis=1)                       # (N, 3 rows, 3)
    Cc = np.stack([nc, ec, -uc], axis=2)                     # (m, 3, 3 columns)
    return np.einsum("ojk,cka->ocja", O, Cc)


def _compose(V, Q):
    """{bx, by, bz: [K_N | K_E | K_D]} from V[name] (N, m), unscaled, and Q (N, m, 3, 3)"""
    from gravinv3dhmc_amd import constants
    T = np.empty(Q.shape)
    for (i, j), name in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), TENSOR):
        T[:, :, i, j] = T[:, :, j, i] = V[name]
    B = constants.CM * constants.T2NT * np.einsum("ocij,ocja->ocia", T, Q)
    B[:, :, 2, :] *= -1.0                                    # z up -> bz down
    return {comp: np.hstack([B[:, :, r, a] for a in range(3)]) for r, comp in enumerate(BCOMPS)}


def _tensor_scale():
    from gravinv3dhmc_amd import constants
    return constants.SI2EOTVOS * constants.G


def _case(G, g, case):
    """(lon, lat, h, model with magnetization-free cells, bounds in column order, number of trailing zero columns)"""
    mesher = G.mesher
    if case == "g":
        mesh = mesher.TesseroidMesh(tuple(g["g_area"]), tuple(g["g_spacing"]))
        return g["g_lon"], g["g_lat"], g["g_h"], mesh, g["g_bounds"], 0
    cells = g[case + "_cells"]
    model = [mesher.Tesseroid(*c) for c in cells]
    w, e, s, n, top, bottom = cells.T
    tiny = ((e - w) <= 1e-6) | ((n - s) <= 1e-6) | ((top - bottom) <= 1e-3)
    if case == "d":
        model.insert(int(g["d_none"]), None)
    order = np.r_[np.flatnonzero(~tiny), np.flatnonzero(tiny)]
    return g[case + "_lon"], g[case + "_lat"], g[case + "_h"], model, cells[order], int(tiny.sum())


def _with_vectors(G, model, vec):
    """the model with one magnetization vector per (non-None) cell"""
    if hasattr(model, "addprop"):
        model.addprop("magnetization", vec)
        return model
    out, k = [], 0
    for c in model:
        if c is None:
            out.append(None)
            continue
        out.append(G.mesher.Tesseroid(*c.get_bounds(), props={"magnetization": vec[k]}))
        k += 1
    return out


def _warnings(fn, *a, **k):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn(*a, **k)
    return out, [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]


# ----------------------------------------------------------------------------- 1. entries against the reference

@pytest.fixture(scope="module")
def expected():
    """the composed kernels of every case, built once"""
    cache = {}

    def get(G, case):
        if case not in cache:
            g = gold("tess_comp_cases.npz")
            lon, lat, h, model, bounds, ndrop = _case(G, g, case)
            V = {name: g["%s_K_%s" % (case, name)] / _tensor_scale() for name in TENSOR}
            cache[case] = _compose(V, _Q(lon, lat, bounds))
        return cache[case]
    return get


@pytest.mark.parametrize("case", ["g", "n", "d"])
@pytest.mark.parametrize("comp", BCOMPS)
def test_entries_results_and_warnings_against_the_references_tensor(G, expected, comp, case):
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    lon, lat, h, model, bounds, ndrop = _case(G, g, case)
    K_exp = expected(G, case)[comp]
    m = bounds.shape[0]
    tol = NEAR_TENSOR if case == "n" else 1e-10
    rng = np.random.default_rng(17)
    pmag = rng.normal(size=3)
    fn = getattr(tesseroid, comp)
    (res, K), msgs = _warnings(fn, lon, lat, h, model, pmag=pmag)
    assert K.shape == K_exp.shape == (lon.size, 3 * m) and np.isfinite(K).all()
    err = relmax(K, K_exp)
    print("%s, case %s: max |dK| / max|K| = %.3e" % (comp, case, err))
    assert err <= tol, err
    if ndrop:                                               # trailing zero columns in each of the three blocks
        for a in range(3):
            assert not K[:, (a + 1) * m - ndrop:(a + 1) * m].any() and K[:, a * m:(a + 1) * m - ndrop].any()
    r_exp = K_exp @ np.repeat(pmag, m)
    assert relmax(res, r_exp) <= tol, relmax(res, r_exp)
    # the warnings of the tensor fields on the same case
    nwarn = int(g["%s_warn_gzz" % case])
    small = 1 if case == "d" else 0
    assert sum("Ignoring this tesseroid" in s for s in msgs) == small
    assert any("Stopped dividing" in s for s in msgs) == (nwarn - small > 0)
    # per-cell vectors (the kept cells first, as the columns)
    vec = rng.normal(size=(m, 3))
    if case == "g":
        cells_vec = vec
    else:
        cells = g[case + "_cells"]
        idx = [int(np.flatnonzero((cells == b).all(axis=1))[0]) for b in bounds]
        cells_vec = np.empty((m, 3))
        cells_vec[idx] = vec
    (res_v, K_v), _ = _warnings(fn, lon, lat, h, _with_vectors(G, model, cells_vec))
    assert np.array_equal(K_v, K)
    r_exp = K_exp @ np.ascontiguousarray(vec.T).ravel()
    assert relmax(res_v, r_exp) <= tol, relmax(res_v, r_exp)
    # without the kernel: the store-free pass, the same warnings
    (res2, K2), msgs2 = _warnings(fn, lon, lat, h, model, pmag=pmag, return_kernel=False)
    assert K2 is None and relmax(res2, res) <= 1e-12, relmax(res2, res)
    assert sorted(set(msgs2)) == sorted(set(msgs))
    # cells without the property are skipped; none left is an error
    with pytest.raises(ValueError):
        fn(lon, lat, h, model if case != "g" else G.mesher.TesseroidMesh(tuple(g["g_area"]), tuple(g["g_spacing"])))


# ----------------------------------------------------------------------------- 2. the point dipole

def test_signs_and_frames_against_the_point_dipole(G):
    from gravinv3dhmc_amd import constants
    from gravinv3dhmc_amd.gravmag import tesseroid
    R = constants.MEAN_EARTH_RADIUS
    w, e, s, n, top, bottom = 29.95, 30.05, 79.95, 80.05, 0.0, -10000.0
    cell = [G.mesher.Tesseroid(w, e, s, n, top, bottom)]
    # across the pole, on the cell's meridian, on its parallel, and two general azimuths
    lon = np.array([-150.0, 30.0, 120.0, 100.0, -40.0])
    lat = np.array([80.0, 55.0, 80.0, 50.0, 62.0])
    h = np.full(5, 400e3)
    r1, r2 = R + bottom, R + top
    volume = (r2 ** 3 - r1 ** 3) / 3.0 * (np.sin(n * D2R) - np.sin(s * D2R)) * ((e - w) * D2R)
    nc, ec, uc = (v[0] for v in _frames([30.0], [80.0]))
    src = (R + 0.5 * (top + bottom)) * uc
    no, eo, uo = _frames(lon, lat)
    obs = (R + h)[:, None] * uo
    d = obs - src
    dist = np.linalg.norm(d, axis=1)
    cosang = np.clip((uo @ uc), -1, 1)
    assert np.all(np.arccos(cosang) / D2R >= 10.0) and np.all(np.arccos(cosang) / D2R <= 40.0)
    rhat = d / dist[:, None]
    for a, axis in enumerate((nc, ec, -uc)):
        mu = 1.5 * volume * axis                              # 1.5 A/m along the cell's axis a
        B = constants.CM * constants.T2NT * (3.0 * (rhat @ mu)[:, None] * rhat - mu[None, :]) / dist[:, None] ** 3
        want = {"bx": np.sum(B * no, axis=1), "by": np.sum(B * eo, axis=1), "bz": -np.sum(B * uo, axis=1)}
        mag = np.zeros(3)
        mag[a] = 1.5
        Bn = np.linalg.norm(B, axis=1)
        for comp in BCOMPS:
            res, K = getattr(tesseroid, comp)(lon, lat, h, cell, pmag=mag)
            err = np.abs(res - want[comp]) / Bn
            print("axis %d, %s: |dB| / |B| = %s" % (a, comp, np.array2string(err, precision=2)))
            assert np.all(err <= 1e-3), (a, comp, err)
            assert relmax(K[:, a] * 1.5, res) <= 1e-12


# ----------------------------------------------------------------------------- 3. the total field

def _fdir(inc, dec, n):
    i, d = np.broadcast_to(np.asarray(inc, dtype=float), (n,)) * D2R, np.broadcast_to(np.asarray(dec, dtype=float), (n,)) * D2R
    return np.stack([np.cos(i) * np.cos(d), np.cos(i) * np.sin(d), np.sin(i)], axis=1)


@pytest.fixture(scope="module")
def g_fields(G):
    """bx, by, bz of the "g" geometry with one set of per-cell vectors: (vec, {comp: (result, K)})"""
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    mesh = G.mesher.TesseroidMesh(tuple(g["g_area"]), tuple(g["g_spacing"]))
    vec = np.random.default_rng(23).normal(size=(mesh.size, 3))
    mesh.addprop("magnetization", vec)
    return vec, mesh, {c: getattr(tesseroid, c)(g["g_lon"], g["g_lat"], g["g_h"], mesh) for c in BCOMPS}


def test_tf_is_the_projection_at_the_observation(G, g_fields):
    from gravinv3dhmc_amd.gravmag import tesseroid
    g = gold("tess_comp_cases.npz")
    lon, lat, h = g["g_lon"], g["g_lat"], g["g_h"]
    vec, mesh, B = g_fields
    n = lon.size
    rng = np.random.default_rng(29)
    for inc, dec in ((62.0, -11.0), (rng.uniform(-80, 80, n), rng.uniform(-180, 180, n))):
        f = _fdir(inc, dec, n)
        res, K = tesseroid.tf(lon, lat, h, mesh, inc, dec)
        want = sum(f[:, k] * B[c][0] for k, c in enumerate(BCOMPS))
        Kw = sum(f[:, k, None] * B[c][1] for k, c in enumerate(BCOMPS))
        assert np.abs(res - want).max() <= 1e-13 * np.abs(want).max()
        assert np.abs(K - Kw).max() <= 1e-13 * np.abs(Kw).max()
        res2, none = tesseroid.tf(lon, lat, h, mesh, inc, dec, return_kernel=False)
        assert none is None and relmax(res2, res) <= 1e-12
    with pytest.raises(ValueError):
        tesseroid.tf(lon, lat, h, mesh, np.zeros(n - 1), 0.0)


# ----------------------------------------------------------------------------- 4. the store as a vector-data store

SHAPE = (2, 4, 6)                                             # the "g" mesh: nr, nlat, nlon
BASE = {"tf": 4.0, "bx": -700.0, "by": 300.0, "bz": 55.0}     # clearly different block means (uT)


def _module(G, g_fields, data, weights=None, mangle=(90, 0), **kw):
    g = gold("tess_comp_cases.npz")
    vec, mesh, B = g_fields
    n = g["g_lon"].size
    f = _fdir(mangle[0], mangle[1], n)
    d = {c: B[c][0] + BASE[c] for c in BCOMPS}
    d["tf"] = sum(f[:, k] * B[c][0] for k, c in enumerate(BCOMPS)) + BASE["tf"]
    dobs = [d[c] for c in data]
    mv = G.TesseroidMagVectorModule(dobs, tuple(g["g_area"]), tuple(g["g_spacing"]), (g["g_lon"], g["g_lat"], g["g_h"]),
                                    data=data, weights=weights, mangle=mangle, verbose=False, **kw)
    return mv, dobs, f


def test_module_kernel_blocks_and_the_tf_projection(G, g_fields):
    vec, mesh, B = g_fields
    n, m = 12, 48
    inc, dec = np.linspace(-70, 70, n), np.linspace(-170, 170, n)
    mv, dobs, f = _module(G, g_fields, ("tf", "bx", "by", "bz"), mangle=(inc, dec))
    assert mv.Aw.shape == (4 * n, 3 * m) and mv.mshape == SHAPE and mv.components == ("tf", "bx", "by", "bz")
    info = mv._engine.multi_info()
    assert info["components"] == [0, 1, 2, 3]
    for a in range(3):
        blocks = {c: mv.kernel(a, c) for c in ("tf",) + BCOMPS}
        for c in BCOMPS:
            assert relmax(blocks[c], B[c][1][:, a * m:(a + 1) * m]) <= 1e-12
        want = sum(f[:, k, None] * blocks[c] for k, c in enumerate(BCOMPS))
        assert np.abs(blocks["tf"] - want).max() <= 1e-13 * np.abs(want).max()
    # one tf block alone: the same rows; the store keeps its block table
    one, dobs1, _ = _module(G, g_fields, ("tf",), mangle=(inc, dec))
    assert one._vector and one.Aw.shape == (n, 3 * m) and one._engine.multi_info()["components"] == [0]
    for a in range(3):
        assert np.abs(one.kernel(a, "tf") - mv.kernel(a, "tf")).max() <= 1e-13 * np.abs(mv.kernel(a, "tf")).max()
    model = np.ascontiguousarray(vec.T).ravel()
    assert np.abs(one.forward(model) - (dobs1[0] - BASE["tf"])).max() <= 1e-12 * np.abs(dobs1[0]).max()
    mv._engine.close()
    one._engine.close()


@pytest.mark.parametrize("weights", [None, "std"])
def test_store_behaves_as_a_vector_data_store(G, g_fields, weights):
    n, m, M = 12, 48, 144
    mv, dobs, _ = _module(G, g_fields, BCOMPS, weights=weights)
    eng = mv._engine
    w = mv.weights
    if weights == "std":
        sd = np.array([np.std(d) for d in dobs])
        assert relmax(w, sd[0] / sd) <= 1e-14
    else:
        assert np.array_equal(w, np.ones(3))
    Aw = np.array(eng.download_G())
    wm = mv.Wm.diagonal()
    wb = np.repeat(w, n)
    assert Aw.shape == (3 * n, M)
    A = np.vstack([g_fields[2][c][1] for c in BCOMPS])
    assert relmax(wm, np.sqrt(((A * wb[:, None]) ** 2).sum(axis=0))) <= 1e-10
    assert relmax(Aw * wm[None, :], A * wb[:, None]) <= 1e-10
    dobsw = wb * np.concatenate(dobs)
    rng = np.random.default_rng(7)
    mwapr = 0.001 * wm
    lam, amp_beta = 0.4, 0.05
    for amp in (0.0, lam):
        if amp > 0:
            mv.set_amplitude(amp, amp_beta)
        for reg in ("Damping", "TV"):
            P = VecDataProblem(Aw, dobsw, 3, mwapr, reg, 0.7, 0.001, wm=wm, shape=SHAPE, lam=amp, amp_beta=amp_beta)
            x = rng.uniform(-0.02, 0.02, M) * wm
            a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            b = P.misfit_and_grad(x)
            assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-10, (reg, amp)
            assert relmax(a[2], b[2]) <= 1e-10 and abs(a[3] - b[3]) <= 1e-10 * abs(b[3])
            pm, om = mv.block_means()
            assert relmax(pm, P.pred_mean) <= 1e-10 and relmax(om, P.obs_mean) <= 1e-10
            # ONE mean over all rows is far outside the tolerance
            Pg = VecDataProblem(Aw, dobsw, 3, mwapr, reg, 0.7, 0.001, wm=wm, shape=SHAPE, lam=amp, amp_beta=amp_beta,
                                global_mean=True)
            assert abs(a[0] - Pg.misfit_and_grad(x)[0]) > 1e-3 * abs(a[0])
    # one trajectory of 5 steps on the chain (the amplitude term on; a step half the stability limit of its curvature)
    dt = min(0.02, 1.0 / np.sqrt(2.0 * lam / (amp_beta * wm.min() ** 2)))
    low, high = -0.02 * wm, 0.02 * wm
    P = VecDataProblem(Aw, dobsw, 3, mwapr, "TV", 1.0, 0.001, wm=wm, shape=SHAPE, lam=lam, amp_beta=amp_beta)
    eng.set_reg("TV", 1.0, 0.001, SHAPE, mwapr)
    p0 = rng.normal(size=M) * 0.3
    eng.chain_init(mwapr, low, high)
    acc, o = eng.chain_trajectory(p0, dt, 5, 0.0)
    xo, acco, oo = P.leapfrog(mwapr, p0, dt, 5, low, high, 0.0)
    assert acc == acco and relmax(o, oo) <= 1e-9 and relmax(eng.chain_get_x(), xo) <= 1e-9
    assert eng.chain_stats()["resident_launches"] == 0 and not eng.fold_info()["on"]
    eng.close()


def test_hmcsample_with_the_posterior_stream(G, g_fields, tmp_path, capsys):
    mv, dobs, _ = _module(G, g_fields, BCOMPS, amplitude=0.3, amplitude_beta=0.05)
    M = 144
    G.HMCSample(mv, 40, 2, 0.02, [3, 6], np.full(M, 0.001), np.full(M, 0.001),
                np.c_[np.full(M, -5.0), np.full(M, 5.0)], "mandatory", 1000, mv.dobs,
                "Fixed", 0.8, 1.0, "TV", 0.001, 100, 0.3, nbest=10, myrank=0, save_folder=str(tmp_path / "chain"),
                sample_sink="none", posterior_stream=True)
    capsys.readouterr()
    st = mv._engine.posterior_stream_read()
    assert st["n_per_chain"].tolist() == [40]
    assert st["mean"].shape == (M,) and st["std"].shape == (M,)
    assert np.isfinite(st["mean"]).all() and np.isfinite(st["std"]).all() and (st["std"] > 0).any()
    assert mv.to_vectors(st["mean"]).shape == (48, 3) and mv.amplitude(st["mean"]).shape == (48,)
    mv._engine.close()


# ----------------------------------------------------------------------------- 5. refusals and errors

def test_refusals_and_errors(G, g_fields):
    from gravinv3dhmc_amd import _lib
    g = gold("tess_comp_cases.npz")
    b = np.ascontiguousarray(g["g_bounds"])
    M = 144
    NAME = "tesseroid magnetization store"
    e = G.Engine(16386, M)                                   # 3 x 5462 stacked rows
    with pytest.raises(NotImplementedError, match=NAME):
        e.set_cells_tess_mag(b, 8, BCOMPS, (1.0, 1.0, 1.0))
    e.close()
    for comps, w, N in ((("bx", "bx"), (1.0, 1.0), 24), (("bx", "by"), (1.0, 0.0), 24), (("bx", "by"), (1.0, np.inf), 24),
                        (("bx", "by"), (1.0, 1.0), 25)):
        e = G.Engine(N, M)
        with pytest.raises(ValueError):
            e.set_cells_tess_mag(b, 8, comps, w)
        e.close()
    e = G.Engine(24, M)
    with pytest.raises(ValueError):
        e.set_cells_tess_mag(b, 8, ("tf", "bz"), (1.0, 1.0))                       # a tf block needs fdir
    ci = lambda *v: (_lib.C.c_int * len(v))(*v)
    assert e._lib.gh_set_cells_tess_mag(e._h, _lib.ptr(b), 8.0, 2, ci(0, 3), _lib.ptr(np.ones(2)), None) == _lib.GH_ERR_ARG
    assert e._lib.gh_set_cells_tess_mag(e._h, _lib.ptr(b), 8.0, 5, ci(0, 1, 2, 3, 1), _lib.ptr(np.ones(5)),
                                        None) == _lib.GH_ERR_ARG
    assert e._lib.gh_set_cells_tess_mag(e._h, _lib.ptr(b), 0.0, 2, ci(1, 2), _lib.ptr(np.ones(2)), None) == _lib.GH_ERR_ARG
    bad = b.copy()
    bad[3, 4], bad[3, 5] = bad[3, 5], bad[3, 4]                                    # top < bottom
    with pytest.raises(ValueError, match="invalid tesseroid dimensions"):
        e.set_cells_tess_mag(bad, 8, ("bx", "by"), (1.0, 1.0))
    e.close()
    e = G.Engine(24, M + 1)                                                        # M % 3
    assert e._lib.gh_set_cells_tess_mag(e._h, _lib.ptr(b), 8.0, 2, ci(1, 2), _lib.ptr(np.ones(2)), None) == _lib.GH_ERR_ARG
    e.close()
    e = G.Engine(24, M)
    e.set_obs(np.zeros(24), np.zeros(24), np.zeros(24))                            # not fresh
    with pytest.raises(ValueError, match="fresh"):
        e.set_cells_tess_mag(b, 8, ("bx", "by"), (1.0, 1.0))
    e.close()
    e = G.Engine(24, M)
    e.set_matrix_free(True)
    with pytest.raises(NotImplementedError, match=NAME):
        e.set_cells_tess_mag(b, 8, ("bx", "by"), (1.0, 1.0))
    e.close()
    e = G.Engine(24, M)
    e.set_shift_invariant(True)
    with pytest.raises(NotImplementedError, match=NAME):
        e.set_cells_tess_mag(b, 8, ("bx", "by"), (1.0, 1.0))
    e.close()

    mv, dobs, _ = _module(G, g_fields, BCOMPS)
    with pytest.raises(NotImplementedError, match=NAME):
        G.HMCSampleBatch(mv, 2, 2, 0, 0.02, [3, 8], np.zeros((2, M)), np.zeros(M), np.c_[-np.ones(M), np.ones(M)],
                         "mandatory", 1000, mv.dobs, "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)
    eng = mv._engine
    x = np.random.default_rng(3).normal(size=M)
    before = eng.forward(x)
    for call in (lambda: eng.set_matrix_free(True), lambda: eng.set_shift_invariant(True),
                 lambda: eng.compress_wavelet(3, SHAPE, 0.001, 2), lambda: eng.upload_G(np.zeros((36, M))),
                 lambda: eng.batch_init(np.zeros((2, M)), -np.ones(M), np.ones(M)),
                 lambda: eng._chk(eng._lib.gh_shard_init(eng._h, _lib.C.create_string_buffer(128), 0, 1, M, 0)),
                 lambda: eng._chk(eng._lib.gh_shard_init_rows(eng._h, _lib.C.create_string_buffer(128), 0, 1, 36, 0)),
                 lambda: eng.b_result("bx", np.zeros((48, 3)))):
        with pytest.raises(NotImplementedError, match=NAME):
            call()
    with pytest.raises(NotImplementedError, match="vector-data magnetization"):
        eng.set_cells(np.tile(b, (3, 1)), _lib.CELL_TESSEROID)
    with pytest.raises(ValueError):
        eng.tess_b_result("tf", np.zeros((48, 3)))                                 # no fdir on this context
    with pytest.raises(ValueError):
        eng.tess_b_result("bx", np.zeros((47, 3)))
    # the context still evaluates the same forward product
    assert np.array_equal(eng.forward(x), before)
    vec = g_fields[0]
    assert relmax(eng.tess_b_result("by", vec), g_fields[2]["by"][0]) <= 1e-12
    eng.close()
    # the prism modules keep refusing the spherical case
    d = [np.zeros(12)] * 3
    obs = (g["g_lon"], g["g_lat"], g["g_h"])
    with pytest.raises(NotImplementedError):
        G.MagVectorModule(d, tuple(g["g_area"]), tuple(g["g_spacing"]), obs, data=BCOMPS, coordinate="spherical",
                          verbose=False)
    with pytest.raises(NotImplementedError):
        G.GravMagModule(d[0], tuple(g["g_area"]), tuple(g["g_spacing"]), obs, field="magnetic", coordinate="spherical",
                        verbose=False)


# ----------------------------------------------------------------------------- 6. a second shape at the kernel's edges

def test_second_shape_against_the_single_field_kernels(G):
    """17 observations x 5 cells: ld = 32 for one block of 17 rows, the padding rows zeroed by the threads behind each
    column's points; 85 pairs in two workgroups, the second one ragged."""
    from gravinv3dhmc_amd.gravmag import tesseroid
    rng = np.random.default_rng(41)
    cells = np.array([[10.0, 12.0, 40.0, 41.5, 0.0, -30e3], [12.0, 13.0, 40.0, 41.5, -5e3, -40e3],
                      [-3.0, 1.0, -12.0, -9.0, 1e3, -60e3], [170.0, 178.0, 60.0, 66.0, 0.0, -100e3],
                      [11.0, 11.5, 41.0, 41.25, 0.0, -2e3]])
    lon = np.r_[rng.uniform(8, 15, 9), rng.uniform(-180, 180, 8)]
    lat = np.r_[rng.uniform(38, 44, 9), rng.uniform(-80, 80, 8)]
    h = np.r_[rng.uniform(20e3, 60e3, 9), rng.uniform(200e3, 450e3, 8)]
    dens = [G.mesher.Tesseroid(*c, props={"density": 1.0}) for c in cells]
    V = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name in TENSOR:
            V[name] = getattr(tesseroid, name)(lon, lat, h, dens)[1] / _tensor_scale()
        want = _compose(V, _Q(lon, lat, cells))
        mag = [G.mesher.Tesseroid(*c) for c in cells]
        for comp in BCOMPS:
            res, K = getattr(tesseroid, comp)(lon, lat, h, mag, pmag=[0.3, -1.0, 2.0])
            assert K.shape == (17, 15)
            err = np.abs(K - want[comp]).max() / np.abs(want[comp]).max()
            print("%s, 17 x 5: max |dK| / max|K| = %.3e" % (comp, err))
            assert err <= 1e-12, (comp, err)
