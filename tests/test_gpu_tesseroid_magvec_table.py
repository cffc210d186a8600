"""GPU suite of the tesseroid magnetization store on the shift-invariant table (TesseroidMagVectorModule(...,
shift_invariant=True), gh_set_cells_tess_mag_table): the data block as one more coordinate of the observation class, the
axis block (N, E, D) as one of the table's cell row, the north-south mirror with a sign per class times a sign per row.
The dense store of the same module, pinned elsewhere to the reference's tensor fixtures, is the yardstick.

Geometry (that of tests/test_gpu_tesseroid_multicomp.py): 12 longitudes (30 degrees) around the full circle x 4 latitude
bands (-60 ... 60) x 2 layers = 96 cells, M = 288 unknowns, 24 table rows; observations on the cells' longitude spacing x
latitudes (-45, -15, 15, 45) at 250 km = 48 points, 144 stacked rows for three components, 4 nb classes.  "odd_bands":
three 30-degree bands (-45 ... 45) and observation latitudes (-30, 0, 30): 72 cells, 18 table rows of which the 6 middle
ones are their own mirror images (12 items), 3 nb classes of which the one at 0 degrees is its own.

Tolerances: the table against the dense store 1e-10 relative to each block's largest magnitude (the same entries, one DFT
round trip apart); chains: the same decisions, energies and final x to 1e-9 (tests/test_gpu_tesseroid_multicomp.py, for
the same reason).  The signs from direct evaluation: 1e-10 of the entry.  The table of more than 16384 rows against the
store-free pass: 1e-8 of the block's maximum, the bound of tests/test_gpu_tesseroid_magnetic.py for entries against an
independent evaluation."""
import os

import numpy as np
import pytest

from helpers import relmax

pytestmark = pytest.mark.gpu

BCOMPS = ("bx", "by", "bz")
WEIGHTS = {"bx": 1.0, "by": 0.7, "bz": 900.0, "tf": 0.05}
MRANGE, MSPACING, SHAPE = (-180, 180, -60, 60, 0, -200000), (-100000, 30, 30), (2, 4, 12)
MRANGE_ODD, SHAPE_ODD = (-180, 180, -45, 45, 0, -200000), (2, 3, 12)
LATS, LATS_ODD = (-45.0, -15.0, 15.0, 45.0), (-30.0, 0.0, 30.0)
NAME = "tesseroid magnetization store"
AMP, AMP_BETA = 0.5, 0.05


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _obs(shift=0.0, inclusive=False, lats=LATS):
    lons = np.arange(-180, 181 if inclusive else 180, 30.0)
    lon, lat = [a.ravel() for a in np.meshgrid(lons, np.asarray(lats) + shift, indexing="ij")]
    return lon, lat, np.full(lon.size, 250000.0)


def _model(shape):
    """a property-major model (A/m): every axis present in both hemispheres and both layers"""
    v = np.zeros((3,) + tuple(shape))
    v[0, :, 0, 2:7] = 0.8
    v[0, :, -1, 3:9] = -0.5
    v[0, 1, 1, 5:8] = 0.3
    v[1, :, 1:, 1:6] = 0.4
    v[1, 0, 0, 8:11] = -0.6
    v[2, :, :2, 4:10] = -0.7
    v[2, 1, -1, 0:3] = 0.9
    return v.ravel()


def _module(G, obs, dobs, data=BCOMPS, mrange=MRANGE, **kw):
    kw.setdefault("weights", tuple(WEIGHTS[c] for c in data))
    return G.TesseroidMagVectorModule(dobs, mrange, MSPACING, obs, data=data, verbose=False, **kw)


CASES = {"mirror": dict(rows=12), "no_mirror_switch": dict(env={"GRAVHMC_LW_MIRROR": "0"}, rows=24),
         "shifted_5deg": dict(shift=5.0, rows=24), "lon_inclusive": dict(inclusive=True, rows=12),
         "odd_bands": dict(odd=True, rows=12)}


def _pair(G, monkeypatch, case, data=BCOMPS, seed=11, **kw):
    """(dense module, table module, points, shape) on the case's geometry with synthetic data: the dense store's own
    forward of the block model plus noise"""
    cfg = CASES[case]
    for k, v in cfg.get("env", {}).items():
        monkeypatch.setenv(k, v)
    odd = cfg.get("odd", False)
    obs = _obs(cfg.get("shift", 0.0), cfg.get("inclusive", False), LATS_ODD if odd else LATS)
    mrange, shape = (MRANGE_ODD, SHAPE_ODD) if odd else (MRANGE, SHAPE)
    n = obs[0].size
    nb = len(data)
    probe = _module(G, obs, [np.zeros(n)] * nb, data=data, mrange=mrange, **kw)
    d = probe.forward(_model(shape)).reshape(nb, n)
    probe._engine.close()
    rng = np.random.default_rng(seed)
    dobs = [r + 0.02 * np.abs(r).max() * rng.normal(size=n) for r in d]
    dense = _module(G, obs, dobs, data=data, mrange=mrange, amplitude=AMP, amplitude_beta=AMP_BETA, **kw)
    table = _module(G, obs, dobs, data=data, mrange=mrange, amplitude=AMP, amplitude_beta=AMP_BETA,
                    shift_invariant=True, **kw)
    assert mrange is MRANGE_ODD or dense.mshape == SHAPE
    return dense, table, n, shape


def _blockmax(v, ref, nblk):
    """largest deviation of v from ref per block, relative to the block's largest magnitude"""
    v, ref = np.asarray(v).reshape(nblk, -1), np.asarray(ref).reshape(nblk, -1)
    return max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(v, ref))


def _against_dense(dense, table, nb, shape, tag):
    """Wm, forward, misfit_and_grad (Damping and TV, the amplitude term on) and the block means: the worst deviation"""
    wd, wt = dense.Wm.diagonal(), table.Wm.diagonal()
    e_w = relmax(wt, wd)
    model = _model(shape)
    e_fwd = _blockmax(table.forward(model), dense.forward(model), nb)
    M = wd.size
    rng = np.random.default_rng(5)
    mwapr = 0.001 * wd
    worst = 0.0
    for reg in ("Damping", "TV"):
        x = rng.uniform(-0.02, 0.02, M) * wd
        a = table.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        (pa, oa), (pb, ob) = table.block_means(), dense.block_means()
        assert dense.last_amplitude > 0
        errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), _blockmax(a[2], b[2], nb), abs(a[3] - b[3]) / abs(b[3]),
                abs(a[4] - b[4]) / max(abs(b[4]), 1e-300), relmax(oa, ob),
                (np.abs(pa - pb) / np.abs(np.asarray(b[2]).reshape(nb, -1)).max(axis=1)).max(),
                abs(table.last_amplitude - dense.last_amplitude) / dense.last_amplitude]
        print("  %s %s: value, gradient, prediction, data term, model term, obs means, pred means, Phi: %s"
              % (tag, reg, " ".join("%.2e" % e for e in errs)))
        worst = max(worst, max(errs))
    print("tesseroid magnetization table [%s]: vs dense: Wm %.2e forward %.2e potential/gradient/means %.2e"
          % (tag, e_w, e_fwd, worst))
    return e_w, e_fwd, worst


# ----------------------------------------------------------------------------- 1. the table against the dense store

@pytest.mark.parametrize("case", list(CASES))
def test_table_against_the_dense_store(G, monkeypatch, case):
    dense, table, n, shape = _pair(G, monkeypatch, case)
    nb = len(BCOMPS)
    et, ed = table._engine, dense._engine
    assert et.shift_invariant_harmonic()["form"] == "streamed"
    info = et.shift_invariant_info()
    nlat = shape[1]
    assert info["n_lon"] == 12 and info["n_rows"] == 3 * shape[0] * nlat and info["n_classes"] == nlat * nb
    if case != "odd_bands":
        assert info["n_rows"] == 24 and info["n_classes"] == 4 * nb
    # (7 frequencies padded to 8 complex entries of 16 bytes; one row per mirrored pair, or per cell row)
    assert et.shift_invariant_harmonic()["table_bytes"] == info["n_classes"] * 8 * 16 * CASES[case]["rows"], case
    tol = 1e-10
    e_w, e_fwd, worst = _against_dense(dense, table, nb, shape, case)
    assert e_w < tol and e_fwd < tol and worst < tol
    # a chain of 6 short trajectories from fixed momenta on both engines: the same decisions, energies and final x
    wd = dense.Wm.diagonal()
    M = wd.size
    rng = np.random.default_rng(9)
    mwapr = 0.001 * wd
    # (half the stability limit of the amplitude term's curvature, as tests/test_gpu_tesseroid_magnetic.py steps)
    dt = min(0.02, 1.0 / np.sqrt(2.0 * AMP / (AMP_BETA * wd.min() ** 2)))
    trajs = [(int(rng.integers(2, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(6)]
    outs = {}
    for tag, e in (("table", et), ("dense", ed)):
        e.set_reg("TV", 1.0, 0.001, shape, mwapr)
        e.chain_init(mwapr, -0.02 * wd, 0.02 * wd)
        res = []
        e.run_chain(iter(trajs), dt, lambda L, acc, o, xx, res=res: res.append((acc, o.copy())))
        outs[tag] = (res, e.chain_get_x(), e.amplitude_last())
    assert len(outs["table"][0]) == len(outs["dense"][0]) == 6
    for (a1, o1), (a2, o2) in zip(outs["table"][0], outs["dense"][0]):
        assert a1 == a2 and relmax(o1, o2) < 1e-9
    assert relmax(outs["table"][1], outs["dense"][1]) < 1e-9
    assert outs["dense"][2] > 0 and abs(outs["table"][2] - outs["dense"][2]) < 1e-9 * outs["dense"][2]
    assert et.chain_stats()["resident_launches"] == 0 and not et.fold_info()["on"]
    et.close()
    ed.close()


# ----------------------------------------------------------------------------- 2. the total field

def test_total_field_on_the_table(G, monkeypatch):
    data = ("tf", "bz")
    dense, table, n, shape = _pair(G, monkeypatch, "mirror", data=data, mangle=(60, 10))
    info = table._engine.shift_invariant_info()
    assert table._engine.shift_invariant_harmonic()["form"] == "streamed"
    assert info["n_rows"] == 24 and info["n_classes"] == 8
    # the unmirrored size although the geometry is symmetric: the total field is no pure sign under the mirror
    assert table._engine.shift_invariant_harmonic()["table_bytes"] == 8 * 8 * 16 * 24
    e_w, e_fwd, worst = _against_dense(dense, table, 2, shape, "tf, bz")
    assert e_w < 1e-10 and e_fwd < 1e-10 and worst < 1e-10
    dense._engine.close()
    table._engine.close()
    # one direction per circle of latitude: a class has one direction
    obs = _obs()
    inc = 40.0 + 0.5 * obs[1]
    dec = 5.0 - 0.1 * obs[1]
    dobs = [np.linspace(-1, 1, n), np.linspace(2, -1, n)]
    dense = _module(G, obs, dobs, data=data, mangle=(inc, dec))
    table = _module(G, obs, dobs, data=data, mangle=(inc, dec), shift_invariant=True)
    model = _model(SHAPE)
    assert relmax(table.Wm.diagonal(), dense.Wm.diagonal()) < 1e-10
    assert _blockmax(table.forward(model), dense.forward(model), 2) < 1e-10
    dense._engine.close()
    table._engine.close()
    # a direction that varies along a circle of latitude: no table
    with pytest.raises(NotImplementedError, match="varies within a class"):
        _module(G, obs, dobs, data=data, mangle=(inc + 0.01 * obs[0], dec), shift_invariant=True)
    # the library's own check (the module's runs on inc, dec before the library sees the directions)
    from gravinv3dhmc_amd.gravmag import tesseroid
    bounds = G.mesher.TesseroidMesh(MRANGE, MSPACING).cell_bounds()
    e = G.Engine(2 * n, 3 * bounds.shape[0])
    e.set_cells_tess_mag(bounds, 8.0, data, (1.0, 1.0), tesseroid._field_directions(inc + 0.01 * obs[0], dec, n),
                         shift_invariant=True)
    e.set_obs(*obs)
    with pytest.raises(NotImplementedError, match=NAME + ": the total field's direction varies within a class"):
        e.build_G()
    e.close()


# ----------------------------------------------------------------------------- 3. the signs, from direct evaluation

def test_mirror_signs_against_direct_evaluation(G):
    """One northern cell seen from (lon, lat, h) against its mirror image seen from (lon, -lat, h), unit magnetization
    along each axis in turn: every one of the nine entries is non-zero and obeys b = s_b s_a a."""
    from gravinv3dhmc_amd.gravmag import tesseroid
    from gravinv3dhmc_amd.inversion import magvector
    cls, axs = magvector.mirror_signs(BCOMPS)
    assert cls == (-1.0, 1.0, 1.0) and axs == (-1.0, 1.0, 1.0)
    lon, lat, h = np.array([37.0]), np.array([33.0]), np.array([250000.0])
    north = G.mesher.TesseroidMesh((10, 40, 20, 50, 0, -100000), (-100000, 30, 30))
    south = G.mesher.TesseroidMesh((10, 40, -50, -20, 0, -100000), (-100000, 30, 30))
    assert north.size == 1 and south.size == 1
    for b, comp in enumerate(BCOMPS):
        for ax in range(3):
            unit = np.zeros(3)
            unit[ax] = 1.0
            a = getattr(tesseroid, comp)(lon, lat, h, north, pmag=unit)[0][0]
            m = getattr(tesseroid, comp)(lon, -lat, h, south, pmag=unit)[0][0]
            assert abs(a) > 0 and abs(m - cls[b] * axs[ax] * a) <= 1e-10 * abs(a), (comp, ax, a, m)


# ----------------------------------------------------------------------------- 4. the row sign is sharp

def test_the_row_sign_is_sharp(G, monkeypatch):
    """The N-axis columns of the mirrored rows carry a share of the prediction far above the tolerance (asserted on the
    host from the dense kernel, so the case cannot pass by smallness); then the mirrored table, the table without the
    mirror and the dense store agree."""
    dense, table, n, shape = _pair(G, monkeypatch, "mirror")
    model = _model(shape)
    m = dense._cells
    full = dense.forward(model).reshape(3, n)
    # cell rows (layer, latitude band): bands 2, 3 are the mirror images of 1, 0 -- the table keeps the rows of bands 0, 1
    band = np.arange(m) // 12 % 4
    for b, comp in ((0, "bx"), (2, "bz")):
        KN = dense.kernel(0, comp)
        flipped = KN[:, band >= 2] @ model[:m][band >= 2]
        assert np.abs(2 * flipped).max() > 1e-3 * np.abs(full[b]).max(), comp
    want = dense.forward(model)
    dense._engine.close()
    monkeypatch.setenv("GRAVHMC_LW_MIRROR", "0")
    _d, plain, _, _ = _pair(G, monkeypatch, "mirror")
    _d._engine.close()
    assert table._engine.shift_invariant_harmonic()["table_bytes"] * 2 == plain._engine.shift_invariant_harmonic()["table_bytes"]
    a, p = table.forward(model), plain.forward(model)
    print("mirrored table against the plain one %.2e, against the dense store %.2e"
          % (_blockmax(a, p, 3), _blockmax(a, want, 3)))
    assert _blockmax(a, p, 3) < 1e-10 and _blockmax(a, want, 3) < 1e-10 and _blockmax(p, want, 3) < 1e-10
    table._engine.close()
    plain._engine.close()


# ----------------------------------------------------------------------------- 5. the existing instantiations

def test_existing_instantiations_are_unchanged(G, monkeypatch):
    """A smoke check that the new template parameter did not disturb the signed multi-component sweep and gz's (their
    own files remain the real check): the tables against their dense forms on this geometry."""
    obs = _obs()
    n = obs[0].size
    rng = np.random.default_rng(2)
    rho = np.zeros(SHAPE)
    rho[:, 1:3, 2:7] = 0.4
    rho[1, 0, 8:11] = -0.2
    rho = rho.ravel()
    dobs = [rng.normal(size=n), rng.normal(size=n)]
    kw = dict(components=("gzz", "gxz"), weights=(1.0, 0.7), verbose=False)
    pairs = [(G.TesseroidMultiComponentModule(dobs, MRANGE, MSPACING, obs, **kw),
              G.TesseroidMultiComponentModule(dobs, MRANGE, MSPACING, obs, shift_invariant=True, **kw), 2)]
    monkeypatch.setenv("GRAVHMC_LONSYM_WIDE", "2")
    pairs.append((G.GravMagModule(dobs[0], MRANGE, MSPACING, obs, coordinate="spherical", verbose=False),
                  G.GravMagModule(dobs[0], MRANGE, MSPACING, obs, coordinate="spherical", verbose=False,
                                  shift_invariant=True), 1))
    for dense, table, nb in pairs:
        assert table._engine.shift_invariant_harmonic()["form"] == "streamed"
        wd = dense.Wm.diagonal()
        assert relmax(table.Wm.diagonal(), wd) < 1e-10
        fa = table.forward(rho) if nb > 1 else table._engine.forward(rho * wd)
        fb = dense.forward(rho) if nb > 1 else dense._engine.forward(rho * wd)
        assert _blockmax(fa, fb, nb) < 1e-10
        x = rng.uniform(0, 0.5, wd.size) * wd
        a = table.misfit_and_grad(x, 0.001 * wd, None, None, "mandatory", 1000, 0.7, regulization="TV", beta=0.001)
        b = dense.misfit_and_grad(x, 0.001 * wd, None, None, "mandatory", 1000, 0.7, regulization="TV", beta=0.001)
        assert abs(a[0] - b[0]) < 1e-10 * abs(b[0]) and relmax(a[1], b[1]) < 1e-10 and _blockmax(a[2], b[2], nb) < 1e-10
        dense._engine.close()
        table._engine.close()


# ----------------------------------------------------------------------------- 6. refusals

def test_refusals_on_the_table(G):
    obs = _obs()
    n = obs[0].size
    dobs = [np.linspace(-1, 1, n)] * 3
    # a carved mesh: the cells no longer form full rows
    tlon, tlat = [a.ravel() for a in np.meshgrid(np.linspace(-180, 180, 25), np.linspace(-60, 60, 9), indexing="ij")]
    topo = np.where((tlon > 0) & (tlat > 0), -150000.0, 1000.0)
    with pytest.raises(NotImplementedError, match="shift-invariant store: the " + NAME + ": the cell"):
        _module(G, obs, dobs, shift_invariant=True, mtopo=(tlon, tlat, topo))
    lon = obs[0].copy()
    lon[5] += 1.234
    with pytest.raises(NotImplementedError, match=NAME + ": the observation longitudes"):
        _module(G, (lon, obs[1], obs[2]), dobs, shift_invariant=True)
    with pytest.raises(NotImplementedError, match=NAME):
        _module(G, obs, dobs, shift_invariant=True, wavelet="3D")
    with pytest.raises(NotImplementedError, match=NAME):
        _module(G, obs, dobs, shift_invariant=True, matrix_free=True)
    mv = _module(G, obs, dobs, shift_invariant=True)
    eng = mv._engine
    M = mv.Wm.diagonal().size
    with pytest.raises(NotImplementedError, match=NAME):
        G.HMCSampleBatch(mv, 2, 2, 0, 0.02, [3, 8], np.zeros((2, M)), np.zeros(M), np.c_[-np.ones(M), np.ones(M)],
                         "mandatory", 1000, mv.dobs, "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)
    with pytest.raises(NotImplementedError, match=NAME):
        mv.kernel(0, "bx")
    with pytest.raises(NotImplementedError, match=NAME):
        mv.A
    wm = mv.Wm.diagonal()
    for call in (lambda: eng.compress_wavelet(3, SHAPE, 0.001, 2), lambda: eng.set_matrix_free(True),
                 lambda: eng.batch_init(np.stack([0.001 * wm, 0.002 * wm]), -wm, wm),
                 lambda: eng.upload_G(np.zeros((eng.N, eng.M)))):
        with pytest.raises(NotImplementedError, match=NAME):
            call()
    x = np.random.default_rng(3).normal(size=M)
    assert np.isfinite(eng.forward(x)).all()                       # (the context still works)
    eng.close()
    # the prism forms have no table
    xp, yp = [a.ravel() for a in np.meshgrid(np.linspace(0, 2000, 5), np.linspace(0, 3000, 4))]
    with pytest.raises(NotImplementedError, match="shift-invariant"):
        G.MagVectorModule([np.zeros(xp.size)] * 3, (0, 2000, 0, 3000, 0, 1000), (500, 500, 500),
                          (xp, yp, np.zeros_like(xp)), data=BCOMPS, shift_invariant=True, verbose=False)
    with pytest.raises(NotImplementedError, match="shift-invariant"):
        G.MagVectorModule(np.zeros(xp.size), (0, 2000, 0, 3000, 0, 1000), (500, 500, 500),
                          (xp, yp, np.zeros_like(xp)), shift_invariant=True, verbose=False)
    from gravinv3dhmc_amd import mesher
    pb = mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (500, 500, 500)).cell_bounds()
    for set_cells in (lambda e: e.set_cells_mvi(pb, (0.0, 0.0, 1.0)),
                      lambda e: e.set_cells_mvi_data(pb, None, BCOMPS, np.ones(3))):
        e = G.Engine(3 * xp.size, 3 * pb.shape[0])
        set_cells(e)
        with pytest.raises(NotImplementedError, match="magnetization"):
            e.set_shift_invariant(True)
        e.close()


# ----------------------------------------------------------------------------- 7. HMCSample on the table

def test_hmcsample_end_to_end_on_the_table(G, monkeypatch, tmp_path, capsys):
    dense, table, n, shape = _pair(G, monkeypatch, "mirror")
    M = table.Wm.diagonal().size
    folder = str(tmp_path / "chain")
    G.HMCSample(table, 6, 2, 0.01, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, -5.0), np.full(M, 5.0)],
                "mandatory", 1000, table.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 100, 0.3, nbest=10, myrank=0,
                save_folder=folder, sample_sink="binary", posterior_stream=True)
    out = capsys.readouterr().out
    assert "chain 0:" in out and "accept ratio" in out
    assert os.path.exists(folder + "0/model.bin") and os.path.getsize(folder + "0/model.bin") > 0
    model = np.fromfile(folder + "0/model.bin").reshape(-1, M)
    assert model.shape[0] == 6 and np.isfinite(model).all() and np.abs(model).max() > 0
    st = table._engine.posterior_stream_read()
    assert st["n_per_chain"].tolist() == [6] and np.isfinite(st["mean"]).all()
    assert table.to_vectors(st["mean"]).shape == (M // 3, 3) and table.amplitude(st["mean"]).shape == (M // 3,)
    assert table.direction(model[0])[0].shape == (M // 3,)
    assert np.array_equal(table.from_vectors(table.to_vectors(model[0])), model[0])
    phi = table.Amplitude(model[0])
    assert phi[0] > 0 and abs(phi[0] - dense.Amplitude(model[0])[0]) <= 1e-12 * phi[0]
    err = _blockmax(table.forward(model[0]), dense.forward(model[0]), 3)
    print("first accepted model, table against dense forward: %.2e" % err)
    assert err < 1e-10
    table._engine.close()
    dense._engine.close()


# ----------------------------------------------------------------------------- 8. more than 16384 stacked rows

def test_more_than_16384_rows_build_on_the_table(G):
    """2-degree longitudes (n = 180) x 31 observation latitudes x 3 components = 16740 stacked rows on one layer of four
    latitude bands: the dense constructor refuses, the table builds (31 x 180 x 4 traversals) and its bx block agrees
    with the store-free pass of tesseroid.bx."""
    from gravinv3dhmc_amd.gravmag import tesseroid
    mrange, mspacing, shape = (-180, 180, -60, 60, 0, -100000), (-100000, 30, 2), (1, 4, 180)
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 180, 2.0), np.linspace(-75, 75, 31), indexing="ij")]
    obs = (lon, lat, np.full(lon.size, 250000.0))
    n = lon.size
    assert 3 * n == 16740
    dobs = [np.cos(np.deg2rad(lon)) * (b + 1.0) for b in range(3)]
    with pytest.raises(NotImplementedError, match="16384"):
        G.TesseroidMagVectorModule(dobs, mrange, mspacing, obs, data=BCOMPS, verbose=False)
    mv = G.TesseroidMagVectorModule(dobs, mrange, mspacing, obs, data=BCOMPS, verbose=False, shift_invariant=True)
    assert mv.mshape == shape
    info = mv._engine.shift_invariant_info()
    assert info["n_lon"] == 180 and info["n_rows"] == 12 and info["n_classes"] == 93
    wm = mv.Wm.diagonal()
    M = wm.size
    assert M == 3 * 720 and np.isfinite(wm).all() and (wm > 0).all()
    x = np.random.default_rng(1).uniform(-0.02, 0.02, M) * wm
    out = mv.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.7, regulization="TV", beta=0.001)
    assert np.isfinite(out[0]) and np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
    vec = np.zeros((3,) + shape)                      # a block model
    vec[0, 0, 1:3, 20:60] = 1.0
    vec[1, 0, 0, 100:140] = -0.5
    vec[2, 0, 3, 50:90] = 0.7
    model = vec.reshape(3, -1)
    fwd = mv.forward(model.ravel())[:n]
    mesh = G.mesher.TesseroidMesh(mrange, mspacing)
    mesh.addprop("magnetization", np.ascontiguousarray(model.T))
    ref = tesseroid.bx(obs[0], obs[1], obs[2], mesh, return_kernel=False)[0]
    err = np.abs(fwd - ref).max() / np.abs(ref).max()
    print("16740 stacked rows: bx of the table against the store-free pass %.2e" % err)
    assert err <= 1e-8
    mv._engine.close()
