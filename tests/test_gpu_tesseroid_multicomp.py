"""GPU suite of the tesseroid multi-component inversion (TesseroidMultiComponentModule, GH_CELL_TESSEROID_MULTI): the
dense store's row blocks against the single-component engines, the module against the NumPy restatement of the
multi-component model (tests/multicomp_host.py) built from those blocks, the shift-invariant table (the component block
as one more coordinate of the class, the signed north-south mirror, the means per block) against the dense store, the
sign table against direct evaluation, gz on the streamed form unchanged, the refusals and HMCSample end to end.

Geometry: 12 longitudes (30 degrees) around the full circle x 4 latitude rows (-60 ... 60) x 2 layers = 8 cell rows, 96
cells; observations on the cells' longitude spacing x latitudes (-45, -15, 15, 45) at 250 km = 48 points; gzz (even under
both reflections, the tensor's scale), gxz (odd under the north-south mirror), gy (odd in the longitude difference, the
Gs scale) and gz (ratio 1.6) = 192 stacked rows: a mirrored pair, both signs, more than one block.

Tolerances: blocks against the single-component engines bit for bit; against the restatement 1e-10 (that of
tests/test_gpu_multicomp.py for the same quantities); the table against the dense store the store's stated 1e-10,
relative to each block's largest magnitude; chains as tests/test_gpu_mfbatch.py compares its gz table with the stored
kernel (the same decisions, energies and final x to 1e-9)."""
import os

import numpy as np
import pytest

from helpers import relmax
from multicomp_host import MultiProblem, std_weights

pytestmark = pytest.mark.gpu

COMPS = ("gzz", "gxz", "gy", "gz")
RATIOS = (8.0, 8.0, 1.6, 1.6)
ALL = ("potential", "geoid", "gx", "gy", "gz", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
MRANGE, MSPACING = (-180, 180, -60, 60, 0, -200000), (-100000, 30, 30)
SHAPE = (2, 4, 12)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _obs(shift=0.0, inclusive=False):
    lons = np.arange(-180, 181 if inclusive else 180, 30.0)
    lon, lat = [a.ravel() for a in np.meshgrid(lons, np.array([-45.0, -15.0, 15.0, 45.0]) + shift, indexing="ij")]
    return lon, lat, np.full(lon.size, 250000.0)


def _mesh(G):
    mesh = G.mesher.TesseroidMesh(MRANGE, MSPACING)
    assert mesh.shape == SHAPE
    return mesh


@pytest.fixture(scope="module")
def blocks(G):
    """The single-component kernels of the geometry (engines pinned to the reference's goldens elsewhere): computed
    once, read only."""
    from gravinv3dhmc_amd import _lib
    obs = _obs()
    bounds = _mesh(G).cell_bounds()
    out = {}
    for c, r in zip(COMPS, RATIOS):
        e = G.Engine(obs[0].size, bounds.shape[0])
        e.set_obs(*obs)
        e.set_cells(bounds, _lib.CELL_TESSEROID, r, component=c)
        e.build_G()
        out[c] = np.array(e.download_G())
        out[c].setflags(write=False)
        e.close()
    return out


def _rho():
    rho = np.zeros(SHAPE)
    rho[:, 1:3, 2:7] = 0.4
    rho[1, 0, 8:11] = -0.2
    return rho.ravel()


@pytest.fixture(scope="module")
def dobs(blocks):
    rng = np.random.default_rng(3)
    out = []
    for c in COMPS:
        d = blocks[c] @ _rho()
        out.append(d + 0.02 * np.abs(d).max() * rng.normal(size=d.size))
    return out


def _module(G, obs, dobs, comps=COMPS, **kw):
    return G.TesseroidMultiComponentModule(dobs, MRANGE, MSPACING, obs, components=comps, verbose=False, **kw)


def _blockmax(v, ref, nblk):
    """largest deviation of v from ref per block, relative to the block's largest magnitude"""
    v, ref = np.asarray(v).reshape(nblk, -1), np.asarray(ref).reshape(nblk, -1)
    return max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(v, ref))


# ----------------------------------------------------------------------------- 1. the dense store

def test_dense_blocks_are_the_single_component_kernels(G, blocks):
    from gravinv3dhmc_amd import _lib
    obs = _obs()
    n = obs[0].size
    bounds = _mesh(G).cell_bounds()
    e = G.Engine(len(COMPS) * n, bounds.shape[0])
    e.set_cells_tess_multi(bounds, COMPS, RATIOS, np.ones(len(COMPS)))
    e.set_obs(*obs)
    e.build_G()
    S = np.array(e.download_G())
    assert S.shape == (len(COMPS) * n, bounds.shape[0])
    for b, c in enumerate(COMPS):
        assert np.array_equal(S[b * n:(b + 1) * n], blocks[c]), c
    info = e.multi_info()
    assert info["components"] == [_lib.COMPONENTS[c] for c in COMPS] and np.array_equal(info["weights"], np.ones(4))
    st = e.kernel_stats()
    assert st["warn_cells"] == 0 and st["leaves"] >= len(COMPS) * n * bounds.shape[0]
    e.close()


@pytest.mark.parametrize("weights", ["std", (2.0, 0.013, 700.0, 0.07)])
def test_dense_module_against_the_restatement(G, blocks, dobs, weights):
    obs = _obs()
    n = obs[0].size
    mc = _module(G, obs, dobs, weights=weights)
    assert np.array_equal(mc.ratios, RATIOS)                      # (ratio=None: the reference's per field)
    w = std_weights(dobs) if isinstance(weights, str) else np.asarray(weights, dtype=float)
    assert relmax(mc.weights, w) <= 1e-10 and mc.weights[0] == w[0]
    wb = np.repeat(w, n)
    assert relmax(mc.Wb.diagonal(), wb) <= 1e-10
    eng = mc._engine
    Aw = np.array(eng.download_G())
    wm = mc.Wm.diagonal()
    WA = np.vstack([blocks[c] for c in COMPS]) * wb[:, None]
    assert relmax(wm, np.sqrt((WA ** 2).sum(axis=0))) <= 1e-10
    assert relmax(Aw * wm[None, :], WA) <= 1e-10
    dobsw = wb * np.concatenate(dobs)
    assert relmax(mc.dobsw, dobsw) <= 1e-10
    rho = _rho()
    fwd = mc.forward(rho)
    for b, c in enumerate(COMPS):
        assert relmax(fwd[b * n:(b + 1) * n], blocks[c] @ rho) <= 1e-10, c
        assert relmax(mc.kernel(c), blocks[c]) <= 1e-10, c
    rng = np.random.default_rng(7)
    M = wm.size
    mwapr = 0.001 * wm
    worst = 0.0
    for reg in ("Damping", "TV"):
        P = MultiProblem(Aw, dobsw, len(COMPS), mwapr, reg, 0.7, 0.001, wm=wm, shape=SHAPE)
        for _ in range(2):
            x = rng.uniform(0, 0.5, M) * wm
            a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            b = P.misfit_and_grad(x)
            pm, om = mc.block_means()
            errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
                    abs(a[4] - b[4]) / max(abs(b[4]), 1e-300), relmax(pm, P.pred_mean), relmax(om, P.obs_mean)]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-10, (reg, errs)
    print("dense tesseroid multi-component store, weights %r: worst against the restatement %.3e" % (weights, worst))
    assert eng.chain_stats()["resident_launches"] == 0 and not eng.fold_info()["on"]
    eng.close()


# ----------------------------------------------------------------------------- 2. the table against the dense store

CASES = {"mirror": dict(), "no_mirror_switch": dict(env={"GRAVHMC_LW_MIRROR": "0"}), "shifted_5deg": dict(shift=5.0),
         "lon_inclusive": dict(inclusive=True)}


def _pair(G, monkeypatch, case, comps=COMPS, ratios=RATIOS, seed=11):
    """(dense module, table module, observations' count) on the case's geometry, with synthetic data"""
    from gravinv3dhmc_amd import _lib
    cfg = CASES[case]
    for k, v in cfg.get("env", {}).items():
        monkeypatch.setenv(k, v)
    obs = _obs(cfg.get("shift", 0.0), cfg.get("inclusive", False))
    n = obs[0].size
    bounds = _mesh(G).cell_bounds()
    rng = np.random.default_rng(seed)
    data = []
    for c, r in zip(comps, ratios):
        e = G.Engine(n, bounds.shape[0])
        e.set_obs(*obs)
        e.set_cells(bounds, _lib.CELL_TESSEROID, r, component=c)
        e.build_G()
        d = e.forward(_rho())
        e.close()
        data.append(d + 0.02 * np.abs(d).max() * rng.normal(size=n))
    w = (1.0, 0.7, 900.0, 0.05)[:len(comps)]
    dense = _module(G, obs, data, comps=comps, weights=w)
    table = _module(G, obs, data, comps=comps, weights=w, shift_invariant=True)
    return dense, table, n


@pytest.mark.parametrize("case", list(CASES))
def test_table_against_the_dense_store(G, monkeypatch, case):
    dense, table, n = _pair(G, monkeypatch, case)
    nb = len(COMPS)
    et, ed = table._engine, dense._engine
    assert et.shift_invariant_harmonic()["form"] == "streamed"
    info = et.shift_invariant_info()
    assert info["n_lon"] == 12 and info["n_rows"] == 8 and info["n_classes"] == 4 * nb
    per_row = info["n_classes"] * ((12 // 2 + 1 + 7) // 8 * 8) * 16
    rows = 4 if case in ("mirror", "lon_inclusive") else 8        # (the mirror halves the table; shifted: no mirror exists)
    assert et.shift_invariant_harmonic()["table_bytes"] == per_row * rows, case
    tol = 1e-10
    wd, wt = dense.Wm.diagonal(), table.Wm.diagonal()
    e_w = relmax(wt, wd)
    rho = _rho()
    e_fwd = _blockmax(table.forward(rho), dense.forward(rho), nb)
    M = wd.size
    rng = np.random.default_rng(5)
    mwapr = 0.001 * wd
    worst = 0.0
    for reg in ("Damping", "TV"):
        x = rng.uniform(0, 0.5, M) * wd
        a = table.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        (pa, oa), (pb, ob) = table.block_means(), dense.block_means()
        errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), _blockmax(a[2], b[2], nb), abs(a[3] - b[3]) / abs(b[3]),
                abs(a[4] - b[4]) / max(abs(b[4]), 1e-300), relmax(oa, ob),
                (np.abs(pa - pb) / np.abs(np.asarray(b[2]).reshape(nb, -1)).max(axis=1)).max()]
        worst = max(worst, max(errs))
    print("tesseroid multi-component table [%s]: %r; vs dense: Wm %.2e forward %.2e potential/gradient/means %.2e"
          % (case, info, e_w, e_fwd, worst))
    assert e_w < tol and e_fwd < tol and worst < tol
    with pytest.raises(NotImplementedError, match="tesseroid multi-component store"):
        table.kernel("gzz")
    # a chain of 6 short trajectories from fixed momenta: the same decisions, energies and final x
    trajs = [(int(rng.integers(2, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(6)]
    outs = {}
    for tag, e in (("table", et), ("dense", ed)):
        e.set_reg("TV", 1.0, 0.001, SHAPE, mwapr)
        e.chain_init(mwapr, 0.0 * wd, 0.5 * wd)
        res = []
        e.run_chain(iter(trajs), 0.02, lambda L, acc, o, xx, res=res: res.append((acc, o.copy())))
        outs[tag] = (res, e.chain_get_x())
    assert len(outs["table"][0]) == len(outs["dense"][0]) == 6
    for (a1, o1), (a2, o2) in zip(outs["table"][0], outs["dense"][0]):
        assert a1 == a2 and relmax(o1, o2) < 1e-9
    assert relmax(outs["table"][1], outs["dense"][1]) < 1e-9
    et.close()
    ed.close()


# ----------------------------------------------------------------------------- 3. the signs

def test_sign_table_against_direct_evaluation(G):
    """Every field of one cell seen from (lon, lat, h) against the mirror image cell seen from (lon, -lat, h): -1 for
    gx, gxy, gxz (the local north axis flips), +1 for the others."""
    lon, lat, h = np.array([37.0]), np.array([33.0]), np.array([250000.0])
    north = G.mesher.TesseroidMesh((10, 40, 20, 50, 0, -100000), (-100000, 30, 30))
    south = G.mesher.TesseroidMesh((10, 40, -50, -20, 0, -100000), (-100000, 30, 30))
    for m in (north, south):
        assert m.size == 1
        m.addprop("density", np.ones(1))
    for c in ALL:
        a = getattr(G.tesseroid, c)(lon, lat, h, north)[0][0]
        b = getattr(G.tesseroid, c)(lon, -lat, h, south)[0][0]
        s = -1.0 if c in ("gx", "gxy", "gxz") else 1.0
        assert abs(a) > 0 and abs(b - s * a) <= 1e-10 * abs(a), (c, a, b)


def test_the_mirror_s_sign_is_sharp(G, monkeypatch, blocks):
    """gxz on the mirrored table against the table without the mirror; flipping the sign would move it by far more
    than the tolerance (asserted on the host first, so the case cannot pass by smallness)."""
    n = 48
    K = blocks["gxz"]
    rho = _rho()
    # the mirrored cell rows' share of gxz's prediction: what a wrong sign would flip.  Cell rows (layer, latitude
    # band): bands 0, 1 are the mirror images of 3, 2 -- the table keeps the rows of bands 0 and 1.
    band = np.arange(K.shape[1]) // 12 % 4
    flipped = K[:, band >= 2] @ rho[band >= 2]
    full = K @ rho
    assert np.abs(2 * flipped).max() > 1e-3 * np.abs(full).max()
    dense, table, n2 = _pair(G, monkeypatch, "mirror")
    dense._engine.close()
    monkeypatch.setenv("GRAVHMC_LW_MIRROR", "0")
    _d, plain, _ = _pair(G, monkeypatch, "mirror")
    _d._engine.close()
    assert n2 == n
    assert table._engine.shift_invariant_harmonic()["table_bytes"] * 2 == plain._engine.shift_invariant_harmonic()["table_bytes"]
    a, b = table.forward(rho)[n:2 * n], plain.forward(rho)[n:2 * n]
    err = np.abs(a - b).max() / np.abs(b).max()
    print("gxz block, mirrored table against the plain one: %.2e" % err)
    assert err < 1e-10
    assert relmax(b, full) < 1e-10
    table._engine.close()
    plain._engine.close()


# ----------------------------------------------------------------------------- 4. gz on the streamed form: unchanged

def test_gz_on_the_streamed_form_is_unchanged(G, monkeypatch):
    """GravMagModule(coordinate='spherical', shift_invariant=True) on this geometry, streamed form forced: forward and
    gradient bit for bit what the library gave before the signed mirror existed (tests/golden/tess_multicomp_gz.npz)."""
    monkeypatch.setenv("GRAVHMC_LONSYM_WIDE", "2")
    gold = np.load(os.path.join(HERE, "golden", "tess_multicomp_gz.npz"))
    obs = _obs()
    gm = G.GravMagModule(gold["dobs"], MRANGE, MSPACING, obs, coordinate="spherical", verbose=False, shift_invariant=True)
    assert gm._engine.shift_invariant_harmonic()["form"] == "streamed"
    wm = gm.Wm.diagonal()
    assert np.array_equal(wm, gold["wm"])
    fwd = gm._engine.forward(gold["x"])
    out = gm.misfit_and_grad(gold["x"], 0.001 * wm, None, None, "mandatory", 1000, 0.7, regulization="Damping", beta=0.001)
    assert np.array_equal(fwd, gold["forward"])
    assert np.array_equal(out[1], gold["grad"]) and out[0] == float(gold["misfit"])
    gm._engine.close()


# ----------------------------------------------------------------------------- 5. one component

def test_gz_alone_is_the_spherical_gravmag_module(G, dobs):
    obs = _obs()
    mc = _module(G, obs, [dobs[3]], comps=("gz",), weights=(1.0,))
    gm = G.GravMagModule(dobs[3], MRANGE, MSPACING, obs, coordinate="spherical", verbose=False)
    wm = gm.Wm.diagonal()
    assert np.array_equal(mc.ratios, [1.6]) and np.array_equal(mc.Wm.diagonal(), wm)
    assert np.array_equal(np.asarray(mc.Aw), np.asarray(gm.Aw))
    rng = np.random.default_rng(5)
    for reg in ("Damping", "TV"):
        x = rng.uniform(0, 0.5, wm.size) * wm
        a = mc.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = gm.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]
    mc._engine.close()
    gm._engine.close()


# ----------------------------------------------------------------------------- 6. refusals

def test_refusals(G, dobs):
    from gravinv3dhmc_amd import _lib
    obs = _obs()
    STORE = "tesseroid multi-component store"
    for kw in ({"wavelet": "3D"}, {"matrix_free": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match=STORE):
            _module(G, obs, dobs, **kw)
    # the table on a geometry without the structure: refused with the store's reason
    lon = obs[0].copy()
    lon[5] += 1.234
    with pytest.raises(NotImplementedError, match="shift-invariant store: the observation longitudes"):
        _module(G, (lon, obs[1], obs[2]), dobs, shift_invariant=True)
    for si in (False, True):
        mc = _module(G, obs, dobs, shift_invariant=si)
        eng = mc._engine
        wm = mc.Wm.diagonal()
        M = wm.size
        with pytest.raises(NotImplementedError, match=STORE):
            G.HMCSampleBatch(mc, 2, 4, 0, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001),
                             np.c_[np.full(M, 0.0), np.full(M, 0.5)], "mandatory", 1000, mc.dobs,
                             "Fixed", 0.8, 1.0, "MS", 0.001, 100, 0.3, save_folder="unused_chain")
        with pytest.raises(NotImplementedError, match=STORE):
            eng.batch_init(np.stack([0.001 * wm, 0.002 * wm]), 0.0 * wm, 0.5 * wm)
        with pytest.raises(NotImplementedError, match=STORE):
            eng.compress_wavelet(3, SHAPE, 0.001, 2)
        with pytest.raises(NotImplementedError, match=STORE):
            eng.upload_G(np.zeros((eng.N, eng.M)))
        with pytest.raises(NotImplementedError, match=STORE):
            eng.set_matrix_free(True)
        with pytest.raises(ValueError, match=STORE):
            eng.set_data(mc.dobsw, np.zeros(eng.N))                    # grav_fix
        assert not eng.fold_info()["on"] and eng.chain_stats()["resident_launches"] == 0
        eng.close()
    # the library's own checks
    cell = np.array([[0, 30, 0, 30, 0, -1000.0]])
    e = G.Engine(4, 1)
    with pytest.raises(ValueError):
        e.set_cells_tess_multi(cell, ("gz", "gz"), (1.6, 1.6), (1.0, 1.0))
    with pytest.raises(ValueError):
        e.set_cells_tess_multi(cell, ("gz", "gzz"), (1.6, 8.0), (1.0, 0.0))
    with pytest.raises(ValueError, match="ratio"):
        e.set_cells_tess_multi(cell, ("gz", "gzz"), (1.6, 0.0), (1.0, 1.0))
    with pytest.raises(ValueError, match="dimensions"):
        e.set_cells_tess_multi(np.array([[30, 0, 0, 30, 0, -1000.0]]), ("gz", "gzz"), (1.6, 8.0), (1.0, 1.0))
    with pytest.raises(ValueError):
        e.set_cells_tess_multi(cell, ("gz", "gzz", "gxx"), (1.6, 8.0, 8.0), (1.0, 1.0, 1.0))     # 4 rows, 3 blocks
    e.set_cells_tess_multi(cell, ("gz", "gzz"), (1.6, 8.0), (1.0, 1.0))
    with pytest.raises(NotImplementedError, match="gh_set_cells_tess_multi"):
        e.set_cells(cell, _lib.CELL_TESSEROID)
    e.close()
    e = G.Engine(4, 1)
    e.set_obs(np.zeros(4), np.zeros(4), np.full(4, 1000.0))
    with pytest.raises(ValueError, match="fresh context"):
        e.set_cells_tess_multi(cell, ("gz", "gzz"), (1.6, 8.0), (1.0, 1.0))
    e.close()
    # more than 16384 stacked rows on the dense form
    e = G.Engine(16386, 1)
    e.set_cells_tess_multi(cell, ("gz", "gzz"), (1.6, 8.0), (1.0, 1.0))
    e.set_obs(np.zeros(8193), np.zeros(8193), np.full(8193, 1000.0))
    with pytest.raises(NotImplementedError, match="16384"):
        e.build_G()
    e.close()


def test_the_pinned_old_refusals_still_fire(G, dobs):
    from gravinv3dhmc_amd import _lib
    obs = _obs()
    with pytest.raises(NotImplementedError, match="gz only"):
        G.GravMagModule(dobs[0], MRANGE, MSPACING, obs, coordinate="spherical", component="gzz", verbose=False)
    with pytest.raises(NotImplementedError, match="multi-component store"):
        G.MultiComponentModule(dobs, MRANGE, MSPACING, obs, components=COMPS, coordinate="spherical", verbose=False)
    bounds = _mesh(G).cell_bounds()
    e = G.Engine(obs[0].size, bounds.shape[0])
    e.set_shift_invariant(True)
    e.set_obs(*obs)
    e.set_cells(bounds, _lib.CELL_TESSEROID, 8.0, component="gzz")
    with pytest.raises(NotImplementedError, match="component"):
        e.build_G()
    e.close()


# ----------------------------------------------------------------------------- 7. HMCSample on the table

def test_hmcsample_end_to_end_on_the_table(G, tmp_path, capsys, dobs):
    obs = _obs()
    mc = _module(G, obs, dobs, shift_invariant=True)
    M = mc.Wm.diagonal().size
    folder = str(tmp_path / "chain")
    lo, hi = -0.3, 0.5
    G.HMCSample(mc, 6, 2, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, lo), np.full(M, hi)],
                "mandatory", 1000, mc.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 100, 0.3, nbest=100, myrank=0,
                save_folder=folder, sample_sink="binary")
    capsys.readouterr()
    model = np.fromfile(folder + "0/model.bin").reshape(-1, M)
    assert model.shape[0] >= 1 and np.isfinite(model).all()
    assert (model >= lo).all() and (model <= hi).all()
    fwd = mc.forward(model[-1])
    assert fwd.shape == (len(COMPS) * obs[0].size,) and np.isfinite(fwd).all()
    mc._engine.close()
