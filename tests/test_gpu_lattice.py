"""GPU suite (`-m gpu`): the translation-invariant store of regular prism grids under gridded data
(csrc/lattice.hip.h, host_lattice.h).

The kernel's edges (lat_pass_kernel: a thread owns R = 8 consecutive outputs of the fast lattice axis and consumes 8
inputs per step; a workgroup's 64 lanes are TR output rows x nobt blocks of 8 outputs, at most 64 blocks = 512
outputs of one row; its four waves take four consecutive input rows; the forward sums chunks of layers).  The
adjoint's outputs are the ny cells of a row and its inputs the qy observations of a row, the forward's the other
way round, so (ny, qy) exercises both passes:
  * one below, at, one above the register block: ny, qy in 7, 8, 9;
  * one below, at, one above the tile of the fast axis: ny and qy together, then qy over ny = 2, in 511, 512, 513;
  * a table row crossing 64 lanes: ny = 40, qy = 33 with nx = 3, nz = 2;
  * a window narrower than one register block: qy = 3 under ny = 12, and ny = 2 under qy = 513;
  * output rows that do not fill the last tile of rows (nx = 7 with TR = 4), input rows that do not fill the last step
    of four (px = 5, nx = 7), one row only (nx = 1, px = 1);
  * more than one layer per forward chunk (5 layers, 130 x 513 observations: 66690 rows, beyond 16384).
Bounds: 1e-10 / 1e-11 / 1e-12 as in test_gpu_fold.py and test_gpu_magvecdata.py; the table itself bit for bit.
Every shape keeps observations over the whole length of its cell rows: the operator is the WEIGHTED kernel, and a
column of cells far from every observation (3 points over the middle of 511 cells: column norms 4e7 apart) multiplies
the last bit of the entry function -- the library's against the oracle's, whatever the store -- by that ratio, beyond
1e-10 (measured on the oracle alone with entries perturbed by one ulp of the largest: 2e-8 there, <= 1e-12 on the
shapes below)."""
import numpy as np
import pytest

from helpers import relmax
from lattice_cases import c2_linspace, detect, geometry

pytestmark = pytest.mark.gpu

H7 = 2000.0 / 7

#: name -> geometry(); the host suite's shapes ...
SHAPES = {
    "centres": dict(cells=(7, 5, 3), obs=(7, 5)),
    "beyond": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, H7), origin=(317.3, -911.7)),
    "inside": dict(cells=(7, 5, 3), obs=(3, 2), first=(2, 1), h=(H7, 150.0)),
    "corners": dict(cells=(7, 5, 3), obs=(8, 6), frac=(0.0, 0.0)),
    "near 1e6": dict(cells=(7, 5, 3), obs=(8, 6), h=(H7, H7), origin=(1.0e6 + 0.3, -1.0e6 - 0.7), frac=(0.0, 0.0)),
    "shuffled": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, 150.0), shuffle=5),
    "nx = 1": dict(cells=(1, 5, 3), obs=(4, 5)),
    "ny = 1": dict(cells=(7, 1, 3), obs=(7, 3), first=(0, -1)),
    "nz = 1": dict(cells=(7, 5, 1), obs=(7, 5)),
    "layers": dict(cells=(4, 3, 4), obs=(4, 3), tops=(0.0, 30.0, 170.0, 180.5, 1000.0)),
    # ... and one for each edge of the kernel
    "R-1": dict(cells=(3, 7, 2), obs=(5, 9), h=(H7, H7)),
    "R": dict(cells=(3, 8, 2), obs=(5, 8), h=(H7, H7)),
    "R+1": dict(cells=(3, 9, 2), obs=(5, 7), h=(H7, H7)),
    "tile-1 adjoint": dict(cells=(1, 511, 1), obs=(1, 511)),
    "tile adjoint": dict(cells=(1, 512, 1), obs=(1, 512)),
    "tile+1 adjoint": dict(cells=(2, 513, 1), obs=(1, 513)),
    "tile-1 forward": dict(cells=(2, 2, 1), obs=(1, 511), first=(0, -255)),
    "tile forward": dict(cells=(2, 2, 1), obs=(1, 512), first=(0, -255)),
    "tile+1 forward": dict(cells=(2, 2, 2), obs=(2, 513), first=(0, -255)),
    "row across 64 lanes": dict(cells=(3, 40, 2), obs=(4, 33), first=(0, 3), h=(H7, H7)),
    "covered row across 64 lanes": dict(cells=(3, 40, 2), obs=(4, 40), h=(H7, H7), tops=(0.0, 300.0, 700.0)),
    "narrow window": dict(cells=(2, 12, 2), obs=(3, 3), first=(0, 4)),
    "row tiles": dict(cells=(7, 100, 2), obs=(5, 100), first=(1, 0), frac=(0.0, 0.5)),
}
# (the rows of 511 ... 513 cells or points are on the 100 m grid: at 2000/7 m the prism formulas' own cancellation
# between a cell and a point 146 km away shows in gx as 2.5e-10 of the largest entry -- the entry function, not the store)
ON_100M = {"centres", "corners", "nx = 1", "ny = 1", "nz = 1", "layers", "tile-1 adjoint", "tile adjoint", "tile+1 adjoint",
           "tile-1 forward", "tile forward", "tile+1 forward", "narrow window", "row tiles"}

TF_DIR = (0.3, -0.5, 0.8124038404635961)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


_REF = {}


def reference(orc, name):
    """obs, bounds6 and the oracle's weighted gz kernel and weights of a shape: computed once, shared, left unchanged"""
    if name not in _REF:
        obs, b6 = geometry(**SHAPES[name])
        Aw, wm = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
        for a in (obs, b6, Aw, wm):
            a.setflags(write=False)
        _REF[name] = (obs, b6, Aw, wm)
    return _REF[name]


def engine(G, obs, b6, table, kind=0, **kw):
    eng = G.Engine(obs.shape[1], b6.shape[0])
    if table:
        eng.set_translation_invariant(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, kind, **kw)
    eng.build_G()
    return eng


def representative(obs, b6):
    """(observation, cell) of the pair with the smallest (p, q) of every offset: arrays of the table's shape"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    k, u, v = np.meshgrid(np.arange(nz), np.arange(nx + px - 1), np.arange(ny + qy - 1), indexing="ij")
    du, dv = u - (nx - 1), v - (ny - 1)
    p, q = np.maximum(du, 0), np.maximum(dv, 0)
    return ool[p * qy + q], col[(k * nx + (p - du)) * ny + (q - dv)]


KINDS = {"gz": (0, {}), "gzz": (3, {"component": "gzz"}), "gx": (3, {"component": "gx"}),
         "tf": (2, {"direction": TF_DIR})}


# ------------------------------------------------------------------------------------------ 1. the table

@pytest.mark.parametrize("field", sorted(KINDS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_table_is_the_dense_stores_entry_of_the_representative_pair(G, name, field):
    obs, b6 = geometry(**SHAPES[name])
    kind, kw = KINDS[field]
    lat = engine(G, obs, b6, True, kind, **kw)
    dense = engine(G, obs, b6, False, kind, **kw)
    info = lat.translation_invariant_info()
    T = lat.translation_invariant_table()
    A = np.asarray(dense.download_G())
    i, j = representative(obs, b6)
    nx, ny, nz = SHAPES[name]["cells"]
    px, qy = SHAPES[name]["obs"]
    assert info["on"] and (info["nx"], info["ny"], info["nz"], info["px"], info["qy"]) == (nx, ny, nz, px, qy)
    assert T.shape == (nz, nx + px - 1, ny + qy - 1) and info["table_bytes"] == T.size * 8
    assert np.array_equal(T, A[i, j])
    print(name, field, "max_dev", info["max_dev"])
    assert info["max_dev"] <= 1e-12
    if name in ON_100M:
        assert info["max_dev"] == 0.0
    lat.close()
    dense.close()


# ------------------------------------------------------------------------------ 2., 3. weights and operator

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_weights_forward_adjoint_against_oracle(G, orc, name):
    obs, b6, Aw, wm_o = reference(orc, name)
    N, M = Aw.shape
    eng = engine(G, obs, b6, True)
    wm = eng.weight(0.5)
    print(name, "weights", relmax(wm, wm_o))
    assert relmax(wm, wm_o) <= 1e-11
    rng = np.random.default_rng(11)
    x, r = rng.uniform(-1, 1, M) * wm_o, rng.normal(size=N)
    fw, ad = eng.forward(x), eng.adjoint(r)
    fo, ao = orc.forward(Aw, x), orc.adjoint(Aw, r)
    print(name, "forward", relmax(fw, fo), "adjoint", relmax(ad, ao))
    assert relmax(fw, fo) <= 1e-10 and relmax(ad, ao) <= 1e-10
    eng.close()


# -------------------------------------------------------------------------- 8. more than 16384 observations

@pytest.mark.parametrize("kw", [dict(cells=(4, 4, 1), obs=(130, 130), first=(-63, -63), h=(H7, H7), origin=(317.3, -911.7)),
                                dict(cells=(2, 2, 5), obs=(130, 513), first=(-64, -255))],
                         ids=["130x130 over 4x4x1", "130x513 over 2x2x5: layers per chunk"])
def test_more_than_16384_observations(G, orc, kw):
    obs, b6 = geometry(**kw)
    Aw, wm_o = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
    N, M = Aw.shape
    assert N > 16384
    eng = engine(G, obs, b6, True)
    # (points up to 65 cells from the mesh at 2000/7 m: the prism formula's own cancellation shows as 3e-12 of the largest
    # entry between the first and the last pair of an offset -- reported, the operator below is what is bounded)
    print("max_dev", eng.translation_invariant_info()["max_dev"])
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    rng = np.random.default_rng(12)
    x, r = rng.uniform(-1, 1, M) * wm_o, rng.normal(size=N)
    assert relmax(eng.forward(x), orc.forward(Aw, x)) <= 1e-10
    assert relmax(eng.adjoint(r), orc.adjoint(Aw, r)) <= 1e-10
    # the epilogue of the two-pass matrix-free form: misfit and gradient beyond 16384 rows
    dobs = orc.forward(Aw, 0.02 * wm_o) + 0.01 * rng.normal(size=N)
    eng.set_data(dobs)
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    P = orc.Problem(Aw, dobs, 0.001 * wm, "Damping", 1.0, 0.01, wm=wm, shape=(1, 1, M))
    out, ref = eng.misfit_and_grad(0.03 * wm), P.misfit_and_grad(0.03 * wm)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10 and relmax(out[2], ref[2]) <= 1e-10
    eng.close()


# --------------------------------------------------------------------- 4., 6., 7. the chain against the oracle

def _trajectories(rng, M, wm):
    return [(L, rng.normal(size=M) * 0.02 * wm, float(rng.uniform())) for L in (2, 3, 4, 5, 6, 2, 3, 4, 5, 6)]


def _chain_setup(eng, reg, shape, dobs, wm):
    eng.set_data(dobs)
    eng.set_reg(reg, 1.0, 0.01, shape, 0.001 * wm)


# (the chain's gradient is that of the WEIGHTED kernel: the shape with every cell row under observations, see above)
CHAIN_SHAPES = ("beyond", "shuffled", "covered row across 64 lanes")
#: step sizes at which the oracle accepts some of the ten trajectories and rejects others (MS, TV) or nearly all
DT = {"Damping": 0.2, "Smoothness": 0.2, "TV": 0.2, "MS": 0.02}


@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
@pytest.mark.parametrize("name", sorted(CHAIN_SHAPES))
def test_chain_against_oracle_and_bitwise_paths(G, orc, name, reg):
    obs, b6, Aw, wm_o = reference(orc, name)
    N, M = Aw.shape
    nx, ny, nz = SHAPES[name]["cells"]
    shape = (1, 1, M) if "shuffle" in SHAPES[name] else (nz, nx, ny)  # (stencils follow the caller's cell order)
    rng = np.random.default_rng(7)
    eng = engine(G, obs, b6, True)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    rho = np.zeros(M)
    rho[rng.choice(M, max(1, M // 10), replace=False)] = 0.03
    dobs = Aw @ (wm * rho) + 1e-3 * np.abs(Aw @ (wm * rho)).max() * rng.normal(size=N)
    _chain_setup(eng, reg, shape, dobs, wm)
    P = orc.Problem(Aw, dobs, 0.001 * wm, reg, 1.0, 0.01, wm=wm, shape=shape)
    low, high = 0.0 * wm, 0.05 * wm
    dt = DT[reg]
    trajs = _trajectories(rng, M, wm)

    xt = rng.uniform(0, 0.05, M) * wm
    out, ref = eng.misfit_and_grad(xt), P.misfit_and_grad(xt)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10
    assert relmax(out[2], ref[2]) <= 1e-10

    # trajectory by trajectory against the oracle
    eng.chain_init(0.001 * wm, low, high)
    plain, clamps = [], 0
    xo = 0.001 * wm
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        x = eng.chain_get_x()
        plain.append((acc, o.copy(), x))
        xo, acco, oo, _ = P.leapfrog(xo, p0, dt, L, low, high, u)
        assert bool(acc) == bool(acco)
        assert relmax(o, oo) <= 1e-10 and relmax(x, xo) <= 1e-10
        clamps += int(acc and (np.any(x == low) or np.any(x == high)))
    assert 0 < sum(a for a, _, _ in plain) and clamps > 0

    # run_chain with the next trajectory's first step piped into the last sweep: the same bits
    eng.chain_init(0.001 * wm, low, high)
    piped, last = [], 0.001 * wm
    eng.run_chain(iter(trajs), dt, lambda L, a_, o_, x_: piped.append((a_, o_.copy(), x_)), want_x=True, batch=4,
                  overlap=True)
    assert len(piped) == len(plain)
    for (a1, o1, x1), (a2, o2, x2) in zip(plain, piped):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last)

    # stateless leapfrog: the same bits as the chain
    x = 0.001 * wm
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        x, acc2, o2, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        assert acc2 == acc and np.array_equal(x, xs) and np.array_equal(o2, o)

    # a second engine: the same bits
    eng2 = engine(G, obs, b6, True)
    assert np.array_equal(eng2.weight(0.5), wm)
    assert np.array_equal(eng2.translation_invariant_table(), eng.translation_invariant_table())
    _chain_setup(eng2, reg, shape, dobs, wm)
    eng2.chain_init(0.001 * wm, low, high)
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        acc2, o2 = eng2.chain_trajectory(p0, dt, L, u)
        assert acc2 == acc and np.array_equal(o2, o) and np.array_equal(eng2.chain_get_x(), xs)
    eng2.close()
    eng.close()


# ----------------------------------------------------------- 5. the chain against dense: a component and tf

@pytest.mark.parametrize("field", ["gzz", "tf"])
def test_chain_of_a_component_and_tf_against_the_dense_store(G, monkeypatch, field):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    obs, b6 = geometry(**SHAPES["beyond"])
    nx, ny, nz = SHAPES["beyond"]["cells"]
    N, M = obs.shape[1], b6.shape[0]
    kind, kw = KINDS[field]
    lat, dense = engine(G, obs, b6, True, kind, **kw), engine(G, obs, b6, False, kind, **kw)
    wm = dense.weight(0.5)
    assert relmax(lat.weight(0.5), wm) <= 1e-11
    rng = np.random.default_rng(8)
    rho = np.zeros(M)
    rho[rng.choice(M, M // 10, replace=False)] = 0.03
    d0 = dense.forward(wm * rho)
    assert relmax(lat.forward(wm * rho), d0) <= 1e-10
    dobs = d0 + 1e-3 * np.abs(d0).max() * rng.normal(size=N)
    low, high = 0.0 * wm, 0.05 * wm
    trajs = _trajectories(rng, M, wm)
    for eng in (lat, dense):
        _chain_setup(eng, "TV", (nz, nx, ny), dobs, wm)
        eng.chain_init(0.001 * wm, low, high)
    xt = rng.uniform(0, 0.05, M) * wm
    out, ref = lat.misfit_and_grad(xt), dense.misfit_and_grad(xt)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10
    # (no oracle of these fields to choose a step size with: a large one, whose trajectories the test may all reject, and
    # two small ones whose energy error is small enough to accept)
    accepted = 0
    for dt in (0.05, 0.005, 0.0005):
        for L, p0, u in trajs:
            a1, o1 = lat.chain_trajectory(p0, dt, L, u)
            a2, o2 = dense.chain_trajectory(p0, dt, L, u)
            assert bool(a1) == bool(a2) and relmax(o1, o2) <= 1e-10
            assert relmax(lat.chain_get_x(), dense.chain_get_x()) <= 1e-10
            accepted += int(a1)
    assert accepted > 0
    lat.close()
    dense.close()


# ------------------------------------------------------------------------------------------ 9. the module

MODULE = dict(mrange=(0.0, 7 * 150.0, 0.0, 5 * 150.0, 0.0, 450.0), mspacing=(150.0, 150.0, 150.0))


def _module_obs(G):
    """gridded data above the cell centres of the module's own mesh, whatever axis it calls x"""
    mesh = G.mesher.PrismMesh(MODULE["mrange"], MODULE["mspacing"])
    b6 = mesh.cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    return xp, yp, np.full(xp.size, -20.0), b6.shape[0]


@pytest.mark.parametrize("kw", [{}, {"component": "gzz"}, {"field": "magnetic", "mangle": (60, 10)}], ids=["gz", "gzz", "magnetic"])
def test_module_matches_the_dense_module(G, tmp_path, monkeypatch, capsys, kw):
    monkeypatch.chdir(tmp_path)
    xp, yp, zp, M = _module_obs(G)
    rng = np.random.default_rng(21)

    def make(dobs, ti):
        return G.GravMagModule(dobs, MODULE["mrange"], MODULE["mspacing"], (xp, yp, zp), verbose=False,
                               translation_invariant=ti, **kw)

    # data of a block of anomalous cells, from the dense module's own kernel, plus noise
    probe = make(np.zeros(xp.size), False)
    wm = probe.Wm.diagonal()
    rho = np.zeros(M)
    rho[M // 3:M // 3 + M // 8] = 0.015
    d = probe._engine.forward(wm * rho)
    probe._engine.close()
    dobs = d + 0.01 * np.abs(d).max() * rng.normal(size=d.size)
    lat, dense = make(dobs, True), make(dobs, False)
    info = lat.translation_invariant_info()
    assert info["on"] and info["nx"] * info["ny"] * info["nz"] == M and not dense.translation_invariant_info()["on"]
    assert lat.matrix_free and lat.translation_invariant and not dense.translation_invariant
    assert relmax(lat.Wm.diagonal(), wm) <= 1e-11
    x = rng.uniform(0, 1, M) * wm
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        a = lat.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-11
    assert relmax(lat._engine.forward(x), dense._engine.forward(x)) <= 1e-10
    rows = [_sample(G, mod, M, tag) for tag, mod in (("lat", lat), ("dense", dense))]
    capsys.readouterr()
    assert rows[0].shape == rows[1].shape == (6, M)
    # (1e-8: one unit of the text sink's last digit, as the difference of two printed numbers comes out in binary)
    assert np.abs(rows[0] - rows[1]).max() <= 1e-8 * (1 + 1e-6)
    lat._engine.close()
    dense._engine.close()


def _sample(G, mod, M, tag):
    """a few draws of HMCSample with a fixed seed (posterior stream on): the accepted rows of the 8-digit text sink"""
    folder = "%s_chain" % tag
    G.HMCSample(mod, 6, 2, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, 0.0), np.full(M, 0.02)],
                "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3, nbest=100, myrank=0,
                save_folder=folder, posterior_stream=True)
    return np.atleast_2d(np.loadtxt(folder + "0/model.dat"))


# ---------------------------------------------------------------------------------------- 10. refusals

def test_refusals_name_the_store(G):
    from gravinv3dhmc_amd import _lib
    obs, b6 = geometry(**SHAPES["centres"])
    N, M = obs.shape[1], b6.shape[0]
    store = "translation-invariant store"

    # geometry without the structure: the reason, with "spacing" for the linspace grid
    o2, c2 = c2_linspace()
    eng = G.Engine(o2.shape[1], c2.shape[0])
    eng.set_translation_invariant(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in o2])
    eng.set_cells(c2, 0)
    with pytest.raises(NotImplementedError, match="spacing") as e:
        eng.build_G()
    assert store in str(e.value)
    eng.close()

    # combinations with the other matrix-free forms: GH_ERR_ARG
    eng = G.Engine(N, M)
    eng.set_translation_invariant(True)
    for call in (eng.set_matrix_free, eng.set_shift_invariant):
        with pytest.raises(ValueError, match=store):
            call(True)
    eng.close()
    eng = G.Engine(N, M)
    eng.set_matrix_free(True)
    with pytest.raises(ValueError, match="translation_invariant"):
        eng.set_translation_invariant(True)
    eng.close()

    # tesseroids
    eng = G.Engine(N, M)
    eng.set_translation_invariant(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    tb = np.ascontiguousarray(np.stack([b6[:, 0] * 1e-3, b6[:, 1] * 1e-3, b6[:, 2] * 1e-3, b6[:, 3] * 1e-3, -b6[:, 4],
                                        -b6[:, 5] - 1.0], axis=1))
    eng.set_cells(tb, 1)
    with pytest.raises(NotImplementedError, match=store):
        eng.build_G()
    eng.close()

    # a store of blocks (dense_single_chain_refuse's wording)
    eng = G.Engine(2 * N, M)
    eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 1.0])
    with pytest.raises(NotImplementedError, match="gh_set_translation_invariant: not supported on"):
        eng.set_translation_invariant(True)
    eng.close()
    eng = G.Engine(2 * N, M)
    eng.set_translation_invariant(True)
    with pytest.raises(NotImplementedError):
        eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 1.0])
    eng.close()

    # what does not run on the built store
    eng = engine(G, obs, b6, True)
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    x0 = np.stack([0.01 * wm, 0.02 * wm])
    for what, call in (("wavelet", lambda: eng.compress_wavelet(1, (1, 1, M), 0.001, 2)),
                       ("batch", lambda: eng.batch_init(x0, 0.0 * wm, 1.0 * wm)),
                       ("upload", lambda: eng.upload_G(np.zeros((N, M)))),
                       ("bscg", lambda: eng.bscg_run(np.ones((2, N)), np.zeros(N), 0.01 * wm, 0.0, 1.0, 0.0, 2, 4))):
        with pytest.raises(NotImplementedError, match=store):
            call()
        print("refused:", what)
    lib = _lib.load()
    import ctypes
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 2 * M), (lib.gh_shard_init_rows, 2 * N)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        assert rc == _lib.GH_ERR_UNSUPPORTED and store.encode() in lib.gh_last_error(eng._h)
    with pytest.raises(ValueError):
        eng.download_G()
    eng.close()

    # switched on and off again: the dense store, bit for bit
    eng = G.Engine(N, M)
    eng.set_translation_invariant(True)
    eng.set_translation_invariant(False)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, 0)
    eng.build_G()
    ref = engine(G, obs, b6, False)
    assert not eng.translation_invariant_info()["on"]
    assert np.array_equal(np.asarray(eng.download_G()), np.asarray(ref.download_G()))
    eng.close()
    ref.close()


def test_module_refusals(G):
    xp, yp, zp, M = _module_obs(G)
    dobs = np.zeros(xp.size)
    store = "translation-invariant store"

    def make(**kw):
        return G.GravMagModule(dobs, MODULE["mrange"], MODULE["mspacing"], (xp, yp, zp), verbose=False, **kw)

    class Ranks:
        world, rank = 2, 0

    for kw in (dict(wavelet="1D"), dict(shard=Ranks()), dict(matrix_free=True), dict(shift_invariant=True),
               dict(mtopo=(xp, yp, zp))):
        with pytest.raises(NotImplementedError, match=store):
            make(translation_invariant=True, **kw)
    with pytest.raises(NotImplementedError, match=store):
        G.GravMagModule(dobs, (0, 10, 0, 10, 0, 1000), (1000, 1, 1), (xp, yp, zp), verbose=False, coordinate="spherical",
                        translation_invariant=True)
    # as before: the shift-invariant store is for spherical models
    with pytest.raises(NotImplementedError, match="shift-invariant store is for spherical"):
        make(shift_invariant=True)
    # the linspace grid of the benchmark's geometry: the detection's reason
    n = 7
    yl, xl = [a.ravel() for a in np.meshgrid(np.linspace(0, 150.0 * 5, 5), np.linspace(0, 150.0 * n, n))]
    with pytest.raises(NotImplementedError, match="spacing") as e:
        G.GravMagModule(np.zeros(xl.size), MODULE["mrange"], MODULE["mspacing"], (xl, yl, np.zeros_like(xl)), verbose=False,
                        translation_invariant=True)
    assert store in str(e.value)
    from gravinv3dhmc_amd.inversion import hmc
    mod = make(translation_invariant=True)
    with pytest.raises(NotImplementedError, match=store):
        hmc.HMCSampleBatch(mod, 2, 2, 1, 0.01, [2, 3], np.full(M, 0.001), np.full(M, 0.001),
                           np.c_[np.zeros(M), np.full(M, 0.02)], "mandatory", 1000, dobs, "Fixed", 0.8, 1.0, "TV", 0.001,
                           5, 0.3)
