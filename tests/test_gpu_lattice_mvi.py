"""GPU suite (`-m gpu`): the magnetization-vector store on the translation-invariant table (gh_set_cells_mvi_table,
csrc/latmvi.hip.h; host_lattice.h) -- the axis of a column as one more layer coordinate, T[b][ax nz + k][u][v].

  1. the fill: every (data block, axis) table against the dense gh_set_cells_mvi_data store, bit for bit -- the entries
     of every offset's first pair, and on coordinates whose differences are exact the expanded table, entry for entry;
     the tf block against gh_set_cells_mvi's store too; max_dev;
  2. weights, forward and adjoint at the edges of the new index arithmetic (lattice_mvi_cases.EDGE_CASES) against
     magvecdata_host.stack on the dense store's unweighted entries;
  3. a forward chunk that holds layers of two axes, and more than 16384 rows, through the host table operator on the
     device's tables, with the per-block epilogue;
  4. potential, block means, amplitude term and chains of ten trajectories under the four regularisers, the coupling
     off and on, against VecDataProblem on the expanded tables and the dense engine; run_chain, leapfrog, the
     trajectory feeder and a second engine bit for bit;
  5. MagVectorModule(translation_invariant=True) against the dense module, both data forms; past 16384 rows;
  6. refusals.
Bounds: the table bit for bit; wm 1e-11; forward, adjoint, potential, gradient, chain 1e-10; the two modules' potentials
1e-12 / 1e-11 (tests/test_gpu_lattice_multi.py's)."""
import numpy as np
import pytest

import lattice_mvi_cases as C
from helpers import relmax
from lattice_cases import c2_linspace, detect, geometry
from lattice_multi_cases import TableOperator
from magvecdata_host import VecDataProblem, stack
from magvector_host import amplitude_term

pytestmark = pytest.mark.gpu

VSTORE, TABLE = "vector-data magnetization store", "translation-invariant table"
FOLD_MAX_DEV = 1e-7
ALL = ("tf", "bx", "by", "bz")


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


_DENSE = {}


def dense_blocks(G, name):
    """obs, bounds6 and K[comp] = (3, n, m), the unweighted entries of the dense vector-data store of all four data
    components (download_G before weight): computed once per shape, shared, left unchanged"""
    if name not in _DENSE:
        obs, b6 = C.shape(name)
        n, m = obs.shape[1], b6.shape[0]
        eng = C.mvi_engine(G, obs, b6, ALL, np.ones(4), False)
        A = np.array(eng.download_G())
        eng.close()
        K = {c: np.stack([A[b * n:(b + 1) * n, ax * m:(ax + 1) * m] for ax in range(3)]) for b, c in enumerate(ALL)}
        for a in [obs, b6] + list(K.values()):
            a.setflags(write=False)
        _DENSE[name] = (obs, b6, K)
    return _DENSE[name]


# ------------------------------------------------------------------------------------------ 1. the fill

@pytest.mark.parametrize("data", [("tf",), ALL], ids=["tf", "all four"])
@pytest.mark.parametrize("name", C.FILL_SHAPES)
def test_tables_are_the_dense_stores_entries(G, name, data):
    obs, b6, K = dense_blocks(G, name)
    nx, ny, nz = C.SHAPES[name]["cells"]
    px, qy = C.SHAPES[name]["obs"]
    lat = C.mvi_engine(G, obs, b6, data, np.ones(len(data)), True)
    info = lat.translation_invariant_info()
    T = lat.translation_invariant_table()
    assert info["on"] and (info["nx"], info["ny"], info["nz"], info["px"], info["qy"]) == (nx, ny, nz, px, qy)
    assert info["axes"] == 3 and info["chunks"] * info["layers_per_chunk"] >= 3 * nz
    assert T.shape == (len(data), 3, nz, nx + px - 1, ny + qy - 1) and info["table_bytes"] == T.size * 8
    i, j = C.representative(obs, b6)

    def same(T3, K3, c):
        """the table of a block is the dense store's entries: of every offset's first pair, and -- coordinates whose
        differences are exact -- of ALL pairs, the expanded table entry for entry"""
        for ax in range(3):
            assert np.array_equal(T3[ax], K3[ax][i, j]), (c, ax)
        if name in C.EXACT_SHAPES:
            assert np.array_equal(C.expand_axes(T3, obs, b6), K3), c

    for b, c in enumerate(data):
        same(T[b], K[c], c)
    if data == ("tf",):
        # gh_set_cells_mvi's store: the same entries
        one = C.mvi_engine(G, obs, b6, data, None, False, dense_mvi=True)
        A = np.array(one.download_G())
        one.close()
        m = b6.shape[0]
        same(T[0], np.stack([A[:, ax * m:(ax + 1) * m] for ax in range(3)]), "gh_set_cells_mvi")
    print(name, data, "max_dev", info["max_dev"])
    assert info["max_dev"] <= FOLD_MAX_DEV
    with pytest.raises(ValueError):
        lat.download_G()
    lat.close()


# --------------------------------------------------------------------------------- 2. the operator at the edges

@pytest.mark.parametrize("case", C.EDGE_CASES, ids=["%s: %s" % (e[0], "+".join(e[1])) for e in C.EDGE_CASES])
def test_weights_forward_adjoint_at_the_index_edges(G, case):
    name, data, w = case
    obs, b6, K = dense_blocks(G, name)
    n, m = obs.shape[1], b6.shape[0]
    Aw, wm_o, _, _ = stack(K, data, w)
    eng = C.mvi_engine(G, obs, b6, data, w, True)
    wm = eng.weight(0.5)
    rng = np.random.default_rng(11)
    x, r = rng.uniform(-1, 1, 3 * m) * wm_o, rng.normal(size=len(data) * n)
    fw, ad, fo, ao = eng.forward(x), eng.adjoint(r), Aw @ x, Aw.T @ r
    ef = max(relmax(fw[b * n:(b + 1) * n], fo[b * n:(b + 1) * n]) for b in range(len(data)))
    ea = max(relmax(ad[ax * m:(ax + 1) * m], ao[ax * m:(ax + 1) * m]) for ax in range(3))     # (axis by axis)
    print(name, data, "weights", relmax(wm, wm_o), "forward", ef, "adjoint", ea)
    assert relmax(wm, wm_o) <= 1e-11 and ef <= 1e-10 and ea <= 1e-10
    info = eng.multi_info()
    assert len(info["components"]) == len(data) and np.array_equal(info["weights"], np.asarray(w))
    eng.close()


# -------------------------------------------------------- 3. chunks across two axes, more than 16384 rows

class TableProblem(VecDataProblem):
    """VecDataProblem on a TableOperator instead of the stacked array"""

    def __init__(self, op, dobsw, ncomp, mwapr, wm):
        self.Aw, (self.N, self.M) = op, op.shape
        self.ncomp, self.n = ncomp, self.N // ncomp
        self.dobsw, self.mwapr = np.asarray(dobsw, dtype=np.float64), np.asarray(mwapr, dtype=np.float64)
        self.reg, self.alpha, self.beta = "Damping", 1.0, 0.01
        self.wm = np.asarray(wm, dtype=np.float64)
        self.wm2, self.shape = self.wm ** 2, (1, 1, self.M // 3)
        self.lam, self.global_mean, self.phi = 0.0, False, 0.0


def _against_the_table_operator(eng, obs, b6, data, w, what):
    """weights, forward, adjoint, potential and the blocks' means of a built table engine against the host operator
    on the engine's own tables (whose entries test 1 pins), over 3 nz layers on the expanded cell map"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    n, m, nb = px * qy, nx * ny * nz, len(data)
    T = eng.translation_invariant_table()
    op = TableOperator([T[b].reshape(3 * nz, T.shape[-2], T.shape[-1]) for b in range(nb)], w, (nx, ny, 3 * nz, px, qy),
                       C.axis_maps(col, m), ool)
    wm = eng.weight(0.5)
    rng = np.random.default_rng(12)
    x, r = rng.uniform(-1, 1, 3 * m) * op.wm, rng.normal(size=nb * n)
    fw, fo = eng.forward(x), op @ x
    ef = max(relmax(fw[b * n:(b + 1) * n], fo[b * n:(b + 1) * n]) for b in range(nb))
    ad, ao = eng.adjoint(r), op.T @ r
    ea = max(relmax(ad[ax * m:(ax + 1) * m], ao[ax * m:(ax + 1) * m]) for ax in range(3))
    print(what, "weights", relmax(wm, op.wm), "forward", ef, "adjoint", ea)
    assert relmax(wm, op.wm) <= 1e-11 and ef <= 1e-10 and ea <= 1e-10
    # the per-block epilogue: misfit, gradient and the blocks' means
    dobsw = op @ (0.3 * op.wm) + 0.01 * np.abs(fo).max() * rng.normal(size=nb * n) + np.repeat(np.arange(1.0, nb + 1), n)
    eng.set_data(dobsw)
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, m), 0.01 * op.wm)
    P = TableProblem(op, dobsw, nb, 0.01 * op.wm, op.wm)
    out, ref = eng.misfit_and_grad(0.5 * x), P.misfit_and_grad(0.5 * x)
    print(what, "value", abs(out[0] - ref[0]) / abs(ref[0]), "grad", relmax(out[1], ref[1]), "dpre", relmax(out[2], ref[2]))
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10 and relmax(out[2], ref[2]) <= 1e-10
    info = eng.multi_info()
    assert relmax(info["pred_mean"], P.pred_mean) <= 1e-10 and relmax(info["obs_mean"], P.obs_mean) <= 1e-10


def test_a_forward_chunk_holds_layers_of_two_axes(G):
    data, w = ("bx", "by", "bz"), np.array((2.0, 1.0, 0.125))
    kw = dict(obs=(130, 130), first=(-55, -55), zobs=-15.0)
    # (15 layers in 8 chunks of 2 on a 256-CU device: chunk 2 is the last layer of x and the first of y; where the device
    # at hand plans otherwise, the layers are chosen from its plan)
    for nz in (5, 4, 7, 8, 10, 11):
        obs, b6 = geometry(cells=(20, 20, nz), **kw)
        eng = C.mvi_engine(G, obs, b6, data, w, True)
        info = eng.translation_invariant_info()
        lpc = info["layers_per_chunk"]
        chunks = [set(L // nz for L in range(c * lpc, min(3 * nz, (c + 1) * lpc))) for c in range(info["chunks"])]
        if any(len(s) == 2 for s in chunks):
            break
        eng.close()
    print("layers", 3 * nz, "chunks", info["chunks"], "of", lpc, "axes per chunk", chunks)
    assert info["nz"] == nz and any(len(s) == 2 for s in chunks)
    assert eng.N == 3 * 16900
    _against_the_table_operator(eng, obs, b6, data, w, "straddle")
    eng.close()


BEYOND = {"tf 130x130": (("tf",), (1.0,), dict(cells=(20, 20, 2), obs=(130, 130), first=(-55, -55), zobs=-15.0)),
          "3 x 75x75": (("bx", "by", "bz"), (2.0, 1.0, 0.125),
                        dict(cells=(20, 20, 2), obs=(75, 75), first=(-27, -27), h=(C.H7, C.H7), origin=(317.3, -911.7),
                             zobs=-15.0))}


@pytest.mark.parametrize("case", sorted(BEYOND))
def test_more_than_16384_rows(G, case):
    data, w, kw = BEYOND[case]
    obs, b6 = geometry(**kw)
    assert len(data) * obs.shape[1] > 16384
    eng = C.mvi_engine(G, obs, b6, data, np.asarray(w), True)
    print(case, "max_dev", eng.translation_invariant_info()["max_dev"])
    _against_the_table_operator(eng, obs, b6, data, np.asarray(w), case)
    eng.close()


# ---------------------------------------------------------------- 4. potential, means, amplitude and chains

def _setup(eng, reg, shape3, dobsw, wm, lam):
    eng.set_data(dobsw)
    eng.set_reg(reg, 1.0, 0.01, shape3, 0.01 * wm)
    if lam > 0:
        eng.set_amplitude(lam, C.AMP_BETA, 1.0)


@pytest.mark.parametrize("lam", [0.0, C.LAMBDA], ids=["plain", "amplitude"])
@pytest.mark.parametrize("reg", C.REGS)
@pytest.mark.parametrize("case", sorted(C.CHAIN_CASES))
def test_potential_and_chain_against_the_restatement_and_bitwise_paths(G, monkeypatch, case, reg, lam):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    name, data, weights = C.CHAIN_CASES[case]
    obs, b6 = C.shape(name)
    n, m = obs.shape[1], b6.shape[0]
    wts = np.ones(len(data)) if weights is None else np.asarray(weights)
    eng = C.mvi_engine(G, obs, b6, data, wts, True)
    # the reference: the restatement on the engine's own tables, expanded (test 1 pins their entries); the host's
    # kernels, on which the case was conditioned, are the same to rounding: the same decisions
    T = eng.translation_invariant_table()
    K = {c: C.expand_axes(T[b], obs, b6) for b, c in enumerate(data)}
    Kh = C.host_blocks(obs, b6, C.direction())
    assert max(relmax(K[c], Kh[c]) for c in data) <= 1e-9
    w, wm_o, dobsw, shape3, P, low, high, x0, trajs, xt, dt = C.chain_case(K, case, reg, lam)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    _setup(eng, reg, shape3, dobsw, wm_o, lam)

    out, ref = eng.misfit_and_grad(xt), P.misfit_and_grad(xt)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10
    assert relmax(out[2], ref[2]) <= 1e-10
    info = eng.multi_info()
    assert relmax(info["pred_mean"], P.pred_mean) <= 1e-10 and relmax(info["obs_mean"], P.obs_mean) <= 1e-10
    if lam > 0:
        phi, gp, amp = eng.amplitude_eval(xt)
        pr, gr, ar = amplitude_term(xt, wm_o, C.AMP_BETA)
        assert abs(eng.amplitude_last() - P.phi) <= 1e-10 * abs(P.phi)
        assert abs(phi - pr) <= 1e-10 * abs(pr) and relmax(gp, gr) <= 1e-10 and relmax(amp, ar) <= 1e-10

    # trajectory by trajectory against the restatement
    eng.chain_init(x0, low, high)
    plain, clamps, xo = [], 0, x0
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        x = eng.chain_get_x()
        plain.append((acc, o.copy(), x))
        xo, acco, oo = P.leapfrog(xo, p0, dt, L, low, high, u)
        assert bool(acc) == bool(acco)
        assert relmax(o, oo) <= 1e-10 and relmax(x, xo) <= 1e-10
        clamps += int(acc and (np.any(x == low) or np.any(x == high)))
    accepted = sum(bool(a) for a, _, _ in plain)
    print(case, reg, lam, "accepted", accepted, "of", len(plain), "accepted states on a bound", clamps)
    assert 0 < accepted < len(plain) and clamps > 0

    # run_chain with the next trajectory's first step piped into the last sweep: the same bits
    eng.chain_init(x0, low, high)
    piped, last = [], x0
    eng.run_chain(iter(trajs), dt, lambda L, a_, o_, x_: piped.append((a_, o_.copy(), x_)), want_x=True, batch=4,
                  overlap=True)
    assert len(piped) == len(plain)
    for (a1, o1, x1), (a2, o2, x2) in zip(plain, piped):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last)

    # stateless leapfrog: the same bits as the chain
    x = x0
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        x, acc2, o2, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        assert acc2 == acc and np.array_equal(x, xs) and np.array_equal(o2, o)

    # a second engine: the same bits; the dense engine (its weighting lies in the store): 1e-10.  The unweighted total
    # field alone is gh_set_cells_mvi's dense store, of one block without a block table.
    eng2 = C.mvi_engine(G, obs, b6, data, wts, True)
    assert np.array_equal(eng2.weight(0.5), wm) and np.array_equal(eng2.translation_invariant_table(), T)
    dense = C.mvi_engine(G, obs, b6, data, wts, False)
    assert bool(dense.multi) == (weights is not None)
    assert relmax(dense.weight(0.5), wm) <= 1e-11
    for e in (eng2, dense):
        _setup(e, reg, shape3, dobsw, wm_o, lam)
        e.chain_init(x0, low, high)
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        acc2, o2 = eng2.chain_trajectory(p0, dt, L, u)
        assert acc2 == acc and np.array_equal(o2, o) and np.array_equal(eng2.chain_get_x(), xs)
        acc3, o3 = dense.chain_trajectory(p0, dt, L, u)
        assert bool(acc3) == bool(acc) and relmax(o3, o) <= 1e-10 and relmax(dense.chain_get_x(), xs) <= 1e-10
    for e in (eng, eng2, dense):
        e.close()


@pytest.mark.parametrize("case", ["tf", "vector"])
def test_trajectory_feeder_gives_the_loops_bits(G, monkeypatch, case):
    from gravinv3dhmc_amd.inversion.rng import LegacyDraws
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    name, data, weights = C.CHAIN_CASES[case]
    obs, b6 = C.shape(name)
    wts = np.ones(len(data)) if weights is None else np.asarray(weights)
    w, wm, dobsw, shape3, P, low, high, x0, trajs, xt, dt = C.chain_case(C.host_blocks(obs, b6, C.direction()), case, "TV",
                                                                         C.LAMBDA)
    runs = []
    for feed in (True, False):
        monkeypatch.setenv("GRAVHMC_CHAIN_FEED", "1" if feed else "0")
        eng = C.mvi_engine(G, obs, b6, data, wts, True)
        eng.weight(0.5)
        _setup(eng, "TV", shape3, dobsw, wm, C.LAMBDA)
        eng.chain_init(x0, low, high)
        res = []
        draws = LegacyDraws(3 * b6.shape[0], (2, 6), float(0.3 * wm.mean()), limit=8, seed=11)
        try:
            eng.run_chain(draws, dt, lambda L, a, o, x: res.append((int(L), bool(a), np.array(o), None if x is None else
                                                                    np.array(x))), overlap=True, want_x=True)
        finally:
            draws.release()
        assert (eng.feed_stats()["run"] > 0) == feed
        runs.append((res, eng.chain_get_x()))
        eng.close()
    (fed, xf), (ref, xr) = runs
    assert len(fed) == len(ref) == 8 and np.array_equal(xf, xr)
    for (L1, a1, o1, x1), (L2, a2, o2, x2) in zip(fed, ref):
        assert L1 == L2 and a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2))
    print(case, "accepted", sum(r[1] for r in fed), "of", len(fed))


# ------------------------------------------------------------------------------------------ 5. the module

MODULE = dict(mrange=(0.0, 7 * 150.0, 0.0, 5 * 150.0, 0.0, 450.0), mspacing=(150.0, 150.0, 150.0))


def _centres(G, mrange, mspacing, height=-20.0):
    """gridded data above the cell centres of the module's own mesh, whatever axis it calls x: (x, y, z), bounds6"""
    b6 = G.mesher.PrismMesh(mrange, mspacing).cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    return (xp, yp, np.full(xp.size, height)), np.ascontiguousarray(b6)


def _sample(G, mod, M, tag, stream):
    """a few draws of HMCSample with a fixed seed: the accepted rows of the 8-digit text sink"""
    folder = "%s_chain" % tag
    ch = G.HMCSample(mod, 6, 2, 0.05, [3, 8], np.full(M, 0.01), np.full(M, 0.01), np.c_[np.full(M, -1.0), np.full(M, 1.0)],
                     "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3, nbest=100, myrank=0,
                     save_folder=folder, posterior_stream=stream)
    return np.atleast_2d(np.loadtxt(folder + "0/model.dat")), ch


@pytest.mark.parametrize("data", [("tf",), ("tf", "bx", "bz")], ids=["tf", "vector"])
def test_module_matches_the_dense_module(G, tmp_path, monkeypatch, capsys, data):
    monkeypatch.chdir(tmp_path)
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n, M = obs[0].size, 3 * b6.shape[0]
    rng = np.random.default_rng(21)
    vector = data != ("tf",)

    def make(dobs, ti, **kw):
        return G.MagVectorModule(dobs if vector else dobs[0], MODULE["mrange"], MODULE["mspacing"], obs, mangle=(C.INC, C.DEC),
                                 data=data, weights="std" if vector else None, verbose=False, translation_invariant=ti, **kw)

    probe = make([rng.normal(size=n) for _ in data], False)
    truth = np.zeros(M)
    for ax, val in enumerate((0.6, -0.9, 0.4)):
        truth[ax * (M // 3) + M // 9:ax * (M // 3) + M // 9 + M // 24] = val
    d = probe.forward(truth)
    probe._engine.close()
    dobs = [d[c * n:(c + 1) * n] + 0.01 * np.abs(d[c * n:(c + 1) * n]).max() * rng.normal(size=n) for c in range(len(data))]
    lat, dense = make(dobs, True, amplitude=0.02, amplitude_beta=1.0), make(dobs, False, amplitude=0.02, amplitude_beta=1.0)
    info = lat.translation_invariant_info()
    assert info["on"] and info["axes"] == 3 and 3 * info["nx"] * info["ny"] * info["nz"] == M and lat.translation_invariant
    assert not dense.translation_invariant and not dense._engine.translation_invariant_info()["on"]
    wm = dense.Wm.diagonal()
    assert relmax(lat.Wm.diagonal(), wm) <= 1e-11
    if vector:
        assert np.array_equal(lat.weights, dense.weights)
        assert relmax(lat.Wb.diagonal(), dense.Wb.diagonal()) <= 1e-10 and relmax(lat.dobsw, dense.dobsw) <= 1e-10
    x = rng.uniform(-1, 1, M) * wm
    for reg in C.REGS:
        a = lat.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        print(data, reg, abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]))
        assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-11
        assert abs(lat.last_amplitude - dense.last_amplitude) <= 1e-12 * abs(dense.last_amplitude)
        if vector:
            assert relmax(lat.block_means()[0], dense.block_means()[0]) <= 1e-10
    model = rng.uniform(-1, 1, M)
    fl, fd = lat.forward(model), dense.forward(model)
    assert max(relmax(fl[c * n:(c + 1) * n], fd[c * n:(c + 1) * n]) for c in range(len(data))) <= 1e-10
    (pa, ga, aa), (pb, gb, ab) = lat.Amplitude(model), dense.Amplitude(model)
    assert abs(pa - pb) <= 1e-12 * abs(pb) and relmax(ga, gb) <= 1e-11 and relmax(aa, ab) <= 1e-11
    assert np.array_equal(lat.from_vectors(lat.to_vectors(model)), model)
    assert np.array_equal(lat.amplitude(model), dense.amplitude(model))
    assert all(np.array_equal(p, q) for p, q in zip(lat.direction(model), dense.direction(model)))
    for what in (lambda: lat.Aw, lambda: lat.A, lambda: lat.kernel("x", data[0] if vector else None)):
        with pytest.raises(NotImplementedError, match="magnetiz") as e:
            what()
        assert "translation-invariant table" in str(e.value)
    rows = [_sample(G, mod, M, tag, False)[0] for tag, mod in (("lat", lat), ("dense", dense))]
    assert rows[0].shape == rows[1].shape and rows[0].shape[1] == M and rows[0].shape[0] > 0
    # (1e-8: one unit of the text sink's last digit, as the difference of two printed numbers comes out in binary)
    assert np.abs(rows[0] - rows[1]).max() <= 1e-8 * (1 + 1e-6)
    _, ch = _sample(G, lat, M, "stream", True)
    capsys.readouterr()
    post = lat._engine.posterior_stream_read()
    assert np.all(np.isfinite(post["mean"])) and np.all(np.isfinite(post["std"]))
    with pytest.raises(NotImplementedError, match=VSTORE):
        G.HMCSampleBatch(lat, 2, 1, 1, 0.1, (1, 2), None, None, None, "mandatory", 1.0, None, False, 1.0, 1.0, "Damping",
                         0.01, 1, None)
    lat._engine.close()
    dense._engine.close()


def test_module_beyond_the_dense_forms_limit(G, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    mrange, mspacing = (0.0, 13000.0, 0.0, 13000.0, 0.0, 100.0), (100.0, 100.0, 100.0)
    obs, b6 = _centres(G, mrange, mspacing, -50.0)
    n, M = obs[0].size, 3 * b6.shape[0]
    assert n == 16900
    rng = np.random.default_rng(31)
    dobs = rng.normal(size=n)
    with pytest.raises(NotImplementedError, match="16384"):
        G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=(C.INC, C.DEC), verbose=False)
    mod = G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=(C.INC, C.DEC), verbose=False, translation_invariant=True)
    assert mod._engine.N == n and mod.translation_invariant_info()["on"]
    G.HMCSample(mod, 2, 1, 0.05, [2, 3], np.full(M, 0.01), np.full(M, 0.01), np.c_[np.full(M, -1.0), np.full(M, 1.0)],
                "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "Damping", 0.001, 5, 0.3, nbest=100, myrank=0,
                save_folder="big_chain", sample_sink="none")
    capsys.readouterr()
    assert np.all(np.isfinite(mod._engine.chain_get_x()))
    mod._engine.close()


# ---------------------------------------------------------------------------------------------- 6. refusals

def test_engine_refusals_name_the_store_and_the_table(G):
    import ctypes
    from gravinv3dhmc_amd import _lib
    obs, b6 = C.shape("beyond")
    n, m = obs.shape[1], b6.shape[0]
    data, w = ("tf", "bz"), np.array([1.0, 0.5])
    o3 = [np.ascontiguousarray(v) for v in obs]

    e = G.Engine(2 * n, 3 * m)
    with pytest.raises(ValueError):
        e.set_cells_mvi_data(b6, C.direction(), ("bz", "bz"), w, translation_invariant=True)
    e.close()
    e = G.Engine(16386, 3)
    e.set_cells_mvi_data(np.array([[0, 1, 0, 1, 0, 1.0]]), C.direction(), data, w, translation_invariant=True)  # (no row limit)
    e.close()

    # a geometry without the structure: the detection's reason, from build_G
    o2, c2 = c2_linspace()
    e = G.Engine(2 * o2.shape[1], 3 * c2.shape[0])
    e.set_cells_mvi_data(c2, C.direction(), data, w, translation_invariant=True)
    e.set_obs(*[np.ascontiguousarray(v) for v in o2])
    with pytest.raises(NotImplementedError, match="spacing") as err:
        e.build_G()
    assert "translation-invariant" in str(err.value)
    e.close()

    # the other doors stay shut, in either order; the table asked for with the cells cannot be taken away
    for first in (G.Engine.set_cells_mvi, G.Engine.set_cells_mvi_data):
        e = G.Engine(n if first is G.Engine.set_cells_mvi else 2 * n, 3 * m)
        first(e, b6, C.direction(), *(() if first is G.Engine.set_cells_mvi else (data, w)))
        with pytest.raises(NotImplementedError, match="gh_set_translation_invariant: not supported on"):
            e.set_translation_invariant(True)
        e.close()
        e = G.Engine(2 * n, 3 * m)
        e.set_translation_invariant(True)
        with pytest.raises(NotImplementedError):
            first(e, b6, C.direction(), *(() if first is G.Engine.set_cells_mvi else (data, w)))
        e.close()
    e = G.Engine(2 * n, 3 * m)
    e.set_cells_mvi_data(b6, C.direction(), data, w, translation_invariant=True)
    for on in (True, "chains", "replicates", False):
        with pytest.raises(NotImplementedError, match=VSTORE) as err:
            e.set_translation_invariant(on)
        assert "translation-invariant" in str(err.value)
    for call in (e.set_matrix_free, e.set_shift_invariant):
        with pytest.raises(NotImplementedError, match=VSTORE) as err:
            call(True)
        assert TABLE in str(err.value)
    e.close()

    # what does not run on the built store
    eng = C.mvi_engine(G, obs, b6, data, w, True)
    wm = eng.weight(0.5)
    with pytest.raises(NotImplementedError, match=VSTORE) as err:
        eng.set_data(np.zeros(2 * n), np.zeros(2 * n))            # grav_fix
    assert TABLE in str(err.value)
    eng.set_data(np.zeros(2 * n))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, m), 0.0 * wm)
    x0 = np.stack([0.01 * wm, 0.02 * wm])
    for what, call in (("wavelet", lambda: eng.compress_wavelet(1, (1, 1, 3 * m), 0.001, 2)),
                       ("batch_init", lambda: eng.batch_init(x0, 0.0 * wm, 1.0 * wm)),
                       ("upload", lambda: eng.upload_G(np.zeros((2 * n, 3 * m)))),
                       ("bscg", lambda: eng.bscg_run(np.ones((2, 2 * n)), np.zeros(2 * n), 0.01 * wm, 0.0, 1.0, 0.0, 2, 4))):
        with pytest.raises(NotImplementedError, match=VSTORE) as err:
            call()
        assert TABLE in str(err.value), what
    lib = _lib.load()
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 6 * m), (lib.gh_shard_init_rows, 4 * n)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        text = lib.gh_last_error(eng._h)
        assert rc == _lib.GH_ERR_UNSUPPORTED and VSTORE.encode() in text and TABLE.encode() in text
    with pytest.raises(ValueError):
        eng.download_G()
    # the results of the cells work as on the dense context
    mag = np.random.default_rng(2).normal(size=(m, 3))
    dense = C.mvi_engine(G, obs, b6, data, w, False)
    assert np.array_equal(eng.b_result("bz", mag), dense.b_result("bz", mag))
    for e in (eng, dense):
        e.close()
    one, dense = C.mvi_engine(G, obs, b6, ("tf",), np.ones(1), True), C.mvi_engine(G, obs, b6, ("tf",), None, False, dense_mvi=True)
    assert np.array_equal(one.tf_result(mag), dense.tf_result(mag))
    # every other context's dictionary stays what it is
    assert "axes" not in dense.translation_invariant_info()
    for e in (one, dense):
        e.close()
