"""GPU suite (`-m gpu`): the multi-component store on the translation-invariant table (gh_set_cells_multi_table,
csrc/lattice.hip.h: the row blocks; host_lattice.h) -- C gravity components of one regular prism grid under gridded
data, one table T[b][k][u][v] per component, no limit on the stacked rows.

  1. the block tables bit for bit: the dense multi-component store's entries of the representative pairs, and the
     single-component table engines' tables;
  2. weights, forward and adjoint at the blocks' edges (lattice_multi_cases: px = 1, 4, 5; TR = 4 under px = 5; R-1,
     R+1; a row across 64 lanes) with C = 1, 2, 3 and 11 blocks of distinct data weights, against multicomp_host.stack
     on the dense store's unweighted blocks;
  3. potential and chain against multicomp_host.MultiProblem, the four regularisers; piped run_chain, stateless
     leapfrog and a second engine bit for bit; the dense multi-component engine to 1e-10;
  4. beyond 16384 stacked rows: the per-block epilogue against single-component dense engines;
  5. C = 1 with weight 1 against the single-component table engine; one block of gz at weight 1 against the scalar gz
     table bit for bit: table, weights, forward, adjoint (the gathers and column norms are written once, for n blocks);
  6. MultiComponentModule(translation_invariant=True) against the dense module, HMCSample with the posterior stream;
  7. the module past the dense form's limit (2 x 100 x 100 rows) against GravMagModule(translation_invariant=True);
  8. refusals.
Bounds: the table bit for bit; wm 1e-11, forward / adjoint / potential / chain 1e-10 (the project's bounds for these
quantities, tests/test_gpu_lattice.py); C = 1 against the single-component engine 1e-12 (tests/test_gpu_multicomp.py's
bound for the dense pair); the module's potential 1e-12 on the value and 1e-11 on the gradient (the single-block module
test)."""
import numpy as np
import pytest

from helpers import relmax
from lattice_cases import c2_linspace, detect
from lattice_multi_cases import (ALL_COMPONENTS, ALL_WEIGHTS, CHAIN_SHAPES, EDGE_SHAPES, SHAPES, TABLE_SHAPES, TableOperator,
                                 multi_engine, shape, single_engine, table_problem)
from multicomp_host import MultiProblem, stack, std_weights

pytestmark = pytest.mark.gpu

REGS = ("Damping", "MS", "Smoothness", "TV")
STORE, TABLE = "multi-component store", "translation-invariant"


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


_BLOCKS = {}


def dense_blocks(G, name, comps):
    """obs, bounds6 and the unweighted blocks of the dense multi-component store (download_G before weight) of a shape:
    computed once per (shape, components), shared, left unchanged"""
    key = (name, tuple(comps))
    if key not in _BLOCKS:
        obs, b6 = shape(name)
        n = obs.shape[1]
        eng = multi_engine(G, obs, b6, comps, np.ones(len(comps)), False)
        A = np.array(eng.download_G())
        eng.close()
        K = [np.ascontiguousarray(A[b * n:(b + 1) * n]) for b in range(len(comps))]
        for a in [obs, b6] + K:
            a.setflags(write=False)
        _BLOCKS[key] = (obs, b6, K)
    return _BLOCKS[key]


def representative(obs, b6):
    """(observation, cell) of the pair with the smallest (p, q) of every offset: arrays of a block table's shape"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    k, u, v = np.meshgrid(np.arange(nz), np.arange(nx + px - 1), np.arange(ny + qy - 1), indexing="ij")
    du, dv = u - (nx - 1), v - (ny - 1)
    p, q = np.maximum(du, 0), np.maximum(dv, 0)
    return ool[p * qy + q], col[(k * nx + (p - du)) * ny + (q - dv)]


# ------------------------------------------------------------------------------------------ 1. the table

@pytest.mark.parametrize("name", TABLE_SHAPES)
def test_block_tables_are_the_dense_stores_entries_and_the_single_tables(G, name):
    comps = ("gz", "gzz", "gxy")
    obs, b6, K = dense_blocks(G, name, comps)
    nx, ny, nz = SHAPES[name]["cells"]
    px, qy = SHAPES[name]["obs"]
    lat = multi_engine(G, obs, b6, comps, (2.0, 1.0, 0.125), True)
    info = lat.translation_invariant_info()
    T = lat.translation_invariant_table()
    assert info["on"] and (info["nx"], info["ny"], info["nz"], info["px"], info["qy"]) == (nx, ny, nz, px, qy)
    assert T.shape == (3, nz, nx + px - 1, ny + qy - 1) and info["table_bytes"] == T.size * 8
    i, j = representative(obs, b6)
    for b, c in enumerate(comps):
        assert np.array_equal(T[b], K[b][i, j]), c          # (the weights are not in the table)
        one = single_engine(G, obs, b6, c, True)
        assert np.array_equal(T[b], one.translation_invariant_table()), c
        one.close()
    print(name, "max_dev", info["max_dev"])
    assert info["max_dev"] <= 1e-12
    with pytest.raises(ValueError):
        lat.download_G()
    lat.close()


# --------------------------------------------------------------------------- 2. the operator at the block edges

@pytest.mark.parametrize("C", [1, 2, 3, 11])
@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_weights_forward_adjoint_at_the_block_edges(G, name, C):
    comps, w = ALL_COMPONENTS[:C], np.array(ALL_WEIGHTS[:C])
    obs, b6, K = dense_blocks(G, name, comps)
    n, M = K[0].shape
    Aw, wm_o, _ = stack(K, w)
    eng = multi_engine(G, obs, b6, comps, w, True)
    wm = eng.weight(0.5)
    rng = np.random.default_rng(11)
    x, r = rng.uniform(-1, 1, M) * wm_o, rng.normal(size=C * n)
    fw, ad = eng.forward(x), eng.adjoint(r)
    fo, ao = Aw @ x, Aw.T @ r
    # (the forward block by block: a missing or swapped w_b of a block of small entries would hide under the largest)
    ef = max(relmax(fw[b * n:(b + 1) * n], fo[b * n:(b + 1) * n]) for b in range(C))
    print(name, "C", C, "weights", relmax(wm, wm_o), "forward", ef, "adjoint", relmax(ad, ao))
    assert relmax(wm, wm_o) <= 1e-11
    assert ef <= 1e-10 and relmax(ad, ao) <= 1e-10
    info = eng.multi_info()
    assert len(info["components"]) == C and np.array_equal(info["weights"], w)
    eng.close()


# ------------------------------------------------------------------------------------ 3. potential and chain

#: Step sizes chosen on the CPU with MultiProblem alone, on kernels of the three fields evaluated there (chain_problem
#: below with them): the shapes differ in stiffness, so each has its own per regulariser.  At every one the ten
#: trajectories are accepted in part and rejected in part and an accepted state lies on a bound; the closest Metropolis
#: decision is |log u + dH| >= 1.3e-2 away.  (accepted of ten)
DT = {"beyond": {"Damping": 0.4, "MS": 0.02, "Smoothness": 0.25, "TV": 0.15},                          # 9, 7, 7, 7
      "shuffled": {"Damping": 0.5, "MS": 0.02, "Smoothness": 0.4, "TV": 0.25},                         # 1, 9, 5, 5
      "covered row across 64 lanes": {"Damping": 0.25, "MS": 0.008, "Smoothness": 0.25, "TV": 0.15}}   # 7, 9, 4, 4
CHAIN_COMPS = ("gz", "gzz", "gxy")


def chain_problem(K, name, reg):
    """The chain test's problem from the unweighted blocks K of CHAIN_COMPS on a shape: (Aw, wm, w, dobsw, shape3, the
    MultiProblem, low, high, the ten trajectories, a test point)"""
    n, M = K[0].shape
    nx, ny, nz = SHAPES[name]["cells"]
    shape3 = (1, 1, M) if "shuffle" in SHAPES[name] else (nz, nx, ny)  # (stencils follow the caller's cell order)
    rng = np.random.default_rng(7)
    rho = np.zeros(M)
    rho[rng.choice(M, max(1, M // 10), replace=False)] = 0.03
    dobs = []
    for Kb in K:
        d = Kb @ rho
        dobs.append(d + 1e-3 * np.abs(d).max() * rng.normal(size=n))
    w = std_weights(dobs)
    Aw, wm, wb = stack(K, w)
    dobsw = wb * np.concatenate(dobs)
    P = MultiProblem(Aw, dobsw, len(K), 0.001 * wm, reg, 1.0, 0.01, wm=wm, shape=shape3)
    low, high = 0.0 * wm, 0.05 * wm
    trajs = [(L, rng.normal(size=M) * 0.02 * wm, float(rng.uniform())) for L in (2, 3, 4, 5, 6, 2, 3, 4, 5, 6)]
    xt = rng.uniform(0, 0.05, M) * wm
    return Aw, wm, w, dobsw, shape3, P, low, high, trajs, xt


def _setup(eng, reg, shape3, dobsw, wm):
    eng.set_data(dobsw)
    eng.set_reg(reg, 1.0, 0.01, shape3, 0.001 * wm)


@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("name", CHAIN_SHAPES)
def test_potential_and_chain_against_the_restatement_and_bitwise_paths(G, monkeypatch, name, reg):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    obs, b6, K = dense_blocks(G, name, CHAIN_COMPS)
    Aw, wm_o, w, dobsw, shape3, P, low, high, trajs, xt = chain_problem(K, name, reg)
    eng = multi_engine(G, obs, b6, CHAIN_COMPS, w, True)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    _setup(eng, reg, shape3, dobsw, wm_o)
    dt = DT[name][reg]

    out, ref = eng.misfit_and_grad(xt), P.misfit_and_grad(xt)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10
    assert relmax(out[2], ref[2]) <= 1e-10
    info = eng.multi_info()
    assert relmax(info["pred_mean"], P.pred_mean) <= 1e-10 and relmax(info["obs_mean"], P.obs_mean) <= 1e-10

    # trajectory by trajectory against the restatement
    x0 = 0.001 * wm_o
    eng.chain_init(x0, low, high)
    plain, clamps = [], 0
    xo = x0
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        x = eng.chain_get_x()
        plain.append((acc, o.copy(), x))
        xo, acco, oo = P.leapfrog(xo, p0, dt, L, low, high, u)
        assert bool(acc) == bool(acco)
        assert relmax(o, oo) <= 1e-10 and relmax(x, xo) <= 1e-10
        clamps += int(acc and (np.any(x == low) or np.any(x == high)))
    accepted = sum(bool(a) for a, _, _ in plain)
    print(name, reg, "accepted", accepted, "of", len(plain), "accepted states on a bound", clamps)
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

    # a second engine: the same bits; the dense multi-component engine (its weighting lies in the store): 1e-10
    eng2 = multi_engine(G, obs, b6, CHAIN_COMPS, w, True)
    assert np.array_equal(eng2.weight(0.5), wm)
    assert np.array_equal(eng2.translation_invariant_table(), eng.translation_invariant_table())
    dense = multi_engine(G, obs, b6, CHAIN_COMPS, w, False)
    assert relmax(dense.weight(0.5), wm) <= 1e-11
    for e in (eng2, dense):
        _setup(e, reg, shape3, dobsw, wm_o)
        e.chain_init(x0, low, high)
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        acc2, o2 = eng2.chain_trajectory(p0, dt, L, u)
        assert acc2 == acc and np.array_equal(o2, o) and np.array_equal(eng2.chain_get_x(), xs)
        acc3, o3 = dense.chain_trajectory(p0, dt, L, u)
        assert bool(acc3) == bool(acc) and relmax(o3, o) <= 1e-10 and relmax(dense.chain_get_x(), xs) <= 1e-10
    for e in (eng, eng2, dense):
        e.close()


# ---------------------------------------------------------------------------- 4. beyond 16384 stacked rows

H7 = 2000.0 / 7
BEYOND = {"3 x 75x75 over 4x4x1": (("gz", "gzz", "gxy"), dict(cells=(4, 4, 1), obs=(75, 75), first=(-35, -35), h=(H7, H7),
                                                             origin=(317.3, -911.7))),
          "2 x 130x513 over 2x2x5: layers per chunk": (("gz", "gzz"), dict(cells=(2, 2, 5), obs=(130, 513),
                                                                          first=(-64, -255)))}


@pytest.mark.parametrize("case", sorted(BEYOND))
def test_more_than_16384_stacked_rows(G, case):
    from lattice_cases import geometry
    comps, kw = BEYOND[case]
    obs, b6 = geometry(**kw)
    n, M, C = obs.shape[1], b6.shape[0], len(comps)
    assert C * n > 16384 and (n <= 16384 or C == 2)
    # the reference kernels block by block, from single-component DENSE engines
    K = []
    for c in comps:
        one = single_engine(G, obs, b6, c, False)
        K.append(np.array(one.download_G()))
        one.close()
    w = np.array(ALL_WEIGHTS[:C])
    Aw, wm_o, wb = stack(K, w)
    eng = multi_engine(G, obs, b6, comps, w, True)
    print(case, "max_dev", eng.translation_invariant_info()["max_dev"])
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    rng = np.random.default_rng(12)
    x, r = rng.uniform(-1, 1, M) * wm_o, rng.normal(size=C * n)
    fw, fo = eng.forward(x), Aw @ x
    assert max(relmax(fw[b * n:(b + 1) * n], fo[b * n:(b + 1) * n]) for b in range(C)) <= 1e-10
    assert relmax(eng.adjoint(r), Aw.T @ r) <= 1e-10
    # the per-block epilogue beyond 16384 rows: misfit, gradient and the blocks' means
    dobsw = Aw @ (0.02 * wm_o) + 0.01 * rng.normal(size=C * n) + np.repeat(np.arange(1.0, C + 1), n)
    eng.set_data(dobsw)
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm_o)
    P = MultiProblem(Aw, dobsw, C, 0.001 * wm_o, "Damping", 1.0, 0.01, wm=wm_o, shape=(1, 1, M))
    out, ref = eng.misfit_and_grad(0.03 * wm_o), P.misfit_and_grad(0.03 * wm_o)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10 and relmax(out[2], ref[2]) <= 1e-10
    info = eng.multi_info()
    print(case, "means", info["pred_mean"], P.pred_mean)
    assert relmax(info["pred_mean"], P.pred_mean) <= 1e-10 and relmax(info["obs_mean"], P.obs_mean) <= 1e-10
    eng.close()


# -------------------------------------------------------------------------------------- 5. C = 1, weight 1

@pytest.mark.parametrize("comp", ["gz", "gzz"])
def test_one_block_of_weight_one_is_the_single_component_table_engine(G, monkeypatch, comp):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    obs, b6 = shape("beyond")
    nx, ny, nz = SHAPES["beyond"]["cells"]
    n, M = obs.shape[1], b6.shape[0]
    mc, one = multi_engine(G, obs, b6, (comp,), (1.0,), True), single_engine(G, obs, b6, comp, True)
    assert np.array_equal(mc.translation_invariant_table()[0], one.translation_invariant_table())
    wm = one.weight(0.5)
    assert relmax(mc.weight(0.5), wm) <= 1e-12
    rng = np.random.default_rng(5)
    x, r = rng.uniform(-1, 1, M) * wm, rng.normal(size=n)
    assert relmax(mc.forward(x), one.forward(x)) <= 1e-12 and relmax(mc.adjoint(r), one.adjoint(r)) <= 1e-12
    rho = np.zeros(M)
    rho[rng.choice(M, M // 10, replace=False)] = 0.03
    d0 = one.forward(wm * rho)
    dobs = d0 + 1e-3 * np.abs(d0).max() * rng.normal(size=n)
    low, high = 0.0 * wm, 0.05 * wm
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.02 * wm, float(rng.uniform())) for _ in range(5)]
    outs = []
    for e in (mc, one):
        e.set_data(dobs)
        e.set_reg("TV", 1.0, 0.01, (nz, nx, ny), 0.001 * wm)
    xt = rng.uniform(0, 0.05, M) * wm
    a, b = mc.misfit_and_grad(xt), one.misfit_and_grad(xt)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-12 and relmax(a[2], b[2]) <= 1e-12
    for e in (mc, one):
        e.chain_init(0.001 * wm, low, high)
        res = []
        for L, p0, u in trajs:
            acc, o = e.chain_trajectory(p0, 0.02, L, u)
            res.append((acc, o.copy(), e.chain_get_x()))
        outs.append(res)
    for (a1, o1, x1), (a2, o2, x2) in zip(*outs):
        assert bool(a1) == bool(a2) and relmax(o1, o2) <= 1e-12 and relmax(x1, x2) <= 1e-12
    mc.close()
    one.close()


#: 5 x 7 x 2 under 6 x 9: qy and ny no multiples of 8, N = 54 far below a workgroup; 9 x 11 x 2 under 17 x 19: N = 323
#: reaches the gather's second workgroup with a ragged tail
UNIT_BLOCK_SHAPES = {"54 points": dict(cells=(5, 7, 2), obs=(6, 9)), "323 points": dict(cells=(9, 11, 2), obs=(17, 19))}


@pytest.mark.parametrize("name", sorted(UNIT_BLOCK_SHAPES))
def test_single_block_of_unit_weight_is_the_scalar_table(G, name):
    """One row block of gz at weight 1.0 is the scalar gz table, bit for bit: 1.0 * r == r in the gather of r, and
    0.0 + (1.0 * 1.0) * s == s in the column norms, contracted to an FMA or not.  The table's gathers and column norms
    are written once, for n blocks, on this property."""
    from gravinv3dhmc_amd import _lib
    from lattice_cases import geometry
    obs, b6 = geometry(**UNIT_BLOCK_SHAPES[name])
    n, M = obs.shape[1], b6.shape[0]
    one = G.Engine(n, M)
    one.set_translation_invariant(True)
    one.set_obs(*[np.ascontiguousarray(v) for v in obs])
    one.set_cells(b6, _lib.CELL_PRISM)
    one.build_G()
    mc = multi_engine(G, obs, b6, ("gz",), (1.0,), True)
    assert one.translation_invariant_info()["on"] and mc.translation_invariant_info()["on"]
    assert np.array_equal(mc.translation_invariant_table()[0], one.translation_invariant_table())
    wm = one.weight(0.5)
    assert np.array_equal(mc.weight(0.5), wm)
    rng = np.random.default_rng(17)
    x, r = rng.uniform(-1, 1, M) * wm, rng.normal(size=n)
    assert np.array_equal(mc.forward(x), one.forward(x))
    assert np.array_equal(mc.adjoint(r), one.adjoint(r))
    mc.close()
    one.close()


# ------------------------------------------------------------------------------------------ 6. the module

MODULE = dict(mrange=(0.0, 7 * 150.0, 0.0, 5 * 150.0, 0.0, 450.0), mspacing=(150.0, 150.0, 150.0))
MODULE_COMPS = ("gz", "gzz", "gxx")


def _centres(G, mrange, mspacing, height=-20.0):
    """gridded data above the cell centres of the module's own mesh, whatever axis it calls x: (x, y, z), bounds6"""
    b6 = G.mesher.PrismMesh(mrange, mspacing).cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    return (xp, yp, np.full(xp.size, height)), np.ascontiguousarray(b6)


def _sample(G, mod, M, tag):
    """a few draws of HMCSample with a fixed seed (posterior stream on): the accepted rows of the 8-digit text sink"""
    folder = "%s_chain" % tag
    G.HMCSample(mod, 6, 2, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, 0.0), np.full(M, 0.02)],
                "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3, nbest=100, myrank=0,
                save_folder=folder, posterior_stream=True)
    return np.atleast_2d(np.loadtxt(folder + "0/model.dat"))


def test_module_matches_the_dense_module(G, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n, M = obs[0].size, b6.shape[0]
    rng = np.random.default_rng(21)

    def make(dobs, ti):
        return G.MultiComponentModule(dobs, MODULE["mrange"], MODULE["mspacing"], obs, components=MODULE_COMPS,
                                      weights="std", verbose=False, translation_invariant=ti)

    # data of a block of anomalous cells, from the dense module's own kernels, plus noise
    probe = make([rng.normal(size=n) for _ in MODULE_COMPS], False)
    rho = np.zeros(M)
    rho[M // 3:M // 3 + M // 8] = 0.015
    d = probe.forward(rho)
    probe._engine.close()
    dobs = [d[c * n:(c + 1) * n] + 0.01 * np.abs(d[c * n:(c + 1) * n]).max() * rng.normal(size=n) for c in range(3)]
    lat, dense = make(dobs, True), make(dobs, False)
    info = lat.translation_invariant_info()
    assert info["on"] and info["nx"] * info["ny"] * info["nz"] == M and lat.translation_invariant
    assert info["table_bytes"] == lat._engine.translation_invariant_table().size * 8
    assert not dense.translation_invariant and not dense._engine.translation_invariant_info()["on"]
    wm = dense.Wm.diagonal()
    assert relmax(lat.Wm.diagonal(), wm) <= 1e-11
    assert np.array_equal(lat.weights, dense.weights)
    assert relmax(lat.Wb.diagonal(), dense.Wb.diagonal()) <= 1e-10 and relmax(lat.dobsw, dense.dobsw) <= 1e-10
    x = rng.uniform(0, 1, M) * wm
    for reg in REGS:
        a = lat.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, 0.001 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        print(reg, abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]))
        assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-11
        assert relmax(lat.block_means()[0], dense.block_means()[0]) <= 1e-10
    model = rng.uniform(0, 0.02, M)
    fl, fd = lat.forward(model), dense.forward(model)
    assert max(relmax(fl[c * n:(c + 1) * n], fd[c * n:(c + 1) * n]) for c in range(3)) <= 1e-10
    for what in (lambda: lat.Aw, lambda: lat.A, lambda: lat.kernel("gzz")):
        with pytest.raises(NotImplementedError, match=STORE) as e:
            what()
        assert TABLE in str(e.value)
    rows = [_sample(G, mod, M, tag) for tag, mod in (("lat", lat), ("dense", dense))]
    capsys.readouterr()
    assert rows[0].shape == rows[1].shape and rows[0].shape[1] == M and rows[0].shape[0] > 0
    # (1e-8: one unit of the text sink's last digit, as the difference of two printed numbers comes out in binary)
    assert np.abs(rows[0] - rows[1]).max() <= 1e-8 * (1 + 1e-6)
    lat._engine.close()
    dense._engine.close()


# ------------------------------------------------------------------------------ 7. the module past the limit

def test_module_beyond_the_dense_forms_limit(G):
    mrange, mspacing = (0.0, 10000.0, 0.0, 10000.0, 0.0, 100.0), (100.0, 100.0, 100.0)
    comps = ("gz", "gzz")
    obs, b6 = _centres(G, mrange, mspacing, -50.0)
    n, M = obs[0].size, b6.shape[0]
    assert n == 10000 and M == 10000
    rng = np.random.default_rng(31)
    dobs = [rng.normal(size=n), 40.0 * rng.normal(size=n)]
    with pytest.raises(NotImplementedError, match="16384") as e:
        G.MultiComponentModule(dobs, mrange, mspacing, obs, components=comps, verbose=False)
    assert "translation_invariant" in str(e.value)
    mc = G.MultiComponentModule(dobs, mrange, mspacing, obs, components=comps, verbose=False, translation_invariant=True)
    assert mc._engine.N == 2 * n and mc.translation_invariant_info()["on"]
    model = np.zeros(M)
    model[rng.choice(M, 200, replace=False)] = 0.02
    fwd = mc.forward(model)
    tables = []
    for c, name in enumerate(comps):
        gm = G.GravMagModule(dobs[c], mrange, mspacing, obs, component=name, verbose=False, translation_invariant=True)
        one = gm._engine.forward(model * gm.Wm.diagonal())
        print(name, "forward against GravMagModule(translation_invariant=True)", relmax(fwd[c * n:(c + 1) * n], one))
        assert relmax(fwd[c * n:(c + 1) * n], one) <= 1e-10
        tables.append(gm._engine.translation_invariant_table())
        gm._engine.close()
    # misfit_and_grad against the restatement on those two engines' kernels: their tables, expanded on the host as an
    # operator (the stack is 20000 x 10000: never formed)
    rc, dims, _, col, _, ool = detect(np.stack(obs), b6)
    assert rc == 0
    op = TableOperator(tables, mc.weights, dims, col, ool)
    wm = mc.Wm.diagonal()
    assert relmax(wm, op.wm) <= 1e-11
    x, mwapr = rng.uniform(0, 0.02, M) * wm, 0.001 * wm
    P = table_problem(op, mc.dobsw, 2, mwapr, "Damping", 0.7, 0.001, wm)
    a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization="Damping", beta=0.001)
    b = P.misfit_and_grad(x)
    print("value", abs(a[0] - b[0]) / abs(b[0]), "grad", relmax(a[1], b[1]), "dpre", relmax(a[2], b[2]))
    assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-10 and relmax(a[2], b[2]) <= 1e-10
    pm, om = mc.block_means()
    assert relmax(pm, P.pred_mean) <= 1e-10 and relmax(om, P.obs_mean) <= 1e-10
    mc._engine.close()


# ---------------------------------------------------------------------------------------------- 8. refusals

def test_engine_refusals_name_the_store(G):
    from gravinv3dhmc_amd import _lib
    obs, b6 = shape("beyond")
    n, M = obs.shape[1], b6.shape[0]
    comps, w = ("gz", "gzz"), np.array([1.0, 0.5])
    o3 = [np.ascontiguousarray(v) for v in obs]

    # the checks of gh_set_cells_multi, but the row limit
    e = G.Engine(2 * n, M)
    with pytest.raises(ValueError):
        e.set_cells_multi(b6, ("gz", "gz"), w, translation_invariant=True)
    with pytest.raises(ValueError):
        e.set_cells_multi(b6, comps, (1.0, 0.0), translation_invariant=True)
    with pytest.raises(ValueError):
        e.set_cells_multi(b6, ("gz", "gzz", "gxx", "gxy", "gyy"), np.ones(5), translation_invariant=True)  # 144 rows
    e.set_obs(*[np.tile(v, 2) for v in o3])
    with pytest.raises(ValueError, match="fresh context"):
        e.set_cells_multi(b6, comps, w, translation_invariant=True)
    e.close()
    e = G.Engine(16386, 1)
    e.set_cells_multi(np.array([[0, 1, 0, 1, 0, 1.0]]), comps, w, translation_invariant=True)   # (no row limit)
    e.close()

    # a geometry without the structure: the detection's reason, from build_G
    o2, c2 = c2_linspace()
    e = G.Engine(2 * o2.shape[1], c2.shape[0])
    e.set_cells_multi(c2, comps, w, translation_invariant=True)
    e.set_obs(*[np.ascontiguousarray(v) for v in o2])
    with pytest.raises(NotImplementedError, match="spacing") as err:
        e.build_G()
    assert TABLE in str(err.value)
    e.close()

    # the two pinned call sequences still refuse; the table asked for with the cells cannot be taken away
    e = G.Engine(2 * n, M)
    e.set_cells_multi(b6, comps, w)
    with pytest.raises(NotImplementedError, match="gh_set_translation_invariant: not supported on"):
        e.set_translation_invariant(True)
    e.close()
    e = G.Engine(2 * n, M)
    e.set_translation_invariant(True)
    with pytest.raises(NotImplementedError):
        e.set_cells_multi(b6, comps, w)
    e.close()
    e = G.Engine(2 * n, M)
    e.set_cells_multi(b6, comps, w, translation_invariant=True)
    for on in (True, False):
        with pytest.raises(NotImplementedError, match=STORE):
            e.set_translation_invariant(on)
    for call in (e.set_matrix_free, e.set_shift_invariant):
        with pytest.raises(NotImplementedError, match=STORE) as err:
            call(True)
        assert TABLE in str(err.value)
    e.close()

    # what does not run on the built store
    eng = multi_engine(G, obs, b6, comps, w, True)
    wm = eng.weight(0.5)
    with pytest.raises(ValueError, match=STORE):
        eng.set_data(np.zeros(2 * n), np.zeros(2 * n))            # grav_fix
    eng.set_data(np.zeros(2 * n))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    x0 = np.stack([0.01 * wm, 0.02 * wm])
    for what, call in (("wavelet", lambda: eng.compress_wavelet(1, (1, 1, M), 0.001, 2)),
                       ("batch_init", lambda: eng.batch_init(x0, 0.0 * wm, 1.0 * wm)),
                       ("upload", lambda: eng.upload_G(np.zeros((2 * n, M)))),
                       ("bscg", lambda: eng.bscg_run(np.ones((2, 2 * n)), np.zeros(2 * n), 0.01 * wm, 0.0, 1.0, 0.0, 2, 4))):
        with pytest.raises(NotImplementedError, match=STORE):
            call()
        print("refused:", what)
    lib = _lib.load()
    import ctypes
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 2 * M), (lib.gh_shard_init_rows, 4 * n)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        assert rc == _lib.GH_ERR_UNSUPPORTED and STORE.encode() in lib.gh_last_error(eng._h)
    with pytest.raises(ValueError):
        eng.download_G()
    assert not eng.fold_info()["on"] and eng.chain_stats()["resident_launches"] == 0
    eng.close()

    # translation_invariant=False: the dense store, bit for bit what it was
    a = G.Engine(2 * n, M)
    a.set_cells_multi(b6, comps, w, translation_invariant=False)
    b = G.Engine(2 * n, M)
    b.set_cells_multi(b6, comps, w)
    for e in (a, b):
        e.set_obs(*o3)
        e.build_G()
    assert not a.translation_invariant_info()["on"]
    assert np.array_equal(np.asarray(a.download_G()), np.asarray(b.download_G()))
    a.close()
    b.close()


def test_module_refusals_name_the_store_and_the_table(G):
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n, M = obs[0].size, b6.shape[0]
    rng = np.random.default_rng(3)
    dobs = [rng.normal(size=n) for _ in MODULE_COMPS]

    def make(**kw):
        return G.MultiComponentModule(dobs, MODULE["mrange"], MODULE["mspacing"], obs, components=MODULE_COMPS,
                                      verbose=False, translation_invariant=True, **kw)

    for kw in (dict(wavelet="1D"), dict(shard=object()), dict(matrix_free=True), dict(shift_invariant=True),
               dict(mtopo=obs), dict(coordinate="spherical")):
        with pytest.raises(NotImplementedError, match=STORE) as e:
            make(**kw)
        assert TABLE in str(e.value)
    # the linspace grid (n points from one end of the mesh to the other): the detection's reason
    yl, xl = [a.ravel() for a in np.meshgrid(np.linspace(0, 150.0 * 5, 5), np.linspace(0, 150.0 * 7, 7))]
    with pytest.raises(NotImplementedError, match="spacing") as e:
        G.MultiComponentModule([rng.normal(size=xl.size) for _ in MODULE_COMPS], MODULE["mrange"], MODULE["mspacing"],
                               (xl, yl, np.zeros_like(xl)), components=MODULE_COMPS, verbose=False,
                               translation_invariant=True)
    assert TABLE in str(e.value)
    mod = make()
    with pytest.raises(NotImplementedError, match=STORE):
        G.HMCSampleBatch(mod, 2, 2, 1, 0.01, [2, 3], np.full(M, 0.001), np.full(M, 0.001),
                         np.c_[np.zeros(M), np.full(M, 0.02)], "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "TV",
                         0.001, 5, 0.3)
    mod._engine.close()
