"""GPU suite (`-m gpu`): chain batches on the multi-component translation-invariant table (csrc/latbatch.hip.h: the forms
over row blocks; batch.hip.h: batch_finish_blocks_kernel; Engine.set_cells_multi(..., translation_invariant="chains")).

The reference is multicomp_host.MultiProblem -- the stacked weighted kernel with one mean per block -- on the tables the
engine under test keeps, expanded on the host (the tables themselves are pinned to the dense store's entries by
test_gpu_lattice_multi.py); test_lattice_multi_batch_host.py checks on the CPU that the restated block passes are that
kernel's products, that a wrong model (one global mean, swapped weights, a dropped block) is 1e-6 or more away, and that
the chains' trajectories keep a Metropolis margin of 1e-3.  Bound: 1e-10 relative, the project's for table chains;
decisions identical.  Each case first reads the plan back and compares it with the restated one."""
import numpy as np
import pytest

from helpers import relmax
import lattice_batch_cases as lb
import lattice_multi_batch_cases as mb
from multicomp_host import MultiProblem, stack
from test_gpu_lattice_batch import MODULE, compare_carry, compare_with_oracle, run_carry, run_rounds

pytestmark = pytest.mark.gpu

STORE = "translation-invariant store"


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def multi_engine(G, obs, b6, comps, weights, table):
    eng = G.Engine(len(comps) * obs.shape[1], b6.shape[0])
    eng.set_cells_multi(b6, comps, np.asarray(weights, dtype=float), translation_invariant=table)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    return eng


def check_plan(eng, dims, nb):
    plan = eng.translation_invariant_batch_plan()
    assert plan["on"] and plan["cus"] > 0
    assert plan == mb.plan(dims, plan["cus"], nb)
    return plan


def setup(eng, reg, shape, dobs, mwapr):
    eng.set_data(dobs)
    eng.set_reg(reg, 1.0, 0.01, shape, mwapr)


# ------------------------------------------------------------------------------------------------ 1. the passes

@pytest.mark.parametrize("name", sorted(mb.BLOCK_CASES) + ["BIG"])
def test_passes_at_the_blocks_edges(G, name):
    """One round of all 16 slots, L = 1 .. 3, Damping: the proposals' potentials are the block forward and the finish with
    one mean per block, the accepted states the block adjoint and the update, per chain."""
    C = 2 if name == "BIG" else mb.BLOCK_CASES[name]
    comps, w = mb.ALL_COMPONENTS[:C], np.array(mb.ALL_WEIGHTS[:C])
    obs, b6 = mb.geometry(**(mb.BIG if name == "BIG" else mb.PASS_CASES[name]))
    dims, col, ool = lb.lattice(obs, b6)
    eng = multi_engine(G, obs, b6, comps, w, "chains")
    plan = check_plan(eng, dims, C)
    assert plan["fits"]
    if name == "layers per chunk":
        assert plan["chunks"] < dims[2]
    T = eng.translation_invariant_table()
    wm = eng.weight(0.5)
    M = b6.shape[0]
    if name == "BIG":
        assert C * obs.shape[1] == 33800 > 16384
        A = mb.TableOperator(list(T), w, dims, col, ool)
        wm_o = A.wm
    else:
        A, wm_o, _ = stack([mb.expand(Tb, dims, col, ool) for Tb in T], w)
    assert relmax(wm, wm_o) <= 1e-11
    rnd = mb.pass_round(A, wm_o)
    if name == "BIG":
        P = mb.table_problem(A, rnd["dobs"], C, rnd["mwapr"], "Damping", 1.0, 0.01, wm_o, shape=(1, 1, M))
    else:
        P = MultiProblem(A, rnd["dobs"], C, rnd["mwapr"], "Damping", 1.0, 0.01, wm=wm_o, shape=(1, 1, M))
    ref, margin, n_acc = mb.pass_reference(P, rnd)
    print(name, "margin", margin, "accepted", n_acc)
    assert margin >= 1e-6 and n_acc > 0
    setup(eng, "Damping", (1, 1, M), rnd["dobs"], rnd["mwapr"])
    eng.batch_init(rnd["x0s"], rnd["low"], rnd["high"])
    acc, out5 = eng.batch_trajectory(rnd["p0s"], rnd["dt"], rnd["Ls"], rnd["us"])
    worst = 0.0
    for c in range(mb.CB):
        xo, acco, oo = ref[c]
        worst = max(worst, relmax(out5[c], oo), relmax(eng.batch_get_x(c), xo))
        assert bool(acc[c]) == bool(acco)
    print(name, "worst", worst)
    assert worst <= 1e-10
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the chains

@pytest.mark.parametrize("reg", mb.REGS)
@pytest.mark.parametrize("name", mb.CHAIN_CASES)
def test_chains_against_the_restatement_the_single_chain_table_and_bitwise_paths(G, name, reg):
    comps, w = mb.CHAIN_COMPONENTS, np.array(mb.CHAIN_WEIGHTS)
    obs, b6 = mb.geometry(**mb.PASS_CASES[name])
    dims, col, ool = lb.lattice(obs, b6)
    eng = multi_engine(G, obs, b6, comps, w, "chains")
    check_plan(eng, dims, 3)
    K = [mb.expand(Tb, dims, col, ool) for Tb in eng.translation_invariant_table()]
    # (the step sizes were chosen on the CPU with the suite's closed-form kernels: the same kernels)
    host = max(relmax(K[b], mb.prism_kernel(c, obs, b6)) for b, c in enumerate(comps))
    print(name, reg, "tables against the host kernels", host)
    assert host <= 1e-9
    Aw, wm_o, prob = mb.chain_setup(name, reg, K, w)
    P = mb.problem(Aw, prob, 3, reg, wm_o)
    ref, margin = mb.chains(P, prob, mb.CB)
    assert margin >= 1e-6
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    setup(eng, reg, prob["shape"], prob["dobs"], prob["mwapr"])

    # 16 chains, different L per chain: rounds in lock-step against the restatement
    rounds = run_rounds(eng, prob, mb.CB)
    worst = compare_with_oracle(rounds, ref, mb.CB)
    n_acc = sum(int(r[0].sum()) for r in rounds)
    print(name, reg, "16 chains vs restatement", worst, "accepted", n_acc, "of", mb.CB * 4)
    assert worst <= 1e-10 and 0 < n_acc < mb.CB * 4
    # the blocks' means of the final states
    pm = eng.batch_block_means()
    assert pm.shape == (mb.CB, 3)
    worst_m = 0.0
    for c in range(mb.CB):
        P.misfit_and_grad(rounds[-1][2][c])
        worst_m = max(worst_m, relmax(pm[c], P.pred_mean))
    print(name, reg, "block means", worst_m)
    assert worst_m <= 1e-10

    # each chain against the single-chain block table fed the same draws
    one = multi_engine(G, obs, b6, comps, w, True)
    assert np.array_equal(one.weight(0.5), wm)
    setup(one, reg, prob["shape"], prob["dobs"], prob["mwapr"])
    worst1 = 0.0
    for c in range(mb.CB):
        one.chain_init(prob["x0"], prob["low"], prob["high"])
        for t, (L, p0s, us) in enumerate(prob["rounds"]):
            a1, o1 = one.chain_trajectory(p0s[c], prob["dt"], L[c], float(us[c]))
            assert bool(a1) == bool(rounds[t][0][c])
            worst1 = max(worst1, relmax(rounds[t][1][c], o1), relmax(rounds[t][2][c], one.chain_get_x()))
    print(name, reg, "16 chains vs single-chain block table", worst1)
    assert worst1 <= 1e-10
    one.close()

    # a second engine: bit for bit
    eng2 = multi_engine(G, obs, b6, comps, w, "chains")
    assert np.array_equal(eng2.weight(0.5), wm)
    setup(eng2, reg, prob["shape"], prob["dobs"], prob["mwapr"])
    for (a1, o1, x1), (a2, o2, x2) in zip(rounds, run_rounds(eng2, prob, mb.CB)):
        assert np.array_equal(a1, a2) and np.array_equal(o1, o2) and np.array_equal(x1, x2)
    eng2.close()

    # gh_batch_run with carry-over against the rounds: bit for bit (accepted results carry their state)
    in_flight, got = run_carry(eng, prob, mb.CB)
    assert in_flight  # (different L per chain: a call leaves trajectories in flight)
    compare_carry(eng, got, rounds, mb.CB)

    # the first 1 and 5 chains run alone against the same chains among 16: bit for bit, on both paths
    for C in (1, 5):
        alone = run_rounds(eng, prob, C)
        for (a1, o1, x1), (a2, o2, x2) in zip(rounds, alone):
            assert np.array_equal(a1[:C], a2) and np.array_equal(o1[:C], o2) and np.array_equal(x1[:C], x2)
        assert np.array_equal(eng.batch_block_means(), pm[:C])
        _, got = run_carry(eng, prob, C)
        compare_carry(eng, got, rounds, C)
    # the single-chain calls still run on the context
    eng.chain_init(prob["x0"], prob["low"], prob["high"])
    eng.close()


# ------------------------------------------------------------------------------------------- 3. one block of weight 1

@pytest.mark.parametrize("comp", ["gz", "gzz"])
def test_one_block_of_weight_one_is_the_single_block_batch_bit_for_bit(G, comp):
    name, reg = "beyond", "TV"
    obs, b6 = mb.geometry(**mb.PASS_CASES[name])
    N, M = obs.shape[1], b6.shape[0]
    dims, _, _ = lb.lattice(obs, b6)
    single = G.Engine(N, M)
    single.set_translation_invariant("chains")
    single.set_obs(*[np.ascontiguousarray(v) for v in obs])
    if comp == "gz":
        single.set_cells(b6, 0)      # (gz is the prisms' own kind)
    else:
        single.set_cells(b6, 3, component=comp)
    single.build_G()
    multi = multi_engine(G, obs, b6, (comp,), (1.0,), "chains")
    assert np.array_equal(multi.translation_invariant_table()[0], single.translation_invariant_table())
    p1, pm = single.translation_invariant_batch_plan(), multi.translation_invariant_batch_plan()
    assert pm.pop("blocks") == 1 and pm == p1 == lb.plan(dims, p1["cus"])
    wm = single.weight(0.5)
    assert np.array_equal(multi.weight(0.5), wm)
    Aw, wm_h, _ = stack([mb.prism_kernel(comp, obs, b6)], (1.0,))
    prob = lb.chain_problem(name, reg, Aw, wm_h, seed=8)
    n_acc = 0
    for dt in (lb.DT[reg], 0.01, 0.001):
        prob["dt"] = dt
        for e in (single, multi):
            setup(e, reg, prob["shape"], prob["dobs"], prob["mwapr"])
        a, b = run_rounds(single, prob, mb.CB), run_rounds(multi, prob, mb.CB)
        for (a1, o1, x1), (a2, o2, x2) in zip(a, b):
            assert np.array_equal(a1, a2) and np.array_equal(o1, o2) and np.array_equal(x1, x2)
        n_acc += sum(int(r[0].sum()) for r in a)
        _, got = run_carry(multi, prob, mb.CB)
        compare_carry(multi, got, a, mb.CB)
    print(comp, "accepted", n_acc, "of", 3 * mb.CB * 4)
    assert 0 < n_acc < 3 * mb.CB * 4
    single.close()
    multi.close()


# ------------------------------------------------------------------------------------------------ 4. the module

def test_hmcsample_batch_on_the_block_tables_with_the_posterior_stream(G, tmp_path, monkeypatch, capsys):
    """HMCSampleBatch on MultiComponentModule(translation_invariant="chains") with posterior_stream=True: per chain the
    accepted counts and model.dat rows of HMCSample on translation_invariant=True with seed + rank (1e-8: one unit of the
    text sink's last digit); R-hat across the chains is finite."""
    monkeypatch.chdir(tmp_path)
    comps = ("gz", "gzz", "gxx")
    mesh = G.mesher.PrismMesh(MODULE["mrange"], MODULE["mspacing"])
    b6 = mesh.cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    zp, M, n = np.full(xp.size, -20.0), b6.shape[0], xp.size
    rng = np.random.default_rng(21)

    def make(dobs, ti):
        return G.MultiComponentModule(dobs, MODULE["mrange"], MODULE["mspacing"], (xp, yp, zp), components=comps,
                                      weights="std", verbose=False, translation_invariant=ti)

    probe = make([rng.normal(size=n) for _ in comps], True)
    rho = np.zeros(M)
    rho[M // 3:M // 3 + M // 8] = 0.015
    d = probe.forward(rho)
    probe._engine.close()
    dobs = [d[c * n:(c + 1) * n] + 0.01 * np.abs(d[c * n:(c + 1) * n]).max() * rng.normal(size=n) for c in range(3)]
    C, nsamp, ndraws, seed = 3, 6, 2, 5
    bat = make(dobs, "chains")
    assert bat.translation_invariant and bat.translation_invariant_chains and bat._engine._translation_invariant_chains
    plan = bat.translation_invariant_batch_plan()
    assert plan["on"] and plan["fits"] and plan["blocks"] == 3
    assert bat.translation_invariant_info()["on"]
    with pytest.raises(NotImplementedError, match="multi-component store"):
        bat.Aw
    args = (0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, 0.0), np.full(M, 0.02)], "mandatory", 1000,
            bat.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, seed, 0.3)
    G.HMCSampleBatch(bat, C, nsamp, ndraws, *args, save_folder="bat_chain", sample_sink="text", posterior_stream=True)
    st = bat._engine.posterior_stream_read()
    rhat = np.asarray(st["rhat"])
    print("R-hat max", np.nanmax(rhat), "cells with a value", int(np.isfinite(rhat).sum()), "of", M, "n", st["n_per_chain"])
    assert rhat.shape == (M,) and np.isfinite(np.nanmax(rhat)) and np.isfinite(rhat).sum() > M // 2
    assert list(st["n_per_chain"][:C]) == [nsamp] * C
    bat._engine.close()
    for r in range(C):
        one = make(dobs, True)
        G.HMCSample(one, nsamp, ndraws, *args, nbest=100, myrank=r, save_folder="one_chain")
        one._engine.close()
        a = np.atleast_2d(np.loadtxt("bat_chain%d/model.dat" % r))
        b = np.atleast_2d(np.loadtxt("one_chain%d/model.dat" % r))
        assert a.shape == b.shape == (nsamp, M)     # the same accepted counts
        assert np.abs(a - b).max() <= 1e-8 * (1 + 1e-6)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_an_extent_beyond_the_batch_tile_is_refused_by_batch_init(G):
    kw = lb.REFUSED_CASES["y833"]
    obs, b6 = mb.geometry(**kw)
    N, M = obs.shape[1], b6.shape[0]
    eng = multi_engine(G, obs, b6, ("gz", "gzz"), (2.0, 1.0), "chains")
    plan = eng.translation_invariant_batch_plan()
    assert plan == mb.plan(tuple(kw["cells"]) + tuple(kw["obs"]), plan["cus"], 2) and plan["on"] and not plan["fits"]
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(2 * N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    for _ in range(2):
        with pytest.raises(NotImplementedError, match=STORE) as e:
            eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)
        assert "LDS tile" in str(e.value) and "833" in str(e.value)
    eng.chain_init(0.01 * wm, 0.0 * wm, 1.0 * wm)      # the single chain runs on it as before
    eng.close()


def test_refusals_on_the_table_of_blocks_that_takes_batches(G):
    from gravinv3dhmc_amd import _lib
    import ctypes
    obs, b6 = mb.geometry(**mb.PASS_CASES["beyond"])
    N, M = 2 * obs.shape[1], b6.shape[0]
    eng = multi_engine(G, obs, b6, ("gz", "gzz"), (2.0, 1.0), "chains")
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    for what, call in (("wavelet", lambda: eng.compress_wavelet(1, (1, 1, M), 0.001, 2)),
                       ("upload", lambda: eng.upload_G(np.zeros((N, M)))),
                       ("bscg", lambda: eng.bscg_run(np.ones((2, N)), np.zeros(N), 0.01 * wm, 0.0, 1.0, 0.0, 2, 4))):
        with pytest.raises(NotImplementedError, match=STORE):
            call()
        print("refused:", what)
    lib = _lib.load()
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 2 * M), (lib.gh_shard_init_rows, 2 * N)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        assert rc == _lib.GH_ERR_UNSUPPORTED and STORE.encode() in lib.gh_last_error(eng._h)
    with pytest.raises((NotImplementedError, ValueError)):
        eng.set_translation_invariant("chains")         # (stays refused: built, and the table is this context's form)
    eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)   # ... and the batch itself runs
    eng.close()
    # one form at a time, before the build as well
    eng = G.Engine(N, M)
    eng.set_cells_multi(b6, ["gz", "gzz"], [2.0, 1.0], translation_invariant="chains")
    for call in (eng.set_matrix_free, eng.set_shift_invariant):
        with pytest.raises(ValueError, match=STORE):
            call(True)
    for mode in (True, "chains", False):
        with pytest.raises(NotImplementedError, match="gh_set_cells_multi_table"):
            eng.set_translation_invariant(mode)         # (the table is this context's form)
    eng.close()
    eng = G.Engine(N, M)
    with pytest.raises(ValueError, match="chains"):
        eng.set_cells_multi(b6, ["gz", "gzz"], [2.0, 1.0], translation_invariant="replicates")
    eng.close()


def test_the_other_stores_of_blocks_keep_refusing_hmcsamplebatch(G):
    """a MagVectorModule(data=...) engine and a TesseroidMultiComponentModule engine, each with its own text: the sampler's
    rows are asked with the engines' own attributes (no device work behind them)"""
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import hmc

    class Model:
        def __init__(self, eng):
            self._engine = eng

    M = 12
    args = (2, 2, 1, 0.01, [2, 3], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.zeros(M), np.full(M, 0.02)], "mandatory",
            1000, np.zeros(3), "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3)
    mag = G.Engine(8, M)
    mag._set_store(_lib.CELL_PRISM_MVI_DATA, cols=3, rows=2, table=True)
    tess = G.Engine(8, M)
    tess._set_store(_lib.CELL_TESSEROID_MULTI, rows=2, table=True)
    for eng, text in ((mag, "MagVectorModule with data="), (tess, "TesseroidMultiComponentModule")):
        eng._translation_invariant_chains = True        # (the flag opens neither)
        with pytest.raises(NotImplementedError, match=text):
            hmc.HMCSampleBatch(Model(eng), *args)
        eng.close()
