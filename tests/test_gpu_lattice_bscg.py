"""GPU suite (`-m gpu`): the bootstrap batch and the conjugate-gradient inversion on the translation-invariant store
(csrc/latbatch.hip.h: latb_pass_kernel<LATB_CG>, csrc/host_bscg.h; Engine.set_translation_invariant("replicates"),
BootStrap / ConjugateGradient(translation_invariant=True)).

References: oracle.cg_port.bootstrap_counts on the restated operator of lattice_bscg_cases.py (the oracle's kernel, its
table, expanded again), whose cases test_lattice_bscg_host.py conditions on the CPU; the reference's own runs
(tests/golden/cg_small.npz, bs_small.npz), whose geometry is on the lattice; oracle.cg_port.bootstrap on the oracle's
kernel at 600 x 6000.  gzz and the total field have no oracle kernel: there the table is held to the dense engine's own
bscg_run, HIP against HIP.  Bounds: TOL_BSCG = 1e-10 (the project's trajectory bound, what tests/test_gpu_bscg.py holds
the dense batch to) for the batch, 1e-7 for the sequential paths (test_gpu_parity.py's bound for them); lengths equal.
Each group prints its worst relmax."""
import ctypes

import numpy as np
import pytest

from conftest import gold
from helpers import relmax
import lattice_batch_cases as lb
import lattice_bscg_cases as lc
from lattice_cases import geometry

pytestmark = pytest.mark.gpu

TF_DIR = (0.3, -0.5, 0.8124038404635961)
KINDS = {"gzz": (3, {"component": "gzz"}), "tf": (2, {"direction": TF_DIR})}
STORE = "translation-invariant store"
WORST = {}


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def engine(G, obs, b6, mode, kind=0, **kw):
    eng = G.Engine(obs.shape[1], b6.shape[0])
    if mode:
        eng.set_translation_invariant(mode)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, kind, **kw)
    eng.build_G()
    return eng


def table_engine(G, d):
    """The case's engine in mode "replicates": the plan read back and equal to the restated one, the weights the oracle's"""
    eng = engine(G, d.obs, d.b6, "replicates")
    plan = eng.translation_invariant_batch_plan()
    assert plan["on"] and plan["cus"] > 0 and plan == lb.plan(d.dims, plan["cus"])
    wm = eng.weight(0.5)
    assert relmax(wm, d.wm) <= 1e-11
    return eng, plan


def run(eng, d, counts=None, maxk=None):
    maxk = maxk or d.maxk
    res = eng.bscg_run(d.counts if counts is None else counts, d.dobs, d.mw0, d.low, d.high, lc.BETA2, d.q, maxk)
    assert eng.bscg_stats() == {"forward_sweeps": 2 * maxk + 1, "adjoint_sweeps": maxk, "lock_steps": maxk}
    return res


def against(res, ref, where, tol=lc.TOL_BSCG):
    """Lengths equal, the four results of every replicate within tol; returns the worst relmax"""
    assert np.array_equal(res[4], ref.n_entries), (where, res[4], ref.n_entries)
    assert np.array_equal(res[5], ref.n_alpha), (where, res[5], ref.n_alpha)
    worst = 0.0
    for b in range(len(ref.n_alpha)):
        for name, v, w in zip(lc.NAMES, res, ref.results()):
            assert v[b].shape == w[b].shape
            err = relmax(v[b], w[b])
            worst = max(worst, err)
            assert err <= tol, (where, "replicate %d" % b, name, err)
    return worst


def same_bits(a, b):
    for v, w in zip(a, b):
        assert np.array_equal(v, w)


# ------------------------------------------------------------------------------------------------ 1. the passes

@pytest.mark.parametrize("name", list(lc.CASE_NAMES) + ["big"])
def test_passes_at_their_edges_against_the_oracle(G, name):
    d = lc.make(name)  # inputs and the oracle's run, before an engine is touched
    eng, plan = table_engine(G, d)
    assert plan["fits"]
    if name == "layers per chunk":
        assert plan["chunks"] < d.dims[2]
    if name == "big":
        assert d.N == 16900 and d.N % 16 != 0
    res = run(eng, d)
    eng.close()
    worst = against(res, d.ref, name)
    WORST["passes"] = max(WORST.get("passes", 0.0), worst)
    print("%s (%d x %d, B = %d, maxk = %d, q = %g): worst relmax against the oracle %.2e (group so far %.2e)"
          % (name, d.N, d.M, d.B, d.maxk, d.q, worst, WORST["passes"]))


# ------------------------------------------------------------------------------------------------ 2. branches and slots

def test_branches_of_the_recurrence_and_what_a_slot_keeps(G):
    """One group of 16 at "beyond" (bounds (0.2, 0.8), q = 0.5, maxk = 6): slot 0 counts only observations fitted from the
    start and freezes at k = 1 beside 15 that run to the end; then a group of 3 of those replicates in 16 slots, the 16
    permuted over the slots, and the group a second time: per replicate the same bits."""
    d = lc.make(lc.BRANCH)
    ref = d.ref
    assert (ref.n_alpha[0], ref.n_entries[0]) == (2, 0) and (ref.n_alpha[1:] == d.maxk).all()
    eng, _ = table_engine(G, d)
    res = run(eng, d)
    worst = against(res, ref, "group of 16")
    assert (res[0] == d.low).any() and (res[0] == d.high).any()
    # a group of 3 in 16 slots: the oracle's run, and the bits those replicates had in the group of 16
    c3, slots = d.group_of_three()
    three = run(eng, d, counts=c3)
    worst = max(worst, against(three, d.run(d.Aw, c3), "group of 3"))
    for v, w in zip(three, res):
        assert np.array_equal(v, w[slots])
    # ... and on a fresh engine
    fresh, _ = table_engine(G, d)
    same_bits(run(fresh, d, counts=c3), three)
    fresh.close()
    # the 16 permuted over the slots: the same bits per replicate
    perm = np.random.default_rng(3).permutation(d.B)
    assert (perm != np.arange(d.B)).sum() >= d.B - 2
    moved = run(eng, d, counts=d.counts[perm])
    for v, w in zip(moved, res):
        assert np.array_equal(v, w[perm])
    # a second run after the others: identical bits
    same_bits(run(eng, d), res)
    # maxk = 2 after maxk = 6 (the result block reused with other offsets): the oracle
    worst = max(worst, against(run(eng, d, maxk=2), d.run(d.Aw, d.counts, maxk=2), "maxk = 2 after maxk = 6"))
    eng.close()
    print("branch (%d x %d, B = 16, maxk = 6, q = 0.5): worst relmax against the oracle %.2e" % (d.N, d.M, worst))


# ------------------------------------------------------------------------------------------------ 3. other kinds

@pytest.mark.parametrize("field", ["gzz", "tf"])
def test_a_component_and_the_total_field_against_the_dense_store(G, monkeypatch, field):
    """HIP against HIP: the oracle has no kernel of these fields, so the table's bscg_run is held to the dense engine's own
    bscg_run on the same geometry (which tests/test_gpu_bscg_oracle.py holds to the oracle on uploaded matrices).  The
    oracle's recurrence on the dense store's downloaded kernel says how far the case is from its branch edges."""
    from oracle import cg_port
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    obs, b6 = geometry(**lb.PASS_CASES["beyond"])
    kind, kw = KINDS[field]
    dense = engine(G, obs, b6, False, kind, **kw)
    wm_d = dense.weight(0.5)
    Aw = np.asfortranarray(np.asarray(dense.download_G())[:obs.shape[1]])
    B, maxk, q = 16, 5, 0.5
    # (the stop test's threshold is absolute, data < 0.1, and these fields have other units than gz: the models' unit is
    # the power of ten that puts the start model's data near 10, as gz's are -- from the dense store's kernel alone)
    scale = 10.0 ** np.round(np.log10(10.0 / np.abs(Aw @ (0.5 * wm_d)).max()))
    # (no oracle kernel to settle a seed with on the CPU: the first of eight seeds whose draw the oracle's recurrence, on
    # the dense store's downloaded kernel, finds off every branch edge -- the host suite's conditions -- is the case)
    for seed in range(lc.SEED0 + 50, lc.SEED0 + 58):
        dobs, counts, mw0 = lc.recipe(np.random.default_rng(seed), Aw, wm_d, B, scale=scale)
        ref = cg_port.bootstrap_counts(Aw, wm_d, counts, dobs, mw0, (0.0, scale), lc.BETA2, q, maxk)
        margins = [abs(m) for tr in ref.trace for m in tr["margin"].values()]
        stops = [abs(v - lc.STOP) for tr in ref.trace for v in tr["seen"]]
        ok = (min(margins, default=0.0) >= 1e-4 and min(stops, default=0.0) >= 1e-2 and (ref.n_alpha == maxk).sum() >= B // 2)
        print(field, "seed %d, models' unit %g: smallest alpha-rule margin %.2e, smallest distance from the stop threshold "
              "%.2e, replicates that run to the end %d" % (seed, scale, min(margins, default=np.inf),
                                                           min(stops, default=np.inf), (ref.n_alpha == maxk).sum()))
        if ok:
            break
    assert ok
    args = (counts, dobs, mw0, 0.0, scale, lc.BETA2, q, maxk)
    want = dense.bscg_run(*args)
    dense.close()
    eng = engine(G, obs, b6, "replicates", kind, **kw)
    assert relmax(eng.weight(0.5), wm_d) <= 1e-11
    got = eng.bscg_run(*args)
    assert eng.bscg_stats() == {"forward_sweeps": 2 * maxk + 1, "adjoint_sweeps": maxk, "lock_steps": maxk}
    eng.close()
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])
    assert np.array_equal(got[4], ref.n_entries) and np.array_equal(got[5], ref.n_alpha)
    worst = max(relmax(v, w) for v, w in zip(got[:4], want[:4]))
    print(field, "table against the dense store (HIP against HIP): worst relmax %.2e" % worst)
    assert worst <= lc.TOL_BSCG


# ------------------------------------------------------------------------------------------------ 4. the reference's runs

@pytest.fixture(scope="module")
def small(G):
    """The problem of test_bootstrap_matches_reference, on the table: 42 observations x 120 cells, bounds (0, 1), maxk = 5"""
    g = gold("cg_small.npz")
    bs = G.BootStrap(tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"]), g["dobs"], (0.0, 1.0), samples=3,
                     beta=0.1, maxk=5, verbose=False, translation_invariant=True)
    assert (bs.dsize, bs.msize) == (42, 120)
    return bs


def test_bootstrap_on_the_table_against_the_reference_run(G, small, capsys):
    b = gold("bs_small.npz")
    info = small.translation_invariant_info()
    assert info["on"] and info["table_bytes"] == 4 * 10 * 12 * 8
    assert (info["nx"], info["ny"], info["nz"], info["px"], info["qy"]) == (5, 6, 4, 6, 7)
    assert isinstance(small.Aw, G.engine.DeviceMatrix) and small.translation_invariant
    assert small._engine.translation_invariant_batch_plan()["on"]
    m0 = np.full(small.msize, 0.001)
    worst = {}
    for what, kw, tol in (("batch=2", {"batch": 2}, lc.TOL_BSCG), ("batch=16", {"batch": 16}, lc.TOL_BSCG),
                          ("sequential", {}, 1e-7)):
        res = small.BSCG(m0, **kw)
        capsys.readouterr()
        worst[what] = max(relmax(v, b[name]) for name, v in zip(lc.NAMES, res))
        for name, v in zip(lc.NAMES, res):
            assert v.shape == b[name].shape
    with capsys.disabled():
        print("BootStrap on the table against bs_small.npz:", ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert worst["batch=2"] <= lc.TOL_BSCG and worst["batch=16"] <= lc.TOL_BSCG and worst["sequential"] <= 1e-7
    # CG_batch of one replicate's counts is CG on the same object, to the sequential path's bound
    np.random.seed(1)
    counts = np.bincount(np.random.choice(np.arange(42), size=42, replace=True), minlength=42).astype(np.float64)
    one = small.CG_batch(counts, small.dobs, m0)[0]
    want = small.CG(counts, small.dobs, m0)
    capsys.readouterr()
    for v, w in zip(one, want):
        assert len(v) == len(w) and relmax(np.asarray(v, float), np.asarray(w, float)) <= 1e-7


def test_conjugate_gradient_on_the_table_against_the_reference_run(G, capsys):
    g = gold("cg_small.npz")
    cg = G.ConjugateGradient(g["dobs"], tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"]), verbose=False,
                             translation_invariant=True)
    M = cg.msize
    assert (cg.dsize, M, cg.mshape) == (42, 120, tuple(g["shape"]))
    info = cg.translation_invariant_info()
    assert info["on"] and info["table_bytes"] == 4 * 10 * 12 * 8 and cg.translation_invariant
    assert not cg._engine.translation_invariant_batch_plan()["on"]  # (mode 1: the single-vector passes)
    worst = {}
    for reg in ("MS", "Damping", "Smoothness", "TV"):
        res = cg.CG(np.full(M, 0.001), np.full(M, 0.001), (0.0, 1.0), regularization=reg, beta=0.01, q=0.9, maxk=8)
        capsys.readouterr()
        worst[reg] = max(relmax(np.asarray(v, float), g[reg + "_" + name])
                         for name, v in zip(("model", "data", "dmis", "mmis", "alpha"), res))
    cg._engine.close()
    print("ConjugateGradient on the table against cg_small.npz:", ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1e-7, worst


# ------------------------------------------------------------------------------------------------ 5. several workgroups

def test_several_workgroups_against_the_oracle_port(G, capsys):
    """20 x 30 x 10 cells under 20 x 30 stations above the cell centres, 600 x 6000: three tiles of output rows and two
    MFMA tiles along y in the adjoint, ten layers.  `samples=5, maxk=4`: BSCG(batch=4) (groups of 4 and 1) and the
    sequential BSCG() on the table against oracle.cg_port.bootstrap on the oracle's kernel, as
    test_gpu_bscg.py::test_several_row_and_column_blocks_against_the_oracle_port holds the dense store."""
    from oracle import cg_port, oracle
    mesh = G.mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    xp, yp = [a.ravel() for a in np.meshgrid(50.0 + 100.0 * np.arange(20), 50.0 + 100.0 * np.arange(30), indexing="ij")]
    zp = np.zeros_like(xp)
    K = oracle.prism_gz_kernel(xp, yp, zp, mesh.cell_bounds())
    rho = np.zeros(mesh.shape)
    rho[3:7, 10:20, 7:13] = 0.8
    dobs = K @ rho.ravel() + 0.05 * np.random.default_rng(7).standard_normal(xp.size)
    m0 = np.full(mesh.size, 0.001)
    ref = cg_port.bootstrap(K, dobs, (0.0, 1.0), m0, samples=5, beta=0.1, maxk=4)
    bs = G.BootStrap((0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (xp, yp, zp), dobs, (0.0, 1.0), samples=5, beta=0.1,
                     maxk=4, verbose=False, translation_invariant=True)
    assert (bs.dsize, bs.msize) == (600, 6000) and bs.translation_invariant_info()["on"]
    plan = bs._engine.translation_invariant_batch_plan()
    assert plan["fits"] and plan["adj_grid"] > 1 and plan["fwd_grid"] > 1 and plan["pp_rows"] == plan["adj_grid"] * 10
    seq = bs.BSCG(m0)
    bat = bs.BSCG(m0, batch=4)
    capsys.readouterr()
    for name, r, s, v in zip(lc.NAMES, ref, seq, bat):
        es, eb = relmax(s, r), relmax(v, r)
        print("%s: sequential %.3e, batch %.3e against the oracle port" % (name, es, eb))
        assert es <= lc.TOL_BSCG, "sequential " + name
        assert eb <= lc.TOL_BSCG, "batch " + name
    assert bs._engine.bscg_stats() == {"forward_sweeps": 9, "adjoint_sweeps": 4, "lock_steps": 4}
    bs._engine.close()


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals_in_mode_replicates(G):
    from gravinv3dhmc_amd import _lib
    obs, b6 = geometry(**lb.PASS_CASES["beyond"])
    N, M = obs.shape[1], b6.shape[0]
    eng = engine(G, obs, b6, "replicates")
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    for what, call in (("batch_init", lambda: eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)),
                       ("wavelet", lambda: eng.compress_wavelet(1, (1, 1, M), 0.001, 2)),
                       ("upload", lambda: eng.upload_G(np.zeros((N, M))))):
        with pytest.raises(NotImplementedError, match=STORE) as e:
            call()
        if what == "batch_init":
            assert "single chain" in str(e.value)
        print("refused:", what)
    lib = _lib.load()
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 2 * M), (lib.gh_shard_init_rows, 2 * N)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        assert rc == _lib.GH_ERR_UNSUPPORTED and STORE.encode() in lib.gh_last_error(eng._h)
    # ... and the bootstrap batch itself runs, and the single chain beside it
    res = eng.bscg_run(np.ones((2, N)), eng.forward(0.3 * wm), 0.5 * wm, 0.0, 1.0, lc.BETA2, 0.9, 3)
    assert np.isfinite(res[0]).all()
    eng.chain_init(0.01 * wm, 0.0 * wm, 1.0 * wm)
    eng.close()

    # the modes: 0, 1, 2 and 4; the other forms stay one at a time under mode 4
    eng = G.Engine(N, M)
    for bad in (3, 5, 8, -1):
        assert lib.gh_set_translation_invariant(eng._h, bad) == _lib.GH_ERR_ARG
    eng.set_translation_invariant("replicates")
    for call in (eng.set_matrix_free, eng.set_shift_invariant):
        with pytest.raises(ValueError, match=STORE):
            call(True)
    eng.close()


def test_an_extent_beyond_the_batch_tile_is_refused_by_bscg_run(G, capsys):
    """y833, the first extent whose tile passes the 160 KB of a workgroup: bscg_run is refused with the plan's reason and
    the byte count, never a failed launch; BootStrap.CG of one replicate's counts runs on the same object."""
    ny = 833
    xp, yp = np.full(ny, 50.0), 50.0 + 100.0 * np.arange(ny)
    rng = np.random.default_rng(5)
    bs = G.BootStrap((0, 100, 0, 100.0 * ny, 0, 100), (100, 100, 100), (xp, yp, np.zeros(ny)), np.zeros(ny), (0.0, 1.0),
                     samples=2, beta=0.1, maxk=3, verbose=False, translation_invariant=True)
    assert (bs.dsize, bs.msize) == (ny, ny) and bs.translation_invariant_info()["on"]
    plan = bs._engine.translation_invariant_batch_plan()
    assert plan == lb.plan((1, ny, 1, 1, ny), plan["cus"]) and plan["on"] and not plan["fits"]
    wm = bs.Wm.diagonal()
    bs.dobs = bs._engine.forward(wm * rng.uniform(0.05, 0.95, ny))
    counts = lc.draw_counts(rng, 1, ny)
    m0 = np.full(ny, 0.5)
    for _ in range(2):  # (refused every time: nothing half-made stays behind)
        with pytest.raises(NotImplementedError, match=STORE) as e:
            bs.CG_batch(counts, bs.dobs, m0)
        assert "too long for the batch pass's LDS tile" in str(e.value) and "gh_bscg_run" in str(e.value)
        assert "833 cells, 833 observations" in str(e.value) and str(192 * 840 + 64 * 64) in str(e.value)
    model, dmis, mmis, alpha = bs.CG(counts[0], bs.dobs, m0)
    capsys.readouterr()
    assert model.shape == (ny,) and np.isfinite(model).all() and len(alpha) >= 2
    bs._engine.close()


def test_the_table_of_blocks_still_refuses_the_bootstrap_batch(G):
    obs, b6 = geometry(**lb.PASS_CASES["beyond"])
    N, M = obs.shape[1], b6.shape[0]
    eng = G.Engine(2 * N, M)
    eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 1.0], translation_invariant=True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    wm = eng.weight(0.5)
    with pytest.raises(NotImplementedError, match="bootstrap batch"):
        eng.bscg_run(np.ones((2, 2 * N)), np.zeros(2 * N), 0.01 * wm, 0.0, 1.0, lc.BETA2, 0.9, 4)
    with pytest.raises(NotImplementedError):
        eng.set_translation_invariant("replicates")
    assert not eng.translation_invariant_batch_plan()["on"]
    eng.close()
