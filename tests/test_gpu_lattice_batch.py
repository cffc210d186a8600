"""GPU suite (`-m gpu`): chain batches on the translation-invariant store (csrc/latbatch.hip.h, host_lattice.h:
latb_plan; Engine.set_translation_invariant("chains")).

The reference is the suite's own: lattice_batch_cases.py restates the two gathers and the batch correlation in NumPy and
test_lattice_batch_host.py checks that restatement against the expanded dense operator on the CPU; here the restated
operator, as a matrix, drives oracle.Problem.  Bound: 1e-10 relative, the existing suites' tolerance for a changed
order of summation (test_gpu_lattice.py); decisions identical -- the CPU suite checks that every trajectory of the
chains' cases keeps a Metropolis margin of 1e-6, the cases without an oracle kernel (gzz, tf) check it here before they
compare.  The kernel's edges (latb_pass_kernel: a wave owns 2 output rows x up to 4 MFMA tiles of 16 outputs, a
workgroup 8 output rows, K-steps of 4 inputs over rows padded to 8, forward chunks of layers capped at 32) are the
PASS_CASES of lattice_batch_cases.py; each case first reads the plan back and compares it with the restated one."""
import numpy as np
import pytest

from helpers import relmax
import lattice_batch_cases as lb
from lattice_cases import geometry

pytestmark = pytest.mark.gpu

TF_DIR = (0.3, -0.5, 0.8124038404635961)
KINDS = {"gz": (0, {}), "gzz": (3, {"component": "gzz"}), "tf": (2, {"direction": TF_DIR})}
STORE = "translation-invariant store"


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def engine(G, obs, b6, mode, kind=0, **kw):
    eng = G.Engine(obs.shape[1], b6.shape[0])
    if mode:
        eng.set_translation_invariant(mode)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, kind, **kw)
    eng.build_G()
    return eng


_REF = {}


def reference(orc, name):
    """obs, b6, the restated weighted operator (N x M), the oracle's weights and the lattice of a case: computed once,
    shared, left unchanged"""
    if name not in _REF:
        obs, b6 = geometry(**(lb.BIG if name == "big" else lb.PASS_CASES[name]))
        A, wm = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))  # (A: weighted)
        dims, col, ool = lb.lattice(obs, b6)
        T = lb.table_of(A * wm[None, :], dims, col, ool)
        Aw = np.asfortranarray(lb.expanded(T, dims, col, ool) * (1.0 / wm)[None, :])
        for a in (obs, b6, Aw, wm):
            a.setflags(write=False)
        _REF[name] = (obs, b6, Aw, wm, dims)
    return _REF[name]


def check_plan(eng, dims):
    plan = eng.translation_invariant_batch_plan()
    assert plan["on"] and plan["cus"] > 0
    assert plan == lb.plan(dims, plan["cus"])
    return plan


def setup(eng, reg, shape, dobs, wm):
    eng.set_data(dobs)
    eng.set_reg(reg, 1.0, 0.01, shape, 0.001 * wm)


# ------------------------------------------------------------------------------------------------ 1. the passes

@pytest.mark.parametrize("name", sorted(lb.PASS_CASES) + ["big"])
def test_passes_against_the_restated_operator(G, orc, name):
    """One round of all 16 slots, L = 1 .. 3: the proposals' potentials are the forward pass, the accepted states the
    adjoint pass and the update, per chain."""
    obs, b6, Aw, wm_o, dims = reference(orc, name)
    N, M = Aw.shape
    eng = engine(G, obs, b6, "chains")
    plan = check_plan(eng, dims)
    assert plan["fits"]
    if name == "layers per chunk":
        assert plan["chunks"] < dims[2]
    if name == "big":
        assert N == 16900 and N % 16 != 0
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    rng = np.random.default_rng(17)
    rho = np.zeros(M)
    rho[rng.choice(M, max(1, M // 10), replace=False)] = 0.03
    d0 = Aw @ (wm * rho)
    dobs = d0 + 1e-3 * np.abs(d0).max() * rng.normal(size=N)
    setup(eng, "Damping", (1, 1, M), dobs, wm)
    P = orc.Problem(Aw, dobs, 0.001 * wm, "Damping", 1.0, 0.01, wm=wm, shape=(1, 1, M))
    low, high = 0.0 * wm, 0.05 * wm
    x0s = rng.uniform(0.0, 0.05, (lb.CB, M)) * wm
    p0s = rng.normal(size=(lb.CB, M)) * 0.02 * wm
    us = rng.uniform(size=lb.CB)
    Ls = [1 + c % 3 for c in range(lb.CB)]
    dt = 0.1
    ref = [P.leapfrog(x0s[c], p0s[c], dt, Ls[c], low, high, float(us[c])) for c in range(lb.CB)]
    margin = min(abs(np.log(us[c]) + (ref[c][2][4] - ref[c][2][3])) for c in range(lb.CB))
    print(name, "margin", margin, "accepted", sum(r[1] for r in ref))
    assert margin >= 1e-6 and sum(r[1] for r in ref) > 0
    eng.batch_init(x0s, low, high)
    acc, out5 = eng.batch_trajectory(p0s, dt, Ls, us)
    worst = 0.0
    for c in range(lb.CB):
        xo, acco, oo, _ = ref[c]
        worst = max(worst, relmax(out5[c], oo), relmax(eng.batch_get_x(c), xo))
        assert bool(acc[c]) == bool(acco)
    print(name, "worst", worst)
    assert worst <= 1e-10
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the chains

def run_rounds(eng, prob, C):
    eng.batch_init(np.stack([prob["x0"]] * C), prob["low"], prob["high"])
    out = []
    for L, p0s, us in prob["rounds"]:
        acc, o5 = eng.batch_trajectory(p0s[:C], prob["dt"], L[:C], us[:C])
        out.append((np.array(acc), o5.copy(), np.stack([eng.batch_get_x(c) for c in range(C)])))
    return out


def run_carry(eng, prob, C, T=2):
    """The lists through gh_batch_run in carry-over mode -- a call ends when the first chain has started its T offers,
    the others keep a trajectory in flight -- for as long as every chain can be offered T, then the drain.  Per chain
    the results in order of completion; the chains end up with different numbers of them."""
    n = len(prob["rounds"])
    eng.batch_init(np.stack([prob["x0"]] * C), prob["low"], prob["high"])
    started, got = [0] * C, [[] for _ in range(C)]
    in_flight = False

    def take(res):
        acc, out5, xs, ns, nd = res
        for c in range(C):
            started[c] += int(ns[c])
            for i in range(int(nd[c])):
                got[c].append((bool(acc[c, i]), out5[c, i].copy(), xs[c, i].copy()))

    while max(started) + T <= n:
        off = [list(range(started[c], started[c] + T)) for c in range(C)]
        take(eng.batch_run([[prob["rounds"][t][1][c] for t in off[c]] for c in range(C)], prob["dt"],
                           [[prob["rounds"][t][0][c] for t in off[c]] for c in range(C)],
                           [[prob["rounds"][t][2][c] for t in off[c]] for c in range(C)], want_x=True, carry=True))
        in_flight = in_flight or any(started[c] > len(got[c]) for c in range(C))
    take(eng.batch_run([[] for _ in range(C)], prob["dt"], np.zeros((C, 0)), np.zeros((C, 0)), want_x=True, carry=True))
    assert all(started[c] == len(got[c]) >= T for c in range(C))
    return in_flight, got


def compare_carry(eng, got, rounds, C):
    """bit for bit the rounds' results, trajectory by trajectory of every chain; the chain's state is its last one's"""
    for c in range(C):
        for t, (a, o, x) in enumerate(got[c]):
            assert a == bool(rounds[t][0][c]) and np.array_equal(o, rounds[t][1][c])
            if a:
                assert np.array_equal(x, rounds[t][2][c])
        assert np.array_equal(eng.batch_get_x(c), rounds[len(got[c]) - 1][2][c])


def compare_with_oracle(rounds, ref, C):
    worst = 0.0
    for (acc, o5, xs), (acco, oo, xo) in zip(rounds, ref):
        assert np.array_equal(acc, acco[:C])
        worst = max(worst, relmax(o5, oo[:C]), relmax(xs, xo[:C]))
    return worst


@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
@pytest.mark.parametrize("name", lb.CHAIN_CASES)
def test_chains_against_oracle_single_chain_and_bitwise_paths(G, orc, name, reg):
    obs, b6, Aw, wm_o, dims = reference(orc, name)
    N, M = Aw.shape
    prob = lb.chain_problem(name, reg, Aw, wm_o)
    P = orc.Problem(Aw, prob["dobs"], prob["mwapr"], reg, 1.0, 0.01, wm=wm_o, shape=prob["shape"])
    ref, margin = lb.oracle_chains(P, prob, lb.CB)
    assert margin >= 1e-6
    eng = engine(G, obs, b6, "chains")
    check_plan(eng, dims)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    setup(eng, reg, prob["shape"], prob["dobs"], wm_o)

    # 16 chains, different L per chain: rounds in lock-step against the oracle
    rounds = run_rounds(eng, prob, lb.CB)
    worst = compare_with_oracle(rounds, ref, lb.CB)
    n_acc = sum(int(r[0].sum()) for r in rounds)
    clamps = sum(int(np.any(r[2] == prob["low"]) or np.any(r[2] == prob["high"])) for r in rounds)
    print(name, reg, "16 chains vs oracle", worst, "accepted", n_acc, "of", lb.CB * lb.N_ROUNDS)
    assert worst <= 1e-10 and 0 < n_acc < lb.CB * lb.N_ROUNDS and clamps > 0

    # each chain against the single-chain table fed the same draws
    one = engine(G, obs, b6, True)
    assert np.array_equal(one.weight(0.5), wm)
    setup(one, reg, prob["shape"], prob["dobs"], wm_o)
    worst1 = 0.0
    for c in range(lb.CB):
        one.chain_init(prob["x0"], prob["low"], prob["high"])
        for t, (L, p0s, us) in enumerate(prob["rounds"]):
            a1, o1 = one.chain_trajectory(p0s[c], prob["dt"], L[c], float(us[c]))
            assert bool(a1) == bool(rounds[t][0][c])
            worst1 = max(worst1, relmax(rounds[t][1][c], o1), relmax(rounds[t][2][c], one.chain_get_x()))
    print(name, reg, "16 chains vs single-chain table", worst1)
    assert worst1 <= 1e-10
    one.close()

    # two runs: bit for bit
    again = run_rounds(eng, prob, lb.CB)
    for (a1, o1, x1), (a2, o2, x2) in zip(rounds, again):
        assert np.array_equal(a1, a2) and np.array_equal(o1, o2) and np.array_equal(x1, x2)

    # gh_batch_run with carry-over against the rounds: bit for bit (accepted results carry their state)
    in_flight, got = run_carry(eng, prob, lb.CB)
    assert in_flight  # (different L per chain: a call leaves trajectories in flight)
    compare_carry(eng, got, rounds, lb.CB)

    # chain 0 of the 16-chain batch against the same chain run alone with C = 1: bit for bit
    alone = run_rounds(eng, prob, 1)
    for (a1, o1, x1), (a2, o2, x2) in zip(rounds, alone):
        assert a1[0] == a2[0] and np.array_equal(o1[0], o2[0]) and np.array_equal(x1[0], x2[0])
    eng.close()


@pytest.mark.parametrize("C", [1, 3])
def test_fewer_chains_than_slots(G, orc, C):
    name, reg = "shuffled", "TV"
    obs, b6, Aw, wm_o, dims = reference(orc, name)
    prob = lb.chain_problem(name, reg, Aw, wm_o)
    P = orc.Problem(Aw, prob["dobs"], prob["mwapr"], reg, 1.0, 0.01, wm=wm_o, shape=prob["shape"])
    ref, margin = lb.oracle_chains(P, prob, C)
    assert margin >= 1e-6
    eng = engine(G, obs, b6, "chains")
    eng.weight(0.5)
    setup(eng, reg, prob["shape"], prob["dobs"], wm_o)
    rounds = run_rounds(eng, prob, C)
    worst = compare_with_oracle(rounds, ref, C)
    print(C, "chains vs oracle", worst)
    assert worst <= 1e-10
    _, got = run_carry(eng, prob, C)
    compare_carry(eng, got, rounds, C)
    eng.close()


@pytest.mark.parametrize("field", ["gzz", "tf"])
def test_chains_of_a_component_and_tf_table(G, orc, monkeypatch, field):
    """gzz and tf tables: the oracle on the dense store's weighted kernel of the same field, and the single-chain table"""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    name, reg = "beyond", "TV"
    obs, b6 = geometry(**lb.PASS_CASES[name])
    kind, kw = KINDS[field]
    dense = engine(G, obs, b6, False, kind, **kw)
    wm_d = dense.weight(0.5)
    Aw = np.asfortranarray(np.asarray(dense.download_G())[:obs.shape[1]])
    dense.close()
    prob = lb.chain_problem(name, reg, Aw, wm_d, seed=8)
    # (no oracle kernel of these fields to choose a step size with on the CPU: a large one, whose trajectories the test may
    # all reject, and two smaller ones; every one of them is compared)
    eng = engine(G, obs, b6, "chains", kind, **kw)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_d) <= 1e-11
    one = engine(G, obs, b6, True, kind, **kw)
    one.weight(0.5)
    n_acc = n_all = 0
    for dt in (0.4, 0.05, 0.005):
        prob["dt"] = dt
        P = orc.Problem(Aw, prob["dobs"], prob["mwapr"], reg, 1.0, 0.01, wm=wm_d, shape=prob["shape"])
        ref, margin = lb.oracle_chains(P, prob, lb.CB)
        print(field, dt, "margin", margin)
        assert margin >= 1e-6
        for e in (eng, one):
            setup(e, reg, prob["shape"], prob["dobs"], wm_d)
        rounds = run_rounds(eng, prob, lb.CB)
        worst = compare_with_oracle(rounds, ref, lb.CB)
        for c in (0, 7, 15):
            one.chain_init(prob["x0"], prob["low"], prob["high"])
            for t, (L, p0s, us) in enumerate(prob["rounds"]):
                a1, o1 = one.chain_trajectory(p0s[c], dt, L[c], float(us[c]))
                assert bool(a1) == bool(rounds[t][0][c])
                worst = max(worst, relmax(rounds[t][1][c], o1), relmax(rounds[t][2][c], one.chain_get_x()))
        print(field, dt, "worst", worst, "accepted", sum(int(r[0].sum()) for r in rounds))
        assert worst <= 1e-10
        n_acc += sum(int(r[0].sum()) for r in rounds)
        n_all += lb.CB * lb.N_ROUNDS
    assert 0 < n_acc < n_all
    eng.close()
    one.close()


# ------------------------------------------------------------------------------------------------ 3. the module

MODULE = dict(mrange=(0.0, 7 * 150.0, 0.0, 5 * 150.0, 0.0, 450.0), mspacing=(150.0, 150.0, 150.0))


def test_hmcsample_batch_on_the_table_with_the_posterior_stream(G, tmp_path, monkeypatch, capsys):
    """HMCSampleBatch on GravMagModule(translation_invariant="chains") with posterior_stream=True: per chain the accepted
    counts and model.dat rows of HMCSample on the table with seed + rank (atol 2e-8, the tolerance of
    test_hmcsample_batch_on_a_matrix_free_global_model); R-hat across the chains is finite."""
    from gravinv3dhmc_amd import posterior
    monkeypatch.chdir(tmp_path)
    mesh = G.mesher.PrismMesh(MODULE["mrange"], MODULE["mspacing"])
    b6 = mesh.cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    zp, M = np.full(xp.size, -20.0), b6.shape[0]
    rng = np.random.default_rng(21)

    def make(dobs, ti):
        return G.GravMagModule(dobs, MODULE["mrange"], MODULE["mspacing"], (xp, yp, zp), verbose=False,
                               translation_invariant=ti)

    probe = make(np.zeros(xp.size), True)
    wm = probe.Wm.diagonal()
    rho = np.zeros(M)
    rho[M // 3:M // 3 + M // 8] = 0.015
    d = probe._engine.forward(wm * rho)
    probe._engine.close()
    dobs = d + 0.01 * np.abs(d).max() * rng.normal(size=d.size)
    C, nsamp, ndraws, seed = 3, 6, 2, 5
    args = (0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.full(M, 0.0), np.full(M, 0.02)], "mandatory", 1000,
            dobs, "Fixed", 0.8, 1.0, "TV", 0.001, seed, 0.3)
    bat = make(dobs, "chains")
    assert bat.translation_invariant and bat._engine._translation_invariant_chains
    G.HMCSampleBatch(bat, C, nsamp, ndraws, *args, save_folder="bat_chain", posterior_stream=True)
    sm = posterior.summarize_stream(bat, dobs)
    rhat = np.asarray(sm["rhat"])
    print("R-hat max", sm["rhat_max"], "cells with a value", int(np.isfinite(rhat).sum()), "of", M, "n", sm["n_per_chain"])
    # (a cell every sample of which sits on a bound has no variance and no R-hat: rhat_max is the NaN-aware maximum)
    assert rhat.shape == (M,) and np.isfinite(sm["rhat_max"]) and np.isfinite(rhat).sum() > M // 2
    assert list(sm["n_per_chain"][:C]) == [nsamp] * C
    bat._engine.close()
    for r in range(C):
        one = make(dobs, True)
        G.HMCSample(one, nsamp, ndraws, *args, nbest=100, myrank=r, save_folder="one_chain")
        one._engine.close()
        a = np.atleast_2d(np.loadtxt("bat_chain%d/model.dat" % r))
        b = np.atleast_2d(np.loadtxt("one_chain%d/model.dat" % r))
        assert a.shape == b.shape == (nsamp, M)     # the same accepted counts
        assert np.abs(a - b).max() <= 2e-8
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ 4. refusals

def test_refusals_on_a_context_that_takes_batches(G):
    from gravinv3dhmc_amd import _lib
    import ctypes
    obs, b6 = geometry(**lb.PASS_CASES["beyond"])
    N, M = obs.shape[1], b6.shape[0]
    eng = engine(G, obs, b6, "chains")
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
    # ... and the batch itself runs
    eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)
    eng.close()

    # the other forms stay one at a time under mode 2
    eng = G.Engine(N, M)
    eng.set_translation_invariant("chains")
    for call in (eng.set_matrix_free, eng.set_shift_invariant):
        with pytest.raises(ValueError, match=STORE):
            call(True)
    eng.close()

    # the plan of a context that does not take batches is off
    eng = engine(G, obs, b6, True)
    assert not eng.translation_invariant_batch_plan()["on"]
    eng.close()


def test_batches_on_the_table_of_blocks_stay_refused(G):
    obs, b6 = geometry(**lb.PASS_CASES["beyond"])
    N, M = obs.shape[1], b6.shape[0]
    eng = G.Engine(2 * N, M)
    eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 1.0], translation_invariant=True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(2 * N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    with pytest.raises(NotImplementedError):
        eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)
    with pytest.raises(NotImplementedError):
        eng.set_translation_invariant("chains")
    assert not eng.translation_invariant_batch_plan()["on"]
    eng.close()


@pytest.mark.parametrize("name", sorted(lb.REFUSED_CASES))
def test_an_extent_beyond_the_batch_tile_is_refused_by_batch_init(G, name):
    """From the first extent whose tile passes the 160 KB of a workgroup on (the last one that fits, y832, runs among the
    passes' cases): GH_ERR_UNSUPPORTED from batch_init naming the store and the extent, never a failed launch."""
    kw = lb.REFUSED_CASES[name]
    obs, b6 = geometry(**kw)
    N, M = obs.shape[1], b6.shape[0]
    eng = engine(G, obs, b6, "chains")
    plan = eng.translation_invariant_batch_plan()
    dims = tuple(kw["cells"]) + tuple(kw["obs"])
    assert plan == lb.plan(dims, plan["cus"]) and plan["on"] and not plan["fits"]
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.0 * wm)
    for _ in range(2):  # (refused every time: nothing half-made stays behind)
        with pytest.raises(NotImplementedError, match=STORE) as e:
            eng.batch_init(np.stack([0.01 * wm, 0.02 * wm]), 0.0 * wm, 1.0 * wm)
        assert str(kw["cells"][1]) in str(e.value) and str(kw["obs"][1]) in str(e.value)
    # reading the plan leaves the context's last error text alone
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    before = lib.gh_last_error(eng._h)
    assert STORE.encode() in before
    eng.translation_invariant_batch_plan()
    assert lib.gh_last_error(eng._h) == before
    # the single chain runs on it as before
    eng.chain_init(0.01 * wm, 0.0 * wm, 1.0 * wm)
    eng.close()


def test_the_mode_is_0_1_or_2(G):
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    eng = G.Engine(4, 4)
    for bad in (3, -1):
        assert lib.gh_set_translation_invariant(eng._h, bad) == _lib.GH_ERR_ARG
    eng.close()
