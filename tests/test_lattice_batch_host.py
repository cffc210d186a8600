"""CPU suite: the door to chain batches on the translation-invariant store (translation_invariant="chains") and the
suite's own reference for test_gpu_lattice_batch.py -- the NumPy restatement of csrc/latbatch.hip.h
(lattice_batch_cases.py) against the expanded dense operator, the restated plan at its edges, and the conditioning of
the chains' cases on the oracle: every trajectory the GPU suite runs has a Metropolis margin
|log u + (Hnew - Hcur)| >= 1e-6, so that 1e-10 of a potential of ~1e2 cannot flip a decision."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)
import lattice_batch_cases as lb
from lattice_cases import geometry

REFUSAL = "the translation-invariant store (translation_invariant=True; single chain)"


class _Lib:
    """gh_set_translation_invariant alone: records what the engine passes"""

    def __init__(self):
        self.modes = []

    def gh_set_translation_invariant(self, h, mode):
        self.modes.append(mode)
        return 0


def _stub_engine():
    from gravinv3dhmc_amd.engine import Engine
    eng = object.__new__(Engine)
    eng._lib, eng._h = _Lib(), None
    return eng


def test_engine_accepts_chains_and_rejects_other_strings():
    eng = _stub_engine()
    eng.set_translation_invariant("chains")
    assert eng._lib.modes == [2] and eng._translation_invariant is True and eng._translation_invariant_chains is True
    eng.set_translation_invariant(True)
    assert eng._lib.modes == [2, 1] and eng._translation_invariant is True and eng._translation_invariant_chains is False
    eng.set_translation_invariant(False)
    assert eng._lib.modes == [2, 1, 0] and eng._translation_invariant is False and not eng._translation_invariant_chains
    for bad in ("chain", "Chains", "", "batch", "True"):
        with pytest.raises(ValueError, match="chains"):
            eng.set_translation_invariant(bad)
    assert eng._lib.modes == [2, 1, 0]


class _Stop(Exception):
    pass


@pytest.mark.parametrize("kw", [{}, {"component": "gzz"}, {"field": "magnetic", "mangle": (60, 10)}], ids=["gz", "gzz", "magnetic"])
def test_module_hands_chains_to_the_engine(monkeypatch, kw):
    """GravMagModule(translation_invariant="chains") with component= and field="magnetic": the engine is asked for the
    table that takes batches before it sees the observations (no device: the engine is a recorder)"""
    from gravinv3dhmc_amd.inversion import potential
    asked = []

    class Recorder:
        def __init__(self, N, M, device=0):
            pass

        def set_translation_invariant(self, on=True):
            asked.append(on)

        def set_obs(self, *a):
            raise _Stop()

    monkeypatch.setattr(potential, "Engine", Recorder)
    xp, yp = [a.ravel() for a in np.meshgrid(75.0 + 150.0 * np.arange(7), 75.0 + 150.0 * np.arange(5), indexing="ij")]
    for ti, want in (("chains", "chains"), (True, True)):
        with pytest.raises(_Stop):
            potential.GravMagModule(np.zeros(xp.size), (0.0, 1050.0, 0.0, 750.0, 0.0, 450.0), (150.0, 150.0, 150.0),
                                    (xp, yp, np.full(xp.size, -20.0)), verbose=False, translation_invariant=ti, **kw)
        assert asked[-1] == want
    # the refusals of translation_invariant=True hold for "chains" as well
    with pytest.raises(NotImplementedError, match="translation-invariant store"):
        potential.GravMagModule(np.zeros(xp.size), (0.0, 1050.0, 0.0, 750.0, 0.0, 450.0), (150.0, 150.0, 150.0),
                                (xp, yp, np.full(xp.size, -20.0)), verbose=False, translation_invariant="chains", wavelet="1D")


def test_sampler_skips_the_tables_row_for_chains_only():
    from gravinv3dhmc_amd.inversion import hmc

    class Eng:
        pass

    class Model:
        def __init__(self, **attrs):
            self._engine = Eng()
            for k, v in attrs.items():
                setattr(self._engine, k, v)

        def kernelw(self):
            raise _Stop()

    M = 4
    args = (2, 2, 1, 0.01, [2, 3], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.zeros(M), np.full(M, 0.02)], "mandatory",
            1000, np.zeros(3), "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3)
    with pytest.raises(NotImplementedError) as e:
        hmc.HMCSampleBatch(Model(_translation_invariant=True), *args)
    assert REFUSAL in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        hmc.HMCSampleBatch(Model(_translation_invariant=True, _translation_invariant_chains=False), *args)
    assert REFUSAL in str(e.value)
    assert (("_translation_invariant",), REFUSAL) in hmc._NO_BATCH and hmc._TABLE_ROW in hmc._NO_BATCH
    with pytest.raises(_Stop):
        hmc.HMCSampleBatch(Model(_translation_invariant=True, _translation_invariant_chains=True), *args)
    # the table of blocks keeps refusing, whatever the flag says
    with pytest.raises(NotImplementedError, match="MultiComponentModule"):
        hmc.HMCSampleBatch(Model(multi=True, _translation_invariant=True, _translation_invariant_chains=True), *args)


# ----------------------------------------------------------------------------- the restatement against dense

@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("name", sorted(lb.PASS_CASES))
def test_restated_gathers_and_correlation_against_the_expanded_operator(orc, name):
    obs, b6 = geometry(**lb.PASS_CASES[name])
    A = np.ascontiguousarray(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
    N, M = A.shape
    dims, col, ool = lb.lattice(obs, b6)
    T = lb.table_of(A, dims, col, ool)
    # the table stands for the dense operator (entries of one offset agree to the prism formula's own rounding)
    E = lb.expanded(T, dims, col, ool)
    assert np.abs(E - A).max() <= 1e-11 * np.abs(A).max()
    rng = np.random.default_rng(3)
    X, R = rng.normal(size=(M, lb.CB)), rng.normal(size=(N, lb.CB))
    X[:, 5] = 0.0  # (an empty slot among live ones)
    iw = 1.0 / rng.uniform(0.5, 2.0, M)
    ld = (N + 15) // 16 * 16
    D = lb.forward16(T, X, iw, dims, col, ool)
    S = lb.adjoint16(T, lb.to_rt(R, ld), dims, col, ool)
    Dref, Sref = E @ (X * iw[:, None]), E.T @ R
    assert np.abs(D - Dref).max() <= 1e-12 * np.abs(Dref).max()
    assert np.abs(S - Sref).max() <= 1e-12 * np.abs(Sref).max()
    assert not D[:, 5].any()
    # a chain's column does not depend on what the other slots hold
    X1 = np.zeros_like(X)
    X1[:, 0] = X[:, 0]
    assert np.array_equal(lb.forward16(T, X1, iw, dims, col, ool)[:, 0], D[:, 0])


def test_restated_plan_at_its_edges():
    def dims(name):
        kw = lb.PASS_CASES[name]
        return (kw["cells"][0], kw["cells"][1], kw["cells"][2], kw["obs"][0], kw["obs"][1])

    for cus in (64, 256, 304):
        p = lb.plan(dims("y16"), cus)
        assert (p["adj_ntiles"], p["adj_FT"], p["adj_WT"], p["adj_WL"]) == (1, 1, 16, 32) and p["fits"]
        p = lb.plan(dims("y17"), cus)
        assert (p["adj_ntiles"], p["adj_FT"], p["adj_WT"], p["adj_WL"]) == (2, 1, 32, 24 + 32)
        p = lb.plan(dims("y64"), cus)
        assert (p["fwd_ntiles"], p["fwd_FT"], p["fwd_WT"]) == (4, 1, 64)
        p = lb.plan(dims("y65"), cus)
        assert (p["fwd_ntiles"], p["fwd_FT"], p["fwd_WT"], p["fwd_grid"]) == (5, 2, 48, 2)
        p = lb.plan(dims("rows beyond one tile"), cus)
        assert p["adj_grid"] == 2 and p["fwd_grid"] == 2 and p["pp_rows"] == 4
        p = lb.plan(dims("layers per chunk"), cus)
        assert p["lpc"] == 2 and p["chunks"] == 17  # more layers than slab rows
        # 200 cells under 200 stations along y fit
        p = lb.plan((200, 200, 60, 200, 200), cus)
        assert p["fits"] and p["adj_lds"] == (8 * (200 + 64) + 16 * 200) * 8 and p["chunks"] <= 32
        # the tile is 192 NFip + 64 WT bytes, all of the kernel's LDS: the last extents within 160 KB, the first beyond
        p = lb.plan(lb.FITTING_EDGES["y832"], cus)
        assert p["fits"] and p["adj_lds"] == p["fwd_lds"] == 192 * 832 + 64 * 64 == lb.LDS_MAX
        p = lb.plan(lb.FITTING_EDGES["qy840 over ny32"], cus)
        assert p["fits"] and p["adj_lds"] == 192 * 840 + 64 * 32 <= lb.LDS_MAX
        p = lb.plan(lb.FITTING_EDGES["qy848 over ny16"], cus)
        assert p["fits"] and p["adj_lds"] == 192 * 848 + 64 * 16 == lb.LDS_MAX
        for name, kw in lb.REFUSED_CASES.items():
            p = lb.plan(tuple(kw["cells"]) + tuple(kw["obs"]), cus)
            assert not p["fits"] and max(p["adj_lds"], p["fwd_lds"]) > lb.LDS_MAX, name
        p = lb.plan(tuple(lb.REFUSED_CASES["y833"]["cells"]) + tuple(lb.REFUSED_CASES["y833"]["obs"]), cus)
        assert p["adj_lds"] == 192 * 840 + 64 * 64
        p = lb.plan((1, 64, 1, 1, 848), cus)
        assert p["adj_lds"] == 192 * 848 + 64 * 64 > lb.LDS_MAX


# ------------------------------------------------------------------------------------- the chains' conditioning

@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
@pytest.mark.parametrize("name", lb.CHAIN_CASES)
def test_chain_cases_are_well_conditioned(orc, name, reg):
    obs, b6 = geometry(**lb.PASS_CASES[name])
    Aw, wm = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
    prob = lb.chain_problem(name, reg, Aw, wm)
    P = orc.Problem(Aw, prob["dobs"], prob["mwapr"], reg, 1.0, 0.01, wm=wm, shape=prob["shape"])
    rounds, margin = lb.oracle_chains(P, prob, lb.CB)
    acc = np.array([r[0] for r in rounds])
    clamped = sum(int(np.any(r[2] == prob["low"]) or np.any(r[2] == prob["high"])) for r in rounds)
    print(name, reg, "margin", margin, "accepted", int(acc.sum()), "of", acc.size, "clamped rounds", clamped)
    assert margin >= 1e-6
    assert 0 < acc.sum() < acc.size  # accepted and rejected trajectories
    assert clamped > 0               # states clamped on a bound
