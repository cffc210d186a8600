"""CPU suite: the door to the bootstrap batch on the translation-invariant store -- Engine.set_translation_invariant(
"replicates"), BootStrap / ConjugateGradient(translation_invariant=True) -- and the generator of
test_gpu_lattice_bscg.py's cases (lattice_bscg_cases.py), checked on the oracle alone: conditioning (float64 and
longdouble runs agree to TOL_BSCG / 10), branch margins (every alpha-rule margin |.| >= 1e-4, every data value the stop
test saw at least 1e-2 from its threshold 0.1), the clamp acting in at least half the cases, sharpness (one entry of the
weighted operator scaled by 1 + 1e-4 moves the results by more than 100 TOL_BSCG)."""
import numpy as np
import pytest

from conftest import ROOT, gold  # noqa: F401  (puts the repository on sys.path)
import lattice_batch_cases as lb
import lattice_bscg_cases as lc
from lattice_cases import detect

STORE = "translation-invariant store"


# ------------------------------------------------------------------------------------------------ the engine's door

class _Lib:
    """gh_set_translation_invariant alone: records what the engine passes"""

    def __init__(self):
        self.modes = []

    def gh_set_translation_invariant(self, h, mode):
        self.modes.append(mode)
        return 0


def test_engine_accepts_replicates_and_rejects_other_strings():
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.engine import Engine
    eng = object.__new__(Engine)
    eng._lib, eng._h = _Lib(), None
    assert _lib.TABLE_REPLICATES == 4 and _lib.TABLE_CHAINS == 2
    eng.set_translation_invariant("replicates")
    assert eng._lib.modes == [_lib.TABLE_REPLICATES] and eng._translation_invariant is True
    assert eng._translation_invariant_replicates is True and eng._translation_invariant_chains is False
    eng.set_translation_invariant("chains")
    assert eng._lib.modes[-1] == 2 and eng._translation_invariant_chains is True
    assert eng._translation_invariant_replicates is False
    eng.set_translation_invariant(True)
    assert eng._lib.modes[-1] == 1 and not eng._translation_invariant_replicates and not eng._translation_invariant_chains
    n = len(eng._lib.modes)
    for bad in ("chain", "Chains", "", "batch", "True", "replicate", "Replicates"):
        with pytest.raises(ValueError, match="chains"):
            eng.set_translation_invariant(bad)
    assert len(eng._lib.modes) == n


# ------------------------------------------------------------------------------------------------ the modules' door

class _Stop(Exception):
    pass


def _recorder(asked):
    class Recorder:
        def __init__(self, N, M, device=0):
            asked.append(("engine", N, M))

        def set_translation_invariant(self, on=True):
            asked.append(("mode", on))

        def set_obs(self, *a):
            asked.append(("obs",))
            raise _Stop()

    return Recorder


def _small():
    g = gold("cg_small.npz")
    return g, tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"])


def test_modules_hand_the_mode_to_the_engine_before_the_observations(monkeypatch):
    from gravinv3dhmc_amd.inversion import reginv
    g, mrange, mspacing, obs = _small()
    asked = []
    monkeypatch.setattr(reginv, "Engine", _recorder(asked))
    with pytest.raises(_Stop):
        reginv.BootStrap(mrange, mspacing, obs, g["dobs"], (0.0, 1.0), samples=3, beta=0.1, maxk=5, verbose=False,
                         translation_invariant=True)
    assert asked == [("engine", 42, 120), ("mode", "replicates"), ("obs",)]
    del asked[:]
    with pytest.raises(_Stop):
        reginv.ConjugateGradient(g["dobs"], mrange, mspacing, obs, verbose=False, translation_invariant=True)
    assert asked == [("engine", 42, 120), ("mode", True), ("obs",)]
    # without the keyword the engine is not asked: call for call what it was
    for make in (lambda: reginv.BootStrap(mrange, mspacing, obs, g["dobs"], (0.0, 1.0), verbose=False),
                 lambda: reginv.ConjugateGradient(g["dobs"], mrange, mspacing, obs, verbose=False),
                 lambda: reginv.BootStrap(mrange, mspacing, obs, g["dobs"], (0.0, 1.0), verbose=False,
                                          translation_invariant=False)):
        del asked[:]
        with pytest.raises(_Stop):
            make()
        assert asked == [("engine", 42, 120), ("obs",)]


def test_modules_refuse_what_the_store_does_not_combine_with_before_any_device_work(monkeypatch):
    from gravinv3dhmc_amd.inversion import reginv
    g, mrange, mspacing, obs = _small()
    asked = []
    monkeypatch.setattr(reginv, "Engine", _recorder(asked))
    topo = (np.array([0.0, 2000.0]), np.array([0.0, 3000.0]), np.array([-10.0, -10.0]))
    for kw in ({"wavelet": "1D"}, {"wavelet": "3D"}, {"mtopo": topo}):
        with pytest.raises(NotImplementedError, match=STORE):
            reginv.BootStrap(mrange, mspacing, obs, g["dobs"], (0.0, 1.0), verbose=False, translation_invariant=True, **kw)
        with pytest.raises(NotImplementedError, match=STORE):
            reginv.ConjugateGradient(g["dobs"], mrange, mspacing, obs, verbose=False, translation_invariant=True, **kw)
    with pytest.raises(NotImplementedError, match=STORE):
        reginv.ConjugateGradient(g["dobs"], (0, 10, 0, 10, 1000, 2000), (1, 1, 100), obs, coordinate="spherical",
                                 verbose=False, translation_invariant=True)
    assert asked == []
    # the keyword is a named parameter in front of the topography's **kwargs
    import inspect
    for cls in (reginv.BootStrap, reginv.ConjugateGradient):
        p = inspect.signature(cls.__init__).parameters
        assert p["translation_invariant"].default is False
        assert p["translation_invariant"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert list(p)[-1] == "kwargs" and list(p)[-2] == "translation_invariant"


def test_the_reference_runs_geometry_is_on_the_lattice():
    """tests/golden/cg_small.npz: 5 x 6 x 4 cells of 400 x 500 x 250 m under 6 x 7 stations above the cell corners"""
    from gravinv3dhmc_amd import mesher
    g, mrange, mspacing, obs = _small()
    b6 = mesher.PrismMesh(mrange, mspacing).cell_bounds(active_only=True)
    rc, dims = detect(np.stack([np.asarray(v, dtype=np.float64) for v in obs]), b6)[:2]
    assert rc == 0 and tuple(dims) == (5, 6, 4, 6, 7)
    assert np.allclose(b6[0, 1] - b6[0, 0], 400.0) and np.allclose(b6[0, 3] - b6[0, 2], 500.0)


# ------------------------------------------------------------------------------------------------ the generator

def test_case_table_rotates_and_covers_every_pass_case():
    assert set(lc.CASE_NAMES) == set(lb.PASS_CASES)
    assert set(p[0] for p in lc.PARAMS.values()) == {1, 5, 15, 16}
    assert set(lc.PARAMS[n][1] for n in lc.CASE_NAMES) == {2, 3, 5}
    assert set(lc.PARAMS[n][2] for n in lc.CASE_NAMES) == {0.9, 0.5}
    assert lc.PARAMS[lc.BRANCH][:3] == (16, 6, 0.5)
    assert len(set(p[3] for p in lc.PARAMS.values())) == len(lc.PARAMS)


_CLAMPED = {}


@pytest.mark.parametrize("name", list(lc.CASE_NAMES) + ["big", lc.BRANCH])
def test_case_is_well_conditioned_off_its_branch_edges_and_sharp(name):
    d = lc.make(name)
    ref = d.ref
    assert (d.counts >= 0).all() and np.array_equal(d.counts, np.round(d.counts))
    assert (d.counts.sum(axis=1)[1 if name == lc.BRANCH else 0:] >= d.N).all()
    for row, _ in d.probes():
        ordinary = d.counts[1:] if name == lc.BRANCH else d.counts
        assert (ordinary[:, row] >= 1).all()
    c = lc.conditions(d, sharp=name != "big")  # (BIG: exempt from the sharpness bound, lattice_bscg_cases.py)
    _CLAMPED[name] = c["clamped"] > 0
    print("%s (%d x %d, B = %d, maxk = %d, q = %g, seed %d): float64 / longdouble spread %.2e, smallest alpha-rule margin "
          "%.2e, smallest distance from the stop threshold %.2e, clamped cells %d, probes move the oracle by %s"
          % (name, d.N, d.M, d.B, d.maxk, d.q, d.seed, c["spread"], c["margin"], c["stop"], c["clamped"],
             ", ".join("%.2e" % m for m in c["moved"])))
    assert c["spread"] <= lc.TOL_BSCG / 10, (name, c["spread"])
    assert c["margin"] >= 1e-4, (name, c["margin"])
    assert c["stop"] >= 1e-2, (name, c["stop"])
    assert name == "big" or min(c["moved"]) >= 100 * lc.TOL_BSCG, (name, c["moved"])
    if name == lc.BRANCH:
        # slot 0 freezes at k = 1 -- no misfit entry, two regularisation factors -- and every other slot runs to the end
        assert (ref.n_entries[0], ref.n_alpha[0]) == (0, 2) and ref.trace[0]["seen"][0] < lc.STOP
        assert (ref.n_entries[1:] == d.maxk - 1).all() and (ref.n_alpha[1:] == d.maxk).all()
        assert (ref.models == d.low).any() and (ref.models == d.high).any()
        c3, slots = d.group_of_three()
        three = d.run(d.Aw, c3)
        assert list(three.n_alpha) == [2, d.maxk, d.maxk]
        for v, w in zip(three.results(), ref.results()):
            assert np.array_equal(v, w[slots])  # (the oracle's replicates do not know their slot either)


def test_the_clamp_acts_in_at_least_half_the_cases():
    names = list(lc.CASE_NAMES)
    for name in names:
        if name not in _CLAMPED:
            ref = lc.make(name).ref
            _CLAMPED[name] = sum(lo + hi for tr in ref.trace for lo, hi in tr["clamped"]) > 0
    n = sum(_CLAMPED[name] for name in names)
    print("the clamp acted in %d of %d cases" % (n, len(names)))
    assert 2 * n >= len(names)
