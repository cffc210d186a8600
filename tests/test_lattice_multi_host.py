"""Host suite of the multi-component store on the translation-invariant table: what MultiComponentModule(
translation_invariant=True) decides before an Engine exists (tests/test_module_layer_host.py's technique: the name the
module's file has for the engine is replaced, so the first device call is seen), that the existing ladder keeps its
recorded texts with translation_invariant=False, the binding of gh_set_cells_multi_table, and the suite's own host-side
operator (lattice_multi_cases.TableOperator) against the expanded tables.  No device."""
import json
import os

import numpy as np
import pytest

import module_layer_cases as cases
from conftest import GOLD
from lattice_cases import detect, geometry
from lattice_multi_cases import TableOperator, expand
from multicomp_host import stack

STORE, TABLE = "multi-component store", "translation-invariant"
MRANGE, MSPACING = (0.0, 700.0, 0.0, 500.0, 0.0, 300.0), (100.0, 100.0, 100.0)


class _Reached(Exception):
    """raised by the engine's stand-in: the constructor got to its device work"""


class _FakeEngine:
    calls = []

    def __init__(self, N, M, device=0):
        self.N, self.M = N, M
        _FakeEngine.calls.append(("Engine", N, M))

    def set_cells_multi(self, bounds, components, weights, translation_invariant=False):
        _FakeEngine.calls.append(("set_cells_multi", tuple(components), bool(translation_invariant)))
        raise _Reached()


@pytest.fixture()
def multicomp(monkeypatch):
    from gravinv3dhmc_amd.inversion import multicomp as m
    _FakeEngine.calls = []
    monkeypatch.setattr(m, "Engine", _FakeEngine)
    return m


def _centres(nx, ny, h=100.0):
    xp, yp = [a.ravel() for a in np.meshgrid((np.arange(nx) + 0.5) * h, (np.arange(ny) + 0.5) * h, indexing="ij")]
    return xp, yp, np.full(xp.size, -20.0)


def _make(m, n_obs=None, obs=None, comps=("gz", "gzz"), mrange=MRANGE, **kw):
    obs = _centres(5, 7) if obs is None else obs      # (the mesher's x runs over mrange's second pair)
    n = obs[0].size
    dobs = [np.arange(n, dtype=float) + k * k for k in range(len(comps))]
    return m.MultiComponentModule(dobs, mrange, MSPACING, obs, components=comps, verbose=False, **kw)


def test_lib_declares_the_entry_point():
    from gravinv3dhmc_amd import _lib
    assert "gh_set_cells_multi_table" in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["gh_set_cells_multi_table"] == _lib.PROTOTYPES["gh_set_cells_multi"]


@pytest.mark.parametrize("kw", [dict(wavelet="1D"), dict(wavelet="3D"), dict(matrix_free=True), dict(shift_invariant=True),
                                dict(shard=object()), dict(mtopo=_centres(2, 2)), dict(coordinate="spherical")],
                         ids=["wavelet1D", "wavelet3D", "matrix_free", "shift_invariant", "shard", "mtopo", "spherical"])
def test_refusals_on_the_table_come_before_device_work(multicomp, kw):
    with pytest.raises(NotImplementedError, match=STORE) as e:
        _make(multicomp, translation_invariant=True, **kw)
    assert TABLE in str(e.value) and _FakeEngine.calls == []


def test_the_ladder_on_the_table_keeps_the_parsers_order(multicomp):
    with pytest.raises(ValueError, match="coordinate"):
        _make(multicomp, translation_invariant=True, coordinate="polar")
    with pytest.raises(TypeError, match="topo"):
        _make(multicomp, translation_invariant=True, topo=None)
    with pytest.raises(ValueError, match="must be one of"):            # (the data parser first, as without the table)
        _make(multicomp, translation_invariant=True, comps=("gz", "gzx"), wavelet="1D")
    with pytest.raises(NotImplementedError, match="spherical"):        # (then the coordinate, then the rest in order)
        _make(multicomp, translation_invariant=True, coordinate="spherical", wavelet="1D")
    with pytest.raises(NotImplementedError, match="wavelet"):
        _make(multicomp, translation_invariant=True, wavelet="1D", matrix_free=True)
    assert _FakeEngine.calls == []


def test_20000_rows_pass_the_ladder_and_reach_the_engine(multicomp):
    obs = _centres(100, 100)
    mrange = (0.0, 10000.0, 0.0, 10000.0, 0.0, 100.0)
    with pytest.raises(_Reached):
        _make(multicomp, obs=obs, mrange=mrange, translation_invariant=True)
    assert _FakeEngine.calls == [("Engine", 20000, 10000), ("set_cells_multi", ("gz", "gzz"), True)]
    # the dense form refuses them before device work, and -- the data being gridded on the mesh -- points at the table
    _FakeEngine.calls = []
    with pytest.raises(NotImplementedError, match="16384") as e:
        _make(multicomp, obs=obs, mrange=mrange)
    assert "translation_invariant=True has no such limit" in str(e.value) and STORE in str(e.value)
    assert _FakeEngine.calls == []
    # ... and not where the geometry has no table: points L / (n - 1) apart, or a carved mesh
    lin = [a.ravel() for a in np.meshgrid(np.linspace(0, 10000, 100), np.linspace(0, 10000, 100), indexing="ij")]
    for kw in (dict(obs=(lin[0], lin[1], np.zeros(10000))), dict(obs=obs, mtopo=_centres(2, 2))):
        with pytest.raises(NotImplementedError, match="16384") as e:
            _make(multicomp, mrange=mrange, **kw)
        assert "translation_invariant" not in str(e.value)


def test_within_the_limit_both_forms_reach_the_engine(multicomp):
    for ti in (False, True):
        _FakeEngine.calls = []
        with pytest.raises(_Reached):
            _make(multicomp, translation_invariant=ti)
        assert _FakeEngine.calls == [("Engine", 70, 105), ("set_cells_multi", ("gz", "gzz"), ti)]


def test_the_existing_ladder_keeps_its_recorded_texts():
    """translation_invariant=False given by name: every recorded host case of the multi-component module, exactly"""
    from gravinv3dhmc_amd.inversion import MultiComponentModule
    with open(os.path.join(GOLD, "module_layer.json")) as f:
        golden = json.load(f)["host"]

    class Explicit(MultiComponentModule):
        def __init__(self, *a, **kw):
            super().__init__(*a, translation_invariant=False, **kw)

    seen = 0
    for name, thunk in cases.host_cases():
        if not name.startswith("multi."):
            continue
        cls, args, kw = _case_of(thunk)
        assert cls is MultiComponentModule
        try:
            Explicit(*args, **kw)
            got = "no exception"
        except Exception as e:  # noqa: BLE001 (the recorded cases raise ValueError, TypeError, NotImplementedError)
            got = "%s: %s" % (type(e).__name__, e)
        assert got == golden[name], name
        seen += 1
    assert seen >= 20


def _case_of(thunk):
    """(class, args, keywords) of a host case's thunk `lambda: cls(*args, **kw)`"""
    cells = dict(zip(thunk.__code__.co_freevars, (c.cell_contents for c in thunk.__closure__)))
    return cells["cls"], cells["args"], dict(cells["kw"])


def test_table_operator_is_the_expanded_stack():
    """the GPU suite's host-side operator (FFT convolutions of the tables' layers) against the dense expansion"""
    rng = np.random.default_rng(2)
    obs, b6 = geometry(cells=(3, 5, 2), obs=(4, 6), first=(-1, 1), shuffle=4)
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    tables = [rng.normal(size=(nz, nx + px - 1, ny + qy - 1)) for _ in range(3)]
    w = np.array([2.0, 1.0, 0.125])
    Aw, wm, _ = stack([expand(T, dims, col, ool) for T in tables], w)
    op = TableOperator(tables, w, dims, col, ool)
    assert op.shape == Aw.shape and op.T.shape == Aw.T.shape
    assert np.abs(op.wm - wm).max() <= 1e-13 * wm.max()
    x, r = rng.normal(size=Aw.shape[1]), rng.normal(size=Aw.shape[0])
    assert np.abs(op @ x - Aw @ x).max() <= 1e-13 * np.abs(Aw @ x).max()
    assert np.abs(op.T @ r - Aw.T @ r).max() <= 1e-13 * np.abs(Aw.T @ r).max()
