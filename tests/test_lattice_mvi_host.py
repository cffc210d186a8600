"""Host suite of the magnetization-vector store on the translation-invariant table (gh_set_cells_mvi_table,
csrc/latmvi.hip.h): the binding, what Engine.set_cells_mvi_data and MagVectorModule(translation_invariant=True) hand on
and refuse before an Engine exists (tests/test_lattice_multi_host.py's technique), the NumPy restatement of "the axis
is one more layer coordinate" against the expanded [A_x | A_y | A_z] stack, and the conditioning of the chains the GPU
suite runs: accepted, rejected and clamped trajectories, no Metropolis decision within 1e-6, no amplification of
rounding beyond the GPU suite's bound, and the mistakes the GPU suite must see at least 1e-6 away.  No device."""
import os
import re

import numpy as np
import pytest

import lattice_mvi_cases as C
from helpers import relmax
from lattice_cases import detect
from lattice_multi_cases import TableOperator, expand
from magvecdata_host import VecDataProblem, stack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSTORE, STORE, TABLE = "vector-data magnetization store", "magnetization-vector store", "translation-invariant table"
MRANGE, MSPACING = (0.0, 700.0, 0.0, 500.0, 0.0, 300.0), (100.0, 100.0, 100.0)


# ------------------------------------------------------------------------------------------ the binding

def test_header_declares_and_library_exports_the_entry_points():
    from gravinv3dhmc_amd import _lib
    with open(os.path.join(ROOT, "include", "gravhmc.h")) as f:
        header = f.read()
    assert re.search(r"int gh_set_cells_mvi_table\(gh_ctx \*ctx, const double \*bounds6, double fx, double fy, double fz, "
                     r"int ncomp, const int \*comps,\s+const double \*weights\);", header)
    assert "int gh_translation_invariant_axes(const gh_ctx *ctx, int *axes, int *chunks, int *layers_per_chunk);" in header
    assert _lib.PROTOTYPES["gh_set_cells_mvi_table"] == _lib.PROTOTYPES["gh_set_cells_mvi_data"]
    lib = _lib.load()
    assert lib.gh_set_cells_mvi_table and lib.gh_translation_invariant_axes


class _RecorderLib:
    """stands in for the loaded library: every call is recorded and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


@pytest.mark.parametrize("table", [False, True])
def test_engine_hands_the_keyword_to_the_entry_point(table):
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.engine import Engine, Store
    eng = Engine.__new__(Engine)
    eng._lib, eng._h, eng.N, eng.M, eng._store = _RecorderLib(), None, 12, 9, Store(None, 1, 1, False)
    eng.set_cells_mvi_data(np.zeros((3, 6)), (0.0, 0.6, 0.8), ("tf",), np.ones(1), translation_invariant=table)
    assert eng._lib.calls == ["gh_set_cells_mvi_table" if table else "gh_set_cells_mvi_data"]
    assert getattr(eng, "_translation_invariant", False) is table
    # (on the table the unweighted total field is a store of one block as well: the table has no other door)
    assert eng._store.kind == (_lib.CELL_PRISM_MVI_DATA if table else _lib.CELL_PRISM_MVI) and eng.mvi
    assert bool(eng.multi) is table
    eng._h = None


# ------------------------------------------------------------------------------------------ the module

class _Reached(Exception):
    """raised by the engine's stand-in: the constructor got to its device work"""


class _FakeEngine:
    calls = []

    def __init__(self, N, M, device=0):
        _FakeEngine.calls.append(("Engine", N, M))

    def set_cells_mvi(self, bounds, direction):
        _FakeEngine.calls.append(("set_cells_mvi",))
        raise _Reached()

    def set_cells_mvi_data(self, bounds, direction, components, weights, translation_invariant=False):
        _FakeEngine.calls.append(("set_cells_mvi_data", tuple(components), translation_invariant))
        raise _Reached()


@pytest.fixture()
def magvector(monkeypatch):
    from gravinv3dhmc_amd.inversion import magvector as m
    _FakeEngine.calls = []
    monkeypatch.setattr(m, "Engine", _FakeEngine)
    return m


def _centres(nx, ny, h=100.0):
    xp, yp = [a.ravel() for a in np.meshgrid((np.arange(nx) + 0.5) * h, (np.arange(ny) + 0.5) * h, indexing="ij")]
    return xp, yp, np.full(xp.size, -20.0)


def _make(m, data=("tf",), obs=None, mrange=MRANGE, **kw):
    obs = _centres(5, 7) if obs is None else obs
    n = obs[0].size
    dobs = [np.arange(n, dtype=float) + k * k for k in range(len(data))]
    if data == ("tf",) and "weights" not in kw:
        dobs = dobs[0]
    return m.MagVectorModule(dobs, mrange, MSPACING, obs, mangle=(C.INC, C.DEC), data=data, verbose=False, **kw)


@pytest.mark.parametrize("data", [("tf",), ("bx", "by", "bz")])
def test_module_hands_the_keyword_on(magvector, data):
    with pytest.raises(_Reached):
        _make(magvector, data=data, translation_invariant=True)
    assert _FakeEngine.calls == [("Engine", len(data) * 35, 3 * 105), ("set_cells_mvi_data", data, True)]
    _FakeEngine.calls = []
    with pytest.raises(_Reached):
        _make(magvector, data=data)
    assert _FakeEngine.calls[1] == (("set_cells_mvi",) if data == ("tf",) else ("set_cells_mvi_data", data, False))


@pytest.mark.parametrize("data", [("tf",), ("bx", "by", "bz")])
def test_more_than_16384_rows_reach_the_engine_on_the_table_alone(magvector, data):
    obs, mrange = _centres(130, 130), (0.0, 13000.0, 0.0, 13000.0, 0.0, 100.0)
    with pytest.raises(_Reached):
        _make(magvector, data=data, obs=obs, mrange=mrange, translation_invariant=True)
    assert _FakeEngine.calls[0] == ("Engine", len(data) * 16900, 3 * 16900)
    _FakeEngine.calls = []
    with pytest.raises(NotImplementedError, match="takes at most 16384"):
        _make(magvector, data=data, obs=obs, mrange=mrange)
    assert _FakeEngine.calls == []


@pytest.mark.parametrize("data", [("tf",), ("bx", "by", "bz")])
@pytest.mark.parametrize("kw", [dict(mtopo=_centres(2, 2)), dict(wavelet="1D"), dict(matrix_free=True),
                                dict(shift_invariant=True), dict(shard=object()), dict(coordinate="spherical"),
                                dict(translation_invariant="chains")],
                         ids=["mtopo", "wavelet", "matrix_free", "shift_invariant", "shard", "spherical", "chains"])
def test_refusals_on_the_table_come_before_device_work(magvector, kw, data):
    kw = dict(dict(translation_invariant=True), **kw)
    with pytest.raises(NotImplementedError, match=STORE if data == ("tf",) else VSTORE) as e:
        _make(magvector, data=data, **kw)
    assert TABLE in str(e.value) and _FakeEngine.calls == []


def test_the_ladder_on_the_table_keeps_the_multi_component_modules_order(magvector):
    with pytest.raises(ValueError, match="translation_invariant"):
        _make(magvector, translation_invariant="batches")
    with pytest.raises(ValueError, match="coordinate"):
        _make(magvector, translation_invariant=True, coordinate="polar")
    with pytest.raises(TypeError, match="topo"):
        _make(magvector, translation_invariant=True, topo=None)
    with pytest.raises(NotImplementedError, match="spherical"):        # (the coordinate, then the rest in order)
        _make(magvector, translation_invariant=True, coordinate="spherical", wavelet="1D")
    with pytest.raises(NotImplementedError, match="wavelet"):
        _make(magvector, translation_invariant=True, wavelet="1D", matrix_free=True)
    with pytest.raises(NotImplementedError, match="matrix_free"):
        _make(magvector, translation_invariant=True, matrix_free=True, shift_invariant=True)
    with pytest.raises(NotImplementedError, match="shift_invariant"):
        _make(magvector, translation_invariant=True, shift_invariant=True, shard=object())
    with pytest.raises(NotImplementedError, match="shard"):
        _make(magvector, translation_invariant=True, shard=object(), mtopo=_centres(2, 2))
    with pytest.raises(NotImplementedError, match="mtopo"):
        _make(magvector, translation_invariant="chains", mtopo=_centres(2, 2))
    assert _FakeEngine.calls == []


def test_batch_refusal_text_is_the_vector_stores_own():
    """the rows of the magnetization-vector stores come before the table's: the text HMCSampleBatch has"""
    from gravinv3dhmc_amd.inversion import hmc

    class _Eng:
        multi, mvi, joint, tess_mag, tess_multi = 1, True, False, False, False
        _translation_invariant = True

    class _Model:
        _engine = _Eng()

    with pytest.raises(NotImplementedError) as e:
        hmc.HMCSampleBatch(_Model(), 2, 1, 1, 0.1, (1, 2), None, None, None, "mandatory", 1.0, None, False, 1.0, 1.0,
                           "Damping", 0.01, 1, None)
    assert str(e.value) == ("HMCSampleBatch does not run the vector-data magnetization store (MagVectorModule with "
                            "data=): sample its chains one at a time with HMCSample")


# ------------------------------------------------------------------------- the restatement: the axis as a layer

RESTATED = sorted(set(C.FILL_SHAPES) | {e[0] for e in C.EDGE_CASES})


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", RESTATED)
def test_axis_as_layer_is_the_expanded_stack(name, nb):
    obs, b6 = C.shape(name)
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    n, m = px * qy, nx * ny * nz
    rng = np.random.default_rng(3)
    T = rng.normal(size=(nb, 3 * nz, nx + px - 1, ny + qy - 1))     # (random tables: nothing of the field is used)
    for w in (np.ones(nb), np.array((2.0, 0.125, 3.0))[:nb]):
        op = TableOperator(list(T), w, (nx, ny, 3 * nz, px, qy), C.axis_maps(col, m), ool)
        # the reference: [A_x | A_y | A_z] of every block, expanded layer by layer on the geometry's own maps
        A = np.vstack([np.hstack([expand(T[b, ax * nz:(ax + 1) * nz], dims, col, ool) for ax in range(3)]) for b in range(nb)])
        Wb = np.repeat(w, n)[:, None]
        wm = np.sqrt(((Wb * A) ** 2).sum(axis=0))
        Aw = Wb * A / wm[None, :]
        x, r = rng.normal(size=3 * m), rng.normal(size=nb * n)
        assert op.shape == (nb * n, 3 * m)
        assert relmax(op.wm, wm) <= 1e-12
        assert relmax(op @ x, Aw @ x) <= 1e-12 and relmax(op.T @ r, Aw.T @ r) <= 1e-12


def test_axis_tables_expand_to_the_host_kernels():
    """axis_tables and expand_axes are each other's inverse on a translation-invariant kernel"""
    obs, b6 = C.shape("shuffled")
    K = C.host_blocks(obs, b6, C.direction())
    for c in ("tf", "by"):
        assert relmax(C.expand_axes(C.axis_tables(K[c], obs, b6), obs, b6), K[c]) <= 1e-12


# ------------------------------------------------------------------------------------------ the chains' cases

_K = {}


def host_kernels(case):
    if case not in _K:
        obs, b6 = C.shape(C.CHAIN_CASES[case][0])
        _K[case] = C.host_blocks(obs, b6, C.direction())
    return _K[case]


def _run(P, x0, trajs, dt, low, high):
    out = P.chain(x0, trajs, dt, low, high)
    accepted = sum(bool(a) for a, _, _ in out)
    clamps = sum(int(a and (np.any(x == low) or np.any(x == high))) for a, _, x in out)
    margin = min(abs(np.log(u) + (o[4] - o[3])) for (_, _, u), (_, o, _) in zip(trajs, out))
    return out, accepted, clamps, margin


@pytest.mark.parametrize("lam", [0.0, C.LAMBDA], ids=["plain", "amplitude"])
@pytest.mark.parametrize("reg", C.REGS)
@pytest.mark.parametrize("case", sorted(C.CHAIN_CASES))
def test_chain_cases_accept_reject_clamp_and_decide_clearly(case, reg, lam):
    w, wm, dobsw, shape3, P, low, high, x0, trajs, xt, dt = C.chain_case(host_kernels(case), case, reg, lam)
    _, accepted, clamps, margin = _run(P, x0, trajs, dt, low, high)
    print(case, reg, lam, "accepted", accepted, "clamped", clamps, "margin", margin)
    assert 0 < accepted < len(trajs) and clamps > 0
    assert margin >= 1e-6
    # ... and do not amplify rounding beyond the bound the GPU suite compares states with (1e-10)
    rng = np.random.default_rng(1)
    K2 = {c: k * (1.0 + 1e-15 * rng.normal(size=k.shape)) for c, k in host_kernels(case).items()}
    P2 = C.chain_case(K2, case, reg, lam)[4]
    moved = max(relmax(b[2], a[2]) for a, b in zip(_run(P, x0, trajs, dt, low, high)[0], _run(P2, x0, trajs, dt, low, high)[0]))
    print(case, reg, lam, "entries perturbed by 1e-15 move a state by", moved)
    assert moved <= 1e-11


@pytest.mark.parametrize("case", sorted(C.CHAIN_CASES))
def test_wrong_models_lie_far_from_the_right_one(case):
    data = C.CHAIN_CASES[case][1]
    K = host_kernels(case)
    w, wm, dobsw, shape3, P, low, high, x0, trajs, xt, dt = C.chain_case(K, case, "Damping", 0.0)
    right, _, _, _ = _run(P, x0, trajs, dt, low, high)
    U = P.misfit_and_grad(xt)[0]
    wrong = C.wrong_kernels(K, data)
    assert len(wrong) == (3 if "bx" in data and "by" in data else 2)
    for name, Kw in wrong.items():
        Aw2, wm2, _, _ = stack(Kw, data, w)
        Pw = VecDataProblem(Aw2, dobsw, len(data), 0.01 * wm, "Damping", 1.0, 0.01, wm=wm2, shape=shape3)
        out, _, _, _ = _run(Pw, x0, trajs, dt, low, high)
        dU = abs(Pw.misfit_and_grad(xt)[0] - U) / abs(U)
        dx = relmax(out[-1][2], right[-1][2])
        print(case, name, "potential", dU, "state", dx)
        assert dU >= 1e-6 and dx >= 1e-6
