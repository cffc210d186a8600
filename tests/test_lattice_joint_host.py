"""Host suite of the joint gravity-magnetic store on the translation-invariant table (gh_set_cells_joint_table,
csrc/latjoint.hip.h): the binding, what Engine.set_cells and JointModule(translation_invariant=True) hand on and refuse
before an Engine exists, the forward's plan restated for 256 compute units (a chunking that ignores the boundary between
the properties puts layers of both into one chunk of the large shape; the joint store's does not), the conditioning of
the chains the GPU suite runs -- accepted, rejected and clamped trajectories, no Metropolis decision within 1e-6, no
amplification of rounding beyond the GPU suite's bound -- and the mistakes the GPU suite must see at least 1e-6 away.
No device."""
import os
import re

import numpy as np
import pytest

import lattice_joint_cases as C
from helpers import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSTORE = "the joint store on the translation-invariant table"
MRANGE, MSPACING = (0.0, 700.0, 0.0, 500.0, 0.0, 300.0), (100.0, 100.0, 100.0)


# ------------------------------------------------------------------------------------------ the binding

def test_header_declares_and_library_exports_the_entry_point():
    from gravinv3dhmc_amd import _lib
    with open(os.path.join(ROOT, "include", "gravhmc.h")) as f:
        header = f.read()
    assert "int gh_set_cells_joint_table(gh_ctx *ctx, const double *bounds6, double fx, double fy, double fz);" in header
    assert re.search(r"gh_set_cells_joint_table context: T\[2\]\[nz\]", header)
    assert _lib.PROTOTYPES["gh_set_cells_joint_table"] == _lib.PROTOTYPES["gh_set_cells_joint"]
    lib = _lib.load()
    assert lib.gh_set_cells_joint_table


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
    eng._lib, eng._h, eng.N, eng.M, eng._store = _RecorderLib(), None, 12, 6, Store(None, 1, 1, False)
    eng.set_cells(np.zeros((3, 6)), _lib.CELL_PRISM_JOINT, direction=(0.0, 0.6, 0.8), translation_invariant=table)
    assert eng._lib.calls == ["gh_set_cells_joint_table" if table else "gh_set_cells_joint"]
    assert getattr(eng, "_translation_invariant", False) is table
    assert eng._store.kind == _lib.CELL_PRISM_JOINT and eng.joint and not eng.multi
    eng._h = None


def test_engine_keeps_the_door_for_the_joint_store():
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.engine import Engine, Store
    eng = Engine.__new__(Engine)
    eng._lib, eng._h, eng.N, eng.M, eng._store = _RecorderLib(), None, 12, 6, Store(None, 1, 1, False)
    with pytest.raises(ValueError, match="translation_invariant"):
        eng.set_cells(np.zeros((6, 6)), _lib.CELL_PRISM, translation_invariant=True)
    with pytest.raises(ValueError, match="translation_invariant"):
        eng.set_cells(np.zeros((3, 6)), _lib.CELL_PRISM_JOINT, direction=(0.0, 0.6, 0.8), translation_invariant="chains")
    assert eng._lib.calls == []
    eng._h = None


# ------------------------------------------------------------------------------------------ the module

class _Reached(Exception):
    """raised by the engine's stand-in: the constructor got to its device work"""


class _FakeEngine:
    calls = []

    def __init__(self, N, M, device=0):
        _FakeEngine.calls.append(("Engine", N, M))

    def set_cells(self, bounds, kind, **kw):
        _FakeEngine.calls.append(("set_cells", kind, kw.get("translation_invariant", False)))
        raise _Reached()


@pytest.fixture()
def joint(monkeypatch):
    from gravinv3dhmc_amd.inversion import joint as m
    _FakeEngine.calls = []
    monkeypatch.setattr(m, "Engine", _FakeEngine)
    return m


def _centres(nx, ny, h=100.0):
    xp, yp = [a.ravel() for a in np.meshgrid((np.arange(nx) + 0.5) * h, (np.arange(ny) + 0.5) * h, indexing="ij")]
    return xp, yp, np.full(xp.size, -20.0)


def _make(m, obs=None, mrange=MRANGE, **kw):
    obs = _centres(5, 7) if obs is None else obs
    n = obs[0].size
    return m.JointModule(np.arange(n, dtype=float), np.arange(n, dtype=float) ** 2, mrange, MSPACING, obs,
                         mangle=(C.INC, C.DEC), verbose=False, **kw)


def test_module_hands_the_keyword_on(joint):
    from gravinv3dhmc_amd import _lib
    with pytest.raises(_Reached):
        _make(joint, translation_invariant=True)
    assert _FakeEngine.calls == [("Engine", 70, 210), ("set_cells", _lib.CELL_PRISM_JOINT, True)]
    _FakeEngine.calls = []
    with pytest.raises(_Reached):
        _make(joint)
    assert _FakeEngine.calls == [("Engine", 70, 210), ("set_cells", _lib.CELL_PRISM_JOINT, False)]


def test_more_than_16384_points_reach_the_engine(joint):
    """no limit on the host: the dense store's is the library's own (gh_set_cells_joint), the table has none"""
    obs, mrange = _centres(130, 130), (0.0, 13000.0, 0.0, 13000.0, 0.0, 100.0)
    with pytest.raises(_Reached):
        _make(joint, obs=obs, mrange=mrange, translation_invariant=True)
    assert _FakeEngine.calls[0] == ("Engine", 2 * 16900, 2 * 16900)


@pytest.mark.parametrize("kw", [dict(mtopo=_centres(2, 2)), dict(translation_invariant="chains")], ids=["mtopo", "chains"])
def test_refusals_on_the_table_come_before_device_work(joint, kw):
    kw = dict(dict(translation_invariant=True), **kw)
    with pytest.raises(NotImplementedError, match=TSTORE):
        _make(joint, **kw)
    assert _FakeEngine.calls == []


def test_the_existing_refusals_stay_first(joint):
    with pytest.raises(NotImplementedError, match="spherical"):
        _make(joint, translation_invariant="chains", coordinate="spherical")
    with pytest.raises(NotImplementedError, match="wavelet"):
        _make(joint, translation_invariant="chains", wavelet="1D")
    obs = _centres(5, 7)
    with pytest.raises(ValueError, match="same length"):
        joint.JointModule(np.zeros(35), np.zeros(34), MRANGE, MSPACING, obs, verbose=False, translation_invariant="chains")
    with pytest.raises(ValueError, match="translation_invariant"):
        _make(joint, translation_invariant="batches")
    assert _FakeEngine.calls == []


def test_batch_refusal_names_the_store_on_the_table():
    from gravinv3dhmc_amd.inversion import hmc

    class _Eng:
        joint, multi, mvi, tess_mag, tess_multi = True, 0, False, False, False
        _translation_invariant = True

    class _Model:
        _engine = _Eng()

    def batch():
        hmc.HMCSampleBatch(_Model(), 2, 1, 1, 0.1, (1, 2), None, None, None, "mandatory", 1.0, None, False, 1.0, 1.0,
                           "Damping", 0.01, 1, None)

    with pytest.raises(NotImplementedError, match=TSTORE):
        batch()
    _Eng._translation_invariant = False          # (the dense module: the text it always had)
    with pytest.raises(NotImplementedError) as e:
        batch()
    assert str(e.value) == ("HMCSampleBatch does not run the joint gravity-magnetic kernel (JointModule): sample its "
                            "chains one at a time with HMCSample")


# ------------------------------------------------------------------------------------------ the forward's plan

def test_the_large_shapes_chunks_would_cross_the_boundary_on_256_cus():
    cells, obs = C.SHAPES[C.BIG]["cells"], C.SHAPES[C.BIG]["obs"]
    nz = cells[2]
    lpc, plain, joint = C.forward_plan(cells, obs, 256)
    # the formula every table has: 2 layers per chunk, and 21 is odd -- layers 20 (gz) and 21 (tf) in one chunk
    assert lpc == 2 and [20, 21] in plain
    assert any(len({L // nz for L in c}) == 2 for c in plain)
    # the joint store's: the same layers per chunk, cut per property, the same number of chunks each
    assert len(joint) % 2 == 0 and max(len(c) for c in joint) == lpc
    half = len(joint) // 2
    assert all({L // nz for L in c} == {0} for c in joint[:half]) and all({L // nz for L in c} == {1} for c in joint[half:])
    assert sorted(L for c in joint for L in c) == list(range(2 * nz))
    assert 2 * obs[0] * obs[1] > 2 * 16384


@pytest.mark.parametrize("cus", [1, 8, 64, 104, 256, 304])
@pytest.mark.parametrize("name", sorted(C.SHAPES))
def test_the_joint_plan_never_crosses_and_covers_every_layer(name, cus):
    cells, obs = C.SHAPES[name]["cells"], C.SHAPES[name]["obs"]
    nz = cells[2]
    _, _, joint = C.forward_plan(cells, obs, cus)
    half = len(joint) // 2
    assert len(joint) == 2 * half and all(len(c) > 0 for c in joint)
    assert all(max(c) < nz for c in joint[:half]) and all(min(c) >= nz for c in joint[half:])
    assert sorted(L for c in joint for L in c) == list(range(2 * nz))


# ------------------------------------------------------------------------------------------ the restatement

_K = {}


def host_kernels(name):
    if name not in _K:
        obs, b6 = C.shape(name)
        _K[name] = C.host_kernels(obs, b6)
        for k in _K[name]:
            k.setflags(write=False)
    return _K[name]


def test_host_gz_is_the_oracles():
    from oracle import oracle
    obs, b6 = C.shape("shuffled 4,5,3 / 6,7")
    assert relmax(host_kernels("shuffled 4,5,3 / 6,7")[0], oracle.prism_gz_kernel(obs[0], obs[1], obs[2], b6)) <= 1e-12


@pytest.mark.parametrize("name", C.SMALL)
def test_block_operator_is_the_stacked_store(name):
    op = C.Blocks(*host_kernels(name))
    A = np.asarray(op)
    rng = np.random.default_rng(3)
    x, r = rng.normal(size=2 * op.m), rng.normal(size=2 * op.n)
    assert op.shape == A.shape == (2 * op.n, 2 * op.m) and op.T.shape == (2 * op.m, 2 * op.n)
    assert relmax(op @ x, A @ x) <= 1e-12 and relmax(op.T @ r, A.T @ r) <= 1e-12
    _, _, dobsw, xt = C.case_data(op)
    assert relmax(C.gradient(op, xt, dobsw), 2.0 * (A.T @ (A @ xt - dobsw))) <= 1e-12


# ------------------------------------------------------------------------------------------ sharpness

@pytest.mark.parametrize("name", C.SMALL)
def test_wrong_passes_lie_far_from_the_right_one(name):
    op = C.Blocks(*host_kernels(name))
    _, _, dobsw, xt = C.case_data(op)
    g = C.gradient(op, xt, dobsw)
    for mistake in C.MISTAKES:
        d = relmax(C.gradient(op, xt, dobsw, mistake), g)
        print(name, mistake, d)
        assert d > 1e-6


def test_a_chunk_summed_across_the_boundary_lies_far_from_the_right_one():
    op = C.Blocks(*host_kernels(C.BIG))
    _, _, dobsw, xt = C.case_data(op)
    nz = C.SHAPES[C.BIG]["cells"][2]
    _, plain, _ = C.forward_plan(C.SHAPES[C.BIG]["cells"], C.SHAPES[C.BIG]["obs"], 256)
    crossing = [c for c in plain if len({L // nz for L in c}) == 2]
    assert crossing == [[nz - 1, nz]]
    d = relmax(C.gradient(op, xt, dobsw, across=(nz, nz - 1)), C.gradient(op, xt, dobsw))
    print("layer", nz - 1, "of the density summed into the tf rows:", d)
    assert d > 1e-6


# ------------------------------------------------------------------------------------------ the chains' cases

@pytest.mark.parametrize("lam", [0.0, C.LAMBDA], ids=["plain", "cross-gradient"])
@pytest.mark.parametrize("reg", C.REGS)
@pytest.mark.parametrize("name", C.CHAIN_SHAPES)
def test_chain_cases_accept_reject_clamp_and_decide_clearly(name, reg, lam):
    K = host_kernels(name)
    op, dobsw, P, low, high, x0, trajs, xt, dt = C.chain_case(K, name, reg, lam)
    out, accepted, clamps, margin = C.run_chain(P, x0, trajs, dt, low, high)
    print(name, reg, lam, "accepted", accepted, "clamped", clamps, "margin", margin)
    assert [t[0] for t in trajs] == [2, 3, 4, 5, 6, 2, 3, 4, 5, 6]
    assert 0 < accepted < len(trajs) and clamps > 0
    assert margin >= 1e-6
    if lam > 0:
        assert max(o[3] for o in out) > 0.0         # (the coupling is in the potential)
    # ... and do not amplify rounding beyond the bound the GPU suite compares states with (1e-10)
    rng = np.random.default_rng(1)
    K2 = tuple(k * (1.0 + 1e-15 * rng.normal(size=k.shape)) for k in K)
    P2 = C.chain_case(K2, name, reg, lam)[2]
    out2 = C.run_chain(P2, x0, trajs, dt, low, high)[0]
    moved = max(relmax(b[2], a[2]) for a, b in zip(out, out2))
    print(name, reg, lam, "entries perturbed by 1e-15 move a state by", moved)
    assert moved <= 1e-11
