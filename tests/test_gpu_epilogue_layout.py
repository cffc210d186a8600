"""GPU suite of the single chain's work-buffer layout (csrc/host_layout.h): the cases in which the offsets inside
StateSet::part matter most, each asserting through gh_debug_work_layout the layout it meant to reach.

Magnetization vector at 300 cells per property (3 x 10 x 10): R takes 3 ceil(300 / 256) = 6 blocks against the
ceil(900 / 256) = 4 of a single property of that many cells, the largest excess there is, and the amplitude term's 2
partials follow them -- at 2100 rows in `part` (the epilogue that leaves partials), at 600 rows in a buffer of their
own (finish_kernel).  Against the NumPy restatement (tests/magvector_host.py) at test_gpu_magvector.py's bounds:
1e-12 for the potential's values and gradient, 1e-10 for a trajectory.

Row shards set up after an evaluation: the partial sums of p'p (one per 256 cells) would outgrow the buffers sized
for the sweep's teams; the call is refused and the context stays as it was.  Set up first, the same context matches
the unsharded engine: both sum the same 2048 products per entry in another order, each good to 2048 eps / 2 in the
worst case, 2.3e-13 -- the bound is 1e-12 for the values, the prediction and the gradient."""
import ctypes as C

import numpy as np
import pytest

from helpers import relmax
from magvector_host import MagVectorProblem
from test_gpu_magvector import _data, _errs, _module, _obs

pytestmark = pytest.mark.gpu

MRANGE, MSPACING, SHAPE = (0, 2000, 0, 3000, 0, 900), (300, 300, 200), (3, 10, 10)
LAYOUT = ("allocated", "slab_rows", "slab2_rows", "pp", "pp0", "dsum", "bsum", "n_dpart", "n_regpart", "reg_blocks",
          "part_form", "part_size", "reg_at", "coupling_at", "h_scal_size", "slab_live")
PART_NONE, PART_PLAIN, PART_MVI = 0, 1, 2


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def work_layout(eng):
    from gravinv3dhmc_amd import _lib
    out = (C.c_int64 * 16)()
    assert _lib.load().gh_debug_work_layout(eng._h, out) == _lib.GH_OK
    return dict(zip(LAYOUT, out))


@pytest.mark.parametrize("lam", [0.0, 0.6], ids=["amplitude-off", "amplitude-on"])
@pytest.mark.parametrize("nx,ny", [(60, 35), (30, 20)], ids=["2100-rows-partials", "600-rows-amppart"])
def test_magnetization_vector_at_300_cells_per_property(G, nx, ny, lam):
    obs = _obs(nx, ny)
    n = obs[0].size
    dobs, _ = _data(G, obs, MRANGE, MSPACING, SHAPE, (slice(1, None), slice(3, 7), slice(3, 7)), seed=13)
    mv = _module(G, obs, dobs, MRANGE, MSPACING)
    eng = mv._engine
    assert mv.Aw.shape == (n, 900)
    Aw = np.array(eng.download_G())
    wm = mv.Wm.diagonal()
    M, amp_beta = wm.size, 0.05
    if lam > 0:
        mv.set_amplitude(lam, amp_beta)
    rng = np.random.default_rng(11)
    mwapr = 0.001 * wm
    for reg in ("TV", "MS"):
        P = MagVectorProblem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm, shape=SHAPE, lam=lam, amp_beta=amp_beta)
        x = rng.uniform(-0.02, 0.02, M) * wm
        a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        ev, eg = _errs(a, P.misfit_and_grad(x))
        print("N = %d, lambda = %g, %s: values %r, gradient %.3e" % (n, lam, reg, ev, eg))
        assert max(ev) <= 1e-12 and eg <= 1e-12, (reg, ev, eg)
        if lam > 0:
            assert abs(mv.last_amplitude - P.phi) <= 1e-12 * P.phi
    lay = work_layout(eng)
    print(lay)
    assert lay["allocated"] == 1 and lay["n_regpart"] == 6 and lay["reg_blocks"] == 2
    assert lay["n_dpart"] >= (n + 31) // 32 and lay["reg_at"] == lay["n_dpart"] and lay["coupling_at"] == lay["n_dpart"] + 6
    if n >= 2048:
        # the partials form: |r|^2, six blocks of R, two of Phi, inside n_dpart + ceil(900 / 256) + 3 + 2
        assert lay["part_form"] == PART_MVI and lay["part_size"] == lay["n_dpart"] + 4 + 3 + 2
        assert lay["coupling_at"] + 2 <= lay["part_size"] and lay["dsum"] >= lay["slab_rows"]
    else:
        assert lay["part_form"] == PART_NONE and lay["dsum"] == 0
    # one leapfrog trajectory that is accepted, with clamps on the way (the step: test_gpu_magvector.py)
    low, high = -0.02 * wm, 0.02 * wm
    dt = 0.02 if lam == 0 else min(0.02, 1.0 / np.sqrt(2.0 * lam / (amp_beta * wm.min() ** 2)))
    P = MagVectorProblem(Aw, dobs, mwapr, "TV", 1.0, 0.001, wm=wm, shape=SHAPE, lam=lam, amp_beta=amp_beta)
    eng.set_reg("TV", 1.0, 0.001, SHAPE, mwapr)
    p0 = rng.normal(size=M) * 0.3
    xg, acc, o, _ = eng.leapfrog(mwapr, p0, dt, 6, low, high, 0.0)
    xo, acco, oo = P.leapfrog(mwapr, p0, dt, 6, low, high, 0.0)
    print("trajectory: out5 %.3e, x %.3e, accepted %r" % (relmax(o, oo), relmax(xg, xo), acco))
    assert acco, ("the restatement's own trajectory is to be accepted", dt, oo[3], oo[4])
    assert np.any(xo == high) or np.any(xo == low)
    assert acc == acco and relmax(o, oo) <= 1e-10 and relmax(xg, xo) <= 1e-10
    after = work_layout(eng)
    assert {k: v for k, v in after.items() if k != "slab_live"} == {k: v for k, v in lay.items() if k != "slab_live"}
    eng.close()


def _dense_problem(seed=5, N=2048, M=1200):
    rng = np.random.default_rng(seed)
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.5, 2.0, size=M))
    return A, rng.normal(size=N) + 10.0, rng.uniform(0.0, 0.1, size=M), rng.uniform(0.0, 1.0, size=M)


def _prepared(G, A, dobs, mwapr, shard_first):
    from gravinv3dhmc_amd import _lib
    N, M = A.shape
    eng = G.Engine(N, M)
    lay = eng.sweep_layout()
    assert lay["n_teams"] == 4 and lay["n_panels"] == 1, lay           # 300 columns per team: 4 against ceil(1200 / 256) = 5
    cb = _lib.ALLREDUCE_FN(lambda user, buf, count: 0)                  # a world of one: the sum is what is there
    shard = lambda: _lib.load().gh_shard_init_rows_callback(eng._h, C.cast(cb, C.c_void_p), None, 0, 1, N, 0)
    if shard_first:
        assert shard() == _lib.GH_OK
    eng.upload_G(A)
    eng.weight(0.5)
    eng.set_data(dobs, None)
    eng.set_reg("Damping", 0.5, 0.01, (1, 1, M), mwapr)
    return eng, shard, cb


def test_row_shards_after_an_evaluation_are_refused(G, monkeypatch):
    from gravinv3dhmc_amd import _lib
    monkeypatch.setenv("GRAVHMC_MIN_COLS", "300")
    A, dobs, mwapr, x = _dense_problem()
    eng, shard, cb = _prepared(G, A, dobs, mwapr, shard_first=False)
    assert work_layout(eng)["allocated"] == 0
    d1 = eng.forward(x)
    lay = work_layout(eng)
    print(lay)
    assert lay["allocated"] == 1 and lay["pp"] == 4 and lay["pp0"] == 5 and lay["slab_rows"] == 4
    mg = eng.misfit_and_grad(x)
    assert shard() == _lib.GH_ERR_ARG
    msg = _lib.load().gh_last_error(eng._h).decode()
    print(msg)
    assert msg.startswith("gh_shard_init_rows: call before the first evaluation") and "5 partial sums" in msg
    assert np.array_equal(eng.forward(x), d1)                            # the context as it was, bit for bit
    again = eng.misfit_and_grad(x)
    assert again[0] == mg[0] and np.array_equal(again[1], mg[1]) and np.array_equal(again[2], mg[2])
    assert work_layout(eng) == lay
    eng.close()
    # set up before any evaluation: five partials from the start, and the potential of the unsharded engine
    eng, shard, cb = _prepared(G, A, dobs, mwapr, shard_first=True)
    sh = eng.misfit_and_grad(x)
    lay = work_layout(eng)
    print(lay)
    assert lay["allocated"] == 1 and lay["pp"] == 5
    assert abs(sh[0] - mg[0]) <= 1e-12 * abs(mg[0]) and relmax(sh[1], mg[1]) <= 1e-12 and relmax(sh[2], mg[2]) <= 1e-12
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(sh[3:], mg[3:]))
    eng.close()
