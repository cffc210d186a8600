"""The trajectory feeder's drawer and queue without a GPU: gh_debug_feed_dry_run runs them with a host stub in
place of the runner, and np.random.RandomState(seed), run by hand in the reference's order, is what it must
reproduce bit for bit -- L, u, the probed entries of every momentum, the look-ahead, and the generator's state
after exactly the bounded number of draws."""
import ctypes as C

import numpy as np
import pytest

from gravinv3dhmc_amd import _lib
from gravinv3dhmc_amd.inversion.rng import LegacyDraws


def _by_hand(seed, M, n, Lrange, plan, sigma):
    rs = np.random.RandomState(seed)
    rows = []
    for k in range(n):
        L = plan[k] if plan is not None else rs.randint(Lrange[0], Lrange[1] + 1)
        p0 = rs.randn(M) * sigma
        u = rs.rand()
        # (np.cumsum adds in order, as the stub does)
        rows.append((int(L), float(u), p0[0], p0[M // 2], p0[M - 1], np.cumsum(p0)[-1]))
    return rows, rs.get_state()


def _dry_run(draws, M, rows, n):
    lib = _lib.load()
    Ls, look = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    us, probe = np.zeros(n), np.zeros((n, 4))
    n_out, drawn = C.c_int64(-1), C.c_int64(-1)
    ip = C.POINTER(C.c_int)
    rc = lib.gh_debug_feed_dry_run(*draws.feed_args(), M, rows, n, Ls.ctypes.data_as(ip), _lib.ptr(us), _lib.ptr(probe),
                                   look.ctypes.data_as(ip), C.byref(n_out), C.byref(drawn))
    assert rc == 0
    draws.feed_drew(drawn.value)
    return Ls, us, probe, look, n_out.value, drawn.value


@pytest.mark.parametrize("sigma_kind", ["scalar", "vector"])
@pytest.mark.parametrize("stream", ["lrange", "plan"])
@pytest.mark.parametrize("M", [1, 2, 7, 50001])
def test_dry_run_is_the_legacy_stream(built_lib, M, stream, sigma_kind):
    seed, n, rows = 1234 + M, 7, 3
    Lrange = (5, 20)
    plan = [3, 1, 18, 7, 2, 11, 5] if stream == "plan" else None
    sigma = 0.37 if sigma_kind == "scalar" else 0.05 + np.linspace(0.0, 1.0, M) ** 2
    want, state = _by_hand(seed, M, n, Lrange, plan, sigma)
    draws = LegacyDraws(M, Lrange, sigma, fixed_L=plan, limit=None if plan is not None else n, seed=seed)
    try:
        Ls, us, probe, look, n_out, drawn = _dry_run(draws, M, rows, n)
        assert n_out == n and drawn == n
        for k in range(n):
            got = (int(Ls[k]), float(us[k])) + tuple(probe[k])
            assert got == want[k], (k, got, want[k])
        # the look-ahead was handed over for every trajectory but the last
        assert look.tolist() == [1] * (n - 1) + [0]
        # the stream is used up: nothing more is drawn
        assert len(draws.take_block(1)[0]) == 0
        # the generator stands where the hand-run one stands after exactly n trajectories
        key = np.zeros(624, dtype=np.uint32)
        pos, has_gauss, cached = C.c_int(), C.c_int(), C.c_double()
        draws._lib.gh_rng_get_state(draws._h, key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos), C.byref(has_gauss),
                                    C.byref(cached))
        assert np.array_equal(key, state[1]) and pos.value == state[2]
        assert has_gauss.value == state[3] and (not state[3] or cached.value == state[4])
    finally:
        draws.release()


def test_global_stream_goes_back_to_numpy_after_release(built_lib):
    """Adopted from np.random, drawn by the feeder's drawer, handed back: np.random continues where a hand-run
    generator stands after exactly the bounded number of trajectories."""
    M, n = 7, 5
    np.random.seed(99)
    want, state = _by_hand(99, M, n, (5, 20), None, 0.5)
    draws = LegacyDraws(M, (5, 20), 0.5, limit=n)
    try:
        Ls, us, probe, look, n_out, drawn = _dry_run(draws, M, 4, n)
    finally:
        draws.release()
    assert (n_out, drawn) == (n, n) and [int(v) for v in Ls] == [w[0] for w in want]
    rs = np.random.RandomState()
    rs.set_state(state)
    assert np.random.rand() == rs.rand() and np.random.randn() == rs.randn()


def test_dry_run_refuses_an_unbounded_stream(built_lib):
    draws = LegacyDraws(4, (5, 20), 1.0, seed=1)
    try:
        with pytest.raises(AssertionError):
            _dry_run(draws, 4, 3, 4)
    finally:
        draws.release()
