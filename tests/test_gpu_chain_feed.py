"""The trajectory feeder (csrc/host_feed.h, Engine.run_chain's dispatch) against the loop it replaces: every case
runs the same random stream twice, on two engines in one process -- through the feeder and with
GRAVHMC_CHAIN_FEED=0 -- and wants the decisions, out5, the delivered models, the chain's final state and synthetic
data and the speculative-step counters equal bit for bit.  One case is checked against the CPU oracle as well.
Shapes: tests/feed_cases.py (the dense sweep at N = 120, M = 480) and the smallest paired fold of
tests/fold_oracle_cases.py; GRAVHMC_RESIDENT=0 keeps both off the resident kernel."""
import numpy as np
import pytest

import feed_cases
import fold_oracle_cases as fc
from helpers import relmax

pytestmark = pytest.mark.gpu

PLAN = [3, 1, 18, 7, 2, 11, 5, 9, 4]      # mixed lengths 1 .. 18


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _engine(G, monkeypatch, d, env=None, matrix_free=False):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    eng = G.Engine(d.N, d.M)
    if matrix_free:
        eng.set_matrix_free(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in d.obs])
    eng.set_cells(d.b6, 0)
    eng.build_G()
    eng.weight(0.5)
    eng.set_data(d.dobs)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, d.mwapr)
    return eng


class Run(object):
    """One stream on one engine: the results as on_result got them, and the chain afterwards."""

    def __init__(self, eng, monkeypatch, d, dt, feed, seed=11, Lrange=(5, 20), plan=None, limit=None, sigma=1.0,
                 on_result=None, window=0, **kw):
        from gravinv3dhmc_amd.inversion.rng import LegacyDraws
        monkeypatch.setenv("GRAVHMC_CHAIN_FEED", "1" if feed else "0")
        if window:
            eng.posterior_window(window)
        eng.chain_init(d.x0, d.low, d.high)
        self.res = []

        def keep(L, acc, o, x):
            self.res.append((int(L), bool(acc), np.array(o), None if x is None else np.array(x)))
            return on_result(len(self.res)) if on_result is not None else None

        draws = LegacyDraws(d.M, Lrange, sigma, fixed_L=plan, limit=limit, seed=seed)
        try:
            eng.run_chain(draws, dt, keep, overlap=True, **kw)
        finally:
            draws.release()
        self.feed = eng.feed_stats()
        self.x, self.dsyn, self.stats = eng.chain_get_x(), eng.chain_get_dsyn(), eng.chain_stats()
        self.post = eng.posterior_read() if window else None
        # the path that was asked for is the path that ran
        assert (self.feed["run"] > 0) == bool(feed and self.res), self.feed


def _same(a, b, what):
    assert len(a.res) == len(b.res), (what, len(a.res), len(b.res))
    for t, ((L1, a1, o1, x1), (L2, a2, o2, x2)) in enumerate(zip(a.res, b.res)):
        assert L1 == L2 and a1 == a2 and np.array_equal(o1, o2), (what, t)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2)), (what, t, "x")
    assert np.array_equal(a.x, b.x) and np.array_equal(a.dsyn, b.dsyn), what
    for k in ("spec_hits", "spec_misses"):
        assert a.stats[k] == b.stats[k], (what, k, a.stats, b.stats)
    assert a.feed["run"] == len(a.res)


def _both(G, monkeypatch, d, dt, env=None, matrix_free=False, **kw):
    fed_eng = _engine(G, monkeypatch, d, env, matrix_free)
    ref_eng = _engine(G, monkeypatch, d, env, matrix_free)
    fed = Run(fed_eng, monkeypatch, d, dt, True, **kw)
    ref = Run(ref_eng, monkeypatch, d, dt, False, **kw)
    return fed, ref, fed_eng, ref_eng


@pytest.mark.parametrize("stream", ["plan-1", "plan-2", "plan-3", "plan-4", "plan-9", "lrange-7"])
def test_dense_sweep_streams(G, monkeypatch, stream):
    d = feed_cases.dense()
    kind, n = stream.split("-")
    kw = {"plan": PLAN[:int(n)]} if kind == "plan" else {"limit": int(n)}
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt, env={"GRAVHMC_FEED_ROWS": 3}, want_x=True, **kw)
    assert len(ref.res) == int(n) and fed.feed["rows"] == 3 and fed.feed["drawn"] == int(n)
    _same(fed, ref, stream)
    print("%s: %d accepted of %d, spec hits %d misses %d, feeder waits %r" % (
        stream, sum(r[1] for r in fed.res), len(fed.res), fed.stats["spec_hits"], fed.stats["spec_misses"], fed.feed))
    e1.close()
    e2.close()


def test_rejections_discard_the_speculative_step(G, monkeypatch):
    d = feed_cases.dense()
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt_reject, env={"GRAVHMC_FEED_ROWS": 3}, seed=feed_cases.SEED_REJECT,
                             limit=12, want_x=True)
    acc = [r[1] for r in ref.res]
    print("decisions of the reference path:", "".join("A" if a else "r" for a in acc), ref.stats)
    assert len(acc) == 12 and sum(acc) >= 2 and 12 - sum(acc) >= 2
    # (a rejected proposal discards the step taken ahead for its successor; only the stream's last has none)
    assert ref.stats["spec_misses"] >= 12 - sum(acc) - 1
    _same(fed, ref, "rejections")
    e1.close()
    e2.close()


def test_stop_at_accepts_and_record_from(G, monkeypatch):
    d = feed_cases.dense()
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt, env={"GRAVHMC_FEED_ROWS": 4}, stop_at_accepts=3, record_from=1,
                             want_x=True, window=4)
    assert sum(r[1] for r in ref.res) == 3 and ref.res[-1][1]
    _same(fed, ref, "stop_at_accepts")
    # the window holds the accepted states after the first, the same ones on both paths
    assert fed.post["n"] == ref.post["n"] == 2 and fed.post["total"] == ref.post["total"]
    assert np.array_equal(fed.post["mean"], ref.post["mean"]) and np.array_equal(fed.post["std"], ref.post["std"])
    # the drawer was never more than rows - 2 trajectories ahead of the runner
    assert 0 <= fed.feed["drawn"] - fed.feed["run"] <= fed.feed["rows"] - 2, fed.feed
    e1.close()
    e2.close()


def test_early_stop_by_on_result(G, monkeypatch):
    d = feed_cases.dense()
    eng = _engine(G, monkeypatch, d, {"GRAVHMC_FEED_ROWS": 4})
    refused = []

    def on_result(n):
        if n == 1:
            # the context belongs to its feeder: refused with an error, not a crash
            try:
                eng.forward(d.x0)
            except ValueError as e:
                refused.append(str(e))
        return n < 2

    run = Run(eng, monkeypatch, d, d.dt, True, on_result=on_result)
    assert len(run.res) == 2 and 2 <= run.feed["run"] <= 3, run.feed
    assert len(refused) == 1 and "feeder" in refused[0], refused
    # the engine is the caller's again
    assert eng.forward(d.x0).shape == (d.N,)
    # and what ran is the stream's beginning: the first two results of the whole stream on the loop
    ref_eng = _engine(G, monkeypatch, d, {"GRAVHMC_FEED_ROWS": 4})
    ref = Run(ref_eng, monkeypatch, d, d.dt, False, limit=2)
    for (L1, a1, o1, _), (L2, a2, o2, _) in zip(run.res, ref.res):
        assert L1 == L2 and a1 == a2 and np.array_equal(o1, o2)
    eng.close()
    ref_eng.close()


def test_folded_and_paired_store(G, monkeypatch):
    d = fc.make("P-44")
    env = dict(d.spec.env(), GRAVHMC_FOLD_MIN_MB=0, GRAVHMC_FEED_ROWS=3)
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt, env=env, plan=[2, 5, 1, 4, 3, 6], want_x=True)
    assert len(ref.res) == 6
    assert e1.fold_info()["pair_on"] and e2.fold_info()["pair_on"]
    _same(fed, ref, "fold")
    e1.close()
    e2.close()


def test_matrix_free(G, monkeypatch):
    d = feed_cases.dense()
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt, env={"GRAVHMC_FEED_ROWS": 3}, matrix_free=True, plan=PLAN[:4],
                             want_x=True)
    assert len(ref.res) == 4
    _same(fed, ref, "matrix-free")
    e1.close()
    e2.close()


def test_against_the_cpu_oracle(G, monkeypatch):
    d = feed_cases.dense()
    trajs = d.stream(11, 5, plan=PLAN[:5])
    want = d.oracle_chain(trajs, d.dt)           # before an engine is touched
    eng = _engine(G, monkeypatch, d, {"GRAVHMC_FEED_ROWS": 3})
    run = Run(eng, monkeypatch, d, d.dt, True, seed=11, plan=PLAN[:5], want_x=True)
    assert len(run.res) == 5
    x = d.x0
    for t, ((L, acc, o, xr), (wacc, wo, wx, _)) in enumerate(zip(run.res, want)):
        x = xr if xr is not None else x
        e_o, e_x = relmax(o, wo), relmax(x, wx)
        print("trajectory %d (L = %d, %s): out5 %.2e, x %.2e" % (t, L, "accepted" if wacc else "rejected", e_o, e_x))
        assert L == trajs[t][0] and acc == wacc
        assert e_o <= 1e-10 and e_x <= 1e-10, (t, e_o, e_x)
    assert relmax(run.x, want[-1][2]) <= 1e-10
    eng.close()


def test_vector_sigma(G, monkeypatch):
    d = feed_cases.dense()
    sigma = 0.5 + np.linspace(0.0, 1.0, d.M) ** 2
    fed, ref, e1, e2 = _both(G, monkeypatch, d, d.dt, env={"GRAVHMC_FEED_ROWS": 3}, sigma=sigma, limit=3, want_x=True)
    assert len(ref.res) == 3
    _same(fed, ref, "vector sigma")
    e1.close()
    e2.close()
