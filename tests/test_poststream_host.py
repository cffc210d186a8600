"""CPU suite: the streaming posterior's C-ABI surface, the front end's argument checks (before any device work) and
the NumPy restatement of its arithmetic (tests/poststream_host.py) against plain NumPy."""
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
from poststream_host import Stream, batch_means_ess, close, gelman_rubin

NAMES = ("gh_posterior_stream", "gh_posterior_stream_slot", "gh_posterior_stream_add", "gh_posterior_stream_read",
         "gh_posterior_stream_quantiles", "gh_posterior_stream_hist", "gh_posterior_stream_free")


def test_prototypes_in_header_and_binding():
    from gravinv3dhmc_amd import Engine, _lib, posterior
    with open(os.path.join(ROOT, "include", "gravhmc.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES, name
        assert "int %s(gh_ctx *ctx" % name in header, name
    for name in ("posterior_stream", "posterior_stream_slot", "posterior_stream_add", "posterior_stream_read",
                 "posterior_stream_quantiles", "posterior_stream_hist", "posterior_stream_free"):
        assert callable(getattr(Engine, name)), name
    assert callable(posterior.summarize_stream)


def test_argument_checks_fire_before_device_work():
    from gravinv3dhmc_amd import Engine
    eng = Engine.__new__(Engine)          # (no device context: the checks come first)
    eng.M = 5
    lo, hi = np.zeros(5), np.ones(5)
    for kw, what in (({"chains": 0}, "chains"), ({"chains": 17}, "chains"), ({"bins": 1}, "bins"), ({"bins": 257}, "bins"),
                     ({"batch_len": 0}, "batch_len"), ({"record_from": -1}, "record_from")):
        args = dict(chains=2, bins=8, batch_len=2, lo=lo, hi=hi)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            Engine.posterior_stream(eng, **args)
    bad = hi.copy()
    bad[3] = -1.0
    with pytest.raises(ValueError, match="hi < lo at cell 3"):
        Engine.posterior_stream(eng, 2, lo=lo, hi=bad)
    with pytest.raises(ValueError, match="bounds"):
        Engine.posterior_stream(eng, 2)
    with pytest.raises(ValueError, match="no posterior stream"):
        Engine.posterior_stream_read(eng)
    with pytest.raises(ValueError, match="no posterior stream"):
        Engine.posterior_stream_quantiles(eng, [0.5])


def test_samplers_take_the_keywords_and_default_to_none():
    from gravinv3dhmc_amd.inversion import hmc
    s = inspect.signature(hmc.HMCSample).parameters
    assert s["posterior_stream"].default is None and s["posterior_slot"].default == 0
    assert inspect.signature(hmc.HMCSampleBatch).parameters["posterior_stream"].default is None
    with pytest.raises(ValueError, match="unknown option"):
        hmc._open_stream(None, {"bin": 3}, 1, 0, 1, np.zeros((2, 2)))
    assert hmc._open_stream(None, None, 1, 0, 1, np.zeros((2, 2))) is False


def _data(seed=0, C=3, n=11, M=40):
    rng = np.random.default_rng(seed)
    sd = rng.uniform(0.5, 2.0, M)
    mu = rng.uniform(-10, 10, M) * sd
    rows = mu + sd * rng.normal(size=(C, n, M))
    lo, hi = rows.min(axis=(0, 1)) - 0.1, rows.max(axis=(0, 1)) + 0.1
    return rows, lo, hi


def test_restatement_against_plain_numpy():
    C, n, M, b, B = 3, 11, 40, 4, 16
    rows, lo, hi = _data(C=C, n=n, M=M)
    s = Stream(C, M, B, b, lo, hi)
    for i in range(n):
        for c in range(C):
            s.add(c, rows[c, i])
    st = s.read()
    flat = rows.reshape(C * n, M)
    scale = np.abs(rows).max()
    assert np.array_equal(st["n_per_chain"], [n] * C) and np.array_equal(s.K, [n // b] * C)
    assert close(st["mean"], flat.mean(axis=0), scale) and close(st["std"], flat.std(axis=0), scale)
    assert close(st["chain_mean"], rows.mean(axis=1), scale)
    assert close(st["chain_M2"], n * rows.var(axis=1), scale)
    assert close(st["rhat"], gelman_rubin(rows), scale, 1e-11)
    assert close(st["ess"], sum(batch_means_ess(rows[c], b) for c in range(C)), scale, 1e-10)
    # histogram: np.histogram's equal bins; the quantile lies in the bin that holds the empirical one
    for j in (0, 7, M - 1):
        assert np.array_equal(s.H[:, j], np.histogram(flat[:, j], bins=B, range=(lo[j], hi[j]))[0])
    assert s.H.sum(axis=0).tolist() == [C * n] * M
    qs = (0.0, 0.025, 0.25, 0.5, 0.9, 0.975, 1.0)
    got = s.quantiles(qs)
    ref = np.quantile(flat, qs, axis=0, method="inverted_cdf")
    assert np.all(np.abs(got - ref) <= (hi - lo) / B * (1 + 1e-12))
    assert np.all(np.diff(got, axis=0) >= 0)


def test_restatement_edge_cases():
    M, B, b = 6, 7, 2
    lo = np.array([0.0, 0.0, 1.5, 0.0, -1.0, 0.0])
    hi = np.array([1.0, 1.0, 1.5, 1.0, 1.0, 1.0])
    s = Stream(2, M, B, b, lo, hi)
    assert np.all(np.isnan(s.read()["mean"])) and np.all(np.isnan(s.quantiles([0.5])))
    r0 = np.array([0.0, 1.0, 1.5, 2.5, 0.3, 0.5])      # at lo, at hi, hi == lo, outside, inside, constant
    r1 = np.array([1.0, 0.0, 1.5, -3.0, -0.2, 0.5])
    s.add(0, r0)
    assert s.bins_of(r0).tolist() == [0, B - 1, 0, B - 1, 4, 3]
    assert s.bins_of(r1).tolist() == [B - 1, 0, 0, 0, 2, 3]
    st = s.read()
    assert np.all(np.isnan(st["rhat"])) and np.all(np.isnan(st["ess"]))     # one chain, no complete batch pair
    assert np.array_equal(st["mean"], r0) and np.array_equal(st["std"], np.zeros(M))
    for row in (r1, r0, r1):
        s.add(0, row)
    for row in (r1, r0, r0, r1):
        s.add(1, row)
    st = s.read()
    assert np.isnan(st["rhat"][[2, 5]]).all() and not np.isnan(st["rhat"][[0, 1, 3, 4]]).any()   # W == 0 -> NaN
    assert np.isnan(st["ess"][[2, 5]]).all()                                                    # 0 / 0
    assert s.quantiles([0.5])[0, 2] == 1.5
    # different lengths: R-hat undefined, the pooled moments are still numpy's
    s.add(1, r0)
    st = s.read()
    assert np.all(np.isnan(st["rhat"]))
    allrows = np.array([r0, r1, r0, r1, r1, r0, r0, r1, r0])
    assert close(st["mean"], allrows.mean(axis=0), 3.0) and close(st["std"], allrows.std(axis=0), 3.0)
    # a trailing partial batch is ignored
    assert s.K.tolist() == [2, 2] and s.n.tolist() == [4, 5]
