"""The streaming posterior on the device (csrc/poststream.hip.h) against its NumPy restatement
(tests/poststream_host.py): explicit rows, and every chain path that feeds it against the rows the same run wrote
to model.bin.

Tolerance: mean, std, chain_M2, R-hat, ESS and the quantiles at 1e-12 relative with a floor of 1e-12 max|m|.
Welford and batch means are O(n eps kappa) with n <= 64 and kappa = sqrt(1 + mean^2 / var); the explicit data
are drawn with |mean| <= 10 std, so the bound is about 7e-14 and 1e-12 leaves a factor of ~14 for constants.
Histogram counts, sample counts and NaN patterns are exact."""
import os

import numpy as np
import pytest

from conftest import gold
from helpers import c1_inputs
from poststream_host import Stream, close

pytestmark = pytest.mark.gpu

QS = (0.025, 0.25, 0.5, 0.9, 0.975)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _explicit(M, C=3, n=11, bins=(16, 7), seed=5):
    """Rows (C, n, M) and bounds with the edge cases: samples at lo and at hi, outside the bounds, a cell with
    hi == lo, a cell constant over all samples; every other sample away from the interior bin edges."""
    rng = np.random.default_rng(seed)
    sd = rng.uniform(0.5, 2.0, M)
    mu = rng.uniform(-10, 10, M) * sd
    rows = mu + sd * np.clip(rng.normal(size=(C, n, M)), -3.9, 3.9)
    lo, hi = mu - 4 * sd, mu + 4 * sd
    for B in bins * 2:                       # (twice: a nudge for one bin count may land on an edge of the other)
        t = (rows - lo) / (hi - lo) * B
        near = np.abs(t - np.round(t)) < 1e-6
        rows = np.where(near, rows + 1e-4 * (hi - lo), rows)
    for B in bins:
        t = (rows - lo) / (hi - lo) * B
        assert np.abs(t - np.round(t)).min() >= 1e-9 * B
    rows[0, 0, 0:10] = lo[0:10]
    rows[1, 3, 5:15] = hi[5:15]
    rows[2, 5, 20:25] = hi[20:25] + 2 * (hi - lo)[20:25]
    rows[2, 5, 25:30] = lo[25:30] - 3 * (hi - lo)[25:30]
    lo[30] = hi[30] = 1.5
    rows[:, :, 31] = mu[31] + 0.25 * sd[31]
    return rows, lo, hi


def _compare(eng, ref, rows_all, lo, hi, bins, qs=QS):
    """The device stream against the restatement `ref`; rows_all: every recorded row (for the empirical quantiles)."""
    st, rt = eng.posterior_stream_read(), ref.read()
    scale = float(np.abs(rows_all).max())
    assert np.array_equal(st["n_per_chain"], rt["n_per_chain"])
    assert np.array_equal(eng.posterior_stream_hist(), ref.H)
    worst = {}
    for k in ("mean", "std", "rhat", "ess", "chain_mean", "chain_M2"):
        assert np.array_equal(np.isnan(st[k]), np.isnan(rt[k])), k
        ok = ~np.isnan(rt[k])
        worst[k] = float((np.abs(st[k][ok] - rt[k][ok]) / np.maximum(np.abs(rt[k][ok]), scale)).max()) if ok.any() else 0.0
    q, qr = eng.posterior_stream_quantiles(qs), ref.quantiles(qs)
    worst["quantiles"] = float((np.abs(q - qr) / np.maximum(np.abs(qr), scale)).max())
    print("stream against the restatement, worst relative deviations:", worst)
    for k, v in worst.items():
        assert v <= 1e-12, (k, v)
    assert close(q, qr, scale)
    # within one bin width of the empirical quantile wherever that one lies inside the bounds; else in the end bin
    emp = np.quantile(rows_all, qs, axis=0, method="inverted_cdf")
    width = np.broadcast_to((hi - lo) / bins, q.shape)
    lo_, hi_ = np.broadcast_to(lo, q.shape), np.broadcast_to(hi, q.shape)
    inside = (emp >= lo_) & (emp <= hi_)
    assert np.all(np.abs(q - emp)[inside] <= width[inside] * (1 + 1e-12))
    below, above = emp < lo_, emp > hi_
    assert np.all(q[below] <= (lo_ + width)[below]) and np.all(q[above] >= (hi_ - width)[above])
    return st


@pytest.mark.parametrize("M", [120, 6000])
@pytest.mark.parametrize("bins", [16, 7])
def test_explicit_rows_against_the_restatement(G, M, bins):
    C, n, b = 3, 11, 4
    rows, lo, hi = _explicit(M, C, n)
    eng = G.Engine(4, M)
    eng.posterior_stream(C, bins=bins, batch_len=b, lo=lo, hi=hi)
    ref = Stream(C, M, bins, b, lo, hi)
    empty = eng.posterior_stream_read()
    assert np.all(np.isnan(empty["mean"])) and empty["n_per_chain"].tolist() == [0, 0, 0]
    for i in range(n):
        for c in range(C):
            eng.posterior_stream_add(c, rows[c, i])
            ref.add(c, rows[c, i])
    st = _compare(eng, ref, rows.reshape(C * n, M), lo, hi, bins)
    assert st["n_per_chain"].tolist() == [n] * C
    assert np.isnan(st["rhat"][31]) and np.isnan(st["ess"][31])            # W == 0 on the constant cell
    assert np.count_nonzero(np.isnan(st["rhat"])) == 1 and np.count_nonzero(np.isnan(st["ess"])) == 1
    assert eng.posterior_stream_quantiles([0.5])[0, 30] == 1.5
    H = eng.posterior_stream_hist()
    assert H.dtype == np.uint32 and H.shape == (bins, M) and np.all(H.sum(axis=0) == C * n)
    assert H[1:, 30].sum() == 0 and H[-1, 20:25].min() >= 1 and H[0, 25:30].min() >= 1
    with pytest.raises(ValueError, match="slot"):
        eng.posterior_stream_add(C, rows[0, 0])
    with pytest.raises(ValueError, match="slot"):
        eng.posterior_stream_slot(C)
    eng.close()


def test_slot_order_and_repeatability(G):
    M, C, n, bins, b = 301, 3, 11, 16, 4
    rows, lo, hi = _explicit(M, C, n)

    def run(order, chains=C):
        eng = G.Engine(4, M)
        eng.posterior_stream(chains, bins=bins, batch_len=b, lo=lo, hi=hi)
        for c, i in order:
            eng.posterior_stream_add(c, rows[c, i])
        st, H = eng.posterior_stream_read(), eng.posterior_stream_hist()
        eng.close()
        return st, H

    a, Ha = run([(c, i) for i in range(n) for c in range(C)])
    b_, Hb = run([(c, i) for c in (2, 0, 1) for i in range(n)])
    for k in ("chain_mean", "chain_M2", "mean", "std", "rhat", "ess"):
        assert np.array_equal(a[k], b_[k], equal_nan=True), k
    assert np.array_equal(Ha, Hb)
    alone, _ = run([(1, i) for i in range(n)])
    assert np.array_equal(alone["chain_mean"][1], a["chain_mean"][1]) and np.array_equal(alone["chain_M2"][1], a["chain_M2"][1])
    assert alone["n_per_chain"].tolist() == [0, n, 0] and np.all(np.isnan(alone["rhat"]))
    # (the pooled mean of one chain is n mean / n: two roundings away from the chain's own)
    np.testing.assert_allclose(alone["mean"], a["chain_mean"][1], rtol=4e-16, atol=0)


def _module_small(G, p):
    return G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]), verbose=False)


def _small_args(M, lo, hi, Sigma, reg, dobs):
    return (np.full(M, 0.001 + lo), np.full(M, 0.001), np.c_[np.full(M, lo), np.full(M, hi)], "mandatory", 1000, dobs,
            "Fixed", 0.8, 1.0, reg, 0.001, 100, float(Sigma))


def _rows(folder, M):
    return np.fromfile(folder + "/model.bin").reshape(-1, M)


def _against_files(eng, folders, M, lo, hi, bins, b, pick=slice(None)):
    rows = [_rows(f, M)[pick] for f in folders]
    ref = Stream(len(rows), M, bins, b, lo, hi)
    for i in range(max(len(r) for r in rows)):
        for c, r in enumerate(rows):
            if i < len(r):
                ref.add(c, r[i])
    return _compare(eng, ref, np.concatenate(rows), np.full(M, lo), np.full(M, hi), bins), rows


@pytest.mark.parametrize("resident", ["1", "0"])
def test_hmcsample_feeds_the_stream_beside_the_ring(G, tmp_path, capsys, monkeypatch, resident):
    """Single chain, resident chain kernel and sweep per launch: the stream equals the restatement over the rows of
    model.bin; the ring still returns np.mean / np.std of the last rows."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    c, p = gold("chain_small.npz"), gold("potential_small.npz")
    M = p["wm"].size
    dt, Sigma, lo, hi, n = c["a_cfg"]
    gm = _module_small(G, p)
    folder = str(tmp_path / "single_chain")
    G.HMCSample(gm, 9, 2, float(dt), [5, 20], *_small_args(M, lo, hi, Sigma, str(c["a_reg"]), p["dobs"]),
                save_folder=folder, sample_sink="binary", posterior_last=5, posterior_stream={"bins": 16, "batch_len": 4})
    capsys.readouterr()
    eng = gm._engine
    assert (eng.chain_stats()["resident_launches"] > 0) == (resident == "1")
    st, rows = _against_files(eng, [folder + "0"], M, lo, hi, 16, 4)
    assert st["n_per_chain"].tolist() == [9] and rows[0].shape == (9, M)
    ring = eng.posterior_read()
    assert ring["n"] == 5 and ring["total"] == 9
    np.testing.assert_allclose(ring["mean"], rows[0][-5:].mean(axis=0), rtol=1e-12, atol=1e-12 * hi)
    np.testing.assert_allclose(ring["std"], rows[0][-5:].std(axis=0), rtol=1e-9, atol=1e-12 * hi)
    from gravinv3dhmc_amd import posterior
    sm = posterior.summarize_stream(gm, p["dobs"], q=(0.1, 0.9))
    assert sm["n"] == 9 and sm["quantiles"].shape == (2, M) and np.isnan(sm["rhat_max"]) and np.array_equal(sm["mean"], st["mean"])
    # a second stream without a free is refused; after a free the engine takes a new one
    with pytest.raises(ValueError, match="already allocated"):
        eng.posterior_stream(1, lo=lo, hi=hi)
    eng.posterior_stream_free()
    eng.posterior_stream(2, lo=lo, hi=hi)
    assert eng.posterior_stream_read()["n_per_chain"].tolist() == [0, 0]
    eng.close()


@pytest.mark.parametrize("form", ["lockstep", "turns", "mfma"])
def test_hmcsample_batch_small_every_form(G, tmp_path, capsys, monkeypatch, form):
    """Three chains on chain_small's problem: in lock-step inside the resident batch kernel, taking turns in the
    resident chain kernel (GRAVHMC_RESIDENT_BATCH=0) and as an MFMA batch (finish_chains); the 'none' sink leaves the
    same stream bits as the 'binary' one."""
    if form == "turns":
        monkeypatch.setenv("GRAVHMC_RESIDENT_BATCH", "0")
    if form == "mfma":
        monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    c, p = gold("chain_small.npz"), gold("potential_small.npz")
    M = p["wm"].size
    dt, Sigma, lo, hi, n = c["a_cfg"]
    out = {}
    for sink in ("binary", "none"):
        gm = _module_small(G, p)
        folder = str(tmp_path / ("batch_%s_chain" % sink))
        G.HMCSampleBatch(gm, 3, 8, 1, float(dt), [5, 20], *_small_args(M, lo, hi, Sigma, str(c["a_reg"]), p["dobs"]),
                         save_folder=folder, sample_sink=sink, posterior_stream={"bins": 16, "batch_len": 2})
        capsys.readouterr()
        eng = gm._engine
        rb, cs = eng.batch_resident_stats(), eng.chain_stats()
        assert (rb["launches"] > 0) == (form == "lockstep"), rb
        assert (cs["resident_launches"] > 0) == (form != "mfma"), cs
        if sink == "binary":
            st, rows = _against_files(eng, [folder + str(r) for r in range(3)], M, lo, hi, 16, 2)
            assert st["n_per_chain"].tolist() == [8, 8, 8] and not np.all(np.isnan(st["rhat"]))
        else:
            assert not os.path.exists(folder + "0/model.bin")
        out[sink] = (eng.posterior_stream_read(), eng.posterior_stream_hist())
        eng.close()
    for k in ("chain_mean", "chain_M2", "mean", "std", "rhat", "ess"):
        assert np.array_equal(out["binary"][0][k], out["none"][0][k], equal_nan=True), k
    assert np.array_equal(out["binary"][1], out["none"][1])


def test_hmcsample_batch_c1_lockstep(G, tmp_path, capsys):
    g = gold("c1_chain.npz")
    mesh, xp, yp, zp = c1_inputs()
    gm = G.GravMagModule(g["dobs"], (0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (xp, yp, zp), verbose=False)
    M = 6000
    folder = str(tmp_path / "c1_batch_chain")
    G.HMCSampleBatch(gm, 3, 6, 1, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.zeros(M), np.ones(M)],
                     "mandatory", 1000, g["dobs"], "Fixed", 0.8, 1.0, "Damping", 0.001, 100, 0.001, save_folder=folder,
                     sample_sink="binary", posterior_stream={"bins": 7, "batch_len": 2})
    capsys.readouterr()
    eng = gm._engine
    rb = eng.batch_resident_stats()
    assert rb["launches"] > 0 and rb["timeouts"] == 0, rb
    st, _ = _against_files(eng, [folder + str(r) for r in range(3)], M, 0.0, 1.0, 7, 2)
    assert st["n_per_chain"].tolist() == [6, 6, 6]
    eng.close()


def test_mfma_batch_beyond_the_resident_limit(G):
    """A store too large for the resident kernels (5003 x 1234): gh_batch_run's finish_chains feeds the stream from the
    interleaved Xc; the restatement runs over the accepted rows the same calls return."""
    rng = np.random.default_rng(3)
    N, M, C, T = 5003, 1234, 3, 4
    A = np.asfortranarray(rng.normal(size=(N, M)))
    e = G.Engine(N, M)
    e.upload_G(A)
    wm = e.weight(0.5)
    e.set_data(rng.normal(size=N) * 20)
    e.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    e.batch_init(x0s, 0.0 * wm, 0.5 * wm)
    e.posterior_stream(C, bins=16, batch_len=2, record_from=1, lo=0.0, hi=0.5)
    ref = Stream(C, M, 16, 2, 0.0, 0.5)
    seen, rows_all = [0] * C, []
    for _ in range(3):
        acc, out5, xs = e.batch_run(rng.normal(size=(C, T, M)) * 0.02, 0.004, rng.integers(1, 6, size=(C, T)),
                                    rng.uniform(size=(C, T)), want_x=True)
        for c in range(C):
            for t in range(T):
                if acc[c, t]:
                    seen[c] += 1
                    if seen[c] > 1:
                        ref.add_x(c, xs[c, t], wm)
                        rows_all.append(xs[c, t] * (1.0 / wm))
    assert e.chain_stats()["resident_launches"] == 0 and e.batch_resident_stats()["launches"] == 0
    assert e.batch_fused_stats()["timeouts"] == 0
    assert sum(seen) > C                                                   # (something was recorded)
    st = _compare(e, ref, np.array(rows_all), np.zeros(M), np.full(M, 0.5), 16)
    assert st["n_per_chain"].tolist() == [s - 1 for s in seen]
    e.close()


def test_shift_invariant_persistent_launch(G, tmp_path, capsys):
    """Single chain on the small global grid of test_gpu_mfbatch.py, the harmonic pass as one persistent launch."""
    rng = np.random.default_rng(27)
    mrange, mspacing = (-180, 180, -90, 90, 0, -3000000), (-1000000, 15, 10)
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 181, 10.0), np.arange(-90, 91, 15.0), indexing="ij")]
    h = np.full_like(lon, 30000.0)
    mesh = G.mesher.TesseroidMesh(mrange, mspacing)
    M, N = mesh.size, lon.size
    dense = G.GravMagModule(np.zeros(N), mrange, mspacing, (lon, lat, h), coordinate="spherical", verbose=False)
    rho = np.zeros(mesh.shape)
    rho[1:, 4:8, 10:20] = 0.3
    dobs = dense._engine.forward(dense.Wm.diagonal() * rho.ravel()) * (1.0 + 0.01 * rng.normal(size=N))
    dense._engine.close()
    gm = G.GravMagModule(dobs, mrange, mspacing, (lon, lat, h), coordinate="spherical", verbose=False, shift_invariant=True)
    folder = str(tmp_path / "table")
    G.HMCSample(gm, 8, 1, 0.005, [5, 20], np.full(M, 0.001), np.full(M, 0.001), np.c_[np.zeros(M), np.full(M, 0.8)],
                "mandatory", 1000, dobs, "Fixed", 0.8, 0.05, "Damping", 0.01, 100, 0.001, myrank=0, save_folder=folder,
                sample_sink="binary", posterior_last=0, posterior_stream={"bins": 16, "batch_len": 2})
    capsys.readouterr()
    eng = gm._engine
    rs = eng.shift_invariant_resident_stats()
    assert rs["launches"] > 0 and rs["timeouts"] == 0, rs
    st, _ = _against_files(eng, [folder + "0"], M, 0.0, 0.8, 16, 2)
    assert st["n_per_chain"].tolist() == [8]
    eng.close()


def test_burn_in_window(G, tmp_path, capsys):
    """record_from = 2, record_count = 3: exactly the accepted samples 3..5 of each chain."""
    c, p = gold("chain_small.npz"), gold("potential_small.npz")
    M = p["wm"].size
    dt, Sigma, lo, hi, n = c["a_cfg"]
    gm = _module_small(G, p)
    eng = gm._engine
    eng.posterior_stream(3, bins=16, batch_len=2, record_from=2, record_count=3, lo=lo, hi=hi)
    folder = str(tmp_path / "window_chain")
    G.HMCSampleBatch(gm, 3, 7, 0, float(dt), [5, 20], *_small_args(M, lo, hi, Sigma, str(c["a_reg"]), p["dobs"]),
                     save_folder=folder, sample_sink="binary", posterior_stream=True)
    capsys.readouterr()
    st, rows = _against_files(eng, [folder + str(r) for r in range(3)], M, lo, hi, 16, 2, pick=slice(2, 5))
    assert st["n_per_chain"].tolist() == [3, 3, 3] and all(r.shape == (3, M) for r in rows)
    eng.close()


def test_refusals(G):
    from gravinv3dhmc_amd.dist import Ranks, make_sharded_engine
    env = {k: os.environ.pop(k, None) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        sh = make_sharded_engine(8, 24, Ranks(), backend="gloo")
        with pytest.raises(NotImplementedError, match="posterior stream"):
            sh.posterior_stream(2, lo=0.0, hi=1.0)
        sh.close()
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    eng = G.Engine(4, 24)
    eng.posterior_stream(2, lo=0.0, hi=1.0)
    with pytest.raises(ValueError, match="already allocated"):
        eng.posterior_stream(2, lo=0.0, hi=1.0)
    eng.close()
