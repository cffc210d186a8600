"""GPU suite (`-m gpu`): a context that is REUSED -- a second kernel, weights after a batch or a stream exists, a second
compression -- against the CPU oracle on its final configuration, and bit for bit against a fresh engine configured
once with that configuration.

The cases, their inputs and the oracle's results come from tests/lifecycle_cases.py (generated before an engine is
touched; tests/test_lifecycle_host.py checks that the result of each stale store lies at least 1e-6 from the oracle's).
Every scenario runs a reused engine E and a fresh engine F.  E against the oracle: decisions identical, out5, x and
the displacement of every trajectory to TOL = 1e-10 in relmax (the stream: 1e-12, as tests/test_gpu_poststream.py);
E against F: np.array_equal (the paths are reproducible by design, DESIGN "order" rows).  A scenario that failed
against the oracle on F as well would be a finding about the family, not about reuse: F is checked first.

The derived stores these scenarios pin (csrc/gravhmc.hip, kernel_changed): the MFMA operand-order copy of G (two-pass
batch adjoint), the wavelet rows and their dense form, the cross-gradient normalisers, the stream's 1 / wm -- and the
states that must not survive a change (every *_init again)."""
import contextlib
import io

import numpy as np
import pytest

import lifecycle_cases as lc
from helpers import relmax
from poststream_host import close as stream_close

pytestmark = pytest.mark.gpu

TOL = lc.TOL
SWITCHES = ("GRAVHMC_RESIDENT", "GRAVHMC_BATCH_TEAM", "GRAVHMC_BATCH_RELAYOUT", "GRAVHMC_BATCH_SPEC", "GRAVHMC_DWT_LDS",
            "GRAVHMC_BATCH_TEAM_TEST_ABORT", "GRAVHMC_FOLD_MIN_MB", "GRAVHMC_FOLD", "GRAVHMC_FOLD_PAIR")
QS = (0.025, 0.25, 0.5, 0.9, 0.975)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _env(monkeypatch, env):
    """The switches are read when an engine first plans the path: set before Engine(...), kept for its life."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _kernel(eng, pb, build=False, weight=True):
    """pb's kernel into the context, from the oracle's entries or assembled on the device, and its weights."""
    if build:
        eng.set_obs(*pb.obs)
        eng.set_cells(pb.cells, 0)
        eng.build_G()
    else:
        eng.upload_G(pb.K)
    if weight:
        wm = eng.weight(0.5)
        assert relmax(wm, pb.wm) <= (1e-11 if build else 1e-14)
        return wm


def _problem(eng, pb, build=False):
    wm = _kernel(eng, pb, build)
    eng.set_data(pb.dobs, pb.gfix)
    eng.set_reg(pb.reg, pb.alpha, pb.beta, pb.shape, pb.mwapr)
    return wm


def _rounds(eng, ch):
    """batch_init, then batch_trajectory in rounds; batch_get_x of every chain after every round."""
    res = lc.Ref(ch.C, ch.T, ch.M)
    eng.batch_init(ch.x0s, ch.low, ch.high)
    for t in range(ch.T):
        acc, out5 = eng.batch_trajectory(ch.p0s[:, t], ch.dt, ch.Ls[:, t], ch.us[:, t])
        res.acc[:, t], res.out5[:, t] = acc, out5
        for c in range(ch.C):
            res.xs[c, t] = eng.batch_get_x(c)
    return res


def _single(eng, ch):
    """chain_init, then the one chain's trajectories in one run_chain call (the resident kernel where it is on)."""
    res = lc.Ref(1, ch.T, ch.M)
    eng.chain_init(ch.x0s[0], ch.low, ch.high)
    got = []
    draws = [(int(ch.Ls[0, t]), ch.p0s[0, t], float(ch.us[0, t])) for t in range(ch.T)]
    eng.run_chain(iter(draws), ch.dt, lambda L, a, o, x: got.append((a, o.copy(), None if x is None else x.copy())),
                  want_x=True, batch=ch.T)
    assert len(got) == ch.T
    cur = ch.x0s[0]
    for t, (a, o, x) in enumerate(got):
        if a:
            cur = x
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = a, o, cur
    assert np.array_equal(eng.chain_get_x(), cur)
    return res


def _against_oracle(ch, res, what):
    """Decisions, out5, x and displacement of every chain and trajectory; returns the worst relmax."""
    ref, worst = ch.ref, 0.0
    for c in range(ch.C):
        for t in range(ch.T):
            where = (what, "chain %d" % c, "trajectory %d" % t, "L %d" % ch.Ls[c, t])
            assert bool(res.acc[c, t]) == bool(ref.acc[c, t]), where + (res.out5[c, t], ref.out5[c, t])
            own_before = ch.x0s[c] if t == 0 else res.xs[c, t - 1]
            x0 = lc.before(ch, ref, c, t)
            e_o = relmax(res.out5[c, t], ref.out5[c, t])
            e_x = relmax(res.xs[c, t], ref.xs[c, t])
            e_d = 0.0
            if ref.acc[c, t]:
                e_d = relmax(res.xs[c, t] - x0, ref.xs[c, t] - x0)
            else:
                assert np.array_equal(res.xs[c, t], own_before), where
            worst = max(worst, e_o, e_x, e_d)
            print("%s: out5 %.2e, x %.2e, displacement %.2e" % (" ".join(where), e_o, e_x, e_d))
            assert e_o <= TOL and e_x <= TOL and e_d <= TOL, where + (e_o, e_x, e_d)
    return worst


def _same_bits(a, b, what):
    assert np.array_equal(a.acc, b.acc), what
    assert np.array_equal(a.out5, b.out5), (what, "out5", relmax(a.out5, b.out5))
    assert np.array_equal(a.xs, b.xs), (what, "x", relmax(a.xs, b.xs))


# ----------------------------------------------------------------------------- kernel A, then kernel B

FORMS = {
    # id: (case, environment, build_G instead of upload_G, members of the team form expected)
    "two-pass-48x200": ("two-pass-48x200", {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0}, False, 0),
    "two-pass-37x203": ("two-pass-37x203", {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0}, False, 0),
    "column-major-37x203": ("two-pass-37x203", {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0, "GRAVHMC_BATCH_RELAYOUT": 0},
                            False, 0),
    "build_G-48x200": ("two-pass-48x200", {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0}, True, 0),
    "team-3585x7": ("team-3585x7", {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 1}, False, 9),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_on_kernel_a_then_kernel_b(G, monkeypatch, form):
    cid, env, build, members = FORMS[form]
    s = lc.two_kernels(cid)
    if members:
        from gravinv3dhmc_amd import isa_check
        assert isa_check.team_form_cleared(), "the build's scan has not cleared batch_team_kernel (%s)" % isa_check.STAMP
    _env(monkeypatch, env)
    N, M = s.spec.N, s.spec.M
    # F: configured once with the final configuration
    F = G.Engine(N, M)
    _problem(F, s.B, build)
    rF = _rounds(F, s.chB)
    assert F.batch_fused_stats()["members"] == members
    F.close()
    worstF = _against_oracle(s.chB, rF, form + " fresh")
    # E: problem A with one round, then problem B
    E = G.Engine(N, M)
    _problem(E, s.A, build)
    rA = _rounds(E, s.chA)
    _problem(E, s.B, build)
    rE = _rounds(E, s.chB)
    st = E.batch_fused_stats()
    E.close()
    assert st["members"] == members and st["timeouts"] == 0 and (st["launches"] > 0) == (members > 0), st
    worstA = _against_oracle(s.chA, rA, form + " reused, on A")
    worstE = _against_oracle(s.chB, rE, form + " reused, on B")
    _same_bits(rE, rF, form)
    print("%s: worst relmax against the oracle: fresh %.2e, reused on A %.2e, reused on B %.2e; reused == fresh bit for bit"
          % (form, worstF, worstA, worstE))


@pytest.mark.parametrize("resident", ["1", "0"])
def test_single_chain_on_kernel_a_then_kernel_b(G, monkeypatch, resident):
    """One chain through run_chain: inside the resident chain kernel (the default at this size) and sweep per launch."""
    s = lc.two_kernels("two-pass-48x200")
    _env(monkeypatch, {"GRAVHMC_RESIDENT": resident})
    N, M = s.spec.N, s.spec.M
    chA, chB = _first_chain(s.chA), _first_chain(s.chB)
    F = G.Engine(N, M)
    _problem(F, s.B)
    rF = _single(F, chB)
    assert (F.chain_stats()["resident_launches"] > 0) == (resident == "1")
    F.close()
    worstF = _against_oracle(chB, rF, "single chain fresh")
    E = G.Engine(N, M)
    _problem(E, s.A)
    rA = _single(E, chA)
    _problem(E, s.B)
    rE = _single(E, chB)
    assert (E.chain_stats()["resident_launches"] > 0) == (resident == "1")
    E.close()
    worst = max(_against_oracle(chA, rA, "single chain reused, on A"), _against_oracle(chB, rE, "single chain reused, on B"))
    _same_bits(rE, rF, "single chain")
    print("single chain, GRAVHMC_RESIDENT=%s: worst relmax against the oracle: fresh %.2e, reused %.2e" % (resident, worstF, worst))


class _First(object):
    """Chain 0 of a Chains as a Chains of one."""

    def __init__(self, ch):
        self.M, self.C, self.T, self.dt, self.low, self.high = ch.M, 1, ch.T, ch.dt, ch.low, ch.high
        self.x0s, self.Ls, self.p0s, self.us = ch.x0s[:1], ch.Ls[:1], ch.p0s[:1], ch.us[:1]
        self.ref = lc.Ref(1, ch.T, ch.M)
        self.ref.acc[:], self.ref.out5[:], self.ref.xs[:] = ch.ref.acc[:1], ch.ref.out5[:1], ch.ref.xs[:1]


def _first_chain(ch):
    return _First(ch)


def test_bootstrap_batch_on_kernel_a_then_kernel_b(G, monkeypatch):
    """bscg_run contracts the same operand-order copy of G in its adjoint (host_bscg.h): replicates on A, then on B,
    against oracle.cg_port.bootstrap_counts on B and a fresh engine's bits."""
    s = lc.bscg()
    _env(monkeypatch, {"GRAVHMC_BATCH_TEAM": 0})
    N, M = s.B.spec.N, s.B.spec.M
    p = lc.BSCG

    def run(eng, r):
        res = eng.bscg_run(r["counts"], r["dobs"], r["mw0"], p["bounds"][0], p["bounds"][1], p["beta2"], p["q"], p["maxk"])
        ref, worst = r["ref"], 0.0
        assert np.array_equal(res[4], ref.n_entries) and np.array_equal(res[5], ref.n_alpha)
        for name, v, w in zip(lc.BSCG_NAMES, res, ref.results()):
            for b in range(p["B"]):
                dev = relmax(v[b], w[b])
                worst = max(worst, dev)
                assert dev <= TOL, ("kernel " + r["pb"].which, "replicate %d" % b, name, dev)
        return res, worst

    F = G.Engine(N, M)
    _kernel(F, s.B)
    resF, worstF = run(F, s.runs[1])
    F.close()
    E = G.Engine(N, M)
    _kernel(E, s.A)
    _, worstA = run(E, s.runs[0])
    _kernel(E, s.B)
    resE, worstE = run(E, s.runs[1])
    E.close()
    for v, w in zip(resE, resF):
        assert np.array_equal(v, w)
    print("bootstrap batch: worst relmax against the oracle: fresh %.2e, reused on A %.2e, reused on B %.2e" % (worstF, worstA, worstE))


# ----------------------------------------------------------------------------- batch before weights

def test_batch_before_weights(G, monkeypatch):
    """upload_G, data, reg, batch_init, a round; weight; batch_init, rounds: no second kernel, yet the adjoint's copy of
    the unweighted G must not serve the weighted one."""
    s = lc.before_weights()
    b = s.B
    _env(monkeypatch, {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0})
    N, M = s.spec.N, s.spec.M

    def data_reg(eng):
        eng.set_data(b.dobs, b.gfix)
        eng.set_reg("TV", b.alpha, b.beta, b.shape, s.mwapr)

    F = G.Engine(N, M)
    _kernel(F, b)
    data_reg(F)
    rF = _rounds(F, s.chW)
    F.close()
    worstF = _against_oracle(s.chW, rF, "before weights, fresh")
    E = G.Engine(N, M)
    _kernel(E, b, weight=False)
    data_reg(E)
    rU = _rounds(E, s.chU)
    wm = E.weight(0.5)
    assert relmax(wm, b.wm) <= 1e-14
    rE = _rounds(E, s.chW)
    E.close()
    worstU = _against_oracle(s.chU, rU, "before weights, reused, unweighted")
    worstE = _against_oracle(s.chW, rE, "before weights, reused, weighted")
    _same_bits(rE, rF, "before weights")
    print("batch before weights: worst relmax against the oracle: fresh %.2e, unweighted %.2e, weighted %.2e"
          % (worstF, worstU, worstE))


# ----------------------------------------------------------------------------- wavelet rows

def _csr_against_oracle(eng, Aw, dims, shape, nnz):
    """test_wavelet_transform_and_csr_vs_oracle's comparison: entries within rounding of the threshold may fall on
    either side."""
    from oracle import wavelet as ow
    ref = ow.compress_kernel(Aw, dims, shape, lc.WAVELET_THR).toarray()
    got = eng.download_csr().toarray()
    packed = ow.wavedec3_packed(Aw, shape)[0] if dims == 3 else ow.wavedec1_packed(Aw)
    edge = np.abs(np.abs(packed) - lc.WAVELET_THR) < 1e-12
    assert got.shape == ref.shape
    assert np.array_equal((got != 0) | edge, (ref != 0) | edge)
    dev = float(np.abs(got - ref)[~edge].max())
    assert dev < 1e-14
    assert abs(nnz - (ref != 0).sum()) <= edge.sum()
    return ref, dev


@pytest.mark.parametrize("path", ["resident", "sweep"])
def test_wavelet_rows_follow_the_kernel(G, monkeypatch, path):
    from oracle import wavelet as ow
    w = lc.wavelet()
    a, b, shape = w.A, w.B, w.spec.shape
    _env(monkeypatch, {} if path == "resident" else {"GRAVHMC_RESIDENT": 0, "GRAVHMC_DWT_LDS": 1})
    N, M = w.spec.N, w.spec.M
    F = G.Engine(N, M)
    _problem(F, b)
    nnzF, ncF = F.compress_wavelet(1, None, lc.WAVELET_THR, 2)
    fwdF = [F.forward_wavelet(x) for x in w.xs]
    rF = _single(F, w.ch)
    assert (F.chain_stats()["resident_launches"] > 0) == (path == "resident")
    csrF = F.download_csr()
    F.close()
    worstF = _against_oracle(w.ch, rF, "wavelet fresh")

    E = G.Engine(N, M)
    _problem(E, a)
    nnzA, ncA = E.compress_wavelet(3, shape, lc.WAVELET_THR, 2)
    refA, _ = _csr_against_oracle(E, np.asarray(E.download_G()), 3, shape, nnzA)
    for x in w.xs:
        assert relmax(E.forward_wavelet(x), refA @ ow.model_coeffs(x, 3, shape)) <= 1e-12
    # a compressed context refuses a second compression of the SAME kernel
    with pytest.raises(ValueError, match="already compressed"):
        E.compress_wavelet(1, None, lc.WAVELET_THR, 2)
    # kernel B: the rows of A are gone
    _problem(E, b)
    for call in (lambda: E.forward_wavelet(w.xs[0]), E.download_csr, lambda: E.model_coeffs(w.xs[0])):
        with pytest.raises(ValueError, match="gh_compress_wavelet"):
            call()
    worst_dense = 0.0
    for x in w.xs:
        got, ref = E.misfit_and_grad(x), w.PB_dense.misfit_and_grad(x)
        dev = max(abs(got[0] - ref[0]) / abs(ref[0]), relmax(got[1], ref[1]), relmax(got[2], ref[2]))
        worst_dense = max(worst_dense, dev)
        assert dev <= TOL, ("dense forward of B after the new kernel", dev)
    # a second compression, other dims and another Mp
    nnzB, ncB = E.compress_wavelet(1, None, lc.WAVELET_THR, 2)
    assert ncB == w.csrB.shape[1] != ncA and (nnzB, ncB) == (nnzF, ncF)
    AwB = np.asarray(E.download_G())
    refB, csr_dev = _csr_against_oracle(E, AwB, 1, None, nnzB)
    csrE = E.download_csr()
    assert np.array_equal(csrE.indptr, csrF.indptr) and np.array_equal(csrE.indices, csrF.indices)
    assert np.array_equal(csrE.data, csrF.data)
    worst_fwd = 0.0
    for x, fF in zip(w.xs, fwdF):
        f = E.forward_wavelet(x)
        dev = relmax(f, refB @ ow.model_coeffs(x, 1))
        worst_fwd = max(worst_fwd, dev)
        assert dev <= 1e-12
        assert np.array_equal(f, fF)
    rE = _single(E, w.ch)
    assert (E.chain_stats()["resident_launches"] > 0) == (path == "resident")
    E.close()
    worstE = _against_oracle(w.ch, rE, "wavelet reused, %s" % path)
    _same_bits(rE, rF, "wavelet " + path)
    print("wavelet (%s): dense forward of B after the new kernel %.2e, CSR %.2e, forward_wavelet %.2e, chain fresh %.2e, "
          "reused %.2e" % (path, worst_dense, csr_dev, worst_fwd, worstF, worstE))


# ----------------------------------------------------------------------------- cross-gradient normalisers

def _joint_engine(G, z, cells, obs):
    from gravinv3dhmc_amd import _lib, utils
    n, m = obs[0].size, cells.shape[0]
    eng = G.Engine(2 * n, 2 * m)
    eng.set_cells(cells, _lib.CELL_PRISM_JOINT, direction=utils.dircos(*z["mangle"]))
    eng.set_obs(*obs)
    eng.build_G()
    return eng


def _joint_chain(eng, c):
    """the scenario's chain trajectory by trajectory, Phi of the state after each"""
    ch = c.ch
    res, phis = lc.Ref(1, ch.T, ch.M), []
    eng.chain_init(ch.x0s[0], ch.low, ch.high)
    for t in range(ch.T):
        acc, out5 = eng.chain_trajectory(ch.p0s[0, t], ch.dt, int(ch.Ls[0, t]), float(ch.us[0, t]))
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = acc, out5, eng.chain_get_x()
        phis.append(eng.cross_gradient_last())
    return res, np.array(phis)


def test_cross_gradient_normalisers_follow_the_weights(G, monkeypatch):
    """weight, set_cross_gradient, evaluate; then the kernel of other points (a joint context keeps its cells), weight,
    and cross_gradient_eval and a chain WITHOUT another set_cross_gradient: the normalisers are those of the new weights."""
    from conftest import gold
    from gravinv3dhmc_amd import mesher
    c = lc.crossgrad()
    z = gold("joint_small.npz")
    _env(monkeypatch, {})
    with contextlib.redirect_stdout(io.StringIO()):
        mesh = mesher.PrismMesh(tuple(z["a_mrange"]), tuple(z["a_mspacing"]))
    cells = mesh.cell_bounds(active_only=True)
    hx, hy, hz = c.spacing

    def final(eng):
        eng.set_data(c.dobswB)
        eng.set_reg(c.reg, c.alpha, c.beta, c.shape, c.mwaprB)

    F = _joint_engine(G, z, cells, c.obsB)
    wmF = F.weight(0.5)
    assert relmax(wmF, c.wmB) <= TOL and relmax(F.joint_std(), c.stdB) <= TOL
    F.set_cross_gradient(c.lam, c.shape, hx, hy, hz, c.SCALE)
    final(F)
    evF = [F.cross_gradient_eval(mw) for mw in c.mws]
    rF, phF = _joint_chain(F, c)
    F.close()
    worstF = _against_oracle(c.ch, rF, "cross-gradient fresh")

    E = _joint_engine(G, z, cells, c.obsA)
    wmA = E.weight(0.5)
    assert relmax(wmA, c.wmA) <= TOL
    E.set_cross_gradient(c.lam, c.shape, hx, hy, hz, c.SCALE)
    for mw in c.mws:
        phi, grad, t = E.cross_gradient_eval(mw)
        rphi, rgrad, rt = c.phi(mw, c.wmA)
        assert abs(phi - rphi) <= TOL * abs(rphi) and relmax(grad, rgrad) <= TOL and relmax(t, rt) <= TOL
    # other points, other weights; set_cross_gradient is NOT called again
    E.set_obs(*c.obsB)
    E.build_G()
    wmB = E.weight(0.5)
    assert np.array_equal(wmB, wmF)
    final(E)
    worst_phi = 0.0
    for mw, (phiF, gradF, tF) in zip(c.mws, evF):
        phi, grad, t = E.cross_gradient_eval(mw)
        rphi, rgrad, rt = c.phi(mw, c.wmB)
        dev = max(abs(phi - rphi) / abs(rphi), relmax(grad, rgrad), relmax(t, rt))
        worst_phi = max(worst_phi, dev)
        assert dev <= TOL, ("Phi, its gradient and t on the new weights", dev)
        assert phi == phiF and np.array_equal(grad, gradF) and np.array_equal(t, tF)
    rE, phE = _joint_chain(E, c)
    E.close()
    worstE = _against_oracle(c.ch, rE, "cross-gradient reused")
    _same_bits(rE, rF, "cross-gradient")
    assert np.array_equal(phE, phF)
    print("cross-gradient: Phi / gradient / t on the new weights %.2e, chain fresh %.2e, reused %.2e" % (worst_phi, worstF, worstE))


# ----------------------------------------------------------------------------- the stream's 1 / wm

def _stream_against(eng, ref, scale):
    """counts, histogram and NaN pattern exact; moments, R-hat, ESS and quantiles to 1e-12 (tests/test_gpu_poststream.py)"""
    st, rt = eng.posterior_stream_read(), ref.read()
    assert np.array_equal(st["n_per_chain"], rt["n_per_chain"])
    assert np.array_equal(eng.posterior_stream_hist(), ref.H)
    worst = 0.0
    for k in ("mean", "std", "rhat", "ess", "chain_mean", "chain_M2"):
        assert np.array_equal(np.isnan(st[k]), np.isnan(rt[k])), k
        ok = ~np.isnan(rt[k])
        if ok.any():
            dev = float((np.abs(st[k][ok] - rt[k][ok]) / np.maximum(np.abs(rt[k][ok]), scale)).max())
            worst = max(worst, dev)
            assert dev <= 1e-12, (k, dev)
    q, qr = eng.posterior_stream_quantiles(QS), ref.quantiles(QS)
    assert stream_close(q, qr, scale)
    return worst, st, eng.posterior_stream_hist(), q


def _record(eng, ch, ref, wm):
    """ch's chain through run_chain (accepted states go to the stream); the restatement gets the device's own rows"""
    res = _single(eng, ch)
    for t in range(ch.T):
        if res.acc[0, t]:
            ref.add_x(0, res.xs[0, t], wm)
    return res


def _same_stream(a, b):
    for k in ("n_per_chain", "mean", "std", "rhat", "ess", "chain_mean", "chain_M2"):
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3], equal_nan=True)


@pytest.mark.parametrize("resident", ["1", "0"])
def test_stream_allocated_before_the_weights(G, monkeypatch, resident):
    from poststream_host import Stream
    s = lc.stream()
    b = s.B
    _env(monkeypatch, {"GRAVHMC_RESIDENT": resident})
    N, M = s.spec.N, s.spec.M
    scale = float(max(np.abs(s.lo).max(), np.abs(s.hi).max()))

    def run(stream_first):
        eng = G.Engine(N, M)
        eng.upload_G(b.K)
        if stream_first:
            eng.posterior_stream(1, bins=lc.STREAM_BINS, batch_len=lc.STREAM_BATCH, lo=s.lo, hi=s.hi)
        wm = eng.weight(0.5)
        if not stream_first:
            eng.posterior_stream(1, bins=lc.STREAM_BINS, batch_len=lc.STREAM_BATCH, lo=s.lo, hi=s.hi)
        eng.set_data(b.dobs, b.gfix)
        eng.set_reg(b.reg, b.alpha, b.beta, b.shape, b.mwapr)
        ref = Stream(1, M, lc.STREAM_BINS, lc.STREAM_BATCH, s.lo, s.hi)
        res = _record(eng, s.chB, ref, wm)
        out = _stream_against(eng, ref, scale)
        eng.close()
        return res, out

    rF, sF = run(False)
    worstF = _against_oracle(s.chB, rF, "stream fresh")
    rE, sE = run(True)
    worstE = _against_oracle(s.chB, rE, "stream allocated before the weights")
    _same_bits(rE, rF, "stream")
    _same_stream(sE, sF)
    assert sE[1]["n_per_chain"].tolist() == [int(s.chB.ref.acc.sum())]
    print("stream before the weights (GRAVHMC_RESIDENT=%s): chain %.2e / %.2e, stream against the restatement %.2e / %.2e"
          % (resident, worstF, worstE, sF[0], sE[0]))


def test_stream_outlives_its_weights(G, monkeypatch):
    """Allocated after the weights of A, samples of A; kernel B with new weights, samples of B: each row is recorded with
    the weights of ITS kernel.  F: a context that never held A's kernel, given A's rows explicitly, then B."""
    from poststream_host import Stream
    s = lc.stream()
    a, b = s.A, s.B
    _env(monkeypatch, {})
    N, M = s.spec.N, s.spec.M
    scale = float(max(np.abs(s.lo).max(), np.abs(s.hi).max()))
    E = G.Engine(N, M)
    wmA = _kernel(E, a)
    E.posterior_stream(1, bins=lc.STREAM_BINS, batch_len=lc.STREAM_BATCH, lo=s.lo, hi=s.hi)
    E.set_data(a.dobs, a.gfix)
    E.set_reg(a.reg, a.alpha, a.beta, a.shape, a.mwapr)
    ref = Stream(1, M, lc.STREAM_BINS, lc.STREAM_BATCH, s.lo, s.hi)
    rA = _record(E, s.chA, ref, wmA)        # (the device's own weights: the stored reciprocal's bits)
    rowsA = [rA.xs[0, t] * (1.0 / wmA) for t in range(s.chA.T) if rA.acc[0, t]]
    wmB = _problem(E, b)
    rB = _record(E, s.chB, ref, wmB)
    sE = _stream_against(E, ref, scale)
    E.close()
    worst = max(_against_oracle(s.chA, rA, "stream outlives, on A"), _against_oracle(s.chB, rB, "stream outlives, on B"))
    F = G.Engine(N, M)
    wmF = _problem(F, b)
    assert np.array_equal(wmF, wmB)
    F.posterior_stream(1, bins=lc.STREAM_BINS, batch_len=lc.STREAM_BATCH, lo=s.lo, hi=s.hi)
    refF = Stream(1, M, lc.STREAM_BINS, lc.STREAM_BATCH, s.lo, s.hi)
    for m in rowsA:
        F.posterior_stream_add(0, m)
        refF.add(0, m)
    rF = _record(F, s.chB, refF, wmF)
    sF = _stream_against(F, refF, scale)
    F.close()
    _same_bits(rB, rF, "stream outlives")
    _same_stream(sE, sF)
    print("stream that outlives its weights: chains %.2e, stream against the restatement %.2e (fresh %.2e)" % (worst, sE[0], sF[0]))


# ----------------------------------------------------------------------------- the folded store

def test_folded_store_follows_the_geometry(G, monkeypatch):
    """The store that is keyed by the kernel's generation: a symmetric grid, another symmetric grid, an asymmetric
    one, each with build_G and weight and a chain on the sweeps; fold_info says "on", "on" and the detector's reason.
    After set_cells WITHOUT a rebuild forward, adjoint and misfit_and_grad are still the stored kernel's."""
    f = lc.fold()
    _env(monkeypatch, {"GRAVHMC_RESIDENT": 0, "GRAVHMC_FOLD_MIN_MB": 0})
    N, M = f.spec.N, f.spec.M
    fresh = []
    for pb, ch, reason in zip(f.stages, f.ch, f.REASONS):
        F = G.Engine(N, M)
        _problem(F, pb, build=True)
        fresh.append(_single(F, ch))
        info = F.fold_info()
        assert (info["on"], info["reason"]) == (reason == "on", reason), info
        F.close()
    E = G.Engine(N, M)
    worst = []
    for k, (pb, ch, reason) in enumerate(zip(f.stages, f.ch, f.REASONS)):
        _problem(E, pb, build=True)
        rE = _single(E, ch)
        info = E.fold_info()
        assert (info["on"], info["reason"]) == (reason == "on", reason), (k, info)
        worst.append(max(_against_oracle(ch, fresh[k], "fold stage %d fresh" % k), _against_oracle(ch, rE, "fold stage %d reused" % k)))
        _same_bits(rE, fresh[k], "fold stage %d" % k)
    # other cells, no rebuild: the stored kernel (the last stage's) goes on serving
    last = f.stages[2]
    E.set_cells(f.stages[0].cells, 0)
    d, g, mg = E.forward(f.x), E.adjoint(f.r), E.misfit_and_grad(f.x)
    ref = f.P[2].misfit_and_grad(f.x)
    dev = max(relmax(d, last.Aw @ f.x), relmax(g, last.Aw.T @ f.r), abs(mg[0] - ref[0]) / abs(ref[0]), relmax(mg[1], ref[1]),
              relmax(mg[2], ref[2]))
    E.close()
    assert dev <= TOL, dev
    print("fold: chains against the oracle per stage %s, stored kernel after set_cells without a rebuild %.2e"
          % (", ".join("%.2e" % w for w in worst), dev))


# ----------------------------------------------------------------------------- built once

def _table_engines(G, monkeypatch):
    """(name, make_engine, chain) of the three stores that are built once"""
    import lattice_cases
    import lonsym_oracle_cases as loc
    from oracle import oracle
    two = lc.two_kernels("two-pass-48x200")

    def configure(eng, pb):
        # (the store's own entries: its weights are compared with the oracle's in the store's own suite)
        eng.set_obs(*pb.obs)
        eng.set_cells(pb.cells, 0)
        eng.build_G()
        eng.weight(0.5)
        eng.set_data(pb.dobs, pb.gfix)
        eng.set_reg(pb.reg, pb.alpha, pb.beta, pb.shape, pb.mwapr)
        return eng

    def matrix_free():
        eng = G.Engine(two.spec.N, two.spec.M)
        eng.set_matrix_free(True)
        return configure(eng, two.B)

    d = loc.make("h-n3")

    def shift_invariant():
        for k, v in loc.BY_ID["h-n3"].env.items():
            monkeypatch.setenv(k, str(v))
        eng = G.Engine(d.N, d.M)
        eng.set_shift_invariant(True)
        eng.set_obs(*d.obs)
        eng.set_cells(d.bounds, 1, 1.6)
        eng.build_G()
        eng.weight(0.5)
        eng.set_data(d.dobs, d.gfix)
        eng.set_reg(d.reg, d.alpha, d.beta, d.shape, d.mwapr)
        return eng

    obs, b6 = lattice_cases.geometry(cells=(3, 2, 2), obs=(3, 2))
    lat = lc.Problem(oracle, lc.Spec("table-6x12", 6, (2, 2, 3), "Damping", False, C=1, T=4), "T", geometry=(obs, b6))
    lat_ch = lc.Chains(lat.oracle(), 12, 1, 4, seed=71)

    def translation_invariant():
        eng = G.Engine(6, 12)
        eng.set_translation_invariant(True)
        configure(eng, lat)
        assert eng.translation_invariant_info()["on"]
        return eng

    return [("matrix-free", matrix_free, _first_chain(two.chB)), ("shift-invariant", shift_invariant, _first_chain(d)),
            ("translation-invariant", translation_invariant, lat_ch)]


def _trajectories(eng, ch, ts):
    out = []
    for t in ts:
        acc, out5 = eng.chain_trajectory(ch.p0s[0, t], ch.dt, int(ch.Ls[0, t]), float(ch.us[0, t]))
        out.append((acc, out5, eng.chain_get_x()))
    return out


@pytest.mark.parametrize("store", [0, 1, 2], ids=["matrix-free", "shift-invariant", "translation-invariant"])
def test_a_second_build_of_a_store_built_once_is_refused_and_changes_nothing(G, monkeypatch, store):
    _env(monkeypatch, {})
    name, make, ch = _table_engines(G, monkeypatch)[store]
    F = make()
    F.chain_init(ch.x0s[0], ch.low, ch.high)
    rF = _trajectories(F, ch, range(ch.T))
    F.close()
    E = make()
    E.chain_init(ch.x0s[0], ch.low, ch.high)
    rE = _trajectories(E, ch, [0])
    with pytest.raises(ValueError, match="built once"):
        E.build_G()
    rE += _trajectories(E, ch, range(1, ch.T))        # (no chain_init in between: the refusal left the state alone)
    E.close()
    for t, ((a, o, x), (aF, oF, xF)) in enumerate(zip(rE, rF)):
        assert a == aF and np.array_equal(o, oF) and np.array_equal(x, xF), (name, t)
        assert bool(a) == bool(ch.ref.acc[0, t]), (name, t)


# ----------------------------------------------------------------------------- state that must not survive

def test_chain_and_batch_state_do_not_survive_a_change(G, monkeypatch):
    """After set_data, set_reg, weight, compress_wavelet, upload_G or build_G every call that runs on the chain's or the
    batch's state answers with an error naming its *_init and changes nothing; after the init again the results are
    those of a fresh engine.  (No getter keeps serving the last state: chain_get_x, chain_get_dsyn, batch_get_x refuse
    as well.)"""
    s = lc.two_kernels("two-pass-48x200")
    b = s.B
    ch1, ch = _first_chain(s.chB), s.chB
    _env(monkeypatch, {"GRAVHMC_RESIDENT": 0, "GRAVHMC_BATCH_TEAM": 0})
    N, M = s.spec.N, s.spec.M
    F = G.Engine(N, M)
    _problem(F, b)
    rF1, rF = _single(F, ch1), _rounds(F, ch)
    F.close()

    from gravinv3dhmc_amd.inversion.rng import LegacyDraws
    E = G.Engine(N, M)
    _problem(E, b)
    E.posterior_window(4)
    p0, L, u = ch.p0s[0, 0], int(ch.Ls[0, 0]), float(ch.us[0, 0])
    draws = LegacyDraws(M, [1, 3], 1.0, limit=2, seed=1)
    chain_calls = [("chain_trajectory", lambda: E.chain_trajectory(p0, ch.dt, L, u)),
                   ("run_chain", lambda: E.run_chain(iter([(L, p0, u)]), ch.dt, lambda *a: None, batch=1)),
                   ("chain_get_x", E.chain_get_x), ("chain_get_dsyn", E.chain_get_dsyn), ("posterior_add", E.posterior_add),
                   # (gh_chain_feed_open itself: run_chain asks gh_chain_feed_usable first and would not get there)
                   ("the feeder's open", lambda: E._run_chain_feed(draws, ch.dt, lambda *a: None, 0, 0, False))]
    batch_calls = [("batch_trajectory", lambda: E.batch_trajectory(ch.p0s[:, 0], ch.dt, ch.Ls[:, 0], ch.us[:, 0])),
                   ("batch_run", lambda: E.batch_run(ch.p0s[:, :1], ch.dt, ch.Ls[:, :1], ch.us[:, :1], carry=True)),
                   ("batch_get_x", lambda: E.batch_get_x(0)), ("batch_block_means", E.batch_block_means)]
    changes = [("set_data", lambda: E.set_data(b.dobs, b.gfix)),
               ("set_reg", lambda: E.set_reg(b.reg, b.alpha, b.beta, b.shape, b.mwapr)),
               ("upload_G", lambda: _kernel(E, b, weight=False)),
               ("weight", lambda: E.weight(0.5)),
               ("build_G + weight", lambda: _kernel(E, b, build=True)),
               # (last: the MFMA batch has no compressed forward, a batch_init after it would be refused)
               ("compress_wavelet", lambda: E.compress_wavelet(3, b.shape, lc.WAVELET_THR, 2))]
    for what, change in changes:
        E.chain_init(ch.x0s[0], ch.low, ch.high)
        E.batch_init(ch.x0s, ch.low, ch.high)
        change()
        for name, call in chain_calls:
            with pytest.raises(ValueError, match="gh_chain_init"):
                call()
        for name, call in batch_calls:
            with pytest.raises(ValueError, match="gh_batch_init"):
                call()
        if what in ("upload_G", "build_G + weight", "compress_wavelet"):
            # (an unweighted kernel the next change weights; the device's own entries, compared with the oracle in the
            # scenarios above and not with F's bits; the compressed forward)
            continue
        r1, r = _single(E, ch1), _rounds(E, ch)
        _same_bits(r1, rF1, "single chain after " + what)
        _same_bits(r, rF, "batch after " + what)
    draws.release()
    E.close()
