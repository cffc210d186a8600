"""The generator of tests/lifecycle_cases.py on the CPU: every scenario of tests/test_gpu_context_lifecycle.py has
accepted and rejected trajectories with a Metropolis margin of at least 1e-6 on the oracle, the NumPy potential with
separate operators reproduces the oracle when nothing is stale, and every restatement of "what the device would
compute with the stale store" lies at least SHARP = 1e-6 (relative) from the oracle's result on the final
configuration, in every quantity the device test compares under its bound of 1e-10 (1e-12 for the stream).  A decision
that differs counts as an infinite distance.  The smallest distance and margin found are printed."""
import numpy as np
import pytest

import lifecycle_cases as lc
from helpers import relmax

FOUND = {"distance": np.inf, "margin": np.inf}


def _note(what, dist=None, margin=None):
    if dist is not None:
        FOUND["distance"] = min(FOUND["distance"], dist)
    if margin is not None:
        FOUND["margin"] = min(FOUND["margin"], margin)
    print("%s: smallest distance %s, smallest margin %s | so far %.3e / %.3e"
          % (what, "%.3e" % dist if dist is not None else "-", "%.3e" % margin if margin is not None else "-",
             FOUND["distance"], FOUND["margin"]))


def _sharp(ch, stale, what):
    d = lc.distances(ch, ch.ref, stale)
    for key, v in d.items():
        assert v >= lc.SHARP, (what, key, v)
    return min(d.values())


def _faithful(ch, fresh, what):
    d = lc.distances(ch, ch.ref, fresh)
    assert max(d.values()) <= lc.TOL, (what, d)


@pytest.mark.parametrize("cid", ["two-pass-48x200", "two-pass-37x203", "team-3585x7"])
def test_kernel_a_then_b_stale_operand_copy_cannot_hide(cid):
    s = lc.two_kernels(cid)
    assert s.A.K.shape == s.B.K.shape == (s.spec.N, s.spec.M)
    assert relmax(s.A.Aw, s.B.Aw) > 0.1 and relmax(s.A.wm, s.B.wm) > 0.1 and relmax(s.A.dobs, s.B.dobs) > 1e-3
    _faithful(s.chB, s.fresh_split(), cid)
    _note(cid, _sharp(s.chB, s.stale_gb(), cid), min(s.chA.margin, s.chB.margin))


def test_bootstrap_batch_stale_operand_copy_cannot_hide():
    s = lc.bscg()
    ref = s.runs[1]["ref"]
    assert ref.n_entries.min() >= 1                     # every replicate produced misfit rows to compare
    for name, v, w in zip(lc.BSCG_NAMES, s.fresh_split(), ref.results()):
        assert relmax(v, w) <= 1e-12, name
    worst = np.inf
    for name, v, w in zip(lc.BSCG_NAMES, s.stale_gb(), ref.results()):
        d = min(relmax(v[b], w[b]) for b in range(lc.BSCG["B"]))      # every replicate sees it
        assert d >= lc.SHARP, (name, d)
        worst = min(worst, d)
    _note("bootstrap batch", worst)


def test_batch_before_weights_unweighted_adjoint_cannot_hide():
    s = lc.before_weights()
    _faithful(s.chW, s.fresh_split(), "before weights")
    _note("batch before weights", _sharp(s.chW, s.stale_gb(), "before weights"), min(s.chU.margin, s.chW.margin))


def test_wavelet_rows_of_the_old_kernel_cannot_hide():
    w = lc.wavelet()
    assert w.csrA.shape[1] != w.csrB.shape[1]          # another Mp: the second compression cannot reuse the blocks
    _faithful(w.ch, w.fresh_split(), "wavelet")
    worst = _sharp(w.ch, w.stale_chain(), "wavelet chain")
    stale = w.stale_potential()
    for x in w.xs:
        a, b = stale.misfit_and_grad(x), w.PB_dense.misfit_and_grad(x)
        d = min(abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]))
        assert d >= lc.SHARP
        worst = min(worst, d)
    # the compressed forward of B is itself visible against the dense one: the chain after the second compression
    # cannot pass on the dense forward
    worst = min(worst, _sharp(w.ch, lc.replay(w.PB_dense, w.ch), "wavelet chain on the dense forward"))
    # CSR values: the rows of A against those of B in B's layout
    A3 = w.ow.compress_kernel(w.A.Aw, 1, None, lc.WAVELET_THR).toarray()
    d = relmax(A3, w.csrB.toarray())
    assert d >= lc.SHARP
    _note("wavelet", min(worst, d), w.ch.margin)


def test_cross_gradient_normalisers_of_the_old_weights_cannot_hide():
    from conftest import gold
    c = lc.crossgrad()
    z = gold("joint_small.npz")
    # the restated weighting of a joint store reproduces the reference's (the golden file's)
    assert relmax(c.wmA, z["a_wm"]) <= 1e-13 and relmax(c.AwA, z["a_Aw"]) <= 1e-13 and relmax(c.stdA, z["a_std"]) <= 1e-13
    assert np.abs(c.wmB / c.wmA - 1.0).min() > 1e-4       # no cell keeps its weight
    worst = _sharp(c.ch, c.stale_chain(), "cross-gradient chain")
    for mw in c.mws:
        a, b = c.phi(mw, c.wmA), c.phi(mw, c.wmB)
        d = min(abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]))
        assert d >= lc.SHARP
        worst = min(worst, d)
    # the coupling is visible in U at the chains' centre
    U = c.PB.misfit_and_grad(c.centre)
    assert c.lam * c.PB.last_phi > 1e-2 * U[0]
    _note("cross-gradient", worst, c.ch.margin)


def test_stream_weights_cannot_hide():
    s = lc.stream()
    assert len(s.rows(s.chA)) >= 2 and len(s.rows(s.chB)) >= 2 * lc.STREAM_BATCH
    d1 = lc.stream_distance(s.stale_before_weights(), s.expected_before_weights())
    d2 = lc.stream_distance(s.stale_outlives(), s.expected_outlives())
    assert d1 >= lc.SHARP and d2 >= lc.SHARP
    # the rows of B lie inside the histogram's bounds, so the quantiles are those of the samples
    for x in s.rows(s.chB):
        m = x / s.B.wm
        assert np.all(m > s.lo) and np.all(m < s.hi)
    _note("stream", min(d1, d2), min(s.chA.margin, s.chB.margin))


def test_folded_store_of_the_old_geometry_cannot_hide():
    f = lc.fold()
    worst = min(_sharp(f.ch[k], f.stale_fold(k), "fold stage %d" % k) for k in (1, 2))
    _note("fold", worst, min(ch.margin for ch in f.ch))


def test_smallest_distance_and_margin():
    """(runs last: what the tests above found)"""
    for cid in ("two-pass-48x200", "two-pass-37x203", "team-3585x7"):
        test_kernel_a_then_b_stale_operand_copy_cannot_hide(cid)
    test_bootstrap_batch_stale_operand_copy_cannot_hide()
    test_batch_before_weights_unweighted_adjoint_cannot_hide()
    test_wavelet_rows_of_the_old_kernel_cannot_hide()
    test_cross_gradient_normalisers_of_the_old_weights_cannot_hide()
    test_stream_weights_cannot_hide()
    test_folded_store_of_the_old_geometry_cannot_hide()
    print("smallest sharpness distance %.3e (bar %.0e), smallest Metropolis margin %.3e (bar %.0e)"
          % (FOUND["distance"], lc.SHARP, FOUND["margin"], lc.MARGIN))
    assert FOUND["distance"] >= lc.SHARP and FOUND["margin"] >= lc.MARGIN
