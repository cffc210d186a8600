"""Host checks of the cross-gradient coupling: the NumPy restatement the GPU suite compares against
(tests/crossgrad_host.py) against central differences and on models whose gradients are parallel, and the
three entry points in the header and in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from crossgrad_host import cross_gradient


def _case(shape, geometric, seed):
    rng = np.random.default_rng(seed)
    m = int(np.prod(shape))
    hz = 1.0 * 1.3 ** np.arange(shape[0] - 1) if geometric else np.ones(shape[0] - 1)
    hx, hy = (1.5, 2.25) if geometric else (1.0, 1.0)
    wm = rng.uniform(0.5, 2.0, size=2 * m)
    return m, hx, hy, hz, wm, rng


@pytest.mark.parametrize("shape,geometric", [((3, 4, 5), False), ((4, 5, 6), True)])
def test_restatement_gradient_against_central_differences(shape, geometric):
    m, hx, hy, hz, wm, rng = _case(shape, geometric, 11)
    scale = (1.0, 1.0) if not geometric else (0.7, 3.0)
    mw = rng.normal(size=2 * m)
    phi, grad, t = cross_gradient(mw, wm, shape, hx, hy, hz, scale)
    assert phi > 0 and t.shape == (m, 3)
    assert abs(phi - np.sum(t * t)) <= 1e-14 * phi
    eps = 1e-5
    num = np.empty(2 * m)
    for j in range(2 * m):
        e = np.zeros(2 * m)
        e[j] = eps
        num[j] = (cross_gradient(mw + e, wm, shape, hx, hy, hz, scale)[0]
                  - cross_gradient(mw - e, wm, shape, hx, hy, hz, scale)[0]) / (2 * eps)
    dev = np.abs(grad - num).max() / np.abs(grad).max()
    print("shape %r: analytic against central differences %.2e of the largest entry" % (shape, dev))
    assert dev <= 1e-7


@pytest.mark.parametrize("shape,geometric", [((3, 4, 5), False), ((4, 5, 6), True)])
def test_restatement_vanishes_for_linearly_related_models(shape, geometric):
    m, hx, hy, hz, wm, rng = _case(shape, geometric, 12)
    u = rng.normal(size=m)
    w = -2.5 * u + 0.75
    mw = np.concatenate([u, w]) * wm
    phi_rand = cross_gradient(rng.normal(size=2 * m) * wm, wm, shape, hx, hy, hz)[0]
    phi, grad, t = cross_gradient(mw, wm, shape, hx, hy, hz)
    # (each component of t is the difference of two products equal up to their rounding, ~1e-16 of |Du| |Dw|: Phi is
    # ~1e-32 of the Phi of unrelated models of the same size)
    print("Phi of w = a u + b: %.2e (unrelated models: %.2e)" % (phi, phi_rand))
    assert phi <= 1e-24 * phi_rand
    assert np.abs(grad).max() <= 1e-12
    # values on a dyadic grid, unit weights, dyadic spacings: every operation is exact and so is the zero
    ui = rng.integers(-8, 9, size=m).astype(np.float64)
    hz2 = 2.0 ** np.arange(shape[0] - 1)
    phi, grad, t = cross_gradient(np.concatenate([ui, 2.0 * ui + 3.0]), np.ones(2 * m), shape, 1.0, 2.0, hz2)
    assert phi == 0.0 and not grad.any() and not t.any()
    # one model flat: exactly zero whatever the other is (flat at 0 under any weights -- mw wm / wm need not give a
    # constant back to the last bit -- and at any value under unit weights)
    phi, grad, t = cross_gradient(np.concatenate([u, np.zeros(m)]) * wm, wm, shape, hx, hy, hz)
    assert phi == 0.0 and not grad.any() and not t.any()
    phi, grad, t = cross_gradient(np.concatenate([np.full(m, 0.3), u]), np.ones(2 * m), shape, hx, hy, hz)
    assert phi == 0.0 and not grad.any() and not t.any()


def test_cross_gradient_entry_points_declared_and_exported(built_lib):
    from gravinv3dhmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gravhmc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in ("gh_set_cross_gradient", "gh_cross_gradient_eval", "gh_cross_gradient_last"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
