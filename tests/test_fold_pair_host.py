"""CPU suite: the diagonal reflection tau on top of the two grid mirrors (gh_fold_detect_pair, csrc/host_fold.h)
and the paired sweep's work list, checked against the geometry in NumPy.

tau: (x, y) -> (cx + (y - cy), cy + (x - cx)), c the centre of the cells' extent.  One refusal case reads "one
observation moved by 1e-6 ... the mirror fold is still detected"; a single moved observation loses its mirror images
too (tests/test_fold_host.py::test_refusals_with_reasons[moved_obs]), so both readings are checked: the observation
alone (no mirrors, hence no pairing) and the observation together with its three mirror images (mirrors kept, tau
lost)."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)
from test_fold_host import c2_geometry, detect

FOLD_ON, FOLD_OBS = 0, 4
PAIR_ON, PAIR_NO_FOLD, PAIR_OBS, PAIR_CELLS = 0, 3, 4, 5


def square_geometry(n_obs, cells, side=2000.0, depth=1000.0, n_obs_y=None):
    """cells = (nx, ny, nz) on [0, side]^2 x [0, depth], n_obs x n_obs_y observations on the same square."""
    from gravinv3dhmc_amd import mesher
    nx, ny, nz = cells
    mesh = mesher.PrismMesh((0, side, 0, side, 0, depth), (depth / nz, side / ny, side / nx))
    n_obs_y = n_obs if n_obs_y is None else n_obs_y
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, side, n_obs_y), np.linspace(0, side, n_obs))]
    return np.stack([xp, yp, np.zeros_like(xp)]), np.ascontiguousarray(mesh.cell_bounds())


def detect_pair(obs, b6):
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    b6 = np.ascontiguousarray(b6, dtype=np.float64)
    N, M = obs.shape[1], b6.shape[0]
    ot = np.full(N, -1, dtype=np.int32)
    ct = np.full(M, -1, dtype=np.int32)
    work = np.full((max(M // 4, 1), 2), -7, dtype=np.int32)
    nw, pr = ctypes.c_int64(-1), ctypes.c_int(-1)
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int)
    x, y, z = (np.ascontiguousarray(obs[k]) for k in range(3))
    rc = lib.gh_fold_detect_pair(N, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), M,
                                 b6.ctypes.data_as(dp), ot.ctypes.data_as(ip), ct.ctypes.data_as(ip),
                                 work.ctypes.data_as(ip), ctypes.byref(nw), ctypes.byref(pr))
    return rc, pr.value, ot, ct, work[:max(nw.value, 0)]


def check_tau(obs, b6, ot, ct):
    cx = 0.5 * (b6[:, 0].min() + b6[:, 1].max())
    cy = 0.5 * (b6[:, 2].min() + b6[:, 3].max())
    tol = 8 * np.finfo(float).eps * max(np.abs(b6[:, :4]).max(), np.abs(obs[:2]).max())
    x, y, z = obs
    N, M = x.size, b6.shape[0]
    assert np.array_equal(ot[ot], np.arange(N)) and np.array_equal(ct[ct], np.arange(M))
    assert np.abs(x[ot] - (cx + (y - cy))).max() <= tol and np.abs(y[ot] - (cy + (x - cx))).max() <= tol
    assert np.array_equal(z[ot], z)
    assert np.abs(b6[ct, 0:2] - (cx + (b6[:, 2:4] - cy))).max() <= tol
    assert np.abs(b6[ct, 2:4] - (cy + (b6[:, 0:2] - cx))).max() <= tol
    assert np.array_equal(b6[ct, 4:6], b6[:, 4:6])


def check_work(co, ct, work):
    """Every orbit exactly once; the partner is the orbit of the tau images; leaders ascending, smaller index leads."""
    n_orb = co.shape[0]
    orbit_of = np.empty(co.size, dtype=np.int64)
    orbit_of[co.ravel()] = np.repeat(np.arange(n_orb), 4)
    partner = orbit_of[ct[co[:, 0]]]
    for k in range(1, 4):
        assert np.array_equal(orbit_of[ct[co[:, k]]], partner)
    lead, other = work[:, 0].astype(np.int64), work[:, 1].astype(np.int64)
    assert np.all(np.diff(lead) > 0)
    single = other < 0
    assert np.all(other[single] == -1) and np.array_equal(partner[lead[single]], lead[single])
    assert np.array_equal(partner[lead[~single]], other[~single]) and np.all(lead[~single] < other[~single])
    assert np.array_equal(np.sort(np.concatenate([lead, other[~single]])), np.arange(n_orb))
    return int((~single).sum()), int(single.sum())


def test_c2_pairs_and_single_orbits():
    obs, b6 = c2_geometry()
    rc, pr, ot, ct, work = detect_pair(obs, b6)
    assert rc == FOLD_ON and pr == PAIR_ON
    check_tau(obs, b6, ot, ct)
    _, _, co = detect(obs, b6)
    assert check_work(co, ct, work) == (61250, 2500)
    assert work.shape[0] == 63750


def test_shuffled_problem_has_the_same_pairs():
    obs, b6 = square_geometry(20, (20, 20, 6))
    rng = np.random.default_rng(5)
    po, pc = rng.permutation(obs.shape[1]), rng.permutation(b6.shape[0])
    obs_s, b6_s = obs[:, po], b6[pc]
    rc, pr, ot, ct, work = detect_pair(obs_s, b6_s)
    assert rc == FOLD_ON and pr == PAIR_ON
    check_tau(obs_s, b6_s, ot, ct)
    _, _, co = detect(obs_s, b6_s)
    n_pairs, n_single = check_work(co, ct, work)
    rc0, pr0, ot0, ct0, work0 = detect_pair(obs, b6)
    assert rc0 == FOLD_ON and pr0 == PAIR_ON
    check_tau(obs, b6, ot0, ct0)
    _, _, co0 = detect(obs, b6)
    assert check_work(co0, ct0, work0) == (n_pairs, n_single) == (10 * 9 // 2 * 6, 10 * 6)
    # the same involution and the same pairs of orbits: shuffled position k holds original index po[k] / pc[k]
    assert np.array_equal(po[ot], ot0[po]) and np.array_equal(pc[ct], ct0[pc])

    def pairs(co_, work_, back):
        cells = lambda o: tuple(sorted(back[co_[o]]))  # noqa: E731
        return sorted(tuple(sorted([cells(a)] + ([cells(b)] if b >= 0 else []))) for a, b in work_)
    assert pairs(co, work, pc) == pairs(co0, work0, np.arange(b6.shape[0]))
    # deterministic
    again = detect_pair(obs_s, b6_s)
    assert np.array_equal(again[4], work) and np.array_equal(again[2], ot) and np.array_equal(again[3], ct)


@pytest.mark.parametrize("case", ["cells_20x30", "dx_ne_dy", "obs_20x30", "moved_orbit"])
def test_refusals_keep_the_mirror_fold(case):
    if case == "cells_20x30":
        obs, b6 = c2_geometry(20, 30, 6)           # [0, 2000] x [0, 3000], 20 x 30 observations
        want = (PAIR_OBS, PAIR_CELLS)
    elif case == "dx_ne_dy":
        obs, b6 = square_geometry(20, (10, 20, 5))  # a square extent, cells 200 x 100
        want = (PAIR_CELLS,)
    elif case == "obs_20x30":
        obs, b6 = square_geometry(20, (10, 10, 5), n_obs_y=30)
        want = (PAIR_OBS,)
    else:
        # an observation and its three mirror images moved by 1e-6 along x, away from the centre
        obs, b6 = square_geometry(20, (10, 10, 5))
        _, oi, _ = detect(obs, b6)
        orbit = oi[np.any(oi == 37, axis=1)][0]
        obs = obs.copy()
        obs[0, orbit] += 1e-6 * np.sign(obs[0, orbit] - 1000.0)
        want = (PAIR_OBS,)
    rc, pr, _, _, work = detect_pair(obs, b6)
    assert rc == FOLD_ON, (case, rc)
    assert pr in want, (case, pr)
    assert work.shape[0] == 0
    assert detect(obs, b6)[0] == FOLD_ON


def test_one_moved_observation_has_neither_mirrors_nor_pairing():
    obs, b6 = square_geometry(20, (10, 10, 5))
    obs = obs.copy()
    obs[0, 37] += 1e-6
    rc, pr, _, _, work = detect_pair(obs, b6)
    assert rc == FOLD_OBS and pr == PAIR_NO_FOLD and work.shape[0] == 0
