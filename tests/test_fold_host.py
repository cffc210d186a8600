"""CPU suite: detection of the two grid mirrors the folded store relies on (gh_fold_detect, csrc/host_fold.h),
checked against the geometry in NumPy."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

FOLD_ON, FOLD_OBS, FOLD_CELLS, FOLD_FIXED = 0, 4, 5, 6


def c2_geometry(nx=100, ny=100, nz=50):
    """bench.py's C2 workload: cells and observations in its own order."""
    from gravinv3dhmc_amd import mesher
    mesh = mesher.PrismMesh((0, 100.0 * nx, 0, 100.0 * ny, 0, 100.0 * nz), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * ny, ny), np.linspace(0, 100.0 * nx, nx))]
    return np.stack([xp, yp, np.zeros_like(xp)]), np.ascontiguousarray(mesh.cell_bounds())


def detect(obs, b6):
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    b6 = np.ascontiguousarray(b6, dtype=np.float64)
    N, M = obs.shape[1], b6.shape[0]
    oi = np.full(N, -1, dtype=np.int32)
    co = np.full(M, -1, dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int)
    x, y, z = (np.ascontiguousarray(obs[k]) for k in range(3))
    rc = lib.gh_fold_detect(N, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), M,
                            b6.ctypes.data_as(dp), oi.ctypes.data_as(ip), co.ctypes.data_as(ip))
    return rc, oi.reshape(-1, 4), co.reshape(-1, 4)


def check_tables(obs, b6, oi, co):
    """The tables are a free Z2 x Z2 action by the two mirrors about the centre of the cells' extent."""
    cx = 0.5 * (b6[:, 0].min() + b6[:, 1].max())
    cy = 0.5 * (b6[:, 2].min() + b6[:, 3].max())
    N, M = obs.shape[1], b6.shape[0]
    # every index exactly once: a partition into orbits of four, each led by its smallest index, in order
    assert np.array_equal(np.sort(oi.ravel()), np.arange(N))
    assert np.array_equal(np.sort(co.ravel()), np.arange(M))
    assert np.all(oi[:, 0] == oi.min(axis=1)) and np.all(np.diff(oi[:, 0]) > 0)
    assert np.all(co[:, 0] == co.min(axis=1)) and np.all(np.diff(co[:, 0]) > 0)
    tol = 8 * np.finfo(float).eps * 1e4
    x, y, z = obs
    f = oi[:, 0]
    # s_x, s_y, s_xy of each fundamental observation
    for g, (mx, my) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        i = oi[:, g]
        assert np.abs(x[i] - (2 * cx - x[f] if mx else x[f])).max() <= tol
        assert np.abs(y[i] - (2 * cy - y[f] if my else y[f])).max() <= tol
        assert np.array_equal(z[i], z[f])
    j0 = co[:, 0]
    for g, (mx, my) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        j = co[:, g]
        ex = np.stack([2 * cx - b6[j0, 1], 2 * cx - b6[j0, 0]], 1) if mx else b6[j0, 0:2]
        ey = np.stack([2 * cy - b6[j0, 3], 2 * cy - b6[j0, 2]], 1) if my else b6[j0, 2:4]
        assert np.abs(b6[j, 0:2] - ex).max() <= tol
        assert np.abs(b6[j, 2:4] - ey).max() <= tol
        assert np.array_equal(b6[j, 4:6], b6[j0, 4:6])
    # free: no observation or cell is its own image
    for t in (oi, co):
        for a in range(4):
            for b in range(a + 1, 4):
                assert np.all(t[:, a] != t[:, b])


def test_c2_pairing_is_a_free_action_of_both_mirrors():
    obs, b6 = c2_geometry()
    rc, oi, co = detect(obs, b6)
    assert rc == FOLD_ON
    assert oi.shape == (2500, 4) and co.shape == (125000, 4)
    check_tables(obs, b6, oi, co)


def test_shuffled_cells_and_observations_are_still_paired():
    obs, b6 = c2_geometry(20, 30, 6)
    rng = np.random.default_rng(5)
    po, pc = rng.permutation(obs.shape[1]), rng.permutation(b6.shape[0])
    obs_s, b6_s = obs[:, po], b6[pc]
    rc, oi, co = detect(obs_s, b6_s)
    assert rc == FOLD_ON
    check_tables(obs_s, b6_s, oi, co)
    # the same orbits as the ordered problem's: shuffled position k holds original index po[k]
    rc0, oi0, co0 = detect(obs, b6)
    assert rc0 == FOLD_ON
    orbits = lambda t, back: sorted(tuple(sorted(back[r])) for r in t)  # noqa: E731
    assert orbits(oi, po) == orbits(oi0, np.arange(obs.shape[1]))
    assert orbits(co, pc) == orbits(co0, np.arange(b6.shape[0]))


@pytest.mark.parametrize("case", ["odd_obs_grid", "odd_cell_grid", "moved_obs", "raised_obs", "asym_cells"])
def test_refusals_with_reasons(case):
    obs, b6 = c2_geometry(20, 30, 6)
    want = None
    if case == "odd_obs_grid":
        # 21 x 32 observations on [0, 2000] x [0, 3000]: a line of them on the mirror x = 1000
        yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 32), np.linspace(0, 2000, 21))]
        obs = np.stack([xp, yp, np.zeros_like(xp)])
        want = (FOLD_FIXED,)
    elif case == "odd_cell_grid":
        # 21 x 30 x 6 cells on [0, 2100]: a column of cells across the mirror x = 1050 (22 x 30 observations)
        _, b6 = c2_geometry(21, 30, 6)
        yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2100, 22))]
        obs = np.stack([xp, yp, np.zeros_like(xp)])
        want = (FOLD_FIXED,)
    elif case == "moved_obs":
        obs = obs.copy()
        obs[0, 37] += 1e-6
        want = (FOLD_OBS,)
    elif case == "raised_obs":
        obs = obs.copy()
        obs[2, 11] = 1e-3
        want = (FOLD_OBS,)
    elif case == "asym_cells":
        b6 = b6.copy()
        b6[b6[:, 1] == 2000.0, 1] = 2100.0  # the last column of cells wider: the extent's centre moves
        want = (FOLD_CELLS, FOLD_OBS)
    rc, _, _ = detect(obs, b6)
    assert rc in want, (case, rc)
