"""CPU suite: detection of the structure the translation-invariant store relies on (gh_lattice_detect,
csrc/host_lattice.h) -- cells a full product of equal x-intervals, equal y-intervals and layers, observations a full
rectangle of the lattice of the cells' spacings at one height -- checked against the geometry in NumPy."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)
from lattice_cases import (LATTICE_CELLS, LATTICE_DUPLICATE, LATTICE_HEIGHTS, LATTICE_ON, LATTICE_RECT, LATTICE_SPACING,
                           c2_linspace, detect, geometry)


def check_maps(obs, b6, dims, loc, col, loo, ool):
    """The maps place every cell and observation on the lattice and invert each other."""
    nx, ny, nz, px, qy = dims
    N, M = obs.shape[1], b6.shape[0]
    assert nx * ny * nz == M and px * qy == N
    k, a, b = loc.T
    p, q = loo.T
    assert k.min() == 0 and k.max() == nz - 1 and a.min() == 0 and a.max() == nx - 1 and b.min() == 0 and b.max() == ny - 1
    assert p.min() == 0 and p.max() == px - 1 and q.min() == 0 and q.max() == qy - 1
    # inverses (so every lattice site is taken exactly once)
    assert np.array_equal(col[(k * nx + a) * ny + b], np.arange(M))
    assert np.array_equal(ool[p * qy + q], np.arange(N))
    mag = max(np.abs(b6[:, :4]).max(), np.abs(obs[:2]).max())
    tol = 8 * np.finfo(float).eps * mag
    x0, y0 = b6[:, 0].min(), b6[:, 2].min()
    hx, hy = (b6[:, 1].max() - x0) / nx, (b6[:, 3].max() - y0) / ny
    assert np.abs(b6[:, 0] - (x0 + a * hx)).max() <= 2 * tol and np.abs(b6[:, 1] - (x0 + (a + 1) * hx)).max() <= 2 * tol
    assert np.abs(b6[:, 2] - (y0 + b * hy)).max() <= 2 * tol and np.abs(b6[:, 3] - (y0 + (b + 1) * hy)).max() <= 2 * tol
    # one (z1, z2), bit for bit, per layer, layers ordered by their values
    layers = sorted(set(map(tuple, b6[:, 4:6])))
    assert len(layers) == nz
    assert np.array_equal(b6[:, 4:6], np.array(layers)[k])
    # observations: one height, the lattice of the cells' spacings
    assert np.all(obs[2] == obs[2, 0])
    assert np.abs(obs[0] - (obs[0].min() + p * hx)).max() <= 2 * tol * (1 + px / nx)
    assert np.abs(obs[1] - (obs[1].min() + q * hy)).max() <= 2 * tol * (1 + qy / ny)


FOUND = {
    "centres 7x5x3 under 7x5": dict(cells=(7, 5, 3), obs=(7, 5)),
    "9x8 beyond the mesh on every side": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2)),
    "3x2 inside": dict(cells=(7, 5, 3), obs=(3, 2), first=(2, 1)),
    "corners 8x6 on z = 0": dict(cells=(7, 5, 3), obs=(8, 6), frac=(0.0, 0.0)),
    "spacing 2000/7, offsets 317.3 / -911.7": dict(cells=(7, 5, 3), obs=(7, 5), h=(2000.0 / 7, 2000.0 / 7),
                                                    origin=(317.3, -911.7)),
    "coordinates near 1e6": dict(cells=(7, 5, 3), obs=(8, 6), h=(2000.0 / 7, 2000.0 / 7), origin=(1.0e6 + 0.3, -1.0e6 - 0.7),
                                 frac=(0.0, 0.0)),
    "shuffled": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(2000.0 / 7, 150.0), shuffle=5),
    "nx = 1": dict(cells=(1, 5, 3), obs=(4, 5)),
    "ny = 1": dict(cells=(7, 1, 3), obs=(7, 3), first=(0, -1)),
    "nz = 1": dict(cells=(7, 5, 1), obs=(7, 5)),
    "layers of unequal thickness": dict(cells=(4, 3, 4), obs=(4, 3), tops=(0.0, 30.0, 170.0, 180.5, 1000.0)),
    "many points over few cells": dict(cells=(4, 4, 1), obs=(130, 130), first=(-63, -63), h=(2000.0 / 7, 2000.0 / 7),
                                       origin=(317.3, -911.7)),
}


@pytest.mark.parametrize("name", sorted(FOUND))
def test_structure_found_and_maps_invert(name):
    kw = FOUND[name]
    obs, b6 = geometry(**kw)
    rc, dims, loc, col, loo, ool = detect(obs, b6)
    assert rc == LATTICE_ON, name
    assert dims == tuple(kw["cells"]) + tuple(kw["obs"])
    check_maps(obs, b6, dims, loc, col, loo, ool)


def test_maps_invert_the_shuffle():
    kw = dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(2000.0 / 7, 150.0))
    obs0, b0 = geometry(**kw)
    obs1, b1 = geometry(shuffle=11, **kw)
    rc0, dims0, _, col0, _, ool0 = detect(obs0, b0)
    rc1, dims1, _, col1, _, ool1 = detect(obs1, b1)
    assert rc0 == LATTICE_ON and rc1 == LATTICE_ON and dims0 == dims1
    # the unshuffled order IS the lattice order; through the maps the shuffled arrays are the unshuffled ones
    assert np.array_equal(col0, np.arange(b0.shape[0])) and np.array_equal(ool0, np.arange(obs0.shape[1]))
    assert np.array_equal(b1[col1], b0) and np.array_equal(obs1[:, ool1], obs0)


def _base():
    return geometry(cells=(7, 5, 3), obs=(7, 5), h=(2000.0 / 7, 2000.0 / 7), origin=(317.3, -911.7))


def test_c2_linspace_geometry_is_not_on_the_cells_spacing():
    obs, b6 = c2_linspace()
    assert detect(obs, b6)[0] == LATTICE_SPACING
    obs, b6 = c2_linspace(100, 2)  # bench.py's own extent along x and y
    assert detect(obs, b6)[0] == LATTICE_SPACING


def test_one_observation_moved_by_a_millionth_of_the_spacing():
    obs, b6 = _base()
    obs[0, 17] += 1e-6 * 2000.0 / 7
    assert detect(obs, b6)[0] == LATTICE_SPACING
    obs, b6 = _base()
    obs[1, 0] -= 1e-6 * 2000.0 / 7
    assert detect(obs, b6)[0] == LATTICE_SPACING


def test_one_height_changed_by_one_ulp():
    obs, b6 = geometry(cells=(7, 5, 3), obs=(7, 5), zobs=-1.0)
    obs[2, 9] = np.nextafter(obs[2, 9], 0.0)
    assert detect(obs, b6)[0] == LATTICE_HEIGHTS


def test_one_observation_removed():
    obs, b6 = _base()
    for i in (0, 17, obs.shape[1] - 1):
        assert detect(np.delete(obs, i, axis=1), b6)[0] == LATTICE_RECT
    # a whole inner row of the rectangle missing: a gap in the lattice
    assert detect(obs[:, (obs[0] < obs[0, 10]) | (obs[0] > obs[0, 10])], b6)[0] == LATTICE_RECT


def test_one_cell_removed():
    obs, b6 = _base()
    for j in (0, 40, b6.shape[0] - 1):
        assert detect(obs, np.delete(b6, j, axis=0))[0] == LATTICE_CELLS


def test_one_duplicate_point_or_cell():
    obs, b6 = _base()
    assert detect(np.concatenate([obs, obs[:, 3:4]], axis=1), b6)[0] == LATTICE_DUPLICATE
    assert detect(obs, np.concatenate([b6, b6[12:13]], axis=0))[0] == LATTICE_DUPLICATE


def test_one_column_of_cells_one_percent_wider():
    obs, b6 = _base()
    wide = b6.copy()
    last = wide[:, 1] == wide[:, 1].max()
    wide[last, 1] += 0.01 * 2000.0 / 7
    assert detect(obs, wide)[0] == LATTICE_CELLS
    # ... and an inner column, its neighbour narrower by as much
    wide = b6.copy()
    edge = np.unique(b6[:, 1])[2]
    wide[wide[:, 1] == edge, 1] += 0.01 * 2000.0 / 7
    wide[wide[:, 0] == edge, 0] += 0.01 * 2000.0 / 7
    assert detect(obs, wide)[0] == LATTICE_CELLS


def test_a_segmented_mesh_is_not_a_regular_product():
    obs, b6 = _base()
    # the top layer's cells split in two along x: twice the columns there, not a product
    top = b6[:, 4] == b6[:, 4].min()
    left, right = b6[top].copy(), b6[top].copy()
    mid = 0.5 * (left[:, 0] + left[:, 1])
    left[:, 1], right[:, 0] = mid, mid
    assert detect(obs, np.concatenate([b6[~top], left, right]))[0] == LATTICE_CELLS
