"""Geometries of the translation-invariant store's suites (test_lattice_host.py, test_gpu_lattice.py): regular prism
grids under gridded data, built the way a user would build them (origin + index * spacing)."""
import ctypes

import numpy as np

LATTICE_ON, LATTICE_CELLS, LATTICE_HEIGHTS, LATTICE_SPACING, LATTICE_RECT, LATTICE_DUPLICATE = range(6)


def geometry(cells, obs, h=(100.0, 100.0), origin=(0.0, 0.0), first=(0, 0), frac=(0.5, 0.5), tops=None, zobs=0.0,
             shuffle=None):
    """cells = (nx, ny, nz) prisms of h = (hx, hy) from origin, layer k between tops[k] and tops[k + 1] (default:
    100 m each, from 0 down); obs = (px, qy) points at origin + (first + index + frac) * h -- frac 0.5: above cell
    centres, 0: above cell corners -- at height zobs.  Returns obs (3, N) with p slowest and bounds6 (M, 6) with
    the layer slowest, then a, then b; shuffle: a seed, both in a random order."""
    nx, ny, nz = cells
    px, qy = obs
    tops = np.arange(nz + 1) * 100.0 if tops is None else np.asarray(tops, dtype=float)
    xe = origin[0] + np.arange(nx + 1) * h[0]
    ye = origin[1] + np.arange(ny + 1) * h[1]
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    b6 = np.stack([xe[a], xe[a + 1], ye[b], ye[b + 1], tops[k], tops[k + 1]], axis=1)
    xo = origin[0] + (first[0] + np.arange(px) + frac[0]) * h[0]
    yo = origin[1] + (first[1] + np.arange(qy) + frac[1]) * h[1]
    p, q = [v.ravel() for v in np.meshgrid(np.arange(px), np.arange(qy), indexing="ij")]
    o = np.stack([xo[p], yo[q], np.full(p.size, float(zobs))])
    if shuffle is not None:
        rng = np.random.default_rng(shuffle)
        o = o[:, rng.permutation(o.shape[1])]
        b6 = b6[rng.permutation(b6.shape[0])]
    return np.ascontiguousarray(o), np.ascontiguousarray(b6)


def c2_linspace(n=10, nz=3):
    """bench.py's C2 geometry at n x n x nz: n points from one end of the mesh to the other, L / (n - 1) apart."""
    from gravinv3dhmc_amd import mesher
    mesh = mesher.PrismMesh((0, 100.0 * n, 0, 100.0 * n, 0, 100.0 * nz), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * n, n), np.linspace(0, 100.0 * n, n))]
    return np.stack([xp, yp, np.zeros_like(xp)]), np.ascontiguousarray(mesh.cell_bounds())


def detect(obs, b6):
    """gh_lattice_detect: (code, dims or None, lat_of_cell (M, 3), cell_of_lat, lat_of_obs (N, 2), obs_of_lat)"""
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    b6 = np.ascontiguousarray(b6, dtype=np.float64)
    N, M = obs.shape[1], b6.shape[0]
    dims = np.zeros(5, dtype=np.int32)
    loc, col = np.full(3 * M, -1, dtype=np.int32), np.full(M, -1, dtype=np.int32)
    loo, ool = np.full(2 * N, -1, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    x, y, z = (np.ascontiguousarray(obs[k]) for k in range(3))
    rc = lib.gh_lattice_detect(N, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), M,
                               b6.ctypes.data_as(dp), dims.ctypes.data_as(ip), loc.ctypes.data_as(ip),
                               col.ctypes.data_as(ip), loo.ctypes.data_as(ip), ool.ctypes.data_as(ip))
    return rc, (tuple(int(v) for v in dims) if rc == LATTICE_ON else None), loc.reshape(M, 3), col, loo.reshape(N, 2), ool
