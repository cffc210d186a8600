"""The gravity fields of tesseroids (spherical prisms) on the GPU.

Mirror of the reference's `gravmag.tesseroid.gz` (gravmag/tesseroid.py:421-431 -> _dispatcher
:156-186 -> _forward_model :189-232 -> _tesseroid_numba.gz, _tesseroid_numba.py:32-71): same
arguments and return `(result, kernel2d)`; adaptive 2x2x2 Gauss-Legendre quadrature with the
distance-size ratio `ratio` (1.6 for gz) and a 100-entry subdivision stack.  Likewise its other
fields (tesseroid.py:324-508 -> _tesseroid_numba.py:161-341): `potential` (G per g/cm^3), `geoid` (m),
`gx`, `gy` (mGal) and the gradient tensor `gxx`, `gxy`, `gxz`, `gyy`, `gyz`, `gzz` (Eotvos), with the
reference's default ratios (RATIO_V = 1, RATIO_G = 1.6, RATIO_GG = 8).  The local frame of the
computation point is x north, y east, z up, except gz (z down).  `return_kernel=False` computes
`result` without storing the kernel (the matrix-free passes), so any number of observations and any
mesh whose kernel would not fit in memory work; `gz` keeps its dense assembly.
"""
import warnings

import numpy as np

from .. import _lib
from ..engine import Engine
from ._common import active_cells

RATIO_V = 1        # tesseroid.py:76
RATIO_G = 1.6      # tesseroid.py:77
RATIO_GG = 8       # tesseroid.py:78
STACK_SIZE = 100   # tesseroid.py:79

_WARN_DIVIDE = ("Stopped dividing a tesseroid because it's dimensions would be below the minimum "
                "numerical threshold (1e-6 degrees or 1e-3 m). Will compute without division. "
                "Cannot guarantee the accuracy of the solution.")
_WARN_SMALL = ("Encountered tesseroid with dimensions smaller than the numerical threshold "
               "(1e-6 degrees or 1e-3 m). Ignoring this tesseroid.")


def _valid_cells(bounds, rho):
    """tesseroid.py:126-153: assert w<=e, s<=n, top>=bottom; drop degenerate cells with a warning."""
    w, e, s, n, top, bottom = bounds.T
    bad = ~((w <= e) & (s <= n) & (top >= bottom))
    if bad.any():
        raise AssertionError("Invalid tesseroid dimensions {}".format(list(bounds[np.flatnonzero(bad)[0]])))
    tiny = ((e - w) <= 1e-6) | ((n - s) <= 1e-6) | ((top - bottom) <= 1e-3)
    if tiny.any():
        warnings.warn(_WARN_SMALL, RuntimeWarning)
    return tiny


def build_engine(lon, lat, height, model, dens=None, ratio=RATIO_G, device=0, component=None, matrix_free=False):
    """Assemble the kernel of the non-degenerate cells; returns (engine, densities, n_dropped).

    component: a gravity field other than gz (a name of _lib.COMPONENTS; None is gz).  matrix_free: never
    store the kernel (the entries are evaluated inside each pass; the subdivision's warnings and overflow
    are still reported by build_G)."""
    lon, lat, height = (np.asarray(a, dtype=np.float64) for a in (lon, lat, height))
    assert lon.shape == lat.shape == height.shape, "Input coordinate arrays must have same shape"
    assert ratio > 0, "Invalid ratio {}. Must be > 0.".format(ratio)
    bounds, rho, _ = active_cells(model, dens)
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'density' property (and no dens given)")
    tiny = _valid_cells(bounds, rho)
    if tiny.all():
        raise ValueError("every tesseroid is below the numerical size threshold")
    keep = ~tiny
    eng = Engine(lon.size, int(keep.sum()), device=device)
    if component is None and not matrix_free:
        eng.set_obs(lon, lat, height)
        eng.set_cells(bounds[keep], _lib.CELL_TESSEROID, ratio)
        eng.build_G()
    else:
        try:
            if matrix_free:
                eng.set_matrix_free(True)
            eng.set_obs(lon, lat, height)
            eng.set_cells(bounds[keep], _lib.CELL_TESSEROID, ratio, component=component)
            eng.build_G()
        except Exception:
            eng.close()
            raise
    if eng.kernel_stats()["warn_cells"] > 0:
        warnings.warn(_WARN_DIVIDE, RuntimeWarning)
    return eng, rho[keep], int(tiny.sum())


def gz(lon, lat, height, model, dens=None, ratio=RATIO_G, njobs=1, pool=None,
       return_kernel=True, device=0):
    """Radial (z down) gravity of the tesseroid model and its sensitivity matrix, mGal.

    Degenerate cells (tesseroid.py:139-147) are skipped by the reference's loop WITHOUT
    advancing its column counter, so the kept cells fill the leading columns of kernel2d and
    one all-zero column per skipped cell trails; the same shape is returned here."""
    assert njobs > 0, "Invalid number of jobs {}. Must be > 0.".format(njobs)
    eng, rho, ndrop = build_engine(lon, lat, height, model, dens, ratio, device)
    try:
        result = eng.forward(rho)
        kernel2d = None
        if return_kernel:
            kernel2d = eng.download_G()
            if ndrop:
                kernel2d = np.asfortranarray(
                    np.hstack([kernel2d, np.zeros((kernel2d.shape[0], ndrop))]))
    finally:
        eng.close()
    return result, kernel2d


def _field(component, lon, lat, height, model, dens, ratio, njobs, return_kernel, device):
    """(result, kernel2d) of one field other than gz.  The checks, warnings, `dens` override, cells without
    density and dropped degenerate cells (with their trailing zero columns) are gz's.  With return_kernel the
    kernel is assembled densely (N <= 16384 per device) and `result` is its product with the densities;
    without it `result` comes from the matrix-free forward pass and no kernel is ever stored."""
    assert njobs > 0, "Invalid number of jobs {}. Must be > 0.".format(njobs)
    eng, rho, ndrop = build_engine(lon, lat, height, model, dens, ratio, device, component=component,
                                   matrix_free=not return_kernel)
    try:
        result = eng.forward(rho)
        kernel2d = None
        if return_kernel:
            kernel2d = eng.download_G()
            if ndrop:
                kernel2d = np.asfortranarray(
                    np.hstack([kernel2d, np.zeros((kernel2d.shape[0], ndrop))]))
    finally:
        eng.close()
    return result, kernel2d


def potential(lon, lat, height, model, dens=None, ratio=RATIO_V, njobs=1, pool=None,
              return_kernel=True, device=0):
    """Gravitational potential of the tesseroid model and its kernel (G times the sum of kernelV)."""
    return _field("potential", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def geoid(lon, lat, height, model, dens=None, ratio=RATIO_V, njobs=1, pool=None,
          return_kernel=True, device=0):
    """Geoid height of the tesseroid model and its kernel in m: the potential times 1/g0 (G/g0)."""
    return _field("geoid", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gx(lon, lat, height, model, dens=None, ratio=RATIO_G, njobs=1, pool=None,
       return_kernel=True, device=0):
    """North gravity component in mGal and its kernel."""
    return _field("gx", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gy(lon, lat, height, model, dens=None, ratio=RATIO_G, njobs=1, pool=None,
       return_kernel=True, device=0):
    """East gravity component in mGal and its kernel.

    As in the reference (tesseroid.py:397-398), gy is scaled with the spherical constant Gs = 6.673e-11,
    1000 times smaller than the G of gx, gz and every other field: values are 1000 times smaller than a
    scaling with G would give.  The quirk is kept so that results match the reference."""
    return _field("gy", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gxx(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gxx gravity gradient in Eotvos and its kernel."""
    return _field("gxx", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gxy(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gxy gravity gradient in Eotvos and its kernel."""
    return _field("gxy", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gxz(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gxz gravity gradient in Eotvos and its kernel."""
    return _field("gxz", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gyy(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gyy gravity gradient in Eotvos and its kernel."""
    return _field("gyy", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gyz(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gyz gravity gradient in Eotvos and its kernel."""
    return _field("gyz", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)


def gzz(lon, lat, height, model, dens=None, ratio=RATIO_GG, njobs=1, pool=None,
        return_kernel=True, device=0):
    """gzz gravity gradient in Eotvos and its kernel (z up)."""
    return _field("gzz", lon, lat, height, model, dens, ratio, njobs, return_kernel, device)
