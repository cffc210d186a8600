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

The magnetic fields `bx`, `by`, `bz` (north, east, down at the observation) and `tf` of a magnetization VECTOR per
cell, given north-east-down at the cell's centre, have no counterpart in the reference: by Poisson's relation
they are the six second derivatives above, evaluated in one traversal of the subdivision, times the rotation
`local_frame_rotation` between the cell's and the observation's frames (uT; CM * T2NT).
"""
import warnings

import numpy as np

from .. import _lib
from ..engine import Engine
from ._common import active_cells, active_cells_mag

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


# ----------------------------------------------------------------------------- the magnetic fields

def _frame(lon, lat):
    """North, east and up unit vectors (ECEF) at longitude / latitude in degrees, each (..., 3)."""
    lam, phi = np.deg2rad(np.asarray(lon, dtype=np.float64)), np.deg2rad(np.asarray(lat, dtype=np.float64))
    sl, cl, sp, cp = np.sin(lam), np.cos(lam), np.sin(phi), np.cos(phi)
    zero = np.zeros_like(sl)
    return (np.stack([-sp * cl, -sp * sl, cp], axis=-1), np.stack([-sl, cl, zero], axis=-1),
            np.stack([cp * cl, cp * sl, sp], axis=-1))


def local_frame_rotation(lon_o, lat_o, lon_c, lat_c):
    """Q = [n_o e_o u_o]^T [n_c e_c -u_c]: takes a vector given north-east-DOWN at (lon_c, lat_c) to its components
    north-east-UP at (lon_o, lat_o), degrees.  Scalars give a (3, 3) array, arrays (broadcast against each other)
    (..., 3, 3).  The magnetic fields below rotate every cell's magnetization with it; a global inducing field
    B0 given in ECEF is (m_N, m_E, m_D) = [n_c e_c -u_c]^T B0 chi / mu0 per cell."""
    lon_o, lat_o, lon_c, lat_c = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64)
                                                       for a in (lon_o, lat_o, lon_c, lat_c)))
    no, eo, uo = _frame(lon_o, lat_o)
    nc, ec, uc = _frame(lon_c, lat_c)
    O = np.stack([no, eo, uo], axis=-2)           # rows: the observation's axes
    Cc = np.stack([nc, ec, -uc], axis=-1)         # columns: the cell's axes
    return O @ Cc


def _field_directions(inc, dec, n):
    """(n, 3) unit vectors (cos I cos D, cos I sin D, sin I) from scalars or one inclination / declination per
    observation point, in degrees."""
    inc, dec = np.asarray(inc, dtype=np.float64), np.asarray(dec, dtype=np.float64)
    for a in (inc, dec):
        if a.ndim > 0 and a.size != n:
            raise ValueError("inc and dec must be scalars or one value per observation point (%d), got %d"
                             % (n, a.size))
    inc, dec = np.broadcast_to(inc.ravel() if inc.ndim else inc, (n,)), np.broadcast_to(dec.ravel() if dec.ndim else dec, (n,))
    i, d = np.deg2rad(inc), np.deg2rad(dec)
    return np.ascontiguousarray(np.stack([np.cos(i) * np.cos(d), np.cos(i) * np.sin(d), np.sin(i)], axis=1))


_MAG_ROWS = 16384  # observation points of one tesseroid magnetization context


def _b_field(component, lon, lat, height, model, pmag, ratio, njobs, return_kernel, device, fdir=None):
    """(result, K) of one magnetic component.  The checks and RuntimeWarnings are _field's, the cells' vectors,
    `pmag` and the skipped cells prism._b_field's.  With return_kernel K = [K_N | K_E | K_D] is assembled densely
    (N <= 16384) and `result` is its product with the vectors; without it `result` comes from the store-free pass
    (gh_tess_b_result), 16384 points at a time, and no kernel is ever stored."""
    assert njobs > 0, "Invalid number of jobs {}. Must be > 0.".format(njobs)
    lon, lat, height = (np.asarray(a, dtype=np.float64) for a in (lon, lat, height))
    assert lon.shape == lat.shape == height.shape, "Input coordinate arrays must have same shape"
    assert ratio > 0, "Invalid ratio {}. Must be > 0.".format(ratio)
    if pmag is not None and np.shape(pmag) != (3,):
        raise ValueError("pmag must be a vector (m_N, m_E, m_D)")
    try:
        bounds, mag3, _ = active_cells_mag(model, pmag, None)
    except TypeError:       # (a scalar intensity: there is no field direction to put it along)
        raise ValueError("the 'magnetization' of every cell must be a vector (m_N, m_E, m_D)")
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'magnetization' property (and no pmag given)")
    if mag3.shape != (bounds.shape[0], 3):
        raise ValueError("the 'magnetization' of every cell must be a vector (m_N, m_E, m_D)")
    tiny = _valid_cells(bounds, None)
    if tiny.all():
        raise ValueError("every tesseroid is below the numerical size threshold")
    keep = ~tiny
    ndrop, cells = int(tiny.sum()), int(keep.sum())
    bounds, mag3 = bounds[keep], np.ascontiguousarray(mag3[keep])
    lon, lat, height = lon.ravel(), lat.ravel(), height.ravel()
    n = lon.size
    warn = False
    if return_kernel:
        eng = Engine(n, 3 * cells, device=device)
        try:
            eng.set_cells_tess_mag(bounds, ratio, (component,), (1.0,), fdir)
            eng.set_obs(lon, lat, height)
            eng.build_G()
            warn = eng.kernel_stats()["warn_cells"] > 0
            result = eng.forward(np.ascontiguousarray(mag3.T).ravel())
            kernel = eng.download_G()
        finally:
            eng.close()
        if ndrop:                                 # (trailing zero columns in each of the three blocks, as gz's)
            z = np.zeros((n, ndrop))
            kernel = np.asfortranarray(np.hstack(
                [np.hstack([kernel[:, a * cells:(a + 1) * cells], z]) for a in range(3)]))
    else:
        kernel = None
        result = np.empty(n)
        for i in range(0, n, _MAG_ROWS):
            j = min(n, i + _MAG_ROWS)
            eng = Engine(j - i, 3 * cells, device=device)
            try:
                eng.set_cells_tess_mag(bounds, ratio, (component,), (1.0,), None if fdir is None else fdir[i:j])
                eng.set_obs(lon[i:j], lat[i:j], height[i:j])
                result[i:j] = eng.tess_b_result(component, mag3)
                warn = warn or eng.kernel_stats()["warn_cells"] > 0
            finally:
                eng.close()
    if warn:
        warnings.warn(_WARN_DIVIDE, RuntimeWarning)
    return result, kernel


def bx(lon, lat, height, model, pmag=None, ratio=RATIO_GG, njobs=1, pool=None, return_kernel=True, device=0):
    """North component (at the observation) of the anomalous magnetic induction of the tesseroid model in uT, and
    its kernel.

    A cell's 'magnetization' is the vector (m_N, m_E, m_D) in A/m in the north-east-down frame at the cell's centre,
    uniform over the cell in the Cartesian sense; pmag (such a vector) overrides it for every cell; cells without the
    property are skipped.  Returns (result[N], K[N, 3 M_active]) with K = [K_N | K_E | K_D], the component for a
    unit magnetization of every kept cell along its north, east and down axis (degenerate cells are dropped with
    gz's warning and leave trailing zero columns in each block)."""
    return _b_field("bx", lon, lat, height, model, pmag, ratio, njobs, return_kernel, device)


def by(lon, lat, height, model, pmag=None, ratio=RATIO_GG, njobs=1, pool=None, return_kernel=True, device=0):
    """East component of the anomalous magnetic induction in uT and its kernel [K_N | K_E | K_D] (see bx)."""
    return _b_field("by", lon, lat, height, model, pmag, ratio, njobs, return_kernel, device)


def bz(lon, lat, height, model, pmag=None, ratio=RATIO_GG, njobs=1, pool=None, return_kernel=True, device=0):
    """Downward component of the anomalous magnetic induction in uT and its kernel [K_N | K_E | K_D] (see bx)."""
    return _b_field("bz", lon, lat, height, model, pmag, ratio, njobs, return_kernel, device)


def tf(lon, lat, height, model, inc, dec, pmag=None, ratio=RATIO_GG, njobs=1, pool=None, return_kernel=True,
       device=0):
    """Total-field anomaly f_o . (bx, by, bz) of the tesseroid model in uT and its kernel [K_N | K_E | K_D] (see bx).

    inc, dec: inclination and declination in degrees of the regional field AT THE OBSERVATIONS, scalars or one value
    per observation point: f_o = (cos I cos D, cos I sin D, sin I) in the point's north-east-down frame."""
    fdir = _field_directions(inc, dec, int(np.asarray(lon).size))
    return _b_field("tf", lon, lat, height, model, pmag, ratio, njobs, return_kernel, device, fdir=fdir)
