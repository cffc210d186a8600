"""gz and the total-field magnetic anomaly of right rectangular prisms on the GPU.

Mirror of the reference's `gravmag.prism.gz` (gravmag/prism.py:911-918 -> _dispatcher_gravity
:998-1038 -> _gz :291-316 -> _prism.gz, _prism.pyx:265-290): same arguments, same return
`(result, kernel2d)` in mGal for densities in g/cm^3.  And of `gravmag.prism.tf` (prism.py:975 ->
_dispatcher_magnetic :1140-1180 -> _tf :665-733 -> _prism.tf, _prism.pyx:80-113): `(result, kernel2d)`
in uT for magnetizations in A/m (CM * T2NT, constants.py).  `njobs`/`pool` are accepted and
ignored (the reference uses them for host multiprocessing; the assembly here is one HIP
launch over all (observation, cell) pairs).
"""
import numpy as np

from .. import _lib
from ..engine import Engine
from .. import utils
from ._common import active_cells, active_cells_mag


def build_engine(xp, yp, zp, prisms, dens=None, device=0):
    """Assemble the dense kernel for `prisms` on the device; returns (engine, densities)."""
    xp, yp, zp = (np.asarray(a, dtype=np.float64) for a in (xp, yp, zp))
    if xp.shape != yp.shape or xp.shape != zp.shape:
        raise ValueError("Input arrays xp, yp, and zp must have same length!")
    bounds, rho, _ = active_cells(prisms, dens)
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'density' property (and no dens given)")
    eng = Engine(xp.size, bounds.shape[0], device=device)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(bounds, _lib.CELL_PRISM)
    eng.build_G()
    return eng, rho


def gz(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """Vertical gravity of the prism model and its sensitivity matrix.

    Returns (result[N], kernel2d[N, M_active]); kernel2d is Fortran-ordered.  Pass
    return_kernel=False to skip the device->host copy of the matrix (returns None)."""
    eng, rho = build_engine(xp, yp, zp, prisms, dens, device)
    try:
        result = eng.forward(rho)
        kernel2d = eng.download_G() if return_kernel else None
    finally:
        eng.close()
    return result, kernel2d


def build_engine_tf(xp, yp, zp, prisms, inc, dec, pmag=None, device=0):
    """Cells of the total-field kernel on the device (G not built yet); returns (engine, magnetization
    table (M, 3) of the kept cells)."""
    xp, yp, zp = (np.asarray(a, dtype=np.float64) for a in (xp, yp, zp))
    if xp.shape != yp.shape or xp.shape != zp.shape:
        raise ValueError("Input arrays xp, yp, and zp must have same length!")
    f = utils.dircos(inc, dec)
    bounds, mag3, _ = active_cells_mag(prisms, pmag, f)
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'magnetization' property (and no pmag given)")
    eng = Engine(xp.size, bounds.shape[0], device=device)
    try:
        eng.set_obs(xp, yp, zp)
        eng.set_cells(bounds, _lib.CELL_PRISM_TF, direction=f)
    except Exception:
        eng.close()
        raise
    return eng, mag3


def tf(xp, yp, zp, prisms, inc, dec, pmag=None, njobs=1, pool=None, return_kernel=True, device=0):
    """Total-field magnetic anomaly of the prism model and its sensitivity matrix, in uT.

    inc, dec: the regional field's inclination and declination in degrees.  A cell's
    'magnetization' is a vector (mx, my, mz) in A/m or a scalar intensity along the field; pmag (the
    same two forms) overrides it for every cell.  Returns (result[N], kernel2d[N, M_active]):
    kernel2d does not depend on the magnetization (a unit magnetization along the field) and is
    Fortran-ordered.  Pass return_kernel=False to skip its assembly (returns None)."""
    eng, mag3 = build_engine_tf(xp, yp, zp, prisms, inc, dec, pmag, device)
    try:
        result = eng.tf_result(mag3)
        kernel2d = None
        if return_kernel:
            eng.build_G()
            kernel2d = eng.download_G()
    finally:
        eng.close()
    return result, kernel2d
