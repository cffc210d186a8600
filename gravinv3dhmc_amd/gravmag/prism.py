"""The gravity fields and the total-field magnetic anomaly of right rectangular prisms on the GPU.

Mirror of the reference's `gravmag.prism.gz` (gravmag/prism.py:911-918 -> _dispatcher_gravity
:998-1038 -> _gz :291-316 -> _prism.gz, _prism.pyx:265-290): same arguments, same return
`(result, kernel2d)` in mGal for densities in g/cm^3.  Likewise its other gravity fields
(prism.py:875-972 -> _potential, _geoid, _gx, ... _gzz :102-662 -> _prism.pyx:36-68, 206-509):
`potential` (G, SI units per g/cm^3), `geoid` (m), `gx`, `gy` (mGal) and the gradient tensor `gxx`,
`gxy`, `gxz`, `gyy`, `gyz`, `gzz` (Eotvos).  And of `gravmag.prism.tf` (prism.py:975 ->
_dispatcher_magnetic :1140-1180 -> _tf :665-733 -> _prism.tf, _prism.pyx:80-113): `(result, kernel2d)`
in uT for magnetizations in A/m (CM * T2NT, constants.py).  And of its `_bx`, `_by`, `_bz`
(prism.py:735-870 -> _prism.bx / by / bz, _prism.pyx:114-202): `bx`, `by`, `bz` return the reference's `res` in
uT and, beside it, the kernel [K_x | K_y | K_z] of unit-axis columns, which the reference does not form.
`njobs`/`pool` are accepted and
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


def _b_field(component, xp, yp, zp, prisms, pmag, return_kernel, device):
    """(result, K) of one component of the anomalous induction: the result in the reference's accumulation order
    (gh_b_result) from the cells' magnetization VECTORS (or pmag for every cell; cells without the property are
    skipped), K = [K_x | K_y | K_z] (N x 3 M_active, Fortran-ordered; None without return_kernel) from the dense
    assembly: column a M_active + c is the component of cell c magnetized 1 A/m along axis a."""
    xp, yp, zp = (np.asarray(a, dtype=np.float64) for a in (xp, yp, zp))
    if xp.shape != yp.shape or xp.shape != zp.shape:
        raise ValueError("Input arrays xp, yp, and zp must have same shape!")
    if pmag is not None and np.shape(pmag) != (3,):
        raise ValueError("pmag must be a vector (mx, my, mz)")
    try:
        bounds, mag3, _ = active_cells_mag(prisms, pmag, None)
    except TypeError:       # (a scalar intensity: there is no field direction to put it along)
        raise ValueError("the 'magnetization' of every cell must be a vector (mx, my, mz)")
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'magnetization' property (and no pmag given)")
    if mag3.shape != (bounds.shape[0], 3):
        raise ValueError("the 'magnetization' of every cell must be a vector (mx, my, mz)")
    eng = Engine(xp.size, 3 * bounds.shape[0], device=device)
    try:
        eng.set_cells_mvi_data(bounds, None, (component,), (1.0,))
        eng.set_obs(xp.ravel(), yp.ravel(), zp.ravel())
        result = eng.b_result(component, mag3)
        kernel = None
        if return_kernel:
            eng.build_G()
            kernel = eng.download_G()
    finally:
        eng.close()
    return result, kernel


def bx(xp, yp, zp, prisms, pmag=None, njobs=1, pool=None, return_kernel=True, device=0):
    """North component of the anomalous magnetic induction of the prism model in uT, and its kernel.

    A cell's 'magnetization' is a vector (mx, my, mz) in A/m; pmag (a vector) overrides it for every cell; cells
    without the property are skipped.  Returns (result[N], K[N, 3 M_active]) with K = [K_x | K_y | K_z], the
    component for a unit magnetization of every kept cell along x north, y east and z down."""
    return _b_field("bx", xp, yp, zp, prisms, pmag, return_kernel, device)


def by(xp, yp, zp, prisms, pmag=None, njobs=1, pool=None, return_kernel=True, device=0):
    """East component of the anomalous magnetic induction in uT and its kernel [K_x | K_y | K_z] (see bx)."""
    return _b_field("by", xp, yp, zp, prisms, pmag, return_kernel, device)


def bz(xp, yp, zp, prisms, pmag=None, njobs=1, pool=None, return_kernel=True, device=0):
    """Downward component of the anomalous magnetic induction in uT and its kernel [K_x | K_y | K_z] (see bx)."""
    return _b_field("bz", xp, yp, zp, prisms, pmag, return_kernel, device)


def build_engine_component(xp, yp, zp, prisms, component, dens=None, device=0):
    """Cells of one gravity component's kernel on the device (G not built yet); returns (engine, densities)."""
    xp, yp, zp = (np.asarray(a, dtype=np.float64) for a in (xp, yp, zp))
    if xp.shape != yp.shape or xp.shape != zp.shape:
        raise ValueError("Input arrays xp, yp, and zp must have same length!")
    bounds, rho, _ = active_cells(prisms, dens)
    if bounds.shape[0] == 0:
        raise ValueError("mesh has no cell with a 'density' property (and no dens given)")
    eng = Engine(xp.size, bounds.shape[0], device=device)
    try:
        eng.set_obs(xp, yp, zp)
        eng.set_cells(bounds, _lib.CELL_PRISM_COMP, component=component)
    except Exception:
        eng.close()
        raise
    return eng, rho


def _field(component, xp, yp, zp, prisms, dens, return_kernel, device):
    """(result, kernel2d) of one component: the result in the reference's accumulation order
    (gh_prism_result), the kernel from the dense assembly, Fortran-ordered (None without return_kernel)."""
    eng, rho = build_engine_component(xp, yp, zp, prisms, component, dens, device)
    try:
        result = eng.prism_result(rho)
        kernel2d = None
        if return_kernel:
            eng.build_G()
            kernel2d = eng.download_G()
    finally:
        eng.close()
    return result, kernel2d


def potential(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """Gravitational potential of the prism model and its kernel (G times the reference's kernelpot sum)."""
    return _field("potential", xp, yp, zp, prisms, dens, return_kernel, device)


def geoid(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """Geoid height of the prism model and its kernel: the potential times 1/g0 (G/g0)."""
    return _field("geoid", xp, yp, zp, prisms, dens, return_kernel, device)


def gx(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """North gravity component in mGal and its kernel."""
    return _field("gx", xp, yp, zp, prisms, dens, return_kernel, device)


def gy(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """East gravity component in mGal and its kernel."""
    return _field("gy", xp, yp, zp, prisms, dens, return_kernel, device)


def gxx(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gxx gravity gradient in Eotvos and its kernel."""
    return _field("gxx", xp, yp, zp, prisms, dens, return_kernel, device)


def gxy(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gxy gravity gradient in Eotvos and its kernel.  As in the reference, a point on the line of a
    vertical edge above the prism takes a perturbed distance there: large but finite values."""
    return _field("gxy", xp, yp, zp, prisms, dens, return_kernel, device)


def gxz(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gxz gravity gradient in Eotvos and its kernel (the reference's perturbed distance on the line of
    an edge along y)."""
    return _field("gxz", xp, yp, zp, prisms, dens, return_kernel, device)


def gyy(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gyy gravity gradient in Eotvos and its kernel."""
    return _field("gyy", xp, yp, zp, prisms, dens, return_kernel, device)


def gyz(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gyz gravity gradient in Eotvos and its kernel (the reference's perturbed distance on the line of
    an edge along x)."""
    return _field("gyz", xp, yp, zp, prisms, dens, return_kernel, device)


def gzz(xp, yp, zp, prisms, dens=None, njobs=1, pool=None, return_kernel=True, device=0):
    """gzz gravity gradient in Eotvos and its kernel."""
    return _field("gzz", xp, yp, zp, prisms, dens, return_kernel, device)
