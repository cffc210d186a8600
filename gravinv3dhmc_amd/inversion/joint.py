"""Joint gravity-magnetic inversion on prism meshes, evaluated on the GPU.

Host-side mirror of the reference's `inversion.potential.JointModule` (inversion/potential.py:847-1812): the
density and the magnetization of the same prisms under the same observation points, with the block-diagonal
kernel A = [[A_gz, 0], [0, A_tf]], the data balance Wb = diag(1 ... 1, s ... s), s = std(A_gz) / std(A_tf),
the column-norm weights Wm of A, and the potential |Aw mw - dobsw|^2 + alpha R(mw) with no mean removal --
plus, on request, the cross-gradient term lambda |grad rho x grad kappa|^2 that ties the two models' structure.

The device keeps H = [Aw_gz | Aw_tf] (N rows, 2M columns): the zero blocks are never stored or read
(libgravhmc's GH_CELL_PRISM_JOINT).  `Aw` is a device handle whose array is the reference's 2N x 2M layout.
"""
import numpy as np
from scipy.sparse import block_diag, coo_matrix

from .. import _lib, utils
from ..engine import Engine
from .potential import _diag, _mesh, _OnTable, _Potential

_TSTORE = "the joint store on the translation-invariant table"


def fd3d(shape):
    """The reference's 3D finite-difference matrix (potential.py:266-361), CSR: for every z-layer its x then its y
    differences, then the differences between consecutive layers; each row is cell - next cell."""
    nz, ny, nx = (int(v) for v in shape)
    idx = np.arange(nz * ny * nx).reshape(nz, ny, nx)
    per_layer = (nx - 1) * ny + (ny - 1) * nx
    rows, a, b = [], [], []
    for k in range(nz):
        ax = idx[k, :, :-1].ravel()
        ay = idx[k, :-1, :].ravel()
        a += [ax, ay]
        b += [ax + 1, ay + nx]
        rows.append(per_layer * k + np.arange(ax.size + ay.size))
    if nz > 1:
        az = idx[:-1].ravel()
        a.append(az)
        b.append(az + nx * ny)
        rows.append(per_layer * nz + np.arange(az.size))
    a, b, rows = np.concatenate(a), np.concatenate(b), np.concatenate(rows)
    nderivs = per_layer * nz + nx * ny * (nz - 1)
    I = np.repeat(rows, 2)
    J = np.column_stack([a, b]).ravel()
    V = np.tile([1, -1], rows.size)
    return coo_matrix((V, (I, J)), (nderivs, nx * ny * nz)).tocsr()


class JointModule(_OnTable, _Potential):
    """Joint gravity (gz) and total-field magnetic inversion model on one MI355X.

    Parameters are the reference's (potential.py:848-851): dobs_gz, dobs_tf (the same N observation points),
    mrange = (xmin, xmax, ymin, ymax, zmin, zmax), mspacing = (dz, dy, dx), obsurface = [xobs, yobs, height],
    mratio, mangle = (inclination, declination) of the regional field; `mtopo=(x, y, topography)` carves the
    mesh (active cells only, as GravMagModule).  device: GPU ordinal (extension).

    crossgradient = lambda, cg_scale = (s_rho, s_kappa) (extension; see set_cross_gradient): with lambda > 0 every
    potential evaluation and every chain adds lambda * Phi, Phi = sum |grad(rho / s_rho) x grad(kappa / s_kappa)|^2
    over the cells with a forward neighbour on all three axes (Gallardo & Meju 2003), evaluated on the device.
    The differences are taken over RELATIVE spacings: every centre distance of the mesh divided by the smallest
    of them, so that a cubic mesh gets the unit differences of fd3d and lambda has the order of magnitude of
    alpha (with metres Phi would be ~1e-7 for O(1) models).  The reported model value stays R; Phi is
    `last_cross_gradient`.  Default 0: off, nothing is launched or changed.

    Attributes as the reference: meshrho, meshmag, mshape, mxs/mys/mzs, dobs, dobsw, Wb, Wm, WmInv, WmSquare,
    Aw (a device handle; np.asarray(Aw) is the 2N x 2M stacked layout).  A, kernel_gz and kernel_tf are formed
    on request from the device copy: Aw's blocks times Wm and over Wb, equal to the reference's to rounding,
    not bit for bit.

    Divergences: coordinate="spherical" and wavelet compression raise NotImplementedError (the reference's
    branches are broken); Smoothness and TV work, with the block-diagonal operator fd3djoint (the reference
    raises AttributeError there: it calls a missing fd3d).  CrossGradient is implemented (the reference's body is
    `pass`) and can be switched into the potential.

    translation_invariant=True (extension) keeps the translation-invariant table instead of the kernel (a regular mesh
    -- no mratio growth or mtopo -- under observations that are a full rectangle of the lattice of the cells'
    horizontal spacings at one height, GravMagModule's translation_invariant): one table of 2 nz layers, the gz table
    then the tf table, each layer meeting its own observation block alone (csrc/latjoint.hip.h) -- two tables of 15.8 MB
    where 100 x 100 x 50 cells under 100 x 100 stations store two blocks of 40 GB, and no limit of 16384 points.
    HMCSample (posterior_stream too), misfit_and_grad, forward, the four regularisers, crossgradient= /
    set_cross_gradient / CrossGradient / last_cross_gradient, std_gz, std_tf, Wb, dobsw, Wm, WmInv, WmSquare and
    translation_invariant_info() work on it as on the dense module and agree with it to 1e-10 (the bound the suites test); Aw, A, kernel_gz and
    kernel_tf do not exist (the kernel is never stored), and mtopo=, HMCSampleBatch and translation_invariant="chains"
    are refused (NotImplementedError naming the joint store on the translation-invariant table), as is a geometry
    without the structure, with the reason.  The default False is the module as it always was.
    """
    _props = 2  # (density and magnetization of the same mesh)
    _store = _TSTORE

    def __init__(self, dobs_gz, dobs_tf, mrange, mspacing, obsurface, mratio=1, coordinate="cartesian", njobs=1,
                 mangle=(90, 0), wavelet=False, device=0, verbose=True, crossgradient=0.0, cg_scale=(1.0, 1.0),
                 translation_invariant=False, **kwargs):
        self._say = print if verbose else (lambda *a, **k: None)
        if coordinate == "spherical":
            # (the reference's spherical branch never defines kernel_tf: potential.py:885-895)
            raise NotImplementedError("joint inversion on tesseroids (coordinate='spherical') is not supported")
        if coordinate != "cartesian":
            raise ValueError("Please choose coordinate from(cartesian, spherical)!")
        if wavelet not in (False, None):
            raise NotImplementedError("wavelet compression of the joint kernel is not supported")
        dobs_gz = np.asarray(dobs_gz, dtype=np.float64).ravel()
        dobs_tf = np.asarray(dobs_tf, dtype=np.float64).ravel()
        n = int(np.asarray(obsurface[0]).size)
        if dobs_gz.size != dobs_tf.size or dobs_gz.size != n:
            raise ValueError("dobs_gz (%d), dobs_tf (%d) and the observation points (%d) must have the same length"
                             % (dobs_gz.size, dobs_tf.size, n))
        if isinstance(translation_invariant, str) and translation_invariant != "chains":
            raise ValueError("translation_invariant must be True or False, not %r" % (translation_invariant,))
        if translation_invariant:
            self.translation_invariant = True   # (the default module keeps the attributes it always had: the class's False)
        if translation_invariant == "chains":
            raise NotImplementedError("%s (translation_invariant=True) runs one chain: batches of joint models "
                                      "(translation_invariant=\"chains\") are not built" % _TSTORE)
        if translation_invariant and kwargs:
            raise NotImplementedError("%s (translation_invariant=True) does not combine with mtopo: a carved mesh is "
                                      "not a full regular product of cells" % _TSTORE)
        self.dobs_gz, self.dobs_tf = dobs_gz, dobs_tf
        self.mrange = mrange
        self.mspacing = mspacing
        self.mratio = mratio
        self.lonobs, self.latobs, self.heightobs = obsurface[0], obsurface[1], obsurface[2]
        self.inc, self.dec = mangle[0], mangle[1]
        self.njobs = njobs
        self.wavelet = wavelet
        self.device = device

        self._say("Joint inversion in {} coordinate.".format(coordinate))
        mesh = _mesh(False, mrange, mspacing, mratio)
        self._carve(mesh, kwargs.values())  # (any keyword is the topography, as in the reference)
        meshrho, meshmag = mesh.copy(), mesh.copy()
        meshrho.addprop('density', np.zeros(mesh.size))
        meshmag.addprop('magnetization', utils.ang2vec(np.zeros(mesh.size), self.inc, self.dec))
        self.meshrho, self.meshmag = meshrho, meshmag

        bounds = mesh.cell_bounds(active_only=True)
        m = bounds.shape[0]
        eng = Engine(2 * n, 2 * m, device=device)
        if self.translation_invariant:
            eng.set_cells(bounds, _lib.CELL_PRISM_JOINT, direction=utils.dircos(self.inc, self.dec),
                          translation_invariant=True)
        else:
            eng.set_cells(bounds, _lib.CELL_PRISM_JOINT, direction=utils.dircos(self.inc, self.dec))
        eng.set_obs(self.lonobs, self.latobs, self.heightobs)
        eng.build_G()  # (on the table: NotImplementedError with the detection's reason where the structure is absent)
        self._engine = eng

        self.mshape = mesh.shape
        self.mxs, self.mys, self.mzs = mesh.get_xs(), mesh.get_ys(), mesh.get_zs()
        self.weightKDM()
        eng.set_data(self.dobsw)
        # centre distances of the mesh relative to the smallest of them (the cross-gradient term's spacings)
        zc = np.array([0.5 * sum(mesh._layer_z(k)) for k in range(mesh.shape[0])])
        hz = np.diff(zc)
        hmin = min([float(mesh.dims[0]), float(mesh.dims[1])] + [float(v) for v in hz])
        self._cg_spacing = (mesh.dims[0] / hmin, mesh.dims[1] / hmin, hz / hmin)
        self._cg = None  # (lambda, scale) once the engine holds the coupling's geometry
        if crossgradient != 0:
            self.set_cross_gradient(crossgradient, cg_scale)
        else:
            self._cg_scale = tuple(float(v) for v in cg_scale)

    # ------------------------------------------------------------------ weighting
    def weightKDM(self):
        """Wm (column 2-norms of A), Wb (std_gz / std_tf on the tf rows), Aw = Wb A Wm^-1 and dobsw = Wb dobs
        (potential.py:1003-1065), on the device."""
        self._weight(0.5, zero_safe=True)
        std_gz, std_tf = self._engine.joint_std()
        self.std_gz, self.std_tf = std_gz, std_tf
        n = self.dobs_gz.size
        wb = np.append(np.ones(n), np.ones(n) * (std_gz / std_tf))
        self.Wb = _diag(wb)
        self.dobs = np.append(self.dobs_gz, self.dobs_tf)
        self.dobsw = self.Wb @ self.dobs
        if self.translation_invariant:
            self._hide_Aw()

    @property
    def A(self):
        """The unweighted stacked kernel, 2N x 2M, from the device copy (Wb^-1 Aw Wm; rounding differs)."""
        self._no_table("A")
        A = np.asarray(self.Aw)
        wb = self.Wb.diagonal()
        return (A / wb[:, None]) * self.Wm.diagonal()[None, :]

    @property
    def kernel_gz(self):
        self._no_table("kernel_gz")
        n, m = self.dobs_gz.size, self.Wm.shape[0] // 2
        return np.ascontiguousarray(self.A[:n, :m])

    @property
    def kernel_tf(self):
        self._no_table("kernel_tf")
        n, m = self.dobs_gz.size, self.Wm.shape[0] // 2
        return np.ascontiguousarray(self.A[n:, m:])

    def forward(self, model):
        """Unweighted forward A @ model (potential.py:1067-1073): 2N values, gz first."""
        model = np.asarray(model, dtype=np.float64)
        wm = self.Wm.diagonal()
        wb = self.Wb.diagonal()
        return self._engine.forward(model * wm) / wb

    def fd3djoint(self, shape):
        """The reference's block-diagonal finite-difference matrix of the two properties (potential.py:1075-1220)."""
        R = fd3d(shape)
        return block_diag([R, R], format="csr")

    # ------------------------------------------------------------------ cross-gradient coupling
    def _send_cross_gradient(self, lam, scale):
        if self.topocarve:
            cells = self._props * int(np.prod(self.mshape))
            raise ValueError("CrossGradient needs the full (uncarved) mesh: %d x shape %r has %d cells, model has %d"
                             % (self._props, self.mshape, cells, self._engine.M))
        hx, hy, hz = self._cg_spacing
        self._engine.set_cross_gradient(lam, self.mshape, hx, hy, hz, scale)
        self._cg = (float(lam), scale)

    def set_cross_gradient(self, lam, scale=None):
        """Switch the cross-gradient coupling lam * Phi into the potential (lam = 0: off again; results are then
        those of a module that never had it).  scale = (s_rho, s_kappa) > 0 normalises the two physical models
        (kept from the last call when None).  The spacings are the mesh's centre distances relative to the smallest
        of them (see the class docstring).  A carved mesh (mtopo=) raises ValueError."""
        scale = tuple(float(v) for v in (self._cg_scale if scale is None else scale))
        if len(scale) != 2:
            raise ValueError("scale must be (s_rho, s_kappa)")
        if lam == 0 and self._cg is None and scale[0] > 0 and scale[1] > 0:
            self._cg_scale = scale  # (never switched on: nothing to switch off)
            return
        self._send_cross_gradient(lam, scale)
        self._cg_scale = scale

    def CrossGradient(self, model):
        """The cross-gradient term of the stacked PHYSICAL model (2M entries: density, then magnetization):
        (Phi, dPhi/dmodel, t as an (M, 3) array), with the normalisers of set_cross_gradient and lambda = 1
        (potential.py:1558, empty in the reference)."""
        model = np.asarray(model, dtype=np.float64).ravel()
        if self._cg is None:
            self._send_cross_gradient(0.0, self._cg_scale)
        wm = self.Wm.diagonal()
        phi, grad, t = self._engine.cross_gradient_eval(model * wm)
        return phi, grad * wm, t

    @property
    def last_cross_gradient(self):
        """Phi of the last misfit_and_grad, or of the state the chain is in; 0 while the coupling is off."""
        return self._engine.cross_gradient_last()
