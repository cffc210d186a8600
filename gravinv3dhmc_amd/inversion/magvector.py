"""Magnetization vector inversion on prism meshes (Cartesian form, Lelievre & Oldenburg 2009), evaluated on the GPU.

GravMagModule(field="magnetic") and the magnetic block of JointModule invert ONE scalar per cell, the magnetization
along the regional field.  Remanence turns the magnetization away from the field, and a scalar inversion then puts
the body in the wrong place.  MagVectorModule gives every cell three unknowns (mx, my, mz) in A/m -- x north, y east,
z down -- and the kernel A = [A_x | A_y | A_z] (libgravhmc's GH_CELL_PRISM_MVI): column a M/3 + c is the total-field
anomaly in uT of prism c magnetized 1 A/m along axis a.  Model vectors are property-major: [mx of every cell; my; mz].

The store is an ordinary dense N x M kernel: the column-norm weights Wm are taken over all M columns, the data term
removes the mean as the magnetic GravMagModule does, Damping and MS act on the M entries as they are, Smoothness and
TV apply the stencil to each component on its own.  The amplitude term lambda * sum_c s_c / (s_c + beta), s_c =
|m_c|^2, is the one term that ties the three components of a cell together; it is off by default.
"""
import time

import numpy as np

from .. import mesher, utils
from ..engine import DeviceMatrix, Engine
from .potential import _diag, _Potential

_STORE = "the magnetization-vector store"


class MagVectorModule(_Potential):
    """The magnetization vector of every prism under total-field data, on one MI355X.

    dobs: the N total-field anomalies (uT) at obsurface = [xobs, yobs, height]; mrange, mspacing, mratio, mseg,
    mdivisionsection, weightfactor, mtopo=(x, y, topography), device and verbose as GravMagModule; mangle =
    (inclination, declination) of the regional field in degrees.

    amplitude = lambda, amplitude_beta = beta: with lambda > 0 every potential evaluation and every chain adds
    lambda * Phi, Phi = sum_c s_c / (s_c + beta) with s_c = mx_c^2 + my_c^2 + mz_c^2 of the PHYSICAL model in A/m (the
    minimum-support functional of the amplitude: compact bodies), evaluated on the device.  The reported model value
    stays R; Phi is `last_amplitude`.  Default 0: off, nothing is launched or changed.

    Attributes: mesh, mshape, mxs/mys/mzs, dobs, Wm, WmInv, WmSquare (M = 3 x cells entries), Aw (a device handle).
    A and kernel(axis) are formed on request from the device copy (Aw Wm: equal to the assembled blocks to rounding).

    HMCSample and misfit_and_grad work on it as on GravMagModule; bounds such as [-mmax, mmax] per component go
    through `boundaries`.  Not supported (NotImplementedError): coordinate="spherical", wavelet compression, the
    matrix-free mode, the shift-invariant store, shards, HMCSampleBatch and more than 16384 observations (the store
    runs on the fused sweep).  Smoothness and TV need the full mesh (ValueError on a carved one).
    """
    _props = 3  # (mx, my and mz of the same mesh)

    def __init__(self, dobs, mrange, mspacing, obsurface, mangle=(90, 0), mratio=1, mseg=False, mdivisionsection=[],
                 weightfactor=0.5, amplitude=0.0, amplitude_beta=0.01, device=0, verbose=True, coordinate="cartesian",
                 wavelet=False, matrix_free=False, shift_invariant=False, shard=None, **kwargs):
        self._say = print if verbose else (lambda *a, **k: None)
        unknown = sorted(set(kwargs) - {"mtopo"})
        if unknown:
            raise TypeError("unexpected keyword argument %r" % unknown[0])
        if coordinate == "spherical":
            raise NotImplementedError("%s holds prism fields: tesseroids (coordinate='spherical') are not supported"
                                      % _STORE)
        if coordinate != "cartesian":
            raise ValueError("Please choose coordinate from(cartesian, spherical)!")
        if wavelet not in (False, None):
            raise NotImplementedError("wavelet compression of %s is not supported" % _STORE)
        if matrix_free:
            raise NotImplementedError("%s is dense: the matrix-free mode is not supported" % _STORE)
        if shift_invariant:
            raise NotImplementedError("%s is dense: the shift-invariant store is not supported" % _STORE)
        if shard is not None:
            raise NotImplementedError("%s is not sharded" % _STORE)
        dobs = np.asarray(dobs, dtype=np.float64).ravel()
        n = int(np.asarray(obsurface[0]).size)
        if dobs.size != n:
            raise ValueError("dobs has %d values, the observation points are %d" % (dobs.size, n))
        if n > 16384:
            raise NotImplementedError("%d observations: %s takes at most 16384 (it runs on the fused sweep)"
                                      % (n, _STORE))
        if not (amplitude >= 0) or not (amplitude_beta > 0):
            raise ValueError("amplitude must be >= 0 and amplitude_beta > 0")

        self.dobs = dobs
        self.mrange, self.mspacing, self.mratio = mrange, mspacing, mratio
        self.mseg, self.mdivisionsection = mseg, mdivisionsection
        self.weightfactor = weightfactor
        self.lonobs, self.latobs, self.heightobs = obsurface[0], obsurface[1], obsurface[2]
        self.inc, self.dec = mangle[0], mangle[1]
        self.topocarve = False
        self.wavelet = False
        self.device = device

        self._say("Calculating magnetic field (magnetization vector) in cartesian coordinate.")
        mesh = (mesher.PrismMeshSegment(mrange, mspacing, mdivisionsection) if mseg
                else mesher.PrismMesh(mrange, mspacing, mratio))
        if "mtopo" in kwargs:
            value = kwargs["mtopo"]
            self.topocarve = True
            self.mask = mesh.carvetopo(value[0], value[1], value[2])
        mesh.addprop('magnetization', np.zeros((mesh.size, 3)))
        self.mesh = mesh

        bounds = mesh.cell_bounds(active_only=True)
        self._cells = int(bounds.shape[0])
        self._say("Start of calculate kernel")
        start = time.time()
        eng = Engine(n, 3 * self._cells, device=device)
        eng.set_cells_mvi(bounds, utils.dircos(self.inc, self.dec))
        eng.set_obs(self.lonobs, self.latobs, self.heightobs)
        eng.build_G()
        self._say("kernel.shape", (n, 3 * self._cells))
        self._say("End of calculate kernel:%.6f s" % (time.time() - start))
        self._engine = eng

        self.mshape = mesh.shape
        self.mxs, self.mys, self.mzs = mesh.get_xs(), mesh.get_ys(), mesh.get_zs()
        self._say("Start to weight kernel")
        start = time.time()
        self.sensitivityWeighting()
        self._say("End of weighting kernel: %.6f s" % (time.time() - start))
        eng.set_data(self.dobs)
        self._amp = None  # (lambda, beta) once the engine holds the term
        self._amp_beta = float(amplitude_beta)
        if amplitude != 0:
            self.set_amplitude(amplitude, amplitude_beta)

    # ------------------------------------------------------------------ weighting
    def sensitivityWeighting(self):
        """Column-norm weighting Wm over all M columns and Aw = A Wm^-1, on the device."""
        wm = self._engine.weight(self.weightfactor)
        with np.errstate(divide='ignore'):
            inv = 1.0 / wm
        self.Wm = _diag(wm)
        self.WmInv = _diag(inv)
        self.WmSquare = _diag(wm * wm)
        self.Aw = DeviceMatrix(self._engine)

    def kernelw(self):
        """(Aw, WmInv, Wm) as the sampler expects; Aw is a device handle."""
        return self.Aw, self.WmInv, self.Wm

    @property
    def A(self):
        """The unweighted kernel [A_x | A_y | A_z], N x M, from the device copy (Aw Wm; rounding differs)."""
        return np.asarray(self.Aw) * self.Wm.diagonal()[None, :]

    def kernel(self, axis):
        """Block A_axis (N x M/3, uT per A/m along axis 0 / "x" north, 1 / "y" east, 2 / "z" down), from the device
        copy."""
        a = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        if a not in (0, 1, 2):
            raise ValueError("axis must be 0, 1, 2 or 'x', 'y', 'z', got %r" % (axis,))
        m = self._cells
        Aw = np.asarray(self.Aw)[:, a * m:(a + 1) * m]
        return np.asfortranarray(Aw * self.Wm.diagonal()[None, a * m:(a + 1) * m])

    def forward(self, model):
        """Unweighted forward A @ model (uT): model is the property-major M vector in A/m."""
        model = np.asarray(model, dtype=np.float64).ravel()
        return self._engine.forward(model * self.Wm.diagonal())

    # ------------------------------------------------------------------ the model as vectors
    def to_vectors(self, model):
        """The property-major M vector as an (M/3, 3) array of (mx, my, mz) per cell."""
        model = np.asarray(model, dtype=np.float64).ravel()
        if model.size != 3 * self._cells:
            raise ValueError("model must have M = %d entries, got %d" % (3 * self._cells, model.size))
        return np.ascontiguousarray(model.reshape(3, self._cells).T)

    def from_vectors(self, v):
        """An (M/3, 3) array of (mx, my, mz) per cell as the property-major M vector."""
        v = np.asarray(v, dtype=np.float64)
        if v.shape != (self._cells, 3):
            raise ValueError("vectors must be (M/3, 3) = (%d, 3), got %r" % (self._cells, v.shape))
        return np.ascontiguousarray(v.T).ravel()

    def amplitude(self, model):
        """|m_c| of every cell (host)."""
        return np.sqrt(np.sum(self.to_vectors(model) ** 2, axis=1))

    def direction(self, model):
        """(inclination, declination) in degrees of every cell's vector (host): the inverse of utils.ang2vec --
        inclination positive down, declination from north towards east; (0, 0) for a zero vector."""
        v = self.to_vectors(model)
        deg = 180. / np.pi
        inc = np.arctan2(v[:, 2], np.hypot(v[:, 0], v[:, 1])) * deg
        dec = np.arctan2(v[:, 1], v[:, 0]) * deg
        return inc, dec

    # ------------------------------------------------------------------ amplitude coupling
    def set_amplitude(self, lam, beta=None):
        """Switch the amplitude coupling lam * Phi into the potential (lam = 0: off again; results are then those of
        a module that never had it).  beta > 0 is kept from the last call when None."""
        beta = self._amp_beta if beta is None else float(beta)
        if lam == 0 and self._amp is None and beta > 0:
            self._amp_beta = beta  # (never switched on: nothing to switch off)
            return
        self._engine.set_amplitude(lam, beta, 1.0)
        self._amp = (float(lam), beta)
        self._amp_beta = beta

    def Amplitude(self, model):
        """The amplitude term of the PHYSICAL model (M entries, property-major): (Phi, dPhi/dmodel, |m_c| per cell),
        with the beta of set_amplitude and lambda = 1.  A pure evaluation once the coupling has been set (any lambda,
        0 included: pass amplitude= or call set_amplitude before a chain starts).  On a module whose coupling was
        NEVER set, the first call sets it with lambda = 0, and setting the term invalidates a running chain: the
        engine then asks for chain_init again."""
        model = np.asarray(model, dtype=np.float64).ravel()
        if self._amp is None:
            self._engine.set_amplitude(0.0, self._amp_beta, 1.0)
            self._amp = (0.0, self._amp_beta)
        wm = self.Wm.diagonal()
        phi, grad, amp = self._engine.amplitude_eval(model * wm)
        return phi, grad * wm, amp

    @property
    def last_amplitude(self):
        """Phi of the last misfit_and_grad, or of the state the chain is in; 0 while the coupling is off."""
        return self._engine.amplitude_last()
