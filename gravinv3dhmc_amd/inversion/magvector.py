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

Vector data.  The total field is the projection of B on the regional direction: it cannot by itself fix a rotated
(remanent) magnetization.  With data=("bx", "by", "bz") -- any distinct choice of "tf", "bx", "by", "bz" -- the rows
of the store are blocks of those components at the same points (libgravhmc's GH_CELL_PRISM_MVI_DATA), block b in its
own units times a data weight w_b.  The rows then behave as MultiComponentModule's: Wm are the column norms of Wb A,
and the data term removes the mean of every block on its own,

    r_b = (d_b - mean d_b) - (dobsw_b - mean dobsw_b),   data_value = sum_b |r_b|^2,   grad = 2 Aw^T r

with d = Aw mw, Aw = Wb A Wm^-1, dobsw = Wb dobs.  The columns, the regularisers and the amplitude term stay as above.
"""
import numpy as np

from .. import _lib, utils
from ..engine import Engine
from .potential import _BlockStore

_STORE = "the magnetization-vector store"
_VSTORE = "the vector-data magnetization store"
_TSTORE = "the tesseroid magnetization store"


def mirror_signs(data):
    """The signs the entries of the tesseroid magnetization store take under the reflection through the equatorial
    plane, (class_signs, axis_signs): K[(b, mirrored point), (a, mirrored cell)] = class_signs[b] axis_signs[a]
    K[(b, point), (a, cell)].  Local north flips at both ends, east and down do not: class_signs has -1 for "bx" and
    +1 for "by" and "bz", one per component of data; axis_signs is (-1, +1, +1) for the cell's (N, E, D).  The total
    field projects on a direction of its own at the observation and is no pure sign: its entry is None, and the
    shift-invariant table is built without the north-south mirror when "tf" is among the data."""
    data = (data,) if isinstance(data, str) else tuple(data)
    for b in data:
        if b not in _lib.BCOMPONENTS:
            raise ValueError("data component %r: must be one of %s" % (b, ", ".join(_lib.BCOMPONENTS)))
    return tuple(None if b == "tf" else -1.0 if b == "bx" else 1.0 for b in data), (-1.0, 1.0, 1.0)


class MagVectorModule(_BlockStore):
    """The magnetization vector of every prism under total-field data, on one MI355X.

    dobs: the N total-field anomalies (uT) at obsurface = [xobs, yobs, height]; mrange, mspacing, mratio, mseg,
    mdivisionsection, weightfactor, mtopo=(x, y, topography), device and verbose as GravMagModule; mangle =
    (inclination, declination) of the regional field in degrees.

    data: the data components, a tuple drawn from "tf", "bx", "by", "bz" (distinct).  The default ("tf",) with
    weights=None is the module as it always was.  Otherwise dobs is a sequence of len(data) arrays, or a dict keyed by
    component, each of the N values at the N points, in uT; mangle is needed only when "tf" is among them.  weights:
    None (ones), "std" (w_b = std(dobs_0) / std(dobs_b), MultiComponentModule's rule) or one positive number per
    component.  The module then has components, weights, Wb, dobs (stacked, component-major) and dobsw = Wb dobs;
    forward(model) returns the component-major stack, each block in its own units; kernel(axis, component) selects a
    block; block_means() the means of the last evaluation.  Everything else works as on the default module.

    amplitude = lambda, amplitude_beta = beta: with lambda > 0 every potential evaluation and every chain adds
    lambda * Phi, Phi = sum_c s_c / (s_c + beta) with s_c = mx_c^2 + my_c^2 + mz_c^2 of the PHYSICAL model in A/m (the
    minimum-support functional of the amplitude: compact bodies), evaluated on the device.  The reported model value
    stays R; Phi is `last_amplitude`.  Default 0: off, nothing is launched or changed.

    Attributes: mesh, mshape, mxs/mys/mzs, dobs, Wm, WmInv, WmSquare (M = 3 x cells entries), Aw (a device handle).
    A and kernel(axis) are formed on request from the device copy (Aw Wm: equal to the assembled blocks to rounding).

    HMCSample and misfit_and_grad work on it as on GravMagModule; bounds such as [-mmax, mmax] per component go
    through `boundaries`.  Not supported (NotImplementedError): coordinate="spherical", wavelet compression, the
    matrix-free mode, the shift-invariant store, shards, HMCSampleBatch and more than 16384 observations -- stacked
    rows len(data) x N under vector data -- (the store runs on the fused sweep).  Smoothness and TV need the full mesh (ValueError on a carved one).

    translation_invariant=True keeps the translation-invariant table instead of the kernel (a regular mesh -- no mratio
    growth, mseg or mtopo -- under observations that are a full rectangle of the lattice of the cells' horizontal
    spacings at one height, GravMagModule's translation_invariant): the axis of a column is one more layer coordinate
    of the table, T[component][axis nz + layer][dx][dy], the kernel is never stored and the 16384-row limit does not
    apply.  HMCSample (posterior_stream too), misfit_and_grad, the four regularisers, set_amplitude / Amplitude /
    last_amplitude, forward, block_means, Wm, Wb, dobsw, to_vectors / from_vectors / amplitude / direction and
    translation_invariant_info() work on it; Aw, A and kernel(axis, component) do not exist (NotImplementedError).  It
    does not combine with mtopo, wavelet, matrix_free, shift_invariant, shard or coordinate="spherical", and
    translation_invariant="chains" is refused -- batches of magnetization vectors are not built -- (NotImplementedError
    naming the store and the table); NotImplementedError with the reason if the geometry lacks the structure.
    """
    _props, _prop = 3, 'magnetization'  # (mx, my and mz of the same mesh)
    _names, _arg, _word, _none_weight = _lib.BCOMPONENTS, "data", "data component", True
    _store = property(lambda self: _VSTORE if self._vector else _STORE)

    def __init__(self, dobs, mrange, mspacing, obsurface, mangle=(90, 0), mratio=1, mseg=False, mdivisionsection=[],
                 weightfactor=0.5, amplitude=0.0, amplitude_beta=0.01, device=0, verbose=True, coordinate="cartesian",
                 wavelet=False, matrix_free=False, shift_invariant=False, shard=None, data=("tf",), weights=None,
                 translation_invariant=False, **kwargs):
        self._say = print if verbose else (lambda *a, **k: None)
        self._only_mtopo(kwargs)
        data = self._block_names(data)
        n = int(np.asarray(obsurface[0]).size)
        # the default is the module as it always was: one block of the total field, one mean, no block table
        self._vector = self._spherical or not (data == ("tf",) and weights is None)
        if self._vector:
            dobs, w = self._block_data(data, dobs, weights, n)
        if isinstance(translation_invariant, str) and translation_invariant != "chains":
            raise ValueError("translation_invariant must be True or False, not %r" % (translation_invariant,))
        if translation_invariant:
            self.translation_invariant = True
            self._refuse_on_table(coordinate, wavelet, matrix_free, shift_invariant, shard, kwargs)
            if translation_invariant == "chains":
                raise NotImplementedError("%s on the translation-invariant table (translation_invariant=True) runs one "
                                          "chain: batches of magnetization vectors (translation_invariant=\"chains\") are "
                                          "not built" % self._store)
        else:
            self._refuse(coordinate, wavelet, matrix_free, shift_invariant, shard, len(data) if self._vector else 0, n)
        if not self._vector:
            dobs, w = [np.asarray(dobs, dtype=np.float64).ravel()], np.ones(1)
            if dobs[0].size != n:
                raise ValueError("dobs has %d values, the observation points are %d" % (dobs[0].size, n))
            if n > 16384 and not translation_invariant:
                raise NotImplementedError("%d observations: %s takes at most 16384 (it runs on the fused sweep)"
                                          % (n, self._store))
        if not (amplitude >= 0) or not (amplitude_beta > 0):
            raise ValueError("amplitude must be >= 0 and amplitude_beta > 0")
        self.inc, self.dec = mangle[0], mangle[1]
        title = "Calculating magnetic field (magnetization vector) in %s coordinate." % coordinate
        self._assemble(Engine, title, data, dobs, w, n, mrange, mspacing, obsurface, mratio, mseg, mdivisionsection,
                       weightfactor, shift_invariant, device, kwargs.values())
        if translation_invariant:
            self._hide_Aw()
        self._cells = self._engine.M // 3
        self._amp = None  # (lambda, beta) once the engine holds the term
        self._amp_beta = float(amplitude_beta)
        if amplitude != 0:
            self.set_amplitude(amplitude, amplitude_beta)

    def _set_cells(self, eng, bounds):
        direction = utils.dircos(self.inc, self.dec) if "tf" in self.components else None
        if self.translation_invariant:
            # (the default form too: one block of the total field with one mean, the store the table has a door for)
            eng.set_cells_mvi_data(bounds, direction, self.components, self.weights, translation_invariant=True)
        elif self._vector:
            eng.set_cells_mvi_data(bounds, direction, self.components, self.weights)
        else:
            eng.set_cells_mvi(bounds, direction)

    @property
    def A(self):
        """The unweighted kernel [A_x | A_y | A_z], N x M, from the device copy (Aw Wm; rounding differs)."""
        self._no_table("A")
        A = np.asarray(self.Aw) * self.Wm.diagonal()[None, :]
        return A / self.Wb.diagonal()[:, None] if self._vector else A

    def kernel(self, axis, component=None):
        """Block A_axis (N x M/3, uT per A/m along axis 0 / "x" north, 1 / "y" east, 2 / "z" down), from the device
        copy.  Under vector data: of the data component `component` alone (N rows), or with component=None of every
        row block (len(data) N rows), in the components' own units."""
        self._no_table("kernel(%r, %r)" % (axis, component))
        a = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        if a not in (0, 1, 2):
            raise ValueError("axis must be 0, 1, 2 or 'x', 'y', 'z', got %r" % (axis,))
        if component is not None and component not in self.components:
            raise ValueError("component %r is not one of this module's %r" % (component, self.components))
        m = self._cells
        Aw = np.asarray(self.Aw)[:, a * m:(a + 1) * m]
        if self._vector:
            if component is None:
                Aw = Aw / self.Wb.diagonal()[:, None]
            else:
                b, n = self.components.index(component), self._n
                Aw = Aw[b * n:(b + 1) * n] / self.weights[b]
        return np.asfortranarray(Aw * self.Wm.diagonal()[None, a * m:(a + 1) * m])

    def block_means(self):
        """Under vector data: (means of the last evaluation's weighted prediction Aw mw, means removed from the weighted
        observations), one per data component."""
        if not self._vector:
            raise ValueError("block_means: the module has one block of total-field data (data=('tf',))")
        return super().block_means()

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


class TesseroidMagVectorModule(MagVectorModule):
    """The magnetization vector of every tesseroid under magnetic data, on one MI355X: MagVectorModule(data=...) on a
    spherical mesh (libgravhmc's GH_CELL_TESS_MVI_DATA), for satellite and global surveys.

    obsurface = (lon, lat, height) in degrees and metres; mrange = (west, east, south, north, top, bottom), mspacing =
    (dr, dlat, dlon), mratio, mseg, mdivisionsection as the spherical GravMagModule (TesseroidMesh /
    TesseroidMeshSegment); mtopo carves the mesh.  Every cell has the unknowns (m_N, m_E, m_D) in A/m in the
    north-east-down frame at its centre; model vectors are property-major.  data: distinct components of "tf", "bx",
    "by", "bz" -- north, east and down at each observation -- with dobs a sequence (or dict) of len(data) arrays;
    weights None, "std" or numbers; mangle = (inclination, declination) in degrees of the regional field AT THE
    OBSERVATIONS, scalars or one value per observation point, needed by a "tf" block alone.  ratio: the
    subdivision's distance-size ratio (None: RATIO_GG = 8).

    HMCSample, misfit_and_grad, forward, kernel(axis, component) with axis 0 / 1 / 2 ("x" north, "y" east, "z" down AT
    THE CELL), block_means(), Amplitude / amplitude / direction, to_vectors / from_vectors work as on MagVectorModule:
    the rows are row blocks with a data weight and a mean each, always (a single tf block too).

    shift_invariant=True keeps the shift-invariant table instead of the kernel (regular global grids: every cell row
    a full circle of longitudes, observations on the cells' longitude spacing): the data block is one more coordinate
    of the observation class, the axis block (N, E, D) one of the cell row; nothing is stored per (observation,
    cell) and the 16384-row limit does not apply.  On a grid symmetric about the equator the table is halved by the
    north-south mirror, whose entries take the signs of mirror_signs(data).  With "tf" among the data the table is
    built WITHOUT that mirror (the total field is no pure sign under it), and inc, dec must be equal, bit for bit,
    over every class of observations (same latitude and height; scalars always are).  HMCSample (posterior_stream
    too), misfit_and_grad, forward, block_means, Amplitude / amplitude / direction, to_vectors / from_vectors work on
    the table; Aw, A and kernel(axis, component) do not exist there (NotImplementedError).  NotImplementedError with
    the store's reason if the geometry lacks the structure.

    Not supported (NotImplementedError naming the tesseroid magnetization store): wavelet compression, the
    matrix-free mode, shards, HMCSampleBatch, and more than 16384 stacked rows without shift_invariant=True."""
    _spherical = _has_table = True
    _store = _TSTORE

    def __init__(self, dobs, mrange, mspacing, obsurface, data=("bx", "by", "bz"), weights=None, mangle=(90, 0),
                 amplitude=0.0, amplitude_beta=0.01, mratio=1, mseg=False, mdivisionsection=[], weightfactor=0.5,
                 device=0, verbose=True, wavelet=False, matrix_free=False, shift_invariant=False, shard=None,
                 ratio=None, **kwargs):
        from ..gravmag import tesseroid
        self._ratio = tesseroid.RATIO_GG if ratio is None else ratio
        if not (self._ratio > 0):
            raise ValueError("Invalid ratio {}. Must be > 0.".format(ratio))
        data = (data,) if isinstance(data, str) else tuple(data)
        if shift_invariant and abs((mrange[1] - mrange[0]) - 360.0) > 1e-9 * 360.0:
            # (decided on the host, before any device work: a regional mesh has no table; the library tests the rest)
            raise NotImplementedError("shift-invariant store: %s: a row of cells does not cover the full circle of "
                                      "longitudes" % _TSTORE)
        self._fdir = None
        if "tf" in data:
            self._fdir = tesseroid._field_directions(mangle[0], mangle[1], int(np.asarray(obsurface[0]).size))
            if shift_invariant:
                self._fdir = self._class_directions(self._fdir, mangle, obsurface)
        super().__init__(dobs, mrange, mspacing, obsurface, mangle=mangle, mratio=mratio, mseg=mseg,
                         mdivisionsection=mdivisionsection, weightfactor=weightfactor, amplitude=amplitude,
                         amplitude_beta=amplitude_beta, device=device, verbose=verbose, coordinate="spherical",
                         wavelet=wavelet, matrix_free=matrix_free, shift_invariant=shift_invariant, shard=shard,
                         data=data, weights=weights, **kwargs)

    @staticmethod
    def _class_directions(fdir, mangle, obsurface):
        """The table has one set of entries per class of observations (same latitude and height): inc and dec must
        be equal, bit for bit, over every class.  Returns fdir with every point taking its class's first direction
        (the same bits for the same angles, however the vector was evaluated)."""
        n = fdir.shape[0]
        lat, h = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel()) for a in obsurface[1:3])
        if lat.size != n or h.size != n:
            return fdir                    # (the constructor reports the shapes)
        key = np.stack([lat.view(np.int64), h.view(np.int64)], axis=1)
        _, first, cls = np.unique(key, axis=0, return_index=True, return_inverse=True)
        cls = cls.ravel()
        for ang in mangle[:2]:
            ang = np.asarray(ang, dtype=np.float64)
            if ang.ndim == 0:
                continue
            bits = np.ascontiguousarray(ang.ravel()).view(np.int64)
            if not np.array_equal(bits, bits[first][cls]):
                raise NotImplementedError("shift-invariant store: %s: the total field's direction varies within a "
                                          "class of observations (same latitude and height)" % _TSTORE)
        return np.ascontiguousarray(fdir[first][cls])

    def _set_cells(self, eng, bounds):
        eng.set_cells_tess_mag(bounds, self._ratio, self.components, self.weights, self._fdir,
                               shift_invariant=self.shift_invariant)
