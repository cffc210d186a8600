"""Several prism gravity components of one density model inverted together, evaluated on the GPU.

Gradiometry surveys deliver several components at the same stations -- gz with gzz, or the full tensor -- and
their value lies in being inverted together: gzz and gxx / gyy sharpen edges and shallow structure, gz holds depth
and total mass.  MultiComponentModule stacks the kernels of C components of the same mesh in row blocks of ONE
dense store (libgravhmc's GH_CELL_PRISM_MULTI): rows [c N, (c + 1) N) of A hold component c in its own units,
the entries of gravmag.prism.<component>.  A data weighting Wb balances the blocks, the column norms Wm are those
of Wb A, and the data term removes the mean of every block on its own:

    r_c = (d_c - mean d_c) - (dobs_c - mean dobs_c),   data_value = sum_c |r_c|^2,   grad = 2 Aw^T r

with d = Aw mw, Aw = Wb A Wm^-1 and dobs the weighted observations.  With one component the module is
GravMagModule(component=c).  The sweep, the weighting and the regularisers are the single-component ones: they see a
dense store of C N rows.
"""
import time

import numpy as np

from .. import _lib, mesher
from ..engine import DeviceMatrix, Engine
from .potential import _diag, _Potential

_STORE = "the multi-component store"


class MultiComponentModule(_Potential):
    """C gravity components of one prism density model, inverted together on one MI355X.

    dobs: a sequence of C arrays, or a dict keyed by component, each of the N values observed at the N stations
    obsurface = [xobs, yobs, height]; components: C distinct names of the prism gravity fields ("gz", "gzz", "gxx",
    ...: _lib.COMPONENTS), the order of the row blocks.  mrange, mspacing, mratio, mseg, mdivisionsection,
    weightfactor, mtopo=(x, y, topography), device and verbose as GravMagModule.

    weights: "std" gives block c the data weight w_c = std(dobs_0) / std(dobs_c) (JointModule's rule: w_0 = 1); a
    sequence of C positive numbers is used as given.

    Attributes: components, weights, mesh, mshape, mxs/mys/mzs, dobs (the C N stacked observations, component-major),
    dobsw = Wb dobs, Wb, Wm, WmInv, WmSquare, Aw (a device handle; np.asarray(Aw) is the weighted C N x M store).
    A and kernel(component) are formed on request from the device copy (Wb^-1 Aw Wm: equal to prism.<component>'s
    kernel to rounding, not bit for bit).

    HMCSample and misfit_and_grad work on it as on GravMagModule.  Not supported (NotImplementedError): tesseroids
    (coordinate="spherical"), wavelet compression, the matrix-free mode, the shift-invariant store, shards,
    HMCSampleBatch, and more than 16384 stacked rows C N (the store runs on the fused sweep).  The folded store is
    chosen for gz prisms alone: this store is never folded (Engine.fold_info() tells).
    """
    _props = 1
    _spherical = False   # (TesseroidMultiComponentModule: tesseroids, and the shift-invariant store)
    _store = _STORE

    def __init__(self, dobs, mrange, mspacing, obsurface, components=("gz",), weights="std", mratio=1, mseg=False,
                 mdivisionsection=[], weightfactor=0.5, coordinate="cartesian", wavelet=False, device=0, verbose=True,
                 shard=None, matrix_free=False, shift_invariant=False, **kwargs):
        self._say = print if verbose else (lambda *a, **k: None)
        components = (components,) if isinstance(components, str) else tuple(components)
        if len(components) == 0:
            raise ValueError("components is empty: name at least one of %s" % ", ".join(_lib.COMPONENTS))
        for c in components:
            if c not in _lib.COMPONENTS:
                raise ValueError("component %r: must be one of %s" % (c, ", ".join(_lib.COMPONENTS)))
        if len(set(components)) != len(components):
            raise ValueError("components must be distinct, got %r" % (components,))
        if isinstance(dobs, dict):
            if set(dobs) != set(components):
                raise ValueError("dobs has the components %r, expected %r" % (sorted(dobs), sorted(components)))
            dobs = [dobs[c] for c in components]
        dobs = [np.asarray(d, dtype=np.float64).ravel() for d in dobs]
        if len(dobs) != len(components):
            raise ValueError("%d observation vectors for %d components" % (len(dobs), len(components)))
        n = int(np.asarray(obsurface[0]).size)
        for c, d in zip(components, dobs):
            if d.size != n:
                raise ValueError("dobs of %s has %d values, the observation points are %d" % (c, d.size, n))
        if isinstance(weights, str):
            if weights != "std":
                raise ValueError("weights must be 'std' or one positive number per component")
            sd = np.array([np.std(d) for d in dobs])
            if not np.all(sd > 0):
                raise ValueError("weights='std' needs observations that vary in every component")
            w = sd[0] / sd
        else:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if w.size != len(components) or not np.all(np.isfinite(w)) or not np.all(w > 0):
                raise ValueError("weights must be 'std' or one positive number per component")
        unknown = sorted(set(kwargs) - {"mtopo"})
        if unknown:
            raise TypeError("unexpected keyword argument %r" % unknown[0])
        _STORE = self._store
        if coordinate == "spherical" and not self._spherical:
            raise NotImplementedError("%s holds prism fields: tesseroids (coordinate='spherical') are not supported"
                                      % _STORE)
        if coordinate != ("spherical" if self._spherical else "cartesian"):
            raise ValueError("Please choose coordinate from(cartesian, spherical)!")
        if wavelet not in (False, None):
            raise NotImplementedError("wavelet compression of %s is not supported" % _STORE)
        if matrix_free:
            raise NotImplementedError("%s is dense: the matrix-free mode is not supported" % _STORE)
        if shift_invariant and not self._spherical:
            raise NotImplementedError("%s is dense: the shift-invariant store is not supported" % _STORE)
        if shard is not None:
            raise NotImplementedError("%s is not sharded" % _STORE)
        if len(components) * n > 16384 and not shift_invariant:
            raise NotImplementedError("%d components x %d observations = %d rows: %s takes at most 16384 (it runs on "
                                      "the fused sweep)%s" % (len(components), n, len(components) * n, _STORE,
                                                               "; shift_invariant=True has no such limit"
                                                               if self._spherical else ""))

        self.components = components
        self.weights = w
        self.mrange, self.mspacing, self.mratio = mrange, mspacing, mratio
        self.mseg, self.mdivisionsection = mseg, mdivisionsection
        self.weightfactor = weightfactor
        self.lonobs, self.latobs, self.heightobs = obsurface[0], obsurface[1], obsurface[2]
        self.topocarve = False
        self.wavelet = False
        self.device = device

        self.shift_invariant = bool(shift_invariant)
        self._say("Calculating gravity field ({}) in {} coordinate.".format(", ".join(components), coordinate))
        mesh = self._make_mesh()
        if "mtopo" in kwargs:
            value = kwargs["mtopo"]
            self.topocarve = True
            self.mask = mesh.carvetopo(value[0], value[1], value[2])
        mesh.addprop('density', np.zeros(mesh.size))
        self.mesh = mesh

        bounds = mesh.cell_bounds(active_only=True)
        self._say("Start of calculate kernel")
        start = time.time()
        eng = Engine(len(components) * n, bounds.shape[0], device=device)
        self._set_cells(eng, bounds, components, w)
        eng.set_obs(self.lonobs, self.latobs, self.heightobs)
        self._build(eng)
        self._say("kernel.shape", (len(components) * n, bounds.shape[0]))
        self._say("End of calculate kernel:%.6f s" % (time.time() - start))
        self._engine = eng
        self._n = n

        self.mshape = mesh.shape
        self.mxs, self.mys, self.mzs = mesh.get_xs(), mesh.get_ys(), mesh.get_zs()
        self._say("Start to weight kernel")
        start = time.time()
        self.sensitivityWeighting()
        self._say("End of weighting kernel: %.6f s" % (time.time() - start))
        self.dobs = np.concatenate(dobs)
        self.dobsw = self.Wb @ self.dobs
        eng.set_data(self.dobsw)

    # ------------------------------------------------------------------ the store (the spherical module's differ)
    def _make_mesh(self):
        return (mesher.PrismMeshSegment(self.mrange, self.mspacing, self.mdivisionsection) if self.mseg
                else mesher.PrismMesh(self.mrange, self.mspacing, self.mratio))

    def _set_cells(self, eng, bounds, components, w):
        eng.set_cells_multi(bounds, components, w)

    def _build(self, eng):
        eng.build_G()

    # ------------------------------------------------------------------ weighting
    def sensitivityWeighting(self):
        """Wb (w_c on block c), Wm (column norms of Wb A to the power 2 weightfactor) and Aw = Wb A Wm^-1, on the
        device."""
        wm = self._engine.weight(self.weightfactor)
        with np.errstate(divide='ignore'):
            inv = 1.0 / wm
        self.Wm = _diag(wm)
        self.WmInv = _diag(inv)
        self.WmSquare = _diag(wm * wm)
        self.Wb = _diag(np.repeat(self.weights, self._n))
        self.Aw = DeviceMatrix(self._engine)

    def kernelw(self):
        """(Aw, WmInv, Wm) as the sampler expects; Aw is a device handle."""
        return self.Aw, self.WmInv, self.Wm

    @property
    def A(self):
        """The unweighted stacked kernel, C N x M, from the device copy (Wb^-1 Aw Wm; rounding differs)."""
        return (np.asarray(self.Aw) / self.Wb.diagonal()[:, None]) * self.Wm.diagonal()[None, :]

    def kernel(self, component):
        """The N x M kernel of one component, in its own units, from the device copy."""
        if component not in self.components:
            raise ValueError("component %r is not one of this module's %r" % (component, self.components))
        c = self.components.index(component)
        n = self._n
        Aw = np.asarray(self.Aw)[c * n:(c + 1) * n]
        return np.asfortranarray((Aw / self.weights[c]) * self.Wm.diagonal()[None, :])

    def forward(self, model):
        """Unweighted forward A @ model: C N predicted values, component-major, each block in its own units."""
        model = np.asarray(model, dtype=np.float64)
        return self._engine.forward(model * self.Wm.diagonal()) / self.Wb.diagonal()

    def block_means(self):
        """(means of the last evaluation's weighted prediction Aw mw, means removed from the weighted observations),
        one per component."""
        info = self._engine.multi_info()
        return info["pred_mean"], info["obs_mean"]


_TESS_STORE = "the tesseroid multi-component store"


def _default_ratio(component):
    """The reference's distance-size ratio of a tesseroid field (gravmag/tesseroid.py)."""
    from ..gravmag import tesseroid
    if component in ("potential", "geoid"):
        return tesseroid.RATIO_V
    if component in ("gx", "gy", "gz"):
        return tesseroid.RATIO_G
    return tesseroid.RATIO_GG


class TesseroidMultiComponentModule(MultiComponentModule):
    """C gravity components of one tesseroid density model, inverted together on one MI355X: MultiComponentModule on a
    spherical mesh (libgravhmc's GH_CELL_TESSEROID_MULTI), for satellite gradiometry -- gzz, gxx, gyy, gxz ... measured
    together at orbit height.

    obsurface = (lon, lat, height) in degrees and metres; mrange = (west, east, south, north, top, bottom), mspacing =
    (dr, dlat, dlon), mratio, mseg, mdivisionsection as the spherical GravMagModule (TesseroidMesh /
    TesseroidMeshSegment); mtopo carves the mesh.  components: distinct names of the tesseroid gravity fields
    (gravmag.tesseroid.potential ... gzz), gz included, in the observations' local north-east-down frames; dobs,
    weights ("std" or numbers), Wb, dobsw, block_means(), forward(model), kernel(component), HMCSample and
    misfit_and_grad as MultiComponentModule.

    ratio: the distance-size ratio of the adaptive subdivision.  None takes the reference's per field (RATIO_V = 1 for
    potential / geoid, RATIO_G = 1.6 for gx / gy / gz, RATIO_GG = 8 for the tensor); a number applies to all
    components; a sequence gives one per component.  The attribute ratios holds them.

    shift_invariant=True keeps the shift-invariant table instead of the stacked kernel (regular global grids: every
    cell row a full circle of longitudes, observations on the cells' longitude spacing): the component block is one
    more coordinate of the observation class, G is never stored and the 16384-row limit does not apply; on a grid
    symmetric about the equator the table is halved by the signed north-south mirror.  NotImplementedError with the
    store's reason if the geometry lacks the structure.  On the table Aw, A and kernel(component) do not exist
    (NotImplementedError).

    With components=("gz",) and weight 1 the dense form is GravMagModule(coordinate="spherical"): one block with one
    mean, and block_means() raises ValueError.  Not supported (NotImplementedError naming the tesseroid
    multi-component store): wavelet compression, the matrix-free mode, shards, HMCSampleBatch, and more than 16384
    stacked rows without shift_invariant=True."""
    _spherical = True
    _store = _TESS_STORE

    def __init__(self, dobs, mrange, mspacing, obsurface, components=("gzz",), weights="std", ratio=None,
                 shift_invariant=False, mratio=1, mseg=False, mdivisionsection=[], weightfactor=0.5, device=0,
                 verbose=True, wavelet=False, matrix_free=False, shard=None, **kwargs):
        comps = (components,) if isinstance(components, str) else tuple(components)
        if ratio is None:
            ratios = [_default_ratio(c) for c in comps]
        elif np.ndim(ratio) == 0:
            ratios = [float(ratio)] * len(comps)
        else:
            ratios = [float(r) for r in ratio]
            if len(ratios) != len(comps):
                raise ValueError("%d ratios for %d components" % (len(ratios), len(comps)))
        for r in ratios:
            if not (r > 0):
                raise ValueError("Invalid ratio {}. Must be > 0.".format(r))
        self.ratios = np.asarray(ratios, dtype=np.float64)
        super().__init__(dobs, mrange, mspacing, obsurface, components=comps, weights=weights, mratio=mratio, mseg=mseg,
                         mdivisionsection=mdivisionsection, weightfactor=weightfactor, coordinate="spherical",
                         wavelet=wavelet, device=device, verbose=verbose, shard=shard, matrix_free=matrix_free,
                         shift_invariant=shift_invariant, **kwargs)

    def _make_mesh(self):
        return (mesher.TesseroidMeshSegment(self.mrange, self.mspacing, self.mdivisionsection) if self.mseg
                else mesher.TesseroidMesh(self.mrange, self.mspacing, self.mratio))

    def _set_cells(self, eng, bounds, components, w):
        if self.shift_invariant:
            eng.set_shift_invariant(True)
        eng.set_cells_tess_multi(bounds, components, self.ratios, w)

    def _build(self, eng):
        eng.build_G()   # (NotImplementedError with the store's reason where the table does not apply)
        if eng.kernel_stats()["warn_cells"] > 0:
            import warnings
            from ..gravmag.tesseroid import _WARN_DIVIDE
            warnings.warn(_WARN_DIVIDE, RuntimeWarning)

    def _no_table(self, what):
        if self.shift_invariant:
            raise NotImplementedError("%s: %s keeps the shift-invariant table, the kernel is never stored" %
                                      (what, _TESS_STORE))

    @property
    def A(self):
        self._no_table("A")
        return super().A

    def kernel(self, component):
        if component not in self.components:
            raise ValueError("component %r is not one of this module's %r" % (component, self.components))
        self._no_table("kernel(%r)" % (component,))
        return super().kernel(component)

    def block_means(self):
        if not self._engine._store.table:
            raise ValueError("block_means: the module has one block of unweighted gz (GravMagModule's store)")
        return super().block_means()
