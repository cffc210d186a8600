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
import numpy as np

from .. import _lib
from ..engine import Engine
from .potential import _BlockStore


class MultiComponentModule(_BlockStore):
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
    HMCSampleBatch, and more than 16384 stacked rows C N (the store runs on the fused sweep) without
    translation_invariant=True.  The folded store is chosen for gz prisms alone: this store is never folded
    (Engine.fold_info() tells).

    translation_invariant=True keeps one translation-invariant table per component instead of the stacked kernel
    (regular meshes -- no mratio growth, mseg or mtopo -- under gridded data: the observations a full rectangle of the
    lattice of the cells' horizontal spacings at one height, GravMagModule's translation_invariant): the component
    block is one more coordinate of the table, T[c][layer][dx][dy], G is never stored and the 16384-row limit does
    not apply (the full tensor over 100 x 100 x 50 cells under 100 x 100 stations: 95 MB).  HMCSample (with
    posterior_stream too), misfit_and_grad, forward(model), block_means(), Wb, dobsw, Wm and
    translation_invariant_info() work on it; Aw, A and kernel(component) do not exist (NotImplementedError).
    NotImplementedError with the detection's reason if the geometry lacks the structure, and -- naming the
    multi-component store and the translation-invariant table -- with mtopo, wavelet, matrix_free, shift_invariant,
    shard and coordinate="spherical".

    translation_invariant="chains" is translation_invariant=True in all of this -- the same tables, refusals, forward,
    block_means and translation_invariant_info -- and HMCSampleBatch runs on it as well: up to 16 chains share every
    staged table value of every component (csrc/latbatch.hip.h, the forms over row blocks), so that one run leaves
    R-hat across chains behind (posterior_stream=True).  translation_invariant_batch_plan() tells the partition, and
    whether the extent along y fits the batch tile (832 cells under 832 stations at most; beyond it HMCSampleBatch
    raises NotImplementedError and HMCSample still runs).  Any other string is a ValueError.
    """
    _props, _prop = 1, 'density'
    _names, _arg, _word, _none_weight = _lib.COMPONENTS, "components", "component", False
    _store = "the multi-component store"

    def __init__(self, dobs, mrange, mspacing, obsurface, components=("gz",), weights="std", mratio=1, mseg=False,
                 mdivisionsection=[], weightfactor=0.5, coordinate="cartesian", wavelet=False, device=0, verbose=True,
                 shard=None, matrix_free=False, shift_invariant=False, translation_invariant=False, **kwargs):
        self._say = print if verbose else (lambda *a, **k: None)
        components = self._block_names(components)
        n = int(np.asarray(obsurface[0]).size)
        dobs, w = self._block_data(components, dobs, weights, n)
        self._only_mtopo(kwargs)
        if isinstance(translation_invariant, str) and translation_invariant != "chains":
            raise ValueError("translation_invariant must be True, False or \"chains\", not %r" % (translation_invariant,))
        if translation_invariant:
            self.translation_invariant = True
            self.translation_invariant_chains = translation_invariant == "chains"
            self._refuse_on_table(coordinate, wavelet, matrix_free, shift_invariant, shard, kwargs)
        else:
            if len(components) * n > 16384 and not self._spherical and coordinate == "cartesian":
                self._rows_hint = self._table_hint(mrange, mspacing, mratio, mseg, mdivisionsection, obsurface, kwargs)
            self._refuse(coordinate, wavelet, matrix_free, shift_invariant, shard, len(components), n)
        title = "Calculating gravity field ({}) in {} coordinate.".format(", ".join(components), coordinate)
        self._assemble(Engine, title, components, dobs, w, n, mrange, mspacing, obsurface, mratio, mseg,
                       mdivisionsection, weightfactor, shift_invariant, device, kwargs.values())
        if translation_invariant:
            self._hide_Aw()

    @staticmethod
    def _table_hint(mrange, mspacing, mratio, mseg, mdivisionsection, obsurface, kwargs):
        """What the refusal of more than 16384 rows adds: the way to the translation-invariant table, where the geometry
        has its structure (the library's detection, on the host) -- and nothing where it has not."""
        import ctypes as C
        if kwargs:     # (mtopo: a carved mesh)
            return ""
        try:
            from .potential import _mesh
            b6 = np.ascontiguousarray(_mesh(False, mrange, mspacing, mratio, mseg, mdivisionsection).cell_bounds(),
                                      dtype=np.float64)
            x, y, z = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in obsurface[:3])
            lib = _lib.load()
        except (OSError, ValueError, TypeError, IndexError):
            return ""
        n, m = x.size, b6.shape[0]
        if y.size != n or z.size != n:
            return ""
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        dims = np.zeros(5, dtype=np.int32)
        maps = [np.zeros(k, dtype=np.int32) for k in (3 * m, m, 2 * n, n)]
        rc = lib.gh_lattice_detect(n, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), m,
                                   b6.ctypes.data_as(dp), dims.ctypes.data_as(ip), *[a.ctypes.data_as(ip) for a in maps])
        return "; translation_invariant=True has no such limit" if rc == 0 else ""

    def _set_cells(self, eng, bounds):
        eng.set_cells_multi(bounds, self.components, self.weights,
                            translation_invariant="chains" if self.translation_invariant_chains else self.translation_invariant)

    def translation_invariant_batch_plan(self):
        """The engine's translation_invariant_batch_plan(): the partition of the chain batch's two passes on the tables
        (translation_invariant="chains"; "on" is False otherwise), with "blocks", the number of components."""
        return self._engine.translation_invariant_batch_plan()

    @property
    def A(self):
        """The unweighted stacked kernel, C N x M, from the device copy (Wb^-1 Aw Wm; rounding differs)."""
        self._no_table("A")
        return (np.asarray(self.Aw) / self.Wb.diagonal()[:, None]) * self.Wm.diagonal()[None, :]

    def kernel(self, component):
        """The N x M kernel of one component, in its own units, from the device copy."""
        if component not in self.components:
            raise ValueError("component %r is not one of this module's %r" % (component, self.components))
        self._no_table("kernel(%r)" % (component,))
        c = self.components.index(component)
        n = self._n
        Aw = np.asarray(self.Aw)[c * n:(c + 1) * n]
        return np.asfortranarray((Aw / self.weights[c]) * self.Wm.diagonal()[None, :])


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
    _spherical = _has_table = True
    _store = "the tesseroid multi-component store"
    _rows_hint = "; shift_invariant=True has no such limit"

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

    def _set_cells(self, eng, bounds):
        if self.shift_invariant:
            eng.set_shift_invariant(True)
        eng.set_cells_tess_multi(bounds, self.components, self.ratios, self.weights)

    def block_means(self):
        if not self._engine._store.table:
            raise ValueError("block_means: the module has one block of unweighted gz (GravMagModule's store)")
        return super().block_means()
