"""Potential energy U(x) and its gradient for HMC gravity inversion, evaluated on the GPU.

Host-side mirror of the reference's `inversion.potential.GravMagModule`
(inversion/potential.py:34-845): same constructor arguments, same public attributes the
drivers and the sampler read (`mshape`, `mask`, `mxs/mys/mzs`, `Wm`, `WmInv`, `WmSquare`,
`Aw`, `mesh`), same `kernelw()` / `misfit_and_grad()` signatures and error behaviour.
What differs is where the work happens: the kernel matrix is assembled, weighted and kept in
HBM by libgravhmc (one HIP launch each instead of the Python cell loop of prism.py:291-316
and the N x M Python loop of potential.py:241-244); `Aw` is a device handle that is copied
back only on request.
"""
import time

import numpy as np
from scipy.sparse import coo_matrix

from .. import _lib, mesher, utils
from ..engine import DeviceMatrix, Engine


def _digest(a):
    """64-bit content digest of a contiguous float64 vector (for GravMagModule._use_reg)."""
    a = np.ascontiguousarray(a)
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(a.data)
    except ImportError:
        import zlib
        b = a.view(np.uint8)
        return (zlib.crc32(b) << 32) | zlib.adler32(b)


def _diag(values):
    row = np.arange(0, values.shape[0])
    return coo_matrix((values, (row, row))).tocsr()


def _mesh(spherical, mrange, mspacing, mratio=1, mseg=False, mdivisionsection=()):
    """The mesh of a module: tesseroids or prisms, dz growing by mratio or, with mseg, piecewise constant."""
    if spherical:
        return (mesher.TesseroidMeshSegment(mrange, mspacing, mdivisionsection) if mseg
                else mesher.TesseroidMesh(mrange, mspacing, mratio))
    return (mesher.PrismMeshSegment(mrange, mspacing, mdivisionsection) if mseg
            else mesher.PrismMesh(mrange, mspacing, mratio))


class _Potential(object):
    """What every inversion module shares: the steps of its constructor that do not depend on the store (the mtopo
    carve, the assembly with the tesseroid divide warning, the column weighting, kernelw), the model transform, the
    regulariser sent to the engine, misfit_and_grad and the reference's wrappers.  `_props`: properties that share the
    mesh `mshape` (the stencil regularisers act on each of them on its own)."""
    _props = 1

    def _carve(self, mesh, topos):
        """mtopo=(x, y, topography): mask the cells above the surface (potential.py:92-96, 899-903)."""
        self.topocarve = False
        for value in topos:
            self.topocarve = True
            self.mask = mesh.carvetopo(value[0], value[1], value[2])

    @staticmethod
    def _build(eng, spherical):
        """build_G (NotImplementedError with the store's reason where a table does not apply), and the reference's
        warning for tesseroids that could not be divided further."""
        eng.build_G()
        if spherical and eng.kernel_stats()["warn_cells"] > 0:
            import warnings
            from ..gravmag.tesseroid import _WARN_DIVIDE
            warnings.warn(_WARN_DIVIDE, RuntimeWarning)

    def _weight(self, weightfactor, zero_safe=False):
        """Column-norm weighting Wm and Aw = A Wm^-1 (potential.py:232-264), on the device.  WmInv of an empty column
        is infinite; zero_safe: 0 there (JointModule)."""
        wm = self._engine.weight(weightfactor)
        with np.errstate(divide='ignore'):
            inv = np.where(wm == 0, 0.0, 1.0 / wm) if zero_safe else 1.0 / wm
        self.Wm = _diag(wm)
        self.WmInv = _diag(inv)
        self.WmSquare = _diag(wm * wm)
        self.Aw = DeviceMatrix(self._engine)

    def kernelw(self):
        """(Aw, WmInv, Wm) as the sampler expects (potential.py:584-589, 1561-1566); Aw is a device handle."""
        return self.Aw, self.WmInv, self.Wm

    def _to_mw(self, x, low, high, constraint, log_fator):
        if constraint == 'logarithmic':
            return (low + high * np.e ** (log_fator * x)) / (1 + np.e ** (log_fator * x))
        elif constraint == 'mandatory':
            return x
        raise ValueError("Please choose right boundary constraint(mandatory, logarithmic)!")

    def _use_reg(self, regulization, alpha, beta, mwapr):
        if regulization not in _lib.REG_KINDS:
            raise ValueError("Please choose regularization from 'MS','Damping', 'Smoothness', 'TV'.")
        mwapr = np.asarray(mwapr, dtype=np.float64)
        # The decision to (re)send the regulariser must be the same on every rank of a sharded
        # model (gh_set_reg is collective there) and must notice in-place edits: it depends only
        # on the VALUES -- kind, alpha, beta and the content of the full mwapr vector -- never on
        # addresses.  The content is compared through a 64-bit digest of its bytes (xxh3: ~10 GB/s,
        # one pass, no second copy of the vector kept; zlib.crc32 pair where xxhash is missing).
        key = (regulization, float(alpha), float(beta))
        digest = (mwapr.shape, _digest(mwapr))
        last = self._engine._reg_key
        if last is None or last[0] != key or last[1] != digest:
            m_model = getattr(self._engine, "M_global", self._engine.M)
            cells = self._props * int(np.prod(self.mshape))
            if regulization in ("Smoothness", "TV") and cells != m_model:
                raise ValueError("Smoothness/TV need the full (uncarved) mesh: %sshape %r has %d "
                                 "cells, model has %d" % ("" if self._props == 1 else "%d x " % self._props,
                                                          self.mshape, cells, m_model))
            self._engine.set_reg(regulization, alpha, beta, self.mshape, mwapr)
            self._engine._reg_key = (key, digest)

    def misfit_and_grad(self, x, mwapr, low, high, constraint, log_fator, alpha,
                        regulization='Damping', beta=0.01):
        """(misfit, grad, dpre, data_value, model_value) -- potential.py:812-845 (JointModule: 1780-1812)."""
        mw = self._to_mw(x, low, high, constraint, log_fator)
        self._use_reg(regulization, alpha, beta, mwapr)
        return self._engine.misfit_and_grad(mw)

    # wrappers the reference keeps for an (unused) adaptive regularisation factor
    def data(self, x, low, high, constraint, log_fator):
        mw = self._to_mw(x, low, high, constraint, log_fator)
        self._use_reg("Damping", 0.0, 0.01, np.zeros(self._engine.M))
        return self._engine.misfit_and_grad(mw)[3]

    def _model(self, kind, x, mwapr, low, high, constraint, log_fator, beta=0.01):
        mw = self._to_mw(x, low, high, constraint, log_fator)
        self._use_reg(kind, 1.0, beta, mwapr)
        return self._engine.misfit_and_grad(mw)[4]

    def model_MS(self, x, mwapr, low, high, constraint, log_fator, beta):
        return self._model("MS", x, mwapr, low, high, constraint, log_fator, beta)

    def model_Damping(self, x, mwapr, low, high, constraint, log_fator):
        return self._model("Damping", x, mwapr, low, high, constraint, log_fator)

    def model_Smoothness(self, x, mwapr, low, high, constraint, log_fator):
        return self._model("Smoothness", x, mwapr, low, high, constraint, log_fator)

    def model_TV(self, x, mwapr, low, high, constraint, log_fator, beta):
        return self._model("TV", x, mwapr, low, high, constraint, log_fator, beta)


class GravMagModule(_Potential):
    """Gravity / magnetic inversion model: mesh + sensitivity matrix + potential, on one MI355X.

    Parameters are the reference's (potential.py:35-58):

    * cartesian: mrange = (xmin, xmax, ymin, ymax, zmin, zmax), mspacing = (dz, dy, dx),
      obsurface = [xobs, yobs, height]; y East, x North, z Down.
    * spherical: mrange = (west, east, south, north, top, bottom), mspacing = (dr, dlat, dlon),
      obsurface = [lons, lats, height].
    * fixed / grav_fix: field of cells that do not take part in the inversion.
    * mratio: geometric growth of dz; mseg / mdivisionsection: piecewise dz.
    * weightfactor: exponent of the column-norm sensitivity weighting (0.5 = 2-norm).
    * wavelet: False, '1D' or '3D' (compressed forward operator).
    * field: "gravity" (gz, mGal per g/cm^3) or "magnetic" (cartesian only: the total-field anomaly in uT
      per A/m of magnetization along the regional field of mangle = (inclination, declination) in degrees,
      gravmag.prism.tf).
    * component: the gravity field of a cartesian gravity model (extension; the reference's module inverts gz
      only): "gz" (default), "potential", "geoid", "gx", "gy" or a gradient-tensor component "gxx", "gxy",
      "gxz", "gyy", "gyz", "gzz" -- the kernel of gravmag.prism.<component>, in its units.  Spherical models
      take gz only (NotImplementedError), the magnetic field none (ValueError).
    * mtopo=(x, y, topography) keyword: carve the mesh with a topography surface.
    * device: GPU ordinal (extension; the reference has no such argument).
    * shard: a `dist.Ranks` object: the cells of ONE model are split in column blocks over the
      ranks' GPUs (each holds N x M/world of G); shard_backend "rccl" or "gloo"; shard_planes=True
      splits in whole z-planes, which the Smoothness/TV regularisers need on a sharded model.
      shard_axis="rows": the OBSERVATIONS are split instead (row blocks, the model replicated: a gradient
      all-reduce per step); the wavelet-compressed forward works on row blocks only.
    * matrix_free: never store G; re-evaluate the prism / tesseroid entries in every potential
      evaluation (for kernels larger than HBM; the global tesseroid example: ~5x slower per step than
      the dense path).
    * shift_invariant: spherical models whose cell rows cover the full circle of longitudes with the
      observations on the same spacing (example/global/main_global.py:25-28): keep the table
      K[i, (c, k)] = T[c][class_i][(m_i - k) mod n] (35 MB for the global example) instead of G
      (4.25 GB); NotImplementedError from the constructor if the geometry lacks the structure.
    * translation_invariant: cartesian models whose mesh is regular (no mratio growth, mseg or mtopo) with the
      observations a full rectangle of the lattice of the cells' horizontal spacings at one height (gridded data
      above cell centres, cell corners or anywhere else): keep the table T[layer][dx][dy] (15.8 MB for 100 x 100 x 50
      cells under 100 x 100 points) instead of G (40 GB); works with component= and field="magnetic", behaves as
      matrix_free=True wherever the stored kernel would be needed, has no limit on N.  NotImplementedError from the
      constructor with the reason if the geometry lacks the structure (utils.regular puts n points L / (n - 1)
      apart, the cells are L / n wide), and with wavelet, shard, matrix_free, shift_invariant, mtopo and
      HMCSampleBatch.  translation_invariant="chains" is the same table with HMCSampleBatch: up to 16 chains share
      every read of it (R-hat from the posterior stream), the other refusals unchanged.
    """

    def __init__(self, dobs, mrange, mspacing, obsurface, fixed=False, grav_fix=[],
                 mratio=1, mseg=False, mdivisionsection=[], weightfactor=0.5,
                 coordinate="cartesian", njobs=1, field="gravity",
                 mangle=(90, 0), wavelet=False, device=0, verbose=True, shard=None,
                 shard_backend="rccl", matrix_free=False, shard_planes=False, shift_invariant=False, shard_axis="cells",
                 component="gz", translation_invariant=False, **kwargs):
        self.dobs = dobs
        self.fixed = fixed
        self.grav_fix = grav_fix
        self.mrange = mrange
        self.mspacing = mspacing
        self.mratio = mratio
        self.weightfactor = weightfactor
        self.mseg = mseg
        self.mdivisionsection = mdivisionsection
        self.lonobs = obsurface[0]
        self.latobs = obsurface[1]
        self.heightobs = obsurface[2]
        self.inc, self.dec = mangle[0], mangle[1]
        self.njobs = njobs
        self.wavelet = wavelet
        self.device = device
        self._say = print if verbose else (lambda *a, **k: None)

        if field not in ("gravity", "magnetic") or coordinate not in ("cartesian", "spherical"):
            raise ValueError("Please choose coordinate from(cartesian, spherical) and field "
                             "from(gravity, magnetic)!")
        if field == "magnetic" and coordinate == "spherical":
            # (the reference's branch is `pass`, then a NameError on the undefined mesh: potential.py:106-108)
            raise NotImplementedError("the magnetic field on tesseroids (coordinate='spherical') is not supported")
        magnetic = field == "magnetic"
        if component not in _lib.COMPONENTS:
            raise ValueError("component must be one of %s" % ", ".join(_lib.COMPONENTS))
        if component != "gz":
            if magnetic:
                raise ValueError("component=%r is a gravity field: the magnetic field is the total-field anomaly"
                                 % component)
            if coordinate == "spherical":
                raise NotImplementedError("component=%r on tesseroids (coordinate='spherical') is not supported: "
                                          "spherical models take gz only" % component)
        self.component = component
        if wavelet not in (False, None, '1D', '3D'):
            raise ValueError("wavelet must be False, '1D' or '3D'")
        if component != "gz":
            self._say("Calculating {} field ({}) in {} coordinate.".format(field, component, coordinate))
        else:
            self._say("Calculating {} field in {} coordinate.".format(field, coordinate))
        spherical = coordinate == "spherical"
        if translation_invariant:
            store = "the translation-invariant store (translation_invariant=True)"
            if spherical:
                raise NotImplementedError(store + " is for cartesian (prism) models; spherical grids: shift_invariant")
            for on, why in ((wavelet, "wavelet: the compressor's rows need the stored kernel"),
                            (shard is not None and getattr(shard, "world", 1) > 1, "shard: one GPU holds the table"),
                            (matrix_free, "matrix_free: one form at a time (the store already never stores G)"),
                            (shift_invariant, "shift_invariant: that table is for spherical grids"),
                            (bool(kwargs), "mtopo: a carved mesh is not a full regular product of cells")):
                if on:
                    raise NotImplementedError(store + " does not combine with " + why)
        mesh = _mesh(spherical, mrange, mspacing, mratio, mseg, mdivisionsection)
        self._carve(mesh, kwargs.values())  # (any keyword is the topography, as in the reference)
        if magnetic:
            # (potential.py:139: zero magnetization along the field; the reference's magnetic branch always
            # builds PrismMesh and ignores mseg (potential.py:131) -- mseg is honoured here as for gravity)
            mesh.addprop('magnetization', utils.ang2vec(np.zeros(mesh.size), self.inc, self.dec))
        else:
            mesh.addprop('density', np.zeros(mesh.size))
        self.mesh = mesh

        bounds = mesh.cell_bounds(active_only=True)
        N = int(np.asarray(self.lonobs).size)
        self._say("Start of calculate kernel")
        start = time.time()
        if shard is not None and shard.world > 1:
            if shard_axis not in ("cells", "rows"):
                raise ValueError("shard_axis must be 'cells' (column blocks) or 'rows' (row blocks)")
            if wavelet and shard_axis != "rows":
                raise NotImplementedError("wavelet forward on a kernel sharded in column blocks is not supported "
                                          "(shard_axis='rows': every rank compresses its own rows)")
            from ..dist import make_sharded_engine
            align = 1
            if shard_planes:
                if bounds.shape[0] != mesh.size:
                    raise ValueError("shard_planes needs the full (uncarved) mesh")
                align = int(mesh.shape[1]) * int(mesh.shape[2])
            eng = make_sharded_engine(N, bounds.shape[0], shard, backend=shard_backend, align=align, axis=shard_axis)
        else:
            eng = Engine(N, bounds.shape[0], device=device)
        if matrix_free:
            eng.set_matrix_free(True)      # (with wavelet: the compressor's rows are evaluated, never stored)
        if shift_invariant:
            if not spherical:
                raise NotImplementedError("the shift-invariant store is for spherical (tesseroid) models")
            eng.set_shift_invariant(True)
        if translation_invariant:
            # ("chains": the table that also takes HMCSampleBatch; any other string is the engine's ValueError)
            eng.set_translation_invariant(translation_invariant if isinstance(translation_invariant, str) else True)
        self.matrix_free = bool(matrix_free or shift_invariant or translation_invariant)
        self.translation_invariant = bool(translation_invariant)
        eng.set_obs(self.lonobs, self.latobs, self.heightobs)
        if spherical:
            self._say("Number of effective tesseroids", bounds.shape[0])
            eng.set_cells(bounds, _lib.CELL_TESSEROID, 1.6)
        elif magnetic:
            eng.set_cells(bounds, _lib.CELL_PRISM_TF, direction=utils.dircos(self.inc, self.dec))
        elif component != "gz":
            eng.set_cells(bounds, _lib.CELL_PRISM_COMP, component=component)
        else:
            eng.set_cells(bounds, _lib.CELL_PRISM)
        self._build(eng, spherical)
        if magnetic:
            self._say("End of calculate kernel:", time.time() - start)   # (potential.py:149)
        else:
            if not spherical:
                self._say("kernel.shape", (N, bounds.shape[0]))
            self._say("End of calculate kernel:%.6f s" % (time.time() - start))
        self._engine = eng

        self.mshape = mesh.shape
        self.mxs, self.mys, self.mzs = mesh.get_xs(), mesh.get_ys(), mesh.get_zs()
        self._say("Start to weight kernel")
        start = time.time()
        self.sensitivityWeighting()
        self._say("End of weighting kernel: %.6f s" % (time.time() - start))
        eng.set_data(self.dobs, self.grav_fix if self.fixed else None)
        if wavelet in ('1D', '3D'):
            # gravmag/compressor1D.py / compressor3D.py: db4, level 2, 'periodization',
            # threshold 1e-3, CSR -- built and applied on the device
            self._say("Using {} wavelet to compress kernel.".format(wavelet))
            eng.compress_wavelet(3 if wavelet == '3D' else 1, self.mshape, 0.001, 2)

    def translation_invariant_info(self):
        """The engine's translation_invariant_info(): on, nx, ny, nz, px, qy, table_bytes, max_dev, build_ms."""
        return self._engine.translation_invariant_info()

    @property
    def Awcp(self):
        """Compressed kernel as scipy CSR (copied from the device on request)."""
        if not self.wavelet:
            raise AttributeError("Awcp exists only with wavelet='1D' or '3D'")
        return self._engine.download_csr()

    # ------------------------------------------------------------------ weighting
    def sensitivityWeighting(self):
        """Column-norm weighting Wm and Aw = A Wm^-1 (potential.py:232-264), on the device."""
        self._weight(self.weightfactor)


class _OnTable(object):
    """What the modules whose store also runs on a table instead of the stored kernel share (the stores of row blocks,
    JointModule): the info, the hidden device handle, and the refusal of what is formed from the kernel.  A class states
    `_store`, the store's name in the refusals."""
    translation_invariant = shift_invariant = False

    def translation_invariant_info(self):
        """The engine's translation_invariant_info(): on, nx, ny, nz, px, qy, table_bytes (all blocks), max_dev (the
        largest of the blocks'), build_ms; on a table of magnetization vectors also axes, chunks, layers_per_chunk."""
        return self._engine.translation_invariant_info()

    def _hide_Aw(self):
        """On the translation-invariant table no store is behind the device handle the constructor leaves: the sampler
        keeps it (kernelw), the attribute Aw raises."""
        self._Aw = self.__dict__.pop("Aw")

    # ------------------------------------------------------------------ what is formed from the store
    def _no_table(self, what):
        if self.translation_invariant:
            raise NotImplementedError("%s: %s keeps the translation-invariant table, the kernel is never stored" %
                                      (what, self._store))
        if self.shift_invariant:
            raise NotImplementedError("%s: %s keeps the shift-invariant table, the kernel is never stored" %
                                      (what, self._store))

    def __getattr__(self, name):
        # (reached for an attribute that does not exist: Aw on the translation-invariant table, where no store is behind
        # the device handle the constructor leaves)
        if name == "Aw" and self.__dict__.get("translation_invariant"):
            self._no_table("Aw")
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def kernelw(self):
        """(Aw, WmInv, Wm) as the sampler expects; Aw is a device handle (on the table: of the tables)."""
        return (self._Aw if self.translation_invariant else self.Aw), self.WmInv, self.Wm


class _BlockStore(_OnTable, _Potential):
    """The modules whose store stacks row blocks -- data components of the same cells at the same points, block b in
    its own units times a data weight w_b, with a mean of its own (MultiComponentModule, MagVectorModule and their
    tesseroid forms) -- share the parser of their data, the ladder of their refusals, their construction and what is
    formed from Wb.  A class states `_names` (the table of its components' names), `_arg` and `_word` (what its texts
    call the argument and one component), `_none_weight` (weights=None means ones), `_store` (the store's name in the
    refusals), `_spherical` and `_has_table` (tesseroids; shift_invariant=True keeps the shift-invariant table), `_prop`
    and `_props` (the mesh property, and its unknowns per cell), and `_set_cells(eng, bounds)`, the engine call."""
    _spherical = False
    _has_table = False
    _rows_hint = ""     # (what the refusal of more than 16384 rows adds)
    _vector = True      # (False on MagVectorModule's default form alone: one block of the total field, no Wb)

    # ------------------------------------------------------------------ the arguments
    def _block_names(self, names):
        names = (names,) if isinstance(names, str) else tuple(names)
        if len(names) == 0:
            raise ValueError("%s is empty: name at least one of %s" % (self._arg, ", ".join(self._names)))
        for c in names:
            if c not in self._names:
                raise ValueError("%s %r: must be one of %s" % (self._word, c, ", ".join(self._names)))
        if len(set(names)) != len(names):
            raise ValueError("%ss must be distinct, got %r" % (self._word, names))
        return names

    def _block_data(self, names, dobs, weights, n):
        """(the blocks' observation vectors, their data weights) from a sequence or dict dobs of n values per block and
        weights "std", numbers or (with `_none_weight`) None."""
        if isinstance(dobs, dict):
            if set(dobs) != set(names):
                raise ValueError("dobs has the components %r, expected %r" % (sorted(dobs), sorted(names)))
            dobs = [dobs[c] for c in names]
        dobs = [np.asarray(d, dtype=np.float64).ravel() for d in dobs]
        if len(dobs) != len(names):
            raise ValueError("%d observation vectors for %d %ss" % (len(dobs), len(names), self._word))
        for c, d in zip(names, dobs):
            if d.size != n:
                raise ValueError("dobs of %s has %d values, the observation points are %d" % (c, d.size, n))
        bad = "weights must be %s'std' or one positive number per %s" % ("None, " if self._none_weight else "", self._word)
        if weights is None and self._none_weight:
            w = np.ones(len(names))
        elif isinstance(weights, str):
            if weights != "std":
                raise ValueError(bad)
            sd = np.array([np.std(d) for d in dobs])
            if not np.all(sd > 0):
                raise ValueError("weights='std' needs observations that vary in every component")
            w = sd[0] / sd
        else:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if w.size != len(names) or not np.all(np.isfinite(w)) or not np.all(w > 0):
                raise ValueError(bad)
        return dobs, w

    @staticmethod
    def _only_mtopo(kwargs):
        unknown = sorted(set(kwargs) - {"mtopo"})
        if unknown:
            raise TypeError("unexpected keyword argument %r" % unknown[0])

    def _refuse(self, coordinate, wavelet, matrix_free, shift_invariant, shard, blocks=0, n=0):
        """What the store does not do, decided before any device work; blocks x n: its stacked rows."""
        store = self._store
        if coordinate == "spherical" and not self._spherical:
            raise NotImplementedError("%s holds prism fields: tesseroids (coordinate='spherical') are not supported"
                                      % store)
        if coordinate != ("spherical" if self._spherical else "cartesian"):
            raise ValueError("Please choose coordinate from(cartesian, spherical)!")
        if wavelet not in (False, None):
            raise NotImplementedError("wavelet compression of %s is not supported" % store)
        if matrix_free:
            raise NotImplementedError("%s is dense: the matrix-free mode is not supported" % store)
        if shift_invariant and not self._has_table:
            raise NotImplementedError("%s is dense: the shift-invariant store is not supported" % store)
        if shard is not None:
            raise NotImplementedError("%s is not sharded" % store)
        if blocks * n > 16384 and not shift_invariant:
            raise NotImplementedError("%d %ss x %d observations = %d rows: %s takes at most 16384 (it runs on the fused "
                                      "sweep)%s" % (blocks, self._word, n, blocks * n, store, self._rows_hint))

    # ------------------------------------------------------------------ the construction
    def _assemble(self, engine, title, names, dobs, w, n, mrange, mspacing, obsurface, mratio, mseg, mdivisionsection,
                  weightfactor, shift_invariant, device, topos):
        """Mesh, assembly, weighting and data of the blocks `names` with the observation vectors dobs and the data
        weights w at the n points of obsurface, with the lines the constructors print.  engine: Engine, by the name
        the class's own file has for it (the host suites replace that name to see where device work starts)."""
        self.components, self.weights, self._n = names, w, n
        self.mrange, self.mspacing, self.mratio = mrange, mspacing, mratio
        self.mseg, self.mdivisionsection = mseg, mdivisionsection
        self.weightfactor = weightfactor
        self.lonobs, self.latobs, self.heightobs = obsurface[0], obsurface[1], obsurface[2]
        self.wavelet = False
        self.device = device
        self.shift_invariant = bool(shift_invariant)

        self._say(title)
        mesh = _mesh(self._spherical, mrange, mspacing, mratio, mseg, mdivisionsection)
        self._carve(mesh, topos)
        mesh.addprop(self._prop, np.zeros(mesh.size if self._props == 1 else (mesh.size, self._props)))
        self.mesh = mesh

        bounds = mesh.cell_bounds(active_only=True)
        self._say("Start of calculate kernel")
        start = time.time()
        eng = engine(len(dobs) * n, self._props * bounds.shape[0], device=device)
        self._set_cells(eng, bounds)
        eng.set_obs(self.lonobs, self.latobs, self.heightobs)
        self._build(eng, self._spherical)
        self._say("kernel.shape", (eng.N, eng.M))
        self._say("End of calculate kernel:%.6f s" % (time.time() - start))
        self._engine = eng

        self.mshape = mesh.shape
        self.mxs, self.mys, self.mzs = mesh.get_xs(), mesh.get_ys(), mesh.get_zs()
        self._say("Start to weight kernel")
        start = time.time()
        self.sensitivityWeighting()
        self._say("End of weighting kernel: %.6f s" % (time.time() - start))
        self.dobs = np.concatenate(dobs)
        if self._vector:
            self.dobsw = self.Wb @ self.dobs
        eng.set_data(self.dobsw if self._vector else self.dobs)

    def sensitivityWeighting(self):
        """Wb (w_b on block b), Wm (column norms of Wb A to the power 2 weightfactor, over all M columns) and
        Aw = Wb A Wm^-1, on the device."""
        self._weight(self.weightfactor)
        if self._vector:
            self.Wb = _diag(np.repeat(self.weights, self._n))

    # ------------------------------------------------------------------ on the translation-invariant table
    translation_invariant = translation_invariant_chains = False

    def _refuse_on_table(self, coordinate, wavelet, matrix_free, shift_invariant, shard, kwargs):
        """What the store does not do on the translation-invariant table, decided before any device work (the rows are
        not limited there)."""
        store = "%s on the translation-invariant table (translation_invariant=True)" % self._store
        if coordinate == "spherical":
            raise NotImplementedError("%s holds prism fields: tesseroids (coordinate='spherical') are not supported"
                                      % store)
        if coordinate != "cartesian":
            raise ValueError("Please choose coordinate from(cartesian, spherical)!")
        for on, why in ((wavelet not in (False, None), "wavelet: the compressor's rows need the stored kernel"),
                        (matrix_free, "matrix_free: one form at a time (the table already never stores G)"),
                        (shift_invariant, "shift_invariant: that table is for spherical grids"),
                        (shard is not None, "shard: one GPU holds the table"),
                        (bool(kwargs), "mtopo: a carved mesh is not a full regular product of cells")):
            if on:
                raise NotImplementedError(store + " does not combine with " + why)

    def forward(self, model):
        """Unweighted forward A @ model of the physical model (M entries, property-major): the predicted values,
        component-major, each block in its own units."""
        model = np.asarray(model, dtype=np.float64).ravel()
        d = self._engine.forward(model * self.Wm.diagonal())
        return d / self.Wb.diagonal() if self._vector else d

    def block_means(self):
        """(means of the last evaluation's weighted prediction Aw mw, means removed from the weighted observations),
        one per block."""
        info = self._engine.multi_info()
        return info["pred_mean"], info["obs_mean"]
