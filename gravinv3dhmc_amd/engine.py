"""numpy-facing wrapper of one libgravhmc context (one problem resident on one MI355X)."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64, ptr


#: What an engine's context holds, as the library's table of cell stores has it (csrc/host_cells.h): the kind that was
#: asked for (a CELL_* value; None before the cells), the column blocks (M = cols x cells), the row blocks that share
#: the observation points (N = rows x points) and whether the library keeps a block table for them (multi_info).
Store = collections.namedtuple("Store", "kind cols rows table")


class DeviceMatrix(object):
    """Handle of the (weighted) kernel matrix resident in HBM.

    Stands in for the dense ndarray the reference hands around as `Aw`
    (potential.py:584-589); `np.asarray(handle)` / `.to_numpy()` copies it back,
    Fortran-ordered N x M, only when somebody really asks for it."""

    def __init__(self, engine):
        self._engine = engine
        self.shape = (engine.N, engine.M)
        self.dtype = np.dtype(np.float64)
        self.ndim = 2

    def to_numpy(self):
        eng = self._engine
        if eng.joint:
            # the joint store holds H = [Aw_gz | Aw_tf] (N/2 rows): the stacked layout, zero blocks included
            H = eng.download_G()
            n, m = eng.N // 2, eng.M // 2
            A = np.zeros((eng.N, eng.M), order="F")
            A[:n, :m] = H[:, :m]
            A[n:, m:] = H[:, m:]
            return A
        return eng.download_G()

    def __array__(self, dtype=None, copy=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype)

    @property
    def T(self):
        return self.to_numpy().T

    def __repr__(self):
        return "DeviceMatrix(shape=%r, device=%d)" % (self.shape, self._engine.device)


class Engine(object):
    def __init__(self, N, M, device=0):
        self._lib = _lib.load()
        self.N, self.M, self.device = int(N), int(M), int(device)
        h = C.c_void_p()
        rc = self._lib.gh_create(C.byref(h), self.device, self.N, self.M)
        check(rc, None)
        self._h = h
        self._reg_key = None
        self._chain_valid = False
        self._store = Store(None, 1, 1, False)

    # -- the store (read by the inversion modules) -----------------------------------
    def _set_store(self, kind, cols=1, rows=1, table=False):
        self._store = Store(kind, cols, rows, table)

    joint = property(lambda self: self._store.kind == _lib.CELL_PRISM_JOINT)
    mvi = property(lambda self: self._store.cols == 3)
    tess_mag = property(lambda self: self._store.kind == _lib.CELL_TESS_MVI_DATA)
    tess_multi = property(lambda self: self._store.kind == _lib.CELL_TESSEROID_MULTI)
    #: the length of the block table; 0 without one
    multi = property(lambda self: self._store.rows if self._store.table else 0)

    @staticmethod
    def _blocks(names, components, weights, ratios=None):
        """The row blocks of a store as the library takes them: (values, C array of them, weights, ratios) of the
        components, names of `names` (_lib.COMPONENTS or _lib.BCOMPONENTS) or their values."""
        comps = [names.get(c, -1) if isinstance(c, str) else int(c) for c in components]
        if any(c not in names.values() for c in comps):
            raise ValueError("%scomponent must be one of %s"
                             % ("data " if names is _lib.BCOMPONENTS else "", ", ".join(names)))
        w, r = f64(weights), None if ratios is None else f64(ratios)
        if w.shape != (len(comps),) or (r is not None and r.shape != (len(comps),)):
            raise ValueError("one data weight%s per component" % ("" if r is None else " and one ratio"))
        return comps, (C.c_int * max(len(comps), 1))(*comps), w, r

    # -- lifetime -----------------------------------------------------------------
    def close(self):
        self.__dict__.pop("_p0_pool", None)     # (the blocks go with the context)
        if getattr(self, "_h", None):
            self._lib.gh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        check(rc, self._h)

    def _vecM(self, v, what):
        """Contiguous float64 copy/view of a model vector; the library copies exactly M doubles."""
        v = f64(v)
        if v.shape != (self.M,):
            raise ValueError("%s must have M = %d entries, got shape %r" % (what, self.M, v.shape))
        return v

    def _vecN(self, v, what):
        v = f64(v)
        if v.shape != (self.N,):
            raise ValueError("%s must have N = %d entries, got shape %r" % (what, self.N, v.shape))
        return v

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_int64(0)
        self._chk(self._lib.gh_device_info(self._h, name, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "cus": cus.value, "mem_bytes": mem.value}

    def synchronize(self):
        self._chk(self._lib.gh_synchronize(self._h))

    # -- kernel matrix ------------------------------------------------------------
    def set_obs(self, a, b, c):
        a, b, c = f64(a), f64(b), f64(c)
        # (joint gravity-magnetic context: both blocks share the N/2 observation points)
        # (multi-component context: all blocks share the N / ncomp points)
        n = self.N // self._store.rows
        if not (a.shape == b.shape == c.shape == (n,)):
            raise ValueError("Input arrays xp, yp, and zp must have same length!")
        self._chk(self._lib.gh_set_obs(self._h, ptr(a), ptr(b), ptr(c)))

    def set_cells(self, bounds6, kind, ratio=1.6, direction=None, component=None, translation_invariant=False):
        """kind CELL_PRISM / CELL_TESSEROID (ratio: the tesseroid distance-size ratio), or CELL_PRISM_TF with
        direction = (fx, fy, fz), the unit vector of the regional field (utils.dircos(inc, dec)).
        component (kind CELL_PRISM or CELL_PRISM_COMP for prisms, CELL_TESSEROID or CELL_TESSEROID_COMP for
        tesseroids): the gravity field, a name of _lib.COMPONENTS or a COMP_* value; "gz" is kind CELL_PRISM /
        CELL_TESSEROID itself (gh_set_cells_prism / gh_set_cells_tess).
        CELL_PRISM_JOINT: the M/2 prisms (bounds (M/2, 6)) of a joint gravity-magnetic model -- gz and the total
        field along direction, inverted together (gh_set_cells_joint); call it before set_obs.
        translation_invariant=True, with CELL_PRISM_JOINT alone (gh_set_cells_joint_table): the joint store on the
        translation-invariant table, the property of a column one more layer coordinate and each layer on its own
        observation block (csrc/latjoint.hip.h), no 16384-point limit; build_G raises NotImplementedError with the
        reason if the geometry lacks the structure.  Every other kind takes the table from
        set_translation_invariant."""
        b = f64(bounds6)
        if translation_invariant and int(kind) != _lib.CELL_PRISM_JOINT:
            raise ValueError("set_cells: translation_invariant=True is the joint store's door to the table "
                             "(CELL_PRISM_JOINT); other kinds: set_translation_invariant")
        if isinstance(translation_invariant, str):
            raise ValueError("set_cells: translation_invariant must be True or False, not %r" % (translation_invariant,))
        if int(kind) == _lib.CELL_PRISM_JOINT:
            if b.shape != (self.M // 2, 6):
                raise ValueError("bounds table of a joint model must be (M/2, 6)")
            if direction is None or len(direction) != 3:
                raise ValueError("the joint kernel's total field needs direction = (fx, fy, fz)")
            fx, fy, fz = (float(v) for v in direction)
            fn = self._lib.gh_set_cells_joint_table if translation_invariant else self._lib.gh_set_cells_joint
            self._chk(fn(self._h, ptr(b), fx, fy, fz))
            if translation_invariant:
                self._translation_invariant = True
            self._set_store(_lib.CELL_PRISM_JOINT, cols=2, rows=2)
            return
        if b.shape != (self.M, 6):
            raise ValueError("bounds table must be (M, 6)")
        if int(kind) in (_lib.CELL_TESSEROID, _lib.CELL_TESSEROID_COMP) and \
                (component is not None or int(kind) == _lib.CELL_TESSEROID_COMP):
            comp = _lib.COMPONENTS.get(component, -1) if isinstance(component, str) else component
            if comp not in _lib.COMPONENTS.values():
                raise ValueError("component must be one of %s" % ", ".join(_lib.COMPONENTS))
            if comp == _lib.COMP_GZ:   # (today's call: the same context)
                self._chk(self._lib.gh_set_cells(self._h, ptr(b), _lib.CELL_TESSEROID, float(ratio)))
            else:
                self._chk(self._lib.gh_set_cells_tess(self._h, ptr(b), int(comp), float(ratio)))
            return
        if component is not None or int(kind) == _lib.CELL_PRISM_COMP:
            if int(kind) not in (_lib.CELL_PRISM, _lib.CELL_PRISM_COMP):
                raise ValueError("a gravity component is a field of prisms or tesseroids (kind CELL_PRISM / "
                                 "CELL_PRISM_COMP / CELL_TESSEROID / CELL_TESSEROID_COMP)")
            comp = _lib.COMPONENTS.get(component, -1) if isinstance(component, str) else component
            if comp not in _lib.COMPONENTS.values():
                raise ValueError("component must be one of %s" % ", ".join(_lib.COMPONENTS))
            self._chk(self._lib.gh_set_cells_prism(self._h, ptr(b), int(comp)))
            return
        if int(kind) == _lib.CELL_PRISM_TF:
            if direction is None or len(direction) != 3:
                raise ValueError("the magnetic (total-field) kernel needs direction = (fx, fy, fz)")
            fx, fy, fz = (float(v) for v in direction)
            self._chk(self._lib.gh_set_cells_tf(self._h, ptr(b), fx, fy, fz))
            return
        self._chk(self._lib.gh_set_cells(self._h, ptr(b), int(kind), float(ratio)))

    def set_cells_multi(self, bounds6, components, weights, translation_invariant=False):
        """The M prisms of a multi-component model (gh_set_cells_multi): the gravity fields `components` (names of
        _lib.COMPONENTS or COMP_* values, distinct) of the same cells at the same N / len(components) points, stacked
        in row blocks of one store, block c with the data weight weights[c] > 0; call it before set_obs.
        translation_invariant=True (gh_set_cells_multi_table): one translation-invariant table per block instead of
        the dense store, no 16384-row limit; build_G raises NotImplementedError with the reason if the geometry lacks
        the structure.  translation_invariant="chains" (gh_set_cells_multi_table_chains): the same tables, which also
        take chain batches (batch_init, batch_trajectory, batch_run, batch_block_means; csrc/latbatch.hip.h); any other
        string is a ValueError."""
        if isinstance(translation_invariant, str) and translation_invariant != "chains":
            raise ValueError("set_cells_multi: translation_invariant must be True, False or \"chains\", not %r"
                             % (translation_invariant,))
        chains = translation_invariant == "chains"
        b = f64(bounds6)
        if b.shape != (self.M, 6):
            raise ValueError("bounds table must be (M, 6)")
        comps, carr, w, _ = self._blocks(_lib.COMPONENTS, components, weights)
        fn = self._lib.gh_set_cells_multi_table_chains if chains else \
            self._lib.gh_set_cells_multi_table if translation_invariant else self._lib.gh_set_cells_multi
        self._chk(fn(self._h, ptr(b), len(comps), carr, ptr(w)))
        if translation_invariant:
            self._translation_invariant = True
            self._translation_invariant_chains = chains
        self._set_store(_lib.CELL_PRISM_MULTI, rows=len(comps), table=True)

    def set_cells_tess_multi(self, bounds6, components, ratios, weights):
        """The M tesseroids (w, e, s, n, top, bottom) of a multi-component model (gh_set_cells_tess_multi): rows as
        set_cells_multi, block c the tesseroid field components[c] assembled at the distance-size ratio ratios[c] > 0,
        with the data weight weights[c] > 0.  Dense, or -- set_shift_invariant(True) before build_G -- on the
        shift-invariant table.  Call it before set_obs.  (The unweighted gz alone is the CELL_TESSEROID context.)"""
        b = f64(bounds6)
        if b.shape != (self.M, 6):
            raise ValueError("bounds table must be (M, 6)")
        comps, carr, w, r = self._blocks(_lib.COMPONENTS, components, weights, ratios)
        self._chk(self._lib.gh_set_cells_tess_multi(self._h, ptr(b), len(comps), carr, ptr(r), ptr(w)))
        # (the unweighted gz alone is the tesseroid store itself: one block, no block table)
        self._set_store(_lib.CELL_TESSEROID_MULTI, rows=len(comps), table=not (comps == [_lib.COMP_GZ] and w[0] == 1.0))

    def set_cells_mvi(self, bounds6, direction):
        """The M/3 prisms (bounds (M/3, 6)) of a magnetization-vector model (gh_set_cells_mvi): three unknowns
        (mx, my, mz) per prism, model vectors property-major, the total field along direction = (fx, fy, fz);
        call it before set_obs."""
        b = f64(bounds6)
        if self.M % 3 != 0 or b.shape != (self.M // 3, 6):
            raise ValueError("bounds table of a magnetization-vector model must be (M/3, 6)")
        if direction is None or len(direction) != 3:
            raise ValueError("the magnetization-vector kernel's total field needs direction = (fx, fy, fz)")
        fx, fy, fz = (float(v) for v in direction)
        self._chk(self._lib.gh_set_cells_mvi(self._h, ptr(b), fx, fy, fz))
        self._set_store(_lib.CELL_PRISM_MVI, cols=3)

    def set_cells_mvi_data(self, bounds6, direction, components, weights, translation_invariant=False):
        """The M/3 prisms (bounds (M/3, 6)) of a magnetization-vector model under vector data (gh_set_cells_mvi_data):
        the data `components` (names of _lib.BCOMPONENTS or BCOMP_* values, distinct) at the same N / len(components)
        points, stacked in row blocks, block b with the data weight weights[b] > 0; columns as set_cells_mvi.
        direction = (fx, fy, fz) serves a "tf" block alone (None: zeros).  Call it before set_obs.
        translation_invariant=True (gh_set_cells_mvi_table): the store on the translation-invariant table, the axis of a
        column one more layer coordinate (csrc/latmvi.hip.h), no 16384-row limit; build_G raises NotImplementedError
        with the reason if the geometry lacks the structure.  The unweighted total field alone is then a store of one
        block as well."""
        b = f64(bounds6)
        if self.M % 3 != 0 or b.shape != (self.M // 3, 6):
            raise ValueError("bounds table of a magnetization-vector model must be (M/3, 6)")
        comps, carr, w, _ = self._blocks(_lib.BCOMPONENTS, components, weights)
        if direction is None:
            if _lib.BCOMP_TF in comps:
                raise ValueError("a total-field block needs direction = (fx, fy, fz)")
            direction = (0.0, 0.0, 0.0)
        if len(direction) != 3:
            raise ValueError("direction must be (fx, fy, fz)")
        fx, fy, fz = (float(v) for v in direction)
        fn = self._lib.gh_set_cells_mvi_table if translation_invariant else self._lib.gh_set_cells_mvi_data
        self._chk(fn(self._h, ptr(b), fx, fy, fz, len(comps), carr, ptr(w)))
        if translation_invariant:
            self._translation_invariant = True
        # (the unweighted total field alone is the magnetization-vector store itself: one block, no block table)
        if comps == [_lib.BCOMP_TF] and w[0] == 1.0 and not translation_invariant:
            self._set_store(_lib.CELL_PRISM_MVI, cols=3)
        else:
            self._set_store(_lib.CELL_PRISM_MVI_DATA, cols=3, rows=len(comps), table=True)

    def b_result(self, component, mag3):
        """bx, by or bz (uT; component a name or BCOMP_* value) at the observation points of a magnetization-vector
        context whose M/3 cells are magnetized with mag3[M/3, 3] (A/m), in the reference's accumulation order
        (gh_b_result); needs no G."""
        comp = _lib.BCOMPONENTS.get(component, -1) if isinstance(component, str) else int(component)
        m = f64(mag3)
        if not self.mvi or m.shape != (self.M // 3, 3):
            raise ValueError("magnetization must be (M/3, 3) on a magnetization-vector context")
        out = np.empty(self.N // self._store.rows)
        self._chk(self._lib.gh_b_result(self._h, comp, ptr(m), ptr(out)))
        return out

    def set_cells_tess_mag(self, bounds6, ratio, components, weights, fdir=None, shift_invariant=False):
        """The M/3 tesseroids (bounds (M/3, 6): w, e, s, n, top, bottom) of a magnetization-vector model under magnetic
        data (gh_set_cells_tess_mag): rows as set_cells_mvi_data, columns [K_N | K_E | K_D] for a unit magnetization
        along north, east and down at each cell's centre.  fdir (N / len(components), 3): the unit vectors of the total
        field at the observation points, needed by a "tf" block (or tess_b_result("tf")) alone.  Dense, or -- with
        shift_invariant=True (gh_set_cells_tess_mag_table: no 16384-row limit), or set_shift_invariant(True) AFTER this
        call and before build_G -- on the shift-invariant table: the axis block is then a coordinate of the table's
        cell row, the data block one of the observation class.  Call it before set_obs."""
        b = f64(bounds6)
        if self.M % 3 != 0 or b.shape != (self.M // 3, 6):
            raise ValueError("bounds table of a magnetization-vector model must be (M/3, 6)")
        comps, carr, w, _ = self._blocks(_lib.BCOMPONENTS, components, weights)
        if fdir is None:
            if _lib.BCOMP_TF in comps:
                raise ValueError("a total-field block needs fdir, one unit vector per observation point")
            fp = None
        else:
            fdir = f64(fdir)
            if len(comps) == 0 or fdir.shape != (self.N // len(comps), 3):
                raise ValueError("fdir must be (N / components, 3)")
            fp = ptr(fdir)
        fn = self._lib.gh_set_cells_tess_mag_table if shift_invariant else self._lib.gh_set_cells_tess_mag
        self._chk(fn(self._h, ptr(b), float(ratio), len(comps), carr, ptr(w), fp))
        if shift_invariant:
            self._shift_invariant = True
        self._set_store(_lib.CELL_TESS_MVI_DATA, cols=3, rows=len(comps), table=True)

    def tess_b_result(self, component, mag3):
        """tf, bx, by or bz (uT; component a name or BCOMP_* value) at the observation points of a tesseroid
        magnetization context whose M/3 cells carry mag3[M/3, 3] = (m_N, m_E, m_D) in A/m, without a store
        (gh_tess_b_result); kernel_stats() then reports this pass."""
        comp = _lib.BCOMPONENTS.get(component, -1) if isinstance(component, str) else int(component)
        m = f64(mag3)
        if not self.tess_mag or m.shape != (self.M // 3, 3):
            raise ValueError("magnetization must be (M/3, 3) on a tesseroid magnetization context")
        out = np.empty(self.N // self._store.rows)
        self._chk(self._lib.gh_tess_b_result(self._h, comp, ptr(m), ptr(out)))
        return out

    def set_amplitude(self, lam, beta, scale=1.0):
        """Amplitude coupling lam * sum_c s_c / (s_c + beta) of a weighted magnetization-vector context
        (gh_set_amplitude), s_c the squared amplitude of cell c's physical vector over scale.  lam = 0 switches the
        term off."""
        self._chk(self._lib.gh_set_amplitude(self._h, float(lam), float(beta), float(scale)))
        self._chain_valid = False

    def amplitude_eval(self, mw, want_grad=True, want_amp=True):
        """(Phi, dPhi/dmw or None, the cells' amplitudes (M/3) or None) of the amplitude term alone, lam = 1, with beta
        and scale of the last set_amplitude (gh_amplitude_eval)."""
        mw = self._vecM(mw, "mw")
        val = C.c_double(0)
        grad = np.empty(self.M) if want_grad else None
        amp = np.empty(self.M // 3) if want_amp else None
        self._chk(self._lib.gh_amplitude_eval(self._h, ptr(mw), C.byref(val), ptr(grad), ptr(amp)))
        return val.value, grad, amp

    def amplitude_last(self):
        """Phi of the last misfit_and_grad, or of the state the chain is in (gh_amplitude_last); 0 while off."""
        val = C.c_double(0)
        self._chk(self._lib.gh_amplitude_last(self._h, C.byref(val)))
        return val.value

    def multi_info(self):
        """The row blocks of a multi-component context (gh_multi_info): components (COMP_* values), weights, the
        per-block means of the last evaluation's prediction Aw mw and of the weighted observations."""
        n = C.c_int(0)
        comps = (C.c_int * _lib.MULTI_MAX)()
        w, pm, om = np.zeros(_lib.MULTI_MAX), np.zeros(_lib.MULTI_MAX), np.zeros(_lib.MULTI_MAX)
        self._chk(self._lib.gh_multi_info(self._h, C.byref(n), comps, ptr(w), ptr(pm), ptr(om)))
        k = n.value
        return {"components": [int(v) for v in comps[:k]], "weights": w[:k].copy(), "pred_mean": pm[:k].copy(),
                "obs_mean": om[:k].copy()}

    def tf_result(self, mag3):
        """Total-field anomaly (uT) of the CELL_PRISM_TF or CELL_PRISM_MVI cells magnetized with mag3[M, 3] (A/m), in the
        reference's accumulation order (gh_tf_result); needs no G."""
        m = f64(mag3)
        cells = self.M // 3 if self.mvi else self.M   # (magnetization-vector context: M/3 prisms)
        if m.shape != (cells, 3):
            raise ValueError("magnetization must be (%s, 3)" % ("M/3" if cells != self.M else "M"))
        out = np.empty(self.N)
        self._chk(self._lib.gh_tf_result(self._h, ptr(m), ptr(out)))
        return out

    def prism_result(self, dens):
        """The field of the prism cells (CELL_PRISM or CELL_PRISM_COMP) with densities dens[M] (g/cm^3), in
        the reference's accumulation order (gh_prism_result); needs no G."""
        d = f64(dens)
        if d.shape != (self.M,):
            raise ValueError("density must be (M,)")
        out = np.empty(self.N)
        self._chk(self._lib.gh_prism_result(self._h, ptr(d), ptr(out)))
        return out

    def set_matrix_free(self, on=True, exact=None):
        """Never store G.  exact (tesseroids): True = a far pair's GLQ leaf in the reference's operation
        order (_tesseroid_numba.py:207-222), False = the throughput form (~1e-14 from it); None leaves
        the choice to the environment (GRAVHMC_MF_EXACT, default the throughput form)."""
        self._chk(self._lib.gh_set_matrix_free(self._h, 1 if on else 0))
        if exact is not None:
            self._chk(self._lib.gh_set_matrix_free_exact(self._h, 1 if exact else 0))

    def set_shift_invariant(self, on=True):
        """Regular spherical grids (every cell row a full circle of longitudes, observations on the same
        spacing): keep K[i, (c, k)] = T[c][class_i][(m_i - k) mod n] instead of G (gh_set_shift_invariant);
        build_G raises NotImplementedError with the reason if the geometry lacks the structure."""
        self._chk(self._lib.gh_set_shift_invariant(self._h, 1 if on else 0))
        self._shift_invariant = bool(on)

    def shift_invariant_info(self):
        n, na, nc, tb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self._lib.gh_shift_invariant_info(self._h, C.byref(n), C.byref(na), C.byref(nc), C.byref(tb)))
        return {"n_lon": n.value, "n_classes": na.value, "n_rows": nc.value, "table_bytes": tb.value}

    def shift_invariant_harmonic(self):
        """The store in the longitude-harmonic domain: on, form ("registers": csrc/lonsymh.hip.h, "streamed":
        csrc/lonsymw.hip.h for grids beyond 126 longitudes / 64 observation classes), frequencies, bytes of T^, workgroups."""
        on, nf, tb, wg = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(0)
        self._chk(self._lib.gh_shift_invariant_harmonic(self._h, C.byref(on), C.byref(nf), C.byref(tb), C.byref(wg)))
        return {"on": bool(on.value), "form": {0: None, 1: "registers", 2: "streamed"}[on.value], "n_freq": nf.value,
                "table_bytes": tb.value, "workgroups": wg.value}

    def shift_invariant_plan(self):
        """What build_G decided for the store (gh_shift_invariant_plan; read-only): the form, n / na / nc / nf, the direct
        form's work items (W, KB, AG, thr, items, grid, lds, direct_ok, direct_refusal 0 .. 4), the register form's rows
        per workgroup (rp, rw, hgrid, hlds), the streamed form's layout (nfp, pairs, wmirror, witems, wgrid, wrows, wparts;
        0 where another form runs), the slots (n_xslots, max_extra) and the persistent launch (resident_planned,
        resident_usable with the regulariser set now, nwg, resident_lds)."""
        out = (C.c_int32 * 32)()
        self._chk(self._lib.gh_shift_invariant_plan(self._h, out))
        names = ("form", "n", "na", "nc", "nf", "W", "KB", "AG", "thr", "items", "grid", "lds", "direct_ok", "direct_refusal",
                 "rp", "rw", "hgrid", "hlds", "nfp", "pairs", "wmirror", "witems", "wgrid", "wrows", "wparts", "n_xslots",
                 "max_extra", "resident_planned", "resident_usable", "nwg", "resident_lds", "on")
        d = dict(zip(names, (int(v) for v in out)))
        d["form"] = ("direct", "registers", "streamed")[d["form"]] if d["on"] else None
        for k in ("direct_ok", "wmirror", "resident_planned", "resident_usable", "on"):
            d[k] = bool(d[k])
        return d

    def set_translation_invariant(self, on=True):
        """Regular prism grids under gridded data (cells a full product of equal x- and y-intervals and layers,
        observations a full rectangle of the lattice of the cells' spacings at one height): keep the table
        T[k][p - a + nx - 1][q - b + ny - 1] instead of G (gh_set_translation_invariant, csrc/lattice.hip.h);
        build_G raises NotImplementedError with the reason if the geometry lacks the structure.  on="chains": the same
        table, which also takes chain batches (batch_init, batch_trajectory, batch_run; csrc/latbatch.hip.h);
        on="replicates": the same table, which also takes the bootstrap batch (bscg_run) and refuses chain batches; any
        other string is a ValueError."""
        if isinstance(on, str) and on not in ("chains", "replicates"):
            raise ValueError("set_translation_invariant: on must be True, False, \"chains\" or \"replicates\", not %r" % (on,))
        chains, replicates = on == "chains", on == "replicates"
        mode = _lib.TABLE_CHAINS if chains else _lib.TABLE_REPLICATES if replicates else (1 if on else 0)
        self._chk(self._lib.gh_set_translation_invariant(self._h, mode))
        self._translation_invariant = bool(on)
        self._translation_invariant_chains = chains
        self._translation_invariant_replicates = replicates

    def translation_invariant_batch_plan(self):
        """What the batch passes of set_translation_invariant("chains") planned on the built table
        (gh_translation_invariant_batch_plan; read-only): on, fits (False: batch_init refuses the extent), TR / RW (output
        rows per workgroup / wave), NT (tiles of 16 outputs per wave at most), max_chunks, cus, and per pass
        adj_* / fwd_*: ntiles, FT, WT, WL, grid, lds; lpc (layers per forward chunk), chunks (slab rows), pp_rows.  On
        the tables of set_cells_multi(..., translation_invariant="chains") also blocks, the number of row blocks (the
        forward's grid is that many workgroups deep)."""
        out = (C.c_int32 * 24)()
        self._chk(self._lib.gh_translation_invariant_batch_plan(self._h, out))
        names = ("on", "fits", "TR", "RW", "NT", "max_chunks", "cus") + tuple(
            "%s_%s" % (p, n) for p in ("adj", "fwd") for n in ("ntiles", "FT", "WT", "WL", "grid", "lds")) + (
            "lpc", "chunks", "pp_rows")
        d = dict(zip(names, (int(v) for v in out)))
        d["on"], d["fits"] = bool(d["on"]), bool(d["fits"])
        if out[22]:
            d["blocks"] = int(out[22])
        return d

    def translation_invariant_info(self):
        """on, the lattice's extents nx, ny, nz (cells) and px, qy (observations), table_bytes, and of the build:
        max_dev (the entries of the first and the last pair of an offset, as a fraction of the largest entry) and
        build_ms.  On a table of magnetization vectors (set_cells_mvi_data(..., translation_invariant=True)) also axes
        (3: the table has axes x nz layers), chunks and layers_per_chunk (the forward's partition of those layers)."""
        i = [C.c_int(0) for _ in range(6)]
        tb, md, bm = C.c_int64(0), C.c_double(0), C.c_double(0)
        self._chk(self._lib.gh_translation_invariant_info(self._h, *[C.byref(v) for v in i], C.byref(tb), C.byref(md),
                                                          C.byref(bm)))
        d = {"on": bool(i[0].value), "nx": i[1].value, "ny": i[2].value, "nz": i[3].value, "px": i[4].value,
             "qy": i[5].value, "table_bytes": tb.value, "max_dev": md.value, "build_ms": bm.value}
        if self._store.kind in (_lib.CELL_PRISM_MVI_DATA, _lib.CELL_PRISM_JOINT) and d["on"]:
            # (the joint store on the table, set_cells(..., CELL_PRISM_JOINT, translation_invariant=True): axes = 2, half
            # of the chunks each property's)
            a = [C.c_int(0) for _ in range(3)]
            self._chk(self._lib.gh_translation_invariant_axes(self._h, *[C.byref(v) for v in a]))
            if a[0].value == (2 if self.joint else 3):
                d.update(axes=a[0].value, chunks=a[1].value, layers_per_chunk=a[2].value)
        return d

    def translation_invariant_table(self):
        """The table as it lies on the device: (nz, nx + px - 1, ny + qy - 1); on a multi-component context
        (set_cells_multi(..., translation_invariant=True)) the C blocks' tables, (C, nz, nx + px - 1, ny + qy - 1)."""
        t = self.translation_invariant_info()
        if not t["on"]:
            raise ValueError("no table resident (set_translation_invariant, build_G)")
        shape = (t["nz"], t["nx"] + t["px"] - 1, t["ny"] + t["qy"] - 1)
        if self.joint:        # (the joint store: (2, nz, ., .), gz then tf, the property a layer coordinate)
            shape = (t["axes"],) + shape
        elif t.get("axes"):   # (magnetization vectors: (C, 3, nz, ., .), the axis a layer coordinate)
            shape = (self._store.rows, t["axes"]) + shape
        T = np.empty(((self._store.rows,) + shape) if self._store.kind == _lib.CELL_PRISM_MULTI else shape)
        self._chk(self._lib.gh_translation_invariant_table(self._h, ptr(T)))
        return T

    #: reasons of fold_info (GH_FOLD_* of include/gravhmc.h)
    FOLD_REASONS = ("on", "undecided", "switched off", "not gz prisms", "observations not mirror-symmetric",
                    "cells not mirror-symmetric", "fixed point", "small", "path", "no memory", "deviation")

    #: reasons of fold_info's pair keys (GH_FOLD_PAIR_* of include/gravhmc.h)
    FOLD_PAIR_REASONS = ("on", "undecided", "switched off", "no fold", "observations not square", "cells not square",
                         "rows")

    def fold_info(self):
        """The stored kernel folded over the grid's two mirrors (csrc/fold.hip.h): on (the single-chain sweeps
        read it), reason (FOLD_REASONS), bytes of the folded store, largest deviation of an entry from its orbit's
        mean relative to the orbit's largest entry, milliseconds of its build.  The diagonal reflection on top of
        them: pair_on (a sweep reads one block per pair of orbits), pair_reason (FOLD_PAIR_REASONS), pairs and
        single_orbits (the sweep's work items), bytes_per_sweep (what a sweep reads of the store)."""
        on, rs, sb, md, bm = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        self._chk(self._lib.gh_fold_info(self._h, C.byref(on), C.byref(rs), C.byref(sb), C.byref(md), C.byref(bm)))
        pon, prs, npr, nsg, bps = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_fold_pair_info(self._h, C.byref(pon), C.byref(prs), C.byref(npr), C.byref(nsg),
                                              C.byref(bps)))
        return {"on": bool(on.value), "reason": self.FOLD_REASONS[rs.value], "store_bytes": sb.value,
                "max_dev": md.value, "build_ms": bm.value, "pair_on": bool(pon.value),
                "pair_reason": self.FOLD_PAIR_REASONS[prs.value], "pairs": npr.value, "single_orbits": nsg.value,
                "bytes_per_sweep": bps.value}

    def matrix_free_stats(self):
        """Entries / GLQ leaves evaluated and launches of the fused matrix-free pass since
        profile_enable(True)."""
        e, l, n, ne, nl = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_matrix_free_stats(self._h, C.byref(e), C.byref(l), C.byref(n), C.byref(ne),
                                                 C.byref(nl)))
        return {"entries": e.value, "leaves": l.value, "launches": n.value,
                "near_entries": ne.value, "near_leaves": nl.value}

    def build_G(self):
        self._chk(self._lib.gh_build_G(self._h))

    def kernel_stats(self):
        w, l = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_kernel_stats(self._h, C.byref(w), C.byref(l)))
        return {"warn_cells": w.value, "leaves": l.value}

    def upload_G(self, A):
        A = np.asarray(A, dtype=np.float64)
        if A.shape != (self.N, self.M):
            raise ValueError("kernel must be N x M")
        if A.flags.f_contiguous:
            self._chk(self._lib.gh_upload_G(self._h, ptr(A), self.N, 1))
        else:
            A = np.ascontiguousarray(A)
            self._chk(self._lib.gh_upload_G(self._h, ptr(A), self.M, 0))

    def download_G(self):
        """The stored kernel, N x M, Fortran-ordered; a joint context's store H = [Aw_gz | Aw_tf] is N/2 x M."""
        rows = self.N // 2 if self.joint else self.N
        A = np.empty((self.M, rows))
        self._chk(self._lib.gh_download_G(self._h, ptr(A), rows))
        return A.T  # rows x M, Fortran-ordered view

    def joint_layout(self):
        """Sweep workgroups per block and epilogue stages of a joint context (gh_joint_layout)."""
        wg, st = C.c_int(0), C.c_int(0)
        self._chk(self._lib.gh_joint_layout(self._h, C.byref(wg), C.byref(st)))
        return {"workgroups_per_block": wg.value, "epilogue_stages": st.value}

    def set_cross_gradient(self, lam, shape, hx, hy, hz, scale=(1.0, 1.0)):
        """Cross-gradient coupling lam * sum |grad u x grad w|^2 of a weighted joint context (gh_set_cross_gradient):
        shape = (nz, ny, nx) of one property's mesh, hx, hy and hz (nz - 1 centre distances) the spacings as given,
        scale = (s_rho, s_kappa) the normalisers of the two physical models.  lam = 0 switches the term off."""
        shape = [int(v) for v in shape]
        if len(shape) != 3:
            raise ValueError("shape must be (nz, ny, nx)")
        hz = np.atleast_1d(f64(hz))
        if hz.shape != (max(shape[0] - 1, 0),):
            raise ValueError("hz must have nz - 1 = %d entries, got shape %r" % (shape[0] - 1, hz.shape))
        scale = f64(scale)
        if scale.shape != (2,):
            raise ValueError("scale must be (s_rho, s_kappa)")
        if hz.size == 0:
            hz = np.ones(1)   # (an extent of 1 is refused by the library; it still wants an address)
        self._chk(self._lib.gh_set_cross_gradient(self._h, float(lam), ptr(scale), (C.c_int * 3)(*shape), float(hx),
                                                  float(hy), ptr(hz)))
        self._chain_valid = False

    def cross_gradient_eval(self, mw, want_grad=True, want_t=True):
        """(Phi, dPhi/dmw or None, t as (M/2, 3) or None) of the cross-gradient term alone, lam = 1, with the geometry
        of the last set_cross_gradient (gh_cross_gradient_eval)."""
        mw = self._vecM(mw, "mw")
        val = C.c_double(0)
        grad = np.empty(self.M) if want_grad else None
        t = np.empty((self.M // 2, 3)) if want_t else None
        self._chk(self._lib.gh_cross_gradient_eval(self._h, ptr(mw), C.byref(val), ptr(grad), ptr(t)))
        return val.value, grad, t

    def cross_gradient_last(self):
        """Phi of the last misfit_and_grad, or of the state the chain is in (gh_cross_gradient_last); 0 while off."""
        val = C.c_double(0)
        self._chk(self._lib.gh_cross_gradient_last(self._h, C.byref(val)))
        return val.value

    def sweep_layout(self):
        """Instantiation and column partition of the dense fused sweep (gh_sweep_layout): team width tw, ept2
        (double2 per thread), pf, nt, n_teams, cols_per_team, grid and n_panels."""
        i = [C.c_int(0) for _ in range(7)]
        cpt = C.c_int64(0)
        self._chk(self._lib.gh_sweep_layout(self._h, C.byref(i[0]), C.byref(i[1]), C.byref(i[2]), C.byref(i[3]),
                                            C.byref(i[4]), C.byref(cpt), C.byref(i[5]), C.byref(i[6])))
        return {"tw": i[0].value, "ept2": i[1].value, "pf": i[2].value, "nt": i[3].value, "n_teams": i[4].value,
                "cols_per_team": cpt.value, "grid": i[5].value, "n_panels": i[6].value}

    def joint_std(self):
        """(std_gz, std_tf): population std of the unweighted blocks of a weighted joint context (gh_joint_std)."""
        out = np.empty(2)
        self._chk(self._lib.gh_joint_std(self._h, ptr(out)))
        return float(out[0]), float(out[1])

    def weight(self, weightfactor=0.5):
        wm = np.empty(self.M)
        self._chk(self._lib.gh_weight(self._h, float(weightfactor), ptr(wm)))
        return wm

    # -- potential ----------------------------------------------------------------
    def set_data(self, dobs, grav_fix=None):
        dobs = f64(dobs)
        if dobs.shape != (self.N,):
            raise ValueError("dobs must have N entries")
        gf = f64(grav_fix) if grav_fix is not None else None
        self._chk(self._lib.gh_set_data(self._h, ptr(dobs), ptr(gf)))

    def set_reg(self, regularization, alpha, beta, shape, mwapr):
        if regularization not in _lib.REG_KINDS:
            raise ValueError("Please choose regularization from 'MS','Damping', 'Smoothness', 'TV'.")
        mwapr = f64(mwapr)
        if mwapr.shape != (self.M,):
            raise ValueError("mwapr must have M entries")
        shp = (C.c_int * 3)(*[int(s) for s in shape]) if shape is not None else None
        self._chk(self._lib.gh_set_reg(self._h, _lib.REG_KINDS[regularization], float(alpha),
                                       float(beta), shp, ptr(mwapr)))
        self._chain_valid = False
        self._reg_key = None   # (GravMagModule._use_reg records what it sent after this call)

    def forward(self, mw):
        mw = self._vecM(mw, "mw")
        d = np.empty(self.N)
        self._chk(self._lib.gh_forward(self._h, ptr(mw), ptr(d)))
        return d

    def adjoint(self, r):
        r = self._vecN(r, "r")
        g = np.empty(self.M)
        self._chk(self._lib.gh_adjoint(self._h, ptr(r), ptr(g)))
        return g

    def misfit_and_grad(self, x):
        x = self._vecM(x, "x")
        out3, grad, dpre = np.empty(3), np.empty(self.M), np.empty(self.N)
        self._chk(self._lib.gh_misfit_and_grad(self._h, ptr(x), ptr(out3), ptr(grad), ptr(dpre)))
        return out3[0], grad, dpre, out3[1], out3[2]

    def reg_eval(self, regularization, mw, mwapr, beta=0.01, shape=None, ms_grad_den_mw=False,
                 want_grad=True):
        """(value, grad) of one regulariser alone (alpha = 1)."""
        if regularization not in _lib.REG_KINDS:
            raise ValueError("Please choose regularization from 'MS','Damping', 'Smoothness', 'TV'.")
        mw, mwapr = self._vecM(mw, "mw"), self._vecM(mwapr, "mwapr")
        shp = (C.c_int * 3)(*[int(s) for s in shape]) if shape is not None else None
        val = C.c_double(0)
        grad = np.empty(self.M) if want_grad else None
        self._chk(self._lib.gh_reg_eval(self._h, _lib.REG_KINDS[regularization], float(beta), shp,
                                        1 if ms_grad_den_mw else 0, ptr(mw), ptr(mwapr),
                                        C.byref(val), ptr(grad)))
        return val.value, grad

    # -- wavelet-compressed forward -----------------------------------------------
    def compress_wavelet(self, dims, shape=None, thr=1e-3, levels=2):
        shp = (C.c_int * 3)(*[int(v) for v in shape]) if shape is not None else None
        nnz, ncols = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_compress_wavelet(self._h, int(dims), shp, float(thr), int(levels),
                                                C.byref(nnz), C.byref(ncols)))
        self.wavelet_nnz, self.wavelet_ncols = nnz.value, ncols.value
        return nnz.value, ncols.value

    def download_csr(self):
        from scipy.sparse import csr_matrix
        indptr = np.empty(self.N + 1, dtype=np.int64)
        indices = np.empty(max(self.wavelet_nnz, 1), dtype=np.int32)
        data = np.empty(max(self.wavelet_nnz, 1))
        self._chk(self._lib.gh_download_csr(self._h, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                            indices.ctypes.data_as(C.POINTER(C.c_int32)), ptr(data)))
        n = self.wavelet_nnz
        return csr_matrix((data[:n], indices[:n], indptr), shape=(self.N, self.wavelet_ncols))

    def model_coeffs(self, mw):
        mw = self._vecM(mw, "mw")
        out = np.empty(self.wavelet_ncols)
        self._chk(self._lib.gh_model_coeffs(self._h, ptr(mw), ptr(out)))
        return out

    def forward_wavelet(self, mw):
        mw = self._vecM(mw, "mw")
        d = np.empty(self.N)
        self._chk(self._lib.gh_forward_wavelet(self._h, ptr(mw), ptr(d)))
        return d

    # -- chain --------------------------------------------------------------------
    def chain_init(self, x0, low, high):
        x0, low, high = self._vecM(x0, "x0"), self._vecM(low, "low"), self._vecM(high, "high")
        self._chk(self._lib.gh_chain_init(self._h, ptr(x0), ptr(low), ptr(high)))
        self._chain_valid = True

    def chain_trajectory(self, p0, dt, L, u):
        p0 = self._vecM(p0, "p0")
        acc = C.c_int(0)
        out5 = np.empty(5)
        self._chk(self._lib.gh_chain_trajectory(self._h, ptr(p0), float(dt), int(L), float(u),
                                                C.byref(acc), ptr(out5)))
        return bool(acc.value), out5

    def chain_prefetch_momentum(self, p0_next):
        p0_next = self._vecM(p0_next, "p0_next")
        self._chk(self._lib.gh_chain_prefetch_momentum(self._h, ptr(p0_next)))

    def chain_stats(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_chain_stats(self._h, C.byref(a), C.byref(b)))
        la, ev = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_chain_resident_stats(self._h, C.byref(la), C.byref(ev)))
        q, tl, to, late = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int64(0)
        self._chk(self._lib.gh_team_sweep_stats(self._h, C.byref(q), C.byref(tl), C.byref(to), C.byref(late)))
        rb = self.batch_resident_stats()
        return {"spec_hits": a.value, "spec_misses": b.value,
                "resident_launches": la.value, "resident_evaluations": ev.value + rb["lock_steps"],
                "resident_batch_launches": rb["launches"], "resident_batch_lock_steps": rb["lock_steps"],
                "team_members": q.value, "team_launches": tl.value, "team_timeouts": to.value,
                "team_late_parts": late.value}

    TEAM_REFUSALS = (None, "switch off", "matrix-free / joint", "single panel", "Q > 8", "too few CUs", "tpx < 1", "LDS",
                     "residency")

    def team_info(self):
        """What the team sweep (csrc/teamsweep.hip.h) and the row panels would do with this problem as it stands
        (gh_team_sweep_plan; read-only, callable before the first sweep): `on`, `refusal` (None or one of
        TEAM_REFUSALS), the team's figures (0 past the refusal) and the row panels'."""
        out = (C.c_int32 * 16)()
        self._chk(self._lib.gh_team_sweep_plan(self._h, out))
        names = ("on", "refusal", "Q", "panel_rows", "last_rows", "tpx", "n_teams", "cols_per_team", "grid", "lag",
                 "lds_bytes", "n_panels", "rows_per_panel", "last_panel_rows")
        d = dict(zip(names, (int(v) for v in out)))
        d["on"] = bool(d["on"])
        d["refusal"] = self.TEAM_REFUSALS[d["refusal"]]
        return d

    def resident_info(self, chains=1):
        """What the resident kernels would do with this problem (gh_chain_resident_plan; read-only): the partition
        of csrc/resident.hip.h, its LDS request for `chains` chains, and whether `chains` chains would run in
        lock-step (csrc/resbatch.hip.h).  Needs the kernel, set_data and set_reg."""
        out = (C.c_int32 * 16)()
        self._chk(self._lib.gh_chain_resident_plan(self._h, int(chains), out))
        names = ("usable", "cpw", "nwg", "rc", "ct", "split", "stream", "lds_cols", "lds_bytes", "lds_max", "lockstep",
                 "ks", "nt", "lockstep_lds_bytes", "planned")
        d = dict(zip(names, (int(v) for v in out)))
        for k in ("usable", "split", "stream", "lockstep", "planned"):
            d[k] = bool(d[k])
        return d

    def _prepare_batch(self, blk, look, want_x):
        """Arguments of one gh_chain_run call over a block (Ls, p0s[K, M], us) of trajectories,
        marshalled on the calling thread (the 4 MB per momentum of C2 are copied here, not between
        two batches on the GPU).  `look`: the block whose first row is the next trajectory."""
        Ls, p0s, us = blk
        K = len(Ls)
        p0s = self._loc_rows(p0s)
        if p0s.shape != (K, self.M):
            raise ValueError("p0 must have M = %d entries, got shape %r" % (self.M, p0s.shape[1:]))
        return {"K": K, "Ls": np.ascontiguousarray(Ls, dtype=np.int32), "p0s": p0s,
                "us": np.ascontiguousarray(us, dtype=np.float64),
                "look": self._loc_rows(look[1][:1])[0] if look is not None else None,
                "acc": (C.c_int * K)(), "out5": np.empty((K, 5)),
                "xs": np.empty((K, self.M)) if want_x else None, "n_run": C.c_int(0)}

    def _run_batch(self, a, dt, stop_at, record_from, want_x, entered=None):
        """One gh_chain_run call over a prepared block; returns the number of trajectories run.
        `entered` (threading.Event) is set right before the library call (which releases the GIL)."""
        if entered is not None:
            entered.set()
        self._chk(self._lib.gh_chain_run(self._h, a["K"], a["Ls"].ctypes.data_as(C.POINTER(C.c_int)),
                                         ptr(a["p0s"]), ptr(a["us"]), float(dt),
                                         ptr(a["look"]), int(stop_at), int(record_from), a["acc"],
                                         ptr(a["out5"]), ptr(a["xs"]), C.byref(a["n_run"])))
        return a["n_run"].value   # results: a["acc"], a["out5"], a["xs"] (first n_run rows)

    def default_batch(self):
        """Trajectories per gh_chain_run call: enough to hide the per-call cost (Python round trip:
        ~0.5 ms of idle GPU per call at C2; momentum upload; for small problems the launch of the
        resident chain kernel), few enough that the host draw of the next batch still overlaps the
        GPU (C2: 4, C1: 128)."""
        if getattr(self, "_shift_invariant", False):
            # (the shift-invariant store's passes take tens of microseconds: a call's fixed costs -- two extra evaluations
            # of the persistent launch, the staging of the momenta -- want more trajectories to spread over)
            return int(max(4, min(128, (24 << 20) // (8 * max(1, self.M)))))
        return int(max(4, min(128, (6 << 20) // (8 * max(1, self.M)))))

    def _vec_any(self, v):
        """One momentum as a caller hands it over (full length; a sharded engine slices it later)."""
        v = f64(v)
        if v.ndim != 1:
            raise ValueError("p0 must be a vector, got shape %r" % (v.shape,))
        return v

    def _loc_rows(self, p0s):
        """This engine's columns of a block of momenta, contiguous float64 [K, M]."""
        return np.ascontiguousarray(p0s, dtype=np.float64)

    def _full_vec(self, v):
        return v

    def run_chain(self, draws, dt, on_result, stop_at_accepts=0, record_from=0, want_x=False,
                  batch=None, overlap=False):
        """Pipelined trajectories: `draws` yields (L, p0, u) in RNG-stream order.  Batches of
        trajectories run inside one library call (gh_chain_run: momentum of trajectory k+1
        announced before trajectory k, so an accepted proposal's last sweep already takes the
        next first step; small dense problems: one launch of the resident chain kernel per batch)
        while the next batch is drawn on the host.
        `on_result(L, accepted, out5, x)` is called per finished trajectory (x = chain state after
        an accepted trajectory if want_x, else None) and may return False to stop.
        overlap=True hands a finished batch to `on_result` while the next one already runs (the
        device never waits for Python's bookkeeping or file output); a stop requested by
        `on_result` -- as opposed to `stop_at_accepts`, which the library itself honours, or the
        end of `draws` -- then takes effect one batch late.
        One chain on the sweep launches, fed from a LegacyDraws with overlap=True and the default batch, runs on the
        library's trajectory feeder instead (_run_chain_feed): same stream, same results, no Python between two
        trajectories.  Generators, GRAVHMC_HOST_RNG=numpy, sharded engines, the persistent launches, an explicit
        `batch`, overlap=False and GRAVHMC_CHAIN_FEED=0 keep the loop below."""
        import threading
        if batch is None and overlap and type(self) is Engine and self._feed_usable(draws):
            return self._run_chain_feed(draws, dt, on_result, stop_at_accepts, record_from, want_x)
        if batch is None:
            batch = self.default_batch()
        # The momenta of a batch are drawn / gathered into page-locked blocks of the library (three of them in
        # rotation: the batch that runs, the one being drawn, one spare): the library sends them to the GPU from there
        # -- a copy from ordinary memory goes through a staging buffer first, 23 MB per call at 72 000 cells.
        # (kept with the engine between calls: page-locking tens of MB costs milliseconds)
        pool = self.__dict__.setdefault("_p0_pool", {"i": 0, "blocks": []})

        def p0_block(n, width):
            if n * width * 8 * 3 > (2 << 30) or n < 2:
                return np.empty((n, width))
            if not pool["blocks"] or pool["blocks"][0].shape[1] != width or pool["blocks"][0].shape[0] < n:
                for b in pool["blocks"]:
                    self.pinned_free(b)
                pool["blocks"] = [self.pinned_empty((max(n, batch), width)) for _ in range(3)]
            pool["i"] = (pool["i"] + 1) % 3
            return pool["blocks"][pool["i"]][:n]

        if hasattr(draws, "take_block"):
            # a source that fills blocks itself (inversion.rng.LegacyDraws): rows after the lookahead
            # are drawn straight into the batch's arrays
            def take(n, head=None):
                if head is None:
                    if n < 2:
                        return draws.take_block(n)
                    out = (np.empty(n, dtype=np.int32), p0_block(n, draws.M), np.empty(n))
                    got = len(draws.take_block(n, out=out, at=0)[0])
                    return tuple(o[:got] for o in out)
                out = (np.empty(n, dtype=np.int32), p0_block(n, head[1].shape[1]), np.empty(n))
                out[0][0], out[1][0], out[2][0] = head[0][0], head[1][0], head[2][0]
                got = len(draws.take_block(n - 1, out=out, at=1)[0]) if n > 1 else 0
                return tuple(o[:1 + got] for o in out)
        else:
            it = iter(draws)

            def take(n, head=None):
                rows = []
                for _ in range(n - (0 if head is None else 1)):
                    d = next(it, None)
                    if d is None:
                        break
                    rows.append(d)
                Ls = [int(head[0][0])] if head is not None else []
                ps = [head[1][0]] if head is not None else []
                us = [float(head[2][0])] if head is not None else []
                Ls += [int(d[0]) for d in rows]
                ps += [self._vec_any(d[1]) for d in rows]
                us += [float(d[2]) for d in rows]
                if not Ls:
                    return (np.empty(0, dtype=np.int32), np.empty((0, 0)), np.empty(0))
                blk = p0_block(len(ps), ps[0].shape[0])
                for i, pv in enumerate(ps):
                    blk[i] = pv
                return (np.asarray(Ls, dtype=np.int32), blk, np.asarray(us, dtype=np.float64))

        # one worker thread for the whole chain takes the library calls (a thread per call costs
        # ~0.1 ms of idle device between two batches of a small problem)
        import queue
        jobs = queue.Queue()

        def worker():
            while True:
                item = jobs.get()
                if item is None:
                    return
                prepared, res, entered, done = item
                try:
                    res["n"] = self._run_batch(prepared, dt, stop_at_accepts, record_from, want_x, entered)
                except BaseException as e:  # re-raised in the caller's thread
                    res["e"] = e
                finally:
                    entered.set()
                    done.set()

        th = threading.Thread(target=worker, daemon=True)
        th.start()

        def start(prepared):
            res = {"a": prepared}
            entered, done = threading.Event(), threading.Event()
            jobs.put((prepared, res, entered, done))
            # the GPU has its work before this thread goes back to drawing (np.random's generator
            # holds the GIL for the ~10 ms a C2 momentum takes)
            entered.wait()
            return done, res

        def finish(job):
            job[0].wait()
            if "e" in job[1]:
                raise job[1]["e"]
            return job[1]["n"], job[1]["a"]

        def some(blk):
            return blk is not None and len(blk[0]) > 0

        try:
            # a momentum of >= 1 MB takes milliseconds to draw: the first call then carries ONE
            # trajectory, so the device starts after two draws instead of batch + 1
            cur = take(1 if self.M * 8 >= (1 << 20) else batch)
            look = take(1) if some(cur) else None
            look = look if some(look) else None
            job = start(self._prepare_batch(cur, look, want_x)) if some(cur) else None
            while some(cur):
                # the lookahead trajectory opens the next batch; the rest is drawn and marshalled
                # while the GPU runs
                nxt = take(batch, head=look) if look is not None else None
                nlook = take(1) if some(nxt) else None
                nlook = nlook if some(nlook) else None
                nprepared = self._prepare_batch(nxt, nlook, want_x) if some(nxt) else None
                n_run, a = finish(job)
                short = n_run < len(cur[0])               # the library stopped at stop_at_accepts
                job = start(nprepared) if (overlap and some(nxt) and not short) else None
                stop = False
                acc, out5, xs = a["acc"], a["out5"], a["xs"]
                for k in range(n_run):
                    x = xs[k].copy() if (want_x and acc[k]) else None
                    if on_result(int(cur[0][k]), bool(acc[k]), out5[k],
                                 self._full_vec(x) if x is not None else None) is False:
                        stop = True
                        break
                if stop or short or not some(nxt):
                    if job is not None:
                        finish(job)
                    break
                if job is None:
                    job = start(nprepared)
                cur, look = nxt, nlook
        finally:
            jobs.put(None)
            th.join()

    def _feed_usable(self, draws):
        from .inversion.rng import LegacyDraws
        if not isinstance(draws, LegacyDraws):
            return False
        usable = C.c_int(0)
        self._chk(self._lib.gh_chain_feed_usable(self._h, C.byref(usable)))
        return bool(usable.value)

    def _run_chain_feed(self, draws, dt, on_result, stop_at_accepts, record_from, want_x):
        """run_chain on the library's feeder (gh_chain_feed_*): a drawer and a runner thread of the library take the
        stream from `draws`' generator and run the chain; this thread only hands the results to `on_result`, in
        order.  A stop asked for by `on_result` ends the chain after the trajectory in flight."""
        import sys
        lib = self._lib
        K = 4 if (want_x and self.M * 8 >= (1 << 20)) else 16
        Ls, acc = (C.c_int * K)(), (C.c_int * K)()
        out5 = np.empty((K, 5))
        xs = np.empty((K, self.M)) if want_x else None
        n, fin = C.c_int(0), C.c_int(0)
        self._chk(lib.gh_chain_feed_open(self._h, *draws.feed_args(), float(dt), int(stop_at_accepts), int(record_from),
                                         1 if want_x else 0))
        try:
            stop = False
            while not stop and not fin.value:
                # (a bounded wait: the interpreter sees its signals between two calls)
                self._chk(lib.gh_chain_feed_next(self._h, K, 200, Ls, acc, ptr(out5), ptr(xs), C.byref(n), C.byref(fin)))
                for k in range(n.value):
                    x = xs[k].copy() if (want_x and acc[k]) else None
                    if on_result(int(Ls[k]), bool(acc[k]), out5[k].copy(), x) is False:
                        stop = True
                        break
        finally:
            drawn, run = C.c_int64(0), C.c_int64(0)
            rc = lib.gh_chain_feed_close(self._h, C.byref(drawn), C.byref(run))
            draws.feed_drew(drawn.value)
            self._feed_last = {"drawn": drawn.value, "run": run.value}
            if rc != 0 and sys.exc_info()[0] is None:
                self._chk(rc)

    def feed_stats(self):
        """Counters of the trajectory feeder (gh_chain_feed_stats; of the open one, else of the last): seconds the
        runner waited for a draw, the drawer for a free row, the runner for the result queue; the rows of the ring;
        trajectories drawn and run by the last feeder."""
        a, b, c_, rows = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int(0)
        self._chk(self._lib.gh_chain_feed_stats(self._h, C.byref(a), C.byref(b), C.byref(c_), C.byref(rows)))
        last = getattr(self, "_feed_last", {"drawn": 0, "run": 0})
        return {"runner_wait_draw_s": a.value, "drawer_wait_row_s": b.value, "runner_wait_queue_s": c_.value,
                "rows": rows.value, "drawn": last["drawn"], "run": last["run"]}

    def chain_get_x(self):
        x = np.empty(self.M)
        self._chk(self._lib.gh_chain_get_x(self._h, ptr(x)))
        return x

    def chain_get_dsyn(self):
        d = np.empty(self.N)
        self._chk(self._lib.gh_chain_get_dsyn(self._h, ptr(d)))
        return d

    # -- several chains per GPU (MFMA) ----------------------------------------------
    def batch_init(self, x0s, low, high):
        x0s = np.ascontiguousarray(np.atleast_2d(x0s), dtype=np.float64)
        if x0s.ndim != 2 or x0s.shape[1] != self.M:
            raise ValueError("x0s must be (C, M)")
        self._batch_C = x0s.shape[0]
        low, high = self._vecM(low, "low"), self._vecM(high, "high")
        self._chk(self._lib.gh_batch_init(self._h, self._batch_C, ptr(x0s), ptr(low), ptr(high)))

    def batch_trajectory(self, p0s, dt, Ls, us):
        Cn = self._batch_C
        p0s = np.ascontiguousarray(np.atleast_2d(p0s), dtype=np.float64)
        if p0s.shape != (Cn, self.M):
            raise ValueError("p0s must be (C, M)")
        Ls_ = (C.c_int * Cn)(*[int(v) for v in Ls])
        us_ = np.ascontiguousarray(us, dtype=np.float64)
        acc = (C.c_int * Cn)()
        out5 = np.empty((Cn, 5))
        self._chk(self._lib.gh_batch_trajectory(self._h, ptr(p0s), float(dt), Ls_, ptr(us_), acc,
                                                ptr(out5)))
        return [bool(a) for a in acc], out5

    def batch_run(self, p0s, dt, Ls, us, want_x=False, carry=False, entered=None):
        """Up to T further trajectories of every chain, the chains desynchronised (gh_batch_run).
        p0s: (C, T, M) array, or C lists of T momentum vectors (not copied); Ls (C, T), us (C, T):
        the trajectories each chain has not started yet.  Returns accepted (C, S) bool, out5
        (C, S, 5), xs (C, S, M) or None -- per chain in order of completion, S = T slots, T + 1
        with carry -- and, with carry=True, (n_started, n_done): the call then ends as soon as a chain has nothing left to
        start, the others keep their trajectory in flight for the next call (T = 0, i.e. C empty
        lists, drains them).  `entered` (threading.Event) is set right before the library call, which releases the
        interpreter lock: a caller that runs this on a worker thread waits for it before it starts drawing the next
        offers on a dozen threads, so the GPU has its work first."""
        Cn = len(p0s)
        T = len(p0s[0]) if Cn else 0
        if any(len(r) != T for r in p0s):
            raise ValueError("p0s must hold the same number of M-vectors for every chain")
        if T and isinstance(p0s[0][0], (int, np.integer)):
            # row ADDRESSES (LegacyDraws.take_ring: M float64 values each, alive for the call)
            addr = np.ascontiguousarray(p0s, dtype=np.uint64).reshape(Cn * T)
            ptrs = addr.ctypes.data_as(C.POINTER(_lib._dp))
        else:
            rows = [[f64(p) for p in chain] for chain in p0s]
            if any(p.shape != (self.M,) for r in rows for p in r):
                raise ValueError("p0s must hold the same number of M-vectors for every chain")
            ptrs = (_lib._dp * max(1, Cn * T))(*[ptr(p) for r in rows for p in r])
        To = T + 1 if carry else T            # result slots per chain
        Ls = np.ascontiguousarray(Ls, dtype=np.int32).reshape(Cn, T)
        us = np.ascontiguousarray(us, dtype=np.float64).reshape(Cn, T)
        acc = np.zeros((Cn, To), dtype=np.int32)
        out5 = np.zeros((Cn, To, 5))
        xs = np.empty((Cn, To, self.M)) if want_x else None
        ns = np.zeros(Cn, dtype=np.int32)
        nd = np.zeros(Cn, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        if entered is not None:
            entered.set()
        self._chk(self._lib.gh_batch_run(self._h, int(T), ip(Ls) if T else None, ptrs if T else None,
                                         ptr(us) if T else None, float(dt), ip(acc), ptr(out5), ptr(xs),
                                         ip(ns) if carry else None, ip(nd) if carry else None))
        if carry:
            return acc.astype(bool), out5, xs, ns, nd
        return acc.astype(bool), out5, xs

    def shift_invariant_resident_stats(self):
        """The harmonic pass of the shift-invariant store as one persistent launch per run_chain call
        (csrc/lonres.hip.h): grid, launches, evaluations, trajectories, time-outs."""
        wg, t = C.c_int(0), C.c_int(0)
        l, e, tr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_shift_invariant_resident_stats(self._h, C.byref(wg), C.byref(l), C.byref(e), C.byref(tr),
                                                              C.byref(t)))
        return {"workgroups": wg.value, "launches": l.value, "evaluations": e.value, "trajectories": tr.value,
                "timeouts": t.value}

    def pinned_empty(self, shape):
        """A float64 array in page-locked host memory of the library (gh_pinned_alloc): momentum rows drawn into
        it go to the device without a gather on the host.  It lives until pinned_free(array) or close()."""
        n = int(np.prod(shape))
        p = C.c_void_p()
        self._chk(self._lib.gh_pinned_alloc(self._h, max(1, n) * 8, C.byref(p)))
        buf = (C.c_double * max(1, n)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.float64, count=n).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def pinned_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is None:
            raise ValueError("not an array of pinned_empty")
        self._chk(self._lib.gh_pinned_free(self._h, C.c_void_p(p)))

    def batch_staging_stats(self):
        """Momentum rows of the lock-step form sent straight from pinned memory / gathered on the host first."""
        d, s = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_batch_staging_stats(self._h, C.byref(d), C.byref(s)))
        return {"rows_direct": d.value, "rows_staged": s.value}

    def batch_fused_stats(self):
        """Team form of the matrix-free batch (one evaluation per entry and step): grid, launches, time-outs."""
        m, r, l, t = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(0)
        self._chk(self._lib.gh_batch_fused_stats(self._h, C.byref(m), C.byref(r), C.byref(l), C.byref(t)))
        return {"members": m.value, "ranges": r.value, "launches": l.value, "timeouts": t.value}

    def batch_resident_stats(self):
        """Chains in lock-step inside the resident batch kernel (csrc/resbatch.hip.h): launches, lock-steps,
        evaluations of all chains, lock-steps lost to rejected speculative first steps, time-outs."""
        l, s, cs, lo, t = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        self._chk(self._lib.gh_batch_resident_stats(self._h, C.byref(l), C.byref(s), C.byref(cs), C.byref(lo),
                                                    C.byref(t)))
        return {"launches": l.value, "lock_steps": s.value, "chain_steps": cs.value, "lost_steps": lo.value,
                "timeouts": t.value}

    def matrix_free_team_stats(self):
        """Team form of the single-chain matrix-free pass: grid, launches, time-outs."""
        m, r, l, t = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(0)
        self._chk(self._lib.gh_matrix_free_team_stats(self._h, C.byref(m), C.byref(r), C.byref(l), C.byref(t)))
        return {"members": m.value, "ranges": r.value, "launches": l.value, "timeouts": t.value}

    def batch_get_x(self, chain):
        x = np.empty(self.M)
        self._chk(self._lib.gh_batch_get_x(self._h, int(chain), ptr(x)))
        return x

    # -- bootstrap replicates of the CG inversion in lock-step -------------------------
    def batch_block_means(self):
        """The means of the row blocks of the chains' current weighted predictions, (C, blocks), as the batch's
        evaluation removes them (gh_batch_block_means): a batch on set_cells_multi(..., translation_invariant="chains")."""
        out = np.zeros((16, max(self._store.rows, 1)))
        self._chk(self._lib.gh_batch_block_means(self._h, ptr(out)))
        return out[:self._batch_C].copy()

    def bscg_run(self, counts, dobs, mw0, rhomin, rhomax, beta2, q, maxk):
        """Up to 16 replicates of BootStrap.CG on one read of G per product (csrc/bscg.hip.h).  counts: (B, N) draw
        counts; dobs: N; mw0: the weighted start model.  Returns the unweighted models (B, M), the data and model
        misfit rows (B, maxk - 1), the regularisation factors (B, maxk) and how many entries of each are valid."""
        counts = np.atleast_2d(f64(counts))
        B = int(counts.shape[0])
        if counts.shape[1] != self.N:
            raise ValueError("bscg_run: counts must have shape (B, N = %d)" % self.N)
        dobs, mw0 = f64(dobs), f64(mw0)
        if dobs.shape != (self.N,) or mw0.shape != (self.M,):
            raise ValueError("bscg_run: dobs must have N = %d entries and mw0 M = %d" % (self.N, self.M))
        maxk = int(maxk)
        rows, e = max(B, 1), max(maxk - 1, 1)
        models = np.zeros((rows, self.M))
        dmis, mmis, alpha = np.zeros((rows, e)), np.zeros((rows, e)), np.zeros((rows, max(maxk, 1)))
        n_entries, n_alpha = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self._chk(self._lib.gh_bscg_run(self._h, B, ptr(counts), ptr(dobs), ptr(mw0), float(rhomin), float(rhomax),
                                        float(beta2), float(q), maxk, ptr(models), ptr(dmis), ptr(mmis), ptr(alpha),
                                        n_entries.ctypes.data_as(ip), n_alpha.ctypes.data_as(ip)))
        return models, dmis, mmis, alpha, n_entries, n_alpha

    def bscg_stats(self):
        """Sweeps of G and lock-steps of the last bscg_run group: 2 maxk + 1 forward, maxk adjoint, whatever B."""
        f, a, s = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_bscg_stats(self._h, C.byref(f), C.byref(a), C.byref(s)))
        return {"forward_sweeps": f.value, "adjoint_sweeps": a.value, "lock_steps": s.value}

    # -- posterior window ---------------------------------------------------------
    def posterior_window(self, K=100):
        self._chk(self._lib.gh_posterior_window(self._h, int(K)))
        self._has_window = True

    def posterior_add(self):
        self._chk(self._lib.gh_posterior_add(self._h))

    def posterior_read(self, want_arrays=True):
        n, tot = C.c_int64(0), C.c_int64(0)
        mean = np.empty(self.M) if want_arrays else None
        sd = np.empty(self.M) if want_arrays else None
        self._chk(self._lib.gh_posterior_read(self._h, C.byref(n), C.byref(tot), ptr(mean), ptr(sd)))
        return {"n": n.value, "total": tot.value, "mean": mean, "std": sd}

    # -- streaming posterior --------------------------------------------------------
    def posterior_stream(self, chains, bins=64, batch_len=10, record_from=0, record_count=2 ** 62, lo=None, hi=None):
        """Running statistics of whole runs of up to 16 chains on the device (gh_posterior_stream): per chain slot
        mean / M2 and batch means of `batch_len` samples, one pooled histogram of `bins` bins over [lo, hi] per
        cell (unweighted model bounds: scalars or M-vectors).  Chain slot c records its accepted states number
        record_from + 1 ... record_from + record_count.  Before or after weight(): the stream follows the weights the engine
        has when a state is recorded."""
        chains, bins, batch_len = int(chains), int(bins), int(batch_len)
        if not 1 <= chains <= 16:
            raise ValueError("posterior_stream: chains must be 1..16")
        if not 2 <= bins <= 256:
            raise ValueError("posterior_stream: bins must be 2..256")
        if batch_len < 1:
            raise ValueError("posterior_stream: batch_len must be >= 1")
        if int(record_from) < 0 or int(record_count) < 0:
            raise ValueError("posterior_stream: record_from and record_count must be >= 0")
        if lo is None or hi is None:
            raise ValueError("posterior_stream: needs the model bounds lo and hi of the histogram")
        lo = f64(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.M,)))
        hi = f64(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.M,)))
        if not np.all(hi >= lo):
            raise ValueError("posterior_stream: hi < lo at cell %d" % int(np.argmin(hi >= lo)))
        self._chk(self._lib.gh_posterior_stream(self._h, chains, bins, batch_len, int(record_from), int(record_count),
                                                ptr(lo), ptr(hi)))
        self._stream = (chains, bins)

    def posterior_stream_slot(self, slot):
        """The chain slot the single-chain paths (run_chain, posterior_add) feed from here on."""
        self._chk(self._lib.gh_posterior_stream_slot(self._h, int(slot)))

    def posterior_stream_add(self, slot, m):
        """One explicit UNWEIGHTED model row into chain slot `slot`."""
        self._chk(self._lib.gh_posterior_stream_add(self._h, int(slot), ptr(self._vecM(m, "m"))))

    def _stream_shape(self):
        st = getattr(self, "_stream", None)
        if st is None:
            raise ValueError("no posterior stream: call posterior_stream first")
        return st

    def posterior_stream_read(self):
        """n_per_chain (chains), pooled mean / std / rhat / ess (M each), chain_mean / chain_M2 (chains, M)."""
        chains, _ = self._stream_shape()
        n = np.zeros(chains, dtype=np.int64)
        out = {k: np.empty(self.M) for k in ("mean", "std", "rhat", "ess")}
        cm, cq = np.empty((chains, self.M)), np.empty((chains, self.M))
        self._chk(self._lib.gh_posterior_stream_read(self._h, n.ctypes.data_as(C.POINTER(C.c_int64)), ptr(out["mean"]),
                                                     ptr(out["std"]), ptr(out["rhat"]), ptr(out["ess"]), ptr(cm), ptr(cq)))
        out.update(n_per_chain=n, chain_mean=cm, chain_M2=cq)
        return out

    def posterior_stream_quantiles(self, q):
        """Quantiles q (each in [0, 1]) per cell from the pooled histogram: (len(q), M)."""
        self._stream_shape()
        q = f64(np.atleast_1d(q))
        if q.ndim != 1 or not 1 <= q.size <= 32 or not np.all((q >= 0) & (q <= 1)):
            raise ValueError("posterior_stream_quantiles: 1..32 quantiles in [0, 1]")
        out = np.empty((q.size, self.M))
        self._chk(self._lib.gh_posterior_stream_quantiles(self._h, int(q.size), ptr(q), ptr(out)))
        return out

    def posterior_stream_hist(self):
        """The pooled histogram counts, (bins, M) uint32."""
        _, bins = self._stream_shape()
        out = np.empty((bins, self.M), dtype=np.uint32)
        self._chk(self._lib.gh_posterior_stream_hist(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def posterior_stream_free(self):
        self._chk(self._lib.gh_posterior_stream_free(self._h))
        self._stream = None

    def leapfrog(self, x, p0, dt, L, low, high, u, want_dsyn=True):
        x = self._vecM(x, "x").copy()
        p0, low, high = self._vecM(p0, "p0"), self._vecM(low, "low"), self._vecM(high, "high")
        acc = C.c_int(0)
        out5 = np.empty(5)
        dsyn = np.empty(self.N) if want_dsyn else None
        self._chk(self._lib.gh_leapfrog(self._h, ptr(x), ptr(p0), float(dt), int(L), ptr(low),
                                        ptr(high), float(u), C.byref(acc), ptr(out5), ptr(dsyn)))
        return x, bool(acc.value), out5, dsyn

    # -- measurement --------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self._lib.gh_profile_enable(self._h, 1 if on else 0))

    def stream_read_gbps(self, nt=True, reps=3):
        """Attainable streaming-read rate (GB/s) of this device over the stored kernel matrix."""
        ms = C.c_double(0)
        self._chk(self._lib.gh_measure_stream_read(self._h, 1 if nt else 0, int(reps), C.byref(ms)))
        return self.N * self.M * 8 / (ms.value * 1e-3) / 1e9

    def profile_read(self):
        ms, n, b = C.c_double(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.gh_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(b)))
        return {"sweep_ms": ms.value, "sweeps": n.value, "bytes_per_sweep": b.value}
