"""The scripted cases behind tests/golden/module_layer.json: what the six inversion modules (GravMagModule, JointModule,
MultiComponentModule, TesseroidMultiComponentModule, MagVectorModule, TesseroidMagVectorModule) and HMCSampleBatch
refuse before a device is touched, and everything a constructed module carries and answers.

TEST INFRASTRUCTURE ONLY.  tests/make_golden_module_layer.py runs the cases on the package the fixture is made from and
records them; tests/test_module_layer_host.py and tests/test_gpu_module_layer.py replay them on the package under test
and compare exactly.

A host case is (name, thunk): the thunk must raise, and the exception's class name and text are recorded.  With two
faults in one call the text tells the order of the checks.  A device case is (name, constructor thunk, options): the
module is built with verbose=True and its printed lines, warnings, attributes and SHA-256 digests are recorded.
"""
import contextlib
import hashlib
import io
import re
import warnings

import numpy as np

# ------------------------------------------------------------------------------------------------------------ host
MRANGE, MSPACING = (0, 2000, 0, 3000, 0, 900), (300, 750, 500)     # 3 x 4 x 4 cells
TRANGE, TSPACING = (-180, 180, -60, 60, 0, -200000), (-100000, 30, 30)   # 2 x 4 x 12 tesseroids, the full circle


def _line(n=6, c=2):
    """tests/test_multicomp_host.py::_args: c data vectors at n points on a line"""
    x = np.linspace(0, 2000, n)
    rng = np.random.default_rng(0)
    return [rng.normal(size=n) for _ in range(c)], (x, x.copy(), np.full(n, -30.0))


def _big(n, c):
    x = np.linspace(0, 2000, n)
    return [np.arange(n, dtype=float) + k for k in range(c)], (x, x, np.zeros(n))


class _Ranks:
    world, rank = 2, 0


def _carving():
    """a surface that dips into the 3 x 4 x 4 mesh on one side (tests/test_gpu_multicomp.py::test_carved_mesh)"""
    xs, ys = np.meshgrid(np.linspace(0, 2000, 9), np.linspace(0, 3000, 9))
    return xs.ravel(), ys.ravel(), np.where(xs.ravel() < 1000, -350.0, 100.0)


def host_cases():
    from gravinv3dhmc_amd.inversion import (GravMagModule, JointModule, MagVectorModule, MultiComponentModule,
                                            TesseroidMagVectorModule, TesseroidMultiComponentModule)
    cases = []
    d, obs = _line()

    def add(name, cls, *args, **kw):
        kw.setdefault("verbose", False)
        cases.append((name, lambda: cls(*args, **kw)))

    # ---- GravMagModule
    def gm(name, **kw):
        add("gravmag." + name, GravMagModule, d[0], MRANGE, MSPACING, obs, **kw)

    gm("field", field="electric")
    gm("coordinate", coordinate="polar")
    gm("magnetic_spherical", field="magnetic", coordinate="spherical")
    gm("component_unknown", component="gzx")
    gm("component_magnetic", component="gzz", field="magnetic")
    gm("component_spherical", component="gzz", coordinate="spherical")
    gm("wavelet", wavelet="2D")
    gm("ti.spherical", translation_invariant=True, coordinate="spherical")
    gm("ti.wavelet", translation_invariant=True, wavelet="1D")
    gm("ti.shard", translation_invariant=True, shard=_Ranks())
    gm("ti.matrix_free", translation_invariant=True, matrix_free=True)
    gm("ti.shift_invariant", translation_invariant=True, shift_invariant=True)
    gm("ti.mtopo", translation_invariant=True, mtopo=_carving())
    gm("shard_axis", shard=_Ranks(), shard_axis="diagonal")
    gm("shard_wavelet_cells", shard=_Ranks(), wavelet="1D")
    gm("shard_planes_carved", shard=_Ranks(), shard_planes=True, mtopo=_carving())
    gm("order.field_component", field="electric", component="gzx")
    gm("order.magnetic_spherical_component", field="magnetic", coordinate="spherical", component="gzx")
    gm("order.component_wavelet", component="gzx", wavelet="2D")
    gm("order.component_magnetic_wavelet", component="gzz", field="magnetic", wavelet="2D")
    gm("order.wavelet_ti_spherical", wavelet="2D", translation_invariant=True, coordinate="spherical")
    gm("order.ti_spherical_wavelet", translation_invariant=True, coordinate="spherical", wavelet="1D")
    gm("order.ti_wavelet_shard", translation_invariant=True, wavelet="1D", shard=_Ranks())
    gm("order.ti_shard_matrix_free", translation_invariant=True, shard=_Ranks(), matrix_free=True)
    gm("order.ti_matrix_free_shift_invariant", translation_invariant=True, matrix_free=True, shift_invariant=True)
    gm("order.ti_shift_invariant_mtopo", translation_invariant=True, shift_invariant=True, mtopo=_carving())
    gm("order.shard_axis_wavelet", shard=_Ranks(), shard_axis="diagonal", wavelet="1D")
    gm("order.shard_wavelet_planes", shard=_Ranks(), wavelet="1D", shard_planes=True, mtopo=_carving())

    # ---- JointModule
    def jm(name, dg=d[0], dt=d[1], **kw):
        add("joint." + name, JointModule, dg, dt, MRANGE, MSPACING, obs, **kw)

    jm("spherical", coordinate="spherical")
    jm("coordinate", coordinate="polar")
    jm("wavelet", wavelet="1D")
    jm("lengths_tf", dt=d[1][:-1])
    jm("lengths_points", dg=d[0][:-1], dt=d[1][:-1])
    jm("order.spherical_wavelet", coordinate="spherical", wavelet="1D")
    jm("order.coordinate_wavelet", coordinate="polar", wavelet="1D")
    jm("order.wavelet_lengths", wavelet="1D", dt=d[1][:-1])

    # ---- the stores of row blocks: the data parser and the ladder of refusals, on each of the four classes
    def blocks(tag, cls, word, two, three, mrange, mspacing, none_weight, ladder_extra):
        """word: the keyword of the components ("components" / "data"); two, three: valid names; ladder_extra: keywords
        the class needs to reach the ladder"""
        def mk(name, dobs=d, o=obs, comps=two, mr=mrange, **kw):
            kw[word] = comps
            add("%s.%s" % (tag, name), cls, dobs, mr, mspacing, o, **kw)

        mk("empty", dobs=[], comps=())
        mk("unknown", comps=(two[0], "gzx"))
        mk("repeated", comps=(two[1], two[1]))
        mk("dict_names", dobs={two[0]: d[0], three[2]: d[1]})
        mk("count", dobs=d[:1])
        mk("length", dobs=[d[0], d[1][:-1]])
        mk("weights_word", weights="var")
        mk("weights_std0", dobs=[d[0], np.zeros(6)], weights="std")
        for k, w in enumerate(((1.0,), (1.0, -2.0), (1.0, 0.0), (1.0, np.inf), (1.0, np.nan))):
            mk("weights_numbers%d" % k, weights=w)
        mk("keyword", topo=None)
        mk("wavelet1D", wavelet="1D")
        mk("wavelet3D", wavelet="3D")
        mk("matrix_free", matrix_free=True)
        mk("shard", shard=object())
        big, bobs = _big(8193, 2)
        mk("rows_8193x2", dobs=big, o=bobs)
        big1, bobs1 = _big(16385, 1)
        mk("rows_16385", dobs=big1, o=bobs1, comps=two[:1], weights=(1.0,))
        mk("string_component", dobs=d[:1], comps=two[0], weights="var")
        # two faults: the order of the checks
        mk("order.unknown_repeated", comps=("gzx", "gzx"))
        mk("order.unknown_length", comps=(two[0], "gzx"), dobs=[d[0], d[1][:-1]])
        mk("order.repeated_dict", comps=(two[1], two[1]), dobs={three[2]: d[0]})
        mk("order.dict_weights", dobs={two[0]: d[0], three[2]: d[1]}, weights="var")
        mk("order.count_length", dobs=[d[0][:-1]])
        mk("order.length_weights", dobs=[d[0], d[1][:-1]], weights="var")
        mk("order.weights_word_keyword", weights="var", topo=None)
        mk("order.weights_std0_wavelet", dobs=[d[0], np.zeros(6)], weights="std", wavelet="1D")
        mk("order.weights_numbers_wavelet", weights=(1.0, -2.0), wavelet="1D")
        mk("order.keyword_empty", topo=None, dobs=[], comps=())
        mk("order.keyword_wavelet", topo=None, wavelet="1D")
        mk("order.wavelet_matrix_free", wavelet="1D", matrix_free=True)
        mk("order.matrix_free_shard", matrix_free=True, shard=object())
        mk("order.shard_rows", shard=object(), dobs=big, o=bobs)
        if none_weight:
            mk("order.rows_amplitude", dobs=big, o=bobs, amplitude=-1.0)
        if not ladder_extra:     # (the prism classes take `coordinate` and refuse the shift-invariant store)
            mk("spherical", coordinate="spherical")
            mk("coordinate", coordinate="polar")
            mk("shift_invariant", shift_invariant=True)
            mk("order.weights_spherical", weights="var", coordinate="spherical")
            mk("order.spherical_wavelet", coordinate="spherical", wavelet="1D")
            mk("order.coordinate_wavelet", coordinate="polar", wavelet="1D")
            mk("order.matrix_free_shift_invariant", matrix_free=True, shift_invariant=True)
            mk("order.shift_invariant_shard", shift_invariant=True, shard=object())
        return mk

    blocks("multi", MultiComponentModule, "components", ("gz", "gzz"), ("gz", "gzz", "gxx"), MRANGE, MSPACING,
           False, False)
    mk = blocks("tess_multi", TesseroidMultiComponentModule, "components", ("gz", "gzz"), ("gz", "gzz", "gxx"),
                TRANGE, TSPACING, False, True)
    mk("ratio_count", ratio=(1.6,))
    mk("ratio_zero", ratio=0.0)
    mk("ratio_negative", ratio=(8.0, -1.0))
    mk("ratio_nan", ratio=float("nan"))
    mk("order.ratio_count_unknown", ratio=(1.6,), comps=("gz", "gzx"))
    mk("order.ratio_zero_empty", ratio=0.0, dobs=[], comps=())
    mk("order.ratio_keyword", ratio=0.0, topo=None)

    mk = blocks("magvec", MagVectorModule, "data", ("bx", "bz"), ("bx", "bz", "tf"), MRANGE, MSPACING, True, False)
    mk("tf_weights_word", dobs=d[:1], comps=("tf",), weights="var")
    mk("amplitude", amplitude=-1.0)
    mk("amplitude_beta", amplitude_beta=0.0)
    mk("order.amplitude_coordinate", amplitude=-1.0, coordinate="polar")
    mk("order.keyword_unknown", topo=None, comps=("bx", "gzx"))

    def mv(name, dobs=d[0], o=obs, **kw):   # the default form: one block of the total field, no weights
        add("magvec.default." + name, MagVectorModule, dobs, MRANGE, MSPACING, o, **kw)

    big1, bobs1 = _big(16385, 1)
    mv("keyword", topo=None)
    mv("spherical", coordinate="spherical")
    mv("coordinate", coordinate="polar")
    mv("wavelet", wavelet="1D")
    mv("matrix_free", matrix_free=True)
    mv("shift_invariant", shift_invariant=True)
    mv("shard", shard=object())
    mv("length", dobs=d[0][:-1])
    mv("rows_16385", dobs=big1[0], o=bobs1)
    mv("amplitude", amplitude=-1.0)
    mv("amplitude_nan", amplitude=float("nan"))
    mv("amplitude_beta", amplitude_beta=0.0)
    mv("order.keyword_spherical", topo=None, coordinate="spherical")
    mv("order.spherical_wavelet", coordinate="spherical", wavelet="1D")
    mv("order.wavelet_matrix_free", wavelet="1D", matrix_free=True)
    mv("order.matrix_free_shift_invariant", matrix_free=True, shift_invariant=True)
    mv("order.shift_invariant_shard", shift_invariant=True, shard=object())
    mv("order.shard_length", shard=object(), dobs=d[0][:-1])
    mv("order.length_rows", dobs=d[0], o=bobs1)
    mv("order.rows_amplitude", dobs=big1[0], o=bobs1, amplitude=-1.0)
    mv("order.length_amplitude", dobs=d[0][:-1], amplitude=-1.0)

    mk = blocks("tess_magvec", TesseroidMagVectorModule, "data", ("bx", "bz"), ("bx", "bz", "tf"), TRANGE,
                TSPACING, True, True)
    mk("ratio_zero", ratio=0.0)
    mk("ratio_negative", ratio=-8.0)
    mk("regional_table", shift_invariant=True, mr=MRANGE)
    mk("amplitude", amplitude=-1.0)
    mk("amplitude_beta", amplitude_beta=0.0)
    mk("order.ratio_regional", ratio=0.0, shift_invariant=True, mr=MRANGE)
    mk("order.ratio_keyword", ratio=0.0, topo=None)
    mk("order.keyword_unknown", topo=None, comps=("bx", "gzx"))
    # the regional mesh and the total field's direction within a class of observations (host decisions of the table)
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 180, 30.0), (-45.0, -15.0, 15.0, 45.0), indexing="ij")]
    tobs = (lon, lat, np.full(lon.size, 250000.0))
    td = [np.sin(np.arange(lon.size) + k) for k in range(2)]
    inc = np.full(lon.size, 60.0)
    inc[5] = 61.0   # (points 1, 5, 9 ... share latitude -15 and the height)

    def tm(name, mrange=TRANGE, **kw):
        add("tess_magvec." + name, TesseroidMagVectorModule, td, mrange, TSPACING, tobs, **kw)

    tm("table.regional", mrange=(-30, 30, -60, 60, 0, -200000), data=("bx", "bz"), shift_invariant=True)
    tm("table.direction_in_class", data=("tf", "bz"), mangle=(inc, 10.0), shift_invariant=True)
    tm("table.mangle_count", data=("tf", "bz"), mangle=(inc[:-1], 10.0))
    tm("order.regional_direction", mrange=(-30, 30, -60, 60, 0, -200000), data=("tf", "bz"), mangle=(inc, 10.0),
       shift_invariant=True)
    tm("order.direction_keyword", data=("tf", "bz"), mangle=(inc, 10.0), shift_invariant=True, topo=None)
    tm("order.direction_wavelet", data=("tf", "bz"), mangle=(inc, 10.0), shift_invariant=True, wavelet="1D")
    tm("order.table_matrix_free_shard", data=("bx", "bz"), shift_invariant=True, matrix_free=True, shard=object())

    # ---- HMCSampleBatch on stand-ins that carry the probed attributes alone
    from gravinv3dhmc_amd.inversion import hmc

    def batch(name, constraint="mandatory", **attrs):
        eng = type("_E", (), attrs)()
        model = type("_M", (), {"_engine": eng})()
        cases.append(("batch." + name, lambda: hmc.HMCSampleBatch(
            model, 2, 1, 0, 0.01, [1, 2], np.zeros((2, 3)), np.zeros(3), np.zeros((3, 2)), constraint, 1000,
            np.zeros(2), "Fixed", 0.8, 1.0, "Damping", 0.01, 0, 0.3)))

    batch("joint", joint=True)
    batch("tess_mag", tess_mag=True)
    batch("tess_multi", tess_multi=True)
    batch("mvi_data", multi=3, mvi=True)
    batch("multi", multi=2)
    batch("mvi", mvi=True)
    batch("translation_invariant", _translation_invariant=True)
    batch("order.constraint_joint", constraint="logarithmic", joint=True)
    batch("order.joint_tess_mag", joint=True, tess_mag=True)
    batch("order.tess_mag_tess_multi", tess_mag=True, tess_multi=True)
    batch("order.tess_multi_mvi_data", tess_multi=True, multi=3, mvi=True)
    batch("order.multi_translation_invariant", multi=2, _translation_invariant=True)
    batch("order.mvi_translation_invariant", mvi=True, _translation_invariant=True)
    batch("order.multi0_mvi", multi=0, mvi=True)
    return cases


def run_host_case(thunk):
    """'<exception class name>: <its text>'; '' if the thunk raises nothing"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            thunk()
    except Exception as ex:  # noqa: BLE001 (the class is what is recorded)
        return "%s: %s" % (type(ex).__name__, ex)
    return ""


def run_host():
    return {name: run_host_case(thunk) for name, thunk in host_cases()}


# ---------------------------------------------------------------------------------------------------------- device
PRANGE, PSPACING = (0, 2000, 0, 3000, 0, 900), (300, 750, 500)      # tests/test_gpu_multicomp.py
SEG_SPACING, SEG_SECTIONS = ([150, 300], 750, 500), [0, 300, 900]    # mseg: two layers of 150 m over two of 300 m
REGS = ("Damping", "MS", "Smoothness", "TV")
BATCH_ARGS = ("mandatory", 1000, None, "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3)


def _pobs(nx=7, ny=5):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(100, 2900, ny), np.linspace(50, 1950, nx))]
    return xp, yp, np.full(xp.size, -30.0)


def _tobs():
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 180, 30.0), (-45.0, -15.0, 15.0, 45.0), indexing="ij")]
    return lon, lat, np.full(lon.size, 250000.0)


def _dobs(n, c, seed=3):
    """c data vectors of n values in very different units, none constant"""
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=n) + 0.5 * k) * 10.0 ** k for k in range(c)]


def _lattice():
    """the smallest grid of tests/lattice_cases.py with more than one cell along every axis: 3 x 2 x 2 cells of 100 m
    under gridded data above the cell centres"""
    mrange, mspacing = (0.0, 300.0, 0.0, 200.0, 0.0, 200.0), (100.0, 100.0, 100.0)
    xp, yp = [a.ravel() for a in np.meshgrid(50.0 + 100.0 * np.arange(3), 50.0 + 100.0 * np.arange(2), indexing="ij")]
    return mrange, mspacing, (xp, yp, np.full(xp.size, -20.0))


def device_cases():
    """(name, thunk that builds the module, options).  Options: kernels: the kernel(...) argument tuples to record;
    names: attributes that are properties holding arrays; regs: the regularisers to evaluate."""
    import gravinv3dhmc_amd as G
    cases = []
    pobs, tobs = _pobs(), _tobs()
    np_, nt = pobs[0].size, tobs[0].size
    carve = _carving()

    def add(name, cls, *args, kernels=(), names=(), regs=REGS, batch=True, **kw):
        cases.append((name, lambda: cls(*args, verbose=True, **kw),
                      dict(kernels=kernels, names=names, regs=regs, batch=batch)))

    # ---- prisms
    d = _dobs(np_, 3)

    def gm(name, mspacing=PSPACING, **kw):
        add("gravmag." + name, G.GravMagModule, d[0], PRANGE, mspacing, pobs, batch=False, **kw)

    gm("gz")
    gm("gzz", component="gzz")
    gm("magnetic", field="magnetic", mangle=(60, 10))
    gm("mseg", mspacing=SEG_SPACING, mseg=True, mdivisionsection=SEG_SECTIONS)
    gm("mtopo", mtopo=carve)
    fix = np.zeros(np_)
    fix[::3] = 0.25
    gm("fixed", fixed=True, grav_fix=fix)
    gm("matrix_free", matrix_free=True)
    gm("wavelet1D", wavelet="1D")
    lrange, lspacing, lobs = _lattice()
    add("gravmag.translation_invariant", G.GravMagModule, _dobs(lobs[0].size, 1)[0], lrange, lspacing, lobs,
        translation_invariant=True)

    jk = dict(names=("kernel_gz", "kernel_tf"))
    add("joint.plain", G.JointModule, d[0], d[1], PRANGE, PSPACING, pobs, mangle=(60, 10), **jk)
    add("joint.mtopo", G.JointModule, d[0], d[1], PRANGE, PSPACING, pobs, mangle=(60, 10), mtopo=carve, **jk)
    add("joint.crossgradient", G.JointModule, d[0], d[1], PRANGE, PSPACING, pobs, mangle=(60, 10), crossgradient=0.3,
        cg_scale=(0.5, 2.0), **jk)

    def mc(name, dobs, comps, mspacing=PSPACING, **kw):
        add("multi." + name, G.MultiComponentModule, dobs, PRANGE, mspacing, pobs, components=comps,
            kernels=[(c,) for c in ((comps,) if isinstance(comps, str) else comps)] + [("gyy",)], **kw)

    mc("gz_gzz_std", d[:2], ("gz", "gzz"), weights="std")
    mc("three_weights", d, ("gzz", "gz", "gxy"), weights=(2.0, 1.0, 0.125))
    mc("dict", {"gzz": d[1], "gz": d[0]}, ("gz", "gzz"))
    mc("one", d[:1], "gzz")
    mc("mtopo", d[:2], ("gz", "gzz"), mtopo=carve)
    mc("mseg", d[:2], ("gz", "gzz"), mspacing=SEG_SPACING, mseg=True, mdivisionsection=SEG_SECTIONS)

    def mv(name, dobs, **kw):
        data = kw.get("data", ("tf",))
        data = (data,) if isinstance(data, str) else data
        vector = not (data == ("tf",) and kw.get("weights") is None)
        kernels = [(a,) for a in (0, 1, "z", 3)]
        if vector:
            kernels += [(0, b) for b in data] + [("y", "gz")]
        add("magvec." + name, G.MagVectorModule, dobs, PRANGE, PSPACING, pobs, mangle=(60, 10), kernels=kernels, **kw)

    mv("default", d[0])
    mv("tf_weight", d[:1], data=("tf",), weights=(2.0,))
    mv("tf_unit_weight", d[:1], data=("tf",), weights=(1.0,))   # (the engine keeps the magnetization-vector store)
    mv("bxyz_std", d, data=("bx", "by", "bz"), weights="std")
    mv("tf_bz", d[:2], data=("tf", "bz"))
    mv("amplitude", d[0], amplitude=0.5, amplitude_beta=0.05)
    mv("mtopo", d[0], mtopo=carve)

    # ---- tesseroids
    t = _dobs(nt, 3, seed=4)

    def tg(name, **kw):
        add("gravmag.spherical." + name, G.GravMagModule, t[0], TRANGE, TSPACING, tobs, coordinate="spherical",
            batch=False, **kw)

    tg("dense")
    tg("shift_invariant", shift_invariant=True)

    def tc(name, dobs, comps, **kw):
        add("tess_multi." + name, G.TesseroidMultiComponentModule, dobs, TRANGE, TSPACING, tobs, components=comps,
            kernels=[(c,) for c in comps] + [("gyy",)], **kw)

    tc("ratio_none", t[:2], ("gzz", "gx"))
    tc("ratio_scalar", t[:2], ("gzz", "gx"), ratio=2.0)
    tc("ratio_sequence", t[:2], ("gzz", "gx"), ratio=(4.0, 1.0), weights=(1.0, 3.0))
    tc("shift_invariant", t[:2], ("gzz", "gx"), shift_invariant=True)
    tc("gz_alone", t[:1], ("gz",), weights=(1.0,))

    def tv(name, dobs, data, **kw):
        add("tess_magvec." + name, G.TesseroidMagVectorModule, dobs, kw.pop("mrange", TRANGE), TSPACING, tobs,
            data=data, kernels=[(0,), ("z", data[0]), (3,), (1, "gz")], **kw)

    inc = 60.0 + 0.25 * np.arange(nt)
    dec = np.linspace(-10.0, 10.0, nt)
    tv("bxyz", t, ("bx", "by", "bz"), weights=(1.0, 0.7, 900.0))
    tv("tf_per_point", t[:1], ("tf",), mangle=(inc, dec))
    tv("table_mirror", t, ("bx", "by", "bz"), weights="std", shift_invariant=True)
    tv("table_tf", t[:2], ("tf", "bz"), mangle=(55.0, -7.0), shift_invariant=True)
    tv("amplitude", t[:2], ("bx", "bz"), amplitude=0.5, amplitude_beta=0.05)
    tv("table_regional", t[:2], ("bx", "bz"), shift_invariant=True, mrange=(-30, 30, -60, 60, 0, -200000))

    # ---- the divide warning: 2 x 2 x 1 tesseroids of one degree and 20 km under the 6 points of
    # tests/geometry_bit_cases.py, the last 2.5 km above the inside of a cell (flagged at ratio 8)
    wrange, wspacing = (0, 2, 0, 2, 0, -20000), (-20000, 1, 1)
    wobs = (np.array([0.2, 1.8, 0.7333, 1.25, 1.0, 0.4]), np.array([0.3, 0.3, 1.7, 1.0, 0.9, 0.6]),
            np.array([40000.0, 41500.0, 43000.0, 40500.0, 52000.0, 2500.0]))
    wd = _dobs(6, 2, seed=5)
    add("gravmag.spherical.near", G.GravMagModule, wd[0], wrange, wspacing, wobs, coordinate="spherical", batch=False)
    add("tess_multi.near", G.TesseroidMultiComponentModule, wd, wrange, wspacing, wobs, components=("gzz", "gz"),
        kernels=[("gzz",)])
    add("tess_magvec.near", G.TesseroidMagVectorModule, wd, wrange, wspacing, wobs, data=("bx", "bz"),
        kernels=[(0, "bx")])
    return cases


def _sha(*arrays):
    """'<the first 16 hex digits of the SHA-256 of the arrays' float64 bytes, one after the other> <their shapes>'"""
    arrays = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return "%s %s" % (h.hexdigest()[:16], ",".join("x".join(str(n) for n in a.shape) or "scalar" for a in arrays))


def _rec(fn):
    """the digest of what fn returns (one over all entries, if a tuple), or the class and text of what it raises"""
    try:
        v = fn()
    except Exception as ex:  # noqa: BLE001
        return "%s: %s" % (type(ex).__name__, ex)
    if isinstance(v, tuple):
        return _sha(*v)
    if hasattr(v, "diagonal") and not isinstance(v, np.ndarray):
        v = v.diagonal()
    return _sha(v)


def _mask(text):
    return [re.sub(r"(kernel: ?)[-+0-9.e]+", r"\1<t>", line) for line in text.splitlines()]


def _describe(v):
    shape = getattr(v, "shape", None)
    return type(v).__name__ + ("" if shape is None else "[%s]" % "x".join(str(int(s)) for s in shape))


def run_device_case(case):
    """Everything the case's module prints, warns, carries and answers (see the module docstring)."""
    name, make, opt = case
    out = {}
    buf = io.StringIO()
    mod = None
    from gravinv3dhmc_amd import _lib
    _lib.load()     # (outside the record: what loading the library prints or warns is not the module's)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        warnings.simplefilter("ignore", ResourceWarning)
        try:
            with contextlib.redirect_stdout(buf):
                mod = make()
        except Exception as ex:  # noqa: BLE001
            out["constructor"] = "%s: %s" % (type(ex).__name__, ex)
    out["printed"] = _mask(buf.getvalue())
    out["warnings"] = ["%s: %s" % (w.category.__name__, w.message) for w in caught]
    if mod is None:
        return out
    try:
        out["vars"] = " ".join("%s:%s" % (k, _describe(v)) for k, v in sorted(vars(mod).items()))
        for k in ("Wm", "WmInv", "WmSquare", "Wb", "weights", "dobs", "dobsw", "A") + tuple(opt["names"]):
            if k in vars(mod) or hasattr(type(mod), k):   # (what a module does not have, "vars" tells)
                out[k] = _rec(lambda: getattr(mod, k))
        out["Aw"] = _rec(lambda: np.asarray(mod.Aw))
        out["kernelw"] = [type(v).__name__ for v in mod.kernelw()]
        for args in opt["kernels"]:
            out["kernel%r" % (args,)] = _rec(lambda: mod.kernel(*args))
        M = mod.Wm.shape[0]
        wm = mod.Wm.diagonal()
        model = 0.05 + 0.125 * ((np.arange(M) * 7) % 5 - 1.5)
        if hasattr(mod, "forward"):
            out["forward"] = _rec(lambda: mod.forward(model))
        x, mwapr = model * wm, 0.01 * wm
        for reg in opt["regs"]:
            out["misfit_and_grad[%s]" % reg] = _rec(
                lambda: mod.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.05))
        if hasattr(mod, "block_means"):
            out["block_means"] = _rec(mod.block_means)
        if opt["batch"]:
            from gravinv3dhmc_amd.inversion import hmc
            a = list(BATCH_ARGS)
            a[2] = np.zeros(mod._engine.N)
            out["HMCSampleBatch"] = _rec(lambda: hmc.HMCSampleBatch(
                mod, 2, 2, 1, 0.01, [2, 3], np.full(M, 0.001), np.full(M, 0.001),
                np.c_[np.zeros(M), np.full(M, 0.02)], *a))
    finally:
        mod._engine.close()
    return out


def run_device():
    return {c[0]: run_device_case(c) for c in device_cases()}
