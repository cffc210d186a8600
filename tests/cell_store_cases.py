"""The scripted cases behind tests/golden/cell_store_refusals.json: what every gh_set_cells_* entry point refuses (and
what it accepts), what the stores refuse of each other, and the bits of the smallest valid context of every cell kind.

TEST INFRASTRUCTURE ONLY.  tests/make_golden_cell_refusals.py runs the cases on the library the fixture is made from and
records them; tests/test_gpu_cell_store_refusals.py replays them on the library under test and compares exactly.

A refusal case is (name, N, M, steps); a step is (C-ABI function, arguments) with the arguments as plain Python values:
None is a null pointer, a list or an array becomes a C array of the prototype's element type.  EVERY step's return code is
recorded, with gh_last_error's text where the code is not GH_OK, so a case that ends in GH_OK pins that too.
N = M = 12 (divisible by 2, 3 and 4) unless a case is about the sizes; the cells are four valid ones repeated.
"""
import ctypes as C
import hashlib

import numpy as np

NAN, INF = float("nan"), float("inf")

# ------------------------------------------------------------------------------------------------------------ geometry
#: 2 x 2 x 1 prisms (x1, x2, y1, y2, z1, z2), repeated to 16 cells: enough for every M the cases use
_P4 = np.array([[0, 1000, 0, 1000, 0, 500], [1000, 2000, 0, 1000, 0, 500],
                [0, 1000, 1000, 2000, 0, 500], [1000, 2000, 1000, 2000, 0, 500]], dtype=float)
#: 2 x 2 x 1 tesseroids (w, e, s, n, top, bottom): one degree wide, 20 km thick
_T4 = np.array([[0, 1, 0, 1, 0, -20000], [1, 2, 0, 1, 0, -20000],
                [0, 1, 1, 2, 0, -20000], [1, 2, 1, 2, 0, -20000]], dtype=float)
#: the smallest full circle the shift-invariant table accepts (2 longitudes per cell row; host_lonsym.h refuses "fewer
#: than 2 longitudes per cell row"): 2 x 2 x 1 tesseroids of 180 degrees
_C4 = np.array([[-180, 0, -30, 0, 0, -200000], [0, 180, -30, 0, 0, -200000],
                [-180, 0, 0, 30, 0, -200000], [0, 180, 0, 30, 0, -200000]], dtype=float)
PB = np.tile(_P4, (4, 1))
TB = np.tile(_T4, (4, 1))
TB_BAD = TB.copy()
TB_BAD[1, :2] = (2.0, 1.0)   # cell 1: w > e
#: 12 points above the prisms (z up is negative), 12 above the tesseroids at 40 km: close enough to split the cells
_g = np.meshgrid(np.linspace(150, 1850, 4), np.linspace(200, 1800, 3), indexing="ij")
P_OBS = (_g[0].ravel(), _g[1].ravel(), -60.0 - 5.0 * np.arange(12.0))
_g = np.meshgrid(np.linspace(0.2, 1.8, 4), np.linspace(0.3, 1.7, 3), indexing="ij")
T_OBS = (_g[0].ravel(), _g[1].ravel(), 40000.0 + 500.0 * np.arange(12.0))
#: 4 points on the circle's longitude spacing, two classes
C_OBS = (np.array([-90.0, 90.0, -90.0, 90.0]), np.array([-15.0, -15.0, 15.0, 15.0]), np.full(4, 1.0e6))
DIR = (0.6, 0.0, 0.8)
FDIR = np.tile(np.array(DIR), (12, 1))
FDIR_NAN = FDIR.copy()
FDIR_NAN[2, 1] = NAN
BUF = np.zeros(64)

GCOMPS, GW, GR = [4, 2, 10], [1.0, 2.0, 0.5], [1.6, 1.6, 8.0]   # gz, gx, gzz
BCOMPS, BW = [1, 2, 3], [1.0, 0.7, 900.0]                       # bx, by, bz

#: the entry points of the stores of blocks, each with a call that a fresh (12, 12) context accepts
BLOCK_EPS = ("joint", "mvi", "mvi_data", "tess_mag", "tess_mag_table", "multi", "tess_multi")
LIST_EPS = ("mvi_data", "tess_mag", "tess_mag_table", "multi", "tess_multi")


def ep(name, bounds="default", d=DIR, n=3, comps="default", w="default", r="default", ratio=2.0, fdir=None):
    """the step that calls gh_set_cells_<name> with valid arguments, but for those given"""
    tess = name.startswith("tess")
    if isinstance(bounds, str):
        bounds = TB if tess else PB
    grav = name in ("multi", "tess_multi")
    if isinstance(comps, str):
        comps = (GCOMPS if grav else BCOMPS)[:n]
    if isinstance(w, str):
        w = (GW if grav else BW)[:n]
    if isinstance(r, str):
        r = GR[:n]
    fn = "gh_set_cells_" + name
    if name in ("joint", "mvi", "tf"):
        return (fn, [bounds, d[0], d[1], d[2]])
    if name == "mvi_data":
        return (fn, [bounds, d[0], d[1], d[2], n, comps, w])
    if name in ("tess_mag", "tess_mag_table"):
        return (fn, [bounds, ratio, n, comps, w, fdir])
    if name == "multi":
        return (fn, [bounds, n, comps, w])
    if name == "tess_multi":
        return (fn, [bounds, n, comps, r, w])
    raise KeyError(name)


SET_OBS = ("gh_set_obs", [P_OBS[0], P_OBS[1], P_OBS[2]])
SET_OBS_TESS = ("gh_set_obs", [T_OBS[0], T_OBS[1], T_OBS[2]])
MF, LS = ("gh_set_matrix_free", [1]), ("gh_set_shift_invariant", [1])
SHARD = ("gh_shard_init_callback", ["allreduce", None, 0, 1, "M", 0])   # a world of one rank: sh.kind != 0
BSCG = ("gh_bscg_run", [4, None, None, None, 0.0, 1.0, 1.0, 0.5, 8, None, None, None, None, None, None])
PLAIN = ("gh_set_cells", [PB, 0, 1.6])
INFO = ("gh_multi_info", [None, None, None, None, None])
RESULTS = [("gh_tf_result", [BUF, BUF]), ("gh_b_result", [1, BUF, BUF]), ("gh_tess_b_result", [1, BUF, BUF]),
           ("gh_prism_result", [BUF, BUF])]

#: a context of every cell kind, of the table forms and of the three delegations: (name, the steps that make it)
KINDS = [("prism", [PLAIN]), ("tesseroid", [("gh_set_cells", [TB, 1, 1.6])]), ("tf", [ep("tf")]),
         ("prism_comp", [("gh_set_cells_prism", [PB, 5])]), ("tess_comp", [("gh_set_cells_tess", [TB, 10, 8.0])]),
         ("joint", [ep("joint")]), ("multi", [ep("multi")]), ("mvi", [ep("mvi")]), ("mvi_data", [ep("mvi_data")]),
         ("tess_mag", [ep("tess_mag")]), ("tess_multi", [ep("tess_multi")]),
         ("tess_mag_table", [ep("tess_mag_table")]), ("tess_multi_table", [LS, ep("tess_multi")]),
         ("mvi_data_is_mvi", [ep("mvi_data", n=1, comps=[0], w=[1.0])]),
         ("tess_multi_is_tesseroid", [ep("tess_multi", n=1, comps=[4], w=[1.0], r=[1.6])]),
         ("prism_gz_is_prism", [("gh_set_cells_prism", [PB, 4])]),
         ("tess_gz_is_tesseroid", [("gh_set_cells_tess", [TB, 4, 1.6])])]


def refusal_cases():
    cases = []

    def add(name, steps, N=12, M=12):
        cases.append((name, N, M, list(steps)))

    # ---- each entry point's own arguments
    add("set_cells.null", [("gh_set_cells", [None, 0, 1.6])])
    add("set_cells.kind", [("gh_set_cells", [PB, 7, 1.6])])
    add("set_cells.ratio0", [("gh_set_cells", [TB, 1, 0.0])])
    add("tf.null", [ep("tf", bounds=None)])
    add("tf.nan", [ep("tf", d=(0.6, NAN, 0.8))])
    for fn in ("gh_set_cells_prism", "gh_set_cells_tess"):
        tail = [1.6] if fn.endswith("tess") else []
        b = TB if fn.endswith("tess") else PB
        add(fn[13:] + ".null", [(fn, [None, 5] + tail)])
        add(fn[13:] + ".comp-1", [(fn, [b, -1] + tail)])
        add(fn[13:] + ".comp11", [(fn, [b, 11] + tail)])
    add("tess.bounds", [("gh_set_cells_tess", [TB_BAD, 10, 8.0])])
    add("tess.ratio0", [("gh_set_cells_tess", [TB, 10, 0.0])])
    add("tess.gz_ratio0", [("gh_set_cells_tess", [TB, 4, 0.0])])
    add("tess.bounds_before_gz", [("gh_set_cells_tess", [TB_BAD, 4, 1.6])])
    for e in BLOCK_EPS:
        add(e + ".null", [ep(e, bounds=None)])
    for e in LIST_EPS:
        cmax = 4 if e not in ("multi", "tess_multi") else 11
        add(e + ".null_comps", [ep(e, comps=None)])
        add(e + ".null_weights", [ep(e, w=None)])
        add(e + ".n0", [ep(e, n=0)])
        add(e + ".nmax", [ep(e, n=cmax + 1, comps=list(range(cmax + 1)), w=[1.0] * (cmax + 1), r=[1.6] * (cmax + 1))])
        add(e + ".comp_low", [ep(e, comps=[1, -1, 3])])
        add(e + ".comp_high", [ep(e, comps=[1, cmax, 3])])
        add(e + ".duplicate", [ep(e, comps=[1, 3, 1])])
        for tag, v in (("0", 0.0), ("neg", -1.0), ("inf", INF), ("nan", NAN)):
            add(e + ".weight_" + tag, [ep(e, w=[1.0, v, 2.0])])
        add(e + ".N13", [ep(e)], N=13)
    add("tess_multi.null_ratios", [ep("tess_multi", r=None)])
    add("tess_multi.ratio0", [ep("tess_multi", r=[1.6, 0.0, 8.0])])
    add("tess_multi.ratio_nan", [ep("tess_multi", r=[1.6, 1.6, NAN])])
    for e in ("tess_mag", "tess_mag_table"):
        add(e + ".ratio0", [ep(e, ratio=0.0)])
        add(e + ".fdir_nan", [ep(e, fdir=FDIR_NAN)])
        add(e + ".tf_without_fdir", [ep(e, comps=[0, 1, 2])])
        add(e + ".tf_with_fdir", [ep(e, comps=[0, 1, 2], fdir=FDIR)])
    for e in ("mvi", "mvi_data", "tess_mag", "tess_mag_table"):
        add(e + ".M13", [ep(e)], M=13)
    add("joint.N13", [ep("joint")], N=13)
    add("joint.M13", [ep("joint")], M=13)
    for e in ("joint", "mvi", "mvi_data"):
        add(e + ".nan", [ep(e, d=(NAN, 0.0, 0.8))])
    for e in ("tess_mag", "tess_mag_table", "tess_multi"):
        add(e + ".bounds", [ep(e, bounds=TB_BAD)])

    # ---- the state of the context
    for e in BLOCK_EPS:
        add(e + ".after_set_obs", [SET_OBS, ep(e)])
        add(e + ".after_set_cells", [PLAIN, ep(e)])
        for other in BLOCK_EPS:
            add("%s.after_%s" % (e, other), [ep(other), ep(e)])
        add(e + ".matrix_free_first", [MF, ep(e)])
        add(e + ".shift_invariant_first", [LS, ep(e)])
        add(e + ".sharded", [SHARD, ep(e)])
        # (the refusal comes before any allocation of the size)
        add(e + ".rows16386", [ep(e)], N=16386, M=6)
    add("joint.rows32770", [ep("joint")], N=32770, M=6)

    # ---- two faults at once: the order of the checks
    add("order.multi.component_on_used_context", [SET_OBS, ep("multi", comps=[4, 99, 2])])
    add("order.mvi.M13_and_nan", [ep("mvi", d=(NAN, 0.0, 0.8))], M=13)
    add("order.joint.N13_and_nan", [ep("joint", d=(NAN, 0.0, 0.8))], N=13)
    add("order.tess_mag.bounds_and_matrix_free", [MF, ep("tess_mag", bounds=TB_BAD)])
    add("order.multi.matrix_free_and_rows", [MF, ep("multi")], N=16386, M=6)
    add("order.tess_multi.weight_and_ratio", [ep("tess_multi", w=[1.0, 0.0, 2.0], r=[1.6, 0.0, 8.0])])
    add("order.mvi_data.N13_and_M13", [ep("mvi_data")], N=13, M=13)
    add("order.tess_mag.sharded_and_rows", [SHARD, ep("tess_mag")], N=16386, M=6)
    add("order.mvi_data.rows_before_delegation", [ep("mvi_data", n=1, comps=[0], w=[1.0])], N=16386, M=6)

    # ---- what a context of each kind answers the others: the result passes, the block table, the bootstrap batch,
    # gh_set_cells, the matrix-free mode and the table
    for name, steps in KINDS:
        obs = SET_OBS_TESS if name.startswith("tess") else SET_OBS
        add("cross." + name, steps + [obs] + RESULTS + [INFO, BSCG, PLAIN, MF, LS])
    add("cross.tess_mag.table_after_build", [ep("tess_mag"), SET_OBS_TESS, ("gh_build_G", []), LS])
    return cases


# ------------------------------------------------------------------------------------------------------------ running
def _convert(lib_mod, argtype, v, M, keep):
    if v is None:
        return None
    if isinstance(v, str):
        if v == "M":
            return M
        fn = lib_mod.ALLREDUCE_FN(lambda user, buf, count: 0)
        keep.append(fn)
        return C.cast(fn, C.c_void_p)
    if isinstance(v, (list, tuple, np.ndarray)):
        if argtype is C.POINTER(C.c_int):
            a = (C.c_int * max(len(v), 1))(*[int(x) for x in v])
            keep.append(a)
            return a
        a = np.ascontiguousarray(v, dtype=np.float64).copy()
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_double))
    return v


def run_refusal_case(lib_mod, case):
    """[[return code, gh_last_error's text or ""], ...] of the case's steps on a context of its own"""
    name, N, M, steps = case
    lib = lib_mod.load()
    h = C.c_void_p()
    rc = lib.gh_create(C.byref(h), 0, N, M)
    assert rc == 0, (name, rc)
    out, keep = [], []
    try:
        for fn, args in steps:
            types = lib_mod.PROTOTYPES[fn][1][1:]
            assert len(types) == len(args), (name, fn)
            rc = getattr(lib, fn)(h, *[_convert(lib_mod, t, v, M, keep) for t, v in zip(types, args)])
            msg = lib.gh_last_error(h) if rc != 0 else b""
            out.append([int(rc), msg.decode("utf-8", "replace")])
    finally:
        lib.gh_destroy(h)
    return out


def run_refusals(lib_mod):
    return {c[0]: run_refusal_case(lib_mod, c) for c in refusal_cases()}


# --------------------------------------------------------------------------------------------------------------- bits
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _hexes(v):
    return [float(x).hex() for x in np.asarray(v, dtype=float).ravel()]


def _prism(n):
    return tuple(a[:n] for a in P_OBS)


def _tess(n):
    return tuple(a[:n] for a in T_OBS)


#: the smallest valid context of every kind: 12 rows in all, 2 x 2 x 1 cells times the column blocks.
#: (name, N, M, how the engine gets its cells, the observation points, on the table?)
BIT_CASES = [
    ("prism", 12, 4, lambda e, L: e.set_cells(_P4, L.CELL_PRISM), _prism(12), False),
    ("tesseroid", 12, 4, lambda e, L: e.set_cells(_T4, L.CELL_TESSEROID, ratio=1.6), _tess(12), False),
    ("tf", 12, 4, lambda e, L: e.set_cells(_P4, L.CELL_PRISM_TF, direction=DIR), _prism(12), False),
    ("prism_comp", 12, 4, lambda e, L: e.set_cells(_P4, L.CELL_PRISM_COMP, component="gxz"), _prism(12), False),
    ("tess_comp", 12, 4, lambda e, L: e.set_cells(_T4, L.CELL_TESSEROID_COMP, ratio=8.0, component="gzz"), _tess(12),
     False),
    ("joint", 12, 8, lambda e, L: e.set_cells(_P4, L.CELL_PRISM_JOINT, direction=DIR), _prism(6), False),
    ("multi", 12, 4, lambda e, L: e.set_cells_multi(_P4, ("gz", "gx", "gzz"), GW), _prism(4), False),
    ("mvi", 12, 12, lambda e, L: e.set_cells_mvi(_P4, DIR), _prism(12), False),
    ("mvi_data", 12, 12, lambda e, L: e.set_cells_mvi_data(_P4, DIR, ("tf", "bx", "bz"), BW), _prism(4), False),
    ("tess_mag", 12, 12, lambda e, L: e.set_cells_tess_mag(_T4, 2.0, ("tf", "bx", "bz"), BW, fdir=FDIR[:4]), _tess(4),
     False),
    ("tess_multi", 12, 4, lambda e, L: e.set_cells_tess_multi(_T4, ("gz", "gx", "gzz"), GR, GW), _tess(4), False),
    ("tess_mag_table", 12, 12,
     lambda e, L: e.set_cells_tess_mag(_C4, 2.0, ("bx", "by", "bz"), BW, shift_invariant=True), C_OBS, True),
    ("tess_multi_table", 12, 4,
     lambda e, L: (e.set_shift_invariant(True), e.set_cells_tess_multi(_C4, ("gz", "gx", "gzz"), GR, GW)), C_OBS, True),
]


def run_bit_case(pkg, case, values=False):
    """The case's context through gravinv3dhmc_amd.engine.Engine: SHA-256 of download_G()'s bytes (the dense forms), of
    weight()'s wm and of forward() of a fixed mw; kernel_stats(); multi_info(), or the text it refuses with.
    values: the arrays themselves too, as hex floats (to look at a quantity that does not reproduce)."""
    name, N, M, cells, obs, table = case
    L = pkg._lib
    eng = pkg.engine.Engine(N, M)
    out = {}
    try:
        cells(eng, L)
        eng.set_obs(*obs)
        eng.build_G()
        out["kernel_stats"] = eng.kernel_stats()
        arrays = {}
        if not table:
            arrays["G"] = eng.download_G().T   # (M x rows, C-ordered: the bytes as the library wrote them)
        arrays["wm"] = eng.weight()
        arrays["forward"] = eng.forward((0.25 + 0.125 * np.arange(M)) * arrays["wm"])
        for k, a in arrays.items():
            out[k] = _sha(a)
            out[k + "_shape"] = list(np.shape(a))
            if values:
                out[k + "_values"] = _hexes(a)
        try:
            mi = eng.multi_info()
            out["multi_info"] = {"components": mi["components"], "weights": _hexes(mi["weights"]),
                                 "pred_mean": _hexes(mi["pred_mean"]), "obs_mean": _hexes(mi["obs_mean"])}
        except NotImplementedError as ex:
            out["multi_info"] = str(ex)
    finally:
        eng.close()
    return out


def run_bits(pkg, values=False):
    return {c[0]: run_bit_case(pkg, c, values) for c in BIT_CASES}
