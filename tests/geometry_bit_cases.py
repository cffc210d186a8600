"""The scripted cases behind tests/golden/geometry_bits.json: the bits of everything that is assembled from the prism
corner (csrc/kernels.hip.h: prism_each_corner, prism_v6) and from the tesseroid traversal (tess_traverse) -- stores,
result passes and the matrix-free passes -- beyond what tests/cell_store_cases.py pins.

TEST INFRASTRUCTURE ONLY.  tests/make_golden_geometry_bits.py runs the cases on the library the fixture is made from and
records them; tests/test_gpu_geometry_bits.py replays them on the library under test and compares exactly.  The cells are
the 2 x 2 x 1 of cell_store_cases; a case is (name, tesseroid pairs or 0, function of the package -> record).
"""
import numpy as np

from cell_store_cases import DIR, _P4, _T4, _sha

# ------------------------------------------------------------------------------------------------------------ geometry
#: 8 points at the prisms (z down).  0 .. 4 lie above them, off every corner's lines: dx and dy take both signs, so
#: safe_atan2_d takes its three non-zero branches (y > 0 & x < 0, y < 0 & x < 0, the plain one) and safe_log_d its log.
#: 5 lies BELOW the cells on the vertical line of the four cells' common edge: dx == 0, dy == 0, dz < 0 at the corners of
#:   x = y = 1000 -- gxy's perturbed distance; every other field has dz + r == 0 there (safe_log_d's zero branch) and
#:   dz dy == dz dx == dx dy == 0 (safe_atan2_d's zero branch).
#: 6 lies on the plane of the tops, north of the cells on the line of the edge x = 1000: dx == 0, dz == 0, dy < 0 at the
#:   corners of x = 1000, z = 0 -- gxz's perturbed distance (dy + r == 0 for the others).
#: 7 lies on the plane of the bottoms, east of the cells on the line of the edge y = 1000: dy == 0, dz == 0, dx < 0 at
#:   the corners of y = 1000, z = 500 -- gyz's perturbed distance (dx + r == 0 for the others).
P_PTS = (np.array([150.0, 1283.0, 716.5, 1850.0, 990.0, 1000.0, 1000.0, 2100.0]),
         np.array([200.0, 1000.5, 1800.0, 1001.0, 330.0, 1000.0, 2100.0, 1000.0]),
         np.array([-60.0, -75.0, -90.0, -105.0, -35.0, 600.0, 0.0, 500.0]))
P_BRANCH = {5: "gxy perturbed distance; safe_log_d(0), safe_atan2_d(0, .)", 6: "gxz perturbed distance; safe_log_d(0)",
            7: "gyz perturbed distance; safe_log_d(0)"}
NP_ = 8

#: 6 points at the tesseroids: five at 40 km and above (every cell within the distance that splits it, at every
#: ratio used), the last 2.5 km above the inside of cell 0 -- the radial split reaches its 1 km floor there at ratio 8,
#: so the cell is flagged (warn_cells > 0)
T_PTS = (np.array([0.2, 1.8, 0.7333, 1.25, 1.0, 0.4]), np.array([0.3, 0.3, 1.7, 1.0, 0.9, 0.6]),
         np.array([40000.0, 41500.0, 43000.0, 40500.0, 52000.0, 2500.0]))
NT = 6
#: 16 points for the matrix-free near-field table, which is kept only while it lists at most 1/64 of the pairs: point 0
#: lies 30 km up off the outer corner of cell 0, within the splitting distance (1.6 x 111 km) of that cell alone; the 15
#: others at 400 km and above split no cell.  One pair of 64 in the table.
T_FAR = (np.r_[-0.3, np.linspace(0.1, 1.9, 15)], np.r_[-0.3, 0.1 + 1.8 * ((7 * np.arange(15)) % 15) / 14.0],
         np.r_[30000.0, 400000.0 + 7000.0 * np.arange(15)])

GCOMP = ("potential", "geoid", "gx", "gy", "gz", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
#: the reference's ratio of every tesseroid field (RATIO_V, RATIO_G, RATIO_GG)
TRATIO = dict(potential=1.0, geoid=1.0, gx=1.6, gy=1.6, gz=1.6, gxx=8.0, gxy=8.0, gxz=8.0, gyy=8.0, gyz=8.0, gzz=8.0)
BCOMP = ("tf", "bx", "by", "bz")
BW4 = (1.0, 0.7, 900.0, 1.3)

#: models that differ from cell to cell
DENS = np.array([0.5, -1.25, 2.0, 0.3125])
MAG3 = np.array([[1.0, -0.5, 0.25], [0.125, 2.0, -1.5], [-0.75, 0.375, 3.0], [1.75, -2.25, -0.0625]])
#: a unit direction per tesseroid point
_inc, _dec = np.radians(20.0 + 9.0 * np.arange(NT)), np.radians(-15.0 + 7.0 * np.arange(NT))
FDIR6 = np.c_[np.cos(_inc) * np.cos(_dec), np.cos(_inc) * np.sin(_dec), np.sin(_inc)]


def _store(eng, out, dense=True):
    """build_G, then the digests of the store, of weight()'s wm and of forward() of a model that differs per cell"""
    eng.build_G()
    out["kernel_stats"] = eng.kernel_stats()
    if not dense:
        st = eng.matrix_free_stats()
        out["near_field"] = {"entries": st["near_entries"], "leaves": st["near_leaves"]}
    if dense:
        out["G"] = _sha(eng.download_G().T)
    wm = eng.weight()
    out["wm"] = _sha(wm)
    out["forward"] = _sha(eng.forward((0.25 + 0.125 * np.arange(eng.M)) * wm))


def _run(pkg, N, M, cells, obs, body, matrix_free=False):
    eng = pkg.engine.Engine(N, M)
    out = {}
    try:
        if matrix_free:
            eng.set_matrix_free(True)
        cells(eng, pkg._lib)
        eng.set_obs(*obs)
        body(eng, out)
    finally:
        eng.close()
    return out


def _prism_comp(comp):
    def body(eng, out):
        _store(eng, out)
        out["result"] = _sha(eng.prism_result(DENS))
    return lambda pkg: _run(pkg, NP_, 4, lambda e, L: e.set_cells(_P4, L.CELL_PRISM, component=comp), P_PTS, body)


def _prism_tf(pkg):
    def body(eng, out):
        _store(eng, out)
        out["result"] = _sha(eng.tf_result(MAG3))
    return _run(pkg, NP_, 4, lambda e, L: e.set_cells(_P4, L.CELL_PRISM_TF, direction=DIR), P_PTS, body)


def _prism_mvi(pkg):
    def body(eng, out):
        _store(eng, out)
        out["result"] = _sha(eng.tf_result(MAG3))
        for c in BCOMP[1:]:
            out["result_" + c] = _sha(eng.b_result(c, MAG3))
    return _run(pkg, NP_, 12, lambda e, L: e.set_cells_mvi(_P4, DIR), P_PTS, body)


def _prism_mvi_data(pkg):
    def body(eng, out):
        _store(eng, out)
        for c in BCOMP[1:]:
            out["result_" + c] = _sha(eng.b_result(c, MAG3))
    return _run(pkg, 4 * NP_, 12, lambda e, L: e.set_cells_mvi_data(_P4, DIR, BCOMP, BW4), P_PTS, body)


def _prism_joint(pkg):
    return _run(pkg, 2 * NP_, 8, lambda e, L: e.set_cells(_P4, L.CELL_PRISM_JOINT, direction=DIR), P_PTS, _store)


def _tess_comp(comp, matrix_free=False, pts=T_PTS):
    def cells(e, L):
        e.set_cells(_T4, L.CELL_TESSEROID, ratio=TRATIO[comp], component=comp)
    return lambda pkg: _run(pkg, pts[0].size, 4, cells, pts, lambda e, o: _store(e, o, not matrix_free), matrix_free)


def _tess_mag(pkg):
    def body(eng, out):
        _store(eng, out)
        for c in BCOMP:
            out["result_" + c] = _sha(eng.tess_b_result(c, MAG3))
            out["result_" + c + "_kernel_stats"] = eng.kernel_stats()
    return _run(pkg, 4 * NT, 12, lambda e, L: e.set_cells_tess_mag(_T4, 8.0, BCOMP, BW4, fdir=FDIR6), T_PTS, body)


CASES = [("prism." + c, 0, _prism_comp(c)) for c in GCOMP] + \
        [("prism.tf", 0, _prism_tf), ("prism.mvi", 0, _prism_mvi), ("prism.mvi_data", 0, _prism_mvi_data),
         ("prism.joint", 0, _prism_joint)] + \
        [("tess." + c, NT * 4, _tess_comp(c)) for c in GCOMP] + \
        [("tess.mag", NT * 4, _tess_mag), ("tess.matrix_free.gxz", NT * 4, _tess_comp("gxz", True)),
         # (a matrix-free gz context reports no kernel_stats: its build stores and counts nothing.  At T_PTS every pair
         # splits -- tess.gz's leaves -- so no near-field table is kept and the passes subdivide inside; at T_FAR the
         # table is filled, and ITS leaves show that the subdivision ran)
         ("tess.matrix_free.gz", 0, _tess_comp("gz", True)), ("tess.matrix_free.gz.near", 0, _tess_comp("gz", True, T_FAR))]


def run_all(pkg):
    return {name: fn(pkg) for name, _, fn in CASES}


def all_stats(rec):
    """every kernel_stats() of a case's record"""
    return [v for k, v in rec.items() if k.endswith("kernel_stats")]


def subdivision_ran(doc):
    """What makes a record worth keeping: every tesseroid pass shows more leaves than (point, cell) pairs -- else the
    subdivision has not run, and a copy of it cannot go wrong --, a filled near-field table more leaves than entries,
    there is such a table, and some pass flags a cell.  Returns the text of what is missing, or None."""
    warned = tables = 0
    for name, pairs, _ in CASES:
        for st in all_stats(doc[name]) if pairs else []:
            if st["leaves"] <= pairs:
                return "%s: %d leaves for %d pairs" % (name, st["leaves"], pairs)
            warned += st["warn_cells"] > 0
        nf = doc[name].get("near_field", {"entries": 0})
        if nf["entries"]:
            tables += 1
            if nf["leaves"] <= nf["entries"]:
                return "%s: near-field table of %d leaves for %d entries" % (name, nf["leaves"], nf["entries"])
    if not tables:
        return "no matrix-free case fills a near-field table"
    return None if warned else "no tesseroid pass flags a cell (warn_cells > 0)"
