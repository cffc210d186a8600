"""Generate the fixture of the tesseroid gravity fields tests/golden/tess_comp_cases.npz from the reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_tess.py
The file holds DATA only: inputs and the reference's outputs of gravmag.tesseroid.<field> (result,
kernel2d, the number of RuntimeWarnings it emits) for the ten fields other than gz, each at its default
ratio.  ref_harness runs _tesseroid_numba as plain Python (numba is stubbed), so the cases are small.
Every array is a deterministic function of the fixed inputs below: two runs write the same arrays.
(Not collected by pytest: the name does not start with test_.)

Cases:
  g_*   a coarse global mesh (2 x 4 x 6 cells, densities 0.1 .. 0.5), observations on a 4 x 3 grid at 250 km
  n_*   near-field, polar and thin cells (the geometries of oracle/make_golden.py::tess_cases) with
        observations between 2 and 250 km above them; the thin cell makes the reference warn
  d_*   the `dens` override (2.5 for every cell) on a list model that holds a None cell (skipped), a cell
        below the size threshold (dropped with a warning, a trailing zero column) and a regular cell
  o_*   one cell and one observation where the reference raises OverflowError at RATIO_GG
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
#: the fields of tesseroid.py:324-508 other than gz, in GH_COMP_* order
FIELDS = ("potential", "geoid", "gx", "gy", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")

# the cases' geometry (the GPU tests rebuild the models from these arrays)
G_AREA, G_SPACING = (-180.0, 180.0, -90.0, 90.0, 0.0, -1.0e6), (-500000.0, 45.0, 60.0)
N_CELLS = np.array([[10, 10.5, 20, 20.5, 0, -1000], [10, 10.5, 20, 20.5, -1000, -3000],
                    [10, 11, 20, 21, 2000, -5000], [10, 10.5, 20, 20.5, 0, -500],
                    [-180, -150, 60, 90, 0, -300000], [0, 3, -90, -87, -2.7e6, -3e6]], float)
N_LON = np.array([10.25, 10.0, 10.6, 12.0, 10.25, -170.0, 0.0, 100.0])
N_LAT = np.array([20.25, 20.0, 20.4, 22.0, 20.3, 89.0, -90.0, -45.0])
N_H = np.array([2500.0, 5000.0, 3000.0, 20000.0, 10000.0, 50000.0, 250000.0, 250000.0])
D_CELLS = np.array([[10, 11, 20, 21, 0, -20000], [10, 10 + 1e-7, 21, 22, 0, -20000],
                    [12, 14, 20, 22, 0, -50000]], float)
D_NONE = 1          # the None entry goes in front of D_CELLS[D_NONE]
D_DENS = 2.5
D_LON, D_LAT, D_H = np.array([10.5, 13.0, 20.0]), np.array([20.5, 21.0, 25.0]), np.full(3, 100000.0)
# (an observation 1 m above the north-east top corner of a thick cell: the subdivision follows the last child
# pushed, deepest there)
O_CELL = np.array([[0, 60, 0, 60, 0, -3e6]], float)
O_LON, O_LAT, O_H = np.array([60.0]), np.array([60.0]), np.array([1.0])


class _ListModel(list):
    """A plain list of tesseroids with a `props` dict, as tesseroid.py's _check_input reads model.props."""
    props = {"density": None}


def _list_model(R, cells, rho, none_at=None):
    out = _ListModel(R.mesher.Tesseroid(*c, props={"density": float(d)}) for c, d in zip(cells, rho))
    if none_at is not None:
        out.insert(none_at, None)
    return out


def _run(R, field, lon, lat, h, model, **kw):
    """(result, kernel2d, number of RuntimeWarnings) of the reference's tesseroid.<field>."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with contextlib.redirect_stdout(io.StringIO()):
            res, K = getattr(R.tesseroid, field)(lon, lat, h, model, **kw)
    return res, K, sum(1 for x in w if issubclass(x.category, RuntimeWarning))


def main():
    R = ref_harness.load()
    out = {}
    # coarse global mesh
    mesh = R.mesher.TesseroidMesh(G_AREA, G_SPACING)
    g_rho = np.linspace(0.1, 0.5, mesh.size)
    mesh.addprop("density", g_rho)
    g_lon, g_lat = [a.ravel() for a in np.meshgrid(np.linspace(-150, 120, 4), np.linspace(-60, 60, 3))]
    g_h = np.full_like(g_lon, 250000.0)
    out.update(g_lon=g_lon, g_lat=g_lat, g_h=g_h, g_rho=g_rho, g_area=np.array(G_AREA), g_spacing=np.array(G_SPACING),
               g_bounds=np.array([c.get_bounds() for c in mesh]))
    # near field
    n_rho = np.linspace(0.2, 0.7, len(N_CELLS))
    n_model = _list_model(R, N_CELLS, n_rho)
    out.update(n_cells=N_CELLS, n_rho=n_rho, n_lon=N_LON, n_lat=N_LAT, n_h=N_H)
    # dens override, a None cell and a degenerate one
    d_rho = np.array([0.3, 0.4, 0.5])
    d_model = _list_model(R, D_CELLS, d_rho, none_at=D_NONE)
    out.update(d_cells=D_CELLS, d_rho=d_rho, d_none=D_NONE, d_dens=D_DENS, d_lon=D_LON, d_lat=D_LAT, d_h=D_H)
    for f in FIELDS:
        r, K, nw = _run(R, f, g_lon, g_lat, g_h, mesh)
        out.update({"g_result_" + f: r, "g_K_" + f: K, "g_warn_" + f: nw})
        r, K, nw = _run(R, f, N_LON, N_LAT, N_H, n_model)
        out.update({"n_result_" + f: r, "n_K_" + f: K, "n_warn_" + f: nw})
        r, K, nw = _run(R, f, D_LON, D_LAT, D_H, d_model, dens=D_DENS)
        out.update({"d_result_" + f: r, "d_K_" + f: K, "d_warn_" + f: nw})
        print(f, "warnings", out["g_warn_" + f], out["n_warn_" + f], out["d_warn_" + f], flush=True)
    # overflow at RATIO_GG
    o_model = _list_model(R, O_CELL, [1.0])
    try:
        _run(R, "gzz", O_LON, O_LAT, O_H, o_model)
        raise AssertionError("the overflow geometry did not overflow")
    except OverflowError:
        pass
    out.update(o_cells=O_CELL, o_lon=O_LON, o_lat=O_LAT, o_h=O_H, o_field=np.array("gzz"))
    np.savez_compressed(os.path.join(GOLD, "tess_comp_cases.npz"), **out)
    print("tess_comp_cases", {k: np.shape(v) for k, v in out.items() if k.endswith("_gzz")})


if __name__ == "__main__":
    main()
