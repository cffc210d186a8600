"""Host side of the prism gravity components (no GPU): the reference's constants, the public
functions of gravmag.prism, the refusals of GravMagModule(component=...) and the C ABI."""
import inspect
import os

import numpy as np
import pytest

from conftest import gold

COMPS = ("potential", "geoid", "gx", "gy", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_references_bits():
    from gravinv3dhmc_amd import constants
    g = gold("prism_comp_cases.npz")
    assert constants.SI2EOTVOS == 1000000000.0 and constants.g0 == 9.80
    assert np.array_equal(np.float64(constants.SI2EOTVOS), g["SI2EOTVOS"])
    assert np.array_equal(np.float64(constants.g0), g["g0"])
    # the scales of the kernels, rounded once as prism.py rounds them
    assert constants.G * constants.SI2EOTVOS == 0.00000006673 * 1000000000.0
    assert constants.G / constants.g0 == 0.00000006673 / 9.80


def test_prism_exposes_every_gravity_field_with_the_references_parameters():
    from gravinv3dhmc_amd.gravmag import prism
    for name in COMPS + ("gz",):
        fn = getattr(prism, name)
        params = list(inspect.signature(fn).parameters)
        assert params[:7] == ["xp", "yp", "zp", "prisms", "dens", "njobs", "pool"], (name, params)
        assert params[7:] == ["return_kernel", "device"], (name, params)


def _obs():
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 4), np.linspace(0, 2000, 3))]
    return xp, yp, np.zeros_like(xp)


def test_module_refuses_a_component_on_tesseroids_and_with_the_magnetic_field():
    import gravinv3dhmc_amd as g
    lon, lat = np.meshgrid(np.linspace(0, 10, 3), np.linspace(-5, 5, 3))
    for comp in ("gzz", "potential", "gx"):
        with pytest.raises(NotImplementedError, match="spherical"):
            g.GravMagModule(np.zeros(9), (0, 10, -5, 5, 0, -10000), (5000, 5, 5),
                            (lon.ravel(), lat.ravel(), np.full(9, 1000.0)), coordinate="spherical",
                            component=comp, verbose=False)
        with pytest.raises(ValueError, match="magnetic"):
            g.GravMagModule(np.zeros(12), (0, 2000, 0, 3000, 0, 1000), (250, 500, 400), _obs(),
                            field="magnetic", component=comp, verbose=False)
    with pytest.raises(ValueError, match="component"):
        g.GravMagModule(np.zeros(12), (0, 2000, 0, 3000, 0, 1000), (250, 500, 400), _obs(),
                        component="gzx", verbose=False)


def test_module_takes_component_as_a_named_parameter():
    import gravinv3dhmc_amd as g
    params = inspect.signature(g.GravMagModule.__init__).parameters
    assert params["component"].default == "gz"
    assert params["component"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_c_abi_declares_and_binds_the_component_entry_points():
    from gravinv3dhmc_amd import _lib
    assert _lib.CELL_PRISM_COMP == 3
    assert [_lib.COMPONENTS[c] for c in ("potential", "geoid", "gx", "gy", "gz") + COMPS[4:]] == list(range(11))
    assert {"gh_set_cells_prism", "gh_prism_result"} <= set(_lib.PROTOTYPES)
    with open(os.path.join(ROOT, "include", "gravhmc.h")) as f:
        header = f.read()
    assert "int gh_set_cells_prism(gh_ctx *ctx, const double *bounds6, int component);" in header
    assert "int gh_prism_result(gh_ctx *ctx, const double *dens, double *result);" in header
    assert "GH_CELL_PRISM_COMP = 3" in header
    for i, c in enumerate(("POTENTIAL", "GEOID", "GX", "GY", "GZ", "GXX", "GXY", "GXZ", "GYY", "GYZ", "GZZ")):
        assert "GH_COMP_%s = %d" % (c, i) in header


def test_fixtures_cover_every_singular_branch():
    """The stored geometries put points on the edge lines where gxy / gxz / gyz take the reference's
    perturbed distance, on both sides, and on the guards safe_log(0) / safe_atan2(0, .)."""
    g = gold("prism_comp_cases.npz")
    pts = np.c_[g["xp"], g["yp"], g["zp"]]
    fired = {"gxy": 0, "gxz": 0, "gyz": 0}
    other_side = dict(fired)
    for b in g["cells"]:
        X, Y, Z = b[[1, 0]], b[[3, 2]], b[[5, 4]]
        for x in X:
            for y in Y:
                for z in Z:
                    d = np.c_[x - pts[:, 0], y - pts[:, 1], z - pts[:, 2]]
                    for comp, (a, c, e) in (("gxy", (0, 1, 2)), ("gxz", (0, 2, 1)), ("gyz", (1, 2, 0))):
                        line = (d[:, a] == 0) & (d[:, c] == 0)
                        fired[comp] += int(np.sum(line & (d[:, e] < 0)))
                        other_side[comp] += int(np.sum(line & (d[:, e] > 0)))
    assert min(fired.values()) > 0 and min(other_side.values()) > 0, (fired, other_side)
    for comp in g["comps"]:
        assert np.isfinite(g["K_" + str(comp)]).all()
