"""Host side of the total-field magnetic field (no GPU): the field direction, the reference's
scale factor and the rule that decides which prisms take part (gravmag/prism.py:665-733,
1140-1160)."""
import numpy as np
import pytest

from conftest import gold


def test_dircos_and_ang2vec_match_the_reference_bits():
    from gravinv3dhmc_amd import utils
    g = gold("prism_tf_cases.npz")
    for d, (inc, dec) in enumerate(g["dirs"]):
        assert np.array_equal(np.array(utils.dircos(inc, dec)), g["dircos"][d])
        assert np.array_equal(utils.ang2vec(np.array([0.0, 1.0, -2.5, 7.0]), inc, dec), g["ang2vec"][d])
    v = utils.ang2vec(2.0, 60.0, -10.0)          # a scalar intensity: one vector
    assert v.shape == (3,) and np.allclose(np.linalg.norm(v), 2.0, rtol=1e-15)
    f = utils.dircos(90.0, 0.0)                   # vertical field: straight down
    assert abs(f[2] - 1.0) < 1e-15 and abs(f[0]) < 1e-16 and f[1] == 0.0


def test_total_field_scale_is_the_references_micro_tesla_factor():
    from gravinv3dhmc_amd import constants
    assert constants.CM == 1e-7 and constants.T2NT == 1e6
    assert constants.CM * constants.T2NT == 0.09999999999999999


def test_skip_rule_on_a_carved_mesh():
    from gravinv3dhmc_amd import mesher, utils
    from gravinv3dhmc_amd.gravmag._common import active_cells_mag
    mesh = mesher.PrismMesh((0, 400, 0, 600, 0, 300), (100, 100, 100))
    xs, ys = np.meshgrid(np.linspace(0, 400, 9), np.linspace(0, 600, 9))
    mask = mesh.carvetopo(xs.ravel(), ys.ravel(), -150.0 + 0.5 * xs.ravel())
    assert len(mask) > 0
    f = utils.dircos(60.0, -10.0)
    # no property, no pmag: nothing is visited
    b, m, _ = active_cells_mag(mesh, None, f)
    assert b.shape == (0, 6) and m.shape == (0, 3)
    rng = np.random.default_rng(0)
    for prop in (rng.normal(size=(mesh.size, 3)), rng.normal(size=mesh.size)):
        mesh.addprop("magnetization", prop)
        b, m, idx = active_cells_mag(mesh, None, f)
        # the reference's loop: every cell of the mesh, carved ones are None
        rows, mags = [], []
        for cell in mesh:
            if cell is None or "magnetization" not in cell.props:
                continue
            rows.append(cell.get_bounds())
            v = cell.props["magnetization"]
            mags.append([v * f[0], v * f[1], v * f[2]] if np.ndim(v) == 0 else list(v))
        assert np.array_equal(b, np.array(rows)) and np.array_equal(m, np.array(mags))
        assert len(idx) == mesh.size - len(mask)
    b, m, _ = active_cells_mag(mesh, 2.5, f)     # pmag overrides the property on every kept cell
    assert b.shape[0] == mesh.size - len(mask)
    assert np.array_equal(m, np.tile([2.5 * f[0], 2.5 * f[1], 2.5 * f[2]], (b.shape[0], 1)))


def test_skip_rule_on_a_list_of_prisms():
    from gravinv3dhmc_amd import mesher, utils
    from gravinv3dhmc_amd.gravmag._common import active_cells_mag
    f = utils.dircos(-45.0, 120.0)
    cells = [mesher.Prism(0, 1, 0, 1, 0, 1, props={"magnetization": [1.0, 2.0, 3.0]}),
             None,
             mesher.Prism(1, 2, 0, 1, 0, 1),                                     # no property
             mesher.Prism(2, 3, 0, 1, 0, 1, props={"magnetization": 4.0}),       # an intensity along f
             mesher.Prism(3, 4, 0, 1, 0, 1, props={"density": 1.0})]             # still no magnetization
    b, m, idx = active_cells_mag(cells, None, f)
    assert idx is None
    assert np.array_equal(b, np.array([[0, 1, 0, 1, 0, 1], [2, 3, 0, 1, 0, 1]], float))
    assert np.array_equal(m, np.array([[1.0, 2.0, 3.0], [4.0 * f[0], 4.0 * f[1], 4.0 * f[2]]]))
    b, m, _ = active_cells_mag(cells, [0.5, -1.0, 2.0], f)                     # pmag: only None is skipped
    assert b.shape == (4, 6) and np.array_equal(m, np.tile([0.5, -1.0, 2.0], (4, 1)))
    b, m, _ = active_cells_mag([None, None], None, f)
    assert b.shape == (0, 6) and m.shape == (0, 3)


def test_magnetic_field_on_tesseroids_is_refused():
    import gravinv3dhmc_amd as g
    lon, lat = np.meshgrid(np.linspace(0, 10, 3), np.linspace(-5, 5, 3))
    with pytest.raises(NotImplementedError, match="magnetic"):
        g.GravMagModule(np.zeros(9), (0, 10, -5, 5, 0, -10000), (5000, 5, 5),
                        (lon.ravel(), lat.ravel(), np.full(9, 1000.0)), coordinate="spherical",
                        field="magnetic", verbose=False)
    with pytest.raises(ValueError):
        g.GravMagModule(np.zeros(9), (0, 10, -5, 5, 0, -10000), (5000, 5, 5),
                        (lon.ravel(), lat.ravel(), np.full(9, 1000.0)), field="gravity-gradient", verbose=False)


def test_c_abi_declares_the_total_field_entry_points():
    from gravinv3dhmc_amd import _lib
    assert _lib.CELL_PRISM_TF == 2
    assert {"gh_set_cells_tf", "gh_tf_result"} <= set(_lib.PROTOTYPES)
