"""Host-side checks of the joint gravity-magnetic inversion (JointModule): exports, the refusals that fire
before any device work, the fixtures' shapes and the block-diagonal finite-difference operator."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import gold


def test_joint_exports():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import JointModule
    assert g.JointModule is JointModule
    assert "JointModule" in g.__all__
    assert _lib.CELL_PRISM_JOINT == 5
    assert all(f in _lib.PROTOTYPES for f in ("gh_set_cells_joint", "gh_joint_std", "gh_joint_layout"))


def _args(n=6):
    x = np.linspace(0, 2000, n)
    return (np.zeros(n), np.zeros(n), (0, 2000, 0, 3000, 0, 900), (300, 750, 500), (x, x.copy(), np.zeros(n)))


def test_joint_refusals_before_device_work():
    from gravinv3dhmc_amd.inversion import JointModule
    gz, tf, mrange, mspacing, obs = _args()
    with pytest.raises(NotImplementedError):
        JointModule(gz, tf, mrange, mspacing, obs, coordinate="spherical", verbose=False)
    for wv in ("1D", "3D"):
        with pytest.raises(NotImplementedError):
            JointModule(gz, tf, mrange, mspacing, obs, wavelet=wv, verbose=False)
    with pytest.raises(ValueError):
        JointModule(gz, tf[:-1], mrange, mspacing, obs, verbose=False)
    with pytest.raises(ValueError):
        JointModule(gz[:-1], tf[:-1], mrange, mspacing, obs, verbose=False)
    with pytest.raises(ValueError):
        JointModule(gz, tf, mrange, mspacing, obs, coordinate="polar", verbose=False)


def test_joint_fixture_shapes():
    z = gold("joint_small.npz")
    for g in ("a", "b"):
        n = z[g + "_xp"].size
        shape = tuple(int(v) for v in z[g + "_shape"])
        m = int(np.prod(shape))
        assert z[g + "_Aw"].shape == (2 * n, 2 * m)
        assert z[g + "_A"].shape == (2 * n, 2 * m)
        assert z[g + "_wm"].shape == (2 * m,) and z[g + "_wb"].shape == (2 * n,)
        assert z[g + "_dobsw"].shape == (2 * n,)
        # the zero blocks of the stacked layout
        assert not z[g + "_Aw"][:n, m:].any() and not z[g + "_Aw"][n:, :m].any()
        for reg in ("Damping", "MS", "Smoothness", "TV"):
            assert z[g + "_" + reg + "_grad"].shape == (3, 2 * m)
            assert z[g + "_" + reg + "_dpre"].shape == (3, 2 * n)
    # geometry b: n not a multiple of 16, an odd number of cells on every axis
    assert z["b_xp"].size % 16 != 0 and all(int(v) % 2 == 1 for v in z["b_shape"])
    c = gold("chain_small_joint.npz")
    for tag in ("a", "b"):
        assert len(c[tag + "_lines"]) > 0
        assert c[tag + "_model"].shape[-1] == z["a_wm"].size


def test_fd3djoint_matches_reference_operator():
    """fd3djoint against the reference's own fd3djoint, stored for the two fixture meshes."""
    from gravinv3dhmc_amd.inversion import JointModule
    jm = object.__new__(JointModule)   # (fd3djoint needs no device state)
    z = gold("joint_small.npz")
    for g in ("a_", "b_"):
        ref = sp.csr_matrix((z[g + "fd3djoint_data"], z[g + "fd3djoint_indices"], z[g + "fd3djoint_indptr"]),
                            shape=tuple(z[g + "fd3djoint_shape"]))
        J = jm.fd3djoint(tuple(int(v) for v in z[g + "shape"]))
        assert J.shape == ref.shape
        assert (J != ref).nnz == 0


def test_fd3djoint_is_block_diagonal():
    from gravinv3dhmc_amd.inversion import JointModule
    from gravinv3dhmc_amd.inversion.joint import fd3d
    jm = object.__new__(JointModule)   # (fd3djoint needs no device state)
    for shape in ((3, 4, 4), (3, 5, 7), (1, 1, 3), (2, 1, 1)):
        R = fd3d(shape)
        J = jm.fd3djoint(shape)
        assert J.shape == (2 * R.shape[0], 2 * R.shape[1])
        assert (J != sp.block_diag([R, R], format="csr")).nnz == 0


def test_fd3d_rows_are_neighbour_differences():
    from gravinv3dhmc_amd.inversion.joint import fd3d
    nz, ny, nx = 3, 5, 7
    R = fd3d((nz, ny, nx)).toarray()
    assert R.shape == (((nx - 1) * ny + (ny - 1) * nx) * nz + nx * ny * (nz - 1), nx * ny * nz)
    assert np.all(R.sum(axis=1) == 0) and np.all((R == 1).sum(axis=1) == 1)
    # the first row of a layer: x difference of its first two cells; the first z row: layer 0 minus layer 1
    assert R[0, 0] == 1 and R[0, 1] == -1
    zrow = ((nx - 1) * ny + (ny - 1) * nx) * nz
    assert R[zrow, 0] == 1 and R[zrow, nx * ny] == -1
