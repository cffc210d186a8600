"""Host-side checks of the tesseroid magnetization store on the shift-invariant table: the exports, the sign rule of the
north-south mirror (magvector.mirror_signs -- the library applies the same rule), the index maps of the table restated in
NumPy, and the structure itself on a point-dipole kernel built with tesseroid.local_frame_rotation: the nine entries
under the equatorial reflection, the invariance under a common shift of the longitudes, and the total field's failure to
be a pure sign.  (The tesseroid forward runs on the device: the same signs are asserted against direct evaluation, and
the table against the dense store, in tests/test_gpu_tesseroid_magvec_table.py.)"""
import itertools

import numpy as np
import pytest

BCOMPS = ("bx", "by", "bz")
MRANGE, MSPACING = (-180, 180, -60, 60, 0, -200000), (-100000, 30, 30)


def test_exports():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import magvector
    assert callable(magvector.mirror_signs)
    assert "gh_set_cells_tess_mag_table" in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["gh_set_cells_tess_mag_table"] == _lib.PROTOTYPES["gh_set_cells_tess_mag"]
    assert magvector.TesseroidMagVectorModule._has_table and not magvector.MagVectorModule._has_table
    assert g.TesseroidMagVectorModule is magvector.TesseroidMagVectorModule
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.__file__), "..", "include", "gravhmc.h")).read()
    assert "int gh_set_cells_tess_mag_table(" in header


def test_mirror_signs_for_every_subset():
    from gravinv3dhmc_amd.inversion.magvector import mirror_signs
    sign = {"tf": None, "bx": -1.0, "by": 1.0, "bz": 1.0}
    every = ("tf", "bx", "by", "bz")
    for k in range(1, 5):
        for data in itertools.permutations(every, k):
            cls, axs = mirror_signs(data)
            assert cls == tuple(sign[b] for b in data), data
            assert axs == (-1.0, 1.0, 1.0)
    assert mirror_signs("bx") == ((-1.0,), (-1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="gz"):
        mirror_signs(("bx", "gz"))


def test_index_maps():
    """column -> (axis, cell row, longitude) and stacked row -> (data block, class, slot): the table's entry of (row i,
    column j) sits where the assembly kernel's store layout puts it, and the sweep's j = c n + k addresses the
    property-major model as it is."""
    n, nc1, na1, nb = 12, 8, 4, 3                  # longitudes, rows of cells, (latitude, height) classes, data blocks
    m, P = nc1 * n, na1 * n                         # cells, observation points (one per slot here)
    M, N = 3 * m, nb * P
    ldT = (nb * na1 * n + 15) // 16 * 16
    j = np.arange(M)
    a, row, k = j // m, j % m // n, j % n
    assert np.array_equal(j, a * m + row * n + k)
    c = a * nc1 + row                               # the table's cell row, of nc = 3 nc1
    assert c.max() == 3 * nc1 - 1 and np.array_equal(j, c * n + k)
    i = np.arange(N)
    b, point = i // P, i % P
    cls, slot = point // n, point % n               # (points class-major in this restatement)
    klass = b * na1 + cls
    assert klass.max() == nb * na1 - 1
    # the entry K[i, j] is the table's (row c, class, shift d = slot - k mod n) ...
    ii, jj = np.meshgrid(i, j, indexing="ij")
    d = (slot[ii] - k[jj]) % n
    t_index = c[jj] * ldT + klass[ii] * n + d
    # ... which is the assembly kernel's layout A[(a m' + c') ld + q Nb + l] with m' = nc1 cells of longitude index 0,
    # Nb = na1 n synthetic points l = cls n + d, and ld = ldT
    mp, Nb = nc1, na1 * n
    l = cls[ii] * n + d
    a_index = (a[jj] * mp + row[jj]) * ldT + b[ii] * Nb + l
    assert np.array_equal(t_index, a_index)
    assert t_index.max() < 3 * nc1 * ldT and len(np.unique(t_index)) == 3 * nc1 * nb * na1 * n


def _dipole_kernel(lon_o, lat_o, r_o, lon_c, lat_c, r_c):
    """K[b, a]: component b (north, east, down at the observation) of the field of a point dipole at the cell with unit
    moment along the cell's axis a (north, east, down there), up to a constant"""
    from gravinv3dhmc_amd.gravmag import tesseroid
    no, eo, uo = tesseroid._frame(lon_o, lat_o)
    _, _, uc = tesseroid._frame(lon_c, lat_c)
    r = r_o * uo - r_c * uc
    dist = np.linalg.norm(r)
    rh = r / dist
    T = (3.0 * np.outer(rh, rh) - np.eye(3)) / dist ** 3            # ECEF
    O = np.stack([no, eo, uo], axis=1)                              # columns: the observation's north, east, up
    Q = tesseroid.local_frame_rotation(lon_o, lat_o, lon_c, lat_c)  # cell NED -> observation NEU
    return np.diag([1.0, 1.0, -1.0]) @ (O.T @ T @ O) @ Q


GEOM = dict(lon_o=37.0, lat_o=33.0, r_o=6378137.0 + 250e3, lon_c=21.0, lat_c=48.0, r_c=6378137.0 - 50e3)


def test_the_nine_entries_under_the_equatorial_reflection():
    from gravinv3dhmc_amd.inversion.magvector import mirror_signs
    cls, axs = mirror_signs(BCOMPS)
    K = _dipole_kernel(**GEOM)
    Km = _dipole_kernel(**dict(GEOM, lat_o=-GEOM["lat_o"], lat_c=-GEOM["lat_c"]))
    S = np.outer(cls, axs)
    assert (np.abs(K) > 1e-3 * np.abs(K).max()).all()              # every entry takes part
    assert np.abs(Km - S * K).max() <= 1e-13 * np.abs(K).max()
    # every other assignment of signs to the three components and the three axes fails clearly
    for s in itertools.product((-1.0, 1.0), repeat=6):
        S2 = np.outer(s[:3], s[3:])
        if not np.array_equal(S2, S):
            assert np.abs(Km - S2 * K).max() > 1e-3 * np.abs(K).max(), s


def test_invariance_under_a_common_longitude_shift():
    K = _dipole_kernel(**GEOM)
    for shift in (30.0, -147.5, 211.0):
        Ks = _dipole_kernel(**dict(GEOM, lon_o=GEOM["lon_o"] + shift, lon_c=GEOM["lon_c"] + shift))
        assert np.abs(Ks - K).max() <= 1e-13 * np.abs(K).max()
    # (a shift of one end alone changes every entry: the invariance is not vacuous)
    Kd = _dipole_kernel(**dict(GEOM, lon_o=GEOM["lon_o"] + 30.0))
    assert np.abs(Kd - K).max() > 1e-2 * np.abs(K).max()


def test_the_total_field_is_no_pure_sign_under_the_mirror():
    """tf = f_o . (bx, by, bz): with the same (inc, dec) at the mirrored observation no sign per axis maps the entries --
    why the table is built without the mirror when "tf" is among the data.  (Straight down, tf is bz and has one.)"""
    from gravinv3dhmc_amd.gravmag import tesseroid
    K = _dipole_kernel(**GEOM)
    Km = _dipole_kernel(**dict(GEOM, lat_o=-GEOM["lat_o"], lat_c=-GEOM["lat_c"]))
    f = tesseroid._field_directions(60.0, 10.0, 1)[0]
    tf, tfm = f @ K, f @ Km
    for a in range(3):
        assert min(abs(tfm[a] - tf[a]), abs(tfm[a] + tf[a])) > 1e-3 * np.abs(tf).max(), a
    down = tesseroid._field_directions(90.0, 0.0, 1)[0]
    assert np.abs(down @ Km - np.array([-1.0, 1.0, 1.0]) * (down @ K)).max() <= 1e-13 * np.abs(K).max()


def test_refusals_before_device_work():
    from gravinv3dhmc_amd.inversion import MagVectorModule, TesseroidMagVectorModule as TM
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 180, 30.0), np.array([-45.0, -15.0, 15.0, 45.0]),
                                               indexing="ij")]
    obs = (lon, lat, np.full(lon.size, 250000.0))
    d = [np.zeros(lon.size)] * 2
    NAME = "tesseroid magnetization store"
    for kw in ({"wavelet": "3D"}, {"matrix_free": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match=NAME):
            TM(d, MRANGE, MSPACING, obs, data=("bx", "bz"), shift_invariant=True, verbose=False, **kw)
    # the total field's direction must be one per class of observations, bit for bit
    with pytest.raises(NotImplementedError, match=NAME + ": the total field's direction varies within a class"):
        TM(d, MRANGE, MSPACING, obs, data=("tf", "bz"), mangle=(60.0 + 1e-13 * lon, 10.0), shift_invariant=True,
           verbose=False)
    with pytest.raises(NotImplementedError, match="varies within a class"):
        TM(d, MRANGE, MSPACING, obs, data=("tf", "bz"), mangle=(60.0, 10.0 + 0.01 * lon), shift_invariant=True,
           verbose=False)
    # the dense form keeps its row limit and says where there is none
    n = 5462
    x = np.linspace(-170, 170, n)
    with pytest.raises(NotImplementedError, match=NAME + " takes at most 16384"):
        TM([np.zeros(n)] * 3, MRANGE, MSPACING, (x, np.zeros(n), np.full(n, 250000.0)), verbose=False)
    # the prism stores have no table
    for data in (("tf",), BCOMPS):
        dd = np.zeros(4) if data == ("tf",) else [np.zeros(4)] * 3
        with pytest.raises(NotImplementedError, match="shift-invariant"):
            MagVectorModule(dd, (0, 1, 0, 1, 0, 1), (1, 1, 1), (np.zeros(4), np.zeros(4), np.zeros(4)), data=data,
                            shift_invariant=True, verbose=False)


def test_class_directions_take_the_first_of_each_class():
    from gravinv3dhmc_amd.gravmag import tesseroid
    from gravinv3dhmc_amd.inversion import TesseroidMagVectorModule as TM
    lat = np.array([10.0, -10.0, 10.0, -10.0, 10.0])
    h = np.array([1.0, 1.0, 1.0, 1.0, 2.0])
    inc = np.array([50.0, 40.0, 50.0, 40.0, 30.0])
    f = tesseroid._field_directions(inc, 5.0, 5)
    out = TM._class_directions(f, (inc, 5.0), (np.zeros(5), lat, h))
    assert np.array_equal(out, f)
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[1], out[3])
