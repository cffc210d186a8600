"""Host-side checks of the tesseroid magnetic fields (gravmag.tesseroid.bx / by / bz / tf, TesseroidMagVectorModule,
GH_CELL_TESS_MVI_DATA): the rotation between local frames, exports and signatures, the C ABI's symbols, and the
argument validation and refusals decided before a device is touched."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BCOMPS = ("bx", "by", "bz")


# ----------------------------------------------------------------------------- local_frame_rotation

def test_rotation_is_orthogonal_and_proper_between_like_handed_frames():
    from gravinv3dhmc_amd.gravmag.tesseroid import local_frame_rotation
    rng = np.random.default_rng(0)
    k = 50
    Q = local_frame_rotation(rng.uniform(-180, 180, k), rng.uniform(-90, 90, k), rng.uniform(-180, 180, k),
                             rng.uniform(-90, 90, k))
    assert Q.shape == (k, 3, 3)
    eye = np.einsum("kij,klj->kil", Q, Q)
    assert np.abs(eye - np.eye(3)).max() <= 1e-14
    # (n, e, -u) is right-handed, (n, e, u) left-handed: Q takes north-east-DOWN at the cell to north-east-UP at the
    # observation, so det Q = -1, and between like-handed frames -- N, E, D -> x, y, -z -- the determinant is +1
    assert np.abs(np.linalg.det(Q) + 1.0).max() <= 1e-14
    assert np.abs(np.linalg.det(np.diag([1.0, 1.0, -1.0]) @ Q) - 1.0).max() <= 1e-14
    # broadcasting: observations against one cell, and scalars
    assert local_frame_rotation(np.zeros(4), np.zeros(4), 1.0, 2.0).shape == (4, 3, 3)
    assert local_frame_rotation(0.0, 0.0, 1.0, 2.0).shape == (3, 3)


def test_rotation_at_the_cell_itself_turns_down_into_up():
    """o = c: north and east coincide, the cell's down axis is minus the observation's up axis -- Q = diag(1, 1, -1),
    the identity in the N, E, D -> x, y, -z sense"""
    from gravinv3dhmc_amd.gravmag.tesseroid import local_frame_rotation
    for lon, lat in ((0.0, 0.0), (37.0, -52.0), (-179.5, 89.0), (180.0, -89.9)):
        Q = local_frame_rotation(lon, lat, lon, lat)
        assert np.abs(Q - np.diag([1.0, 1.0, -1.0])).max() <= 1e-15, (lon, lat)


def test_rotation_matches_hand_written_cases():
    from gravinv3dhmc_amd.gravmag.tesseroid import local_frame_rotation
    # across the date line on the equator: o at lon 179, c at lon -179 -- 2 degrees apart about the polar axis.
    # n_o = n_c = z; e and u turn by 2 degrees in the equatorial plane.
    a = np.deg2rad(2.0)
    Q = local_frame_rotation(179.0, 0.0, -179.0, 0.0)
    # The cell lies EAST of the observation: its up vector leans east as seen from o (u_c . e_o = sin a), and its east
    # vector dips below o's horizon (e_c . u_o = -sin a).
    want = np.array([[1.0, 0.0, 0.0],
                     [0.0, np.cos(a), -np.sin(a)],         # e_o . e_c = cos a,  e_o . (-u_c) = -sin a
                     [0.0, -np.sin(a), -np.cos(a)]])       # u_o . e_c = -sin a,  u_o . (-u_c) = -cos a
    assert np.abs(Q - want).max() <= 1e-14
    # the same two longitudes the short way round give the same matrix as 179 -> 181
    assert np.abs(Q - local_frame_rotation(179.0, 0.0, 181.0, 0.0)).max() <= 1e-14
    # pole-adjacent: o at (0, 89), c at (180, 89): across the pole, 2 degrees apart along the meridian plane.
    # North at o points to the pole, north at c too -- from the other side: n_o . n_c = -cos 2deg, e_o = -e_c.
    Q = local_frame_rotation(0.0, 89.0, 180.0, 89.0)
    want = np.array([[-np.cos(a), 0.0, -np.sin(a)],        # n_o . (-u_c) = -sin a
                     [0.0, -1.0, 0.0],
                     [np.sin(a), 0.0, -np.cos(a)]])        # u_o . n_c = sin a,  u_o . (-u_c) = -cos a
    assert np.abs(Q - want).max() <= 1e-14


# ----------------------------------------------------------------------------- exports, signatures, the ABI

def test_public_names_and_signatures():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import inversion
    from gravinv3dhmc_amd.gravmag import tesseroid
    assert g.TesseroidMagVectorModule is inversion.TesseroidMagVectorModule and "TesseroidMagVectorModule" in g.__all__
    assert issubclass(g.TesseroidMagVectorModule, g.MagVectorModule)
    want = ["lon", "lat", "height", "model", "pmag", "ratio", "njobs", "pool", "return_kernel", "device"]
    for name in BCOMPS:
        sig = inspect.signature(getattr(tesseroid, name))
        assert list(sig.parameters) == want, name
        assert [sig.parameters[k].default for k in want[4:]] == [None, tesseroid.RATIO_GG, 1, None, True, 0]
    sig = inspect.signature(tesseroid.tf)
    assert list(sig.parameters) == want[:4] + ["inc", "dec"] + want[4:]
    assert callable(tesseroid.local_frame_rotation)
    sig = inspect.signature(g.TesseroidMagVectorModule.__init__)
    assert sig.parameters["data"].default == ("bx", "by", "bz") and sig.parameters["weights"].default is None
    assert sig.parameters["amplitude"].default == 0.0 and "coordinate" not in sig.parameters
    for name in ("set_cells_tess_mag", "tess_b_result"):
        assert callable(getattr(g.Engine, name))
    for name in ("HMCSample", "misfit_and_grad", "forward", "kernel", "block_means", "Amplitude", "amplitude", "direction",
                 "to_vectors", "from_vectors"):
        assert hasattr(g.TesseroidMagVectorModule, name) or hasattr(g, name), name


def test_abi_symbols_and_enum_values():
    from gravinv3dhmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gravhmc.h")).read()
    assert _lib.CELL_TESS_MVI_DATA == 9 and re.search(r"GH_CELL_TESS_MVI_DATA = 9\b", header)
    # (a new value: none of the earlier ones moved)
    assert re.search(r"GH_CELL_PRISM_MULTI = 6, GH_CELL_PRISM_MVI = 7, GH_CELL_PRISM_MVI_DATA = 8", header)
    assert (_lib.CELL_PRISM, _lib.CELL_TESSEROID, _lib.CELL_PRISM_MVI, _lib.CELL_PRISM_MVI_DATA) == (0, 1, 7, 8)
    for sym, nargs in (("gh_set_cells_tess_mag", 7), ("gh_tess_b_result", 4)):
        assert re.search(r"\bint %s\(gh_ctx \*ctx" % sym, header), sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs
    src = open(os.path.join(ROOT, "gravinv3dhmc_amd", "csrc", "gravhmc.hip")).read()
    assert '#include "tessmag.hip.h"' in src
    kern = open(os.path.join(ROOT, "gravinv3dhmc_amd", "csrc", "tessmag.hip.h")).read()
    for name in ("tess_mag_kernel", "tess_mag_result_kernel", "tess_mag_cellframe_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % name, kern), name


# ----------------------------------------------------------------------------- validation before any device work

@pytest.fixture
def no_device(monkeypatch):
    """Engine raises: a call that gets as far as the device fails the test with this error"""
    import gravinv3dhmc_amd.gravmag.tesseroid as tess
    import gravinv3dhmc_amd.inversion.magvector as mvmod

    class Touched(AssertionError):
        pass

    def boom(*a, **k):
        raise Touched("device work started")

    monkeypatch.setattr(mvmod, "Engine", boom)
    monkeypatch.setattr(tess, "Engine", boom)
    return Touched


def _mesh(vectors=True):
    import gravinv3dhmc_amd as g
    mesh = g.mesher.TesseroidMesh((-10, 10, 40, 50, 0, -40000), (-20000, 5, 5))
    if vectors:
        mesh.addprop("magnetization", np.ones((mesh.size, 3)))
    return mesh


def test_field_functions_validate_before_device_work(no_device):
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd.gravmag import tesseroid
    mesh = _mesh()
    x = np.linspace(0, 5, 6)
    h = np.full(6, 300e3)
    for name in BCOMPS + ("tf",):
        fn = getattr(tesseroid, name)
        extra = (60.0, 5.0) if name == "tf" else ()
        with pytest.raises(AssertionError, match="same shape"):
            fn(x, x[:-1], h, mesh, *extra)
        with pytest.raises(AssertionError, match="ratio"):
            fn(x, x, h, mesh, *extra, ratio=0)
        with pytest.raises(AssertionError, match="jobs"):
            fn(x, x, h, mesh, *extra, njobs=0)
        with pytest.raises(ValueError, match="pmag"):
            fn(x, x, h, mesh, *extra, pmag=2.5)
        with pytest.raises(ValueError, match="magnetization"):              # no cell has the property
            fn(x, x, h, _mesh(vectors=False), *extra)
        scalar = _mesh(vectors=False)
        scalar.addprop("magnetization", np.ones(scalar.size))               # intensities: there is no field to put them along
        with pytest.raises(ValueError, match="vector"):
            fn(x, x, h, scalar, *extra)
        bad = [g.mesher.Tesseroid(0, 1, 0, 1, 0, -1000, props={"magnetization": (1, 0, 0)})]
        bad[0].e = -1.0
        with pytest.raises(AssertionError, match="Invalid tesseroid dimensions"):
            fn(x, x, h, bad, *extra)
        tiny = [g.mesher.Tesseroid(0, 1e-7, 0, 1, 0, -1000, props={"magnetization": (1, 0, 0)})]
        with pytest.warns(RuntimeWarning, match="Ignoring this tesseroid"), pytest.raises(ValueError, match="threshold"):
            fn(x, x, h, tiny, *extra)
        with pytest.raises(no_device):
            fn(x, x, h, mesh, *extra)
    for inc, dec in ((np.zeros(5), 0.0), (0.0, np.zeros(7))):
        with pytest.raises(ValueError, match="per observation"):
            tesseroid.tf(x, x, h, mesh, inc, dec)
    with pytest.raises(no_device):
        tesseroid.tf(x, x, h, mesh, np.full(6, 60.0), np.linspace(-5, 5, 6))


def _args(n=6, ncomp=3):
    rng = np.random.default_rng(0)
    lon, lat = np.linspace(-8, 8, n), np.linspace(41, 49, n)
    return ([rng.normal(size=n) for _ in range(ncomp)], (-10, 10, 40, 50, 0, -40000), (-20000, 5, 5),
            (lon, lat, np.full(n, 300e3)))


def test_module_value_errors_before_device_work(no_device):
    from gravinv3dhmc_amd import TesseroidMagVectorModule as TM
    d, mrange, mspacing, obs = _args()
    for data in (("bx", "gz", "bz"), ("bx", "by", "bx"), (), ("b",)):
        with pytest.raises(ValueError):
            TM(d[:len(data)], mrange, mspacing, obs, data=data, verbose=False)
    with pytest.raises(ValueError):                                       # the wrong count
        TM(d[:2], mrange, mspacing, obs, verbose=False)
    with pytest.raises(ValueError):                                       # the wrong length
        TM([d[0], d[1][:-1], d[2]], mrange, mspacing, obs, verbose=False)
    with pytest.raises(ValueError):                                       # a dict with other keys
        TM({"bx": d[0], "by": d[1], "tf": d[2]}, mrange, mspacing, obs, verbose=False)
    for w in ("var", [1.0, 2.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError):
            TM(d, mrange, mspacing, obs, weights=w, verbose=False)
    with pytest.raises(ValueError):
        TM(d, mrange, mspacing, obs, amplitude=-1.0, verbose=False)
    with pytest.raises(ValueError):                                       # per-observation angles of the wrong length
        TM(d[:1], mrange, mspacing, obs, data=("tf",), mangle=(np.zeros(5), 0.0), verbose=False)
    with pytest.raises(ValueError):
        TM(d, mrange, mspacing, obs, ratio=0.0, verbose=False)
    with pytest.raises(TypeError):
        TM(d, mrange, mspacing, obs, topo=None, verbose=False)
    # valid arguments do reach the device: the guard itself works
    with pytest.raises(no_device):
        TM(d, mrange, mspacing, obs, verbose=False)
    with pytest.raises(no_device):
        TM({"bz": d[0], "tf": d[1]}, mrange, mspacing, obs, data=("tf", "bz"), weights="std",
           mangle=(np.full(6, 60.0), 3.0), verbose=False)
    with pytest.raises(no_device):
        TM(d[:1], mrange, mspacing, obs, data="tf", mangle=(60.0, 3.0), verbose=False)


def test_module_refusals_name_the_store(no_device):
    from gravinv3dhmc_amd import MagVectorModule as MV, TesseroidMagVectorModule as TM
    d, mrange, mspacing, obs = _args()
    for kw in ({"wavelet": "1D"}, {"matrix_free": True}, {"shift_invariant": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match="the tesseroid magnetization store"):
            TM(d, mrange, mspacing, obs, verbose=False, **kw)
        with pytest.raises(NotImplementedError, match="the tesseroid magnetization store"):
            TM(d[:1], mrange, mspacing, obs, data=("tf",), verbose=False, **kw)
    n = 5462                                                              # 3 x 5462 = 16386 stacked rows
    x = np.linspace(-8, 8, n)
    with pytest.raises(NotImplementedError, match="16384.*tesseroid magnetization store|tesseroid.*16384"):
        TM([np.zeros(n)] * 3, mrange, mspacing, (x, x + 45, np.zeros(n)), verbose=False)
    # the prism module keeps refusing the spherical case, naming its own stores
    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        MV(d, mrange, mspacing, obs, data=BCOMPS, coordinate="spherical", verbose=False)
    with pytest.raises(NotImplementedError, match="the magnetization-vector store"):
        MV(d[0], mrange, mspacing, obs, coordinate="spherical", verbose=False)


def test_hmcsamplebatch_refuses_the_store_by_name():
    import gravinv3dhmc_amd as g

    class _E:
        mvi = True
        multi = 3
        tess_mag = True

    class _M:
        _engine = _E()

    with pytest.raises(NotImplementedError, match="tesseroid magnetization store"):
        g.HMCSampleBatch(_M(), 2, 1, 0, 0.01, [1, 2], np.zeros((2, 3)), np.zeros(3), np.zeros((3, 2)), "mandatory",
                         1000, np.zeros(2), "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)
