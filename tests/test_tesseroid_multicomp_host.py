"""Host-side checks of the tesseroid multi-component inversion (TesseroidMultiComponentModule): exports, the argument
validation and the refusals decided before a device is touched, and the default ratios.  (The sign table of the
north-south mirror is asserted against direct evaluation in tests/test_gpu_tesseroid_multicomp.py: the tesseroid
forward runs on the device.)"""
import numpy as np
import pytest

MRANGE, MSPACING = (-180, 180, -60, 60, 0, -200000), (-100000, 30, 30)


def _args(c=2):
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 180, 30.0), np.array([-45.0, -15.0, 15.0, 45.0]),
                                               indexing="ij")]
    rng = np.random.default_rng(0)
    return [rng.normal(size=lon.size) for _ in range(c)], (lon, lat, np.full(lon.size, 250000.0))


def test_exports():
    import gravinv3dhmc_amd as g
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.inversion import MultiComponentModule, TesseroidMultiComponentModule
    assert g.TesseroidMultiComponentModule is TesseroidMultiComponentModule
    assert "TesseroidMultiComponentModule" in g.__all__
    assert issubclass(TesseroidMultiComponentModule, MultiComponentModule)
    assert _lib.CELL_TESSEROID_MULTI == 10
    assert "gh_set_cells_tess_multi" in _lib.PROTOTYPES
    assert hasattr(g.Engine, "set_cells_tess_multi")
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.__file__), "..", "include", "gravhmc.h")).read()
    assert "GH_CELL_TESSEROID_MULTI = 10" in header and "int gh_set_cells_tess_multi(" in header


def test_argument_validation():
    from gravinv3dhmc_amd.inversion import TesseroidMultiComponentModule as TM
    d, obs = _args()
    with pytest.raises(ValueError, match="empty"):
        TM([], MRANGE, MSPACING, obs, components=(), verbose=False)
    with pytest.raises(ValueError, match="gzx"):
        TM(d, MRANGE, MSPACING, obs, components=("gz", "gzx"), verbose=False)
    with pytest.raises(ValueError, match="distinct"):
        TM(d, MRANGE, MSPACING, obs, components=("gzz", "gzz"), verbose=False)
    with pytest.raises(ValueError):
        TM(d[:1], MRANGE, MSPACING, obs, components=("gz", "gzz"), verbose=False)       # one vector, two components
    with pytest.raises(ValueError):
        TM([d[0], d[1][:-1]], MRANGE, MSPACING, obs, components=("gz", "gzz"), verbose=False)   # length mismatch
    with pytest.raises(ValueError):
        TM({"gz": d[0], "gxx": d[1]}, MRANGE, MSPACING, obs, components=("gz", "gzz"), verbose=False)
    for w in ("var", (1.0,), (1.0, -2.0), (1.0, 0.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            TM(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), weights=w, verbose=False)
    for r in (0.0, -1.0, (1.6, 0.0), (1.6,), (1.6, 8.0, 8.0)):
        with pytest.raises(ValueError):
            TM(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), ratio=r, verbose=False)
    with pytest.raises(TypeError):
        TM(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), topo=None, verbose=False)
    with pytest.raises(TypeError):
        TM(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), coordinate="cartesian", verbose=False)


def test_refusals_before_device_work():
    from gravinv3dhmc_amd.inversion import TesseroidMultiComponentModule as TM
    d, obs = _args()
    for kw in ({"wavelet": "1D"}, {"wavelet": "3D"}, {"matrix_free": True}, {"shard": object()}):
        with pytest.raises(NotImplementedError, match="tesseroid multi-component store"):
            TM(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), verbose=False, **kw)
    # more stacked rows than the fused sweep holds: refused with the limit, and told where there is none
    n = 8193
    x = np.linspace(-170, 170, n)
    big = [np.arange(n, dtype=float), np.arange(n, dtype=float)]
    with pytest.raises(NotImplementedError, match="tesseroid multi-component store takes at most 16384.*shift_invariant"):
        TM(big, MRANGE, MSPACING, (x, np.zeros(n), np.full(n, 250000.0)), components=("gz", "gzz"), verbose=False)


def test_the_old_refusals_stay():
    from gravinv3dhmc_amd.inversion import GravMagModule, MultiComponentModule
    d, obs = _args()
    with pytest.raises(NotImplementedError, match="multi-component store"):
        MultiComponentModule(d, MRANGE, MSPACING, obs, components=("gz", "gzz"), coordinate="spherical", verbose=False)
    with pytest.raises(NotImplementedError, match="multi-component store"):
        MultiComponentModule(d, (0, 1, 0, 1, 0, 1), (1, 1, 1), obs, components=("gz", "gzz"), shift_invariant=True,
                             verbose=False)
    with pytest.raises(NotImplementedError, match="gz only"):
        GravMagModule(d[0], MRANGE, MSPACING, obs, coordinate="spherical", component="gzz", verbose=False)


def test_default_ratios_are_the_reference_s_per_field():
    from gravinv3dhmc_amd.gravmag import tesseroid
    from gravinv3dhmc_amd.inversion.multicomp import _default_ratio
    assert (tesseroid.RATIO_V, tesseroid.RATIO_G, tesseroid.RATIO_GG) == (1, 1.6, 8)
    for c in ("potential", "geoid"):
        assert _default_ratio(c) == tesseroid.RATIO_V
    for c in ("gx", "gy", "gz"):
        assert _default_ratio(c) == tesseroid.RATIO_G
    for c in ("gxx", "gxy", "gxz", "gyy", "gyz", "gzz"):
        assert _default_ratio(c) == tesseroid.RATIO_GG
    # the defaults of the forward functions themselves
    import inspect
    for c in ("potential", "geoid", "gx", "gy", "gz", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz"):
        assert inspect.signature(getattr(tesseroid, c)).parameters["ratio"].default == _default_ratio(c), c
