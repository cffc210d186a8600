"""CPU suite: the oracle against the golden vectors generated from the reference
(oracle/make_golden.py) and against the reference's committed run logs."""
import numpy as np

from conftest import gold
from helpers import relmax
from oracle import oracle


def test_prism_entries_bit_exact():
    g = gold("prism_cases.npz")
    K = oracle.prism_gz_kernel(g["xp"], g["yp"], g["zp"], g["cells"])
    assert np.array_equal(K, g["K"])  # same libm, same operation order as _prism.pyx


def test_c1_kernel_spot_values():
    from helpers import c1_inputs
    g = gold("c1_spot.npz")
    mesh, xp, yp, zp = c1_inputs()
    K = oracle.prism_gz_kernel(xp, yp, zp, mesh.cell_bounds())
    assert np.array_equal(K[g["ii"], g["jj"]], g["Kij"])
    assert np.array_equal(K[:, 0], g["K_col0"]) and np.array_equal(K[0, :], g["K_row0"])
    np.testing.assert_allclose(np.sqrt((K ** 2).sum(0)), g["colnorm"], rtol=1e-14)
    gz = K @ g["rho"]
    assert relmax(gz, g["gz"]) < 1e-12  # the reference accumulates per corner before scaling
    # SURVEY 8c scalar goldens
    assert K[0, 0] == 0.6468726475750967 and K[0, 5999] == 0.00012912876871222398
    assert abs(np.linalg.norm(K) - 41.533528108117984) < 1e-12


def test_uniformgrid_log_initial_mw():
    """`initial mw` of example/uniformgrid/logout_T1.txt:29-31: 0.001 * column norms with the
    2-decimal observation file."""
    from gravinv3dhmc_amd import mesher
    e = gold("example_inputs.npz")
    obs = e["uni_obs"]
    mesh = mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    K = oracle.prism_gz_kernel(obs[:, 0], obs[:, 1], obs[:, 2], mesh.cell_bounds())
    _, wm = oracle.col_weight(K)
    mw = 0.001 * wm
    np.testing.assert_allclose(mw[:3], e["uni_initial_mw_head"], rtol=5e-9)
    np.testing.assert_allclose(mw[-3:], e["uni_initial_mw_tail"], rtol=5e-9)


def test_tesseroid_entries():
    g = gold("tess_cases.npz")
    K, info = oracle.tess_gz_kernel(g["lon"], g["lat"], g["h"], g["bounds"], return_info=True)
    assert relmax(K, g["K"]) < 1e-13
    assert info["leaves"] == int(g["leaves"])
    assert relmax(K @ g["rho"], g["gz"]) < 1e-12
    Kn, info = oracle.tess_gz_kernel(g["n_lon"], g["n_lat"], g["n_h"], g["n_cells"], return_info=True)
    assert relmax(Kn, g["n_K"]) < 1e-13
    assert info["err_cells"] == int((g["n_err"] != 0).sum()) and info["leaves"] == int(g["n_leaves"])


def test_weighting_and_potential():
    g = gold("potential_small.npz")
    from gravinv3dhmc_amd import mesher
    mesh = mesher.PrismMesh(tuple(g["mrange"]), tuple(g["mspacing"]))
    K = oracle.prism_gz_kernel(g["xp"], g["yp"], g["zp"], mesh.cell_bounds())
    Aw, wm = oracle.col_weight(K)
    assert relmax(Aw, g["Aw"]) < 1e-15 and relmax(wm, g["wm"]) < 1e-15
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        for tag, gf in (("", None), ("_fix", g["gfix"])):
            P = oracle.Problem(Aw, g["dobs"], g["mwapr"], reg, float(g["alpha"]), float(g["beta"]),
                               wm=wm, shape=g["shape"], grav_fix=gf)
            for i, x in enumerate(g["xs"]):
                m, grad, dpre, dv, mv = P.misfit_and_grad(x)
                assert abs(m - g[reg + tag + "_misfit"][i]) <= 1e-13 * abs(m)
                assert relmax(grad, g[reg + tag + "_grad"][i]) < 1e-13
                assert relmax(dpre, g[reg + tag + "_dpre"][i]) < 1e-13
                assert abs(dv - g[reg + tag + "_data"][i]) <= 1e-13 * abs(dv)
                assert abs(mv - g[reg + tag + "_model"][i]) <= 1e-13 * abs(mv)


def test_stencil_matches_fd3d_operator():
    """The regulariser stencil against an explicit copy of the reference's fd3d matrix."""
    rng = np.random.default_rng(3)
    shape = (3, 4, 5)
    M = int(np.prod(shape))
    R = oracle.fd3d_dense(shape)
    mw, apr = rng.normal(size=M), rng.normal(size=M)
    v = mw - apr
    val, grad = oracle.regulariser("Smoothness", mw, apr, shape=shape)
    np.testing.assert_allclose(val, (R @ v) @ (R @ v), rtol=1e-13)
    np.testing.assert_allclose(grad, 2 * R.T @ R @ v, rtol=1e-12, atol=1e-13)
    t = R @ v
    s = np.sqrt(t ** 2 + 0.01)
    val, grad = oracle.regulariser("TV", mw, apr, beta=0.01, shape=shape)
    np.testing.assert_allclose(val, s.sum(), rtol=1e-13)
    np.testing.assert_allclose(grad, R.T @ (t / s), rtol=1e-12, atol=1e-13)


def test_leapfrog_trajectories():
    g = gold("leapfrog_small.npz")
    p = gold("potential_small.npz")
    n_acc = n_clamp = 0
    for i in range(int(g["n"])):
        k = lambda s: g["%d_%s" % (i, s)]
        P = oracle.Problem(p["Aw"], p["dobs"], k("mwapr"), str(k("reg")), 1.0, 0.001, wm=p["wm"],
                           shape=p["shape"])
        x, acc, out, dsyn = P.leapfrog(k("x_in"), k("p0"), float(k("dt")), int(k("L")), k("low"),
                                       k("high"), float(k("u")))
        assert acc == bool(k("acc"))
        assert relmax(x, k("x_out")) < 1e-12
        assert abs(out[0] - float(k("U"))) <= 1e-12 * abs(out[0])
        assert abs(out[1] - float(k("Ud"))) <= 1e-12 * abs(out[1])
        assert relmax(dsyn, k("dsyn")) < 1e-12
        n_acc += acc
        n_clamp += bool(((x == k("low")) | (x == k("high"))).any())
    assert 0 < n_acc < int(g["n"]) and n_clamp > 0  # both branches and the bounds are exercised


def _run_chain(P, wm, x, low, high, dt, Lrange, Sigma, seed, n, N, M, alpha=1.0):
    """The reference's sample loop (hmc.py:295-343) around oracle trajectories."""
    np.random.seed(seed)
    rows, i = [], 0
    while i < n:
        L = np.random.randint(Lrange[0], Lrange[1] + 1)
        p0 = np.random.randn(M) * Sigma
        u = np.random.rand()
        x, acc, out, _ = P.leapfrog(x, p0, dt, L, low, high, u)
        rows.append((out[1] / N + alpha * out[2] / M, out[1] / N, out[2] / M, acc))
        i += acc
    return np.array(rows), x


def test_c1_chain_rows():
    """First rows of misfit.dat of the reference run on C1 + Damping."""
    from helpers import c1_inputs
    g = gold("c1_chain.npz")
    mesh, xp, yp, zp = c1_inputs()
    Aw, wm = oracle.col_weight(oracle.prism_gz_kernel(xp, yp, zp, mesh.cell_bounds()))
    M, N = wm.size, xp.size
    P = oracle.Problem(Aw, g["dobs"], 0.001 * wm, "Damping", 1.0, 0.001, wm=wm)
    rows, x = _run_chain(P, wm, 0.001 * wm, 0.0 * wm, 1.0 * wm, 0.01, [5, 20], 0.001, 100, 5, N, M)
    ref = g["misfit"]
    np.testing.assert_allclose(rows[:, 1] * N, ref[:, 1], rtol=1e-7)   # files hold 8 decimals
    np.testing.assert_allclose(rows[:, 2] * M, ref[:, 2], rtol=1e-7)
    np.testing.assert_allclose(x / wm, g["model_last"], atol=2e-8)


def test_realdata_log_lines():
    """example/realdata/logout_T0.txt chain 0 and 1: tesseroid kernel on the carved segment
    mesh + weighting + Damping + fixed cells + NumPy legacy RNG, all printed digits."""
    from gravinv3dhmc_amd import mesher
    e = gold("example_inputs.npz")
    obs, topo = e["real_obs"], e["real_topo"]
    mesh = mesher.TesseroidMeshSegment((106.5, 118.5, 16, 28, 2000, -60000),
                                       ([-1000, -2000, -5000], 0.5, 0.5),
                                       [2000, -5000, -15000, -60000])
    mask = mesh.carvetopo(topo[:, 0], topo[:, 1], topo[:, 2])
    b = mesh.cell_bounds()
    assert b.shape == (10427, 6)
    K = oracle.tess_gz_kernel(obs[:, 0], obs[:, 1], obs[:, 2], b)
    Aw, wm = oracle.col_weight(K)
    N, M = Aw.shape
    init = 0.01 * wm
    np.testing.assert_allclose(init[:3], e["real_T0_initial_mw_head"], rtol=5e-8)
    np.testing.assert_allclose(init[-3:], e["real_T0_initial_mw_tail"], rtol=5e-8)
    keep = np.ones(mesh.size, bool)
    keep[np.array(mask)] = False
    prior = e["real_aprior"][keep] * wm            # utils.rho2carve + Wm @ aprior
    P = oracle.Problem(Aw, obs[:, 3], prior, "Damping", 1.0, 0.01, wm=wm, grav_fix=e["real_gravsea"])
    for rank, key, n in ((0, "real_T0_chain0", 6), (1, "real_T0_chain1", 3)):
        rows, _ = _run_chain(P, wm, init, -0.5 * wm, 0.5 * wm, 0.01, [5, 20], 0.01, 100 + rank, n, N, M)
        ref = e[key][:len(rows)]
        assert np.all(rows[:, 3] == 1)
        np.testing.assert_allclose(rows[:, 0], ref[:, 0], atol=6e-8 * 10, rtol=2e-10)
        np.testing.assert_allclose(rows[:, 1], ref[:, 1], atol=6e-8 * 10, rtol=2e-10)
        np.testing.assert_allclose(rows[:, 2], ref[:, 3], atol=6e-8 * 10, rtol=2e-10)


def test_numpy_port_matches_oracle():
    """The NumPy/BLAS mirror used as bench.py's cpu_baseline equals the pinned C oracle."""
    from oracle.numpy_port import NumpyProblem
    p = gold("potential_small.npz")
    g = gold("leapfrog_small.npz")
    for i in range(int(g["n"])):
        k = lambda s: g["%d_%s" % (i, s)]
        reg = str(k("reg"))
        if reg not in ("Damping", "MS"):
            continue
        P = NumpyProblem(p["Aw"], p["dobs"], k("mwapr"), reg, 1.0, 0.001, wm=p["wm"])
        x, acc, out, dsyn = P.leapfrog(k("x_in"), k("p0"), float(k("dt")), int(k("L")), k("low"),
                                       k("high"), float(k("u")))
        assert acc == bool(k("acc")) and relmax(x, k("x_out")) < 1e-12
        assert abs(out[0] - float(k("U"))) <= 1e-12 * abs(out[0])


def test_wavelet_restatement_reproduces_reference_logs():
    """PyWavelets is not vendored with the reference: the db4/periodization restatement
    (oracle/wavelet.py) is pinned by the misfit lines of the reference's committed wavelet runs,
    example/uniformgrid/logout_T1.txt (chains 0, 1) and example/segmentgrid/logout_T0.txt."""
    from gravinv3dhmc_amd import mesher
    from oracle import wavelet as w
    e = gold("example_inputs.npz")

    def run(obs, mesh, ref, rank, n):
        K = oracle.prism_gz_kernel(obs[:, 0], obs[:, 1], obs[:, 2], mesh.cell_bounds())
        Aw, wm = oracle.col_weight(K)
        N, M = Aw.shape
        shape = mesh.shape
        csr = w.compress_kernel(Aw, 3, shape)
        assert csr.shape == (N, 6820)                    # 11 x 31 x 20 packed coefficients
        P = oracle.Problem(Aw, obs[:, 3], 0.001 * wm, "MS", 1.0, 0.001, wm=wm, shape=shape, csr=csr,
                           dwt=lambda x: w.model_coeffs(x, 3, shape))
        rows, _ = _run_chain(P, wm, 0.001 * wm, 0 * wm, 1 * wm, 0.01, [5, 20], 0.001, 100 + rank, n, N, M)
        np.testing.assert_allclose(rows[:, :3], ref[:len(rows)][:, [0, 1, 3]], rtol=0, atol=1.01e-7)

    uni = mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    run(e["uni_obs"], uni, e["uni_T1_chain0"], 0, 6)
    run(e["uni_obs"], uni, e["uni_T1_chain1"], 1, 4)
    seg = mesher.PrismMeshSegment((0, 2000, 0, 3000, 0, 2100), ([100, 200, 300], 100, 100),
                                  [0, 300, 900, 2100])
    run(e["seg_obs"], seg, e["seg_T0_chain0"], 0, 4)


def test_wavelet_orthonormal_on_even_lengths():
    from oracle import wavelet as w
    rng = np.random.default_rng(0)
    x = rng.normal(size=(3, 8 * 12 * 16))
    c, shp = w.wavedec3_packed(x, (8, 12, 16))
    assert shp == (8, 12, 16)
    np.testing.assert_allclose((c ** 2).sum(1), (x ** 2).sum(1), rtol=1e-13)
    y = rng.normal(size=8 * 12 * 16)
    np.testing.assert_allclose(c @ w.model_coeffs(y, 3, (8, 12, 16)), x @ y, rtol=1e-12)
    c1 = w.wavedec1_packed(x)
    np.testing.assert_allclose((c1 ** 2).sum(1), (x ** 2).sum(1), rtol=1e-13)
    assert w.wavedec3_packed(np.zeros(6000), (10, 30, 20))[1] == (11, 31, 20)


def test_cg_port_matches_reference_golden():
    """oracle/cg_port.py against the reference's ConjugateGradient.CG outputs (cg_small.npz)."""
    from oracle import cg_port
    g = gold("cg_small.npz")
    M = int(np.prod(g["shape"]))
    for reg in ("MS", "Damping", "Smoothness", "TV"):
        res = cg_port.cg(g["K"], g["dobs"], tuple(g["shape"]), np.full(M, 0.001), np.full(M, 0.001),
                         (0.0, 1.0), reg, 0.01, 0.9, 8)
        for name, v in zip(("model", "data", "dmis", "mmis", "alpha"), res):
            assert relmax(v, g[reg + "_" + name]) < 1e-9, (reg, name)


def test_wavelet_odd_lengths_pinned_by_ratiogrid_log():
    """example/ratiogrid/logout_T1.txt: geometric-dz mesh of shape (19, 30, 30) -- odd lengths on
    both wavelet levels (19 -> 10 -> 5, 15 -> 8) -- wavelet 3D + MS, including a REJECTED proposal
    (accept ratio 66.67 % on line 3).  Pins the odd-length periodization of oracle/wavelet.py."""
    from gravinv3dhmc_amd import mesher
    from oracle import wavelet as w
    e = gold("example_inputs.npz")
    obs = e["ratio_obs"]
    mesh = mesher.PrismMesh((0, 6000, 0, 6000, 0, 6000), (200, 200, 200), 1.05)
    assert mesh.shape == (19, 30, 30)
    Aw, wm = oracle.col_weight(oracle.prism_gz_kernel(obs[:, 0], obs[:, 1], obs[:, 2], mesh.cell_bounds()))
    np.testing.assert_allclose((0.001 * wm)[:3], e["ratio_initial_mw_head"], rtol=5e-9)
    np.testing.assert_allclose((0.001 * wm)[-3:], e["ratio_initial_mw_tail"], rtol=5e-9)
    N, M = Aw.shape
    shape = mesh.shape
    csr = w.compress_kernel(Aw, 3, shape)
    assert csr.shape == (N, 21 * 31 * 31 - 0) or csr.shape[1] == w.model_coeffs(np.zeros(M), 3, shape).size
    P = oracle.Problem(Aw, obs[:, 3], 0.001 * wm, "MS", 1.0, 0.001, wm=wm, shape=shape, csr=csr,
                       dwt=lambda x: w.model_coeffs(x, 3, shape))
    rows, _ = _run_chain(P, wm, 0.001 * wm, 0 * wm, 0.4 * wm, 0.01, [5, 20], 0.001, 100, 3, N, M)
    ref = e["ratio_T1_chain0"][:len(rows)]
    np.testing.assert_allclose(rows[:, :3], ref[:, [0, 1, 3]], rtol=0, atol=1.01e-7)
    ratio = 100.0 * np.cumsum(rows[:, 3]) / np.arange(1, len(rows) + 1)
    np.testing.assert_allclose(ratio, ref[:, 4], atol=0.006)
    assert (rows[:, 3] == 0).any()          # the rejected proposal of the log is reproduced


GLOBAL_MW_HEAD = np.array([10.29561741, 10.015107, 9.91994061])     # example/global/logout_T1.txt:42-43
GLOBAL_MW_TAIL = np.array([0.07159403, 0.07159418, 0.07159425])


def global_inputs():
    """Config C4 geometry (example/global/main_global.py:25-28, model_global.py:159-162)."""
    from gravinv3dhmc_amd import mesher
    mesh = mesher.TesseroidMesh((-180, 180, -90, 90, 0, -3000000), (-300000, 3, 3))
    lon, lat = [a.ravel() for a in np.meshgrid(np.linspace(-180, 180, 121), np.linspace(-90, 90, 61),
                                               indexing="ij")]
    return mesh, lon, lat, np.full_like(lon, 5000.0)


def test_global_log_initial_mw_columns():
    """`initial mw` of example/global/logout_T1.txt (0.01 x column norms of the 7381 x 72000
    tesseroid kernel): the six printed cells need only six columns of the kernel."""
    mesh, lon, lat, h = global_inputs()
    b = mesh.cell_bounds()
    assert b.shape == (72000, 6) and lon.size == 7381
    cols = np.r_[0, 1, 2, 71997, 71998, 71999]
    K = oracle.tess_gz_kernel(lon, lat, h, b[cols])
    mw = 0.01 * np.sqrt((K ** 2).sum(0))
    np.testing.assert_allclose(mw[:3], GLOBAL_MW_HEAD, rtol=5e-9)
    np.testing.assert_allclose(mw[3:], GLOBAL_MW_TAIL, rtol=0, atol=5.1e-9)   # 8 decimals printed


def test_bootstrap_port_matches_reference_golden():
    from oracle import cg_port
    g, b = gold("cg_small.npz"), gold("bs_small.npz")
    M = int(np.prod(g["shape"]))
    res = cg_port.bootstrap(g["K"], g["dobs"], (0.0, 1.0), np.full(M, 0.001), samples=3, beta=0.1, maxk=5)
    for name, v in zip(("models", "dmis", "mmis", "alpha"), res):
        assert relmax(v, b[name]) < 1e-9, name


def test_bootstrap_port_with_wavelet_forward_is_the_reference_formulation():
    """oracle/cg_port.bootstrap(wavelet=...): reginv.py:546-553,590-593,608-617 as written -- the data term
    and its gradient take the predicted data from the compressed unresampled operator (original row order)
    against the resampled observations; checked term by term against that formulation spelled out here."""
    from oracle import cg_port, oracle as orc, wavelet as ow
    g = gold("cg_small.npz")
    shape = tuple(int(v) for v in g["shape"])
    M = int(np.prod(shape))
    a = cg_port.bootstrap(g["K"], g["dobs"], (0.0, 1.0), np.full(M, 0.001), samples=2, beta=0.1, maxk=2,
                          wavelet="3D", shape=shape)
    assert np.isfinite(a[0]).all() and a[0].shape == (2, M)
    # first CG step of replicate 0 by hand: alpha = 0, I = 2 AwS^T (Awcp W(mw) - dS), k = I.I / |AwS I|^2
    Aw, wm = orc.col_weight(g["K"])
    N = Aw.shape[0]
    np.random.seed(0)
    idx = np.random.choice(np.arange(N), size=N, replace=True, p=None)
    AwS, dS = Aw[idx, :], g["dobs"][idx]
    mw = wm * 0.001
    dpre = ow.compress_kernel(Aw, 3, shape) @ ow.model_coeffs(mw, 3, shape)
    I = 2 * AwS.T @ (dpre - dS)
    k = (I @ I) / np.linalg.norm(AwS @ I) ** 2
    m1 = np.clip((mw - k * I) / wm, 0.0, 1.0)
    # (maxk = 2: the second iteration moves on from m1; compare the regularisation factor it derives from it)
    data1 = np.linalg.norm(ow.compress_kernel(Aw, 3, shape) @ ow.model_coeffs(wm * m1, 3, shape) - dS) ** 2
    model1 = np.sum(wm * wm * (wm * m1) ** 2 / ((wm * m1) ** 2 + 0.1 ** 2))
    assert abs(a[3][0, 1] - data1 / model1) < 1e-9 * abs(data1 / model1)


def test_oracle_prism_kernel_is_the_reference_kernel_bit_for_bit():
    """The C restatement against the reference's own `_prism.gz` (gravmag/_prism.pyx compiled unmodified by
    oracle/build_ref.py) on random and singular geometries: prism_random.npz holds its output
    (oracle/make_golden.py)."""
    from oracle import oracle as orc
    g = gold("prism_random.npz")
    assert g["K"].shape == (200, 3)
    assert np.array_equal(orc.prism_gz_kernel(g["xp"], g["yp"], g["zp"], g["cells"]), g["K"])
