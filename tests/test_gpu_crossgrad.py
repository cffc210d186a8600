"""GPU suite of the cross-gradient coupling of the joint inversion (gh_set_cross_gradient, JointModule): the term
alone, inside misfit_and_grad through both epilogue forms, whole chains, and that off means off.  The host side
of every comparison is the NumPy restatement in tests/crossgrad_host.py (the reference's CrossGradient is an empty
method); everything at lambda = 0 is compared with the reference-generated goldens.

Tolerances are DESIGN section 2's: 1e-10 relative for potential, gradient and scalars against a host restatement,
1e-9 for chains.  Each test prints the deviation it measured before it asserts."""
import contextlib
import io

import numpy as np
import pytest

from conftest import gold
from crossgrad_host import JointHostProblem, cross_gradient, legacy_draws, relative_spacings
from helpers import relmax

pytestmark = pytest.mark.gpu

MANGLE = (60.0, -10.0)
REGS = ("Damping", "MS", "Smoothness", "TV")


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _grid(n_y, n_x, x1=2000.0, y1=3000.0, h=0.0):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, y1, n_y), np.linspace(0, x1, n_x))]
    return xp, yp, np.full_like(xp, h)


def _mesh(G, mrange, mspacing, mratio=1):
    with contextlib.redirect_stdout(io.StringIO()):
        return G.mesher.PrismMesh(mrange, mspacing, mratio)


def _joint_engine(G, obs, cells):
    from gravinv3dhmc_amd import _lib, utils
    n, m = obs[0].size, cells.shape[0]
    eng = G.Engine(2 * n, 2 * m)
    eng.set_cells(cells, _lib.CELL_PRISM_JOINT, direction=utils.dircos(*MANGLE))
    eng.set_obs(*obs)
    eng.build_G()
    return eng


def _module(G, z, g, **kw):
    xp, yp, zp = z[g + "_xp"], z[g + "_yp"], z[g + "_zp"]
    return G.JointModule(z[g + "_dobs_gz"], z[g + "_dobs_tf"], tuple(z[g + "_mrange"]), tuple(z[g + "_mspacing"]),
                         (xp, yp, zp), mangle=tuple(z["mangle"]), verbose=False, **kw)


def _close(a, b, tol, what):
    dev = abs(a - b) / max(abs(b), 1e-300)
    print("%s: %.3e (bound %.0e)" % (what, dev, tol))
    assert dev <= tol, what


# ----------------------------------------------------------------------------- 1. the term alone

@pytest.mark.parametrize("geom", ["cubic", "anisotropic", "mratio"])
def test_cross_gradient_eval_against_restatement(G, geom):
    if geom == "cubic":
        mesh, scale = _mesh(G, (0, 2000, 0, 3000, 0, 1000), (250, 250, 250)), (1.0, 1.0)
    elif geom == "anisotropic":
        mesh, scale = _mesh(G, (0, 2000, 0, 3000, 0, 1000), (250, 300, 200)), (0.5, 4.0)
    else:
        mesh, scale = _mesh(G, (0, 2000, 0, 3000, 0, 1500), (100, 300, 250), 1.4), (2.0, 0.25)
    shape = mesh.shape
    m = mesh.size
    hx, hy, hz = relative_spacings(mesh)
    if geom == "cubic":
        assert hx == 1.0 and hy == 1.0 and np.all(hz == 1.0)
    if geom == "mratio":
        assert hz.max() > 1.2 * hz.min()
    eng = _joint_engine(G, _grid(6, 5), mesh.cell_bounds(active_only=True))
    wm = eng.weight(0.5)
    eng.set_cross_gradient(0.0, shape, hx, hy, hz, scale)   # (the geometry; the term stays out of the potential)
    rng = np.random.default_rng(5)
    for k in range(2):
        mw = rng.normal(size=2 * m) * wm
        phi, grad, t = eng.cross_gradient_eval(mw)
        rphi, rgrad, rt = cross_gradient(mw, wm, shape, hx, hy, hz, scale)
        _close(phi, rphi, 1e-10, "%s random %d: Phi" % (geom, k))
        print("   gradient %.3e, t %.3e" % (relmax(grad, rgrad), relmax(t, rt)))
        assert relmax(grad, rgrad) <= 1e-10 and relmax(t, rt) <= 1e-10
    phi_rand, gmax = rphi, np.abs(rgrad).max()
    # two linearly related models: zero up to the rounding of w = a u + b and of mw winv (each component of t is the
    # difference of two products equal to ~1e-16 of |Du| |Dw|, so Phi is ~1e-32 of the Phi of unrelated models;
    # under the column-norm weights of a real kernel no pair of models is related to the last bit -- the case where
    # every operation is exact, and the zero with it, is in test_crossgrad_host.py)
    u = rng.normal(size=m)
    mw = np.concatenate([u, -2.5 * u + 0.75]) * wm
    phi, grad, t = eng.cross_gradient_eval(mw)
    print("%s linearly related: Phi %.3e of %.3e, gradient %.3e of %.3e" % (geom, phi, phi_rand, np.abs(grad).max(), gmax))
    assert phi <= 1e-24 * phi_rand and np.abs(grad).max() <= 1e-12 * gmax
    # one property flat (at 0: mw wm^-1 gives exactly 0 back): Phi, gradient and t exactly 0
    for flat in (0, 1):
        parts = [rng.normal(size=m) * wm[:m], rng.normal(size=m) * wm[m:]]
        parts[flat] = np.zeros(m)
        phi, grad, t = eng.cross_gradient_eval(np.concatenate(parts))
        assert phi == 0.0 and not grad.any() and not t.any(), (geom, flat)
    eng.close()


# ----------------------------------------------------------------------------- 2. inside misfit_and_grad

@pytest.mark.parametrize("geom", ["a", "b"])
def test_misfit_and_grad_with_coupling_against_goldens(G, geom):
    z = gold("joint_small.npz")
    g = geom + "_"
    jm = _module(G, z, geom)
    shape = tuple(int(v) for v in z[g + "shape"])
    assert jm.mshape == shape
    wm = jm.Wm.diagonal()
    mesh = _mesh(G, tuple(z[g + "mrange"]), tuple(z[g + "mspacing"]))
    spacing = relative_spacings(mesh)
    mwapr, alpha, beta = z[g + "mwapr"], float(z["alpha"]), float(z["beta"])
    worst = 0.0
    for lam, scale in ((5.0, (1.0, 1.0)), (400.0, (0.5, 2.0))):
        jm.set_cross_gradient(lam, scale)
        for reg in REGS:
            for k, x in enumerate(z[g + "xs"]):
                mis, grad, dpre, dv, mv = jm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, alpha,
                                                             regulization=reg, beta=beta)
                phi, pg, _ = cross_gradient(x, wm, shape, *spacing, scale=scale)
                ref_mis = z[g + reg + "_misfit"][k] + lam * phi
                ref_grad = z[g + reg + "_grad"][k] + lam * pg
                dev = [abs(mis - ref_mis) / abs(ref_mis), relmax(grad, ref_grad), relmax(dpre, z[g + reg + "_dpre"][k]),
                       abs(dv - z[g + reg + "_data"][k]) / abs(z[g + reg + "_data"][k]),
                       abs(mv - z[g + reg + "_model"][k]) / max(abs(z[g + reg + "_model"][k]), 1e-300),
                       abs(jm.last_cross_gradient - phi) / max(abs(phi), 1e-30)]
                worst = max(worst, max(dev))
                assert max(dev) <= 1e-10, (reg, k, lam, dev)
                # U - U_data - alpha U_model = lambda Phi
                assert abs((mis - dv - alpha * mv) - lam * phi) <= 1e-10 * abs(mis), (reg, k, lam)
                if k > 0:
                    assert lam * phi > 1e-6 * abs(mis), "the coupling must be visible in U at this tolerance"
    print("geometry %s: largest relative deviation %.3e (bound 1e-10)" % (geom, worst))
    jm._engine.close()


# ----------------------------------------------------------------------------- 3. both epilogue forms

@pytest.mark.parametrize("n_y,n_x,mspacing,stages", [(30, 20, (250, 300, 200), 1), (30, 20, (250, 100, 100), 2),
                                                     (60, 40, (250, 100, 100), 1)])
def test_coupling_through_both_epilogue_forms(G, n_y, n_x, mspacing, stages):
    obs = _grid(n_y, n_x)
    mesh = _mesh(G, (0, 2000, 0, 3000, 0, 1000), mspacing)
    shape, m, n = mesh.shape, mesh.size, obs[0].size
    eng = _joint_engine(G, obs, mesh.cell_bounds(active_only=True))
    assert eng.joint_layout()["epilogue_stages"] == stages
    wm = eng.weight(0.5)
    H = eng.download_G()
    Aw = np.zeros((2 * n, 2 * m))
    Aw[:n, :m], Aw[n:, m:] = H[:, :m], H[:, m:]
    rng = np.random.default_rng(3)
    x = rng.normal(size=2 * m)
    dobsw = rng.normal(size=2 * n)
    eng.set_data(dobsw)
    mwapr = rng.normal(size=2 * m) * 0.1
    spacing = relative_spacings(mesh)
    alpha, beta, scale = 0.5, 0.01, (1.0 / np.median(wm[:m]), 1.0 / np.median(wm[m:]))
    phi, pg, _ = cross_gradient(x, wm, shape, *spacing, scale=scale)
    lam = 0.05 * (np.sum((Aw @ x - dobsw) ** 2)) / phi     # (a coupling worth 5 % of the data term)
    eng.set_cross_gradient(lam, shape, *spacing, scale=scale)
    worst = 0.0
    for kind in REGS:
        eng.set_reg(kind, alpha, beta, shape, mwapr)      # (a regulariser change keeps the coupling)
        P = JointHostProblem(Aw, dobsw, wm, shape, kind, alpha, beta, mwapr, lam, spacing, scale)
        U, grad, d, U_data, R = P.misfit_and_grad(x)
        mis, g, dpre, dv, mv = eng.misfit_and_grad(x)
        dev = [abs(mis - U) / abs(U), relmax(g, grad), relmax(dpre, d), abs(dv - U_data) / U_data,
               abs(mv - R) / abs(R), abs(eng.cross_gradient_last() - phi) / phi]
        worst = max(worst, max(dev))
        assert max(dev) <= 1e-10, (kind, dev)
    print("n = %d, m = %d, %d stage(s): largest relative deviation %.3e (bound 1e-10)" % (n, m, stages, worst))
    eng.close()


# ----------------------------------------------------------------------------- 4, 5. chains

CHAIN = dict(reg="Smoothness", alpha=0.8, beta=0.001, lam=500.0, scale=(1.0, 1.0), dt=0.01, Sigma=0.001, seed=100,
             Lrange=[5, 20], n=8)


def _host_chain(jm, z, count):
    """The chain of CHAIN on the host: [(accepted, out5, Phi, clamped)], final x."""
    shape = tuple(int(v) for v in z["a_shape"])
    M2 = jm.Wm.shape[0]
    spacing = relative_spacings(_mesh(__import__("gravinv3dhmc_amd"), tuple(z["a_mrange"]), tuple(z["a_mspacing"])))
    P = JointHostProblem(np.asarray(jm.Aw), jm.dobsw, jm.Wm.diagonal(), shape, CHAIN["reg"], CHAIN["alpha"],
                         CHAIN["beta"], np.full(M2, 0.001), CHAIN["lam"], spacing, CHAIN["scale"])
    lo, hi = np.zeros(M2), np.ones(M2)
    x = np.full(M2, 0.001)
    draws = legacy_draws(CHAIN["seed"], M2, CHAIN["Lrange"], CHAIN["Sigma"], count)
    out = []
    for L, p0, u in draws:
        x, acc, o, phi, clamped = P.leapfrog(x, p0, CHAIN["dt"], L, lo, hi, u)
        out.append((acc, o, phi, clamped))
    return draws, out, x


def test_chain_with_coupling_against_numpy_leapfrog(G):
    z = gold("joint_small.npz")
    jm = _module(G, z, "a", crossgradient=CHAIN["lam"], cg_scale=CHAIN["scale"])
    M2 = jm.Wm.shape[0]
    draws, ref, xref = _host_chain(jm, z, CHAIN["n"])
    assert any(r[3] > 0 for r in ref), "no trajectory of the restatement clamps at a bound"
    assert any(not r[0] for r in ref) and any(r[0] for r in ref), "the restatement needs accepts and rejections"
    eng = jm._engine
    jm._use_reg(CHAIN["reg"], CHAIN["alpha"], CHAIN["beta"], np.full(M2, 0.001))
    eng.chain_init(np.full(M2, 0.001), np.zeros(M2), np.ones(M2))
    got = []
    eng.run_chain(iter(draws), CHAIN["dt"], lambda L, acc, o, xs: got.append((bool(acc), np.array(o))) or True, batch=3)
    assert len(got) == len(ref)
    worst = 0.0
    for k, ((acc, o), (racc, ro, rphi, _)) in enumerate(zip(got, ref)):
        dev = np.abs(o - ro) / np.abs(ro)
        print("trajectory %d: accepted %s/%s, out5 deviation %s" % (k, acc, racc, " ".join("%.2e" % v for v in dev)))
        worst = max(worst, dev.max())
        assert acc == racc, k
        assert dev.max() <= 1e-9, (k, dev)
    x = eng.chain_get_x()
    print("final x: %.3e; Phi of the final state %.6e against %.6e" % (relmax(x, xref), jm.last_cross_gradient, ref[-1][2]))
    assert relmax(x, xref) <= 1e-9
    assert abs(jm.last_cross_gradient - ref[-1][2]) <= 1e-9 * ref[-1][2]
    assert eng.chain_stats()["spec_hits"] >= 1, "the speculative first step was never used"
    jm._engine.close()


def test_hmcsample_with_coupling_writes_the_chain_rows(G, tmp_path, capsys):
    """The chain of test_chain_with_coupling_against_numpy_leapfrog through HMCSample, from the same seed: the sampler
    multiplies the start, the prior model and the bounds by Wm, so they are handed over divided by it."""
    z = gold("joint_small.npz")
    jm = _module(G, z, "a", crossgradient=CHAIN["lam"], cg_scale=CHAIN["scale"])
    M2 = jm.Wm.shape[0]
    wm = jm.Wm.diagonal()
    _, ref, _ = _host_chain(jm, z, CHAIN["n"])
    accepted = [r for r in ref if r[0]]
    # (the sampler stops at the nsamples-th accepted trajectory and writes accepted ones only: the rejections of this
    # chain are the other test's ground)
    nsamples = len(accepted)
    assert nsamples >= 3
    folder = str(tmp_path / "run_cg_chain")
    G.HMCSample(jm, nsamples, 0, CHAIN["dt"], CHAIN["Lrange"], 0.001 / wm, 0.001 / wm,
                np.c_[np.zeros(M2), 1.0 / wm], "mandatory", 1000, jm.dobs, "Fixed", 1.0, CHAIN["alpha"],
                CHAIN["reg"], CHAIN["beta"], CHAIN["seed"], CHAIN["Sigma"], nbest=100, myrank=0, save_folder=folder)
    capsys.readouterr()
    rows = np.atleast_2d(np.loadtxt(folder + "0/misfit.dat"))
    assert rows.shape[0] == nsamples
    for k, (row, r) in enumerate(zip(rows, accepted)):
        want = r[1][:3]
        dev = np.abs(row[:3] - want) / np.abs(want)
        print("row %d: %s" % (k, " ".join("%.2e" % v for v in dev)))
        # (misfit.dat holds eight decimals)
        assert np.all(np.abs(row[:3] - want) <= 1e-9 * np.abs(want) + 1e-8), k
    assert abs(jm.last_cross_gradient - accepted[-1][2]) <= 1e-9 * accepted[-1][2]
    jm._engine.close()


# ----------------------------------------------------------------------------- 6. off means off

def test_off_means_off(G, tmp_path, capsys):
    z = gold("joint_small.npz")
    c = gold("chain_small_joint.npz")
    mwapr, alpha, beta = z["a_mwapr"], float(z["alpha"]), float(z["beta"])

    def outputs(jm):
        out = []
        for reg in REGS:
            for x in z["a_xs"]:
                out.append(jm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, alpha, regulization=reg, beta=beta))
        return out

    def chain(jm, tag):
        M2 = jm.Wm.shape[0]
        dt, Sigma, lo, hi, n = c["a_cfg"]
        folder = str(tmp_path / tag)
        G.HMCSample(jm, int(n), 0, float(dt), [5, 20], np.full(M2, 0.001 + lo), np.full(M2, 0.001),
                    np.c_[np.full(M2, lo), np.full(M2, hi)], "mandatory", 1000, jm.dobs, "Fixed", 0.8, 1.0,
                    str(c["a_reg"]), 0.001, 100, float(Sigma), nbest=100, myrank=0, save_folder=folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        return lines, np.loadtxt(folder + "0/misfit.dat"), np.loadtxt(folder + "0/model.dat")

    plain = _module(G, z, "a")
    base, base_chain = outputs(plain), chain(plain, "plain")
    assert base_chain[0] == [str(s) for s in c["a_lines"]]
    np.testing.assert_allclose(base_chain[1], c["a_misfit"], atol=2e-8, rtol=1e-9)
    assert plain.last_cross_gradient == 0.0
    plain._engine.close()
    zero = _module(G, z, "a", crossgradient=0.0)
    toggled = _module(G, z, "a")
    toggled.set_cross_gradient(3.0)
    on = toggled.misfit_and_grad(z["a_xs"][1], mwapr, None, None, "mandatory", 1000, alpha, regulization="TV", beta=beta)
    assert on[0] != base[3 * 3 + 1][0] and toggled.last_cross_gradient > 0
    toggled.set_cross_gradient(0.0)
    for tag, jm in (("zero", zero), ("toggled", toggled)):
        for a, b in zip(outputs(jm), base):
            assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4], tag
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), tag
        got = chain(jm, tag)
        assert got[0] == base_chain[0], tag
        assert np.array_equal(got[1], base_chain[1]) and np.array_equal(got[2], base_chain[2]), tag
        assert jm.last_cross_gradient == 0.0
        jm._engine.close()


def test_regulariser_change_keeps_the_coupling(G):
    z = gold("joint_small.npz")
    jm = _module(G, z, "a", crossgradient=2.0)
    mwapr, x = z["a_mwapr"], z["a_xs"][2]
    wm = jm.Wm.diagonal()
    spacing = relative_spacings(_mesh(G, tuple(z["a_mrange"]), tuple(z["a_mspacing"])))
    phi = cross_gradient(x, wm, jm.mshape, *spacing)[0]
    for reg, alpha in (("Damping", 0.7), ("TV", 0.7), ("TV", 0.3), ("MS", 0.3)):
        mis, _, _, dv, mv = jm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, alpha, regulization=reg, beta=0.001)
        assert abs((mis - dv - alpha * mv) - 2.0 * phi) <= 1e-10 * abs(mis), (reg, alpha)
        assert abs(jm.last_cross_gradient - phi) <= 1e-10 * phi
    jm._engine.close()


# ----------------------------------------------------------------------------- 7. refusals

def test_cross_gradient_refusals(G):
    from gravinv3dhmc_amd import _lib
    mesh = _mesh(G, (0, 2000, 0, 3000, 0, 900), (300, 750, 500))
    obs, cells = _grid(6, 5), mesh.cell_bounds(active_only=True)
    shape, m = mesh.shape, mesh.size
    hz = np.ones(shape[0] - 1)
    # a gz-only context
    eng = G.Engine(obs[0].size, m)
    eng.set_obs(*obs)
    eng.set_cells(cells, _lib.CELL_PRISM)
    eng.build_G()
    eng.weight(0.5)
    with pytest.raises(NotImplementedError, match="joint"):
        eng.set_cross_gradient(1.0, shape, 1.0, 1.0, hz)
    with pytest.raises(NotImplementedError, match="joint"):
        eng.cross_gradient_eval(np.zeros(m))
    eng.close()
    je = _joint_engine(G, obs, cells)
    with pytest.raises(ValueError):                       # before gh_weight
        je.set_cross_gradient(1.0, shape, 1.0, 1.0, hz)
    je.weight(0.5)
    with pytest.raises(ValueError):                       # evaluation before the geometry is set
        je.cross_gradient_eval(np.zeros(2 * m))
    bad = [dict(shape=(shape[0], shape[1], shape[2] + 1)), dict(lam=-1.0), dict(scale=(0.0, 1.0)), dict(scale=(1.0, -2.0)),
           dict(shape=(1, shape[1], shape[2] * shape[0]), hz=np.ones(0)), dict(hx=0.0), dict(hz=hz * -1.0)]
    for kw in bad:
        a = dict(lam=1.0, shape=shape, hx=1.0, hy=1.0, hz=hz, scale=(1.0, 1.0))
        a.update(kw)
        with pytest.raises(ValueError):
            je.set_cross_gradient(a["lam"], a["shape"], a["hx"], a["hy"], a["hz"], a["scale"])
    je.set_cross_gradient(1.0, shape, 1.0, 1.0, hz)       # (and the valid call goes through)
    je.close()
    # a carved module
    z = gold("joint_small.npz")
    xp, yp = z["a_xp"], z["a_yp"]
    topo = (xp, yp, np.full(xp.size, -350.0) + 100.0 * np.sin(xp / 500.0))
    for kw in (dict(crossgradient=1.0), {}):
        try:
            jm = _module(G, z, "a", mtopo=topo, **kw)
        except ValueError as e:
            assert kw and "uncarved" in str(e)
            continue
        assert not kw
        if jm._engine.M == 2 * int(np.prod(jm.mshape)):
            pytest.fail("the topography carved nothing: the refusal was not exercised")
        with pytest.raises(ValueError, match="uncarved"):
            jm.set_cross_gradient(1.0)
        jm._engine.close()
