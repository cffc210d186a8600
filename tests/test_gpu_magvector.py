"""GPU suite of the magnetization-vector inversion (MagVectorModule, GH_CELL_PRISM_MVI): the three blocks of the store
against the reference's fixtures and against the total-field engine, forward results, the potential, a trajectory and
chains against the NumPy restatement (tests/magvector_host.py) on the downloaded store, the per-property stencil, the
amplitude coupling, HMCSample end to end, the refusals and a carved mesh.

Tolerances.  Blocks against the reference: 1e-10 max|K|, what tests/test_gpu_magnetic.py allows its tf entries.
Potential against the restatement: tests/test_gpu_joint.py's for its comparison with host products -- 1e-12 for the
values and the prediction, 1e-11 for the gradient.  That file compares no single trajectory or chain with a
restatement; those take 1e-10, the tolerance every other store's chains are held to against their restatements
(tests/test_gpu_multicomp.py): a trajectory chains up to 8 evaluations, each good to 1e-12, through updates that can
amplify a rounding difference by the ratio of the step to the state, two orders at these step sizes."""
import ctypes as C

import numpy as np
import pytest

from conftest import gold
from helpers import c1_inputs, relmax
from magvector_host import MagVectorProblem, amplitude_term, regulariser

pytestmark = pytest.mark.gpu

REGS = ("Damping", "MS", "Smoothness", "TV")
MRANGE, MSPACING = (0, 2000, 0, 3000, 0, 900), (300, 750, 500)
SHAPE = (3, 4, 4)
MANGLE = (60.0, -10.0)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _mvi_engine(G, xp, yp, zp, cells, inc, dec):
    from gravinv3dhmc_amd import utils
    eng = G.Engine(np.asarray(xp).size, 3 * np.asarray(cells).shape[0])
    eng.set_cells_mvi(cells, utils.dircos(inc, dec))
    eng.set_obs(xp, yp, zp)
    return eng


def _tf_engine(G, xp, yp, zp, cells, inc, dec):
    from gravinv3dhmc_amd import _lib, utils
    eng = G.Engine(np.asarray(xp).size, np.asarray(cells).shape[0])
    eng.set_obs(xp, yp, zp)
    eng.set_cells(cells, _lib.CELL_PRISM_TF, direction=utils.dircos(inc, dec))
    return eng


def _obs(nx=7, ny=5):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(100, 2900, ny), np.linspace(50, 1950, nx))]
    return xp, yp, np.full(xp.size, -30.0)


def _body(shape, sl, vec):
    """property-major model: the vector vec in the cells of the slice sl, zero elsewhere"""
    v = np.zeros(shape + (3,))
    v[sl] = vec
    return np.ascontiguousarray(v.reshape(-1, 3).T).ravel()


def _data(G, obs, mrange, mspacing, shape, sl, seed=3):
    """Total field of a body magnetized AWAY from the regional field (remanence), plus noise and a base level"""
    from gravinv3dhmc_amd import utils
    mesh = G.mesher.PrismMesh(mrange, mspacing)
    eng = _mvi_engine(G, obs[0], obs[1], obs[2], mesh.cell_bounds(), *MANGLE)
    model = _body(shape, sl, utils.ang2vec(1.5, -20.0, 75.0))
    d = eng.tf_result(np.ascontiguousarray(model.reshape(3, -1).T))
    eng.close()
    rng = np.random.default_rng(seed)
    return d + 0.02 * np.abs(d).max() * rng.normal(size=d.size) + 4.0, model


def _module(G, obs, dobs, mrange=MRANGE, mspacing=MSPACING, **kw):
    return G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=MANGLE, verbose=False, **kw)


def _small(G, **kw):
    obs = _obs()
    dobs, truth = _data(G, obs, MRANGE, MSPACING, SHAPE, (slice(1, None), slice(1, 3), slice(1, 3)))
    return _module(G, obs, dobs, **kw), obs, dobs, truth


def _errs(a, b):
    return [abs(a[0] - b[0]) / abs(b[0]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
            abs(a[4] - b[4]) / max(abs(b[4]), 1e-300)], relmax(a[1], b[1])


# ----------------------------------------------------------------------------- 1. the blocks against the reference

def test_blocks_against_the_reference(G):
    g = gold("mvi_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    m = cells.shape[0]
    worst = 0.0
    for d, (inc, dec) in enumerate(g["dirs"]):
        eng = _mvi_engine(G, xp, yp, zp, cells, inc, dec)
        eng.build_G()
        A = eng.download_G()
        assert A.shape == (xp.size, 3 * m) and np.isfinite(A).all()
        for a in range(3):
            ref = g["A%d_%d" % (d, a)]
            err = np.abs(A[:, a * m:(a + 1) * m] - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            print("f = %r, block %s: max |dA|/max|A| = %.3e" % ((inc, dec), "xyz"[a], err))
            assert err <= 1e-10, (inc, dec, a, err)
        eng.close()
    print("blocks against the reference: worst %.3e" % worst)


def test_c1_columns_against_the_reference(G):
    z = gold("mvi_small.npz")
    mesh, xp, yp, zp = c1_inputs()
    inc, dec = z["c1_mangle"]
    eng = _mvi_engine(G, xp, yp, zp, mesh.cell_bounds(), inc, dec)
    eng.build_G()
    A = eng.download_G()
    assert A.shape == (600, 18000)
    err = np.abs(A[:, z["c1_cols"]] - z["c1_K"]).max() / np.abs(z["c1_K"]).max()
    print("C1 columns of [A_x | A_y | A_z]: max |dA|/max|A| = %.3e" % err)
    assert err <= 1e-10
    assert not eng.fold_info()["on"]
    eng.close()


# ----------------------------------------------------------------------------- 2. consistency with the tf engine

def test_blocks_are_consistent_with_the_total_field_kernel(G):
    """f = e_x: block x is the CELL_PRISM_TF kernel.  Oblique f: sum_a f_a A_a is.  The reference's own arrays
    (tests/golden/mvi_cases.npz against prism_tf_cases.npz) deviate from that identity by 1.5e-16, 0, 5.7e-16 and
    7.4e-16 of the largest entry at the four directions -- computed below from the fixtures, not taken from the
    device -- and the device gets twice the deviation of its direction.  (inc = 0, dec = 0 gives f = (1, 0, 6e-17):
    cos(pi/2) is not 0 in floating point, so e_x holds to that, on the reference's side too.)"""
    from gravinv3dhmc_amd import utils
    g, tfc = gold("mvi_cases.npz"), gold("prism_tf_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    m = cells.shape[0]
    for d, (inc, dec) in enumerate(g["dirs"]):
        f = utils.dircos(inc, dec)
        Kref = tfc["K%d" % d]
        dev_ref = np.abs(sum(f[a] * g["A%d_%d" % (d, a)] for a in range(3)) - Kref).max() / np.abs(Kref).max()
        eng = _mvi_engine(G, xp, yp, zp, cells, inc, dec)
        eng.build_G()
        A = eng.download_G()
        eng.close()
        tf = _tf_engine(G, xp, yp, zp, cells, inc, dec)
        tf.build_G()
        K = tf.download_G()
        tf.close()
        dev = np.abs(sum(f[a] * A[:, a * m:(a + 1) * m] for a in range(3)) - K).max() / np.abs(K).max()
        print("f = %r: |sum f_a A_a - K| / max|K|: reference %.3e, device %.3e" % ((inc, dec), dev_ref, dev))
        assert dev <= 2 * dev_ref, (inc, dec, dev, dev_ref)
        if (inc, dec) == (0.0, 0.0):
            dx_ref = np.abs(g["A%d_0" % d] - Kref).max() / np.abs(Kref).max()
            dx = np.abs(A[:, :m] - K).max() / np.abs(K).max()
            print("f = e_x: |A_x - K| / max|K|: reference %.3e, device %.3e" % (dx_ref, dx))
            assert dx <= 2 * dx_ref


# ----------------------------------------------------------------------------- 3. forward results

def test_forward_results_against_the_reference(G):
    g = gold("mvi_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    for d, (inc, dec) in enumerate(g["dirs"]):
        eng = _mvi_engine(G, xp, yp, zp, cells, inc, dec)
        for key, mag in (("res_vec%d" % d, g["mag"]), ("res_vec2_%d" % d, g["mag2"])):
            res = eng.tf_result(mag)                                   # (needs no G)
            assert relmax(res, g[key]) <= 1e-10
        with pytest.raises(ValueError):
            eng.tf_result(np.zeros((3 * cells.shape[0], 3)))
        eng.build_G()
        wm = eng.weight(0.5)
        model = np.ascontiguousarray(g["mag"].T).ravel()
        assert relmax(eng.forward(model * wm), g["res_vec%d" % d]) <= 1e-10
        eng.close()
    z = gold("mvi_small.npz")
    mv = G.MagVectorModule(z["res_vec"], tuple(z["mrange"]), tuple(z["mspacing"]), (z["xp"], z["yp"], z["zp"]),
                           mangle=tuple(z["mangle"]), verbose=False)
    assert mv.mshape == tuple(z["shape"]) and mv.Aw.shape == (42, 3 * z["cells"].shape[0])
    model = mv.from_vectors(z["vec"])
    assert relmax(mv.forward(model), z["res_vec"]) <= 1e-10
    assert relmax(mv._engine.tf_result(z["vec"]), z["res_vec"]) <= 1e-10
    for a in range(3):
        assert relmax(mv.kernel("xyz"[a]), z["A"][a]) <= 1e-10 and relmax(mv.kernel(a), z["A"][a]) <= 1e-10
    assert relmax(mv.A, np.hstack(list(z["A"]))) <= 1e-10
    with pytest.raises(ValueError):
        mv.kernel(3)
    mv._engine.close()


# ----------------------------------------------------------------------------- 4. potential, trajectory, chain

def _phi_of_the_kept_state(mv, x_kept, wm, lam, amp_beta, tol):
    """last_amplitude after a trajectory or a chain: Phi of the state the chain is left in (x_kept: the restatement's),
    whether the proposal was accepted or not; 0 while the coupling is off"""
    if lam > 0:
        phi = amplitude_term(x_kept, wm, amp_beta)[0]
        assert phi > 0 and abs(mv.last_amplitude - phi) <= tol * phi, (mv.last_amplitude, phi)
    else:
        assert mv.last_amplitude == 0.0


def _check_against_restatement(G, mv, dobs, shape, lam=0.0, amp_beta=0.05, n_chain=5, n_over=3):
    eng = mv._engine
    Aw = np.array(eng.download_G())
    wm = mv.Wm.diagonal()
    M = wm.size
    assert relmax(wm, np.sqrt(((Aw * wm[None, :]) ** 2).sum(axis=0))) <= 1e-10
    rng = np.random.default_rng(7)
    mwapr = 0.001 * wm
    worst = worst_g = 0.0
    if lam > 0:
        mv.set_amplitude(lam, amp_beta)
    for reg in REGS:
        P = MagVectorProblem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape, lam=lam, amp_beta=amp_beta)
        for _ in range(2):
            x = rng.uniform(-0.02, 0.02, M) * wm
            a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            b = P.misfit_and_grad(x)
            ev, eg = _errs(a, b)
            worst, worst_g = max(worst, max(ev)), max(worst_g, eg)
            assert max(ev) <= 1e-12 and eg <= 1e-11, (reg, ev, eg)
            if lam > 0:
                assert abs(mv.last_amplitude - P.phi) <= 1e-12 * P.phi
                assert abs(a[0] - (a[3] + 0.7 * a[4] + lam * mv.last_amplitude)) <= 1e-12 * abs(a[0])
            else:
                assert mv.last_amplitude == 0.0
    low, high = -0.02 * wm, 0.02 * wm
    # The step of the trajectories that are to be ACCEPTED.  The Metropolis test is u < exp(-dH), so even u = 0 rejects
    # once exp(-dH) underflows (dH > 745): the step has to keep the integrator stable.  The data term's curvature
    # (2 Aw^T Aw, unit columns) is a few hundred here and 0.02 is well inside 2 / sqrt(curvature).  The amplitude
    # term's is larger: d2/du2 of s / (s + beta) is at most 2 / beta (at s = 0), and u = mw / wm, so in mw it reaches
    # 2 lam / (amp_beta min(wm)^2) -- 3.6e5 on the 2100-row case, where 0.02 blows the energy up by thousands.  Half
    # the stability limit 2 / sqrt(curvature), worked out from wm and not from what the device returns.
    dt = 0.02 if lam == 0 else min(0.02, 1.0 / np.sqrt(2.0 * lam / (amp_beta * wm.min() ** 2)))
    P = MagVectorProblem(Aw, dobs, mwapr, "TV", 1.0, 0.001, wm=wm, shape=shape, lam=lam, amp_beta=amp_beta)
    eng.set_reg("TV", 1.0, 0.001, shape, mwapr)
    # one trajectory that runs into the bounds and is rejected (a Metropolis variate next to 1 after an overshoot)
    p0 = rng.normal(size=M) * 3.0
    xg, acc, o, _ = eng.leapfrog(mwapr, p0, 0.02, 8, low, high, 1.0 - 1e-9)
    xo, acco, oo = P.leapfrog(mwapr, p0, 0.02, 8, low, high, 1.0 - 1e-9)
    assert acc == acco and not acc and relmax(o, oo) <= 1e-10 and relmax(xg, xo) <= 1e-10
    _phi_of_the_kept_state(mv, mwapr, wm, lam, amp_beta, 1e-12)      # (rejected: the state given, bit for bit)
    # ... and one that is accepted, with clamps on the way
    p0 = rng.normal(size=M) * 0.3
    xg, acc, o, _ = eng.leapfrog(mwapr, p0, dt, 6, low, high, 0.0)
    xo, acco, oo = P.leapfrog(mwapr, p0, dt, 6, low, high, 0.0)
    assert acco, ("the restatement's own trajectory is to be accepted", dt, oo[3], oo[4])
    assert acc == acco and relmax(o, oo) <= 1e-10 and relmax(xg, xo) <= 1e-10
    assert np.any(xo == high) or np.any(xo == low)
    _phi_of_the_kept_state(mv, xo, wm, lam, amp_beta, 1e-10)         # (accepted: the new state, good to 1e-10)
    # (a Metropolis variate of 0 accepts while exp(-dH) > 0, which the step above sees to; one next to 1 rejects an
    # overshoot: both decisions occur at every size)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, 0.0)]
    trajs += [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(n_chain - 1)]
    trajs += [(8, rng.normal(size=M) * 3.0, 1.0 - 1e-9) for _ in range(n_over)]
    trajs += [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(2)]
    ref = P.chain(mwapr, trajs, dt, low, high)
    eng.chain_init(mwapr, low, high)
    res = []
    eng.run_chain(iter(trajs), dt, lambda L, acc, o, x: res.append((acc, o.copy(), x)), want_x=True)
    assert len(res) == len(ref)
    assert any(a for a, _, _ in ref) and any(not a for a, _, _ in ref)
    for (a1, o1, x1), (a2, o2, x2) in zip(res, ref):
        assert a1 == a2 and relmax(o1, o2) <= 1e-10 and (x1 is None or relmax(x1, x2) <= 1e-10)
        worst = max(worst, relmax(o1, o2))
    assert relmax(eng.chain_get_x(), ref[-1][2]) <= 1e-10
    _phi_of_the_kept_state(mv, ref[-1][2], wm, lam, amp_beta, 1e-10)
    st = eng.chain_stats()
    assert st["resident_launches"] == 0 and not eng.fold_info()["on"]
    print("N = %d, M = %d, lambda = %g: worst value %.3e, gradient %.3e; decisions %r"
          % (Aw.shape[0], M, lam, worst, worst_g, [a for a, _, _ in ref]))


def test_potential_trajectory_and_chain_against_the_restatement(G):
    mv, obs, dobs, _ = _small(G)
    assert mv._engine.sweep_layout()["tw"] == 1
    _check_against_restatement(G, mv, dobs, SHAPE)
    mv._engine.close()


@pytest.mark.parametrize("nx,ny", [(60, 35), (90, 70)])
def test_potential_trajectory_and_chain_on_the_multi_wave_sweeps(G, nx, ny):
    """2100 rows (4-wave teams) and 6300 rows (16-wave teams) over 3 x 720 columns: the epilogue that leaves partials
    (N >= 2048), with and without the amplitude term."""
    mrange, mspacing, shape = (0, 2000, 0, 3000, 0, 900), (150, 250, 200), (6, 12, 10)
    obs = _obs(nx, ny)
    n = obs[0].size
    dobs, _ = _data(G, obs, mrange, mspacing, shape, (slice(2, None), slice(4, 8), slice(3, 7)), seed=13)
    mv = _module(G, obs, dobs, mrange, mspacing)
    lay = mv._engine.sweep_layout()
    print("rows %d, sweep layout %r" % (n, lay))
    assert n >= 2048 and lay["tw"] == (4 if n <= 4096 else 16) and lay["n_panels"] == 1 and lay["grid"] > 64
    assert mv.Aw.shape == (n, 2160)
    _check_against_restatement(G, mv, dobs, shape, n_chain=3, n_over=1)
    _check_against_restatement(G, mv, dobs, shape, lam=0.6, n_chain=3, n_over=1)
    mv._engine.close()


# ----------------------------------------------------------------------------- 5. the stencil per property

def test_the_stencil_acts_on_each_property_alone(G):
    mv, obs, dobs, _ = _small(G)
    eng = mv._engine
    m = 48
    wm = mv.Wm.diagonal()
    zero = np.zeros(3 * m)
    # flat within each property, jumps between the blocks: nothing crosses a block boundary
    x = np.repeat([1.0, -5.0, 40.0], m)
    for kind in ("Smoothness", "TV"):
        v, g = eng.reg_eval(kind, x, zero, beta=1e-300 if kind == "TV" else 0.01, shape=SHAPE)
        assert abs(v) <= 1e-100 and np.abs(g).max() <= 1e-100, kind
    # smooth within each property: the value of the three blocks summed
    rng = np.random.default_rng(2)
    k, j, i = np.meshgrid(np.arange(3), np.arange(4), np.arange(4), indexing="ij")
    ramp = (0.3 * k + 0.1 * j - 0.2 * i).ravel()
    x = np.concatenate([ramp, 5.0 - 2.0 * ramp, 40.0 + 0.5 * ramp * ramp])
    for kind in REGS:
        v, g = eng.reg_eval(kind, x, zero, beta=0.01, shape=SHAPE)
        vr, gr = regulariser(kind, x, zero, wm * wm, 0.01, SHAPE)
        one = [eng.reg_eval(kind, np.concatenate([x[h * m:(h + 1) * m]] * 3), zero, beta=0.01, shape=SHAPE)[0]
               for h in range(3)]
        assert abs(v - vr) <= 1e-12 * abs(vr) and relmax(g, gr) <= 1e-12, kind
        if kind in ("Smoothness", "TV", "Damping"):                 # (MS weighs with Wm^2, which differs per block)
            assert abs(v - sum(one) / 3.0) <= 1e-12 * abs(v), kind
    # a shape whose product is M, not M/3
    with pytest.raises(ValueError):
        eng.reg_eval("Smoothness", x, zero, shape=(9, 4, 4))
    with pytest.raises(ValueError):
        eng.set_reg("TV", 1.0, 0.01, (9, 4, 4), zero)
    with pytest.raises(ValueError):
        eng.set_reg("Smoothness", 1.0, 0.01, (3, 4, 12), zero)
    eng.close()


# ----------------------------------------------------------------------------- 6. the amplitude term

def test_amplitude_term_against_the_restatement(G):
    mv, obs, dobs, truth = _small(G)
    eng = mv._engine
    wm = mv.Wm.diagonal()
    M = wm.size
    rng = np.random.default_rng(5)
    mwapr = 0.001 * wm
    x = rng.uniform(-0.02, 0.02, M) * wm
    args = (x, mwapr, None, None, "mandatory", 1000, 0.7)
    fresh = {reg: mv.misfit_and_grad(*args, regulization=reg, beta=0.001) for reg in REGS}
    assert mv.last_amplitude == 0.0
    # the term alone: value, gradient and amplitudes, for the physical model and for mw
    for beta, scale in ((0.05, 1.0), (2.0, 0.3)):
        eng.set_amplitude(0.0, beta, scale)
        phi, grad, amp = eng.amplitude_eval(x)
        pr, gr, ar = amplitude_term(x, wm, beta, scale)
        assert abs(phi - pr) <= 1e-12 * pr and relmax(grad, gr) <= 1e-12 and relmax(amp, ar) <= 1e-12
        assert eng.amplitude_eval(x, want_grad=False, want_amp=False)[1:] == (None, None)
    mv.set_amplitude(0.0, 0.05)
    model = x / wm
    phi, grad, amp = mv.Amplitude(model)
    pr, gr, ar = amplitude_term(x, wm, 0.05)
    assert abs(phi - pr) <= 1e-12 * pr and relmax(grad, gr * wm) <= 1e-12
    assert relmax(amp, mv.amplitude(model)) <= 1e-12 and relmax(amp, ar) <= 1e-12
    # switched on: U takes lambda Phi, out[4] stays R, amplitude_last returns Phi
    lam = 0.8
    mv.set_amplitude(lam, 0.05)
    for reg in REGS:
        a = mv.misfit_and_grad(*args, regulization=reg, beta=0.001)
        f = fresh[reg]
        assert a[4] == f[4] and a[3] == f[3] and np.array_equal(a[2], f[2])
        assert abs(mv.last_amplitude - pr) <= 1e-12 * pr
        assert abs(a[0] - (f[0] + lam * pr)) <= 1e-12 * abs(a[0])
        assert relmax(a[1], f[1] + lam * gr) <= 1e-11
    # switched off again: bit-identical to the context that never had it
    mv.set_amplitude(0.0)
    for reg in REGS:
        a = mv.misfit_and_grad(*args, regulization=reg, beta=0.001)
        f = fresh[reg]
        assert a[0] == f[0] and a[3] == f[3] and a[4] == f[4]
        assert np.array_equal(a[1], f[1]) and np.array_equal(a[2], f[2])
        assert mv.last_amplitude == 0.0
    # errors
    for bad in ((-1.0, 0.05, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, 0.05, 0.0), (np.nan, 0.05, 1.0)):
        with pytest.raises(ValueError):
            eng.set_amplitude(*bad)
    eng.close()
    # before gh_weight: an argument error; on any other store: unsupported
    mesh = G.mesher.PrismMesh(MRANGE, MSPACING)
    e2 = _mvi_engine(G, obs[0], obs[1], obs[2], mesh.cell_bounds(), *MANGLE)
    e2.build_G()
    with pytest.raises(ValueError, match="gh_weight"):
        e2.set_amplitude(1.0, 0.05)
    e2.close()
    tf = _tf_engine(G, obs[0], obs[1], obs[2], mesh.cell_bounds(), *MANGLE)
    tf.build_G()
    tf.weight(0.5)
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        tf.set_amplitude(1.0, 0.05)
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        tf.amplitude_eval(np.zeros(48))
    tf.close()


def test_the_amplitude_term_follows_a_new_weighting(G):
    """Assembled and weighted again with another weightfactor, the term set before uses the NEW 1 / Wm."""
    obs = _obs()
    mesh = G.mesher.PrismMesh(MRANGE, MSPACING)
    eng = _mvi_engine(G, obs[0], obs[1], obs[2], mesh.cell_bounds(), *MANGLE)
    eng.build_G()
    wm = eng.weight(0.5)
    eng.set_amplitude(0.7, 0.05, 2.0)
    x = np.random.default_rng(4).normal(size=wm.size) * 0.3 * wm
    eng.build_G()
    wm2 = eng.weight(0.3)
    assert relmax(wm2, wm) > 0.1
    phi, grad, amp = eng.amplitude_eval(x)
    pr, gr, ar = amplitude_term(x, wm2, 0.05, 2.0)
    assert abs(phi - pr) <= 1e-12 * pr and relmax(grad, gr) <= 1e-12 and relmax(amp, ar) <= 1e-12
    eng.close()


def test_chain_with_the_amplitude_term_against_the_restatement(G):
    mv, obs, dobs, _ = _small(G, amplitude=0.6, amplitude_beta=0.05)
    _check_against_restatement(G, mv, dobs, SHAPE, lam=0.6, amp_beta=0.05)
    # the chain must be started again after the term changes
    eng = mv._engine
    mv.set_amplitude(0.3)
    with pytest.raises(ValueError):
        eng.chain_trajectory(np.zeros(eng.M), 0.02, 3, 0.5)
    eng.close()


# ----------------------------------------------------------------------------- 7. HMCSample end to end

def test_hmcsample_end_to_end(G, tmp_path, capsys):
    """Data of a body magnetized away from the field.  The restatement runs the same chain with the sampler's own
    draws -- np.random.seed(seed + rank), then per trajectory randint for L, randn(M) * Sigma, rand (hmc.py) -- and
    formats its potentials as the sampler does: the printed lines must be equal, digit for digit."""
    mv, obs, dobs, truth = _small(G, amplitude=0.5, amplitude_beta=0.05)
    M = mv.Wm.shape[0]
    wm = mv.Wm.diagonal()
    mmax, dt, Sigma, seed, nsamples, ndraws, Lrange = 2.0, 0.02, 0.3, 100, 6, 2, [3, 8]
    folder = str(tmp_path / "run_chain")
    capsys.readouterr()
    G.HMCSample(mv, nsamples, ndraws, dt, Lrange, np.full(M, 0.001), np.full(M, 0.001),
                np.c_[np.full(M, -mmax), np.full(M, mmax)], "mandatory", 1000, mv.dobs,
                "Fixed", 0.8, 1.0, "TV", 0.001, seed, Sigma, nbest=100, myrank=0, save_folder=folder)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
    Aw = np.array(mv._engine.download_G())
    P = MagVectorProblem(Aw, dobs, 0.001 * wm, "TV", 1.0, 0.001, wm=wm, shape=SHAPE, lam=0.5, amp_beta=0.05)
    rs = np.random.RandomState(seed)
    x, i, ncount, ref_lines, ref_misfit, ref_model = 0.001 * wm, 0, 0, [], [], []
    while i < ndraws + nsamples:
        L = rs.randint(Lrange[0], Lrange[1] + 1)
        p0 = rs.randn(M) * Sigma
        u = rs.rand()
        x, acc, o = P.leapfrog(x, p0, dt, int(L), -mmax * wm, mmax * wm, u)
        ud, um = o[1] / dobs.size, o[2] / M
        if acc:
            if i >= ndraws:
                ref_misfit.append([o[0], o[1], o[2], ud + 1.0 * um, ud, um, 1.0])
                ref_model.append(x / wm)
            i += 1
        ncount += 1
        ref_lines.append("chain {}: {:.2%}, misfit(total, data, alpha, model)=({:.7f},{:.7f},{:.2f},{:.7f}) "
                         "-- accept ratio {:.2%}".format(0, i / (ndraws + nsamples), ud + 1.0 * um, ud, 1.0, um,
                                                         i / ncount))
    assert lines == ref_lines
    model = np.loadtxt(folder + "0/model.dat")
    misfit = np.loadtxt(folder + "0/misfit.dat")
    assert model.shape == (nsamples, M) and misfit.shape == (nsamples, 7)
    np.testing.assert_allclose(misfit, np.array(ref_misfit), atol=2e-8, rtol=1e-9)
    np.testing.assert_allclose(model, np.array(ref_model), atol=2e-8)
    assert np.all(np.abs(model) <= mmax)
    # the sampled vectors: amplitude and direction per cell
    v = mv.to_vectors(model[-1])
    assert v.shape == (48, 3) and np.array_equal(mv.from_vectors(v), model[-1])
    inc, dec = mv.direction(model[-1])
    assert inc.shape == dec.shape == (48,) and relmax(mv.amplitude(model[-1]), np.linalg.norm(v, axis=1)) <= 1e-14
    mv._engine.close()


# ----------------------------------------------------------------------------- 8. refusals

def test_refusals(G):
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    obs = _obs()
    n = obs[0].size
    mesh = G.mesher.PrismMesh(MRANGE, MSPACING)
    cells = mesh.cell_bounds()
    dobs = np.random.default_rng(0).normal(size=n)
    for kw in ({"coordinate": "spherical"}, {"wavelet": "3D"}, {"matrix_free": True}, {"shift_invariant": True},
               {"shard": object()}):
        with pytest.raises(NotImplementedError, match="magnetization-vector"):
            _module(G, obs, dobs, **kw)
    mv = _module(G, obs, dobs)
    M = mv.Wm.shape[0]
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        G.HMCSampleBatch(mv, 2, 2, 0, 0.02, [3, 8], np.zeros((2, M)), np.zeros(M), np.c_[-np.ones(M), np.ones(M)],
                         "mandatory", 1000, dobs, "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)
    eng = mv._engine
    h = eng._h
    assert not eng.fold_info()["on"]
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        eng.compress_wavelet(3, SHAPE, 0.001, 2)
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        eng.upload_G(np.zeros((n, M)))
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        eng.batch_init(np.zeros((2, M)), -np.ones(M), np.ones(M))
    ident = (C.c_char * 128)()
    for fn, args in (("gh_shard_init", (ident, 0, 2, C.c_int64(2 * M), C.c_int64(0))),
                     ("gh_shard_init_rows", (ident, 0, 2, C.c_int64(2 * n), C.c_int64(0)))):
        assert getattr(lib, fn)(h, *args) == _lib.GH_ERR_UNSUPPORTED
        assert b"magnetization-vector" in lib.gh_last_error(h)
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        eng.set_cells(np.tile(cells, (3, 1)), _lib.CELL_PRISM)              # the context takes no other kind
    eng.close()
    e = G.Engine(n, cells.shape[0])
    with pytest.raises(ValueError, match="kind must be"):
        e.set_cells(cells, _lib.CELL_PRISM_MVI)                             # gh_set_cells refuses the new kind
    e.close()
    # matrix-free asked for before the cells, the cells asked for late, M not a multiple of 3, too many rows
    e = G.Engine(n, 3 * cells.shape[0])
    e.set_matrix_free(True)
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        e.set_cells_mvi(cells, (0.0, 0.0, 1.0))
    e.close()
    e = G.Engine(n, 3 * cells.shape[0])
    e.set_cells_mvi(cells, (0.0, 0.0, 1.0))
    for post in ("set_matrix_free", "set_shift_invariant"):
        with pytest.raises(NotImplementedError, match="magnetization-vector"):
            getattr(e, post)(True)
    e.close()
    e = G.Engine(n, 3 * cells.shape[0])
    e.set_obs(*obs)
    with pytest.raises(ValueError):
        e.set_cells_mvi(cells, (0.0, 0.0, 1.0))                              # not a fresh context
    e.close()
    e = G.Engine(n, 3 * cells.shape[0] + 1)
    assert lib.gh_set_cells_mvi(e._h, _lib.ptr(np.ascontiguousarray(cells)), 0.0, 0.0, 1.0) == _lib.GH_ERR_ARG
    e.close()
    e = G.Engine(16385, 3 * cells.shape[0])
    with pytest.raises(NotImplementedError, match="magnetization-vector"):
        e.set_cells_mvi(cells, (0.0, 0.0, 1.0))
    e.close()
    # gh_tf_result keeps refusing what is not a magnetic model
    e = G.Engine(n, cells.shape[0])
    e.set_obs(*obs)
    e.set_cells(cells, _lib.CELL_PRISM)
    with pytest.raises(ValueError):
        e.tf_result(np.zeros((cells.shape[0], 3)))
    e.close()


# ----------------------------------------------------------------------------- 9. a carved mesh

def test_carved_mesh_with_damping_and_ms(G):
    obs = _obs()
    xs, ys = np.meshgrid(np.linspace(0, 2000, 9), np.linspace(0, 3000, 9))
    topo = np.where(xs.ravel() < 1000, -350.0, 100.0)             # the surface dips into the mesh on one side
    dobs, _ = _data(G, obs, MRANGE, MSPACING, SHAPE, (slice(1, None), slice(1, 3), slice(1, 3)))
    mv = _module(G, obs, dobs, mtopo=(xs.ravel(), ys.ravel(), topo))
    M = mv.Wm.shape[0]
    cells = M // 3
    assert mv.topocarve and M % 3 == 0 and 0 < cells < 48 and mv.Aw.shape == (obs[0].size, M)
    eng = mv._engine
    Aw = np.array(eng.download_G())
    wm = mv.Wm.diagonal()
    rng = np.random.default_rng(3)
    mwapr = 0.001 * wm
    x = rng.uniform(-0.02, 0.02, M) * wm
    for reg in ("Damping", "MS"):
        P = MagVectorProblem(Aw, dobs, mwapr, reg, 0.7, 0.001, wm=wm)
        a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        ev, eg = _errs(a, P.misfit_and_grad(x))
        assert max(ev) <= 1e-12 and eg <= 1e-11, (reg, ev, eg)
    for reg in ("Smoothness", "TV"):
        with pytest.raises(ValueError, match="uncarved"):
            mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
    assert mv.to_vectors(x).shape == (cells, 3)
    # the amplitude term needs no mesh: it works on the carved model too
    mv.set_amplitude(0.4, 0.05)
    a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization="MS", beta=0.001)
    P = MagVectorProblem(Aw, dobs, mwapr, "MS", 0.7, 0.001, wm=wm, lam=0.4, amp_beta=0.05)
    ev, eg = _errs(a, P.misfit_and_grad(x))
    assert max(ev) <= 1e-12 and eg <= 1e-11
    eng.close()
