"""GPU suite of the vector magnetic data: gravmag.prism.bx / by / bz and MagVectorModule(data=...) on the
GH_CELL_PRISM_MVI_DATA store -- columns and results against the reference's fixtures, bit equality with today's
magnetization-vector store, the stacked store, weights, per-block means, potential, amplitude term, trajectories and a
chain against the NumPy restatement (tests/magvecdata_host.py), the direction of a remanent body, and the refusals.

Shapes: n_obs 37, 64, 65 (stacked blocks of 111, 192, 195 rows start off and on a 64-row boundary, the stack ends
mid-tile); meshes of 4 x 3 x 2 and 5 x 3 x 3 cells (M = 72 and 135) and one carved mesh.

Tolerances.  Columns and results against the reference: 1e-10 max|K|, what tests/test_gpu_magnetic.py and
tests/test_gpu_magvector.py allow the tf entries against _prism.tf (no b component needs more).  The stacked store, Wm,
Wb and the blocks' means against the restatement: 1e-10 (tests/test_gpu_multicomp.py).  Potential values and the
prediction 1e-12, the gradient 1e-11; trajectories and chains 1e-10 (tests/test_gpu_magvector.py)."""
import numpy as np
import pytest

from conftest import gold
from helpers import relmax
from magvecdata_host import (COMPS, DIR_ALPHA, DIR_ITERS, VecDataProblem, cg_invert, cos_moment, direction_case, stack,
                             std_weights)

pytestmark = pytest.mark.gpu

REGS = ("Damping", "MS", "Smoothness", "TV")
BCOMPS = ("bx", "by", "bz")
BASE = {"tf": 4.0, "bx": -700.0, "by": 300.0, "bz": 55.0}      # clearly different block means (uT)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def Z():
    z = gold("mvi_vecdata_module.npz")
    return z, {c: z["K_" + c] for c in COMPS}


def _prisms(G, cells, mags):
    out = []
    for b, m in zip(cells, mags):
        p = G.mesher.Prism(*[float(v) for v in b])
        if m is not None:
            p.addprop("magnetization", m)
        out.append(p)
    return out


# ----------------------------------------------------------------------------- 1. columns and results

@pytest.mark.parametrize("comp", BCOMPS)
def test_columns_and_results_against_the_reference(G, comp):
    g = gold("prism_bxyz_cases.npz")
    xp, yp, zp, cells, mag = g["xp"], g["yp"], g["zp"], g["cells"], g["mag"]
    m, ns = cells.shape[0], int(g["n_singular"])
    fn = getattr(G.prism, comp)
    res, K = fn(xp, yp, zp, _prisms(G, cells, list(mag)))
    assert K.shape == (xp.size, 3 * m) and np.isfinite(K).all()
    for a in range(3):
        ref = g["K_%s_%d" % (comp, a)]
        blk = K[:, a * m:(a + 1) * m]
        err = np.abs(blk - ref).max() / np.abs(ref).max()
        err_s = np.abs(blk[:ns] - ref[:ns]).max() / np.abs(ref).max()
        print("%s, axis %s: max |dK|/max|K| = %.3e (singular points %.3e)" % (comp, "xyz"[a], err, err_s))
        assert err <= 1e-10, (comp, a, err)
    assert relmax(res, g["res_vec_" + comp]) <= 1e-10
    # a cell without the property is skipped: no columns of it, no share in the result
    skip = [mag[0], mag[1], None, mag[3]]
    res, K9 = fn(xp, yp, zp, _prisms(G, cells, skip))
    keep = [c for c in range(m) if c != int(g["skipped"])]
    assert K9.shape == (xp.size, 9) and np.array_equal(K9, K[:, [a * m + c for a in range(3) for c in keep]])
    assert relmax(res, g["res_skip_" + comp]) <= 1e-10
    # pmag replaces every cell's property, the skipped cell's too; no kernel on request
    res, none = fn(xp, yp, zp, _prisms(G, cells, skip), pmag=list(g["pvec"]), return_kernel=False)
    assert none is None and relmax(res, g["res_pmag_" + comp]) <= 1e-10
    with pytest.raises(ValueError):
        fn(xp, yp, zp, _prisms(G, cells, [None] * m))


def test_mesh_results_and_the_symmetric_columns(G, Z):
    z, K = Z
    mesh = G.mesher.PrismMesh(tuple(z["mrange"]), tuple(z["mspacing"]))
    assert np.array_equal(mesh.cell_bounds(), z["cells"])
    mesh.addprop("magnetization", z["vec"])
    got = {}
    for comp in BCOMPS:
        res, got[comp] = getattr(G.prism, comp)(z["xp"], z["yp"], z["zp"], mesh)
        assert relmax(res, z["d_" + comp]) <= 1e-10
        assert relmax(got[comp], np.hstack(list(K[comp]))) <= 1e-10
    # one second derivative serves bx's y column and by's x column: the same sums, the same bits
    m = 24
    assert np.array_equal(got["bx"][:, m:2 * m], got["by"][:, :m])
    assert np.array_equal(got["bx"][:, 2 * m:], got["bz"][:, :m])
    assert np.array_equal(got["by"][:, 2 * m:], got["bz"][:, m:2 * m])


# ----------------------------------------------------------------------------- 2. equality with the MVI store

def _trajs(rng, M, n):
    return [(int(rng.integers(2, 7)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(n)]


def test_the_total_field_alone_is_todays_store_bit_for_bit(G, Z):
    from gravinv3dhmc_amd import utils
    z, _ = Z
    n = 37
    obs = (z["xp"][:n], z["yp"][:n], z["zp"][:n])
    mrange, mspacing, mangle = tuple(z["mrange"]), tuple(z["mspacing"]), tuple(z["mangle"])
    dobs = z["d_tf"][:n] + 4.0
    old = G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=mangle, verbose=False)
    dflt = G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=mangle, data=("tf",), verbose=False)
    new = G.MagVectorModule([dobs], mrange, mspacing, obs, mangle=mangle, data=("tf",), weights=[1.0], verbose=False)
    assert not dflt._vector and new._vector
    M = 72
    rng = np.random.default_rng(11)
    wm = old.Wm.diagonal()
    mwapr, x = 0.001 * wm, rng.uniform(-0.02, 0.02, M) * wm
    trajs = _trajs(rng, M, 4)
    ref = None
    for mv in (old, dflt, new):
        out = [np.asarray(mv.Aw), mv.Wm.diagonal(), mv.forward(x / wm)]
        mv.set_amplitude(0.4, 0.05)
        for reg in REGS:
            a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            out += [np.asarray(v, dtype=np.float64) for v in a]
        eng = mv._engine
        eng.set_reg("TV", 1.0, 0.001, tuple(z["shape"]), mwapr)
        eng.chain_init(mwapr, -0.02 * wm, 0.02 * wm)
        eng.run_chain(iter(trajs), 0.005, lambda L, acc, o, xx: out.extend([np.array(float(acc)), o.copy()]))
        out.append(eng.chain_get_x())
        if ref is None:
            ref = out
        else:
            assert len(out) == len(ref) and all(np.array_equal(p, q) for p, q in zip(out, ref))
        eng.close()
    # a tf block beside another component: before the weighting, bit for bit the MVI store; the bz block prism.bz's
    cells = z["cells"]
    f = utils.dircos(*mangle)
    e1 = G.Engine(n, M)
    e1.set_cells_mvi(cells, f)
    e1.set_obs(*obs)
    e1.build_G()
    e2 = G.Engine(2 * n, M)
    e2.set_cells_mvi_data(cells, f, ("tf", "bz"), (1.0, 1.0))
    e2.set_obs(*obs)
    e2.build_G()
    S = e2.download_G()
    assert np.array_equal(S[:n], e1.download_G())
    mesh = G.mesher.PrismMesh(mrange, mspacing)
    mesh.addprop("magnetization", z["vec"])
    assert np.array_equal(S[n:], G.prism.bz(*obs, mesh)[1])
    info = e2.multi_info()
    assert info["components"] == [0, 3] and np.array_equal(info["weights"], [1.0, 1.0])
    e1.close()
    e2.close()


# ----------------------------------------------------------------------------- 3. the restatement

def _errs(a, b):
    return [abs(a[0] - b[0]) / abs(b[0]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
            abs(a[4] - b[4]) / max(abs(b[4]), 1e-300)], relmax(a[1], b[1])


def _check_against_restatement(mv, data, w, dobs, shape, A_ref=None, regs=REGS, lam=0.4, amp_beta=0.05):
    """mv against VecDataProblem on the store downloaded from the device.  A_ref: the unweighted stack of reference
    columns, where the fixture has them."""
    eng = mv._engine
    nc, n = len(data), mv._n
    Aw = np.array(eng.download_G())
    wm = mv.Wm.diagonal()
    M = wm.size
    wb = np.repeat(w, n)
    assert Aw.shape == (nc * n, M) and relmax(mv.weights, w) <= 1e-10 and relmax(mv.Wb.diagonal(), wb) <= 1e-10
    dobsw = wb * np.concatenate(dobs)
    assert relmax(mv.dobsw, dobsw) <= 1e-10 and np.array_equal(mv.dobs, np.concatenate(dobs))
    if A_ref is not None:
        WA = A_ref * wb[:, None]
        assert relmax(wm, np.sqrt((WA ** 2).sum(axis=0))) <= 1e-10
        assert relmax(Aw * wm[None, :], WA) <= 1e-10 and relmax(mv.A, A_ref) <= 1e-10
        m = M // 3
        for b, comp in enumerate(data):
            for a in range(3):
                assert relmax(mv.kernel("xyz"[a], comp), A_ref[b * n:(b + 1) * n, a * m:(a + 1) * m]) <= 1e-10
        assert relmax(mv.kernel(1), A_ref[:, m:2 * m]) <= 1e-10
    else:
        assert relmax(wm, np.sqrt(((Aw * wm[None, :]) ** 2).sum(axis=0))) <= 1e-10
    with pytest.raises(ValueError):
        mv.kernel(0, "gz")
    rng = np.random.default_rng(7)
    mwapr = 0.001 * wm
    model = rng.normal(size=M)
    assert relmax(mv.forward(model), (Aw @ (model * wm)) / wb) <= 1e-10
    worst = worst_g = worst_m = 0.0
    for amp in (0.0, lam):
        if amp > 0:
            mv.set_amplitude(amp, amp_beta)
        for reg in regs:
            P = VecDataProblem(Aw, dobsw, nc, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape, lam=amp, amp_beta=amp_beta)
            Pg = VecDataProblem(Aw, dobsw, nc, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape, lam=amp, amp_beta=amp_beta,
                                global_mean=True)
            x = rng.uniform(-0.02, 0.02, M) * wm
            a = mv.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            b = P.misfit_and_grad(x)
            ev, eg = _errs(a, b)
            pm, om = mv.block_means()
            em = max(relmax(pm, P.pred_mean), relmax(om, P.obs_mean))
            worst, worst_g, worst_m = max(worst, max(ev)), max(worst_g, eg), max(worst_m, em)
            assert max(ev) <= 1e-12 and eg <= 1e-11 and em <= 1e-10, (data, reg, amp, ev, eg, em)
            if amp > 0:
                assert abs(mv.last_amplitude - P.phi) <= 1e-12 * P.phi
                assert abs(a[0] - (a[3] + 0.7 * a[4] + amp * mv.last_amplitude)) <= 1e-12 * abs(a[0])
            else:
                assert mv.last_amplitude == 0.0
            # sharpness: ONE mean over all rows is far outside the tolerance (several blocks), as is a dropped weight
            if nc > 1:
                assert abs(a[0] - Pg.misfit_and_grad(x)[0]) > 1e-3 * abs(a[0])
            if w[-1] != 1.0:
                wd = np.repeat(list(w[:-1]) + [1.0], n)
                Pd = VecDataProblem(Aw, wd * np.concatenate(dobs), nc, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape,
                                    lam=amp, amp_beta=amp_beta)
                assert abs(a[0] - Pd.misfit_and_grad(x)[0]) > 1e-3 * abs(a[0])
    # trajectories with given momenta, the amplitude term on: a step half the stability limit of the term's curvature
    # 2 lam / (amp_beta min(wm)^2) (tests/test_gpu_magvector.py), worked out from wm
    reg = regs[-1]
    dt = min(0.02, 1.0 / np.sqrt(2.0 * lam / (amp_beta * wm.min() ** 2)))
    low, high = -0.02 * wm, 0.02 * wm
    P = VecDataProblem(Aw, dobsw, nc, mwapr, reg, 1.0, 0.001, wm=wm, shape=shape, lam=lam, amp_beta=amp_beta)
    eng.set_reg(reg, 1.0, 0.001, shape, mwapr)
    for L, p0, u, step in ((8, rng.normal(size=M) * 3.0, 1.0 - 1e-9, 0.02), (6, rng.normal(size=M) * 0.3, 0.0, dt),
                           (3, rng.normal(size=M) * 0.3, 0.5, dt)):
        xg, acc, o, _ = eng.leapfrog(mwapr, p0, step, L, low, high, u)
        xo, acco, oo = P.leapfrog(mwapr, p0, step, L, low, high, u)
        assert acc == acco and relmax(o, oo) <= 1e-10 and relmax(xg, xo) <= 1e-10
    trajs = [(int(rng.integers(1, 7)), rng.normal(size=M) * 0.3, 0.0), (8, rng.normal(size=M) * 3.0, 1.0 - 1e-9),
             (int(rng.integers(1, 7)), rng.normal(size=M) * 0.3, float(rng.uniform()))]
    ref = P.chain(mwapr, trajs, dt, low, high)
    eng.chain_init(mwapr, low, high)
    res = []
    eng.run_chain(iter(trajs), dt, lambda L, acc, o, x: res.append((acc, o.copy(), x)), want_x=True)
    assert len(res) == len(ref) and any(a for a, _, _ in ref) and any(not a for a, _, _ in ref)
    for (a1, o1, x1), (a2, o2, x2) in zip(res, ref):
        assert a1 == a2 and relmax(o1, o2) <= 1e-10 and (x1 is None or relmax(x1, x2) <= 1e-10)
    assert relmax(eng.chain_get_x(), ref[-1][2]) <= 1e-10
    assert eng.chain_stats()["resident_launches"] == 0 and not eng.fold_info()["on"]
    print("%r, %d x %d rows, M = %d: worst value %.3e, gradient %.3e, means %.3e; decisions %r"
          % (data, nc, n, M, worst, worst_g, worst_m, [a for a, _, _ in ref]))


CASES = [(("bx", "by", "bz"), "std"), (("tf", "bz"), (1.0, 2.5)), (("bz",), (0.5,))]


@pytest.mark.parametrize("n", [37, 64, 65])
@pytest.mark.parametrize("data,weights", CASES, ids=["bxyz", "tf_bz", "bz"])
def test_module_against_the_restatement(G, Z, data, weights, n):
    z, K = Z
    obs = (z["xp"][:n], z["yp"][:n], z["zp"][:n])
    dobs = [z["d_" + c][:n] + BASE[c] for c in data]
    w = std_weights(dobs) if weights == "std" else np.array(weights)
    mv = G.MagVectorModule(dict(zip(data, dobs)) if n == 64 else dobs, tuple(z["mrange"]), tuple(z["mspacing"]), obs,
                           mangle=tuple(z["mangle"]), data=data, weights=weights, verbose=False)
    assert mv.components == data and mv.Aw.shape == (len(data) * n, 72) and mv.mshape == tuple(z["shape"])
    A_ref = stack(K, data, w, n=n)[3]
    _check_against_restatement(mv, data, w, dobs, tuple(int(v) for v in z["shape"]), A_ref)
    mv._engine.close()


def _device_columns(G, obs, mesh, data, mangle):
    """the unweighted stack from the single-field front-ends (each held to the reference in test 1 and in
    tests/test_gpu_magvector.py)"""
    from gravinv3dhmc_amd import utils
    cells = mesh.cell_bounds(active_only=True)
    blocks = []
    for comp in data:
        if comp == "tf":
            e = G.Engine(obs[0].size, 3 * cells.shape[0])
            e.set_cells_mvi(cells, utils.dircos(*mangle))
            e.set_obs(*obs)
            e.build_G()
            blocks.append(np.array(e.download_G()))
            e.close()
        else:
            blocks.append(np.array(getattr(G.prism, comp)(*obs, mesh, pmag=[1.0, 0.0, 0.0])[1]))
    return np.vstack(blocks)


def test_second_mesh_with_a_column_count_off_the_tile(G, Z):
    """5 x 3 x 3 cells: M = 135, no multiple of the column tile; 37 points"""
    z, _ = Z
    n = 37
    obs = (z["xp"][:n], z["yp"][:n], z["zp"][:n])
    mrange, mspacing, mangle = (0, 2000, 0, 3000, 0, 900), (300, 1000, 400), tuple(z["mangle"])
    mesh = G.mesher.PrismMesh(mrange, mspacing)
    assert mesh.shape == (3, 3, 5)
    rng = np.random.default_rng(5)
    data = ("tf", "bx", "by", "bz")
    A = _device_columns(G, obs, mesh, data, mangle)
    truth = rng.normal(size=135)
    dobs = [A[b * n:(b + 1) * n] @ truth + BASE[c] for b, c in enumerate(data)]
    mv = G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=mangle, data=data, weights="std", verbose=False)
    assert mv.Aw.shape == (4 * n, 135)
    _check_against_restatement(mv, data, std_weights(dobs), dobs, (3, 3, 5), A)
    mv._engine.close()


def test_carved_mesh(G, Z):
    z, _ = Z
    n = 37
    obs = (z["xp"][:n], z["yp"][:n], z["zp"][:n])
    mrange, mspacing, mangle = tuple(z["mrange"]), tuple(z["mspacing"]), tuple(z["mangle"])
    xs, ys = np.meshgrid(np.linspace(0, 2000, 9), np.linspace(0, 3000, 9))
    topo = np.where(xs.ravel() < 1000, -500.0, 100.0)               # the surface dips into the mesh on one side
    data = ("bx", "by", "bz")
    dobs = [z["d_" + c][:n] + BASE[c] for c in data]
    mv = G.MagVectorModule(dobs, mrange, mspacing, obs, mangle=mangle, data=data, weights=(1.0, 0.5, 2.0),
                           mtopo=(xs.ravel(), ys.ravel(), topo), verbose=False)
    M = mv.Wm.shape[0]
    assert mv.topocarve and M % 3 == 0 and 0 < M // 3 < 24 and mv.Aw.shape == (3 * n, M)
    A = _device_columns(G, obs, mv.mesh, data, mangle)
    _check_against_restatement(mv, data, np.array([1.0, 0.5, 2.0]), dobs, None, A, regs=("Damping", "MS"))
    x = np.zeros(M)
    with pytest.raises(ValueError, match="uncarved"):
        mv.misfit_and_grad(x, x, None, None, "mandatory", 1000, 0.7, regulization="TV", beta=0.001)
    mv._engine.close()


# ----------------------------------------------------------------------------- 5. vector data recover the direction

def test_vector_data_recover_the_direction(G):
    """The restatement's inversion (tests/test_magvecdata_host.py: 40 conjugate-gradient steps on the quadratic
    potential, from gradients alone) with the device evaluating the gradient: the net moment of the recovered model
    points along the true one, as it does on the host, and the two models agree."""
    data = ("bx", "by", "bz")
    z, truth, dobs, P, wm_ref = direction_case(gold("mvi_vecdata_module.npz"), data)
    n = 65
    mv = G.MagVectorModule(dobs, tuple(z["mrange"]), tuple(z["mspacing"]), (z["xp"], z["yp"], z["zp"]),
                           mangle=tuple(z["mangle"]), data=data, verbose=False)
    wm = mv.Wm.diagonal()
    assert mv.Aw.shape == (3 * n, 72) and relmax(wm, wm_ref) <= 1e-10
    zero = np.zeros(72)
    grad = lambda x: mv.misfit_and_grad(x, zero, None, None, "mandatory", 1000, DIR_ALPHA, regulization="Damping")[1]
    got = cg_invert(grad, 72, DIR_ITERS) / wm
    host = cg_invert(lambda x: P.misfit_and_grad(x)[1], 72, DIR_ITERS) / wm_ref
    c, ch = cos_moment(got, truth), cos_moment(host, truth)
    print("cosine to the true net moment: device %.6f, restatement %.6f" % (c, ch))
    assert ch >= 0.99 and c >= 0.99
    inc, dec = mv.direction(got)
    amp = mv.amplitude(got)
    body = np.flatnonzero(np.abs(z["vec"]).sum(axis=1))
    assert set(np.argsort(amp)[-2:]) == set(body)
    mv._engine.close()


# ----------------------------------------------------------------------------- 6. refusals on a device context

def test_refusals(G, Z):
    from gravinv3dhmc_amd import _lib
    z, _ = Z
    cells = z["cells"]
    e = G.Engine(16386, 72)                                          # 3 x 5462 = 16386 > 16384 stacked rows
    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        e.set_cells_mvi_data(cells, None, ("bx", "by", "bz"), (1.0, 1.0, 1.0))
    e.close()
    e = G.Engine(16385, 72)
    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        e.set_cells_mvi_data(cells, None, ("bz",), (1.0,))
    e.close()
    for comps, w, N in ((("bx", "bx"), (1.0, 1.0), 74), (("bx", "by"), (1.0, 0.0), 74), (("bx", "by"), (1.0, 1.0), 75)):
        e = G.Engine(N, 72)
        with pytest.raises(ValueError):
            e.set_cells_mvi_data(cells, None, comps, w)
        e.close()
    e = G.Engine(74, 72)
    with pytest.raises(ValueError):
        e.set_cells_mvi_data(cells, None, ("tf", "bz"), (1.0, 1.0))  # a tf block needs the direction
    assert e._lib.gh_set_cells_mvi_data(e._h, _lib.ptr(np.ascontiguousarray(cells)), 0.0, 0.0, 1.0, 5,
                                        (_lib.C.c_int * 5)(0, 1, 2, 3, 1), _lib.ptr(np.ones(5))) == _lib.GH_ERR_ARG
    e.set_matrix_free(True)
    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        e.set_cells_mvi_data(cells, None, ("bx", "by"), (1.0, 1.0))
    e.close()
    n = 37
    obs = (z["xp"][:n], z["yp"][:n], z["zp"][:n])
    dobs = [z["d_" + c][:n] for c in BCOMPS]
    mv = G.MagVectorModule(dobs, tuple(z["mrange"]), tuple(z["mspacing"]), obs, data=BCOMPS, verbose=False)
    M = 72
    with pytest.raises(NotImplementedError, match="vector-data magnetization store"):
        G.HMCSampleBatch(mv, 2, 2, 0, 0.02, [3, 8], np.zeros((2, M)), np.zeros(M), np.c_[-np.ones(M), np.ones(M)],
                         "mandatory", 1000, mv.dobs, "Fixed", 0.8, 1.0, "Damping", 0.01, 1, 0.3)
    eng = mv._engine
    for call in (lambda: eng.set_matrix_free(True), lambda: eng.set_shift_invariant(True),
                 lambda: eng.compress_wavelet(3, tuple(z["shape"]), 0.001, 2), lambda: eng.upload_G(np.zeros((3 * n, M))),
                 lambda: eng.batch_init(np.zeros((2, M)), -np.ones(M), np.ones(M)),
                 lambda: eng.set_cells(np.tile(cells, (3, 1)), _lib.CELL_PRISM)):
        with pytest.raises(NotImplementedError, match="vector-data magnetization"):
            call()
    with pytest.raises(ValueError):
        eng.b_result("tf", z["vec"])                                 # the total field's result is tf_result's
    assert relmax(eng.b_result("by", z["vec"]), z["d_by"][:n]) <= 1e-10
    assert not eng.fold_info()["on"]
    eng.close()
