"""Generate the fixtures of the prism gravity components tests/golden/*_comp*.npz, *_gzz.npz from the reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_grav.py [name ...]
The files hold DATA only: inputs and the reference's outputs (_prism.<comp> columns, prism._<comp>
results, a gzz GravMagModule's weights and potential, HMCSample console lines and sample files).
Every array is a deterministic function of the seeds below: two runs write the same arrays.
(Not collected by pytest: the name does not start with test_.)

How the gradient module is pinned: the reference's GravMagModule inverts gz only (its gravity branch
calls prism.gz, inversion/potential.py:110-128), so there is no reference gzz module to run.  The
fixtures build the reference's gravity module on the small problem of make_golden_tf._small_problem,
then set `gm.A` to the reference's own `prism.gzz` kernel of the module's mesh and call the reference's
`sensitivityWeighting()` again.  Everything downstream of the kernel (the weights, misfit_and_grad, the
regularisers, HMCSample) is then the reference's own code on the gzz kernel.
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
#: every gravity field of prism.py:875-972, in GH_COMP_* order
COMPS = ("potential", "geoid", "gx", "gy", "gz", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")
#: the components of the C1 columns
C1_COMPS = ("gzz", "gxy", "gx")


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _scale(R, comp):
    """The factor prism._<comp> applies to kernel2d (prism.py:151,178,231,...,659)."""
    c = R.constants
    if comp == "potential":
        return c.G
    if comp == "geoid":
        return c.G / c.g0
    if comp in ("gx", "gy", "gz"):
        return c.G * c.SI2MGAL
    return c.G * c.SI2EOTVOS


def _columns(R, comp, xp, yp, zp, cells):
    """Columns of _prism.<comp> for the given cells, scaled as prism._<comp> scales kernel2d."""
    fn = getattr(R._prism, "potential" if comp == "geoid" else comp)   # (prism._geoid: prism.py:174)
    K = np.zeros((xp.size, len(cells)))
    for c, b in enumerate(cells):
        res, k1 = np.zeros(xp.size), np.zeros(xp.size)
        fn(xp, yp, zp, *[float(v) for v in b], 1.0, res, k1)
        K[:, c] = k1
    K *= _scale(R, comp)
    return K


def _ref_result(R, comp, xp, yp, zp, cells, dens_list, dens=None):
    """prism._<comp>'s `result` and kernel2d on a list of reference prisms; dens_list[c] None = no property."""
    prisms = []
    for b, d in zip(cells, dens_list):
        p = R.mesher.Prism(*[float(v) for v in b])
        if d is not None:
            p.addprop("density", d)
        prisms.append(p)
    kept = sum(1 for d in dens_list if d is not None or dens is not None)
    res, K = np.zeros(xp.size), np.zeros((xp.size, kept))
    getattr(R.prism, "_" + comp)(xp, yp, zp, res, K, prisms, dens)
    return res, K


def prism_comp_cases(R):
    """Singular and random (obs, cell) geometries through _prism.<comp> for all eleven components, plus
    prism._<comp> results with per-cell densities, a cell without the property and the dens override."""
    cells = np.array([[0, 100, 0, 100, 0, 100], [-50, 50, -30, 70, 10, 60],
                      [1000, 1100, 2000, 2100, 900, 1000], [0, 100, 0, 100, 100, 300.5]], dtype=float)
    pts = []
    for x in (-100.0, 0.0, 50.0, 100.0, 250.0):          # corners, edges, faces, outside
        for y in (-100.0, 0.0, 50.0, 100.0, 180.0):
            for z in (0.0, -10.0, 100.0, 50.0):
                pts.append((x, y, z))
    # x + r = 0 / y + r = 0 / z + r = 0 (the point in line with an edge, beyond the corner), dx*dy = 0
    pts += [(200.0, 0.0, 0.0), (0.0, 200.0, 0.0), (0.0, 0.0, 300.0), (100.0, 250.0, 100.0),
            (250.0, 100.0, 100.0), (100.0, 100.0, -40.0), (50.0, 0.0, -5.0), (0.0, 50.0, -5.0)]
    # on the lines of the edges, on both sides of the prism: dx = dy = 0 with dz < 0 / dz > 0 (gxy's
    # perturbed distance, _prism.pyx:346-351), dx = dz = 0 with dy < 0 / > 0 (gxz, :380-385), dy = dz = 0
    # with dx < 0 / > 0 (gyz, :443-448) -- for cells 0 and 1
    pts += [(0.0, 0.0, 150.0), (100.0, 0.0, 400.0), (0.0, 100.0, -30.0), (100.0, 100.0, 1000.0),
            (0.0, 150.0, 0.0), (100.0, -60.0, 100.0), (0.0, 400.0, 100.0), (100.0, 300.0, 300.5),
            (150.0, 0.0, 0.0), (-80.0, 100.0, 100.0), (700.0, 100.0, 0.0), (-50.0, 0.0, 300.5),
            (-50.0, -30.0, 200.0), (50.0, 70.0, 0.0), (-50.0, 300.0, 10.0), (50.0, -90.0, 60.0),
            (400.0, -30.0, 10.0), (-60.0, 70.0, 60.0)]
    pts += [(1e4, 2e4, 0.0), (-3e3, 5.0, -200.0), (1050.0, 2050.0, 0.0), (33.3, 66.6, -0.01)]
    rng = np.random.default_rng(31)
    n = 120
    rnd = np.c_[rng.uniform(-500, 2500, n), rng.uniform(-500, 3500, n), -rng.uniform(0, 50, n)]
    pts = np.vstack([np.array(pts), rnd])
    xp, yp, zp = [np.ascontiguousarray(pts[:, i]) for i in range(3)]
    dens = rng.normal(size=len(cells)) * 2.0
    mixed = [float(dens[0]), float(dens[1]), None, float(dens[3])]
    out = dict(xp=xp, yp=yp, zp=zp, cells=cells, dens=dens, comps=np.array(COMPS))
    for comp in COMPS:
        K = _columns(R, comp, xp, yp, zp, cells)
        res, Kr = _ref_result(R, comp, xp, yp, zp, cells, list(dens))
        assert np.array_equal(Kr, K), "prism._%s's kernel2d differs from the scaled _prism.%s columns" % (comp, comp)
        out["K_" + comp] = K
        out["res_" + comp] = res
        # one cell without the property (skipped), and the dens override (every cell kept, the property ignored)
        out["res_mixed_" + comp], _ = _ref_result(R, comp, xp, yp, zp, cells, mixed)
        out["res_dens_" + comp], _ = _ref_result(R, comp, xp, yp, zp, cells, mixed, dens=2.5)
        print("prism_comp_cases", comp, K.shape, "finite:", np.isfinite(K).all(), "max|K| %.3e" % np.abs(K).max())
    out["SI2EOTVOS"] = np.array(R.constants.SI2EOTVOS)
    out["g0"] = np.array(R.constants.g0)
    np.savez_compressed(os.path.join(GOLD, "prism_comp_cases.npz"), **out)


def c1_comp_columns(R):
    """32 columns each of the gzz, gxy and gx kernels at C1's geometry (600 obs x 20x30x10 prisms)."""
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    zp = np.zeros_like(xp)
    mesh = _quiet(R.mesher.PrismMesh, (0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    mesh.addprop("density", np.zeros(mesh.size))
    out = {}
    rng = np.random.default_rng(6)
    for comp in C1_COMPS:
        _, K = getattr(R.prism, comp)(xp, yp, zp, mesh)
        cols = np.sort(rng.choice(K.shape[1], 32, replace=False))
        out["cols_" + comp] = cols
        out["K_" + comp] = np.ascontiguousarray(K[:, cols])
        print("c1_comp_columns", comp, K.shape, "->", out["K_" + comp].shape)
    np.savez_compressed(os.path.join(GOLD, "c1_comp_columns.npz"), **out)


def _small_problem(R):
    """make_golden_tf._small_problem's geometry and data on the reference's gravity module, re-weighted
    with the reference's gzz kernel (the docstring at the top)."""
    mrange, mspacing = (0, 2000, 0, 3000, 0, 1000), (250, 500, 400)
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 7), np.linspace(0, 2000, 6))]
    zp = np.zeros_like(xp)
    dobs = np.random.default_rng(0).normal(size=xp.size)
    gm = _quiet(R.potential.GravMagModule, dobs, mrange, mspacing, (xp, yp, zp))
    _, gm.A = R.prism.gzz(xp, yp, zp, gm.mesh)
    gm.sensitivityWeighting()
    del gm.A
    return gm, (xp, yp, zp), dobs, mrange, mspacing


def potential_small_gzz(R):
    gm, (xp, yp, zp), dobs, mrange, mspacing = _small_problem(R)
    wm = gm.Wm.diagonal()
    M = wm.size
    rng = np.random.default_rng(1)
    xs = np.stack([0.001 * wm, rng.uniform(0, 1, M) * wm, rng.uniform(-1, 1, M) * wm])
    mwapr = 0.001 * wm
    out = dict(xp=xp, yp=yp, zp=zp, dobs=dobs, Aw=np.asfortranarray(gm.Aw), wm=wm, xs=xs, mwapr=mwapr,
               shape=np.array(gm.mshape), mrange=np.array(mrange, float), mspacing=np.array(mspacing, float),
               component=np.array("gzz"), alpha=0.7, beta=0.001)
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        res = [gm.misfit_and_grad(x, mwapr, None, None, 'mandatory', 1000, 0.7, regulization=reg, beta=0.001)
               for x in xs]
        out[reg + "_misfit"] = np.array([r[0] for r in res])
        out[reg + "_grad"] = np.stack([r[1] for r in res])
        out[reg + "_dpre"] = np.stack([r[2] for r in res])
        out[reg + "_data"] = np.array([r[3] for r in res])
        out[reg + "_model"] = np.array([r[4] for r in res])
    np.savez_compressed(os.path.join(GOLD, "potential_small_gzz.npz"), **out)
    print("potential_small_gzz", gm.Aw.shape)


def chain_small_gzz(R):
    """Whole reference HMCSample runs on the small gzz module: console lines + sample files."""
    gm, _, dobs, _, _ = _small_problem(R)
    M = gm.Wm.shape[0]
    out = {}
    tmp = tempfile.mkdtemp(prefix="gold_gzz_")
    try:
        for tag, reg, dt, Sigma, lo, hi, n in (("a", "Damping", 0.01, 0.001, 0.0, 1.0, 12),
                                                ("b", "TV", 0.02, 0.3, 0.0, 0.02, 12)):
            folder = os.path.join(tmp, "hmc_%s_chain" % tag)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                R.hmc.HMCSample(gm, n, 0, dt, [5, 20], np.full(M, 0.001 + lo), np.full(M, 0.001),
                                np.c_[np.full(M, lo), np.full(M, hi)], "mandatory", 1000, dobs,
                                "Fixed", 0.8, 1.0, reg, 0.001, 100, Sigma, nbest=100, myrank=0,
                                save_folder=folder, plotsamples=False, im=[0, 0])
            lines = [l for l in buf.getvalue().splitlines() if l.startswith("chain ")]
            out[tag + "_lines"] = np.array(lines)
            out[tag + "_misfit"] = np.loadtxt(folder + "0/misfit.dat")
            out[tag + "_model"] = np.loadtxt(folder + "0/model.dat")
            out[tag + "_cfg"] = np.array([dt, Sigma, lo, hi, n])
            out[tag + "_reg"] = np.array(reg)
            print("chain_small_gzz", tag, len(lines), "lines; last:", lines[-1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(GOLD, "chain_small_gzz.npz"), **out)


def main():
    os.makedirs(GOLD, exist_ok=True)
    R = ref_harness.load()
    names = sys.argv[1:] or ["prism_comp_cases", "c1_comp_columns", "potential_small_gzz", "chain_small_gzz"]
    for name in names:
        globals()[name](R)
    return 0


if __name__ == "__main__":
    sys.exit(main())
