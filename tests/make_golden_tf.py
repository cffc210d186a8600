"""Generate the total-field magnetic fixtures tests/golden/*_tf.npz from the reference itself.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_tf.py [name ...]
The files hold DATA only: inputs and the reference's outputs (prism.tf / _prism.tf columns and
results, a magnetic GravMagModule's weights and potential, HMCSample console lines and sample
files).  Every array is a deterministic function of the seeds below: two runs write the same
arrays.  (Not collected by pytest: the name does not start with test_.)
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
DIRS = np.array([(90.0, 0.0), (0.0, 0.0), (60.0, -10.0), (-45.0, 120.0)])
#: (inc, dec) of the module and chain fixtures, and of the C1 columns
MANGLE = (60.0, -10.0)
C1_MANGLE = (50.0, 30.0)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _scale(R):
    return R.constants.CM * R.constants.T2NT


def _columns(R, xp, yp, zp, cells, inc, dec):
    """Columns of _prism.tf for the given cells, scaled as prism._tf scales kernel2d."""
    fx, fy, fz = R.prism.utils.dircos(inc, dec)
    K = np.zeros((xp.size, len(cells)))
    for c, b in enumerate(cells):
        res, k1 = np.zeros(xp.size), np.zeros(xp.size)
        R._prism.tf(xp, yp, zp, *[float(v) for v in b], 1.0, 1.0, 1.0, fx, fy, fz, res, k1)
        K[:, c] = k1
    K *= _scale(R)
    return K


def _ref_result(R, xp, yp, zp, cells, mags, inc, dec, pmag=None):
    """prism._tf's `result` (and kernel2d) on a list of reference prisms; mags[c] None = no property."""
    prisms = []
    for b, m in zip(cells, mags):
        p = R.mesher.Prism(*[float(v) for v in b])
        if m is not None:
            p.addprop("magnetization", m)
        prisms.append(p)
    kept = sum(1 for m in mags if m is not None or pmag is not None)
    res, K = np.zeros(xp.size), np.zeros((xp.size, kept))
    R.prism._tf(xp, yp, zp, res, K, prisms, inc, dec, pmag)
    return res, K


def prism_tf_cases(R):
    """Singular and random (obs, cell) geometries through _prism.tf at four field directions, plus
    prism._tf results for per-cell vectors, scalar intensities, a cell without the property and pmag."""
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
    pts += [(1e4, 2e4, 0.0), (-3e3, 5.0, -200.0), (1050.0, 2050.0, 0.0), (33.3, 66.6, -0.01)]
    rng = np.random.default_rng(21)
    n = 120
    rnd = np.c_[rng.uniform(-500, 2500, n), rng.uniform(-500, 3500, n), -rng.uniform(0, 50, n)]
    pts = np.vstack([np.array(pts), rnd])
    xp, yp, zp = [np.ascontiguousarray(pts[:, i]) for i in range(3)]
    out = dict(xp=xp, yp=yp, zp=zp, cells=cells, dirs=DIRS)
    mag = rng.normal(size=(len(cells), 3)) * 2.0
    scal = np.array([1.5, -0.75, 3.0, 0.25])
    for d, (inc, dec) in enumerate(DIRS):
        K = _columns(R, xp, yp, zp, cells, inc, dec)
        out["K%d" % d] = K
        res_v, Kv = _ref_result(R, xp, yp, zp, cells, list(mag), inc, dec)
        assert np.array_equal(Kv, K), "prism._tf's kernel2d differs from the scaled _prism.tf columns"
        out["res_vec%d" % d] = res_v
        # scalar intensities (times dircos) and one cell without the property (skipped)
        mixed = [float(scal[0]), mag[1], None, float(scal[3])]
        out["res_mixed%d" % d], _ = _ref_result(R, xp, yp, zp, cells, mixed, inc, dec)
        out["res_pmag%d" % d], _ = _ref_result(R, xp, yp, zp, cells, [None] * len(cells), inc, dec, pmag=2.5)
        out["res_pvec%d" % d], _ = _ref_result(R, xp, yp, zp, cells, mixed, inc, dec, pmag=[0.3, -1.2, 0.8])
        print("prism_tf_cases", (inc, dec), K.shape, "finite:", np.isfinite(K).all())
    out.update(mag=mag, scal=scal)
    # utils.dircos / ang2vec of the reference at the four directions and a few intensities
    out["dircos"] = np.array([R.prism.utils.dircos(i, d) for i, d in DIRS])
    out["ang2vec"] = np.stack([R.prism.utils.ang2vec(np.array([0.0, 1.0, -2.5, 7.0]), i, d) for i, d in DIRS])
    np.savez_compressed(os.path.join(GOLD, "prism_tf_cases.npz"), **out)


def c1_tf_columns(R):
    """64 columns of the tf kernel at C1's geometry (600 obs x 20x30x10 prisms) through prism.tf."""
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    zp = np.zeros_like(xp)
    mesh = _quiet(R.mesher.PrismMesh, (0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    inc, dec = C1_MANGLE
    mesh.addprop("magnetization", R.prism.utils.ang2vec(np.zeros(mesh.size), inc, dec))
    _, K = R.prism.tf(xp, yp, zp, mesh, inc, dec)
    cols = np.sort(np.random.default_rng(5).choice(K.shape[1], 64, replace=False))
    Kc = np.ascontiguousarray(K[:, cols])
    np.savez_compressed(os.path.join(GOLD, "c1_tf_columns.npz"), cols=cols, K=Kc, mangle=np.array(C1_MANGLE))
    print("c1_tf_columns", K.shape, "->", Kc.shape)


def _small_problem(R):
    mrange, mspacing = (0, 2000, 0, 3000, 0, 1000), (250, 500, 400)
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 7), np.linspace(0, 2000, 6))]
    zp = np.zeros_like(xp)
    dobs = np.random.default_rng(0).normal(size=xp.size)
    gm = _quiet(R.potential.GravMagModule, dobs, mrange, mspacing, (xp, yp, zp), field="magnetic",
                mangle=MANGLE)
    return gm, (xp, yp, zp), dobs, mrange, mspacing


def potential_small_tf(R):
    gm, (xp, yp, zp), dobs, mrange, mspacing = _small_problem(R)
    wm = gm.Wm.diagonal()
    M = wm.size
    rng = np.random.default_rng(1)
    xs = np.stack([0.001 * wm, rng.uniform(0, 1, M) * wm, rng.uniform(-1, 1, M) * wm])
    mwapr = 0.001 * wm
    out = dict(xp=xp, yp=yp, zp=zp, dobs=dobs, Aw=np.asfortranarray(gm.Aw), wm=wm, xs=xs, mwapr=mwapr,
               shape=np.array(gm.mshape), mrange=np.array(mrange, float), mspacing=np.array(mspacing, float),
               mangle=np.array(MANGLE), alpha=0.7, beta=0.001)
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        res = [gm.misfit_and_grad(x, mwapr, None, None, 'mandatory', 1000, 0.7, regulization=reg, beta=0.001)
               for x in xs]
        out[reg + "_misfit"] = np.array([r[0] for r in res])
        out[reg + "_grad"] = np.stack([r[1] for r in res])
        out[reg + "_dpre"] = np.stack([r[2] for r in res])
        out[reg + "_data"] = np.array([r[3] for r in res])
        out[reg + "_model"] = np.array([r[4] for r in res])
    np.savez_compressed(os.path.join(GOLD, "potential_small_tf.npz"), **out)
    print("potential_small_tf", gm.Aw.shape)


def chain_small_tf(R):
    """Whole reference HMCSample runs on the small magnetic module: console lines + sample files."""
    gm, _, dobs, _, _ = _small_problem(R)
    M = gm.Wm.shape[0]
    out = {}
    tmp = tempfile.mkdtemp(prefix="gold_tf_")
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
            print("chain_small_tf", tag, len(lines), "lines; last:", lines[-1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(GOLD, "chain_small_tf.npz"), **out)


def main():
    os.makedirs(GOLD, exist_ok=True)
    R = ref_harness.load()
    names = sys.argv[1:] or ["prism_tf_cases", "c1_tf_columns", "potential_small_tf", "chain_small_tf"]
    for name in names:
        globals()[name](R)
    return 0


if __name__ == "__main__":
    sys.exit(main())
