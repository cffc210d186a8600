"""Generate the magnetization-vector fixtures tests/golden/mvi_*.npz from the reference itself.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_mvi.py [name ...]
The files hold DATA only: inputs and the reference's outputs (prism.tf / prism._tf results and kernel2d).  Every
array is a deterministic function of the seeds below.  (Not collected by pytest: the name does not start with test_.)

What the reference delivers for a magnetization along an axis.  _prism.tf accumulates TWO sums per observation
(_prism.pyx:101-111): `res` with the magnetization it is given, and kernel1D, which always uses m = f -- the
field direction -- whatever (mx, my, mz) is.  So prism.tf(..., pmag=e_a)'s kernel2d is the INDUCED kernel for every
axis a (recorded below as kernel2d<d>_<a>, and asserted equal to prism_tf_cases' K<d>): it does not hold the columns
of A_a.  The column of A_a for prism c is prism.tf's `result` on that one prism with pmag = e_a -- the same corner
loop, the reference's operation order (bx = v1*1 + v2*0 + v3*0, ..., then fx*bx + fy*by + fz*bz), one sum per
observation scaled once by CM*T2NT.  Those are the blocks A<d>_<a> the device is compared with.
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
#: (inc, dec): f = e_z, f = e_x, and two oblique directions (prism_tf_cases' own four)
DIRS = np.array([(90.0, 0.0), (0.0, 0.0), (60.0, -10.0), (-45.0, 120.0)])
MANGLE = (60.0, -10.0)
C1_MANGLE = (50.0, 30.0)
AXES = np.eye(3)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _tf(R, xp, yp, zp, cells, inc, dec, pmag=None, mags=None):
    """prism._tf on a list of reference prisms: (result, kernel2d)"""
    prisms = []
    for i, b in enumerate(cells):
        p = R.mesher.Prism(*[float(v) for v in b])
        if mags is not None:
            p.addprop("magnetization", list(mags[i]))
        prisms.append(p)
    res, K = np.zeros(xp.size), np.zeros((xp.size, len(cells)))
    R.prism._tf(xp, yp, zp, res, K, prisms, inc, dec, pmag)
    return res, K


def _blocks(R, xp, yp, zp, cells, inc, dec):
    """[A_x, A_y, A_z]: column c of A_a = prism._tf's result on prism c alone with pmag = e_a"""
    out = []
    for a in range(3):
        A = np.zeros((xp.size, len(cells)))
        for c, b in enumerate(cells):
            A[:, c], _ = _tf(R, xp, yp, zp, [b], inc, dec, pmag=[float(v) for v in AXES[a]])
        out.append(A)
    return out


def mvi_cases(R):
    """prism_tf_cases' geometries (observations on faces, edges and corners, in line with edges, far away, random)
    at its four field directions: the three blocks, the reference's kernel2d with pmag = e_a, and prism.tf results
    for per-cell vectors whose direction differs from the field."""
    tfc = np.load(os.path.join(GOLD, "prism_tf_cases.npz"))
    xp, yp, zp, cells = tfc["xp"], tfc["yp"], tfc["zp"], tfc["cells"]
    out = dict(xp=xp, yp=yp, zp=zp, cells=cells, dirs=DIRS)
    rng = np.random.default_rng(33)
    mag = rng.normal(size=(len(cells), 3)) * 2.0
    mag2 = np.array([[0.0, 1.5, 0.0], [-2.0, 0.0, 0.5], [0.0, 0.0, -3.0], [1.0, 1.0, 1.0]])
    out.update(mag=mag, mag2=mag2)
    for d, (inc, dec) in enumerate(DIRS):
        assert np.array_equal(DIRS[d], tfc["dirs"][d])
        A = _blocks(R, xp, yp, zp, cells, inc, dec)
        for a in range(3):
            out["A%d_%d" % (d, a)] = A[a]
            _, K2 = _tf(R, xp, yp, zp, cells, inc, dec, pmag=[float(v) for v in AXES[a]])
            # (the reference's kernel2d ignores pmag: it is the induced kernel, whatever the axis)
            assert np.array_equal(K2, tfc["K%d" % d]), "kernel2d with pmag = e_%d differs from the induced kernel" % a
            out["kernel2d%d_%d" % (d, a)] = K2
        out["res_vec%d" % d], _ = _tf(R, xp, yp, zp, cells, inc, dec, mags=mag)
        out["res_vec2_%d" % d], _ = _tf(R, xp, yp, zp, cells, inc, dec, mags=mag2)
        print("mvi_cases", (inc, dec), [np.isfinite(a).all() for a in A])
    np.savez_compressed(os.path.join(GOLD, "mvi_cases.npz"), **out)


def _c1(R):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    zp = np.zeros_like(xp)
    mesh = _quiet(R.mesher.PrismMesh, (0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    return xp, yp, zp, mesh


def mvi_small(R):
    """A 64-column sample of the store [A_x | A_y | A_z] at C1's geometry (600 obs x 20x30x10 prisms: 18000 columns,
    column a * 6000 + c is prism c magnetized along axis a), and a small module-sized problem: the blocks of a
    2 x 6 x 4 mesh under 42 points with prism.tf's result for per-cell vectors."""
    xp, yp, zp, mesh = _c1(R)
    inc, dec = C1_MANGLE
    cols = np.sort(np.random.default_rng(5).choice(3 * mesh.size, 64, replace=False))
    K = np.zeros((xp.size, cols.size))
    for k, col in enumerate(cols):
        a, c = divmod(int(col), mesh.size)
        p = mesh[c]
        K[:, k], _ = _tf(R, xp, yp, zp, [[p.x1, p.x2, p.y1, p.y2, p.z1, p.z2]], inc, dec,
                         pmag=[float(v) for v in AXES[a]])
    out = dict(c1_cols=cols, c1_mangle=np.array(C1_MANGLE), c1_K=K)
    print("mvi_small: C1 columns", K.shape, "axes", np.bincount(cols // mesh.size, minlength=3))
    # the small problem
    mrange, mspacing = (0, 2000, 0, 3000, 0, 1000), (500, 500, 500)
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 7), np.linspace(0, 2000, 6))]
    zp = np.full(xp.size, -20.0)
    mesh = _quiet(R.mesher.PrismMesh, mrange, mspacing)
    cells = np.array([[p.x1, p.x2, p.y1, p.y2, p.z1, p.z2] for p in mesh], dtype=float)
    inc, dec = MANGLE
    A = _blocks(R, xp, yp, zp, cells, inc, dec)
    rng = np.random.default_rng(2)
    vec = rng.normal(size=(mesh.size, 3))
    mesh.addprop("magnetization", vec)
    res, _ = R.prism.tf(xp, yp, zp, mesh, inc, dec)
    out.update(xp=xp, yp=yp, zp=zp, mrange=np.array(mrange, float), mspacing=np.array(mspacing, float),
               shape=np.array(mesh.shape), mangle=np.array(MANGLE), cells=cells, A=np.stack(A), vec=vec, res_vec=res)
    print("mvi_small: module problem", np.stack(A).shape)
    np.savez_compressed(os.path.join(GOLD, "mvi_small.npz"), **out)


def main():
    os.makedirs(GOLD, exist_ok=True)
    R = ref_harness.load()
    for name in sys.argv[1:] or ["mvi_cases", "mvi_small"]:
        globals()[name](R)
    return 0


if __name__ == "__main__":
    sys.exit(main())
