"""Generate the vector-magnetic fixtures tests/golden/prism_bxyz_cases.npz and mvi_vecdata_module.npz from the
reference itself.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_bxyz.py [name ...]
The files hold DATA only: inputs and the reference's outputs (_prism.bx / by / bz / tf columns for unit
magnetizations along the axes, prism._bx / _by / _bz results).  Every array is a deterministic function of the
seeds below: two runs write the same arrays.  (Not collected by pytest: the name does not start with test_.)
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
COMPS = ("bx", "by", "bz")
#: (inc, dec) of the tf blocks
MANGLE = (60.0, -10.0)
AXES = np.eye(3)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _scale(R):
    return R.constants.CM * R.constants.T2NT


def _b_columns(R, comp, xp, yp, zp, cells, axis):
    """Columns of _prism.<comp> for the given cells magnetized 1 A/m along `axis`, scaled as prism._<comp> scales res."""
    fn = getattr(R._prism, comp)
    mx, my, mz = (float(v) for v in AXES[axis])
    K = np.zeros((xp.size, len(cells)))
    for c, b in enumerate(cells):
        res = np.zeros(xp.size)
        fn(xp, yp, zp, *[float(v) for v in b], mx, my, mz, res)
        K[:, c] = res
    K *= _scale(R)
    return K


def _tf_columns(R, xp, yp, zp, cells, axis, inc, dec):
    """Columns of _prism.tf's `res` for the given cells magnetized 1 A/m along `axis`, scaled as prism._tf scales res."""
    fx, fy, fz = R.prism.utils.dircos(inc, dec)
    mx, my, mz = (float(v) for v in AXES[axis])
    K = np.zeros((xp.size, len(cells)))
    for c, b in enumerate(cells):
        res, k1 = np.zeros(xp.size), np.zeros(xp.size)
        R._prism.tf(xp, yp, zp, *[float(v) for v in b], mx, my, mz, fx, fy, fz, res, k1)
        K[:, c] = res
    K *= _scale(R)
    return K


def _prisms(R, cells, mags):
    out = []
    for b, m in zip(cells, mags):
        p = R.mesher.Prism(*[float(v) for v in b])
        if m is not None:
            p.addprop("magnetization", m)
        out.append(p)
    return out


def prism_bxyz_cases(R):
    """The singular and random (obs, cell) geometries of prism_tf_cases through _prism.bx / by / bz for unit
    magnetizations along x, y and z, plus prism._bx / _by / _bz results for per-cell vectors, a cell without the
    property and pmag; and the tf blocks of the same geometry at one field direction."""
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
    n_singular = len(pts)
    rng = np.random.default_rng(21)
    n = 120
    rnd = np.c_[rng.uniform(-500, 2500, n), rng.uniform(-500, 3500, n), -rng.uniform(0, 50, n)]
    pts = np.vstack([np.array(pts), rnd])
    xp, yp, zp = [np.ascontiguousarray(pts[:, i]) for i in range(3)]
    mag = rng.normal(size=(len(cells), 3)) * 2.0
    pvec = np.array([0.3, -1.2, 0.8])
    out = dict(xp=xp, yp=yp, zp=zp, cells=cells, mag=mag, pvec=pvec, n_singular=n_singular, mangle=np.array(MANGLE),
               skipped=2)
    skip = [mag[0], mag[1], None, mag[3]]
    for comp in COMPS:
        for a in range(3):
            K = _b_columns(R, comp, xp, yp, zp, cells, a)
            out["K_%s_%d" % (comp, a)] = K
            print("prism_bxyz_cases", comp, "xyz"[a], K.shape, "finite:", np.isfinite(K).all())
        fn = getattr(R.prism, "_" + comp)
        out["res_vec_" + comp] = fn(xp, yp, zp, _prisms(R, cells, list(mag)))
        out["res_skip_" + comp] = fn(xp, yp, zp, _prisms(R, cells, skip))
        out["res_pmag_" + comp] = fn(xp, yp, zp, _prisms(R, cells, skip), pmag=list(pvec))
    for a in range(3):
        out["K_tf_%d" % a] = _tf_columns(R, xp, yp, zp, cells, a, *MANGLE)
    out["dircos"] = np.array(R.prism.utils.dircos(*MANGLE))
    np.savez_compressed(os.path.join(GOLD, "prism_bxyz_cases.npz"), **out)


def mvi_vecdata_module(R):
    """A 4 x 3 x 2 mesh under 65 scattered points: the twelve reference blocks (tf, bx, by, bz) x (x, y, z), a compact
    body magnetized well off the field direction and the reference's tf / bx / by / bz of it."""
    mrange, mspacing = (0, 2000, 0, 3000, 0, 900), (450, 1000, 500)
    mesh = _quiet(R.mesher.PrismMesh, mrange, mspacing)
    cells = np.array([[p.x1, p.x2, p.y1, p.y2, p.z1, p.z2] for p in mesh], dtype=float)
    rng = np.random.default_rng(65)
    n = 65
    xp = np.ascontiguousarray(rng.uniform(50, 1950, n))
    yp = np.ascontiguousarray(rng.uniform(100, 2900, n))
    zp = np.ascontiguousarray(-rng.uniform(20, 60, n))
    inc, dec = MANGLE
    out = dict(xp=xp, yp=yp, zp=zp, cells=cells, shape=np.array(mesh.shape), mrange=np.array(mrange, float),
               mspacing=np.array(mspacing, float), mangle=np.array(MANGLE))
    for comp in COMPS:
        out["K_" + comp] = np.stack([_b_columns(R, comp, xp, yp, zp, cells, a) for a in range(3)])
    out["K_tf"] = np.stack([_tf_columns(R, xp, yp, zp, cells, a, inc, dec) for a in range(3)])
    # the body: the two cells in the middle of the lower layer, 2 A/m at (inc, dec) = (-25, 100), far from (60, -10)
    nz, ny, nx = mesh.shape
    vec = np.zeros((nz, ny, nx, 3))
    vec[1, 1, 1:3] = R.prism.utils.ang2vec(2.0, -25.0, 100.0)
    vec = vec.reshape(-1, 3)
    out["vec"] = vec
    mesh.addprop("magnetization", vec)
    for comp in COMPS:
        out["d_" + comp] = getattr(R.prism, "_" + comp)(xp, yp, zp, mesh)
    res, K = np.zeros(n), np.zeros((n, len(cells)))
    R.prism._tf(xp, yp, zp, res, K, mesh, inc, dec)
    out["d_tf"] = res
    np.savez_compressed(os.path.join(GOLD, "mvi_vecdata_module.npz"), **out)
    print("mvi_vecdata_module", out["K_bx"].shape, mesh.shape)


def main():
    os.makedirs(GOLD, exist_ok=True)
    R = ref_harness.load()
    names = sys.argv[1:] or ["prism_bxyz_cases", "mvi_vecdata_module"]
    for name in names:
        globals()[name](R)
    return 0


if __name__ == "__main__":
    sys.exit(main())
