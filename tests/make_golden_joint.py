"""Generate the joint gravity-magnetic fixtures tests/golden/*_joint.npz from the reference itself.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle.ref_harness), so it runs where the
fixtures are made, never on the GPU machine:
    python tests/make_golden_joint.py [name ...]
The files hold DATA only: inputs and the reference's outputs (a JointModule's weighted kernel, weights,
balanced data, potential and finite-difference operator fd3djoint; HMCSample console lines and sample files).  Every array is a deterministic
function of the seeds below: two runs write the same arrays.  (Not collected by pytest: the name does not
start with test_.)
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
MANGLE = (60.0, -10.0)
#: (mrange, mspacing, observation grid (ny_obs, nx_obs), observation height, seed) of the two geometries:
#: "a" a 3 x 4 x 4 mesh under 30 observations; "b" 3 x 5 x 7 cells (odd on every axis) under 42 (not a
#: multiple of 16)
GEOMS = {
    "a": ((0, 2000, 0, 3000, 0, 900), (300, 750, 500), (6, 5), 0.0, 3),
    "b": ((0, 2100, 0, 2500, 0, 900), (300, 500, 300), (7, 6), -25.0, 4),
}
REGS = ("Damping", "MS", "Smoothness", "TV")


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _inputs(geom):
    mrange, mspacing, (nyo, nxo), h, seed = GEOMS[geom]
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(mrange[2], mrange[3], nyo),
                                             np.linspace(mrange[0], mrange[1], nxo))]
    zp = np.full_like(xp, h)
    rng = np.random.default_rng(seed)
    dobs_gz = rng.normal(size=xp.size) * 0.5
    dobs_tf = rng.normal(size=xp.size) * 20.0
    return mrange, mspacing, (xp, yp, zp), dobs_gz, dobs_tf


def _module(R, geom):
    mrange, mspacing, obs, dobs_gz, dobs_tf = _inputs(geom)
    jm = _quiet(R.potential.JointModule, dobs_gz, dobs_tf, mrange, mspacing, obs, mangle=MANGLE)
    # Smoothness and TV call self.fd3d, which the reference's JointModule lacks; its own block-diagonal
    # operator fd3djoint is what they are meant to use, so the fixtures take their values from it.
    jm.fd3d = jm.fd3djoint
    return jm, mrange, mspacing, obs, dobs_gz, dobs_tf


def joint_small(R):
    out = {}
    for geom in GEOMS:
        jm, mrange, mspacing, (xp, yp, zp), dobs_gz, dobs_tf = _module(R, geom)
        wm = jm.Wm.diagonal()
        M2 = wm.size
        rng = np.random.default_rng(11)
        xs = np.stack([0.001 * wm, rng.uniform(0, 1, M2) * wm, rng.uniform(-1, 1, M2) * wm])
        mwapr = 0.001 * wm
        g = geom + "_"
        out.update({g + "xp": xp, g + "yp": yp, g + "zp": zp, g + "dobs_gz": dobs_gz, g + "dobs_tf": dobs_tf,
                    g + "mrange": np.array(mrange, float), g + "mspacing": np.array(mspacing, float),
                    g + "shape": np.array(jm.mshape), g + "Aw": np.asfortranarray(jm.Aw), g + "wm": wm,
                    g + "wb": jm.Wb.diagonal(), g + "dobsw": jm.dobsw,
                    g + "std": np.array([np.std(jm.kernel_gz), np.std(jm.kernel_tf)]),
                    g + "A": np.asfortranarray(jm.A), g + "xs": xs, g + "mwapr": mwapr})
        # the reference's own block-diagonal finite-difference operator of this mesh, as CSR arrays
        fdj = jm.fd3djoint(jm.mshape).tocsr()
        fdj.sort_indices()
        out.update({g + "fd3djoint_data": fdj.data.astype(np.float64), g + "fd3djoint_indices": fdj.indices,
                    g + "fd3djoint_indptr": fdj.indptr, g + "fd3djoint_shape": np.array(fdj.shape)})
        for reg in REGS:
            res = [jm.misfit_and_grad(x, mwapr, None, None, 'mandatory', 1000, 0.7, regulization=reg, beta=0.001)
                   for x in xs]
            out[g + reg + "_misfit"] = np.array([r[0] for r in res])
            out[g + reg + "_grad"] = np.stack([r[1] for r in res])
            out[g + reg + "_dpre"] = np.stack([r[2] for r in res])
            out[g + reg + "_data"] = np.array([r[3] for r in res])
            out[g + reg + "_model"] = np.array([r[4] for r in res])
        print("joint_small", geom, jm.Aw.shape, "s =", jm.Wb.diagonal()[-1])
    out.update(mangle=np.array(MANGLE), alpha=0.7, beta=0.001)
    np.savez_compressed(os.path.join(GOLD, "joint_small.npz"), **out)


def chain_small_joint(R):
    """Whole reference HMCSample runs on the joint module of geometry "a": console lines + sample files."""
    jm = _module(R, "a")[0]
    M2 = jm.Wm.shape[0]
    out = {}
    tmp = tempfile.mkdtemp(prefix="gold_joint_")
    try:
        for tag, reg, dt, lo, hi, n in (("a", "Damping", 0.01, 0.0, 1.0, 12), ("b", "MS", 0.01, 0.0, 1.0, 4)):
            folder = os.path.join(tmp, "hmc_%s_chain" % tag)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                R.hmc.HMCSample(jm, n, 0, dt, [5, 20], np.full(M2, 0.001 + lo), np.full(M2, 0.001),
                                np.c_[np.full(M2, lo), np.full(M2, hi)], "mandatory", 1000, jm.dobs,
                                "Fixed", 0.8, 1.0, reg, 0.001, 100, 0.001, nbest=100, myrank=0,
                                save_folder=folder, plotsamples=False, im=[0, 0])
            lines = [l for l in buf.getvalue().splitlines() if l.startswith("chain ")]
            out[tag + "_lines"] = np.array(lines)
            out[tag + "_misfit"] = np.loadtxt(folder + "0/misfit.dat")
            out[tag + "_model"] = np.loadtxt(folder + "0/model.dat")
            out[tag + "_cfg"] = np.array([dt, 0.001, lo, hi, n])
            out[tag + "_reg"] = np.array(reg)
            print("chain_small_joint", tag, len(lines), "lines; last:", lines[-1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(GOLD, "chain_small_joint.npz"), **out)


def main():
    os.makedirs(GOLD, exist_ok=True)
    R = ref_harness.load()
    names = sys.argv[1:] or ["joint_small", "chain_small_joint"]
    for name in names:
        globals()[name](R)
    return 0


if __name__ == "__main__":
    sys.exit(main())
