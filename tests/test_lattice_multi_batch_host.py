"""CPU suite: the door to chain batches on the multi-component translation-invariant table
(translation_invariant="chains" on MultiComponentModule, gh_set_cells_multi_table_chains) and the suite's own reference for
test_gpu_lattice_multi_batch.py -- the NumPy restatement of the row-block batch forms (lattice_multi_batch_cases.py)
against the expanded stacked weighted kernel, the restated plan, and the conditioning of the chains' cases: a wrong model
(one global mean, two weights swapped, a block dropped) is far from the right one, and every trajectory the GPU suite runs
keeps a Metropolis margin |log u + (Hnew - Hcur)| >= 1e-3."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import lattice_batch_cases as lb
import lattice_multi_batch_cases as mb
from multicomp_host import stack


# ----------------------------------------------------------------------------------------------------- the door

def test_header_declares_and_the_library_exports_the_entry_point(built_lib):
    """(fails without the feature) in the manner of test_c_abi_exports_every_declared_symbol"""
    from gravinv3dhmc_amd import _lib
    with open(os.path.join(ROOT, "include", "gravhmc.h")) as f:
        declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", f.read()))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("gh_set_cells_multi_table_chains", "gh_batch_block_means"):
        assert name in declared and name in exported and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["gh_set_cells_multi_table_chains"] == _lib.PROTOTYPES["gh_set_cells_multi_table"]


class _Eng:
    def __init__(self, **attrs):
        for k, v in attrs.items():
            setattr(self, k, v)


def _refused(hmc, eng):
    """the row of _NO_BATCH that stops the engine, as HMCSampleBatch walks them"""
    for row in hmc._NO_BATCH:
        if hmc._table_takes_batches(eng, row):
            continue
        if all(getattr(eng, a, False) for a in row[0]):
            return row[1]
    return None


def test_sampler_admits_the_multi_engine_with_chains_and_no_other_row():
    from gravinv3dhmc_amd import _lib
    from gravinv3dhmc_amd.engine import Store
    from gravinv3dhmc_amd.inversion import hmc
    store = Store(_lib.CELL_PRISM_MULTI, 1, 3, True)
    door = _Eng(multi=3, _store=store, _translation_invariant=True, _translation_invariant_chains=True)
    assert hmc._table_takes_batches(door, hmc._MULTI_ROW) and hmc._table_takes_batches(door, hmc._TABLE_ROW)
    assert _refused(hmc, door) is None
    # multi alone, and multi on the table that was not asked to take batches
    assert "MultiComponentModule" in _refused(hmc, _Eng(multi=3, _store=store))
    assert "MultiComponentModule" in _refused(hmc, _Eng(multi=3, _store=store, _translation_invariant=True,
                                                        _translation_invariant_chains=False))
    # the flag opens no other row
    for attrs, word in ((dict(multi=3, mvi=True), "MagVectorModule with data="), (dict(tess_multi=True, multi=3), "Tesseroid"),
                        (dict(joint=True), "JointModule"), (dict(tess_mag=True, multi=3, mvi=True), "TesseroidMagVector"),
                        (dict(mvi=True), "MagVectorModule")):
        eng = _Eng(_translation_invariant=True, _translation_invariant_chains=True,
                   _store=Store(_lib.CELL_PRISM_MVI_DATA, 3, 3, True), **attrs)
        assert word in _refused(hmc, eng), attrs
    assert sum(row is hmc._MULTI_ROW for row in hmc._NO_BATCH) == 1


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


def test_engine_hands_chains_to_the_new_entry_point_and_rejects_other_strings():
    from gravinv3dhmc_amd.engine import Engine, Store
    b6 = np.zeros((4, 6))
    for ti, fn, chains in ((False, "gh_set_cells_multi", False), (True, "gh_set_cells_multi_table", False),
                           ("chains", "gh_set_cells_multi_table_chains", True)):
        eng = object.__new__(Engine)
        eng._lib, eng._h, eng.M, eng._store = _Lib(), None, 4, Store(None, 1, 1, False)
        eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 2.0], translation_invariant=ti)
        assert eng._lib.calls == [fn]
        assert bool(getattr(eng, "_translation_invariant", False)) == bool(ti)
        assert bool(getattr(eng, "_translation_invariant_chains", False)) == chains
        assert eng.multi == 2
    for bad in ("replicates", "chain", "Chains", "", "True"):
        eng = object.__new__(Engine)
        eng._lib, eng._h, eng.M = _Lib(), None, 4
        with pytest.raises(ValueError, match="chains"):
            eng.set_cells_multi(b6, ["gz", "gzz"], [1.0, 2.0], translation_invariant=bad)
        assert eng._lib.calls == []


class _Reached(Exception):
    pass


def test_module_hands_chains_to_the_engine_and_keeps_the_tables_refusals(monkeypatch):
    from gravinv3dhmc_amd.inversion import multicomp as m
    asked = []

    class Recorder:
        def __init__(self, N, M, device=0):
            pass

        def set_cells_multi(self, bounds, components, weights, translation_invariant=False):
            asked.append(translation_invariant)
            raise _Reached()

    monkeypatch.setattr(m, "Engine", Recorder)
    xp, yp = [a.ravel() for a in np.meshgrid(50.0 + 100.0 * np.arange(5), 50.0 + 100.0 * np.arange(7), indexing="ij")]
    obs = (xp, yp, np.full(xp.size, -20.0))
    dobs = [np.arange(xp.size, dtype=float) + k * k for k in range(2)]
    args = (dobs, (0.0, 700.0, 0.0, 500.0, 0.0, 300.0), (100.0, 100.0, 100.0), obs)
    for ti in ("chains", True):
        with pytest.raises(_Reached):
            m.MultiComponentModule(*args, components=("gz", "gzz"), verbose=False, translation_invariant=ti)
        assert asked[-1] == ti
    n = len(asked)
    for kw in (dict(wavelet="1D"), dict(matrix_free=True), dict(shift_invariant=True), dict(shard=object()),
               dict(coordinate="spherical")):
        with pytest.raises(NotImplementedError, match="multi-component store") as e:
            m.MultiComponentModule(*args, components=("gz", "gzz"), verbose=False, translation_invariant="chains", **kw)
        assert "translation-invariant" in str(e.value)
    with pytest.raises(ValueError, match="chains"):
        m.MultiComponentModule(*args, components=("gz", "gzz"), verbose=False, translation_invariant="replicates")
    assert len(asked) == n


# ----------------------------------------------------------------------- the restatement against the stacked kernel

@pytest.mark.parametrize("name", sorted(mb.BLOCK_CASES))
def test_restated_block_passes_against_the_stacked_kernel(name):
    """tables of random entries (the restatement knows no physics): forward16 / adjoint16 over the blocks and the finish
    against Aw @ X, Aw.T @ R and the per-block means of the expanded stacked weighted kernel"""
    nb = mb.BLOCK_CASES[name]
    obs, b6 = mb.geometry(**mb.PASS_CASES[name])
    dims, col, ool = lb.lattice(obs, b6)
    nx, ny, nz, px, qy = dims
    rng = np.random.default_rng(3)
    tables = [rng.normal(size=(nz, nx + px - 1, ny + qy - 1)) for _ in range(nb)]
    w = np.array(mb.ALL_WEIGHTS[:nb])
    Aw, wm, _ = stack([mb.expand(T, dims, col, ool) for T in tables], w)
    N, M = Aw.shape
    assert N == nb * px * qy
    ld = (N + 15) // 16 * 16
    X, R = rng.normal(size=(M, mb.CB)), rng.normal(size=(N, mb.CB))
    X[:, 5] = 0.0  # (an empty slot among live ones)
    iw = 1.0 / wm
    D = mb.forward16_blocks(tables, w, X, iw, dims, col, ool)
    S = mb.adjoint16_blocks(tables, w, mb.to_rt(R, ld), dims, col, ool) * iw[:, None]
    Dref, Sref = Aw @ X, Aw.T @ R
    assert np.abs(D - Dref).max() <= 1e-12 * np.abs(Dref).max()
    assert np.abs(S - Sref).max() <= 1e-12 * np.abs(Sref).max()
    assert not D[:, 5].any()
    # a chain's column does not depend on what the other slots hold
    X1 = np.zeros_like(X)
    X1[:, 0] = X[:, 0]
    assert np.array_equal(mb.forward16_blocks(tables, w, X1, iw, dims, col, ool)[:, 0], D[:, 0])
    # the finish: one mean per block and chain; a patch of Rt may hold rows of two blocks
    dobs = rng.normal(size=N)
    dobs_c = dobs - np.repeat(dobs.reshape(nb, -1).mean(axis=1), N // nb)
    Rt, ud, means = mb.finish_blocks(D, dobs_c, nb, ld)
    from multicomp_host import MultiProblem
    P = MultiProblem(Aw, dobs, nb, np.zeros(M), alpha=0.0)  # (the data term alone)
    for c in (0, 7, 15):
        out = P.misfit_and_grad(X[:, c])
        assert abs(ud[c] - out[3]) <= 1e-12 * max(out[3], 1e-300)
        assert np.abs(means[c] - P.pred_mean).max() <= 1e-12 * np.abs(Dref).max()
        g = 2.0 * (mb.adjoint16_blocks(tables, w, Rt, dims, col, ool) * iw[:, None])[:, c]
        assert np.abs(g - out[1]).max() <= 1e-11 * np.abs(out[1]).max()
    if name == "y7":
        assert (N // nb) % 16 != 0 and ld == 96 and not Rt.reshape(-1)[mb.rt_offset(np.arange(N, ld)[:, None], np.arange(16))].any()


def test_restated_plan_with_the_block_on_grid_z():
    def dims(name):
        kw = mb.PASS_CASES[name]
        return tuple(kw["cells"]) + tuple(kw["obs"])

    cus = 256
    for nb in (1, 2, 11):
        for name in ("y17", "y65", "rows beyond one tile"):
            p, one = mb.plan(dims(name), cus, nb), lb.plan(dims(name), cus)
            # the passes are the single block's: the blocks take turns in the tile
            assert all(p[k] == v for k, v in one.items() if k not in ("lpc", "chunks")) and p["blocks"] == nb
        # nz = 33 over one workgroup per chunk and block: 32 chunks at most
        p = mb.plan(dims("layers per chunk"), cus, nb)
        assert (p["lpc"], p["chunks"]) == (2, 17) and p["chunks"] < 33
    # the README's shapes: 6 and 2 blocks; 4 cus / (nb grid) workgroups wanted per chunk
    p = mb.plan((100, 100, 50, 100, 100), cus, 6)
    assert p["fits"] and p["fwd_grid"] == 13 * 2 and (p["lpc"], p["chunks"]) == (8, 7)     # (7 = ceil(1024 / (6 x 26)))
    p1 = mb.plan((100, 100, 50, 100, 100), cus, 1)
    assert (p1["lpc"], p1["chunks"]) == (2, 25) == (lb.plan((100, 100, 50, 100, 100), cus)["lpc"], 25)
    p = mb.plan((200, 200, 60, 200, 200), cus, 2)
    assert p["fits"] and p["fwd_grid"] == 25 * 4 and (p["lpc"], p["chunks"]) == (10, 6)
    # few compute units and many blocks: one chunk
    p = mb.plan(dims("layers per chunk"), 2, 11)
    assert (p["lpc"], p["chunks"]) == (33, 1)


# ------------------------------------------------------------------------------------- the chains' conditioning

def test_host_kernels_against_the_oracle_and_a_difference_of_gz():
    """the suite's closed-form gz is the oracle's; gzz against the central difference of gz along z (30 m above the cells,
    where the field is smooth: 1e-8 of the largest entry)"""
    from oracle import oracle
    obs, b6 = mb.geometry(zobs=-30.0, **mb.PASS_CASES["beyond"])
    gz = mb.prism_kernel("gz", obs, b6)
    ref = oracle.prism_gz_kernel(obs[0], obs[1], obs[2], b6)
    assert np.abs(gz - ref).max() <= 1e-12 * np.abs(ref).max()
    h = 1e-2
    up, dn = obs.copy(), obs.copy()
    up[2] += h
    dn[2] -= h
    # (mGal per m -> Eotvos: 1e4)
    gzz_fd = (mb.prism_kernel("gz", up, b6) - mb.prism_kernel("gz", dn, b6)) / (2 * h) * 1e4
    gzz = mb.prism_kernel("gzz", obs, b6)
    assert np.abs(gzz - gzz_fd).max() <= 1e-8 * np.abs(gzz).max()
    # gxy: symmetric in the mirror (dx, dy) -> (dy, dx) of the same formula, odd in either offset alone
    gxy = mb.prism_kernel("gxy", obs, b6)
    flip = b6.copy()
    flip[:, 2], flip[:, 3] = 2 * obs[1, 0] - b6[:, 3], 2 * obs[1, 0] - b6[:, 2]      # (mirror the cells in y about point 0)
    assert np.abs(mb.prism_kernel("gxy", obs[:, :1], flip) + gxy[:1]).max() <= 1e-12 * np.abs(gxy).max()


_CHAIN = {}


def chain_case(name, reg):
    key = (name, reg)
    if key not in _CHAIN:
        obs, b6 = mb.geometry(**mb.PASS_CASES[name])
        K = [mb.prism_kernel(c, obs, b6) for c in mb.CHAIN_COMPONENTS]
        Aw, wm, prob = mb.chain_setup(name, reg, K, mb.CHAIN_WEIGHTS)
        P = mb.problem(Aw, prob, 3, reg, wm)
        _CHAIN[key] = (K, Aw, wm, prob, mb.chains(P, prob, mb.CB))
    return _CHAIN[key]


@pytest.mark.parametrize("reg", mb.REGS)
@pytest.mark.parametrize("name", mb.CHAIN_CASES)
def test_chain_cases_accept_reject_and_keep_a_margin(name, reg):
    K, Aw, wm, prob, (rounds, margin) = chain_case(name, reg)
    acc = np.array([r[0] for r in rounds])
    clamped = sum(int(np.any(r[2] == prob["low"]) or np.any(r[2] == prob["high"])) for r in rounds)
    print(name, reg, "dt", prob["dt"], "margin", margin, "accepted", int(acc.sum()), "of", acc.size, "clamped rounds", clamped)
    assert acc.size == mb.CB * 4 and 0 < acc.sum() < acc.size
    assert margin >= 1e-3


def _gap(rounds, wrong):
    """the largest relative difference of out5 and x between two sets of trajectories"""
    g = 0.0
    for (a1, o1, x1), (a2, o2, x2) in zip(rounds, wrong):
        g = max(g, np.abs(o1 - o2).max() / np.abs(o1).max(), np.abs(x1 - x2).max() / np.abs(x1).max())
    return g


@pytest.mark.parametrize("reg", mb.REGS)
@pytest.mark.parametrize("name", mb.CHAIN_CASES)
def test_a_wrong_model_is_far_from_the_right_one(name, reg):
    """what 1e-10 on the GPU tells apart: one global mean, two weights swapped, a block dropped"""
    K, Aw, wm, prob, (rounds, _) = chain_case(name, reg)
    n = K[0].shape[0]
    wrong = {"global mean": mb.problem(Aw, prob, 3, reg, wm, global_mean=True)}
    w = list(mb.CHAIN_WEIGHTS)
    w[0], w[1] = w[1], w[0]
    Aw_s = np.vstack([K[b] * w[b] for b in range(3)]) / wm[None, :]
    wrong["weights swapped"] = mb.problem(Aw_s, prob, 3, reg, wm)
    Aw_d = Aw.copy()
    Aw_d[2 * n:] = 0.0
    wrong["block dropped"] = mb.problem(Aw_d, prob, 3, reg, wm)
    for what, P in wrong.items():
        gap = _gap(rounds, mb.chains(P, prob, mb.CB)[0])
        print(name, reg, what, "gap", gap)
        assert gap >= 1e-6, what
