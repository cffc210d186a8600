"""GPU suite (`-m gpu`): the joint gravity-magnetic store on the translation-invariant table (gh_set_cells_joint_table,
csrc/latjoint.hip.h; lat_pass_kernel's block-diagonal form, csrc/lattice.hip.h) -- the property of a column as one more
layer coordinate, T[b nz + k][u][v], and every layer on its own observation block.

  1. the table's blocks are the scalar gz and tf tables, bit for bit, on every shape;
  2. std_gz, std_tf and Wm against the dense store (the large shape: against NumPy on the host kernels);
  3. forward, gradient, |r|^2 of both blocks and R under the four regularisers, the cross-gradient term off and on,
     against the dense store and crossgrad_host's joint problem; on the large shape (20 480 points per block, forward
     chunks of two layers that a chunking blind to the properties would sum across their boundary) against the host
     alone, where the dense store must still refuse;
  4. chains of ten trajectories against the host problem, a second run and the trajectory feeder bit for bit;
  5. JointModule(translation_invariant=True) against the dense module: weights, potential, forward, the coupling,
     HMCSample with the same seed, with posterior_stream=True too;
  6. refusals, and the default module untouched;
Bounds: the table bit for bit; everything else 1e-10 of the largest magnitude (tests/test_gpu_lattice_mvi.py's)."""
import numpy as np
import pytest

import lattice_joint_cases as C
from helpers import relmax
from lattice_cases import c2_linspace

pytestmark = pytest.mark.gpu

TSTORE, JSTORE = "the joint store on the translation-invariant table", "the joint gravity-magnetic kernel"
FOLD_MAX_DEV = 1e-7
TOL = 1e-10


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


_HOST = {}


def host_store(name):
    """obs, bounds6 and the host's store of a shape (lattice_joint_cases.Blocks on NumPy's kernels): computed once per
    shape, shared, left unchanged"""
    if name not in _HOST:
        obs, b6 = C.shape(name)
        K = C.host_kernels(obs, b6)
        for a in (obs, b6) + K:
            a.setflags(write=False)
        _HOST[name] = (obs, b6, C.Blocks(*K))
    return _HOST[name]


def plan_of(info):
    """the forward's chunks of a built joint table, as lists of layers, from what the engine reports"""
    nz, lpc, half = info["nz"], info["layers_per_chunk"], info["chunks"] // 2
    assert info["chunks"] == 2 * half and half == (nz + lpc - 1) // lpc
    return [list(range(b * nz + c * lpc, min((b + 1) * nz, b * nz + (c + 1) * lpc))) for b in range(2) for c in range(half)]


# ------------------------------------------------------------------------------------------ 1. the table

@pytest.mark.parametrize("name", sorted(C.SHAPES))
def test_table_blocks_are_the_scalar_tables(G, name):
    obs, b6, _ = host_store(name)
    nx, ny, nz = C.SHAPES[name]["cells"]
    px, qy = C.SHAPES[name]["obs"]
    lat = C.joint_engine(G, obs, b6, True)
    info = lat.translation_invariant_info()
    T = lat.translation_invariant_table()
    assert info["on"] and (info["nx"], info["ny"], info["nz"], info["px"], info["qy"]) == (nx, ny, nz, px, qy)
    assert info["axes"] == 2
    assert T.shape == (2, nz, nx + px - 1, ny + qy - 1) and info["table_bytes"] == T.size * 8
    chunks = plan_of(info)
    assert sorted(L for c in chunks for L in c) == list(range(2 * nz))
    assert all(len({L // nz for L in c}) == 1 for c in chunks)
    for b, field in enumerate(("gz", "tf")):
        one = C.scalar_engine(G, obs, b6, field)
        assert np.array_equal(T[b], one.translation_invariant_table()), field
        assert "axes" not in one.translation_invariant_info()
        one.close()
    print(name, "max_dev", info["max_dev"], "chunks", info["chunks"], "of", info["layers_per_chunk"])
    assert info["max_dev"] <= FOLD_MAX_DEV
    with pytest.raises(ValueError):
        lat.download_G()
    lat.close()


# ------------------------------------------------------------------------------------------ 2. the weights

@pytest.mark.parametrize("name", sorted(C.SHAPES))
def test_std_and_weights(G, name):
    obs, b6, op = host_store(name)
    lat = C.joint_engine(G, obs, b6, True)
    wm, std = lat.weight(0.5), lat.joint_std()
    print(name, "against the host: wm", relmax(wm, op.wm), "std", [abs(a - b) / b for a, b in zip(std, op.std)])
    assert relmax(wm, op.wm) <= TOL and all(abs(a - b) <= TOL * b for a, b in zip(std, op.std))
    if name != C.BIG:
        dense = C.joint_engine(G, obs, b6, False)
        wd, sd = dense.weight(0.5), dense.joint_std()
        print(name, "against the dense store: wm", relmax(wm, wd), "std", [abs(a - b) / b for a, b in zip(std, sd)])
        assert relmax(wm, wd) <= TOL and all(abs(a - b) <= TOL * b for a, b in zip(std, sd))
        dense.close()
    lat.close()


# ------------------------------------------------------------------------------------------ 3. the potential

def _set(eng, name, reg, lam, dobsw, wm):
    eng.set_data(dobsw)
    eng.set_reg(reg, 1.0, 0.01, C.mesh_shape(name), 0.01 * wm)
    if lam > 0:
        hx, hy, hz = C.spacing(name)
        eng.set_cross_gradient(lam, C.mesh_shape(name), hx, hy, hz, C.CG_SCALE)


def _same_evaluation(out, ref, n, what):
    """(U, grad, dpre, |r|^2, R) of an engine against those of a reference: the gradient, |r|^2 of each block (from the
    predictions), the data and the model term"""
    (U, g, d, data, model), (Ur, gr, dr, datar, modelr) = out, ref
    e = dict(U=abs(U - Ur) / abs(Ur), grad=relmax(g, gr), gz=relmax(d[:n], dr[:n]), tf=relmax(d[n:], dr[n:]),
             data=abs(data - datar) / abs(datar), R=abs(model - modelr) / max(abs(modelr), 1e-300))
    print(what, e)
    assert max(e.values()) <= TOL, (what, e)


@pytest.mark.parametrize("lam", [0.0, C.LAMBDA], ids=["plain", "cross-gradient"])
@pytest.mark.parametrize("name", C.SMALL)
def test_potential_against_the_dense_store_and_the_host(G, name, lam):
    if lam > 0 and name not in C.COUPLED:
        # (one layer: no cell has a forward neighbour along z, and the library says so)
        obs, b6, _ = host_store(name)
        lat = C.joint_engine(G, obs, b6, True)
        lat.weight(0.5)
        with pytest.raises(ValueError, match="at least 2"):
            hx, hy, hz = C.spacing(name)
            lat.set_cross_gradient(lam, C.mesh_shape(name), hx, hy, hz, C.CG_SCALE)
        lat.close()
        return
    obs, b6, op = host_store(name)
    n = op.n
    _, _, dobsw, xt = C.case_data(op)
    lat, dense = C.joint_engine(G, obs, b6, True), C.joint_engine(G, obs, b6, False)
    for e in (lat, dense):
        e.weight(0.5)
    fw, fd, fh = lat.forward(xt), dense.forward(xt), op @ xt
    for b in range(2):
        assert relmax(fw[b * n:(b + 1) * n], fd[b * n:(b + 1) * n]) <= TOL and relmax(fw[b * n:(b + 1) * n], fh[b * n:(b + 1) * n]) <= TOL
    for reg in C.REGS:
        for e in (lat, dense):
            _set(e, name, reg, lam, dobsw, op.wm)
        P = C.problem(op, name, dobsw, reg, lam)
        out = lat.misfit_and_grad(xt)
        U, g, d, data, model = P.misfit_and_grad(xt)
        r = d - dobsw
        _same_evaluation(out, (U, g, d, data, model), n, "%s %s %g host" % (name, reg, lam))
        _same_evaluation(out, dense.misfit_and_grad(xt), n, "%s %s %g dense" % (name, reg, lam))
        rl = out[2] - dobsw
        for b in range(2):
            r2, r2h = rl[b * n:(b + 1) * n] @ rl[b * n:(b + 1) * n], r[b * n:(b + 1) * n] @ r[b * n:(b + 1) * n]
            assert abs(r2 - r2h) <= TOL * max(r @ r, r2h)
        if lam > 0:
            assert abs(lat.cross_gradient_last() - P.last_phi) <= TOL * abs(P.last_phi) and P.last_phi > 0
            assert abs(lat.cross_gradient_last() - dense.cross_gradient_last()) <= TOL * abs(P.last_phi)
    for e in (lat, dense):
        e.close()


def test_the_large_shape_builds_where_the_dense_store_refuses(G):
    """20 480 points per block.  Fails on a library without the joint store's door to the table."""
    obs, b6, op = host_store(C.BIG)
    n, nz = op.n, C.SHAPES[C.BIG]["cells"][2]
    assert n == 20480 > 16384
    with pytest.raises(NotImplementedError, match="16384"):
        C.joint_engine(G, obs, b6, False)
    lat = C.joint_engine(G, obs, b6, True)
    info = lat.translation_invariant_info()
    chunks = plan_of(info)
    print("layers per chunk", info["layers_per_chunk"], "chunks", info["chunks"])
    # more than one layer per chunk, the same number of chunks for each property, none across the boundary
    assert info["layers_per_chunk"] > 1 and info["chunks"] % 2 == 0
    assert all(len({L // nz for L in c}) == 1 for c in chunks) and max(len(c) for c in chunks) == info["layers_per_chunk"]
    assert nz % info["layers_per_chunk"] != 0          # (a chunking of the 2 nz layers as they lie would cross)
    wm = lat.weight(0.5)
    assert relmax(wm, op.wm) <= TOL
    _, _, dobsw, xt = C.case_data(op)
    fw, fh = lat.forward(xt), op @ xt
    assert relmax(fw[:n], fh[:n]) <= TOL and relmax(fw[n:], fh[n:]) <= TOL
    for lam in (0.0, C.LAMBDA):
        for reg in C.REGS:
            _set(lat, C.BIG, reg, lam, dobsw, op.wm)
            P = C.problem(op, C.BIG, dobsw, reg, lam)
            _same_evaluation(lat.misfit_and_grad(xt), P.misfit_and_grad(xt), n, "%s %s %g host" % (C.BIG, reg, lam))
    # a short chain runs on it
    low, high = -1.5 * op.wm, 1.5 * op.wm
    lat.chain_init(0.01 * op.wm, low, high)
    rng = np.random.default_rng(5)
    x, P = 0.01 * op.wm, C.problem(op, C.BIG, dobsw, "TV", C.LAMBDA)
    for L in (2, 3):
        p0, u = rng.normal(size=2 * op.m) * 0.6 * op.wm, float(rng.uniform())
        acc, o = lat.chain_trajectory(p0, 0.02, L, u)
        x, acch, oh, _, _ = P.leapfrog(x, p0, 0.02, L, low, high, u)
        assert bool(acc) == bool(acch) and relmax(o, oh) <= TOL and relmax(lat.chain_get_x(), x) <= TOL
    lat.close()


def test_more_than_64_chunks_per_property_take_the_two_stage_epilogue(G):
    """65 layers under 6 stations: 65 forward chunks per property, each half of the live slab rows folded into slab2
    segments first (joint_two_stage: fewer than 2048 rows, more than 64 slab rows per block)"""
    from lattice_cases import geometry
    obs, b6 = geometry(cells=(2, 3, 65), obs=(2, 3), tops=np.arange(66) * 20.0, zobs=-15.0)
    op = C.Blocks(*C.host_kernels(obs, b6))
    n = op.n
    lat, dense = C.joint_engine(G, obs, b6, True), C.joint_engine(G, obs, b6, False)
    info = lat.translation_invariant_info()
    assert info["nz"] == 65 and info["chunks"] // 2 > 64 and n < 2048
    assert lat.joint_layout()["epilogue_stages"] == 2
    for e in (lat, dense):
        assert relmax(e.weight(0.5), op.wm) <= TOL
    _, _, dobsw, xt = C.case_data(op)
    for reg in ("Damping", "TV"):
        for e in (lat, dense):
            e.set_data(dobsw)
            e.set_reg(reg, 1.0, 0.01, (65, 2, 3), 0.01 * op.wm)
        P = C._Problem(op, dobsw, op.wm, (65, 2, 3), reg, 1.0, 0.01, 0.01 * op.wm, 0.0, (1.0, 1.0, np.ones(64)))
        out = lat.misfit_and_grad(xt)
        _same_evaluation(out, P.misfit_and_grad(xt), n, "65 layers %s host" % reg)
        _same_evaluation(out, dense.misfit_and_grad(xt), n, "65 layers %s dense" % reg)
    for e in (lat, dense):
        e.close()


# ------------------------------------------------------------------------------------------ 4. the chains

def _chain(eng, x0, low, high, trajs, dt):
    eng.chain_init(x0, low, high)
    out = []
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        out.append((bool(acc), o.copy(), eng.chain_get_x(), eng.cross_gradient_last()))
    return out


@pytest.mark.parametrize("lam", [0.0, C.LAMBDA], ids=["plain", "cross-gradient"])
@pytest.mark.parametrize("reg", C.REGS)
@pytest.mark.parametrize("name", C.CHAIN_SHAPES)
def test_chains_against_the_host_and_bitwise_paths(G, monkeypatch, name, reg, lam):
    from gravinv3dhmc_amd.inversion.rng import LegacyDraws
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    obs, b6, op = host_store(name)
    _, dobsw, P, low, high, x0, trajs, xt, dt = C.chain_case(op.K, name, reg, lam)

    def engine():
        eng = C.joint_engine(G, obs, b6, True)
        eng.weight(0.5)
        _set(eng, name, reg, lam, dobsw, op.wm)
        return eng

    eng = engine()
    plain = _chain(eng, x0, low, high, trajs, dt)
    ref, accepted, clamps, margin = C.run_chain(P, x0, trajs, dt, low, high)
    for (a, o, x, phi), (ah, oh, xh, phih) in zip(plain, ref):
        assert a == bool(ah)
        assert relmax(o, oh) <= TOL and relmax(x, xh) <= TOL
    # (Phi of the states the chain passed through, against the largest of them: at the flat start it is rounding alone)
    assert relmax([t[3] for t in plain], [t[3] for t in ref]) <= TOL
    print(name, reg, lam, "accepted", accepted, "of", len(plain), "on a bound", clamps, "margin", margin)
    assert 0 < accepted < len(plain) and clamps > 0
    # a second run of the same engine, and a second engine: the same bits
    eng2 = engine()
    for again in (_chain(eng, x0, low, high, trajs, dt), _chain(eng2, x0, low, high, trajs, dt)):
        for (a1, o1, x1, p1), (a2, o2, x2, p2) in zip(plain, again):
            assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, x2) and p1 == p2
    eng2.close()
    eng.close()
    # the trajectory feeder and the Python loop: the same bits
    runs = []
    for feed in (None, "0"):
        if feed is None:
            monkeypatch.delenv("GRAVHMC_CHAIN_FEED", raising=False)
        else:
            monkeypatch.setenv("GRAVHMC_CHAIN_FEED", feed)
        e = engine()
        e.chain_init(x0, low, high)
        res = []
        draws = LegacyDraws(2 * op.m, (2, 6), float(0.6 * op.wm.mean()), limit=10, seed=11)
        try:
            e.run_chain(draws, dt, lambda L, a, o, x: res.append((int(L), bool(a), np.array(o), None if x is None else
                                                                    np.array(x))), overlap=True, want_x=True)
        finally:
            draws.release()
        runs.append((res, e.chain_get_x(), e.feed_stats()["run"]))
        e.close()
    (fed, xf, nf), (loop, xl, nl) = runs
    assert nf > 0 and nl == 0
    assert len(fed) == len(loop) == 10 and np.array_equal(xf, xl)
    for (L1, a1, o1, x1), (L2, a2, o2, x2) in zip(fed, loop):
        assert L1 == L2 and a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2))


# ------------------------------------------------------------------------------------------ 5. the module

MODULE = dict(mrange=(0.0, 7 * 150.0, 0.0, 5 * 150.0, 0.0, 450.0), mspacing=(150.0, 150.0, 150.0))


def _centres(G, mrange, mspacing, height=-20.0, extra=(0, 0)):
    """gridded data above the cell centres of the module's own mesh, whatever axis it calls x -- and `extra` more
    stations of the same lattice beyond its far edges: (x, y, z), bounds6"""
    b6 = G.mesher.PrismMesh(mrange, mspacing).cell_bounds()
    xc, yc = np.unique(0.5 * (b6[:, 0] + b6[:, 1])), np.unique(0.5 * (b6[:, 2] + b6[:, 3]))
    xc = xc[0] + (xc[1] - xc[0]) * np.arange(xc.size + extra[0])
    yc = yc[0] + (yc[1] - yc[0]) * np.arange(yc.size + extra[1])
    xp, yp = [a.ravel() for a in np.meshgrid(xc, yc, indexing="ij")]
    return (xp, yp, np.full(xp.size, height)), np.ascontiguousarray(b6)


def _sample(G, mod, M, tag):
    """a few draws of HMCSample with a fixed seed, the accepted samples folded into the posterior stream as well: the
    accepted rows of the binary sink (float64, every bit of the sample), the chain"""
    folder = "%s_chain" % tag
    ch = G.HMCSample(mod, 6, 2, 0.05, [3, 8], np.full(M, 0.01), np.full(M, 0.01), np.c_[np.full(M, -1.0), np.full(M, 1.0)],
                     "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "TV", 0.001, 5, 0.3, nbest=100, myrank=0,
                     save_folder=folder, sample_sink="binary", posterior_stream=True)
    return np.fromfile(folder + "0/model.bin").reshape(-1, M), ch


def test_module_matches_the_dense_module(G, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n, m = obs[0].size, b6.shape[0]
    M = 2 * m
    rng = np.random.default_rng(21)

    def make(dgz, dtf, ti, **kw):
        return G.JointModule(dgz, dtf, MODULE["mrange"], MODULE["mspacing"], obs, mangle=(C.INC, C.DEC), verbose=False,
                             **dict(kw, **(dict(translation_invariant=True) if ti else {})))

    probe = make(rng.normal(size=n), rng.normal(size=n), False)
    truth = np.zeros(M)
    truth[m // 3:m // 3 + m // 8], truth[m + m // 3:m + m // 3 + m // 8] = 0.4, 0.02
    d = probe.forward(truth)
    probe._engine.close()
    dgz = d[:n] + 0.01 * np.abs(d[:n]).max() * rng.normal(size=n)
    dtf = d[n:] + 0.01 * np.abs(d[n:]).max() * rng.normal(size=n)
    lat, dense = make(dgz, dtf, True, crossgradient=C.LAMBDA), make(dgz, dtf, False, crossgradient=C.LAMBDA)
    info = lat.translation_invariant_info()
    assert info["on"] and info["axes"] == 2 and 2 * info["nx"] * info["ny"] * info["nz"] == M and lat.translation_invariant
    assert info["table_bytes"] == 2 * info["nz"] * (info["nx"] + info["px"] - 1) * (info["ny"] + info["qy"] - 1) * 8
    assert info["chunks"] % 2 == 0 and info["max_dev"] <= FOLD_MAX_DEV
    assert not dense.translation_invariant and not dense._engine.translation_invariant_info()["on"]
    wm = dense.Wm.diagonal()
    assert relmax(lat.Wm.diagonal(), wm) <= TOL and relmax(lat.WmSquare.diagonal(), dense.WmSquare.diagonal()) <= TOL
    assert relmax(lat.WmInv.diagonal(), dense.WmInv.diagonal()) <= TOL
    assert abs(lat.std_gz - dense.std_gz) <= TOL * dense.std_gz and abs(lat.std_tf - dense.std_tf) <= TOL * dense.std_tf
    assert relmax(lat.Wb.diagonal(), dense.Wb.diagonal()) <= TOL and relmax(lat.dobsw, dense.dobsw) <= TOL
    x = rng.uniform(-1, 1, M) * wm
    for reg in C.REGS:
        a = lat.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5, regulization=reg, beta=0.001)
        _same_evaluation(a, b, n, "module %s" % reg)
        assert abs(lat.last_cross_gradient - dense.last_cross_gradient) <= TOL * abs(dense.last_cross_gradient)
        assert dense.last_cross_gradient > 0
    model = rng.uniform(-1, 1, M)
    fl, fd = lat.forward(model), dense.forward(model)
    assert relmax(fl[:n], fd[:n]) <= TOL and relmax(fl[n:], fd[n:]) <= TOL
    (pa, ga, ta), (pb, gb, tb) = lat.CrossGradient(model), dense.CrossGradient(model)
    assert abs(pa - pb) <= TOL * abs(pb) and relmax(ga, gb) <= TOL and relmax(ta, tb) <= TOL
    lat.set_cross_gradient(0.0)
    dense.set_cross_gradient(0.0)
    a = lat.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5)
    _same_evaluation(a, dense.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5), n, "module, coupling off")
    assert lat.last_cross_gradient == 0.0
    for mod in (lat, dense):
        mod.set_cross_gradient(C.LAMBDA)
    for what in (lambda: lat.Aw, lambda: lat.A, lambda: lat.kernel_gz, lambda: lat.kernel_tf):
        with pytest.raises(NotImplementedError, match=TSTORE):
            what()
    assert dense.kernel_gz.shape == (n, m) and lat.kernelw()[0] is not None
    # HMCSample with the same seed: the same accept / reject sequence, the accepted samples
    import re
    capsys.readouterr()
    rl, cl = _sample(G, lat, M, "lat")
    seq_l = re.findall(r"accept ratio ([0-9.]+)%", capsys.readouterr().out)
    rd, cd = _sample(G, dense, M, "dense")
    seq_d = re.findall(r"accept ratio ([0-9.]+)%", capsys.readouterr().out)
    assert rl.shape == rd.shape == (6, M)
    # every accepted sample, row by row
    worst = max(relmax(a_, b_) for a_, b_ in zip(rl, rd))
    print("accepted samples of the table against the dense module's:", worst)
    assert worst <= TOL
    # (the ratio after every trajectory is accepted / run so far: equal sequences are equal accept / reject sequences)
    assert len(seq_l) >= rl.shape[0] and seq_l == seq_d and cl.trajectories == cd.trajectories
    assert relmax(lat._engine.chain_get_x(), dense._engine.chain_get_x()) <= TOL
    # the posterior stream of the same run: against the dense module's stream, and against the rows it was fed
    pl, pd = lat._engine.posterior_stream_read(), dense._engine.posterior_stream_read()
    print("stream mean", relmax(pl["mean"], pd["mean"]), "std", relmax(pl["std"], pd["std"]))
    assert relmax(pl["mean"], pd["mean"]) <= TOL and relmax(pl["std"], pd["std"]) <= TOL
    assert relmax(np.ravel(pl["mean"]), rl.mean(axis=0)) <= TOL
    with pytest.raises(NotImplementedError, match=TSTORE):
        G.HMCSampleBatch(lat, 2, 1, 1, 0.1, (1, 2), None, None, None, "mandatory", 1.0, None, False, 1.0, 1.0, "Damping",
                         0.01, 1, None)
    lat._engine.close()
    dense._engine.close()


def test_module_beyond_the_dense_forms_limit(G, tmp_path, monkeypatch, capsys):
    """130 x 130 stations: the dense module raises, the table module builds and samples.  Fails on a module without
    translation_invariant=."""
    monkeypatch.chdir(tmp_path)
    mrange, mspacing = (0.0, 600.0, 0.0, 400.0, 0.0, 200.0), (100.0, 100.0, 100.0)
    obs, b6 = _centres(G, mrange, mspacing, -50.0)
    nxc, nyc = np.unique(obs[0]).size, np.unique(obs[1]).size
    obs, b6 = _centres(G, mrange, mspacing, -50.0, extra=(130 - nxc, 130 - nyc))
    n, M = obs[0].size, 2 * b6.shape[0]
    assert n == 16900
    rng = np.random.default_rng(31)
    dgz, dtf = rng.normal(size=n), rng.normal(size=n)
    with pytest.raises(NotImplementedError, match="16384"):
        G.JointModule(dgz, dtf, mrange, mspacing, obs, mangle=(C.INC, C.DEC), verbose=False)
    mod = G.JointModule(dgz, dtf, mrange, mspacing, obs, mangle=(C.INC, C.DEC), verbose=False, translation_invariant=True)
    assert mod._engine.N == 2 * n and mod.translation_invariant_info()["on"]
    G.HMCSample(mod, 2, 1, 0.05, [2, 3], np.full(M, 0.01), np.full(M, 0.01), np.c_[np.full(M, -1.0), np.full(M, 1.0)],
                "mandatory", 1000, mod.dobs, "Fixed", 0.8, 1.0, "Damping", 0.001, 5, 0.3, nbest=100, myrank=0,
                save_folder="big_chain", sample_sink="none")
    capsys.readouterr()
    assert np.all(np.isfinite(mod._engine.chain_get_x()))
    mod._engine.close()


# ---------------------------------------------------------------------------------------------- 6. refusals

def test_module_refusals_name_the_store_and_the_table(G):
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n = obs[0].size
    d = np.zeros(n)
    kw = dict(mangle=(C.INC, C.DEC), verbose=False, translation_invariant=True)
    with pytest.raises(NotImplementedError, match=TSTORE):
        G.JointModule(d, d, MODULE["mrange"], MODULE["mspacing"], obs, mtopo=(obs[0], obs[1], np.full(n, 100.0)), **kw)
    with pytest.raises(NotImplementedError, match=TSTORE):
        G.JointModule(d, d, MODULE["mrange"], MODULE["mspacing"], obs, **dict(kw, translation_invariant="chains"))
    # a geometry without the structure: n points from one end of the mesh to the other are L / (n - 1) apart
    xs, ys = np.linspace(0.0, 1050.0, 7), np.linspace(0.0, 750.0, 5)
    xp, yp = [a.ravel() for a in np.meshgrid(xs, ys, indexing="ij")]
    with pytest.raises(NotImplementedError, match=TSTORE) as err:
        G.JointModule(np.zeros(35), np.zeros(35), MODULE["mrange"], MODULE["mspacing"], (xp, yp, np.full(35, -20.0)), **kw)
    assert "spacing" in str(err.value)
    # the existing refusals stay first and unchanged
    with pytest.raises(NotImplementedError, match="spherical"):
        G.JointModule(d, d, MODULE["mrange"], MODULE["mspacing"], obs, coordinate="spherical", **kw)
    with pytest.raises(NotImplementedError, match="wavelet"):
        G.JointModule(d, d, MODULE["mrange"], MODULE["mspacing"], obs, wavelet="1D", **kw)
    with pytest.raises(ValueError, match="same length"):
        G.JointModule(d, d[:-1], MODULE["mrange"], MODULE["mspacing"], obs, **kw)


def test_engine_refusals(G):
    import ctypes
    from gravinv3dhmc_amd import _lib
    name = "4,9,3 / 5,8"
    obs, b6, op = host_store(name)
    n, m = op.n, op.m
    # gh_set_cells_joint's checks, without the row limit
    e = G.Engine(2 * n + 1, 2 * m)
    with pytest.raises(ValueError, match="even"):
        e.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
    e.close()
    e = G.Engine(2 * n, 2 * m)
    e.set_obs(*[np.ascontiguousarray(v) for v in np.concatenate([obs, obs], axis=1)])
    with pytest.raises(ValueError, match="fresh context"):
        e.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
    e.close()
    e = G.Engine(2 * 16386, 2)
    e.set_cells(np.array([[0, 1, 0, 1, 0, 1.0]]), _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
    e.close()
    for form in (G.Engine.set_matrix_free, G.Engine.set_translation_invariant):
        e = G.Engine(2 * n, 2 * m)
        form(e, True)
        with pytest.raises(NotImplementedError):
            e.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
        e.close()
    # a geometry without the structure: the detection's reason, from build_G
    o2, c2 = c2_linspace()
    e = G.Engine(2 * o2.shape[1], 2 * c2.shape[0])
    e.set_cells(c2, _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
    e.set_obs(*[np.ascontiguousarray(v) for v in o2])
    with pytest.raises(NotImplementedError, match=TSTORE) as err:
        e.build_G()
    assert "spacing" in str(err.value)
    e.close()
    # the table asked for with the cells cannot be taken away, and the other forms stay shut
    e = G.Engine(2 * n, 2 * m)
    e.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=C.direction(), translation_invariant=True)
    for on in (True, "chains", "replicates", False):
        with pytest.raises(NotImplementedError, match=JSTORE) as err:
            e.set_translation_invariant(on)
        assert "translation-invariant" in str(err.value)
    for call in (e.set_matrix_free, e.set_shift_invariant):
        with pytest.raises(NotImplementedError, match=JSTORE) as err:
            call(True)
        assert "translation-invariant table" in str(err.value)
    e.close()
    # what does not run on the built store: as on the dense store, each naming the store
    eng = C.joint_engine(G, obs, b6, True)
    wm = eng.weight(0.5)
    with pytest.raises(ValueError, match="grav_fix"):
        eng.set_data(np.zeros(2 * n), np.zeros(2 * n))
    eng.set_data(np.zeros(2 * n))
    eng.set_reg("Damping", 1.0, 0.01, C.mesh_shape(name), 0.0 * wm)
    x0 = np.stack([0.01 * wm, 0.02 * wm])
    for what, call in (("wavelet", lambda: eng.compress_wavelet(1, (1, 1, 2 * m), 0.001, 2)),
                       ("batch_init", lambda: eng.batch_init(x0, 0.0 * wm, 1.0 * wm)),
                       ("upload", lambda: eng.upload_G(np.zeros((2 * n, 2 * m)))),
                       ("bscg", lambda: eng.bscg_run(np.ones((2, 2 * n)), np.zeros(2 * n), 0.01 * wm, 0.0, 1.0, 0.0, 2, 4))):
        with pytest.raises(NotImplementedError, match="joint"):
            call()
    lib = _lib.load()
    id128 = ctypes.create_string_buffer(128)
    for fn, size in ((lib.gh_shard_init, 4 * m), (lib.gh_shard_init_rows, 4 * n)):
        rc = fn(eng._h, id128, 0, 2, size, 0)
        assert rc == _lib.GH_ERR_UNSUPPORTED and b"joint" in lib.gh_last_error(eng._h)
    with pytest.raises(ValueError):
        eng.download_G()
    info = eng.fold_info()
    assert not info["on"]
    eng.close()


def test_the_default_module_is_the_old_entry_points_engine(G):
    """translation_invariant=False: one dense evaluation of the module, bit for bit that of an engine built through
    gh_set_cells_joint by hand"""
    from gravinv3dhmc_amd import _lib
    obs, b6 = _centres(G, MODULE["mrange"], MODULE["mspacing"])
    n, m = obs[0].size, b6.shape[0]
    rng = np.random.default_rng(41)
    dgz, dtf = rng.normal(size=n), rng.normal(size=n)
    mod = G.JointModule(dgz, dtf, MODULE["mrange"], MODULE["mspacing"], obs, mangle=(C.INC, C.DEC), verbose=False)
    assert mod.translation_invariant is False and not mod.translation_invariant_info()["on"]
    assert np.asarray(mod.Aw).shape == (2 * n, 2 * m)
    eng = G.Engine(2 * n, 2 * m)
    assert eng._lib.gh_set_cells_joint(eng._h, _lib.ptr(b6), *C.direction()) == 0
    eng._set_store(_lib.CELL_PRISM_JOINT, cols=2, rows=2)
    eng.set_obs(*obs)
    eng.build_G()
    wm = eng.weight(0.5)
    assert np.array_equal(wm, mod.Wm.diagonal()) and eng.joint_std() == (mod.std_gz, mod.std_tf)
    eng.set_data(mod.dobsw)
    eng.set_reg("TV", 0.5, 0.001, mod.mshape, 0.01 * wm)
    x = rng.uniform(-1, 1, 2 * m) * wm
    a = mod.misfit_and_grad(x, 0.01 * wm, None, None, "mandatory", 1000, 0.5, regulization="TV", beta=0.001)
    b = eng.misfit_and_grad(x)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
    eng.close()
    mod._engine.close()
