"""GPU suite (`-m gpu`): every instantiation of the dense fused sweep (sweep_kernel<TW, EPT2, PF, NT, JOINT>,
csrc/kernels.hip.h) against the CPU oracle.

configure_sweep (csrc/host_sweep.h) picks the instantiation in gh_create from ld = roundup16(N): one-wave teams up
to 1024 rows, four-wave teams up to 4096, eight-wave teams up to 6144 and sixteen-wave teams up to 16384, with
EPT2 = ceil(ld / (128 TW)) double2 per thread (7 becomes 8).  Every case asserts the layout it meant to reach
(Engine.sweep_layout), runs with the resident chain kernel off (GRAVHMC_RESIDENT=0) on uploaded random matrices (the
fold never engages: "not gz prisms"), and checks
  * the weights (weight_kernel<TW, EPT2>) against oracle.col_weight per column, the columns scaled over
    1e-20 .. 1e20 and one of them zero;
  * forward and adjoint against numpy, per entry relative to |A||x| and |A|^T|r|;
  * misfit_and_grad against oracle.Problem, with a data mean 10^3 times the data's spread (the mean removal), grav_fix
    in half the cases and every regulariser at every team width;
  * five trajectories through chain_trajectory, run_chain (the next trajectory's first step fused with the final
    half step: SW_SPEC) and leapfrog against oracle.Problem.leapfrog: the same decisions, accepted and rejected
    ones, cells clamped at both bounds, out5 and x to 1e-10; the three paths and a second run bit for bit;
  * the switches include/gravhmc.h calls tuning: GRAVHMC_PF / _NT give the same bits, GRAVHMC_TW / _WG_PER_CU /
    _MIN_COLS the oracle's results, and every sixteen-wave case also runs the two-launch epilogue
    (GRAVHMC_EPILOGUE1=0);
  * the column partition's edges: per team width a grid with fewer columns than the chip has teams, and a full grid
    of at least four columns per team with a short last team.
The joint store (JOINT = true) at 600, 2400, 5000 and 8192 observations per block reaches every team width; it is
checked against a numpy restatement of its potential (no mean removal) and of the leapfrog (oracle/numpy_port.py)."""
import contextlib
import io

import numpy as np
import pytest

from helpers import metropolis_u, relmax, shape3 as _shape, stable_dt as _dt

pytestmark = pytest.mark.gpu

SWITCHES = ("GRAVHMC_PF", "GRAVHMC_NT", "GRAVHMC_TW", "GRAVHMC_TW8", "GRAVHMC_WG_PER_CU", "GRAVHMC_MIN_COLS",
            "GRAVHMC_EPILOGUE1")
TOL_TRAJ = 1e-10
WANT = (True, False, True, False, True)   # decisions of the five trajectories


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cus(G):
    eng = G.Engine(16, 16)
    n = eng.device_info()["cus"]
    eng.close()
    return n


def _env(monkeypatch, env):
    """The switches of configure_sweep are read in gh_create (GRAVHMC_EPILOGUE1 at the first evaluation): set them
    before Engine(...) and keep them for the engine's life."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _team_columns(lay, M):
    """Columns of every team of the sweep launch, restated from sweep_kernel's partition (non-joint)."""
    cpt, n = lay["cols_per_team"], lay["n_teams"]
    if lay["tw"] == 1:
        out = []
        for b in range(lay["grid"]):
            jend = min(4 * cpt * (b + 1), M)
            for w in range(4):
                jb = 4 * cpt * b + w
                out.append((jend - jb + 3) // 4 if jb < jend else 0)
        return out
    return [max(0, min((t + 1) * cpt, M) - t * cpt) for t in range(n)]


# ----------------------------------------------------------------------------- trajectories

def _trajectories(P, x0, dt, rng):
    """Five trajectories of the oracle's chain from x0 in a box of +-1.5 dt: the decisions of WANT, a rejection only
    where the oracle's H rose by > 0.01, u half-way between 0 or 1 and exp(-dH) (far from the Metropolis edge).
    Returns low, high, the (L, p0, u) and the oracle's (accepted, out5, x) per trajectory."""
    M = x0.size
    low, high = x0 - 1.5 * dt, x0 + 1.5 * dt
    trajs, ref = [], []
    x = x0.copy()
    n_lo = n_hi = 0
    for want in WANT:
        for attempt in range(60):
            L = int(rng.integers(2, 7))
            scale = 0.7 ** attempt if want else 2.0 + 0.5 * attempt
            p0 = rng.normal(size=M) * scale
            o = P.leapfrog(x, p0, dt, L, low, high, 0.5)[2]
            dH = o[4] - o[3]
            if (want and dH < 5.0) or (not want and dH > 0.01):
                break
        else:
            raise AssertionError("no trajectory for the decision %r" % want)
        u = metropolis_u(dH, want)
        # the cells the first drift pushes past a bound (clamped, momentum reflected)
        xs = x + dt * (p0 - 0.5 * dt * P.misfit_and_grad(x)[1])
        n_lo += int((xs < low).sum())
        n_hi += int((xs > high).sum())
        xn, acc, o, _ = P.leapfrog(x, p0, dt, L, low, high, u)
        assert acc == want
        trajs.append((L, p0, float(u)))
        ref.append((acc, o, xn))
        x = xn
    assert n_lo > 0 and n_hi > 0, (n_lo, n_hi)
    return low, high, trajs, ref


def _paths(eng, x0, low, high, dt, trajs):
    """The trajectories through the three entry points that issue the fused modes."""
    eng.chain_init(x0, low, high)
    chain = []
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        chain.append((acc, o.copy(), eng.chain_get_x()))
    eng.chain_init(x0, low, high)
    piped = []
    eng.run_chain(iter(trajs), dt, lambda L, a, o, x: piped.append((a, o.copy(), None if x is None else x.copy())),
                  want_x=True, batch=2, overlap=True)
    piped_x = eng.chain_get_x()
    x, lf = x0, []
    for L, p0, u in trajs:
        x, acc, o, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        lf.append((acc, o.copy(), x.copy()))
    return chain, piped, piped_x, lf


def _check_paths(res, ref):
    chain, piped, piped_x, lf = res
    assert len(chain) == len(piped) == len(lf) == len(ref)
    for (a1, o1, x1), (a2, o2, x2), (a3, o3, x3), (ao, oo, xo) in zip(chain, piped, lf, ref):
        assert a1 == ao
        assert relmax(o1, oo) <= TOL_TRAJ, (o1, oo)
        assert relmax(x1, xo) <= TOL_TRAJ
        # the three paths: the same bits
        assert a1 == a2 == a3
        assert np.array_equal(o1, o2) and np.array_equal(o1, o3)
        assert np.array_equal(x1, x3)
        assert x2 is None or np.array_equal(x1, x2)
    assert np.array_equal(piped_x, chain[-1][2])


def _flat(res):
    chain, piped, piped_x, lf = res
    out = [np.asarray([a for a, _, _ in chain + piped + lf])]
    for run in (chain, piped, lf):
        for _, o, x in run:
            out.append(o)
            if x is not None:
                out.append(x)
    return out + [piped_x]


def _same_bits(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ----------------------------------------------------------------------------- dense cases

# (id, N, M or "full" / shape, regulariser, grav_fix, switches, expected (tw, ept2) or an edge of the partition)
BASE = [
    ("n100", 100, (3, 7, 11), "Damping", True, {}, (1, 1)),
    ("n250", 250, (4, 9, 13), "MS", False, {}, (1, 2)),
    ("n300", 300, (5, 8, 9), "Smoothness", True, {}, (1, 3)),
    ("n500", 500, (3, 11, 17), "TV", False, {}, (1, 4)),
    ("n600", 600, (6, 10, 11), "MS", True, {}, (1, 5)),
    ("n700", 700, (5, 9, 14), "Damping", False, {}, (1, 6)),
    ("n850", 850, (7, 8, 13), "TV", True, {}, (1, 8)),
    ("n1024", 1024, (4, 13, 15), "Smoothness", False, {}, (1, 8)),
    ("n1025", 1025, (5, 11, 13), "Damping", True, {}, (4, 3)),
    ("n1800", 1800, (4, 12, 17), "MS", False, {}, (4, 4)),
    ("n2500", 2500, (6, 9, 13), "Smoothness", True, {}, (4, 5)),
    ("n3000", 3000, (5, 10, 15), "TV", False, {}, (4, 6)),
    ("n3300", 3300, (4, 11, 19), "MS", True, {}, (4, 8)),
    ("n4096", 4096, (7, 9, 11), "Damping", False, {}, (4, 8)),
    ("n4097", 4097, (5, 12, 13), "Damping", True, {}, (8, 5)),
    ("n6144", 6144, (6, 11, 12), "MS", False, {}, (8, 6)),
    ("n4097-tw8off", 4097, (4, 13, 14), "TV", False, {"GRAVHMC_TW8": 0}, (16, 3)),
    ("n6145", 6145, (5, 13, 14), "Smoothness", True, {}, (16, 4)),
    ("n10000", 10000, (6, 12, 13), "TV", True, {}, (16, 5)),
    ("n12000", 12000, (7, 11, 13), "Damping", False, {}, (16, 6)),
    ("n14000", 14000, (6, 13, 13), "MS", True, {}, (16, 8)),
    ("n16384", 16384, (7, 12, 13), "Smoothness", False, {}, (16, 8)),
]

# the column partition's edges: "few" -- fewer columns than the chip has teams (one-wave teams: some empty);
# "full" -- a full grid of >= 4 columns per team, the last team short (one workgroup per CU keeps it small)
EDGES = [
    ("tw1-few", 300, (2, 5, 5), "TV", True, {}, (1, 3, "few")),
    ("tw1-full", 600, "full", "Smoothness", False, {"GRAVHMC_WG_PER_CU": 1}, (1, 5, "full")),
    ("tw4-few", 1800, (2, 5, 10), "Damping", True, {}, (4, 4, "few")),
    ("tw4-full", 2500, "full", "MS", False, {"GRAVHMC_WG_PER_CU": 1}, (4, 5, "full")),
    ("tw8-few", 4097, (2, 6, 10), "Smoothness", False, {}, (8, 5, "few")),
    ("tw8-full", 6144, "full", "TV", True, {"GRAVHMC_WG_PER_CU": 1}, (8, 6, "full")),
    ("tw16-few", 6145, (2, 5, 9), "MS", False, {}, (16, 4, "few")),
    ("tw16-full", 10000, "full", "Damping", True, {"GRAVHMC_WG_PER_CU": 1}, (16, 5, "full")),
]

# the overrides the header calls tuning: the oracle's results
OVERRIDES = [
    ("tw4-at-1000", 1000, (5, 10, 10), "MS", True, {"GRAVHMC_TW": 4}, (4, 2)),
    ("tw16-at-1000", 1000, (4, 10, 12), "TV", False, {"GRAVHMC_TW": 16}, (16, 1)),
    ("tw8-at-3000", 3000, (5, 9, 12), "Smoothness", True, {"GRAVHMC_TW": 8}, (8, 3)),
    ("tw16-at-3000", 3000, (3, 13, 14), "Damping", False, {"GRAVHMC_TW": 16}, (16, 2)),
    ("min-cols-3", 600, (5, 10, 14), "Damping", True, {"GRAVHMC_MIN_COLS": 3}, (1, 5)),
    ("wg1-min-cols-5", 12000, (6, 10, 14), "MS", False, {"GRAVHMC_WG_PER_CU": 1, "GRAVHMC_MIN_COLS": 5}, (16, 6)),
]


class _Case(object):
    """Inputs and the oracle's answers of one dense case."""

    def __init__(self, orc, N, shape, reg, fix, seed):
        self.N, self.shape, self.reg = N, shape, reg
        M = self.M = shape[0] * shape[1] * shape[2]
        rng = np.random.default_rng(seed)
        base = np.asfortranarray(rng.normal(size=(N, M)))
        # weights: columns over 1e-20 .. 1e20, one zero column
        self.wide = np.asfortranarray(base * 10.0 ** rng.uniform(-20, 20, size=M))
        self.zero = int(rng.integers(M))
        self.wide[:, self.zero] = 0.0
        self.Aw_wide, self.wm_wide = orc.col_weight(self.wide, 0.5)
        # the potential: columns over 0.5 .. 2, data with a mean 10^3 times its spread
        self.A = np.asfortranarray(base * rng.uniform(0.5, 2.0, size=M))
        self.Aw, self.wm = orc.col_weight(self.A, 0.5)
        self.dobs = rng.normal(size=N) + 1e3
        self.gfix = rng.normal(size=N) * 5 + 40.0 if fix else None
        self.alpha = 0.05 / N if reg == "MS" else 0.5
        self.beta = 0.01
        self.mwapr = rng.uniform(0.0, 0.1, size=M)
        self.P = orc.Problem(self.Aw, self.dobs, self.mwapr, reg, self.alpha, self.beta, wm=self.wm, shape=shape,
                             grav_fix=self.gfix)
        self.xm = rng.uniform(0.0, 1.0, size=M)
        self.mg = self.P.misfit_and_grad(self.xm)
        self.x0 = rng.uniform(0.3, 0.7, size=M)
        self.dt = _dt(self.P, self.x0, rng)
        self.low, self.high, self.trajs, self.ref = _trajectories(self.P, self.x0, self.dt, rng)
        self.xr = rng.normal(size=M), rng.normal(size=N)


def _exercise(eng, c, repeat=False):
    """Every call of the case on one engine; returns its outputs."""
    out = {}
    eng.upload_G(c.wide)
    out["wm_wide"] = eng.weight(0.5)
    Gw = eng.download_G()
    out["G_wide"] = Gw
    x, r = c.xr
    out["d"], out["g"] = eng.forward(x), eng.adjoint(r)
    eng.upload_G(c.A)
    out["wm"] = eng.weight(0.5)
    eng.set_data(c.dobs, c.gfix)
    eng.set_reg(c.reg, c.alpha, c.beta, c.shape, c.mwapr)
    out["mg"] = eng.misfit_and_grad(c.xm)
    out["paths"] = _paths(eng, c.x0, c.low, c.high, c.dt, c.trajs)
    if repeat:
        out["again"] = _paths(eng, c.x0, c.low, c.high, c.dt, c.trajs)
    return out


def _check_oracle(out, c):
    # weights, per column; the zero column keeps wm = 0 and its entries
    wm, wo = out["wm_wide"], c.wm_wide
    assert wm[c.zero] == 0.0 and wo[c.zero] == 0.0
    nz = wo != 0
    assert (np.abs(wm[nz] - wo[nz]) <= 1e-14 * wo[nz]).all(), np.max(np.abs(wm[nz] - wo[nz]) / wo[nz])
    Gw = out["G_wide"]
    assert not Gw[:, c.zero].any()
    colmax = np.abs(c.Aw_wide).max(axis=0)
    assert (np.abs(Gw - c.Aw_wide).max(axis=0) <= 3e-14 * colmax).all()
    # products against numpy on the stored matrix, per entry
    x, r = c.xr
    scale_d = np.abs(Gw) @ np.abs(x)
    scale_g = np.abs(Gw).T @ np.abs(r)
    assert (np.abs(out["d"] - Gw @ x) / scale_d).max() < 1e-14 * max(1, np.sqrt(c.M))
    assert out["g"][c.zero] == 0.0
    g_ref = Gw.T @ r
    nz = scale_g > 0
    assert (np.abs(out["g"][nz] - g_ref[nz]) / scale_g[nz]).max() < 1e-14 * max(1, np.sqrt(c.N))
    # the potential
    assert relmax(out["wm"], c.wm) <= 1e-14
    a, b = out["mg"], c.mg
    assert abs(a[0] - b[0]) <= 1e-11 * abs(b[0]), (a[0], b[0])
    assert relmax(a[1], b[1]) <= 1e-11 and relmax(a[2], b[2]) <= 1e-11
    _check_paths(out["paths"], c.ref)


def _flat_out(out):
    mg = out["mg"]
    return [out["wm_wide"], out["G_wide"], out["d"], out["g"], out["wm"], np.asarray(mg[0]), mg[1], mg[2],
            np.asarray(mg[3:])] + _flat(out["paths"])


def _run_case(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect, alt=True):
    if shape == "full":
        tw = expect[0]
        teams = cus * (4 if tw == 1 else 1)   # one workgroup per CU
        shape = _shape(4 * teams - 1)
    c = _Case(orc, N, shape, reg, fix, seed=sum(map(ord, cid)) * 7919 + N)
    _env(monkeypatch, env)
    eng = G.Engine(N, c.M)
    lay = eng.sweep_layout()
    print("%s: N = %d, M = %d, %s" % (cid, N, c.M, lay))
    assert (lay["tw"], lay["ept2"]) == tuple(expect[:2]), lay
    assert lay["n_panels"] == 1
    cols = _team_columns(lay, c.M)
    assert sum(cols) == c.M and len(cols) == lay["n_teams"]
    if len(expect) == 3:
        per_launch = cus * (4 if lay["tw"] == 1 else 1)
        if expect[2] == "few":
            assert c.M < per_launch
            if lay["tw"] == 1:
                assert 0 in cols          # empty one-wave teams
            else:
                assert lay["cols_per_team"] == 1 and lay["n_teams"] == c.M
        else:
            assert lay["n_teams"] == per_launch and lay["cols_per_team"] >= 4
            assert 0 < cols[-1] < lay["cols_per_team"]
    if "GRAVHMC_MIN_COLS" in env:
        assert lay["cols_per_team"] >= int(env["GRAVHMC_MIN_COLS"])
    out = _exercise(eng, c, repeat=True)
    eng.close()
    _check_oracle(out, c)
    # a second run of the same trajectories on the same engine: the same bits
    _same_bits(_flat(out["paths"]), _flat(out["again"]))
    ref_bits = _flat_out(out)
    if alt:
        # PF and NT change where the requests go, not the arithmetic: the same bits
        pf = 1 if lay["pf"] == 2 else 2
        _env(monkeypatch, dict(env, GRAVHMC_PF=pf, GRAVHMC_NT=1))
        eng = G.Engine(N, c.M)
        lay2 = eng.sweep_layout()
        assert (lay2["pf"], lay2["nt"]) == (pf, 1) and lay2["tw"] == lay["tw"] and lay2["ept2"] == lay["ept2"]
        out2 = _exercise(eng, c)
        eng.close()
        _same_bits(_flat_out(out2), ref_bits)
    if lay["tw"] == 16:
        # the two-launch epilogue (the mean of d formed after the slab is reduced)
        _env(monkeypatch, dict(env, GRAVHMC_EPILOGUE1=0))
        eng = G.Engine(N, c.M)
        assert eng.sweep_layout() == lay
        out3 = _exercise(eng, c)
        eng.close()
        _check_oracle(out3, c)


@pytest.mark.parametrize("cid,N,shape,reg,fix,env,expect", BASE, ids=[b[0] for b in BASE])
def test_sweep_instantiation_against_oracle(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect):
    _run_case(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect)


@pytest.mark.parametrize("cid,N,shape,reg,fix,env,expect", EDGES, ids=[e[0] for e in EDGES])
def test_sweep_partition_edges_against_oracle(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect):
    _run_case(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect, alt=False)


@pytest.mark.parametrize("cid,N,shape,reg,fix,env,expect", OVERRIDES, ids=[o[0] for o in OVERRIDES])
def test_sweep_tuning_overrides_against_oracle(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect):
    _run_case(G, orc, monkeypatch, cus, cid, N, shape, reg, fix, env, expect, alt=False)


# ----------------------------------------------------------------------------- joint store

MANGLE = (60.0, -10.0)


def _grid(n_y, n_x, x1=2000.0, y1=3000.0, h=0.0):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, y1, n_y), np.linspace(0, x1, n_x))]
    return xp, yp, np.full_like(xp, h)


def _cells(G, mrange, mspacing):
    with contextlib.redirect_stdout(io.StringIO()):
        mesh = G.mesher.PrismMesh(mrange, mspacing)
    return mesh.cell_bounds(active_only=True)


def _joint_engine(G, obs, cells, mangle=MANGLE):
    from gravinv3dhmc_amd import _lib, utils
    n, m = obs[0].size, cells.shape[0]
    eng = G.Engine(2 * n, 2 * m)
    eng.set_cells(cells, _lib.CELL_PRISM_JOINT, direction=utils.dircos(*mangle))
    eng.set_obs(*obs)
    eng.build_G()
    return eng


class _JointProblem(object):
    """The joint potential |H x - dobsw|^2 + alpha R(x - mwapr) on the block-diagonal H = diag(Hg, Ht) (no mean
    removal; Smoothness and TV per property with fd3d blocks), and oracle/numpy_port.py's leapfrog restated for it."""

    def __init__(self, H, m, dobsw, mwapr, reg, alpha, beta, wm, shape):
        import scipy.sparse as sp
        from gravinv3dhmc_amd.inversion.joint import fd3d
        self.Hg, self.Ht, self.m, self.n = np.asfortranarray(H[:, :m]), np.asfortranarray(H[:, m:]), m, H.shape[0]
        self.dobsw, self.mwapr, self.reg, self.alpha, self.beta = dobsw, mwapr, reg, alpha, beta
        self.wm2 = wm * wm
        self.R = sp.block_diag([fd3d(shape)] * 2, format="csr")

    def forward(self, x):
        return np.concatenate([self.Hg @ x[:self.m], self.Ht @ x[self.m:]])

    def adjoint(self, r):
        return np.concatenate([self.Hg.T @ r[:self.n], self.Ht.T @ r[self.n:]])

    def model(self, v):
        if self.reg == "Damping":
            return v @ v, 2 * v
        if self.reg == "MS":
            den = v * v + self.beta
            return np.sum(self.wm2 * v * v / den), 2 * self.beta * self.wm2 * v / den ** 2
        t = self.R @ v
        if self.reg == "Smoothness":
            return t @ t, 2 * (self.R.T @ t)
        s = np.sqrt(t * t + self.beta)
        return np.sum(s), self.R.T @ (t / s)

    def misfit_and_grad(self, x):
        dpre = self.forward(x)
        r = dpre - self.dobsw
        dv = r @ r
        mv, mg = self.model(x - self.mwapr)
        return dv + self.alpha * mv, 2 * self.adjoint(r) + self.alpha * mg, dpre, dv, mv

    def leapfrog(self, xcur, p0, dt, L, low, high, u):
        pnew, xnew = p0 * 1.0, xcur * 1.0
        K = np.dot(pnew, pnew) * 0.5
        U, grad, dsyn, U_data, U_model = self.misfit_and_grad(xnew)
        Hcur = K + U
        pnew -= dt * grad * 0.5
        for i in range(L):
            xnew += dt * pnew
            idx1, idx2 = xnew > high, xnew < low
            xnew[idx1], pnew[idx1] = high[idx1], -pnew[idx1]
            xnew[idx2], pnew[idx2] = low[idx2], -pnew[idx2]
            Unew, grad, dsyn_new, Unew_data, Unew_model = self.misfit_and_grad(xnew)
            pnew -= dt * grad if i < L - 1 else dt * grad * 0.5
        Hnew = np.dot(pnew, pnew) * 0.5 + Unew
        if Hnew < Hcur or u < np.exp(-(Hnew - Hcur)):
            return xnew, True, np.array([Unew, Unew_data, Unew_model, Hcur, Hnew]), dsyn_new
        return xcur, False, np.array([U, U_data, U_model, Hcur, Hnew]), dsyn


# (observations per block n = n_y n_x, prism spacing, regulariser of the trajectories, expected (tw, ept2))
JOINT = [
    ((30, 20), (250, 300, 200), "Damping", (1, 5)),
    ((60, 40), (200, 250, 250), "MS", (4, 5)),
    ((100, 50), (250, 200, 250), "Smoothness", (8, 5)),
    ((128, 64), (250, 250, 250), "TV", (16, 4)),    # 8192 observations per block: below the 16384 cap
]


@pytest.mark.parametrize("grid,mspacing,reg,expect", JOINT, ids=["n%d" % (j[0][0] * j[0][1]) for j in JOINT])
def test_joint_sweep_instantiation_against_numpy(G, monkeypatch, grid, mspacing, reg, expect):
    _env(monkeypatch, {})
    obs = _grid(*grid)
    mrange = (0, 2000, 0, 3000, 0, 1000)
    cells = _cells(G, mrange, mspacing)
    shape = (int(round(1000 / mspacing[0])), int(round(3000 / mspacing[1])), int(round(2000 / mspacing[2])))
    n, m = obs[0].size, cells.shape[0]
    assert m == shape[0] * shape[1] * shape[2]
    eng = _joint_engine(G, obs, cells)
    lay = eng.sweep_layout()
    print("joint n = %d, m = %d: %s" % (n, m, lay))
    assert (lay["tw"], lay["ept2"]) == expect and lay["n_panels"] == 1
    wm = eng.weight(0.5)
    H = eng.download_G()
    rng = np.random.default_rng(n + m)
    # forward and adjoint, per entry
    x, r = rng.normal(size=2 * m), rng.normal(size=2 * n)
    absP = _JointProblem(np.abs(H), m, np.zeros(2 * n), np.zeros(2 * m), "Damping", 0.0, 0.0, wm, shape)
    P0 = _JointProblem(H, m, np.zeros(2 * n), np.zeros(2 * m), "Damping", 0.0, 0.0, wm, shape)
    d, g = eng.forward(x), eng.adjoint(r)
    assert (np.abs(d - P0.forward(x)) / absP.forward(np.abs(x))).max() < 1e-14 * np.sqrt(m)
    assert (np.abs(g - P0.adjoint(r)) / absP.adjoint(np.abs(r))).max() < 1e-14 * np.sqrt(n)
    # the potential, every regulariser; data at the scale of H x
    dobsw = P0.forward(rng.uniform(0.3, 0.7, size=2 * m)) + rng.normal(size=2 * n) * np.abs(d).mean()
    eng.set_data(dobsw)
    mwapr = rng.uniform(0.0, 0.1, size=2 * m)
    xm = rng.uniform(0.0, 1.0, size=2 * m)
    beta = 0.01
    probs = {}
    for kind in ("Damping", "MS", "Smoothness", "TV"):
        # (MS: its curvature scales with wm^2; kept a small part of the data term's, as in the dense cases)
        alpha = 0.5 if kind != "MS" else 0.05 * np.abs(d).mean() ** 2 / np.mean(wm * wm)
        P = probs[kind] = _JointProblem(H, m, dobsw, mwapr, kind, alpha, beta, wm, shape)
        eng.set_reg(kind, alpha, beta, shape, mwapr)
        a, b = eng.misfit_and_grad(xm), P.misfit_and_grad(xm)
        assert abs(a[0] - b[0]) <= 1e-11 * abs(b[0]), kind
        assert relmax(a[1], b[1]) <= 1e-11 and relmax(a[2], b[2]) <= 1e-11, kind
        assert abs(a[3] - b[3]) <= 1e-11 * abs(b[3]) and abs(a[4] - b[4]) <= 1e-11 * abs(b[4]), kind
    # five trajectories against the restated leapfrog, through the three paths, and again
    P = probs[reg]
    eng.set_reg(reg, P.alpha, beta, shape, mwapr)
    x0 = rng.uniform(0.3, 0.7, size=2 * m)
    dt = _dt(P, x0, rng)
    low, high, trajs, ref = _trajectories(P, x0, dt, rng)
    res = _paths(eng, x0, low, high, dt, trajs)
    _check_paths(res, ref)
    _same_bits(_flat(res), _flat(_paths(eng, x0, low, high, dt, trajs)))
    eng.close()
