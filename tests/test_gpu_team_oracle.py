"""GPU suite (`-m gpu`): everything that runs when N > 16384 -- teamsweep_kernel<1024, 5, 3, LAG2> (csrc/teamsweep.hip.h),
the row-panel form of sweep_kernel with SW_GACC and vec_update_kernel (launch_sweep, csrc/host_sweep.h) -- against the CPU
oracle at its layout edges.

The cases, their inputs and the oracle's trajectories come from tests/team_oracle_cases.py (generated before an engine is
touched; tests/test_team_oracle_host.py checks the restated plans, the generator, and each case's conditioning and
sharpness).  A case first asserts Engine.team_info() and Engine.sweep_layout() against the plans restated at the device's
CU count, so it runs on the layout it names or fails.  Then, to the case's bound max(TOL_TRAJ, 10 x the spread of the
oracle under a reversal of the observation rows) in relmax:
  * weight(0.5) (to 1e-11), forward, adjoint and misfit_and_grad at a random model (adjoint-only panels with SW_GACC,
    forward-only panels);
  * the trajectories one by one through chain_trajectory (no speculation: the fused steps on teams, the last half step
    in row panels through vec_update_kernel): the decision, out5, chain_get_x() and the displacement x - x_before; after
    a rejection the state before, bit for bit; chain_get_dsyn() at the end;
  * again from chain_init through run_chain(batch=4, overlap=True), where an accepted proposal's last sweep takes the
    next first step (on teams: SW_PFIN | SW_SPEC, the |p|^2 partials of the teams and the zeroing of the panels' own):
    spec_hits and spec_misses both grow, decisions, states and potentials have the plain pass's bits.  The proposal's
    Hamiltonian holds |p|^2 summed per team there and per block of 256 cells in the plain pass -- two orders of one sum
    of M positive terms: equal to M x 2^-52 in relmax (on MI355X one proposal of twelve differs in its last bit at
    M = 637, none in the other cases), and to the oracle to the bound;
  * a second engine gives the first one's bits in both passes; the stateless leapfrog (chain_init + one trajectory) gives
    the bits of the chain's first trajectory, and meets the oracle from a later state.
Team cases: team_members == Q, team_launches > 0 and equal on both engines, no time-out.  Panel and refused cases: no
team launch (a refused plan reports no members)."""
import numpy as np
import pytest

import team_oracle_cases as tc
from helpers import relmax

pytestmark = pytest.mark.gpu

SWITCHES = ("GRAVHMC_TEAM", "GRAVHMC_TEAM_LAG", "GRAVHMC_TEAM_TPX", "GRAVHMC_TEAM_TEST_ABORT", "GRAVHMC_MIN_COLS", "GRAVHMC_TW",
            "GRAVHMC_PF", "GRAVHMC_NT", "GRAVHMC_WG_PER_CU")
TEAM_KEYS = ("on", "refusal", "Q", "panel_rows", "last_rows", "tpx", "n_teams", "cols_per_team", "grid", "lag", "lds_bytes")
PANEL_KEYS = ("n_panels", "rows_per_panel", "last_panel_rows")


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def cus(G):
    eng = G.Engine(16, 16)
    n = eng.device_info()["cus"]
    eng.close()
    return n


def _engine(G, monkeypatch, d):
    """The switches are read when the context is created and when it plans: set before Engine(...), kept for its life."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in d.spec.env.items():
        monkeypatch.setenv(k, str(v))
    eng = G.Engine(d.N, d.M)
    eng.upload_G(d.A)
    return eng


def _plans_match(eng, d, cus):
    """team_info() and sweep_layout() against the restated plans at this device's CU count, and the table's figures."""
    s = d.spec
    ts, pp = s.plans(cus)
    info, lay = eng.team_info(), eng.sweep_layout()
    assert dict((k, info[k]) for k in TEAM_KEYS) == dict((k, ts[k]) for k in TEAM_KEYS), (s.id, info, ts)
    assert dict((k, info[k]) for k in PANEL_KEYS) == dict((k, pp[k]) for k in PANEL_KEYS), (s.id, info, pp)
    want = {"tw": 16, "ept2": pp["ept2"], "pf": pp["pf"], "nt": 0, "n_teams": pp["panel_teams"], "cols_per_team": pp["panel_cols"],
            "grid": pp["panel_teams"], "n_panels": pp["n_panels"]}
    assert lay == want, (s.id, lay, want)
    both = dict(pp, **ts)
    if ts["on"]:
        both.update(tc.derived(ts, d.M))
    assert all(both[k] == v for k, v in s.expect.items()), (s.id, both, s.expect)
    return ts, pp


def _plain(eng, d):
    """The trajectories one by one through chain_trajectory; chain_get_x after each."""
    res = tc.Ref(1, d.T, d.M, d.N)
    eng.chain_init(d.x0s[0], d.low, d.high)
    for t in range(d.T):
        acc, o = eng.chain_trajectory(d.p0s[0, t], d.dt, int(d.Ls[0, t]), float(d.us[0, t]))
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = acc, o, eng.chain_get_x()
    return res, eng.chain_get_dsyn()


def _speculated(eng, d):
    """The same trajectories through run_chain in batches of four, every next momentum announced."""
    res = tc.Ref(1, d.T, d.M, d.N)
    eng.chain_init(d.x0s[0], d.low, d.high)
    out = []
    trajs = [(int(d.Ls[0, t]), d.p0s[0, t], float(d.us[0, t])) for t in range(d.T)]
    eng.run_chain(iter(trajs), d.dt, lambda L, acc, o, x: out.append((acc, o.copy(), x)), want_x=True, batch=4, overlap=True)
    assert len(out) == d.T
    cur = d.x0s[0]
    for t, (acc, o, x) in enumerate(out):
        assert (x is not None) == bool(acc)
        cur = x if acc else cur
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = acc, o, cur
    x_end = eng.chain_get_x()
    assert np.array_equal(x_end, cur), (d.spec.id, "final state")
    return res, eng.chain_get_dsyn()


def _against_oracle(d, res, what, tol):
    ref, worst = d.ref, 0.0
    for t in range(d.T):
        where = (d.spec.id, what, "trajectory %d" % t, "L %d" % d.Ls[0, t])
        assert bool(res.acc[0, t]) == bool(ref.acc[0, t]), where + (res.out5[0, t], ref.out5[0, t])
        own_before = d.x0s[0] if t == 0 else res.xs[0, t - 1]
        x0 = tc.before(d, ref, 0, t)
        e_o = relmax(res.out5[0, t], ref.out5[0, t])
        e_x = relmax(res.xs[0, t], ref.xs[0, t])         # (after a rejection too)
        e_d = 0.0
        if ref.acc[0, t]:
            e_d = relmax(res.xs[0, t] - x0, ref.xs[0, t] - x0)
        else:
            assert np.array_equal(res.xs[0, t], own_before), where
        worst = max(worst, e_o, e_x, e_d)
        assert e_o <= tol, where + (e_o, tol, res.out5[0, t], ref.out5[0, t])
        assert e_x <= tol, where + (e_x, tol, int(np.abs(res.xs[0, t] - ref.xs[0, t]).argmax()))
        assert e_d <= tol, where + (e_d, tol, int(np.abs(res.xs[0, t] - ref.xs[0, t]).argmax()))
    return worst


def _same_bits(a, b):
    assert np.array_equal(a.acc, b.acc) and np.array_equal(a.out5, b.out5) and np.array_equal(a.xs, b.xs)


def _one_engine(G, monkeypatch, d, cus, tol):
    """Everything one engine is asked; returns what a second engine must repeat bit for bit, and the worst relmax per
    group of results."""
    s = d.spec
    orc = d.orc
    eng = _engine(G, monkeypatch, d)
    ts, pp = _plans_match(eng, d, cus)              # (read-only: before the first sweep)
    wm = eng.weight(0.5)
    w = {"weight": relmax(wm, d.wm)}
    assert w["weight"] <= 1e-11, (s.id, w)
    assert _plans_match(eng, d, cus) == (ts, pp)
    eng.set_data(d.dobs, d.gfix)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, 0.001 * wm)
    # adjoint-only and forward-only sweeps: row panels in every case
    fwd, adj = eng.forward(d.x_probe), eng.adjoint(d.r_probe)
    a, b = eng.misfit_and_grad(d.x_probe), d.P.misfit_and_grad(d.x_probe)
    w["panels"] = max(relmax(fwd, orc.forward(d.Aw, d.x_probe)), relmax(adj, orc.adjoint(d.Aw, d.r_probe)),
                      abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]))
    assert w["panels"] <= tol, (s.id, "forward / adjoint / misfit_and_grad", w, tol)
    st0 = eng.chain_stats()
    assert st0["team_launches"] == 0
    plain, dsyn = _plain(eng, d)
    w["plain"] = max(_against_oracle(d, plain, "chain_trajectory", tol), relmax(dsyn, d.ref.dsyn[0, -1]))
    assert relmax(dsyn, d.ref.dsyn[0, -1]) <= tol, (s.id, "chain_get_dsyn", w, tol)
    st1 = eng.chain_stats()
    assert (st1["spec_hits"], st1["spec_misses"]) == (st0["spec_hits"], st0["spec_misses"])
    spec, dsyn2 = _speculated(eng, d)
    st2 = eng.chain_stats()
    assert st2["spec_hits"] > st1["spec_hits"] and st2["spec_misses"] > st1["spec_misses"], (s.id, st1, st2)
    w["speculated"] = max(_against_oracle(d, spec, "run_chain", tol), relmax(dsyn2, d.ref.dsyn[0, -1]))
    assert relmax(dsyn2, d.ref.dsyn[0, -1]) <= tol
    # the plain pass's bits; the proposal's Hamiltonian: |p|^2 in another order of its M terms
    assert np.array_equal(spec.acc, plain.acc) and np.array_equal(spec.xs, plain.xs)
    assert np.array_equal(spec.out5[0, :, :4], plain.out5[0, :, :4]) and np.array_equal(dsyn2, dsyn)
    h_spec, h_plain = spec.out5[0, :, 4], plain.out5[0, :, 4]
    w["h_bits"] = int((h_spec != h_plain).sum())
    assert np.abs(h_spec - h_plain).max() <= d.M * 2.0 ** -52 * np.abs(h_plain).max(), (s.id, h_spec, h_plain)
    # stateless: the chain's first trajectory bit for bit, and a later one from the oracle's state against the oracle
    x1, acc1, o1, ds1 = eng.leapfrog(d.x0s[0], d.p0s[0, 0], d.dt, int(d.Ls[0, 0]), d.low, d.high, float(d.us[0, 0]))
    assert acc1 == bool(plain.acc[0, 0]) and np.array_equal(o1, plain.out5[0, 0]) and np.array_equal(x1, plain.xs[0, 0])
    t = int(np.nonzero(d.ref.acc[0] & (d.Ls[0] >= 2))[0][0])
    x2, acc2, o2, ds2 = eng.leapfrog(tc.before(d, d.ref, 0, t), d.p0s[0, t], d.dt, int(d.Ls[0, t]), d.low, d.high, float(d.us[0, t]))
    w["stateless"] = max(relmax(o2, d.ref.out5[0, t]), relmax(x2, d.ref.xs[0, t]), relmax(ds2, d.ref.dsyn[0, t]))
    assert acc2 and w["stateless"] <= tol, (s.id, "leapfrog", t, w, tol)
    st = eng.chain_stats()
    eng.close()
    assert st["team_timeouts"] == 0
    if ts["on"]:
        assert st["team_members"] == ts["Q"] and st["team_launches"] > 0, (s.id, st)
    else:
        assert st["team_members"] == 0 and st["team_launches"] == 0, (s.id, st)
    return (plain, spec, dsyn, o1, x1, o2, x2, st["team_launches"]), w


@pytest.mark.parametrize("cid", [s.id for s in tc.CASES])
def test_case_against_oracle(G, monkeypatch, cus, cid):
    s = tc.BY_ID[cid]
    d = tc.make(cid, cus)       # inputs and the oracle's trajectories, before an engine is touched
    tol = d.bound()
    assert tc.TOL_TRAJ <= tol <= 1e-9 and d.N * d.M * 8 <= 90e6
    first, w = _one_engine(G, monkeypatch, d, cus, tol)
    second, _ = _one_engine(G, monkeypatch, d, cus, tol)
    _same_bits(first[0], second[0])
    _same_bits(first[1], second[1])
    assert all(np.array_equal(a, b) for a, b in zip(first[2:7], second[2:7])) and first[7] == second[7]
    ts, pp = s.plans(cus)
    how = ("teams: Q %d x %d rows (last %d), %d teams x %d columns, lag %d" % (ts["Q"], ts["panel_rows"], ts["last_rows"],
                                                                             ts["n_teams"], ts["cols_per_team"], ts["lag"])
           if ts["on"] else "row panels (%s): %d x %d rows (last %d)" % (ts["refusal"], pp["n_panels"], pp["rows_per_panel"],
                                                                         pp["last_panel_rows"]))
    print("%s (%s): N = %d, M = %d, %s%s, %s, team launches %d; spread %.2e, bound %.2e; worst relmax against the oracle: "
          "weight %.1e, panels %.2e, plain %.2e, speculated %.2e, stateless %.2e; proposals whose Hamiltonian differs in bits "
          "between the passes: %d of %d" % (cid, s.group, d.N, d.M, d.reg, " + grav_fix" if s.fix else "", how, first[7],
                                            d.spread(), tol, w["weight"], w["panels"], w["plain"], w["speculated"],
                                            w["stateless"], w["h_bits"], d.T))
