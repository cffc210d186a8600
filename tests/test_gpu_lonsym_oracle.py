"""GPU suite (`-m gpu`): the shift-invariant tesseroid store (csrc/lonsym.hip.h, lonsymh.hip.h, lonsymw.hip.h, lonres.hip.h,
host_lonsym.h, host_lonres.h) against the CPU oracle at its plan edges: weights, forward, adjoint, misfit_and_grad and every
trajectory against the oracle on its own dense tesseroid kernel.

The cases, their inputs and the oracle's trajectories come from tests/lonsym_oracle_cases.py (generated before an engine is
touched; tests/test_lonsym_oracle_host.py checks the restated plans, the conditioning and how sharp each case is).  Every
case sets its switches before the engine exists and first asserts Engine.shift_invariant_plan() against the plan restated
at the device's CU count, then the figures its table entry names: a case runs on the layout it names or fails.  Compared:
weight(0.5) to 1e-11; forward, adjoint and misfit_and_grad at a random model, and per trajectory the decision, out5, the
state and the displacement (after a rejection: the state before, bit for bit), to TOL_TRAJ = 1e-10 in relmax.

The trajectories run as five run_chain launches of unequal length (one of them a single trajectory), then all of them again
in one launch.  On the persistent launch shift_invariant_resident_stats() counts exactly those launches and no time-out,
GRAVHMC_RESIDENT_LOCAL=0 and a second engine give the default's bits, and chain_trajectory (launches per phase on the same
engine) meets the oracle.  On the launches per phase (direct, registers with GRAVHMC_LONSYM_RESIDENT=0 or where the
persistent launch is refused, streamed) the persistent launch counts nothing, and run_chain however the list is cut,
chain_trajectory, the stateless leapfrog and a second engine give the same bits.  Three chains (gh_batch_*): taking turns in
the persistent launch and on their own streams.  The direct form's refusals and n = 1025: gh_build_G names the reason."""
import re

import numpy as np
import pytest

import lonsym_oracle_cases as lc
from helpers import relmax
from test_gpu_resident_oracle import _against_oracle, _final_states, _same_bits, _single, _turns

pytestmark = pytest.mark.gpu

TOL_TRAJ = lc.TOL_TRAJ
SWITCHES = ("GRAVHMC_LONSYM_HARMONIC", "GRAVHMC_LONSYM_WIDE", "GRAVHMC_LONSYM_W", "GRAVHMC_LONSYM_ROWS", "GRAVHMC_LONSYM_FUSED",
            "GRAVHMC_LONSYM_RESIDENT", "GRAVHMC_LONSYM_TIMING", "GRAVHMC_LW_MIRROR", "GRAVHMC_LW_WAVES_PER_CU", "GRAVHMC_LW_FWD",
            "GRAVHMC_LW_BREAK", "GRAVHMC_LW_LDS_PAD", "GRAVHMC_RESIDENT_LOCAL", "GRAVHMC_LONRES_TEST_ABORT")
PLAN_KEYS = ("form", "n", "na", "nc", "nf", "W", "KB", "AG", "thr", "items", "grid", "lds", "direct_ok", "direct_refusal", "rp", "rw",
             "hgrid", "hlds", "nfp", "pairs", "wmirror", "witems", "wgrid", "wrows", "wparts", "n_xslots", "max_extra",
             "resident_planned", "resident_usable", "nwg", "resident_lds")
STATELESS = 4       # trajectories repeated with the stateless leapfrog


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


def _environment(monkeypatch, env):
    """The switches are read when the table is built (GRAVHMC_LONSYM_RESIDENT: at the first plan, GRAVHMC_RESIDENT_LOCAL: at
    every launch): set before Engine(...) and kept for its life."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _table(G, spec, N, M, obs, bounds):
    eng = G.Engine(N, M)
    eng.set_shift_invariant(True)
    eng.set_obs(*obs)
    eng.set_cells(bounds, 1, 1.6)
    eng.build_G()
    return eng


def _engine(G, monkeypatch, d, spec, env):
    _environment(monkeypatch, dict(spec.env, **env))
    eng = _table(G, spec, d.N, d.M, d.obs, d.bounds)
    e_w = relmax(eng.weight(0.5), d.wm)
    assert e_w <= lc.TOL_WEIGHT, (spec.id, "weight(0.5)", e_w)
    eng.set_data(d.dobs, d.gfix)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, d.mwapr)
    return eng, e_w


def _plan_matches(eng, spec, cus, env):
    """shift_invariant_plan() against the restated plan at this device's CU count, then the figures the table names."""
    info = eng.shift_invariant_plan()
    p = spec.plan(cus, env)
    assert "refused" not in p and info["on"], (spec.id, p, info)
    got, want = dict((k, info[k]) for k in PLAN_KEYS), dict((k, p[k]) for k in PLAN_KEYS)
    assert got == want, (spec.id, dict((k, (got[k], want[k])) for k in PLAN_KEYS if got[k] != want[k]))
    both = dict(info, **lc.derived(p))
    assert all(both[k] == v for k, v in spec.expect.items()), (spec.id, dict((k, both.get(k)) for k in spec.expect), spec.expect)
    return p


def _products(eng, d, what):
    """forward, adjoint and misfit_and_grad at the case's random model and residual; the worst relmax."""
    ref = d.quantities(d.P)
    mg = eng.misfit_and_grad(d.xr)
    got = [eng.forward(d.xr), eng.adjoint(d.rr), np.array([mg[0], mg[3], mg[4]]), mg[1], mg[2]]
    names = ("forward", "adjoint", "misfit / data / model values", "gradient", "predicted data")
    worst = 0.0
    for name, a, b in zip(names, got, ref):
        e = relmax(a, b)
        assert e <= TOL_TRAJ, (d.spec.id, what, name, e)
        worst = max(worst, e)
    return worst


def _one_by_one(eng, d):
    """chain_trajectory per trajectory: a Ref."""
    res = lc.Ref(1, d.T, d.M, d.N)
    eng.chain_init(d.x0s[0], d.low, d.high)
    cur = d.x0s[0]
    for t in range(d.T):
        acc, o = eng.chain_trajectory(d.p0s[0, t], d.dt, int(d.Ls[0, t]), float(d.us[0, t]))
        cur = eng.chain_get_x() if acc else cur
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = acc, o, cur
    return res


def _stateless(eng, d, res):
    """gh_leapfrog from the states run_chain went through: the same bits."""
    for t in range(min(STATELESS, d.T)):
        x0 = d.x0s[0] if t == 0 else res.xs[0, t - 1]
        x, acc, o, _ = eng.leapfrog(x0, d.p0s[0, t], d.dt, int(d.Ls[0, t]), d.low, d.high, float(d.us[0, t]))
        assert bool(acc) == bool(res.acc[0, t]) and np.array_equal(o, res.out5[0, t]), (d.spec.id, "stateless leapfrog", t)
        if acc:
            assert np.array_equal(x, res.xs[0, t]), (d.spec.id, "stateless leapfrog", t)


def _passes(eng, d, what, persistent, both=True):
    """The cut pass and the pass in one launch on one engine, each against the oracle; the persistent launch's counts."""
    st0 = eng.shift_invariant_resident_stats()
    res, n, x_end, d_end = _single(eng, d, d.launches())
    assert n == d.T
    worst = _against_oracle(d, res, what)
    e_x, e_d = relmax(x_end, d.ref.xs[0, -1]), relmax(d_end, d.ref.dsyn[0, -1])
    assert e_x <= TOL_TRAJ and e_d <= TOL_TRAJ, (d.spec.id, what, "chain_get_x / chain_get_dsyn", e_x, e_d)
    st = eng.shift_invariant_resident_stats()
    cuts = len(d.launches())
    assert st["timeouts"] == 0, (d.spec.id, what, st)
    assert st["launches"] - st0["launches"] == (cuts if persistent else 0), (d.spec.id, what, st0, st)
    if persistent:
        assert st["trajectories"] - st0["trajectories"] == d.T and st["workgroups"] > 0, (d.spec.id, what, st)
    res2 = None
    if both:
        res2, n2, x2, _ = _single(eng, d, [(0, d.T)])
        assert n2 == d.T
        worst = max(worst, _against_oracle(d, res2, what + ", one launch"))
        st2 = eng.shift_invariant_resident_stats()
        assert st2["timeouts"] == 0 and st2["launches"] - st["launches"] == (1 if persistent else 0), (d.spec.id, what, st2)
    return res, res2, max(worst, e_x, e_d)


# ----------------------------------------------------------------------------- the tests

def test_no_case_skips_on_a_256_cu_device(cus):
    """Every layout of the table fits one MI355X: a case may skip only where it wants more workgroups than the device has
    CUs."""
    assert max(s.cus_min for s in lc.CASES) == 256
    if cus >= 256:
        assert all(s.cus_min <= cus for s in lc.CASES)


@pytest.mark.parametrize("cid", [s.id for s in lc.CASES if s.C == 1])
def test_store_against_oracle(G, monkeypatch, cus, cid):
    s = lc.BY_ID[cid]
    if s.cus_min > cus:
        pytest.skip("%s wants %d workgroups, the device has %d CUs" % (cid, s.cus_min, cus))
    d = lc.make(cid)        # inputs and the oracle's trajectories, before an engine is touched
    persistent = bool(s.plan(cus)["resident_planned"])
    forms = [("default", {}), ("a second engine", {})]
    if persistent:
        forms.append(("GRAVHMC_RESIDENT_LOCAL=0", {"GRAVHMC_RESIDENT_LOCAL": 0}))
    runs, worst, e_w, e_p = [], 0.0, 0.0, 0.0
    for k, (what, env) in enumerate(forms):
        eng, e_w = _engine(G, monkeypatch, d, s, env)
        p = _plan_matches(eng, s, cus, env)
        if k == 0:
            e_p = _products(eng, d, what)
        r1, r2, w = _passes(eng, d, what, persistent, both=k == 0)
        worst = max(worst, w)
        runs.append(r1)
        if k == 0:
            one = _one_by_one(eng, d)
            worst = max(worst, _against_oracle(d, one, "chain_trajectory"))
            if not persistent:
                # (inside the persistent launch an evaluation forms its residuals against the mean of the evaluation
                # before, lonres.hip.h: where a launch is cut changes the last bits there, not here)
                _same_bits(r1, r2)
                _same_bits(r1, one)
                _stateless(eng, d, r1)
            assert eng.shift_invariant_resident_stats()["timeouts"] == 0
        eng.close()
    for r in runs[1:]:
        _same_bits(runs[0], r)
    print("%s (%s): n = %d, na = %d, nc = %d, N = %d, M = %d, slots %s (max_extra %d), %s%s, %s%s: weights %.2e, products %.2e, "
          "trajectories %.2e against the oracle"
          % (cid, s.group, s.n, s.na, s.nc, d.N, d.M, s.slots, s.max_extra, d.reg, " + grav_fix" if d.gfix is not None else "",
             p["form"], " persistent on %d workgroups, rw %d" % (p["nwg"], p["rw"]) if persistent else
             (" rw %d hgrid %d" % (p["rw"], p["hgrid"]) if p["form"] == "registers" else
              " pairs %d items %d parts %d mirror %d" % (p["pairs"], p["witems"], p["wparts"], p["wmirror"]) if p["form"] == "streamed"
              else " W %d KB %d AG %d thr %d items %d" % (p["W"], p["KB"], p["AG"], p["thr"], p["items"])), e_w, e_p, worst))


@pytest.mark.parametrize("cid", [s.id for s in lc.CHAINS])
def test_chains_on_the_store_against_oracle(G, monkeypatch, cus, cid):
    """gh_batch_* on the store: batch_run, batch_trajectory, batch_run.  Where the persistent launch is usable the chains
    take turns in it (one launch per chain and call), otherwise every chain runs on its own stream."""
    s = lc.BY_ID[cid]
    if s.cus_min > cus:
        pytest.skip("%s wants %d workgroups, the device has %d CUs" % (cid, s.cus_min, cus))
    d = lc.make(cid)
    eng, e_w = _engine(G, monkeypatch, d, s, {})
    p = _plan_matches(eng, s, cus, {})
    res, n_run, calls = _turns(eng, d)
    worst = max(_against_oracle(d, res, "chains"), _final_states(eng, d, res, n_run))
    st = eng.shift_invariant_resident_stats()
    eng.close()
    assert st["timeouts"] == 0 and st["launches"] == (calls * d.C if p["resident_planned"] else 0), (cid, st)
    print("%s (%s): n = %d, na = %d, nc = %d, N = %d, M = %d, C = %d, %s%s, %s, %s: weights %.2e, trajectories %.2e against the "
          "oracle" % (cid, s.group, s.n, s.na, s.nc, d.N, d.M, d.C, d.reg, " + grav_fix" if d.gfix is not None else "", p["form"],
                      "turns in the persistent launch on %d workgroups" % p["nwg"] if p["resident_planned"] else "own streams",
                      e_w, worst))


@pytest.mark.parametrize("rid", [r.id for r in lc.REFUSALS])
def test_refusals_name_their_reason(G, monkeypatch, rid):
    """n = 1025 (no form takes it) and the smallest shapes of the direct form's four limits with the harmonic forms off:
    gh_build_G fails with the reason the restated plan names."""
    r = [q for q in lc.REFUSALS if q.id == rid][0]
    assert r.plan() == {"refused": r.why}
    _environment(monkeypatch, r.env)
    bounds, obs, _, _ = lc.geometry(r)
    eng = G.Engine(obs[0].size, bounds.shape[0])
    eng.set_shift_invariant(True)
    eng.set_obs(*obs)
    eng.set_cells(bounds, 1, 1.6)
    with pytest.raises(NotImplementedError, match=re.escape("shift-invariant store: " + r.why)):
        eng.build_G()
    assert not eng.shift_invariant_plan()["on"]
    eng.close()
