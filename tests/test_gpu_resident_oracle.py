"""GPU suite (`-m gpu`): the resident kernels (csrc/resident.hip.h, csrc/resbatch.hip.h, host_resident.h,
host_resbatch.h) against the CPU oracle at their partition edges, every trajectory of every chain against
oracle.Problem.leapfrog on the same matrix.

The cases, their inputs and the oracle's trajectories come from tests/resident_oracle_cases.py (generated before an
engine is touched; tests/test_resident_oracle_host.py checks the restated plans, the generator and how sharp each case
is).  Every case fixes its partition with GRAVHMC_RESIDENT_WGS and first asserts Engine.resident_info() against the
restated plan at the device's CU count and LDS size, so a case runs on the layout it names or fails.  Compared per
trajectory: the decision, out5, the state and the displacement x - x_before (after a rejection: the state before, bit for
bit), to TOL_TRAJ = 1e-10 in relmax; at the end chain_get_x / chain_get_dsyn (batch_get_x); the number of resident
launches is the number of launches the case cut, and nothing timed out.

One chain (run_chain(batch=...) per launch): five launches whose tags run on, one of them a single trajectory with an
odd number of evaluations, then all trajectories again in one launch that stop_at_accepts ends mid-batch.  A second
engine, GRAVHMC_RESIDENT_LOCAL=0 and (where the plan keeps a register copy next to the LDS one) GRAVHMC_RESIDENT_REGS=0
give the default form's bits; split and stream associate the sums differently and meet the oracle only.  Chains taking
turns (GRAVHMC_RESIDENT_BATCH=0): batch_run, batch_trajectory, batch_run, the last two on the state the launch before
left on the device.  Chains in lock-step (GRAVHMC_RESIDENT_BATCH=1): carry-over offers, a drain, batch_trajectory, a
plain batch_run, as tests/test_gpu_resbatch.py drives C1.  The compressed forward (tests/golden/potential_small.npz,
wavelet 1D and 3D, TV): one chain and three in lock-step, to max(TOL_TRAJ, 10 x the spread between the oracle's two host
forms of that forward)."""
import numpy as np
import pytest

import resident_oracle_cases as rc
from helpers import relmax

pytestmark = pytest.mark.gpu

TOL_TRAJ = rc.TOL_TRAJ
SWITCHES = ("GRAVHMC_RESIDENT", "GRAVHMC_RESIDENT_WGS", "GRAVHMC_RESIDENT_REGS", "GRAVHMC_RESIDENT_CT", "GRAVHMC_RESIDENT_LOCAL",
            "GRAVHMC_RESIDENT_BATCH", "GRAVHMC_RESIDENT_STREAM", "GRAVHMC_RESIDENT_STREAM_MB", "GRAVHMC_RESIDENT_TIMING",
            "GRAVHMC_RESIDENT_TEST_ABORT", "GRAVHMC_RESBATCH_TEST_ABORT")
INFO_KEYS = ("cpw", "nwg", "rc", "ct", "split", "stream", "lds_cols")


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
    """The switches are read when the context plans (GRAVHMC_RESIDENT_LOCAL: at every launch): set before Engine(...)
    and kept for its life."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GRAVHMC_RESIDENT", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _engine(G, monkeypatch, d, env):
    _environment(monkeypatch, dict(d.spec.env, **env))
    eng = G.Engine(d.N, d.M)
    eng.upload_G(d.A)
    wm = eng.weight(0.5)
    assert relmax(wm, d.wm) <= 1e-14
    eng.set_data(d.dobs, d.gfix)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, 0.001 * wm)
    return eng


def _plan_matches(eng, d, cus, env):
    """resident_info() against the restated plan at this device's CU count and LDS size; returns (plan, lock-step plan)."""
    s = d.spec
    info = eng.resident_info(d.C)
    e = dict(s.env, **env)
    p = rc.resident_plan(d.N, d.M, cus, info["lds_max"], e)
    assert p is not None and info["planned"] and info["usable"] == rc.resident_usable(p, d.reg), (s.id, info, p)
    assert dict((k, info[k]) for k in INFO_KEYS) == dict((k, p[k]) for k in INFO_KEYS), (s.id, info, p)
    assert info["lds_bytes"] == rc.chains_lds_bytes(p, d.C) and eng.resident_info(1)["lds_bytes"] == p["lds"], (s.id, info, p)
    ls = rc.resbatch_plan(p, d.reg, d.C, d.gfix is not None, info["lds_max"], e)
    assert info["lockstep"] == (ls is not None), (s.id, info, ls)
    if ls is not None:
        assert (info["ks"], info["nt"], info["lockstep_lds_bytes"]) == (ls["ks"], ls["nt"], ls["lds"]), (s.id, info, ls)
    if info["lds_max"] == rc.LDS_MAX and not any(k.startswith("GRAVHMC_RESIDENT_REGS") for k in env):  # the table's figures
        both = dict(p, **rc.derived(p, d.M))
        assert all(both[k] == v for k, v in s.expect.items()), (s.id, both, s.expect)
    return p, ls


def _against_oracle(d, res, what, n_run=None, tol=TOL_TRAJ):
    """Decisions, out5, x and displacement of the first n_run[c] trajectories of every chain; the worst relmax."""
    ref, worst = d.ref, 0.0
    for c in range(d.C):
        for t in range(d.T if n_run is None else int(n_run[c])):
            where = (d.spec.id, what, "chain %d" % c, "trajectory %d" % t, "L %d" % d.Ls[c, t])
            assert bool(res.acc[c, t]) == bool(ref.acc[c, t]), where + (res.out5[c, t], ref.out5[c, t])
            own_before = d.x0s[c] if t == 0 else res.xs[c, t - 1]
            x0 = rc.before(d, ref, c, t)
            e_o = relmax(res.out5[c, t], ref.out5[c, t])
            e_x = relmax(res.xs[c, t], ref.xs[c, t])
            e_d = 0.0
            if ref.acc[c, t]:
                e_d = relmax(res.xs[c, t] - x0, ref.xs[c, t] - x0)
            else:
                assert np.array_equal(res.xs[c, t], own_before), where
            worst = max(worst, e_o, e_x, e_d)
            assert e_o <= tol, where + (e_o, res.out5[c, t], ref.out5[c, t])
            assert e_x <= tol, where + (e_x, int(np.abs(res.xs[c, t] - ref.xs[c, t]).argmax()))
            assert e_d <= tol, where + (e_d, int(np.abs(res.xs[c, t] - ref.xs[c, t]).argmax()))
    return worst


def _same_bits(a, b, n_run=None):
    for c in range(a.acc.shape[0]):
        n = a.acc.shape[1] if n_run is None else int(n_run[c])
        assert np.array_equal(a.acc[c, :n], b.acc[c, :n]) and np.array_equal(a.out5[c, :n], b.out5[c, :n])
        assert np.array_equal(a.xs[c, :n], b.xs[c, :n])


# ----------------------------------------------------------------------------- the drivers

def _single(eng, d, pieces, stop_at=0):
    """run_chain over the given (first, end) ranges, one library call (one launch) each; returns the results, the number
    of trajectories run, chain_get_x and chain_get_dsyn at the end."""
    res = rc.Ref(1, d.T, d.M, d.N)
    eng.chain_init(d.x0s[0], d.low, d.high)
    out = []
    for a, b in pieces:
        trajs = [(int(d.Ls[0, t]), d.p0s[0, t], float(d.us[0, t])) for t in range(a, b)]
        eng.run_chain(iter(trajs), d.dt, lambda L, acc, o, x: out.append((acc, o.copy(), x)), stop_at_accepts=stop_at,
                      want_x=True, batch=b - a)
    cur = d.x0s[0]
    for t, (acc, o, x) in enumerate(out):
        assert (x is not None) == bool(acc)
        cur = x if acc else cur
        res.acc[0, t], res.out5[0, t], res.xs[0, t] = acc, o, cur
    x_end, d_end = eng.chain_get_x(), eng.chain_get_dsyn()
    assert np.array_equal(x_end, cur), (d.spec.id, "final state")
    return res, len(out), x_end, d_end


def _single_passes(eng, d, what, tol=TOL_TRAJ):
    """The cut pass and the stop_at_accepts pass on one engine; launches and evaluations counted."""
    st0 = eng.chain_stats()
    res, n, x_end, d_end = _single(eng, d, d.launches())
    assert n == d.T
    worst = _against_oracle(d, res, what, tol=tol)
    e_x, e_d = relmax(x_end, d.ref.xs[0, -1]), relmax(d_end, d.ref.dsyn[0, -1])
    assert e_x <= tol and e_d <= tol, (d.spec.id, what, "chain_get_x / chain_get_dsyn", e_x, e_d)
    st = eng.chain_stats()
    ev = d.launch_evaluations()
    assert st["resident_launches"] - st0["resident_launches"] == len(ev), (d.spec.id, what, st)
    assert st["resident_evaluations"] - st0["resident_evaluations"] == sum(ev), (d.spec.id, what, st, ev)
    # all trajectories offered to ONE launch that ends at the STOP_AT-th acceptance
    k = d.stop_index()
    res2, n2, x2, d2 = _single(eng, d, [(0, d.T)], stop_at=rc.STOP_AT)
    assert n2 == k + 1, (d.spec.id, what, "stop_at_accepts", n2, k)
    worst = max(worst, _against_oracle(d, res2, what + ", stop_at_accepts", n_run=[n2], tol=tol))
    e_x, e_d = relmax(x2, d.ref.xs[0, k]), relmax(d2, d.ref.dsyn[0, k])
    assert e_x <= tol and e_d <= tol, (d.spec.id, what, "stop_at_accepts: chain_get_x / chain_get_dsyn", e_x, e_d)
    st2 = eng.chain_stats()
    assert st2["resident_launches"] - st["resident_launches"] == 1
    assert st2["resident_evaluations"] - st["resident_evaluations"] == 1 + int(d.Ls[0, :k + 1].sum())
    assert st2["resident_batch_launches"] == 0
    return res, res2, n2, max(worst, e_x, e_d)


def _turns(eng, d):
    """batch_run (two trajectories per chain), batch_trajectory, batch_run (two more): three launches when the chains
    take turns in the resident chain kernel, the second and third on the state kept on the device."""
    res = rc.Ref(d.C, d.T, d.M, d.N)
    n_run = [5] * d.C
    eng.batch_init(d.x0s, d.low, d.high)
    cur = [d.x0s[c] for c in range(d.C)]

    def run(t0, t1):
        acc, out5, xs = eng.batch_run(d.p0s[:, t0:t1], d.dt, d.Ls[:, t0:t1], d.us[:, t0:t1], want_x=True)
        for c in range(d.C):
            for t in range(t0, t1):
                if acc[c, t - t0]:
                    cur[c] = xs[c, t - t0].copy()
                res.acc[c, t], res.out5[c, t], res.xs[c, t] = acc[c, t - t0], out5[c, t - t0], cur[c]

    run(0, 2)
    acc, out5 = eng.batch_trajectory(d.p0s[:, 2], d.dt, d.Ls[:, 2], d.us[:, 2])
    for c in range(d.C):
        cur[c] = eng.batch_get_x(c)
        res.acc[c, 2], res.out5[c, 2], res.xs[c, 2] = acc[c], out5[c], cur[c]
    run(3, 5)
    for c in range(d.C):
        assert np.array_equal(eng.batch_get_x(c), cur[c]), (d.spec.id, c, "final state")
    return res, n_run, 3


def _lockstep(eng, d):
    """Two carry-over calls offering two trajectories per chain (a call ends when a chain has nothing left to start, the
    others stay in flight), a drain, batch_trajectory, a plain batch_run of one trajectory: every chain runs the head of
    its own list, as far as the carry-over calls took it plus two.  Returns the results, the trajectories run per chain
    and the launches of the lock-step kernel (the drain launches only where something was in flight)."""
    C = d.C
    res = rc.Ref(C, d.T, d.M, d.N)
    eng.batch_init(d.x0s, d.low, d.high)
    cur = [d.x0s[c] for c in range(C)]
    pos, done = [0] * C, [0] * C

    def take(acc, out5, xs, nd):
        for c in range(C):
            for i in range(int(nd[c])):
                t = done[c]
                if acc[c, i]:
                    cur[c] = xs[c, i].copy()
                res.acc[c, t], res.out5[c, t], res.xs[c, t] = acc[c, i], out5[c, i], cur[c]
                done[c] += 1

    launches = 0
    for _ in range(2):
        rows = lambda a: [[a[c, pos[c] + i] for i in range(2)] for c in range(C)]
        acc, out5, xs, ns, nd = eng.batch_run(rows(d.p0s), d.dt, rows(d.Ls), rows(d.us), want_x=True, carry=True)
        assert max(ns) == 2 and min(ns) >= 0        # (the call ended because a chain ran out of offers)
        for c in range(C):
            pos[c] += int(ns[c])
        take(acc, out5, xs, nd)
        launches += 1
    in_flight = any(pos[c] > done[c] for c in range(C))
    acc, out5, xs, ns, nd = eng.batch_run([[] for _ in range(C)], d.dt, np.zeros((C, 0)), np.zeros((C, 0)), want_x=True, carry=True)
    take(acc, out5, xs, nd)
    launches += 1 if in_flight else 0
    assert pos == done and min(pos) >= 1 and max(pos) <= 4, (d.spec.id, pos, done)
    pick = lambda a: np.stack([a[c, pos[c]] for c in range(C)])
    acc, out5 = eng.batch_trajectory(pick(d.p0s), d.dt, pick(d.Ls), pick(d.us))
    for c in range(C):
        cur[c] = eng.batch_get_x(c)
        res.acc[c, pos[c]], res.out5[c, pos[c]], res.xs[c, pos[c]] = acc[c], out5[c], cur[c]
        pos[c] += 1
    acc, out5, xs = eng.batch_run(pick(d.p0s)[:, None], d.dt, pick(d.Ls)[:, None], pick(d.us)[:, None], want_x=True)
    for c in range(C):
        if acc[c, 0]:
            cur[c] = xs[c, 0].copy()
        res.acc[c, pos[c]], res.out5[c, pos[c]], res.xs[c, pos[c]] = acc[c, 0], out5[c, 0], cur[c]
        pos[c] += 1
        assert np.array_equal(eng.batch_get_x(c), cur[c]), (d.spec.id, c, "final state")
    return res, pos, launches + 2


def _final_states(eng, d, res, n_run, tol=TOL_TRAJ):
    worst = 0.0
    for c in range(d.C):
        e = relmax(eng.batch_get_x(c), d.ref.xs[c, int(n_run[c]) - 1])
        assert e <= tol, (d.spec.id, "batch_get_x", c, e)
        worst = max(worst, e)
    used = [bool(d.ref.acc[c, t]) for c in range(d.C) for t in range(int(n_run[c]))]
    assert any(used) and not all(used)
    return worst


# ----------------------------------------------------------------------------- the tests

def test_no_case_skips_on_a_256_cu_device(cus):
    """Every partition of the tables fits one MI355X: a case may skip only where it wants more workgroups than the
    device has CUs."""
    need = max(s.wgs for s in rc.CASES)
    assert need == 256
    if cus >= 256:
        assert all(s.wgs <= cus for s in rc.CASES)


@pytest.mark.parametrize("cid", [s.id for s in rc.SINGLE])
def test_single_chain_against_oracle(G, monkeypatch, cus, cid):
    s = rc.BY_ID[cid]
    if s.wgs > cus:
        pytest.skip("%s wants %d workgroups, the device has %d CUs" % (cid, s.wgs, cus))
    d = rc.make(cid)        # inputs and the oracle's trajectories, before an engine is touched
    forms = [("default", {}), ("a second engine", {})]
    p = s.plan(cus)
    if s.group in ("topology", "rows"):
        forms.append(("GRAVHMC_RESIDENT_LOCAL=0", {"GRAVHMC_RESIDENT_LOCAL": 0}))
    if p["ct"] > 0 and not p["split"]:
        forms.append(("GRAVHMC_RESIDENT_REGS=0", {"GRAVHMC_RESIDENT_REGS": 0}))
    runs, worst = [], 0.0
    for what, env in forms:
        eng = _engine(G, monkeypatch, d, env)
        p, _ = _plan_matches(eng, d, cus, env)
        if "GRAVHMC_RESIDENT_REGS" in env and "GRAVHMC_RESIDENT_REGS" not in s.env:
            assert p["ct"] == 0 and not p["split"] and not p["stream"]
        r1, r2, n2, w = _single_passes(eng, d, what)
        eng.close()
        worst = max(worst, w)
        runs.append((r1, r2, n2))
    for r1, r2, n2 in runs[1:]:     # the order of every sum is defined by logical indices
        _same_bits(runs[0][0], r1)
        _same_bits(runs[0][1], r2, n_run=[n2])
    p = s.plan(cus)
    print("%s (%s): N = %d, M = %d %r, %s%s, %d x %d columns, rc %d ct %d%s%s, lds_cols %d, forms %d: worst relmax against "
          "the oracle %.2e" % (cid, s.group, d.N, d.M, d.shape, d.reg, " + grav_fix" if s.fix else "", p["nwg"], p["cpw"],
                               p["rc"], p["ct"], " split" if p["split"] else "", " stream" if p["stream"] else "",
                               p["lds_cols"], len(forms), worst))


@pytest.mark.parametrize("cid", [s.id for s in rc.TURNS + rc.FIT])
def test_chains_taking_turns_against_oracle(G, monkeypatch, cus, cid):
    s = rc.BY_ID[cid]
    if s.wgs > cus:
        pytest.skip("%s wants %d workgroups, the device has %d CUs" % (cid, s.wgs, cus))
    d = rc.make(cid)
    env = {"GRAVHMC_RESIDENT_BATCH": 0}
    eng = _engine(G, monkeypatch, d, env)
    p, ls = _plan_matches(eng, d, cus, env)
    assert ls is None
    fits = rc.chains_fit(p, d.reg, d.C, eng.resident_info(d.C)["lds_max"])
    res, n_run, launches = _turns(eng, d)
    worst = max(_against_oracle(d, res, "taking turns", n_run=n_run), _final_states(eng, d, res, n_run))
    st = eng.chain_stats()
    eng.close()
    # (where the chains do not fit the LDS next to the columns, the MFMA batch takes them: no resident launch)
    assert st["resident_launches"] == (launches if fits else 0) and st["resident_batch_launches"] == 0, (cid, fits, st)
    if fits:
        assert st["resident_evaluations"] == d.C + int(d.Ls[:, :5].sum()), (cid, st)
    print("%s: N = %d, M = %d, C = %d, %s, %s: worst relmax against the oracle %.2e"
          % (cid, d.N, d.M, d.C, d.reg, "resident launches %d" % st["resident_launches"] if fits else "MFMA batch", worst))


@pytest.mark.parametrize("cid", [s.id for s in rc.LOCKSTEP])
def test_chains_in_lockstep_against_oracle(G, monkeypatch, cus, cid):
    s = rc.BY_ID[cid]
    if s.wgs > cus:
        pytest.skip("%s wants %d workgroups, the device has %d CUs" % (cid, s.wgs, cus))
    d = rc.make(cid)
    eng = _engine(G, monkeypatch, d, {})
    p, ls = _plan_matches(eng, d, cus, {})
    assert (ls is not None) == bool(s.lockstep), (cid, ls)
    if ls is not None:
        assert all(ls[k] == v for k, v in s.lockstep.items())
        res, n_run, launches = _lockstep(eng, d)
    else:
        res, n_run, launches = _turns(eng, d)       # resbatch_plan refuses: the chains take turns
    worst = max(_against_oracle(d, res, "lock-step" if ls else "taking turns", n_run=n_run), _final_states(eng, d, res, n_run))
    st, rb = eng.chain_stats(), eng.batch_resident_stats()
    eng.close()
    assert rb["timeouts"] == 0
    if ls is not None:
        # (+ 1: the launch of the chain kernel without trajectories that evaluates the starts, resbatch_state)
        assert rb["launches"] == launches and st["resident_launches"] == 1 and rb["chain_steps"] > 0, (cid, rb, st)
    else:
        assert rb["launches"] == 0 and st["resident_launches"] == launches, (cid, rb, st)
    print("%s: N = %d, M = %d %r, C = %d, %s%s, %d x %d columns, %s, trajectories per chain %d .. %d: worst relmax against "
          "the oracle %.2e" % (cid, d.N, d.M, d.shape, d.C, d.reg, " + grav_fix" if s.fix else "", p["nwg"], p["cpw"],
                               "KS %d NT %d" % (ls["ks"], ls["nt"]) if ls else "taking turns", min(n_run), max(n_run), worst))


@pytest.mark.parametrize("wavelet", ["1D", "3D"])
def test_compressed_forward_against_oracle(G, monkeypatch, wavelet):
    """LDS holds the dense model-space form of the compressed forward, the dots read Aw from the register copy
    (GREG in lock-step): one chain, and three chains in lock-step, on the device's own kernel and weights."""
    from conftest import gold
    _environment(monkeypatch, {})
    g = gold("potential_small.npz")
    dims = 3 if wavelet == "3D" else 1
    worst = []
    for C in (1, 3):
        gm = G.GravMagModule(g["dobs"], tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"]), wavelet=wavelet,
                             verbose=False)
        wm = gm.Wm.diagonal()
        Aw = np.asarray(gm.Aw)
        assert relmax(Aw, g["Aw"]) <= 1e-11 and relmax(wm, g["wm"]) <= 1e-11
        d = rc.compressed(dims, C, Aw, wm)
        assert gm.Awcp.shape == d.csr.shape and gm.Awcp.nnz == d.csr.nnz
        tol = d.bound()
        gm._use_reg("TV", d.alpha, d.beta, d.mwapr)
        eng = gm._engine
        info = eng.resident_info(C)
        cus = eng.device_info()["cus"]
        p = rc.resident_plan(d.N, d.M, cus, info["lds_max"])
        assert info["usable"] and dict((k, info[k]) for k in INFO_KEYS) == dict((k, p[k]) for k in INFO_KEYS) and p["ct"] > 0
        if C == 1:
            w = _single_passes(eng, d, "compressed forward " + wavelet, tol=tol)[3]
        else:
            assert info["lockstep"] and (info["ks"], info["nt"]) == (5, 1)
            assert info["lockstep_lds_bytes"] == rc.resbatch_lds_doubles(p["ld"], p["cpw"], False, True) * 8
            res, n_run, launches = _lockstep(eng, d)
            w = max(_against_oracle(d, res, "compressed forward %s, lock-step" % wavelet, n_run=n_run, tol=tol),
                    _final_states(eng, d, res, n_run, tol=tol))
            rb = eng.batch_resident_stats()
            assert rb["launches"] == launches and rb["timeouts"] == 0, rb
        eng.close()
        worst.append(w)
        print("compressed forward %s, %d chain(s): spread of the host forms %.2e, bound %.2e, worst relmax against the oracle "
              "%.2e" % (wavelet, C, d.spread(), tol, w))
