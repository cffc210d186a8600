"""GPU suite (`-m gpu`): the stored-kernel chain batch (csrc/batch.hip.h, csrc/batchteam.hip.h, host_batch.h,
host_batchrun.h) against the CPU oracle, every chain of a batch against oracle.Problem.leapfrog on the same matrix.

The cases, their inputs and the oracle's trajectories come from tests/batch_oracle_cases.py (generated before an
engine is touched; tests/test_batch_oracle_host.py checks the generator and how sharp each case is).  Every case
runs with the resident kernels off (GRAVHMC_RESIDENT=0) through three drivers -- batch_trajectory in lock-step
rounds, batch_run with want_x, batch_run with GRAVHMC_BATCH_SPEC=0 -- and compares per chain and trajectory the
decision, out5, the reported x and batch_get_x after every round (after a rejection: the state before, bit for bit),
out5, x and the displacement x - x_before to TOL_TRAJ = 1e-10 in relmax.  A second engine given the same calls must
give the same bits.

Two passes (GRAVHMC_BATCH_TEAM=0, members == 0): the adjoint's row patches and ring of three, the forward's row
blocks and waves past ld, single / missing / partial column tiles, column blocks with a short last block, more pairs
of tiles than waves; the column-major adjoint (GRAVHMC_BATCH_RELAYOUT=0) on three of them, bit for bit with the
operand-ordered copy.  Teams (GRAVHMC_BATCH_TEAM=1): 8, 9 and 32 members, just outside the range (members == 0),
1 .. 4 tiles per range with a short last range, one tile, fewer tiles than ranges; members and ranges asserted
against bteam_plan restated from the CU count, launches > 0 and no time-out.  (The team kernel's time-out path stays
with tests/test_gpu_parity.py.)"""
import numpy as np
import pytest

import batch_oracle_cases as bc
from helpers import relmax

pytestmark = pytest.mark.gpu

TOL_TRAJ = bc.TOL_TRAJ
SWITCHES = ("GRAVHMC_BATCH_TEAM", "GRAVHMC_BATCH_RELAYOUT", "GRAVHMC_BATCH_SPEC", "GRAVHMC_BATCH_TEAM_TEST_ABORT")


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


def _engine(G, monkeypatch, d, env):
    """GRAVHMC_BATCH_TEAM / _RELAYOUT are read at the first batch_init: set before Engine(...), kept for its life."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = G.Engine(d.N, d.M)
    eng.upload_G(d.A)
    wm = eng.weight(0.5)
    assert relmax(wm, d.wm) <= 1e-14
    eng.set_data(d.dobs, d.gfix)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, 0.001 * wm)
    return eng


def _lockstep(eng, d):
    """batch_trajectory in rounds; batch_get_x of every chain after every round."""
    res = bc.Ref(d.C, d.T, d.M)
    eng.batch_init(d.x0s, d.low, d.high)
    for t in range(d.T):
        acc, out5 = eng.batch_trajectory(d.p0s[:, t], d.dt, d.Ls[:, t], d.us[:, t])
        res.acc[:, t], res.out5[:, t] = acc, out5
        for c in range(d.C):
            res.xs[c, t] = eng.batch_get_x(c)
    return res


def _desync(eng, d, monkeypatch, spec):
    """batch_run with want_x (x is reported after accepted trajectories); the final states through batch_get_x."""
    if spec:
        monkeypatch.delenv("GRAVHMC_BATCH_SPEC", raising=False)
    else:
        monkeypatch.setenv("GRAVHMC_BATCH_SPEC", "0")      # (read by every call)
    res = bc.Ref(d.C, d.T, d.M)
    eng.batch_init(d.x0s, d.low, d.high)
    acc, out5, xs = eng.batch_run(d.p0s, d.dt, d.Ls, d.us, want_x=True)
    monkeypatch.delenv("GRAVHMC_BATCH_SPEC", raising=False)
    res.acc[:], res.out5[:] = acc, out5
    for c in range(d.C):
        cur = d.x0s[c]
        for t in range(d.T):
            if acc[c, t]:
                cur = xs[c, t]
            res.xs[c, t] = cur
        assert np.array_equal(eng.batch_get_x(c), cur), (c, "final state")
    return res


def _against_oracle(d, res, what):
    """Decisions, out5, x and displacement of every chain and trajectory; returns the worst relmax."""
    ref, worst = d.ref, 0.0
    for c in range(d.C):
        for t in range(d.T):
            where = (d.spec.id, what, "chain %d" % c, "trajectory %d" % t, "L %d" % d.Ls[c, t])
            assert bool(res.acc[c, t]) == bool(ref.acc[c, t]), where + (res.out5[c, t], ref.out5[c, t])
            own_before = d.x0s[c] if t == 0 else res.xs[c, t - 1]
            x0 = bc.before(d, ref, c, t)
            e_o = relmax(res.out5[c, t], ref.out5[c, t])
            e_x = relmax(res.xs[c, t], ref.xs[c, t])
            e_d = 0.0
            if ref.acc[c, t]:
                e_d = relmax(res.xs[c, t] - x0, ref.xs[c, t] - x0)
            else:
                assert np.array_equal(res.xs[c, t], own_before), where
            worst = max(worst, e_o, e_x, e_d)
            assert e_o <= TOL_TRAJ, where + (e_o, res.out5[c, t], ref.out5[c, t])
            assert e_x <= TOL_TRAJ, where + (e_x, int(np.abs(res.xs[c, t] - ref.xs[c, t]).argmax()))
            assert e_d <= TOL_TRAJ, where + (e_d, int(np.abs(res.xs[c, t] - ref.xs[c, t]).argmax()))
    return worst


def _drivers(eng, d, monkeypatch):
    return [("lock-step", _lockstep(eng, d)), ("batch_run", _desync(eng, d, monkeypatch, True)),
            ("batch_run without the speculative step", _desync(eng, d, monkeypatch, False))]


def _same_bits(a, b):
    for (_, ra), (_, rb) in zip(a, b):
        assert np.array_equal(ra.acc, rb.acc) and np.array_equal(ra.out5, rb.out5) and np.array_equal(ra.xs, rb.xs)


def _layout(d, cus):
    """The case's own arithmetic: the partition it meant to reach."""
    s, p, tp = d.spec, bc.two_pass_plan(d.N, d.M, cus), bc.team_plan(d.N, d.M, cus)
    assert p["cols_per_block"] % 16 == 0 and 0 < p["last_block"] <= p["cols_per_block"]
    if s.M == "colblocks":
        assert p["cols_per_block"] >= 32 and p["n_colblocks"] > 1
        assert p["last_block"] < p["cols_per_block"] and p["last_block"] % 16 != 0
    if s.M == "pairs":
        assert p["npairs"] > p["n_waves"] == 16 * cus
    if s.team:
        assert tp["members"] == s.expect, tp
    if isinstance(s.M, tuple):
        assert tp["tpr"] == s.M[1] and 0 < tp["last_range"] and (s.M[1] == 1 or tp["last_range"] < tp["tpr"]), tp
    if s.id == "t-one-tile":
        assert p["ntiles"] == 1 and tp["ranges"] == 1
    if s.id == "t-few-tiles":
        assert tp["ranges"] == p["ntiles"] < cus // tp["members"]
    return p, tp


def _run_case(G, monkeypatch, cus, cid):
    d = bc.make(cid, cus)           # inputs and the oracle's trajectories, before an engine is touched
    s = d.spec
    p, tp = _layout(d, cus)
    env = {"GRAVHMC_BATCH_TEAM": 1 if s.team else 0}
    if s.team:
        from gravinv3dhmc_amd import isa_check
        assert isa_check.team_form_cleared(), "the build's scan has not cleared batch_team_kernel (%s)" % isa_check.STAMP
    runs = []
    for _ in range(2):              # a second engine given the same calls: the same bits
        eng = _engine(G, monkeypatch, d, env)
        eng.batch_init(d.x0s, d.low, d.high)
        st = eng.batch_fused_stats()
        assert (st["members"], st["ranges"]) == (tp["members"], tp["ranges"]) if s.team else st["members"] == 0, st
        runs.append(_drivers(eng, d, monkeypatch))
        st = eng.batch_fused_stats()
        eng.close()
        if s.team and s.expect:
            assert st["launches"] > 0 and st["timeouts"] == 0 and st["members"] == s.expect, st
        else:
            assert st["launches"] == 0 and st["members"] == 0, st
    worst = max(_against_oracle(d, res, what) for what, res in runs[0])
    _same_bits(runs[0], runs[1])
    if s.colmajor:
        # the column-major adjoint (no operand-ordered copy of G): the oracle's results, the relayout form's bits
        eng = _engine(G, monkeypatch, d, dict(env, GRAVHMC_BATCH_RELAYOUT=0))
        cm = _drivers(eng, d, monkeypatch)
        assert eng.batch_fused_stats()["members"] == 0
        eng.close()
        worst = max([worst] + [_against_oracle(d, res, what + ", column-major") for what, res in cm])
        _same_bits(runs[0], cm)
    print("%s (%s): N = %d, M = %d %r, C = %d, %s%s, np = %d, column blocks %d x %d + %d, members %d x ranges %d x %d "
          "tiles: worst relmax against the oracle %.2e"
          % (cid, s.group, d.N, d.M, d.shape, d.C, d.reg, " + grav_fix" if s.fix else "", p["np"], p["n_colblocks"] - 1,
             p["cols_per_block"], p["last_block"], tp["members"], tp["ranges"], tp["tpr"], worst))


@pytest.mark.parametrize("cid", [s.id for s in bc.TWO_PASS])
def test_two_pass_batch_against_oracle(G, monkeypatch, cus, cid):
    _run_case(G, monkeypatch, cus, cid)


@pytest.mark.parametrize("cid", [s.id for s in bc.TEAMS])
def test_batch_on_teams_against_oracle(G, monkeypatch, cus, cid):
    _run_case(G, monkeypatch, cus, cid)
