"""GPU suite (`-m gpu`): the bootstrap CG batch (Engine.bscg_run; csrc/bscg.hip.h, csrc/host_bscg.h) against the CPU
oracle, every replicate of a group against oracle.cg_port.bootstrap_counts in float64 on the same weighted matrix.

The cases, their inputs and the oracle's runs come from tests/bscg_oracle_cases.py (generated before an engine is
touched; tests/test_bscg_oracle_host.py checks the oracle's counts form, how well conditioned and how sharp each case
is, and that no branch of the recurrence sits on its edge).  Per case: models, dmis, mmis and alpha to
TOL_BSCG = 1e-10 in relmax, n_entries and n_alpha equal, bscg_stats() == 2 maxk + 1 forwards, maxk adjoints, maxk
lock-steps, and the layout the case was written for from bscg_run's launch arithmetic restated at the device's CU
count.  Groups: the adjoint's row patches and ring of three; single / missing / partial column tiles; the forward's
row blocks and the second and third pass of the 1024-thread loops; the grid-stride of the direction and step kernels;
column blocks with a short last block and more pairs of tiles than waves; the column-major adjoint
(GRAVHMC_BATCH_RELAYOUT=0) on three of them, bit for bit with the operand-ordered copy; contexts with bteam_plan on
(the adjoint's grid and bscg_mu_kernel's rows from the enlarged n_waves); one group of 16 that takes every branch of
the recurrence, and what a slot keeps from the group before."""
import numpy as np
import pytest

import bscg_oracle_cases as bc
from helpers import relmax

pytestmark = pytest.mark.gpu

TOL_BSCG = bc.TOL_BSCG
SWITCHES = ("GRAVHMC_BATCH_TEAM", "GRAVHMC_BATCH_RELAYOUT")
WORST = {}


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
    """GRAVHMC_BATCH_TEAM / _RELAYOUT are read when the batch buffers are made: set before Engine(...)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = G.Engine(d.N, d.M)
    eng.upload_G(d.A)
    wm = eng.weight(0.5)
    assert relmax(wm, d.wm) <= 1e-14
    return eng


def _run(eng, d, counts=None, maxk=None):
    maxk = maxk or d.maxk
    res = eng.bscg_run(d.counts if counts is None else counts, d.dobs, d.mw0, d.low, d.high, bc.BETA2, d.q, maxk)
    assert eng.bscg_stats() == {"forward_sweeps": 2 * maxk + 1, "adjoint_sweeps": maxk, "lock_steps": maxk}
    return res


def _against_oracle(d, res, ref, what):
    """Lengths equal, the four results of every replicate to TOL_BSCG; returns the worst relmax."""
    where = (d.spec.id, what)
    assert np.array_equal(res[4], ref.n_entries), where + (res[4], ref.n_entries)
    assert np.array_equal(res[5], ref.n_alpha), where + (res[5], ref.n_alpha)
    worst = 0.0
    for b in range(len(ref.n_alpha)):
        for name, v, w in zip(bc.NAMES, res, ref.results()):
            assert v[b].shape == w[b].shape
            err = relmax(v[b], w[b])
            worst = max(worst, err)
            assert err <= TOL_BSCG, where + ("replicate %d" % b, name, err, int(np.abs(v[b] - w[b]).argmax()))
    return worst


def _same_bits(a, b):
    for v, w in zip(a, b):
        assert np.array_equal(v, w)


def _layout(d, cus):
    """The case's own arithmetic: the launch it meant to reach."""
    s, p = d.spec, bc.plan(d.N, d.M, cus, d.spec.team)
    assert p["cols_per_block"] % 16 == 0 and 0 < p["last_block"] <= p["cols_per_block"]
    assert p["np"] == bc.roundup16(d.N) // 16 and p["ntiles"] == bc.cdiv(d.M, 16)
    if s.group in ("patches", "tiles", "branches"):
        assert p["npairs"] <= p["n_waves"] == 4 and p["nblk"] == p["ntiles"] and p["rowblocks"] == 1
    if s.group == "rowblocks":
        assert p["rowblocks"] == bc.cdiv(p["ld"], 512) and p["ld_passes"] == bc.cdiv(p["ld"], 1024)
        assert d.N < 1025 or (p["n_passes"] > 1 and p["ld_passes"] > 1)
    if s.group == "stride":
        assert p["nblk"] == 1024 and p["cell_passes"] == bc.cdiv(p["ntiles"], 1024)
        assert d.M == 16384 or p["cell_passes"] > 1
    if s.M == "colblocks":
        assert p["cols_per_block"] >= 32 and p["n_colblocks"] > 1
        assert p["last_block"] < p["cols_per_block"] and p["last_block"] % 16 != 0
    if s.M == "pairs":
        assert p["npairs"] > p["n_waves"] == 16 * cus and p["adjoint_waves"] == p["n_waves"]
    if s.team:
        assert bc.team_plan(d.N, d.M, cus)["members"] > 0
        assert p["adjoint_waves"] >= p["members"] * p["ranges"] > p["n_waves"]
    else:
        assert p["members"] == 0
    return p


@pytest.mark.parametrize("cid", [s.id for s in bc.TABLE])
def test_bscg_group_against_oracle(G, monkeypatch, cus, cid):
    d = bc.make(cid, cus)           # inputs and the oracle's run, before an engine is touched
    s = d.spec
    p = _layout(d, cus)
    env = {} if s.team else {"GRAVHMC_BATCH_TEAM": 0}
    eng = _engine(G, monkeypatch, d, env)
    res = _run(eng, d)
    st = eng.batch_fused_stats()    # (the batch buffers' plan: what bscg_run sized its adjoint grid from)
    eng.close()
    assert (st["members"], st["ranges"]) == (p["members"], p["ranges"]), st
    assert st["launches"] == 0
    worst = _against_oracle(d, res, d.ref, "relaid-out adjoint")
    if s.colmajor:
        # the column-major adjoint (no operand-ordered copy of G): the oracle's results, the relayout form's bits
        eng = _engine(G, monkeypatch, d, dict(env, GRAVHMC_BATCH_RELAYOUT=0))
        cm = _run(eng, d)
        eng.close()
        worst = max(worst, _against_oracle(d, cm, d.ref, "column-major adjoint"))
        _same_bits(res, cm)
    WORST[s.group] = max(WORST.get(s.group, 0.0), worst)
    print("%s (%s): N = %d, M = %d, B = %d, maxk = %d, q = %g, np = %d, %d tiles, column blocks %d x %d + %d, adjoint "
          "waves %d, nblk %d x %d passes: worst relmax against the oracle %.2e (group so far %.2e)"
          % (cid, s.group, d.N, d.M, d.B, d.maxk, d.q, p["np"], p["ntiles"], p["n_colblocks"] - 1, p["cols_per_block"],
             p["last_block"], p["adjoint_waves"], p["nblk"], p["cell_passes"], worst, WORST[s.group]))


def test_branches_of_the_recurrence_and_what_a_slot_keeps(G, monkeypatch, cus):
    """One group of 16 (49 x 47, bounds (0.2, 0.8), q = 0.5, maxk = 6) in which the oracle's trace shows alpha <- q alpha
    taken and not taken at one k, a replicate frozen at k = 1 beside 15 that run to the end, and cells on both
    bounds (tests/test_bscg_oracle_host.py asserts each); then, on that engine: a group of 3 with other counts (a
    freeze at k = 3 among them), the 16 permuted over the slots, and maxk = 2 after maxk = 6."""
    d = bc.make(bc.BRANCH.id, cus)
    _layout(d, cus)
    ref = d.ref
    assert (ref.n_alpha[0], ref.n_entries[0]) == (2, 0) and (ref.n_alpha[1:] == d.maxk).all()
    env = {"GRAVHMC_BATCH_TEAM": 0}
    eng = _engine(G, monkeypatch, d, env)
    res = _run(eng, d)
    worst = _against_oracle(d, res, ref, "group of 16")
    assert (res[0] == d.low).any() and (res[0] == d.high).any()
    # a group of 3 with other counts after the group of 16: the bits of that group on a fresh engine
    c3 = d.group_of_three()
    ref3 = d.run(d.Aw, c3)
    after16 = _run(eng, d, counts=c3)
    fresh = _engine(G, monkeypatch, d, env)
    alone = _run(fresh, d, counts=c3)
    _same_bits(after16, alone)
    assert np.array_equal(alone[4], ref3.n_entries) and np.array_equal(alone[5], ref3.n_alpha)
    assert list(alone[5]) == [4, 2, d.maxk]
    # the 16 permuted over the slots: the same bits per replicate
    perm = np.random.default_rng(3).permutation(d.B)
    assert (perm != np.arange(d.B)).sum() >= d.B - 2
    moved = _run(eng, d, counts=d.counts[perm])
    for v, w in zip(moved, res):
        assert np.array_equal(v, w[perm])
    # maxk = 2 after maxk = 6 (the result block reused with other offsets): the bits of a fresh engine, the oracle
    two = _run(eng, d, maxk=2)
    _same_bits(two, _run(fresh, d, maxk=2))
    worst = max(worst, _against_oracle(d, two, d.run(d.Aw, d.counts, maxk=2), "maxk = 2 after maxk = 6"))
    eng.close()
    fresh.close()
    print("branch (49 x 47, B = 16, maxk = 6, q = 0.5): worst relmax against the oracle %.2e" % worst)
