"""The cases of everything that runs when N > 16384 against the CPU oracle (tests/test_gpu_team_oracle.py on the device,
tests/test_team_oracle_host.py for the generator, the restated plans and how sharp and how well conditioned every case
is): teamsweep_kernel<1024, 5, 3, LAG2> (csrc/teamsweep.hip.h), the row-panel form of sweep_kernel with its SW_GACC
accumulation (launch_sweep in csrc/host_sweep.h) and vec_update_kernel with the hand-over of the |p|^2 partials.

Two plans are restated here from (N, M, CUs, lag, cap): team_shape (csrc/host_sweep.h) and the row-panel branch of
configure_sweep (n_panels, panel_rows, EPT2, PF and the column partition).  The team cases run with GRAVHMC_TEAM_TPX=1
unless they say otherwise: 8 teams at every Q on any device with at least 64 CUs, so a handful of columns reaches every
run length of the rotation (three register buffers, two columns of lag, one column parked in LDS, a tail of its own for
the columns cnt - 2 and cnt - 1).

A case is a random Fortran-ordered matrix (column scales over 0.1 .. 3, weighted with 0.5), data with a mean 10^3 times
their spread, grav_fix in half the cases, the four regularisers in rotation, ONE chain in a box of +-1.5 dt and T = 12
trajectories with L in 1 .. 6 (the first L = 1), six accepted and six rejected.  Everything the device is compared with
comes from oracle.Problem.leapfrog before an engine exists.  The variate of a trajectory sits half-way between the
oracle's exp(-dH) and 0 or 1 (helpers.metropolis_u); a rejection is used only where dH > 0.01.

Conditioning.  A column's dot with r is a sum over 16385 .. 81680 observations, and the oracle's own result depends on
the order of that sum.  Data.spread(): the distance between the oracle on (A, dobs, grav_fix) and the oracle on the same
problem with the observation rows reversed -- the same mathematics, every sum over the observations in another order.
The device is held to Data.bound() = max(TOL_TRAJ, 10 x spread); a case whose spread exceeds MAX_SPREAD gets a shorter
list of trajectories (Spec.T), never a looser bound, so every bound stays at or below 1e-9.

Sharpness.  Data.probes(): (a) a line of 16 rows in all columns, (b) the rows of one member or panel in one column, each
scaled by 1 + delta, must move the oracle alone by more than 100 x the case's bound (delta = 1e-4 unless the table says
1e-3)."""
import functools

import numpy as np

from helpers import metropolis_u, relmax, shape3, stable_dt

TOL_TRAJ = 1e-10
MAX_SPREAD = 1e-10
DELTA = 1e-4

# csrc/teamsweep.hip.h, csrc/host_sweep.h
TS_THREADS, TS_EPT2, TS_MAXQ, TS_MAXWAVES = 1024, 5, 8, 16
TS_LDS_SMALL = (2 * TS_MAXWAVES + 4) * 8
LDS_MAX = 160 * 1024
PANEL_MAX_ROWS = 10240
ONE_WORKGROUP_ROWS = 16384
REFUSALS = (None, "switch off", "matrix-free / joint", "single panel", "Q > 8", "too few CUs", "tpx < 1", "LDS", "residency")


def roundup16(n):
    return (n + 15) // 16 * 16


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- the plans, restated

def member_cap(lag):
    """Rows a member holds of a column: five double2 per thread; with two columns of lag its part of r and the parked
    column share the LDS."""
    cap = TS_THREADS * TS_EPT2 * 2
    if lag == 2:
        cap = min(cap, (LDS_MAX - TS_LDS_SMALL) // 16 // 16 * 16)
    return cap


def panel_plan(N, M, cus, env=None):
    """configure_sweep for a stored kernel on one device: the row panels (one: a workgroup holds a column) and, for
    N > 16384, the instantiation and the column partition of the panel launches."""
    env = env or {}
    ld = roundup16(N)
    if ld <= ONE_WORKGROUP_ROWS:
        return {"ld": ld, "n_panels": 1, "rows_per_panel": ld, "last_panel_rows": ld}
    n_panels = cdiv(ld, PANEL_MAX_ROWS)
    rows = roundup16(cdiv(ld, n_panels))
    e = cdiv(rows, 16 * 128)
    if e == 7:
        e = 8
    pf = 2 if e == 5 else 1
    cpt = max(cdiv(M, cus), int(env.get("GRAVHMC_MIN_COLS", 1)))       # one workgroup of 16 waves per CU
    n_teams = cdiv(M, cpt)
    return {"ld": ld, "n_panels": n_panels, "rows_per_panel": rows, "last_panel_rows": ld - (n_panels - 1) * rows,
            "tw": 16, "ept2": e, "pf": pf, "nt": 0, "panel_cols": cpt, "panel_teams": n_teams,
            "n_pp": max(n_teams, 128, cdiv(M, 256)), "update_blocks": cdiv(M, 256)}


def team_shape(N, M, cus, lag=2, tpx_cap=0, env=None):
    """team_shape of csrc/host_sweep.h with the refusals that need no device in front of it: `on`, `refusal` and the
    figures Engine.team_info() names (0 past the refusal)."""
    env = env or {}
    ld = roundup16(N)
    s = {"on": False, "refusal": None, "Q": 0, "panel_rows": 0, "last_rows": 0, "tpx": 0, "n_teams": 0, "cols_per_team": 0,
         "grid": 0, "lag": 0, "lds_bytes": 0}

    def refused(why):
        assert why in REFUSALS
        s["refusal"] = why
        return s

    if int(env.get("GRAVHMC_TEAM", 1)) == 0:
        return refused("switch off")
    if ld <= ONE_WORKGROUP_ROWS:
        return refused("single panel")
    s["lag"] = lag = 1 if lag == 1 else 2
    s["Q"] = Q = max(2, cdiv(ld, member_cap(lag)))
    if Q > TS_MAXQ:
        return refused("Q > 8")
    if cus < 8 * Q:
        return refused("too few CUs")
    s["panel_rows"] = rows = roundup16(cdiv(ld, Q))
    s["last_rows"] = max(0, ld - (Q - 1) * rows)
    s["tpx"] = tpx = min(32, cus // 8) // Q
    if tpx < 1:
        return refused("tpx < 1")
    if tpx_cap > 0:
        s["tpx"] = tpx = min(tpx, tpx_cap)
    s["grid"] = 8 * tpx * Q
    s["n_teams"] = 8 * tpx
    s["cols_per_team"] = cdiv(M, 8 * tpx)
    s["lds_bytes"] = rows * lag * 8 + TS_LDS_SMALL
    if s["lds_bytes"] > LDS_MAX:
        return refused("LDS")
    s["on"] = True
    return s


def derived(s, M):
    """What teamsweep_kernel derives from the shape: the rows of every member, the live threads of the fifth double2
    slot, the column runs of the teams."""
    Q, rows, ld = s["Q"], s["panel_rows"], (s["Q"] - 1) * s["panel_rows"] + s["last_rows"]
    member_rows = [min(rows, max(0, ld - q * rows)) for q in range(Q)]
    cpt = s["cols_per_team"]
    runs = [max(0, min(M, (t + 1) * cpt) - t * cpt) for t in range(s["n_teams"])]
    return {"member_rows": member_rows,
            "fifth_slot": [max(0, min(TS_THREADS, r // 2 - 4 * TS_THREADS)) for r in member_rows],
            "runs": runs, "idle_teams": sum(1 for r in runs if r == 0)}


# ----------------------------------------------------------------------------- the case tables

S, D, MS, TV = "Smoothness", "Damping", "MS", "TV"
REGS = (D, S, MS, TV)


class Spec(object):
    """M: a number, or ("grid", a, b): a x n_teams + b columns at the device's team count (no cap on the teams).
    expect: the figures the table names (keys of team_shape, derived or panel_plan)."""

    def __init__(self, cid, group, N, M, reg, fix, lag=2, tpx=1, team=True, env=None, expect=None, T=12, delta=DELTA, seed=0):
        self.id, self.group, self.N, self.M, self.reg, self.fix, self.lag, self.tpx = cid, group, N, M, reg, fix, lag, tpx
        self.team, self.expect, self.T, self.delta, self.C = team, expect or {}, T, delta, 1
        self.seed = sum(map(ord, cid)) * 7919 + N + seed           # of the generator of the trajectories
        self.env = dict(env or {})
        self.env["GRAVHMC_TEAM"] = 1 if team else 0
        if team:
            self.env["GRAVHMC_TEAM_LAG"] = lag
            if tpx:
                self.env["GRAVHMC_TEAM_TPX"] = tpx

    def size(self, cus=256):
        if isinstance(self.M, tuple):
            n_teams = team_shape(self.N, 1, cus, self.lag)["n_teams"]
            return self.M[1] * n_teams + self.M[2]
        return self.M

    def plans(self, cus=256):
        """(team shape, row-panel plan) at a CU count."""
        M = self.size(cus)
        return team_shape(self.N, M, cus, self.lag, self.tpx or 0, self.env), panel_plan(self.N, M, cus, self.env)


def _mk(group, rows, **kw):
    """rows: (N, M, expect[, overrides]); regularisers in rotation, grav_fix in every second case."""
    out = []
    for k, row in enumerate(rows):
        N, M, expect = row[:3]
        extra = dict(kw, **(row[3] if len(row) > 3 else {}))
        tag = "%s-%dx%s" % (group[0], N, M if not isinstance(M, tuple) else "%dT%+d" % M[1:])
        out.append(Spec(tag, group, N, M, extra.pop("reg", REGS[(k + len(group)) % 4]), k % 2 == 1, expect=expect, **extra))
    return out


# the members of a team: Q = 2 .. 8, the refusal at 9 (lag 2, 8 teams)
MEMBERS = _mk("members", [
    (16385, 37, {"Q": 2, "panel_rows": 8208, "last_rows": 8192, "fifth_slot": [8, 0], "runs": [5] * 7 + [2]}),
    (20416, 15, {"Q": 2, "panel_rows": 10208, "last_rows": 10208, "fifth_slot": [1008, 1008]}),
    (20417, 23, {"Q": 3, "panel_rows": 6816, "last_rows": 6800}),
    (30624, 8, {"Q": 3, "panel_rows": 10208, "last_rows": 10208, "runs": [1] * 8}),
    (30625, 29, {"Q": 4, "panel_rows": 7664, "last_rows": 7648}),
    (40833, 37, {"Q": 5, "panel_rows": 8176, "last_rows": 8144}),
    (51041, 5, {"Q": 6, "panel_rows": 8512, "last_rows": 8496, "runs": [1] * 5 + [0] * 3}),
    (61249, 49, {"Q": 7, "panel_rows": 8752, "last_rows": 8752, "runs": [7] * 7 + [0]}),
    (81664, 41, {"Q": 8, "panel_rows": 10208, "last_rows": 10208, "runs": [6] * 6 + [5, 0], "grid": 64}),
    # (one valid row in the last 16-row line of 81680: at 1e-4 it moves the oracle by 1.5e-8, 72 x the bound -- delta raised)
    (81665, 40, {"on": False, "refusal": "Q > 8", "Q": 9, "n_panels": 8, "rows_per_panel": 10224, "last_panel_rows": 10112},
     {"delta": 1e-3}),
])

# one column of lag (GRAVHMC_TEAM_LAG=1): 10240 rows per member, every thread live in all five slots
LAG1 = _mk("lag1", [
    (20480, 15, {"Q": 2, "panel_rows": 10240, "last_rows": 10240, "fifth_slot": [1024, 1024]}),
    (20481, 23, {"Q": 3, "panel_rows": 6832}),
    (16385, 8, {"runs": [1] * 8}),
    (16385, 15, {"runs": [2] * 7 + [1]}),
    (16385, 23, {"runs": [3] * 7 + [2]}),
    (16385, 29, {"runs": [4] * 7 + [1]}),
], lag=1)

# the column runs of the 8 teams at N = 16385: the rotation's prologue alone, one turn, a turn plus one and plus two,
# and the tail's parked column after each of them
RUNS = _mk("runs", [
    (16385, 1, {"runs": [1] + [0] * 7}),
    (16385, 5, {"runs": [1] * 5 + [0] * 3}),
    (16385, 8, {"runs": [1] * 8}),
    (16385, 9, {"runs": [2] * 4 + [1] + [0] * 3}),
    (16385, 16, {"runs": [2] * 8}),
    (16385, 23, {"runs": [3] * 7 + [2]}),
    (16385, 24, {"runs": [3] * 8}),
    (16385, 29, {"runs": [4] * 7 + [1]}),
    (16385, 37, {"runs": [5] * 7 + [2]}),
    (16385, 49, {"runs": [7] * 7 + [0]}),
    (16385, 57, {"runs": [8] * 7 + [1]}),
])

# the device's own team count (no cap): every team's run from the CU count
GRID = _mk("grid", [
    (16385, ("grid", 5, -3), {"Q": 2}),
    (30625, ("grid", 3, 1), {"Q": 4}),
], tpx=None)

# row panels (GRAVHMC_TEAM=0): adjoint-only panels with SW_GACC, vec_update_kernel, forward-only panels
PANELS = _mk("panels", [
    (16385, 40, {"n_panels": 2, "rows_per_panel": 8208, "last_panel_rows": 8192, "ept2": 5, "pf": 2}),
    (20480, 40, {"n_panels": 2, "rows_per_panel": 10240, "last_panel_rows": 10240, "ept2": 5, "pf": 2}),
    (20481, 40, {"n_panels": 3, "rows_per_panel": 6832, "last_panel_rows": 6832, "ept2": 4, "pf": 1}),
    (30721, 40, {"n_panels": 4, "rows_per_panel": 7696, "last_panel_rows": 7648, "ept2": 4, "pf": 1}),
    # (a single cell; the generator's first stream leaves it on the lower bound after every trajectory: the next one)
    (16385, 1, {"n_panels": 2, "update_blocks": 1}, {"reg": D, "seed": 1}),
    (81665, 40, {"n_panels": 8, "rows_per_panel": 10224, "last_panel_rows": 10112, "ept2": 5}, {"delta": 1e-3}),
    (16385, 257, {"n_panels": 2, "update_blocks": 2}),
    (16385, 300, {"n_panels": 2}, {"env": {"GRAVHMC_MIN_COLS": 4}}),
], team=False)

CASES = MEMBERS + LAG1 + RUNS + GRID + PANELS
BY_ID = dict((s.id, s) for s in CASES)
FORCED_L = {0: 1}


# ----------------------------------------------------------------------------- inputs and oracle trajectories

class Ref(object):
    """What the oracle's chain did: decisions (1, T), out5 (1, T, 5), the states after every trajectory (1, T, M) and
    their synthetic data (1, T, N)."""

    def __init__(self, C, T, M, N):
        self.acc = np.zeros((C, T), dtype=bool)
        self.out5 = np.zeros((C, T, 5))
        self.xs = np.zeros((C, T, M))
        self.dsyn = np.zeros((C, T, N))


def _problem(orc, data, A, dobs=None, gfix=None):
    Aw, wm = orc.col_weight(A, 0.5)
    dobs = data.dobs if dobs is None else dobs
    gfix = data.gfix if gfix is None else gfix
    P = orc.Problem(Aw, dobs, 0.001 * wm, data.reg, data.alpha, data.beta, wm=wm, shape=data.shape, grav_fix=gfix)
    return P, wm


def replay(P, data):
    """The case's trajectories (its L, p0, u) on the problem P: a Ref."""
    ref = Ref(data.C, data.T, data.M, data.N)
    for c in range(data.C):
        x = data.x0s[c]
        for t in range(data.T):
            x, acc, o, ds = P.leapfrog(x, data.p0s[c, t], data.dt, int(data.Ls[c, t]), data.low, data.high, float(data.us[c, t]))
            ref.acc[c, t], ref.out5[c, t], ref.xs[c, t], ref.dsyn[c, t] = acc, o, x, ds
    return ref


def before(data, ref, c, t):
    return data.x0s[c] if t == 0 else ref.xs[c, t - 1]


def distance(data, ref, other):
    """The largest difference between two results in the quantities the device test compares: decisions, out5, x after
    every trajectory and the displacement of every accepted one, each in relmax."""
    if not np.array_equal(ref.acc, other.acc):
        return np.inf
    worst = 0.0
    for c in range(data.C):
        for t in range(data.T):
            x0 = before(data, ref, c, t)
            worst = max(worst, relmax(other.out5[c, t], ref.out5[c, t]), relmax(other.xs[c, t], ref.xs[c, t]))
            if ref.acc[c, t]:
                worst = max(worst, relmax(other.xs[c, t] - x0, ref.xs[c, t] - x0))
    return worst


class Data(object):
    """Inputs of one case at one CU count and the oracle's trajectories."""

    def __init__(self, orc, spec, cus):
        self.spec, self.cus, self.orc = spec, cus, orc
        N, M, T = spec.N, spec.size(cus), spec.T
        self.N, self.M, self.C, self.T, self.reg = N, M, 1, T, spec.reg
        self.shape = shape3(M)
        # (the matrix depends on the shape alone: the cases on one shape share it)
        rng = np.random.default_rng(N * 100003 + M)
        self.A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.1, 3.0, size=M))
        self.dobs = rng.normal(size=N) + 1e3
        gfix = rng.normal(size=N) * 5 + 40.0
        self.gfix = gfix if spec.fix else None
        self.alpha = 0.05 / N if spec.reg == "MS" else 0.5
        self.beta = 0.01
        self.P, self.wm = _problem(orc, self, self.A)
        self.Aw = self.P.Aw
        self._generate(np.random.default_rng(spec.seed))
        self._spread = None

    def _generate(self, rng):
        P, spec, M, N, T = self.P, self.spec, self.M, self.N, self.T
        xc = rng.uniform(0.3, 0.7, size=M)
        self.dt = dt = stable_dt(P, xc, rng)
        self.low, self.high = xc - 1.5 * dt, xc + 1.5 * dt
        self.x0s = xc + dt * rng.uniform(-1.0, 1.0, size=(1, M))
        self.x_probe = xc + dt * rng.uniform(-1.0, 1.0, size=M)        # forward / misfit_and_grad at a random model
        self.r_probe = rng.normal(size=N)                               # adjoint of a random residual
        self.Ls = np.zeros((1, T), dtype=np.int32)
        self.p0s = np.zeros((1, T, M))
        self.us = np.zeros((1, T))
        self.ref = ref = Ref(1, T, M, N)
        on_low = on_high = 0
        x = self.x0s[0]
        for t in range(T):
            want = t % 2 == 0
            for attempt in range(200):
                L = FORCED_L.get(t, int(rng.integers(1, 7)))
                scale = 0.7 ** (attempt % 20) if want else 2.0 + 0.5 * (attempt % 20)
                p0 = rng.normal(size=M) * scale
                xn, _, o, _ = P.leapfrog(x, p0, dt, L, self.low, self.high, 0.0)
                dH = o[4] - o[3]
                if not want and dH > 0.01:
                    break
                # an accepted state: while no accepted state has had a cell on a bound, it must bring one (a single
                # cell: one bound at a time)
                lo = on_low > 0 or bool((xn == self.low).any())
                hi = on_high > 0 or bool((xn == self.high).any())
                if M == 1 and on_low == 0 and on_high == 0:
                    lo = hi = lo or hi
                if want and dH < 5.0 and ((lo and hi) or attempt >= 150):
                    break
            else:
                raise AssertionError("%s: no trajectory for the decision %r" % (spec.id, want))
            u = metropolis_u(dH, want)
            xn, acc, o, ds = P.leapfrog(x, p0, dt, L, self.low, self.high, u)
            assert acc == want
            if acc:
                on_low += int((xn == self.low).sum())
                on_high += int((xn == self.high).sum())
            self.Ls[0, t], self.p0s[0, t], self.us[0, t] = L, p0, u
            ref.acc[0, t], ref.out5[0, t], ref.xs[0, t], ref.dsyn[0, t] = acc, o, xn, ds
            x = xn
        self.on_bounds = (on_low, on_high)
        self.check()

    def check(self):
        """The generator's own conditions."""
        ref, s = self.ref, self.spec
        half = self.T // 2
        assert ref.acc.sum() == self.T - half and (~ref.acc).sum() == half and half >= 2, s.id
        assert self.Ls[0, 0] == 1 and self.Ls.min() >= 1 and self.Ls.max() <= 6, s.id
        assert (ref.acc[0] & (self.Ls[0] >= 2)).any(), s.id         # (fused steps whose proposal is kept)
        assert self.on_bounds[0] > 0 and self.on_bounds[1] > 0, (s.id, self.on_bounds)
        # (a single cell that ends every trajectory on a bound shows nothing of the matrix in its states)
        assert any(ref.acc[0, t] and ((ref.xs[0, t] > self.low) & (ref.xs[0, t] < self.high)).any() for t in range(self.T)), s.id
        for t in range(self.T):
            if not ref.acc[0, t]:
                assert np.array_equal(ref.xs[0, t], before(self, ref, 0, t))

    def spread(self):
        """The oracle against itself with the observation rows reversed (every sum over the observations in another
        order), on this case's trajectories."""
        if self._spread is None:
            gf = None if self.gfix is None else self.gfix[::-1].copy()
            P = _problem(self.orc, self, np.asfortranarray(self.A[::-1]), self.dobs[::-1].copy(), gf)[0]
            other = replay(P, self)
            other.dsyn = other.dsyn[:, :, ::-1]
            self._spread = distance(self, self.ref, other)
        return self._spread

    def bound(self):
        return max(TOL_TRAJ, 10.0 * self.spread())

    def layout(self):
        """The rows of the members (team cases) or of the panels the case's kernels cut the observations into, and the
        column runs of its teams."""
        ts, pp = self.spec.plans(self.cus)
        if ts["on"]:
            d = derived(ts, self.M)
            return ts["panel_rows"], ts["Q"], d["runs"]
        cpt, n = pp["panel_cols"], pp["panel_teams"]
        return pp["rows_per_panel"], pp["n_panels"], [max(0, min(self.M, (t + 1) * cpt) - t * cpt) for t in range(n)]

    def probes(self):
        """(name, row slice, column slice) of the blocks of A the sensitivity is measured at."""
        rows, parts, runs = self.layout()
        N, M, ld = self.N, self.M, roundup16(self.N)
        last0 = (parts - 1) * rows
        part = lambda q: slice(q * rows, min(N, (q + 1) * rows))
        every = slice(0, M)
        out = [("a: the last valid 16-row line", slice(ld - 16, N), every),
               ("a: the first line of the last member or panel", slice(last0, last0 + 16), every),
               ("a: the last line of member or panel 0", slice(rows - 16, rows), every),
               ("b: member or panel 0, first column of team 0", part(0), slice(0, 1)),
               ("b: the last member or panel, last column of the last non-empty team", part(parts - 1), slice(M - 1, M))]
        cpt = max(runs)
        full = [t for t, r in enumerate(runs) if r >= 3]
        if full and self.spec.team:
            t = full[len(full) // 2]
            j = t * cpt + runs[t] - 2
            out.append(("b: a middle member, the column at cnt - 2 of team %d (finished from LDS)" % t, part(parts // 2),
                        slice(j, j + 1)))
        return out

    def perturbed(self, rows, cols, delta):
        """The oracle's results with A[rows, cols] scaled by 1 + delta (weights, mwapr and all)."""
        A = self.A.copy(order="F")
        A[rows, cols] *= 1.0 + delta
        return replay(_problem(self.orc, self, A)[0], self)


@functools.lru_cache(maxsize=3)
def _cached(cid, cus):
    from oracle import oracle
    return Data(oracle, BY_ID[cid], cus)


def make(cid, cus=256):
    """The case's Data (generated once; treat it as read-only)."""
    return _cached(cid, cus)
