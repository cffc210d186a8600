"""The cases of the resident kernels against the CPU oracle (tests/test_gpu_resident_oracle.py on the device,
tests/test_resident_oracle_host.py for the generator and the restated plans): resident_chain_kernel<RC, CW>
(csrc/resident.hip.h; single chain, chains taking turns, split and stream modes) and resident_batch_kernel<KS, NT, GREG>
(csrc/resbatch.hip.h; chains in lock-step).

The plans are restated here from (N, M, cus, lds_max, env): resident_plan / resident_usable (csrc/host_resident.h),
the fit test of gh_batch_init for C chains, resbatch_plan (csrc/host_resbatch.h), and the quantities the kernels derive
themselves (clusters, row chunks and their owners, passes of 32 rows, the last workgroup's columns).  Every case fixes its
partition with GRAVHMC_RESIDENT_WGS, so the layout a case names is reached on any device with at least that many CUs.

A case is a random Fortran-ordered matrix (column scales over 0.1 .. 3, weighted with 0.5), data with a mean 10^3 times
their spread, grav_fix in half the cases, the four regularisers in rotation (Smoothness and TV on true 3-D shapes whose
rows and planes straddle workgroup boundaries: the neighbours come from another workgroup's published model), C chains
with their own starts in one box of +-1.5 dt and T trajectories per chain with L in 1 .. 6.  Everything the device is
compared with comes from oracle.Problem.leapfrog before an engine exists.  The variate of a trajectory sits half-way
between the oracle's exp(-dH) and 0 or 1 (helpers.metropolis_u); a rejection is used only where dH > 0.01.

DELTA: the relative change of ONE entry of A that moves the oracle's results by more than 100 TOL_TRAJ (the host test
checks it at the entries Data.probes names).  One case (640 x 250 under TV) is too over-determined for 1e-4 at one of its
entries: its delta is raised in the table, as tests/batch_oracle_cases.py does."""
import functools

import numpy as np

from helpers import metropolis_u, relmax, shape3, stable_dt

TOL_TRAJ = 1e-10
DELTA = 1e-4
LDS_MAX = 163840                # bytes a workgroup may have on gfx950 (what the tables below are stated for)

# csrc/resident.hip.h, csrc/resbatch.hip.h
RES_THREADS, RES_WAVES, RES_CLUSTERS, RES_CHUNKS, RES_MAX_WG, RES_REDBUF, RES_MAX_CHAINS = 512, 8, 8, 32, 256, 16 * 33, 16
RB_WAVES = 8


def roundup16(n):
    return (n + 15) // 16 * 16


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- the plans, restated

def resident_lds_doubles(ld, cpw, chains, lds_cols, split):
    return (lds_cols * ld + (8 * ld if split else 0) + ld + RES_REDBUF + 16 + (6 + 2 * chains) * cpw
            + 3 * RES_MAX_CHAINS + 8 + 16)


def resident_stencil_fits(cpw):
    return 6 * cpw <= RES_THREADS and 12 * cpw <= RES_REDBUF


def resident_plan(N, M, cus, lds_max=LDS_MAX, env=None):
    """resident_plan for a dense stored G on one device without the compressed forward: None where it refuses, else
    cpw, nwg, rc, ct, split, stream, lds_cols and the LDS bytes of one chain."""
    env = env or {}
    geti = lambda k, d: int(env.get(k, d))
    ld = roundup16(N)
    if geti("GRAVHMC_RESIDENT", 1) == 0 or ld > 1024:
        return None
    wgs = max(1, min(cus, geti("GRAVHMC_RESIDENT_WGS", cus)))
    cpw = cdiv(M, wgs)
    if cpw > RES_THREADS:
        return None
    nwg = cdiv(M, cpw)
    if nwg > RES_MAX_WG:
        return None
    rc = (ld // 2 + 63) // 64
    regs = geti("GRAVHMC_RESIDENT_REGS", 1) != 0
    p = {"ld": ld, "cpw": cpw, "nwg": nwg, "rc": rc, "ct": 0, "split": False, "stream": False, "lds_cols": cpw}
    lds = resident_lds_doubles(ld, cpw, 1, cpw, False) * 8
    if lds <= lds_max:
        ct = cdiv(cpw, RES_WAVES) if (regs and cpw <= 4 * RES_WAVES) else 0
        p["ct"] = 0 if ct * rc > 20 else ct
    else:
        ct_max = min(4, 20 // rc)
        ct_env = geti("GRAVHMC_RESIDENT_CT", 0)
        p["split"] = True
        for ct in range(1, ct_max + 1):
            if ct_env > 0 and ct != min(ct_env, ct_max):
                continue
            lc = max(0, cpw - ct * RES_WAVES)
            lds = resident_lds_doubles(ld, cpw, 1, lc, True) * 8
            if lds <= lds_max:
                p["ct"], p["lds_cols"] = ct, lc
                break
        if not regs:
            p["ct"] = 0
        if p["ct"] < 1:
            budget = geti("GRAVHMC_RESIDENT_STREAM_MB", 320) << 20
            if geti("GRAVHMC_RESIDENT_STREAM", 1) == 0 or 2 * ld * M * 8 > budget:
                return None
            p["split"], p["stream"], p["ct"] = False, True, 0
            lc = cpw
            while lc > 0 and resident_lds_doubles(ld, cpw, 1, lc, False) * 8 > lds_max:
                lc -= 1
            p["lds_cols"] = lc
            lds = resident_lds_doubles(ld, cpw, 1, lc, False) * 8
            if lds > lds_max:
                return None
    if not 1 <= rc <= 8:
        return None
    p["lds"] = lds
    return p


def resident_usable(p, reg):
    return p is not None and (reg not in ("Smoothness", "TV") or resident_stencil_fits(p["cpw"]))


def chains_lds_bytes(p, C):
    return resident_lds_doubles(p["ld"], p["cpw"], C, p["lds_cols"], p["split"]) * 8


def chains_fit(p, reg, C, lds_max=LDS_MAX):
    """gh_batch_init: C chains take turns in the resident chain kernel (otherwise the MFMA batch takes them)."""
    return resident_usable(p, reg) and 1 <= C <= RES_MAX_CHAINS and chains_lds_bytes(p, C) <= lds_max


def rb_ldp(ld, greg=False):
    want = 16 if greg else 18
    return ld + ((want - ld % 32) + 32) % 32


def resbatch_lds_doubles(ld, cpw, have_fix, greg=False):
    cpw4 = (cpw + 3) & ~3
    return (cpw4 * rb_ldp(ld, greg) + RB_WAVES * (cpw4 // 4) * 64 + cpw4 * 16 + (2 if have_fix else 1) * ld + 128 + 128 + 384
            + 64 + 2 + 16)


def resbatch_plan(p, reg, C, have_fix, lds_max=LDS_MAX, env=None):
    """resbatch_plan's decision: None where the chains take turns, else ks, nt and the LDS bytes."""
    env = env or {}
    if int(env.get("GRAVHMC_RESIDENT_BATCH", 1)) == 0 or C < 2 or C > 16:
        return None
    if not resident_usable(p, reg) or p["split"] or p["stream"] or p["cpw"] > 32 or p["ld"] > 640 or p["ld"] % 16:
        return None
    ks = cdiv(p["ld"], 160) * 5
    nt = cdiv(p["cpw"], 16)
    lds = resbatch_lds_doubles(p["ld"], p["cpw"], have_fix) * 8
    if lds > lds_max or ks not in (5, 10, 15, 20):
        return None
    return {"ks": ks, "nt": nt, "lds": lds, "cpw4": (p["cpw"] + 3) & ~3}


def derived(p, M):
    """What the kernels derive from the plan: clusters and their sizes, row chunks, passes, the last workgroup."""
    nwg, ld, cpw = p["nwg"], p["ld"], p["cpw"]
    ncl = min(nwg, RES_CLUSTERS)
    cn = [(nwg - cg + RES_CLUSTERS - 1) // RES_CLUSTERS for cg in range(RES_CLUSTERS)]
    nch = max(1, min(RES_CHUNKS, nwg // RES_CLUSTERS))
    ch = cdiv(ld, nch)
    nc = M - (nwg - 1) * cpw
    lds_c0 = p["ct"] * RES_WAVES if p["split"] else 0
    nl = min(nc, p["lds_cols"]) if p["stream"] else max(0, nc - lds_c0)
    rows = [max(0, min(ch, ld - k * ch)) for k in range(nch)]       # rows of d owner k sums
    return {"ncl": ncl, "cn": cn, "nch": nch, "ch": ch, "passes": cdiv(ch, 32), "last_nc": nc, "last_nl": nl,
            "lds_c0": lds_c0, "chunk_rows": rows, "empty_chunks": sum(1 for r in rows if r == 0),
            "last_chunk": max(k for k in range(nch) if rows[k] > 0)}


# ----------------------------------------------------------------------------- the case tables

class Spec(object):
    """expect: the figures the table names for the case (plan keys, or derived keys), at 256 CUs and LDS_MAX."""

    def __init__(self, cid, group, N, M, wgs, reg, fix, shape=None, C=1, T=12, expect=None, env=None, delta=DELTA,
                 lockstep=None):
        self.id, self.group, self.N, self.M, self.wgs, self.reg, self.fix = cid, group, N, M, wgs, reg, fix
        self.shape = shape or shape3(M)
        assert self.shape[0] * self.shape[1] * self.shape[2] == M
        self.C, self.T, self.expect, self.delta, self.lockstep = C, T, expect or {}, delta, lockstep
        self.env = dict(env or {}, GRAVHMC_RESIDENT_WGS=wgs)

    def plan(self, cus=256, lds_max=LDS_MAX, env=None):
        e = dict(self.env)
        e.update(env or {})
        return resident_plan(self.N, self.M, cus, lds_max, e)


S, D, MS, TV = "Smoothness", "Damping", "MS", "TV"

# resident_chain_kernel, one chain.  (The figures: `expect` below, asserted by the host test at 256 and 304 CUs.)
TOPOLOGY = [
    Spec("x-1x1", "topology", 1, 1, 1, D, False, expect={"nwg": 1, "ncl": 1, "cpw": 1}),
    Spec("x-2x7", "topology", 2, 7, 7, MS, True, expect={"nwg": 7, "ncl": 7, "cpw": 1, "cn": [1] * 7 + [0]}),
    Spec("x-16x9", "topology", 16, 9, 8, S, False, shape=(1, 3, 3), expect={"cpw": 2, "nwg": 5, "last_nc": 1}),
    Spec("x-33x70", "topology", 33, 70, 12, TV, True, shape=(2, 5, 7),
         expect={"cpw": 6, "nwg": 12, "cn": [2, 2, 2, 2, 1, 1, 1, 1], "nch": 1, "ch": 48, "passes": 2}),
    Spec("x-127x37", "topology", 127, 37, 16, D, True,
         expect={"cpw": 3, "nwg": 13, "nch": 1, "ch": 128, "passes": 4}),
    Spec("x-128x64", "topology", 128, 64, 64, MS, False, expect={"cpw": 1, "nwg": 64, "nch": 8, "ch": 16}),
    Spec("x-129x130", "topology", 129, 130, 130, S, True, shape=(2, 5, 13),
         expect={"ld": 144, "nwg": 130, "cn": [17, 17, 16, 16, 16, 16, 16, 16], "nch": 16, "ch": 9}),
    Spec("x-130x137", "topology", 130, 137, 137, D, False, expect={"ld": 144, "nwg": 137, "nch": 17, "ch": 9, "empty_chunks": 1}),
    Spec("x-384x255", "topology", 384, 255, 255, TV, False, shape=(3, 5, 17),
         expect={"nwg": 255, "nch": 31, "ch": 13, "cn": [32] * 7 + [31], "empty_chunks": 1}),
    Spec("x-250x256", "topology", 250, 256, 256, MS, True, expect={"nwg": 256, "cn": [32] * 8, "nch": 32, "ch": 8}),
    Spec("x-16x2047", "topology", 16, 2047, 256, S, True, shape=(23, 1, 89),
         expect={"cpw": 8, "nwg": 256, "last_nc": 7, "nch": 32, "ch": 1, "empty_chunks": 16}),
]

ROWS = [
    Spec("r-385x200", "rows", 385, 200, 24, TV, False, shape=(2, 4, 25),
         expect={"ld": 400, "rc": 4, "ct": 2, "cpw": 9, "nwg": 23, "last_nc": 2, "nch": 2}),
    Spec("r-511x96", "rows", 511, 96, 24, D, True, expect={"rc": 4, "ct": 1, "cpw": 4, "nwg": 24}),
    Spec("r-513x104", "rows", 513, 104, 8, S, False, shape=(2, 4, 13),
         expect={"rc": 5, "ct": 2, "cpw": 13, "nwg": 8}),
    Spec("r-600x384", "rows", 600, 384, 16, MS, True, expect={"ld": 608, "rc": 5, "ct": 3, "cpw": 24, "nwg": 16}),
    # (640 rows over 250 columns under TV: column 8 of a workgroup moves the oracle by 7.0e-9 at 1e-4 -- delta raised)
    Spec("r-640x250", "rows", 640, 250, 10, TV, True, shape=(2, 5, 25), delta=1e-3, expect={"rc": 5, "ct": 4, "cpw": 25, "nwg": 10}),
    Spec("r-768x40", "rows", 768, 40, 8, D, False, expect={"rc": 6, "ct": 1, "cpw": 5, "nwg": 8}),
    Spec("r-800x72", "rows", 800, 72, 8, S, True, shape=(2, 4, 9), expect={"rc": 7, "ct": 2, "cpw": 9, "nwg": 8}),
    Spec("r-897x33", "rows", 897, 33, 8, MS, False,
         expect={"ld": 912, "rc": 8, "ct": 1, "cpw": 5, "nwg": 7, "last_nc": 3}),
    Spec("r-256x330", "rows", 256, 330, 10, TV, False, shape=(2, 3, 55), expect={"cpw": 33, "ct": 0, "split": False, "stream": False}),
    Spec("r-1000x136", "rows", 1000, 136, 8, D, True, expect={"rc": 8, "cpw": 17, "ct": 0, "split": False, "stream": False}),
]

SPLIT = [
    Spec("s-641x330", "split", 641, 330, 10, TV, True, shape=(2, 3, 55),
         expect={"split": True, "ct": 2, "cpw": 33, "lds_cols": 17}),
    Spec("s-700x290", "split", 700, 290, 8, MS, False, expect={"split": True, "ct": 3, "cpw": 37, "lds_cols": 13, "last_nc": 31, "last_nl": 7}),
    Spec("s-1023x160", "split", 1023, 160, 8, S, False, shape=(2, 4, 20),
         expect={"split": True, "rc": 8, "ct": 2, "cpw": 20, "lds_cols": 4}),
    Spec("s-1023x145", "split", 1023, 145, 8, D, True,
         expect={"split": True, "rc": 8, "ct": 2, "cpw": 19, "last_nc": 12, "last_nl": 0}),
]

STREAM = [
    Spec("m-1024x203", "stream", 1024, 203, 7, MS, True, expect={"stream": True, "cpw": 29, "lds_cols": 18, "ct": 0}),
    Spec("m-1000x300", "stream", 1000, 300, 8, TV, False, shape=(2, 3, 50),
         expect={"stream": True, "cpw": 38, "lds_cols": 18, "last_nc": 34}),
    Spec("m-1024x305", "stream", 1024, 305, 16, D, False, env={"GRAVHMC_RESIDENT_REGS": 0},
         expect={"stream": True, "cpw": 20, "last_nc": 5, "last_nl": 5}),
    Spec("m-1024x1737", "stream", 1024, 1737, 64, S, True, shape=(3, 3, 193), expect={"stream": True, "cpw": 28, "nwg": 63, "last_nc": 1}),
]

SINGLE = TOPOLOGY + ROWS + SPLIT + STREAM

# chains taking turns in resident_chain_kernel (GRAVHMC_RESIDENT_BATCH=0): the same matrices with C chains
TURNS = [Spec("t-%s-c%d" % (b.id, C), "turns", b.N, b.M, b.wgs, b.reg, b.fix, shape=b.shape, C=C, T=5, env=b.env, delta=None)
         for b in (TOPOLOGY[3], ROWS[0], SPLIT[0], STREAM[1]) for C in (2, 5, 16)]
# 1024 x 203 on 7 workgroups: four chains fit the LDS, five do not (the MFMA batch takes them)
FIT = [Spec("f-1024x203-c4", "fit", 1024, 203, 7, MS, True, C=4, T=5, delta=None),
       Spec("f-1024x203-c5", "fit", 1024, 203, 7, MS, True, C=5, T=5, delta=None)]

# resident_batch_kernel (GRAVHMC_RESIDENT_BATCH=1).  lockstep: {ks, nt} the case reaches, False: resbatch_plan refuses
# and the chains take turns.
LOCKSTEP = [
    Spec("l-16x8", "lockstep", 16, 8, 8, D, False, C=2, T=6, lockstep={"ks": 5, "nt": 1, "cpw4": 4}, expect={"cpw": 1, "nwg": 8}),
    Spec("l-33x9", "lockstep", 33, 9, 8, S, True, shape=(1, 3, 3), C=3, T=6, lockstep={"ks": 5, "nt": 1},
         expect={"cpw": 2, "nwg": 5, "last_nc": 1}),
    Spec("l-150x24", "lockstep", 150, 24, 8, TV, False, shape=(2, 3, 4), C=16, T=6, lockstep={"ks": 5, "nt": 1},
         expect={"ld": 160, "cpw": 3}),
    Spec("l-161x136", "lockstep", 161, 136, 8, MS, True, C=5, T=6, lockstep={"ks": 10, "nt": 2}, expect={"cpw": 17}),
    Spec("l-320x128", "lockstep", 320, 128, 8, S, False, shape=(2, 8, 8), C=15, T=6, lockstep={"ks": 10, "nt": 1}, expect={"cpw": 16}),
    Spec("l-321x130", "lockstep", 321, 130, 8, TV, True, shape=(2, 5, 13), C=16, T=6, lockstep={"ks": 15, "nt": 2},
         expect={"cpw": 17, "last_nc": 11}),
    Spec("l-430x256", "lockstep", 430, 256, 8, D, True, C=4, T=6, lockstep={"ks": 15, "nt": 2}, expect={"cpw": 32, "ld": 432}),
    Spec("l-481x160", "lockstep", 481, 160, 8, MS, False, C=16, T=6, lockstep={"ks": 20, "nt": 2}, expect={"cpw": 20}),
    Spec("l-640x160", "lockstep", 640, 160, 8, S, True, shape=(5, 4, 8), C=7, T=6, lockstep={"ks": 20, "nt": 2},
         expect={"ld": 640, "cpw": 20}),
    Spec("l-625x250", "lockstep", 625, 250, 250, TV, False, shape=(2, 5, 25), C=16, T=6, lockstep={"ks": 20, "nt": 1},
         expect={"cpw": 1, "nwg": 250, "nch": 31, "cn": [32, 32] + [31] * 6}),
    Spec("l-100x137", "lockstep", 100, 137, 137, D, False, C=2, T=6, lockstep={"ks": 5, "nt": 1}, expect={"nwg": 137, "nch": 17}),
    Spec("l-641x80", "lockstep", 641, 80, 8, MS, True, C=3, T=6, lockstep=False, expect={"ld": 656}),
    Spec("l-256x330", "lockstep", 256, 330, 10, S, False, shape=(6, 5, 11), C=3, T=6, lockstep=False, expect={"cpw": 33}),
    Spec("l-640x200", "lockstep", 640, 200, 8, TV, True, shape=(2, 4, 25), C=3, T=6, lockstep=False, expect={"cpw": 25, "ld": 640}),
]

CASES = SINGLE + TURNS + FIT + LOCKSTEP
BY_ID = dict((s.id, s) for s in CASES)

# the launches a single chain's 12 trajectories are cut into (run_chain(batch=...) per piece): tags continue over five
# launches, the second holds ONE trajectory of L = 2 -- with the evaluation at its start an odd number, so the parity
# buffers restart at 0 while the tag runs on -- and the chain's first trajectory has L = 1
CUTS = (3, 1, 4, 2, 2)
FORCED_L = {0: 1, 3: 2}
STOP_AT = 2                      # second pass: one launch of all 12 with stop_at_accepts (ends mid-batch)


# ----------------------------------------------------------------------------- inputs and oracle trajectories

class Ref(object):
    """What the oracle's chains did: decisions (C, T), out5 (C, T, 5), the states after every trajectory (C, T, M) and
    their synthetic data (C, T, N)."""

    def __init__(self, C, T, M, N):
        self.acc = np.zeros((C, T), dtype=bool)
        self.out5 = np.zeros((C, T, 5))
        self.xs = np.zeros((C, T, M))
        self.dsyn = np.zeros((C, T, N))


def _problem(orc, data, A):
    Aw, wm = orc.col_weight(A, 0.5)
    P = orc.Problem(Aw, data.dobs, 0.001 * wm, data.reg, data.alpha, data.beta, wm=wm, shape=data.shape, grav_fix=data.gfix)
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
    """The largest difference between two results in the quantities the device test compares: decisions, out5, x and the
    displacement of every trajectory, each in relmax."""
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
    """Inputs of one case and the oracle's trajectories."""

    def __init__(self, orc, spec):
        self.spec = spec
        N, M, C, T = spec.N, spec.M, spec.C, spec.T
        self.N, self.M, self.C, self.T, self.shape, self.reg = N, M, C, T, spec.shape, spec.reg
        # (the matrix depends on the shape alone: the cases on one shape share it)
        rng = np.random.default_rng(N * 100003 + M)
        self.A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.1, 3.0, size=M))
        self.dobs = rng.normal(size=N) + 1e3
        gfix = rng.normal(size=N) * 5 + 40.0
        self.gfix = gfix if spec.fix else None
        self.alpha = 0.05 / N if spec.reg == "MS" else 0.5
        self.beta = 0.01
        self.P, self.wm = _problem(orc, self, self.A)
        self._generate(np.random.default_rng(sum(map(ord, spec.id)) * 7919 + N))

    def _generate(self, rng):
        """Starts, box and trajectories of the C chains on self.P."""
        P, spec, M, N, C, T = self.P, self.spec, self.M, self.N, self.C, self.T
        xc = rng.uniform(0.3, 0.7, size=M)
        self.dt = dt = stable_dt(P, xc, rng)
        self.low, self.high = xc - 1.5 * dt, xc + 1.5 * dt
        self.x0s = xc + dt * rng.uniform(-1.0, 1.0, size=(C, M))
        self.Ls = np.zeros((C, T), dtype=np.int32)
        self.p0s = np.zeros((C, T, M))
        self.us = np.zeros((C, T))
        self.ref = ref = Ref(C, T, M, N)
        on_low = on_high = 0
        for c in range(C):
            x = self.x0s[c]
            for t in range(T):
                want = (c + t) % 2 == 0
                for attempt in range(200):
                    L = int(rng.integers(1, 7))
                    if C == 1:
                        L = FORCED_L.get(t, L)
                    elif (c, t) == (0, 1):
                        L = 1
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
                self.Ls[c, t], self.p0s[c, t], self.us[c, t] = L, p0, u
                ref.acc[c, t], ref.out5[c, t], ref.xs[c, t], ref.dsyn[c, t] = acc, o, xn, ds
                x = xn
        self.on_bounds = (on_low, on_high)
        self.check()

    def check(self):
        """The generator's own conditions."""
        ref, s = self.ref, self.spec
        assert ref.acc.sum() >= 3 and (~ref.acc).sum() >= 3, s.id
        assert self.C * self.T >= 10 and (self.Ls == 1).any() and self.Ls.min() >= 1 and self.Ls.max() <= 6, s.id
        assert self.on_bounds[0] > 0 and self.on_bounds[1] > 0, (s.id, self.on_bounds)
        for c in range(self.C):
            for t in range(self.T):
                if not ref.acc[c, t]:
                    assert np.array_equal(ref.xs[c, t], before(self, ref, c, t))
        if self.C == 1:
            assert sum(CUTS) == self.T and 1 in CUTS and len(CUTS) >= 3
            ev = self.launch_evaluations()
            assert any(e % 2 == 1 for e in ev[:-1]), (s.id, ev)
            # the second pass ends mid-batch
            assert 0 < self.stop_index() < self.T - 1, s.id

    def launches(self):
        """Single chain: the (first, end) trajectory ranges of the launches."""
        out, k = [], 0
        for n in CUTS:
            out.append((k, k + n))
            k += n
        return out

    def launch_evaluations(self):
        """Evaluations per launch of a single chain: one at the start (the state is not kept between launches) and one
        per leapfrog step."""
        return [1 + int(self.Ls[0, a:b].sum()) for a, b in self.launches()]

    def stop_index(self):
        """The trajectory whose acceptance is the STOP_AT-th: the last one a launch with stop_at_accepts runs."""
        return int(np.nonzero(np.cumsum(self.ref.acc[0]) == STOP_AT)[0][0])

    def probes(self, cus=256):
        """The entries of A the sensitivity is measured at, named."""
        p = self.spec.plan(cus)
        d = derived(p, self.M)
        cpw, nwg = p["cpw"], p["nwg"]
        out = [("last valid row, last column", (self.N - 1, self.M - 1)),
               ("first row of the last non-empty chunk, first column of the last workgroup",
                (min(d["last_chunk"] * d["ch"], self.N - 1), (nwg - 1) * cpw))]
        mid = (nwg // 2) * cpw
        if p["split"]:
            out += [("last register-held column of a middle workgroup", (self.N // 2, mid + d["lds_c0"] - 1)),
                    ("first LDS column of a middle workgroup", (self.N // 2, mid + d["lds_c0"]))]
        if p["stream"]:
            out += [("last LDS column", (self.N // 2, mid + p["lds_cols"] - 1)),
                    ("first streamed column", (self.N // 2, mid + p["lds_cols"])),
                    ("last streamed column", (self.N // 2, mid + cpw - 1))]
        if cpw > 8:
            out.append(("column 8 of a workgroup", (self.N // 3, mid + 8)))
        return out

    def perturbed(self, orc, entry, delta):
        """The oracle's results with A[entry] scaled by 1 + delta (weights, mwapr and all)."""
        A = self.A.copy(order="F")
        A[entry] *= 1.0 + delta
        return replay(_problem(orc, self, A)[0], self)


# ----------------------------------------------------------------------------- the compressed forward

class _CompressedSpec(object):
    def __init__(self, dims, C):
        self.id, self.dims, self.C, self.T = "w-%dD-c%d" % (dims, C), dims, C, (12 if C == 1 else 6)
        self.reg, self.fix, self.delta = "TV", False, None


class Compressed(Data):
    """tests/golden/potential_small.npz (42 x 120, shape (4, 6, 5)) with the wavelet-compressed forward under TV, as
    tests/test_gpu_parity.py builds BASELINE configs[2]: the forward is csr(DWT rows of Aw, thresholded) . DWT(x), the
    adjoint the exact dense Aw.  On the device LDS holds F = csr . W as a dense matrix and the dots read Aw from the
    register copy, so the association of the forward's sums is neither the oracle's DWT-then-SpMV nor a dense F applied
    row by row.  spread(): the distance between those two host forms on this case's trajectories; the device is held to
    bound() = max(TOL_TRAJ, 10 x spread)."""

    def __init__(self, orc, dims, C, Aw, wm, dobs, shape):
        from oracle import wavelet as ow
        self.spec = _CompressedSpec(dims, C)
        self.N, self.M = Aw.shape
        self.C, self.T, self.shape, self.reg = C, self.spec.T, tuple(int(s) for s in shape), "TV"
        self.dims, self.wm, self.dobs, self.gfix, self.alpha, self.beta = dims, wm, dobs, None, 1.0, 0.001
        self.mwapr = 0.001 * wm
        self.csr = ow.compress_kernel(Aw, dims, self.shape)
        dwt = lambda v: ow.model_coeffs(v, dims, self.shape)
        self.P = orc.Problem(Aw, dobs, self.mwapr, "TV", self.alpha, self.beta, wm=wm, shape=self.shape, csr=self.csr, dwt=dwt)
        # the same operator as ONE dense float64 matrix applied row by row: F = csr . W, W's columns the DWT of unit vectors
        from scipy.sparse import csr_matrix
        W = np.stack([dwt(e) for e in np.eye(self.M)], axis=1)
        self.F = np.asarray(self.csr @ W)
        N, M = self.N, self.M                                           # (every entry stored: a dense row product)
        full = csr_matrix((self.F.ravel(), np.tile(np.arange(M), N), np.arange(0, N * M + 1, M)), shape=(N, M))
        self.P_dense = orc.Problem(Aw, dobs, self.mwapr, "TV", self.alpha, self.beta, wm=wm, shape=self.shape, csr=full,
                                   dwt=lambda v: v)
        self._generate(np.random.default_rng(4242 + 10 * dims + C))

    def spread(self):
        return distance(self, self.ref, replay(self.P_dense, self))

    def bound(self):
        return max(TOL_TRAJ, 10.0 * self.spread())


def compressed(dims, C, Aw=None, wm=None):
    """The compressed-forward case; Aw, wm: the device's own kernel and weights (default: the golden file's)."""
    import os
    from oracle import oracle
    p = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "potential_small.npz"))
    return Compressed(oracle, dims, C, p["Aw"] if Aw is None else Aw, p["wm"] if wm is None else wm, p["dobs"], p["shape"])


@functools.lru_cache(maxsize=4)
def _cached(cid):
    from oracle import oracle
    return Data(oracle, BY_ID[cid])


def make(cid):
    """The case's Data (generated once; treat it as read-only)."""
    return _cached(cid)
