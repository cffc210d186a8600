"""The cases of the shift-invariant tesseroid store against the CPU oracle (tests/test_gpu_lonsym_oracle.py on the device,
tests/test_lonsym_oracle_host.py for the generator, the restated plans and how sharp each case is): the direct
correlations (csrc/lonsym.hip.h), the register form and its launches per phase (lonsymh.hip.h), the streamed form
(lonsymw.hip.h) and the persistent launch (lonres.hip.h), planned by csrc/host_lonsym.h and host_lonres.h.

The plans are restated here from (n, na, nc, the rows' and classes' geometry, the slots, cus, env): lonsym_build's choice
of the form, the direct form's work items and its four refusals, rp / rw / hgrid of the register form (a workgroup w works
on the rows w + r hgrid, r < rw, and loops where hgrid rw < nc), the streamed form's pitch, pairs per thread, mirror items
and parts, lonres_plan, and what lonsymh_resident_kernel derives itself (clusters, their chunks of the E = na nf entries,
the classes' owners).  GRAVHMC_LONSYM_ROWS fixes the rows per workgroup, so the layout a case names is reached on any
device with at least as many CUs as the case has workgroups.

A case is a band of tesseroid rows -- ny latitude rows x nz layers of n cells on a linspace of the full circle -- under
observation classes (latitude, height) on the cells' longitudes.  `slots` says how many observations every (class,
longitude) slot holds: "ones", "dup" (the first longitude twice, once as lon + 360), "multi" (slots of 2 and 3 spread over
the classes), "x3" (one slot of 4: three beyond its first), "empty" (a third of the last class's slots hold nothing),
"single" (the first class is ONE observation).  The full dense K, its weights, data with a mean 10^3 times their spread,
grav_fix in about half the cases, shuffled observation order in some, the four regularisers in rotation (TV and Smoothness
where a workgroup boundary is the point), 12 trajectories with L in 1 .. 6 from oracle.Problem.leapfrog: everything comes
from the oracle before an engine exists (the generator is tests/resident_oracle_cases.py's).

K_sym: K as the store holds it, K[(a, m), (c, k)] := T[a][(m - k) mod n][c] with T the oracle's entries of every class
at every shift against the cells of longitude index 0 (and, in the mirror cases, the mirrored row's entries taken from its
partner).  The oracle on K_sym and on K must agree to TOL_TRAJ / 10 (the host test), or the bound would measure the
oracle's own spread.  DELTA: the relative change of one table entry's worth of K -- every K[i, (c, k)] with one (c, a,
shift) -- that moves the oracle by more than 100 TOL_TRAJ at the entries Data.probes names."""
import functools

import numpy as np

import resident_oracle_cases as rc
from helpers import relmax  # noqa: F401  (re-exported for the two test files)
from resident_oracle_cases import CUTS, STOP_AT, Ref, before, cdiv, distance, replay  # noqa: F401

TOL_TRAJ = rc.TOL_TRAJ
TOL_WEIGHT = 1e-11
DELTA = 1e-4
LDS_MAX = 163840

# csrc/lonsym.hip.h, lonsymh.hip.h, lonsymw.hip.h, lonres.hip.h
LS_THREADS, LS_WAVES, LS_MAXITEMS = 1024, 16, 4
LH_THREADS, LH_AK = 256, 16
LW_THREADS, LW_NMAX = 256, 1024
LR_MAXWG, RES_CLUSTERS = 256, 8
DIRECT_WHY = (None,
              "more than 1024 longitudes per cell row",
              "too many (class, longitude block) work items for one workgroup",
              "a cell row's table and the residual grid do not fit the LDS",
              "a cell row's table has more than 8192 entries")


# ----------------------------------------------------------------------------- the plans, restated

def lonsymh_lds_doubles(n, nf, na, rw):
    return 2 * na * nf + 2 * n + rw * (8 * nf + 2 * nf + n + 8 * nf) + 16


def lonsymw_lds_doubles(n, nf):
    return 2 * n + 16 * nf + 4 * nf + 2 * nf + 16


def lonres_lds_doubles(n, nf, na, rw):
    return lonsymh_lds_doubles(n, nf, na, rw) + 2 * rw + 2 * 64 + 128 + 8 * 64 + 2 * 64 + 3 * LR_MAXWG + 64


def _near(x, y):
    return abs(x - y) <= 1e-9 * max(1.0, abs(x), abs(y))


def mirror_items(rows, classes):
    """lonsym_build's north-south pairing: None where a class or a row has no partner, else (item_c, item_c2, amir)."""
    na, nc = len(classes), len(rows)
    amir = [-1] * na
    for a in range(na):
        for b in range(na):
            if _near(classes[b][0], -classes[a][0]) and _near(classes[b][1], classes[a][1]):
                amir[a] = b
                break
        if amir[a] < 0:
            return None
    if any(amir[amir[a]] != a for a in range(na)):
        return None
    rmir = [-1] * nc
    for c in range(nc):
        q = rows[c]
        for c2 in range(nc):
            r2 = rows[c2]
            if _near(r2[0], -q[1]) and _near(r2[1], -q[0]) and _near(r2[2], q[2]) and _near(r2[3], q[3]):
                rmir[c] = c2
                break
        if rmir[c] < 0:
            return None
    if any(rmir[rmir[c]] != c for c in range(nc)):
        return None
    itc = [c for c in range(nc) if rmir[c] >= c]
    return itc, [(-1 if rmir[c] == c else rmir[c]) for c in itc], amir


def plan(n, rows, classes, max_extra, n_xslots, cus, env=None, lds_max=LDS_MAX):
    """lonsym_build + lonres_plan for a single-component gz table.  {"refused": reason} where gh_build_G fails, else the
    keys of Engine.shift_invariant_plan()."""
    env = env or {}
    geti = lambda k, d: int(env.get(k, d))
    na, nc = len(classes), len(rows)
    p = {"on": True, "n": n, "na": na, "nc": nc, "nf": n // 2 + 1, "n_xslots": n_xslots, "max_extra": max_extra}
    AG = (na + 63) // 64
    nb16 = (n + 15) // 16
    W = 16 if (geti("GRAVHMC_LONSYM_W", 16) == 16 and 4 <= AG * nb16 <= LS_WAVES) else 8
    KB = cdiv(n, W)
    thr = 512 if (W == 16 and AG * KB <= 8 and n <= 512) else 1024
    steps = KB * W
    SW = (steps + 15) // 16 * 16 + 1
    lds = 8 * ((2 * na + 1) * SW + steps + 8 + AG * KB * W + 32)
    code = 0
    if n > LS_THREADS:
        code = 1
    elif AG * KB > (thr // 64) * (1 if W == 16 else LS_MAXITEMS):
        code = 2
    elif lds > 160 * 1024 - 512:
        code = 3
    elif na * n > 8 * LS_THREADS:
        code = 4
    p.update(W=W, KB=KB, AG=AG, thr=thr, lds=lds, direct_ok=code == 0, direct_refusal=code,
             items=cdiv(AG * KB, thr // 64), grid=min(nc, cus))
    wide_sw = geti("GRAVHMC_LONSYM_WIDE", 1)
    wide_can = 2 <= n <= LW_NMAX and wide_sw != 0
    if code and not wide_can:
        return {"refused": DIRECT_WHY[code]}
    nf = p["nf"]
    rp = max(cdiv(nc, cus), geti("GRAVHMC_LONSYM_ROWS", 1))
    rw = min(rp, 4)
    hlds = 8 * lonsymh_lds_doubles(n, nf, na, rw)
    harmonic = geti("GRAVHMC_LONSYM_HARMONIC", 1) != 0
    harm = (wide_sw != 2 and harmonic and nf <= 64 and na <= 4 * LH_AK and n <= 1024 and hlds <= 160 * 1024 - 512)
    p.update(rp=rp, rw=rw, hlds=hlds, hgrid=cdiv(nc, rp) if harm else 0)
    wide = not harm and wide_can and (harmonic or wide_sw == 2 or code != 0)
    p.update(nfp=0, pairs=0, wmirror=False, witems=0, wgrid=0, wrows=0, wparts=0)
    if wide:
        nfp = (nf + 7) // 8 * 8
        mi = mirror_items(rows, classes) if geti("GRAVHMC_LW_MIRROR", 1) != 0 else None
        ni = len(mi[0]) if mi else nc
        waves_row = cdiv(na * nfp, 64)
        parts = max(1, (cus * geti("GRAVHMC_LW_WAVES_PER_CU", 32) + waves_row - 1) // waves_row)
        parts = min(parts, max(1, ni // 8), 64)
        wrows = cdiv(ni, parts)
        p.update(nfp=nfp, pairs=1 if nf <= LW_THREADS else 2 if nf <= 2 * LW_THREADS else 3, wmirror=mi is not None, witems=ni,
                 wgrid=min(ni, cus * 8), wrows=wrows, wparts=cdiv(ni, wrows))
    if not harm and not wide and code:
        return {"refused": DIRECT_WHY[code]}
    p["form"] = "registers" if harm else "streamed" if wide else "direct"
    res = (harm and geti("GRAVHMC_LONSYM_RESIDENT", 1) != 0 and na <= p["hgrid"] <= LR_MAXWG and p["hgrid"] * rw >= nc
           and na <= 64 and 2 <= n <= 126 and max_extra <= 2 and 8 * lonres_lds_doubles(n, nf, na, rw) <= lds_max)
    p.update(resident_planned=bool(res), resident_usable=bool(res), nwg=p["hgrid"] if res else 0,
             resident_lds=8 * lonres_lds_doubles(n, nf, na, rw) if res else 0)
    return p


def derived(p):
    """What the kernels derive from the plan.  Register form: the rows of every workgroup (per pass of the launches' loop),
    the class groups in use.  Streamed form: the rows of every part.  Persistent launch: clusters, the entries of the
    cluster sum a member produces, members without an entry, the classes' owners."""
    d = {}
    if p["form"] == "registers":
        g, rw, nc = p["hgrid"], p["rw"], p["nc"]
        passes = []
        base0 = 0
        while base0 < nc:
            passes.append([[w + base0 + r * g for r in range(rw) if w + base0 + r * g < nc] for w in range(g) if w + base0 < nc])
            base0 += g * rw
        d.update(passes=len(passes), rows_of=passes[0], ragged=len(set(len(r) for r in passes[0])) > 1 or len(passes[0]) < g,
                 class_groups=cdiv(p["na"], LH_AK), last_group_classes=p["na"] - (cdiv(p["na"], LH_AK) - 1) * LH_AK)
    if p["form"] == "streamed":
        ni, wr = p["witems"], p["wrows"]
        d.update(part_rows=[min(wr, ni - k * wr) for k in range(p["wparts"])])
    if p.get("resident_planned"):
        nwg, E = p["nwg"], p["na"] * p["nf"]
        cn = [(nwg - cg + RES_CLUSTERS - 1) // RES_CLUSTERS for cg in range(RES_CLUSTERS)]
        ch = [cdiv(E, c) if c else 0 for c in cn]
        idle = sum(1 for w in range(nwg) if (w // RES_CLUSTERS) * ch[w % RES_CLUSTERS] >= E)
        owners = [a * nwg // p["na"] for a in range(p["na"])]
        d.update(ncl=min(nwg, RES_CLUSTERS), cn=cn, ch=ch, idle_members=idle, owners=owners, E=E)
    return d


# ----------------------------------------------------------------------------- the case table

def band(ny, nz, lat0, dlat, dz=150000.0, lats=None):
    """ny latitude rows x nz layers (south, north, top, bottom), layer-major as a mesh of shape (nz, ny, n) orders them."""
    edges = list(lats) if lats is not None else [lat0 + dlat * j for j in range(ny + 1)]
    assert len(edges) == ny + 1
    return [(edges[j], edges[j + 1], -dz * k, -dz * (k + 1)) for k in range(nz) for j in range(ny)]


def classes_at(lats, heights=(30000.0,)):
    return [(float(la), float(h)) for h in heights for la in lats]


class Spec(object):
    """expect: the figures the table names for the case (keys of plan() or derived()), on any CU count >= `cus_min`.
    data: the id of the case whose inputs and trajectories this one shares (the same problem on another form)."""

    def __init__(self, cid, group, n, ny, nz, classes, slots, reg, fix, env=None, expect=None, lat0=-6.0, dlat=4.0, lats=None,
                 shuffle=False, delta=DELTA, data=None, cus_min=1, C=1, T=12):
        self.id, self.group, self.n, self.ny, self.nz = cid, group, n, ny, nz
        self.rows = band(ny, nz, lat0, dlat, lats=lats)
        self.classes, self.slots, self.reg, self.fix = classes, slots, reg, fix
        self.env, self.expect, self.shuffle, self.delta, self.data = dict(env or {}), expect or {}, shuffle, delta, data or cid
        self.shape = (nz, ny, n)
        self.nc, self.na, self.M = ny * nz, len(classes), ny * nz * n
        self.cus_min, self.C, self.T = cus_min, C, T
        self.counts = slot_counts(slots, self.na, n)
        self.max_extra = int(max(0, self.counts.max() - 1))
        self.n_xslots = int((self.counts > 1).sum())
        self.N = int(self.counts.sum())

    def plan(self, cus=256, env=None, lds_max=LDS_MAX):
        e = dict(self.env)
        e.update(env or {})
        return plan(self.n, self.rows, self.classes, self.max_extra, self.n_xslots, cus, e, lds_max)


def slot_counts(kind, na, n):
    c = np.ones((na, n), dtype=np.int64)
    if kind == "dup":
        c[:, 0] = 2
    elif kind in ("multi", "x3"):
        c[0, 1 % n] = 2
        c[na // 2, n // 2] = 3
        c[na - 1, n - 1] = 3
        if na > 2:
            c[1, 0] = 2
        if kind == "x3":
            c[0, n - 1] = 4
    elif kind == "empty":
        c[na - 1, ::3] = 0
    elif kind == "single":
        c[0, :] = 0
        c[0, n // 3] = 1
    else:
        assert kind == "ones", kind
    return c


S, D, MS, TV = "Smoothness", "Damping", "MS", "TV"
OFF = {"GRAVHMC_LONSYM_RESIDENT": 0}                                 # the register form on the launches per phase
DIRECT = {"GRAVHMC_LONSYM_HARMONIC": 0, "GRAVHMC_LONSYM_WIDE": 0}
WIDE = {"GRAVHMC_LONSYM_WIDE": 2}
ASYM3 = classes_at((-3.5, 1.25, 7.0))                               # no class has a partner: no mirror
SYM3 = classes_at((-5.0, 0.0, 5.0))


def _lats(k, lo=-20.0, hi=23.0):
    return np.linspace(lo, hi, k)


# lonsymw_sweep_kernel<1 | 2 | 3>: nf = n / 2 + 1 against 256 and 512 (two cell rows, three classes)
PAIRS = [
    Spec("w-510", "pairs", 510, 2, 1, ASYM3, "dup", D, False, expect={"form": "streamed", "nf": 256, "pairs": 1}, dlat=2.0),
    Spec("w-511", "pairs", 511, 2, 1, ASYM3, "ones", MS, True, expect={"form": "streamed", "nf": 256, "pairs": 1}, dlat=2.0,
         shuffle=True),
    Spec("w-512", "pairs", 512, 2, 1, ASYM3, "multi", TV, False, expect={"form": "streamed", "nf": 257, "pairs": 2}, dlat=2.0),
    Spec("w-1022", "pairs", 1022, 2, 1, SYM3, "dup", S, True, lat0=-2.0, dlat=2.0,
         expect={"form": "streamed", "nf": 512, "pairs": 2, "wmirror": True, "witems": 1}),
    Spec("w-1023", "pairs", 1023, 2, 1, ASYM3, "multi", D, True, expect={"form": "streamed", "nf": 512, "pairs": 2, "nfp": 512},
         dlat=2.0, shuffle=True),
    Spec("w-1024", "pairs", 1024, 2, 1, ASYM3, "dup", TV, False, expect={"form": "streamed", "nf": 513, "pairs": 3, "nfp": 520},
         dlat=2.0),
]

# the streamed form's mirror and the parts of its forward product (n = 130: nf = 66, the first beyond the register form)
PARTS = [
    Spec("w-asym-7", "parts", 130, 7, 1, ASYM3, "dup", S, False, expect={"wmirror": False, "witems": 7, "wparts": 1}),
    Spec("w-asym-8", "parts", 130, 4, 2, ASYM3, "ones", TV, True, expect={"witems": 8, "wparts": 1, "wrows": 8}),
    Spec("w-asym-9", "parts", 129, 3, 3, ASYM3, "multi", D, False, expect={"witems": 9, "wparts": 1, "wrows": 9, "nf": 65},
         shuffle=True),
    Spec("w-asym-17", "parts", 130, 17, 1, ASYM3, "dup", TV, True, lat0=-30.0,
         expect={"witems": 17, "wparts": 2, "wrows": 9, "part_rows": [9, 8]}),
    Spec("w-asym-33", "parts", 128, 11, 3, ASYM3, "ones", S, False, lat0=-20.0,
         expect={"form": "streamed", "witems": 33, "wparts": 4, "part_rows": [9, 9, 9, 6]}),
    Spec("w-asym-33-one", "parts", 128, 11, 3, ASYM3, "ones", S, False, lat0=-20.0, env={"GRAVHMC_LW_WAVES_PER_CU": 0},
         expect={"witems": 33, "wparts": 1, "wrows": 33}, data="w-asym-33"),
    Spec("w-mirror", "parts", 129, 5, 2, SYM3, "multi", TV, True, lat0=-10.0,
         expect={"wmirror": True, "witems": 6, "nc": 10}),
    Spec("w-mirror-off", "parts", 129, 5, 2, SYM3, "multi", TV, True, lat0=-10.0, env={"GRAVHMC_LW_MIRROR": 0},
         expect={"wmirror": False, "witems": 10}, data="w-mirror"),
    Spec("w-na65", "parts", 8, 2, 1, classes_at(_lats(65)), "dup", D, True, expect={"form": "streamed", "na": 65, "nf": 5, "nfp": 8}),
]

# lonsymh_sweep_kernel<RW> on the launches per phase: the edges of n, the class groups of LH_AK = 16, rows per workgroup
REGISTERS = [
    Spec("h-n2", "registers", 2, 1, 1, classes_at((2.0,)), "ones", D, False, env=OFF,
         expect={"form": "registers", "nf": 2, "na": 1, "hgrid": 1, "class_groups": 1}),
    Spec("h-n3", "registers", 3, 2, 1, classes_at(_lats(16)), "dup", MS, True, env=OFF,
         expect={"form": "registers", "nf": 2, "class_groups": 1, "last_group_classes": 16}),
    Spec("h-n125", "registers", 125, 7, 1, classes_at(_lats(17)), "multi", TV, False, lat0=-14.0,
         env=dict(OFF, GRAVHMC_LONSYM_ROWS=3, GRAVHMC_LONSYM_FUSED=1),
         expect={"form": "registers", "nf": 63, "rw": 3, "hgrid": 3, "rows_of": [[0, 3, 6], [1, 4], [2, 5]], "ragged": True,
                 "class_groups": 2, "last_group_classes": 1}),
    Spec("h-n126", "registers", 126, 3, 3, classes_at(_lats(32)), "dup", S, True, env=dict(OFF, GRAVHMC_LONSYM_ROWS=2),
         expect={"form": "registers", "nf": 64, "rw": 2, "hgrid": 5, "ragged": True, "class_groups": 2, "last_group_classes": 16},
         shuffle=True),
    Spec("h-n127", "registers", 127, 5, 2, classes_at(_lats(33)), "ones", TV, True, lat0=-10.0, env=dict(OFF, GRAVHMC_LONSYM_ROWS=4),
         expect={"form": "registers", "nf": 64, "rw": 4, "hgrid": 3, "rows_of": [[0, 3, 6, 9], [1, 4, 7], [2, 5, 8]],
                 "class_groups": 3, "last_group_classes": 1, "resident_planned": False}),
    Spec("h-n127-on", "registers", 127, 5, 2, classes_at(_lats(33)), "ones", TV, True, lat0=-10.0, env={"GRAVHMC_LONSYM_ROWS": 4},
         expect={"form": "registers", "resident_planned": False}, data="h-n127"),
    Spec("h-n128", "registers", 128, 2, 1, ASYM3, "dup", D, False, env=OFF, expect={"form": "streamed", "nf": 65, "pairs": 1}),
    Spec("h-na48", "registers", 16, 13, 1, classes_at(_lats(24), (30000.0, 45000.0)), "multi", S, False, lat0=-26.0,
         env=dict(OFF, GRAVHMC_LONSYM_ROWS=4),
         expect={"rw": 4, "hgrid": 4, "rows_of": [[0, 4, 8, 12], [1, 5, 9], [2, 6, 10], [3, 7, 11]], "class_groups": 3,
                 "last_group_classes": 16}),
    Spec("h-na49", "registers", 9, 13, 1, classes_at(_lats(49)), "dup", TV, True, lat0=-26.0, env=dict(OFF, GRAVHMC_LONSYM_ROWS=5),
         expect={"rp": 5, "rw": 4, "hgrid": 3, "passes": 2, "class_groups": 4, "last_group_classes": 1}, shuffle=True),
    Spec("h-na64", "registers", 5, 2, 2, classes_at(_lats(32), (30000.0, 45000.0)), "ones", MS, False,
         env=dict(OFF, GRAVHMC_LONSYM_FUSED=1), expect={"form": "registers", "class_groups": 4, "last_group_classes": 16, "rw": 1}),
    Spec("h-rw1-nc10", "registers", 12, 5, 2, ASYM3, "dup", S, True, lat0=-10.0, env=dict(OFF, GRAVHMC_LONSYM_ROWS=1),
         expect={"rw": 1, "hgrid": 10, "passes": 1}, cus_min=10),
]

# lonsymh_resident_kernel<RW>: the exchange's edges
RESIDENT = [
    Spec("p-1", "persistent", 4, 1, 1, classes_at((1.0,)), "ones", D, False, expect={"nwg": 1, "ncl": 1, "cn": [1] + [0] * 7}),
    Spec("p-2", "persistent", 6, 2, 1, classes_at((-1.0, 3.0)), "dup", MS, True, expect={"nwg": 2, "ncl": 2, "owners": [0, 1]},
         cus_min=2),
    Spec("p-7", "persistent", 8, 7, 1, ASYM3, "multi", TV, False, lat0=-14.0, expect={"nwg": 7, "ncl": 7, "cn": [1] * 7 + [0]},
         cus_min=7),
    Spec("p-8", "persistent", 8, 4, 2, classes_at(_lats(8)), "dup", S, True, lat0=-8.0,
         expect={"nwg": 8, "ncl": 8, "cn": [1] * 8, "owners": list(range(8))}, cus_min=8),
    Spec("p-9", "persistent", 10, 3, 3, classes_at(_lats(4)), "ones", TV, True, expect={"nwg": 9, "cn": [2] + [1] * 7}, cus_min=9,
         shuffle=True),
    Spec("p-17-rw3", "persistent", 8, 10, 5, classes_at(_lats(5)), "multi", TV, False, lat0=-20.0, env={"GRAVHMC_LONSYM_ROWS": 3},
         expect={"nwg": 17, "rw": 3, "ragged": True, "cn": [3] + [2] * 7, "passes": 1}, cus_min=17),
    Spec("p-40-e4", "persistent", 2, 8, 5, classes_at((-2.0, 4.0)), "ones", D, True, lat0=-16.0,
         expect={"nwg": 40, "E": 4, "cn": [5] * 8, "ch": [1] * 8, "idle_members": 8}, cus_min=40),
    Spec("p-refused", "persistent", 6, 2, 2, classes_at(_lats(5)), "dup", MS, False,
         expect={"form": "registers", "hgrid": 4, "na": 5, "resident_planned": False}, cus_min=4),
    Spec("p-256", "persistent", 2, 16, 16, ASYM3, "dup", S, False, lat0=-32.0, expect={"nwg": 256, "cn": [32] * 8, "rw": 1},
         cus_min=256),
    Spec("p-rw2", "persistent", 12, 3, 3, classes_at(_lats(4)), "dup", S, True, env={"GRAVHMC_LONSYM_ROWS": 2},
         expect={"nwg": 5, "rw": 2, "ragged": True, "rows_of": [[0, 5], [1, 6], [2, 7], [3, 8], [4]]}, cus_min=5),
    Spec("p-rw4", "persistent", 6, 7, 2, ASYM3, "multi", TV, True, lat0=-14.0, env={"GRAVHMC_LONSYM_ROWS": 4},
         expect={"nwg": 4, "rw": 4, "ragged": True, "rows_of": [[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10], [3, 7, 11]]}, cus_min=4),
    Spec("p-rp5", "persistent", 6, 11, 1, ASYM3, "dup", S, False, lat0=-22.0, env={"GRAVHMC_LONSYM_ROWS": 5},
         expect={"rp": 5, "rw": 4, "nwg": 3, "passes": 1, "owners": [0, 1, 2]}, cus_min=3),
    Spec("p-rp5-loop", "persistent", 6, 13, 1, ASYM3, "dup", S, False, lat0=-26.0, env={"GRAVHMC_LONSYM_ROWS": 5},
         expect={"rp": 5, "rw": 4, "hgrid": 3, "passes": 2, "resident_planned": False}, cus_min=3),
    Spec("p-n126", "persistent", 126, 3, 1, ASYM3, "multi", D, True, expect={"nwg": 3, "nf": 64}, cus_min=3, shuffle=True),
    Spec("p-na64", "persistent", 4, 8, 8, classes_at(_lats(32), (30000.0, 45000.0)), "dup", D, True, lat0=-16.0,
         expect={"nwg": 64, "na": 64, "owners": list(range(64))}, cus_min=64),
    Spec("p-x3", "persistent", 12, 2, 2, classes_at(_lats(4)), "x3", MS, True,
         expect={"form": "registers", "max_extra": 3, "resident_planned": False}, cus_min=4),
]

# the slots: every kind on the four forms (one problem per kind, shared by its four cases)
_SLOT_FORMS = (("direct", DIRECT, "direct"), ("registers", OFF, "registers"), ("streamed", WIDE, "streamed"),
               ("persistent", {}, "registers"))
SLOTS = []
for _k, (_kind, _reg, _fix, _mx) in enumerate((("ones", TV, False, 0), ("empty", D, True, 0), ("single", S, False, 0),
                                              ("multi", MS, True, 2))):
    for _tag, _env, _form in _SLOT_FORMS:
        _e = {"form": _form, "max_extra": _mx}
        if _tag == "persistent":
            _e["nwg"] = 4
        SLOTS.append(Spec("s-%s-%s" % (_kind, _tag), "slots", 12, 2, 2, classes_at(_lats(4)), _kind, _reg, _fix, env=_env, expect=_e,
                          data="s-%s-direct" % _kind, cus_min=4, shuffle=_k % 2 == 1))

# lonsym_sweep_kernel<ITEMS, W, THREADS>
DIRECTS = [
    Spec("d-8", "direct", 8, 3, 1, ASYM3, "dup", D, False, env=DIRECT, expect={"form": "direct", "W": 8, "KB": 1, "thr": 1024, "items": 1}),
    Spec("d-16", "direct", 16, 2, 2, ASYM3, "multi", TV, True, env=DIRECT, expect={"W": 8, "KB": 2, "items": 1}),
    Spec("d-63", "direct", 63, 3, 1, ASYM3, "dup", S, False, env=DIRECT, expect={"W": 16, "KB": 4, "thr": 512}, shuffle=True),
    Spec("d-64", "direct", 64, 3, 1, ASYM3, "ones", S, True, env=DIRECT, expect={"W": 16, "KB": 4, "thr": 512}),
    Spec("d-65", "direct", 65, 3, 1, ASYM3, "dup", D, True, env=DIRECT, expect={"W": 16, "KB": 5, "thr": 512}),
    Spec("d-128", "direct", 128, 2, 1, ASYM3, "multi", TV, False, env=DIRECT, expect={"W": 16, "KB": 8, "thr": 512}),
    Spec("d-144", "direct", 144, 2, 1, ASYM3, "dup", MS, True, env=DIRECT, expect={"W": 16, "KB": 9, "thr": 1024}),
    Spec("d-512", "direct", 512, 2, 1, ASYM3, "dup", S, False, env=DIRECT, dlat=2.0, expect={"W": 8, "KB": 64, "items": 4}),
    Spec("d-na64", "direct", 8, 2, 1, classes_at(_lats(64)), "dup", D, False, env=DIRECT, expect={"AG": 1, "W": 8, "items": 1}),
    Spec("d-na65", "direct", 8, 2, 1, classes_at(_lats(65)), "dup", TV, True, env=DIRECT, expect={"AG": 2, "W": 8, "items": 1}),
]

# three chains on the store (gh_batch_*): taking turns in the persistent launch, and every chain on its own stream, on the
# ragged rw = 3 layout and on lonsymw_sweep_kernel<2>
CHAINS = [
    Spec("c-rw3-turns", "chains", 8, 10, 5, classes_at(_lats(5)), "multi", TV, False, lat0=-20.0, env={"GRAVHMC_LONSYM_ROWS": 3},
         expect={"nwg": 17, "rw": 3, "ragged": True, "resident_planned": True}, cus_min=17, C=3, T=5),
    Spec("c-rw3-streams", "chains", 8, 10, 5, classes_at(_lats(5)), "multi", TV, False, lat0=-20.0,
         env=dict(OFF, GRAVHMC_LONSYM_ROWS=3), expect={"hgrid": 17, "rw": 3, "ragged": True, "resident_planned": False},
         data="c-rw3-turns", cus_min=17, C=3, T=5),
    Spec("c-w512-streams", "chains", 512, 2, 1, ASYM3, "multi", S, True, dlat=2.0, expect={"form": "streamed", "pairs": 2},
         C=3, T=5, shuffle=True),
]

CASES = PAIRS + PARTS + REGISTERS + RESIDENT + SLOTS + DIRECTS + CHAINS
BY_ID = dict((s.id, s) for s in CASES)
assert len(BY_ID) == len(CASES)


class Refusal(object):
    """A geometry gh_build_G refuses: no oracle data, the reason alone."""

    def __init__(self, cid, n, classes, env, why, ny=1):
        self.id, self.n, self.classes, self.env, self.why = cid, n, classes, env, why
        self.rows = band(ny, 1, -2.0, 4.0)
        self.na, self.nc = len(classes), ny
        self.counts = np.ones((self.na, n), dtype=np.int64)

    def plan(self, cus=256):
        return plan(self.n, self.rows, self.classes, 0, 0, cus, self.env)


REFUSALS = [
    Refusal("r-1025", 1025, ASYM3, {}, DIRECT_WHY[1]),
    Refusal("r-direct-1025", 1025, ASYM3, DIRECT, DIRECT_WHY[1]),
    Refusal("r-direct-513", 513, ASYM3, DIRECT, DIRECT_WHY[2]),
    Refusal("r-direct-1024", 1024, ASYM3, DIRECT, DIRECT_WHY[2]),
    Refusal("r-direct-lds", 16, classes_at(_lats(300, -60.0, 60.0), (30000.0, 45000.0)), DIRECT, DIRECT_WHY[3]),
    Refusal("r-direct-8192", 512, classes_at(_lats(17)), DIRECT, DIRECT_WHY[4]),
]


# ----------------------------------------------------------------------------- inputs and oracle trajectories

def geometry(spec):
    """bounds (M, 6) and the observations (lon, lat, h, class, slot) of a case, in the order the engine gets them."""
    n = spec.n
    edges = np.linspace(-180.0, 180.0, n + 1)
    bounds = np.empty((len(spec.rows), n, 6))
    bounds[:, :, 0], bounds[:, :, 1] = edges[None, :-1], edges[None, 1:]
    for c, (s, nn, top, bot) in enumerate(spec.rows):
        bounds[c, :, 2:] = (s, nn, top, bot)
    lon, lat, h, a_of, m_of = [], [], [], [], []
    for a, (la, hh) in enumerate(spec.classes):
        for m in range(n):
            for q in range(int(spec.counts[a, m])):
                lon.append(edges[m] + (360.0 if q == 1 else 0.0))      # (the second observation of a slot: one turn on)
                lat.append(la)
                h.append(hh)
                a_of.append(a)
                m_of.append(m)
    return bounds.reshape(-1, 6), tuple(np.array(v) for v in (lon, lat, h)), np.array(a_of), np.array(m_of)


class Data(rc.Data):
    """Inputs of one case and the oracle's trajectories (resident_oracle_cases.Data's generator on the tesseroid kernel)."""

    def __init__(self, orc, spec):
        self.spec = spec
        self.bounds, obs, self.a_of, self.m_of = geometry(spec)
        rng = np.random.default_rng(sum(map(ord, spec.data)) * 7919 + spec.n)
        if spec.shuffle:
            perm = rng.permutation(obs[0].size)
            obs, self.a_of, self.m_of = tuple(v[perm] for v in obs), self.a_of[perm], self.m_of[perm]
        self.obs = obs
        self.N, self.M, self.C, self.T, self.shape, self.reg = obs[0].size, spec.M, spec.C, spec.T, spec.shape, spec.reg
        assert self.N == spec.N and self.bounds.shape[0] == spec.M
        self.K = np.asfortranarray(orc.tess_gz_kernel(obs[0], obs[1], obs[2], self.bounds))
        self.alpha = 0.05 / self.N if spec.reg == "MS" else 0.5
        self.beta = 0.01
        Aw, wm = orc.col_weight(self.K, 0.5)
        d_true = Aw @ rng.uniform(0.3, 0.7, size=self.M)
        spread = float(np.abs(d_true).max())
        noisy = d_true + 0.02 * spread * rng.normal(size=self.N)
        self.dobs = noisy + 1e3 * max(float(noisy.std()), 1e-3 * spread)
        self.gfix = (spread * (0.3 * rng.normal(size=self.N) + 2.0)) if spec.fix else None
        self.P, self.wm = _problem(orc, self, self.K)
        self.mwapr = 0.001 * self.wm
        self.xr = rng.uniform(0.3, 0.7, size=self.M)                  # the random model of forward / misfit_and_grad
        self.rr = rng.normal(size=self.N)                             # and the residual of adjoint
        self._generate(rng)

    # -- the store's view of K
    def table(self, orc):
        """T[a][s][c]: the oracle's entry of class a at shift s against the cell of longitude index 0 of row c."""
        n, na, nc = self.spec.n, self.spec.na, self.spec.nc
        edges = np.linspace(-180.0, 180.0, n + 1)
        lon = np.tile(edges[:-1], na)
        lat = np.repeat([c[0] for c in self.spec.classes], n)
        h = np.repeat([c[1] for c in self.spec.classes], n)
        T = orc.tess_gz_kernel(lon, lat, h, self.bounds[::n])
        return np.ascontiguousarray(T.reshape(na, n, nc))

    def from_table(self, T):
        n, nc = self.spec.n, self.spec.nc
        K = np.empty((self.N, self.M), order="F")
        sh = (self.m_of[:, None] - np.arange(n)[None, :]) % n
        for c in range(nc):
            K[:, c * n:(c + 1) * n] = T[self.a_of[:, None], sh, c]
        return K

    def symmetrised(self, orc, mirror):
        T = self.table(orc)
        if mirror:
            itc, itc2, amir = mirror_items(self.spec.rows, self.spec.classes)
            for c, c2 in zip(itc, itc2):
                if c2 >= 0:
                    T[:, :, c2] = T[amir, :, c]
        return self.from_table(T)

    def quantities(self, P):
        """The compared quantities that are no trajectory: forward, adjoint, misfit_and_grad at the random model."""
        mg = P.misfit_and_grad(self.xr)
        return [P.Aw @ self.xr, P.Aw.T @ self.rr, np.array([mg[0], mg[3], mg[4]]), mg[1], mg[2]]

    def far(self, P):
        """distance() of the problem P's results from the case's own, over the trajectories and quantities()."""
        w = distance(self, self.ref, replay(P, self))
        return max([w] + [relmax(a, b) for a, b in zip(self.quantities(P), self.quantities(self.P))])

    def probes(self, cus=256):
        """The table entries (row, class, shifts, signs) the sensitivity is measured at, named."""
        s = self.spec
        p = s.plan(cus)
        d = derived(p)
        n, na, nc = s.n, s.na, s.nc
        out = [("last row, last class, last shift", (nc - 1, na - 1, [n - 1], None))]
        first_row = nc - 1
        if p["form"] == "registers":
            first_row = d["rows_of"][-1][0]
        elif p["form"] == "streamed":
            first_row = (p["wparts"] - 1) * p["wrows"]
            mi = mirror_items(s.rows, s.classes) if p["wmirror"] else None
            first_row = mi[0][first_row] if mi else first_row
        out.append(("first row of the last workgroup or part, first class of the last class group, shift 0",
                    (first_row, (cdiv(na, LH_AK) - 1) * LH_AK, [0], None)))
        if n % 2 == 0 and n > 2:
            out.append(("the highest frequency: alternating signs over the shifts", (nc // 2, na // 2, list(range(n)), "alt")))
        if s.counts.max() >= 3:
            a, m = [int(v[0]) for v in np.nonzero(s.counts >= 3)]
            out.append(("a slot that holds three observations, against the cell under it", (0, a, [0], ("slot", m))))
        return out

    def perturbed(self, orc, probe, delta):
        """The oracle's results with the probe's table entries scaled by 1 + delta (weights, mwapr and all): every
        K[i, (c, k)] with class a and (m_i - k) mod n among the shifts.  ("slot", m): only the observations of slot m --
        what a wrong count of that slot would do."""
        c, a, shifts, how = probe
        n = self.spec.n
        K = self.K.copy(order="F")
        sh = (self.m_of[:, None] - np.arange(n)[None, :]) % n
        f = np.ones(n)
        for q in shifts:
            f[q] = 1.0 + (delta * (-1.0) ** q if how == "alt" else delta)
        rows = self.a_of == a
        if isinstance(how, tuple):
            rows = rows & (self.m_of == how[1])
        K[rows, c * n:(c + 1) * n] *= f[sh[rows]]
        return _problem(orc, self, K)[0]


def _problem(orc, data, K):
    Aw, wm = orc.col_weight(K, 0.5)
    return orc.Problem(Aw, data.dobs, 0.001 * wm, data.reg, data.alpha, data.beta, wm=wm, shape=data.shape, grav_fix=data.gfix), wm


@functools.lru_cache(maxsize=3)
def _cached(data_id):
    from oracle import oracle
    return Data(oracle, BY_ID[data_id])


def make(cid):
    """The case's Data (generated once per shared problem; treat it as read-only)."""
    return _cached(BY_ID[cid].data)
