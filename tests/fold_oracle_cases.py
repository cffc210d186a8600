"""The cases of the folded sweeps against the CPU oracle (tests/test_gpu_fold_oracle.py on the device,
tests/test_fold_oracle_host.py for the generator itself): the case table, the sweep plan of csrc/host_sweep.h and
csrc/host_fold.h restated from the CU count, the mirror and diagonal permutations of a geometry built in NumPy, and
the generator of inputs and oracle trajectories.  No device.

A case is a prism mesh on [0, X] x [0, Y] x [0, Z] under an np.linspace grid of observations on the same rectangle
(flat at z = 0, or at heights that depend on |x - cx| and |y - cy| only), the oracle's own weighted kernel Aw, data
of a sparse model plus noise (not themselves symmetric), one chain in a box of +-1.5 dt around its start and T
trajectories of 1 .. 6 steps.  Everything the device is compared with comes from oracle.Problem.leapfrog on Aw,
before an engine is touched.  The variate u of a trajectory sits half-way between the oracle's exp(-dH) and 0 or 1;
a rejection is used only where dH > 0.01.

"U" cases run fold_sweep_kernel<EPT2> (a rectangular observation grid, cells that are not square, or pairing
switched off), "P" cases fold_pair_sweep_kernel<ROWS> (square cells under square observations).  For both
rows = ceil(ldF / 512) with nF = N / 4 and ldF = roundup(nF, 16).

delta: the relative change of a whole folded row (all images of one fundamental observation) or of a whole work
item (the columns of all its cells) of Aw that moves the oracle's results by more than 100 TOL_TRAJ; per case in the
table (the host test checks it at probes()).  A single entry is no unit here: the store holds orbit means, and these
problems are over-determined."""
import functools

import numpy as np

from batch_oracle_cases import TOL_TRAJ, cdiv, roundup16
from helpers import metropolis_u, relmax, stable_dt

DELTA = 1e-4          # per case unless the table says otherwise
REGS = ("Damping", "MS", "Smoothness", "TV")
WANT = (True, False, True, False, True, True)      # the decisions of a case's trajectories

FOLD_MAX_ROWS = 5                   # csrc/host_fold.h: FOLD_MAX_EPT2
PAIR_MAX_LDS = 160 << 10            # FOLD_PAIR_MAX_LDS
PAIR_SLOT = 64                      # csrc/fold.hip.h: FOLD_PSLOT


# ----------------------------------------------------------------------------- the plans, restated

def fold_rows(N):
    """nF, ldF and the rows per thread of either kernel (ept2 = ceil(2 ldF / 1024) = pair_rows = ceil(ldF / 512))."""
    nF = N // 4
    ldF = roundup16(nF)
    assert cdiv(2 * ldF, 1024) == cdiv(ldF, 512)
    return nF, ldF, cdiv(ldF, 512)


def pair_lds(N):
    return (8 * (N // 4) + 2 * PAIR_SLOT) * 8


def fold_taken(N, paired):
    """fold_use: the fold takes the problem (else reason "path"); the paired form needs its LDS as well."""
    rows = fold_rows(N)[2]
    return rows <= FOLD_MAX_ROWS and (not paired or pair_lds(N) <= PAIR_MAX_LDS)


def dense_layout(N, M, cus, min_cols=None, wg_per_cu=None):
    """configure_sweep (csrc/host_sweep.h) for one panel: team width, columns per team, teams, workgroups.
    wg_per_cu: the residency the grid is sized for -- the code's own figure, which the kernel's occupancy may lower
    (hence the argument: a plan that holds for every value from 1 up to the default holds on the device)."""
    ld = roundup16(N)
    assert ld <= 16384
    tw = 1 if ld <= 1024 else 4 if ld <= 4096 else 8 if ld <= 6144 else 16
    wg_teams = 4 if tw == 1 else 1
    dflt = 1 if tw == 16 else 2 if tw == 8 else 4
    if tw == 4:
        need = cdiv(8 << 20, ld * 8)
        dflt = max(1, min(4, cdiv(need, cus)))
    wpc = dflt if wg_per_cu is None else min(dflt, wg_per_cu)
    if min_cols is None:
        min_cols = 2 if tw == 1 else 1
    cpt = max(cdiv(M, cus * wpc * wg_teams), min_cols)
    n_teams = cdiv(M, cpt)
    grid = cdiv(n_teams, wg_teams)
    if tw == 1:
        n_teams = grid * wg_teams
    return {"tw": tw, "cols_per_team": cpt, "n_teams": n_teams, "grid": grid, "wg_per_cu": dflt}


def fold_plan(items, dense_grid, cus):
    """fold_use: grid = min(CUs x occupancy, the dense sweep's grid, items); per workgroup = ceil(items / grid);
    launched = ceil(items / per workgroup).  Needs dense_grid <= cus (occupancy >= 1 then drops out).  Returns the
    run lengths of the launched workgroups."""
    assert 1 <= dense_grid <= cus, (dense_grid, cus)
    grid = min(dense_grid, items)
    per = cdiv(items, grid)
    launched = cdiv(items, per)
    return [per] * (launched - 1) + [items - per * (launched - 1)]


# ----------------------------------------------------------------------------- the case table

class Spec(object):
    """obs = (n along x, n along y); cells = (nx, ny, nz); paired: which kernel; pair_reason: what fold_info() and
    gh_fold_detect_pair answer; min_cols: GRAVHMC_MIN_COLS of the case; runs: the run lengths it was written for
    (None: whatever the plan gives, one item per workgroup where the CUs allow)."""

    def __init__(self, cid, group, obs, cells, reg, min_cols, paired=False, pair_reason=None, runs=None,
                 switch_off=False, shuffle=False, topo=False, layers=None, extent=None, delta=DELTA, note=""):
        self.id, self.group, self.obs, self.cells, self.reg, self.min_cols = cid, group, obs, cells, reg, min_cols
        self.paired, self.runs, self.switch_off, self.shuffle, self.topo = paired, runs, switch_off, shuffle, topo
        self.layers, self.extent, self.delta, self.note = layers, extent, delta, note
        if pair_reason is None:
            pair_reason = "on" if paired else "switched off" if switch_off else "observations not square"
        self.pair_reason = pair_reason
        self.N, self.M = obs[0] * obs[1], cells[0] * cells[1] * cells[2]
        self.nF, self.ldF, self.rows = fold_rows(self.N)

    @property
    def square(self):
        """the geometry has the diagonal reflection (detected, whether or not the sweep uses it)"""
        return self.paired or self.switch_off

    def counts(self):
        """(pairs, single orbits) of the work list: the quadrant's cell columns off and on its diagonal."""
        if not self.square:
            return 0, 0
        q, nz = self.cells[0] // 2, self.cells[2]
        return q * (q - 1) // 2 * nz, q * nz

    def items(self):
        return sum(self.counts()) if self.paired else self.M // 4

    def env(self):
        e = {"GRAVHMC_MIN_COLS": self.min_cols}
        if self.switch_off:
            e["GRAVHMC_FOLD_PAIR"] = 0
        return e


# the row edges of both kernels, at the smallest shapes that reach them
ROW_EDGES = [
    Spec("U-2x2", "U1", (2, 2), (2, 4, 2), "Damping", 2,
         note="one live row, ld = 16; one double2 pair of 1024 threads"),
    Spec("U-6x6", "U1", (6, 6), (2, 4, 2), "MS", 2, pair_reason="cells not square", extent=(2000.0, 2000.0),
         note="nF = 9 < 16: padding rows inside the only wave that works"),
    Spec("U-32x64", "U1", (32, 64), (4, 6, 3), "Smoothness", 2, note="every thread live, no padding row, n2 = 1024"),
    Spec("U-16x100", "U1", (16, 100), (4, 6, 3), "MS", 2,
         note="nF = ldF = 400: no padding row, the clamped double2 of threads 800 .. 1023 is real: last_in masks it"),
    Spec("U-24x86", "U2", (24, 86), (4, 6, 3), "TV", 2, note="four live rows past 512: last_in for 32 threads, 8 real"),
    Spec("U-64x64-off", "U2", (64, 64), (4, 4, 3), "Damping", 2, switch_off=True, note="second double2 full"),
    Spec("U-64x96", "U3", (64, 96), (4, 6, 3), "MS", 2, note="three double2 full"),
    Spec("U-70x88", "U4", (70, 88), (4, 6, 3), "Smoothness", 2, note="four live rows past 1536"),
    Spec("U-80x128", "U5", (80, 128), (4, 6, 3), "TV", 2, note="nF = 2560: the largest the fold takes, all rows full"),
    Spec("U-100x100-off", "U5", (100, 100), (4, 4, 3), "Damping", 2, switch_off=True,
         note="the benchmark's observations on the fallback kernel"),
    Spec("P-44", "P1", (44, 44), (4, 4, 3), "MS", 2, paired=True,
         note="threads 484 .. 511 idle; LDS holds 4 nF, not 4 ldF"),
    Spec("P-40", "P1", (40, 40), (4, 4, 3), "TV", 2, paired=True,
         note="nF = ldF = 400: threads 400 .. 511 re-read the real row 399 of the block and of r: last_in masks them"),
    Spec("P-46", "P2", (46, 46), (4, 4, 3), "Smoothness", 2, paired=True,
         note="17 live threads in the last row group, the others re-read row nF - 1"),
    Spec("P-64", "P2", (64, 64), (6, 6, 2), "TV", 2, paired=True, note="every thread live in both groups"),
    Spec("P-72", "P3", (72, 72), (4, 4, 3), "Damping", 2, paired=True,
         note="nF = ldF = 1296: 272 live threads in the third group, the others re-read the REAL row nF - 1"),
    Spec("P-90", "P4", (90, 90), (4, 4, 3), "TV", 2, paired=True, note="last group nearly full"),
    Spec("P-92", "P5", (92, 92), (6, 6, 2), "Smoothness", 2, paired=True, note="68 live threads in the fifth group"),
    Spec("P-100", "P5", (100, 100), (4, 4, 3), "MS", 16, paired=True, runs=[3, 3, 3],
         note="the benchmark's instantiation, 157 of 160 KiB LDS"),
]

# how many work items a workgroup runs, at the small row shapes U-24x86 and P-46 (one team per workgroup)
_U, _P = (24, 86), (46, 46)
WORK_LISTS = [
    Spec("U-run1", "runs", _U, (4, 6, 3), "Damping", 2, runs=[1] * 18),
    Spec("U-run2", "runs", _U, (4, 6, 3), "MS", 8, runs=[2] * 9),
    Spec("U-run5553", "runs", _U, (4, 6, 3), "Smoothness", 18, runs=[5, 5, 5, 3]),
    Spec("U-run666", "runs", _U, (4, 6, 3), "TV", 24, runs=[6, 6, 6], note="even: leaves through the second break"),
    Spec("U-run99", "runs", _U, (4, 6, 3), "Damping", 36, runs=[9, 9]),
    Spec("U-run18", "runs", _U, (4, 6, 3), "MS", 72, runs=[18], note="one workgroup: pp_part has nothing to zero"),
    Spec("P-singles-1", "runs", _P, (2, 2, 5), "Smoothness", 2, paired=True, runs=[1] * 5, note="pairs == 0"),
    Spec("P-singles-all", "runs", _P, (2, 2, 5), "TV", 20, paired=True, runs=[5], note="pairs == 0, one workgroup"),
    Spec("P-mix-22221", "runs", _P, (4, 4, 3), "Damping", 10, paired=True, runs=[2, 2, 2, 2, 1],
         note="S P | S S | P S | S P | S"),
    Spec("P-mix-333", "runs", _P, (4, 4, 3), "MS", 16, paired=True, runs=[3, 3, 3], note="S P S in every workgroup"),
    Spec("P-mix-444", "runs", _P, (6, 6, 2), "Smoothness", 24, paired=True, runs=[4, 4, 4],
         note="S P P S | P S S P | P S P S: a single between two pairs"),
    Spec("P-mix-54", "runs", _P, (4, 4, 3), "TV", 24, paired=True, runs=[5, 4], note="S P S S P | S S P S"),
    Spec("U-shuffled", "shuffled", _U, (4, 6, 3), "Smoothness", 8, shuffle=True, runs=[2] * 9),
    Spec("P-shuffled", "shuffled", _P, (4, 4, 3), "TV", 16, paired=True, shuffle=True, runs=[3, 3, 3]),
    Spec("U-topo", "topography", _U, (4, 6, 2), "MS", 8, topo=True, layers=(0.3, 0.7), runs=[2] * 6),
    Spec("P-topo", "topography", _P, (4, 4, 2), "Damping", 8, paired=True, topo=True, layers=(0.3, 0.7),
         runs=[2, 2, 2]),
]

CASES = ROW_EDGES + WORK_LISTS
BY_ID = dict((s.id, s) for s in CASES)

# observation grids one step past the largest the fold takes: six rows per thread
REFUSALS = [((102, 102), (4, 4, 3)), ((84, 122), (4, 6, 3))]


# ----------------------------------------------------------------------------- geometry and its symmetries

def geometry(spec_or_obs, cells=None, topo=False, layers=None, shuffle=False, extent=None):
    """obs (3, N) and b6 (M, 6): cells (nx, ny, nz) on [0, X] x [0, Y] x [0, 1000] (x fastest, then y, then z: the
    mesher's order; extent = (X, Y), by default columns of 500 x 500), n_x x n_y observations on np.linspace grids
    over the same rectangle.
    layers: the fractions of the depth the layers take (default: equal).  topo: heights that depend on the grid
    indices' distance from the centre line only (so that all images of an observation share theirs bit for bit),
    symmetric in the two where the grid is square."""
    if isinstance(spec_or_obs, Spec):
        s = spec_or_obs
        n_obs, cells, topo, layers, shuffle, extent = s.obs, s.cells, s.topo, s.layers, s.shuffle, s.extent
    else:
        n_obs = spec_or_obs
    nx, ny, nz = cells
    X, Y = extent if extent is not None else (500.0 * nx, 500.0 * ny)
    Z = 1000.0
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, Y, n_obs[1]), np.linspace(0, X, n_obs[0]))]
    zp = np.zeros_like(xp)
    if topo:
        jy, ix = [a.ravel() for a in np.meshgrid(np.arange(n_obs[1]), np.arange(n_obs[0]))]
        a = np.abs(2 * ix - (n_obs[0] - 1)) / float(n_obs[0] - 1)
        b = np.abs(2 * jy - (n_obs[1] - 1)) / float(n_obs[1] - 1)
        zp = -(20.0 + 60.0 * (a + b) + 40.0 * (a * b))           # above the cells' top, highest at the corners
    ex, ey = np.linspace(0, X, nx + 1), np.linspace(0, Y, ny + 1)
    fr = np.full(nz, 1.0 / nz) if layers is None else np.asarray(layers, dtype=float)
    assert fr.size == nz and abs(fr.sum() - 1.0) < 1e-12
    ez = np.concatenate([[0.0], Z * np.cumsum(fr)])
    k, j, i = [a.ravel() for a in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")]
    b6 = np.stack([ex[i], ex[i + 1], ey[j], ey[j + 1], ez[k], ez[k + 1]], axis=1)
    obs = np.stack([xp, yp, zp])
    if shuffle:
        rng = np.random.default_rng(3)
        obs = obs[:, rng.permutation(obs.shape[1])]
        b6 = b6[rng.permutation(b6.shape[0])]
    return np.ascontiguousarray(obs), np.ascontiguousarray(b6)


def _ranks(v, tol):
    """rank of each value among the clusters of values closer than tol, and the number of clusters"""
    order = np.argsort(v, kind="stable")
    step = np.concatenate([[0], (np.diff(v[order]) > tol).astype(np.int64)])
    r = np.empty(v.size, dtype=np.int64)
    r[order] = np.cumsum(step)
    return r, int(r.max()) + 1


def _lookup(keys, images):
    """index of the row of `keys` equal to each row of `images` (-1: none)"""
    table = dict((tuple(k), n) for n, k in enumerate(keys.tolist()))
    assert len(table) == keys.shape[0]
    return np.array([table.get(tuple(k), -1) for k in images.tolist()], dtype=np.int64)


class Symmetry(object):
    """The mirrors s_1: x -> 2 cx - x, s_2: y -> 2 cy - y, s_3 = s_1 s_2 and (square geometries) the diagonal
    reflection tau as permutations of the observations (obs_g[g], obs_tau) and of the cells (cell_g[g], cell_tau),
    from the coordinates alone; the orbit tables and the work list in the order of csrc/host_fold.h: orbits
    [i, s_1 i, s_2 i, s_3 i] by their smallest index, work items (leading orbit, partner or -1) by leading orbit."""

    def __init__(self, obs, b6, square):
        x, y, z = obs
        mag = max(np.abs(b6[:, :4]).max(), np.abs(obs[:2]).max())
        tol = 8 * np.finfo(float).eps * mag
        N, M = x.size, b6.shape[0]
        rx, kx = _ranks(x, tol)
        ry, ky = _ranks(y, tol)
        zb = z.view(np.int64)
        key = np.stack([rx, ry, zb], 1)
        img = lambda mx, my: np.stack([kx - 1 - rx if mx else rx, ky - 1 - ry if my else ry, zb], 1)  # noqa: E731
        self.obs_g = [_lookup(key, img(mx, my)) for mx, my in ((0, 0), (1, 0), (0, 1), (1, 1))]
        ex, kex = _ranks(np.concatenate([b6[:, 0], b6[:, 1]]), tol)
        ey, key_ = _ranks(np.concatenate([b6[:, 2], b6[:, 3]]), tol)
        x1, x2, y1, y2 = ex[:M], ex[M:], ey[:M], ey[M:]
        z1, z2 = np.ascontiguousarray(b6[:, 4]).view(np.int64), np.ascontiguousarray(b6[:, 5]).view(np.int64)
        ckey = np.stack([x1, x2, y1, y2, z1, z2], 1)

        def cimg(mx, my):
            a1, a2 = (kex - 1 - x2, kex - 1 - x1) if mx else (x1, x2)
            c1, c2 = (key_ - 1 - y2, key_ - 1 - y1) if my else (y1, y2)
            return np.stack([a1, a2, c1, c2, z1, z2], 1)
        self.cell_g = [_lookup(ckey, cimg(mx, my)) for mx, my in ((0, 0), (1, 0), (0, 1), (1, 1))]
        for p in self.obs_g + self.cell_g:
            assert p.min() >= 0
        self.obs_tau = self.cell_tau = None
        if square:
            assert kx == ky and kex == key_
            self.obs_tau = _lookup(key, np.stack([ry, rx, zb], 1))
            self.cell_tau = _lookup(ckey, np.stack([y1, y2, x1, x2, z1, z2], 1))
            assert self.obs_tau.min() >= 0 and self.cell_tau.min() >= 0
        self.obs_img = self._orbits(self.obs_g, N)
        self.cell_orbit = self._orbits(self.cell_g, M)
        self.work = None
        if square:
            orbit_of = np.empty(M, dtype=np.int64)
            orbit_of[self.cell_orbit.ravel()] = np.repeat(np.arange(M // 4), 4)
            partner = orbit_of[self.cell_tau[self.cell_orbit[:, 0]]]
            self.work = np.array([(o, -1 if p == o else p) for o, p in enumerate(partner) if o <= p], dtype=np.int64)

    @staticmethod
    def _orbits(g, n):
        seen, out = np.zeros(n, dtype=bool), []
        for i in range(n):
            if not seen[i]:
                orb = [i, g[1][i], g[2][i], g[3][i]]
                assert len(set(orb)) == 4
                seen[orb] = True
                out.append(orb)
        return np.array(out, dtype=np.int64)

    def mean(self, Aw):
        """Aw averaged over each orbit: four images, eight where the geometry has tau."""
        A4 = sum(Aw[np.ix_(self.obs_g[g], self.cell_g[g])] for g in range(4)) * 0.25
        if self.obs_tau is None:
            return np.asfortranarray(A4)
        return np.asfortranarray(0.5 * (A4 + A4[np.ix_(self.obs_tau, self.cell_tau)]))

    def row_images(self, f, paired):
        """all images of the fundamental observation f"""
        r = self.obs_img[f]
        return np.unique(np.concatenate([r, self.obs_tau[r]])) if paired else r

    def item_cells(self, w, paired):
        """the cells of work item w: an orbit, with its partner's in the paired sweep"""
        if not paired:
            return self.cell_orbit[w]
        o, o2 = self.work[w]
        return self.cell_orbit[o] if o2 < 0 else np.concatenate([self.cell_orbit[o], self.cell_orbit[o2]])


# ----------------------------------------------------------------------------- inputs and oracle trajectories

class Ref(object):
    """What the oracle's chain did: decisions (T), out5 (T, 5), the states after every trajectory (T, M), and
    misfit_and_grad at the model xt."""

    def __init__(self, T, M):
        self.acc = np.zeros(T, dtype=bool)
        self.out5 = np.zeros((T, 5))
        self.xs = np.zeros((T, M))
        self.mg = None


def replay(P, d):
    """The case's trajectories (its L, p0, u) and its misfit_and_grad on the problem P: a Ref."""
    ref = Ref(d.T, d.M)
    x = d.x0
    for t, (L, p0, u) in enumerate(d.trajs):
        x, acc, o, _ = P.leapfrog(x, p0, d.dt, L, d.low, d.high, u)
        ref.acc[t], ref.out5[t], ref.xs[t] = acc, o, x
    out = P.misfit_and_grad(d.xt)
    ref.mg = (out[0], out[1].copy(), out[2].copy())
    return ref


def mg_distance(mg, ref_mg):
    return max(abs(mg[0] - ref_mg[0]) / abs(ref_mg[0]), relmax(mg[1], ref_mg[1]), relmax(mg[2], ref_mg[2]))


def distance(d, ref, other, mg=True):
    """The largest difference between two results in what the device test compares: decisions, out5 and x of every
    trajectory and (mg) misfit, gradient and predicted data at xt, each in relmax."""
    if not np.array_equal(ref.acc, other.acc):
        return np.inf
    worst = mg_distance(other.mg, ref.mg) if mg else 0.0
    for t in range(d.T):
        worst = max(worst, relmax(other.out5[t], ref.out5[t]), relmax(other.xs[t], ref.xs[t]))
    return worst


class Data(object):
    """Inputs of one case and the oracle's trajectories."""

    def __init__(self, orc, spec):
        self.spec = s = spec
        self.obs, self.b6 = geometry(s)
        self.N, self.M, self.T = s.N, s.M, len(WANT)
        assert self.obs.shape == (3, s.N) and self.b6.shape == (s.M, 6)
        nx, ny, nz = s.cells
        self.shape = (1, 1, s.M) if s.shuffle else (nz, ny, nx)      # (stencils follow the caller's cell order)
        self.reg, self.alpha, self.beta = s.reg, 1.0, 0.01
        rng = np.random.default_rng(sum(map(ord, s.id)) * 7919 + s.N)
        self.Aw, self.wm = orc.col_weight(orc.prism_gz_kernel(self.obs[0], self.obs[1], self.obs[2], self.b6), 0.5)
        rho = np.zeros(s.M)
        rho[rng.choice(s.M, max(1, s.M // 10), replace=False)] = 1.0
        clean = self.Aw @ (self.wm * rho)
        self.dobs = clean + 0.01 * np.abs(clean).max() * rng.normal(size=s.N)
        self.mwapr = 0.001 * self.wm
        self.P = P = self.problem(orc, self.Aw)
        xc = self.wm * rng.uniform(0.3, 0.7, size=s.M)
        self.dt = dt = stable_dt(P, xc, rng)
        self.low, self.high = xc - 1.5 * dt, xc + 1.5 * dt
        self.x0 = xc + dt * rng.uniform(-1.0, 1.0, size=s.M)
        self.xt = xc + dt * rng.uniform(-1.5, 1.5, size=s.M)
        self.trajs = []
        x = self.x0
        for want in WANT:
            for attempt in range(60):
                L = int(rng.integers(1, 7))
                scale = 0.7 ** attempt if want else 2.0 + 0.5 * attempt
                p0 = rng.normal(size=s.M) * scale
                o = P.leapfrog(x, p0, dt, L, self.low, self.high, 0.5)[2]
                dH = o[4] - o[3]
                if (want and dH < 5.0) or (not want and dH > 0.01):
                    break
            else:
                raise AssertionError("%s: no trajectory for the decision %r" % (s.id, want))
            u = float(metropolis_u(dH, want))
            xn, acc, _, _ = P.leapfrog(x, p0, dt, L, self.low, self.high, u)
            assert acc == want
            self.trajs.append((L, p0, u))
            x = xn
        self.ref = replay(P, self)
        self.sym = Symmetry(self.obs, self.b6, s.square)
        self.check()

    def problem(self, orc, Aw):
        return orc.Problem(Aw, self.dobs, self.mwapr, self.reg, self.alpha, self.beta, wm=self.wm, shape=self.shape)

    def clamped(self):
        """cells of the oracle's accepted states that sit on the lower / on the upper bound"""
        xs = self.ref.xs[self.ref.acc]
        return int((xs == self.low).sum()), int((xs == self.high).sum())

    def check(self):
        """The generator's own conditions (c) and (d)."""
        ref = self.ref
        assert list(ref.acc) == list(WANT) and ref.acc.sum() >= 2 and (~ref.acc).sum() >= 2, self.spec.id
        lo, hi = self.clamped()
        assert lo > 0 and hi > 0, (self.spec.id, lo, hi)
        x = self.x0
        for t in range(self.T):
            if not ref.acc[t]:
                assert np.array_equal(ref.xs[t], x)
            x = ref.xs[t]

    def probes(self, runs):
        """(e): the rows and columns of Aw the sensitivity is measured at, as (name, rows or None, columns or None);
        runs: the run lengths of the plan."""
        s, sym = self.spec, self.sym
        f2 = (s.rows - 1) * 512
        out = [("last live row", sym.row_images(s.nF - 1, s.paired), None),
               ("first row of the last group", sym.row_images(f2 if f2 < s.nF else 0, s.paired), None),
               ("last item of the last workgroup", None, sym.item_cells(s.items() - 1, s.paired))]
        if s.group == "runs":
            out.append(("last item of the first workgroup", None, sym.item_cells(runs[0] - 1, s.paired)))
        return out

    def perturbed(self, orc, rows, cols, delta):
        """The oracle's results with the given rows (or columns) of Aw scaled by 1 + delta."""
        Aw = self.Aw.copy(order="F")
        if rows is not None:
            Aw[rows, :] *= 1.0 + delta
        if cols is not None:
            Aw[:, cols] *= 1.0 + delta
        return replay(self.problem(orc, Aw), self)


@functools.lru_cache(maxsize=4)
def _cached(cid):
    from oracle import oracle
    return Data(oracle, BY_ID[cid])


def make(cid):
    """The case's Data (generated once; treat it as read-only)."""
    return _cached(cid)
