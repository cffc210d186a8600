"""Geometries, host kernels and chain cases of the joint gravity-magnetic store on the translation-invariant table
(test_lattice_joint_host.py, test_gpu_lattice_joint.py): the property of a column as one more layer coordinate, and
every layer on its own observation block.

The store is H = [A_gz Wm^-1 | s A_tf Wm^-1], s = std(A_gz) / std(A_tf): `host_kernels` evaluates the two unweighted
blocks on the host (NumPy corner sums, in pieces of observations), `Blocks` weighs them as gh_weight does and is the
operator crossgrad_host.JointHostProblem runs on (`problem`), `forward_plan` restates how the forward pass cuts the
table's 2 nz layers into chunks, `gradient` restates the two passes with the mistakes the GPU suite must be able to
see, and `chain_case` builds the chains the GPU suite runs, whose conditioning the host suite checks without a
device."""
import numpy as np

from crossgrad_host import JointHostProblem
from lattice_cases import geometry
from lattice_mvi_cases import _safe_atan2, _safe_log, host_blocks

H7 = 2000.0 / 7
GZ_SCALE = 0.00000006673 * 100000.0
INC, DEC = 60.0, 25.0           # (an oblique regional field)

SHAPES = {
    # cells nx, ny, nz / stations px, qy
    "3,7,1 / 2,7": dict(cells=(3, 7, 1), obs=(2, 7), zobs=-15.0),                      # nz = 1: each property one layer
    "4,9,3 / 5,8": dict(cells=(4, 9, 3), obs=(5, 8), first=(-1, 0), zobs=-15.0),       # ny, qy around a multiple of 8
    "3,7,2 / 1,9": dict(cells=(3, 7, 2), obs=(1, 9), first=(1, -1), h=(H7, H7), zobs=-15.0),   # px = 1, beyond the mesh
    "shuffled 4,5,3 / 6,7": dict(cells=(4, 5, 3), obs=(6, 7), first=(-1, -1), h=(H7, 150.0), shuffle=5, zobs=-15.0),
    # 20 480 points per block: over the dense store's 16 384; 21 layers in chunks of 2 on 256 CUs
    "3,5,21 / 40,512": dict(cells=(3, 5, 21), obs=(40, 512), first=(-18, -253), zobs=-15.0),
}
BIG = "3,5,21 / 40,512"
SMALL = tuple(s for s in SHAPES if s != BIG)
#: the shapes whose mesh has two cells along every axis: the cross-gradient term needs a forward neighbour on each
COUPLED = tuple(s for s in SHAPES if min(SHAPES[s]["cells"]) >= 2)
CHAIN_SHAPES = ("4,9,3 / 5,8", "shuffled 4,5,3 / 6,7")
REGS = ("Damping", "MS", "Smoothness", "TV")
LAMBDA, CG_SCALE = 0.1, (1.0, 1.0)


def direction():
    from gravinv3dhmc_amd import utils
    return tuple(float(v) for v in utils.dircos(INC, DEC))


def shape(name):
    """(obs (3, n), bounds6 (m, 6)) of a named shape"""
    return geometry(**SHAPES[name])


def mesh_shape(name):
    """(nz, ny, nx) as the stencils take it: the cells lie layer-major, then a, then b (a shuffle keeps the extents: the
    stencils follow the caller's cell order, whatever cells it holds)"""
    nx, ny, nz = SHAPES[name]["cells"]
    return (nz, nx, ny)


def spacing(name):
    """relative spacings (hx, hy, hz[nz - 1]) for the cross-gradient term, unequal on purpose"""
    nz = SHAPES[name]["cells"][2]
    return 1.0, 1.5, 1.0 + 0.25 * np.arange(max(nz - 1, 0))


def host_gz(obs, b6):
    """(n, m): the unweighted gz block, mGal per g/cm^3 -- the corner sums of x ln(y + r) + y ln(x + r) - z atan2(x y, z r)"""
    S = np.zeros((obs.shape[1], b6.shape[0]))
    for k in (1, 0):
        dz = b6[None, :, 4 + k] - obs[2][:, None]
        for j in (1, 0):
            dy = b6[None, :, 2 + j] - obs[1][:, None]
            for i in (1, 0):
                dx = b6[None, :, i] - obs[0][:, None]
                sign = -1.0 if ((1 - i) + (1 - j) + (1 - k)) & 1 else 1.0
                r = np.sqrt(dx * dx + dy * dy + dz * dz)
                S += sign * -(dx * _safe_log(dy + r) + dy * _safe_log(dx + r) - dz * _safe_atan2(dx * dy, dz * r))
    return S * GZ_SCALE


def host_kernels(obs, b6, piece=2048):
    """(K_gz, K_tf), each (n, m) unweighted, evaluated in pieces of observations (all of the large shape at once is about
    100 MB per field and corner)"""
    f = direction()
    n = obs.shape[1]
    Kgz, Ktf = np.empty((n, b6.shape[0])), np.empty((n, b6.shape[0]))
    for i0 in range(0, n, piece):
        o = obs[:, i0:i0 + piece]
        Kgz[i0:i0 + piece] = host_gz(o, b6)
        K3 = host_blocks(o, b6, f)["tf"]
        # (the scalar total field: the magnetization along the regional field)
        Ktf[i0:i0 + piece] = f[0] * K3[0] + f[1] * K3[1] + f[2] * K3[2]
    return Kgz, Ktf


class Blocks:
    """The joint store of the unweighted blocks K_gz, K_tf (n, m): wm (2m, the column 2-norms of each block), std_gz,
    std_tf (population, over all n m entries), s, and the operator Aw = [[K_gz Wm^-1, 0], [0, s K_tf Wm^-1]] on stacked
    vectors -- `op @ x`, `op.T @ r`, `op.shape`; np.asarray(op) the stacked 2n x 2m array (small shapes)."""

    def __init__(self, Kgz, Ktf, _t=None):
        self.K = (np.asarray(Kgz), np.asarray(Ktf))
        self.n, self.m = self.K[0].shape
        if _t is None:
            self.wm = np.concatenate([np.sqrt((K * K).sum(axis=0)) for K in self.K])
            self.std = tuple(float(np.std(K)) for K in self.K)
            self.s = self.std[0] / self.std[1]
        self._t = _t
        self.shape = (2 * self.n, 2 * self.m) if _t is None else (2 * self.m, 2 * self.n)

    @property
    def T(self):
        t = Blocks(*self.K, _t=self)
        t.wm, t.std, t.s = self.wm, self.std, self.s
        return t

    def __matmul__(self, v):
        n, m, wb = self.n, self.m, (1.0, self.s)
        v = np.asarray(v, dtype=np.float64)
        if self._t is None:
            xs = v / self.wm
            return np.concatenate([wb[b] * (self.K[b] @ xs[b * m:(b + 1) * m]) for b in range(2)])
        return np.concatenate([wb[b] * (self.K[b].T @ v[b * n:(b + 1) * n]) for b in range(2)]) / self.wm

    def __array__(self, dtype=None, copy=None):
        n, m = self.n, self.m
        A = np.zeros((2 * n, 2 * m))
        A[:n, :m] = self.K[0] / self.wm[None, :m]
        A[n:, m:] = self.s * self.K[1] / self.wm[None, m:]
        return A


class _Problem(JointHostProblem):
    """crossgrad_host's joint problem on the block operator instead of the stacked array"""

    def __init__(self, op, *a, **kw):
        JointHostProblem.__init__(self, np.zeros((1, 1)), *a, **kw)
        self.Aw = op


def problem(op, name, dobsw, reg, lam, alpha=1.0, beta=0.01):
    return _Problem(op, dobsw, op.wm, mesh_shape(name), reg, alpha, beta, 0.01 * op.wm, lam, spacing(name), CG_SCALE)


# ------------------------------------------------------------------------------------------ the forward's plan

def forward_plan(cells, obs, cus):
    """How the forward pass cuts the table's 2 nz layers into chunks on a device of `cus` compute units: (layers per
    chunk of the planning formula every table has, the chunks that formula makes of 2 nz layers as they lie -- lists of
    layers --, the joint store's chunks, cut per property).  host_lattice.h: lat_plan, lattice_build."""
    nx, ny, nz = cells
    px, qy = obs
    nob = (qy + 7) // 8
    nobt = min(64, nob)
    TR = max(1, min(64 // nobt, px))
    FT = (nob + nobt - 1) // nobt
    gx_fwd = (px + TR - 1) // TR * FT
    L = 2 * nz
    want = max(1, min(L, (4 * cus + gx_fwd - 1) // gx_fwd))
    lpc = (L + want - 1) // want
    plain = [list(range(c, min(L, c + lpc))) for c in range(0, L, lpc)]
    lpj = min(lpc, nz)
    joint = [list(range(b * nz + c, min((b + 1) * nz, b * nz + c + lpj))) for b in range(2) for c in range(0, nz, lpj)]
    return lpc, plain, joint


# ------------------------------------------------------------------------------------------ the passes, restated

MISTAKES = ("blocks' residuals swapped", "s left out of the forward", "s left out of the adjoint", "tf table for both")


def gradient(op, x, dobsw, mistake=None, across=None):
    """2 Aw^T (Aw x - dobsw) of the joint store as the two passes form it, or with one of MISTAKES made on the way;
    across = (nz, layer): the forward's chunk that holds `layer` of the density summed into the tf block's slab rows (a
    chunking that ignores the boundary between the properties; the cells lie layer-major)."""
    n, m, s, wm = op.n, op.m, op.s, op.wm
    Kgz, Ktf = op.K
    if mistake == "tf table for both":
        Kgz = Ktf
    xs = np.asarray(x) / wm
    sf = 1.0 if mistake == "s left out of the forward" else s
    d = [Kgz @ xs[:m], sf * (Ktf @ xs[m:])]
    if across is not None:
        nz, layer = across
        sel = np.zeros(m, dtype=bool)
        sel.reshape(nz, -1)[layer] = True
        part = Kgz[:, sel] @ xs[:m][sel]
        d = [d[0] - part, d[1] + sf * part]
    r = [d[0] - dobsw[:n], d[1] - dobsw[n:]]
    if mistake == "blocks' residuals swapped":
        r = r[::-1]
    sa = 1.0 if mistake == "s left out of the adjoint" else s
    return 2.0 * np.concatenate([Kgz.T @ r[0], sa * (Ktf.T @ r[1])]) / wm


# ------------------------------------------------------------------------------------------ data and chains

def case_data(op, seed=7):
    """(dobs_gz, dobs_tf, dobsw, a test point) of a store: a compact body's fields with 0.1 % noise"""
    n, m = op.n, op.m
    rng = np.random.default_rng(seed)
    body = rng.choice(m, max(1, m // 8), replace=False)
    rho, kap = np.zeros(m), np.zeros(m)
    rho[body], kap[body] = 0.4, 0.02
    d = [op.K[0] @ rho, op.K[1] @ kap]
    dobs = [v + 1e-3 * np.abs(v).max() * rng.normal(size=n) for v in d]
    dobsw = np.concatenate([dobs[0], op.s * dobs[1]])
    xt = rng.uniform(-1.0, 1.0, 2 * m) * op.wm
    return dobs[0], dobs[1], dobsw, xt


#: Step sizes of the chains, chosen on the CPU with JointHostProblem alone on host_kernels' blocks
#: (test_lattice_joint_host checks what they were chosen for: accepted, rejected and clamped trajectories, no
#: Metropolis decision within 1e-6, and trajectories that do not amplify rounding beyond the suite's bound: entries
#: perturbed by 1e-15 move no state by more than 1e-11).  (the coupling off, on)
DT = {"4,9,3 / 5,8": {"Damping": (0.06, 0.06), "MS": (0.05, 0.05), "Smoothness": (0.06, 0.05), "TV": (0.06, 0.06)},
      "shuffled 4,5,3 / 6,7": {"Damping": (0.06, 0.06), "MS": (0.03, 0.03), "Smoothness": (0.05, 0.06), "TV": (0.06, 0.06)}}
MMAX = 1.5
#: the stiffer cases reach no bound of MMAX at a step they accept: theirs are narrower
BOUNDS = {("4,9,3 / 5,8", "MS"): 0.5, ("shuffled 4,5,3 / 6,7", "Damping"): 0.5, ("shuffled 4,5,3 / 6,7", "MS"): 0.2,
          ("shuffled 4,5,3 / 6,7", "Smoothness"): 0.5, ("shuffled 4,5,3 / 6,7", "TV"): 0.5}


def chain_case(K, name, reg, lam):
    """The chain of a shape from its unweighted blocks K = (K_gz, K_tf): (the store, dobsw, the problem, low, high, x0,
    the ten trajectories (L = 2..6 twice), a test point, dt)"""
    op = Blocks(*K)
    _, _, dobsw, xt = case_data(op)
    P = problem(op, name, dobsw, reg, lam)
    mmax = BOUNDS.get((name, reg), MMAX)
    low, high = -mmax * op.wm, mmax * op.wm
    x0 = 0.01 * op.wm
    rng = np.random.default_rng(17)
    trajs = [(L, rng.normal(size=2 * op.m) * 0.6 * op.wm, float(rng.uniform())) for L in (2, 3, 4, 5, 6, 2, 3, 4, 5, 6)]
    return op, dobsw, P, low, high, x0, trajs, xt * mmax, DT[name][reg][1 if lam > 0 else 0]


def run_chain(P, x0, trajs, dt, low, high):
    """the ten trajectories on the host: [(accepted, out5, x, Phi)], accepted, accepted states on a bound, the smallest
    distance of a Metropolis decision from its threshold"""
    out, x = [], x0
    for L, p0, u in trajs:
        x, acc, o, phi, _ = P.leapfrog(x, p0, dt, L, low, high, u)
        out.append((acc, o, x.copy(), phi))
    accepted = sum(bool(a) for a, _, _, _ in out)
    clamps = sum(int(a and (np.any(x == low) or np.any(x == high))) for a, _, x, _ in out)
    margin = min(abs(np.log(u) + (o[4] - o[3])) for (_, _, u), (_, o, _, _) in zip(trajs, out))
    return out, accepted, clamps, margin


def joint_engine(G, obs, b6, table):
    """a built joint engine on the dense store (gh_set_cells_joint) or on the table (gh_set_cells_joint_table)"""
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(2 * obs.shape[1], 2 * b6.shape[0])
    eng.set_cells(b6, _lib.CELL_PRISM_JOINT, direction=direction(), **(dict(translation_invariant=True) if table else {}))
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    return eng


def scalar_engine(G, obs, b6, field):
    """a built scalar engine on the table: "gz" (gh_set_cells_prism) or "tf" (gh_set_cells_tf)"""
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(obs.shape[1], b6.shape[0])
    eng.set_translation_invariant(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    if field == "gz":
        eng.set_cells(b6, _lib.CELL_PRISM)
    else:
        eng.set_cells(b6, _lib.CELL_PRISM_TF, direction=direction())
    eng.build_G()
    return eng
