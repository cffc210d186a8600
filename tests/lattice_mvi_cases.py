"""Geometries, host kernels and chain cases of the magnetization-vector store on the translation-invariant table
(test_lattice_mvi_host.py, test_gpu_lattice_mvi.py): the axis of a column as one more layer coordinate.

The table of a data block has 3 nz layers, layer L = ax nz + k, and cell_of[L][a][b] = ax m + cell_of_geometry[k][a][b]:
`axis_maps` and `axis_tables` restate that in NumPy, `host_blocks` evaluates the nine (data component, axis) prism
kernels on the host (the six second derivatives of 1/r summed over the corners, as the device sums them), and
`chain_case` builds the chains the GPU suite runs, whose conditioning the host suite checks without a device."""
import numpy as np

from lattice_cases import detect, geometry
from lattice_multi_cases import expand
from magvecdata_host import VecDataProblem, stack

H7 = 2000.0 / 7
TF_SCALE = 1e-7 * 1e6
INC, DEC = 60.0, 25.0           # (an oblique regional field)
COMP_ROWS = {"bx": (0, 1, 2), "by": (1, 3, 4), "bz": (2, 4, 5)}   # (of the six sums xx, xy, xz, yy, yz, zz)

SHAPES = {
    # the fill: cells nx, ny, nz / stations px, qy
    "3,7,1 / 2,7": dict(cells=(3, 7, 1), obs=(2, 7), zobs=-15.0),
    "4,9,3 / 5,8": dict(cells=(4, 9, 3), obs=(5, 8), first=(-1, 0), zobs=-15.0),
    "corners": dict(cells=(4, 5, 2), obs=(5, 6), frac=(0.0, 0.0), zobs=-40.0),
    "beyond": dict(cells=(4, 5, 2), obs=(7, 8), first=(-2, -1), h=(H7, H7), origin=(317.3, -911.7), zobs=-15.0),
    "shuffled": dict(cells=(4, 5, 3), obs=(6, 7), first=(-1, -1), h=(H7, 150.0), shuffle=5, zobs=-15.0),
    "beyond, exact": dict(cells=(4, 5, 2), obs=(7, 8), first=(-2, -1), h=(128.0, 64.0), origin=(320.0, -912.0), zobs=-15.0),
    "shuffled, exact": dict(cells=(4, 5, 3), obs=(6, 7), first=(-1, -1), h=(125.0, 150.0), shuffle=5, zobs=-15.0),
    # the index arithmetic's edges
    "nz = 1": dict(cells=(3, 7, 1), obs=(4, 7), h=(H7, H7), zobs=-15.0),
    "ny 9 under qy 7": dict(cells=(3, 9, 2), obs=(5, 7), h=(H7, H7), zobs=-15.0),
    "px = 1": dict(cells=(3, 7, 2), obs=(1, 9), first=(1, -1), h=(H7, H7), zobs=-15.0),
}
FILL_SHAPES = ("3,7,1 / 2,7", "4,9,3 / 5,8", "corners", "beyond, exact", "shuffled, exact", "beyond", "shuffled")
#: ... whose coordinates and spacings are binary fractions: every difference corner - station is exact, so ALL pairs of
#: an offset have the same entry bit for bit and the expanded table is the dense store; on the others the pairs of an
#: offset differ by rounding, and a table entry is the dense store's entry of the offset's first pair
EXACT_SHAPES = FILL_SHAPES[:5]
#: (shape, data components, data weights): one to four blocks of distinct weights
EDGE_CASES = (("nz = 1", ("tf",), (1.0,)), ("nz = 1", ("bz", "tf"), (2.0, 0.125)),
              ("ny 9 under qy 7", ("bx", "by", "bz"), (2.0, 1.0, 0.125)),
              ("px = 1", ("by", "tf", "bx"), (0.5, 3.0, 1.0)),
              ("shuffled", ("tf", "bx", "by", "bz"), (2.0, 1.0, 0.125, 3.0)),
              ("4,9,3 / 5,8", ("bx",), (1.5,)))
#: the chains: (shape, data, weights or None for the module's default form)
CHAIN_CASES = {"tf": ("beyond", ("tf",), None),
               "vector": ("4,9,3 / 5,8", ("bx", "by", "bz"), (2.0, 1.0, 0.125)),
               "mixed shuffled": ("shuffled", ("tf", "bz"), (1.0, 3.0))}
REGS = ("Damping", "MS", "Smoothness", "TV")


def direction():
    from gravinv3dhmc_amd import utils
    return tuple(float(v) for v in utils.dircos(INC, DEC))


def shape(name):
    """(obs (3, n), bounds6 (m, 6)) of a named shape"""
    return geometry(**SHAPES[name])


def _safe_atan2(y, x):
    r = np.arctan2(y, x)
    r = np.where((y > 0) & (x < 0), r - np.pi, r)
    r = np.where((y < 0) & (x < 0), r + np.pi, r)
    return np.where(y == 0, 0.0, r)


def _safe_log(x):
    with np.errstate(divide="ignore"):
        return np.where(x == 0, 0.0, np.log(np.where(x == 0, 1.0, x)))


def host_blocks(obs, b6, f=None):
    """K[comp] = (3, n, m): the unit-axis columns of the data components "bx", "by", "bz" (and "tf" along f) of the
    prisms b6 at the points obs, in uT per A/m -- the corner sums of the six second derivatives of 1/r."""
    S = np.zeros((6, obs.shape[1], b6.shape[0]))
    for k in (1, 0):
        dz = b6[None, :, 4 + k] - obs[2][:, None]
        for j in (1, 0):
            dy = b6[None, :, 2 + j] - obs[1][:, None]
            for i in (1, 0):
                dx = b6[None, :, i] - obs[0][:, None]
                sign = -1.0 if ((1 - i) + (1 - j) + (1 - k)) & 1 else 1.0
                r = np.sqrt(dx * dx + dy * dy + dz * dz)
                v = (-_safe_atan2(dz * dy, dx * r), _safe_log(dz + r), _safe_log(dy + r), -_safe_atan2(dz * dx, dy * r),
                     _safe_log(dx + r), -_safe_atan2(dx * dy, dz * r))
                for q in range(6):
                    S[q] += sign * v[q]
    K = {c: np.stack([S[q] for q in rows]) * TF_SCALE for c, rows in COMP_ROWS.items()}
    if f is not None:
        K["tf"] = f[0] * K["bx"] + f[1] * K["by"] + f[2] * K["bz"]
    return K


def axis_maps(col, m):
    """The expanded cell map: layer ax nz + k holds the columns ax m + cell of the geometry's layer k"""
    col = np.asarray(col)
    return np.concatenate([ax * m + col for ax in range(3)])


def representative(obs, b6):
    """(observation, cell) of the pair with the smallest (p, q) of every offset: arrays (nz, U, V)"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nx, ny, nz, px, qy = dims
    k, u, v = np.meshgrid(np.arange(nz), np.arange(nx + px - 1), np.arange(ny + qy - 1), indexing="ij")
    du, dv = u - (nx - 1), v - (ny - 1)
    p, q = np.maximum(du, 0), np.maximum(dv, 0)
    return ool[p * qy + q], col[(k * nx + (p - du)) * ny + (q - dv)]


def axis_tables(K3, obs, b6):
    """The table (3 nz, U, V) of one data block from its unit-axis columns K3 = (3, n, m): the entry of the pair with
    the smallest (p, q) of every offset, axis-major"""
    i, j = representative(obs, b6)
    return np.concatenate([np.asarray(K3[ax])[i, j] for ax in range(3)])


def expand_axes(T, obs, b6):
    """(3, n, m): the unit-axis columns a block's table T (3 nz, U, V) -- or (3, nz, U, V) -- stands for"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    nz = dims[2]
    T = np.asarray(T).reshape(3, nz, T.shape[-2], T.shape[-1])
    return np.stack([expand(T[ax], dims, col, ool) for ax in range(3)])


def mvi_engine(G, obs, b6, data, weights, table, dense_mvi=False):
    """a built magnetization-vector engine: on the table, the dense vector-data store, or (dense_mvi) gh_set_cells_mvi's"""
    eng = G.Engine(len(data) * obs.shape[1], 3 * b6.shape[0])
    if dense_mvi:
        eng.set_cells_mvi(b6, direction())
    else:
        eng.set_cells_mvi_data(b6, direction() if "tf" in data else None, data, np.asarray(weights, dtype=float),
                               **(dict(translation_invariant=True) if table else {}))
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    return eng


#: Step sizes of the chains, chosen on the CPU with VecDataProblem alone on host_blocks' kernels (test_lattice_mvi_host
#: checks what they were chosen for: accepted, rejected and clamped trajectories, no Metropolis decision within 1e-6,
#: and trajectories that do not amplify rounding beyond the suite's bound: entries perturbed by 1e-15, a few ulps as
#: two orders of summation differ, move no state by more than 1e-11 -- steps nearer the stability limit, where nine
#: of ten are still accepted with the coupling on, amplify it to 1e-7)
#: (the coupling off, on): the amplitude term stiffens the potential
DT = {"tf": {"Damping": (0.44, 0.44), "MS": (0.4, 0.38), "Smoothness": (0.4, 0.36), "TV": (0.208, 0.208)},
      "vector": {"Damping": (0.22, 0.17), "MS": (0.2, 0.16), "Smoothness": (0.22, 0.17), "TV": (0.18, 0.14)},
      "mixed shuffled": {"Damping": (0.3, 0.28), "MS": (0.05, 0.05), "Smoothness": (0.28, 0.26), "TV": (0.22, 0.2)}}
LAMBDA, AMP_BETA = 0.02, 1.0
MMAX = 1.5
#: the two stiffest cases reach no bound of MMAX at a step they accept: theirs are narrower
BOUNDS = {("tf", "TV"): 0.5, ("mixed shuffled", "MS"): 0.2}


def chain_case(K, case, reg, lam):
    """The chain of a case from the unit-axis columns K[comp] = (3, n, m) of its data components: (w, wm, dobsw,
    shape3, the problem, low, high, x0, the ten trajectories, a test point, dt)"""
    name, data, weights = CHAIN_CASES[case]
    nx, ny, nz = SHAPES[name]["cells"]
    n, m = K[data[0]].shape[1:]
    shape3 = (1, 1, m) if "shuffle" in SHAPES[name] else (nz, nx, ny)   # (stencils follow the caller's cell order)
    w = np.ones(len(data)) if weights is None else np.asarray(weights, dtype=float)
    Aw, wm, wb, A = stack(K, data, w)
    rng = np.random.default_rng(7)
    truth = np.zeros(3 * m)
    body = rng.choice(m, max(1, m // 8), replace=False)
    for ax, val in enumerate((0.6, -0.9, 0.4)):
        truth[ax * m + body] = val
    d = A @ truth
    dobs = d + 1e-3 * np.abs(d).max() * rng.normal(size=d.size)
    dobsw = wb * dobs
    P = VecDataProblem(Aw, dobsw, len(data), 0.01 * wm, reg, 1.0, 0.01, wm=wm, shape=shape3, lam=lam, amp_beta=AMP_BETA)
    mmax = BOUNDS.get((case, reg), MMAX)
    low, high = -mmax * wm, mmax * wm
    x0 = 0.01 * wm
    trajs = [(L, rng.normal(size=3 * m) * 0.6 * wm, float(rng.uniform())) for L in (2, 3, 4, 5, 6, 2, 3, 4, 5, 6)]
    xt = rng.uniform(-mmax, mmax, 3 * m) * wm
    return w, wm, dobsw, shape3, P, low, high, x0, trajs, xt, DT[case][reg][1 if lam > 0 else 0]


def wrong_kernels(K, data):
    """The kernels of the mistakes the GPU suite must be able to see: {name: K'} -- the axes x and y swapped, the axis z
    dropped, and (where "bx" and "by" are both data) bx's y table used for by's y"""
    out = {"axes swapped": {c: np.asarray(K[c])[[1, 0, 2]] for c in K},
           "axis dropped": {c: np.asarray(K[c]) * np.array([1.0, 1.0, 0.0])[:, None, None] for c in K}}
    if "bx" in data and "by" in data:
        Kw = {c: np.array(K[c]) for c in K}
        Kw["by"][1] = K["bx"][1]
        out["bx's y table for by's y"] = Kw
    return out
