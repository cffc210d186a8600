"""What the chain batch on the multi-component translation-invariant table is checked against
(test_lattice_multi_batch_host.py, test_gpu_lattice_multi_batch.py): a NumPy restatement of the row-block forms of
csrc/latbatch.hip.h and of batch_finish_blocks_kernel -- the residual gather with w_b, the forward per block into the
stacked rows, the adjoint with the blocks ascending, the finish with one mean per block --, the plan with the block as
the forward's third grid coordinate, and the suite's cases and draws.  Built on lattice_batch_cases (the single-block
restatement) and lattice_multi_cases (components, weights, the table operator)."""
import numpy as np

import lattice_batch_cases as lb
from lattice_batch_cases import BIG, CB, PASS_CASES, correlate, geometry, rt_offset, to_rt  # noqa: F401
from lattice_multi_cases import ALL_COMPONENTS, ALL_WEIGHTS, TableOperator, expand, table_problem  # noqa: F401
from multicomp_host import MultiProblem, stack

#: the passes at the blocks' edges: PASS_CASES geometry -> number of blocks (the first C of ALL_COMPONENTS / ALL_WEIGHTS)
BLOCK_CASES = {
    "y7": 3,                      # 28 rows per block, 84 stacked, ld 96: block boundaries inside Rt patches
    "y8": 2,                      # 32 rows per block: the boundary on a patch edge
    "y17": 2,                     # one MFMA tile + 1
    "y65": 3,                     # the second workgroup along y
    "ny17 under qy7": 2,          # outputs != inputs
    "px = 1": 3,                  # a block is a single input row of the adjoint
    "rows beyond one tile": 2,    # two row tiles in both passes
    "layers per chunk": 2,        # nz = 33: fewer chunks than layers with the block on grid z
    "shuffled": 11,               # every component, the caller's orders permuted, GH_MULTI_MAX blocks
}
#: the chains: shapes, components and weights
CHAIN_CASES = lb.CHAIN_CASES
CHAIN_COMPONENTS = ("gz", "gzz", "gxy")
CHAIN_WEIGHTS = (2.0, 1.0, 0.125)
REGS = ("Damping", "MS", "Smoothness", "TV")
#: step sizes at which the restatement accepts some of a case's 64 trajectories and rejects others, each with a
#: Metropolis margin of 1e-3 or more (test_lattice_multi_batch_host.py checks both on the CPU).  Started from
#: lattice_batch_cases.DT and lowered there until the restatement alone met the condition at all three shapes: the tensor
#: blocks in Eotvos make the column norms (40 .. 370) and with them the potential far steeper than gz's alone, the MS
#: term -- wm^2 v^2 / (v^2 + beta) -- most of all
DT = {"Damping": 0.02, "Smoothness": 0.01, "TV": 0.01, "MS": 2e-5}


# ------------------------------------------------------------------------------------------------ the kernels (host)

_G = 0.00000006673
_SCALE = dict({c: _G * 1000000000.0 for c in ("gxx", "gxy", "gxz", "gyy", "gyz", "gzz")}, potential=_G, geoid=_G / 9.80,
              gx=_G * 100000.0, gy=_G * 100000.0, gz=_G * 100000.0)


def _atan2(y, x):
    """the prism formulas' arctangent: quadrant-folded, 0 at y = 0"""
    r = np.arctan2(y, x)
    r = np.where((y > 0) & (x < 0), r - np.pi, r)
    r = np.where((y < 0) & (x < 0), r + np.pi, r)
    return np.where(y == 0, 0.0, r)


def _log(x):
    with np.errstate(divide="ignore"):
        return np.where(x == 0, 0.0, np.log(np.where(x == 0, 1.0, x)))


def prism_kernel(comp, obs, b6):
    """The n x M kernel of a gravity field (a name of ALL_COMPONENTS) of the prisms b6 at the points obs (3, n), density 1,
    in the product's units: the closed-form corner sums (Nagy et al. 2000).  The points of the suite's geometries lie on
    no edge's line."""
    px, py, pz = [v[:, None] for v in obs]
    K = np.zeros((obs.shape[1], b6.shape[0]))
    for k, zc in enumerate((b6[:, 5], b6[:, 4])):
        for j, yc in enumerate((b6[:, 3], b6[:, 2])):
            for i, xc in enumerate((b6[:, 1], b6[:, 0])):
                dx, dy, dz = xc[None, :] - px, yc[None, :] - py, zc[None, :] - pz
                r = np.sqrt(dx * dx + dy * dy + dz * dz)
                if comp in ("potential", "geoid"):
                    v = (dx * dy * _log(dz + r) + dy * dz * _log(dx + r) + dx * dz * _log(dy + r)
                         - 0.5 * dx * dx * _atan2(dz * dy, dx * r) - 0.5 * dy * dy * _atan2(dz * dx, dy * r)
                         - 0.5 * dz * dz * _atan2(dx * dy, dz * r))
                else:
                    v = {"gx": lambda: -(dy * _log(dz + r) + dz * _log(dy + r) - dx * _atan2(dz * dy, dx * r)),
                         "gy": lambda: -(dz * _log(dx + r) + dx * _log(dz + r) - dy * _atan2(dx * dz, dy * r)),
                         "gz": lambda: -(dx * _log(dy + r) + dy * _log(dx + r) - dz * _atan2(dx * dy, dz * r)),
                         "gxx": lambda: -_atan2(dz * dy, dx * r), "gxy": lambda: _log(dz + r),
                         "gxz": lambda: _log(dy + r), "gyy": lambda: -_atan2(dz * dx, dy * r),
                         "gyz": lambda: _log(dx + r), "gzz": lambda: -_atan2(dx * dy, dz * r)}[comp]()
                K += (-1.0 if (i + j + k) & 1 else 1.0) * v
    return K * _SCALE[comp]


# ------------------------------------------------------------------------------------------------ the block forms

def gather_r_blocks(Rt, w, dims, ool):
    """latb_gather_r_blocks_kernel: rl16[b][px][qyp][16] = w_b Rt[b Nb + obs_of[p, q]][c], zero beyond qy"""
    nx, ny, nz, px, qy = dims
    qyp, Nb = (qy + 7) // 8 * 8, px * qy
    rl = np.zeros((len(w), px, qyp, CB))
    i, c = np.meshgrid(ool, np.arange(CB), indexing="ij")
    for b, wb in enumerate(w):
        rl[b, :, :qy, :] = wb * Rt[rt_offset(b * Nb + i, c)].reshape(px, qy, CB)
    return rl


def forward16_blocks(tables, w, X16, iw, dims, col, ool):
    """D[nb Nb][16]: block b's rows are the single-block forward over T[b] (one gather of X), times w_b"""
    return np.vstack([wb * lb.forward16(T, X16, iw, dims, col, ool) for T, wb in zip(tables, w)])


def adjoint16_blocks(tables, w, Rt, dims, col, ool):
    """S[M][16] in the caller's order (before the division by wm): per (layer, cell row) the blocks ascending, in each
    the observation rows p ascending, into the same sums"""
    nx, ny, nz, px, qy = dims
    rl = gather_r_blocks(Rt, w, dims, ool)
    S = np.zeros((nz, nx, ny, CB))
    for k in range(nz):
        for a in range(nx):
            for b, T in enumerate(tables):
                for p in range(px):
                    S[k, a] += correlate(T[k, p - a + nx - 1], rl[b, p], ny, ny - 1, False)
    out = np.empty((nz * nx * ny, CB))
    out[col] = S.reshape(-1, CB)
    return out


def finish_blocks(D16, dobs_c, nb, ld):
    """batch_finish_blocks_kernel: (Rt (ld x 16, patch-transposed, zero beyond N), data misfit (16), means (16, nb)) of the
    predictions D16 (N, 16) against the centred observations dobs_c (N): one mean per block and chain"""
    N = D16.shape[0]
    Nb = N // nb
    means = D16.reshape(nb, Nb, CB).mean(axis=1)          # (nb, 16)
    R = (D16 - np.repeat(means, Nb, axis=0)) - dobs_c[:, None]
    return to_rt(R, ld), (R * R).sum(axis=0), means.T


def plan(dims, cus, nb):
    """latb_plan on a table of nb blocks: the single block's passes, the forward's chunks planned for nb workgroups per
    chunk and tile; what translation_invariant_batch_plan() must return"""
    d = lb.plan(dims, cus)
    nz = dims[2]
    per = nb * d["fwd_grid"]
    want = max(1, min(nz, lb.MAX_CHUNKS, (4 * cus + per - 1) // per))
    d["lpc"] = (nz + want - 1) // want
    d["chunks"] = (nz + d["lpc"] - 1) // d["lpc"]
    d["blocks"] = nb
    return d


# ------------------------------------------------------------------------------------------------ the passes' round

#: the step of the passes' one round: small enough for the steep stacked potential that the restatement accepts
PASS_DT = 0.002


def pass_round(A, wm, seed=17):
    """The one round of all 16 slots at the blocks' edges, L = 1 .. 3, on the weighted stacked kernel A (an array or an
    operator with @ and shape): dobs (weighted, stacked), mwapr, low, high, x0s, p0s, us, Ls, dt"""
    N, M = A.shape
    rng = np.random.default_rng(seed)
    rho = np.zeros(M)
    rho[rng.choice(M, max(1, M // 10), replace=False)] = 0.03
    d0 = A @ (wm * rho)
    return dict(dobs=d0 + 1e-3 * np.abs(d0).max() * rng.normal(size=N), mwapr=0.001 * wm, low=0.0 * wm, high=0.05 * wm,
                x0s=rng.uniform(0.0, 0.05, (CB, M)) * wm, p0s=rng.normal(size=(CB, M)) * 0.02 * wm, us=rng.uniform(size=CB),
                Ls=[1 + c % 3 for c in range(CB)], dt=PASS_DT)


def pass_reference(P, rnd):
    """the restatement's results of the round, per slot (x, accepted, out5), the smallest Metropolis margin and the number
    accepted"""
    ref = [P.leapfrog(rnd["x0s"][c], rnd["p0s"][c], rnd["dt"], rnd["Ls"][c], rnd["low"], rnd["high"], float(rnd["us"][c]))
           for c in range(CB)]
    margin = min(abs(np.log(rnd["us"][c]) + (ref[c][2][4] - ref[c][2][3])) for c in range(CB))
    return ref, margin, sum(int(r[1]) for r in ref)


# ------------------------------------------------------------------------------------------------ the chains

def chain_setup(name, reg, kernels, weights, seed=7):
    """(Aw, wm, prob) of a chain case on the kernels stacked with the weights: lattice_batch_cases.chain_problem's draws
    with this suite's step sizes; prob["dobs"] are the weighted stacked observations"""
    Aw, wm, _ = stack(kernels, weights)
    prob = lb.chain_problem(name, reg, Aw, wm, seed=seed)
    prob["dt"] = DT[reg]
    return Aw, wm, prob


def problem(Aw, prob, ncomp, reg, wm, **kw):
    return MultiProblem(Aw, prob["dobs"], ncomp, prob["mwapr"], reg, 1.0, 0.01, wm=wm, shape=prob["shape"], **kw)


def chains(P, prob, C):
    """The restatement's trajectories of chains 0 .. C - 1: per round accepted (C), out5 (C, 5), x (C, M); and the smallest
    Metropolis margin |log u + (Hnew - Hcur)| met"""
    xs = [prob["x0"].copy() for _ in range(C)]
    out, margin = [], np.inf
    for L, p0s, us in prob["rounds"]:
        acc, o5 = [], []
        for c in range(C):
            xs[c], a, o = P.leapfrog(xs[c], p0s[c], prob["dt"], L[c], prob["low"], prob["high"], float(us[c]))
            margin = min(margin, abs(np.log(us[c]) + (o[4] - o[3])))
            acc.append(a)
            o5.append(o)
        out.append((np.array(acc), np.array(o5), np.array(xs)))
    return out, margin
