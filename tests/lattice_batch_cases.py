"""What the chain batch on the translation-invariant store is checked against (test_lattice_batch_host.py,
test_gpu_lattice_batch.py): a NumPy restatement of csrc/latbatch.hip.h -- the two gathers, the correlation over
X[M][16], the plan of the two passes -- and the suite's geometries and draws.  Geometry comes from lattice_cases."""
import numpy as np

from lattice_cases import detect, geometry  # noqa: F401  (geometry: re-exported to the suites)

CB = 16
TR, RW, NT, MAX_CHUNKS = 8, 2, 4, 32
LDS_MAX = 160 * 1024
H7 = 2000.0 / 7

#: the passes' edges.  (ny, qy) is the adjoint's (outputs, inputs) and the forward's (inputs, outputs) along the fast axis
#: 7 / 8 / 9: the gathers' padding to 8; 15 / 16 / 17: one MFMA tile of outputs; 63 / 64 / 65: the four tiles of a wave
#: and the second workgroup along y (a table row across 64 lanes)
PASS_CASES = {
    "y7": dict(cells=(3, 7, 2), obs=(4, 7)),
    "y8": dict(cells=(3, 8, 2), obs=(4, 8)),
    "y9": dict(cells=(3, 9, 2), obs=(4, 9)),
    "y15": dict(cells=(3, 15, 2), obs=(4, 15)),
    "y16": dict(cells=(3, 16, 2), obs=(4, 16)),
    "y17": dict(cells=(3, 17, 2), obs=(4, 17)),
    "y63": dict(cells=(2, 63, 1), obs=(3, 63)),
    "y64": dict(cells=(2, 64, 1), obs=(3, 64)),
    "y65": dict(cells=(2, 65, 1), obs=(3, 65)),
    # the last extent the batch tile holds: 192 x 832 + 64 x 64 bytes are the 160 KB of a workgroup to the byte
    "y832": dict(cells=(1, 832, 1), obs=(1, 832)),
    "ny17 under qy7": dict(cells=(3, 17, 2), obs=(4, 7), first=(0, 5)),
    "px = 1": dict(cells=(3, 9, 2), obs=(1, 9), first=(1, 0)),
    "nx = 1": dict(cells=(1, 9, 2), obs=(4, 9)),
    "nz = 1": dict(cells=(3, 9, 1), obs=(4, 9)),
    "rows beyond one tile": dict(cells=(11, 9, 2), obs=(10, 9)),
    "layers per chunk": dict(cells=(2, 5, 33), obs=(3, 5), tops=tuple(20.0 * np.arange(34))),
    "beyond": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, H7), origin=(317.3, -911.7)),
    "corners": dict(cells=(7, 5, 3), obs=(8, 6), frac=(0.0, 0.0)),
    "shuffled": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, 150.0), shuffle=5),
}
#: 130 x 130 stations over 20 x 20 x 2 cells: 16 900 rows, N not a multiple of 16
BIG = dict(cells=(20, 20, 2), obs=(130, 130), first=(-55, -55))
#: the chains' shapes (every cell row under observations: the gradient is the weighted kernel's)
CHAIN_CASES = ("beyond", "shuffled", "y17")
#: extents along y the batch tile cannot hold, which the single-chain table takes: the first one (833 pads to 840:
#: 192 x 840 + 64 x 64 bytes), 848 stations over 64 cells (192 x 848 + 64 x 64), far
REFUSED_CASES = {
    "y833": dict(cells=(1, 833, 1), obs=(1, 833)),
    "qy848 over ny64": dict(cells=(1, 64, 1), obs=(1, 848), first=(0, -392)),
    "y1300": dict(cells=(1, 1300, 1), obs=(1, 1300)),
}
#: ... and the last ones it holds: to the byte the 160 KB of a workgroup (192 x 832 + 64 x 64, 192 x 848 + 64 x 16), which
#: fit only because the kernel has no static LDS beside its tile; 840 stations over 32 cells is 192 x 840 + 64 x 32
FITTING_EDGES = {
    "y832": (1, 832, 1, 1, 832),
    "qy840 over ny32": (1, 32, 1, 1, 840),
    "qy848 over ny16": (1, 16, 1, 1, 848),
}


def lattice(obs, b6):
    """dims (nx, ny, nz, px, qy), cell_of_lat, obs_of_lat"""
    rc, dims, _, col, _, ool = detect(obs, b6)
    assert rc == 0
    return dims, col, ool


def table_of(A, dims, col, ool):
    """T[k][u][v]: the entry of A (N x M, unweighted) of the pair with the smallest (p, q) of every offset"""
    nx, ny, nz, px, qy = dims
    k, u, v = np.meshgrid(np.arange(nz), np.arange(nx + px - 1), np.arange(ny + qy - 1), indexing="ij")
    du, dv = u - (nx - 1), v - (ny - 1)
    p, q = np.maximum(du, 0), np.maximum(dv, 0)
    return np.ascontiguousarray(A[ool[p * qy + q], col[(k * nx + (p - du)) * ny + (q - dv)]])


def expanded(T, dims, col, ool):
    """The dense operator the table stands for, N x M in the caller's orders"""
    nx, ny, nz, px, qy = dims
    p, q, k, a, b = np.meshgrid(np.arange(px), np.arange(qy), np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")
    K = T[k, p - a + nx - 1, q - b + ny - 1].reshape(px * qy, nz * nx * ny)
    A = np.empty_like(K)
    A[np.ix_(ool, col)] = K
    return A


def rt_offset(i, c):
    p, q = i >> 4, i & 15
    return (((p * 2 + (q >> 3)) * 4 + ((q & 7) >> 1)) * CB + c) * 2 + (q & 1)


def to_rt(R16, ld):
    """R[N][16] -> the batch's patch-transposed residuals (ld x 16 doubles), as batch_finish_kernel writes them"""
    Rt = np.zeros(ld * CB)
    i, c = np.meshgrid(np.arange(R16.shape[0]), np.arange(CB), indexing="ij")
    Rt[rt_offset(i, c)] = R16
    return Rt


def gather_x(X16, iw, dims, col):
    """latb_gather_x_kernel: xl16[nz][nx][nyp][16], zero beyond ny"""
    nx, ny, nz, px, qy = dims
    nyp = (ny + 7) // 8 * 8
    xl = np.zeros((nz * nx, nyp, CB))
    xl[:, :ny, :] = (X16[col] * iw[col][:, None]).reshape(nz * nx, ny, CB)
    return xl.reshape(nz, nx, nyp, CB)


def gather_r(Rt, dims, ool):
    """latb_gather_r_blocks_kernel with one block of weight 1: rl16[px][qyp][16], zero beyond qy"""
    nx, ny, nz, px, qy = dims
    qyp = (qy + 7) // 8 * 8
    rl = np.zeros((px, qyp, CB))
    i, c = np.meshgrid(ool, np.arange(CB), indexing="ij")
    rl[:, :qy, :] = Rt[rt_offset(i, c)].reshape(px, qy, CB)
    return rl


def correlate(row, in16, n_out, const, fwd):
    """out[o][c] = sum_i row[+-(i - o) + const] in[i][c] over the padded inputs (values beyond the row count as zero)"""
    n_in = in16.shape[0]
    d = np.arange(n_in)[None, :] - np.arange(n_out)[:, None]
    v = (-d if fwd else d) + const
    ok = (v >= 0) & (v < row.size)
    return np.where(ok, row[np.clip(v, 0, row.size - 1)], 0.0) @ in16


def forward16(T, X16, iw, dims, col, ool):
    """D[N][16] in the caller's order: layers, cell rows a, cells b ascending"""
    nx, ny, nz, px, qy = dims
    xl = gather_x(X16, iw, dims, col)
    D = np.zeros((px, qy, CB))
    for k in range(nz):
        for p in range(px):
            for a in range(nx):
                D[p] += correlate(T[k, p - a + nx - 1], xl[k, a], qy, ny - 1, True)
    out = np.empty((px * qy, CB))
    out[ool] = D.reshape(px * qy, CB)
    return out


def adjoint16(T, Rt, dims, col, ool):
    """S[M][16] in the caller's order (before the division by wm): observation rows p, observations q ascending"""
    nx, ny, nz, px, qy = dims
    rl = gather_r(Rt, dims, ool)
    S = np.zeros((nz, nx, ny, CB))
    for k in range(nz):
        for a in range(nx):
            for p in range(px):
                S[k, a] += correlate(T[k, p - a + nx - 1], rl[p], ny, ny - 1, False)
    out = np.empty((nz * nx * ny, CB))
    out[col] = S.reshape(-1, CB)
    return out


def pass_plan(n_out, n_in_padded):
    ntiles = (n_out + 15) // 16
    FT = (ntiles + NT - 1) // NT
    WT = 16 * ((ntiles + FT - 1) // FT)
    WL = n_in_padded + WT
    # (all of a pass's LDS: the kernel has no static array beside its tile)
    return dict(ntiles=ntiles, FT=FT, WT=WT, WL=WL, lds=(TR * WL + CB * n_in_padded) * 8)


def plan(dims, cus):
    """latb_plan restated: what Engine.translation_invariant_batch_plan() must return for these extents"""
    nx, ny, nz, px, qy = dims
    nyp, qyp = (ny + 7) // 8 * 8, (qy + 7) // 8 * 8
    adj, fwd = pass_plan(ny, qyp), pass_plan(qy, nyp)
    adj["grid"] = (nx + TR - 1) // TR * adj["FT"]
    fwd["grid"] = (px + TR - 1) // TR * fwd["FT"]
    want = max(1, min(nz, MAX_CHUNKS, (4 * cus + fwd["grid"] - 1) // fwd["grid"]))
    lpc = (nz + want - 1) // want
    d = dict(on=True, fits=adj["lds"] <= LDS_MAX and fwd["lds"] <= LDS_MAX, TR=TR, RW=RW, NT=NT, max_chunks=MAX_CHUNKS,
             cus=cus, lpc=lpc, chunks=(nz + lpc - 1) // lpc, pp_rows=adj["grid"] * nz)
    for name, p in (("adj", adj), ("fwd", fwd)):
        for key, val in p.items():
            d["%s_%s" % (name, key)] = val
    return d


# ------------------------------------------------------------------------------------------------ the chains' draws

#: step sizes at which the oracle accepts some of a case's 64 trajectories and rejects others, each with a Metropolis
#: margin of 1e-3 or more (test_lattice_batch_host.py checks both on the CPU)
DT = {"Damping": 0.4, "Smoothness": 0.4, "TV": 0.2, "MS": 0.04}
N_ROUNDS = 4


def chain_problem(name, reg, Aw, wm, seed=7):
    """dobs, shape, low, high, x0 and the draws of a chain case: rounds[t] = (L (16), p0s (16, M), us (16)); different L
    per chain, so that phases mix in one launch"""
    kw = PASS_CASES[name]
    N, M = Aw.shape
    nx, ny, nz = kw["cells"]
    shape = (1, 1, M) if "shuffle" in kw else (nz, nx, ny)  # (stencils follow the caller's cell order)
    rng = np.random.default_rng(seed)
    rho = np.zeros(M)
    rho[rng.choice(M, max(1, M // 10), replace=False)] = 0.03
    d0 = Aw @ (wm * rho)
    dobs = d0 + 1e-3 * np.abs(d0).max() * rng.normal(size=N)
    low, high = 0.0 * wm, 0.05 * wm
    rounds = []
    for t in range(N_ROUNDS):
        L = [2 + (c + t) % 5 for c in range(CB)]
        rounds.append((L, rng.normal(size=(CB, M)) * 0.02 * wm, rng.uniform(size=CB)))
    return dict(dobs=dobs, shape=shape, low=low, high=high, x0=0.001 * wm, mwapr=0.001 * wm, rounds=rounds, dt=DT[reg])


def oracle_chains(P, prob, C):
    """The oracle's trajectories of chains 0 .. C - 1: per round accepted (C), out5 (C, 5), x (C, M); and the smallest
    Metropolis margin |log u + (Hnew - Hcur)| met"""
    xs = [prob["x0"].copy() for _ in range(C)]
    out, margin = [], np.inf
    for L, p0s, us in prob["rounds"]:
        acc, o5 = [], []
        for c in range(C):
            xs[c], a, o, _ = P.leapfrog(xs[c], p0s[c], prob["dt"], L[c], prob["low"], prob["high"], float(us[c]))
            margin = min(margin, abs(np.log(us[c]) + (o[4] - o[3])))
            acc.append(a)
            o5.append(o)
        out.append((np.array(acc), np.array(o5), np.array(xs)))
    return out, margin
