"""Geometries and engines of the multi-component store on the translation-invariant table (test_gpu_lattice_multi.py,
test_lattice_multi_host.py): lattice_cases.geometry's regular prism grids under gridded data, with the shapes of the
single-block suite that the block-aware kernels are looked at on, and the shapes at the blocks' own edges.

The block-aware adjoint runs its steps of four input rows (observation rows p) block after block: a flattened
(block, p) row sequence would put a block boundary inside a step at px = 5 and px = 1 and on a step boundary at
px = 4.  The forward's output rows are the p as well, TR = 64 / ceil(qy / 8) of them per workgroup: qy = 125 gives
TR = 4 under px = 5, a last tile of one row in every block."""
import numpy as np

from lattice_cases import geometry

H7 = 2000.0 / 7

#: the single-block suite's shapes (tests/test_gpu_lattice.py: SHAPES) the block tables are looked at on ...
SHAPES = {
    "beyond": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, H7), origin=(317.3, -911.7)),
    "shuffled": dict(cells=(7, 5, 3), obs=(9, 8), first=(-1, -2), h=(H7, 150.0), shuffle=5),
    "near 1e6": dict(cells=(7, 5, 3), obs=(8, 6), h=(H7, H7), origin=(1.0e6 + 0.3, -1.0e6 - 0.7), frac=(0.0, 0.0)),
    "nx = 1": dict(cells=(1, 5, 3), obs=(4, 5)),
    "layers": dict(cells=(4, 3, 4), obs=(4, 3), tops=(0.0, 30.0, 170.0, 180.5, 1000.0)),
    "R-1": dict(cells=(3, 7, 2), obs=(5, 9), h=(H7, H7)),
    "R+1": dict(cells=(3, 9, 2), obs=(5, 7), h=(H7, H7)),
    "row across 64 lanes": dict(cells=(3, 40, 2), obs=(4, 33), first=(0, 3), h=(H7, H7)),
    "covered row across 64 lanes": dict(cells=(3, 40, 2), obs=(4, 40), h=(H7, H7), tops=(0.0, 300.0, 700.0)),
    # ... and the blocks' edges: one, four and five observation rows; five under an output-row tile of four
    "px = 1": dict(cells=(3, 7, 2), obs=(1, 9), first=(1, -1), h=(H7, H7)),
    "px = 4": dict(cells=(3, 7, 2), obs=(4, 9), first=(0, -1), h=(H7, H7)),
    "px = 5, TR = 4": dict(cells=(3, 9, 2), obs=(5, 125), first=(-1, -58)),
}

TABLE_SHAPES = ("beyond", "shuffled", "near 1e6", "nx = 1", "layers", "R+1", "row across 64 lanes")
EDGE_SHAPES = ("px = 1", "px = 4", "R-1", "px = 5, TR = 4", "R+1", "row across 64 lanes")
CHAIN_SHAPES = ("beyond", "shuffled", "covered row across 64 lanes")

#: every gravity component once: the first C of them are a test's blocks (GH_MULTI_MAX = 11)
ALL_COMPONENTS = ("gz", "gzz", "gxy", "gxx", "gx", "gyy", "potential", "gxz", "gy", "gyz", "geoid")
#: distinct data weights, so that a swapped or missing w_b shows
ALL_WEIGHTS = (2.0, 1.0, 0.125, 3.0, 0.5, 1.5, 0.25, 4.0, 0.75, 5.0, 0.375)


def shape(name):
    """(obs (3, n), bounds6 (M, 6)) of a named shape"""
    return geometry(**SHAPES[name])


def multi_engine(G, obs, b6, comps, weights, table):
    """a built multi-component engine on the dense store or on the translation-invariant table"""
    eng = G.Engine(len(comps) * obs.shape[1], b6.shape[0])
    eng.set_cells_multi(b6, comps, np.asarray(weights, dtype=float), translation_invariant=table)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.build_G()
    return eng


def single_engine(G, obs, b6, comp, table):
    """a built engine of one gravity component (CELL_PRISM_COMP), dense or on the table"""
    eng = G.Engine(obs.shape[1], b6.shape[0])
    if table:
        eng.set_translation_invariant(True)
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, 3, component=comp)
    eng.build_G()
    return eng


def expand(T, dims, col, ool):
    """The n x M kernel a table T (nz, U, V) stands for, in the caller's order of observations and cells (detect's
    cell_of_lat and obs_of_lat): K[obs (p, q), cell (k, a, b)] = T[k][p - a + nx - 1][q - b + ny - 1]."""
    nx, ny, nz, px, qy = dims
    K = np.empty((px * qy, nz * nx * ny))
    p, q = [v.ravel() for v in np.meshgrid(np.arange(px), np.arange(qy), indexing="ij")]
    k, a, b = [v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")]
    K[np.ix_(ool[p * qy + q], col[(k * nx + a) * ny + b])] = T[k[None, :], p[:, None] - a[None, :] + nx - 1,
                                                              q[:, None] - b[None, :] + ny - 1]
    return K


class TableOperator:
    """The weighted stacked kernel Aw = Wb A Wm^-1 of C block tables as an operator (`op @ x`, `op.T @ r`, `op.shape`),
    for a stack too large to expand: the two products are 2-D convolutions of a table's layers (FFT on the host).
    tables: C arrays (nz, U, V); weights: C; dims = (nx, ny, nz, px, qy) and the maps col, ool of lattice_cases.detect."""

    def __init__(self, tables, weights, dims, col, ool, weightfactor=0.5, _t=None):
        from scipy.signal import fftconvolve
        self._conv = fftconvolve
        self.tables, self.w = [np.asarray(T, dtype=np.float64) for T in tables], np.asarray(weights, dtype=np.float64)
        self.dims, self.col, self.ool = tuple(int(v) for v in dims), np.asarray(col), np.asarray(ool)
        nx, ny, nz, px, qy = self.dims
        self.n, self.M = px * qy, nz * nx * ny
        self.shape = (len(self.tables) * self.n, self.M)
        if _t is None:
            # wm: the column norms of Wb A -- the window sums of the squared tables (exact sums, no FFT)
            s = np.zeros((nz, nx, ny))
            for T, w in zip(self.tables, self.w):
                c = np.cumsum(np.cumsum(np.pad(T * T, ((0, 0), (1, 0), (1, 0))), axis=1), axis=2)
                a, b = np.arange(nx)[:, None], np.arange(ny)[None, :]
                u0, v0 = nx - 1 - a, ny - 1 - b      # the window of cell (a, b): u in [u0, u0 + px), v in [v0, v0 + qy)
                s += w * w * (c[:, u0 + px, v0 + qy] - c[:, u0, v0 + qy] - c[:, u0 + px, v0] + c[:, u0, v0])
            wm = np.empty(self.M)
            wm[self.col] = (s ** weightfactor).ravel()
            self.wm = wm
        self._t = _t

    @property
    def T(self):
        t = TableOperator(self.tables, self.w, self.dims, self.col, self.ool, _t=self)
        t.wm, t.shape = self.wm, (self.shape[1], self.shape[0])
        return t

    def __matmul__(self, v):
        nx, ny, nz, px, qy = self.dims
        v = np.asarray(v, dtype=np.float64)
        if self._t is None:        # d = Wb A (x / wm)
            xs = (v / self.wm)[self.col].reshape(nz, nx, ny)
            out = np.empty(self.shape[0])
            for b, (T, w) in enumerate(zip(self.tables, self.w)):
                d = sum(self._conv(T[k], xs[k])[nx - 1:nx - 1 + px, ny - 1:ny - 1 + qy] for k in range(nz))
                blk = np.empty(self.n)
                blk[self.ool] = w * d.ravel()
                out[b * self.n:(b + 1) * self.n] = blk
            return out
        g = np.zeros((nz, nx, ny))  # g = Wm^-1 A^T Wb r
        for b, (T, w) in enumerate(zip(self.tables, self.w)):
            rf = (w * v[b * self.n:(b + 1) * self.n])[self.ool].reshape(px, qy)[::-1, ::-1]
            for k in range(nz):
                g[k] += self._conv(T[k], rf)[px - 1:px - 1 + nx, qy - 1:qy - 1 + ny][::-1, ::-1]
        out = np.empty(self.M)
        out[self.col] = g.ravel()
        return out / self.wm


def table_problem(op, dobsw, ncomp, mwapr, regularization, alpha, beta, wm, shape=None):
    """multicomp_host.MultiProblem on a TableOperator instead of the stacked array: the same potential, data term with
    one mean per block, regularisers and trajectory, with Aw's two products left to the operator."""
    from multicomp_host import MultiProblem

    class TableProblem(MultiProblem):
        def __init__(self):
            self.Aw = op
            self.N, self.M = op.shape
            self.ncomp, self.n = ncomp, self.N // ncomp
            self.dobsw = np.asarray(dobsw, dtype=np.float64)
            self.mwapr = np.asarray(mwapr, dtype=np.float64)
            self.reg, self.alpha, self.beta = regularization, alpha, beta
            self.wm2 = np.asarray(wm, dtype=np.float64) ** 2
            self.shape, self.global_mean = shape, False

    return TableProblem()
