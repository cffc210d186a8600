"""CPU suite: the paired sweep's row order (gh_fold_pair_rows, csrc/host_fold.h: the folded rows folded over the
diagonal reflection tau as well) against a NumPy restatement built from fold_oracle_cases.Symmetry, and the
row-paired operator of csrc/fold.hip.h restated in NumPy on a permuted host copy of the folded blocks against the
eight-image mean of Aw.

Observation grids n x n over cells (4, 4, 3): q = n / 2 a side of the quadrant, nF = q^2 folded rows, q of them their
own partner (the quadrant's diagonal), q (q - 1) / 2 pairs.  n = 2: nF = 1; 4: one pair and two diagonal rows; 62, 64:
496 and 528 pairs around the 512 slots of one pair slot per thread; 88, 90: 990 and 1035 around the 1024 of two;
100: the benchmark's 1225 pairs, 201 of them split."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)
from fold_oracle_cases import Symmetry, geometry
from helpers import relmax

SIDES = (2, 4, 6, 44, 62, 64, 88, 90, 92, 100)
CELLS = (4, 4, 3)
TT = 512
SWAP = np.array([0, 2, 1, 3])
XOR = np.array([[k ^ q for k in range(4)] for q in range(4)])      # XOR[q, k] = k ^ q
FOLD_ON, PAIR_ON = 0, 0


def plan_from_library(obs, b6):
    from gravinv3dhmc_amd import _lib
    lib = _lib.load()
    N, M = obs.shape[1], b6.shape[0]
    ldF = (N // 4 + 15) // 16 * 16
    rows, slots, reason = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    code = np.full(ldF, -7, dtype=np.int32)
    ptab = np.full(6 * TT * 4, -7, dtype=np.int32)
    counts = np.full(3, -7, dtype=np.int64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    x, y, z = (np.ascontiguousarray(obs[k]) for k in range(3))
    b6 = np.ascontiguousarray(b6)
    rc = lib.gh_fold_pair_rows(N, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), M,
                               b6.ctypes.data_as(dp), ctypes.byref(rows), ctypes.byref(slots), code.ctypes.data_as(ip),
                               ptab.ctypes.data_as(ip), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                               ctypes.byref(reason))
    assert rc == FOLD_ON and reason.value == PAIR_ON, (rc, reason.value)
    cols = 2 * (rows.value - slots.value)
    assert np.all(ptab[cols * TT * 4:] == -7)                     # nothing written past the table
    return rows.value, slots.value, code, ptab[:cols * TT * 4].reshape(cols, TT, 4), tuple(int(c) for c in counts)


class Rows(object):
    """rho and c of every folded row from the permutations alone: tau obs_img[f][0] = obs_img[rho f][c_f]."""

    def __init__(self, sym):
        self.img = img = sym.obs_img
        self.nF = nF = img.shape[0]
        self.ldF = (nF + 15) // 16 * 16
        place = np.empty(img.size, dtype=np.int64)
        place[img.ravel()] = np.arange(img.size)
        at = place[sym.obs_tau[img[:, 0]]]
        self.rho, self.c = at >> 2, at & 3
        assert np.array_equal(self.rho[self.rho], np.arange(nF))
        # tau s_g f = s_(swap g ^ c_f) rho f
        for g in range(4):
            assert np.array_equal(sym.obs_tau[img[:, g]], img[self.rho, SWAP[g] ^ self.c])
        self.tau_img = sym.obs_tau[img[:, SWAP]]                   # [f][g] = s_g tau f

    def plan(self):
        """the restated plan: rows, pair slots, code, ptab, (pairs in slots, pairs split, self rows)"""
        nF, ldF = self.nF, self.ldF
        rows = -(-ldF // TT)
        P = (rows - 1) // 2
        cols = 2 * (rows - P)
        code = np.full(ldF, -1, dtype=np.int64)
        ptab = np.full((cols, TT, 4), -1, dtype=np.int64)
        pairs = [f for f in range(nF) if self.rho[f] > f]
        selfs = [f for f in range(nF) if self.rho[f] == f]
        lone = []
        for n, f in enumerate(pairs):
            if n < P * TT:
                s, t = divmod(n, TT)
                code[2 * s * TT + t] = 4 * f
                code[(2 * s + 1) * TT + t] = 4 * self.rho[f] + self.c[f]
                ptab[2 * s, t], ptab[2 * s + 1, t] = self.img[f], self.tau_img[f]
            else:
                lone += [f, self.rho[f]]
        n_split = len(lone) // 2
        for n, f in enumerate(lone + selfs):
            l, t = divmod(n, TT)
            assert (2 * P + l) * TT + t < ldF
            code[(2 * P + l) * TT + t] = 4 * f
            ptab[2 * (P + l), t], ptab[2 * (P + l) + 1, t] = self.img[f], self.tau_img[f]
        return rows, P, code, ptab, (min(len(pairs), P * TT), n_split, len(selfs))


@pytest.fixture(scope="module", params=[(n, False) for n in SIDES] + [(6, True), (64, True), (100, True)],
                ids=lambda p: "%d%s" % (p[0], "-shuffled" if p[1] else ""))
def case(request):
    n, shuffle = request.param
    obs, b6 = geometry((n, n), CELLS, shuffle=shuffle)
    sym = Symmetry(obs, b6, True)
    return n, obs, b6, sym, Rows(sym), plan_from_library(obs, b6)


def test_plan_against_restatement(case):
    n, _, _, _, R, (rows, P, code, ptab, counts) = case
    q = n // 2
    want = R.plan()
    assert (rows, P, counts) == (want[0], want[1], want[4])
    assert np.array_equal(code, want[2]) and np.array_equal(ptab, want[3])
    assert rows <= 5 and P == (rows - 1) // 2 and rows * TT >= R.ldF
    n_pairs = q * (q - 1) // 2
    assert counts == (min(n_pairs, P * TT), max(n_pairs - P * TT, 0), q)
    if n == 100:
        assert (rows, P, counts) == (5, 2, (1024, 201, 50)) and counts[1] * 2 + counts[2] == 452
    if n == 2:
        assert (rows, P, counts) == (1, 0, (0, 0, 1)) and code[0] == 0 and np.all(code[1:] == -1)


def test_row_order_properties(case):
    _, _, _, _, R, (rows, P, code, ptab, counts) = case
    live = code >= 0
    # a permutation of the folded rows
    assert np.array_equal(np.sort(code[live] >> 2), np.arange(R.nF))
    row, c = np.where(live, code >> 2, -1), np.where(live, code & 3, 0)
    k, t = np.divmod(np.arange(R.ldF), TT)
    assert k.max() < rows <= 5                                      # never more than five rows per thread
    # pair slots: both rows in one thread, the second as the representative tau f of its orbit
    for s in range(P):
        a, b = row[2 * s * TT:(2 * s + 1) * TT], row[(2 * s + 1) * TT:(2 * s + 2) * TT]
        assert np.array_equal(a >= 0, b >= 0)
        on = a >= 0
        assert np.array_equal(R.rho[a[on]], b[on]) and np.all(a[on] < b[on])
        assert np.all(c[2 * s * TT:(2 * s + 1) * TT] == 0)
        assert np.array_equal(c[(2 * s + 1) * TT:(2 * s + 2) * TT][on], R.c[a[on]])
    # the other rows: unchanged sub-columns; the two rows of a split pair in neighbouring lanes of one row group
    lone = np.flatnonzero(live & (k >= 2 * P))
    assert np.all(c[lone] == 0)
    where = np.full(R.nF, -1)
    where[row[lone]] = lone
    split = [f for f in row[lone] if R.rho[f] != f]
    assert len(split) == 2 * counts[1]
    for f in split:
        n1, n2 = where[f], where[R.rho[f]]
        assert n2 >= 0 and abs(n1 - n2) == 1 and n1 // TT == n2 // TT and min(n1, n2) % 2 == 0
    # the table: the observations of the slot's first row, and their tau images in the order s_g tau f
    for s in range(rows - P):
        kA = 2 * s if s < P else P + s
        for tt in range(TT):
            nA = kA * TT + tt
            f = row[nA] if nA < R.ldF else -1
            if f < 0:
                assert np.all(ptab[2 * s, tt] == -1) and np.all(ptab[2 * s + 1, tt] == -1)
                continue
            assert np.array_equal(ptab[2 * s, tt], R.img[f]) and np.array_equal(ptab[2 * s + 1, tt], R.tau_img[f])
            if s < P:
                f2, c2 = row[nA + TT], c[nA + TT]
                assert np.array_equal(ptab[2 * s + 1, tt], R.img[f2, np.arange(4) ^ c2])


def tsum(S, w):
    """t(S, w)[..., q] = sum_k S[..., k] w[..., k ^ q]"""
    return np.einsum("...k,...qk->...q", S, w[..., XOR])


def test_row_paired_operator_against_eight_image_mean(case):
    """fold.hip.h's sums on a host copy of the blocks in the new row order: adjoint and forward of every work item
    against the mean of Aw over all eight images, to 1e-13."""
    from oracle import oracle
    n, obs, b6, sym, R, (rows, P, code, ptab, _) = case
    N, M = obs.shape[1], b6.shape[0]
    Aw, _ = oracle.col_weight(oracle.prism_gz_kernel(obs[0], obs[1], obs[2], b6), 0.5)
    A8 = sym.mean(Aw)
    rng = np.random.default_rng(n)
    r, x = rng.normal(size=N), rng.normal(size=M)
    NS = rows - P
    kA = np.array([2 * s if s < P else P + s for s in range(NS)])
    pa, pb = ptab[0::2], ptab[1::2]                                  # (NS, 512, 4)
    ra, rb = np.where(pa >= 0, r[pa], 0.0), np.where(pb >= 0, r[pb], 0.0)
    want_adj, want_fwd = A8.T @ r, np.zeros(N)
    got_adj, got_fwd = np.zeros(M), np.zeros(N)
    for o, o2 in sym.work:
        cells = sym.cell_orbit[o]
        S = A8[np.ix_(sym.obs_img[:, 0], cells)]                    # S[o][f][k]: the store's block, mirror order
        Sp = np.zeros((rows * TT, 4))
        live = np.flatnonzero(code >= 0)
        Sp[live] = S[(code[live] >> 2)[:, None], np.arange(4)[None, :] ^ (code[live] & 3)[:, None]]
        Sp = Sp.reshape(rows, TT, 4)
        A = Sp[kA]
        B = np.zeros_like(A)
        B[:P] = Sp[kA[:P] + 1]
        As, Bs = A[..., SWAP], B[..., SWAP]
        dot = (tsum(A, ra) + tsum(B, rb)).sum(axis=(0, 1))
        dot_t = (tsum(As, rb) + tsum(Bs, ra)).sum(axis=(0, 1))[SWAP]
        tcells = sym.cell_tau[cells]
        got_adj[cells] = dot
        xo = np.broadcast_to(x[cells], A.shape)
        if o2 >= 0:
            got_adj[tcells] = dot_t
            ys = np.broadcast_to(x[tcells][SWAP], A.shape)
            want_fwd += A8[:, cells] @ x[cells] + A8[:, tcells] @ x[tcells]
        else:
            ys = np.zeros(A.shape)
            want_fwd += A8[:, cells] @ x[cells]
            assert relmax(dot_t, want_adj[tcells]) <= 1e-13       # (its own partner: the same cells, not stored twice)
        da, db = tsum(A, xo) + tsum(Bs, ys), tsum(B, xo) + tsum(As, ys)
        np.add.at(got_fwd, pa[pa >= 0], da[pa >= 0])
        np.add.at(got_fwd, pb[pb >= 0], db[pb >= 0])
    assert relmax(got_adj, want_adj) <= 1e-13
    assert relmax(got_fwd, want_fwd) <= 1e-13
