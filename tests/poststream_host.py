"""NumPy restatement of the streaming posterior's arithmetic (csrc/poststream.hip.h), sample by sample and in the
kernel's operation order: what the GPU tests compare the device state with."""
import numpy as np


class Stream(object):
    def __init__(self, chains, M, bins, batch_len, lo, hi):
        self.C, self.M, self.B, self.b = int(chains), int(M), int(bins), int(batch_len)
        self.lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (M,)).copy()
        self.hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (M,)).copy()
        z = lambda: np.zeros((self.C, M))
        self.mean, self.M2, self.bsum, self.bmean, self.bM2 = z(), z(), z(), z(), z()
        self.H = np.zeros((self.B, M), dtype=np.uint32)
        self.n = np.zeros(self.C, dtype=np.int64)
        self.K = np.zeros(self.C, dtype=np.int64)

    def bins_of(self, m):
        lo, hi, B = self.lo, self.hi, self.B
        flat = hi == lo
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (m - lo) / (hi - lo) * B
        k = np.clip(np.floor(np.where(flat, 0.0, t)), 0, B - 1).astype(np.int64)
        return np.where(flat, 0, k)

    def add(self, c, m):
        """One unweighted sample m (M values) of chain slot c."""
        m = np.asarray(m, dtype=np.float64)
        self.n[c] += 1
        n = float(self.n[c])
        d = m - self.mean[c]
        self.mean[c] = self.mean[c] + d / n
        self.M2[c] = self.M2[c] + d * (m - self.mean[c])
        self.bsum[c] = self.bsum[c] + m
        if self.n[c] % self.b == 0:
            self.K[c] += 1
            y = self.bsum[c] / float(self.b)
            e = y - self.bmean[c]
            self.bmean[c] = self.bmean[c] + e / float(self.K[c])
            self.bM2[c] = self.bM2[c] + e * (y - self.bmean[c])
            self.bsum[c] = 0.0
        self.H[self.bins_of(m), np.arange(self.M)] += 1

    def add_x(self, c, x, wm):
        """A weighted state x = wm m: the model value with the stored reciprocal (ring_store_kernel's bits)."""
        self.add(c, np.asarray(x, dtype=np.float64) * (1.0 / np.asarray(wm, dtype=np.float64)))

    def read(self):
        nan = np.full(self.M, np.nan)
        rec = [c for c in range(self.C) if self.n[c] > 0]
        out = {"n_per_chain": self.n.copy(), "chain_mean": self.mean.copy(), "chain_M2": self.M2.copy()}
        if not rec:
            out.update(mean=nan, std=nan.copy(), rhat=nan.copy(), ess=nan.copy())
            return out
        ntot = float(sum(self.n[c] for c in rec))
        sm = np.zeros(self.M)
        for c in rec:
            sm = sm + float(self.n[c]) * self.mean[c]
        pm = sm / ntot
        q = np.zeros(self.M)
        for c in rec:
            q = q + self.M2[c]
        for c in rec:
            d = self.mean[c] - pm
            q = q + float(self.n[c]) * (d * d)
        out["mean"], out["std"] = pm, np.sqrt(q / ntot)
        rhat = nan.copy()
        n0 = int(self.n[rec[0]])
        if len(rec) >= 2 and all(self.n[c] == n0 for c in rec) and n0 >= 2:
            nn = float(n0)
            W, cm = np.zeros(self.M), np.zeros(self.M)
            for c in rec:
                W = W + self.M2[c] / (nn - 1.0)
                cm = cm + self.mean[c]
            W, cm = W / len(rec), cm / len(rec)
            v = np.zeros(self.M)
            for c in rec:
                d = self.mean[c] - cm
                v = v + d * d
            Bv = nn * (v / (len(rec) - 1))
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.sqrt(((nn - 1.0) / nn * W + Bv / nn) / W)
            rhat = np.where(W != 0.0, r, np.nan)
        out["rhat"] = rhat
        ess = np.zeros(self.M)
        for c in rec:
            ec = nan.copy()
            if self.K[c] >= 2:
                den = float(self.b) * self.bM2[c] / float(self.K[c] - 1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    e = float(self.n[c]) * (self.M2[c] / float(self.n[c] - 1)) / den
                ec = np.where(den != 0.0, e, np.nan)
            ess = ess + ec
        out["ess"] = ess
        return out

    def quantiles(self, qs):
        qs = np.atleast_1d(np.asarray(qs, dtype=np.float64))
        ntot = int(self.n.sum())
        out = np.full((qs.size, self.M), np.nan)
        if ntot == 0:
            return out
        H = self.H.astype(np.int64)
        cum = np.cumsum(H, axis=0)
        for iq, q in enumerate(qs):
            target = q * float(ntot)
            for j in range(self.M):
                lo, hi = self.lo[j], self.hi[j]
                if hi == lo:
                    out[iq, j] = lo
                    continue
                for k in range(self.B):
                    h = int(H[k, j])
                    if h != 0 and (float(cum[k, j]) >= target or cum[k, j] == ntot):
                        before = float(cum[k, j] - h)
                        out[iq, j] = lo + (float(k) + (target - before) / float(h)) * (hi - lo) / float(self.B)
                        break
        return out


def gelman_rubin(chains):
    """Textbook potential scale reduction of equally long chains, (C, n, M) -> M."""
    chains = np.asarray(chains, dtype=np.float64)
    n = chains.shape[1]
    W = chains.var(axis=1, ddof=1).mean(axis=0)
    Bv = n * chains.mean(axis=1).var(axis=0, ddof=1)
    return np.sqrt(((n - 1) / n * W + Bv / n) / W)


def batch_means_ess(rows, b):
    """n var / (b var of the means of the complete batches of length b), (n, M) -> M."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    K = n // b
    y = rows[:K * b].reshape(K, b, -1).mean(axis=1)
    return n * rows.var(axis=0, ddof=1) / (b * y.var(axis=0, ddof=1))


def close(a, b, scale, tol=1e-12):
    """|a - b| <= tol max(|b|, scale) where both are numbers; the NaN patterns equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= tol * np.maximum(np.abs(b[ok]), scale)))
