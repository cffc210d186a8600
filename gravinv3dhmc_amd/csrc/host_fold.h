// libgravhmc host side: the stored kernel folded over the grid's two mirrors (fold.hip.h).  Detection of the
// pairing at gh_build_G, eligibility, the lazy build of the folded store, its launches.  Included once by
// gravhmc.hip, after host_sweep.h.
#pragma once

// ------------------------------------------------------------------------------------ detection (host)

namespace fold_detail {

// Sorted clusters of the values of one axis: values closer than tol to their neighbour share a cluster.
struct Axis {
    std::vector<double> lo, hi;
    double tol = 0.0;
    void build(std::vector<double> v, double t)
    {
        tol = t;
        std::sort(v.begin(), v.end());
        for (double x : v) {
            if (lo.empty() || x - hi.back() > tol) {
                lo.push_back(x);
                hi.push_back(x);
            } else {
                hi.back() = x;
            }
        }
    }
    // cluster within tol of x, or -1
    int find(double x) const
    {
        const size_t k = (size_t)(std::upper_bound(lo.begin(), lo.end(), x + tol) - lo.begin());
        if (k == 0) return -1;
        return (x - hi[k - 1] <= tol) ? (int)(k - 1) : -1;
    }
    // cluster of the mirror image 2c - x of each cluster (-1: none); false if some cluster is wider than the
    // tolerance allows or the map is not an involution
    bool mirror(double c, std::vector<int> &m) const
    {
        m.assign(lo.size(), -1);
        for (size_t q = 0; q < lo.size(); ++q) {
            if (hi[q] - lo[q] > 2.0 * tol) return false;
            m[q] = find(2.0 * c - 0.5 * (lo[q] + hi[q]));
        }
        for (size_t q = 0; q < lo.size(); ++q)
            if (m[q] >= 0 && m[(size_t)m[q]] != (int)q) return false;
        return true;
    }
};

typedef std::array<int64_t, 6> Key;

struct Index {
    std::vector<std::pair<Key, int>> v;
    bool build()
    {
        std::sort(v.begin(), v.end());
        for (size_t i = 1; i < v.size(); ++i)
            if (v[i].first == v[i - 1].first) return false;  // two identical points or cells
        return true;
    }
    int find(const Key &k) const
    {
        auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(k, INT_MIN));
        return (it != v.end() && it->first == k) ? it->second : -1;
    }
};

inline int64_t bits(double x)
{
    int64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

// orbits {i, sx i, sy i, sx sy i} of a free Z2 x Z2 action, ordered by their smallest index (the first entry)
inline int orbits(const std::vector<int> &sx, const std::vector<int> &sy, std::vector<int> &out)
{
    const size_t n = sx.size();
    std::vector<char> seen(n, 0);
    out.clear();
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        if (seen[i]) continue;
        const int a = (int)i, b = sx[i], cc = sy[i], d = sy[(size_t)b];
        if (sx[(size_t)cc] != d) return GH_FOLD_CELLS;  // the mirrors do not commute (cannot happen for true mirrors)
        if (a == b || a == cc || a == d || b == cc || b == d || cc == d) return GH_FOLD_FIXED;
        for (int v : {a, b, cc, d}) {
            if (seen[(size_t)v]) return GH_FOLD_FIXED;
            seen[(size_t)v] = 1;
            out.push_back(v);
        }
    }
    return GH_FOLD_ON;
}

}  // namespace fold_detail

// The pairing: centre from the cells' extent, images within a few ulps of the coordinates' magnitude, heights
// (observations) and tops / bottoms (cells) bit for bit, no fixed points.  GH_FOLD_ON and the two tables, or
// the reason.
static int fold_detect_host(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *b6,
                            std::vector<int> &obs_img, std::vector<int> &cell_orbit)
{
    using namespace fold_detail;
    if (N < 4 || M < 4 || N % 4 || M % 4) return N % 4 ? GH_FOLD_OBS : GH_FOLD_CELLS;
    double xmin = b6[0], xmax = b6[1], ymin = b6[2], ymax = b6[3];
    for (int64_t j = 0; j < M; ++j) {
        const double *b = b6 + 6 * j;
        xmin = std::min(xmin, std::min(b[0], b[1]));
        xmax = std::max(xmax, std::max(b[0], b[1]));
        ymin = std::min(ymin, std::min(b[2], b[3]));
        ymax = std::max(ymax, std::max(b[2], b[3]));
    }
    double mag = std::max(std::max(std::fabs(xmin), std::fabs(xmax)), std::max(std::fabs(ymin), std::fabs(ymax)));
    for (int64_t i = 0; i < N; ++i) mag = std::max(mag, std::max(std::fabs(x[i]), std::fabs(y[i])));
    if (!std::isfinite(mag)) return GH_FOLD_OBS;
    // a few ulps of the coordinates' magnitude: rounding of a mirrored grid, nothing a field would notice
    const double tol = 8.0 * DBL_EPSILON * mag;
    const double cx = 0.5 * (xmin + xmax), cy = 0.5 * (ymin + ymax);

    // observations
    std::vector<int> osx((size_t)N), osy((size_t)N);
    {
        Axis ax, ay;
        ax.build(std::vector<double>(x, x + N), tol);
        ay.build(std::vector<double>(y, y + N), tol);
        std::vector<int> mx, my;
        if (!ax.mirror(cx, mx) || !ay.mirror(cy, my)) return GH_FOLD_OBS;
        std::vector<int> qx((size_t)N), qy((size_t)N);
        Index idx;
        idx.v.reserve((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            qx[(size_t)i] = ax.find(x[i]);
            qy[(size_t)i] = ay.find(y[i]);
            idx.v.push_back({Key{qx[(size_t)i], qy[(size_t)i], bits(z[i]), 0, 0, 0}, (int)i});
        }
        if (!idx.build()) return GH_FOLD_OBS;
        for (int64_t i = 0; i < N; ++i) {
            const int a = qx[(size_t)i], b = qy[(size_t)i];
            if (mx[(size_t)a] < 0 || my[(size_t)b] < 0) return GH_FOLD_OBS;
            osx[(size_t)i] = idx.find(Key{mx[(size_t)a], b, bits(z[i]), 0, 0, 0});
            osy[(size_t)i] = idx.find(Key{a, my[(size_t)b], bits(z[i]), 0, 0, 0});
            if (osx[(size_t)i] < 0 || osy[(size_t)i] < 0) return GH_FOLD_OBS;
        }
    }
    // cells: [x1, x2] -> [2c - x2, 2c - x1]
    std::vector<int> csx((size_t)M), csy((size_t)M);
    {
        Axis ax, ay;
        std::vector<double> vx, vy;
        vx.reserve(2 * (size_t)M);
        vy.reserve(2 * (size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            vx.push_back(b6[6 * j]);
            vx.push_back(b6[6 * j + 1]);
            vy.push_back(b6[6 * j + 2]);
            vy.push_back(b6[6 * j + 3]);
        }
        ax.build(std::move(vx), tol);
        ay.build(std::move(vy), tol);
        std::vector<int> mx, my;
        if (!ax.mirror(cx, mx) || !ay.mirror(cy, my)) return GH_FOLD_CELLS;
        std::vector<Key> keys((size_t)M);
        Index idx;
        idx.v.reserve((size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            const double *b = b6 + 6 * j;
            keys[(size_t)j] = Key{ax.find(b[0]), ax.find(b[1]), ay.find(b[2]), ay.find(b[3]), bits(b[4]), bits(b[5])};
            idx.v.push_back({keys[(size_t)j], (int)j});
        }
        if (!idx.build()) return GH_FOLD_CELLS;
        for (int64_t j = 0; j < M; ++j) {
            const Key &k = keys[(size_t)j];
            if (mx[(size_t)k[0]] < 0 || mx[(size_t)k[1]] < 0 || my[(size_t)k[2]] < 0 || my[(size_t)k[3]] < 0)
                return GH_FOLD_CELLS;
            csx[(size_t)j] = idx.find(Key{mx[(size_t)k[1]], mx[(size_t)k[0]], k[2], k[3], k[4], k[5]});
            csy[(size_t)j] = idx.find(Key{k[0], k[1], my[(size_t)k[3]], my[(size_t)k[2]], k[4], k[5]});
            if (csx[(size_t)j] < 0 || csy[(size_t)j] < 0) return GH_FOLD_CELLS;
        }
    }
    // (the mirror maps of clusters are involutions, so are these)
    int rc = orbits(osx, osy, obs_img);
    if (rc != GH_FOLD_ON) return rc == GH_FOLD_CELLS ? GH_FOLD_OBS : rc;
    return orbits(csx, csy, cell_orbit);
}

// The diagonal reflection tau: (x, y) -> (cx + (y - cy), cy + (x - cx)) on top of the two mirrors (square columns,
// the same grid of observations along x and y): clusters and tolerance as above, heights, tops and bottoms bit for
// bit.  GH_FOLD_PAIR_ON and, with pos[i] the place 4 f + g of index i in the mirror table,
//     obs_tau, cell_tau     the involution on the caller's indices
//     row_tau[f] = pos[tau obs_img[f][0]] = 4 f' + c_f,  orb_tau[o] = 4 o' + c_o alike:  tau s_g f = s_(swap(g) ^ c_f) f'
//     work                  (leading orbit, partner or -1), by leading orbit: a pair is led by its smaller index
// or the reason.
static int fold_pair_detect_host(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *b6,
                                 const std::vector<int> &obs_img, const std::vector<int> &cell_orbit, std::vector<int> &obs_tau,
                                 std::vector<int> &cell_tau, std::vector<int> &row_tau, std::vector<int> &orb_tau,
                                 std::vector<int> &work)
{
    using namespace fold_detail;
    double xmin = b6[0], xmax = b6[1], ymin = b6[2], ymax = b6[3];
    for (int64_t j = 0; j < M; ++j) {
        const double *b = b6 + 6 * j;
        xmin = std::min(xmin, std::min(b[0], b[1]));
        xmax = std::max(xmax, std::max(b[0], b[1]));
        ymin = std::min(ymin, std::min(b[2], b[3]));
        ymax = std::max(ymax, std::max(b[2], b[3]));
    }
    double mag = std::max(std::max(std::fabs(xmin), std::fabs(xmax)), std::max(std::fabs(ymin), std::fabs(ymax)));
    for (int64_t i = 0; i < N; ++i) mag = std::max(mag, std::max(std::fabs(x[i]), std::fabs(y[i])));
    const double tol = 8.0 * DBL_EPSILON * mag;
    const double cx = 0.5 * (xmin + xmax), cy = 0.5 * (ymin + ymax);
    // cluster of the other axis each cluster goes to (-1: none)
    auto across = [](const Axis &from, double cf, const Axis &to, double ct, std::vector<int> &m) {
        m.assign(from.lo.size(), -1);
        for (size_t q = 0; q < from.lo.size(); ++q) m[q] = to.find(ct + (0.5 * (from.lo[q] + from.hi[q]) - cf));
    };

    obs_tau.assign((size_t)N, -1);
    {
        Axis ax, ay;
        ax.build(std::vector<double>(x, x + N), tol);
        ay.build(std::vector<double>(y, y + N), tol);
        std::vector<int> x2y, y2x;
        across(ax, cx, ay, cy, x2y);
        across(ay, cy, ax, cx, y2x);
        std::vector<int> qx((size_t)N), qy((size_t)N);
        Index idx;
        idx.v.reserve((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            qx[(size_t)i] = ax.find(x[i]);
            qy[(size_t)i] = ay.find(y[i]);
            idx.v.push_back({Key{qx[(size_t)i], qy[(size_t)i], bits(z[i]), 0, 0, 0}, (int)i});
        }
        if (!idx.build()) return GH_FOLD_PAIR_OBS;
        for (int64_t i = 0; i < N; ++i) {
            const int a = y2x[(size_t)qy[(size_t)i]], b = x2y[(size_t)qx[(size_t)i]];
            if (a < 0 || b < 0) return GH_FOLD_PAIR_OBS;
            if ((obs_tau[(size_t)i] = idx.find(Key{a, b, bits(z[i]), 0, 0, 0})) < 0) return GH_FOLD_PAIR_OBS;
        }
    }
    cell_tau.assign((size_t)M, -1);
    {
        Axis ax, ay;
        std::vector<double> vx, vy;
        vx.reserve(2 * (size_t)M);
        vy.reserve(2 * (size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            vx.push_back(b6[6 * j]);
            vx.push_back(b6[6 * j + 1]);
            vy.push_back(b6[6 * j + 2]);
            vy.push_back(b6[6 * j + 3]);
        }
        ax.build(std::move(vx), tol);
        ay.build(std::move(vy), tol);
        std::vector<int> x2y, y2x;
        across(ax, cx, ay, cy, x2y);
        across(ay, cy, ax, cx, y2x);
        std::vector<Key> keys((size_t)M);
        Index idx;
        idx.v.reserve((size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            const double *b = b6 + 6 * j;
            keys[(size_t)j] = Key{ax.find(b[0]), ax.find(b[1]), ay.find(b[2]), ay.find(b[3]), bits(b[4]), bits(b[5])};
            idx.v.push_back({keys[(size_t)j], (int)j});
        }
        if (!idx.build()) return GH_FOLD_PAIR_CELLS;
        for (int64_t j = 0; j < M; ++j) {
            const Key &k = keys[(size_t)j];
            const int a0 = y2x[(size_t)k[2]], a1 = y2x[(size_t)k[3]], b0 = x2y[(size_t)k[0]], b1 = x2y[(size_t)k[1]];
            if (a0 < 0 || a1 < 0 || b0 < 0 || b1 < 0) return GH_FOLD_PAIR_CELLS;
            if ((cell_tau[(size_t)j] = idx.find(Key{a0, a1, b0, b1, k[4], k[5]})) < 0) return GH_FOLD_PAIR_CELLS;
        }
    }
    // tau is an involution that turns the mirror s_g into s_swap(g): checked on the tables, then kept per row / orbit
    auto rows = [](const std::vector<int> &img, const std::vector<int> &tau, std::vector<int> &rt) {
        const size_t n = img.size();
        std::vector<int> pos(n);
        for (size_t e = 0; e < n; ++e) pos[(size_t)img[e]] = (int)e;
        rt.assign(n / 4, -1);
        for (size_t e = 0; e < n; ++e) {
            const int i = img[e], g = (int)(e & 3);
            if (tau[(size_t)tau[(size_t)i]] != i) return false;
            const int at = pos[(size_t)tau[(size_t)i]] ^ (((g & 1) << 1) | (g >> 1));  // place of tau s_0 f
            if (g == 0) rt[e >> 2] = at;
            if (rt[e >> 2] != at) return false;
        }
        return true;
    };
    if (!rows(obs_img, obs_tau, row_tau)) return GH_FOLD_PAIR_OBS;
    if (!rows(cell_orbit, cell_tau, orb_tau)) return GH_FOLD_PAIR_CELLS;
    work.clear();
    for (size_t o = 0; o < orb_tau.size(); ++o) {
        const int o2 = orb_tau[o] >> 2;
        if (o2 == (int)o) {
            work.push_back((int)o);
            work.push_back(-1);
        } else if ((int)o < o2) {
            work.push_back((int)o);
            work.push_back(o2);
        }
    }
    return GH_FOLD_PAIR_ON;
}

namespace fold_detail {

// The paired sweep's row order (fold.hip.h: thread t of 512 owns the rows k 512 + t, k < rows = ceil(ldF / 512), in
// pair_slots = (rows - 1) / 2 pair slots and rows - 2 pair_slots lone slots).  rho: f -> row_tau[f] >> 2 is an
// involution on the folded rows.  Pairs {f < rho f} by f fill the pair slots, slot by slot, thread by thread; the
// pairs beyond them are split into two lone rows in neighbouring lanes, then the rows with rho f = f follow, through
// the lone rows in the store's order.
//     code[n], n < ldF     4 f + c: row n of the new order is row f of the mirror table with its sub-columns k ^ c
//                          (the second row of a pair slot: rho f as the representative tau f of its orbit), -1: zeros
//     ptab                 fold_pair_cols(rows) x 512 x 4: column 2 s the observations s_g f of the first row of slot
//                          s, column 2 s + 1 the observations s_g tau f; -1 where the thread has no row there
// false: the rows do not fit this plan (rows with rho f = f beyond the lone rows left: no grid has them).
struct PairRows {
    int rows = 0, pair_slots = 0, cols = 0;
    int64_t pairs_in_slots = 0, pairs_split = 0, self_rows = 0;
    std::vector<int> code, ptab;
};

inline bool pair_rows_plan(int nF, int ldF, const std::vector<int> &obs_img, const std::vector<int> &row_tau, PairRows &pr)
{
    constexpr int TT = 512;
    pr.rows = (ldF + TT - 1) / TT;
    pr.pair_slots = ghk::fold_pair_slots(pr.rows);
    pr.cols = ghk::fold_pair_cols(pr.rows);
    pr.pairs_in_slots = pr.pairs_split = pr.self_rows = 0;
    pr.code.assign((size_t)ldF, -1);
    pr.ptab.assign((size_t)pr.cols * TT * 4, -1);
    // slot s of thread t takes row f at store row k 512 + t (its partner row behind it when both)
    auto place = [&](int s, int t, int k, int f, bool both) {
        const int rt = row_tau[(size_t)f], f2 = rt >> 2, cf = rt & 3;
        int *pa = pr.ptab.data() + ((size_t)(2 * s) * TT + (size_t)t) * 4, *pb = pa + (size_t)TT * 4;
        for (int g = 0; g < 4; ++g) {
            pa[g] = obs_img[4 * (size_t)f + g];
            pb[g] = obs_img[4 * (size_t)f2 + (g ^ cf)];
        }
        pr.code[(size_t)k * TT + t] = 4 * f;
        if (both) pr.code[(size_t)(k + 1) * TT + t] = 4 * f2 + cf;
    };
    const int64_t cap = (int64_t)pr.pair_slots * TT;
    // lone rows in the store's order: n = (2 pair_slots + l) 512 + t < ldF
    int64_t lone = 0;
    auto place_lone = [&](int f) -> bool {
        const int64_t n = 2 * cap + lone;
        if (n >= ldF) return false;
        const int l = (int)(lone / TT), t = (int)(lone % TT);
        place(pr.pair_slots + l, t, 2 * pr.pair_slots + l, f, false);
        ++lone;
        return true;
    };
    int64_t np = 0;
    for (int f = 0; f < nF; ++f) {
        const int f2 = row_tau[(size_t)f] >> 2;
        if (f2 <= f) continue;
        if (np < cap) {
            place((int)(np / TT), (int)(np % TT), 2 * (int)(np / TT), f, true);
            ++pr.pairs_in_slots;
        } else {
            if (!place_lone(f) || !place_lone(f2)) return false;
            ++pr.pairs_split;
        }
        ++np;
    }
    for (int f = 0; f < nF; ++f) {
        if ((row_tau[(size_t)f] >> 2) != f) continue;
        if (!place_lone(f)) return false;
        ++pr.self_rows;
    }
    return true;
}

}  // namespace fold_detail

constexpr int FOLD_PAIR_MAX_ROWS = 5;  // rows per thread of fold_pair_sweep_kernel: registers without spills

// the diagonal reflection of a geometry whose mirrors were found: the tables of the paired sweep on the device
static int fold_pair_tables(gh_ctx *c, const double *ox, const double *oy, const double *oz, const double *b6)
{
    gh_ctx::Fold &f = c->fd;
    std::vector<int> obs_tau, cell_tau, row_tau, orb_tau, work;
    f.pair_on = false;
    f.n_work = f.n_pairs = 0;
    f.pair_reason = fold_pair_detect_host(c->N, ox, oy, oz, c->M, b6, f.obs_img, f.cell_orbit, obs_tau, cell_tau, row_tau,
                                          orb_tau, work);
    f.pair_detected = f.pair_reason == GH_FOLD_PAIR_ON;
    if (!f.pair_detected) return GH_OK;
    f.pair_reason = GH_FOLD_PAIR_UNDECIDED;
    f.n_work = (int64_t)(work.size() / 2);
    std::vector<int> wtab((size_t)f.n_work * ghk::FOLD_PAIR_W, 0);
    for (int64_t w = 0; w < f.n_work; ++w) {
        const int o = work[2 * (size_t)w], o2 = work[2 * (size_t)w + 1];
        int *t = wtab.data() + w * ghk::FOLD_PAIR_W;
        for (int h = 0; h < 4; ++h) {
            t[h] = f.cell_orbit[4 * (size_t)o + h];
            t[4 + h] = o2 >= 0 ? cell_tau[(size_t)t[h]] : ~t[h];
        }
        t[8] = o;
        f.n_pairs += o2 >= 0;
    }
    // the sweep's row order (more than five rows per thread: the sweep is refused anyway)
    fold_detail::PairRows pr;
    f.pair_rows_ok = f.ldF <= 512 * FOLD_PAIR_MAX_ROWS && fold_detail::pair_rows_plan(f.nF, f.ldF, f.obs_img, row_tau, pr);
    if (!f.pair_rows_ok) {
        pr.code.assign((size_t)f.ldF, -1);
        pr.ptab.assign(4, -1);
    }
    // (sized for any geometry of the context's N and M: a later build reuses them)
    auto up = [&](int **d, const std::vector<int> &h, size_t cap) -> int {
        TRY(dalloc(c, d, cap, false));
        HIPCHK(c, hipMemcpyAsync(*d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, c->stream));
        return GH_OK;
    };
    TRY(up(&f.wtab_d, wtab, (size_t)f.n_orb * ghk::FOLD_PAIR_W));
    TRY(up(&f.ptab_d, pr.ptab, (size_t)ghk::fold_pair_cols(FOLD_PAIR_MAX_ROWS) * 512 * 4));
    TRY(up(&f.row_code_d, pr.code, (size_t)f.ldF));
    TRY(up(&f.row_tau_d, row_tau, (size_t)f.nF));
    TRY(up(&f.orb_tau_d, orb_tau, (size_t)f.n_orb));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

// gh_build_G of a dense store: look for the pairing (gz prisms only)
static int fold_detect(gh_ctx *c)
{
    gh_ctx::Fold &f = c->fd;
    f.detected = -1;
    f.valid = false;
    f.gen = ~0ull;
    f.reason = GH_FOLD_NOT_GZ;
    f.pair_detected = f.pair_on = false;
    f.pair_reason = GH_FOLD_PAIR_NO_FOLD;
    if (c->cell_kind != GH_CELL_PRISM || c->joint || c->mf || !c->G) return GH_OK;
    std::vector<double> ox((size_t)c->N), oy((size_t)c->N), oz((size_t)c->N), b6((size_t)c->M * 6);
    TRY(d2h(c, ox.data(), c->obs[0], ox.size()));
    TRY(d2h(c, oy.data(), c->obs[1], oy.size()));
    TRY(d2h(c, oz.data(), c->obs[2], oz.size()));
    TRY(d2h(c, b6.data(), c->bounds, b6.size()));
    f.reason = fold_detect_host(c->N, ox.data(), oy.data(), oz.data(), c->M, b6.data(), f.obs_img, f.cell_orbit);
    if (f.reason != GH_FOLD_ON) return GH_OK;
    f.nF = (int)(c->N / 4);
    f.ldF = (f.nF + 15) / 16 * 16;
    f.n_orb = c->M / 4;
    TRY(dalloc(c, &f.obs_img_d, (size_t)c->N, false));
    TRY(dalloc(c, &f.cell_orbit_d, (size_t)c->M, false));
    HIPCHK(c, hipMemcpyAsync(f.obs_img_d, f.obs_img.data(), sizeof(int) * f.obs_img.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(f.cell_orbit_d, f.cell_orbit.data(), sizeof(int) * f.cell_orbit.size(), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host tables stay, but may be reassigned by a later build)
    TRY(fold_pair_tables(c, ox.data(), oy.data(), oz.data(), b6.data()));
    f.detected = 1;
    f.reason = GH_FOLD_UNDECIDED;
    return GH_OK;
}

// ----------------------------------------------------------------------------------- store and launches

constexpr int FOLD_MAX_EPT2 = 5;        // 10240 folded rows: registers without spills (fold_sweep_kernel)
constexpr double FOLD_MAX_DEV = 1e-7;   // sanity bound of the build: catches a wrong pairing, not rounding

typedef void (*fold_fn)(SweepArgs, FoldArgs);

static fold_fn fold_kernel_for(int ept2)
{
    switch (ept2) {
    case 1: return fold_sweep_kernel<1>;
    case 2: return fold_sweep_kernel<2>;
    case 3: return fold_sweep_kernel<3>;
    case 4: return fold_sweep_kernel<4>;
    case 5: return fold_sweep_kernel<5>;
    }
    return nullptr;
}

typedef void (*fold_pair_fn)(SweepArgs, FoldArgs, FoldPairArgs);

static fold_pair_fn fold_pair_kernel_for(int rows)
{
    switch (rows) {
    case 1: return fold_pair_sweep_kernel<1>;
    case 2: return fold_pair_sweep_kernel<2>;
    case 3: return fold_pair_sweep_kernel<3>;
    case 4: return fold_pair_sweep_kernel<4>;
    case 5: return fold_pair_sweep_kernel<5>;
    }
    return nullptr;
}

constexpr size_t FOLD_PAIR_MAX_LDS = 160u << 10;  // the CU's LDS

// what decides whether the paired sweep takes a geometry: two unpadded copies of r and the slots (the sweep itself
// needs less since it folds the rows over tau too; the limit stays where it was)
static size_t fold_pair_lds_limit(const gh_ctx *c)
{
    return ((size_t)8 * c->fd.nF + 2 * FOLD_PSLOT) * sizeof(double);
}

// r behind every entry of the row table, and the slots
static size_t fold_pair_lds(const gh_ctx *c)
{
    return ((size_t)ghk::fold_pair_cols(c->fd.pair_rows) * 512 * 4 + 2 * FOLD_PSLOT) * sizeof(double);
}

static int64_t fold_store_bytes(const gh_ctx *c)
{
    return c->fd.n_orb * 4 * (int64_t)c->fd.ldF * (int64_t)sizeof(double);
}

static FoldArgs fold_args(const gh_ctx *c)
{
    const gh_ctx::Fold &f = c->fd;
    FoldArgs a{};
    a.S = f.S;
    a.obs_img = f.obs_img_d;
    a.cell_orbit = f.cell_orbit_d;
    a.nF = f.nF;
    a.ldF = f.ldF;
    a.n_orb = f.n_orb;
    a.orb_per_team = f.orb_per_team;
    a.n_pp = c->n_teams;
    a.N = c->N;
    return a;
}

static FoldPairArgs fold_pair_args(const gh_ctx *c)
{
    const gh_ctx::Fold &f = c->fd;
    FoldPairArgs p{};
    p.wtab = f.wtab_d;
    p.ptab = f.ptab_d;
    p.n_work = f.n_work;
    p.work_per_team = f.work_per_team;
    return p;
}

// bytes of the store one sweep reads: every block, or the blocks of the paired sweep's work items
static int64_t fold_sweep_bytes(const gh_ctx *c)
{
    const gh_ctx::Fold &f = c->fd;
    return (f.pair_on ? f.n_work : f.n_orb) * 4 * (int64_t)f.ldF * (int64_t)sizeof(double);
}

// Build the folded store of the current dense one (stream-ordered, synchronises once to read the deviation).
static int fold_build(gh_ctx *c)
{
    gh_ctx::Fold &f = c->fd;
    const auto t0 = std::chrono::steady_clock::now();
    TRY(dalloc(c, &f.S, (size_t)(fold_store_bytes(c) / (int64_t)sizeof(double)), false));
    TRY(dalloc(c, &f.dev_bits, 1, false));
    TRY(dalloc(c, &f.zeros, (size_t)c->M));
    HIPCHK(c, hipMemsetAsync(f.dev_bits, 0, sizeof(unsigned long long), c->stream));
    fold_build_kernel<<<dim3((unsigned)f.n_orb), dim3(256), 0, c->stream>>>(c->G, c->ld, fold_args(c), f.S, f.dev_bits);
    HIPCHK(c, hipGetLastError());
    unsigned long long bits = 0;
    HIPCHK(c, hipMemcpyAsync(&bits, f.dev_bits, sizeof bits, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(&f.max_dev, &bits, sizeof bits);
    if (f.pair_on) {
        // the mean over all eight images: the two blocks of a pair averaged entry by entry.  An entry is within
        // max_dev of its four-image mean and that mean within this pass's deviation of the eight-image one: their sum
        // bounds the distance of an entry from the mean the store holds
        HIPCHK(c, hipMemsetAsync(f.dev_bits, 0, sizeof(unsigned long long), c->stream));
        fold_pair_mean_kernel<<<dim3((unsigned)f.n_orb), dim3(256), 0, c->stream>>>(fold_args(c), f.row_tau_d, f.orb_tau_d, f.S,
                                                                                   f.dev_bits);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&bits, f.dev_bits, sizeof bits, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double d8 = 0.0;
        memcpy(&d8, &bits, sizeof bits);
        f.max_dev += d8;
        // the blocks in the paired sweep's row order
        const size_t blk = (size_t)4 * f.ldF * sizeof(double);
        HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(fold_pair_rows_kernel), blk));
        fold_pair_rows_kernel<<<dim3((unsigned)f.n_orb), dim3(512), blk, c->stream>>>(fold_args(c), f.row_code_d, f.S);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    f.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GH_OK;
}

// Does this sweep (one whole panel, single chain) read the folded store?  Decides once per dense store, builds
// the folded store when it qualifies.
static int fold_use(gh_ctx *c, bool *use)
{
    gh_ctx::Fold &f = c->fd;
    *use = false;
    if (f.detected != 1 || f.exact) return GH_OK;
    if (c->sh.kind != 0 || c->wv.on || c->joint || c->mf || c->n_panels != 1) {
        f.reason = GH_FOLD_PATH;
        return GH_OK;
    }
    if (f.gen == c->G_gen) {
        *use = f.valid;
        return GH_OK;
    }
    f.gen = c->G_gen;
    f.valid = false;
    f.pair_on = false;
    if (env_int("GRAVHMC_FOLD", 1) == 0) {
        f.reason = GH_FOLD_SWITCHED_OFF;
        return GH_OK;
    }
    const int64_t min_mb = env_int("GRAVHMC_FOLD_MIN_MB", 512);
    if (c->ld * c->M * (int64_t)sizeof(double) <= (min_mb << 20)) {
        f.reason = GH_FOLD_SMALL;
        return GH_OK;
    }
    // (the resident chain kernel would run the chain on the dense store: chain and stateless calls must agree)
    f.ept2 = (2 * f.ldF + 1023) / 1024;
    if (f.ept2 > FOLD_MAX_EPT2 || (c->ld <= 1024 && env_int("GRAVHMC_RESIDENT", 1) != 0)) {
        f.reason = GH_FOLD_PATH;
        return GH_OK;
    }
    {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (!f.S && (int64_t)free_b < fold_store_bytes(c) + ((int64_t)256 << 20)) {
            f.reason = GH_FOLD_NOMEM;
            return GH_OK;
        }
    }
    // the paired sweep where the diagonal reflection was found and r, r o tau fit the LDS of a CU
    f.pair_on = false;
    f.pair_rows = (f.ldF + 511) / 512;
    if (!f.pair_detected) {
        // (the reason of the detection stays)
    } else if (env_int("GRAVHMC_FOLD_PAIR", 1) == 0) {
        f.pair_reason = GH_FOLD_PAIR_SWITCHED_OFF;
    } else if (fold_pair_lds_limit(c) > FOLD_PAIR_MAX_LDS || f.pair_rows > FOLD_PAIR_MAX_ROWS || !f.pair_rows_ok) {
        f.pair_reason = GH_FOLD_PAIR_ROWS;
    } else if (allow_dynamic_lds(reinterpret_cast<const void *>(fold_pair_kernel_for(f.pair_rows)), fold_pair_lds(c)) !=
               hipSuccess) {
        (void)hipGetLastError();  // (a device that does not grant one workgroup that much)
        f.pair_reason = GH_FOLD_PAIR_ROWS;
    } else {
        f.pair_on = true;
        f.pair_reason = GH_FOLD_PAIR_ON;
    }
    const void *fn = f.pair_on ? reinterpret_cast<const void *>(fold_pair_kernel_for(f.pair_rows))
                               : reinterpret_cast<const void *>(fold_kernel_for(f.ept2));
    const int threads = f.pair_on ? 512 : 1024;
    f.lds = f.pair_on ? fold_pair_lds(c) : ((size_t)4 * f.ldF + 2 * FOLD_SLOT) * sizeof(double);
    HIPCHK(c, allow_dynamic_lds(fn, f.lds));
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, f.lds) != hipSuccess || occ < 1) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int64_t items = f.pair_on ? f.n_work : f.n_orb;
    int grid = (int)std::min<int64_t>(std::min<int64_t>((int64_t)c->cus * occ, c->grid), items);
    const int64_t per_team = (items + grid - 1) / grid;
    f.orb_per_team = f.work_per_team = per_team;
    f.grid = (int)((items + per_team - 1) / per_team);
    // (a slab row, a slab-row sum and a pp partial per workgroup: within the dense sweep's, host_layout.h)
    TRY(work_claim(c, "fold_use", WorkDemand{f.grid, f.grid, f.grid}));
    TRY(fold_build(c));
    if (!(f.max_dev <= FOLD_MAX_DEV)) {
        f.reason = GH_FOLD_DEVIATION;
        return GH_OK;
    }
    f.valid = true;
    f.reason = GH_FOLD_ON;
    *use = true;
    return GH_OK;
}

// gh_forward and gh_adjoint apply the operator itself: the dense store, entry for entry (callers probe columns
// with unit vectors and compare them with the prism formula at 1e-11 of the largest entry; an orbit's mean differs
// from its entries by the formula's own cancellation noise, up to a few 1e-9 of a column's largest entry)
struct FoldExact {
    gh_ctx *c;
    explicit FoldExact(gh_ctx *c_) : c(c_) { c->fd.exact = true; }
    ~FoldExact() { c->fd.exact = false; }
};

static int launch_fold(gh_ctx *c, SweepArgs &a)
{
    gh_ctx::Fold &f = c->fd;
    a.ld = c->ld;
    a.M = c->M;
    a.row0 = 0;
    a.rows = c->ld;
    bool timed = c->prof && c->ev_used + 2 <= c->ev.size() && (c->prof_seen++ % c->prof_stride) == 0;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[c->ev_used], c->stream));
    SweepArgs b = a;  // (the kernel loads every per-cell input unconditionally)
    for (const double **v : {&b.x_in, &b.p_in, &b.low, &b.high, &b.greg, &b.pn_in})
        if (!*v) *v = f.zeros;
    if (f.pair_on)
        hipLaunchKernelGGL(fold_pair_kernel_for(f.pair_rows), dim3(f.grid), dim3(512), f.lds, c->stream, b, fold_args(c),
                           fold_pair_args(c));
    else
        hipLaunchKernelGGL(fold_kernel_for(f.ept2), dim3(f.grid), dim3(1024), f.lds, c->stream, b, fold_args(c));
    if (timed) {
        HIPCHK(c, hipEventRecord(c->ev[c->ev_used + 1], c->stream));
        c->ev_bytes[c->ev_used / 2] = fold_sweep_bytes(c);  // (what this launch reads)
        c->ev_used += 2;
    }
    if (c->prof) c->prof_launches += 1;
    f.launches += 1;
    HIPCHK(c, hipGetLastError());
    return GH_OK;
}
