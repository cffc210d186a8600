// libgravhmc host side: the translation-invariant store of a regular prism grid under gridded data
// (lattice.hip.h).  Detection of the structure (context-free), one table of the forms a store takes on it, the build of
// the table in its steps, the two passes' launches, the batch passes.  Included once by gravhmc.hip, after host_fold.h.
#pragma once

// ------------------------------------------------------------------------------------ detection (host)

// Cells: the full product of nx contiguous x-intervals of one width, ny contiguous y-intervals of one width and nz
// layers (z1, z2 bit for bit), in any order.  Observations: one height (bit for bit), a full px x qy rectangle of
// the lattice of the cells' spacings, in any order.  Coordinates within the fold's tolerance, a few ulps of their
// magnitude.  GH_LATTICE_ON, dims = {nx, ny, nz, px, qy} and the four maps, or the reason.
static int lattice_detect_host(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *b6,
                               int dims[5], std::vector<int> &lat_of_cell, std::vector<int> &cell_of_lat,
                               std::vector<int> &lat_of_obs, std::vector<int> &obs_of_lat)
{
    using namespace fold_detail;
    if (N < 1 || M < 1 || N > INT_MAX || M > INT_MAX) return N < 1 ? GH_LATTICE_RECT : GH_LATTICE_CELLS;
    double mag = 0.0;
    for (int64_t j = 0; j < M; ++j)
        for (int e = 0; e < 4; ++e) mag = std::max(mag, std::fabs(b6[6 * j + e]));
    for (int64_t i = 0; i < N; ++i) mag = std::max(mag, std::max(std::fabs(x[i]), std::fabs(y[i])));
    if (!std::isfinite(mag)) return GH_LATTICE_CELLS;
    const double tol = 8.0 * DBL_EPSILON * mag;

    // cells: the edges of an axis are nx + 1 clusters at e_0 + t h
    Axis ax, ay;
    {
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
    }
    auto spacing = [&](const Axis &a, double &e0, double &h) {
        const size_t n = a.lo.size();
        if (n < 2) return false;
        e0 = 0.5 * (a.lo[0] + a.hi[0]);
        h = (0.5 * (a.lo[n - 1] + a.hi[n - 1]) - e0) / (double)(n - 1);
        if (!(h > 0.0)) return false;
        for (size_t t = 0; t < n; ++t)
            if (a.hi[t] - a.lo[t] > 2.0 * tol || std::fabs(0.5 * (a.lo[t] + a.hi[t]) - (e0 + (double)t * h)) > tol) return false;
        return true;
    };
    double ex0 = 0.0, ey0 = 0.0, hx = 0.0, hy = 0.0;
    if (!spacing(ax, ex0, hx) || !spacing(ay, ey0, hy)) return GH_LATTICE_CELLS;
    const int64_t nx = (int64_t)ax.lo.size() - 1, ny = (int64_t)ay.lo.size() - 1;
    // layers: distinct (z1, z2), ordered by their values
    std::vector<std::pair<double, double>> layers;
    layers.reserve((size_t)M);
    for (int64_t j = 0; j < M; ++j) layers.push_back({b6[6 * j + 4], b6[6 * j + 5]});
    std::sort(layers.begin(), layers.end());
    layers.erase(std::unique(layers.begin(), layers.end(),
                             [](const std::pair<double, double> &p, const std::pair<double, double> &q) {
                                 return bits(p.first) == bits(q.first) && bits(p.second) == bits(q.second);
                             }),
                 layers.end());
    const int64_t nz = (int64_t)layers.size();
    lat_of_cell.assign(3 * (size_t)M, -1);
    {
        Index idx;
        idx.v.reserve((size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            const double *b = b6 + 6 * j;
            const int a0 = ax.find(b[0]), a1 = ax.find(b[1]), b0 = ay.find(b[2]), b1 = ay.find(b[3]);
            if (a0 < 0 || b0 < 0 || a1 != a0 + 1 || b1 != b0 + 1) return GH_LATTICE_CELLS;  // not one interval of the axis
            const int k = (int)(std::lower_bound(layers.begin(), layers.end(), std::make_pair(b[4], b[5])) - layers.begin());
            if (k >= nz || bits(layers[(size_t)k].first) != bits(b[4]) || bits(layers[(size_t)k].second) != bits(b[5]))
                return GH_LATTICE_CELLS;  // (NaN, or -0.0 beside 0.0)
            lat_of_cell[3 * (size_t)j] = k;
            lat_of_cell[3 * (size_t)j + 1] = a0;
            lat_of_cell[3 * (size_t)j + 2] = b0;
            idx.v.push_back({Key{k, a0, b0, 0, 0, 0}, (int)j});
        }
        if (!idx.build()) return GH_LATTICE_DUPLICATE;
    }
    if ((double)nx * (double)ny * (double)nz != (double)M) return GH_LATTICE_CELLS;  // distinct, in range, too few
    cell_of_lat.assign((size_t)M, -1);
    for (int64_t j = 0; j < M; ++j)
        cell_of_lat[((size_t)lat_of_cell[3 * (size_t)j] * (size_t)nx + (size_t)lat_of_cell[3 * (size_t)j + 1]) * (size_t)ny +
                    (size_t)lat_of_cell[3 * (size_t)j + 2]] = (int)j;

    // observations
    for (int64_t i = 1; i < N; ++i)
        if (bits(z[i]) != bits(z[0])) return GH_LATTICE_HEIGHTS;
    Axis ox, oy;
    ox.build(std::vector<double>(x, x + N), tol);
    oy.build(std::vector<double>(y, y + N), tol);
    // the clusters of an axis sit at c_0 + m h with the CELLS' h (SPACING), m = 0, 1, 2, ... without a gap (RECT).
    // (h comes from the cells' extent and carries tol / n of error per step: m steps are allowed tol (1 + m / n))
    auto on_lattice = [&](const Axis &a, double h, int64_t n) {
        const double c0 = 0.5 * (a.lo[0] + a.hi[0]);
        bool gap = false;
        for (size_t t = 0; t < a.lo.size(); ++t) {
            const double ct = 0.5 * (a.lo[t] + a.hi[t]);
            const double m = std::nearbyint((ct - c0) / h);
            if (a.hi[t] - a.lo[t] > 2.0 * tol || std::fabs(ct - (c0 + m * h)) > tol * (1.0 + m / (double)n)) return GH_LATTICE_SPACING;
            gap = gap || m != (double)t;
        }
        return gap ? GH_LATTICE_RECT : GH_LATTICE_ON;
    };
    const int rx = on_lattice(ox, hx, nx), ry = on_lattice(oy, hy, ny);
    if (rx == GH_LATTICE_SPACING || ry == GH_LATTICE_SPACING) return GH_LATTICE_SPACING;
    const int64_t px = (int64_t)ox.lo.size(), qy = (int64_t)oy.lo.size();
    lat_of_obs.assign(2 * (size_t)N, -1);
    {
        Index idx;
        idx.v.reserve((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            const int p = ox.find(x[i]), q = oy.find(y[i]);
            if (p < 0 || q < 0) return GH_LATTICE_SPACING;
            lat_of_obs[2 * (size_t)i] = p;
            lat_of_obs[2 * (size_t)i + 1] = q;
            idx.v.push_back({Key{p, q, 0, 0, 0, 0}, (int)i});
        }
        if (!idx.build()) return GH_LATTICE_DUPLICATE;
    }
    if (rx != GH_LATTICE_ON || ry != GH_LATTICE_ON || (double)px * (double)qy != (double)N) return GH_LATTICE_RECT;
    obs_of_lat.assign((size_t)N, -1);
    for (int64_t i = 0; i < N; ++i)
        obs_of_lat[(size_t)lat_of_obs[2 * (size_t)i] * (size_t)qy + (size_t)lat_of_obs[2 * (size_t)i + 1]] = (int)i;
    dims[0] = (int)nx;
    dims[1] = (int)ny;
    dims[2] = (int)nz;
    dims[3] = (int)px;
    dims[4] = (int)qy;
    return GH_LATTICE_ON;
}

static const char *lattice_reason_text(int reason)
{
    switch (reason) {
    case GH_LATTICE_CELLS:
        return "the cells are not the full product of equal x-intervals, equal y-intervals and layers (a carved or "
               "irregular mesh)";
    case GH_LATTICE_HEIGHTS: return "the observations are at several heights";
    case GH_LATTICE_SPACING:
        return "the observations are not on the cells' spacing (n points from one end of the mesh to the other are "
               "L / (n - 1) apart, the cells L / n)";
    case GH_LATTICE_RECT: return "the observations are not a full rectangle of the lattice";
    case GH_LATTICE_DUPLICATE: return "two observations or two cells coincide";
    case GH_LATTICE_DEVIATION: return "entries of one offset differ beyond the sanity bound";
    case GH_LATTICE_LDS: return "a row of the lattice is too long for the pass's LDS tile";
    }
    return "";
}

// ------------------------------------------------------------------------------------- the table's forms

static const char *const LATTICE_NAME = "the translation-invariant store";

typedef void (*lat_fill_fn)(MfGeom, ghk::LatGeom, double *, double *);
typedef void (*lat_pass_fn)(ghk::LatGeom, ghk::LatPlan, SweepArgs, const double *, int64_t, ghk::LatBlocks);

// What a store is on the table: one row per form, and the code below reads the row.  LAT_SCALAR: a prism store of one
// block (gz, a component, the total field).  LAT_MULTI: the multi-component store, one table per row block (lattice.hip.h,
// "Row blocks").  LAT_MVI: the vector-data magnetization store, the axis of a column as one more layer coordinate under row
// blocks of magnetic data (latmvi.hip.h).  LAT_JOINT: the joint gravity-magnetic store, the property of a column as that
// layer coordinate, a layer on the observation block of its property alone (latjoint.hip.h; "Block-diagonal layers").
enum { LAT_SCALAR = 0, LAT_MULTI, LAT_MVI, LAT_JOINT };
constexpr int PER_COMPONENT = 0;  // a count of a row: one per component of the store's block table (c->mc.n)

struct LatForm {
    const char *name;        // the form as the refusals of what it does not run name it
    const char *build_name;  // ... and as gh_build_G does on a geometry without the structure
    const char *entry;       // the entry point that set the form with its cells -- the table is then the context's form and
                             // stays; null: gh_set_translation_invariant, which may also switch it off again
    int groups;              // layer groups: LatGeom::nz = groups x the geometry's layers, layer L = group nz + k
    int rblocks;             // blocks of r (LatGeom::rl), one per field of the data: also the parts of the store whose
                             // deviation is checked against their own largest entry
    int tables;              // tables T[b] a layer sums over
    lat_pass_fn adj, fwd;    // the two passes
    bool cut;                // the forward's chunks of layers are cut per layer group: a chunk sums into one block of d
};

static const LatForm LAT_FORMS[] = {
    {LATTICE_NAME, LATTICE_NAME, nullptr, 1, 1, 1, ghk::lat_pass_kernel<false, false>, ghk::lat_pass_kernel<true, false>, false},
    {LATTICE_NAME, LATTICE_NAME, "gh_set_cells_multi_table", 1, PER_COMPONENT, PER_COMPONENT,
     ghk::lat_pass_kernel<false, true>, ghk::lat_pass_kernel<true, true>, false},
    {"the vector-data magnetization store on the translation-invariant table", LATTICE_NAME, "gh_set_cells_mvi_table", 3,
     PER_COMPONENT, PER_COMPONENT, ghk::lat_pass_kernel<false, true>, ghk::lat_pass_kernel<true, true>, false},
    {"the joint store on the translation-invariant table", "the joint store on the translation-invariant table",
     "gh_set_cells_joint_table", 2, 2, 1, ghk::lat_pass_kernel<false, false, true>, ghk::lat_pass_kernel<true, false, true>, true},
};
static_assert(sizeof LAT_FORMS / sizeof LAT_FORMS[0] == LAT_JOINT + 1, "one row per LAT_* form");

// ----------------------------------------------------------------------------------- store and launches

struct LatticeHost {
    bool on = false;  // the table is built
    bool mf_before = false;  // what gh_set_matrix_free asked for before the store took c->mf
    const LatForm *form = &LAT_FORMS[LAT_SCALAR];
    // What the table runs: GH_TABLE_SINGLE the single chain; GH_TABLE_CHAINS chain batches too (latbatch.hip.h; on the table
    // of blocks: gh_set_cells_multi_table_chains); GH_TABLE_REPLICATES the bootstrap batch too (gh_bscg_run)
    int runs = GH_TABLE_SINGLE;
    int nr = 1, nb = 1;  // the form's blocks of r and tables, counted (lattice_geometry)
    ghk::LatGeom g = {};
    ghk::LatPlan adj = {}, fwd = {};
    size_t lds_adj = 0, lds_fwd = 0;
    int gx_adj = 0, gx_fwd = 0, chunks = 0;
    double *T = nullptr;
    int *cell_of = nullptr, *obs_of = nullptr;
    double max_dev = 0.0, build_ms = 0.0;
    // The partition of the batch passes (chain batches and the bootstrap batch share it) is made by latb_plan on the
    // built table: bt_state 0 not yet, 1 planned, -1 an extent the batch tile cannot hold
    int bt_state = 0;
    ghk::LatbPlan badj = {}, bfwd = {};
    size_t blds_adj = 0, blds_fwd = 0;
    int bgx_adj = 0, bgx_fwd = 0, bchunks = 0;
    double *xl16 = nullptr, *rl16 = nullptr;
};

static bool lattice_on(const gh_ctx *c) { return c->lat && c->lat->on; }
static const LatForm &lattice_form(const gh_ctx *c) { return *c->lat->form; }
// the store was set onto the table with its cells (LatForm::entry)
static bool lattice_own(const gh_ctx *c) { return c && c->lat && c->lat->form->entry; }
// ... as a table of row blocks: the multi-component store, the vector-data magnetization store
static bool lattice_multi(const gh_ctx *c) { return c && c->lat && c->lat->form->tables == PER_COMPONENT; }
static bool lattice_mvi(const gh_ctx *c) { return c && c->lat && c->lat->form == &LAT_FORMS[LAT_MVI]; }

// What gh_set_translation_invariant does to a context that may take the table (its own checks passed), and what the
// gh_set_cells_*_table entry points do once the store's blocks are set
static void lattice_switch_on(gh_ctx *c, int form, int runs)
{
    c->lat = new LatticeHost();
    c->lat->mf_before = c->mf;
    c->lat->form = &LAT_FORMS[form];
    c->lat->runs = runs;
    c->mf = true;
}

// The blocks of r as the passes and the gathers of r take them.  The data weights hold from gh_weight on, as on the dense
// store (whose rows gh_weight scales): the components' w_b; the joint store's {1, s = std_gz / std_tf} on [gz: ld | tf: ld]
static ghk::LatBlocks lattice_r_blocks(const gh_ctx *c)
{
    ghk::LatBlocks bl{};
    bl.n = c->lat->nr;
    bl.Nb = c->joint ? c->ld : store_points(c);
    for (int b = 0; b < bl.n; ++b) bl.w[b] = (c->weighted && c->mc.n > 0) ? c->mc.w[b] : 1.0;
    if (c->weighted && c->joint) bl.w[1] = c->joint_std[0] / c->joint_std[1];
    return bl;
}

// The tables a layer sums over, as gh_weight's column norms take them: those of Wb A, so the components' weights whether
// or not the context is weighted yet (the joint store's s is not in its column norms, as on the dense store)
static ghk::LatBlocks lattice_tables(const gh_ctx *c)
{
    ghk::LatBlocks bl{};
    bl.n = c->lat->nb;
    for (int b = 0; b < bl.n; ++b) bl.w[b] = c->mc.n > 0 ? c->mc.w[b] : 1.0;
    return bl;
}

// What does not run on the store names it
static int lattice_refuse(gh_ctx *c, const char *who, const char *why)
{
    if (c && c->lat) return fail(c, GH_ERR_UNSUPPORTED, "%s: not supported on %s (%s)", who, LATTICE_NAME, why);
    return GH_OK;
}

// The chain batch runs on the single-block table a context was asked for with gh_set_translation_invariant(2), and on
// the table of blocks asked for with gh_set_cells_multi_table_chains (the one call that sets chains on a multi table)
static bool lattice_chains(const gh_ctx *c) { return c && c->lat && c->lat->runs == GH_TABLE_CHAINS; }
// ... the latter
static bool lattice_multi_chains(const gh_ctx *c) { return lattice_chains(c) && lattice_multi(c); }

// The bootstrap batch runs on the single-block table a context was asked for with gh_set_translation_invariant(4)
static bool lattice_reps(const gh_ctx *c) { return c && c->lat && c->lat->runs == GH_TABLE_REPLICATES; }

// gh_batch_init / gh_batch_trajectory / gh_batch_run: the store's refusal unless the context takes batches
static int lattice_batch_refuse(gh_ctx *c, const char *who)
{
    if (lattice_chains(c)) return GH_OK;
    return lattice_refuse(c, who, "single chain");
}

// The partition of a pass with NRo output rows of NFo outputs and input rows of NFip (padded) inputs
static ghk::LatPlan lat_plan(int NRo, int NFo, int NFip)
{
    ghk::LatPlan p{};
    const int nob = (NFo + ghk::LAT_R - 1) / ghk::LAT_R;
    p.nobt = std::min(64, nob);
    p.TR = std::max(1, std::min(64 / p.nobt, NRo));
    p.FT = (nob + p.nobt - 1) / p.nobt;
    p.WL = NFip + ghk::LAT_R * p.nobt;
    p.lpc = 1;
    return p;
}

static size_t lat_lds_bytes(const ghk::LatPlan &p, int NFip)
{
    return ((size_t)(p.TR + ghk::LAT_G - 1) * (size_t)p.WL + (size_t)ghk::LAT_G * (size_t)NFip +
            (size_t)ghk::LAT_G * 64 * ghk::LAT_R) * sizeof(double);
}

// ------------------------------------------------------------------------ gh_build_G on the table, in its steps

// What the steps hand on
struct LatBuild {
    std::vector<int> col, ool;  // the detection's cell_of_lat, expanded over the layer groups, and its obs_of_lat
    int nzg = 0;                // the geometry's layers
    size_t nT = 0;              // entries of one table: g.nz U V
};

// Detection on the store's points and cells, the dims of the table, the expanded map
static int lattice_geometry(gh_ctx *c, LatBuild &b)
{
    LatticeHost &h = *c->lat;
    const LatForm &f = *h.form;
    h.nr = f.rblocks == PER_COMPONENT ? c->mc.n : f.rblocks;
    h.nb = f.tables == PER_COMPONENT ? c->mc.n : f.tables;
    // (row blocks: the blocks share the N / nb points; layer groups: the M columns are groups of the same M / groups cells)
    const int64_t Np = store_points(c), m = store_cells(c);
    std::vector<double> ox((size_t)Np), oy((size_t)Np), oz((size_t)Np), b6((size_t)m * 6);
    TRY(d2h(c, ox.data(), c->obs[0], ox.size()));
    TRY(d2h(c, oy.data(), c->obs[1], oy.size()));
    TRY(d2h(c, oz.data(), c->obs[2], oz.size()));
    TRY(d2h(c, b6.data(), c->bounds, b6.size()));
    int dims[5] = {0, 0, 0, 0, 0};
    std::vector<int> loc, loo;
    const int reason = lattice_detect_host(Np, ox.data(), oy.data(), oz.data(), m, b6.data(), dims, loc, b.col, loo, b.ool);
    if (reason != GH_LATTICE_ON)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s needs a regular prism grid under gridded data: %s", f.build_name,
                    lattice_reason_text(reason));
    ghk::LatGeom &g = h.g;
    g.nx = dims[0];
    g.ny = dims[1];
    b.nzg = dims[2];
    g.nz = f.groups * b.nzg;
    // the expanded map: layer grp nz + k holds the columns grp m + cell of the geometry's layer k
    b.col.resize((size_t)c->M);
    for (int grp = 1; grp < f.groups; ++grp)
        for (int64_t e = 0; e < m; ++e) b.col[(size_t)(grp * m + e)] = (int)(grp * m) + b.col[(size_t)e];
    g.px = dims[3];
    g.qy = dims[4];
    g.U = g.nx + g.px - 1;
    g.V = g.ny + g.qy - 1;
    g.nyp = (g.ny + 7) / 8 * 8;
    g.qyp = (g.qy + 7) / 8 * 8;
    b.nT = (size_t)g.nz * (size_t)g.U * (size_t)g.V;
    if (b.nT > (size_t)INT_MAX * 4)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s: a table of %zu entries is beyond the fill kernel's grid", LATTICE_NAME, b.nT);
    return GH_OK;
}

// The partition of the two passes and their LDS: arithmetic on the dims, the CUs and the form, nothing else touched.
// Returns whether both tiles are within the 160 KB of a workgroup.
static bool lattice_partition(LatticeHost &h, int cus)
{
    const ghk::LatGeom &g = h.g;
    h.adj = lat_plan(g.nx, g.ny, g.qyp);
    h.fwd = lat_plan(g.px, g.qy, g.nyp);
    h.lds_adj = lat_lds_bytes(h.adj, g.qyp);
    h.lds_fwd = lat_lds_bytes(h.fwd, g.nyp);
    h.gx_adj = (g.nx + h.adj.TR - 1) / h.adj.TR * h.adj.FT;
    h.gx_fwd = (g.px + h.fwd.TR - 1) / h.fwd.TR * h.fwd.FT;
    // forward: chunks of layers, one slab row each -- about four workgroups per CU, no more rows than layers
    // (row blocks: nb gx_fwd workgroups per chunk)
    const int per = h.nb * h.gx_fwd;
    const int want = std::max(1, std::min(g.nz, (4 * cus + per - 1) / per));
    h.fwd.lpc = (g.nz + want - 1) / want;
    h.chunks = (g.nz + h.fwd.lpc - 1) / h.fwd.lpc;
    if (h.form->cut) {
        // a chunk sums into the slab row of ONE observation block, so the chunks of that many layers are cut per layer
        // group -- the same number for each, the first slab rows the first group's
        const int nzg = g.nz / h.form->groups;
        h.fwd.lpc = std::min(h.fwd.lpc, nzg);
        h.chunks = h.form->groups * ((nzg + h.fwd.lpc - 1) / h.fwd.lpc);
    }
    return h.lds_adj <= 160 * 1024 && h.lds_fwd <= 160 * 1024;
}

// The launches that fill the form's store, in their order on the stream: T the entry of the first pair of every offset,
// T2, laid out as T, the entry of the last
static std::vector<std::function<void()>> lattice_fills(gh_ctx *c, const LatBuild &b, double *T2)
{
    const LatticeHost &h = *c->lat;
    const ghk::LatGeom g = h.g;
    double *const T = h.T;
    std::vector<std::function<void()>> fills;
    // lat_fill_kernel<E> with the entry function of the context mg describes, over the layers of lg, at `off` of the store
    auto table = [&](lat_fill_fn fn, const MfGeom &mg, const ghk::LatGeom &lg, size_t off) {
        const unsigned blocks = (unsigned)(((size_t)lg.nz * (size_t)lg.U * (size_t)lg.V + 255) / 256);
        fills.push_back([=] { hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, c->stream, mg, lg, T + off, T2 + off); });
    };
    // (the geometry's own layers: the first group of the expanded map)
    ghk::LatGeom gg = g;
    gg.nz = b.nzg;
    const size_t nTg = (size_t)b.nzg * (size_t)g.U * (size_t)g.V;
    MfGeom mg = mf_geom(c);
    switch ((int)(h.form - LAT_FORMS)) {
    case LAT_SCALAR:
        table(mf_pick<lat_fill_fn>(c, ghk::lat_fill_kernel<MF_E_GEN>, ghk::lat_fill_kernel<MF_E_TF>, ghk::lat_fill_kernel<MF_E_COMP>,
                                   ghk::lat_fill_kernel<MF_E_GEN>), mg, g, 0);
        break;
    case LAT_MULTI:
        // block after block, each with the entry function of a gh_set_cells_prism context of its component at the points
        // the blocks share (gz is the GH_CELL_PRISM context's entry, as gh_set_cells_prism makes it: not among the
        // run-time components)
        mg.N = store_points(c);
        for (int blk = 0; blk < h.nb; ++blk) {
            const bool gz = c->mc.comp[blk] == GH_COMP_GZ;
            mg.kind = gz ? GH_CELL_PRISM : GH_CELL_PRISM_COMP;
            mg.comp = c->mc.comp[blk];
            table(gz ? ghk::lat_fill_kernel<MF_E_GEN> : ghk::lat_fill_kernel<MF_E_COMP>, mg, g, (size_t)blk * b.nT);
        }
        break;
    case LAT_MVI:
        // one launch over the geometric offsets writes every (data block, axis) table (latmvi.hip.h)
        fills.push_back([=] {
            ghk::lat_fill_mvi_kernel<<<dim3((unsigned)((nTg + 255) / 256)), dim3(256), 0, c->stream>>>(
                c->obs[0], c->obs[1], c->obs[2], c->bounds, g, gg.nz, make_double3(c->tf_dir[0], c->tf_dir[1], c->tf_dir[2]),
                block_comps(c), T, T2);
        });
        break;
    case LAT_JOINT:
        // the gz table of a gh_set_cells_prism context on the geometry, then the tf table of a gh_set_cells_tf context,
        // each by that context's launch over the geometry's layers
        mg.N = store_points(c);
        mg.M = store_cells(c);
        mg.kind = GH_CELL_PRISM;
        table(ghk::lat_fill_kernel<MF_E_GEN>, mg, gg, 0);
        mg.kind = GH_CELL_PRISM_TF;
        mg.o3 = c->tf_dir_d;
        table(ghk::lat_fill_kernel<MF_E_TF>, mg, gg, nTg);
        break;
    }
    return fills;
}

// The store's parts (LatForm::rblocks), T against T2: the deviation of a part as a fraction of its own largest entry,
// the largest over the parts kept
static int lattice_deviation(gh_ctx *c, const LatBuild &b, const double *T2)
{
    LatticeHost &h = *c->lat;
    const size_t n = (size_t)h.nb * b.nT / (size_t)h.nr;
    std::vector<double> t1(n), t2(n);
    h.max_dev = 0.0;
    hipError_t e = hipGetLastError();  // (the fills')
    for (int q = 0; q < h.nr; ++q) {
        if (e == hipSuccess) e = hipMemcpyAsync(t1.data(), h.T + (size_t)q * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(t2.data(), T2 + (size_t)q * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess)
            return fail(c, GH_ERR_HIP, "gh_build_G: %s: fill of the table: %s", LATTICE_NAME, hipGetErrorString(e));
        double tmax = 0.0, dmax = 0.0;
        for (size_t i = 0; i < n; ++i) {
            tmax = std::max(tmax, std::fabs(t1[i]));
            dmax = std::max(dmax, std::fabs(t2[i] - t1[i]));
        }
        h.max_dev = std::max(h.max_dev, tmax > 0.0 ? dmax / tmax : (dmax > 0.0 ? HUGE_VAL : 0.0));
    }
    return GH_OK;
}

// gh_build_G of a context with the store switched on: detect, partition, allocate, fill, check
static int lattice_build(gh_ctx *c)
{
    LatticeHost &h = *c->lat;
    ghk::LatGeom &g = h.g;
    const auto t0 = std::chrono::steady_clock::now();
    LatBuild b;
    TRY(lattice_geometry(c, b));
    if (!lattice_partition(h, c->cus))
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s: %s (%d cells, %d observations along y: %zu bytes)", LATTICE_NAME,
                    lattice_reason_text(GH_LATTICE_LDS), g.ny, g.qy, std::max(h.lds_adj, h.lds_fwd));
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(h.form->adj), h.lds_adj));
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(h.form->fwd), h.lds_fwd));
    TRY(dalloc(c, &h.T, (size_t)h.nb * b.nT, false));
    TRY(dalloc(c, &h.cell_of, (size_t)c->M, false));
    TRY(dalloc(c, &h.obs_of, b.ool.size(), false));
    // (zeroed: the padding stays zero)
    TRY(dalloc(c, &g.rl, (size_t)h.nr * (size_t)g.px * (size_t)g.qyp));
    TRY(dalloc(c, &g.xl, (size_t)c->M / (size_t)g.ny * (size_t)g.nyp));
    // (b.col / b.ool outlive their copies: lattice_deviation waits for the stream)
    HIPCHK(c, hipMemcpyAsync(h.cell_of, b.col.data(), sizeof(int) * b.col.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.obs_of, b.ool.data(), sizeof(int) * b.ool.size(), hipMemcpyHostToDevice, c->stream));
    g.T = h.T;
    g.cell_of = h.cell_of;
    g.obs_of = h.obs_of;
    // (T2, laid out as T: released on every way out)
    double *T2p = nullptr;
    HIPCHK(c, hipMalloc((void **)&T2p, (size_t)h.nb * b.nT * sizeof(double)));
    const std::unique_ptr<double, hipError_t (*)(void *)> T2(T2p, hipFree);
    for (const auto &launch : lattice_fills(c, b, T2.get())) launch();
    TRY(lattice_deviation(c, b, T2.get()));
    h.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!(h.max_dev <= FOLD_MAX_DEV))
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s: %s (%.3g of the largest entry)", LATTICE_NAME,
                    lattice_reason_text(GH_LATTICE_DEVIATION), h.max_dev);
    h.on = true;
    return GH_OK;
}

// configure_mf of the store: slab rows = chunks of layers, |p|^2 partials = the adjoint's workgroups
static int lattice_configure(gh_ctx *c)
{
    const LatticeHost &h = *c->lat;
    return set_partition(c, "lattice_configure", h.chunks, (int64_t)h.gx_adj * h.g.nz);
}

// The form's two passes, each behind its gather.  The adjoint's grid is the single table's -- blocks of r run inside the
// kernel, or a layer picks its own -- and the forward takes the table as its third grid coordinate under one gather of x
static int launch_lattice(gh_ctx *c, SweepArgs &a, const double *wm)
{
    const LatticeHost &h = *c->lat;
    const ghk::LatGeom &g = h.g;
    const ghk::LatBlocks bl = lattice_r_blocks(c);
    if (a.mode & SW_ADJ) {
        ghk::lat_gather_r_blocks_kernel<<<dim3((unsigned)((c->N + 255) / 256)), dim3(256), 0, c->stream>>>(g, bl, a.r);
        hipLaunchKernelGGL(h.form->adj, dim3((unsigned)h.gx_adj, (unsigned)g.nz), dim3(ghk::LAT_THREADS), h.lds_adj, c->stream, g,
                           h.adj, a, wm, c->ld, bl);
    }
    if (a.mode & SW_FWD) {
        const double *x = (a.mode & SW_UPD) ? a.x_out : a.x_in;
        ghk::lat_gather_x_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(g, x, wm);
        hipLaunchKernelGGL(h.form->fwd, dim3((unsigned)h.gx_fwd, (unsigned)h.chunks, (unsigned)h.nb), dim3(ghk::LAT_THREADS),
                           h.lds_fwd, c->stream, g, h.fwd, a, wm, c->ld, bl);
    }
    return GH_OK;
}

// ------------------------------------------------------------------------ chain batches (latbatch.hip.h)

// The partition of a batch pass with NFo outputs along the fast axis and input rows of NFip (padded) inputs
static ghk::LatbPlan latb_pass_plan(int NFo, int NFip)
{
    ghk::LatbPlan p{};
    p.ntiles = (NFo + 15) / 16;
    p.FT = (p.ntiles + ghk::LATB_NT - 1) / ghk::LATB_NT;
    p.WT = 16 * ((p.ntiles + p.FT - 1) / p.FT);
    p.WL = NFip + p.WT;
    p.lpc = 1;
    return p;
}

constexpr size_t LATB_LDS_MAX = 160 * 1024;  // LDS of a workgroup on gfx950

static size_t latb_lds_bytes(const ghk::LatbPlan &p, int NFip)
{
    return ((size_t)ghk::LATB_TR * (size_t)p.WL + (size_t)ghk::CB * (size_t)NFip) * sizeof(double);
}

// The partition of the two batch passes on the built table: arithmetic only, made once, nothing else of the context
// touched.  The kernels have no static LDS, so a pass fits where its tile, 192 NFip + 64 WT bytes, is within the 160 KB
// of a workgroup.  Returns whether both passes fit.
static bool latb_plan_make(gh_ctx *c)
{
    LatticeHost &h = *c->lat;
    const ghk::LatGeom &g = h.g;
    if (h.bt_state == 0) {
        h.badj = latb_pass_plan(g.ny, g.qyp);
        h.bfwd = latb_pass_plan(g.qy, g.nyp);
        h.blds_adj = latb_lds_bytes(h.badj, g.qyp);
        h.blds_fwd = latb_lds_bytes(h.bfwd, g.nyp);
        h.bgx_adj = (g.nx + ghk::LATB_TR - 1) / ghk::LATB_TR * h.badj.FT;
        h.bgx_fwd = (g.px + ghk::LATB_TR - 1) / ghk::LATB_TR * h.bfwd.FT;
        // forward: chunks of layers, one slab row each -- about four workgroups per CU, no more rows than layers
        // (row blocks: nb bgx_fwd workgroups per chunk)
        const int per = h.nb * h.bgx_fwd;
        const int want = std::max(1, std::min(std::min(g.nz, ghk::LATB_MAX_CHUNKS), (4 * c->cus + per - 1) / per));
        h.bfwd.lpc = (g.nz + want - 1) / want;
        h.bchunks = (g.nz + h.bfwd.lpc - 1) / h.bfwd.lpc;
        h.bt_state = (h.blds_adj > LATB_LDS_MAX || h.blds_fwd > LATB_LDS_MAX) ? -1 : 1;
    }
    return h.bt_state > 0;
}

// An extent the batch tile cannot hold: GH_ERR_UNSUPPORTED, whoever asks
static int latb_plan(gh_ctx *c, const char *who)
{
    if (latb_plan_make(c)) return GH_OK;
    const LatticeHost &h = *c->lat;
    return fail(c, GH_ERR_UNSUPPORTED, "%s: %s on %s: %s (%d cells, %d observations along y: %zu bytes)", who,
                lattice_reps(c) ? "the bootstrap batch" : "chain batches", LATTICE_NAME,
                "a row of the lattice is too long for the batch pass's LDS tile", h.g.ny, h.g.qy,
                std::max(h.blds_adj, h.blds_fwd));
}

// batch_alloc of the store: the plan, the passes' LDS, the two gathered operands and what the schedules size by
static int latb_alloc(gh_ctx *c)
{
    LatticeHost &h = *c->lat;
    gh_ctx::Batch &b = c->bt;
    const ghk::LatGeom &g = h.g;
    TRY(latb_plan(c, lattice_reps(c) ? "gh_bscg_run" : "gh_batch_init"));
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(ghk::latb_pass_kernel<ghk::LATB_ADJ>), h.blds_adj));
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(ghk::latb_pass_kernel<ghk::LATB_CG>), h.blds_adj));
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(ghk::latb_pass_kernel<ghk::LATB_FWD>), h.blds_fwd));
    if (lattice_multi(c)) {
        HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(ghk::latb_pass_kernel<ghk::LATB_ADJ_MB>), h.blds_adj));
        HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(ghk::latb_pass_kernel<ghk::LATB_FWD_MB>), h.blds_fwd));
        TRY(dalloc(c, &b.bmean, (size_t)ghk::CB * (size_t)h.nb));
    }
    TRY(dalloc(c, &h.xl16, (size_t)g.nz * (size_t)g.nx * (size_t)g.nyp * ghk::CB));  // (zeroed: the padding stays zero)
    TRY(dalloc(c, &h.rl16, (size_t)h.nb * (size_t)g.px * (size_t)g.qyp * ghk::CB));  // (row blocks: [b][px][qyp][16])
    TRY(dalloc(c, &b.iw, (size_t)c->M));
    b.n_waves = h.bgx_adj * g.nz;  // rows of pp_part: one per workgroup of the adjoint
    b.n_colblocks = h.bchunks;
    b.slab_live = h.bchunks;
    b.cols_per_block = 0;
    b.fus_on = false;
    b.mfb_near = false;
    return GH_OK;
}

// forward of all chains at X into the slab: gather + pass
static void latb_launch_forward(gh_ctx *c, const double *X)
{
    const LatticeHost &h = *c->lat;
    const ghk::LatGeom &g = h.g;
    gh_ctx::Batch &b = c->bt;
    const int64_t n16 = c->M * ghk::CB;
    ghk::latb_gather_x_kernel<<<dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream>>>(g, X, b.iw, h.xl16);
    if (lattice_multi(c)) {
        // (row blocks: the block as the grid's third coordinate, under the one gather of X)
        ghk::LatbBlockArgs ba{};
        ba.bl = lattice_r_blocks(c);
        hipLaunchKernelGGL(ghk::latb_pass_kernel<ghk::LATB_FWD_MB>, dim3((unsigned)h.bgx_fwd, (unsigned)h.bchunks, (unsigned)h.nb),
                           dim3(ghk::LATB_THREADS), h.blds_fwd, c->stream, g, h.bfwd, h.xl16, ba, b.iw, b.slab, c->ld);
    } else {
        hipLaunchKernelGGL(ghk::latb_pass_kernel<ghk::LATB_FWD>, dim3((unsigned)h.bgx_fwd, (unsigned)h.bchunks),
                           dim3(ghk::LATB_THREADS), h.blds_fwd, c->stream, g, h.bfwd, h.xl16, ghk::BatchAdjArgs{}, b.iw, b.slab,
                           c->ld);
    }
    b.slab_live = h.bchunks;
}

// adjoint of all chains + the per-chain update: gather + pass
static void latb_launch_adjoint(gh_ctx *c, const ghk::BatchAdjArgs &a)
{
    const LatticeHost &h = *c->lat;
    const ghk::LatGeom &g = h.g;
    const int64_t n16 = c->N * ghk::CB;
    const ghk::LatBlocks bl = lattice_r_blocks(c);
    ghk::latb_gather_r_blocks_kernel<<<dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream>>>(g, bl, a.Rt, h.rl16);
    if (lattice_multi(c)) {
        // (row blocks: the single block's grid, the blocks in turn inside the kernel)
        ghk::LatbBlockArgs ba;
        ba.a = a;
        ba.bl = bl;
        hipLaunchKernelGGL(ghk::latb_pass_kernel<ghk::LATB_ADJ_MB>, dim3((unsigned)h.bgx_adj, (unsigned)g.nz),
                           dim3(ghk::LATB_THREADS), h.blds_adj, c->stream, g, h.badj, h.rl16, ba, c->bt.iw, (double *)nullptr,
                           c->ld);
        return;
    }
    hipLaunchKernelGGL(ghk::latb_pass_kernel<ghk::LATB_ADJ>, dim3((unsigned)h.bgx_adj, (unsigned)g.nz), dim3(ghk::LATB_THREADS),
                       h.blds_adj, c->stream, g, h.badj, h.rl16, a, c->bt.iw, (double *)nullptr, c->ld);
}

// adjoint of all replicates + the CG gradient and its |I|^2 partials (bgx_adj nz rows): gather + pass
static void latb_launch_cg_adjoint(gh_ctx *c, const double *Rt, const ghk::LatbCgArgs &a)
{
    const LatticeHost &h = *c->lat;
    const ghk::LatGeom &g = h.g;
    const int64_t n16 = c->N * ghk::CB;
    ghk::latb_gather_r_blocks_kernel<<<dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream>>>(g, lattice_r_blocks(c), Rt, h.rl16);
    hipLaunchKernelGGL(ghk::latb_pass_kernel<ghk::LATB_CG>, dim3((unsigned)h.bgx_adj, (unsigned)g.nz), dim3(ghk::LATB_THREADS),
                       h.blds_adj, c->stream, g, h.badj, h.rl16, a, c->bt.iw, (double *)nullptr, c->ld);
}
