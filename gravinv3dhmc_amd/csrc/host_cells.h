// libgravhmc host side: what a context holds.  One table with one row per GH_CELL_* kind, the accessors that read it,
// the checks and uploads the gh_set_cells_* entry points share (each written once, taking the caller's name), the
// refusals the stores of blocks answer other calls with, and the assembly of the dense store.  Included once by
// gravhmc.hip.
#pragma once

// the set a store's row blocks draw their components from
enum { COMPS_NONE = 0, COMPS_GRAV, COMPS_MAG };
// whether a store also runs on the shift-invariant table: no; asked for after its cells are set (or with them); any time
enum { TABLE_NO = 0, TABLE_AFTER, TABLE_ANY };

struct CellStore {
    const char *entry;      // the entry point that makes a context of the kind
    const char *name;       // the store as its refusals name it; null: a store of one block, which refuses nothing here
    const char *a_ctx;      // ... and as set_cells sends its caller to `entry`
    const char *rows_name;  // ... and as the calls that look at its rows alone do (the bootstrap batch, gh_set_data)
    int cols;               // column blocks: M = cols x cells
    int comps;              // COMPS_*: row blocks of gravity fields (GH_COMP_*), of magnetic data (GH_BCOMP_*), or none
    bool tess;              // tesseroids; else prisms
    int table;              // TABLE_*
    bool row_limit;         // the dense store's 16384 rows are asked for when the cells are set
};

// (indexed by GH_CELL_*)
static const CellStore CELL_STORES[] = {
    {"gh_set_cells", nullptr, nullptr, nullptr, 1, COMPS_NONE, false, TABLE_NO, false},
    {"gh_set_cells", nullptr, nullptr, nullptr, 1, COMPS_NONE, true, TABLE_ANY, false},
    {"gh_set_cells_tf", nullptr, nullptr, nullptr, 1, COMPS_NONE, false, TABLE_NO, false},
    {"gh_set_cells_prism", nullptr, nullptr, nullptr, 1, COMPS_NONE, false, TABLE_NO, false},
    {"gh_set_cells_tess", nullptr, nullptr, nullptr, 1, COMPS_NONE, true, TABLE_NO, false},
    {"gh_set_cells_joint", "the joint gravity-magnetic kernel", "a joint gravity-magnetic context",
     "the joint gravity-magnetic store", 2, COMPS_NONE, false, TABLE_NO, true},
    {"gh_set_cells_multi", "the multi-component store", "a multi-component context", "the multi-component store", 1,
     COMPS_GRAV, false, TABLE_NO, true},
    {"gh_set_cells_mvi", "the magnetization-vector store", "a magnetization-vector context",
     "the magnetization-vector store", 3, COMPS_NONE, false, TABLE_NO, true},
    // (by their rows, the two stores of magnetic data are the multi-component store)
    {"gh_set_cells_mvi_data", "the vector-data magnetization store", "a vector-data magnetization context",
     "the multi-component store", 3, COMPS_MAG, false, TABLE_NO, true},
    {"gh_set_cells_tess_mag", "the tesseroid magnetization store", "a vector-data magnetization context",
     "the multi-component store", 3, COMPS_MAG, true, TABLE_AFTER, true},
    {"gh_set_cells_tess_multi", "the tesseroid multi-component store", "a tesseroid multi-component context",
     "the tesseroid multi-component store", 1, COMPS_GRAV, true, TABLE_ANY, false},
};
static_assert(sizeof CELL_STORES / sizeof CELL_STORES[0] == GH_CELL_TESSEROID_MULTI + 1, "one row per GH_CELL_* kind");

// (a context without cells yet reads as the plain prism kind: one block each way, no name)
static inline const CellStore &store_of(const gh_ctx *c) { return CELL_STORES[c->cell_kind < 0 ? GH_CELL_PRISM : c->cell_kind]; }
static inline const char *store_name(const gh_ctx *c) { return store_of(c).name; }
// row blocks: the joint store's two fields, a block table's components, else one
static inline int store_blocks(const gh_ctx *c) { return c->joint ? 2 : c->mc.n > 0 ? c->mc.n : 1; }
// the observation points every row block shares, the cells every column block shares
static inline int64_t store_points(const gh_ctx *c) { return c->N / store_blocks(c); }
static inline int64_t store_cells(const gh_ctx *c) { return c->M / store_of(c).cols; }
// The tesseroid forms of the stores of row blocks: the multi-component store's rows assembled by the tesseroid field
// kernels (GH_CELL_TESSEROID_MULTI), and a magnetization vector per cell under row blocks of magnetic data
// (GH_CELL_TESS_MVI_DATA: GH_CELL_PRISM_MVI_DATA but for the assembly); dense, or on the shift-invariant table
static inline bool tess_mag_store(const gh_ctx *c) { return c->cell_kind == GH_CELL_TESS_MVI_DATA; }
static inline bool tess_multi_store(const gh_ctx *c) { return c->cell_kind == GH_CELL_TESSEROID_MULTI && c->mc.n > 0; }

// ------------------------------------------------------------------------- the entry points' checks, each once

static int check_component(gh_ctx *c, const char *who, int set, int comp)
{
    if (set == COMPS_MAG ? comp < GH_BCOMP_TF || comp > GH_BCOMP_BZ : comp < GH_COMP_POTENTIAL || comp > GH_COMP_GZZ)
        return fail(c, GH_ERR_ARG, "%s: component %d is not one of %s", who, comp,
                    set == COMPS_MAG ? "GH_BCOMP_TF (0) .. GH_BCOMP_BZ (3)" : "GH_COMP_POTENTIAL (0) .. GH_COMP_GZZ (10)");
    return GH_OK;
}

// n distinct components of the store's set, each with a finite weight > 0 (and, given ratios, a ratio > 0)
static int check_components(gh_ctx *c, const CellStore &s, int n, const int *comps, const double *weights, const double *ratios)
{
    const int most = s.comps == COMPS_MAG ? GH_BCOMP_MAX : GH_MULTI_MAX;
    if (n < 1 || n > most)
        return fail(c, GH_ERR_ARG, "%s: %d %scomponents: %s takes 1 to %d", s.entry, n, s.comps == COMPS_MAG ? "data " : "",
                    s.name, most);
    for (int b = 0; b < n; ++b) {
        TRY(check_component(c, s.entry, s.comps, comps[b]));
        for (int a = 0; a < b; ++a)
            if (comps[a] == comps[b]) return fail(c, GH_ERR_ARG, "%s: component %d is listed twice", s.entry, comps[b]);
        if (!(weights[b] > 0.0) || !std::isfinite(weights[b]))
            return fail(c, GH_ERR_ARG, "%s: the data weights must be finite and > 0", s.entry);
        if (ratios && !(ratios[b] > 0)) return fail(c, GH_ERR_ARG, "Invalid ratio %g. Must be > 0.", ratios[b]);
    }
    return GH_OK;
}

// w <= e, s <= n, top >= bottom: the reference's assertion (tesseroid.py:137-138)
static int check_tess_bounds(gh_ctx *c, const char *who, const double *bounds6, int64_t cells)
{
    for (int64_t j = 0; j < cells; ++j) {
        const double *b = bounds6 + 6 * j;
        if (!(b[0] <= b[1] && b[2] <= b[3] && b[4] >= b[5]))
            return fail(c, GH_ERR_ARG, "%s: invalid tesseroid dimensions (cell %lld: %g %g %g %g %g %g)", who, (long long)j,
                        b[0], b[1], b[2], b[3], b[4], b[5]);
    }
    return GH_OK;
}

static int check_direction(gh_ctx *c, const char *who, const double *dir)
{
    if (!std::isfinite(dir[0]) || !std::isfinite(dir[1]) || !std::isfinite(dir[2]))
        return fail(c, GH_ERR_ARG, "%s: the field direction must be finite", who);
    return GH_OK;
}

// What a store of blocks asks of the context it is set on: nothing set yet, none of the forms it does not run on, one
// GPU.  (name: the store, as its entry point calls it)
static int check_context(gh_ctx *c, const CellStore &s, const char *name)
{
    static const char *const forms[] = {
        "is dense only (no matrix-free mode, no shift-invariant store)",
        // (a context of unknown kind cannot be asked onto the table)
        "has no matrix-free mode, and takes the shift-invariant table after this call (gh_set_shift_invariant) or with it "
        "(gh_set_cells_tess_mag_table)",
        // (the table may have been asked for already: it is the one form besides the dense store)
        "has no matrix-free mode (dense, or the shift-invariant store)"};
    if (c->joint || c->mvi || c->mc.n > 0 || c->have_obs || c->have_cells || c->have_G || c->work_ready)
        return fail(c, GH_ERR_ARG, "%s: call it first on a fresh context (before gh_set_obs)", s.entry);
    if (s.table == TABLE_ANY ? c->mf && !c->ls : c->mf || c->ls)
        return fail(c, GH_ERR_UNSUPPORTED, "%s: %s %s", s.entry, name, forms[s.table]);
    if (c->sh.kind != 0) return fail(c, GH_ERR_UNSUPPORTED, "%s: %s is not sharded", s.entry, name);
    return GH_OK;
}

// the fused sweep's 16384 rows; ncomp 0: a store without a block table.  (A store that also runs on the table: its
// dense form.)
static int check_row_limit(gh_ctx *c, const CellStore &s, int ncomp)
{
    if (c->N <= 16384) return GH_OK;
    char rows[96];
    if (ncomp > 0)
        snprintf(rows, sizeof rows, "%d components x %lld observations = %lld rows", ncomp, (long long)(c->N / ncomp),
                 (long long)c->N);
    else
        snprintf(rows, sizeof rows, "N = %lld observations", (long long)c->N);
    const bool t = s.table != TABLE_NO;
    return fail(c, GH_ERR_UNSUPPORTED, "%s: %s: %s%s takes at most 16384 (it runs on the fused sweep: no row panels, no team "
                                       "sweep)%s", s.entry, rows, t ? "the dense form of " : "", s.name,
                t ? "; the shift-invariant table has no such limit (gh_set_cells_tess_mag_table)" : "");
}

// ------------------------------------------------------------------------- ... and their uploads

// The bounds of `cells` cells (in a buffer of `room` cells, where that is more) and, given one, the field direction
static int upload_cells(gh_ctx *c, const double *bounds6, int64_t cells, const double *dir, int64_t room = 0)
{
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dalloc(c, &c->bounds, (size_t)std::max(cells, room) * 6));
    TRY(h2d(c, c->bounds, bounds6, (size_t)cells * 6));
    if (dir) {
        std::copy(dir, dir + 3, c->tf_dir);
        TRY(dalloc(c, &c->tf_dir_d, 3));
        TRY(h2d(c, c->tf_dir_d, c->tf_dir, 3));
    }
    return GH_OK;
}

// ------------------------------------------------------------------------- what the stores of blocks refuse

// A context of a store of blocks takes its cells from the store's own entry point, not from set_cells
static int refuse_plain_cells(gh_ctx *c)
{
    const CellStore &s = store_of(c);
    if (s.name) return fail(c, GH_ERR_UNSUPPORTED, "%s takes its cells from %s", s.a_ctx, s.entry);
    return GH_OK;
}

// The stores that are dense and run one chain -- the joint gravity-magnetic store, the multi-component stores and the
// magnetization-vector stores -- refuse `who`, each naming itself.  (The tesseroid forms also run on the
// shift-invariant table, the prisms' multi-component store on the translation-invariant one: still one chain, no
// other form.)
static bool lattice_own(const gh_ctx *c);  // host_lattice.h: a store set onto the translation-invariant table with its cells
// ... with gh_set_cells_multi_table_chains: the table of blocks that takes chain batches.  Not a single-chain store;
// what it does not run either, the table's own refusals name (lattice_refuse and its kin)
static bool lattice_multi_chains(const gh_ctx *c);
static int dense_single_chain_refuse(gh_ctx *c, const char *who)
{
    if (c && store_name(c) && !lattice_multi_chains(c))
        return fail(c, GH_ERR_UNSUPPORTED, "%s: not supported on %s (%s, single chain)", who, store_name(c),
                    store_of(c).table != TABLE_NO           ? "dense or shift-invariant"
                    : lattice_own(c)                        ? "dense or on the translation-invariant table"
                                                            : "dense");
    return GH_OK;
}

// ------------------------------------------------------------------------- what a tesseroid pass reports

// The two device buffers a pass of the tesseroid engine reports into -- the error codes summed per cell, the leaf count
// with the overflow flag -- from their allocation to their release on every way out.  open() allocates and zeroes them
// on the context's stream; the caller launches its kernels with err_cell and stats; harvest() waits for them.
struct TessHarvest {
    int *err_cell = nullptr;
    TessStats *stats = nullptr;
    int64_t cells = 0;
    TessHarvest() = default;
    TessHarvest(const TessHarvest &) = delete;
    TessHarvest &operator=(const TessHarvest &) = delete;
    ~TessHarvest()
    {
        (void)hipFree(err_cell);
        (void)hipFree(stats);
    }
    int open(gh_ctx *c, const char *who, int64_t n_cells)
    {
        cells = n_cells;
        if (hipMalloc((void **)&err_cell, sizeof(int) * (size_t)std::max<int64_t>(cells, 1)) != hipSuccess ||
            hipMalloc((void **)&stats, sizeof(TessStats)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, GH_ERR_NOMEM, "%s: device allocation of the tesseroid pass's buffers failed", who);
        }
        HIPCHK(c, hipMemsetAsync(err_cell, 0, sizeof(int) * (size_t)cells, c->stream));
        HIPCHK(c, hipMemsetAsync(stats, 0, sizeof(TessStats), c->stream));
        return GH_OK;
    }
    // After the launch: the cells with a non-zero code and the leaves of the pass; GH_ERR_OVERFLOW when a stack was full
    // (the counts are then the pass's all the same; any other error leaves them as they are).
    int harvest(gh_ctx *c, int64_t &flagged, int64_t &leaves)
    {
        HIPCHK(c, hipGetLastError());
        std::vector<int> herr((size_t)cells);
        TessStats hs{};
        HIPCHK(c, hipMemcpyAsync(herr.data(), err_cell, sizeof(int) * (size_t)cells, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&hs, stats, sizeof hs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        flagged = (int64_t)std::count_if(herr.begin(), herr.end(), [](int v) { return v != 0; });
        leaves = (int64_t)hs.leaves;
        if (hs.overflow) return fail(c, GH_ERR_OVERFLOW, "tesseroid stack overflow (> %d entries)", TESS_STACK);
        return GH_OK;
    }
};

// ------------------------------------------------------------------------- the assembly of the dense store

// tess_comp_kernel of one field at one ratio over all (observation, cell) pairs: `rows` rows of every column of the
// store from G on (the N observations' entries, then zeros) when G is given, else the statistics alone; warn_cells
// and leaves are added to the context's counts (gh_build_G zeroes them), GH_ERR_OVERFLOW.  conv: the converted
// observations (lon rad, sin lat, cos lat, radius; N each).
static int tess_comp_assemble(gh_ctx *c, const double *conv, double *G, int comp, double ratio, int64_t N, int64_t rows)
{
    typedef void (*tc_fn)(const double *, const double *, const double *, const double *, const double *, int64_t,
                          int64_t, int64_t, int64_t, double, int, double *, int *, TessStats *);
    // (indexed by GH_COMP_*: one instantiation per leaf, the geoid runs the potential's)
    static const tc_fn fns[] = {tess_comp_kernel<GH_COMP_POTENTIAL>, tess_comp_kernel<GH_COMP_POTENTIAL>,
                                tess_comp_kernel<GH_COMP_GX>,        tess_comp_kernel<GH_COMP_GY>,
                                tess_comp_kernel<GH_COMP_GZ>,        tess_comp_kernel<GH_COMP_GXX>,
                                tess_comp_kernel<GH_COMP_GXY>,       tess_comp_kernel<GH_COMP_GXZ>,
                                tess_comp_kernel<GH_COMP_GYY>,       tess_comp_kernel<GH_COMP_GYZ>,
                                tess_comp_kernel<GH_COMP_GZZ>};
    TessHarvest h;
    TRY(h.open(c, "gh_build_G", c->M));
    const int64_t blocks = std::min<int64_t>((rows * c->M + 63) / 64, 1 << 24);
    hipLaunchKernelGGL(fns[comp], dim3((unsigned)blocks), dim3(64), 0, c->stream, conv, conv + N, conv + 2 * N, conv + 3 * N,
                       (const double *)c->bounds, N, c->M, rows, c->ld, ratio, comp, G, h.err_cell, h.stats);
    int64_t flagged = 0, leaves = 0;
    const int rc = h.harvest(c, flagged, leaves);
    c->warn_cells += flagged;
    c->leaves += leaves;
    return rc;
}

// prism_kernel of one field (GH_COMP_*, or PRISM_TF) into `rows` rows of every column of the dense store, from G on:
// the first N of them the observations' entries, the rest zero.
static int prism_assemble(gh_ctx *c, int field, int64_t N, int64_t rows, double *G)
{
    typedef void (*prism_fn)(const double *, const double *, const double *, const double *, int64_t, int64_t,
                             int64_t, double3, double *, int64_t);
    // (indexed by GH_COMP_*, then the total field)
    static const prism_fn fns[] = {prism_kernel<GH_COMP_POTENTIAL>, prism_kernel<GH_COMP_GEOID>,
                                   prism_kernel<GH_COMP_GX>,        prism_kernel<GH_COMP_GY>,
                                   prism_kernel<GH_COMP_GZ>,        prism_kernel<GH_COMP_GXX>,
                                   prism_kernel<GH_COMP_GXY>,       prism_kernel<GH_COMP_GXZ>,
                                   prism_kernel<GH_COMP_GYY>,       prism_kernel<GH_COMP_GYZ>,
                                   prism_kernel<GH_COMP_GZZ>,       prism_kernel<PRISM_TF>};
    const int64_t blocks = std::min<int64_t>((rows * c->M + 255) / 256, 1 << 22);
    hipLaunchKernelGGL(fns[field], dim3((unsigned)blocks), dim3(256), 0, c->stream, c->obs[0], c->obs[1], c->obs[2],
                       (const double *)c->bounds, N, c->M, rows, make_double3(c->tf_dir[0], c->tf_dir[1], c->tf_dir[2]), G,
                       c->ld);
    HIPCHK(c, hipGetLastError());
    return GH_OK;
}

// One pass of the tesseroid magnetization kernels over all (observation point, cell) pairs: the converted
// observations (tess_convert_kernel with sin / cos of the longitude), the cells' frames (tess_mag_cellframe_kernel),
// then `launch`; warn_cells, leaves and GH_ERR_OVERFLOW as tess_comp_assemble reports them.
static int tess_mag_pass(gh_ctx *c, const char *who, const std::function<void(const TessMagObs &, const double *, int *, TessStats *)> &launch)
{
    const int64_t m = store_cells(c), Nb = store_points(c);
    struct Buf {
        double *p = nullptr;
        ~Buf() { (void)hipFree(p); }
    } buf;
    HIPCHK(c, hipMalloc((void **)&buf.p, sizeof(double) * (size_t)(6 * Nb + TESS_MAG_FRAME * m)));
    TessHarvest h;
    TRY(h.open(c, who, m));
    double *o6 = buf.p, *frame = buf.p + 6 * Nb;
    const TessMagObs o{o6, o6 + Nb, o6 + 2 * Nb, o6 + 3 * Nb, o6 + 4 * Nb, o6 + 5 * Nb};
    tess_convert_kernel<<<dim3((unsigned)((Nb + 255) / 256)), dim3(256), 0, c->stream>>>(
        c->obs[0], c->obs[1], c->obs[2], Nb, o6, o6 + Nb, o6 + 2 * Nb, o6 + 3 * Nb, o6 + 4 * Nb, o6 + 5 * Nb);
    tess_mag_cellframe_kernel<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream>>>(c->bounds, m, frame);
    launch(o, frame, h.err_cell, h.stats);
    return h.harvest(c, c->warn_cells, c->leaves);
}

// the data components of a store of magnetic data, as its assembly kernels take them
static BComps block_comps(const gh_ctx *c)
{
    BComps bc{};
    bc.n = c->mc.n;
    for (int b = 0; b < bc.n; ++b) bc.comp[b] = c->mc.comp[b];
    return bc;
}

// The dense store G (ld x M) of the context's kind.  The stores of one field per row block -- a single block too, with
// the context's own component and ratio -- run the field's assembly once per block into its rows of the one store; the
// last block's launch also zeroes the padding rows below it.
static int build_dense(gh_ctx *c)
{
    TRY(dalloc(c, &c->G, (size_t)c->ld * (size_t)c->M, false));
    const int nb = store_blocks(c);
    const int64_t m = store_cells(c), Nb = store_points(c);
    const bool table = c->mc.n > 0;
    // (the stores of magnetic data: the threads behind a column's Nb points zero the padding rows below the stack)
    const int64_t Lr = Nb + (c->ld - c->N);
    const double3 dir = make_double3(c->tf_dir[0], c->tf_dir[1], c->tf_dir[2]);
    switch (c->cell_kind) {
    case GH_CELL_PRISM_JOINT: {
        // both blocks of H = [A_gz | A_tf] in one launch (ld rows of N/2 observations, m = M/2 cells each)
        const int64_t blocks = std::min<int64_t>((c->ld * m + 255) / 256, 1 << 22);
        prism_joint_kernel<<<dim3((unsigned)blocks), dim3(256), 0, c->stream>>>(c->obs[0], c->obs[1], c->obs[2], c->bounds,
                                                                              Nb, m, c->ld, dir, c->G);
        break;
    }
    case GH_CELL_PRISM_MVI: {
        // the three blocks of A = [A_x | A_y | A_z] in one launch (m = M/3 cells, each corner evaluated once)
        const int64_t blocks = std::min<int64_t>((c->ld * m + 255) / 256, 1 << 22);
        prism_mvi_kernel<<<dim3((unsigned)blocks), dim3(256), 0, c->stream>>>(c->obs[0], c->obs[1], c->obs[2], c->bounds,
                                                                            c->N, m, c->ld, dir, c->G);
        break;
    }
    case GH_CELL_PRISM_MVI_DATA: {
        // every (data block, axis block) in one launch (m = M/3 cells, Nb points, each corner evaluated once)
        const int64_t blocks = std::min<int64_t>((Lr * m + 255) / 256, 1 << 22);
        prism_mvi_data_kernel<<<dim3((unsigned)blocks), dim3(256), 0, c->stream>>>(
            c->obs[0], c->obs[1], c->obs[2], c->bounds, Nb, m, c->ld, dir, block_comps(c), c->G);
        break;
    }
    case GH_CELL_TESS_MVI_DATA: {
        // every (data block, axis block) in one launch: one traversal of the subdivision per (point, cell) pair
        const BComps bc = block_comps(c);
        return tess_mag_pass(c, "gh_build_G", [&](const TessMagObs &o, const double *frame, int *err_cell, TessStats *stats) {
            const int64_t blocks = std::min<int64_t>((Lr * m + 63) / 64, 1 << 24);
            tess_mag_kernel<<<dim3((unsigned)blocks), dim3(64), 0, c->stream>>>(
                o, c->bounds, frame, c->tmag_fdir, Nb, m, c->ld, c->ratio, bc, c->G, err_cell, stats);
        });
    }
    case GH_CELL_PRISM:
    case GH_CELL_PRISM_TF:
    case GH_CELL_PRISM_COMP:
    case GH_CELL_PRISM_MULTI:
        for (int b = 0; b < nb; ++b)
            TRY(prism_assemble(c, table ? c->mc.comp[b] : c->cell_kind == GH_CELL_PRISM_TF ? PRISM_TF : c->comp, Nb,
                               b + 1 < nb ? Nb : c->ld - b * Nb, c->G + b * Nb));
        break;
    case GH_CELL_TESSEROID:
    case GH_CELL_TESSEROID_COMP:
    case GH_CELL_TESSEROID_MULTI: {
        // (error cells and leaves summed over the blocks)
        double *conv = nullptr;
        HIPCHK(c, hipMalloc((void **)&conv, sizeof(double) * 4 * (size_t)Nb));
        tess_convert_kernel<<<dim3((unsigned)((Nb + 255) / 256)), dim3(256), 0, c->stream>>>(
            c->obs[0], c->obs[1], c->obs[2], Nb, conv, conv + Nb, conv + 2 * Nb, conv + 3 * Nb);
        int rc = GH_OK;
        for (int b = 0; b < nb && rc == GH_OK; ++b)
            rc = tess_comp_assemble(c, conv, c->G + b * Nb, table ? c->mc.comp[b] : c->comp,
                                    table ? c->mc.ratio[b] : c->ratio, Nb, b + 1 < nb ? Nb : c->ld - b * Nb);
        hipFree(conv);
        return rc;
    }
    default:
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: unknown cell kind %d", c->cell_kind);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}
