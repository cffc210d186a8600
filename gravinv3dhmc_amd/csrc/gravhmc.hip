// libgravhmc: host side of the C-ABI declared in include/gravhmc.h (HIP, gfx950 only).
// One context = one GPU + one stream + one inversion problem resident in HBM.
#include "../../include/gravhmc.h"
#include "kernels.hip.h"
#include "batch.hip.h"
#include "bscg.hip.h"
#include "exchange.hip.h"
#include "resident.hip.h"
#include "resbatch.hip.h"
#include "teamsweep.hip.h"
#include "mfbatch.hip.h"
#include "batchteam.hip.h"
#include "lonsym.hip.h"
#include "lonsymh.hip.h"
#include "lonres.hip.h"
#include "lonsymw.hip.h"
#include "fold.hip.h"
#include "lattice.hip.h"
#include "latmvi.hip.h"
#include "latjoint.hip.h"
#include "latbatch.hip.h"
#include "poststream.hip.h"
#include "tessmag.hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <thread>
#include <vector>

using namespace ghk;
static_assert(COMP_POTENTIAL == GH_COMP_POTENTIAL && COMP_GEOID == GH_COMP_GEOID && COMP_GX == GH_COMP_GX &&
                  COMP_GY == GH_COMP_GY && COMP_GZ == GH_COMP_GZ && COMP_GXX == GH_COMP_GXX && COMP_GXY == GH_COMP_GXY &&
                  COMP_GXZ == GH_COMP_GXZ && COMP_GYY == GH_COMP_GYY && COMP_GYZ == GH_COMP_GYZ &&
                  COMP_GZZ == GH_COMP_GZZ,
              "the kernels' component numbers are the C ABI's GH_COMP_*");
static_assert(MULTI_MAX == GH_MULTI_MAX, "the kernels' row-block table holds the C ABI's GH_MULTI_MAX components");
static_assert(BCOMP_MAX == GH_BCOMP_MAX && BCOMP_MAX <= MULTI_MAX && BCOMP_TF == GH_BCOMP_TF && BCOMP_BX == GH_BCOMP_BX &&
                  BCOMP_BY == GH_BCOMP_BY && BCOMP_BZ == GH_BCOMP_BZ,
              "the kernels' data components are the C ABI's GH_BCOMP_*");

#include "host_rows.h"
#include "host_ctx.h"
#include "host_cells.h"
#include "host_sweep.h"
#include "host_fold.h"
#include "host_lattice.h"
#include "host_lonsym.h"
#include "host_comm.h"
#include "host_wavelet.h"
#include "host_eval.h"
#include "host_poststream.h"
#include "host_resident.h"
#include "host_resbatch.h"
#include "host_lonres.h"
#include "host_batch.h"
#include "host_batchrun.h"
#include "host_bscg.h"
#include "host_chain.h"

extern "C" int gh_chain_feed_close(gh_ctx *c, int64_t *drawn, int64_t *run);
static void feed_free(gh_ctx *c);  // host_feed.h

// ------------------------------------------------------------------------- C-ABI

extern "C" {

const char *gh_last_error(const gh_ctx *ctx)
{
    if (ctx && ctx->feed_open.load(std::memory_order_acquire))
        return "a chain feeder is open on this context: gh_chain_feed_close first";
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int gh_create(gh_ctx **out, int device, int64_t N, int64_t M)
{
    if (!out || N <= 0 || M <= 0) return fail(nullptr, GH_ERR_ARG, "gh_create: bad arguments");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, GH_ERR_HIP, "gh_create: no HIP device available (%s); libgravhmc has no CPU path",
                    hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return fail(nullptr, GH_ERR_ARG, "gh_create: device %d out of range (%d devices)", device, ndev);
    gh_ctx *c = new gh_ctx();
    c->device = device;
    c->N = N;
    c->M = M;
    c->ld = (N + 15) / 16 * 16;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        int rc = fail(nullptr, GH_ERR_HIP, "gh_create: %s", hipGetErrorString(e));
        delete c;
        return rc;
    }
    c->cus = prop.multiProcessorCount;
    int rc = configure_sweep(c);
    if (rc != GH_OK) {
        g_create_error = c->err;
        hipStreamDestroy(c->stream);
        delete c;
        return rc;
    }
    *out = c;
    return GH_OK;
}

void gh_destroy(gh_ctx *c)
{
    if (!c) return;
    gh_chain_feed_close(c, nullptr, nullptr);
    feed_free(c);
    for (gh_ctx *k : c->kids) gh_destroy(k);
    c->kids.clear();
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->sh.comm) {
        std::string err;
        RcclApi *api = rccl_api(err);
        if (api && api->CommDestroy) api->CommDestroy(c->sh.comm);
    }
    if (c->sh.hbuf) hipHostFree(c->sh.hbuf);
    if (c->bt.h) hipHostFree(c->bt.h);
    traj_lists_free(c->rs.lists);
    traj_lists_free(c->rs.ls.lists);
    if (c->ls) {
        traj_lists_free(c->ls->res.lists);
        if (c->ls->res.ev0) hipEventDestroy(c->ls->res.ev0);
        if (c->ls->res.ev1) hipEventDestroy(c->ls->res.ev1);
    }
    for (PinnedBlock &pm : c->pinned) hipHostFree(pm.base);
    for (void *p : c->allocs) hipFree(p);
    if (c->h_scal) hipHostFree(c->h_scal);
    for (hipEvent_t ev : c->ev) hipEventDestroy(ev);
    if (c->copy_ev) hipEventDestroy(c->copy_ev);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    if (c->rs.ev0) hipEventDestroy(c->rs.ev0);
    if (c->rs.ev1) hipEventDestroy(c->rs.ev1);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c->ls;
    delete c->lat;
    delete c;
}

int gh_device_info(const gh_ctx *c, char *name256, int *cus, int64_t *mem_bytes)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return GH_ERR_HIP;
    if (name256) {
        // some ROCm builds leave prop.name empty: fall back to the ISA name
        snprintf(name256, 256, "%s%s%s", prop.name, prop.name[0] ? " " : "AMD Instinct ", prop.gcnArchName);
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (mem_bytes) *mem_bytes = (int64_t)prop.totalGlobalMem;
    return GH_OK;
}

int gh_synchronize(gh_ctx *c)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_set_obs(gh_ctx *c, const double *a, const double *b, const double *cc)
{
    GH_FEED_GUARD(c);
    if (!c || !a || !b || !cc) return fail(c, GH_ERR_ARG, "gh_set_obs: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const double *src[3] = {a, b, cc};
    // (joint store: both blocks share the N/2 points; multi-component store: all blocks share the N/n points)
    const int64_t n = store_points(c);
    for (int i = 0; i < 3; ++i) {
        TRY(dalloc(c, &c->obs[i], (size_t)n));
        TRY(h2d(c, c->obs[i], src[i], (size_t)n));
    }
    // (tesseroids: one height for all observations lets the matrix-free batch hoist what depends on
    // the radius alone out of the entries, mfbatch.hip.h)
    c->obs_h_uniform = true;
    for (int64_t i = 1; i < n && c->obs_h_uniform; ++i) c->obs_h_uniform = cc[i] == cc[0];
    c->obs_h0 = cc[0];
    c->have_obs = true;
    c->fd.detected = 0;
    c->fd.reason = GH_FOLD_UNDECIDED;
    c->G_gen += 1;
    return GH_OK;
}

// The cells and how the kernels read them: the bounds, the kind, the component (GH_COMP_GZ for kinds 0 to 2),
// the tesseroids' ratio and, for the total field, its direction.
static int set_cells(gh_ctx *c, const double *bounds6, int kind, int comp, double ratio, const double *dir = nullptr)
{
    TRY(refuse_plain_cells(c));
    TRY(upload_cells(c, bounds6, c->M, dir));
    c->cell_kind = kind;
    c->comp = comp;
    c->ratio = ratio;
    c->have_cells = true;
    c->fd.detected = 0;
    c->fd.reason = GH_FOLD_UNDECIDED;
    c->G_gen += 1;
    return GH_OK;
}

int gh_set_cells(gh_ctx *c, const double *bounds6, int kind, double ratio)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "gh_set_cells: null pointer");
    if (kind != GH_CELL_PRISM && kind != GH_CELL_TESSEROID)
        return fail(c, GH_ERR_ARG, "gh_set_cells: kind must be 0 (prism) or 1 (tesseroid); the total field, the other "
                                   "gravity fields, the joint, multi-component and magnetization-vector stores have "
                                   "entry points of their own");
    if (kind == GH_CELL_TESSEROID && !(ratio > 0))
        return fail(c, GH_ERR_ARG, "Invalid ratio %g. Must be > 0.", ratio);
    return set_cells(c, bounds6, kind, GH_COMP_GZ, ratio);
}

int gh_set_cells_tf(gh_ctx *c, const double *bounds6, double fx, double fy, double fz)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "gh_set_cells_tf: null pointer");
    const double dir[3] = {fx, fy, fz};
    TRY(check_direction(c, "gh_set_cells_tf", dir));
    return set_cells(c, bounds6, GH_CELL_PRISM_TF, GH_COMP_GZ, c->ratio, dir);
}

// The joint store's cells: dense, or -- on_table -- on the translation-invariant table, where the store has no rows to
// limit (the same checks and the same context otherwise; the geometry is looked at by gh_build_G)
static int set_cells_joint(gh_ctx *c, const double *bounds6, double fx, double fy, double fz, bool on_table)
{
    const CellStore &s = CELL_STORES[GH_CELL_PRISM_JOINT];
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "%s: null pointer", s.entry);
    if (c->N % 2 != 0 || c->M % 2 != 0)
        return fail(c, GH_ERR_ARG, "%s: N and M must be even (the stacked gz + tf lengths)", s.entry);
    const double dir[3] = {fx, fy, fz};
    TRY(check_direction(c, s.entry, dir));
    TRY(check_context(c, s, "the joint kernel"));
    if (c->N / 2 > 16384 && !on_table)
        return fail(c, GH_ERR_UNSUPPORTED, "%s: N/2 = %lld observations: the joint kernel takes at most 16384 (no row "
                                           "panels or team sweep)", s.entry, (long long)(c->N / 2));
    HIPCHK(c, hipSetDevice(c->device));
    // the store has N/2 rows: its ld and the sweep's partition (each block on its own) follow from that
    const int64_t ld0 = c->ld;
    const bool ok0 = c->dense_ok;
    c->joint = true;
    c->ld = (c->N / 2 + 15) / 16 * 16;
    c->dense_ok = true;
    const int rc = configure_sweep(c);
    if (rc != GH_OK) {
        c->joint = false;
        c->ld = ld0;
        c->dense_ok = ok0;
        (void)configure_sweep(c);
        return rc;
    }
    // (bounds: M/2 cells; the kind's data lives with the first half of the context's M)
    TRY(upload_cells(c, bounds6, c->M / 2, dir, c->M));
    c->cell_kind = GH_CELL_PRISM_JOINT;
    c->comp = GH_COMP_GZ;
    c->have_cells = true;
    if (on_table) lattice_switch_on(c, LAT_JOINT, GH_TABLE_SINGLE);
    return GH_OK;
}

int gh_set_cells_joint(gh_ctx *c, const double *bounds6, double fx, double fy, double fz)
{
    GH_FEED_GUARD(c);
    return set_cells_joint(c, bounds6, fx, fy, fz, false);
}

// (the same context as gh_set_cells_joint makes, and that call's name in the refusals)
int gh_set_cells_joint_table(gh_ctx *c, const double *bounds6, double fx, double fy, double fz)
{
    GH_FEED_GUARD(c);
    return set_cells_joint(c, bounds6, fx, fy, fz, true);
}

// What the entry points of the stores of blocks below are called with (null where an entry point has no such argument)
struct BlockCells {
    const double *bounds6, *dir;  // dir: (fx, fy, fz) of the prisms' total field
    int ncomp;
    const int *comps;
    const double *weights, *ratios;  // ratios: one per block (the tesseroid multi-component store)
    double ratio;                    // ... or one for the store (the tesseroid magnetization store)
    const double *fdir;
    // gh_set_cells_tess_mag_table, gh_set_cells_multi_table: onto the store's table -- the shift-invariant one of the
    // tesseroids, the translation-invariant one of the prisms -- in the same call (no limit on the rows)
    bool on_table;
    bool chains = false;  // gh_set_cells_multi_table_chains: the prisms' table of blocks also takes chain batches
};

// The stores of blocks but the joint one, each in the order of its own checks: the component list, the column and row
// blocks, the ratio and the directions, the cells' bounds, the context, the rows; then the uploads and the block table.
static int set_block_cells(gh_ctx *c, int kind, const BlockCells &a)
{
    const CellStore &s = CELL_STORES[kind];
    const bool blocks = s.comps != COMPS_NONE;
    if (blocks) TRY(check_components(c, s, a.ncomp, a.comps, a.weights, a.ratios));
    if (s.cols == 3 && (c->M % 3 != 0 || c->M < 3))
        return fail(c, GH_ERR_ARG, "%s: M = %lld is not three components of the same %s", s.entry, (long long)c->M,
                    s.tess ? "tesseroids" : "prisms");
    if (blocks && c->N % a.ncomp != 0)
        return fail(c, GH_ERR_ARG, "%s: N = %lld is not %d blocks of the same observation points", s.entry, (long long)c->N,
                    a.ncomp);
    const int64_t m = c->M / s.cols, Nb = blocks ? c->N / a.ncomp : c->N;
    if (kind == GH_CELL_TESS_MVI_DATA) {
        if (!(a.ratio > 0)) return fail(c, GH_ERR_ARG, "Invalid ratio %g. Must be > 0.", a.ratio);
        if (!a.fdir && std::find(a.comps, a.comps + a.ncomp, (int)GH_BCOMP_TF) != a.comps + a.ncomp)
            return fail(c, GH_ERR_ARG, "%s: a total-field block needs fdir, one unit vector per observation point", s.entry);
        for (int64_t i = 0; a.fdir && i < 3 * Nb; ++i)
            if (!std::isfinite(a.fdir[i])) return fail(c, GH_ERR_ARG, "%s: the field directions must be finite", s.entry);
    }
    if (a.dir) TRY(check_direction(c, s.entry, a.dir));
    if (s.tess) TRY(check_tess_bounds(c, s.entry, a.bounds6, m));
    TRY(check_context(c, s, s.name));
    if (s.row_limit && !a.on_table) TRY(check_row_limit(c, s, blocks ? a.ncomp : 0));
    // one unweighted block of the field a store of one block holds is that store itself: one block with one mean
    // (on the table it stays a store of one block: gh_set_cells_mvi has no door to the table)
    if (kind == GH_CELL_PRISM_MVI_DATA && a.ncomp == 1 && a.comps[0] == GH_BCOMP_TF && a.weights[0] == 1.0 && !a.on_table)
        return gh_set_cells_mvi(c, a.bounds6, a.dir[0], a.dir[1], a.dir[2]);
    if (kind == GH_CELL_TESSEROID_MULTI && a.ncomp == 1 && a.comps[0] == GH_COMP_GZ && a.weights[0] == 1.0)
        return gh_set_cells(c, a.bounds6, GH_CELL_TESSEROID, a.ratios[0]);  // (kind 1, on either form)
    TRY(upload_cells(c, a.bounds6, m, a.dir));
    if (a.fdir) {
        TRY(dalloc(c, &c->tmag_fdir, (size_t)Nb * 3));
        TRY(h2d(c, c->tmag_fdir, a.fdir, (size_t)Nb * 3));
    }
    // columns: the magnetization-vector store's; rows: the multi-component store's blocks (the tesseroid magnetization
    // store with a single block too: it has no other form)
    c->mvi = s.cols == 3;
    c->mc.n = blocks ? a.ncomp : 0;
    for (int b = 0; b < c->mc.n; ++b) {
        c->mc.comp[b] = a.comps[b];
        c->mc.w[b] = a.weights[b];
        if (a.ratios) c->mc.ratio[b] = a.ratios[b];
    }
    c->cell_kind = kind;
    c->comp = s.comps == COMPS_GRAV ? a.comps[0] : GH_COMP_GZ;
    if (s.tess) c->ratio = a.ratios ? a.ratios[0] : a.ratio;
    c->have_cells = true;
    if (a.on_table && !s.tess) lattice_switch_on(c, s.cols == 3 ? LAT_MVI : LAT_MULTI, a.chains ? GH_TABLE_CHAINS : GH_TABLE_SINGLE);
    return a.on_table && s.tess ? gh_set_shift_invariant(c, 1) : GH_OK;
}

int gh_set_cells_mvi(gh_ctx *c, const double *bounds6, double fx, double fy, double fz)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "gh_set_cells_mvi: null pointer");
    const double dir[3] = {fx, fy, fz};
    return set_block_cells(c, GH_CELL_PRISM_MVI, {bounds6, dir, 0, nullptr, nullptr, nullptr, 0.0, nullptr, false});
}

int gh_set_cells_mvi_data(gh_ctx *c, const double *bounds6, double fx, double fy, double fz, int ncomp, const int *comps,
                          const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_mvi_data: null pointer");
    const double dir[3] = {fx, fy, fz};
    return set_block_cells(c, GH_CELL_PRISM_MVI_DATA, {bounds6, dir, ncomp, comps, weights, nullptr, 0.0, nullptr, false});
}

// (the same context as gh_set_cells_mvi_data makes, and that call's name in the refusals; a single unweighted tf block
// too stays a store of one block here; the geometry is looked at by gh_build_G)
int gh_set_cells_mvi_table(gh_ctx *c, const double *bounds6, double fx, double fy, double fz, int ncomp, const int *comps,
                           const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_mvi_data: null pointer");
    const double dir[3] = {fx, fy, fz};
    return set_block_cells(c, GH_CELL_PRISM_MVI_DATA, {bounds6, dir, ncomp, comps, weights, nullptr, 0.0, nullptr, true});
}

int gh_set_cells_tess_mag(gh_ctx *c, const double *bounds6, double ratio, int ncomp, const int *comps,
                          const double *weights, const double *fdir)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_tess_mag: null pointer");
    return set_block_cells(c, GH_CELL_TESS_MVI_DATA, {bounds6, nullptr, ncomp, comps, weights, nullptr, ratio, fdir, false});
}

// (the same context as gh_set_cells_tess_mag makes, and that call's name in the refusals)
int gh_set_cells_tess_mag_table(gh_ctx *c, const double *bounds6, double ratio, int ncomp, const int *comps,
                                const double *weights, const double *fdir)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_tess_mag: null pointer");
    return set_block_cells(c, GH_CELL_TESS_MVI_DATA, {bounds6, nullptr, ncomp, comps, weights, nullptr, ratio, fdir, true});
}

static const char *const MVI_ONLY = "the amplitude term couples the three blocks of the magnetization-vector store (a "
                                    "GH_CELL_PRISM_MVI, GH_CELL_PRISM_MVI_DATA or GH_CELL_TESS_MVI_DATA context, "
                                    "gh_set_cells_mvi, gh_set_cells_mvi_data, gh_set_cells_tess_mag)";

// amp.sw = 1 / (Wm scale), 0 where Wm is 0: from the weights the store has NOW (gh_weight builds it again)
static int amplitude_weights(gh_ctx *c, double scale)
{
    TRY(dalloc(c, &c->amp.sw, (size_t)c->M));
    std::vector<double> w((size_t)c->M);
    TRY(d2h(c, w.data(), c->wm, (size_t)c->M));
    for (auto &v : w) v = v == 0.0 ? 0.0 : (1.0 / v) / scale;
    return h2d(c, c->amp.sw, w.data(), (size_t)c->M);
}

int gh_set_amplitude(gh_ctx *c, double lambda, double beta, double scale)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!c->mvi) return fail(c, GH_ERR_UNSUPPORTED, "gh_set_amplitude: %s", MVI_ONLY);
    TRY(need(c, c->weighted, "gh_set_amplitude: call gh_weight first (the term acts on mw / Wm)"));
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(c, GH_ERR_ARG, "gh_set_amplitude: lambda must be >= 0");
    if (!(beta > 0.0) || !std::isfinite(beta)) return fail(c, GH_ERR_ARG, "gh_set_amplitude: beta must be > 0");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(c, GH_ERR_ARG, "gh_set_amplitude: scale must be > 0");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(amplitude_weights(c, scale));
    c->amp.lambda = lambda;
    c->amp.beta = beta;
    c->amp.scale = scale;
    c->amp.set = true;
    c->cg.phi_cur = c->cg.phi_last = 0.0;
    c->chain_ready = false;
    return GH_OK;
}

int gh_amplitude_eval(gh_ctx *c, const double *mw, double *value, double *grad, double *amp)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!c->mvi) return fail(c, GH_ERR_UNSUPPORTED, "gh_amplitude_eval: %s", MVI_ONLY);
    if (!mw || !value) return fail(c, GH_ERR_ARG, "gh_amplitude_eval: null pointer");
    TRY(need(c, c->amp.set, "gh_amplitude_eval: call gh_set_amplitude first (lambda = 0 leaves the coupling off)"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_amplitude_eval"));
    const int64_t m = store_cells(c);
    if (amp) TRY(dalloc(c, &c->amp.abuf, (size_t)m));
    TRY(h2d(c, c->xb[3], mw, (size_t)c->M));
    launch_amplitude(c, c->xb[3], 1.0, grad ? c->tmpM : nullptr, false, amp ? c->amp.abuf : nullptr, c->amppart);
    sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->amppart, (int)c->work.amppart, c->st[3].scal);
    HIPCHK(c, hipGetLastError());
    TRY(read_value(c, c->st[3].scal, value));
    if (grad) TRY(d2h(c, grad, c->tmpM, (size_t)c->M));
    if (amp) TRY(d2h(c, amp, c->amp.abuf, (size_t)m));
    return GH_OK;
}

int gh_amplitude_last(const gh_ctx *c, double *phi)
{
    GH_FEED_GUARD(c);
    if (!c || !phi) return GH_ERR_ARG;
    if (!c->mvi) return GH_ERR_UNSUPPORTED;
    *phi = c->cg.phi_last;
    return GH_OK;
}

int gh_set_cells_multi(gh_ctx *c, const double *bounds6, int ncomp, const int *comps, const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_multi: null pointer");
    return set_block_cells(c, GH_CELL_PRISM_MULTI, {bounds6, nullptr, ncomp, comps, weights, nullptr, 0.0, nullptr, false});
}

// (the same context as gh_set_cells_multi makes, and that call's name in the refusals; the geometry is looked at by
// gh_build_G)
int gh_set_cells_multi_table(gh_ctx *c, const double *bounds6, int ncomp, const int *comps, const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_multi: null pointer");
    return set_block_cells(c, GH_CELL_PRISM_MULTI, {bounds6, nullptr, ncomp, comps, weights, nullptr, 0.0, nullptr, true});
}

// (gh_set_cells_multi_table's context, whose table also takes chain batches: latbatch.hip.h, the forms over row blocks)
int gh_set_cells_multi_table_chains(gh_ctx *c, const double *bounds6, int ncomp, const int *comps, const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_multi: null pointer");
    return set_block_cells(c, GH_CELL_PRISM_MULTI, {bounds6, nullptr, ncomp, comps, weights, nullptr, 0.0, nullptr, true, true});
}

int gh_set_cells_tess_multi(gh_ctx *c, const double *bounds6, int ncomp, const int *comps, const double *ratios,
                            const double *weights)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6 || !comps || !ratios || !weights) return fail(c, GH_ERR_ARG, "gh_set_cells_tess_multi: null pointer");
    return set_block_cells(c, GH_CELL_TESSEROID_MULTI, {bounds6, nullptr, ncomp, comps, weights, ratios, 0.0, nullptr, false});
}

int gh_multi_info(gh_ctx *c, int *ncomp, int *comps, double *weights, double *pred_mean, double *obs_mean)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (c->mc.n == 0)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_multi_info: not a context of row blocks (gh_set_cells_multi, "
                                           "gh_set_cells_tess_multi, gh_set_cells_mvi_data with more than the unweighted "
                                           "total field)");
    if (ncomp) *ncomp = c->mc.n;
    for (int b = 0; b < c->mc.n; ++b) {
        if (comps) comps[b] = c->mc.comp[b];
        if (weights) weights[b] = c->mc.w[b];
        if (obs_mean) obs_mean[b] = c->mc.obs_mean[b];
        if (pred_mean) pred_mean[b] = 0.0;
    }
    if (pred_mean && c->mc.bmean) {
        HIPCHK(c, hipSetDevice(c->device));
        TRY(d2h(c, pred_mean, c->mc.bmean, (size_t)c->mc.n));
    }
    return GH_OK;
}

int gh_joint_std(const gh_ctx *c, double std2[2])
{
    GH_FEED_GUARD(c);
    if (!c || !std2) return GH_ERR_ARG;
    if (!c->joint || !c->weighted) return GH_ERR_ARG;
    std2[0] = c->joint_std[0];
    std2[1] = c->joint_std[1];
    return GH_OK;
}

int gh_joint_layout(const gh_ctx *c, int *workgroups_per_block, int *epilogue_stages)
{
    GH_FEED_GUARD(c);
    if (!c || !c->joint) return GH_ERR_ARG;
    if (workgroups_per_block) *workgroups_per_block = c->grid / 2;
    if (epilogue_stages) *epilogue_stages = joint_two_stage(c) ? 2 : 1;
    return GH_OK;
}

// cg.sw = 1 / (Wm scale) per block, 0 where Wm is 0: from the weights the store has NOW (gh_weight builds it again)
static int cross_gradient_weights(gh_ctx *c, const double scale2[2])
{
    const int64_t m = store_cells(c);
    TRY(dalloc(c, &c->cg.sw, (size_t)c->M));
    std::vector<double> w((size_t)c->M);
    TRY(d2h(c, w.data(), c->wm, (size_t)c->M));
    for (int64_t j = 0; j < c->M; ++j) w[(size_t)j] = w[(size_t)j] == 0.0 ? 0.0 : (1.0 / w[(size_t)j]) / scale2[j / m];
    return h2d(c, c->cg.sw, w.data(), (size_t)c->M);
}

int gh_set_cross_gradient(gh_ctx *c, double lambda, const double scale2[2], const int shape3[3], double hx, double hy,
                          const double *hz)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!c->joint)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_set_cross_gradient: the cross-gradient term couples the two blocks of the "
                                           "joint store (a GH_CELL_PRISM_JOINT context, gh_set_cells_joint)");
    if (!scale2 || !shape3 || !hz) return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: null pointer");
    TRY(need(c, c->weighted, "gh_set_cross_gradient: call gh_weight first (the term acts on mw / Wm)"));
    const int64_t m = store_cells(c);
    if (shape3[0] < 2 || shape3[1] < 2 || shape3[2] < 2)
        return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: every extent of the mesh must be at least 2, got (%d,%d,%d)",
                    shape3[0], shape3[1], shape3[2]);
    if ((int64_t)shape3[0] * shape3[1] * shape3[2] != m)
        return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: shape nz*ny*nx must be M/2 = %lld (one property's full mesh), got "
                                   "(%d,%d,%d)", (long long)m, shape3[0], shape3[1], shape3[2]);
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: lambda must be >= 0");
    for (int h = 0; h < 2; ++h)
        if (!(scale2[h] > 0.0) || !std::isfinite(scale2[h]))
            return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: the normalisers must be > 0");
    bool ok = hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy);
    for (int k = 0; ok && k < shape3[0] - 1; ++k) ok = hz[k] > 0.0 && std::isfinite(hz[k]);
    if (!ok) return fail(c, GH_ERR_ARG, "gh_set_cross_gradient: every spacing must be > 0");
    HIPCHK(c, hipSetDevice(c->device));
    gh_ctx::CrossGrad &cg = c->cg;
    // (sized for any later shape: a mesh of m cells has fewer than m layers)
    TRY(dalloc(c, &cg.ihz, (size_t)m));
    TRY(cross_gradient_weights(c, scale2));
    std::vector<double> iz((size_t)shape3[0] - 1);
    for (size_t k = 0; k < iz.size(); ++k) iz[k] = 1.0 / hz[k];
    TRY(h2d(c, cg.ihz, iz.data(), iz.size()));
    cg.ihx = 1.0 / hx;
    cg.ihy = 1.0 / hy;
    for (int k = 0; k < 3; ++k) cg.shape[k] = shape3[k];
    cg.scale[0] = scale2[0];
    cg.scale[1] = scale2[1];
    cg.lambda = lambda;
    cg.set = true;
    cg.phi_cur = cg.phi_last = 0.0;
    c->chain_ready = false;
    return GH_OK;
}

int gh_cross_gradient_eval(gh_ctx *c, const double *mw, double *value, double *grad, double *t)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!c->joint)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_cross_gradient_eval: the cross-gradient term couples the two blocks of the "
                                           "joint store (a GH_CELL_PRISM_JOINT context, gh_set_cells_joint)");
    if (!mw || !value) return fail(c, GH_ERR_ARG, "gh_cross_gradient_eval: null pointer");
    TRY(need(c, c->cg.set, "gh_cross_gradient_eval: call gh_set_cross_gradient first (lambda = 0 leaves the coupling off)"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_cross_gradient_eval"));
    const int64_t m = store_cells(c);
    if (t) TRY(dalloc(c, &c->cg.tbuf, 3 * (size_t)m));
    TRY(h2d(c, c->xb[3], mw, (size_t)c->M));
    launch_cross_gradient(c, c->xb[3], 1.0, grad ? c->tmpM : nullptr, false, t ? c->cg.tbuf : nullptr, c->regpart);
    sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->regpart, c->work.reg_blocks, c->st[3].scal);
    HIPCHK(c, hipGetLastError());
    TRY(read_value(c, c->st[3].scal, value));
    if (grad) TRY(d2h(c, grad, c->tmpM, (size_t)c->M));
    if (t) TRY(d2h(c, t, c->cg.tbuf, 3 * (size_t)m));
    return GH_OK;
}

int gh_cross_gradient_last(const gh_ctx *c, double *phi)
{
    GH_FEED_GUARD(c);
    if (!c || !phi) return GH_ERR_ARG;
    if (!c->joint) return GH_ERR_UNSUPPORTED;
    *phi = c->cg.phi_last;
    return GH_OK;
}

int gh_sweep_layout(const gh_ctx *c, int *tw, int *ept2, int *pf, int *nt, int *n_teams, int64_t *cols_per_team,
                    int *grid, int *n_panels)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (tw) *tw = c->TW;
    if (ept2) *ept2 = c->EPT2;
    if (pf) *pf = c->PF;
    if (nt) *nt = c->NT ? 1 : 0;
    if (n_teams) *n_teams = c->n_teams_sweep;
    if (cols_per_team) *cols_per_team = c->cols_per_team;
    if (grid) *grid = c->grid;
    if (n_panels) *n_panels = c->n_panels;
    return GH_OK;
}

// An observation-space vector of N doubles between the host and the device: as it is, or -- joint store --
// its two halves to / from [gz: ld | tf: ld]
static int h2d_obsvec(gh_ctx *c, double *dst, const double *src)
{
    if (!c->joint) return h2d(c, dst, src, (size_t)c->N);
    const size_t n = (size_t)store_points(c);
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)c->ld * sizeof(double), src, n * sizeof(double), n * sizeof(double), 2,
                               hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

static int d2h_obsvec(gh_ctx *c, double *dst, const double *src)
{
    if (!c->joint) return d2h(c, dst, src, (size_t)c->N);
    const size_t n = (size_t)store_points(c);
    HIPCHK(c, hipMemcpy2DAsync(dst, n * sizeof(double), src, (size_t)c->ld * sizeof(double), n * sizeof(double), 2,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

// The result passes' scaffolding: upload n_in doubles, enqueue launch(device input, device result of N doubles)
// on the context's stream, download the result.
static int run_result(gh_ctx *c, const char *who, const double *in, size_t n_in, double *result,
                      const std::function<void(const double *, double *)> &launch, int64_t n_out = -1)
{
    if (n_out < 0) n_out = c->N;  // (a store of row blocks: its observation points, not its rows)
    HIPCHK(c, hipSetDevice(c->device));
    double *din = nullptr, *dres = nullptr;
    HIPCHK(c, hipMalloc((void **)&din, sizeof(double) * std::max<size_t>(n_in, 1)));
    if (hipMalloc((void **)&dres, sizeof(double) * (size_t)std::max<int64_t>(n_out, 1)) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(din);
        return fail(c, GH_ERR_NOMEM, "%s: device allocation of %lld doubles failed", who, (long long)n_out);
    }
    hipError_t e = hipMemcpyAsync(din, in, sizeof(double) * n_in, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch(din, dres);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(result, dres, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(din);
    hipFree(dres);
    HIPCHK(c, e);
    return GH_OK;
}

int gh_tf_result(gh_ctx *c, const double *mag3, double *result)
{
    GH_FEED_GUARD(c);
    if (!c || !mag3 || !result) return fail(c, GH_ERR_ARG, "gh_tf_result: null pointer");
    TRY(need(c, c->have_obs && c->have_cells, "gh_tf_result: call gh_set_obs and gh_set_cells_tf first"));
    // (on the table the unweighted total field alone is a store of one block: the same cells, the same points)
    const bool table_tf = lattice_mvi(c) && c->mc.n == 1 && c->mc.comp[0] == GH_BCOMP_TF;
    if (c->cell_kind != GH_CELL_PRISM_TF && c->cell_kind != GH_CELL_PRISM_MVI && !table_tf)
        return fail(c, GH_ERR_ARG, "gh_tf_result: the cells are not a total-field magnetic model (gh_set_cells_tf, "
                                   "gh_set_cells_mvi)");
    if (c->sh.kind != 0)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_tf_result: the magnetic field's result runs on an unsharded context");
    // (magnetization-vector store: M / 3 prisms)
    const int64_t cells = store_cells(c);
    return run_result(c, "gh_tf_result", mag3, 3 * (size_t)cells, result, [c, cells](const double *dmag, double *dres) {
        prism_tf_result_kernel<<<dim3((unsigned)((c->N + 255) / 256)), dim3(256), 0, c->stream>>>(
            c->obs[0], c->obs[1], c->obs[2], c->bounds, dmag, c->N, cells, c->tf_dir[0], c->tf_dir[1], c->tf_dir[2],
            dres);
    });
}

int gh_b_result(gh_ctx *c, int component, const double *mag3, double *result)
{
    GH_FEED_GUARD(c);
    if (!c || !mag3 || !result) return fail(c, GH_ERR_ARG, "gh_b_result: null pointer");
    TRY(need(c, c->have_obs && c->have_cells, "gh_b_result: call gh_set_cells_mvi_data (or gh_set_cells_mvi) and gh_set_obs "
                                              "first"));
    if (!c->mvi)
        return fail(c, GH_ERR_ARG, "gh_b_result: the cells are not a magnetization-vector model (gh_set_cells_mvi, "
                                   "gh_set_cells_mvi_data)");
    if (tess_mag_store(c))
        return fail(c, GH_ERR_UNSUPPORTED, "gh_b_result: the prisms' result pass does not run on the tesseroid "
                                           "magnetization store: gh_tess_b_result");
    if (component < GH_BCOMP_BX || component > GH_BCOMP_BZ)
        return fail(c, GH_ERR_ARG, "gh_b_result: component %d is not GH_BCOMP_BX (1), GH_BCOMP_BY (2) or GH_BCOMP_BZ (3); the "
                                   "total field's result is gh_tf_result", component);
    typedef void (*result_fn)(const double *, const double *, const double *, const double *, const double *, int64_t,
                              int64_t, double *);
    static const result_fn fns[] = {prism_b_result_kernel<BCOMP_BX>, prism_b_result_kernel<BCOMP_BY>,
                                    prism_b_result_kernel<BCOMP_BZ>};
    const result_fn fn = fns[component - GH_BCOMP_BX];
    const int64_t cells = store_cells(c), n = store_points(c);
    return run_result(c, "gh_b_result", mag3, 3 * (size_t)cells, result, [c, cells, n, fn](const double *dmag, double *dres) {
        hipLaunchKernelGGL(fn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->obs[0],
                           (const double *)c->obs[1], (const double *)c->obs[2], (const double *)c->bounds, dmag, n, cells,
                           dres);
    }, n);
}

int gh_tess_b_result(gh_ctx *c, int component, const double *mag3, double *result)
{
    GH_FEED_GUARD(c);
    if (!c || !mag3 || !result) return fail(c, GH_ERR_ARG, "gh_tess_b_result: null pointer");
    TRY(need(c, c->have_obs && c->have_cells, "gh_tess_b_result: call gh_set_cells_tess_mag and gh_set_obs first"));
    if (!tess_mag_store(c))
        return fail(c, GH_ERR_ARG, "gh_tess_b_result: the cells are not a tesseroid magnetization model "
                                   "(gh_set_cells_tess_mag)");
    if (component < GH_BCOMP_TF || component > GH_BCOMP_BZ)
        return fail(c, GH_ERR_ARG, "gh_tess_b_result: component %d is not one of GH_BCOMP_TF (0) .. GH_BCOMP_BZ (3)",
                    component);
    if (component == GH_BCOMP_TF && !c->tmag_fdir)
        return fail(c, GH_ERR_ARG, "gh_tess_b_result: the total field needs the directions gh_set_cells_tess_mag takes "
                                   "as fdir");
    const int64_t m = store_cells(c), Nb = store_points(c);
    int rc = GH_OK;
    const int rr = run_result(c, "gh_tess_b_result", mag3, 3 * (size_t)m, result, [&](const double *dmag, double *dres) {
        rc = tess_mag_pass(c, "gh_tess_b_result", [&](const TessMagObs &o, const double *frame, int *err_cell, TessStats *stats) {
            tess_mag_result_kernel<<<dim3((unsigned)Nb), dim3(256), 0, c->stream>>>(
                o, c->bounds, frame, c->tmag_fdir, dmag, Nb, m, c->ratio, component, dres, err_cell, stats);
        });
    }, Nb);
    return rc != GH_OK ? rc : rr;
}

int gh_set_cells_prism(gh_ctx *c, const double *bounds6, int component)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "gh_set_cells_prism: null pointer");
    TRY(check_component(c, "gh_set_cells_prism", COMPS_GRAV, component));
    // gz is the prism kind of gh_set_cells: the same context, the same kernels, the same bits
    if (component == GH_COMP_GZ) return gh_set_cells(c, bounds6, GH_CELL_PRISM, 1.6);
    return set_cells(c, bounds6, GH_CELL_PRISM_COMP, component, c->ratio);
}

int gh_set_cells_tess(gh_ctx *c, const double *bounds6, int component, double ratio)
{
    GH_FEED_GUARD(c);
    if (!c || !bounds6) return fail(c, GH_ERR_ARG, "gh_set_cells_tess: null pointer");
    TRY(check_component(c, "gh_set_cells_tess", COMPS_GRAV, component));
    TRY(check_tess_bounds(c, "gh_set_cells_tess", bounds6, c->M));
    // gz is the tesseroid kind of gh_set_cells: the same context, the same kernels, the same bits
    if (component == GH_COMP_GZ) return gh_set_cells(c, bounds6, GH_CELL_TESSEROID, ratio);
    if (!(ratio > 0)) return fail(c, GH_ERR_ARG, "Invalid ratio %g. Must be > 0.", ratio);
    return set_cells(c, bounds6, GH_CELL_TESSEROID_COMP, component, ratio);
}

int gh_prism_result(gh_ctx *c, const double *dens, double *result)
{
    GH_FEED_GUARD(c);
    if (!c || !dens || !result) return fail(c, GH_ERR_ARG, "gh_prism_result: null pointer");
    TRY(need(c, c->have_obs && c->have_cells, "gh_prism_result: call gh_set_obs and gh_set_cells_prism first"));
    if (c->cell_kind == GH_CELL_TESSEROID_COMP)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_prism_result: a tesseroid gravity component (GH_CELL_TESSEROID_COMP) has "
                                           "no result pass of its own: gh_forward on its kernel");
    if (c->cell_kind != GH_CELL_PRISM && c->cell_kind != GH_CELL_PRISM_COMP)
        return fail(c, GH_ERR_ARG, "gh_prism_result: the cells are not a prism density model (gh_set_cells_prism)");
    if (c->sh.kind != 0)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_prism_result: the prism result runs on an unsharded context");
    return run_result(c, "gh_prism_result", dens, (size_t)c->M, result, [c](const double *ddens, double *dres) {
        prism_comp_result_kernel<<<dim3((unsigned)((c->N + 255) / 256)), dim3(256), 0, c->stream>>>(
            c->obs[0], c->obs[1], c->obs[2], c->bounds, ddens, c->N, c->M, c->comp, dres);
    });
}

int gh_set_matrix_free(gh_ctx *c, int enable)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (enable) TRY(dense_single_chain_refuse(c, "gh_set_matrix_free"));
    if (c->have_G || c->work_ready) return fail(c, GH_ERR_ARG, "gh_set_matrix_free: call before gh_build_G");
    if (c->lat) {
        if (enable) return fail(c, GH_ERR_ARG, "gh_set_matrix_free: %s is switched on: one form at a time", LATTICE_NAME);
        c->lat->mf_before = false;  // (the store keeps c->mf)
        return GH_OK;
    }
    if (c->ls) {
        c->mf_before_ls = enable != 0;  // (takes effect when the shift-invariant store is switched off)
        return GH_OK;
    }
    c->mf = enable != 0;  // (the passes are partitioned in gh_build_G, once the cell kind is known)
    return GH_OK;
}

int gh_set_shift_invariant(gh_ctx *c, int enable)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    // (the tesseroid multi-component store and the tesseroid magnetization store are the stores of row blocks that
    // have the table; the prism forms of the vector stores keep refusing)
    // (a magnetization store that has been built is the dense store: it refuses as it always did)
    if (enable && !(c && (tess_multi_store(c) || (tess_mag_store(c) && !c->have_G && !c->work_ready))))
        TRY(dense_single_chain_refuse(c, "gh_set_shift_invariant"));
    if (c->have_G || c->work_ready) return fail(c, GH_ERR_ARG, "gh_set_shift_invariant: call before gh_build_G");
    if (enable && c->lat) return fail(c, GH_ERR_ARG, "gh_set_shift_invariant: %s is switched on: one form at a time", LATTICE_NAME);
    // (the store is a flavour of the matrix-free mode -- G is never stored -- so enabling it sets c->mf;
    // disabling it puts c->mf back to what gh_set_matrix_free last asked for)
    if (c->ls) c->mf = c->mf_before_ls;
    delete c->ls;
    c->ls = nullptr;
    if (enable) {
        c->ls = new LonSymHost();
        c->mf_before_ls = c->mf;
        c->mf = true;
    }
    return GH_OK;
}

int gh_set_translation_invariant(gh_ctx *c, int enable)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (enable != 0 && enable != 1 && enable != GH_TABLE_CHAINS && enable != GH_TABLE_REPLICATES)
        return fail(c, GH_ERR_ARG, "gh_set_translation_invariant: enable must be 0, 1, 2 or 4 (2: the table that takes chain "
                                   "batches; 4: the table that takes the bootstrap batch)");
    if (enable) TRY(dense_single_chain_refuse(c, "gh_set_translation_invariant"));
    if (c->have_G || c->work_ready) return fail(c, GH_ERR_ARG, "gh_set_translation_invariant: call before gh_build_G");
    if (lattice_own(c))
        return fail(c, GH_ERR_UNSUPPORTED, "gh_set_translation_invariant: %s was set onto %s with its cells "
                                           "(%s): the table is this context's form", store_name(c), LATTICE_NAME,
                    lattice_form(c).entry);
    if (enable && c->ls)
        return fail(c, GH_ERR_ARG, "gh_set_translation_invariant: the shift-invariant store is switched on: one form at a time");
    if (enable && !c->lat && c->mf)
        return fail(c, GH_ERR_ARG, "gh_set_translation_invariant: the matrix-free mode is switched on: one form at a time");
    if (enable && c->have_cells && c->cell_kind != GH_CELL_PRISM && c->cell_kind != GH_CELL_PRISM_COMP &&
        c->cell_kind != GH_CELL_PRISM_TF)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_set_translation_invariant: %s holds prisms (tesseroid grids: gh_set_shift_invariant)",
                    LATTICE_NAME);
    if (enable && c->sh.kind != 0)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_set_translation_invariant: not supported on a sharded context (one GPU holds the table)");
    // (like the longitude table a flavour of the matrix-free mode: enabling it sets c->mf, disabling it puts c->mf back)
    if (c->lat) c->mf = c->lat->mf_before;
    delete c->lat;
    c->lat = nullptr;
    if (enable) lattice_switch_on(c, LAT_SCALAR, enable);
    return GH_OK;
}

int gh_translation_invariant_info(const gh_ctx *c, int *on, int *nx, int *ny, int *nz, int *px, int *qy, int64_t *table_bytes,
                                  double *max_dev, double *build_ms)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const bool o = lattice_on(c);
    const ghk::LatGeom g = o ? c->lat->g : ghk::LatGeom{};
    if (on) *on = o ? 1 : 0;
    if (nx) *nx = g.nx;
    if (ny) *ny = g.ny;
    if (nz) *nz = o ? g.nz / lattice_form(c).groups : 0;  // (the geometry's layers: gh_translation_invariant_axes has the factor)
    if (px) *px = g.px;
    if (qy) *qy = g.qy;
    if (table_bytes) *table_bytes = (int64_t)(o ? c->lat->nb : 1) * g.nz * g.U * g.V * (int64_t)sizeof(double);
    if (max_dev) *max_dev = o ? c->lat->max_dev : 0.0;
    if (build_ms) *build_ms = o ? c->lat->build_ms : 0.0;
    return GH_OK;
}

int gh_translation_invariant_axes(const gh_ctx *c, int *axes, int *chunks, int *layers_per_chunk)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const bool o = lattice_on(c);
    if (axes) *axes = o ? lattice_form(c).groups : 0;
    if (chunks) *chunks = o ? c->lat->chunks : 0;
    if (layers_per_chunk) *layers_per_chunk = o ? c->lat->fwd.lpc : 0;
    return GH_OK;
}

int gh_translation_invariant_batch_plan(gh_ctx *c, int32_t out[24])
{
    GH_FEED_GUARD(c);
    if (!c || !out) return fail(c, GH_ERR_ARG, "gh_translation_invariant_batch_plan: null pointer");
    for (int i = 0; i < 24; ++i) out[i] = 0;
    if (!lattice_on(c) || !(lattice_chains(c) || lattice_reps(c))) return GH_OK;
    LatticeHost &h = *c->lat;
    const bool fits = latb_plan_make(c);  // (arithmetic alone: the context's last error text stays)
    const ghk::LatbPlan *pl[2] = {&h.badj, &h.bfwd};
    out[0] = 1;
    out[1] = fits ? 1 : 0;
    out[2] = ghk::LATB_TR;
    out[3] = ghk::LATB_RW;
    out[4] = ghk::LATB_NT;
    out[5] = ghk::LATB_MAX_CHUNKS;
    out[6] = c->cus;
    for (int q = 0; q < 2; ++q) {
        out[7 + 6 * q] = pl[q]->ntiles;
        out[8 + 6 * q] = pl[q]->FT;
        out[9 + 6 * q] = pl[q]->WT;
        out[10 + 6 * q] = pl[q]->WL;
        out[11 + 6 * q] = q ? h.bgx_fwd : h.bgx_adj;
        out[12 + 6 * q] = (int32_t)std::min<size_t>(q ? h.blds_fwd : h.blds_adj, (size_t)INT32_MAX);
    }
    out[19] = h.bfwd.lpc;
    out[20] = h.bchunks;
    out[21] = h.bgx_adj * h.g.nz;
    out[22] = lattice_multi(c) ? h.nb : 0;  // (the table of blocks: the forward's grid is nb workgroups deep)
    return GH_OK;
}

int gh_translation_invariant_table(gh_ctx *c, double *out)
{
    GH_FEED_GUARD(c);
    if (!c || !out) return fail(c, GH_ERR_ARG, "gh_translation_invariant_table: null pointer");
    TRY(need(c, lattice_on(c), "gh_translation_invariant_table: no table resident (gh_set_translation_invariant, gh_build_G)"));
    HIPCHK(c, hipSetDevice(c->device));
    const ghk::LatGeom &g = c->lat->g;
    return d2h(c, out, c->lat->T, (size_t)c->lat->nb * (size_t)g.nz * (size_t)g.U * (size_t)g.V);  // (block-major)
}

int gh_lattice_detect(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6, int *dims5,
                      int *lat_of_cell, int *cell_of_lat, int *lat_of_obs, int *obs_of_lat)
{
    if (N < 0 || M < 0 || !x || !y || !z || !bounds6 || !dims5 || !lat_of_cell || !cell_of_lat || !lat_of_obs || !obs_of_lat)
        return GH_ERR_ARG;
    std::vector<int> loc, col, loo, ool;
    int dims[5] = {0, 0, 0, 0, 0};
    const int rc = lattice_detect_host(N, x, y, z, M, bounds6, dims, loc, col, loo, ool);
    if (rc == GH_LATTICE_ON) {
        std::copy(dims, dims + 5, dims5);
        std::copy(loc.begin(), loc.end(), lat_of_cell);
        std::copy(col.begin(), col.end(), cell_of_lat);
        std::copy(loo.begin(), loo.end(), lat_of_obs);
        std::copy(ool.begin(), ool.end(), obs_of_lat);
    }
    return rc;
}

int gh_shift_invariant_resident_stats(gh_ctx *c, int *workgroups, int64_t *launches, int64_t *evaluations, int64_t *trajectories,
                                      int *timeouts)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const bool on = lonsym_harmonic(c) && c->ls->res.state > 0;
    if (workgroups) *workgroups = on ? c->ls->hgrid : 0;
    if (launches) *launches = c->ls ? c->ls->res.launches : 0;
    if (evaluations) *evaluations = c->ls ? c->ls->res.evals : 0;
    if (trajectories) *trajectories = c->ls ? c->ls->res.trajectories : 0;
    if (timeouts) *timeouts = c->ls ? c->ls->res.xg.aborts : 0;
    return GH_OK;
}

int gh_shift_invariant_info(const gh_ctx *c, int *n_lon, int *n_classes, int *n_rows, int64_t *table_bytes)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const bool on = lonsym_on(c);
    if (n_lon) *n_lon = on ? c->ls->n : 0;
    if (n_classes) *n_classes = on ? c->ls->na : 0;
    if (n_rows) *n_rows = on ? c->ls->nc : 0;
    if (table_bytes) *table_bytes = on ? lonsym_table_bytes(c) : 0;
    return GH_OK;
}

int gh_shift_invariant_harmonic(const gh_ctx *c, int *on, int *n_freq, int64_t *table_bytes, int *workgroups)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    // on: 1 = the register form (lonsymh.hip.h), 2 = the streamed form for large grids (lonsymw.hip.h)
    const bool h = lonsym_one_row(c);
    if (on) *on = !h ? 0 : c->ls->harm ? 1 : 2;
    if (n_freq) *n_freq = h ? c->ls->nf : 0;
    if (table_bytes) *table_bytes = h ? (c->ls->harm ? (int64_t)c->ls->nc * c->ls->na * c->ls->nf : (int64_t)c->ls->witems * c->ls->na * c->ls->nfp) * 16 : 0;
    if (workgroups) *workgroups = h ? lonsym_grid(c) : 0;
    return GH_OK;
}

int gh_shift_invariant_plan(gh_ctx *c, int32_t out[32])
{
    GH_FEED_GUARD(c);
    if (!c || !out) return fail(c, GH_ERR_ARG, "gh_shift_invariant_plan: null pointer");
    for (int i = 0; i < 32; ++i) out[i] = 0;
    if (!lonsym_on(c)) return GH_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const LonSymHost &h = *c->ls;
    out[0] = h.harm ? 1 : h.wide ? 2 : 0;
    out[1] = h.n;
    out[2] = h.na;
    out[3] = h.nc;
    out[4] = h.nf;
    // the direct correlations (lonsym.hip.h)
    out[5] = h.W;
    out[6] = h.KB;
    out[7] = h.AG;
    out[8] = h.thr;
    out[9] = h.items;
    out[10] = h.grid;
    out[11] = (int32_t)h.lds;
    out[12] = h.direct_ok ? 1 : 0;
    out[13] = h.direct_code;
    // the register form (lonsymh.hip.h)
    out[14] = h.rp;
    out[15] = h.rw;
    out[16] = h.harm ? h.hgrid : 0;
    out[17] = (int32_t)h.hlds;
    // the streamed form (lonsymw.hip.h)
    if (h.wide) {
        out[18] = h.nfp;
        out[19] = h.nf <= LW_THREADS ? 1 : h.nf <= 2 * LW_THREADS ? 2 : 3;
        out[20] = h.wmirror ? 1 : 0;
        out[21] = h.witems;
        out[22] = h.wgrid;
        out[23] = h.wrows;
        out[24] = h.wparts;
    }
    out[25] = h.n_xslots;
    out[26] = h.max_extra;
    // the persistent launch (lonres.hip.h): planned now where it was not yet, as the first gh_chain_run would
    const bool planned = lonres_plan(c);
    out[27] = planned ? 1 : 0;
    out[28] = planned && lonres_usable(c) ? 1 : 0;
    out[29] = planned ? h.hgrid : 0;
    out[30] = planned ? (int32_t)h.res.lds : 0;
    out[31] = 1;
    return GH_OK;
}

int gh_set_matrix_free_exact(gh_ctx *c, int exact)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (c->have_G || c->work_ready) return fail(c, GH_ERR_ARG, "gh_set_matrix_free_exact: call before gh_build_G");
    c->mf_exact_req = exact != 0 ? 1 : 0;
    return GH_OK;
}

// The stored kernel, or the weights folded into it, changed (gh_build_G, gh_upload_G, gh_weight): a new generation.
// What was derived from the old one goes, or is keyed to the generation and made again where it is next used --
// the folded store (fd.gen), the MFMA operand-order copy (bt.Gb_gen), the wavelet rows with their dense form (a
// context is compressed again for its new kernel), the chains' states.  The streaming posterior's 1 / wm follows
// the weights the context has now.
static int kernel_changed(gh_ctx *c)
{
    c->G_gen += 1;
    c->chain_ready = false;
    c->bt.ready = false;
    gh_ctx::Wavelet &w = c->wv;
    if (w.on || w.indptr) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        w.on = false;
        w.F_valid = false;
        w.nnz = 0;
        dev_release(c, w.indptr);
        dev_release(c, w.indices);
        dev_release(c, w.data);
        if (!shard_rows(c)) c->rs.state = 0;  // (planned for the dense form: plan the resident chain kernel again)
        if (c->ls) c->ls->res.state = 0;
    }
    if (c->ps.on) TRY(post_weights(c));
    return GH_OK;
}

int gh_build_G(gh_ctx *c)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->have_obs && c->have_cells, "gh_build_G: call gh_set_obs and gh_set_cells first"));
    HIPCHK(c, hipSetDevice(c->device));
    c->warn_cells = 0;
    c->leaves = 0;
    if (c->mf) {
        if (c->work_ready) return fail(c, GH_ERR_ARG, "gh_build_G: a matrix-free context is built once");
        // (a store of blocks: the tesseroid forms and the prisms' multi-component store get here, by way of their tables)
        if (c->lat) {
            // (... and the joint store, by way of gh_set_cells_joint_table)
            const bool own_table = lattice_own(c);
            if (!own_table) TRY(dense_single_chain_refuse(c, "gh_build_G on the translation-invariant store"));
            if (c->cell_kind != GH_CELL_PRISM && c->cell_kind != GH_CELL_PRISM_COMP && c->cell_kind != GH_CELL_PRISM_TF &&
                !own_table)
                return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s holds prisms (tesseroid grids: gh_set_shift_invariant)",
                            LATTICE_NAME);
            if (c->sh.kind != 0)
                return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s is not supported on a sharded context (one GPU holds the table)",
                            LATTICE_NAME);
        }
        if (store_name(c) && !c->ls && !lattice_own(c))
            return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %s has no matrix-free mode (dense, or the shift-invariant store)",
                        store_name(c));
        c->mf_fused = c->ld <= 16384 && env_int("GRAVHMC_MF_FUSED", 1) != 0;
        if (c->lat) c->mf_fused = false;  // (the table's own two passes, whatever N)
        // (tesseroid components: the two-pass form, with the entry evaluated inside each pass -- no fused KIND;
        // the near-field table and the cell-constant fast leaf are gz's)
        if (c->cell_kind == GH_CELL_TESSEROID_COMP) c->mf_fused = false;
        if (c->cell_kind == GH_CELL_TESSEROID || c->cell_kind == GH_CELL_TESSEROID_COMP) {
            const int64_t N = c->N;
            TRY(dalloc(c, &c->tconv, (size_t)(6 * N)));
            tess_convert_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream>>>(
                c->obs[0], c->obs[1], c->obs[2], N, c->tconv, c->tconv + N, c->tconv + 2 * N,
                c->tconv + 3 * N, c->tconv + 4 * N, c->tconv + 5 * N);
            HIPCHK(c, hipGetLastError());
        }
        if (c->cell_kind == GH_CELL_TESSEROID) {
            c->mf_exact = c->mf_exact_req >= 0 ? c->mf_exact_req != 0 : env_int("GRAVHMC_MF_EXACT", 0) != 0;
            {
                // what depends on the cell alone, once per cell instead of once per (obs, cell) pair
                TRY(dalloc(c, &c->mf_cellc, (size_t)c->M * TESS_NC, false));
                tess_cellconst_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(
                    c->bounds, c->M, c->ratio, c->mf_cellc);
                HIPCHK(c, hipGetLastError());
                TRY(build_near_table(c));
            }
        }
        if (c->ls) TRY(lonsym_build(c));
        if (c->lat) TRY(lattice_build(c));
        // (tesseroid components: the error codes, leaves and overflow of the subdivision, as the dense build
        // reports them, from one pass that stores nothing)
        if (c->cell_kind == GH_CELL_TESSEROID_COMP) TRY(tess_comp_assemble(c, c->tconv, nullptr, c->comp, c->ratio, c->N, c->ld));
        TRY(configure_mf(c));
        TRY(dalloc(c, &c->mf_stats, 1));
        c->have_G = true;
        c->weighted = false;
        c->chain_ready = false;
        c->bt.ready = false;
        return GH_OK;
    }
    if (tess_multi_store(c) && c->N > 16384)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %d components x %lld observations = %lld rows: the dense form of "
                                           "the tesseroid multi-component store takes at most 16384 (it runs on the fused "
                                           "sweep: no row panels, no team sweep); the shift-invariant store has no such "
                                           "limit (gh_set_shift_invariant)", c->mc.n, (long long)store_points(c),
                    (long long)c->N);
    if (tess_mag_store(c) && c->N > 16384)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_build_G: %d components x %lld observations = %lld rows: the dense form of "
                                           "the tesseroid magnetization store takes at most 16384; the shift-invariant "
                                           "table has no such limit (gh_set_cells_tess_mag_table)", c->mc.n,
                    (long long)store_points(c), (long long)c->N);
    if (!c->dense_ok)
        return fail(c, GH_ERR_UNSUPPORTED,
                    "N = %lld: more than 16384 observations per device: shard the observations or use "
                    "the matrix-free mode (gh_set_matrix_free)", (long long)c->N);
    TRY(build_dense(c));
    c->have_G = true;
    c->weighted = false;
    TRY(kernel_changed(c));
    return fold_detect(c);  // (gz prisms on a grid symmetric under both mirrors: host_fold.h)
}

int gh_kernel_stats(const gh_ctx *c, int64_t *warn_cells, int64_t *leaves)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (warn_cells) *warn_cells = c->warn_cells;
    if (leaves) *leaves = c->leaves;
    return GH_OK;
}

int gh_upload_G(gh_ctx *c, const double *A, int64_t ld, int fortran_order)
{
    GH_FEED_GUARD(c);
    if (!c || !A) return fail(c, GH_ERR_ARG, "gh_upload_G: null pointer");
    TRY(dense_single_chain_refuse(c, "gh_upload_G"));
    TRY(lattice_refuse(c, "gh_upload_G", "its entries come from the cells and observations"));
    if (ld < (fortran_order ? c->N : c->M)) return fail(c, GH_ERR_ARG, "gh_upload_G: ld too small");
    if (c->mf) return fail(c, GH_ERR_ARG, "gh_upload_G: context is matrix-free");
    if (!c->dense_ok) return fail(c, GH_ERR_UNSUPPORTED, "N = %lld: more than 16384 observations per device", (long long)c->N);
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dalloc(c, &c->G, (size_t)c->ld * (size_t)c->M, false));
    HIPCHK(c, hipMemsetAsync(c->G, 0, sizeof(double) * (size_t)c->ld * (size_t)c->M, c->stream));
    if (fortran_order) {
        HIPCHK(c, hipMemcpy2DAsync(c->G, (size_t)c->ld * sizeof(double), A, (size_t)ld * sizeof(double),
                                   (size_t)c->N * sizeof(double), (size_t)c->M, hipMemcpyHostToDevice,
                                   c->stream));
    } else {
        // row-major N x M: transpose on the host in column panels (setup path, runs once)
        const int64_t panel = std::max<int64_t>(1, (int64_t)(64 << 20) / (int64_t)(c->N * sizeof(double)));
        std::vector<double> buf((size_t)std::min(panel, c->M) * (size_t)c->N);
        for (int64_t j0 = 0; j0 < c->M; j0 += panel) {
            const int64_t nb = std::min(panel, c->M - j0);
            for (int64_t i = 0; i < c->N; ++i)
                for (int64_t j = 0; j < nb; ++j) buf[(size_t)j * c->N + i] = A[i * ld + j0 + j];
            HIPCHK(c, hipMemcpy2DAsync(c->G + j0 * c->ld, (size_t)c->ld * sizeof(double), buf.data(),
                                       (size_t)c->N * sizeof(double), (size_t)c->N * sizeof(double),
                                       (size_t)nb, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_G = true;
    c->weighted = false;
    c->fd.detected = -1;  // (entries of the caller's: no pairing is assumed)
    c->fd.reason = GH_FOLD_NOT_GZ;
    return kernel_changed(c);
}

int gh_download_G(gh_ctx *c, double *A, int64_t ld)
{
    GH_FEED_GUARD(c);
    if (!c || !A) return fail(c, GH_ERR_ARG, "gh_download_G: null pointer");
    TRY(need(c, c->have_G && !c->mf, "gh_download_G: no kernel matrix resident"));
    // (joint store: H = [Aw_gz | Aw_tf], N/2 rows -- the zero blocks of the stacked A are not stored)
    const int64_t rows = c->joint ? c->N / 2 : c->N;
    if (ld < rows) return fail(c, GH_ERR_ARG, "gh_download_G: ld too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(A, (size_t)ld * sizeof(double), c->G, (size_t)c->ld * sizeof(double),
                               (size_t)rows * sizeof(double), (size_t)c->M, hipMemcpyDeviceToHost,
                               c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_weight(gh_ctx *c, double weightfactor, double *wm_out)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->have_G, "gh_weight: no kernel matrix resident"));
    TRY(need(c, !c->weighted, "gh_weight: kernel is already weighted"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dalloc(c, &c->wm, (size_t)c->M));
    TRY(dalloc(c, &c->wm2, (size_t)c->M));
    if (c->joint) {
        if (weightfactor != 0.5)
            return fail(c, GH_ERR_ARG, "gh_weight: the joint kernel is weighted by the column 2-norms (weightfactor 0.5)");
        // population std of each unweighted block, two passes (weightKDM, potential.py:1050-1051)
        const int64_t m = store_cells(c), n = store_points(c);
        // (on the table: over the entries of one property's table, each weighted by the pairs that have its offset)
        const bool table = lattice_on(c);
        const int64_t entries = table ? (int64_t)(c->lat->g.nz / 2) * c->lat->g.U * c->lat->g.V : c->ld * m;
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((entries + 255) / 256, (int64_t)c->cus * 8));
        double *part = nullptr, *mean = nullptr;
        TRY(dalloc(c, &part, 2 * (size_t)gx));
        TRY(dalloc(c, &mean, 2));
        std::vector<double> hp(2 * (size_t)gx);
        double mu[2], var[2];
        for (int pass = 0; pass < 2; ++pass) {
            if (table)
                ghk::lat_joint_std_kernel<<<dim3(gx, 2), dim3(256), 0, c->stream>>>(c->lat->g, pass, mean, part);
            else
                joint_std_kernel<<<dim3(gx, 2), dim3(256), 0, c->stream>>>(c->G, n, m, c->ld, pass, mean, part);
            HIPCHK(c, hipGetLastError());
            TRY(d2h(c, hp.data(), part, hp.size()));
            for (int h = 0; h < 2; ++h) {
                long double t = 0.0L;
                for (unsigned b = 0; b < gx; ++b) t += hp[(size_t)h * gx + b];
                (pass ? var : mu)[h] = (double)(t / (long double)((double)n * (double)m));
            }
            if (pass == 0) TRY(h2d(c, mean, mu, 2));
        }
        c->joint_std[0] = std::sqrt(var[0]);
        c->joint_std[1] = std::sqrt(var[1]);
    }
    if (c->mc.n > 0) {
        // Wb first: the column norms are those of Wb A, or the component with the largest unit would decide them
        RowBlocks rb{};
        rb.n = c->mc.n;
        rb.Nb = store_points(c);
        bool unit = true;
        for (int b = 0; b < rb.n; ++b) {
            rb.w[b] = c->mc.w[b];
            unit = unit && rb.w[b] == 1.0;
        }
        // (the shift-invariant table took the weights when it was built, the translation-invariant table's passes take
        // them from here on: there is no G)
        if (!unit && !c->mf) {
            const unsigned blocks = (unsigned)std::min<int64_t>((c->ld * c->M + 255) / 256, 1 << 20);
            scale_rowblocks_kernel<<<dim3(blocks), dim3(256), 0, c->stream>>>(c->G, c->ld, c->M, rb);
            HIPCHK(c, hipGetLastError());
        }
    }
    if (lonsym_on(c)) {
        lonsym_colnorm_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(
            lonsym_geom(c), c->ls->a_of, c->ls->m_of, weightfactor, c->wm);
    } else if (lattice_on(c)) {
        lat_colnorm_blocks_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(c->lat->g, lattice_tables(c),
                                                                                                   weightfactor, c->wm);
    } else if (c->mf) {
        hipLaunchKernelGGL(mf_pick(c, mf_colnorm_kernel<MF_E_GEN>, mf_colnorm_kernel<MF_E_TF>, mf_colnorm_kernel<MF_E_COMP>,
                                   mf_colnorm_kernel<MF_E_TESS>),
                           dim3((unsigned)((c->M + 3) / 4)), dim3(256), 0, c->stream, mf_geom(c), weightfactor, c->wm);
    } else if (shard_rows(c)) {
        // row blocks: a column's norm spans the ranks -- local sums of squares, all-reduce, then the power and
        // the scaling of the local rows
        const unsigned blocks = (unsigned)std::min<int64_t>(c->M, (int64_t)c->cus * 16);
        colnorm_kernel<<<dim3(blocks), dim3(256), 0, c->stream>>>(c->G, c->ld, c->M, 1.0, c->wm);
        HIPCHK(c, hipGetLastError());
        TRY(comm_allreduce(c, c->wm, c->M));
        std::vector<double> ss((size_t)c->M);
        TRY(d2h(c, ss.data(), c->wm, (size_t)c->M));
        for (auto &v : ss) v = (weightfactor == 0.5) ? std::sqrt(v) : std::pow(v, weightfactor);
        TRY(h2d(c, c->wm, ss.data(), (size_t)c->M));
        colscale_kernel<<<dim3(blocks), dim3(256), 0, c->stream>>>(c->G, c->ld, c->M, c->wm);
    } else if (c->n_panels > 1) {
        const unsigned blocks = (unsigned)std::min<int64_t>(c->M, (int64_t)c->cus * 16);
        colnorm_kernel<<<dim3(blocks), dim3(256), 0, c->stream>>>(c->G, c->ld, c->M, weightfactor, c->wm);
        colscale_kernel<<<dim3(blocks), dim3(256), 0, c->stream>>>(c->G, c->ld, c->M, c->wm);
    } else {
        weight_fn f = weight_for(c);
        const int threads = (c->TW == 1 ? 4 : c->TW) * 64;
        hipLaunchKernelGGL(f, dim3(c->grid), dim3(threads), 0, c->stream, c->G, c->ld, c->M,
                           c->cols_per_team, c->n_teams_sweep, weightfactor, c->wm);
    }
    HIPCHK(c, hipGetLastError());
    if (c->joint && !c->mf) {
        // Wb: the tf block times s = std_gz / std_tf, folded into the stored kernel (Aw = Wb A Wm^-1); on the table the
        // passes take s from here on (lattice_r_blocks)
        const int64_t m = store_cells(c);
        const double sb = c->joint_std[0] / c->joint_std[1];
        scale_cols_kernel<<<dim3((unsigned)std::min<int64_t>((c->ld * m + 255) / 256, 1 << 20)), dim3(256), 0, c->stream>>>(
            c->G, c->ld, m, m, sb);
        HIPCHK(c, hipGetLastError());
    }
    std::vector<double> w((size_t)c->M);
    TRY(d2h(c, w.data(), c->wm, (size_t)c->M));
    if (wm_out) memcpy(wm_out, w.data(), sizeof(double) * (size_t)c->M);
    for (auto &v : w) v = v * v;  // diag(WmSquare) = ADiag * ADiag (potential.py:253)
    TRY(h2d(c, c->wm2, w.data(), (size_t)c->M));
    // (a coupling term set on the store's earlier weights follows the new ones)
    if (c->mvi && c->amp.set) TRY(amplitude_weights(c, c->amp.scale));
    if (c->joint && c->cg.set) TRY(cross_gradient_weights(c, c->cg.scale));
    c->weighted = true;
    return kernel_changed(c);
}

int gh_set_data(gh_ctx *c, const double *dobs, const double *grav_fix)
{
    GH_FEED_GUARD(c);
    if (!c || !dobs) return fail(c, GH_ERR_ARG, "gh_set_data: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->joint) {
        // dobsw as it is: [gz: ld | tf: ld], no mean removal, no fixed cells (potential.py:1665-1680)
        if (grav_fix) return fail(c, GH_ERR_ARG, "gh_set_data: the joint kernel takes no grav_fix");
        TRY(dalloc(c, &c->dobs_c, 2 * (size_t)c->ld));
        TRY(h2d_obsvec(c, c->dobs_c, dobs));
        c->have_fix = false;
        c->gfix_sum = 0.0;
        c->have_data = true;
        c->chain_ready = false;
        c->bt.ready = false;
        return GH_OK;
    }
    const size_t N = (size_t)c->N;
    TRY(dalloc(c, &c->dobs_c, (size_t)c->ld));
    TRY(dalloc(c, &c->gfix, (size_t)c->ld));
    // dobs - mean(dobs) (potential.py:706); numpy's mean is a pairwise sum
    std::vector<double> t(dobs, dobs + N);
    // pairwise summation with numpy's blocking (8-way unrolled blocks of 128)
    struct PW {
        static double sum(const double *a, size_t n)
        {
            if (n < 8) {
                double r = 0.0;
                for (size_t i = 0; i < n; ++i) r += a[i];
                return r;
            }
            if (n <= 128) {
                double r[8];
                for (int k = 0; k < 8; ++k) r[k] = a[k];
                size_t i = 8;
                for (; i + 8 <= n; i += 8)
                    for (int k = 0; k < 8; ++k) r[k] += a[i + k];
                double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < n; ++i) res += a[i];
                return res;
            }
            size_t n2 = n / 2;
            n2 -= n2 % 8;
            return sum(a, n2) + sum(a + n2, n - n2);
        }
    };
    if (c->mc.n > 0) {
        // Wb dobs in row blocks: every component loses its own mean
        if (grav_fix && lattice_mvi(c))
            return fail(c, GH_ERR_UNSUPPORTED, "gh_set_data with a grav_fix: not supported on %s (every data block loses its own mean)",
                        lattice_form(c).name);
        if (grav_fix)
            return fail(c, GH_ERR_ARG, "gh_set_data: %s takes no grav_fix", store_of(c).rows_name);
        const size_t Nb = (size_t)store_points(c);
        for (int b = 0; b < c->mc.n; ++b) {
            double *tb = t.data() + (size_t)b * Nb;
            const double mb = PW::sum(tb, Nb) / (double)Nb;
            for (size_t i = 0; i < Nb; ++i) tb[i] -= mb;
            c->mc.obs_mean[b] = mb;
        }
        TRY(h2d(c, c->dobs_c, t.data(), N));
        c->have_fix = false;
        c->gfix_sum = 0.0;
        c->have_data = true;
        c->chain_ready = false;
        c->bt.ready = false;
        return GH_OK;
    }
    double mean = PW::sum(t.data(), N) / (double)N;
    if (shard_rows(c)) {
        // (row blocks: the mean of ALL observations -- the sum of the ranks' pairwise sums)
        double v2[1] = {PW::sum(t.data(), N)};
        TRY(comm_allreduce_host(c, v2, 1));
        mean = v2[0] / (double)c->sh.N_global;
    }
    for (auto &v : t) v -= mean;
    TRY(h2d(c, c->dobs_c, t.data(), N));
    c->have_fix = grav_fix != nullptr;
    c->gfix_sum = grav_fix ? PW::sum(grav_fix, N) : 0.0;
    if (grav_fix) TRY(h2d(c, c->gfix, grav_fix, N));
    c->have_data = true;
    c->chain_ready = false;
    c->bt.ready = false;
    return GH_OK;
}

int gh_set_reg(gh_ctx *c, int kind, double alpha, double beta, const int shape3[3], const double *mwapr)
{
    GH_FEED_GUARD(c);
    if (!c || !mwapr) return fail(c, GH_ERR_ARG, "gh_set_reg: null pointer");
    if (kind < 0 || kind > 3)
        return fail(c, GH_ERR_ARG, "Please choose regularization from 'MS','Damping', 'Smoothness', 'TV'.");
    const bool stencil = (kind == GH_REG_SMOOTHNESS || kind == GH_REG_TV);
    if (shard_cols(c) && stencil) {
        // the finite-difference stencil crosses the shard boundaries: shards of whole z-planes
        if (!shape3 || (int64_t)shape3[0] * shape3[1] * shape3[2] != c->sh.M_global)
            return fail(c, GH_ERR_ARG, "gh_set_reg: Smoothness/TV on a sharded model need the GLOBAL shape nz*ny*nx == M_global");
        const int64_t P = (int64_t)shape3[1] * shape3[2];
        if (c->M < P || c->M % P != 0 || c->sh.m0 % P != 0)
            return fail(c, GH_ERR_UNSUPPORTED, "Smoothness/TV on a sharded model need shards of whole z-planes "
                                               "(%lld cells each): partition the cells with that alignment", (long long)P);
    } else if (stencil && c->joint) {
        if (!shape3 || 2 * (int64_t)shape3[0] * shape3[1] * shape3[2] != c->M)
            return fail(c, GH_ERR_ARG, "gh_set_reg: Smoothness/TV on the joint kernel need shape nz*ny*nx == M/2 (one property's mesh)");
    } else if (stencil && c->mvi) {
        if (!shape3 || 3 * (int64_t)shape3[0] * shape3[1] * shape3[2] != c->M)
            return fail(c, GH_ERR_ARG, "gh_set_reg: Smoothness/TV on the magnetization-vector store need shape nz*ny*nx == M/3 "
                                       "(one component's mesh)");
    } else if (stencil) {
        if (!shape3 || (int64_t)shape3[0] * shape3[1] * shape3[2] != c->M)
            return fail(c, GH_ERR_ARG, "gh_set_reg: Smoothness/TV need shape nz*ny*nx == M (carved meshes are not supported by the finite-difference operator)");
    }
    if (kind == GH_REG_MS) TRY(need(c, c->weighted, "gh_set_reg: MS needs gh_weight first (uses Wm^2)"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dalloc(c, &c->mwapr, (size_t)c->M));
    TRY(dalloc(c, &c->wm2, (size_t)c->M));
    TRY(h2d(c, c->mwapr, mwapr, (size_t)c->M));
    c->reg_kind = kind;
    c->alpha = alpha;
    c->beta = beta;
    if (shape3) {
        c->shape[0] = shape3[0];
        c->shape[1] = shape3[1];
        c->shape[2] = shape3[2];
    }
    c->sh.halo = false;
    if (shard_cols(c) && stencil) {
        gh_ctx::Shard &sh = c->sh;
        const int64_t P = (int64_t)shape3[1] * shape3[2];
        const size_t need = (size_t)c->ld + 8 + 2 * (size_t)sh.world * (size_t)P;
        if (need > sh.buf_n) {
            sh.buf = nullptr;  // (the old block stays in the allocation list until gh_destroy)
            TRY(dalloc(c, &sh.buf, need));
            if (sh.hbuf) hipHostFree(sh.hbuf);
            sh.hbuf = nullptr;
            HIPCHK(c, hipHostMalloc((void **)&sh.hbuf, sizeof(double) * need));
            sh.buf_n = need;
        }
        if (sh.P != P) {
            sh.alo = sh.ahi = nullptr;
            TRY(dalloc(c, &sh.alo, (size_t)P));
            TRY(dalloc(c, &sh.ahi, (size_t)P));
        }
        TRY(dalloc(c, &sh.rb, 2));
        sh.P = P;
        // boundary planes of the prior model, once (collective: every rank is in this call)
        double *hb = sh.buf + c->ld + 8;
        const int64_t nh = 2 * (int64_t)sh.world * P;
        halo_pack_kernel<<<dim3((unsigned)std::min<int64_t>(1024, (nh + 255) / 256)), dim3(256), 0, c->stream>>>(
            c->mwapr, c->M, P, sh.rank, sh.world, hb);
        TRY(comm_allreduce(c, sh.buf, (int64_t)c->ld + 8 + nh));
        if (sh.rank > 0)
            HIPCHK(c, hipMemcpyAsync(sh.alo, hb + ((int64_t)(sh.rank - 1) * 2 + 1) * P, sizeof(double) * (size_t)P,
                                     hipMemcpyDeviceToDevice, c->stream));
        if (sh.rank + 1 < sh.world)
            HIPCHK(c, hipMemcpyAsync(sh.ahi, hb + (int64_t)(sh.rank + 1) * 2 * P, sizeof(double) * (size_t)P,
                                     hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        sh.halo = true;
    }
    c->have_reg = true;
    c->chain_ready = false;
    c->bt.ready = false;
    return GH_OK;
}

int gh_forward(gh_ctx *c, const double *mw, double *dpre)
{
    GH_FEED_GUARD(c);
    if (!c || !mw || !dpre) return fail(c, GH_ERR_ARG, "gh_forward: null pointer");
    TRY(need(c, c->have_G, "gh_forward: no kernel matrix resident"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_forward"));
    TRY(h2d(c, c->tmpM, mw, (size_t)c->M));
    SweepArgs a{};
    a.mode = SW_FWD;
    a.x_in = c->tmpM;
    a.slab = c->slab;
    {
        FoldExact exact(c);
        TRY(launch_sweep(c, a));
    }
    reduce_slab(c, nullptr, c->tmpN);
    HIPCHK(c, hipGetLastError());
    if (!shard_rows(c)) TRY(comm_allreduce(c, c->tmpN, c->ld));  // (row blocks: the local rows are complete)
    return d2h_obsvec(c, dpre, c->tmpN);  // (forward-only sweeps never run on teams)
}

int gh_adjoint(gh_ctx *c, const double *r, double *g)
{
    GH_FEED_GUARD(c);
    if (!c || !r || !g) return fail(c, GH_ERR_ARG, "gh_adjoint: null pointer");
    TRY(need(c, c->have_G, "gh_adjoint: no kernel matrix resident"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_adjoint"));
    HIPCHK(c, hipMemsetAsync(c->tmpN, 0, sizeof(double) * (size_t)c->ld * (c->joint ? 2 : 1), c->stream));
    TRY(h2d_obsvec(c, c->tmpN, r));
    SweepArgs a{};
    a.mode = SW_ADJ | SW_GOUT;
    a.r = c->tmpN;
    a.g_out = c->tmpM;
    {
        FoldExact exact(c);
        TRY(launch_sweep(c, a));
    }
    TRY(d2h(c, g, c->tmpM, (size_t)c->M));
    for (int64_t j = 0; j < c->M; ++j) g[j] *= 0.5;  // the sweep writes 2*<G_j, r>
    return GH_OK;
}

int gh_misfit_and_grad(gh_ctx *c, const double *x, double out3[3], double *grad, double *dpre)
{
    GH_FEED_GUARD(c);
    if (!c || !x || !out3 || !grad) return fail(c, GH_ERR_ARG, "gh_misfit_and_grad: null pointer");
    TRY(need(c, c->have_G && c->have_data && c->have_reg,
             "gh_misfit_and_grad: needs a kernel matrix, gh_set_data and gh_set_reg"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_misfit_and_grad"));
    const gh_ctx::StateSet &o = c->st[3];
    TRY(h2d(c, c->xb[3], x, (size_t)c->M));
    TRY(eval_forward(c, c->xb[3], o));
    SweepArgs a{};
    a.mode = SW_ADJ | SW_GOUT;
    a.r = o.r;
    a.greg = o.greg;
    a.g_out = c->tmpM;
    TRY(launch_sweep(c, a));
    TRY(scal_ready(c, o));
    double *h = c->h_scal + c->work.h_state(), *h_phi = c->h_scal + c->work.h_phi();
    HIPCHK(c, hipMemcpyAsync(h, o.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    const bool cg_on = coupling_on(c);
    if (cg_on) HIPCHK(c, hipMemcpyAsync(h_phi, o.phi, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TRY(d2h(c, grad, c->tmpM, (size_t)c->M));
    if (dpre) TRY(d2h_obsvec(c, dpre, o.d));
    TRY(lonsym_epilogue_check(c));
    c->cg.phi_last = cg_on ? *h_phi : 0.0;
    out3[0] = h[2];
    out3[1] = h[0];
    out3[2] = h[1];
    return GH_OK;
}

int gh_reg_eval(gh_ctx *c, int kind, double beta, const int shape3[3], int ms_grad_den_mw, const double *mw,
                const double *mwapr, double *value, double *grad)
{
    GH_FEED_GUARD(c);
    if (!c || !mw || !mwapr || !value) return fail(c, GH_ERR_ARG, "gh_reg_eval: null pointer");
    if (kind < 0 || kind > 3)
        return fail(c, GH_ERR_ARG, "Please choose regularization from 'MS','Damping', 'Smoothness', 'TV'.");
    if (kind == GH_REG_SMOOTHNESS || kind == GH_REG_TV)
        if (!shape3 || (int64_t)shape3[0] * shape3[1] * shape3[2] * reg_props(c) != c->M)
            return fail(c, GH_ERR_ARG, c->joint ? "gh_reg_eval: Smoothness/TV on the joint kernel need shape nz*ny*nx == M/2"
                                       : c->mvi ? "gh_reg_eval: Smoothness/TV on the magnetization-vector store need shape "
                                                  "nz*ny*nx == M/3"
                                                : "gh_reg_eval: Smoothness/TV need shape nz*ny*nx == M");
    if (kind == GH_REG_MS) TRY(need(c, c->weighted, "gh_reg_eval: MS needs gh_weight first (uses Wm^2)"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_reg_eval"));
    double *dx = c->xb[3], *dapr = c->st[3].greg, *dg = c->tmpM;
    TRY(h2d(c, dx, mw, (size_t)c->M));
    TRY(h2d(c, dapr, mwapr, (size_t)c->M));
    // (joint and magnetization-vector stores: one property at a time, in one launch -- fd3djoint: the stencil never
    // crosses into the next block)
    RegArgs ra = reg_args(c, dx, dg, -1);
    ra.ms_grad_den_mw = ms_grad_den_mw;
    ra.kind = kind;
    ra.nz = shape3 ? shape3[0] : 1;
    ra.ny = shape3 ? shape3[1] : 1;
    ra.nx = shape3 ? shape3[2] : (int)ra.M;
    ra.alpha = 1.0;
    ra.beta = beta;
    ra.mwapr = dapr;
    reg_kernel<<<dim3(c->work.n_regpart), dim3(256), 0, c->stream>>>(ra);
    sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->regpart, c->work.n_regpart, c->st[3].scal);
    HIPCHK(c, hipGetLastError());
    TRY(read_value(c, c->st[3].scal, value));
    if (grad) TRY(d2h(c, grad, dg, (size_t)c->M));
    return GH_OK;
}

int gh_compress_wavelet(gh_ctx *c, int dims, const int shape3[3], double thr, int levels,
                        int64_t *nnz_out, int64_t *ncols_out)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(dense_single_chain_refuse(c, "gh_compress_wavelet"));
    TRY(lattice_refuse(c, "gh_compress_wavelet", "the wavelet rows need the stored kernel"));
    TRY(need(c, c->have_G && c->weighted, "gh_compress_wavelet: needs the weighted kernel (gh_weight) first"));
    if (dims != 1 && dims != 3) return fail(c, GH_ERR_ARG, "gh_compress_wavelet: dims must be 1 or 3");
    if (levels < 1 || levels > 4) return fail(c, GH_ERR_ARG, "gh_compress_wavelet: levels must be 1..4");
    if (!(thr >= 0)) return fail(c, GH_ERR_ARG, "gh_compress_wavelet: threshold must be >= 0");
    gh_ctx::Wavelet &w = c->wv;
    if (w.on || w.indptr) return fail(c, GH_ERR_ARG, "gh_compress_wavelet: already compressed");
    // (row blocks hold whole rows of the kernel: the compressor works row by row, compressor3D.py:17-44, so every rank
    // compresses its own rows; column blocks would have to exchange the rows first)
    if (c->sh.kind != 0 && !shard_rows(c))
        return fail(c, GH_ERR_UNSUPPORTED, "wavelet forward on a kernel sharded in column blocks is not supported (row blocks: gh_shard_init_rows)");
    if (dims == 3) {
        if (!shape3 || (int64_t)shape3[0] * shape3[1] * shape3[2] != c->M)
            return fail(c, GH_ERR_ARG, "cannot reshape array of size %lld into shape (%d,%d,%d)",
                        (long long)c->M, shape3 ? shape3[0] : 0, shape3 ? shape3[1] : 0, shape3 ? shape3[2] : 0);
        for (int k = 0; k < 3; ++k) {
            w.shape[k] = shape3[k];
            w.tax[k] = true;
        }
    } else {
        if (c->M > 0x7fffffffLL) return fail(c, GH_ERR_UNSUPPORTED, "model too long");
        w.shape[0] = w.shape[1] = 1;
        w.shape[2] = (int)c->M;
        w.tax[0] = w.tax[1] = false;
        w.tax[2] = true;
    }
    w.dims = dims;
    w.levels = levels;
    w.thr = thr;
    wavelet_plan(w);
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_compress_wavelet"));
    const int64_t N = c->N, M = c->M, Mp = w.Mp;
    // row chunks: 4 buffers of chunk x Mp doubles, bounded to ~2 GB in total
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(512 << 20) / (Mp * 8)));
    double *X = nullptr, *C = nullptr, *S1 = nullptr, *S2 = nullptr;
    int *count = nullptr;
    HIPCHK(c, hipMalloc((void **)&X, sizeof(double) * (size_t)(chunk * M)));
    HIPCHK(c, hipMalloc((void **)&C, sizeof(double) * (size_t)(chunk * Mp)));
    HIPCHK(c, hipMalloc((void **)&S1, sizeof(double) * (size_t)(chunk * Mp)));
    HIPCHK(c, hipMalloc((void **)&S2, sizeof(double) * (size_t)(chunk * Mp)));
    HIPCHK(c, hipMalloc((void **)&count, sizeof(int) * (size_t)N));
    TRY(dalloc(c, &w.indptr, (size_t)N + 1));
    std::vector<int> hcount((size_t)N);
    std::vector<int64_t> hptr((size_t)N + 1, 0);
    int rc = GH_OK;
    for (int pass = 0; pass < 2 && rc == GH_OK; ++pass) {
        if (pass == 1) {
            HIPCHK(c, hipMemcpyAsync(hcount.data(), count, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost,
                                     c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int64_t i = 0; i < N; ++i) hptr[i + 1] = hptr[i] + hcount[i];
            w.nnz = hptr[N];
            if (w.nnz > 0x7fffffff00LL) return fail(c, GH_ERR_UNSUPPORTED, "too many non-zeros");
            TRY(dalloc(c, &w.indices, (size_t)std::max<int64_t>(w.nnz, 1), false));
            TRY(dalloc(c, &w.data, (size_t)std::max<int64_t>(w.nnz, 1), false));
            HIPCHK(c, hipMemcpyAsync(w.indptr, hptr.data(), sizeof(int64_t) * (size_t)(N + 1),
                                     hipMemcpyHostToDevice, c->stream));
        }
        for (int64_t i0 = 0; i0 < N; i0 += chunk) {
            const int64_t nr = std::min(chunk, N - i0);
            if (c->mf) {
                // no stored kernel: the rows are evaluated (twice over the two passes: setup path)
                for (int64_t r0 = 0; r0 < nr; r0 += 32768) {
                    const int64_t rn = std::min<int64_t>(32768, nr - r0);
                    hipLaunchKernelGGL(mf_pick(c, mf_rows_kernel<MF_E_GEN>, mf_rows_kernel<MF_E_TF>,
                                               mf_rows_kernel<MF_E_COMP>, mf_rows_kernel<MF_E_TESS>),
                                       dim3((unsigned)((M + 255) / 256), (unsigned)rn), dim3(256), 0, c->stream,
                                       mf_geom(c), (const double *)c->wm, i0 + r0, rn, X + r0 * M);
                }
            } else {
                gather_rows_kernel<<<dim3((unsigned)((M + 31) / 32), (unsigned)((nr + 31) / 32)), dim3(256), 0,
                                     c->stream>>>(c->G, c->ld, M, i0, nr, X);
            }
            HIPCHK(c, hipMemsetAsync(C, 0, sizeof(double) * (size_t)(nr * Mp), c->stream));
            rc = run_dwt(c, X, M, nr, C, S1, S2);
            if (rc != GH_OK) break;
            if (pass == 0)
                csr_count_kernel<<<dim3((unsigned)nr), dim3(256), 0, c->stream>>>(C, Mp, thr, count + i0);
            else
                csr_fill_kernel<<<dim3((unsigned)nr), dim3(256), 0, c->stream>>>(C, Mp, thr, w.indptr, i0,
                                                                                 w.indices, w.data);
        }
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(X);
    hipFree(C);
    hipFree(S1);
    hipFree(S2);
    hipFree(count);
    if (rc != GH_OK) return rc;
    if (e != hipSuccess) return fail(c, GH_ERR_HIP, "gh_compress_wavelet: %s", hipGetErrorString(e));
    // (a second compression of the same context -- other dims / levels / shape, other Mp -- gets fresh,
    // zeroed scratch: the one-launch transform never writes the gaps of the packed layout and relies
    // on their being zero; the old blocks stay in the allocation list until gh_destroy)
    if (w.coeff_n != Mp) w.coeff = w.s1 = w.s2 = nullptr;
    TRY(dalloc(c, &w.coeff, (size_t)Mp));
    TRY(dalloc(c, &w.s1, (size_t)Mp));
    TRY(dalloc(c, &w.s2, (size_t)Mp));
    w.coeff_n = Mp;
    HIPCHK(c, hipMemsetAsync(w.coeff, 0, sizeof(double) * (size_t)Mp, c->stream));
    wavelet_plan_lds(c);
    w.on = true;
    w.F_valid = false;
    if (!shard_rows(c)) c->rs.state = 0;  // plan the resident chain kernel again (it would need the dense form)
    if (c->ls) c->ls->res.state = 0;  // (the persistent harmonic pass has no compressed forward: planned again, refused)
    c->chain_ready = false;
    c->bt.ready = false;
    if (nnz_out) *nnz_out = w.nnz;
    if (ncols_out) *ncols_out = Mp;
    return GH_OK;
}

int gh_download_csr(gh_ctx *c, int64_t *indptr, int32_t *indices, double *data)
{
    GH_FEED_GUARD(c);
    if (!c || !indptr || !indices || !data) return fail(c, GH_ERR_ARG, "gh_download_csr: null pointer");
    TRY(need(c, c->wv.on, "gh_download_csr: call gh_compress_wavelet first"));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(indptr, c->wv.indptr, sizeof(int64_t) * (size_t)(c->N + 1), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(indices, c->wv.indices, sizeof(int) * (size_t)c->wv.nnz, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(data, c->wv.data, sizeof(double) * (size_t)c->wv.nnz, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_model_coeffs(gh_ctx *c, const double *mw, double *coeff)
{
    GH_FEED_GUARD(c);
    if (!c || !mw || !coeff) return fail(c, GH_ERR_ARG, "gh_model_coeffs: null pointer");
    TRY(need(c, c->wv.on, "gh_model_coeffs: call gh_compress_wavelet first"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(h2d(c, c->tmpM, mw, (size_t)c->M));
    HIPCHK(c, hipMemsetAsync(c->wv.coeff, 0, sizeof(double) * (size_t)c->wv.Mp, c->stream));
    TRY(run_dwt(c, c->tmpM, c->M, 1, c->wv.coeff, c->wv.s1, c->wv.s2));
    return d2h(c, coeff, c->wv.coeff, (size_t)c->wv.Mp);
}

int gh_forward_wavelet(gh_ctx *c, const double *mw, double *dpre)
{
    GH_FEED_GUARD(c);
    if (!c || !mw || !dpre) return fail(c, GH_ERR_ARG, "gh_forward_wavelet: null pointer");
    TRY(need(c, c->wv.on, "gh_forward_wavelet: call gh_compress_wavelet first"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(h2d(c, c->tmpM, mw, (size_t)c->M));
    TRY(wavelet_forward(c, c->tmpM, c->tmpN));
    return d2h(c, dpre, c->tmpN, (size_t)c->N);
}

int gh_chain_init(gh_ctx *c, const double *x0, const double *low, const double *high)
{
    GH_FEED_GUARD(c);
    if (!c || !x0 || !low || !high) return fail(c, GH_ERR_ARG, "gh_chain_init: null pointer");
    TRY(need(c, c->have_G && c->have_data && c->have_reg,
             "gh_chain_init: needs a kernel matrix, gh_set_data and gh_set_reg"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_chain_init"));
    c->cur = 0;
    c->xcur = 0;
    c->spec_valid = c->pn_valid = false;
    c->st_stale = false;
    c->accept_count = 0;
    TRY(h2d(c, c->xb[0], x0, (size_t)c->M));
    TRY(h2d(c, c->low, low, (size_t)c->M));
    TRY(h2d(c, c->high, high, (size_t)c->M));
    TRY(eval_forward(c, c->xb[0], c->st[0]));
    TRY(scal_ready(c, c->st[0]));
    double U[3];
    TRY(read_state_scalars(c, c->st[0], U));
    c->cg.phi_cur = 0.0;
    if (coupling_on(c)) TRY(read_value(c, c->st[0].phi, &c->cg.phi_cur));
    c->cg.phi_last = c->cg.phi_cur;
    TRY(lonsym_epilogue_check(c));
    std::copy(U, U + 3, c->U_cur);  // (only of an evaluation that stands)
    c->chain_ready = true;
    return GH_OK;
}

int gh_chain_prefetch_momentum(gh_ctx *c, const double *p0_next)
{
    GH_FEED_GUARD(c);
    if (!c || !p0_next) return fail(c, GH_ERR_ARG, "gh_chain_prefetch_momentum: null pointer");
    TRY(need(c, c->chain_ready, "gh_chain_prefetch_momentum: call gh_chain_init first"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(h2d(c, c->pn, p0_next, (size_t)c->M));
    // initial kinetic energy of that trajectory, summed exactly like the non-speculative path
    sumsq_kernel<<<dim3(c->work.pp0), dim3(256), 0, c->stream>>>(c->pn, c->M, c->pp0_part);
    {
        std::vector<double> part((size_t)c->work.pp0);
        TRY(d2h(c, part.data(), c->pp0_part, (size_t)c->work.pp0));
        double s = 0.0;
        for (double v : part) s += v;
        c->pn_pp0 = s;
    }
    c->pn_probe[0] = p0_next[0];
    c->pn_probe[1] = p0_next[c->M / 2];
    c->pn_probe[2] = p0_next[c->M - 1];
    c->pn_valid = true;
    return GH_OK;
}

int gh_chain_trajectory(gh_ctx *c, const double *p0, double dt, int L, double u, int *accepted,
                        double out5[5])
{
    GH_FEED_GUARD(c);
    return chain_trajectory_impl(c, p0, dt, L, u, nullptr, accepted, out5);
}

int gh_chain_run(gh_ctx *c, int K, const int *L, const double *p0s, const double *us, double dt,
                 const double *p0_lookahead, int64_t stop_at_accepts, int64_t record_from, int *accepted,
                 double *out5s, double *x_out, int *n_run)
{
    GH_FEED_GUARD(c);
    if (!c || K < 1 || !L || !p0s || !us || !accepted || !out5s || !n_run)
        return fail(c, GH_ERR_ARG, "gh_chain_run: bad arguments");
    TRY(need(c, c->chain_ready, "gh_chain_run: call gh_chain_init first"));
    const size_t M = (size_t)c->M;
    *n_run = 0;
    // already there (a caller that submits batches ahead of looking at the results)
    if (stop_at_accepts > 0 && c->accept_count >= stop_at_accepts) return GH_OK;
    // one persistent launch for the whole batch, where the problem has one and the steps fit its granule tags (32-bit)
    const bool lonres = lonres_usable(c);
    bool fits = false;
    if (lonres || resident_usable(c)) {
        int64_t steps = 0;
        for (int k = 0; k < K; ++k) {
            if (L[k] < 1) return fail(c, GH_ERR_ARG, "gh_chain_run: L must be >= 1");
            steps += L[k];
        }
        fits = steps < ((int64_t)1 << 28);
    }
    if (lonres && fits) {
        // the shift-invariant store in the harmonic domain (lonres.hip.h)
        const int rc = chain_run_lonres(c, c, K, L, p0s, nullptr, us, dt, stop_at_accepts, record_from, accepted, out5s, x_out, n_run);
        if (rc != GH_RESIDENT_ABORTED) return rc;
        *n_run = 0;
    }
    if (fits && resident_usable(c)) {
        const int rc = chain_run_resident(c, K, L, p0s, us, dt, stop_at_accepts, record_from, accepted, out5s, x_out, n_run);
        if (rc != GH_RESIDENT_ABORTED) return rc;
        *n_run = 0;
    }
    for (int k = 0; k < K; ++k) {
        const double *nxt = (k + 1 < K) ? p0s + (size_t)(k + 1) * M : p0_lookahead;
        TRY(chain_trajectory_impl(c, p0s + (size_t)k * M, dt, L[k], us[k], nxt, &accepted[k], out5s + 5 * k));
        *n_run = k + 1;
        if (accepted[k]) {
            TRY(chain_accept_row(c, c, c->xb[c->xcur], record_from, x_out ? x_out + (size_t)k * M : nullptr));
            if (stop_at_accepts > 0 && c->accept_count >= stop_at_accepts) break;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_chain_get_x(gh_ctx *c, double *x)
{
    GH_FEED_GUARD(c);
    if (!c || !x) return fail(c, GH_ERR_ARG, "gh_chain_get_x: null pointer");
    TRY(need(c, c->chain_ready, "gh_chain_get_x: call gh_chain_init first"));
    HIPCHK(c, hipSetDevice(c->device));
    return d2h(c, x, c->xb[c->xcur], (size_t)c->M);
}

int gh_chain_get_dsyn(gh_ctx *c, double *dsyn)
{
    GH_FEED_GUARD(c);
    if (!c || !dsyn) return fail(c, GH_ERR_ARG, "gh_chain_get_dsyn: null pointer");
    TRY(need(c, c->chain_ready, "gh_chain_get_dsyn: call gh_chain_init first"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(chain_state_fresh(c));
    return d2h_obsvec(c, dsyn, c->st[c->cur].d);
}

int gh_chain_stats(gh_ctx *c, int64_t *spec_hits, int64_t *spec_misses)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (spec_hits) *spec_hits = c->spec_hits;
    if (spec_misses) *spec_misses = c->spec_misses;
    return GH_OK;
}

int gh_team_sweep_stats(gh_ctx *c, int *members, int64_t *launches, int *timeouts, int64_t *late_parts)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (late_parts) *late_parts = c->tm.late_polls;
    if (members) *members = c->tm.state != 0 ? c->tm.Q : 0;
    if (launches) *launches = c->tm.launches;
    if (timeouts) *timeouts = c->tm.xg.aborts;
    return GH_OK;
}

int gh_team_sweep_plan(gh_ctx *c, int32_t out[16])
{
    GH_FEED_GUARD(c);
    if (!c || !out) return fail(c, GH_ERR_ARG, "gh_team_sweep_plan: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 16; ++i) out[i] = 0;
    TeamShape s;
    const int why = team_shape_of(c, &s);
    // (a context whose teams gave up for good stays on row panels: the shape is what they ran on)
    out[0] = (why == TEAM_OK && c->tm.state != -1) ? 1 : 0;
    out[1] = why;
    out[2] = s.Q;
    out[3] = (int32_t)s.panel_rows;
    out[4] = (int32_t)s.last_rows;
    out[5] = s.tpx;
    out[6] = s.n_teams;
    out[7] = (int32_t)s.cols_per_team;
    out[8] = s.grid;
    out[9] = s.lag;
    out[10] = (int32_t)s.lds;
    out[11] = c->n_panels;
    out[12] = (int32_t)c->panel_rows;
    out[13] = (int32_t)(c->ld - (int64_t)(c->n_panels - 1) * c->panel_rows);
    return GH_OK;
}

int gh_chain_resident_stats(gh_ctx *c, int64_t *launches, int64_t *evaluations)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (launches) *launches = c->rs.launches;
    if (evaluations) *evaluations = c->rs.evals;
    return GH_OK;
}

int gh_chain_resident_plan(gh_ctx *c, int chains, int32_t out[16])
{
    GH_FEED_GUARD(c);
    if (!c || !out) return fail(c, GH_ERR_ARG, "gh_chain_resident_plan: null pointer");
    if (chains < 1 || chains > RES_MAX_CHAINS) return fail(c, GH_ERR_ARG, "gh_chain_resident_plan: 1..16 chains");
    TRY(need(c, c->have_G && c->have_data && c->have_reg,
             "gh_chain_resident_plan: needs the kernel (gh_build_G / gh_upload_G), gh_set_data and gh_set_reg"));
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 16; ++i) out[i] = 0;
    gh_ctx::Resident &r = c->rs;
    if (!resident_plan(c)) return GH_OK;
    out[0] = resident_usable(c) ? 1 : 0;
    out[1] = r.cpw;
    out[2] = r.nwg;
    out[3] = r.rc;
    out[4] = r.ct;
    out[5] = r.split ? 1 : 0;
    out[6] = r.stream ? 1 : 0;
    out[7] = r.lds_cols;
    out[8] = (int32_t)(resident_lds_doubles(c->ld, r.cpw, chains, r.lds_cols, r.split) * sizeof(double));
    out[9] = r.lds_max;
    int ks = 0, nt = 0;
    size_t lds = 0;
    out[10] = resbatch_shape(c, chains, &ks, &nt, &lds) ? 1 : 0;
    out[11] = ks;
    out[12] = nt;
    out[13] = (int32_t)lds;
    out[14] = 1;
    return GH_OK;
}

int gh_posterior_window(gh_ctx *c, int K)
{
    GH_FEED_GUARD(c);
    if (!c || K < 1) return fail(c, GH_ERR_ARG, "gh_posterior_window: K must be >= 1");
    if (c->ring) return fail(c, GH_ERR_ARG, "gh_posterior_window: window already allocated");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(dalloc(c, &c->ring, (size_t)K * (size_t)c->M));
    TRY(dalloc(c, &c->ring_mean, (size_t)c->M));
    TRY(dalloc(c, &c->ring_sd, (size_t)c->M));
    c->ring_K = K;
    c->ring_next = 0;
    c->ring_count = 0;
    return GH_OK;
}

int gh_posterior_add(gh_ctx *c)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->chain_ready && (c->ring || c->ps.on),
             "gh_posterior_add: needs gh_chain_init and gh_posterior_window"));
    HIPCHK(c, hipSetDevice(c->device));
    if (c->ring) TRY(ring_store_row(c, c, c->xb[c->xcur]));
    // (an explicit call: the caller decides what is recorded, the stream's window does not apply)
    if (c->ps.on) TRY(post_feed_row(c, c->ps.slot, c->xb[c->xcur], c->weighted, c->stream));
    return GH_OK;
}

int gh_posterior_read(gh_ctx *c, int64_t *n_in_window, int64_t *n_total, double *mean, double *sd)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->ring != nullptr, "gh_posterior_read: call gh_posterior_window first"));
    const int nvalid = (int)std::min<int64_t>(c->ring_count, c->ring_K);
    if (n_in_window) *n_in_window = nvalid;
    if (n_total) *n_total = c->ring_count;
    if (nvalid == 0 || (!mean && !sd)) return GH_OK;
    HIPCHK(c, hipSetDevice(c->device));
    ring_stats_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(c->ring, c->M, nvalid,
                                                                                        c->ring_mean, c->ring_sd);
    HIPCHK(c, hipGetLastError());
    if (mean) TRY(d2h(c, mean, c->ring_mean, (size_t)c->M));
    if (sd) TRY(d2h(c, sd, c->ring_sd, (size_t)c->M));
    return GH_OK;
}

int gh_posterior_stream(gh_ctx *c, int chains, int bins, int batch_len, int64_t record_from, int64_t record_count,
                        const double *lo, const double *hi)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!lo || !hi) return fail(c, GH_ERR_ARG, "gh_posterior_stream: null pointer");
    if (c->sh.kind != 0)
        return fail(c, GH_ERR_UNSUPPORTED, "the posterior stream runs on an unsharded context only: with column or row "
                                           "blocks the model or the accept decision lives on several ranks");
    if (chains < 1 || chains > POST_MAX_CHAINS) return fail(c, GH_ERR_ARG, "gh_posterior_stream: 1..16 chain slots");
    if (bins < 2 || bins > POST_MAX_BINS) return fail(c, GH_ERR_ARG, "gh_posterior_stream: 2..256 histogram bins");
    if (batch_len < 1) return fail(c, GH_ERR_ARG, "gh_posterior_stream: batch_len must be >= 1");
    if (record_from < 0 || record_count < 0)
        return fail(c, GH_ERR_ARG, "gh_posterior_stream: record_from and record_count must be >= 0");
    for (int64_t j = 0; j < c->M; ++j)
        if (!(hi[j] >= lo[j])) return fail(c, GH_ERR_ARG, "gh_posterior_stream: hi < lo (or not a number) at cell %lld", (long long)j);
    if (c->ps.on) return fail(c, GH_ERR_ARG, "gh_posterior_stream: stream already allocated (gh_posterior_stream_free first)");
    return post_alloc(c, chains, bins, batch_len, record_from, record_count, lo, hi);
}

int gh_posterior_stream_slot(gh_ctx *c, int slot)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->ps.on, "gh_posterior_stream_slot: call gh_posterior_stream first"));
    if (slot < 0 || slot >= c->ps.d.C) return fail(c, GH_ERR_ARG, "gh_posterior_stream_slot: no such chain slot");
    c->ps.slot = slot;
    return GH_OK;
}

int gh_posterior_stream_add(gh_ctx *c, int slot, const double *m)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!m) return fail(c, GH_ERR_ARG, "gh_posterior_stream_add: null pointer");
    TRY(need(c, c->ps.on, "gh_posterior_stream_add: call gh_posterior_stream first"));
    if (slot < 0 || slot >= c->ps.d.C) return fail(c, GH_ERR_ARG, "gh_posterior_stream_add: no such chain slot");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(h2d(c, c->ps.row, m, (size_t)c->M));
    return post_feed_row(c, slot, c->ps.row, false, c->stream);
}

int gh_posterior_stream_read(gh_ctx *c, int64_t *n_per_chain, double *mean, double *sd, double *rhat, double *ess,
                             double *chain_mean, double *chain_M2)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->ps.on, "gh_posterior_stream_read: call gh_posterior_stream first"));
    return post_read(c, n_per_chain, mean, sd, rhat, ess, chain_mean, chain_M2);
}

int gh_posterior_stream_quantiles(gh_ctx *c, int nq, const double *q, double *out)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->ps.on, "gh_posterior_stream_quantiles: call gh_posterior_stream first"));
    if (nq < 1 || nq > POST_MAX_Q || !q || !out) return fail(c, GH_ERR_ARG, "gh_posterior_stream_quantiles: 1..32 quantiles");
    for (int i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(c, GH_ERR_ARG, "gh_posterior_stream_quantiles: q must lie in [0, 1]");
    return post_quantiles(c, nq, q, out);
}

int gh_posterior_stream_hist(gh_ctx *c, uint32_t *out)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!out) return fail(c, GH_ERR_ARG, "gh_posterior_stream_hist: null pointer");
    TRY(need(c, c->ps.on, "gh_posterior_stream_hist: call gh_posterior_stream first"));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->ps.d.H, sizeof(uint32_t) * (size_t)c->ps.d.B * (size_t)c->M, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_posterior_stream_free(gh_ctx *c)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (!c->ps.on) return GH_OK;
    return post_free(c);
}

int gh_batch_init(gh_ctx *c, int C, const double *x0s, const double *low, const double *high)
{
    GH_FEED_GUARD(c);
    if (!c || !x0s || !low || !high) return fail(c, GH_ERR_ARG, "gh_batch_init: null pointer");
    TRY(dense_single_chain_refuse(c, "gh_batch_init"));  // (passes the table of blocks that takes batches)
    TRY(lattice_batch_refuse(c, "gh_batch_init"));
    if (C < 1 || C > CB) return fail(c, GH_ERR_ARG, "gh_batch_init: 1..16 chains per batch");
    TRY(need(c, c->have_G && c->have_data && c->have_reg,
             "gh_batch_init: needs the kernel (gh_build_G / gh_upload_G), gh_set_data and gh_set_reg"));
    if (c->sh.kind != 0)
        return fail(c, GH_ERR_UNSUPPORTED, "batched chains run on the unsharded kernel only");
    // (the translation-invariant table serves gz, components and the total field alike: a context that takes batches on
    // it passes the three refusals below)
    const bool on_table = lattice_chains(c) && lattice_on(c);
    if (lattice_multi_chains(c) && !on_table)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_batch_init: needs the table of %s (gh_build_G)", LATTICE_NAME);
    if (on_table) TRY(latb_plan(c, "gh_batch_init"));  // (an extent the batch tile cannot hold: refused before anything is made)
    if (c->mf && !on_table && c->cell_kind == GH_CELL_PRISM_TF)
        return fail(c, GH_ERR_UNSUPPORTED, "batched chains on a matrix-free kernel of the magnetic field (total field, "
                                           "GH_CELL_PRISM_TF) are not supported: store the kernel or run single chains");
    if (c->mf && !on_table && c->cell_kind == GH_CELL_PRISM_COMP)
        return fail(c, GH_ERR_UNSUPPORTED, "batched chains on a matrix-free kernel of a prism gravity component other "
                                           "than gz (GH_CELL_PRISM_COMP) are not supported: store the kernel or run "
                                           "single chains");
    if (c->mf && c->cell_kind == GH_CELL_TESSEROID_COMP)
        return fail(c, GH_ERR_UNSUPPORTED, "batched chains on a matrix-free kernel of a tesseroid gravity component "
                                           "other than gz (GH_CELL_TESSEROID_COMP) are not supported: store the kernel "
                                           "or run single chains");
    HIPCHK(c, hipSetDevice(c->device));
    for (int64_t &n : c->bt_accepts) n = 0;
    if (lonsym_on(c)) {
        // (the light contexts of the chains share the tables, not a compressed forward operator)
        if (c->wv.on) return fail(c, GH_ERR_UNSUPPORTED, "batched chains on the shift-invariant store run without the wavelet-compressed forward");
        return kids_make(c, C, x0s, low, high);
    }
    // (the wavelet-compressed forward only where the resident chain kernel takes the batch: the MFMA
    // batch has no compressed forward)
    if (c->wv.on && !(resident_usable(c) && resident_lds_doubles(c->ld, c->rs.cpw, C, c->rs.lds_cols, c->rs.split) *
                                                  sizeof(double) <= (size_t)c->rs.lds_max))
        return fail(c, GH_ERR_UNSUPPORTED, "batched chains with the wavelet-compressed forward need a problem "
                                           "small enough for the resident chain kernel");
    TRY(ensure_work(c, "gh_batch_init"));
    TRY(h2d(c, c->low, low, (size_t)c->M));
    TRY(h2d(c, c->high, high, (size_t)c->M));
    gh_ctx::Resident &r = c->rs;
    r.b_on = false;
    c->bt.run = gh_ctx::Batch::Run();  // anything gh_batch_run left in flight is discarded
    // (the table of blocks: never the resident kernel, which knows one mean)
    if (!lattice_multi_chains(c) && resident_usable(c) &&
        resident_lds_doubles(c->ld, r.cpw, C, r.lds_cols, r.split) * sizeof(double) <= (size_t)r.lds_max) {
        // small problem: the chains take turns inside the resident chain kernel (one launch per
        // round of trajectories, G loaded into LDS once for all of them) -- a sweep of a 30 MB G
        // per launch would leave the MFMA batch bound by launches
        static_assert(CB <= RES_MAX_CHAINS, "chains per batch");
        TRY(dalloc(c, &r.bx, (size_t)CB * (size_t)c->M));
        TRY(dalloc(c, &r.bg, (size_t)CB * (size_t)c->M));
        TRY(dalloc(c, &r.bu, 3 * (size_t)CB));
        TRY(h2d(c, r.bx, x0s, (size_t)C * (size_t)c->M));
        r.b_on = true;
        r.b_state = false;
        c->bt.C = C;
        c->bt.ready = true;
        // two or more chains: all of them in lock-step, one exchange per step of the whole batch (resbatch.hip.h)
        (void)resbatch_plan(c, C);
        return GH_OK;
    }
    return batch_init_mfma(c, C, x0s);
}

int gh_batch_trajectory(gh_ctx *c, const double *p0s, double dt, const int *L, const double *us, int *accepted,
                        double *out5s)
{
    GH_FEED_GUARD(c);
    if (!c || !p0s || !L || !us || !accepted || !out5s) return fail(c, GH_ERR_ARG, "gh_batch_trajectory: null pointer");
    TRY(dense_single_chain_refuse(c, "gh_batch_trajectory"));
    TRY(lattice_batch_refuse(c, "gh_batch_trajectory"));
    gh_ctx::Batch &b = c->bt;
    TRY(need(c, b.ready, "gh_batch_trajectory: call gh_batch_init first"));
    for (int k = 0; k < b.C; ++k)
        if (b.run.live && b.run.active[k])
            return fail(c, GH_ERR_ARG, "gh_batch_trajectory: gh_batch_run left trajectories in flight (drain them with T = 0)");
    b.run.live = false;
    HIPCHK(c, hipSetDevice(c->device));
    const int C = b.C;
    for (int k = 0; k < C; ++k)
        if (L[k] < 1) return fail(c, GH_ERR_ARG, "gh_batch_trajectory: L must be >= 1");
    if (!c->kids.empty()) return kids_run(c, 1, L, nullptr, p0s, us, dt, accepted, out5s, nullptr, 1);
    if (c->rs.b_on && c->rs.ls.on) {
        for (int k = 0; k < C; ++k)
            if (c->rs.ls.active[k])
                return fail(c, GH_ERR_ARG, "gh_batch_trajectory: gh_batch_run left trajectories in flight (drain them with T = 0)");
        int rc = resbatch_state(c);
        if (rc == GH_OK) rc = resbatch_launch(c, 1, L, nullptr, p0s, us, dt, false, accepted, out5s, nullptr, nullptr, nullptr);
        if (rc == GH_OK) return GH_OK;
        if (rc != GH_RESIDENT_ABORTED) return rc;
        c->rs.ls.on = false;  // (nothing was in flight: the chains take turns from here on)
    }
    if (c->rs.b_on) {
        int chain_of[CB];
        for (int k = 0; k < C; ++k) chain_of[k] = k;
        const int rc = batch_resident_turns(c, C, chain_of, L, p0s, us, dt, false, false, accepted, out5s);
        if (rc != GH_RESIDENT_ABORTED) return rc;
    }
    // fp64-MFMA batch, a round in lock-step (host_batchrun.h).  A fused team pass of the round gave up: nothing of the
    // chains' current states was touched -- run the round again (the fused form is off from here on)
    bool failed = false;
    TRY(batch_round_lockstep(c, p0s, dt, L, us, accepted, out5s, &failed));
    if (failed) return gh_batch_trajectory(c, p0s, dt, L, us, accepted, out5s);
    return GH_OK;
}

int gh_batch_run(gh_ctx *c, int T, const int *L, const double *const *p0s, const double *us, double dt,
                 int *accepted, double *out5s, double *x_out, int *n_started, int *n_done)
{
    GH_FEED_GUARD(c);
    if (!c || T < 0 || (T > 0 && (!L || !p0s || !us)) || !accepted || !out5s || ((n_started == nullptr) != (n_done == nullptr)))
        return fail(c, GH_ERR_ARG, "gh_batch_run: bad arguments");
    TRY(dense_single_chain_refuse(c, "gh_batch_run"));
    TRY(lattice_batch_refuse(c, "gh_batch_run"));
    if (T == 0 && !n_done) return fail(c, GH_ERR_ARG, "gh_batch_run: T = 0 (drain) needs n_started / n_done");
    gh_ctx::Batch &b = c->bt;
    TRY(need(c, b.ready, "gh_batch_run: call gh_batch_init first"));
    HIPCHK(c, hipSetDevice(c->device));
    const int C = b.C;
    const size_t M = (size_t)c->M;
    for (int k = 0; k < C * T; ++k)
        if (L[k] < 1 || !p0s[k]) return fail(c, GH_ERR_ARG, "gh_batch_run: L must be >= 1 and every momentum row given");
    if (!c->kids.empty()) {
        // shift-invariant store: every chain runs its T trajectories on its own stream; nothing stays in flight
        TRY(kids_run(c, T, L, p0s, nullptr, us, dt, accepted, out5s, x_out, n_done ? T + 1 : T));
        for (int ch = 0; ch < C && n_done; ++ch) n_started[ch] = n_done[ch] = T;
        return GH_OK;
    }
    // trajectories the lock-step kernel had in flight when it gave up: replayed in front of the new lists
    std::vector<int> pre_ch, pre_L;
    std::vector<double> pre_us, pre_p0;
    if (c->rs.b_on && c->rs.ls.on) {
        gh_ctx::Resident::LockStep &b = c->rs.ls;
        bool any_active = false;
        for (int ch = 0; ch < C; ++ch) any_active = any_active || b.active[ch];
        if (!n_done && any_active)
            return fail(c, GH_ERR_ARG, "gh_batch_run: trajectories in flight from a carry-over call (drain them with T = 0)");
        if (T == 0 && !any_active) {
            for (int ch = 0; ch < C; ++ch) n_started[ch] = n_done[ch] = 0;
            return GH_OK;
        }
        int rc = resbatch_state(c);
        if (rc == GH_OK)
            rc = resbatch_launch(c, T, L, p0s, nullptr, us, dt, n_done != nullptr, accepted, out5s, x_out, n_started, n_done);
        if (rc == GH_OK) return GH_OK;
        if (rc != GH_RESIDENT_ABORTED) return rc;
        b.on = false;
        TRY(resbatch_inflight(c, pre_ch, pre_L, pre_us, pre_p0));
    }
    if (c->rs.b_on && T == 0 && pre_ch.empty()) {
        for (int ch = 0; ch < C; ++ch) n_started[ch] = n_done[ch] = 0;  // nothing is ever left in flight there
        return GH_OK;
    }
    if (c->rs.b_on) {
        // small problem: the chains take turns inside the resident chain kernel, trajectory t of
        // every chain before trajectory t + 1 of any (in front of them what the lock-step kernel left in flight)
        const int P = (int)pre_ch.size(), K = P + C * T;
        std::vector<int> chain_of((size_t)K), Lk((size_t)K), acc((size_t)K), has_pre((size_t)C, 0);
        std::vector<double> pk((size_t)K * M), uk((size_t)K), o5((size_t)K * 5);
        for (int k = 0; k < P; ++k) {
            chain_of[k] = pre_ch[k];
            Lk[k] = pre_L[k];
            uk[k] = pre_us[k];
            memcpy(pk.data() + (size_t)k * M, pre_p0.data() + (size_t)k * M, M * sizeof(double));
            has_pre[(size_t)pre_ch[k]] = 1;
        }
        for (int t = 0; t < T; ++t)
            for (int ch = 0; ch < C; ++ch) {
                const int k = P + t * C + ch, src = ch * T + t;
                chain_of[k] = ch;
                Lk[k] = L[src];
                uk[k] = us[src];
                memcpy(pk.data() + (size_t)k * M, p0s[src], M * sizeof(double));
            }
        const int rc = batch_resident_turns(c, K, chain_of.data(), Lk.data(), pk.data(), uk.data(), dt, x_out != nullptr, P > 0,
                                            acc.data(), o5.data());
        if (rc == GH_OK) {
            const int Tout = n_done ? T + 1 : T;
            for (int k = 0; k < K; ++k) {
                const int ch = chain_of[k];
                const int i = k < P ? 0 : (k - P) / C + has_pre[(size_t)ch];
                const int dst = ch * Tout + i;
                accepted[dst] = acc[k];
                memcpy(out5s + (size_t)dst * 5, o5.data() + (size_t)k * 5, 5 * sizeof(double));
                if (x_out && acc[k])
                    HIPCHK(c, hipMemcpyAsync(x_out + (size_t)dst * M, c->rs.lists.xacc + (size_t)k * M, M * sizeof(double),
                                             hipMemcpyDeviceToHost, c->stream));
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int ch = 0; ch < C && n_done; ++ch) {
                n_started[ch] = T;
                n_done[ch] = T + has_pre[(size_t)ch];
            }
            return GH_OK;
        }
        if (rc != GH_RESIDENT_ABORTED) return rc;
    }
    // fp64-MFMA batch, the chains desynchronised (host_batchrun.h)
    return BatchRun{c, T, L, p0s, us, dt, accepted, out5s, x_out, n_done != nullptr}.go(n_started, n_done);
}

// Diagnostic: the layout the work buffers were allocated by (host_layout.h), so that a
// test can assert the epilogue form it meant to reach.  out[0..15]: allocated (0 / 1), slab rows, slab2 segments, pp,
// pp0, dsum, bsum, n_dpart, n_regpart, R blocks per property, form of `part` (WORK_PART_*), size of `part`,
// offset of R in `part`, offset of the coupling term in `part`, size of h_scal, slab rows the last forward wrote.
int gh_debug_work_layout(const gh_ctx *c, int64_t *out)
{
    GH_FEED_GUARD(c);
    if (!c || !out) return GH_ERR_ARG;
    const WorkLayout &w = c->work;
    const int64_t v[16] = {c->work_ready ? 1 : 0, w.slab_rows, w.slab2_rows, w.pp, w.pp0, w.dsum, w.bsum, w.n_dpart,
                           w.n_regpart, w.reg_blocks, w.part_form, w.size(), w.reg(0), w.coupling(), (int64_t)w.h_size(),
                           c->slab_live};
    std::copy(v, v + 16, out);
    return GH_OK;
}

// Diagnostic (not in the public header): accumulated phase times of the shift-invariant pass
// (GRAVHMC_LONSYM_TIMING=1), 100 MHz ticks of workgroup 0.
int gh_debug_lonsym_timing(gh_ctx *c, long long out8[8])
{
    GH_FEED_GUARD(c);
    if (!c || !out8) return GH_ERR_ARG;
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!c->ls || !c->ls->dbg) return GH_OK;
    HIPCHK(c, hipMemcpyAsync(out8, c->ls->dbg, 8 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

// Diagnostic (not in the public header): accumulated phase times of workgroup 0 of the persistent harmonic pass
// (GRAVHMC_LONSYM_TIMING=1; lonres.hip.h), 100 MHz ticks.
int gh_debug_lonres_timing(gh_ctx *c, long long out16[16])
{
    GH_FEED_GUARD(c);
    if (!c || !out16) return GH_ERR_ARG;
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    if (!c->ls || !c->ls->res.dbg) return GH_OK;
    HIPCHK(c, hipMemcpyAsync(out16, c->ls->res.dbg, 16 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

// Diagnostic (not in the public header): accumulated phase times of the fused matrix-free batch pass
// (GRAVHMC_MFB_TIMING=1), 100 MHz ticks of workgroup (0, 0).
int gh_debug_mfb_timing(gh_ctx *c, long long out8[8])
{
    GH_FEED_GUARD(c);
    if (!c || !out8) return GH_ERR_ARG;
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!c->bt.fus_dbg) return GH_OK;
    HIPCHK(c, hipMemcpyAsync(out8, c->bt.fus_dbg, 8 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}

int gh_batch_fused_stats(gh_ctx *c, int *members, int *ranges, int64_t *launches, int *timeouts)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const gh_ctx::Batch &b = c->bt;
    if (members) *members = b.fus_on ? b.fus_members : 0;
    if (ranges) *ranges = b.fus_on ? b.fus_ranges : 0;
    if (launches) *launches = b.fus_launches;
    if (timeouts) *timeouts = b.fus.aborts;
    return GH_OK;
}

int gh_matrix_free_team_stats(gh_ctx *c, int *members, int *ranges, int64_t *launches, int *timeouts)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const gh_ctx::MfTeam &t = c->mft;
    if (members) *members = t.state == 1 ? t.members : 0;
    if (ranges) *ranges = t.state == 1 ? t.ranges : 0;
    if (launches) *launches = t.launches;
    if (timeouts) *timeouts = t.xg.aborts;
    return GH_OK;
}

int gh_batch_resident_stats(gh_ctx *c, int64_t *launches, int64_t *lock_steps, int64_t *chain_steps, int64_t *lost_steps,
                            int *timeouts)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const gh_ctx::Resident::LockStep &b = c->rs.ls;
    if (launches) *launches = b.launches;
    if (lock_steps) *lock_steps = b.lock_steps;
    if (chain_steps) *chain_steps = b.chain_steps;
    if (lost_steps) *lost_steps = b.lost;
    if (timeouts) *timeouts = b.xg.aborts;
    return GH_OK;
}

int gh_pinned_alloc(gh_ctx *c, size_t bytes, void **host)
{
    GH_FEED_GUARD(c);
    if (!c || !host || bytes == 0) return fail(c, GH_ERR_ARG, "gh_pinned_alloc: null pointer or no bytes");
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    HIPCHK(c, hipHostMalloc(&p, bytes));
    c->pinned.push_back({(char *)p, bytes});
    *host = p;
    return GH_OK;
}

int gh_pinned_free(gh_ctx *c, void *host)
{
    GH_FEED_GUARD(c);
    if (!c || !host) return fail(c, GH_ERR_ARG, "gh_pinned_free: null pointer");
    for (size_t i = 0; i < c->pinned.size(); ++i)
        if (c->pinned[i].base == (char *)host) {
            HIPCHK(c, hipSetDevice(c->device));
            if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipHostFree(host));
            c->pinned.erase(c->pinned.begin() + (long)i);
            return GH_OK;
        }
    return fail(c, GH_ERR_ARG, "gh_pinned_free: not a block of gh_pinned_alloc");
}

int gh_batch_staging_stats(gh_ctx *c, int64_t *rows_direct, int64_t *rows_staged)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (rows_direct) *rows_direct = c->rs.ls.lists.rows_direct;
    if (rows_staged) *rows_staged = c->rs.ls.lists.rows_staged;
    return GH_OK;
}

// Diagnostic only, without a device or a context: how traj_upload would send K rows of M doubles at the addresses
// rows[k], given pinned blocks [bases[b], bases[b] + bytes[b]).  Nothing is read through any of the pointers.
// direct[k]: the row goes from where it lies; run_end[i], i < *n_runs: the row one past copy run i (K entries of room).
int gh_debug_row_copy_plan(int K, const double *const *rows, int64_t M, int n_blocks, const char *const *bases,
                           const int64_t *bytes, char *direct, int *run_end, int *n_runs, int *n_staged)
{
    if (K < 1 || !rows || M < 1 || n_blocks < 0 || (n_blocks && (!bases || !bytes)) || !direct || !run_end || !n_runs || !n_staged)
        return GH_ERR_ARG;
    std::vector<PinnedBlock> blocks;
    for (int b = 0; b < n_blocks; ++b) blocks.push_back({const_cast<char *>(bases[b]), (size_t)bytes[b]});
    const RowCopyPlan p = row_copy_plan(rows, K, (size_t)M, blocks.data(), blocks.size());
    std::copy(p.direct.begin(), p.direct.end(), direct);
    std::copy(p.run_end.begin(), p.run_end.end(), run_end);
    *n_runs = (int)p.run_end.size();
    *n_staged = p.n_staged;
    return GH_OK;
}

int gh_batch_get_x(gh_ctx *c, int chain, double *x)
{
    GH_FEED_GUARD(c);
    if (!c || !x) return fail(c, GH_ERR_ARG, "gh_batch_get_x: null pointer");
    TRY(need(c, c->bt.ready, "gh_batch_get_x: call gh_batch_init first"));
    TRY(need(c, chain >= 0 && chain < c->bt.C, "gh_batch_get_x: no such chain"));
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->kids.empty()) return gh_chain_get_x(c->kids[(size_t)chain], x);
    if (c->rs.b_on) return d2h(c, x, c->rs.bx + (size_t)chain * (size_t)c->M, (size_t)c->M);
    batch_extract_kernel<<<dim3((unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream>>>(c->bt.Xc, chain, c->M,
                                                                                           c->tmpM);
    HIPCHK(c, hipGetLastError());
    return d2h(c, x, c->tmpM, (size_t)c->M);
}

int gh_batch_block_means(gh_ctx *c, double *pred_mean)
{
    GH_FEED_GUARD(c);
    if (!c || !pred_mean) return fail(c, GH_ERR_ARG, "gh_batch_block_means: null pointer");
    TRY(need(c, c->bt.ready, "gh_batch_block_means: call gh_batch_init first"));
    if (!lattice_multi_chains(c) || !c->bt.bmean)
        return fail(c, GH_ERR_UNSUPPORTED, "gh_batch_block_means: not a batch on a table of row blocks "
                                           "(gh_set_cells_multi_table_chains)");
    HIPCHK(c, hipSetDevice(c->device));
    // (from the chains' current predictions, as the evaluation formed them: bt.bmean holds the last evaluation's, which
    // may be a rejected proposal's)
    const int nb = c->lat->nb;
    TRY(dalloc(c, &c->bt.bmean_cur, (size_t)CB * (size_t)nb));
    double *out = c->bt.bmean_cur;
    batch_block_means_kernel<<<dim3(CB), dim3(1024), 0, c->stream>>>(c->bt.Dc, c->have_fix ? c->gfix : nullptr, nb,
                                                                     store_points(c), out);
    HIPCHK(c, hipGetLastError());
    return d2h(c, pred_mean, out, (size_t)c->bt.C * (size_t)nb);
}

int gh_bscg_run(gh_ctx *c, int B, const double *counts, const double *dobs, const double *mw0, double rhomin, double rhomax,
                double beta2, double q, int maxk, double *models, double *dmis, double *mmis, double *alpha, int *n_entries,
                int *n_alpha)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    TRY(bscg_refuse(c, B, maxk));
    if (!counts || !dobs || !mw0 || !models || !dmis || !mmis || !alpha || !n_entries || !n_alpha)
        return fail(c, GH_ERR_ARG, "gh_bscg_run: null pointer");
    if (!(beta2 > 0.0) || !std::isfinite(beta2) || !std::isfinite(q) || !(rhomin <= rhomax))
        return fail(c, GH_ERR_ARG, "gh_bscg_run: needs beta2 > 0, a finite q and rhomin <= rhomax");
    HIPCHK(c, hipSetDevice(c->device));
    return bscg_run(c, B, counts, dobs, mw0, rhomin, rhomax, beta2, q, maxk, models, dmis, mmis, alpha, n_entries, n_alpha);
}

int gh_bscg_stats(const gh_ctx *c, int64_t *forward_sweeps, int64_t *adjoint_sweeps, int64_t *lock_steps)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    if (forward_sweeps) *forward_sweeps = c->bs.forward_sweeps;
    if (adjoint_sweeps) *adjoint_sweeps = c->bs.adjoint_sweeps;
    if (lock_steps) *lock_steps = c->bs.lock_steps;
    return GH_OK;
}

int gh_leapfrog(gh_ctx *c, double *x_inout, const double *p0, double dt, int L, const double *low,
                const double *high, double u, int *accepted, double out5[5], double *dsyn)
{
    GH_FEED_GUARD(c);
    TRY(gh_chain_init(c, x_inout, low, high));
    TRY(gh_chain_trajectory(c, p0, dt, L, u, accepted, out5));
    TRY(gh_chain_get_x(c, x_inout));
    if (dsyn) TRY(gh_chain_get_dsyn(c, dsyn));
    return GH_OK;
}

// Diagnostic (not in the public header): time a pure streaming read of the resident G.
int gh_debug_resident_timing(gh_ctx *c, long long out32[32], int64_t *launches, int64_t *evals)
{
    GH_FEED_GUARD(c);
    if (!c || !out32) return GH_ERR_ARG;
    if (launches) *launches = c->rs.launches;
    if (evals) *evals = c->rs.evals;
    for (int i = 0; i < 32; ++i) out32[i] = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->rs.ls.dbg && c->rs.ls.launches > 0) {
        // chains in lock-step (resbatch.hip.h): its clocks, launches and lock-steps
        if (launches) *launches = c->rs.ls.launches;
        if (evals) *evals = c->rs.ls.lock_steps;
        HIPCHK(c, hipMemcpy(out32, c->rs.ls.dbg, 32 * sizeof(long long), hipMemcpyDeviceToHost));
        return GH_OK;
    }
    if (!c->rs.dbg) return GH_OK;
    HIPCHK(c, hipMemcpy(out32, c->rs.dbg, 32 * sizeof(long long), hipMemcpyDeviceToHost));
    return GH_OK;
}

int gh_debug_stream_read(gh_ctx *c, int blocks, int threads, int nt, int reps, double *ms_out);

int gh_measure_stream_read(gh_ctx *c, int nt, int reps, double *ms_per_pass)
{
    GH_FEED_GUARD(c);
    if (!c || !ms_per_pass || reps < 1) return fail(c, GH_ERR_ARG, "gh_measure_stream_read: bad arguments");
    TRY(need(c, c->have_G && !c->mf, "gh_measure_stream_read: needs a stored kernel matrix"));
    // the best of three launch shapes (the rate of a plain read depends on how many wide loads the
    // chip keeps in flight: 2 x CUs blocks of 256 threads reach ~6.9 TB/s where 2 x CUs of 1024 get 6.5)
    const int shapes[3][2] = {{c->cus * 2, 256}, {c->cus, 512}, {c->cus * 16, 1024}};
    double best = 0.0;
    for (int k = 0; k < 3; ++k) {
        double ms = 0.0;
        TRY(gh_debug_stream_read(c, shapes[k][0], shapes[k][1], nt, reps, &ms));
        if (k == 0 || ms < best) best = ms;
    }
    *ms_per_pass = best;
    return GH_OK;
}

int gh_debug_stream_read(gh_ctx *c, int blocks, int threads, int nt, int reps, double *ms_out)
{
    GH_FEED_GUARD(c);
    if (!c || !c->have_G) return GH_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_work(c, "gh_debug_stream_read"));
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    const int64_t n2 = c->ld * c->M / 2;
    for (int w = 0; w < 2; ++w) {
        if (w == 1) HIPCHK(c, hipEventRecord(e0, c->stream));
        for (int r = 0; r < (w ? reps : 1); ++r) {
            if (nt)
                stream_read_kernel<true><<<dim3(blocks), dim3(threads), 0, c->stream>>>(c->G, n2, c->tmpN);
            else
                stream_read_kernel<false><<<dim3(blocks), dim3(threads), 0, c->stream>>>(c->G, n2, c->tmpN);
        }
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *ms_out = t / reps;
    return GH_OK;
}

int gh_shard_unique_id(void *id128)
{
    if (!id128) return GH_ERR_ARG;
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(nullptr, GH_ERR_COMM, "%s", err.c_str());
    ncclUniqueId id;
    ncclResult_t r = api->GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, GH_ERR_COMM, "ncclGetUniqueId failed");
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, sizeof id);
    return GH_OK;
}

int gh_shard_init(gh_ctx *c, const void *id128, int rank, int world, int64_t M_global, int64_t m0)
{
    GH_FEED_GUARD(c);
    if (!c || !id128) return fail(c, GH_ERR_ARG, "gh_shard_init: null pointer");
    if (c->sh.kind != 0) return fail(c, GH_ERR_ARG, "gh_shard_init: already initialised");
    TRY(dense_single_chain_refuse(c, "gh_shard_init"));
    TRY(lattice_refuse(c, "gh_shard_init", "one GPU holds the table"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(shard_common_init(c, rank, world, M_global, m0));
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(c, GH_ERR_COMM, "%s", err.c_str());
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclResult_t r = api->CommInitRank(&c->sh.comm, world, id, rank);
    if (r != ncclSuccess)
        return fail(c, GH_ERR_COMM, "ncclCommInitRank: %s", api->GetErrorString ? api->GetErrorString(r) : "error");
    c->sh.kind = 1;
    return GH_OK;
}

int gh_shard_init_callback(gh_ctx *c, gh_allreduce_fn fn, void *user, int rank, int world, int64_t M_global,
                           int64_t m0)
{
    GH_FEED_GUARD(c);
    if (!c || !fn) return fail(c, GH_ERR_ARG, "gh_shard_init_callback: null pointer");
    if (c->sh.kind != 0) return fail(c, GH_ERR_ARG, "gh_shard_init: already initialised");
    TRY(dense_single_chain_refuse(c, "gh_shard_init"));
    TRY(lattice_refuse(c, "gh_shard_init", "one GPU holds the table"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(shard_common_init(c, rank, world, M_global, m0));
    c->sh.cb = fn;
    c->sh.user = user;
    c->sh.kind = 2;
    return GH_OK;
}

int gh_shard_init_rows(gh_ctx *c, const void *id128, int rank, int world, int64_t N_global, int64_t n0)
{
    GH_FEED_GUARD(c);
    if (!c || !id128) return fail(c, GH_ERR_ARG, "gh_shard_init_rows: null pointer");
    if (c->sh.kind != 0) return fail(c, GH_ERR_ARG, "gh_shard_init_rows: already initialised");
    TRY(dense_single_chain_refuse(c, "gh_shard_init_rows"));
    TRY(lattice_refuse(c, "gh_shard_init_rows", "one GPU holds the table"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(shard_rows_init(c, rank, world, N_global, n0));
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(c, GH_ERR_COMM, "%s", err.c_str());
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclResult_t r = api->CommInitRank(&c->sh.comm, world, id, rank);
    if (r != ncclSuccess)
        return fail(c, GH_ERR_COMM, "ncclCommInitRank: %s", api->GetErrorString ? api->GetErrorString(r) : "error");
    c->sh.kind = 1;
    return GH_OK;
}

int gh_shard_init_rows_callback(gh_ctx *c, gh_allreduce_fn fn, void *user, int rank, int world, int64_t N_global,
                                int64_t n0)
{
    GH_FEED_GUARD(c);
    if (!c || !fn) return fail(c, GH_ERR_ARG, "gh_shard_init_rows_callback: null pointer");
    if (c->sh.kind != 0) return fail(c, GH_ERR_ARG, "gh_shard_init_rows: already initialised");
    TRY(dense_single_chain_refuse(c, "gh_shard_init_rows"));
    TRY(lattice_refuse(c, "gh_shard_init_rows", "one GPU holds the table"));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(shard_rows_init(c, rank, world, N_global, n0));
    c->sh.cb = fn;
    c->sh.user = user;
    c->sh.kind = 2;
    return GH_OK;
}

int gh_shard_allreduce(gh_ctx *c, double *host_buf, int64_t count)
{
    GH_FEED_GUARD(c);
    if (!c || !host_buf) return fail(c, GH_ERR_ARG, "gh_shard_allreduce: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    return comm_allreduce_host(c, host_buf, count);
}

// values [0, n) of a row; the row's last value (ends_row) is followed by the newline, every other one by a blank
static int64_t format_fixed8_range(const double *v, int64_t n, char *out, int64_t cap, bool ends_row)
{
    static const char DIG2[] =
        "00010203040506070809101112131415161718192021222324252627282930313233343536373839"
        "40414243444546474849505152535455565758596061626364656667686970717273747576777879"
        "8081828384858687888990919293949596979899";
    int64_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (cap - pos < 32) return -1;  // (the fast path writes at most 28 bytes; snprintf checks itself)
        const double x = v[i];
        const double a = std::fabs(x);
        bool fast = a < 9.0e15;  // (false for NaN and infinities too)
        uint64_t ip = 0;
        uint32_t fr = 0;
        if (fast) {
            ip = (uint64_t)a;  // floor of a non-negative value
            const double scaled = (a - (double)ip) * 1e8;  // a - floor(a) is exact; the product is within 1 ulp (1.5e-8)
            const double r = (scaled + 6755399441055744.0) - 6755399441055744.0;  // to nearest, ties to even
            // certain only away from the rounding boundary (and from a tie, which printf breaks on
            // the exact binary value)
            if (std::fabs(std::fabs(scaled - r) - 0.5) < 1e-7) fast = false;
            fr = (uint32_t)r;
            if (fr >= 100000000u) {
                fr -= 100000000u;
                ip += 1;
            }
        }
        if (!fast) {
            const int k = snprintf(out + pos, (size_t)(cap - pos), "%.8f", x);
            if (k < 0 || k >= cap - pos - 2) return -1;
            pos += k;
        } else {
            if (std::signbit(x)) out[pos++] = '-';
            if (ip < 10) {
                out[pos++] = (char)('0' + ip);
            } else {
                char tmp[24];
                int nd = 0;
                do {
                    tmp[nd++] = (char)('0' + ip % 10);
                    ip /= 10;
                } while (ip);
                while (nd) out[pos++] = tmp[--nd];
            }
            out[pos++] = '.';
            const uint32_t hi4 = fr / 10000u, lo4 = fr % 10000u;
            const uint32_t d0 = hi4 / 100u, d1 = hi4 % 100u, d2 = lo4 / 100u, d3 = lo4 % 100u;
            memcpy(out + pos, DIG2 + 2 * d0, 2);
            memcpy(out + pos + 2, DIG2 + 2 * d1, 2);
            memcpy(out + pos + 4, DIG2 + 2 * d2, 2);
            memcpy(out + pos + 6, DIG2 + 2 * d3, 2);
            pos += 8;
        }
        out[pos++] = (i + 1 < n || !ends_row) ? ' ' : '\n';
    }
    return pos;
}


int64_t gh_format_row_fixed8(const double *v, int64_t n, char *out, int64_t cap)
{
    if (!v || !out || n < 0) return -1;
    if (n == 0) {
        if (cap < 1) return -1;
        out[0] = '\n';
        return 1;
    }
    // (a model of 72 000 cells is 0.8 ms of formatting per accepted sample -- as long as three of its trajectories on
    // the GPU: long rows are formatted in up to four pieces side by side and joined; the bytes are the same)
    const int T = (int)std::min<int64_t>(4, n / 16384);
    if (T <= 1) return format_fixed8_range(v, n, out, cap, true);
    std::vector<std::vector<char>> buf((size_t)T);
    std::vector<int64_t> len((size_t)T, -1);
    auto work = [&](int t) {
        const int64_t i0 = n * t / T, i1 = n * (t + 1) / T;
        buf[(size_t)t].resize((size_t)(i1 - i0) * 32 + 64);
        len[(size_t)t] = format_fixed8_range(v + i0, i1 - i0, buf[(size_t)t].data(), (int64_t)buf[(size_t)t].size(), t == T - 1);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (std::thread &x : th) x.join();
    int64_t pos = 0;
    for (int t = 0; t < T; ++t) {
        if (len[(size_t)t] < 0 || pos + len[(size_t)t] > cap) return -1;
        memcpy(out + pos, buf[(size_t)t].data(), (size_t)len[(size_t)t]);
        pos += len[(size_t)t];
    }
    return pos;
}

#include "host_rng.h"

int gh_profile_enable(gh_ctx *c, int enable)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (enable && c->ev.empty()) {
        c->ev.resize(8192);
        for (auto &e : c->ev) HIPCHK(c, hipEventCreate(&e));
        c->ev_bytes.assign(c->ev.size() / 2, 0);
    }
    for (gh_ctx *k : c->kids) TRY(gh_profile_enable(k, enable));
    c->prof = enable != 0;
    c->prof_stride = (c->ld * c->M * 8 < (int64_t)(1 << 30)) ? 16 : 1;
    c->prof_seen = 0;
    c->ev_used = 0;
    c->prof_ms_acc = 0.0;
    c->prof_launches = 0;
    c->prof_res_evals = 0;
    if (enable) {  // (the matrix-free work counters stay readable after profiling is switched off)
        c->mf_launches = 0;
        if (c->mf_stats) HIPCHK(c, hipMemsetAsync(c->mf_stats, 0, sizeof(MfStats), c->stream));
    }
    return GH_OK;
}

int gh_matrix_free_stats(gh_ctx *c, int64_t *entries, int64_t *leaves, int64_t *launches, int64_t *near_entries,
                         int64_t *near_leaves)
{
    GH_FEED_GUARD(c);
    if (c && near_entries) *near_entries = c->mf_near_on ? c->mf_near_n : 0;
    if (c && near_leaves) *near_leaves = c->mf_near_on ? c->mf_near_leaves : 0;
    if (!c) return GH_ERR_ARG;
    TRY(need(c, c->mf && c->mf_stats, "gh_matrix_free_stats: context is not matrix-free (or not built)"));
    HIPCHK(c, hipSetDevice(c->device));
    MfStats h{};
    HIPCHK(c, hipMemcpyAsync(&h, c->mf_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (entries) *entries = (int64_t)h.entries;
    if (leaves) *leaves = (int64_t)h.leaves;
    if (launches) *launches = c->mf_launches;
    return GH_OK;
}

int gh_fold_info(const gh_ctx *c, int *on, int *reason, int64_t *store_bytes, double *max_dev, double *build_ms)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const gh_ctx::Fold &f = c->fd;
    const bool live = f.valid && f.gen == c->G_gen;
    if (on) *on = live ? 1 : 0;
    if (reason) *reason = (f.detected == 1 && f.gen != c->G_gen && f.reason == GH_FOLD_ON) ? GH_FOLD_UNDECIDED : f.reason;
    if (store_bytes) *store_bytes = f.S ? fold_store_bytes(c) : 0;
    if (max_dev) *max_dev = f.max_dev;
    if (build_ms) *build_ms = f.build_ms;
    return GH_OK;
}

int gh_fold_pair_info(const gh_ctx *c, int *on, int *reason, int64_t *pairs, int64_t *single_orbits, int64_t *bytes_per_sweep)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    const gh_ctx::Fold &f = c->fd;
    const bool live = f.valid && f.gen == c->G_gen;
    const bool pair = live && f.pair_on;
    if (on) *on = pair ? 1 : 0;
    if (reason) *reason = (f.pair_detected && !live && f.pair_reason == GH_FOLD_PAIR_ON) ? GH_FOLD_PAIR_UNDECIDED : f.pair_reason;
    if (pairs) *pairs = pair ? f.n_pairs : 0;
    if (single_orbits) *single_orbits = pair ? f.n_work - f.n_pairs : 0;
    if (bytes_per_sweep) *bytes_per_sweep = live ? fold_sweep_bytes(c) : 0;
    return GH_OK;
}

int gh_fold_detect_pair(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                        int *obs_tau, int *cell_tau, int *work, int64_t *n_work, int *pair_reason)
{
    if (N < 0 || M < 0 || !x || !y || !z || !bounds6 || !obs_tau || !cell_tau || !work || !n_work || !pair_reason)
        return GH_ERR_ARG;
    std::vector<int> oi, co, ot, ct, rt, qt, wk;
    *n_work = 0;
    *pair_reason = GH_FOLD_PAIR_NO_FOLD;
    const int rc = fold_detect_host(N, x, y, z, M, bounds6, oi, co);
    if (rc != GH_FOLD_ON) return rc;
    *pair_reason = fold_pair_detect_host(N, x, y, z, M, bounds6, oi, co, ot, ct, rt, qt, wk);
    if (*pair_reason == GH_FOLD_PAIR_ON) {
        std::copy(ot.begin(), ot.end(), obs_tau);
        std::copy(ct.begin(), ct.end(), cell_tau);
        std::copy(wk.begin(), wk.end(), work);
        *n_work = (int64_t)(wk.size() / 2);
    }
    return rc;
}

int gh_fold_pair_rows(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                      int *rows, int *pair_slots, int *code, int *ptab, int64_t *counts, int *pair_reason)
{
    if (N < 0 || M < 0 || !x || !y || !z || !bounds6 || !rows || !pair_slots || !code || !ptab || !counts || !pair_reason)
        return GH_ERR_ARG;
    std::vector<int> oi, co, ot, ct, rt, qt, wk;
    *rows = *pair_slots = 0;
    *pair_reason = GH_FOLD_PAIR_NO_FOLD;
    const int rc = fold_detect_host(N, x, y, z, M, bounds6, oi, co);
    if (rc != GH_FOLD_ON) return rc;
    *pair_reason = fold_pair_detect_host(N, x, y, z, M, bounds6, oi, co, ot, ct, rt, qt, wk);
    if (*pair_reason != GH_FOLD_PAIR_ON) return rc;
    const int nF = (int)(N / 4), ldF = (nF + 15) / 16 * 16;
    fold_detail::PairRows pr;
    if (ldF > 512 * FOLD_PAIR_MAX_ROWS || !fold_detail::pair_rows_plan(nF, ldF, oi, rt, pr)) {
        *pair_reason = GH_FOLD_PAIR_ROWS;
        return rc;
    }
    *rows = pr.rows;
    *pair_slots = pr.pair_slots;
    std::copy(pr.code.begin(), pr.code.end(), code);
    std::copy(pr.ptab.begin(), pr.ptab.end(), ptab);
    counts[0] = pr.pairs_in_slots;
    counts[1] = pr.pairs_split;
    counts[2] = pr.self_rows;
    return rc;
}

int gh_fold_detect(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                   int *obs_img, int *cell_orbit)
{
    if (N < 0 || M < 0 || !x || !y || !z || !bounds6 || !obs_img || !cell_orbit) return GH_ERR_ARG;
    std::vector<int> oi, co;
    const int rc = fold_detect_host(N, x, y, z, M, bounds6, oi, co);
    if (rc == GH_FOLD_ON) {
        std::copy(oi.begin(), oi.end(), obs_img);
        std::copy(co.begin(), co.end(), cell_orbit);
    }
    return rc;
}

int gh_profile_read(gh_ctx *c, double *sweep_ms, int64_t *sweep_launches, int64_t *bytes_per_sweep)
{
    GH_FEED_GUARD(c);
    if (!c) return GH_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // The timed launches of the DOMINANT kind only -- those that read the most bytes of G: the
    // one-read sweeps (one workgroup or a team per column, the whole matrix each) where the path has
    // them next to row-panel launches (a panel each), so that time and bytes per launch are those of
    // one kernel and agree with a kernel trace.  (An evaluation inside the resident chain kernel
    // counts as one sweep of the whole matrix.)
    const int64_t full = c->N * c->M * (int64_t)sizeof(double);
    int64_t maxb = c->prof_res_evals > 0 ? full : 0;
    for (size_t i = 0; i < c->ev_used / 2; ++i) maxb = std::max(maxb, c->ev_bytes[i]);
    double ms = (c->prof_res_evals > 0 && maxb == full) ? c->prof_ms_acc : 0.0;
    int64_t timed = (c->prof_res_evals > 0 && maxb == full) ? c->prof_res_evals : 0;
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        if (c->ev_bytes[i / 2] != maxb) continue;
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
        ms += t;
        timed += 1;
    }
    for (gh_ctx *k : c->kids) {
        // (a batch on the shift-invariant store: the timed passes of all chains -- they overlap on the GPU, the
        // sum of their durations is not wall time)
        double kms = 0.0;
        int64_t kn = 0, kb = 0;
        TRY(gh_profile_read(k, &kms, &kn, &kb));
        ms += kms;
        timed += kn;
        maxb = std::max(maxb, kb);
    }
    if (sweep_ms) *sweep_ms = ms;
    if (sweep_launches) *sweep_launches = timed;
    if (bytes_per_sweep) *bytes_per_sweep = timed > 0 ? maxb : full;
    return GH_OK;
}

}  // extern "C"

#include "host_feed.h"
