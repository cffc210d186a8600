/*
 * gravhmc.h -- C-ABI of the MI355X-native HMC gravity-inversion hot path (libgravhmc.so).
 *
 * The reference (ChuWeiEr/GravInv3DHMC) is pure Python with no FFI/plugin registry; the seam
 * its sampler uses is the duck-typed model object of inversion/hmc.py:30-32,71-83 (calls
 * `model.kernelw()` and `model.misfit_and_grad(...)`) and, one level down, the native kernels
 * `gravmag/_prism.pyx:265-290` (`_prism.gz`) and `gravmag/_tesseroid_numba.py:32-71,335`
 * (`_tesseroid_numba.gz`).  Prisms also carry the reference's other fields: the total-field magnetic
 * anomaly (`_prism.tf`, gh_set_cells_tf) and the ten other gravity fields -- potential, geoid, gx, gy and
 * the gradient tensor gxx ... gzz (`_prism.pyx:36-68, 206-509`, gh_set_cells_prism).  Tesseroids carry
 * the same ten other gravity fields (`_tesseroid_numba.py:161-341`, gh_set_cells_tess).  Several prism
 * gravity fields of one density model can share one store and be inverted together (gh_set_cells_multi; an
 * extension, the reference inverts one field at a time), on a regular grid under gridded data without a limit on the
 * rows (gh_set_cells_multi_table: one translation-invariant table per field; gh_set_cells_multi_table_chains: the
 * same tables, which also take batches of 16 chains per read, gh_batch_*).  The joint gravity-magnetic store
 * (gh_set_cells_joint) runs on that table too, as one table of block-diagonal layers (gh_set_cells_joint_table).  Every entry
 * point below names the reference interface it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: opaque context, host pointers to caller-owned contiguous float64 buffers, sizes
 *     as int64_t.  No Python / torch types.  Calls are synchronous on return.
 *   - every function returns 0 on success or a negative gh_status; the text of the last error
 *     is available from gh_last_error(ctx) (or gh_last_error(NULL) for gh_create failures).
 *   - a context is bound to one GPU and one HIP stream and is NOT thread-safe (the reference is
 *     single-threaded per chain; chains are separate processes, hmc.py:367-369).
 *   - dense matrices are column-major N x M ("Fortran order": one cell = one contiguous column
 *     of N observations), the layout the reference ends up with for Aw (potential.py:259).
 *   - there is no CPU fallback: without a usable HIP device gh_create fails.
 *
 * Environment switches read by the library (diagnostics and A/B measurements; the defaults are what
 * the tests pin and what DESIGN.md's numbers were measured with).  Part of this interface:
 *   code path, SAME arithmetic to rounding of the summation order (results agree to <= 1e-12):
 *     GRAVHMC_RESIDENT=0 (no resident chain kernel), GRAVHMC_RESIDENT_LOCAL / _REGS / _STREAM /
 *     _STREAM_MB / _CT / _WGS (its variants), GRAVHMC_TEAM=0 / GRAVHMC_TEAM_LAG (N > 16384: row panels
 *     / lag of the team sweep), GRAVHMC_EPILOGUE1=0 (two-launch epilogue), GRAVHMC_MF_FUSED=0 /
 *     GRAVHMC_MF_PIPE=0 / GRAVHMC_MF_NEAR=0 (matrix-free: two-pass form / plain build / subdivision
 *     inside the pass instead of the near-field table), GRAVHMC_MFB_FUSED=0 (matrix-free batch: two
 *     passes instead of teams), GRAVHMC_MFB_RU=0 (no one-height specialisation), GRAVHMC_BATCH_SPEC=0,
 *     GRAVHMC_BATCH_RELAYOUT=0, GRAVHMC_BATCH_TEAM=0 (stored-kernel batch: two reads of G per step with a second
 *     copy of G instead of teams reading it once), GRAVHMC_RESIDENT_BATCH=0 (chains of a batch take turns in the
 *     resident kernel instead of running in lock-step), GRAVHMC_LONSYM_HARMONIC=0 / GRAVHMC_LONSYM_FUSED=1 /
 *     GRAVHMC_LONSYM_RESIDENT=0 (shift-invariant store: direct correlations / one-launch epilogue / one launch per
 *     phase instead of the persistent launch), GRAVHMC_LONSYM_WIDE=0 / 2 (the streamed harmonic form of large grids:
 *     off / also where the register form applies), GRAVHMC_LONSYM_W, GRAVHMC_LW_WAVES_PER_CU, GRAVHMC_LW_FWD, GRAVHMC_LW_MIRROR=0 (one row of T^ per cell row),
 *     GRAVHMC_DWT_LDS / _MAX (one-launch wavelet transform);
 *   arithmetic of an entry (within the path's stated 1e-10, ~1e-14 measured): GRAVHMC_MF_EXACT -- the
 *     DEFAULT of gh_set_matrix_free_exact only; that call overrides it; GRAVHMC_FOLD=0 / GRAVHMC_FOLD_MIN_MB (the
 *     sampler's sweeps of a mirror-symmetric gz prism grid on the dense store / the size from which they fold,
 *     gh_fold_info; ~1e-11 measured); GRAVHMC_FOLD_PAIR=0 (the folded sweep reads every block instead of one per
 *     pair of orbits under the diagonal reflection, gh_fold_pair_info);
 *   diagnostics that BREAK the results (timing only): GRAVHMC_LW_BREAK (phases of lonsymw_sweep_kernel off),
 *     GRAVHMC_BT_BREAK; GRAVHMC_LW_LDS_PAD (fewer workgroups per CU, results intact);
 *   tuning without any effect on results: GRAVHMC_PF, _NT, _TW, _TW8, _WG_PER_CU, _MIN_COLS,
 *     _INFLIGHT_MB, GRAVHMC_MF_T, _MF_WG_PER_CU, GRAVHMC_MFB_WG_PER_CU, _MFB_RANGES, GRAVHMC_RNG_THREADS;
 *   test hooks (force a time-out path): GRAVHMC_TEAM_TEST_ABORT, GRAVHMC_RESIDENT_TEST_ABORT,
 *     GRAVHMC_MFB_TEST_ABORT, GRAVHMC_BATCH_TEAM_TEST_ABORT, GRAVHMC_MF_TEAM_TEST_ABORT, GRAVHMC_RESBATCH_TEST_ABORT,
 *     GRAVHMC_LONRES_TEST_ABORT; timing experiments that BREAK results: GRAVHMC_MFB_DBG, GRAVHMC_BT_BREAK, and
 *     GRAVHMC_RESIDENT_TIMING, GRAVHMC_MFB_TIMING (+ GRAVHMC_BT_DBG_MEM / _WAVE: whose), GRAVHMC_LONSYM_TIMING
 *     (per-phase clocks, results intact).
 * (Python side: GRAVHMC_HOST_RNG=numpy draws with np.random itself -- same stream; GRAVHMC_LIB = path
 * of the shared library.)
 */
#ifndef GRAVHMC_H
#define GRAVHMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_ctx gh_ctx;
typedef struct gh_rng gh_rng; /* the reference's random stream, below */

typedef enum {
    GH_OK = 0,
    GH_ERR_ARG = -1,      /* bad argument / call order (ValueError in the reference) */
    GH_ERR_HIP = -2,      /* HIP runtime error, text in gh_last_error */
    GH_ERR_NOMEM = -3,    /* device allocation failed */
    GH_ERR_OVERFLOW = -4, /* tesseroid subdivision stack > 100 entries (OverflowError,
                             _tesseroid_numba.py:53-54) */
    GH_ERR_UNSUPPORTED = -5,
    GH_ERR_COMM = -6      /* collective layer error */
} gh_status;

/* GH_CELL_PRISM_TF: prisms, total-field magnetic anomaly (set with gh_set_cells_tf, not gh_set_cells);
 * GH_CELL_PRISM_COMP: prisms, one gravity field other than gz (set with gh_set_cells_prism);
 * GH_CELL_TESSEROID_COMP: tesseroids, one gravity field other than gz (set with gh_set_cells_tess);
 * GH_CELL_PRISM_JOINT: prisms, gz and the total field inverted together (set with gh_set_cells_joint);
 * GH_CELL_PRISM_MULTI: prisms, several gravity fields of one density model inverted together (gh_set_cells_multi);
 * GH_CELL_PRISM_MVI: prisms, the total field of a magnetization VECTOR per cell (gh_set_cells_mvi);
 * GH_CELL_PRISM_MVI_DATA: prisms, a magnetization vector per cell under VECTOR data -- row blocks of tf, bx, by, bz
 * (gh_set_cells_mvi_data);
 * GH_CELL_TESS_MVI_DATA: tesseroids, a magnetization vector per cell (north, east, down at the cell's centre) under
 * row blocks of tf, bx, by, bz in the observations' local frames, on the dense store (gh_set_cells_tess_mag) or on the
 * shift-invariant table (gh_set_cells_tess_mag_table);
 * GH_CELL_TESSEROID_MULTI: tesseroids, several gravity fields of one density model inverted together, on the dense
 * store or on the shift-invariant table (gh_set_cells_tess_multi) */
enum { GH_CELL_PRISM = 0, GH_CELL_TESSEROID = 1, GH_CELL_PRISM_TF = 2, GH_CELL_PRISM_COMP = 3, GH_CELL_TESSEROID_COMP = 4,
       GH_CELL_PRISM_JOINT = 5, GH_CELL_PRISM_MULTI = 6, GH_CELL_PRISM_MVI = 7, GH_CELL_PRISM_MVI_DATA = 8 };
enum { GH_CELL_TESS_MVI_DATA = 9, GH_CELL_TESSEROID_MULTI = 10 };
/* The magnetic data components of prisms, for gh_set_cells_mvi_data and gh_b_result: the total-field anomaly along
 * the regional field, and the north, east and down components of the anomalous induction (gravmag/prism.py:665-870),
 * all in uT per A/m (CM * T2NT) */
enum { GH_BCOMP_TF = 0, GH_BCOMP_BX = 1, GH_BCOMP_BY = 2, GH_BCOMP_BZ = 3 };
/* data components a GH_CELL_PRISM_MVI_DATA context stacks at most: every GH_BCOMP_* once */
#define GH_BCOMP_MAX 4
/* components a GH_CELL_PRISM_MULTI context stacks at most: every GH_COMP_* once */
#define GH_MULTI_MAX 11
/* The gravity fields of prisms (gravmag/prism.py:875-972), for gh_set_cells_prism, and of tesseroids
 * (gravmag/tesseroid.py:324-508), for gh_set_cells_tess (gy of tesseroids: G * SI2MGAL with the
 * reference's spherical G, Gs = 6.673e-11, 1000 times smaller than the G of every other field) */
enum {
    GH_COMP_POTENTIAL = 0, /* G, per g/cm^3 (SI otherwise) */
    GH_COMP_GEOID = 1,     /* G / g0: the potential over 9.80 m/s^2, in m */
    GH_COMP_GX = 2,        /* G * SI2MGAL: mGal */
    GH_COMP_GY = 3,
    GH_COMP_GZ = 4,
    GH_COMP_GXX = 5,       /* G * SI2EOTVOS: Eotvos */
    GH_COMP_GXY = 6,
    GH_COMP_GXZ = 7,
    GH_COMP_GYY = 8,
    GH_COMP_GYZ = 9,
    GH_COMP_GZZ = 10
};
/* potential.py:827-836 `regulization` strings */
enum { GH_REG_DAMPING = 0, GH_REG_SMOOTHNESS = 1, GH_REG_MS = 2, GH_REG_TV = 3 };

/* ---- lifetime ------------------------------------------------------------------------- */

/* One inversion problem (N observations, M active cells) on GPU `device`. */
int gh_create(gh_ctx **out, int device, int64_t N, int64_t M);
void gh_destroy(gh_ctx *ctx);
const char *gh_last_error(const gh_ctx *ctx);
/* Device facts for logs/benchmarks: name (<=255 chars), CU count, total memory in bytes. */
int gh_device_info(const gh_ctx *ctx, char *name256, int *cus, int64_t *mem_bytes);

/* ---- sensitivity matrix G (the reference's `kernel` / `A`) ---------------------------- */

/* Observation points: (x, y, z) in m for prisms, (lon, lat, height) in deg/deg/m for
 * tesseroids.  Replaces the xp,yp,zp / lon,lat,height arguments of prism.gz (prism.py:911)
 * and tesseroid.gz (tesseroid.py:421). */
int gh_set_obs(gh_ctx *ctx, const double *a, const double *b, const double *c);
/* Active cells in mesh order, M x 6 row-major: x1,x2,y1,y2,z1,z2 (prism) or
 * w,e,s,n,top,bottom (tesseroid); `ratio` is the tesseroid distance-size ratio
 * (tesseroid.py:77, 1.6 for gz), ignored for prisms. */
int gh_set_cells(gh_ctx *ctx, const double *bounds6, int kind, double ratio);
/* Prisms of a total-field magnetic model (GH_CELL_PRISM_TF), M x 6 row-major x1,x2,y1,y2,z1,z2 in mesh
 * order, with the unit vector (fx, fy, fz) = dircos(inc, dec) of the regional field (utils.py:448-474).
 * Entry (i, j) is the total-field anomaly at observation i of prism j magnetized with 1 A/m along the
 * field, in uT (prism.py:665-733 with pmag = 1: CM * T2NT = 10**-7 * 10**6, constants.py:37,41).  The dense
 * assembly, the weighting, every stored-kernel path and the matrix-free passes (fused and two-pass, the
 * wavelet rows) run on it; the matrix-free batch of chains and the shift-invariant store refuse it with
 * GH_ERR_UNSUPPORTED. */
int gh_set_cells_tf(gh_ctx *ctx, const double *bounds6, double fx, double fy, double fz);
/* prism.tf's `result` on a GH_CELL_PRISM_TF context (needs gh_set_obs / gh_set_cells_tf, not G):
 * mag3 is the magnetization (mx, my, mz) in A/m of each of the M cells, M x 3 row-major; result[N]
 * in uT, accumulated corner by corner, cell by cell in mesh order into one sum per observation and
 * scaled once, as the reference does. */
int gh_tf_result(gh_ctx *ctx, const double *mag3, double *result);
/* Magnetization vector inversion in Cartesian form (GH_CELL_PRISM_MVI; Lelievre & Oldenburg 2009): three unknowns
 * (mx, my, mz) in A/m per prism instead of one magnetization along the field, so that remanence may turn the
 * magnetization away from it.  Call on a fresh context whose M is THREE TIMES the number of prisms (bounds6:
 * M/3 x 6 row-major x1,x2,y1,y2,z1,z2 in mesh order), (fx, fy, fz) = dircos(inc, dec) of the regional field.
 * Axes: x north, y east, z down.  Model-space vectors are property-major: [mx of every cell; my; mz].
 * The kernel is A = [A_x | A_y | A_z], an ordinary dense N x M store, column-major with ld rows per column:
 *     A_a[i, c] = CM*T2NT * sum over the corners of prism c of (+-) f . (V e_a)            (column a M/3 + c)
 * the total-field anomaly in uT at point i of prism c magnetized 1 A/m along axis a -- what the reference's
 * _prism.tf accumulates into `res` for that one prism with (mx, my, mz) = e_a, in its operation order
 * (_prism.pyx:72-111; prism.tf's kernel2d does NOT depend on pmag, it is always the column for m = f).  gh_build_G
 * assembles the three blocks in ONE launch that evaluates the six second derivatives of a corner once.
 * Everything the dense single-chain path offers runs on it as on any dense store: gh_weight (column norms over
 * all M columns), gh_set_data (the mean is removed), gh_forward, gh_adjoint, gh_misfit_and_grad, gh_leapfrog,
 * gh_chain_*, gh_download_G, the posterior window.  Damping and MS act on the M entries as they are; Smoothness
 * and TV take shape3 with nz*ny*nx == M/3 and apply the stencil to each component on its own (a shape3 whose
 * product is M is GH_ERR_ARG).  gh_tf_result takes mag3 of M/3 x 3.
 * Dense, single chain only: matrix-free, the shift-invariant store, the wavelet compressor, gh_batch_*,
 * gh_shard_init*, gh_upload_G and N > 16384 return GH_ERR_UNSUPPORTED naming the magnetization-vector store; the
 * resident chain kernel and the folded store are never chosen (chains run on the fused sweep). */
int gh_set_cells_mvi(gh_ctx *ctx, const double *bounds6 /* M/3 x 6 */, double fx, double fy, double fz);
/* Magnetization vector inversion under VECTOR data (GH_CELL_PRISM_MVI_DATA): three-axis magnetometers record
 * (bx, by, bz), and the total field alone -- the projection of B on the regional direction -- cannot fix a rotated
 * (remanent) magnetization.  ncomp distinct data components comps[b] (GH_BCOMP_*) of the same M/3 prisms at the same
 * N / ncomp observation points, stacked in row blocks; the columns are gh_set_cells_mvi's [A_x | A_y | A_z]:
 *     rows [b N/ncomp, (b + 1) N/ncomp), column a M/3 + c:  component comps[b] at the block's points of prism c
 *     magnetized 1 A/m along axis a, in uT -- for bx, by, bz what the reference's _prism.bx / by / bz accumulate for
 *     that one prism with (mx, my, mz) = e_a, times CM*T2NT (_prism.pyx:114-202: bx uses the second derivatives
 *     (xx, xy, xz), by (xy, yy, yz), bz (xz, yz, zz)); a tf block is bit for bit the gh_set_cells_mvi store.
 * The context's N is the STACKED length, observation-space vectors are component-major, M = 3 x prisms and model
 * vectors are property-major.  (fx, fy, fz) is used by a tf block alone (finite in any case).  Call it on a fresh
 * context, BEFORE gh_set_obs, which then takes the N / ncomp points.  gh_build_G assembles every block in ONE launch
 * that evaluates the six second derivatives of a corner once.
 * The store is the union of two the library already has:
 *   rows as gh_set_cells_multi: gh_weight scales block b by weights[b] > 0 (Wb), takes the column norms Wm of Wb A and
 *     leaves Aw = Wb A Wm^-1; gh_set_data takes Wb [dobs_0; ...] and removes the mean of every block on its own
 *     (grav_fix must be null); the data term removes the mean per block on the prediction's side too; gh_multi_info
 *     reports the blocks (comps as GH_BCOMP_*) and their means;
 *   columns as gh_set_cells_mvi: Damping and MS act on the M entries, Smoothness and TV take shape3 with nz*ny*nx ==
 *     M/3 and apply the stencil to each component on its own, gh_set_amplitude couples the three components of a cell.
 * With comps = {GH_BCOMP_TF} and weights = {1} the call IS gh_set_cells_mvi: the context is a GH_CELL_PRISM_MVI one
 * and computes exactly what that call's context computes (one block, one mean; gh_multi_info then refuses).
 * Dense, single chain only, on the fused sweep with the per-block means: matrix-free, the shift-invariant store, the
 * wavelet compressor, gh_batch_*, gh_shard_init*, gh_upload_G and a stacked N > 16384 return GH_ERR_UNSUPPORTED naming
 * the vector-data magnetization store; the resident chain kernel and the folded store are never chosen.
 * Errors: GH_ERR_ARG for ncomp outside 1..GH_BCOMP_MAX, an unknown or repeated component, a weight that is not
 * finite and > 0, M not a multiple of 3, N not a multiple of ncomp, a context that is not fresh. */
int gh_set_cells_mvi_data(gh_ctx *ctx, const double *bounds6 /* M/3 x 6 */, double fx, double fy, double fz, int ncomp,
                          const int *comps, const double *weights);
/* prism._bx / _by / _bz's `res` on a GH_CELL_PRISM_MVI or GH_CELL_PRISM_MVI_DATA context (needs gh_set_obs and the
 * cells, not G): component is GH_BCOMP_BX, _BY or _BZ (the total field: gh_tf_result), mag3 the magnetization
 * (mx, my, mz) in A/m of each of the M/3 prisms, row-major; result (one value per observation POINT: N / ncomp)
 * in uT, accumulated corner by corner, cell by cell in mesh order into one sum per observation and scaled once, as
 * the reference does (prism.py:735-870). */
int gh_b_result(gh_ctx *ctx, int component, const double *mag3 /* M/3 x 3 */, double *result);
/* The magnetic fields of TESSEROIDS (GH_CELL_TESS_MVI_DATA): the spherical form of gh_set_cells_mvi_data.  Frames: at
 * longitude lam and latitude phi the ECEF unit vectors are n = (-sin phi cos lam, -sin phi sin lam, cos phi) (north),
 * e = (-sin lam, cos lam, 0) (east), u = (cos phi cos lam, cos phi sin lam, sin phi) (up).  Cell c carries the
 * magnetization m_c = (m_N, m_E, m_D) in A/m in the north-east-down frame at its CENTRE (the midpoints of its lon / lat
 * bounds), uniform over the cell in the Cartesian sense (sub-tesseroids of the subdivision keep the vector and the
 * frame).  With V_ab(o, c) the unscaled second-derivative sums of the gradient tensor (gh_set_cells_tess with
 * GH_COMP_GXX .. GH_COMP_GZZ, before their scale; observation frame x north, y east, z up; the same subdivision rule,
 * stack and error codes at `ratio`) and Q(o, c) = [n_o e_o u_o]^T [n_c e_c -u_c],
 *     (B_x, B_y, B_zup) = CM T2NT V(o, c) Q(o, c) m_c,    bx = B_x (north), by = B_y (east), bz = -B_zup (down)
 * in uT, at the observation; tf = f_o . (bx, by, bz) with the unit vector f_o = fdir[3 o ..] given PER OBSERVATION
 * point (a global survey has no single regional direction).  The store is [K_N | K_E | K_D]:
 *     rows [b N/ncomp, (b + 1) N/ncomp), column a M/3 + c:  component comps[b] at the block's points of tesseroid c
 *     magnetized 1 A/m along its axis a (north, east, down).
 * bounds6: M/3 x 6 (w, e, s, n in degrees, top, bottom in m; w <= e, s <= n, top >= bottom, else GH_ERR_ARG); ratio > 0
 * (the reference's RATIO_GG = 8 for second derivatives); fdir: N/ncomp x 3, needed only with a GH_BCOMP_TF block, else
 * it may be NULL.  Call it on a fresh context, BEFORE gh_set_obs, which then takes the N / ncomp points (lon, lat in
 * degrees, height in m).  gh_build_G assembles every block in ONE launch that walks the adaptive subdivision once per
 * (point, cell) pair and accumulates the six sums at every leaf; gh_kernel_stats reports its warn_cells and leaves,
 * a full stack is GH_ERR_OVERFLOW.
 * In everything but the assembly the context is a GH_CELL_PRISM_MVI_DATA one, always with its block table (a single
 * unweighted tf block too): gh_weight with block weights, gh_set_data with per-block means, forward / adjoint,
 * gh_misfit_and_grad, gh_leapfrog and gh_chain_* on the fused sweep, gh_set_amplitude, gh_multi_info, Smoothness / TV
 * per component on shape3 with product M/3, the posterior window and stream.
 * Single chain only, dense or on the shift-invariant table (below): matrix-free without the table, the wavelet
 * compressor, gh_batch_*, gh_shard_init*, gh_upload_G and, on the dense form, a stacked N > 16384 return
 * GH_ERR_UNSUPPORTED naming the tesseroid magnetization store; the resident chain kernel and the folded store are never
 * chosen.  A context already asked onto the table (gh_set_shift_invariant BEFORE this call) is refused: its kind is not
 * known yet; ask after this call, or use gh_set_cells_tess_mag_table.
 * Errors: GH_ERR_ARG for ncomp outside 1..GH_BCOMP_MAX, an unknown or repeated component, a weight that is not
 * finite and > 0, M not a multiple of 3, N not a multiple of ncomp, a tf block without fdir, a context that is not
 * fresh. */
int gh_set_cells_tess_mag(gh_ctx *ctx, const double *bounds6 /* M/3 x 6 */, double ratio, int ncomp, const int *comps,
                          const double *weights, const double *fdir /* N/ncomp x 3, or NULL */);
/* The same context on the SHIFT-INVARIANT TABLE: gh_set_cells_tess_mag followed by gh_set_shift_invariant(ctx, 1), in
 * one call and without the limit on the stacked rows (G is never stored).  gh_set_shift_invariant(ctx, 1) between
 * gh_set_cells_tess_mag and gh_build_G does the same for N <= 16384.  On the geometry that store asks for -- the M/3
 * cells in rows of n cells that cover the full circle of longitudes, observation longitudes on the cells' spacing --
 *   the data block is one more coordinate of the observation class, as on a GH_CELL_TESSEROID_MULTI context: a class is
 *   (block b, latitude, height), na = ncomp na1 classes;
 *   the axis block is a coordinate of the table's cell row: column a M/3 + r n + k of the property-major model is cell
 *   row a nc1 + r (nc1 = M / 3 / n), longitude k, of a table of nc = 3 nc1 rows, so j = c n + k addresses the model as
 *   it is;  T[(a nc1 + r) ldT + (b na1 + cls) n + d] is the entry of shift d.  Both frames turn with a common shift of the
 *   longitudes, so every (component, axis) pair depends on lon_i - lon_j alone.
 *   gh_build_G fills the table in ONE launch of the dense assembly's body over the na1 n synthetic points and the nc1
 *   cells of longitude index 0 -- one traversal of the subdivision per (point, cell), every entry times weights[b] --
 *   and agrees with the dense store to 1e-10 of a block's largest entry; warn_cells (n per cell of longitude index 0,
 *   once per cell whatever the axis), leaves and GH_ERR_OVERFLOW as the table of gz reports them.
 *   Only the streamed harmonic form serves this kind (gh_shift_invariant_harmonic: 2; n < 2 or n > 1024 refused), with
 *   the same four plain launches per step.  On a grid symmetric about the equator a row of the transformed table stands
 *   for a mirrored pair of cell rows; local north flips at both ends of the reflection, east and down do not, so the
 *   entry of the partner is s_b s_a K with s_b = -1 for GH_BCOMP_BX and s_a = -1 for the axis N, +1 otherwise: a sign
 *   per class times a sign per table row (GRAVHMC_LW_MIRROR=0: no pairing).  With a GH_BCOMP_TF block the table is
 *   built WITHOUT the mirror (the projection on f_o is no pure sign under it), and fdir must be equal, bit for bit,
 *   over every class of observations (same latitude and height), else GH_ERR_UNSUPPORTED ("the total field's direction
 *   varies within a class of observations").
 *   gh_weight gives the dense store's Wm (column norms of Wb A over all M columns) from the table; the means are
 *   removed per block, from the classes' sums in index order; gh_multi_info, gh_set_amplitude and the regularisers
 *   (per property, with Phi's slot in chains) are the dense store's, evaluated by the same launches.
 * Refused with GH_ERR_UNSUPPORTED and the reason, each naming the tesseroid magnetization store: a geometry without the
 * structure (carved or irregular cells, observation longitudes off the spacing), the wavelet compressor, gh_batch_*,
 * gh_bscg_run, gh_shard_init*, gh_upload_G, gh_set_matrix_free.  The prism forms (GH_CELL_PRISM_MVI,
 * GH_CELL_PRISM_MVI_DATA) have no table. */
int gh_set_cells_tess_mag_table(gh_ctx *ctx, const double *bounds6 /* M/3 x 6 */, double ratio, int ncomp,
                                const int *comps, const double *weights, const double *fdir /* N/ncomp x 3, or NULL */);
/* The field of a GH_CELL_TESS_MVI_DATA context without a store (needs gh_set_obs and the cells, not G): component is a
 * GH_BCOMP_* value (GH_BCOMP_TF needs the context's fdir), mag3 the vector (m_N, m_E, m_D) in A/m of each of the M/3
 * tesseroids, row-major; result (one value per observation POINT: N / ncomp) in uT.  One workgroup per point sums the
 * cells' fields in a fixed order and scales once.  gh_kernel_stats then reports this pass's warn_cells and leaves. */
int gh_tess_b_result(gh_ctx *ctx, int component, const double *mag3 /* M/3 x 3 */, double *result);
/* Amplitude coupling of a weighted GH_CELL_PRISM_MVI context: the minimum-support functional of the cells'
 * amplitude, the one term that ties the three components of a cell together (compact bodies).  With
 *     u_a[c] = mw[a M/3 + c] winv[a M/3 + c] / scale   (winv = 1 / Wm, 0 where Wm is 0),   s_c = sum_a u_a[c]^2,
 *     Phi = sum_c s_c / (s_c + beta),      dPhi/dmw[a M/3 + c] = 2 beta u_a[c] / (s_c + beta)^2 * winv / scale.
 * With lambda > 0 every potential evaluation of the context -- gh_misfit_and_grad, gh_leapfrog, gh_chain_* --
 * becomes U = U_data + alpha R + lambda Phi, grad likewise; the reported U_model stays R (out3[2], out5[2]) and
 * Phi is read with gh_amplitude_last.  One more kernel launch per evaluation, behind the regulariser's; sums in
 * a fixed order.  lambda = 0 switches the term off: the context then launches and returns exactly what it did
 * before the call.  A running chain must be started again (gh_chain_init).  The term keeps winv / scale; a
 * gh_weight after a new gh_build_G builds it again from the new weights, lambda, beta and scale staying.
 * Errors: GH_ERR_UNSUPPORTED on any other store; GH_ERR_ARG before gh_weight, for lambda < 0, beta <= 0 or
 * scale <= 0. */
int gh_set_amplitude(gh_ctx *ctx, double lambda, double beta, double scale);
/* The term alone at mw (M entries), lambda = 1, with beta and scale of the last gh_set_amplitude (whatever its
 * lambda): *value = Phi, grad (M, or NULL) = dPhi/dmw, amp (M/3, or NULL) = the cells' physical amplitudes
 * scale * sqrt(s_c) = |(mx, my, mz)_c|. */
int gh_amplitude_eval(gh_ctx *ctx, const double *mw, double *value, double *grad /* M or NULL */,
                      double *amp /* M/3 or NULL */);
/* Phi of the last gh_misfit_and_grad, or of the state the chain was left in by the last gh_chain_init /
 * trajectory (as out5[0..2]); 0 while the coupling is off. */
int gh_amplitude_last(const gh_ctx *ctx, double *phi);
/* Joint gravity-magnetic inversion (GH_CELL_PRISM_JOINT, inversion/potential.py:847-1812): the density and
 * the magnetization of the same M/2 prisms (bounds6: M/2 x 6 row-major x1,x2,y1,y2,z1,z2 in mesh order)
 * under the same N/2 observation points.  The kernel is block-diagonal, A = [[A_gz, 0], [0, A_tf]] (N x M;
 * the tf block along (fx, fy, fz) as gh_set_cells_tf), but the device stores H = [A_gz | A_tf] only: N/2
 * rows (padded as G) by M columns, the gz block in columns [0, M/2).  Every vector of the interface keeps
 * the stacked shape: observation-space vectors have N entries (gz first), model-space vectors M.
 * N and M must be even.  Call it on a fresh context, BEFORE gh_set_obs, which then takes the N/2 points.
 *   gh_build_G   assembles both blocks in one launch, entry for entry the bits of a gz and a tf context.
 *   gh_weight    (weightfactor 0.5 only) takes the column norms Wm of the unbalanced A, the population
 *                standard deviations std_gz, std_tf of the two unweighted blocks (gh_joint_std), and
 *                leaves Aw = Wb A Wm^-1 with Wb = diag(1 (N/2 times), s (N/2 times)), s = std_gz / std_tf,
 *                folded into the stored tf block.
 *   gh_set_data  takes dobs = dobsw = Wb [dobs_gz; dobs_tf] (N entries) and NO mean is removed; grav_fix
 *                must be null.  The data term is |Aw mw - dobsw|^2 (potential.py:1665-1680).
 *   gh_set_reg / gh_reg_eval: Smoothness and TV take shape3 with nz*ny*nx == M/2 and apply the stencil to
 *                each property on its own (the block-diagonal fd3djoint, potential.py:1075): the regulariser
 *                does not couple the two blocks.
 *   gh_set_cross_gradient adds the one term that does: lambda |grad rho x grad kappa|^2 (off by default).
 * Dense, single chain only: matrix-free, the shift-invariant store, the wavelet compressor, gh_batch_*,
 * gh_shard_init*, gh_upload_G and N/2 > 16384 return GH_ERR_UNSUPPORTED; the resident chain kernel is
 * never chosen (chains run on the fused sweep). */
int gh_set_cells_joint(gh_ctx *ctx, const double *bounds6, double fx, double fy, double fz);
/* The same store on the translation-invariant table (csrc/latjoint.hip.h; gh_set_translation_invariant below has the
 * geometry the table needs): the arguments, the checks -- but the limit on N/2, the table has no rows -- and the context
 * of gh_set_cells_joint, whose name the refusals keep.  gh_build_G then detects the structure on the M/2 cells and N/2
 * points (GH_ERR_UNSUPPORTED naming the joint store on the translation-invariant table, with the reason, where it is
 * absent) and fills ONE table of 2 nz layers, T[2][nz][nx + px - 1][ny + qy - 1]: T[0], bit for bit, the table a
 * gh_set_cells_prism (gz) context builds under gh_set_translation_invariant(ctx, 1) on the geometry, T[1] that of a
 * gh_set_cells_tf context; max_dev is the larger of the two tables' (each against its own largest entry).  The store
 * is block-diagonal: layer b nz + k meets the observation block b alone, in both passes (lat_pass_kernel's
 * block-diagonal form) -- the forward's chunks of layers are cut per property, gh_translation_invariant_axes reports
 * axes = 2, the chunks (half of them each property's) and the layers per chunk.  gh_weight takes Wm from the tables'
 * windows and std_gz, std_tf from their entries weighted by the pairs that share an offset, and from then on the passes
 * multiply the tf block by s = std_gz / std_tf where the dense store has it folded in; gh_set_data, gh_set_reg,
 * gh_set_cross_gradient, gh_forward, gh_adjoint, gh_misfit_and_grad and the single chain (gh_chain_*, the posterior
 * stream) work as on the dense store and agree with it to 1e-10, the bound the suites test.  Refused as on the dense store, and gh_download_G
 * (nothing is stored), gh_set_translation_invariant (the table is this context's form), gh_bscg_run. */
int gh_set_cells_joint_table(gh_ctx *ctx, const double *bounds6, double fx, double fy, double fz);
/* std_gz, std_tf of the unweighted blocks of a weighted GH_CELL_PRISM_JOINT context (numpy.std, ddof 0,
 * over the (N/2) (M/2) entries of each block; two passes on the device) */
int gh_joint_std(const gh_ctx *ctx, double std2[2]);
/* How a GH_CELL_PRISM_JOINT context runs a potential evaluation: the sweep's workgroups per block (each writes
 * one slab row of its block's partial forward product) and the epilogue's stages per block (1: reduce_finish_kernel
 * over the slab rows; 2: below 2048 rows with more than 64 slab rows per block, reduce_reg_kernel folds them into
 * segments first) */
int gh_joint_layout(const gh_ctx *ctx, int *workgroups_per_block, int *epilogue_stages);
/* Several gravity fields of ONE density model inverted together (GH_CELL_PRISM_MULTI): ncomp distinct components
 * comps[b] (GH_COMP_*) of the same M prisms at the same N / ncomp observation points, stacked in row blocks of one
 * dense store: rows [b N/ncomp, (b + 1) N/ncomp) of A hold component b, entry for entry the bits of a
 * gh_set_cells_prism context of that component, in its own units.  The context's N is the stacked length;
 * observation-space vectors are component-major.  weights[b] > 0 is the data weighting of block b.  Call it on a
 * fresh context, BEFORE gh_set_obs, which then takes the N / ncomp points.
 *   gh_build_G   runs the component's assembly kernel once per block into the one store.
 *   gh_weight    scales block b by weights[b] (Wb), takes the column norms Wm of Wb A -- not of A, where the
 *                component with the largest unit would decide them -- and leaves Aw = Wb A Wm^-1.
 *   gh_set_data  takes dobs = Wb [dobs_0; ...; dobs_{ncomp-1}] (N entries) and removes the mean of every block
 *                on its own; grav_fix must be null.
 *   The data term removes the mean per block on the prediction's side too: with d = Aw mw,
 *                r_b = (d_b - mean d_b) - (dobs_b - mean dobs_b),  U_data = sum_b |r_b|^2,  grad = 2 Aw^T r
 *                (one mean over rows that mix units would be meaningless).  The regularisers act on the M cells.
 *   With ncomp = 1 and weights[0] = 1 the context computes what a gh_set_cells_prism context computes.
 * It runs on the fused sweep: N (the stacked length) > 16384 is refused with GH_ERR_UNSUPPORTED, as are
 * matrix-free, the shift-invariant store, the wavelet compressor, gh_batch_*, gh_shard_init* and gh_upload_G; the
 * resident chain kernel and the folded store are never chosen. */
int gh_set_cells_multi(gh_ctx *ctx, const double *bounds6, int ncomp, const int *comps, const double *weights);
/* gh_set_cells_multi and the request for the translation-invariant table (below) in one call: the same checks but the
 * limit of 16384 stacked rows, which the table does not have.  gh_build_G then looks for the structure on the
 * N / ncomp points (GH_ERR_UNSUPPORTED with the reason where it is absent) and keeps ncomp tables
 * T[b][k][u][v], block-major, each entry the unweighted entry of the dense multi-component store bit for bit, each
 * block with a max_dev of its own (the largest is reported and checked).  The data weights are not in the tables:
 * from gh_weight on the adjoint reads w_b r and the forward multiplies its finished sums by w_b; the column norms are
 * (sum_b w_b^2 sum T_b^2)^weightfactor.  One launch per pass: the adjoint runs the blocks in turn into the same
 * accumulators before the one cell update (order of the sums: block, input row, input), the forward takes the block as
 * a grid coordinate under one gather of x.  gh_multi_info, gh_set_data and the per-block means of the data term are
 * those of gh_set_cells_multi.  This call is the only way onto the table: gh_set_cells_multi with
 * gh_set_translation_invariant, in either order, stays refused, and gh_set_translation_invariant on such a context is
 * refused too.  gh_compress_wavelet, gh_batch_*, gh_bscg_run, gh_shard_init*, gh_upload_G, gh_set_matrix_free,
 * gh_set_shift_invariant and a grav_fix return an error naming the store; gh_download_G has no kernel to return.  With
 * ncomp = 1 and weights[0] = 1 the context computes what a gh_set_cells_prism context on the table computes. */
int gh_set_cells_multi_table(gh_ctx *ctx, const double *bounds6, int ncomp, const int *comps, const double *weights);
/* gh_set_cells_multi_table, and the table of blocks also takes chain batches: the same checks, tables, single-chain
 * passes (gh_chain_*, gh_misfit_and_grad, gh_forward, gh_adjoint run exactly as on a gh_set_cells_multi_table context)
 * and refusals, except that gh_batch_init, gh_batch_trajectory and gh_batch_run run on it -- always as the fp64-MFMA
 * batch, never inside the resident kernels -- on the row-block forms of the table's batch passes (csrc/latbatch.hip.h):
 * the forward takes the block as a grid coordinate under one gather of X and multiplies its sums by w_b, the adjoint
 * runs the input rows of block 0, 1, ... into the same MFMA accumulators before the one update per (cell, chain), and
 * the evaluation removes one mean per block and chain (csrc/batch.hip.h: batch_finish_blocks_kernel).  Order of the
 * sums: blocks, input rows, inputs ascending; a chain's result does not depend on the other slots.  With ncomp = 1 and
 * weights[0] = 1 the batch computes, bit for bit, what the batch of a gh_set_translation_invariant(ctx, 2) context of
 * that field computes.  gh_translation_invariant_batch_plan reports the plan (the forward's chunks are planned for
 * ncomp workgroups per chunk and tile), gh_batch_block_means the blocks' means.  An extent along y the batch tile
 * cannot hold is refused by gh_batch_init as in mode 2 (the tile is the single block's: the blocks take turns in it);
 * gh_compress_wavelet, gh_upload_G, gh_bscg_run, gh_shard_init*, gh_set_matrix_free and gh_set_shift_invariant return an
 * error naming the translation-invariant store; gh_set_translation_invariant stays refused. */
int gh_set_cells_multi_table_chains(gh_ctx *ctx, const double *bounds6, int ncomp, const int *comps, const double *weights);
/* gh_set_cells_mvi_data, and the store is built on the translation-invariant table (csrc/latmvi.hip.h) instead of as
 * ld x M doubles: the same arguments, checks and context -- columns [A_x | A_y | A_z] of the M / 3 cells, rows in ncomp
 * blocks of data components, model vectors property-major, the regularisers on three properties, gh_set_amplitude,
 * gh_amplitude_eval, gh_b_result, gh_tf_result (the unweighted tf block alone), gh_multi_info -- without the 16384-row
 * limit.  The axis of a column is one more layer coordinate of the table: layer L = ax nz + k of 3 nz, T[b][L][u][v]
 * the field of data block b of a unit magnetization along ax, every entry the dense store's entry of its pair bit for
 * bit; the passes of gh_set_cells_multi_table run on it unchanged.  gh_build_G looks for the structure on the M / 3
 * cells under the N / ncomp points (GH_ERR_UNSUPPORTED with the reason where it is absent).  One unweighted tf block
 * stays a store of one block with one mean here: it agrees with the gh_set_cells_mvi context to rounding, not bit for
 * bit.  This call is the only way onto the table: gh_set_cells_mvi and gh_set_cells_mvi_data refuse a context with
 * the table switched on, gh_set_translation_invariant refuses a magnetization-vector context.  gh_batch_*,
 * gh_bscg_run, gh_compress_wavelet, gh_shard_init*, gh_upload_G, gh_set_matrix_free, gh_set_shift_invariant and a
 * grav_fix return GH_ERR_UNSUPPORTED naming the vector-data magnetization store and the translation-invariant table;
 * gh_download_G has no kernel to return. */
int gh_set_cells_mvi_table(gh_ctx *ctx, const double *bounds6, double fx, double fy, double fz, int ncomp, const int *comps,
                           const double *weights);
/* The means of the row blocks of the chains' CURRENT predictions Aw mw, pred_mean[chain * ncomp + b] for the C chains of
 * the batch, as the batch's evaluation removes them.  A batch on a gh_set_cells_multi_table_chains context only
 * (GH_ERR_UNSUPPORTED otherwise). */
int gh_batch_block_means(gh_ctx *ctx, double *pred_mean);
/* Several gravity fields of ONE density model of TESSEROIDS inverted together (GH_CELL_TESSEROID_MULTI): the spherical
 * form of gh_set_cells_multi -- satellite gradiometry, gzz, gxx, gyy, gxz ... measured together at orbit height.
 * ncomp distinct components comps[b] (GH_COMP_*, gz included) of the same M tesseroids (w,e,s,n,top,bottom) at the same
 * N / ncomp observation points, component b assembled at the distance-size ratio ratios[b] > 0 and weighted by
 * weights[b] > 0.  The contract is gh_set_cells_multi's: the context's N is the stacked length, observation-space
 * vectors are component-major; call it on a fresh context, BEFORE gh_set_obs, which then takes the N / ncomp points.
 * Errors: those of gh_set_cells_multi and of gh_set_cells_tess (GH_ERR_ARG for a ratio <= 0 or a cell without w <= e,
 * s <= n, top >= bottom).
 * The dense store (the default; any geometry):
 *   gh_build_G   runs the field's assembly kernel once per block into the one store: rows [b N/ncomp, (b + 1) N/ncomp)
 *                are bit for bit the rows of a gh_set_cells_tess(comps[b], ratios[b]) context (GH_COMP_GZ: the bits
 *                of kind 1).  The error cells and leaves gh_kernel_stats reports are summed over the blocks;
 *                GH_ERR_OVERFLOW as for one component.
 *   gh_weight, gh_set_data, the data term with one mean per block on both sides, gh_multi_info, the fused sweep and
 *                the limit of 16384 stacked rows: as gh_set_cells_multi.
 * The shift-invariant store (gh_set_shift_invariant(ctx, 1) before gh_build_G, before or after this call; no row limit,
 * G never stored) on the geometry that store asks for:
 *   the component block is one more coordinate of the observation class: a class is (block, latitude, height), the
 *   stacked observation b N/ncomp + i has the class of point i in block b and i's longitude slot.  One launch fills the
 *   table for all (cell row, class, shift), every entry by its class's field at its class's ratio, scaled as
 *   gh_set_cells_tess scales it and times weights[b]; it agrees with the dense store to 1e-10 of a block's largest
 *   entry.  Only the streamed harmonic form serves this kind, one launch per phase, whatever the environment switches
 *   say (gh_shift_invariant_harmonic: 2); more than 1024 or fewer than 2 longitudes per cell row are refused.  On a
 *   grid symmetric about the equator a row of the transformed table stands for a mirrored pair of cell rows, and the
 *   entry of the partner is the sign of the class times the entry: -1 for gx, gxy, gxz (the observation's north axis
 *   flips), +1 for the potential, geoid, gy, gz, gxx, gyy, gyz, gzz (GRAVHMC_LW_MIRROR=0: no pairing).  The means are
 *   removed per block, from the classes' sums in index order; gh_weight gives the dense store's Wm (column norms of
 *   Wb A) from the table; gh_multi_info as on the dense store.
 * With comps = {GH_COMP_GZ} and weights = {1} the call IS gh_set_cells(kind 1, ratios[0]): the context is a
 * GH_CELL_TESSEROID one and computes exactly what that call's context computes (one block, one mean; gh_multi_info then
 * refuses), on the dense store and on the table.
 * Refused with GH_ERR_UNSUPPORTED, each naming the tesseroid multi-component store: matrix-free without the table,
 * the wavelet compressor, gh_batch_*, gh_bscg_run, gh_shard_init*, gh_upload_G; grav_fix must be null; the resident
 * chain kernel, the folded store and the persistent harmonic pass are never chosen. */
int gh_set_cells_tess_multi(gh_ctx *ctx, const double *bounds6, int ncomp, const int *comps, const double *ratios,
                            const double *weights);
/* The blocks of a GH_CELL_PRISM_MULTI, GH_CELL_TESSEROID_MULTI or GH_CELL_PRISM_MVI_DATA context (comps: GH_COMP_* or GH_BCOMP_* values; every
 * pointer may be null; arrays of GH_MULTI_MAX hold them):
 * their number, components and weights, the mean of each block of the LAST evaluation's prediction Aw mw
 * (gh_misfit_and_grad, or the chain's last step; zeros before the first), and the mean gh_set_data removed from
 * each block of the weighted observations. */
int gh_multi_info(gh_ctx *ctx, int *ncomp, int *comps, double *weights, double *pred_mean, double *obs_mean);
/* Cross-gradient structural coupling of a weighted GH_CELL_PRISM_JOINT context (Gallardo & Meju 2003; the
 * reference's JointModule.CrossGradient, potential.py:1558, is an empty method).  With shape3 = (nz, ny, nx),
 * nz*ny*nx == M/2, x fastest (p = (k ny + j) nx + i), the physical, normalised models are
 *     u[p] = mw[p] winv[p] / scale2[0],   w[p] = mw[M/2 + p] winv[M/2 + p] / scale2[1]
 * (winv = 1 / Wm, 0 where Wm is 0; no prior model is subtracted).  At the cells with i < nx-1, j < ny-1, k < nz-1
 *     Du = ((u[p+1] - u[p]) / hx, (u[p+nx] - u[p]) / hy, (u[p+nx ny] - u[p]) / hz[k]),  Dw likewise,
 *     t = Du x Dw,   Phi = sum_p |t_p|^2
 * and every other cell contributes nothing.  hz has nz-1 entries: the distance between the centres of layers k
 * and k+1.  The spacings are taken as given, in any unit (JointModule passes them relative to the smallest).
 * With lambda > 0 every potential evaluation of the context -- gh_misfit_and_grad, gh_leapfrog, gh_chain_* --
 * becomes U = U_data + alpha R + lambda Phi, grad likewise; the reported U_model stays R (out3[2], out5[2]) and
 * Phi is read with gh_cross_gradient_last.  One more kernel launch per evaluation, behind the regulariser's;
 * sums in a fixed order.  lambda = 0 switches the term off: the context then launches and returns exactly
 * what it did before the call.  A running chain must be started again (gh_chain_init).
 * Errors: GH_ERR_UNSUPPORTED on a context that is not a joint store; GH_ERR_ARG before gh_weight, for a shape whose
 * product is not M/2 or with an extent below 2, lambda < 0, a normaliser <= 0 or a spacing <= 0. */
int gh_set_cross_gradient(gh_ctx *ctx, double lambda, const double scale2[2], const int shape3[3], double hx,
                          double hy, const double *hz /* nz-1 */);
/* The term alone at mw (M entries), lambda = 1, with the shape, spacings and normalisers of the last
 * gh_set_cross_gradient (whatever its lambda): *value = Phi, grad (M, or NULL) = dPhi/dmw, t (3 M/2, or NULL) =
 * the vectors t_p, cell-major, zero at the cells that do not contribute. */
int gh_cross_gradient_eval(gh_ctx *ctx, const double *mw, double *value, double *grad, double *t);
/* Phi of the last gh_misfit_and_grad, or of the state the chain was left in by the last gh_chain_init /
 * trajectory (as out5[0..2]); 0 while the coupling is off. */
int gh_cross_gradient_last(const gh_ctx *ctx, double *phi);
/* The instantiation and column partition configure_sweep chose in gh_create for the dense fused sweep (read only;
 * the fields of a matrix-free context are not used by it): sweep_kernel's team width tw (waves per team: 1, 4,
 * 8, 16), ept2 (double2 per thread holding a column), pf (columns in flight beyond the one being reduced), nt
 * (non-temporal loads of G), n_teams and cols_per_team (the column partition; a joint store's n_teams counts
 * the teams of both blocks), grid (workgroups of one launch) and n_panels (row panels; > 1 beyond 16384 rows).
 * Any pointer may be NULL. */
int gh_sweep_layout(const gh_ctx *ctx, int *tw, int *ept2, int *pf, int *nt, int *n_teams, int64_t *cols_per_team,
                    int *grid, int *n_panels);
/* Prisms of a density model for one gravity field `component` (GH_COMP_*), M x 6 row-major
 * x1,x2,y1,y2,z1,z2 in mesh order.  Entry (i, j) is the field at observation i of prism j with a density
 * of 1 g/cm^3, scaled as prism.py scales kernel2d: G for the potential, G/g0 for the geoid, G*SI2MGAL for
 * gx / gy / gz, G*SI2EOTVOS for the tensor (constants.py).  GH_COMP_GZ makes a GH_CELL_PRISM context, the
 * same bits as gh_set_cells(kind 0); every other component a GH_CELL_PRISM_COMP one.  gxy, gxz and gyz
 * keep the reference's perturbed distance on the line of a vertical / horizontal edge
 * (_prism.pyx:346-351, 380-385, 443-448), so their entries there are large but finite.  The dense
 * assembly, the weighting, every stored-kernel path and the matrix-free passes (fused and two-pass, the
 * wavelet rows) run on it; the matrix-free batch of chains and the shift-invariant store refuse it with
 * GH_ERR_UNSUPPORTED. */
int gh_set_cells_prism(gh_ctx *ctx, const double *bounds6, int component);
/* prism.<component>'s `result` on a GH_CELL_PRISM or GH_CELL_PRISM_COMP context (needs gh_set_obs /
 * gh_set_cells_prism, not G): dens[M] in g/cm^3; result[N] accumulated corner by corner, cell by cell in
 * mesh order into one sum per observation and scaled once, as the reference does.  Unsharded contexts
 * only (GH_ERR_UNSUPPORTED otherwise). */
int gh_prism_result(gh_ctx *ctx, const double *dens, double *result);
/* Tesseroids of a density model for one gravity field `component` (GH_COMP_*), M x 6 row-major
 * w,e,s,n,top,bottom in mesh order, ratio > 0 the distance-size ratio of the adaptive subdivision
 * (tesseroid.py: RATIO_V = 1 for the potential and geoid, RATIO_G = 1.6 for gx / gy / gz, RATIO_GG = 8
 * for the tensor).  Every cell must have w <= e, s <= n, top >= bottom (GH_ERR_ARG otherwise).  Entry (i, j) is _tesseroid_numba.<field>'s kernel2d entry scaled as tesseroid.py
 * scales it: G for the potential, G/g0 for the geoid, G*SI2MGAL for gx, Gs*SI2MGAL for gy (the
 * reference's spherical constant), G*SI2EOTVOS for the tensor.  GH_COMP_GZ makes a GH_CELL_TESSEROID
 * context, the same bits as gh_set_cells(kind 1); every other component a GH_CELL_TESSEROID_COMP one.
 * gh_build_G reports the error-code cells and leaves as for kind 1 and GH_ERR_OVERFLOW when the
 * 100-entry subdivision stack overflows, on a matrix-free context too (one extra pass over the pairs
 * that stores nothing).  Every stored-kernel path and the matrix-free two-pass form run on it; the
 * shift-invariant store, the matrix-free batch of chains and gh_prism_result refuse it with
 * GH_ERR_UNSUPPORTED. */
int gh_set_cells_tess(gh_ctx *ctx, const double *bounds6, int component, double ratio);
/* Matrix-free mode (call before gh_build_G): the kernel matrix is never stored; the prism /
 * tesseroid entries are re-evaluated where they are needed.  With N <= 16384 observations a
 * leapfrog step evaluates every entry ONCE (a workgroup keeps a cell's column on the chip between
 * the dot with r, the leapfrog update and the forward accumulation, like the dense sweep); beyond
 * that an adjoint pass and a forward pass evaluate it twice.  For problems whose G exceeds HBM. */
int gh_set_matrix_free(gh_ctx *ctx, int enable);
/* Arithmetic of the matrix-free tesseroid passes (call before gh_build_G; prisms: no effect).
 * exact = 0 (default): a far pair's 2x2x2 Gauss-Legendre leaf re-arranged for throughput --
 * cos(lon - lon') by the addition theorem, 1 / l^3 from the hardware reciprocal square root and one
 * Newton factor; agrees with the reference's values to ~1e-14 (stated tolerance of the path 1e-10).
 * exact = 1: the leaf in the operation order of gravmag/_tesseroid_numba.py:207-222 (same bits as the
 * dense assembly, ~3x the time).  Which pairs are far is decided by the reference's own distance /
 * size test with the same bits either way (_tesseroid_numba.py:135-157).  Without this call the
 * environment variable GRAVHMC_MF_EXACT (0 / 1) chooses, default 0. */
int gh_set_matrix_free_exact(gh_ctx *ctx, int exact);
/* Shift-invariant store for regular spherical grids (call before gh_build_G; implies that G is never
 * stored).  Where every row of tesseroid cells covers the full circle of longitudes with one spacing
 * and the observations sit on that spacing (example/global/main_global.py:25-28: 3-degree mesh under a
 * 3-degree observation grid) the entry of (observation i, cell (row c, longitude k)) depends on the two
 * longitudes through their difference only (gravmag/_tesseroid_numba.py:207-222: cos(lon - lon')):
 * K[i, (c, k)] = T[c][class of (lat_i, h_i)][(m_i - k) mod n].  gh_build_G then evaluates the table T
 * once with the reference's adaptive engine (near-field pairs included; C4: 600 x 61 x 120 doubles =
 * 35 MB instead of 4.25 GB of G or 5.3e8 evaluations per step) and every pass -- forward, adjoint, the
 * fused leapfrog step -- becomes circular correlations along the longitude served from LDS.  Values
 * agree with the stored kernel to the rounding of cos(lon - lon') at a shifted pair of longitudes
 * (stated tolerance 1e-10).  gh_build_G fails with GH_ERR_UNSUPPORTED and the reason when the geometry
 * lacks the structure (or has more than 1024 longitudes per cell row: the transforms' tables live in the LDS).
 * gh_compress_wavelet works on such a context (the compressor's rows are evaluated, the forward runs on the CSR
 * operator, the gradient on the table's adjoint pass); batches of chains are refused with it. */
int gh_set_shift_invariant(gh_ctx *ctx, int enable);
/* The structure gh_build_G found: longitudes per cell row, observation classes (distinct latitude /
 * height pairs), cell rows, bytes of the table (all 0 when the store is not in use). */
int gh_shift_invariant_info(const gh_ctx *ctx, int *n_lon, int *n_classes, int *n_rows, int64_t *table_bytes);
/* The store in the longitude-harmonic domain (csrc/lonsymh.hip.h; the default where the geometry allows it: at
 * most 126 longitudes per cell row and 64 observation classes; GRAVHMC_LONSYM_HARMONIC=0 keeps the direct
 * correlations): a circular correlation along the longitude is a product per frequency of length-n DFTs, so
 * forward and adjoint cost n_rows x n_classes x (n / 2 + 1) complex multiply-adds each instead of N M real ones
 * (C4: 2.2e6 against 5.3e8) from a complex table T^[row][class][frequency] of the same size, read once per
 * leapfrog step; the clamp-and-reflect update (hmc.py:135-141) happens at the longitudes, between an inverse
 * and a forward transform inside the cell row's workgroup.  Grids beyond that form's limits (up to 1024 longitudes,
 * any number of classes -- a 1-degree global grid: 360 longitudes, 181 classes, 1800 cell rows, T^ = 0.96 GB where
 * the dense kernel would be 339 GB) run the same arithmetic as four streaming launches per step that read T^ twice
 * (csrc/lonsymw.hip.h; GRAVHMC_LONSYM_WIDE=0 off, =2 everywhere); on a grid symmetric about the equator that form
 * keeps one row of T^ per north-south mirrored pair of cell rows and lets every entry read serve both (half the bytes;
 * mirrored entries of the reference's kernel agree to rounding, within the stated 1e-10; GRAVHMC_LW_MIRROR=0: off).  on: 0 = direct correlations, 1 = the register
 * form, 2 = the streamed form; frequencies n / 2 + 1, bytes of T^, workgroups
 * of the pass.  gh_batch_* on a shift-invariant context (BASELINE configs[3]: 8 chains) runs every chain as a
 * light context of its own -- stream, chain state, work buffers -- on the shared tables, one host thread per
 * chain; nothing stays in flight between calls (n_started = n_done = T in carry-over mode). */
/* The harmonic pass as ONE persistent launch per gh_chain_run call (csrc/lonres.hip.h): every workgroup keeps its cell
 * rows' part of the table in registers for the whole batch of trajectories and the workgroups exchange the forward
 * partials, the residuals' transforms and the Metropolis sums through memory (bounded waits; a launch that gives up
 * leaves the chain untouched and the call runs on the launches per phase).  All four regularisers; one chain at a time
 * (example/global/run_main.sh:16 runs one chain per rank; the chains of a gh_batch_* batch take turns).  workgroups: grid of the launch (0: not
 * in use); launches, evaluations (forward + adjoint product each), trajectories so far, timeouts.
 * GRAVHMC_LONSYM_RESIDENT=0 switches it off. */
int gh_shift_invariant_resident_stats(gh_ctx *ctx, int *workgroups, int64_t *launches, int64_t *evaluations,
                                      int64_t *trajectories, int *timeouts);
int gh_shift_invariant_harmonic(const gh_ctx *ctx, int *on, int *n_freq, int64_t *table_bytes, int *workgroups);
/* What gh_build_G decided for the store (read-only, all zero while no table is resident; `Engine.shift_invariant_plan`).
 * out: [0] form (0 direct correlations, 1 registers, 2 streamed), [1] longitudes n, [2] classes, [3] table rows, [4]
 * frequencies; the direct form: [5] longitudes per work item W, [6] longitude blocks KB, [7] class groups AG, [8] threads,
 * [9] work items per wave, [10] grid, [11] LDS bytes, [12] it could run, [13] which of its four limits refuses it (1 ..
 * 4 in the order gh_build_G tests them, 0 none); the register form: [14] cell rows per workgroup rp, [15] rows a
 * workgroup works on at once rw, [16] grid (0: not this form), [17] LDS bytes; the streamed form (0 where it is not
 * chosen): [18] pitch of a row of T^, [19] pairs of longitudes per thread (1 .. 3: the instantiation of the sweep),
 * [20] north-south mirror, [21] rows of T^ kept, [22] grid of the sweep, [23] rows per part of the forward product,
 * [24] parts; the slots: [25] slots that hold several observations, [26] most observations a slot holds beyond its
 * first; the persistent launch: [27] planned (the plan is made by this call where gh_chain_run has not made it yet),
 * [28] usable with the regulariser set now, [29] its grid, [30] its LDS bytes; [31] 1 where the table exists.
 * GRAVHMC_LONSYM_ROWS=r asks the register form for at least r cell rows per workgroup (the layouts of a large grid on a
 * small one; read by gh_build_G). */
int gh_shift_invariant_plan(gh_ctx *ctx, int32_t out[32]);
/* Work of the matrix-free passes since gh_profile_enable(ctx, 1) (fused form only): entries
 * evaluated, 2x2x2 Gauss-Legendre leaves evaluated (tesseroids; = entries for prisms), launches.
 * Tesseroids: the pairs that need the reference's adaptive subdivision (_tesseroid_numba.py:135-157)
 * are a property of the geometry; when they are few (<= 1/64 of the pairs) gh_build_G evaluates
 * them once and keeps them as a sparse near-field list -- near_entries pairs, near_leaves GLQ leaves
 * (0 when the list is not in use and the passes subdivide inside).  Any pointer may be NULL. */
int gh_matrix_free_stats(gh_ctx *ctx, int64_t *entries, int64_t *leaves, int64_t *launches,
                         int64_t *near_entries, int64_t *near_leaves);
/* Assemble the dense kernel on the device.  Replaces the Python cell loop + native calls of
 * prism.py:291-316 -> _prism.pyx:265-290, or tesseroid.py:189-232 -> _tesseroid_numba.py:32-71,
 * including the unit scaling G*SI2MGAL.  For tesseroids returns GH_ERR_OVERFLOW if any
 * (obs, cell) pair needed more than 100 stack entries. */
int gh_build_G(gh_ctx *ctx);
/* Tesseroid diagnostics of the last gh_build_G: number of cells for which the reference
 * would emit its "stopped dividing" RuntimeWarning (tesseroid.py:228-229) and the total
 * number of GLQ leaf evaluations. */
int gh_kernel_stats(const gh_ctx *ctx, int64_t *warn_cells, int64_t *leaves);
/* Explicit dense kernel from the host instead of assembling it (A[i + j*ld] if
 * fortran_order else A[i*ld + j]). */
int gh_upload_G(gh_ctx *ctx, const double *A, int64_t ld, int fortran_order);
/* Copy the device matrix back, column-major with leading dimension ld >= N (what
 * GravMagModule.kernelw() hands out as `Aw`, potential.py:584-589). */
int gh_download_G(gh_ctx *ctx, double *A, int64_t ld);
/* (The `result` output of prism.gz / tesseroid.gz, d = G * rho for the unweighted kernel, is
 * gh_forward called before gh_weight.) */

/* Sensitivity weighting, potential.py:232-264: wm_j = (sum_i G_ij^2)^weightfactor, G <- G *
 * diag(1/wm) in place (columns with zero norm are left untouched, wm_j = 0).  wm_out (M)
 * receives the diagonal of the reference's Wm. */
int gh_weight(gh_ctx *ctx, double weightfactor, double *wm_out);

/* ---- potential (inversion/potential.py:688-845) ---------------------------------------- */

/* Observed data and, optionally, the field of fixed cells (`fixed=True, grav_fix=...`,
 * potential.py:700-703); pass NULL when unused.  The mean of dobs is removed.  On a GH_CELL_PRISM_JOINT
 * context dobs is the balanced dobsw (N entries, gz first), taken as it is: no mean removal, no grav_fix. */
int gh_set_data(gh_ctx *ctx, const double *dobs, const double *grav_fix_or_null);
/* Regulariser: kind (GH_REG_*), alpha (hmc RegulFactor), beta (MS/TV), mesh shape
 * (nz,ny,nx) for Smoothness/TV (must satisfy nz*ny*nx == M), weighted prior
 * mwapr (M).  Needs gh_weight first for MS (uses wm^2 = diag(WmSquare)).
 * On a context that holds a shard of the cells (gh_shard_init*): mwapr is the local part; for
 * Smoothness/TV shape3 is the GLOBAL mesh shape (nz*ny*nx == M_global), every shard must consist
 * of whole z-planes (m0 and M multiples of ny*nx, else GH_ERR_UNSUPPORTED) and the call is
 * collective (the boundary planes of the prior model are exchanged once; those of the model
 * travel with every evaluation's forward partial). */
int gh_set_reg(gh_ctx *ctx, int kind, double alpha, double beta, const int shape3[3],
               const double *mwapr);
/* d = Aw * mw            (potential.py:698, np.dot(self.Aw, mw)) */
int gh_forward(gh_ctx *ctx, const double *mw, double *dpre);
/* g = Aw^T * r           (potential.py:708, np.dot(self.Aw.T, r)) */
int gh_adjoint(gh_ctx *ctx, const double *r, double *g);
/* Drop-in for GravMagModule.misfit_and_grad with constraint='mandatory'
 * (potential.py:812-845): out3 = (misfit, data_value, model_value), grad (M), dpre (N,
 * without grav_fix). */
int gh_misfit_and_grad(gh_ctx *ctx, const double *x, double out3[3], double *grad,
                       double *dpre);

/* Regulariser value and gradient alone (alpha = 1), for optimisers that combine the terms
 * themselves: ConjugateGradient of inversion/reginv.py:271-355.  ms_grad_den_mw = 1 reproduces
 * that file's MS gradient, whose denominator is (mw^2 + beta)^2 (reginv.py:288-292) instead of
 * ((mw - mwapr)^2 + beta)^2 (potential.py:732-735). */
int gh_reg_eval(gh_ctx *ctx, int kind, double beta, const int shape3[3], int ms_grad_den_mw,
                const double *mw, const double *mwapr, double *value, double *grad /* M or NULL */);

/* ---- wavelet-compressed forward operator (gravmag/compressor1D.py, compressor3D.py) ------ */

/* Build the compressed kernel on the device: row-wise db4 / 'periodization' DWT of the weighted
 * kernel (dims = 3: separable over shape3 = (nz,ny,nx) with nz*ny*nx == M; dims = 1: over the
 * flat model, the variant carved meshes need), hard threshold |c| < thr -> 0, CSR with the
 * column layout of pywt.coeffs_to_array.  Replaces compressor3D.kernelcompressor (:17-44) /
 * compressor1D.kernelcompressor (:17-42); the reference uses thr = 1e-3, levels = 2.  After
 * this call gh_misfit_and_grad and the chain evaluate the FORWARD product as
 * Awcp @ DWT(mw) (modelcompressor, compressor3D.py:47-68) while the gradient keeps the exact
 * dense Aw^T (potential.py:693-708).  nnz_out / ncols_out receive the CSR size (N x ncols).
 * Also on a matrix-free or shift-invariant context (the rows are evaluated instead of gathered) and on ROW blocks of
 * a sharded kernel (after gh_shard_init_rows and gh_weight: the compressor works row by row, every rank compresses
 * its own rows -- N, nnz and gh_download_csr are the rank's); refused on column blocks (a row's transform would span
 * the ranks). */
int gh_compress_wavelet(gh_ctx *ctx, int dims, const int shape3[3], double thr, int levels,
                        int64_t *nnz_out, int64_t *ncols_out);
/* The CSR arrays (what GravMagModule.Awcp holds): indptr N+1, indices/data nnz. */
int gh_download_csr(gh_ctx *ctx, int64_t *indptr, int32_t *indices, double *data);
/* Packed wavelet coefficients of a model vector: pywt.coeffs_to_array(wavedec[n](mw))[0]. */
int gh_model_coeffs(gh_ctx *ctx, const double *mw, double *coeff /* ncols */);
/* d = Awcp @ DWT(mw)    (modelcompressor) */
int gh_forward_wavelet(gh_ctx *ctx, const double *mw, double *dpre);

/* ---- HMC chain (inversion/hmc.py:85-177) ----------------------------------------------- */

/* Start (or restart) a chain at weighted model x0 with per-cell bounds low/high (weighted,
 * hmc.py:391-393).  Evaluates the potential at x0 once and keeps x, residual and gradient
 * resident on the device. */
int gh_chain_init(gh_ctx *ctx, const double *x0, const double *low, const double *high);
/* One trajectory of L leapfrog steps with clamp-and-reflect bounds and the Metropolis test
 * (HamitonianMC._leapfrog, hmc.py:85-177).  p0 = randn(M)*Sigma and u = rand() are drawn by
 * the caller in the reference's RNG order (hmc.py:297,95,164).  out5 = (U, U_data, U_model,
 * Hcur, Hnew) with U.. of the state the chain is left in (proposal if accepted, else the
 * starting point).  The device executes one fused sweep of G per leapfrog step (adjoint of
 * step s and forward of step s+1 share the sweep) plus one adjoint-only sweep, which
 * gh_chain_prefetch_momentum can merge into the next trajectory. */
int gh_chain_trajectory(gh_ctx *ctx, const double *p0, double dt, int L, double u,
                        int *accepted, double out5[5]);
/* Announce the momentum of the trajectory AFTER the next gh_chain_trajectory call (same RNG
 * stream, drawn one trajectory ahead).  The last sweep of that call then also takes the
 * announced trajectory's first leapfrog step from the proposal, so an accepted proposal costs L
 * sweeps of G instead of L+1.  Purely an execution-order optimisation: results are bit-identical
 * with and without it; a rejected proposal simply discards the speculative step.  The
 * announcement is consumed by one gh_chain_trajectory call. */
int gh_chain_prefetch_momentum(gh_ctx *ctx, const double *p0_next);
/* K trajectories in one call (the body of HamitonianMC.sample's loop, hmc.py:295-343, without
 * a Python round trip per trajectory): L[k], p0s[k*M..], us[k] in RNG-stream order;
 * p0_lookahead (or NULL) is the momentum of the trajectory after the batch so the speculative
 * first step also crosses batch boundaries.  Accepted proposals are counted since
 * gh_chain_init; the run stops early once `stop_at_accepts` (> 0) have been accepted, and the
 * posterior window (if any) receives every accepted state beyond the first `record_from`
 * (the sampler's ndraws burn-in).  accepted[k], out5s[5k..] as gh_chain_trajectory; x_out (K*M or
 * NULL) receives the chain state after each ACCEPTED trajectory k; n_run = trajectories done. */
int gh_chain_run(gh_ctx *ctx, int K, const int *L, const double *p0s, const double *us, double dt,
                 const double *p0_lookahead, int64_t stop_at_accepts, int64_t record_from,
                 int *accepted, double *out5s, double *x_out, int *n_run);
/* The trajectory feeder: gh_chain_run's loop on two library threads, for ONE chain on the launches of the sweep path.
 * While it is open a DRAWER thread takes the reference's stream from `rng` a trajectory at a time -- L (plan_L[k] where a
 * plan of n_plan lengths is given, else randint(Lmin, Lmax + 1)), randn(M) * sigma (sigma_vec, or NULL: M factors applied
 * after a draw with sigma = 1), rand() -- into a ring of page-locked rows, at most rows - 2 trajectories ahead, and a
 * RUNNER thread runs them as gh_chain_run does: the row after the running one is its look-ahead (the runner waits for
 * it where the upload is issued, never goes without), accepted states are counted, recorded from `record_from` and,
 * with want_x, copied to a second page-locked ring.  The stream ends after `limit` trajectories (< 0: unbounded; a plan
 * bounds it too), the runner after the trajectory that reaches stop_at_accepts (> 0), and gh_chain_feed_close ends both
 * after the trajectory in flight.  The device sees the stream operations of gh_chain_run; results are bit for bit its.
 *   usable: 1 for one chain on the sweep launches (dense, folded, team sweep, matrix-free, wavelet, the plain passes of
 *     the shift-invariant store); 0 where gh_chain_run takes a persistent launch, on a sharded context, and with
 *     GRAVHMC_CHAIN_FEED=0.
 *   next: blocks for at least one result or the end (timeout_ms >= 0: at most that long), returns up to max_rows
 *     (<= 64) in stream order -- L, accepted, out5s[5 i ..], xs[i M ..] (or NULL) for accepted ones -- and finished = 1
 *     once the runner has ended and everything was returned.  A caller that does not call it throttles the chain.
 *   close: joins both threads; drawn = trajectories taken from the stream, run = trajectories run.
 *   stats: seconds the runner waited for a draw, the drawer for a free row, the runner for the result queue (of the
 *     open feeder, else of the last one), and the rows of the ring (32 MiB / 8 M in 4 .. 64; GRAVHMC_FEED_ROWS, >= 3).
 * An error of either thread is kept with its text and returned by next / close.  While a feeder is open every other
 * entry point on the context returns GH_ERR_ARG (gh_last_error names the feeder); gh_destroy closes it first. */
int gh_chain_feed_usable(gh_ctx *ctx, int *usable);
int gh_chain_feed_open(gh_ctx *ctx, gh_rng *rng, const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit,
                       double sigma, const double *sigma_vec, double dt, int64_t stop_at_accepts, int64_t record_from,
                       int want_x);
int gh_chain_feed_next(gh_ctx *ctx, int max_rows, int timeout_ms, int *L, int *accepted, double *out5s, double *xs,
                       int *n, int *finished);
int gh_chain_feed_close(gh_ctx *ctx, int64_t *drawn, int64_t *run);
int gh_chain_feed_stats(gh_ctx *ctx, double *runner_wait_draw_s, double *drawer_wait_row_s, double *runner_wait_queue_s,
                        int *rows);
/* The feeder's drawer and queue with a host stub in place of the runner (no context, no GPU).  Per trajectory k: out_L,
 * out_u, out_probe[4 k ..] = first, middle, last entry and in-order sum of the momentum, out_look[k] = a look-ahead row
 * was handed over.  The stream must be bounded by at most max_out trajectories. */
int gh_debug_feed_dry_run(gh_rng *rng, const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit, double sigma,
                          const double *sigma_vec, int64_t M, int rows, int64_t max_out, int *out_L, double *out_u,
                          double *out_probe, int *out_look, int64_t *n_out, int64_t *drawn);
/* Diagnostic: the layout the single chain's work buffers were allocated by at the first evaluation.  out[0..15]:
 * allocated (0 / 1), slab rows, slab2 segments, |p|^2 partials of the final half step, of a fresh momentum, slab-row
 * sums, sums per row block, |r|^2 partials, R partials, R partials per property, form of the epilogue's partials
 * (0 none, 1 plain, 2 magnetization-vector, 3 multi-component, 4 joint), their size, offset of R's in them, offset
 * of the coupling term's, doubles of the pinned read-back buffer, slab rows the last forward launch wrote. */
int gh_debug_work_layout(const gh_ctx *ctx, int64_t *out);
/* How often the speculative first step was used / discarded. */
int gh_chain_stats(gh_ctx *ctx, int64_t *spec_hits, int64_t *spec_misses);
/* Small dense problems (N <= 1024, one column block per CU fitting its LDS next to the kernel's
 * scratch, one device, stored G): gh_chain_run runs its K trajectories inside ONE
 * launch with G resident in LDS (csrc/resident.hip.h) instead of one sweep per launch.  Same
 * contract and results to rounding (the summation order over the cells differs); environment
 * GRAVHMC_RESIDENT=0 switches it off.  launches / evaluations: how much ran there so far. */
int gh_chain_resident_stats(gh_ctx *ctx, int64_t *launches, int64_t *evaluations);
/* What the resident kernels would do with this context (read-only; needs the kernel, gh_set_data and
 * gh_set_reg).  out: [0] usable with the regulariser set now, [1] columns per workgroup, [2] workgroups,
 * [3] double2 chunks of a column per lane (rc), [4] register-held columns per wave (ct), [5] split (one copy
 * between registers and LDS), [6] stream (columns beyond [7] read from memory in every pass), [7] columns of a
 * workgroup in LDS, [8] LDS bytes a launch with `chains` chains asks for, [9] LDS bytes a workgroup may
 * have, [10] `chains` chains would run in lock-step (csrc/resbatch.hip.h), [11] its k-steps per wave, [12] its
 * column tiles, [13] its LDS bytes, [14] 1 where the plan exists (all zero otherwise), [15] 0. */
int gh_chain_resident_plan(gh_ctx *ctx, int chains, int32_t out[16]);
/* More observations than one workgroup holds of a column (N > 16384, stored G): the fused leapfrog
 * step runs on teams of `members` workgroups that share each column (csrc/teamsweep.hip.h), still
 * ONE read of G per step; adjoint-only / forward-only sweeps and the steps after a team timed out
 * run in row panels.  members: workgroups per team (0: not in use), launches: team sweeps so far,
 * timeouts: launches that gave up (after three the context stays on row panels), late_parts:
 * columns for which some member found its team's parts not yet published when it needed them
 * and had to wait (as of the last synchronisation; columns x members x launches is the total). */
int gh_team_sweep_stats(gh_ctx *ctx, int *members, int64_t *launches, int *timeouts, int64_t *late_parts);
/* What the team sweep and the row panels would do with this context as it stands (read-only: nothing is
 * allocated or launched; callable before the first sweep, after the kernel is stored).  out: [0] the fused
 * step runs on teams, [1] why not: 0 it does, 1 GRAVHMC_TEAM=0, 2 matrix-free, joint or row-sharded store
 * or no stored kernel, 3 a single row panel (N <= 16384), 4 more than 8 members, 5 fewer than 8 CUs per
 * member, 6 no team per XCD slot, 7 the LDS request is refused, 8 the grid would not be resident; [2] members
 * per team Q, [3] rows per member, [4] rows of the last member, [5] teams per XCD slot, [6] teams (8 x [5]),
 * [7] columns per team, [8] workgroups, [9] columns of lag (GRAVHMC_TEAM_LAG), [10] LDS bytes of a workgroup;
 * the row panels every other sweep of such a context runs in: [11] panels, [12] rows per panel, [13] rows of
 * the last panel; [14], [15] 0.  Past the refusal that stopped the plan the team's figures are 0.
 * GRAVHMC_TEAM_TPX=n (diagnostic) lowers [5] to min(n, planned): fewer, longer column runs per team. */
int gh_team_sweep_plan(gh_ctx *ctx, int32_t out[16]);
int gh_chain_get_x(gh_ctx *ctx, double *x /* M */);
int gh_chain_get_dsyn(gh_ctx *ctx, double *dsyn /* N, dpre of the current state */);
/* ---- several chains sharing every sweep of G (fp64 MFMA) ---------------------------------- */

/* Up to 16 independent chains (the reference runs them as separate MPI ranks, hmc.py:367-369) on
 * ONE GPU against ONE copy of G: per leapfrog step the adjoint and the forward products of all
 * chains are two skinny GEMMs on v_mfma_f64_16x16x4 (32 flop per byte of G instead of 0.5), so 16
 * chains cost two sweeps of G per step instead of 16.  Each chain keeps its own trajectory
 * length L[c] (chains that finish early idle until the longest is done) and its own Metropolis
 * variate; every chain reproduces what a single-chain context computes from the same inputs.
 * Host arrays are chain-major: x0s, p0s = C rows of M doubles.  Unsharded kernel only; with the
 * wavelet-compressed forward only where the resident chain kernel takes the batch (GH_ERR_UNSUPPORTED
 * otherwise: the MFMA form has no compressed forward).
 * Problems small enough for the resident chain kernel (see gh_chain_resident_stats) do not use
 * the MFMA form, which would be bound by its launches there: the chains take turns inside one
 * launch of that kernel per gh_batch_trajectory call (same contract, same results to rounding). */
int gh_batch_init(gh_ctx *ctx, int C, const double *x0s, const double *low, const double *high);
int gh_batch_trajectory(gh_ctx *ctx, const double *p0s, double dt, const int *L, const double *us,
                        int *accepted /* C */, double *out5s /* C x 5, as gh_chain_trajectory */);
/* Up to T further trajectories of every chain in one call; arrays are chain-major: L[c*T + t],
 * us[c*T + t] and the momentum p0_rows[c*T + t] (pointer to M doubles: the rows need not be
 * contiguous) are the trajectories chain c has not started yet, in order.
 * The chains do not wait for each other: a chain that has finished a trajectory (its L steps and
 * the final half momentum step) is decided and starts its next one in the very next sweep while
 * the others are in the middle of theirs, so every sweep of G carries a step of every chain that
 * has work.  (Rounds of gh_batch_trajectory leave a chain idle from its own L to the longest L of
 * the round: with the reference's Lrange [5,20] and 16 chains 38 % of the sweeps' capacity.)  Each
 * chain computes exactly what it computes through gh_batch_trajectory.
 * Results are reported per chain in order of completion: accepted[c*S + i], out5s[(c*S + i)*5 ..]
 * and, if x_out != NULL, the state after an ACCEPTED trajectory at x_out[(c*S + i)*M ..], for the
 * i-th trajectory chain c COMPLETED in this call; S = T result slots per chain, S = T + 1 in
 * carry-over mode (the trajectory that came in flight plus up to T new ones).
 * n_started == n_done == NULL: all T trajectories of every chain are run to completion.
 * Otherwise (carry-over mode) the call ends as soon as some chain has nothing left to start; the
 * other chains keep their trajectory in flight and continue it in the next call (same dt), where
 * its result is the first that chain reports.  n_started[c] = how many of this call's T chain c
 * has started (pass the rest again, followed by new ones), n_done[c] = completions reported.
 * T = 0 in that mode drains: the trajectories in flight are completed (at most one result per
 * chain).  gh_batch_init discards anything in flight. */
int gh_batch_run(gh_ctx *ctx, int T, const int *L, const double *const *p0_rows, const double *us,
                 double dt, int *accepted, double *out5s, double *x_out, int *n_started, int *n_done);
int gh_batch_get_x(gh_ctx *ctx, int chain, double *x /* M */);
/* ---- bootstrap replicates of the CG inversion in lock-step (csrc/bscg.hip.h) ----------------- */

/* Up to 16 replicates of BootStrap.CG (reginv.py:631-713) on ONE read of G per product.  The replicates share the
 * weighted kernel Aw and differ in the draw counts c_b[i] (how often observation i was drawn, reginv.py:736-741)
 * applied to the N-vector between forward and adjoint, so the three products of a CG step -- Aw^T R, Aw.Iw,
 * Aw.x_new -- are the chain batch's skinny GEMMs on v_mfma_f64_16x16x4 with a CG epilogue; every product the
 * sequential loop computes a second time is taken from the forward that ended the iteration before.  Per replicate:
 *     D = Aw x,  data(x) = sum_i c[i] (D[i] - dobs[i])^2,  R = c o (D - dobs),  I = 2 Aw^T R + alpha g_MS(x),
 *     MS(x) = sum wm^2 x^2 / (x^2 + beta2),  g_MS = 2 wm^2 x beta2 / (x^2 + beta2)^2      (no prior, beta2 = beta^2),
 *     Iw = I (k = 0) or I + (|I|^2 / |I_old|^2) Iw_old,  kstep = Iw.I / (sum_i c[i] (Aw Iw)[i]^2 + alpha |Iw|^2),
 *     x_new = wm o clamp((x - kstep Iw) o (1 / wm), rhomin, rhomax),
 *     alpha = 0 (k = 0), data(x_1) / MS(x_1) (k = 1), q alpha where data(x_{k-1}) - data(x_k) < 0.01 data(x_{k-1}),
 * and after the update of an iteration k >= 1, data(x_new) < 0.1 freezes the replicate before that iteration's
 * misfit entries are recorded: its model and rows no longer change while the others go on.  The maxk lock-steps
 * are enqueued on the context's stream without a host synchronisation; a group costs 2 maxk + 1 forward and maxk
 * adjoint sweeps of G whatever B (gh_bscg_stats: the counts of the last group).  All sums in a fixed order; a
 * replicate's results do not depend on the slot it runs in.
 * counts: B rows of N; dobs: N, taken as it is (no mean removed); mw0: the start model times Wm.  Out: models, B rows
 * of M, unweighted; dmis / mmis, B rows of maxk - 1 (data(x_new) / N and MS(x_new) / M of iterations 1 ..), of which
 * n_entries[b] are valid; alpha, B rows of maxk, n_alpha[b] valid.
 * Runs on the dense, weighted store of one GPU and uses the chain batch's buffers (a gh_batch_* batch must be
 * initialised again afterwards), or on the weighted translation-invariant table of a
 * gh_set_translation_invariant(ctx, GH_TABLE_REPLICATES) context, where a sweep is a pass over the table and no second
 * copy of G is made.  GH_ERR_UNSUPPORTED, naming the bootstrap batch: a matrix-free, shift-invariant,
 * translation-invariant (modes 1 and 2, gh_set_cells_multi_table),
 * folded, sharded, joint, multi-component or magnetization-vector context, one with the wavelet-compressed forward,
 * an unweighted store, B outside 1..16, maxk < 2; the context stays usable. */
int gh_bscg_run(gh_ctx *ctx, int B, const double *counts /* B x N */, const double *dobs /* N */,
                const double *mw0 /* M, weighted */, double rhomin, double rhomax, double beta2, double q, int maxk,
                double *models /* B x M, unweighted */, double *dmis /* B x (maxk-1) */, double *mmis /* B x (maxk-1) */,
                double *alpha /* B x maxk */, int *n_entries /* B: valid entries of dmis/mmis */, int *n_alpha /* B */);
int gh_bscg_stats(const gh_ctx *ctx, int64_t *forward_sweeps, int64_t *adjoint_sweeps, int64_t *lock_steps);
/* Page-locked host memory for momentum rows (the reference draws a trajectory's momentum with
 * np.random.randn(M) * Sigma into a fresh array, inversion/hmc.py:91): rows of gh_batch_run that lie in such a
 * block go to the device straight from it, adjacent rows of a chain's list in one copy; rows anywhere else
 * are gathered into the library's own staging buffer first (gh_batch_staging_stats counts both kinds, lock-step
 * form).  Blocks live until gh_pinned_free or gh_destroy. */
int gh_pinned_alloc(gh_ctx *ctx, size_t bytes, void **host);
int gh_pinned_free(gh_ctx *ctx, void *host);
int gh_batch_staging_stats(gh_ctx *ctx, int64_t *rows_direct, int64_t *rows_staged);
/* Two or more chains on a problem small enough for the resident chain kernel with every column in LDS
 * (<= 32 cells per CU, N <= 640: BASELINE configs[0] and [2]) do not take turns: ALL chains advance in
 * lock-step inside one launch per gh_batch_run / gh_batch_trajectory call (csrc/resbatch.hip.h) -- one
 * three-hop exchange per step of the whole batch instead of one per chain, both products of all chains
 * as fp64 MFMA GEMMs (the reference runs its chains as separate MPI ranks: inversion/hmc.py:367-369; per
 * chain the arithmetic is inversion/hmc.py:85-177 with inversion/potential.py:698,708).  A chain whose
 * trajectory ended takes the first step of its next one speculatively while its Metropolis sums travel; a
 * rejected proposal costs that chain one lock-step.  launches, lock-steps and evaluations of all chains
 * ("chain-steps") so far, lock-steps lost to rejected speculation, timeouts (a launch that gave up waiting
 * for its workgroups: the chains take turns in the resident chain kernel from then on, trajectories in
 * flight are replayed there).  GRAVHMC_RESIDENT_BATCH=0 switches the form off. */
int gh_batch_resident_stats(gh_ctx *ctx, int64_t *launches, int64_t *lock_steps, int64_t *chain_steps,
                            int64_t *lost_steps, int *timeouts);
/* Batched chains on a MATRIX-FREE context (gh_set_matrix_free): every entry a pass evaluates serves all
 * chains (example/global/run_main.sh:16 runs its chains as separate ranks, each re-evaluating the whole
 * tesseroid kernel, gravmag/_tesseroid_numba.py:32-71).  Two forms: an adjoint/update pass and a forward
 * pass (two evaluations per entry and step, any N), or -- while every workgroup of the launch is
 * resident, one per CU -- ONE pass in which the workgroups holding the row chunks of the same column tiles
 * exchange their partial dots through memory (teams; csrc/mfbatch.hip.h).  members x ranges = grid of the
 * team form (0: not in use), launches so far, timeouts: launches that gave up waiting (after the first the
 * context stays on the two-pass form; gh_batch_trajectory repeats the round, gh_batch_run returns an error
 * and wants gh_batch_init again). */
int gh_batch_fused_stats(gh_ctx *ctx, int *members, int *ranges, int64_t *launches, int *timeouts);
/* The same team form for ONE chain on a matrix-free tesseroid context (the leapfrog steps of
 * gh_chain_trajectory / gh_chain_run; N <= 17920 observations, the near-field list in use, the GPU not shared):
 * a wave keeps its column's dot with r as one number per tile, so a team exchanges 16 doubles per member and
 * tile, and the column-per-workgroup phases of the plain pass (constants, slots, barrier, scalars, update,
 * forward) disappear.  A pass that times out (2 s) switches the form off for good; the trajectory is
 * repeated on the column-per-workgroup pass.  Numbers as above. */
int gh_matrix_free_team_stats(gh_ctx *ctx, int *members, int *ranges, int64_t *launches, int *timeouts);

/* Posterior statistics without text I/O.  The reference appends every accepted
 * model as a '%.8f' text row to model.dat (hmc.py:328-332) and its plot scripts take np.mean /
 * np.std over the last 100 rows (plot_uniform.py:44-55,103-104).  gh_posterior_window reserves a
 * ring of the last K models m = WmInv @ mw in HBM; gh_posterior_add stores the chain's current
 * state (call it for every accepted, post-burn-in sample); gh_posterior_read returns the
 * per-cell mean and population standard deviation over the window. */
int gh_posterior_window(gh_ctx *ctx, int K);
int gh_posterior_add(gh_ctx *ctx);
int gh_posterior_read(gh_ctx *ctx, int64_t *n_in_window, int64_t *n_total, double *mean /* M or NULL */,
                      double *sd /* M or NULL */);
/* Streaming posterior over WHOLE runs of up to 16 chains: every recorded accepted state is read once where it
 * lies in HBM and folded into running statistics of fixed size -- per chain slot Welford mean / M2 and batch
 * means of length batch_len, and one pooled histogram of `bins` equal bins over [lo, hi] per cell (unweighted
 * model bounds, M each; values outside go to the end bins).  Memory: (5 * 8 * chains + 4 * bins) * M bytes,
 * whatever the number of samples.  gh_posterior_stream allocates and zeroes the state (after gh_weight: the
 * reciprocal column norms are kept); from then on chain slot c records its accepted states number
 * record_from + 1 ... record_from + record_count, counted per chain since gh_chain_init / gh_batch_init, on every
 * chain path (gh_chain_run, gh_batch_trajectory, gh_batch_run; chains of a batch beyond `chains` are not
 * recorded); the ring of gh_posterior_window works unchanged beside it.  The single-chain paths feed the slot
 * gh_posterior_stream_slot sets (default 0), so several chains run one after the other fill slots 0 .. chains - 1.
 * gh_posterior_add, being explicit, feeds that slot whatever the window; gh_posterior_stream_add adds an
 * explicit UNWEIGHTED host row to slot c.  gh_posterior_stream_read: samples per slot, per-cell pooled mean and
 * population std (numpy's ddof = 0), Gelman-Rubin R-hat (NaN unless >= 2 slots recorded the same n >= 2 samples,
 * and where the within-chain variance is 0), batch-means effective sample size summed over the recording slots
 * (NaN while a slot has fewer than 2 complete batches), and the per-slot means and M2 (chains x M); any output
 * may be NULL.  gh_posterior_stream_quantiles: nq <= 32 quantiles q in [0, 1] per cell from the histogram
 * (out: nq x M), within one bin width of the empirical quantile.  GH_ERR_UNSUPPORTED on a sharded context;
 * GH_ERR_ARG for chains outside 1..16, bins outside 2..256, batch_len < 1, hi < lo anywhere, a slot >= chains,
 * or a second gh_posterior_stream without gh_posterior_stream_free. */
int gh_posterior_stream(gh_ctx *ctx, int chains, int bins, int batch_len, int64_t record_from, int64_t record_count,
                        const double *lo, const double *hi);
int gh_posterior_stream_slot(gh_ctx *ctx, int slot);
int gh_posterior_stream_add(gh_ctx *ctx, int slot, const double *m_host);
int gh_posterior_stream_read(gh_ctx *ctx, int64_t *n_per_chain /* chains */, double *mean, double *sd, double *rhat,
                             double *ess /* M each */, double *chain_mean, double *chain_M2 /* chains x M each */);
int gh_posterior_stream_quantiles(gh_ctx *ctx, int nq, const double *q, double *out /* nq x M */);
int gh_posterior_stream_hist(gh_ctx *ctx, uint32_t *out /* bins x M */);
int gh_posterior_stream_free(gh_ctx *ctx);
/* Stateless convenience with the signature SURVEY 8b lists: init + trajectory + readback. */
int gh_leapfrog(gh_ctx *ctx, double *x_inout, const double *p0, double dt, int L,
                const double *low, const double *high, double u, int *accepted,
                double out5[5], double *dsyn_or_null);

/* ---- one chain sharded over several GPUs -------------------------- */

/* Column-block sharding: rank g of `world` creates its context with its own cell count
 * (gh_create(N, M_local)) and passes only its cells / slices of every M-vector; N-vectors
 * (dobs, grav_fix, dpre) are replicated.  Per potential evaluation the ranks exchange ONE
 * all-reduce of N+2 doubles (forward partial + regulariser partial); the gradient, the
 * regulariser gradient and the leapfrog updates stay local, so the fused one-read sweep is
 * kept.  Damping and MS with any partition; Smoothness / TV with shards of whole z-planes (the
 * boundary planes of the model travel in the same all-reduce, see gh_set_reg).  Every rank ends up
 * with bit-identical scalars, hence identical Metropolis decisions.  (Row blocks -- every rank a
 * slice of the observations -- need the M-vector gradient all-reduced between the adjoint and the
 * update: two reads of the shard per step; gh_shard_init_rows below)
 *
 * RCCL flavour: rank 0 obtains a 128-byte id with gh_shard_unique_id, the launcher
 * broadcasts it, every rank calls gh_shard_init (ncclCommInitRank, collective).  The
 * all-reduce runs on the context's stream over xGMI. */
int gh_shard_unique_id(void *id128);
int gh_shard_init(gh_ctx *ctx, const void *id128, int rank, int world, int64_t M_global, int64_t m0);
/* Host-staged flavour: the all-reduce is delegated to a caller-supplied function that sums
 * `count` doubles in place across ranks (e.g. torch.distributed over gloo); used where RCCL
 * cannot run (several ranks on one GPU) and by the tests. */
typedef int (*gh_allreduce_fn)(void *user, double *host_buf, int64_t count);
int gh_shard_init_callback(gh_ctx *ctx, gh_allreduce_fn fn, void *user, int rank, int world,
                           int64_t M_global, int64_t m0);
/* Row-block sharding, BASELINE configs[4] as it is worded ("G row-block sharded ... RCCL reduce over xGMI for
 * the misfit sum"; SURVEY 8e.2, first form): rank g creates its context with ITS observations
 * (gh_create(N_local, M)), passes only its rows of every N-vector (obs, dobs, grav_fix; dpre comes back for its
 * rows) and FULL model vectors, which are replicated.  Call right after gh_create / gh_build_G, before
 * gh_weight and gh_set_data (both are collective then: a column's norm and the mean of the data span the
 * ranks).  Per potential evaluation: the local rows' forward product, two scalar all-reduces (sum of the
 * predicted data for the mean removal of potential.py:706, |r|^2 -- "the misfit sum") and, because a column's
 * dot with r spans the ranks, an all-reduce of the M-vector gradient between the adjoint pass and the update
 * -- the fused one-read sweep is not possible: TWO reads of the local shard per leapfrog step, and M doubles
 * per step across the ranks instead of the column form's N + 2.  Updates and the regulariser are replicated
 * (any regulariser, no halo).  Same scalars on every rank, hence identical Metropolis decisions.  Stored
 * kernel only; no batches.  gh_compress_wavelet AFTER this call and gh_weight gives every rank the compressed form of its
 * own rows (the forward of the local rows then runs on it). */
int gh_shard_init_rows(gh_ctx *ctx, const void *id128, int rank, int world, int64_t N_global, int64_t n0);
int gh_shard_init_rows_callback(gh_ctx *ctx, gh_allreduce_fn fn, void *user, int rank, int world,
                                int64_t N_global, int64_t n0);
/* Sum of `count` (<= N) doubles in place across the ranks of the shard group (host buffers):
 * lets the host combine per-rank scalars through the same communicator. */
int gh_shard_allreduce(gh_ctx *ctx, double *host_buf, int64_t count);

/* ---- sample files ---------------------------------------------------------------------- */

/* One text row of the reference's model.dat / misfit.dat (np.savetxt(fmt='%.8f', delimiter=' '),
 * hmc.py:241-249): n values as printf("%.8f") would print them, separated by one blank, closed by
 * '\n'.  Host only, no context: at 5*10^5 cells a row is 5.5 MB of text per accepted sample
 *  and np.savetxt's ~85 ns per value would cost as much as the trajectory on the GPU.
 * Every value is rounded from its exact binary expansion like printf does (values whose scaled
 * fraction lies within 1e-7 of a rounding boundary, and non-finite or huge ones, go through
 * snprintf).  Returns the number of bytes written, or -1 if `cap` (>= 24 n + 2 is always enough
 * for |v| < 1e13) is too small. */
int64_t gh_format_row_fixed8(const double *v, int64_t n, char *out, int64_t cap);

/* ---- the reference's random stream ------------------------------------------------------ */

/* NumPy's legacy RandomState stream on the host, bit for bit (MT19937; doubles from two outputs;
 * polar Gaussian with its cached second value; masked-rejection integers): what the reference
 * draws per trajectory in HamitonianMC.sample / _leapfrog -- L = np.random.randint(Lmin, Lmax + 1)
 * (hmc.py:297), p0 = np.random.randn(M) * Sigma (hmc.py:95), u = np.random.rand() (hmc.py:164) --
 * K trajectories per call, written straight into the arrays gh_chain_run takes.  Host only, no
 * context.  gh_rng_create(seed) is np.random.seed(seed); get / set_state exchange the stream with
 * np.random.get_state() / set_state() (key[624], pos, has_gauss, cached_gaussian). */
/* (typedef struct gh_rng gh_rng; stands at the top, for the feeder's entry points) */
int gh_rng_create(gh_rng **out, uint32_t seed);
void gh_rng_destroy(gh_rng *rng);
int gh_rng_set_state(gh_rng *rng, const uint32_t *key624, int pos, int has_gauss, double cached);
int gh_rng_get_state(const gh_rng *rng, uint32_t *key624, int *pos, int *has_gauss, double *cached);
/* threads of a draw: 1 = the calling thread alone, 2 = the scale pass (the logarithms) on a second thread behind the
 * sequential generation; 0 = default (GRAVHMC_RNG_THREADS, else 2); -1 = 2 where the process has four cores or more */
int gh_rng_set_threads(gh_rng *rng, int threads);
/* host cores this process may use: the affinity mask capped by the cgroup's CPU quota */
int gh_host_cores(void);
int gh_rng_draw_trajectories(gh_rng *rng, int K, int Lmin, int Lmax, int64_t M, double sigma, int *L,
                             double *p0s /* K x M */, double *us /* K */);

/* ---- the stored kernel folded over the grid's mirrors ------------------------------------ */

/* A gz prism store whose cells and observations are symmetric under x -> 2cx - x and y -> 2cy - y (c: the
 * centre of the cells' extent) holds only a quarter of distinct entries: G(s i, s j) = G(i, j) for each
 * mirror s.  gh_build_G looks for the pairing; the first single-chain sweep after the store changed builds the
 * folded store (the mean of each orbit of four entries, a quarter of the bytes) beside the dense one, which
 * stays untouched, and the sampler's single-chain sweeps (gh_chain_*, gh_leapfrog, gh_misfit_and_grad) read it from
 * then on: results equal the dense sweep's to ~1e-11.  gh_forward and gh_adjoint (the operator itself, entry for
 * entry) and the batches stay on the dense store.  Used when the dense store is larger
 * than GRAVHMC_FOLD_MIN_MB (default 512) MiB, the sweep is one panel of at most 10240 folded rows, the chain
 * is not sharded, joint, wavelet-compressed or matrix-free and would not run on the resident chain kernel, the
 * free memory holds the store and no entry deviates from its orbit's mean by more than 1e-7 of its orbit's
 * largest entry; GRAVHMC_FOLD=0 switches it off.  reason: one of GH_FOLD_*. */
enum {
    GH_FOLD_ON = 0,
    GH_FOLD_UNDECIDED = 1,     /* no sampler sweep since the store changed, or no dense prism store */
    GH_FOLD_SWITCHED_OFF = 2,  /* GRAVHMC_FOLD=0 */
    GH_FOLD_NOT_GZ = 3,        /* not a gz prism store built by gh_build_G (other kind or component, gh_upload_G) */
    GH_FOLD_OBS = 4,           /* an observation without its mirror image (position or height) */
    GH_FOLD_CELLS = 5,         /* a cell without its mirror image */
    GH_FOLD_FIXED = 6,         /* an observation on a mirror line, or a cell that is its own image */
    GH_FOLD_SMALL = 7,         /* dense store not larger than the threshold */
    GH_FOLD_PATH = 8,          /* sharded, joint, wavelet, row panels, resident chain kernel, or too many rows */
    GH_FOLD_NOMEM = 9,         /* not enough free device memory for the folded store */
    GH_FOLD_DEVIATION = 10     /* an orbit's entries differ beyond the sanity bound: a wrong pairing */
};
/* on: the sweeps read the folded store; store_bytes, max_dev (largest |entry - orbit mean| / the orbit's
 * largest entry) and build_ms of the last build. */
int gh_fold_info(const gh_ctx *ctx, int *on, int *reason, int64_t *store_bytes, double *max_dev, double *build_ms);
/* The pairing gh_build_G looks for, without a device: N observations (x, y, z), M cells (bounds6 as in
 * gh_set_cells).  Returns one of GH_FOLD_* (GH_FOLD_ON: found).  obs_img (N ints: N/4 rows of the four images
 * s_0 f, s_x f, s_y f, s_xy f of each fundamental observation f) and cell_orbit (M ints: M/4 rows of the four
 * images of each orbit's first cell), both ordered by their first entry, are written when found. */
int gh_fold_detect(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                   int *obs_img, int *cell_orbit);

/* The diagonal reflection on top of the two mirrors.  Where the cells are square columns and the observations the
 * same grid along x and y, the geometry is also symmetric under tau: (x, y) -> (cx + (y - cy), cy + (x - cx)), gz is
 * symmetric under that swap, and the block of a cell orbit o holds the entries of its partner orbit tau o, row for
 * row.  The folded store keeps its size and layout (both blocks of a pair hold the mean over all eight images); the
 * sampler's sweeps read one block per pair and the blocks of the orbits that are their own partners (the cell
 * columns on a diagonal): about half the store.  GRAVHMC_FOLD_PAIR=0 switches it off (the mirror fold then runs
 * alone).  pair reason: one of GH_FOLD_PAIR_*. */
enum {
    GH_FOLD_PAIR_ON = 0,
    GH_FOLD_PAIR_UNDECIDED = 1,     /* no sampler sweep since the store changed */
    GH_FOLD_PAIR_SWITCHED_OFF = 2,  /* GRAVHMC_FOLD_PAIR=0 */
    GH_FOLD_PAIR_NO_FOLD = 3,       /* the mirrors were not found (gh_fold_info tells why) */
    GH_FOLD_PAIR_OBS = 4,           /* not square: an observation without its image under tau */
    GH_FOLD_PAIR_CELLS = 5,         /* not square: a cell without its image under tau */
    GH_FOLD_PAIR_ROWS = 6           /* more folded rows than the paired sweep takes (N > 10176), or rows that do not
                                       fit its slots (gh_fold_pair_rows) */
};
/* on: the sweeps read one block per pair; pairs and single_orbits: the work items of a sweep; bytes_per_sweep: what
 * a sweep reads of the folded store (work items x block bytes; the whole store where the pairing is off, 0 where
 * the fold is). */
int gh_fold_pair_info(const gh_ctx *ctx, int *on, int *reason, int64_t *pairs, int64_t *single_orbits,
                      int64_t *bytes_per_sweep);
/* gh_fold_detect and then tau, without a device.  Returns gh_fold_detect's result; *pair_reason is GH_FOLD_PAIR_ON,
 * _NO_FOLD, _OBS or _CELLS.  When the pairing is found: obs_tau (N ints) and cell_tau (M ints), the involution on
 * the caller's indices; work (M/4 rows of two ints, *n_work of them written): the leading orbit (a row of
 * gh_fold_detect's cell_orbit) and its partner orbit, or -1 for an orbit that is its own partner; a pair is led by
 * its smaller orbit index and listed once, rows ordered by leading orbit. */
int gh_fold_detect_pair(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                        int *obs_tau, int *cell_tau, int *work, int64_t *n_work, int *pair_reason);
/* The row order of the paired sweep, without a device: the folded rows (gh_fold_detect's obs_img, nF = N / 4 of them,
 * ldF = nF rounded up to 16) folded over tau as well.  tau takes the orbit of row f to that of a row rho f; thread t
 * of 512 owns the rows k 512 + t of a block, k < *rows = ceil(ldF / 512): *pair_slots = (*rows - 1) / 2 pair slots
 * (rows 2 s and 2 s + 1: f < rho f and rho f, pairs by f, slot by slot) and the other rows alone (first the pairs the
 * slots do not hold, their two rows in neighbouring lanes, then the rows with rho f = f).  code (ldF ints): row n of
 * that order is row code[n] >> 2 of obs_img with its four sub-columns k ^ (code[n] & 3), -1: a row of zeros.  ptab
 * (2 (*rows - *pair_slots) x 512 x 4 ints, at most 12288): for slot s of thread t column 2 s holds the observations
 * s_g f of its first row, column 2 s + 1 the observations s_g tau f (those of the second row of a pair slot as the
 * store holds it), -1 where the thread has no row.  counts: pairs in slots, pairs split, rows with rho f = f.
 * (Where the paired sweep is on, every block of the folded store is rewritten in that order once, after the means:
 * within a group of w = min(512, ldF - 512 k) rows the sub-columns 0, 1 of all rows, then their sub-columns 2, 3, so
 * that a wave's loads are contiguous.  Size and block stride of the store do not change.)
 * Returns gh_fold_detect's result; *pair_reason as gh_fold_detect_pair, or GH_FOLD_PAIR_ROWS for more than 2560 folded
 * rows or rows that do not fit the slots. */
int gh_fold_pair_rows(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                      int *rows, int *pair_slots, int *code, int *ptab, int64_t *counts, int *pair_reason);

/* ---- the translation-invariant store of regular prism grids under gridded data ----------- */

/* Where the cells are the full product of nx equal x-intervals, ny equal y-intervals and nz layers and the
 * observations a full px x qy rectangle of the lattice of the cells' spacings at one height (above cell centres,
 * cell corners or anywhere else), every prism field of a pair depends on the layer and the lattice offset alone:
 * K[(p, q), (k, a, b)] = T[k][p - a + nx - 1][q - b + ny - 1], nz (nx + px - 1) (ny + qy - 1) doubles instead of
 * N M (csrc/lattice.hip.h).  gh_set_translation_invariant(ctx, 1) before gh_build_G asks for that table instead of
 * G: a flavour of the matrix-free mode (G is never stored; gh_download_G, the folded store, the resident kernels
 * do not apply), with no limit on N.  It holds GH_CELL_PRISM, GH_CELL_PRISM_COMP and GH_CELL_PRISM_TF, and
 * GH_CELL_PRISM_MULTI by way of gh_set_cells_multi_table (one table per row block); tesseroids,
 * the other stores of blocks, the wavelet compression, shards, the batches of chains, gh_bscg_run (but in mode
 * GH_TABLE_REPLICATES, below) and gh_upload_G are refused (GH_ERR_UNSUPPORTED), a combination with gh_set_matrix_free or gh_set_shift_invariant too (GH_ERR_ARG).
 * gh_build_G detects the structure (GH_ERR_UNSUPPORTED with the reason where it is absent), evaluates every table
 * entry with the dense assembly's entry function on the pair with the smallest (p, q) of its offset -- the entry
 * equals the dense store's entry of that pair bit for bit -- and compares it with the entry of the pair with the
 * largest (p, q): max_dev, as a fraction of the largest entry, refused above 1e-7.  Sums run in an order fixed by
 * indices: results are reproducible bit for bit and agree with the dense store's to ~1e-12.
 * gh_set_translation_invariant(ctx, 2) asks for the same table under the same checks and also takes chain batches:
 * gh_batch_init, gh_batch_trajectory and gh_batch_run then run on it, all 16 chain slots sharing every staged table
 * value (csrc/latbatch.hip.h), for gz, components and the total field alike; 0 and 1 mean what they always did,
 * every refusal text included; any other value is GH_ERR_ARG.  An extent along y the batch pass's LDS tile cannot hold
 * -- the tile is 192 bytes per input of a row padded to 8 plus 64 per output of a workgroup's (at most 64), all the LDS
 * the kernels use, within the 163 840 bytes of a workgroup: 832 cells under 832 observations are the last equal extents
 * that fit, 848 the longest side at all -- is refused by gh_batch_init with GH_ERR_UNSUPPORTED; the wavelet forward, shards, gh_bscg_run and
 * gh_upload_G stay refused, and so do batches on gh_set_cells_multi_table (gh_set_cells_multi_table_chains is the
 * table of blocks that takes them).
 * gh_set_translation_invariant(ctx, GH_TABLE_REPLICATES) asks for the same table under the same checks and also takes
 * gh_bscg_run: the bootstrap batch's lock-step on the table's batch passes -- the 16-column forward as the chain batch
 * runs it, and the 16-column adjoint ending with the CG gradient and its |I|^2 partials instead of the leapfrog update
 * (csrc/latbatch.hip.h) -- 2 maxk + 1 forward and maxk adjoint passes over the table per group (gh_bscg_stats), for gz,
 * components and the total field alike, with the results' bits independent of the slot.  gh_batch_* are refused on it
 * with the store's single-chain refusal, the wavelet forward, shards and gh_upload_G as in modes 1 and 2; an extent the
 * batch tile cannot hold is refused by gh_bscg_run (GH_ERR_UNSUPPORTED, the same reason and byte count), and the single
 * vector passes run on it as in mode 1.  gh_bscg_run stays refused in modes 1 and 2 and on gh_set_cells_multi_table.
 * The value is 4: 3 was GH_ERR_ARG before this mode existed and stays so, as does every value other than 0, 1, 2, 4. */
enum { GH_TABLE_OFF = 0, GH_TABLE_SINGLE = 1, GH_TABLE_CHAINS = 2, GH_TABLE_REPLICATES = 4 };
int gh_set_translation_invariant(gh_ctx *ctx, int enable);
/* What the batch passes of a gh_set_translation_invariant(ctx, 2), (ctx, GH_TABLE_REPLICATES) or gh_set_cells_multi_table_chains context planned on the built table (arithmetic alone:
 * the context's last error text is left as it is; all 0
 * otherwise): out[0] on, [1] fits (0: gh_batch_init refuses the extent), [2] output rows per workgroup, [3] per wave,
 * [4] tiles of 16 outputs per wave at most, [5] forward chunks at most, [6] compute units; then for the adjoint
 * ([7]..[12]) and the forward ([13]..[18]): tiles of 16 outputs along y, workgroups along y, outputs per workgroup
 * along y, staged values per table row, grid x, LDS bytes; [19] layers per forward chunk, [20] forward chunks (slab
 * rows), [21] rows of the |p|^2 partials (workgroups of the adjoint), [22] row blocks of a
 * gh_set_cells_multi_table_chains context (the forward's grid is that many workgroups deep; 0 on a single-block table). */
int gh_translation_invariant_batch_plan(gh_ctx *ctx, int32_t out[24]);
/* on: the table is built; the lattice's extents; table_bytes (all row blocks); max_dev (the largest of the blocks)
 * and build_ms of the build. */
int gh_translation_invariant_info(const gh_ctx *ctx, int *on, int *nx, int *ny, int *nz, int *px, int *qy,
                                  int64_t *table_bytes, double *max_dev, double *build_ms);
/* What a table of magnetization vectors adds (gh_set_cells_mvi_table): axes, the layers' factor (3 there, 2 on the
 * joint store's table, gh_set_cells_joint_table, 1 on every other table: the table has axes x nz layers, nz as
 * gh_translation_invariant_info reports it), and the forward pass's partition of those layers, chunks of
 * layers_per_chunk (joint store: chunks / 2 per property, none across the boundary).  All 0 while no table is built. */
int gh_translation_invariant_axes(const gh_ctx *ctx, int *axes, int *chunks, int *layers_per_chunk);
/* The table T[nz][nx + px - 1][ny + qy - 1] (row-major) as it lies on the device; a gh_set_cells_multi_table
 * context: its ncomp tables, block-major; a gh_set_cells_mvi_table context: T[ncomp][3][nz][.][.]; a
 * gh_set_cells_joint_table context: T[2][nz][.][.], gz then tf. */
int gh_translation_invariant_table(gh_ctx *ctx, double *out);
enum {
    GH_LATTICE_ON = 0,
    GH_LATTICE_CELLS = 1,      /* the cells are not a full product of equal x-intervals, equal y-intervals and layers */
    GH_LATTICE_HEIGHTS = 2,    /* observations at several heights */
    GH_LATTICE_SPACING = 3,    /* observations not on the cells' spacing (linspace over the mesh's extent: L / (n - 1)) */
    GH_LATTICE_RECT = 4,       /* observations on the lattice, but not a full rectangle of it */
    GH_LATTICE_DUPLICATE = 5,  /* two observations or two cells coincide */
    GH_LATTICE_DEVIATION = 6,  /* (gh_build_G) entries of one offset differ beyond the sanity bound */
    GH_LATTICE_LDS = 7         /* (gh_build_G) a lattice row too long for the pass's LDS tile */
};
/* The structure gh_build_G looks for, without a device: N observations (x, y, z), M cells (bounds6 as in
 * gh_set_cells), both in any order; coordinates within 8 ulps of their magnitude, heights and layers bit for bit.
 * Returns one of GH_LATTICE_* (GH_LATTICE_ON: found) or GH_ERR_ARG.  When found: dims5 = {nx, ny, nz, px, qy};
 * lat_of_cell (3 M ints: (k, a, b) of each cell; layers ordered by (z1, z2)) and its inverse cell_of_lat (M ints,
 * [k][a][b]); lat_of_obs (2 N ints: (p, q)) and its inverse obs_of_lat (N ints, [p][q]). */
int gh_lattice_detect(int64_t N, const double *x, const double *y, const double *z, int64_t M, const double *bounds6,
                      int *dims5, int *lat_of_cell, int *cell_of_lat, int *lat_of_obs, int *obs_of_lat);

/* ---- measurement ----------------------------------------------------------------------- */

/* HIP-event timing of the G sweeps (the dominant kernel) on the context's stream.
 * enable != 0 starts recording (and clears the counters).  gh_profile_read sums the recorded
 * intervals of the launches that read the most bytes of G (where one-read sweeps and row-panel
 * launches mix, the one-read sweeps alone: one kernel, comparable with a kernel trace): total
 * milliseconds, number of those launches, bytes of G each of them reads. */
int gh_profile_enable(gh_ctx *ctx, int enable);
int gh_profile_read(gh_ctx *ctx, double *sweep_ms, int64_t *sweep_launches,
                    int64_t *bytes_per_sweep);
/* Attainable streaming-read rate of this device on this context's stored G (the figure SURVEY
 * 8d asks to report next to the nominal 8 TB/s): `reps` timed passes of a read-only kernel over
 * the whole matrix with the sweep's load form (16-byte loads, non-temporal for nt != 0, four
 * independent loads in flight per thread), best of three launch shapes; milliseconds per pass. */
int gh_measure_stream_read(gh_ctx *ctx, int nt, int reps, double *ms_per_pass);
/* Block until everything queued on the context's stream has finished. */
int gh_synchronize(gh_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GRAVHMC_H */
