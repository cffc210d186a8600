// libgravhmc host side: the context (one GPU + one stream + one inversion problem resident in
// HBM) and the small helpers every other part uses.  Included once by gravhmc.hip.
#pragma once

#include "host_layout.h"

static thread_local std::string g_create_error;

struct LonSymHost;  // host_lonsym.h
struct LatticeHost; // host_lattice.h
struct gh_feed;     // host_feed.h

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// The host half of a persistent launch's exchange (exchange.hip.h): the abort word its workgroups raise
// when a wait gives up, the 32-bit tags its granules carry across launches, and what a give-up leaves to
// clear.  Every path whose workgroups wait for each other embeds one (xg_* below).
struct ExchangeGuard {
    unsigned *abort_w = nullptr;           // 4 words: [0] raised by a give-up, [1] late polls of the team sweep
    unsigned seen[4] = {0, 0, 0, 0};       // the abort word as last read back (xg_read)
    unsigned tag = 0, tagE = 0, ltag = 0;  // tags used so far (a path uses one, two or three of them)
    std::vector<DevBuf> grans;             // granule buffers zeroed when the tags start again
    bool dirty = false;                    // a launch gave up: its granules carry tags a later launch would use
    bool inflight = false;                 // launched since the abort word was last read back (team family)
    int aborts = 0;                        // launches that gave up
};

// The trajectory lists of a persistent chain launch on the device (element k: trajectory k) and the pinned host
// staging on their way in and out.  Each of the three launches embeds one (traj_lists_* and traj_upload below).
struct TrajLists {
    int cap = 0;  // list elements the device lists hold
    int *L = nullptr, *accepted = nullptr, *chain = nullptr;
    double *p0s = nullptr, *us = nullptr, *out5s = nullptr, *xacc = nullptr;
    double *h_stage = nullptr;   // pinned staging of the momentum rows
    size_t h_stage_n = 0;
    double *h_xstage = nullptr;  // pinned staging of the accepted models on their way out (the lock-step launch)
    size_t h_xstage_n = 0;
    int64_t rows_direct = 0, rows_staged = 0;  // rows sent straight from the caller's pinned memory / gathered first
};

// One state set of the MFMA batch (chain-interleaved): models, alpha * grad R, synthetic data, residuals.
struct BatchSet { double *X, *GREG, *D, *Rt; };

struct gh_ctx {
    int device = 0;
    int64_t N = 0, M = 0, ld = 0;
    int cus = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // upload of the next trajectory's momentum beside the sweeps
    hipEvent_t copy_ev = nullptr;
    std::string err;
    std::vector<void *> allocs;
    // the trajectory feeder (host_feed.h): while feed_open is set two library threads run the chain on this context,
    // and every entry point but gh_chain_feed_next / _close / _stats refuses (GH_FEED_GUARD)
    gh_feed *feed = nullptr;
    std::atomic<int> feed_open{0};

    // geometry / kernel
    double *obs[3] = {nullptr, nullptr, nullptr};
    double *bounds = nullptr;
    bool obs_h_uniform = false;  // every observation at the same height (third coordinate)
    double obs_h0 = 0.0;
    int cell_kind = -1;
    double ratio = 1.6;
    double tf_dir[3] = {0.0, 0.0, 0.0};  // GH_CELL_PRISM_TF: the field direction (fx, fy, fz)
    double *tf_dir_d = nullptr;            // ... and its device copy (MfGeom::o3 of the matrix-free passes)
    int comp = GH_COMP_GZ;                 // GH_CELL_PRISM_COMP / GH_CELL_TESSEROID_COMP: the gravity component (MfGeom::comp)
    // GH_CELL_PRISM_JOINT: H = [Aw_gz | Aw_tf] of ld rows (ld of N/2) and M = 2m columns; observation-space
    // vectors live as [gz: ld | tf: ld] (2 ld doubles), model-space vectors as M
    bool joint = false;
    double joint_std[2] = {0.0, 0.0};      // population std of the unweighted gz / tf blocks (gh_weight)
    // GH_CELL_PRISM_MULTI: n gravity components of the same cells at the same N / n points, stacked in row blocks
    // of one dense store (block b = rows [b N/n, (b + 1) N/n), component comp[b], times w[b] once weighted)
    struct Multi {
        int n = 0;  // 0: not a multi-component context
        int comp[GH_MULTI_MAX] = {};
        double w[GH_MULTI_MAX] = {};
        double ratio[GH_MULTI_MAX] = {};     // GH_CELL_TESSEROID_MULTI: the distance-size ratio of each block's field
        double obs_mean[GH_MULTI_MAX] = {};  // the mean gh_set_data removed from each block of Wb dobs
        double *bsum = nullptr;              // n x (slab rows): sums of the slab rows per block (slab_block_sums_kernel)
        double *bmean = nullptr;             // n: the blocks' means of the last evaluation's prediction
    } mc;
    // GH_CELL_PRISM_MVI: A = [A_x | A_y | A_z] of the same M / 3 prisms at the same N points, an ordinary dense
    // N x M store whose model vectors are property-major (mx of every cell, then my, then mz)
    bool mvi = false;
    double *tmag_fdir = nullptr;  // GH_CELL_TESS_MVI_DATA: the total field's unit vectors, 3 per observation point
    // ... and its amplitude coupling (gh_set_amplitude): lambda > 0 switches it on.  (Phi of the chain's state and
    // of the last evaluation are kept with the cross-gradient term's, cg.phi_cur / cg.phi_last: a context has
    // at most one of the two couplings.)
    struct Amp {
        bool set = false;  // sw is resident
        double lambda = 0.0, beta = 1.0, scale = 1.0;
        double *sw = nullptr, *abuf = nullptr;  // winv / scale (M); the amplitudes of gh_amplitude_eval (M / 3)
    } amp;
    double *amppart = nullptr;  // partials of Phi where the epilogue keeps none (summed by finish_kernel)
    bool have_obs = false, have_cells = false, have_G = false, weighted = false;
    double *G = nullptr;
    int64_t warn_cells = 0, leaves = 0;
    bool mf = false;          // matrix-free: entries are re-evaluated, G is never stored
    bool mf_before_ls = false;  // what gh_set_matrix_free asked for, while the shift-invariant store holds mf
    bool dense_ok = true;     // N fits the register-resident sweep (<= 16384 rows)
    double *tconv = nullptr;  // tesseroid obs converted to (lon rad, sin lat, cos lat, radius)
    int64_t mf_cells_per_chunk = 0;
    // fused matrix-free pass (mf_fused_kernel: every entry evaluated once per step), N <= 16384
    bool mf_fused = false;
    int mf_T = 0, mf_EPT = 0;
    size_t mf_lds = 0;
    double *mf_cellc = nullptr;       // tesseroids: per-cell constants (tess_cellconst_kernel)
    ghk::MfStats *mf_stats = nullptr; // entries / GLQ leaves evaluated while profiling is enabled
    // tesseroids: near-field table (pairs that need the adaptive subdivision: evaluated once, kept)
    bool mf_near_on = false;
    bool mf_pipe = false;    // mf_tess_fast_kernel (next column's constants fetched ahead; r and the column in LDS)
    bool mf_exact = false;   // the root leaf in the reference's operation order (tess_leaf_cc) instead of tess_leaf_fast
    int mf_exact_req = -1;   // gh_set_matrix_free_exact: 0 / 1; -1: not called, the environment (GRAVHMC_MF_EXACT) decides
    int64_t *mf_near_ptr = nullptr;
    int *mf_near_row = nullptr;
    double *mf_near_val = nullptr;
    int64_t mf_near_n = 0, mf_near_leaves = 0;
    int64_t mf_launches = 0;
    // single chain on teams of workgroups (mf_team_kernel, mfbatch.hip.h)
    struct MfTeam {
        int state = 0;  // 0 not planned, 1 usable, -1 not applicable / given up
        int members = 0, ranges = 0, tpr = 0;
        ghk::u64 *gran = nullptr;
        ExchangeGuard xg;  // off at the first give-up
        double *snear = nullptr;
        int64_t launches = 0;
    } mft;
    bool chain_teams_ok = false;  // set by the trajectory code around its sweeps (it handles a time-out)
    // shift-invariant store of a regular spherical grid (lonsym.hip.h): a table instead of G or of
    // per-step evaluations; a flavour of the matrix-free mode (gh_set_shift_invariant)
    LonSymHost *ls = nullptr;
    // translation-invariant store of a regular prism grid under gridded data (lattice.hip.h): the Cartesian
    // counterpart, also a flavour of the matrix-free mode (gh_set_translation_invariant)
    LatticeHost *lat = nullptr;

    // chains of a batch on the shift-invariant store: light contexts of their own (stream, chain state, work
    // buffers) that share this context's tables and problem vectors; run concurrently, one host thread each
    std::vector<gh_ctx *> kids;

    // sweep configuration
    int TW = 0, EPT2 = 0, PF = 1;
    int n_panels = 1;        // row panels of the dense sweep (N > 16384 rows: > 1, two reads of G per step)
    int64_t panel_rows = 0;
    double *gbuf = nullptr;   // gradient accumulated over the panels
    // team sweep (teamsweep.hip.h): N > 16384 with ONE read of G per fused step
    struct Team {
        int state = 0;        // 0 not planned, 1 usable, -1 not applicable / given up
        int Q = 0, tpx = 0, grid = 0;
        int threads = 0, ept2 = 0, depth = 0;  // instantiation of teamsweep_kernel
        int lag = 1;                           // columns between a member's dot and its update
        int64_t panel_rows = 0;                // rows per member
        int64_t cols_per_team = 0;
        size_t lds = 0;
        ghk::u64 *gran = nullptr;
        ExchangeGuard xg;  // off for good after three give-ups
        int64_t launches = 0;
        unsigned late_polls = 0;
    } tm;
    int slab_live = 0;        // rows of the slab the last forward launch wrote
    // one-launch epilogue (reduce_finish_kernel): sums of the slab rows from the sweep, |r|^2 partials
    double *dsum = nullptr;
    bool dsum_live = false;   // the last forward launch delivered dsum for all slab_live rows
    int dsum_n = 0;           // > 0: dsum holds this many partial sums (not one per slab row)
    double gfix_sum = 0.0;
    bool NT = false;
    int n_teams = 0, grid = 0;
    int n_teams_sweep = 0;   // teams of the sweep launch (n_teams may be larger: size of the pp partials)
    int64_t cols_per_team = 0;
    size_t lds_bytes = 0;

    // problem vectors
    double *dobs_c = nullptr, *gfix = nullptr, *mwapr = nullptr, *wm = nullptr, *wm2 = nullptr;
    double *low = nullptr, *high = nullptr;
    bool have_data = false, have_fix = false, have_reg = false;
    int reg_kind = 0, shape[3] = {1, 1, 1};
    double alpha = 1.0, beta = 0.01;
    // cross-gradient coupling of a joint context (gh_set_cross_gradient): lambda > 0 switches it on
    struct CrossGrad {
        bool set = false;  // shape, spacings and normalisers are resident
        double lambda = 0.0, scale[2] = {1.0, 1.0}, ihx = 1.0, ihy = 1.0;
        int shape[3] = {1, 1, 1};
        double *ihz = nullptr, *sw = nullptr, *tbuf = nullptr, *phi_all = nullptr;
        double phi_cur = 0.0, phi_last = 0.0;  // of the chain's current state / of the last evaluation or state
    } cg;

    // chain state: three (r, greg, d, scal) sets and three x buffers rotate between "current
    // sample", "proposal" and "speculative first step of the next trajectory"; set/buffer 3 is
    // private to gh_misfit_and_grad.  Swapping indices makes accept/reject free.
    struct StateSet {
        double *r = nullptr, *greg = nullptr, *d = nullptr, *scal = nullptr;
        double *part = nullptr;        // |r|^2 and R partials of a one-launch epilogue
        double *phi = nullptr;         // Phi of the coupling term (joint store: cross-gradient; MVI store: amplitude)
        mutable bool pending = false;  // scal[0..2] still to be summed from `part` (scal_ready)
    } st[4];
    double *xb[4] = {nullptr, nullptr, nullptr, nullptr};
    double *pb[2] = {nullptr, nullptr};
    double *pn = nullptr;  // momentum of the NEXT trajectory (gh_chain_prefetch_momentum)
    int cur = 0, xcur = 0;
    bool pn_valid = false, spec_valid = false;
    double pn_probe[3] = {0, 0, 0}, spec_probe[3] = {0, 0, 0};
    double spec_dt = 0.0, spec_pp0 = 0.0, pn_pp0 = 0.0, spec_U[3] = {0, 0, 0};
    int spec_set = 0, spec_x = 0, spec_p = 0;
    int64_t spec_hits = 0, spec_misses = 0, accept_count = 0;
    double *slab2 = nullptr;
    double *slab = nullptr, *dpart = nullptr, *regpart = nullptr, *pp_part = nullptr,
           *ppn_part = nullptr, *pp0_part = nullptr, *pn0_part = nullptr, *scal_all = nullptr;
    double *tmpM = nullptr, *tmpN = nullptr;
    // the layout ensure_work allocated them by (host_layout.h); work_ready: they exist, sized once, never again
    WorkLayout work;
    bool work_ready = false, work_epilogue1 = true;
    double *h_scal = nullptr;  // pinned: scalars + partial sums, laid out by work.h_*()
    bool chain_ready = false;
    double U_cur[3] = {0, 0, 0};
    bool st_stale = false;  // the resident chain kernel moved x: st[cur] / U_cur are those of an older sample

    // column-block sharding of ONE chain over several GPUs: this context holds
    // the cells [m0, m0 + M) of M_global; N-vectors are replicated, the forward partials are
    // summed across ranks once per potential evaluation.
    struct Shard {
        int kind = 0;  // 0 single GPU, 1 RCCL all-reduce on the stream, 2 host callback
        int axis = 0;  // 0: the CELLS (columns of G) are split over the ranks; 1: the OBSERVATIONS (rows of G)
        int64_t N_global = 0, n0 = 0;  // axis 1: observations of the whole problem, first one of this rank
        double *rbuf = nullptr;        // axis 1: {sum of d + grav_fix, |r|^2} on their way through the all-reduces
        int rank = 0, world = 1;
        int64_t M_global = 0, m0 = 0;
        ncclComm_t comm = nullptr;
        gh_allreduce_fn cb = nullptr;
        void *user = nullptr;
        double *buf = nullptr;    // device: [d partial (ld) | R partial | pad | boundary planes (halo)]
        double *hbuf = nullptr;   // pinned staging for the callback path
        size_t buf_n = 0;         // doubles in buf / hbuf
        // Smoothness / TV on cells sharded in whole z-planes: the ranks exchange their boundary
        // planes of the model once per evaluation (inside the forward partial's all-reduce)
        bool halo = false;
        int64_t P = 0;            // cells per plane (ny * nx)
        double *alo = nullptr, *ahi = nullptr;  // prior model of the planes below / above
        double *rb = nullptr;     // regulariser partial for its own (2-double) all-reduce
        int64_t collectives = 0;
    } sh;

    // wavelet-compressed forward operator (compressor1D/3D): CSR N x Mp on the device
    struct Wavelet {
        bool on = false;
        int dims = 0, levels = 2;
        int shape[3] = {1, 1, 1};
        int X[5][3];      // X[i]: extents of the blocks level i produces (X[0] = model shape)
        int offd[5][3];   // packed offset of level i's detail pieces (pywt.coeffs_to_array)
        int D[3] = {1, 1, 1};
        bool tax[3] = {false, false, true};  // transformed axes
        int64_t Mp = 0, nnz = 0;
        double thr = 1e-3;
        int64_t *indptr = nullptr;
        int *indices = nullptr;
        double *data = nullptr;
        double *coeff = nullptr, *s1 = nullptr, *s2 = nullptr;  // model-sized scratch
        int64_t coeff_n = 0;                                    // doubles each of them holds
        ghk::DwtLdsPlan lds_plan;  // one-launch transform of one model vector (dwt_lds_kernel)
        size_t lds_bytes = 0;      // 0: the working block does not fit the LDS -> one launch per pass
        double *F = nullptr;  // dense model-space form Awcp W (ld x M, column-major), built on demand
        bool F_valid = false;
    } wv;

    // several chains sharing every sweep of G (fp64 MFMA path, batch.hip.h)
    struct Batch {
        int C = 0;
        double *Xc = nullptr, *Rtc = nullptr, *GREGc = nullptr, *Dc = nullptr;   // current states
        double *Xw[2] = {nullptr, nullptr}, *Pw[2] = {nullptr, nullptr};
        double *Rtw = nullptr, *GREGw = nullptr, *Dw = nullptr, *scal = nullptr;
        // the table of blocks: 16 x (row blocks) means of the last evaluation's predictions, per chain; of the current states'
        // (gh_batch_block_means)
        double *bmean = nullptr, *bmean_cur = nullptr;
        double *slab = nullptr, *regpart = nullptr, *pp_part = nullptr, *pp0_part = nullptr;
        double *stage = nullptr;  // C x M rows as the host passes them
        double *stage2 = nullptr; // second set of rows (gh_batch_run: next trajectories' momenta sent ahead)
        // gh_batch_run: second working set (the sweep reads one, the evaluation writes the other, so the
        // proposal's values survive a speculative first step) and the next trajectories' momenta
        double *GREGw2 = nullptr, *Dw2 = nullptr, *Rtw2 = nullptr, *scal2 = nullptr, *Pn = nullptr, *pn0_part = nullptr;
        double *Gb = nullptr;     // second copy of G in MFMA operand order (adjoint), if HBM allows
        uint64_t Gb_gen = ~0ull;  // G_gen it was laid out from (batch_relayout fills it again for another)
        // matrix-free batch (mfbatch.hip.h): 1 / wm, the near-field pairs as differences to the staged
        // root leaf (column-major: mf_near_ptr / mf_near_row / ndelta; row-major copy: rptr / rcol / rdelta)
        double *iw = nullptr, *Snear = nullptr, *ndelta = nullptr, *rdelta = nullptr;
        int64_t *rptr = nullptr;
        int *rcol = nullptr;
        bool mfb_near = false, near_built = false;
        int mfb_grid_adj = 0, mfb_rchunks = 0, mfb_ranges = 0, mfb_tpr = 0;
        int slab_live = 0;        // blocks of the slab the last matrix-free forward wrote
        // team pass: one evaluation (mfb_fused_kernel) / one read (batch_team_kernel, stored G) per entry and step
        bool fus_on = false;
        int fus_members = 0, fus_ranges = 0, fus_tpr = 0;
        ghk::u64 *fus_gran = nullptr;
        ghk::u64 *fus_granx = nullptr;  // stored kernel on teams (batch_team_kernel): the new positions' granules
        int fus_nval = 0;               // ... and the (cell, chain) pairs of a tile a member updates
        ExchangeGuard fus;             // either team pass (off at the first give-up)
        long long *fus_dbg = nullptr;  // GRAVHMC_MFB_TIMING: per-phase clocks of one workgroup
        double *Pstart = nullptr;      // M x 16: the momentum each trajectory in flight started with (gh_batch_run)
        int64_t fus_launches = 0;
        const double *fus_fwd_of = nullptr;  // the X whose forward partials the last fused launch left in the slab
        double *h = nullptr;      // pinned read-back buffer, laid out by h_*() below
        int n_colblocks = 0, n_regblocks = 0, n_waves = 0, n_pp0 = 0;
        int64_t cols_per_block = 0;
        double U[CB][3];
        bool ready = false;
        int64_t sweeps = 0;
        // scheduler of gh_batch_run: trajectories in flight survive the call (carry-over mode)
        struct Run {
            bool live = false;
            bool active[CB] = {};
            int s_of[CB] = {}, L_cur[CB] = {}, par[CB] = {};
            double u_cur[CB] = {}, pp0[CB] = {};
            int xi = 0, pin = 0, ws = 0;  // ws: working set the next sweep reads
            double dt = 0.0;
        } run;
        // the state sets: the chains' current one, and working set ws (0 / 1) with the models in Xw[xi]
        BatchSet cur() const { return {Xc, GREGc, Dc, Rtc}; }
        BatchSet work(int xi, int ws) const { return {Xw[xi], ws ? GREGw2 : GREGw, ws ? Dw2 : Dw, ws ? Rtw2 : Rtw}; }
        double *scal_of(int ws) const { return ws ? scal2 : scal; }
        // h: 4 scalars per chain slot, then rows of CB partial sums of |p|^2 -- n_waves of the final half step
        // (pp_part), n_pp0 of the initial momenta (pp0_part), n_pp0 of the next trajectories' momenta (pn0_part)
        size_t h_pp() const { return (size_t)CB * 4; }
        size_t h_pp0() const { return h_pp() + (size_t)n_waves * CB; }
        size_t h_pn0() const { return h_pp0() + (size_t)n_pp0 * CB; }
        size_t h_size() const { return h_pn0() + (size_t)n_pp0 * CB; }
        double h_sum(size_t region, int rows, int k) const  // chain k's sum over the rows of a region, in row order
        {
            double s = 0.0;
            for (int w = 0; w < rows; ++w) s += h[region + (size_t)w * CB + k];
            return s;
        }
    } bt;

    // bootstrap replicates of the CG inversion in lock-step (bscg.hip.h, host_bscg.h); the M x 16 and ld x 16
    // vectors live in the chain batch's buffers
    struct Bscg {
        ghk::BscgState *st = nullptr;  // 16 slots
        double *crow = nullptr;        // B x N counts as the host passes them
        double *dobs = nullptr, *mw0 = nullptr, *iw = nullptr;
        double *dirpart = nullptr, *mspart = nullptr;  // per-block partials of Iw.I, |Iw|^2 / of MS(x_new)
        double *res = nullptr;         // result rows: data misfit, model misfit, regularisation factors
        int res_maxk = 0, nblk = 0;
        int64_t forward_sweeps = 0, adjoint_sweeps = 0, lock_steps = 0;  // of the last group
    } bs;

    // resident chain kernel (resident.hip.h): G held in LDS across a whole batch of trajectories
    struct Resident {
        int state = 0;  // 0 not planned yet, 1 usable, -1 not applicable
        int cpw = 0, nwg = 0, rc = 0, ct = 0;  // ct: columns per wave kept in registers
        int lds_cols = 0;     // columns of a workgroup held in LDS
        bool split = false;   // one copy: the first 8 ct columns in registers only, the rest in LDS
        bool stream = false;  // columns beyond lds_cols are read from memory in every pass (resident.hip.h)
        size_t lds = 0;
        ghk::u64 *slabg = nullptr, *xslabg = nullptr, *dclg = nullptr, *scalg = nullptr, *xscalg = nullptr, *xccg = nullptr;
        double *xpub = nullptr;
        ExchangeGuard xg;  // after three give-ups the context stays on the sweep path
        TrajLists lists;
        int *n_run = nullptr;
        int lds_max = 0;
        // several chains sharing the resident G (gh_batch_* on small problems)
        double *bx = nullptr, *bg = nullptr, *bu = nullptr;  // C x M models, C x M gradients, 3 C potentials
        bool b_on = false, b_state = false;
        int64_t launches = 0, evals = 0;
        long long *dbg = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        // the chains in LOCK-STEP (resbatch.hip.h): planned per gh_batch_init
        struct LockStep {
            bool on = false;
            int ks = 0, nt = 0, C = 0;
            size_t lds = 0;
            ghk::u32x4 *xslabg = nullptr, *dclg = nullptr;
            double *slabd = nullptr;
            ghk::u64 *xccg = nullptr, *flagg = nullptr;
            double *xpub = nullptr, *xs = nullptr, *ps = nullptr, *pst = nullptr, *cst = nullptr;
            int *n_io = nullptr;
            TrajLists lists;             // chain-major
            ExchangeGuard xg;           // off at the first give-up
            bool active[16] = {};        // chain has a trajectory in flight (carry-over mode)
            int64_t launches = 0, lock_steps = 0, lost = 0, chain_steps = 0;
            long long *dbg = nullptr;
        } ls;
    } rs;
    int64_t prof_res_evals = 0;

    // the stored kernel folded over the grid's two mirrors (host_fold.h, fold.hip.h): a quarter of G per sweep
    uint64_t G_gen = 0;  // bumped whenever the dense store (or what it is built from) changes
    struct Fold {
        int detected = 0;     // 1: the geometry pairs up (gh_build_G of gz prisms), -1: it does not, 0: not looked
        int reason = GH_FOLD_UNDECIDED;
        uint64_t gen = ~0ull; // G_gen the decision below was made for
        bool valid = false;   // S holds the folded store of G_gen and the sweeps use it
        int nF = 0, ldF = 0;
        int64_t n_orb = 0;
        std::vector<int> obs_img, cell_orbit;  // host tables (nF x 4, n_orb x 4)
        int *obs_img_d = nullptr, *cell_orbit_d = nullptr;
        double *S = nullptr;
        double *zeros = nullptr;  // M zeros: what the sweep reads for an input its mode does not use
        unsigned long long *dev_bits = nullptr;
        int ept2 = 0, grid = 0;
        int64_t orb_per_team = 0;
        size_t lds = 0;
        double max_dev = 0.0, build_ms = 0.0;
        int64_t launches = 0;
        bool exact = false;   // gh_forward / gh_adjoint in progress: the operator itself, on the dense store
        // the diagonal reflection on top of the mirrors (fold_pair_sweep_kernel): a sweep reads one block per pair
        bool pair_detected = false, pair_on = false;
        int pair_reason = GH_FOLD_PAIR_UNDECIDED;
        int64_t n_work = 0, n_pairs = 0, work_per_team = 0;
        int pair_rows = 0;
        bool pair_rows_ok = false;  // the folded rows fit the paired sweep's slots (fold_detail::pair_rows_plan)
        int *wtab_d = nullptr, *row_tau_d = nullptr, *orb_tau_d = nullptr;
        int *ptab_d = nullptr, *row_code_d = nullptr;  // the paired sweep's row order: its table and the store's pass
    } fd;

    // page-locked host memory handed to the caller (gh_pinned_alloc): momentum rows drawn into it go to the device
    // without a gather on the host
    std::vector<PinnedBlock> pinned;

    // ring of the last K accepted samples (posterior statistics without text I/O)
    double *ring = nullptr, *ring_mean = nullptr, *ring_sd = nullptr;
    int ring_K = 0, ring_next = 0;
    int64_t ring_count = 0;

    // streaming posterior over whole runs of up to 16 chains (poststream.hip.h, host_poststream.h)
    struct PostStream {
        bool on = false;
        int slot = 0;                 // the chain slot the single-chain paths feed
        int64_t from = 0, count = 0;  // a chain's accepted states number from + 1 ... from + count are recorded
        ghk::PostState d = {};
        double *lo = nullptr, *hi = nullptr, *iw = nullptr;
        double *row = nullptr;        // M: an explicit host row on its way in (gh_posterior_stream_add)
        double *out = nullptr;        // 4 M: pooled mean, std, R-hat, ESS of the last read
        double *qout = nullptr;       // quantiles of the last read
        size_t qout_n = 0;
        int64_t n[16] = {}, K[16] = {};  // recorded samples / completed batches per chain slot
        int64_t launches = 0;
    } ps;
    int64_t bt_accepts[16] = {};  // accepted trajectories per chain of the batch since gh_batch_init

    // profiling of the sweeps
    bool prof = false;
    int prof_stride = 1;
    int64_t prof_seen = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    double prof_ms_acc = 0.0;
    int64_t prof_launches = 0;
    std::vector<int64_t> ev_bytes;  // bytes of G the timed launch of event pair i read
    int64_t prof_bytes_last = 0;
};

static int fail(gh_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

// First statement of an entry point: the context belongs to its open feeder's threads (its error text included, so
// nothing is written: gh_last_error names the feeder while it is open).
#define GH_FEED_GUARD(c)                                                                    \
    do {                                                                                    \
        if ((c) && (c)->feed_open.load(std::memory_order_acquire)) return GH_ERR_ARG;       \
    } while (0)

#define HIPCHK(c, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail((c), e_ == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP,         \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,    \
                        __LINE__);                                                          \
    } while (0)

template <typename T>
static int dalloc(gh_ctx *c, T **out, size_t count, bool zero = true)
{
    if (*out) return GH_OK;
    void *p = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    HIPCHK(c, hipMalloc(&p, bytes));
    c->allocs.push_back(p);
    if (zero) HIPCHK(c, hipMemsetAsync(p, 0, bytes, c->stream));
    *out = static_cast<T *>(p);
    return GH_OK;
}

// A block of dalloc's given back before gh_destroy (sizes that change with the kernel: the wavelet rows).
template <typename T>
static void dev_release(gh_ctx *c, T *&p)
{
    if (!p) return;
    auto it = std::find(c->allocs.begin(), c->allocs.end(), (void *)p);
    if (it != c->allocs.end()) c->allocs.erase(it);
    hipFree((void *)p);
    p = nullptr;
}

#define TRY(x)                 \
    do {                       \
        int rc_ = (x);         \
        if (rc_ != GH_OK) return rc_; \
    } while (0)

// tags start again on zeroed granules before any of them would pass this
constexpr uint64_t XG_TAG_LIMIT = 0xf0000000ull;

// The abort word (zeroed), and the granule buffers a restart of the tags zeroes, known at plan time.
static int xg_alloc(gh_ctx *c, ExchangeGuard &g, std::vector<DevBuf> grans)
{
    TRY(dalloc(c, &g.abort_w, 4));
    g.grans = std::move(grans);
    return GH_OK;
}

// Before a launch that may advance tag / tagE by up to ahead / aheadE (ltag: by one): after a give-up, or
// where a tag would pass the limit, zero the granules and start the tags again.  rearm: zero the abort word
// before every launch (the resident family); otherwise only after a give-up (the team family, whose kernels
// look at the word at entry and leave while it is raised).
static int xg_prepare(gh_ctx *c, ExchangeGuard &g, bool rearm, uint64_t ahead, uint64_t aheadE = 0)
{
    if (g.dirty || g.tag + ahead > XG_TAG_LIMIT || g.tagE + aheadE > XG_TAG_LIMIT || g.ltag > XG_TAG_LIMIT) {
        for (const DevBuf &b : g.grans) HIPCHK(c, hipMemsetAsync(b.p, 0, b.bytes, c->stream));
        g.tag = g.tagE = g.ltag = 0;
        rearm = rearm || g.dirty;
        g.dirty = false;
    }
    if (rearm) HIPCHK(c, hipMemsetAsync(g.abort_w, 0, sizeof g.seen, c->stream));
    return GH_OK;
}

// Enqueue the copy of the abort word into g.seen; the path's own synchronisation point delivers it.
static int xg_read(gh_ctx *c, ExchangeGuard &g)
{
    HIPCHK(c, hipMemcpyAsync(g.seen, g.abort_w, sizeof g.seen, hipMemcpyDeviceToHost, c->stream));
    return GH_OK;
}

// A launch gave up (g.seen[0] raised): count it; its granules and the abort word are cleared before the next
// launch.  true: the path's strikes are used up.
static bool xg_give_up(ExchangeGuard &g, int strikes)
{
    g.dirty = true;
    return ++g.aborts >= strikes;
}

// Room for n list elements on the device.  Grown rarely (the host batches a fixed number of trajectories per
// call); the old blocks stay in the context's allocation list until gh_destroy.
static int traj_lists_reserve(gh_ctx *c, TrajLists &tl, int n)
{
    if (n <= tl.cap && tl.L) return GH_OK;
    const size_t cap = (size_t)std::max(n, 32), M = (size_t)c->M;
    tl.L = tl.accepted = tl.chain = nullptr;
    tl.p0s = tl.us = tl.out5s = tl.xacc = nullptr;
    TRY(dalloc(c, &tl.L, cap));
    TRY(dalloc(c, &tl.chain, cap));
    TRY(dalloc(c, &tl.accepted, cap));
    TRY(dalloc(c, &tl.p0s, cap * M, false));
    TRY(dalloc(c, &tl.us, cap));
    TRY(dalloc(c, &tl.out5s, cap * 5));
    TRY(dalloc(c, &tl.xacc, cap * M, false));
    tl.cap = (int)cap;
    return GH_OK;
}

// Pinned staging for `rows` momentum rows.
static int traj_lists_stage(gh_ctx *c, TrajLists &tl, int rows)
{
    const size_t M = (size_t)c->M;
    if ((size_t)rows * M <= tl.h_stage_n) return GH_OK;
    if (tl.h_stage) HIPCHK(c, hipHostFree(tl.h_stage));
    tl.h_stage = nullptr;
    tl.h_stage_n = (size_t)std::max(rows, 32) * M;
    HIPCHK(c, hipHostMalloc((void **)&tl.h_stage, tl.h_stage_n * sizeof(double)));
    return GH_OK;
}

static void traj_lists_free(TrajLists &tl)
{
    if (tl.h_stage) hipHostFree(tl.h_stage);
    if (tl.h_xstage) hipHostFree(tl.h_xstage);
    tl.h_stage = tl.h_xstage = nullptr;
    tl.h_stage_n = tl.h_xstage_n = 0;
}

// The K momentum rows (p0flat: adjacent; otherwise p0rows[k]: where each lies), variates and lengths of a launch
// into tl's device lists, on the context's stream.  Rows inside a block of gh_pinned_alloc go straight from where
// they lie, adjacent ones in one copy (a sampler drawing into a ring of such rows: one or two copies per chain);
// the others are gathered into ONE pinned staging buffer first (a few host threads: 6 MB at C1 with 16 chains x 8
// trajectories) -- 128 separate copies of pageable rows cost more than the kernel they feed.
static int traj_upload(gh_ctx *c, TrajLists &tl, int K, const double *p0flat, const double *const *p0rows, const double *us,
                       const int *L)
{
    const size_t M = (size_t)c->M;
    TRY(traj_lists_stage(c, tl, K));
    if (K <= 0) return GH_OK;
    std::vector<const double *> src((size_t)K);
    for (int k = 0; k < K; ++k) src[(size_t)k] = p0flat ? p0flat + (size_t)k * M : p0rows[(size_t)k];
    const RowCopyPlan plan = row_copy_plan(src.data(), K, M, c->pinned.data(), c->pinned.size());
    tl.rows_direct += K - plan.n_staged;
    tl.rows_staged += plan.n_staged;
    if (plan.n_staged > 0)
        rows_gather(tl.h_stage, src.data(), plan.direct.data(), K, M,
                    (size_t)plan.n_staged * M * sizeof(double) >= ((size_t)1 << 20) ? std::min(4, K) : 1);
    int k0 = 0;
    for (int k1 : plan.run_end) {
        const double *from = plan.direct[(size_t)k0] ? src[(size_t)k0] : tl.h_stage + (size_t)k0 * M;
        HIPCHK(c, hipMemcpyAsync(tl.p0s + (size_t)k0 * M, from, (size_t)(k1 - k0) * M * sizeof(double), hipMemcpyHostToDevice,
                                 c->stream));
        k0 = k1;
    }
    HIPCHK(c, hipMemcpyAsync(tl.us, us, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tl.L, L, (size_t)K * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return GH_OK;
}

// While profiling is on: an event in front of and one behind a persistent launch, and the launch's time and
// evaluations into the context's totals once it is known to have finished without giving up (the caller's
// synchronisation point lies in between).
static int prof_launch_mark(gh_ctx *c, hipEvent_t ev)
{
    if (c->prof) HIPCHK(c, hipEventRecord(ev, c->stream));
    return GH_OK;
}

static int prof_launch_end(gh_ctx *c, hipEvent_t ev0, hipEvent_t ev1, int64_t evals)
{
    if (!c->prof) return GH_OK;
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, ev0, ev1));
    c->prof_ms_acc += t;
    c->prof_res_evals += evals;
    return GH_OK;
}

// The Metropolis test of a finished trajectory (hmc.py:158-177).  pp0 / pp1: |p|^2 at its start / end; scal: the
// proposal's scalars as the finishing kernels leave them (data, regulariser, total); U: the chain's current
// potentials (total, data, regulariser), replaced on acceptance.  out5: U of the state the chain is left in, H of
// the current state and of the proposal.
static bool metropolis_step(double pp0, double pp1, const double *scal, double u, double U[3], double out5[5])
{
    const double Unew[3] = {scal[2], scal[0], scal[1]};
    const double Hcur = 0.5 * pp0 + U[0];
    const double Hnew = 0.5 * pp1 + Unew[0];
    const bool acc = (Hnew < Hcur) || (u < std::exp(-(Hnew - Hcur)));
    if (acc) memcpy(U, Unew, sizeof Unew);
    memcpy(out5, U, sizeof Unew);
    out5[3] = Hcur;
    out5[4] = Hnew;
    return acc;
}

static int h2d(gh_ctx *c, double *dst, const double *src, size_t n)
{
    HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // caller-owned pageable memory: do not outlive the call
    return GH_OK;
}

static int d2h(gh_ctx *c, double *dst, const double *src, size_t n)
{
    HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GH_OK;
}
