// libgravhmc host side: the single chain's work buffers, stated once.  work_layout() is a pure function of the
// context's shape: the capacities ensure_work allocates, the offsets inside StateSet::part (the partials a one-launch
// epilogue leaves) and inside the pinned read-back buffer h_scal.  Free of HIP (tests/work_layout_main.cpp includes
// it alone); included by host_ctx.h.  DESIGN.md section 3 has the table of who writes how much.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

// What the sizes depend on, read from the context by work_shape() (host_eval.h).
struct WorkShape {
    int64_t M = 0, ld = 0, N = 0;
    int grid = 0, n_teams = 0, n_panels = 1, TW = 0;
    bool joint = false, mvi = false;
    int mc_n = 0;             // row blocks of the multi-component store (0: none)
    int64_t store_cells = 0;  // cells of one property (M / 2 joint, M / 3 magnetization-vector, else M)
    bool mf = false;
    bool lonsym_on = false, lonsym_one_row = false;
    int lonsym_classes = 0;
    bool shard_rows = false;
    bool epilogue1 = true;  // GRAVHMC_EPILOGUE1, read by the caller at the first evaluation
};

enum WorkPartForm { WORK_PART_NONE = 0, WORK_PART_PLAIN, WORK_PART_MVI, WORK_PART_MULTI, WORK_PART_JOINT };

struct WorkLayout {
    // ---- capacities, in doubles or rows
    int64_t slab_rows = 0;    // rows of c->ld doubles
    int slab2_rows = 0;       // segments of the two-stage reduction (0: no slab2); each ld (joint: 2 ld) doubles
    int pp = 0, pp0 = 0;      // |p|^2 partials of the final half step (pp_part, ppn_part) / of a fresh momentum
    int64_t dsum = 0;         // sums of the slab rows for the one-launch epilogue (0: none)
    int64_t bsum = 0;         // multi-component store: sums per slab row and row block (0: none)
    int64_t amppart = 0;      // amplitude term's partials where the epilogue keeps none
    bool gbuf = false;        // gradient accumulated over row panels / all-reduced over row shards
    // ---- counts the epilogue launches with
    int n_dpart = 0;          // |r|^2 partials, one per 32 rows
    int n_regpart = 0;        // R partials of all properties
    int reg_blocks = 0;       // R partials of one property
    int props = 1;            // properties stacked in the model vector
    // ---- StateSet::part
    int part_form = WORK_PART_NONE;
    int64_t part_size = 0;
    // |r|^2 partials of block h (joint store: 0 gz, 1 tf; every other store has block 0 alone)
    int64_t r2(int h) const { return (int64_t)h * n_dpart; }
    // R partials of property h, behind the |r|^2 partials of all blocks
    int64_t reg(int h) const { return (int64_t)(part_form == WORK_PART_JOINT ? 2 : 1) * n_dpart + (int64_t)h * reg_blocks; }
    // Phi partials of the coupling term (cross-gradient / amplitude), reg_blocks of them, behind those of R
    int64_t coupling() const { return reg(props); }
    int64_t size() const { return part_size; }
    // ---- h_scal, the pinned read-back buffer
    static constexpr size_t h_state() { return 0; }  // scal[0..3] of the state set read back
    static constexpr size_t h_spec() { return 4; }   // scal[0..3] of the speculative first step's set
    static constexpr size_t h_phi() { return 8; }    // Phi of the coupling term (up to h_pp: spare)
    static constexpr size_t h_pp() { return 16; }    // pp partials, room for pp_part and ppn_part
    size_t h_pp0() const { return h_pp() + 2 * (size_t)pp; }
    size_t h_pn0() const { return h_pp0() + (size_t)pp0; }
    size_t h_size() const { return h_pn0() + (size_t)pp0; }
};

// Every value is the parent revision's expression, quoted with its place (host_eval.h of "Pin reused contexts to
// the CPU oracle", ensure_work unless another function is named).
static inline WorkLayout work_layout(const WorkShape &s)
{
    WorkLayout w;
    const int64_t blocks_M = (s.M + 255) / 256;                  // "(c->M + 255) / 256"
    const int64_t blocks_m = (s.store_cells + 255) / 256;        // "(store_cells(c) + 255) / 256"
    const int teams_cap = std::max(s.grid, 128);                 // "std::max(c->grid, 128)"
    const int classes = s.lonsym_on ? s.lonsym_classes : 0;      // "lonsym_on(c) ? lonsym_classes(c) : 0"
    // :447 "lonsym_one_row(c) ? 1 : c->n_panels > 1 ? std::max(c->grid, 128) : c->grid".  One finished row: the harmonic
    // and wide forms of the shift-invariant store.  Row panels: the team sweep writes a row per team, 8 * tpx <= 32 of
    // them, whatever the panel grid.  Else one row per workgroup of the sweep (grid), which also bounds the folded
    // sweep's workgroups (fold_use), the matrix-free teams' ranges + 1 (mft_plan) and the lattice's chunks.
    w.slab_rows = s.lonsym_one_row ? 1 : s.n_panels > 1 ? teams_cap : s.grid;
    // :448-451 "if (c->grid > 64) slab2_rows = max(1, min(16, 16384 / ld))": segments left for the single-block
    // finish_kernel, as many as keep its read at ~128 KB
    w.slab2_rows = s.grid > 64 ? (int)std::max<int64_t>(1, std::min<int64_t>(16, 16384 / s.ld)) : 0;
    w.n_dpart = (int)((s.ld + 31) / 32);                         // :454 "(c->ld + 31) / 32"
    w.props = s.joint ? 2 : s.mvi ? 3 : 1;                       // reg_props: "c->joint ? 2 : c->mvi ? 3 : 1"
    // :490 "reg_props(c) * (int)((c->M / reg_props(c) + 255) / 256)": the regulariser runs per property
    w.n_regpart = w.props * (int)((s.M / w.props + 255) / 256);
    // finalize_joint :122 "nrb = (store_cells(c) + 255) / 256", finalize :199 "ra.nrb = (ra.M + 255) / 256"
    w.reg_blocks = w.props > 1 ? (int)blocks_m : w.n_regpart;
    // :494-495 "dalloc(&c->pp_part, c->n_teams)": one per team of the sweep, per workgroup of the folded, fused
    // matrix-free and lattice adjoint passes, and per 256 cells for vec_update_kernel (row panels, row shards)
    w.pp = s.n_teams;
    w.pp0 = (int)std::min<int64_t>(1024, blocks_M);              // :491 "std::min<int64_t>(1024, (c->M + 255) / 256)"
    w.gbuf = s.n_panels > 1 || s.shard_rows;                     // :443 "c->n_panels > 1 || shard_rows(c)"
    w.amppart = s.mvi ? blocks_m : 0;                            // :487 "(store_cells(c) + 255) / 256"
    // Magnetization-vector stores: R's blocks are counted per property, 3 ceil(m / 256) <= ceil(3 m / 256) + 2, and
    // the amplitude term's ceil(m / 256) partials follow them.  :473-474 and :480-481, the same expression twice:
    // "n_dpart + (M + 255) / 256 + (c->mvi ? 3 + (store_cells(c) + 255) / 256 : 0)"
    const int64_t part_rows = (int64_t)w.n_dpart + blocks_M + (s.mvi ? 3 + blocks_m : 0);
    if (s.joint) {
        // :460 "2 * n_dpart + 3 * ((store_cells(c) + 255) / 256)": |r|^2 of both blocks, R of both, then Phi
        w.part_form = WORK_PART_JOINT;
        w.part_size = 2 * (int64_t)w.n_dpart + 3 * blocks_m;
    } else if (s.mc_n > 0) {
        // :467-468 "max(mc.n * max(grid, 128), lonsym_on ? classes : 0)": a sum per slab row and row block; on the
        // shift-invariant table the classes' sums, which are the blocks' partials there
        w.part_form = WORK_PART_MULTI;
        w.part_size = part_rows;
        w.bsum = std::max<int64_t>((int64_t)s.mc_n * teams_cap, classes);
    } else if (s.ld >= 2048 && ((s.TW > 1 && s.n_panels == 1 && !s.mf) || s.lonsym_on) && s.epilogue1) {
        // :475-476 "max(max(grid, 128), lonsym_on ? classes : 0)": a sum per slab row of the dense sweep (grid), or
        // per class of the shift-invariant pass
        w.part_form = s.mvi ? WORK_PART_MVI : WORK_PART_PLAIN;
        w.part_size = part_rows;
        w.dsum = std::max<int64_t>(teams_cap, classes);
    }
    return w;
}

// What a producer is about to write: slab rows, sums in dsum (or bsum), pp partials.  0: none of that buffer.
struct WorkDemand {
    int64_t slab_rows = 0, dsum = 0;
    int pp = 0;
};

// The first quantity of `d` that the allocated layout `w` cannot hold (nullptr: it fits), with both figures.  No
// sums allocated (no one-launch epilogue): the producers then deliver none.
static inline const char *work_exceeds(const WorkLayout &w, const WorkDemand &d, int64_t *need, int64_t *have)
{
    const int64_t sums = std::max(w.dsum, w.bsum);
    const struct {
        const char *what;
        int64_t need, have;
    } q[] = {{"slab rows", d.slab_rows, w.slab_rows}, {"slab-row sums", sums > 0 ? d.dsum : 0, sums}, {"|p|^2 partials", d.pp, w.pp}};
    for (const auto &e : q)
        if (e.need > e.have) {
            *need = e.need;
            *have = e.have;
            return e.what;
        }
    return nullptr;
}

// What a context of layout `w` asks of the buffers allocated at its first evaluation.  (slab2 and `part` depend on
// ld, M and the store alone; where they are absent the epilogue takes the forms that do without.)
static inline WorkDemand work_demand_of(const WorkLayout &w)
{
    WorkDemand d;
    d.slab_rows = w.slab_rows;
    d.dsum = std::max(w.dsum, w.bsum);
    d.pp = w.pp;
    return d;
}
