// Stand-alone program over csrc/host_layout.h (the single chain's work buffers and the offsets inside them): built
// and run by tests/test_work_layout_host.py under the address and undefined-behaviour sanitizers.  For every shape
// the regions of StateSet::part and of h_scal must be disjoint and end within size(), and the values must equal
// the table below, which is written out by hand from the expressions of the revision before host_layout.h existed
// (csrc/host_eval.h of "Pin reused contexts to the CPU oracle"; "ew:N" is line N of that file, in ensure_work).
//
//   slab rows   ew:447  lonsym_one_row(c) ? 1 : c->n_panels > 1 ? std::max(c->grid, 128) : c->grid
//   slab2 rows  ew:448  if (c->grid > 64) max(1, min(16, 16384 / c->ld))
//   n_dpart     ew:454  (c->ld + 31) / 32
//   part joint  ew:460  2 * n_dpart + 3 * ((store_cells(c) + 255) / 256)
//   bsum        ew:467  max(mc.n * max(c->grid, 128), lonsym_on(c) ? lonsym_classes(c) : 0)
//   part        ew:473, ew:480  n_dpart + (c->M + 255) / 256 + (c->mvi ? 3 + (store_cells(c) + 255) / 256 : 0)
//   one launch  ew:475  c->ld >= 2048 && ((c->TW > 1 && c->n_panels == 1 && !c->mf) || lonsym_on(c)) && GRAVHMC_EPILOGUE1
//   dsum        ew:476  max(max(c->grid, 128), lonsym_on(c) ? lonsym_classes(c) : 0)
//   n_regpart   ew:490  reg_props(c) * ((c->M / reg_props(c) + 255) / 256)
//   pp0         ew:491  min(1024, (c->M + 255) / 256)
//   pp          ew:494  c->n_teams
//   h_scal      ew:509  16 + 2 * c->n_teams + 2 * c->n_pp0
//   R in part   finalize :308, :335  o.part + c->n_dpart;  finalize_joint :139  o.part + 2 * c->n_dpart + h * nrb
//   coupling    finalize :355  o.part + c->n_dpart + c->n_regpart;  finalize_joint :171  o.part + 2 * c->n_dpart + 2 * nrb
//   h_scal use  host_chain.h :151-164  h, h + 4, h + 8, h + 16, h + 16 + 2 * nt, h + 16 + 2 * nt + c->n_pp0
#include "../gravinv3dhmc_amd/csrc/host_layout.h"

#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            g_failed += 1;                                   \
        }                                                    \
    } while (0)

struct Expect {
    int64_t slab_rows, slab2_rows, pp, pp0, dsum, bsum, n_dpart, n_regpart, reg_blocks, form, part_size, reg0, coupling, h_size;
};

struct Case {
    const char *name;
    WorkShape s;
    Expect e;
};

static WorkShape shape(int64_t M, int64_t ld, int grid, int n_teams, int TW = 8, int n_panels = 1)
{
    WorkShape s;
    s.M = M;
    s.ld = ld;
    s.N = ld;
    s.grid = grid;
    s.n_teams = n_teams;
    s.TW = TW;
    s.n_panels = n_panels;
    s.store_cells = M;
    return s;
}

static WorkShape mvi(int64_t m, int64_t ld)
{
    WorkShape s = shape(3 * m, ld, 32, 32);
    s.mvi = true;
    s.store_cells = m;
    return s;
}

static WorkShape joint(int64_t m)
{
    WorkShape s = shape(2 * m, 1024, 16, 16);
    s.joint = true;
    s.store_cells = m;
    return s;
}

static WorkShape multi(int blocks, int64_t ld)
{
    WorkShape s = shape(3000, ld, 40, 40, 4);
    s.mc_n = blocks;
    return s;
}

static WorkShape lonsym_row(int classes, int mc_n)
{
    WorkShape s = shape(8000, 4096, 90, 90, 0);
    s.mf = s.lonsym_on = s.lonsym_one_row = true;
    s.lonsym_classes = classes;
    s.mc_n = mc_n;
    return s;
}

static WorkShape rows_sharded(int n_teams)
{
    WorkShape s = shape(1200, 2048, 4, n_teams);
    s.shard_rows = true;
    return s;
}

static WorkShape no_epilogue1(WorkShape s)
{
    s.epilogue1 = false;
    return s;
}

enum { NONE = WORK_PART_NONE, PLAIN = WORK_PART_PLAIN, MVI = WORK_PART_MVI, MULTI = WORK_PART_MULTI, JOINT = WORK_PART_JOINT };

// expected: slab, slab2, pp, pp0, dsum, bsum, n_dpart, n_regpart, R blocks per property, form, part, R at, coupling at, h_scal
static const Case CASES[] = {
    // below and at the ld >= 2048 threshold of the one-launch epilogue (ew:475); grid 64: no slab2 (ew:448)
    {"plain ld 2032", shape(5000, 2032, 64, 64), {64, 0, 64, 20, 0, 0, 64, 20, 20, NONE, 0, 64, 84, 184}},
    {"plain ld 2048", shape(5000, 2048, 64, 64), {64, 0, 64, 20, 128, 0, 64, 20, 20, PLAIN, 84, 64, 84, 184}},
    {"plain ld 2048, GRAVHMC_EPILOGUE1=0", no_epilogue1(shape(5000, 2048, 64, 64)), {64, 0, 64, 20, 0, 0, 64, 20, 20, NONE, 0, 64, 84, 184}},
    {"plain ld 2048, one-wave teams", shape(5000, 2048, 64, 256, 1), {64, 0, 256, 20, 0, 0, 64, 20, 20, NONE, 0, 64, 84, 568}},
    // past the grid > 64 threshold of the two-stage reduction: 16384 / 2048 = 8 segments, 16384 / 1008 = 16
    {"grid 65, ld 2048", shape(5000, 2048, 65, 65), {65, 8, 65, 20, 128, 0, 64, 20, 20, PLAIN, 84, 64, 84, 186}},
    {"grid 65, ld 1008", shape(5000, 1008, 65, 65), {65, 16, 65, 20, 0, 0, 32, 20, 20, NONE, 0, 32, 52, 186}},
    {"grid 200, ld 2048", shape(60000, 2048, 200, 200), {200, 8, 200, 235, 200, 0, 64, 235, 235, PLAIN, 299, 64, 299, 886}},
    // row panels: max(grid, 128) slab rows for the team sweep, 16384 / 20000 = 0 -> 1 segment, no one-launch form
    {"2 panels", shape(40000, 20000, 100, 157, 16, 2), {128, 1, 157, 157, 0, 0, 625, 157, 157, NONE, 0, 625, 782, 644}},
    // magnetization vector, m cells per property, M = 3 m: R's blocks per property, 3 ceil(m / 256), against the
    // ceil(3 m / 256) + 3 the buffer has room for; the amplitude term's ceil(m / 256) behind them
    {"mvi 255", mvi(255, 2112), {32, 0, 32, 3, 128, 0, 66, 3, 1, MVI, 73, 66, 69, 86}},
    {"mvi 256", mvi(256, 2112), {32, 0, 32, 3, 128, 0, 66, 3, 1, MVI, 73, 66, 69, 86}},
    {"mvi 257", mvi(257, 2112), {32, 0, 32, 4, 128, 0, 66, 6, 2, MVI, 75, 66, 72, 88}},
    {"mvi 300", mvi(300, 2112), {32, 0, 32, 4, 128, 0, 66, 6, 2, MVI, 75, 66, 72, 88}},
    {"mvi 300, ld 608 (finish_kernel with amppart)", mvi(300, 608), {32, 0, 32, 4, 0, 0, 19, 6, 2, NONE, 0, 19, 25, 88}},
    // joint, m cells per block, M = 2 m, 1024 rows per block: |r|^2 of gz, of tf, R of gz, of tf, Phi
    {"joint 256", joint(256), {16, 0, 16, 2, 0, 0, 32, 2, 1, JOINT, 67, 64, 66, 52}},
    {"joint 257", joint(257), {16, 0, 16, 3, 0, 0, 32, 4, 2, JOINT, 70, 64, 68, 54}},
    // multi-component, b row blocks: b * max(grid, 128) sums
    {"multi 1", multi(1, 208), {40, 0, 40, 12, 0, 128, 7, 12, 12, MULTI, 19, 7, 19, 120}},
    {"multi 3", multi(3, 608), {40, 0, 40, 12, 0, 384, 19, 12, 12, MULTI, 31, 19, 31, 120}},
    {"multi 11", multi(11, 2208), {40, 0, 40, 12, 0, 1408, 69, 12, 12, MULTI, 81, 69, 81, 120}},
    // shift-invariant store, one finished slab row, more classes than max(grid, 128)
    {"lonsym one row, 300 classes", lonsym_row(300, 0), {1, 4, 90, 32, 300, 0, 128, 32, 32, PLAIN, 160, 128, 160, 260}},
    {"lonsym one row, 3 blocks, 600 classes", lonsym_row(600, 3), {1, 4, 90, 32, 0, 600, 128, 32, 32, MULTI, 160, 128, 160, 260}},
    {"lonsym one row, 3 blocks, 60 classes", lonsym_row(60, 3), {1, 4, 90, 32, 0, 384, 128, 32, 32, MULTI, 160, 128, 160, 260}},
    // row shards of 1200 cells: vec_update_kernel leaves ceil(1200 / 256) = 5 partials
    {"row shards, 4 teams", rows_sharded(4), {4, 0, 4, 5, 128, 0, 64, 5, 5, PLAIN, 69, 64, 69, 34}},
    {"row shards, 8 teams", rows_sharded(8), {4, 0, 8, 5, 128, 0, 64, 5, 5, PLAIN, 69, 64, 69, 42}},
};

typedef std::vector<std::pair<int64_t, int64_t>> Regions;  // [begin, end)

static void check_regions(const char *name, const char *buffer, const Regions &r, int64_t size)
{
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].first >= 0 && r[i].first <= r[i].second, "%s: %s region %zu is [%lld, %lld)", name, buffer, i,
              (long long)r[i].first, (long long)r[i].second);
        CHECK(r[i].second <= size, "%s: %s region %zu ends at %lld, size %lld", name, buffer, i, (long long)r[i].second,
              (long long)size);
        for (size_t j = 0; j < i; ++j)
            CHECK(r[i].first >= r[j].second || r[j].first >= r[i].second, "%s: %s regions %zu and %zu overlap", name, buffer, j, i);
    }
}

static void check_case(const Case &cs)
{
    const WorkLayout w = work_layout(cs.s);
    const Expect &e = cs.e;
    const int64_t got[] = {w.slab_rows, w.slab2_rows, w.pp, w.pp0, w.dsum, w.bsum, w.n_dpart, w.n_regpart, w.reg_blocks,
                           w.part_form, w.size(), w.reg(0), w.coupling(), (int64_t)w.h_size()};
    const int64_t want[] = {e.slab_rows, e.slab2_rows, e.pp, e.pp0, e.dsum, e.bsum, e.n_dpart, e.n_regpart, e.reg_blocks,
                            e.form, e.part_size, e.reg0, e.coupling, e.h_size};
    static const char *const names[] = {"slab rows", "slab2 rows", "pp", "pp0", "dsum", "bsum", "n_dpart", "n_regpart", "R blocks",
                                        "form", "part size", "R offset", "coupling offset", "h_scal size"};
    for (size_t i = 0; i < sizeof got / sizeof got[0]; ++i)
        CHECK(got[i] == want[i], "%s: %s is %lld, the table has %lld", cs.name, names[i], (long long)got[i], (long long)want[i]);
    CHECK(w.props == (cs.s.joint ? 2 : cs.s.mvi ? 3 : 1), "%s: props %d", cs.name, w.props);
    CHECK(w.n_regpart == w.props * w.reg_blocks, "%s: n_regpart %d, %d x %d blocks", cs.name, w.n_regpart, w.props, w.reg_blocks);
    CHECK(w.gbuf == (cs.s.n_panels > 1 || cs.s.shard_rows), "%s: gbuf", cs.name);
    CHECK(w.amppart == (cs.s.mvi ? w.reg_blocks : 0), "%s: amppart %lld", cs.name, (long long)w.amppart);
    if (w.part_form != WORK_PART_NONE) {
        // with the coupling term (joint: cross-gradient; magnetization vector: amplitude) and without it
        Regions r;
        for (int h = 0; h < (cs.s.joint ? 2 : 1); ++h) r.push_back({w.r2(h), w.r2(h) + w.n_dpart});
        for (int h = 0; h < w.props; ++h) r.push_back({w.reg(h), w.reg(h) + w.reg_blocks});
        check_regions(cs.name, "part", r, w.size());
        CHECK(r.back().second == w.coupling(), "%s: the coupling term's partials do not follow R's", cs.name);
        if (w.props > 1) {
            r.push_back({w.coupling(), w.coupling() + w.reg_blocks});
            check_regions(cs.name, "part with the coupling", r, w.size());
        }
    }
    const Regions h = {{(int64_t)w.h_state(), (int64_t)w.h_state() + 4}, {(int64_t)w.h_spec(), (int64_t)w.h_spec() + 4},
                       {(int64_t)w.h_phi(), (int64_t)w.h_phi() + 1},     {(int64_t)w.h_pp(), (int64_t)w.h_pp() + 2 * w.pp},
                       {(int64_t)w.h_pp0(), (int64_t)w.h_pp0() + w.pp0}, {(int64_t)w.h_pn0(), (int64_t)w.h_pn0() + w.pp0}};
    check_regions(cs.name, "h_scal", h, (int64_t)w.h_size());
    // a layout holds what it asks for itself
    int64_t need = 0, have = 0;
    CHECK(work_exceeds(w, work_demand_of(w), &need, &have) == nullptr, "%s: the layout does not fit itself", cs.name);
}

// demands against an allocated layout: what the producers state at plan time
static void check_demands()
{
    int64_t need = 0, have = 0;
    WorkDemand pp5;
    pp5.pp = 5;  // row shards of 1200 cells
    const char *what = work_exceeds(work_layout(rows_sharded(4)), pp5, &need, &have);
    CHECK(what && !std::strcmp(what, "|p|^2 partials") && need == 5 && have == 4, "row shards on 4 teams: %s %lld %lld",
          what ? what : "(fits)", (long long)need, (long long)have);
    CHECK(!work_exceeds(work_layout(rows_sharded(8)), pp5, &need, &have), "row shards on 8 teams do not fit");
    // the team sweep's 8 * tpx <= 32 rows and partials under row panels
    WorkDemand team;
    team.slab_rows = team.pp = 32;
    CHECK(!work_exceeds(work_layout(shape(40000, 20000, 100, 157, 16, 2)), team, &need, &have), "team sweep does not fit");
    // a grid that grew past the slab
    WorkDemand grown;
    grown.slab_rows = 65;
    what = work_exceeds(work_layout(shape(5000, 2048, 64, 64)), grown, &need, &have);
    CHECK(what && !std::strcmp(what, "slab rows") && need == 65 && have == 64, "65 rows on a slab of 64");
    // more classes than sums; and no sums allocated: none are delivered, nothing to hold
    WorkDemand classes;
    classes.slab_rows = 1;
    classes.dsum = 301;
    what = work_exceeds(work_layout(lonsym_row(300, 0)), classes, &need, &have);
    CHECK(what && !std::strcmp(what, "slab-row sums") && need == 301 && have == 300, "301 classes on 300 sums");
    CHECK(!work_exceeds(work_layout(no_epilogue1(lonsym_row(300, 0))), classes, &need, &have), "sums demanded of a layout without");
}

int main()
{
    for (const Case &cs : CASES) check_case(cs);
    check_demands();
    std::printf("%zu shapes\n", sizeof CASES / sizeof CASES[0]);
    std::printf(g_failed ? "FAILED %d\n" : "ALL OK\n", g_failed);
    return g_failed ? 1 : 0;
}
