// libgravhmc host side: the trajectory feeder of one chain on the sweep path.  Included once by gravhmc.hip.
//
// While a feeder is open on a context two library threads do what Engine.run_chain's Python loop did between two
// gh_chain_run calls: one draws the reference's stream a trajectory at a time (gh_rng_draw_trajectories) into a
// ring of page-locked rows, the other runs chain_trajectory_impl / chain_accept_row from those rows exactly as
// gh_chain_run's loop does -- the row after the one that runs is its look-ahead, obtained LATE (P0Next::late), so it
// need not be drawn when the trajectory starts.  The caller takes results from a queue (gh_chain_feed_next).  The
// waiting of the three is host_feedq.h; the device sees the stream operations it always saw.
#pragma once

#include "host_feedq.h"

struct gh_feed {
    ghfeed::Feeder q;
    // kept with the context between opens (page-locking tens of MB costs milliseconds): momentum rows, model rows
    double *rows_h = nullptr, *xrows_h = nullptr;
    int rows = 0, xslots = 0;
    std::vector<hipEvent_t> x_ev;  // per result slot: the copy of the accepted model into its row
    // what the open feeder runs
    gh_rng *rng = nullptr;
    std::vector<int> plan;
    std::vector<double> sigma_vec;
    int Lmin = 0, Lmax = 0, slots = 0;
    double sigma = 1.0, dt = 0.0;
    int64_t stop_at = 0, record_from = 0;
    bool want_x = false;
    ghfeed::Stats last;  // counters of the feeder that ran last, and what it drew and ran
    int64_t last_drawn = 0, last_run = 0;
};

static void feed_free(gh_ctx *c)
{
    gh_feed *f = c->feed;
    if (!f) return;
    for (hipEvent_t e : f->x_ev) hipEventDestroy(e);
    if (f->rows_h) hipHostFree(f->rows_h);
    if (f->xrows_h) hipHostFree(f->xrows_h);
    delete f;
    c->feed = nullptr;
}

static int feed_rows_default(int64_t M)
{
    const int64_t r = ((int64_t)32 << 20) / (8 * std::max<int64_t>(1, M));
    return std::max(3, env_int("GRAVHMC_FEED_ROWS", (int)std::min<int64_t>(64, std::max<int64_t>(4, r))));
}

// One trajectory of the reference's stream into `row`: L (unless the plan gives it), randn(M) * sigma, rand().
// A vector sigma is one multiply per entry after a draw with sigma = 1: the bits of p0s *= sigma_vec.
static int feed_draw_row(gh_rng *rng, const int *plan, int64_t k, int Lmin, int Lmax, double sigma, const double *sigma_vec,
                         int64_t M, double *row, int *L, double *u)
{
#pragma clang fp contract(off)
    const int rc = gh_rng_draw_trajectories(rng, 1, plan ? 0 : Lmin, plan ? 0 : Lmax, M, sigma_vec ? 1.0 : sigma, L, row, u);
    if (rc != GH_OK) return rc;
    if (plan) *L = plan[k];
    if (sigma_vec)
        for (int64_t i = 0; i < M; ++i) row[i] *= sigma_vec[i];
    return GH_OK;
}

static int feed_check_stream(const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit, int64_t *total)
{
    if (plan_L) {
        if (n_plan < 0) return GH_ERR_ARG;
        for (int64_t i = 0; i < n_plan; ++i)
            if (plan_L[i] < 1) return GH_ERR_ARG;
        *total = limit >= 0 ? std::min(limit, n_plan) : n_plan;
    } else {
        if (Lmin < 1 || Lmax < Lmin) return GH_ERR_ARG;
        *total = limit >= 0 ? limit : -1;
    }
    return GH_OK;
}

extern "C" {

int gh_chain_feed_usable(gh_ctx *c, int *usable)
{
    if (!c || !usable) return fail(c, GH_ERR_ARG, "gh_chain_feed_usable: null pointer");
    GH_FEED_GUARD(c);
    *usable = 0;
    if (!c->chain_ready || c->sh.kind != 0 || env_int("GRAVHMC_CHAIN_FEED", 1) == 0) return GH_OK;
    // (where gh_chain_run has one persistent launch for a batch of trajectories, batches are what it wants)
    if (lonres_usable(c) || resident_usable(c)) return GH_OK;
    *usable = 1;
    return GH_OK;
}

static int feed_open_impl(gh_ctx *c, gh_rng *rng, const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit,
                          double sigma, const double *sigma_vec, double dt, int64_t stop_at_accepts, int64_t record_from,
                          int want_x)
{
    TRY(need(c, c->chain_ready, "gh_chain_feed_open: call gh_chain_init first"));
    int usable = 0;
    TRY(gh_chain_feed_usable(c, &usable));
    if (!usable) return fail(c, GH_ERR_ARG, "gh_chain_feed_open: this context's chain does not run on the sweep path (gh_chain_feed_usable)");
    int64_t total = -1;
    if (feed_check_stream(plan_L, n_plan, Lmin, Lmax, limit, &total) != GH_OK)
        return fail(c, GH_ERR_ARG, "gh_chain_feed_open: lengths must be >= 1, Lmax >= Lmin, the plan not negative");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t M = c->M;
    const int rows = feed_rows_default(M);
    if (!c->feed) c->feed = new gh_feed();
    gh_feed *f = c->feed;
    if (f->rows != rows) {
        if (f->rows_h) HIPCHK(c, hipHostFree(f->rows_h));
        f->rows_h = nullptr;
        f->rows = 0;
        HIPCHK(c, hipHostMalloc((void **)&f->rows_h, (size_t)rows * (size_t)M * sizeof(double)));
        f->rows = rows;
    }
    const int xslots = std::max(2, std::min(16, rows / 2));
    if (want_x && f->xslots != xslots) {
        if (f->xrows_h) HIPCHK(c, hipHostFree(f->xrows_h));
        f->xrows_h = nullptr;
        f->xslots = 0;
        HIPCHK(c, hipHostMalloc((void **)&f->xrows_h, (size_t)xslots * (size_t)M * sizeof(double)));
        f->xslots = xslots;
    }
    f->slots = want_x ? xslots : 64;
    while ((int)f->x_ev.size() < f->slots) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        f->x_ev.push_back(e);
    }
    f->rng = rng;
    f->plan.assign(plan_L ? plan_L : nullptr, plan_L ? plan_L + n_plan : nullptr);
    f->sigma_vec.assign(sigma_vec ? sigma_vec : nullptr, sigma_vec ? sigma_vec + M : nullptr);
    const bool planned = plan_L != nullptr, vec = sigma_vec != nullptr;
    f->Lmin = Lmin;
    f->Lmax = Lmax;
    f->sigma = sigma;
    f->dt = dt;
    f->stop_at = stop_at_accepts;
    f->record_from = record_from;
    f->want_x = want_x != 0;
    // already there, as gh_chain_run: nothing is drawn, nothing runs
    if (stop_at_accepts > 0 && c->accept_count >= stop_at_accepts) total = 0;

    ghfeed::Hooks h;
    h.draw = [f, M, planned, vec](int64_t k, int row, int *L, double *u, std::string &err) -> int {
        const int rc = feed_draw_row(f->rng, planned ? f->plan.data() : nullptr, k, f->Lmin, f->Lmax, f->sigma,
                                     vec ? f->sigma_vec.data() : nullptr, M, f->rows_h + (size_t)row * (size_t)M, L, u);
        if (rc != GH_OK) err = "gh_rng_draw_trajectories failed";
        return rc;
    };
    h.run = [c, f, M](int64_t, int row, int L, double u, int slot, ghfeed::RunCtl &ctl, int *accepted, double out5[5],
                      std::string &err) -> int {
        struct Late {
            gh_feed *f;
            ghfeed::RunCtl *ctl;
            int64_t M;
        } late{f, &ctl, M};
        P0Next nx;
        nx.user = &late;
        nx.late = [](void *user) -> const double * {
            Late *l = static_cast<Late *>(user);
            const int r = l->ctl->next_row();
            return r < 0 ? nullptr : l->f->rows_h + (size_t)r * (size_t)l->M;
        };
        auto body = [&]() -> int {
            TRY(chain_trajectory_impl(c, f->rows_h + (size_t)row * (size_t)M, f->dt, L, u, nx, accepted, out5));
            if (*accepted) {
                double *x_out = f->want_x ? f->xrows_h + (size_t)slot * (size_t)M : nullptr;
                TRY(chain_accept_row(c, c, c->xb[c->xcur], f->record_from, x_out));
                if (x_out) HIPCHK(c, hipEventRecord(f->x_ev[(size_t)slot], c->stream));
                if (f->stop_at > 0 && c->accept_count >= f->stop_at) ctl.stop = true;
            }
            return GH_OK;
        };
        const int rc = body();
        if (rc != GH_OK) err = c->err;
        return rc;
    };
    h.drain = [c](std::string &err) -> int {
        auto body = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return GH_OK;
        };
        const int rc = body();
        if (rc != GH_OK) err = c->err;
        return rc;
    };
    ghfeed::Options o;
    o.rows = rows;
    o.slots = f->slots;
    o.total = total;
    o.test_fail_thread = env_int("GRAVHMC_FEED_TEST_FAIL_THREAD", -1);
    std::string err;
    c->feed_open.store(1, std::memory_order_release);
    const int rc = f->q.open(o, std::move(h), GH_ERR_ARG, err);
    if (rc != GH_OK) {
        c->feed_open.store(0, std::memory_order_release);
        return fail(c, rc, "gh_chain_feed_open: %s", err.c_str());
    }
    return GH_OK;
}

int gh_chain_feed_open(gh_ctx *c, gh_rng *rng, const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit,
                       double sigma, const double *sigma_vec, double dt, int64_t stop_at_accepts, int64_t record_from,
                       int want_x)
{
    if (!c || !rng) return fail(c, GH_ERR_ARG, "gh_chain_feed_open: null pointer");
    GH_FEED_GUARD(c);
    try {
        return feed_open_impl(c, rng, plan_L, n_plan, Lmin, Lmax, limit, sigma, sigma_vec, dt, stop_at_accepts, record_from,
                              want_x);
    } catch (const std::exception &e) {
        // (no exception crosses the C ABI; Feeder::open has joined whatever it had started)
        c->feed_open.store(0, std::memory_order_release);
        return fail(c, GH_ERR_NOMEM, "gh_chain_feed_open: %s", e.what());
    }
}

// Both threads joined: the context is the caller's again, the feeder's error text becomes the context's.
static int feed_end(gh_ctx *c, int64_t *drawn, int64_t *run)
{
    gh_feed *f = c->feed;
    int64_t a = 0, b = 0;
    std::string err;
    const int rc = f->q.close(&a, &b, err);
    f->last = f->q.stats();
    f->last_drawn = a;
    f->last_run = b;
    c->feed_open.store(0, std::memory_order_release);
    if (drawn) *drawn = a;
    if (run) *run = b;
    if (rc != GH_OK) return fail(c, rc, "chain feeder: %s", err.c_str());
    return GH_OK;
}

int gh_chain_feed_next(gh_ctx *c, int max_rows, int timeout_ms, int *L, int *accepted, double *out5s, double *xs, int *n,
                       int *finished)
{
    if (!c || max_rows < 1 || !L || !accepted || !out5s || !n || !finished) return GH_ERR_ARG;
    if (!c->feed_open.load(std::memory_order_acquire)) return fail(c, GH_ERR_ARG, "gh_chain_feed_next: no feeder is open");
    gh_feed *f = c->feed;
    ghfeed::Result res[64];
    std::string err;
    if (xs && f->want_x && hipSetDevice(c->device) != hipSuccess) return GH_ERR_HIP;
    const int rc = f->q.next(std::min(max_rows, 64), timeout_ms, res, n, finished, err);
    const size_t M = (size_t)c->M;
    for (int i = 0; i < *n; ++i) {
        const ghfeed::Result &r = res[i];
        L[i] = r.L;
        accepted[i] = r.accepted;
        memcpy(out5s + 5 * (size_t)i, r.out5, sizeof r.out5);
        if (xs && f->want_x && r.accepted) {
            // (only this slot's event is touched here; the context's own state stays the runner's)
            if (hipEventSynchronize(f->x_ev[(size_t)r.slot]) != hipSuccess) return GH_ERR_HIP;
            memcpy(xs + (size_t)i * M, f->xrows_h + (size_t)r.slot * M, M * sizeof(double));
        }
    }
    if (rc != GH_OK) {
        // the runner has ended with an error: join, so that its text can become the context's
        const int rc2 = feed_end(c, nullptr, nullptr);
        return rc2 != GH_OK ? rc2 : fail(c, rc, "chain feeder: %s", err.c_str());
    }
    return GH_OK;
}

int gh_chain_feed_close(gh_ctx *c, int64_t *drawn, int64_t *run)
{
    if (!c) return GH_ERR_ARG;
    if (drawn) *drawn = 0;
    if (run) *run = 0;
    if (!c->feed) return GH_OK;
    if (c->feed_open.load(std::memory_order_acquire)) return feed_end(c, drawn, run);
    // (ended by an error that gh_chain_feed_next has returned: what that feeder drew and ran)
    if (drawn) *drawn = c->feed->last_drawn;
    if (run) *run = c->feed->last_run;
    return GH_OK;
}

int gh_chain_feed_stats(gh_ctx *c, double *runner_wait_draw_s, double *drawer_wait_row_s, double *runner_wait_queue_s, int *rows)
{
    if (!c) return GH_ERR_ARG;
    ghfeed::Stats s;
    if (c->feed) s = c->feed_open.load(std::memory_order_acquire) ? c->feed->q.stats() : c->feed->last;
    if (runner_wait_draw_s) *runner_wait_draw_s = s.runner_wait_draw_s;
    if (drawer_wait_row_s) *drawer_wait_row_s = s.drawer_wait_row_s;
    if (runner_wait_queue_s) *runner_wait_queue_s = s.runner_wait_queue_s;
    if (rows) *rows = c->feed ? c->feed->rows : 0;
    return GH_OK;
}

// The drawer and the queue of the feeder with a host stub in place of the runner: no context, no GPU.  Per trajectory
// k < max_out: L, u, probe[4 k ..] = first, middle and last entry of the momentum and the sum of the row in order,
// look[k] = whether a look-ahead row was handed over.  n_out: trajectories run; drawn: taken from the stream.
int gh_debug_feed_dry_run(gh_rng *rng, const int *plan_L, int64_t n_plan, int Lmin, int Lmax, int64_t limit, double sigma,
                          const double *sigma_vec, int64_t M, int rows, int64_t max_out, int *out_L, double *out_u,
                          double *out_probe, int *out_look, int64_t *n_out, int64_t *drawn)
{
    if (!rng || M < 1 || rows < 3 || max_out < 0 || !out_L || !out_u || !out_probe || !out_look || !n_out || !drawn)
        return GH_ERR_ARG;
    int64_t total = -1;
    if (feed_check_stream(plan_L, n_plan, Lmin, Lmax, limit, &total) != GH_OK || total < 0 || total > max_out) return GH_ERR_ARG;
    try {
        std::vector<double> ring((size_t)rows * (size_t)M);
        ghfeed::Hooks h;
        h.draw = [&](int64_t k, int row, int *L, double *u, std::string &err) -> int {
            const int rc = feed_draw_row(rng, plan_L, k, Lmin, Lmax, sigma, sigma_vec, M, ring.data() + (size_t)row * (size_t)M, L, u);
            if (rc != GH_OK) err = "gh_rng_draw_trajectories failed";
            return rc;
        };
        h.run = [&](int64_t k, int row, int L, double u, int, ghfeed::RunCtl &ctl, int *accepted, double out5[5], std::string &) -> int {
#pragma clang fp contract(off)
            const double *p = ring.data() + (size_t)row * (size_t)M;
            double s = 0.0;
            for (int64_t i = 0; i < M; ++i) s += p[i];
            out_L[k] = L;
            out_u[k] = u;
            out_probe[4 * k] = p[0];
            out_probe[4 * k + 1] = p[M / 2];
            out_probe[4 * k + 2] = p[M - 1];
            out_probe[4 * k + 3] = s;
            out_look[k] = ctl.next_row() >= 0 ? 1 : 0;
            *accepted = 1;
            for (int i = 0; i < 5; ++i) out5[i] = 0.0;
            return GH_OK;
        };
        ghfeed::Options o;
        o.rows = rows;
        o.slots = 4;
        o.total = total;
        ghfeed::Feeder q;
        std::string err;
        int rc = q.open(o, std::move(h), GH_ERR_ARG, err);
        if (rc != GH_OK) return rc;
        ghfeed::Result res[4];
        for (int fin = 0; !fin && rc == GH_OK;) {
            int n = 0;
            rc = q.next(4, -1, res, &n, &fin, err);
        }
        const int rc2 = q.close(drawn, n_out, err);
        return rc != GH_OK ? rc : rc2;
    } catch (const std::exception &) {
        return GH_ERR_NOMEM;
    }
}

}  // extern "C"
