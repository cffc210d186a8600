// Stand-alone program over csrc/host_feedq.h (the waiting of the trajectory feeder) with stub draw and run
// functions: built and run by tests/test_feed_queue_host.py under the thread sanitizer and under the address and
// undefined-behaviour sanitizers.  Every case ends with close() returned (both threads joined) and checks that
// every row was seen whole by its trajectory: the rows are plain memory, so a row reused too early is a data race
// for the one build and a wrong value for both.
#include "../gravinv3dhmc_amd/csrc/host_feedq.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>

using namespace ghfeed;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            g_failed += 1;                                \
        }                                                 \
    } while (0)

static void nap(int us)
{
    if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

struct Case {
    const char *name = "";
    int rows = 3, slots = 2;
    int64_t total = -1;
    int draw_us = 0, run_us = 0, take_us = 0;
    int64_t fail_run_at = -1, fail_draw_at = -1;
    int stop_at_accepts = 0;   // every second trajectory is accepted (k odd)
    int fail_thread = -1;
    int close_when = 0;        // 0: at the end, 1: before the first draw, 2: during a draw, 3: during a run
    int64_t take_limit = -1;   // the caller stops taking after this many results and closes
};

enum { W = 64 };

struct Stub {
    Case cs;
    std::vector<double> rows, xrows;
    std::atomic<int> in_draw{0}, in_run{0}, gate{0};
    int accepts = 0;
    int64_t looks = 0, no_looks = 0;
};

static int64_t run_case(const Case &cs)
{
    const int fails_before = g_failed;
    Stub st;
    st.cs = cs;
    st.rows.assign((size_t)cs.rows * W, -1.0);
    st.xrows.assign((size_t)cs.slots * W, -1.0);
    Hooks h;
    h.draw = [&st](int64_t k, int row, int *L, double *u, std::string &err) -> int {
        st.in_draw.store(1);
        if (st.cs.close_when == 1)
            while (!st.gate.load()) nap(50);  // (the caller closes before anything is drawn)
        if (k == st.cs.fail_draw_at) {
            err = "stub draw failed";
            return 7;
        }
        double *p = st.rows.data() + (size_t)row * W;
        for (int i = 0; i < W; ++i) {
            p[i] = (double)k;
            if (i == W / 2) nap(st.cs.draw_us);
        }
        *L = (int)(k % 5) + 1;
        *u = 0.25 + (double)k;
        st.in_draw.store(0);
        return 0;
    };
    h.run = [&st](int64_t k, int row, int L, double u, int slot, RunCtl &ctl, int *accepted, double out5[5],
                  std::string &err) -> int {
        st.in_run.store(1);
        CHECK(L == (int)(k % 5) + 1 && u == 0.25 + (double)k, "trajectory %lld got L %d u %g", (long long)k, L, u);
        const double *p = st.rows.data() + (size_t)row * W;
        for (int i = 0; i < W; ++i) CHECK(p[i] == (double)k, "row of %lld holds %g before the run", (long long)k, p[i]);
        nap(st.cs.run_us);
        if (k == st.cs.fail_run_at) {
            err = "stub run failed";
            return 9;
        }
        const int nr = ctl.next_row();
        if (nr >= 0) {
            st.looks += 1;
            const double *q = st.rows.data() + (size_t)nr * W;
            for (int i = 0; i < W; ++i) CHECK(q[i] == (double)(k + 1), "look-ahead of %lld holds %g", (long long)k, q[i]);
        } else {
            st.no_looks += 1;
        }
        for (int i = 0; i < W; ++i) CHECK(p[i] == (double)k, "row of %lld holds %g after the run", (long long)k, p[i]);
        *accepted = (int)(k & 1);
        if (*accepted) {
            double *x = st.xrows.data() + (size_t)slot * W;
            for (int i = 0; i < W; ++i) x[i] = (double)k;
            st.accepts += 1;
            if (st.cs.stop_at_accepts > 0 && st.accepts >= st.cs.stop_at_accepts) ctl.stop = true;
        }
        for (int i = 0; i < 5; ++i) out5[i] = (double)k + i;
        st.in_run.store(0);
        return 0;
    };
    std::atomic<int> drained{0};
    h.drain = [&drained](std::string &) -> int {
        drained.fetch_add(1);
        return 0;
    };
    Options o;
    o.rows = cs.rows;
    o.slots = cs.slots;
    o.total = cs.total;
    o.test_fail_thread = cs.fail_thread;
    int64_t taken = 0, drawn = -1, run = -1;
    std::string err;
    {
        Feeder q;
        const int rc = q.open(o, h, 3, err);
        if (cs.fail_thread >= 0) {
            CHECK(rc == 3 && !q.is_open() && !err.empty(), "%s: open with a failing thread returned %d", cs.name, rc);
            st.gate.store(1);
            CHECK(q.close(&drawn, &run, err) == 0 && run == 0, "%s: close after a failed open", cs.name);
            std::printf("ok   %-40s open refused: %s\n", cs.name, err.c_str());
            return 0;
        }
        CHECK(rc == 0, "%s: open returned %d (%s)", cs.name, rc, err.c_str());
        if (cs.close_when == 2)
            while (!st.in_draw.load()) nap(20);
        if (cs.close_when == 3)
            while (!st.in_run.load()) nap(20);
        int rcn = 0;
        if (cs.close_when == 0) {
            Result res[4];
            for (int fin = 0; !fin;) {
                int n = 0;
                rcn = q.next(4, (taken & 1) ? 50 : -1, res, &n, &fin, err);
                for (int i = 0; i < n; ++i) {
                    const Result &r = res[i];
                    CHECK(r.k == taken && r.slot == (int)(taken % cs.slots) && r.L == (int)(taken % 5) + 1 &&
                              r.out5[4] == (double)taken + 4 && r.accepted == (int)(taken & 1),
                          "%s: result %lld out of order (k %lld)", cs.name, (long long)taken, (long long)r.k);
                    nap(cs.take_us);
                    if (r.accepted) {
                        const double *x = st.xrows.data() + (size_t)r.slot * W;
                        for (int j = 0; j < W; ++j) CHECK(x[j] == (double)r.k, "%s: model row of %lld holds %g", cs.name, (long long)r.k, x[j]);
                    }
                    taken += 1;
                }
                if (rcn != 0) break;
                if (cs.take_limit >= 0 && taken >= cs.take_limit) break;
            }
        }
        // (close before the first draw: the stub's draw is let go only once close is waiting for the threads)
        std::thread opener([&st]() {
            nap(3000);
            st.gate.store(1);
        });
        const int rcc = q.close(&drawn, &run, err);
        opener.join();
        CHECK(!q.is_open(), "%s: still open after close", cs.name);
        CHECK(drained.load() == 1, "%s: the runner drained %d times", cs.name, drained.load());
        const bool want_err = cs.fail_run_at >= 0 || cs.fail_draw_at >= 0;
        if (want_err) {
            const int code = cs.fail_run_at >= 0 ? 9 : 7;
            CHECK((rcn == code || rcc == code) && !err.empty(), "%s: error not returned (next %d close %d)", cs.name, rcn, rcc);
            if (cs.fail_run_at >= 0) CHECK(run == cs.fail_run_at && taken == run, "%s: ran %lld before the failure", cs.name, (long long)run);
            if (cs.fail_draw_at >= 0) CHECK(drawn == cs.fail_draw_at && run <= drawn, "%s: drew %lld before the failure", cs.name, (long long)drawn);
        } else {
            CHECK(rcn == 0 && rcc == 0, "%s: next %d close %d (%s)", cs.name, rcn, rcc, err.c_str());
        }
        // a second close, and a next on the closed feeder, are harmless
        int64_t d2 = 0, r2 = 0;
        int n = 0, fin = 0;
        Result r1;
        CHECK(q.close(&d2, &r2, err) == 0, "%s: second close", cs.name);
        CHECK(q.next(1, 0, &r1, &n, &fin, err) == 0 && n == 0 && fin == 1, "%s: next after close", cs.name);
    }
    // every row accounted for
    // (the drawer is held to rows - 2 beyond the trajectories BEGUN: one that failed was begun and does not count as run)
    const int64_t begun = run + (cs.fail_run_at >= 0 ? 1 : 0);
    CHECK(run >= 0 && drawn >= begun && drawn - begun <= cs.rows - 2, "%s: drawn %lld run %lld rows %d", cs.name, (long long)drawn,
          (long long)run, cs.rows);
    CHECK(st.looks + st.no_looks == run || cs.fail_run_at >= 0, "%s: look-aheads %lld + %lld for %lld runs", cs.name,
          (long long)st.looks, (long long)st.no_looks, (long long)run);
    const bool whole = cs.close_when == 0 && cs.take_limit < 0 && cs.fail_run_at < 0 && cs.fail_draw_at < 0;
    if (whole && cs.stop_at_accepts == 0) {
        CHECK(cs.total >= 0 && drawn == cs.total && run == cs.total && taken == cs.total, "%s: %lld of %lld ran, %lld taken",
              cs.name, (long long)run, (long long)cs.total, (long long)taken);
        // the look-ahead was there for every trajectory but the last
        CHECK(st.looks == (cs.total > 0 ? cs.total - 1 : 0) && st.no_looks == (cs.total > 0 ? 1 : 0), "%s: %lld look-aheads", cs.name,
              (long long)st.looks);
    }
    if (whole && cs.stop_at_accepts > 0) {
        CHECK(run == 2 * (int64_t)cs.stop_at_accepts && taken == run && st.no_looks == 0, "%s: stopped after %lld", cs.name, (long long)run);
    }
    if (cs.close_when == 1) CHECK(run == 0 && drawn <= 1, "%s: ran %lld drew %lld", cs.name, (long long)run, (long long)drawn);
    if (cs.take_limit >= 0) CHECK(run >= taken && run <= taken + cs.slots + 1, "%s: ran %lld, %lld taken", cs.name, (long long)run, (long long)taken);
    std::printf("%s %-40s rows %d slots %d drawn %lld run %lld taken %lld\n", g_failed == fails_before ? "ok  " : "FAIL", cs.name,
                cs.rows, cs.slots, (long long)drawn, (long long)run, (long long)taken);
    return run;
}

int main()
{
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    const int rows_of[2] = {3, 8};
    for (int rows : rows_of) {
        const int64_t totals[7] = {0, 1, 2, rows - 1, rows, rows + 1, 3 * rows + 1};
        for (int64_t total : totals) {
            Case c;
            c.name = "bounded stream";
            c.rows = rows;
            c.slots = rows == 3 ? 2 : 3;
            c.total = total;
            run_case(c);
        }
        Case c;
        c.rows = rows;
        c.slots = 2;
        c.total = 3 * rows + 1;
        c.name = "consumer slower than the runner";
        c.take_us = 3000;
        c.run_us = 100;
        run_case(c);
        c.name = "drawer slower than the runner";
        c.take_us = 0;
        c.draw_us = 3000;
        run_case(c);
        c.name = "runner slower than the drawer";
        c.draw_us = 0;
        c.run_us = 3000;
        run_case(c);
        c.run_us = 200;
        c.draw_us = 200;
        c.name = "stop by accept count, unbounded";
        c.total = -1;
        c.stop_at_accepts = rows == 3 ? 2 : 5;  // (ends in the middle of the ring)
        run_case(c);
        c.stop_at_accepts = 0;
        c.name = "caller stops taking, unbounded";
        c.take_limit = 5;
        run_case(c);
        c.take_limit = -1;
        c.name = "close before the first draw";
        c.close_when = 1;
        run_case(c);
        c.name = "close during a draw";
        c.close_when = 2;
        c.draw_us = 5000;
        run_case(c);
        c.name = "close during a run";
        c.close_when = 3;
        c.draw_us = 0;
        c.run_us = 5000;
        run_case(c);
        c.close_when = 0;
        c.run_us = 100;
        c.total = 3 * rows + 1;
        c.name = "run fails at trajectory k";
        c.fail_run_at = rows + 1;
        run_case(c);
        c.fail_run_at = 0;
        run_case(c);
        c.fail_run_at = -1;
        c.name = "draw fails at trajectory k";
        c.fail_draw_at = rows;
        run_case(c);
        c.fail_draw_at = -1;
        c.name = "first thread cannot be created";
        c.fail_thread = 0;
        run_case(c);
        c.name = "second thread cannot be created";
        c.fail_thread = 1;
        run_case(c);
    }
    std::printf("%s\n", g_failed ? "FAILED" : "ALL OK");
    return g_failed ? 1 : 0;
}
