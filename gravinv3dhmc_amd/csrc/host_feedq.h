// libgravhmc host side: the waiting of the trajectory feeder (host_feed.h).  Nothing of HIP in here: the file is
// compiled on its own, with stub hooks, by tests/feed_queue_main.cpp under the thread and address sanitizers.
//
// Three parties share one mutex: the DRAWER thread fills momentum rows of a ring in stream order, the RUNNER thread
// runs the trajectories from those rows and leaves one result per trajectory in a ring of result slots, the CALLER
// takes the results (next) and ends it (close).  Every wait is a condition variable; nothing spins.
//
//   rows   momentum rows; trajectory k lies in row k % rows.  The drawer starts trajectory j only while
//          j + 1 <= started + rows - 2 (started: trajectories the runner has begun), so it is never more than
//          rows - 2 ahead of the runner, and the row it writes belonged to a trajectory that ended two before the
//          one that runs.  rows >= 3: the row after the running one can always be drawn (the runner waits for it).
//   slots  result slots; trajectory k reports in slot k % slots, which also numbers its row for the accepted model.
//          The runner begins trajectory k only once slot k % slots was handed back, so a slow caller throttles the
//          chain.  A slot is handed back by the call of next AFTER the one that returned it: the caller reads its
//          rows in between.
#pragma once

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

namespace ghfeed {

struct Result {
    int64_t k = 0;  // trajectory number in the stream
    int L = 0, accepted = 0;
    double out5[5] = {0, 0, 0, 0, 0};
    int slot = 0;  // its result slot (the row of the accepted model, where one was asked for: the run hook fills
                   // it, and the caller knows when that row is complete)
};

// What a trajectory's run may ask of the queue while it runs.
struct RunCtl {
    // row of trajectory k + 1 once it is drawn (blocks until then), -1 where the stream has none
    std::function<int()> next_row;
    bool stop = false;       // (out) the runner ends after this trajectory
};

struct Hooks {
    // trajectory k into momentum row `row`: 0, or an error code with its text
    std::function<int(int64_t k, int row, int *L, double *u, std::string &err)> draw;
    // trajectory k from momentum row `row`, reporting in `slot`: 0, or an error code with its text
    std::function<int(int64_t k, int row, int L, double u, int slot, RunCtl &ctl, int *accepted, double out5[5],
                      std::string &err)> run;
    // at the runner's end: whatever completes the work still in flight
    std::function<int(std::string &err)> drain;
};

struct Options {
    int rows = 4, slots = 4;
    int64_t total = -1;         // trajectories of a bounded stream (-1: unbounded)
    int test_fail_thread = -1;  // tests: creating thread 0 (drawer) / 1 (runner) fails
};

struct Stats {
    double runner_wait_draw_s = 0.0, drawer_wait_row_s = 0.0, runner_wait_queue_s = 0.0;
};

class Feeder {
public:
    Feeder() = default;
    Feeder(const Feeder &) = delete;
    Feeder &operator=(const Feeder &) = delete;
    ~Feeder()
    {
        int64_t a, b;
        std::string e;
        close(&a, &b, e);
    }

    bool is_open() const { return open_; }

    // Starts both threads.  An error (bad options, a thread that cannot be created) leaves nothing running.
    int open(const Options &o, Hooks h, int err_code, std::string &err)
    {
        if (open_) {
            err = "feeder: already open";
            return err_code;
        }
        if (o.rows < 3 || o.slots < 1 || !h.draw || !h.run) {
            err = "feeder: needs at least 3 rows, 1 slot and its hooks";
            return err_code;
        }
        opt_ = o;
        hooks_ = std::move(h);
        meta_.assign((size_t)o.rows, Meta{});
        res_.assign((size_t)o.slots, Result{});
        drawn_ = started_ = done_ = published_ = handed_ = released_ = 0;
        stop_ = drawer_done_ = runner_done_ = false;
        rc_ = 0;
        err_.clear();
        stats_ = Stats{};
        try {
            if (o.test_fail_thread == 0) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            drawer_ = std::thread([this]() { drawer_main(); });
            if (o.test_fail_thread == 1) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            runner_ = std::thread([this]() { runner_main(); });
        } catch (const std::exception &e) {
            {
                std::lock_guard<std::mutex> lock(mu_);
                stop_ = true;
            }
            cv_room_.notify_all();
            cv_draw_.notify_all();
            if (drawer_.joinable()) drawer_.join();
            if (runner_.joinable()) runner_.join();
            err = std::string("feeder: cannot create a thread: ") + e.what();
            return err_code;
        }
        open_ = true;
        return 0;
    }

    // Blocks for at least one result or the end (timeout_ms >= 0: at most that long; then n = 0, finished = 0).
    // The slots of the results returned stay the caller's until the next call of next or close.  finished: the
    // runner has ended and every result was returned; the feeder's error, if any, is returned with it.
    int next(int max_rows, int timeout_ms, Result *out, int *n, int *finished, std::string &err)
    {
        *n = 0;
        *finished = 0;
        if (!open_) {
            *finished = 1;
            return 0;
        }
        std::unique_lock<std::mutex> lock(mu_);
        released_ = handed_;
        cv_slot_.notify_all();
        auto ready = [&]() { return published_ > handed_ || runner_done_; };
        if (timeout_ms >= 0) {
            // (against the wall clock, i.e. pthread_cond_timedwait: the steady clock's pthread_cond_clockwait is unknown to
            // older thread sanitizers, which then miss the unlock inside the wait; a clock step only moves this time-out)
            const auto until = std::chrono::system_clock::now() + std::chrono::milliseconds(timeout_ms);
            if (!cv_result_.wait_until(lock, until, ready)) return 0;
        } else {
            cv_result_.wait(lock, ready);
        }
        while (*n < max_rows && handed_ < published_) {
            out[*n] = res_[(size_t)(handed_ % opt_.slots)];
            *n += 1;
            handed_ += 1;
        }
        if (runner_done_ && handed_ == published_) {
            *finished = 1;
            if (rc_ != 0) {
                err = err_;
                return rc_;
            }
        }
        return 0;
    }

    // Ends it after the trajectory in flight and joins both threads.  drawn: trajectories taken from the stream;
    // run: trajectories run.  Returns the feeder's error, if any.  Harmless on a feeder that is not open.
    int close(int64_t *drawn, int64_t *run, std::string &err)
    {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stop_ = true;
        }
        cv_room_.notify_all();
        cv_draw_.notify_all();
        cv_slot_.notify_all();
        if (drawer_.joinable()) drawer_.join();
        if (runner_.joinable()) runner_.join();
        open_ = false;
        *drawn = drawn_;
        *run = done_;
        if (rc_ != 0) err = err_;
        const int rc = rc_;
        rc_ = 0;
        return rc;
    }

    Stats stats()
    {
        std::lock_guard<std::mutex> lock(mu_);
        return stats_;
    }

private:
    struct Meta {
        int L = 0;
        double u = 0.0;
    };
    using clock = std::chrono::steady_clock;

    template <typename Pred>
    void timed_wait(std::condition_variable &cv, std::unique_lock<std::mutex> &lock, double &acc, Pred pred)
    {
        if (pred()) return;
        const clock::time_point t0 = clock::now();
        cv.wait(lock, pred);
        acc += std::chrono::duration<double>(clock::now() - t0).count();
    }

    void set_error(int rc, const std::string &text)  // (mu_ held)
    {
        if (rc_ == 0) {
            rc_ = rc;
            err_ = text;
        }
        stop_ = true;
    }

    void drawer_main()
    {
        for (int64_t j = 0; opt_.total < 0 || j < opt_.total; ++j) {
            {
                std::unique_lock<std::mutex> lock(mu_);
                timed_wait(cv_room_, lock, stats_.drawer_wait_row_s,
                           [&]() { return stop_ || j + 1 <= started_ + opt_.rows - 2; });
                if (stop_) break;
            }
            int L = 0;
            double u = 0.0;
            std::string text;
            const int rc = hooks_.draw(j, (int)(j % opt_.rows), &L, &u, text);
            std::lock_guard<std::mutex> lock(mu_);
            if (rc != 0) {
                set_error(rc, text);
                break;
            }
            meta_[(size_t)(j % opt_.rows)] = Meta{L, u};
            drawn_ = j + 1;
            cv_draw_.notify_all();
        }
        {
            std::lock_guard<std::mutex> lock(mu_);
            drawer_done_ = true;
        }
        cv_draw_.notify_all();
        cv_slot_.notify_all();
    }

    void runner_main()
    {
        for (int64_t k = 0;; ++k) {
            Meta m;
            {
                std::unique_lock<std::mutex> lock(mu_);
                timed_wait(cv_draw_, lock, stats_.runner_wait_draw_s, [&]() { return stop_ || drawer_done_ || drawn_ > k; });
                if (stop_ || drawn_ <= k) break;
                timed_wait(cv_slot_, lock, stats_.runner_wait_queue_s, [&]() { return stop_ || k - released_ < opt_.slots; });
                if (stop_) break;
                started_ = k + 1;
                m = meta_[(size_t)(k % opt_.rows)];
            }
            cv_room_.notify_all();
            RunCtl ctl;
            ctl.next_row = [this, k]() -> int {
                std::unique_lock<std::mutex> lock(mu_);
                timed_wait(cv_draw_, lock, stats_.runner_wait_draw_s, [&]() { return drawer_done_ || drawn_ > k + 1; });
                return drawn_ > k + 1 ? (int)((k + 1) % opt_.rows) : -1;
            };
            Result r;
            r.k = k;
            r.L = m.L;
            r.slot = (int)(k % opt_.slots);
            std::string text;
            const int rc = hooks_.run(k, (int)(k % opt_.rows), m.L, m.u, r.slot, ctl, &r.accepted, r.out5, text);
            bool leave = false;
            {
                std::lock_guard<std::mutex> lock(mu_);
                if (rc != 0) {
                    set_error(rc, text);
                    leave = true;
                } else {
                    res_[(size_t)r.slot] = r;
                    done_ = k + 1;
                    published_ = k + 1;
                    if (ctl.stop) stop_ = leave = true;
                }
            }
            cv_result_.notify_all();
            if (leave) {
                cv_room_.notify_all();
                break;
            }
        }
        std::string text;
        const int rc = hooks_.drain ? hooks_.drain(text) : 0;
        {
            std::lock_guard<std::mutex> lock(mu_);
            if (rc != 0) set_error(rc, text);
            runner_done_ = true;
            stop_ = true;
        }
        cv_result_.notify_all();
        cv_room_.notify_all();
    }

    Options opt_;
    Hooks hooks_;
    std::mutex mu_;
    std::condition_variable cv_draw_;    // a row was drawn, or the drawer ended
    std::condition_variable cv_room_;    // the runner began a trajectory: a row is free
    std::condition_variable cv_slot_;    // the caller handed result slots back
    std::condition_variable cv_result_;  // a result was published, or the runner ended
    std::vector<Meta> meta_;
    std::vector<Result> res_;
    int64_t drawn_ = 0, started_ = 0, done_ = 0, published_ = 0, handed_ = 0, released_ = 0;
    bool stop_ = false, drawer_done_ = false, runner_done_ = false, open_ = false;
    int rc_ = 0;
    std::string err_;
    Stats stats_;
    std::thread drawer_, runner_;
};

}  // namespace ghfeed
