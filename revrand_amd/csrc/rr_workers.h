// The library's host worker threads: one class, two instances (rr_hostrng.hip: the logarithms and square roots of
// rr_legacy_randn; rr_elbo.hip: the members of a device group, queued concurrently).  No HIP, no context: plain C++17,
// tests/workers_stress.cpp drives it under the host compiler's sanitizers without a GPU.
//
// Workers outlive a job: an SVI fit asks for one every ~100 us, thousands of times, and a std::thread per call costs more
// than the work it takes over.  A worker spins for a moment after a job, then sleeps on a condition variable.
//
// INVARIANT.  For every start(n, fn), fn(id) runs exactly once for each id in [0, n) and for no other id; when wait()
// returns, no worker is inside fn or will enter it later -- however the pool grew, shrank or was delayed in between.
//
// Why it holds.  A job is the triple (gen_, want_, fn_/arg_).  It is written in one critical section of mu_ (start) and
// taken in one critical section of mu_ (loop): a worker compares gen_ with the generation it ran last, records gen_ and
// copies want_ and the job UNDER THE SAME LOCK, so what it records is the generation of the job it takes, never an older
// one read earlier.  (The atomic read of gen_ outside the lock is a hint to stop spinning, nothing more.)  Hence
//   - at most once: a worker that took generation g has seen == g, and gen_ only changes in the next start;
//   - a new worker starts with seen = the generation BEFORE the job it is spawned for (both under start's lock);
//   - no other id: id >= want_ records the generation and goes back to waiting;
//   - at least once, and nothing after wait(): call_ is held from start to the end of wait, so gen_, want_ and the job
//     stay as they are until remaining_ reaches 0, which takes one decrement by each of the n workers, each AFTER its
//     fn(id) has returned; a worker that has not yet looked finds the job unchanged, one that has looked does not look
//     again before the next start.
// fn is not copied: it must stay alive until wait() returns (an lvalue of the caller's, which start's signature asks for).
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <vector>

class WorkerPool {
  public:
    // spin_us: how long a worker polls for the next job before it sleeps; caller_yields: how often wait() yields before
    // it sleeps in 200 us slices
    WorkerPool(int spin_us, int caller_yields) : spin_us_(spin_us), caller_yields_(caller_yields) {}
    WorkerPool(const WorkerPool &) = delete;
    WorkerPool &operator=(const WorkerPool &) = delete;
    // (never runs for the library's own two pools; not while a job is under way)
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            gen_.fetch_add(1, std::memory_order_release);  // (ends the spinning of those that are not asleep)
        }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }

    // fn(id) on worker id for each id in [0, n); returns at once.  One job at a time: a second caller waits here until the
    // first one's wait() has returned.
    template <typename F>
    void start(int n, F &fn) {
        call_.lock();
        {
            std::lock_guard<std::mutex> lk(mu_);
            const int64_t before = gen_.load(std::memory_order_relaxed);
            while ((int)th_.size() < n) {
                const int id = (int)th_.size();
                th_.emplace_back([this, id, before] { loop(id, before); });
            }
            fn_ = [](void *f, int id) { (*static_cast<F *>(f))(id); };
            arg_ = const_cast<void *>(static_cast<const void *>(&fn));
            want_ = n;
            remaining_.store(n > 0 ? n : 0, std::memory_order_relaxed);
            gen_.store(before + 1, std::memory_order_release);
        }
        cv_.notify_all();
    }
    // blocks until all n have returned from fn
    void wait() {
        for (int spin = 0; remaining_.load(std::memory_order_acquire) > 0; ++spin) {
            if (spin < caller_yields_) std::this_thread::yield();
            else {
                // (the last worker notifies under mu_, so no wake-up is lost; the slice is a second line of defence.  On the
                // system clock: pthread_cond_timedwait, which ThreadSanitizer's runtime follows -- GCC 11's loses track of mu_
                // across wait_for's pthread_cond_clockwait and then reports locks and races that are not there)
                std::unique_lock<std::mutex> lk(mu_);
                done_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(200),
                                 [this] { return remaining_.load(std::memory_order_acquire) == 0; });
            }
        }
        call_.unlock();
    }

  private:
    void loop(int id, int64_t seen) {
        for (;;) {
            // the hint: spin first (the caller comes back within ~100 us inside a fit), then sleep
            const auto t0 = std::chrono::steady_clock::now();
            bool sleep = false;
            while (gen_.load(std::memory_order_acquire) == seen && !sleep) {
                std::this_thread::yield();
                sleep = std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us_);
            }
            void (*fn)(void *, int);
            void *arg;
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (sleep) cv_.wait(lk, [&] { return gen_.load(std::memory_order_relaxed) != seen; });
                if (stop_) return;
                const int64_t g = gen_.load(std::memory_order_relaxed);
                if (g == seen) continue;
                seen = g;  // the generation of the job taken below, read under the lock that guards the job
                if (id >= want_) continue;
                fn = fn_;
                arg = arg_;
            }
            fn(arg, id);
            if (remaining_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(mu_);
                done_.notify_all();
            }
        }
    }
    const int spin_us_, caller_yields_;
    std::mutex mu_, call_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;     // worker id = index; grown in start, joined in the destructor
    void (*fn_)(void *, int) = nullptr;
    void *arg_ = nullptr;
    int want_ = 0;
    bool stop_ = false;
    std::atomic<int> remaining_{0};
    std::atomic<int64_t> gen_{0};     // written under mu_ only
};

// A pool per process: threads do not survive a fork, so a forked child abandons the pool it inherited (never joins or
// destroys it) and starts its own at its first call.  The pools made here are never destroyed.
class ProcessWorkerPool {
  public:
    ProcessWorkerPool(int spin_us, int caller_yields) : spin_us_(spin_us), caller_yields_(caller_yields) {}
    WorkerPool &get() {
        std::lock_guard<std::mutex> lk(mu_);
        if (!pool_ || pid_ != getpid()) {
            pool_ = new WorkerPool(spin_us_, caller_yields_);
            pid_ = getpid();
        }
        return *pool_;
    }

  private:
    const int spin_us_, caller_yields_;
    std::mutex mu_;
    WorkerPool *pool_ = nullptr;
    pid_t pid_ = 0;
};
