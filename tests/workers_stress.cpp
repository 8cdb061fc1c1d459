// The library's host worker pool (revrand_amd/csrc/rr_workers.h) held to its invariant: for every start(n, fn) each id in
// [0, n) runs fn exactly once, no other id runs it, and nothing runs after wait() -- through growth and shrink, with a
// caller that feeds the workers, with a caller that takes part, under concurrent callers and across a fork.  Host compiler
// only; built once with -fsanitize=thread (run with --no-fork: that runtime refuses new threads after a multithreaded
// fork) and once with -fsanitize=address,undefined -fno-sanitize-recover=all, and run directly (tests/test_workers_host.py).
#include "rr_workers.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <sys/wait.h>

static std::atomic<long long> failures{0}, jobs{0};

#define HOLD(cond, ...)                                \
    do {                                               \
        if (!(cond) && failures.fetch_add(1) < 20) {   \
            printf("FAILED %s: ", #cond);              \
            printf(__VA_ARGS__);                       \
            printf("\n");                              \
        }                                              \
    } while (0)

constexpr int MAXID = 32;

struct CountJob {  // fn(id): one more run of this job by id
    std::atomic<int> ran[MAXID];
    std::atomic<int> strays{0};  // ids outside [0, MAXID)
    CountJob() { for (auto &r : ran) r.store(0); }
    void operator()(int id) {
        if (id < 0 || id >= MAXID) strays.fetch_add(1);
        else ran[id].fetch_add(1);
    }
    void hold(int n, const char *when, int pool, int job) const {
        HOLD(strays.load() == 0, "%s: pool %d job %d", when, pool, job);
        for (int id = 0; id < MAXID; ++id)
            HOLD(ran[id].load() == (id < n ? 1 : 0), "%s: pool %d job %d n=%d: id %d ran %d times", when, pool, job, n, id, ran[id].load());
    }
};

// The pool grows and shrinks; every job is looked at after its own wait(), after the NEXT job's wait() (a late second
// run) and after the pool's threads are joined.
static void growth_and_shrink(int pools) {
    const int N[] = {2, 2, 4, 4, 8, 3, 16, 1};
    constexpr int J = sizeof(N) / sizeof(N[0]);
    const int SPIN[] = {500, 0, 1000, 20};  // (0: the workers sleep at once; 20: they fall asleep between two jobs)
    for (int p = 0; p < pools; ++p) {
        CountJob job[J];  // outlives the pool
        {
            WorkerPool pool(SPIN[p % 4], p % 3 == 0 ? 0 : 4096);
            for (int j = 0; j < J; ++j) {
                pool.start(N[j], job[j]);
                pool.wait();
                job[j].hold(N[j], "after wait", p, j);
                if (j) job[j - 1].hold(N[j - 1], "after the next wait", p, j - 1);
                jobs.fetch_add(1);
                if (p % 5 == 4) std::this_thread::sleep_for(std::chrono::microseconds(40));
            }
        }
        for (int j = 0; j < J; ++j) job[j].hold(N[j], "after join", p, j);
    }
}

// rr_legacy_randn's pattern: the workers claim items from a counter that the caller feeds between start and wait, then closes
static void caller_feeds(int rounds) {
    WorkerPool pool(500, 4096);
    for (int r = 0; r < rounds; ++r) {
        const int items = 1 + r % 37, threads = 1 + r % 4;
        std::vector<std::atomic<int>> done((size_t)items);
        for (auto &d : done) d.store(0);
        std::vector<int> payload((size_t)items, -1);
        std::atomic<int> ready(0), claim(0), entered(0);
        std::atomic<bool> closed(false);
        auto worker = [&](int) {
            entered.fetch_add(1);
            for (;;) {
                const int j = claim.fetch_add(1);
                while (ready.load(std::memory_order_acquire) <= j) {
                    if (closed.load(std::memory_order_acquire) && ready.load(std::memory_order_acquire) <= j) return;
                    std::this_thread::yield();
                }
                HOLD(payload[(size_t)j] == 7 * j + r, "round %d item %d read %d", r, j, payload[(size_t)j]);
                done[(size_t)j].fetch_add(1);
            }
        };
        pool.start(threads, worker);
        for (int j = 0; j < items; ++j) {
            payload[(size_t)j] = 7 * j + r;
            ready.store(j + 1, std::memory_order_release);
        }
        closed.store(true, std::memory_order_release);
        pool.wait();
        HOLD(entered.load() == threads, "round %d: %d workers entered, %d asked for", r, entered.load(), threads);
        for (int j = 0; j < items; ++j) HOLD(done[(size_t)j].load() == 1, "round %d item %d done %d times", r, j, done[(size_t)j].load());
        jobs.fetch_add(1);
    }
}

// The group step's pattern: member 0 on the caller, member i on worker i - 1, statuses by member; member 0's failure
// first, else the first failing member's in member order, with its message
static int group_run(WorkerPool &pool, int n, const int *fail, std::atomic<int> *ran, std::string *msg) {
    struct Slot {
        int rc = 0;
        std::string err;
    };
    auto fn = [&](int i) {
        ran[i].fetch_add(1);
        return fail[i];
    };
    std::vector<Slot> slots((size_t)n - 1);
    auto member = [&](int id) {
        Slot &s = slots[(size_t)id];
        s.rc = fn(id + 1);
        if (s.rc) s.err = "member " + std::to_string(id + 1);
    };
    pool.start(n - 1, member);
    const int rc = fn(0);
    pool.wait();
    if (rc) {
        *msg = "member 0";
        return rc;
    }
    for (const Slot &s : slots)
        if (s.rc) {
            *msg = s.err;
            return s.rc;
        }
    return 0;
}

static void caller_takes_part(int rounds) {
    WorkerPool pool(1000, 1 << 16);
    const int N[] = {2, 3, 4, 2, 8, 4};
    for (int r = 0; r < rounds; ++r) {
        const int n = N[r % 6];
        int fail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // none / one member / two members / member 0 and another
        const int kind = r % 4, a = r % n, b = (r / 4) % n;
        if (kind >= 1) fail[a] = 100 + a;
        if (kind >= 2) fail[b] = 100 + b;
        if (kind == 3) fail[0] = 100;
        int want = 0, who = -1;
        for (int i = n - 1; i >= 0; --i)
            if (fail[i]) want = fail[i], who = i;
        std::atomic<int> ran[8];
        for (auto &x : ran) x.store(0);
        std::string msg;
        const int rc = group_run(pool, n, fail, ran, &msg);
        HOLD(rc == want, "round %d n=%d: status %d, expected %d", r, n, rc, want);
        HOLD(who < 0 || msg == "member " + std::to_string(who), "round %d n=%d: message '%s', expected member %d", r, n, msg.c_str(), who);
        for (int i = 0; i < 8; ++i) HOLD(ran[i].load() == (i < n ? 1 : 0), "round %d n=%d: member %d ran %d times", r, n, i, ran[i].load());
        jobs.fetch_add(1);
    }
}

// Several threads start and wait on one pool: the jobs never overlap and each runs exactly once per id
static void concurrent_callers(int callers, int rounds) {
    WorkerPool pool(500, 4096);
    std::vector<std::atomic<int>> inside((size_t)callers);  // workers inside a job of caller k
    for (auto &x : inside) x.store(0);
    std::vector<std::thread> th;
    for (int k = 0; k < callers; ++k)
        th.emplace_back([&, k] {
            for (int r = 0; r < rounds; ++r) {
                const int n = 1 + (r + k) % 4;
                CountJob count;
                auto fn = [&](int id) {
                    inside[(size_t)k].fetch_add(1);
                    for (int o = 0; o < callers; ++o)
                        HOLD(o == k || inside[(size_t)o].load() == 0, "caller %d round %d overlaps a job of caller %d", k, r, o);
                    count(id);
                    inside[(size_t)k].fetch_sub(1);
                };
                pool.start(n, fn);
                pool.wait();
                HOLD(inside[(size_t)k].load() == 0, "caller %d round %d: a worker is still inside after wait", k, r);
                count.hold(n, "concurrent callers", k, r);
                jobs.fetch_add(1);
            }
        });
    for (auto &t : th) t.join();
}

// A forked child abandons the pool it inherited and gets its own from the per-process accessor; the parent's goes on working
static void across_a_fork() {
    static ProcessWorkerPool workers(500, 4096);
    WorkerPool *mine = &workers.get();
    for (int n : {2, 4}) {
        CountJob count;
        mine->start(n, count);
        mine->wait();
        count.hold(n, "before the fork", 0, n);
        jobs.fetch_add(1);
    }
    fflush(stdout);
    const pid_t child = fork();
    if (child == 0) {  // (_exit: the inherited pool's threads do not exist here, nothing of it may be joined or destroyed)
        WorkerPool *own = &workers.get();
        CountJob count;
        own->start(2, count);
        own->wait();
        bool ok = own != mine && &workers.get() == own;
        for (int id = 0; id < MAXID; ++id) ok = ok && count.ran[id].load() == (id < 2 ? 1 : 0);
        _exit(ok ? 0 : 1);
    }
    HOLD(child > 0, "fork failed");
    int status = -1;
    HOLD(waitpid(child, &status, 0) == child && WIFEXITED(status) && WEXITSTATUS(status) == 0, "the child's job: wait status %d", status);
    HOLD(&workers.get() == mine, "the parent's accessor returned another pool after the fork");
    CountJob count;
    mine->start(3, count);
    mine->wait();
    count.hold(3, "after the fork", 0, 3);
    jobs.fetch_add(2);
}

int main(int argc, char **argv) {
    const bool no_fork = argc > 1 && strcmp(argv[1], "--no-fork") == 0;
    growth_and_shrink(320);
    caller_feeds(400);
    caller_takes_part(480);
    concurrent_callers(4, 300);
    if (!no_fork) across_a_fork();
    printf("%lld jobs %s, %lld failures%s\n", jobs.load(), failures.load() ? "ran" : "hold", failures.load(), no_fork ? " (fork skipped)" : "");
    return failures.load() ? 1 : 0;
}
