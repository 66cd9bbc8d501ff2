// multi_device.h — one index replicated on several devices in one process: the query split and the worker pool that
// runs the shards (host only, no HIP).
//
// cph_multi_search_batch answers a batch with every replica at once: the queries are cut into contiguous shards
// (plan_shards: sizes differ by at most one, none smaller than `min_shard`), each shard runs on ITS replica's persistent
// worker thread, which writes straight into the caller's rows, and the call returns once every shard has finished --
// on error too, so that no worker touches the caller's arrays afterwards.  A failing shard's status and message reach
// the calling thread (the library's error text is thread-local on the worker); with several failures the one of the
// lowest-numbered replica wins.
//
// What a shard IS is a callable, as in search_coalescer.h, so that the policy can be exercised without a GPU:
// tests/multi_device_host runs it under ThreadSanitizer and AddressSanitizer with a stand-in launch.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace cph {

constexpr uint32_t kMaxReplicas = 16;
constexpr uint64_t kDefaultMinShard = 1024;   // queries: a smaller shard does not pay for the extra launch

struct Shard {
    uint32_t replica;
    uint64_t lo, hi;    // queries [lo, hi)
};

// Contiguous shards of n queries over `replicas` replicas (dist.shard_bounds: sizes differ by at most one), as many as
// keep every shard at >= min_shard queries.  Fewer than 2 * min_shard queries: one shard, the whole batch (n = 0
// included), on replica `first`.  Shard j runs on replica (first + j) % replicas.
inline std::vector<Shard> plan_shards(uint64_t n, uint32_t replicas, uint64_t min_shard, uint32_t first) {
    if (replicas == 0) throw std::invalid_argument("no replicas");
    if (min_shard == 0) min_shard = 1;
    first %= replicas;
    uint64_t s = n / min_shard;
    if (s > replicas) s = replicas;
    if (s < 2) return {Shard{first, 0, n}};
    std::vector<Shard> out;
    out.reserve(s);
    const uint64_t base = n / s, rem = n % s;
    for (uint64_t j = 0; j < s; ++j) {
        const uint64_t lo = j * base + (j < rem ? j : rem);
        out.push_back(Shard{(uint32_t)((first + j) % replicas), lo, lo + base + (j < rem ? 1 : 0)});
    }
    return out;
}

// One persistent worker thread per replica.  run() hands every shard of a plan to its replica's worker (FIFO, shared
// by all callers) and returns when all of them have finished.
class ReplicaPool {
public:
    // launch(shard, err): runs one shard, returns a status (0 = ok); on failure it fills `err`.  An exception escaping
    // it counts as status 2 (invalid_argument: 1, bad_alloc: 3), the codes of cph_status.
    using Launch = std::function<int(const Shard&, std::string& err)>;

    // init(replica) runs once on each worker before its first shard (binds the thread to the replica's device).
    ReplicaPool(uint32_t replicas, std::function<void(uint32_t)> init) : workers_(replicas) {
        if (replicas == 0 || replicas > kMaxReplicas) throw std::invalid_argument("replica count out of range");
        try {
            for (uint32_t r = 0; r < replicas; ++r)
                workers_[r].th = std::thread([this, r, init] { loop(r, init); });
        } catch (...) {
            stop();
            throw;
        }
    }
    ReplicaPool(const ReplicaPool&) = delete;
    ReplicaPool& operator=(const ReplicaPool&) = delete;
    ~ReplicaPool() { stop(); }

    uint32_t size() const { return (uint32_t)workers_.size(); }

    // Returns 0, or the status of the lowest-numbered replica whose shard failed (its message in `err`).
    int run(const std::vector<Shard>& plan, const Launch& launch, std::string& err) {
        Join j;
        j.launch = &launch;
        j.remaining = plan.size();
        j.rc.assign(plan.size(), 0);
        j.err.resize(plan.size());
        std::vector<Task> tasks(plan.size());
        for (size_t i = 0; i < plan.size(); ++i) {
            if (plan[i].replica >= workers_.size()) throw std::invalid_argument("shard on a replica that does not exist");
            tasks[i] = Task{&j, plan[i], i};
        }
        for (Task& t : tasks) {
            Worker& w = workers_[t.shard.replica];
            std::lock_guard<std::mutex> lk(w.mu);
            w.q.push_back(&t);
            w.cv.notify_one();
        }
        {
            std::unique_lock<std::mutex> lk(j.mu);
            j.cv.wait(lk, [&] { return j.remaining == 0; });
        }
        int best = -1;
        for (size_t i = 0; i < plan.size(); ++i)
            if (j.rc[i] != 0 && (best < 0 || plan[i].replica < plan[(size_t)best].replica)) best = (int)i;
        if (best < 0) return 0;
        err = j.err[(size_t)best];
        return j.rc[(size_t)best];
    }

private:
    struct Join {
        std::mutex mu;
        std::condition_variable cv;
        size_t remaining = 0;
        const Launch* launch = nullptr;
        std::vector<int> rc;
        std::vector<std::string> err;
    };
    struct Task {
        Join* join = nullptr;
        Shard shard{};
        size_t index = 0;
    };
    struct Worker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::deque<Task*> q;
        bool stop = false;
    };
    std::vector<Worker> workers_;

    void loop(uint32_t r, const std::function<void(uint32_t)>& init) {
        try { if (init) init(r); } catch (...) {}   // (each launch binds its device again and reports a failure itself)
        Worker& w = workers_[r];
        for (;;) {
            Task* t = nullptr;
            {
                std::unique_lock<std::mutex> lk(w.mu);
                w.cv.wait(lk, [&] { return w.stop || !w.q.empty(); });
                if (w.q.empty()) return;    // stopping, nothing left
                t = w.q.front();
                w.q.pop_front();
            }
            int rc = 0;
            std::string e;
            try {
                rc = (*t->join->launch)(t->shard, e);
            } catch (const std::invalid_argument& x) { rc = 1; e = x.what();
            } catch (const std::bad_alloc&) { rc = 3; e = "out of memory";
            } catch (const std::exception& x) { rc = 2; e = x.what();
            } catch (...) { rc = 2; e = "unknown error"; }
            Join& j = *t->join;
            // The caller's Join (and the Task) live on its stack: the last touch is the notify, made under the mutex
            // the caller waits on, so it cannot return before this worker is done with them.
            std::lock_guard<std::mutex> lk(j.mu);
            j.rc[t->index] = rc;
            j.err[t->index] = std::move(e);
            if (--j.remaining == 0) j.cv.notify_all();
        }
    }

    void stop() {
        for (Worker& w : workers_) {
            std::lock_guard<std::mutex> lk(w.mu);
            w.stop = true;
            w.cv.notify_all();
        }
        for (Worker& w : workers_)
            if (w.th.joinable()) w.th.join();
    }
};

}  // namespace cph
