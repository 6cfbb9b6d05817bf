// pool.hpp — the host thread pool the batch builders run on.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace dg {

// Minimal persistent pool: parallel_for over [0, n) with dynamic chunking.
class Pool {
public:
    explicit Pool(int n) {
        for (int i = 0; i < n; i++) workers_.emplace_back([this, i] { loop(i); });
    }
    ~Pool() {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; gen_++; }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    int size() const { return (int)workers_.size(); }
    // fn(index, worker_id); worker ids are 0..size() (the caller participates as id size()).
    void parallel_for(int n, const std::function<void(int, int)> &fn) {
        if (n <= 0) return;
        { std::lock_guard<std::mutex> l(m_); fn_ = &fn; n_ = n; next_.store(0); pending_ = (int)workers_.size(); gen_++; }
        cv_.notify_all();
        run(fn, (int)workers_.size());
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }
private:
    void run(const std::function<void(int, int)> &fn, int wid) {
        for (;;) {
            int i = next_.fetch_add(1);
            if (i >= n_) break;
            fn(i, wid);
        }
    }
    void loop(int wid) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int, int)> *fn;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                fn = fn_;
            }
            if (fn) run(*fn, wid);
            { std::lock_guard<std::mutex> l(m_); if (--pending_ == 0) done_.notify_all(); }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)> *fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

}  // namespace dg
