// host_threads.cpp — the host's two ways of running things side by side: parallel_for over the persistent thread pool, and the farm
// that deals the independent units of a batch to the device contexts (farm_shards, farm_run; shard_pick is in pgm_host.h).
// Needs the standard library, pgm_pool.h and pgm_exception only, so that a stand-alone test program can link it.
#include "pgm_host.h"
#include "../csrc/pgm_pool.h"

#include <algorithm>
#include <cstdlib>
#include <thread>

namespace pgm {

void parallel_for(size_t n, const std::function<void(size_t)> &fn) {
    static unsigned nt = []() {
        unsigned v = std::thread::hardware_concurrency();
        if (const char *e = getenv("PGM_HOST_THREADS")) v = (unsigned)atoi(e);
        return std::max(1u, std::min(v, 16u));
    }();
    static pgm_pool::Pool pool(nt);   // persistent: a level has half a dozen sections of a millisecond or two
    const std::string err = pool.run(n, nt, fn);
    if (!err.empty()) throw pgm_exception(err);
}

std::vector<std::vector<uint32_t>> farm_shards(const std::vector<uint64_t> &cost, int nw) {
    const uint32_t n = (uint32_t)cost.size();
    nw = std::max(1, std::min<int>(nw, (int)std::max(1u, n)));
    std::vector<std::vector<uint32_t>> sh((size_t)nw);
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    std::vector<uint64_t> load((size_t)nw, 0);
    for (uint32_t i : order) {
        size_t w = 0;
        for (size_t k = 1; k < load.size(); ++k) if (load[k] < load[w]) w = k;
        sh[w].push_back(i);
        load[w] += std::max<uint64_t>(cost[i], 1);
    }
    while (sh.size() > 1 && sh.back().empty()) sh.pop_back();
    return sh;
}

void farm_run(const std::vector<std::vector<uint32_t>> &shards, const std::function<void(int)> &fn) {
    std::vector<std::thread> th;
    for (size_t w = 1; w < shards.size(); ++w) if (!shards[w].empty()) th.emplace_back(fn, (int)w);
    if (!shards.empty() && !shards[0].empty()) fn(0);
    for (auto &t : th) t.join();
}

}  // namespace pgm
