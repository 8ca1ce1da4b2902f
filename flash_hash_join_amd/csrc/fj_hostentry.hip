// fj_hostentry.hip -- the host-buffer (NumPy) entry fj_join_host: pageable memory -> pinned staging ring -> HBM, pipelined
// with the join's first pass.  Replaces all twelve pybind entry points hash_join.cpp:603-637 for host arrays.
// (Split out of fj_api.hip in round 4; see fj_host.h for the map.)
#include "fj_host.h"

#include <atomic>
#include <memory>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>
using namespace fjh;

namespace fjh { fj_ctx*& host_ctx() { static fj_ctx* c = nullptr; return c; } }

namespace {

// ---- where the copy threads run ---------------------------------------------------------------------------------------------
// A box of this pool has two sockets; a thread that reads the caller's array from the other socket's memory copies at a
// fraction of the local rate, and round 3's unbound threads landed wherever the scheduler put them (the same entry took 16.6 ms
// on one box and 23.0 on another).  FJ_HOST_COPY_BIND: 2 (default) = every piece is copied by threads bound to the NUMA node
// that HOLDS the piece's source pages (move_pages query of the piece's first page; one thread group per node, created on
// demand), 1 = threads bound to the GPU's node, 0 = unbound.
std::vector<int> parse_cpulist(const std::string& s) {
    std::vector<int> out;
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(',', i); if (j == std::string::npos) j = s.size();
        const std::string tok = s.substr(i, j - i);
        const size_t d = tok.find('-');
        const int a = atoi(tok.c_str()), b = d == std::string::npos ? a : atoi(tok.c_str() + d + 1);
        for (int c = a; c <= b && tok.size(); ++c) out.push_back(c);
        i = j + 1;
    }
    return out;
}
std::vector<int> node_cpus(int node) {                       // CPUs of a NUMA node that this process may run on
    std::vector<int> out;
    char path[128]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return out;
    char buf[4096] = {0};
    if (fgets(buf, sizeof buf, f)) {
        std::string s(buf); while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
        cpu_set_t aff; CPU_ZERO(&aff);
        const bool have = sched_getaffinity(0, sizeof aff, &aff) == 0;
        for (int c : parse_cpulist(s)) if (!have || (c < CPU_SETSIZE && CPU_ISSET(c, &aff))) out.push_back(c);
    }
    fclose(f);
    return out;
}
int node_of_address(const void* p) {                         // NUMA node of the page that holds p (-1: unknown)
    void* page = (void*)((uintptr_t)p & ~(uintptr_t)4095);
    int status = -1;
    if (syscall(SYS_move_pages, 0, 1ul, &page, nullptr, &status, 0) != 0) return -1;
    return status;
}
int node_of_device(int device) {
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof bdf, device) != hipSuccess) return -1;
    for (char* q = bdf; *q; ++q) *q = (char)tolower(*q);
    char path[160]; snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int n = -1; if (fscanf(f, "%d", &n) != 1) n = -1;
    fclose(f);
    return n;
}

// memcpy by a few persistent threads: one core copies pageable -> pinned memory at 10-15 GB/s, PCIe Gen5 x16 moves ~55.  The
// threads spin for the next piece (a condition-variable wake-up per 16-MiB piece cost as much as a fifth of the piece's copy)
// and fall asleep only after ~2 ms without work.
class CopyPool {
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable work_;
    const char* src_ = nullptr; char* dst_ = nullptr; size_t n_ = 0;
    std::atomic<unsigned> gen_{0}, remaining_{0};
    std::atomic<bool> stop_{false};
    void slice(unsigned id, unsigned parts, size_t* off, size_t* len) const {
        const size_t per = ((n_ / parts) + 4095) & ~(size_t)4095;
        *off = std::min(n_, per * id);
        *len = id + 1 == parts ? n_ - *off : std::min(per, n_ - *off);
    }
    void worker(unsigned id, std::vector<int> cpus) {
        if (!cpus.empty()) {
            cpu_set_t set; CPU_ZERO(&set);
            for (int c : cpus) if (c < CPU_SETSIZE) CPU_SET(c, &set);
            (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
        }
        unsigned seen = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (gen_.load(std::memory_order_acquire) == seen && !stop_.load(std::memory_order_relaxed)) {
                if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
                    std::unique_lock<std::mutex> l(m_);
                    work_.wait(l, [&] { return stop_.load() || gen_.load() != seen; });
                    break;
                }
                __builtin_ia32_pause();
            }
            if (stop_.load()) return;
            seen = gen_.load(std::memory_order_acquire);
            size_t off, len; slice(id + 1, (unsigned)th_.size() + 1, &off, &len);
            if (len) memcpy(dst_ + off, src_ + off, len);
            remaining_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
public:
    CopyPool(unsigned nthreads, const std::vector<int>& cpus) { for (unsigned i = 0; i + 1 < nthreads; ++i) th_.emplace_back([this, i, cpus] { worker(i, cpus); }); }
    ~CopyPool() { stop_.store(true); { std::lock_guard<std::mutex> l(m_); } work_.notify_all(); for (auto& t : th_) t.join(); }
    unsigned threads() const { return (unsigned)th_.size() + 1; }
    void copy(void* dst, const void* src, size_t n) {
        if (n < (4u << 20) || th_.empty()) { memcpy(dst, src, n); return; }
        src_ = (const char*)src; dst_ = (char*)dst; n_ = n;
        remaining_.store((unsigned)th_.size(), std::memory_order_relaxed);
        gen_.fetch_add(1, std::memory_order_release);
        { std::lock_guard<std::mutex> l(m_); }                 // (a worker between its predicate check and its sleep)
        work_.notify_all();
        size_t off, len; slice(0, (unsigned)th_.size() + 1, &off, &len);
        if (len) memcpy((char*)dst + off, (const char*)src + off, len);
        while (remaining_.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
    }
};

int copy_bind_mode() { static const int m = getenv("FJ_HOST_COPY_BIND") ? atoi(getenv("FJ_HOST_COPY_BIND")) : 2; return m; }
unsigned copy_threads_for(size_t ncpus) {
    if (const char* e = getenv("FJ_HOST_COPY_THREADS")) return (unsigned)std::max(1, atoi(e));
    // from the CPUs the threads may actually use (the affinity mask, or one node's share of it): a quarter of them, at most 6.  One
    // core copies pageable -> pinned memory at ~14 GB/s and PCIe Gen5 x16 takes ~57: four to six threads keep up, and MORE is worse
    // (profiles/r04_host_entry_probe.txt: 1.11-1.15x a pinned copy with 4-16 threads, 1.37-1.41x with 24-32)
    return (unsigned)std::min<size_t>(6, std::max<size_t>(2, ncpus / 4));
}
// the pool that copies a piece whose source starts at `src`, for the context's device
CopyPool& copy_pool_for(const void* src, int device) {
    static std::mutex mu;
    static std::vector<std::pair<int, std::unique_ptr<CopyPool>>> pools;      // (node or -1, pool)
    int node = -1;
    const int mode = copy_bind_mode();
    if (mode == 2) node = node_of_address(src);
    else if (mode == 1) node = node_of_device(device);
    std::lock_guard<std::mutex> l(mu);
    for (auto& p : pools) if (p.first == node) return *p.second;
    std::vector<int> cpus = node >= 0 ? node_cpus(node) : std::vector<int>();
    size_t ncpus = cpus.size();
    if (ncpus == 0) { cpu_set_t aff; CPU_ZERO(&aff); ncpus = sched_getaffinity(0, sizeof aff, &aff) == 0 ? (size_t)CPU_COUNT(&aff) : std::max(1u, std::thread::hardware_concurrency()); }
    pools.emplace_back(node, std::unique_ptr<CopyPool>(new CopyPool(copy_threads_for(ncpus), cpus)));
    return *pools.back().second;
}

// src (pageable host memory) -> dst (device), `piece` bytes at a time through the context's pinned ring; the copy of piece
// i+1 into the ring overlaps the DMA of piece i.  on_piece(offset, bytes, event) is called once a piece's DMA is enqueued on
// the context's copy stream (the event fires when it has landed).
int h2d_pipelined(fj_ctx* c, void* dst, const void* src, size_t bytes, size_t piece, unsigned* cursor,
                  const std::function<int(size_t, size_t, hipEvent_t)>& on_piece) {
    for (size_t off = 0; off < bytes; off += piece) {
        const size_t n = std::min(piece, bytes - off);
        const unsigned k = (*cursor)++ % 3u;
        HIPCHK(hipEventSynchronize(c->ev[E_H0 + k]));                         // the ring slot's previous DMA has left it
        copy_pool_for((const char*)src + off, c->device).copy(c->stage[k], (const char*)src + off, n);
        HIPCHK(hipMemcpyAsync((char*)dst + off, c->stage[k], n, hipMemcpyHostToDevice, c->side));
        HIPCHK(hipEventRecord(c->ev[E_H0 + k], c->side));
        if (on_piece && on_piece(off, n, c->ev[E_H0 + k])) return 1;
    }
    return 0;
}

}  // namespace
extern "C" {

int fj_join_host(int algo, int bloom, int materialize,
                 const uint64_t* bk, const uint64_t* bv, size_t nb, const uint64_t* pk, size_t np,
                 uint64_t* out_count, double* out_seconds, uint64_t** out_keys, uint64_t** out_vals) {
    if (out_keys) *out_keys = nullptr;
    if (out_vals) *out_vals = nullptr;
    const bool many_host = algo >= 0 && (algo & FJ_ALGO_MANY_TO_MANY) != 0;
    const bool left = algo >= 0 && (algo & FJ_ALGO_LEFT_OUTER) != 0, anti = algo >= 0 && (algo & FJ_ALGO_ANTI) != 0;
    const bool rid = algo >= 0 && (algo & FJ_ALGO_ROW_IDS) != 0;
    const bool full = algo >= 0 && (algo & FJ_ALGO_FULL_OUTER) != 0;
    const bool allc = algo >= 0 && (algo & FJ_ALGO_ALL_COPIES) != 0;
    const bool po = algo >= 0 && (algo & FJ_ALGO_PROBE_ORDER) != 0;
    const bool bo = algo >= 0 && (algo & FJ_ALGO_BUILD_ORDER) != 0;
    const bool gb = algo >= 0 && (algo & FJ_ALGO_GROUP_BY) != 0;
    const bool inv = gb && (algo & FJ_ALGO_INVERSE) != 0;
    const bool kpair = gb && (algo & FJ_ALGO_KEY_PAIR) != 0;                     // a two-column key: build_vals is the second KEY column, *out_keys g first-occurrence row indices
    const bool grows = gb && (algo & FJ_ALGO_GROUP_ROWS) != 0;                   // the rows of every group: *out_vals nb row indices, then g starts
    const bool aall = gb && (algo & FJ_ALGO_AGG_ALL) != 0;
    const bool aarg = gb && (algo & FJ_ALGO_AGG_ARG) != 0;
    const bool amerge = gb && aall && (algo & FJ_ALGO_AGG_MERGE) != 0;            // partial rows in: build_vals is FOUR planes of nb words
    const bool pagg = kpair && aall && !inv;                                     // a two-column key with four aggregates: probe_keys is the VALUE column (np == nb), *out_keys g words of A, *out_vals 5 * g words - B, count, sum, min, max
    if (algo >= 0 && (algo & FJ_ALGO_GROUP_ROWS) && !gb)
        return set_err("fj_join_host: unknown algo %d (FJ_ALGO_GROUP_ROWS modifies FJ_ALGO_GROUP_BY)", algo);
    if (grows && (algo & (FJ_ALGO_INVERSE | FJ_ALGO_ROW_IDS | FJ_ALGO_AGG_MIN | FJ_ALGO_AGG_MAX | FJ_ALGO_AGG_SIGNED | FJ_ALGO_AGG_FLOAT | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_ARG | FJ_ALGO_AGG_MERGE | FJ_ALGO_KEY_PAIR)))
        return set_err("fj_join_host: FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_%s (out_vals is taken by the row indices and the groups' starts, and no value column is read)",
                       (algo & FJ_ALGO_INVERSE) ? "INVERSE" : (algo & FJ_ALGO_ROW_IDS) ? "ROW_IDS" : (algo & FJ_ALGO_AGG_MIN) ? "AGG_MIN" : (algo & FJ_ALGO_AGG_MAX) ? "AGG_MAX" :
                       (algo & FJ_ALGO_AGG_SIGNED) ? "AGG_SIGNED" : (algo & FJ_ALGO_AGG_FLOAT) ? "AGG_FLOAT" : (algo & FJ_ALGO_AGG_ALL) ? "AGG_ALL" : (algo & FJ_ALGO_AGG_ARG) ? "AGG_ARG" :
                       (algo & FJ_ALGO_AGG_MERGE) ? "AGG_MERGE" : "KEY_PAIR");
    if (algo >= 0 && (algo & FJ_ALGO_AGG_MERGE) && !amerge)
        return set_err("fj_join_host: unknown algo %d (FJ_ALGO_AGG_MERGE modifies FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL)", algo);
    if (algo >= 0 && (algo & FJ_ALGO_KEY_PAIR) && !gb)
        return set_err("fj_join_host: unknown algo %d (FJ_ALGO_KEY_PAIR modifies FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE)", algo);
    const int agg_flags = ((bo || gb) ? (FJ_ALGO_AGG_MIN | FJ_ALGO_AGG_MAX | FJ_ALGO_AGG_SIGNED | FJ_ALGO_AGG_FLOAT) : 0) |  // modifiers of FJ_ALGO_BUILD_ORDER / FJ_ALGO_GROUP_BY: unknown without either
                          (gb ? FJ_ALGO_INVERSE | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_ARG | FJ_ALGO_KEY_PAIR | FJ_ALGO_GROUP_ROWS : 0) | (amerge ? FJ_ALGO_AGG_MERGE : 0);                                 // modifiers of FJ_ALGO_GROUP_BY: unknown without it
    if (gb) {                                                  // group-by on one relation (the build side): *out_keys g keys, *out_vals g aggregates; no probe side
        const bool amin = (algo & FJ_ALGO_AGG_MIN) != 0, amax = (algo & FJ_ALGO_AGG_MAX) != 0, asigned = (algo & FJ_ALGO_AGG_SIGNED) != 0;
        if (pagg) {                                            // (the checks of fj_join_device, before the context is created)
            if (many_host || left || anti || full || allc || po || bo)
                return set_err("fj_join_host: FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_%s (it groups one relation: there is no join in it)",
                               many_host ? "MANY_TO_MANY" : left ? "LEFT_OUTER" : anti ? "ANTI" : full ? "FULL_OUTER" : allc ? "ALL_COPIES" : po ? "PROBE_ORDER" : "BUILD_ORDER");
            if (amin || amax || rid || aarg || amerge)
                return set_err("fj_join_host: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_%s (out_vals is taken by column B and the four aggregates of the value column)",
                               amin ? "AGG_MIN" : amax ? "AGG_MAX" : rid ? "ROW_IDS" : aarg ? "AGG_ARG" : "AGG_MERGE");
            if (asigned && (algo & FJ_ALGO_AGG_FLOAT)) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs materialize = 1 (the pairs and their aggregates are the result)");
            if (!out_keys || !out_vals || (nb && (!bk || !bv || !pk)))
                return set_err("fj_join_host: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs build_keys, build_vals, probe_keys, out_keys and out_vals (the key columns A and B, the value column V, column A of the g groups and five planes of g words)");
            if (np != nb) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs np == nb, got np = %zu and nb = %zu (probe_keys is the value column of the one relation)", np, nb);
            if ((uint64_t)nb > (1ull << 40)) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", nb);
        }
        if (amerge) {                                          // FJ_ALGO_AGG_ALL's refusals under this flag's name, ahead of them
            if (many_host || left || anti || full || allc || po || bo)
                return set_err("fj_join_host: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_%s (it merges partial group-by rows: there is no join in it)",
                               many_host ? "MANY_TO_MANY" : left ? "LEFT_OUTER" : anti ? "ANTI" : full ? "FULL_OUTER" : allc ? "ALL_COPIES" : po ? "PROBE_ORDER" : "BUILD_ORDER");
            if (pk || np) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE takes no probe side (probe_keys must be NULL and np 0: the partial rows are the build side)");
            if (amin || amax) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_%s (it merges both the minima and the maxima)", amin ? "MIN" : "MAX");
            if (rid || inv || aarg) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_%s (a partial row is no row of a relation)", rid ? "ROW_IDS" : inv ? "INVERSE" : "AGG_ARG");
            if (asigned && (algo & FJ_ALGO_AGG_FLOAT)) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE needs materialize = 1 (the merged rows are the result)");
            if (!out_keys || !out_vals || (nb && !bv)) return set_err("fj_join_host: FJ_ALGO_AGG_MERGE needs build_vals, out_keys and out_vals (four planes of nb words - count, sum, min, max -, the g distinct keys and four planes of g words)");
        }
        if (many_host || left || anti || full || allc || po || bo)
            return set_err("fj_join_host: FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_%s (it groups one relation: there is no join in it)",
                           many_host ? "MANY_TO_MANY" : left ? "LEFT_OUTER" : anti ? "ANTI" : full ? "FULL_OUTER" : allc ? "ALL_COPIES" : po ? "PROBE_ORDER" : "BUILD_ORDER");
        if (!pagg && (pk || np)) return set_err("fj_join_host: FJ_ALGO_GROUP_BY takes no probe side (probe_keys must be NULL and np 0: the relation to group is the build side)");
        if (aall) {                                            // four aggregates: *out_vals is 4 * g words, plane-major with stride g
            if (amin || amax) return set_err("fj_join_host: FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_%s (it holds both the minimum and the maximum)", amin ? "MIN" : "MAX");
            if (rid || inv) return set_err("fj_join_host: FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_%s (out_vals is taken by the four aggregates)", rid ? "ROW_IDS" : "INVERSE");
            if (asigned && (algo & FJ_ALGO_AGG_FLOAT)) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_AGG_ALL needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)");
            if (!out_keys || !out_vals || (nb && !bv)) return set_err("fj_join_host: FJ_ALGO_AGG_ALL needs build_vals, out_keys and out_vals (the value column, the g distinct keys and four planes of g words)");
        }
        if (aarg) {                                            // the row of each group's extreme: *out_vals is 2 * g words, plane-major with stride g
            if (aall) return set_err("fj_join_host: FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_AGG_ALL (out_vals is taken by the four aggregates)");
            if (rid || inv) return set_err("fj_join_host: FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_%s (out_vals is taken by the row indices and the extremes)", rid ? "ROW_IDS" : "INVERSE");
            if (amin == amax) return set_err("fj_join_host: FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX (%s)", amin ? "both are set: call twice" : "neither is set");
            if (asigned && (algo & FJ_ALGO_AGG_FLOAT)) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_AGG_ARG needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)");
            if (!out_keys || !out_vals || (nb && !bv)) return set_err("fj_join_host: FJ_ALGO_AGG_ARG needs build_vals, out_keys and out_vals (the value column, the g distinct keys and two planes of g words)");
        }
        if (algo & FJ_ALGO_AGG_FLOAT) {                        // the value column and *out_vals hold IEEE-754 doubles
            if (asigned) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (rid || inv) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_%s (positions and group ids are integers)", rid ? "ROW_IDS" : "INVERSE");
            if (nb && !bv) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT with FJ_ALGO_GROUP_BY needs build_vals (the float64 value column, nb words: the count form has no float form)");
        }
        if (inv) {                                             // the group id of every row: *out_vals nb words, no aggregate beside it
            if (amin || amax || asigned)
                return set_err("fj_join_host: FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_%s (the ids group the rows once: every aggregate is a pass of the caller's over them)",
                               amin ? "MIN" : amax ? "MAX" : "SIGNED");
            if (rid) return set_err("fj_join_host: FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS (out_vals is taken: one per-call output)");
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_INVERSE needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)");
        }
        if (kpair) {                                           // the ids as above; *out_keys: the row index of every group's first occurrence
            if (!inv && !pagg) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR modifies FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE (the group ids of a two-column key are its result: FJ_ALGO_INVERSE is missing) or FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL (the pairs with four aggregates of a third column)");
            if (nb && !bv) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR needs build_vals (the second key column, nb words)");
            if ((uint64_t)nb > (1ull << 40)) return set_err("fj_join_host: FJ_ALGO_KEY_PAIR takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", nb);
        }
        if (grows) {                                           // the rows of every group: *out_keys g keys, *out_vals nb row indices then g starts
            if (!materialize) return set_err("fj_join_host: FJ_ALGO_GROUP_ROWS needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)");
            if ((uint64_t)nb > (1ull << 40)) return set_err("fj_join_host: FJ_ALGO_GROUP_ROWS takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", nb);
        }
        if (amin && amax) return set_err("fj_join_host: FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX (one aggregate per call: call twice)");
        if (asigned && !amin && !amax && !aall) return set_err("fj_join_host: FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX (the sum is taken modulo 2^64 and has no sign)");
        if ((amin || amax) && nb && !bv) return set_err("fj_join_host: FJ_ALGO_AGG_%s with FJ_ALGO_GROUP_BY needs build_vals (the value column, nb words)", amin ? "MIN" : "MAX");
        if (rid && (amin || amax)) return set_err("fj_join_host: FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_%s under FJ_ALGO_GROUP_BY (the first occurrence's position IS the aggregate)", amin ? "MIN" : "MAX");
        if (rid && !materialize) return set_err("fj_join_host: FJ_ALGO_ROW_IDS with FJ_ALGO_GROUP_BY needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)");
    }
    if (bo) {                                                  // build-order aggregate join: *out_keys nb counts, *out_vals nb sums (minima, maxima); bv = the PROBE values (np words)
        const bool amin = (algo & FJ_ALGO_AGG_MIN) != 0, amax = (algo & FJ_ALGO_AGG_MAX) != 0, asigned = (algo & FJ_ALGO_AGG_SIGNED) != 0;
        if (algo & FJ_ALGO_REUSE_BUILD)                        // onto a prepared build side, with or without FJ_ALGO_ACCUMULATE (that flag without this one: an unknown algo below)
            return set_err("fj_join_host: FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD%s is not served here (the internal context is shared by every host-buffer call of the process): call fj_join_device on a context of your own",
                           (algo & FJ_ALGO_ACCUMULATE) ? " | FJ_ALGO_ACCUMULATE" : "");
        if (many_host || left || anti || rid || full || allc || po)
            return set_err("fj_join_host: FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_%s (it has one row per build row, at the build row's position)",
                           many_host ? "MANY_TO_MANY" : left ? "LEFT_OUTER" : anti ? "ANTI" : rid ? "ROW_IDS" : full ? "FULL_OUTER" : allc ? "ALL_COPIES" : "PROBE_ORDER");
        if (algo & FJ_ALGO_AGG_FLOAT) {                        // the probe side's value column and *out_vals hold IEEE-754 doubles
            if (asigned) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)");
            if (np && !bv) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT with FJ_ALGO_BUILD_ORDER needs build_vals (here the probe side's float64 value column, np words: the count form has no float form)");
            if (!out_vals) return set_err("fj_join_host: FJ_ALGO_AGG_FLOAT with FJ_ALGO_BUILD_ORDER needs out_vals (the float64 aggregates; the counts alone are the plain count form)");
        }
        if (amin && amax) return set_err("fj_join_host: FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX (one aggregate per call: call twice)");
        if (asigned && !amin && !amax) return set_err("fj_join_host: FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX (the sum is taken modulo 2^64 and has no sign)");
        if (!materialize) return set_err("fj_join_host: FJ_ALGO_BUILD_ORDER needs materialize = 1 (its outputs are the result; P alone is the many-to-many counting join's)");
        if (!out_keys && !out_vals) return set_err("fj_join_host: FJ_ALGO_BUILD_ORDER needs an output (the counts out_keys, the sums out_vals, or both)");
        if ((amin || amax) && !out_vals) return set_err("fj_join_host: FJ_ALGO_AGG_%s needs out_vals (the counts alone are the plain count form of FJ_ALGO_BUILD_ORDER)", amin ? "MIN" : "MAX");
        if (np && out_vals && !bv) return set_err("fj_join_host: FJ_ALGO_BUILD_ORDER with out_vals needs build_vals (here the probe side's value column, np words)");
    }
    if (po) {                                                  // probe-order join: *out_vals np words, *out_keys np BYTES (the mask)
        if (algo & (FJ_ALGO_RETAIN_BUILD | FJ_ALGO_REUSE_BUILD))   // (without FJ_ALGO_PROBE_ORDER: unknown algos below)
            return set_err("fj_join_host: FJ_ALGO_%s_BUILD is not served here (the internal context is shared by every host-buffer call of the process): call fj_join_device on a context of your own",
                           (algo & FJ_ALGO_RETAIN_BUILD) ? "RETAIN" : "REUSE");
        if (many_host || left || anti || full || allc)
            return set_err("fj_join_host: FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_%s (it has one row per probe row, at the probe row's position)",
                           many_host ? "MANY_TO_MANY" : left ? "LEFT_OUTER" : anti ? "ANTI" : full ? "FULL_OUTER" : "ALL_COPIES");
        if (!materialize) return set_err("fj_join_host: FJ_ALGO_PROBE_ORDER needs materialize = 1 (its match count is the counting join's)");
        if (!out_keys && !out_vals) return set_err("fj_join_host: FJ_ALGO_PROBE_ORDER needs an output (out_vals, the byte mask out_keys, or both)");
        if (nb && out_vals && !rid && !bv) return set_err("fj_join_host: FJ_ALGO_PROBE_ORDER with out_vals needs build values (only FJ_ALGO_ROW_IDS and the mask alone read none)");
    }
    if (allc) {                                                // (the checks of fj_join_device, before the context is created)
        if (anti) return set_err("fj_join_host: FJ_ALGO_ALL_COPIES cannot be combined with FJ_ALGO_ANTI (an anti join has no copies to keep)");
        if (many_host) return set_err("fj_join_host: FJ_ALGO_ALL_COPIES cannot be combined with FJ_ALGO_MANY_TO_MANY (that flag alone is the inner join that keeps every copy)");
        if (!left && !full) return set_err("fj_join_host: unknown algo %d (FJ_ALGO_ALL_COPIES modifies FJ_ALGO_LEFT_OUTER or FJ_ALGO_FULL_OUTER; FJ_ALGO_MANY_TO_MANY is the inner form)", algo);
    }
    if (algo < 0 || (algo & ~(FJ_ALGO_MANY_TO_MANY | FJ_ALGO_LEFT_OUTER | FJ_ALGO_ANTI | FJ_ALGO_ROW_IDS | FJ_ALGO_FULL_OUTER | FJ_ALGO_ALL_COPIES | FJ_ALGO_PROBE_ORDER | FJ_ALGO_BUILD_ORDER | FJ_ALGO_GROUP_BY | agg_flags)) > 2) return set_err("fj_join_host: unknown algo %d", algo);
    if (rid && !materialize) return set_err("fj_join_host: FJ_ALGO_ROW_IDS needs materialize = 1 (it changes what the output rows hold)");
    if (left && anti) return set_err("fj_join_host: FJ_ALGO_LEFT_OUTER and FJ_ALGO_ANTI cannot be combined");
    if ((left || anti) && many_host) return set_err("fj_join_host: FJ_ALGO_%s cannot be combined with FJ_ALGO_MANY_TO_MANY", left ? "LEFT_OUTER" : "ANTI");
    if (left && !materialize) return set_err("fj_join_host: FJ_ALGO_LEFT_OUTER needs materialize = 1 (its match count is the counting join's)");
    if (full) {
        if (left || anti) return set_err("fj_join_host: FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_%s", left ? "LEFT_OUTER" : "ANTI");
        if (many_host) return set_err("fj_join_host: FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_MANY_TO_MANY");
        if (!materialize) return set_err("fj_join_host: FJ_ALGO_FULL_OUTER needs materialize = 1 (its match count is the counting join's)");
        if (nb && !bv && !rid) return set_err("fj_join_host: FJ_ALGO_FULL_OUTER needs build values (only FJ_ALGO_ROW_IDS reads none)");
        if (!out_count) return set_err("fj_join_host: FJ_ALGO_FULL_OUTER needs out_count (two words: matched probe rows, unmatched build rows)");
    }
    if (allc) {
        if (!materialize) return set_err("fj_join_host: FJ_ALGO_ALL_COPIES needs materialize = 1 (there is no counting-only form)");
        if (nb && !bv && !rid) return set_err("fj_join_host: FJ_ALGO_ALL_COPIES needs build values (only FJ_ALGO_ROW_IDS reads none)");
        if (!out_count) return set_err("fj_join_host: FJ_ALGO_ALL_COPIES needs out_count (three words: pairs, unmatched build rows, unmatched probe rows)");
    }
    const bool outer_mat = (left || anti) && materialize && !allc;      // left outer / anti join writing rows: np-row device buffers, no emit step
    {
        static std::mutex create_mu;
        std::lock_guard<std::mutex> lk(create_mu);
        if (!host_ctx()) {
            int dev = 0;
            if (const char* d = getenv("FJ_DEVICE")) dev = atoi(d);
            host_ctx() = fj_ctx_create(dev);
            if (!host_ctx()) return 1;
        }
    }
    fj_ctx* c = host_ctx();
    FJ_ENTER(c);
    // an earlier streamed call failed between stream_open and fj_stream_finish: nobody else can abort a stream join on this
    // internal context, so drop it here
    if (stream_abort(c) || begin_step(c, "fj_join_host")) return 1;
    void *dbk, *dbv, *dpk;
    if (get_buf(c, W_H_BK, nb * 8, &dbk) || get_buf(c, W_H_BV, (bo ? np : amerge ? 4 * nb : nb) * 8, &dbv) || get_buf(c, W_H_PK, np * 8, &dpk)) return 1;
    // pieces: >= 16 MiB (the ring's DMA and memcpy run at full rate), at most 48 of them for the probe side (the streamed
    // join takes <= 64 appends), a multiple of 4 KiB
    size_t piece = std::max<size_t>(16u << 20, (np * 8 + 47) / 48);
    piece = (piece + 4095) & ~(size_t)4095;
    if (c->stage_bytes < piece) {
        for (void*& p : c->stage) { if (p) { (void)hipHostFree(p); p = nullptr; } }
        c->stage_bytes = 0;
        for (void*& p : c->stage) HIPCHK(hipHostMalloc(&p, piece, hipHostMallocDefault));
        c->stage_bytes = piece;
    }
    const Options& opt = options();
    const bool use_radix = algo == FJ_ALGO_RADIX || (algo == FJ_ALGO_ADAPTIVE && nb >= opt.radix_threshold) ||
                           (algo == FJ_ALGO_SCALAR && !opt.scalar_hbm_table);
    // A counting join of the partitioned plan starts on the first piece: the build side is copied and partitioned, then every
    // probe piece gets its first partition pass while the next one crosses PCIe (the join hides under the copy; the bloom
    // precheck is skipped here - it saves device time the copy does not leave on the critical path).
    const bool streamed = use_radix && !materialize && nb > 0 && np > 0 && !many_host && !left && !anti && !full && !po && !bo;
    hipStream_t js = nullptr;
    auto t0 = std::chrono::steady_clock::now();
    unsigned cursor = 0;
    fj_timings t; memset(&t, 0, sizeof t); t.sampled_hit_bp = -1;
    u64 count = 0;
    bool joined = false;
    if (h2d_pipelined(c, dbk, bk, nb * 8, piece, &cursor, nullptr)) return 1;
    if (!streamed) {
        if ((anti && !bv) || rid || (po && !out_vals)) dbv = dbk;               // (an anti join reads no value, a row-id join none either, nor does a probe-order join's mask)
        else if (gb) {                                                          // the relation's value column: only the sum / min / max forms that return it read it
            if (kpair) { if (h2d_pipelined(c, dbv, bv, nb * 8, piece, &cursor, nullptr)) return 1; }      // (the second key column)
            else if (!bv || inv || grows) dbv = nullptr;
            else if (materialize && out_vals && h2d_pipelined(c, dbv, bv, (amerge ? 4 * nb : nb) * 8, piece, &cursor, nullptr)) return 1;   // (FJ_ALGO_AGG_MERGE: four planes)
        }
        else if (bo) {                                                          // the probe side's value column, read for the sums only
            if (!out_vals || !np) dbv = nullptr;
            else if (h2d_pipelined(c, dbv, bv, np * 8, piece, &cursor, nullptr)) return 1;
        }
        else if (h2d_pipelined(c, dbv, bv, nb * 8, piece, &cursor, nullptr)) return 1;
        if (h2d_pipelined(c, dpk, pk, np * 8, piece, &cursor, nullptr)) return 1;
        HIPCHK(hipStreamSynchronize(c->side));
    } else {
        HIPCHK(hipStreamSynchronize(c->side));                                  // build keys are in HBM
        const int appends = (int)((np * 8 + piece - 1) / piece);
        if (stream_open(c, nb, 1, np, appends, js, 64, piece / 8)) return 1;
        if (stream_append_build(c, (const u64*)dbk, nb, js)) return 1;
        if (stream_flush_build(c, c->st, js)) return 1;
        auto on_piece = [&](size_t off, size_t n, hipEvent_t landed) -> int {
            HIPCHK(hipStreamWaitEvent(js, landed, 0));
            return fj_stream_append_probe(c, (const u64*)((const char*)dpk + off), n / 8, js);
        };
        if (h2d_pipelined(c, dpk, pk, np * 8, piece, &cursor, on_piece)) return 1;
        uint64_t cnt = 0;
        if (fj_stream_finish(c, js, &cnt, &t)) return 1;          // (a partition beyond the LDS tables: it falls back to the HBM table by itself)
        count = cnt; joined = true;
    }
    const double h2d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    double d2h = 0;
    u64 full_r = 0;
    u64 ac[3] = {0, 0, 0};
    if (allc) {                                                                // every copy of a duplicated build key: count, exact-size device buffers, emit
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           ac, nullptr, nullptr, 0, &t)) return 1;
        count = ac[0];
        const size_t rows = (size_t)(ac[0] + ac[1] + ac[2]);
        void *dok, *dov;
        if (get_buf(c, W_H_OK, std::max<size_t>(rows, 1) * 8, &dok) || get_buf(c, W_H_OV, std::max<size_t>(rows, 1) * 8, &dov)) return 1;
        if (emit_pending(c, (u64*)dok, (u64*)dov, rows, js, &t)) return 1;
        if (out_keys && out_vals) {
            u64* hk = (u64*)malloc(std::max<size_t>(rows, 1) * 8);
            u64* hv = (u64*)malloc(std::max<size_t>(rows, 1) * 8);
            if (!hk || !hv) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", rows); }
            auto t1 = std::chrono::steady_clock::now();
            if (rows) { HIPCHK(hipMemcpy(hk, dok, rows * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(hv, dov, rows * 8, hipMemcpyDeviceToHost)); }
            d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            *out_keys = hk; *out_vals = hv;
        }
        joined = true;
    }
    if (full && !allc) {                                                                // full outer join: (np + nb)-row device buffers, np + r rows back
        void *dok, *dov;
        const size_t cap = np + nb;
        if (get_buf(c, W_H_OK, std::max<size_t>(cap, 1) * 8, &dok) || get_buf(c, W_H_OV, std::max<size_t>(cap, 1) * 8, &dov)) return 1;
        u64 counts[2] = {0, 0};
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           counts, (u64*)dok, (u64*)dov, cap, &t)) return 1;
        count = counts[0]; full_r = counts[1];
        const size_t rows = np + (size_t)full_r;
        if (out_keys && out_vals) {
            u64* hk = (u64*)malloc(std::max<size_t>(rows, 1) * 8);
            u64* hv = (u64*)malloc(std::max<size_t>(rows, 1) * 8);
            if (!hk || !hv) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", rows); }
            auto t1 = std::chrono::steady_clock::now();
            if (rows) { HIPCHK(hipMemcpy(hk, dok, rows * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(hv, dov, rows * 8, hipMemcpyDeviceToHost)); }
            d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            *out_keys = hk; *out_vals = hv;
        }
        joined = true;
    }
    if (outer_mat) {
        void *dok, *dov = nullptr;
        if (get_buf(c, W_H_OK, std::max<size_t>(np, 1) * 8, &dok) || (left && get_buf(c, W_H_OV, std::max<size_t>(np, 1) * 8, &dov))) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           &count, (u64*)dok, (u64*)dov, np, &t)) return 1;
        const size_t rows = left ? np : count;                                 // LEFT: every probe row; ANTI: the unmatched keys
        if (out_keys && (out_vals || !left)) {
            u64* hk = (u64*)malloc(std::max<size_t>(rows, 1) * 8);
            u64* hv = left ? (u64*)malloc(std::max<size_t>(rows, 1) * 8) : nullptr;
            if (!hk || (left && !hv)) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", rows); }
            auto t1 = std::chrono::steady_clock::now();
            if (rows) { HIPCHK(hipMemcpy(hk, dok, rows * 8, hipMemcpyDeviceToHost)); if (left) HIPCHK(hipMemcpy(hv, dov, rows * 8, hipMemcpyDeviceToHost)); }
            d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            *out_keys = hk;
            if (out_vals) *out_vals = hv;
        }
        joined = true;
    }
    if (po) {                                                                  // np words and / or np bytes, in probe order; no emit step
        void *dmask = nullptr, *dov = nullptr;
        if ((out_keys && get_buf(c, W_H_OK, std::max<size_t>(np, 1), &dmask)) || (out_vals && get_buf(c, W_H_OV, std::max<size_t>(np, 1) * 8, &dov))) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           &count, (u64*)dmask, (u64*)dov, np, &t)) return 1;
        void* hm = out_keys ? malloc(std::max<size_t>(np, 1)) : nullptr;
        u64* hv = out_vals ? (u64*)malloc(std::max<size_t>(np, 1) * 8) : nullptr;
        if ((out_keys && !hm) || (out_vals && !hv)) { free(hm); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", np); }
        auto t1 = std::chrono::steady_clock::now();
        if (np && hm) HIPCHK(hipMemcpy(hm, dmask, np, hipMemcpyDeviceToHost));
        if (np && hv) HIPCHK(hipMemcpy(hv, dov, np * 8, hipMemcpyDeviceToHost));
        d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (out_keys) *out_keys = (uint64_t*)hm;
        if (out_vals) *out_vals = hv;
        joined = true;
    }
    if (bo) {                                                                  // nb counts and / or nb sums (minima, maxima), in build order; no emit step
        void *dcnt = nullptr, *dsum = nullptr;
        if ((out_keys && get_buf(c, W_H_OK, std::max<size_t>(nb, 1) * 8, &dcnt)) || (out_vals && get_buf(c, W_H_OV, std::max<size_t>(nb, 1) * 8, &dsum))) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           &count, (u64*)dcnt, (u64*)dsum, nb, &t)) return 1;
        u64* hc = out_keys ? (u64*)malloc(std::max<size_t>(nb, 1) * 8) : nullptr;
        u64* hs = out_vals ? (u64*)malloc(std::max<size_t>(nb, 1) * 8) : nullptr;
        if ((out_keys && !hc) || (out_vals && !hs)) { free(hc); free(hs); return set_err("fj_join_host: out of host memory for %zu rows", nb); }
        auto t1 = std::chrono::steady_clock::now();
        if (nb && hc) HIPCHK(hipMemcpy(hc, dcnt, nb * 8, hipMemcpyDeviceToHost));
        if (nb && hs) HIPCHK(hipMemcpy(hs, dsum, nb * 8, hipMemcpyDeviceToHost));
        d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (out_keys) *out_keys = hc;
        if (out_vals) *out_vals = hs;
        joined = true;
    }
    if (aall || aarg) {                                                        // g keys and four (FJ_ALGO_AGG_ARG: two; with FJ_ALGO_KEY_PAIR: five) planes of g words; the device planes have stride nb
        void *dok = nullptr, *dov = nullptr;
        const size_t cap = std::max<size_t>(nb, 1), planes = pagg ? 5 : aall ? 4 : 2;
        if (get_buf(c, W_H_OK, cap * 8, &dok) || get_buf(c, W_H_OV, planes * cap * 8, &dov)) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, pagg ? (const u64*)dpk : nullptr, pagg ? np : 0, js, 64,   // (the pair form's value column)
                           &count, (u64*)dok, (u64*)dov, cap, &t)) return 1;
        const size_t g = (size_t)count;
        u64* hk = (u64*)malloc(std::max<size_t>(g, 1) * 8);
        u64* hv = (u64*)malloc(std::max<size_t>(g, 1) * planes * 8);
        if (!hk || !hv) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", g); }
        auto t1 = std::chrono::steady_clock::now();
        if (g) {
            HIPCHK(hipMemcpy(hk, dok, g * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy2D(hv, g * 8, dov, cap * 8, g * 8, planes, hipMemcpyDeviceToHost));
        }
        d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        *out_keys = hk; *out_vals = hv;
        joined = true;
    }
    if (grows) {                                                               // g keys; nb row indices and, behind them, g starts (the device planes have stride nb)
        void *dok = nullptr, *dov = nullptr;
        const size_t cap = std::max<size_t>(nb, 1);
        if (get_buf(c, W_H_OK, cap * 8, &dok) || get_buf(c, W_H_OV, 2 * cap * 8, &dov)) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, nullptr, nb, nullptr, 0, js, 64,
                           &count, (u64*)dok, (u64*)dov, cap, &t)) return 1;
        const size_t g = (size_t)count;
        u64* hk = out_keys ? (u64*)malloc(std::max<size_t>(g, 1) * 8) : nullptr;
        u64* hv = out_vals ? (u64*)malloc(std::max<size_t>(nb + g, 1) * 8) : nullptr;
        if ((out_keys && !hk) || (out_vals && !hv)) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", nb + g); }
        auto t1 = std::chrono::steady_clock::now();
        if (g && hk) HIPCHK(hipMemcpy(hk, dok, g * 8, hipMemcpyDeviceToHost));
        if (nb && hv) {
            HIPCHK(hipMemcpy(hv, dov, nb * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hv + nb, (const u64*)dov + cap, g * 8, hipMemcpyDeviceToHost));
        }
        d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (out_keys) *out_keys = hk;
        if (out_vals) *out_vals = hv;
        joined = true;
    }
    if (gb && !aall && !aarg && !grows) {                                                        // g <= nb keys and aggregates; exactly g rows go back (FJ_ALGO_INVERSE: g keys, nb ids)
        void *dok = nullptr, *dov = nullptr;
        const bool ids = inv && (out_vals || kpair);                            // (nobody takes the ids: the plain distinct form - which a two-column key does not have)
        if (inv && !ids) algo &= ~FJ_ALGO_INVERSE;
        if (materialize && (get_buf(c, W_H_OK, std::max<size_t>(nb, 1) * 8, &dok) || ((out_vals || ids) && get_buf(c, W_H_OV, std::max<size_t>(nb, 1) * 8, &dov)))) return 1;
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, nullptr, 0, js, 64,
                           &count, (u64*)dok, (u64*)dov, nb, &t)) return 1;
        if (materialize) {
            const size_t g = (size_t)count;
            u64* hk = out_keys ? (u64*)malloc(std::max<size_t>(g, 1) * 8) : nullptr;
            const size_t gv = ids ? nb : g;
            u64* hv = out_vals ? (u64*)malloc(std::max<size_t>(gv, 1) * 8) : nullptr;
            if ((out_keys && !hk) || (out_vals && !hv)) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %zu rows", std::max(g, gv)); }
            auto t1 = std::chrono::steady_clock::now();
            if (g && hk) HIPCHK(hipMemcpy(hk, dok, g * 8, hipMemcpyDeviceToHost));
            if (gv && hv) HIPCHK(hipMemcpy(hv, dov, gv * 8, hipMemcpyDeviceToHost));
            d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            if (out_keys) *out_keys = hk;
            if (out_vals) *out_vals = hv;
        }
        joined = true;
    }
    if (!joined) {
        if (fj_join_device(c, algo, bloom, materialize, (const u64*)dbk, (const u64*)dbv, nb, (const u64*)dpk, np, js, 64,
                           &count, nullptr, nullptr, 0, &t)) return 1;
    }
    if (materialize && c->pend.valid) {
        void *dok, *dov;
        if (get_buf(c, W_H_OK, count * 8, &dok) || get_buf(c, W_H_OV, count * 8, &dov)) return 1;
        if (emit_pending(c, (u64*)dok, (u64*)dov, count, js, &t)) return 1;
        if (out_keys && out_vals) {
            u64* hk = (u64*)malloc(std::max<size_t>(count, 1) * 8);
            u64* hv = (u64*)malloc(std::max<size_t>(count, 1) * 8);
            if (!hk || !hv) { free(hk); free(hv); return set_err("fj_join_host: out of host memory for %llu pairs", (unsigned long long)count); }
            auto t1 = std::chrono::steady_clock::now();
            if (count) { HIPCHK(hipMemcpy(hk, dok, count * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(hv, dov, count * 8, hipMemcpyDeviceToHost)); }
            d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            *out_keys = hk; *out_vals = hv;
        }
    }
    // h2d_ms: wall time from the first byte copied to the last piece enqueued + joined when the join was streamed under the
    // copy (then total_ms, the device-resident time, lies INSIDE it), else the copies alone
    t.h2d_ms = h2d; t.d2h_ms = d2h;
    t.host_streamed = joined && !outer_mat && !full && !allc && !po && !bo && !gb ? 1 : 0;
    last_timings() = t;
    if (out_count) *out_count = count;
    if (full && !allc) out_count[1] = full_r;
    if (allc) { out_count[1] = ac[1]; out_count[2] = ac[2]; }
    if (out_seconds) *out_seconds = t.total_ms * 1e-3;
    return 0;
}

}  // extern "C"