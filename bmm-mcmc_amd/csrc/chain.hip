// chain.hip -- host driver and C ABI (include/bmm_mcmc.h) of the allocation path.
//
// One bmm_chain = one MCMC chain resident on one GPU: the data matrix, the label
// rows, the integer sufficient statistics, the table image and every trace live in
// HBM; the host only enqueues kernels on the chain's stream.  The sweep loop mirrors
// the reference's (collapsed_gibbs.cpp:84-225, collapsed_gibbs_dp.cpp:98-283,
// stickbreaking.cpp:66-236) with the per-observation loop replaced by batches.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is opened with dlopen when a run spans devices

#include <dlfcn.h>
#include <emmintrin.h>
#include <sched.h>
#include <sys/mman.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

#include "../../include/bmm_mcmc.h"
#include "kernels.hip.h"
#include "ensemble.hip.h"
#include "host_crew.h"

using namespace bmm;
using bmm_host::HostCrew;
using bmm_host::host_threads;

namespace {

thread_local char g_err[512] = "";

// Kernel-steering environment hooks exist only in the test variant of the library
// (-DBMM_DEBUG_HOOKS, lib/libbmmmcmc_hip_dbg.so, built next to the product by the tests):
// the product library never reads the environment.
#ifdef BMM_DEBUG_HOOKS
const char* dbg_env(const char* name) { return getenv(name); }
#else
const char* dbg_env(const char*) { return nullptr; }
#endif

// Test variant only (BMM_DEBUG_FAKE_DEVICES=n): the library then accepts device indices 0 .. n-1, all of them the one
// real device underneath, keeps them apart wherever it reasons about which chains share a device (bmm_multi_run's
// placement, bmm_chain_share_data, bmm_chains_broadcast_planes), and replaces the RCCL broadcast between them by
// device-to-device copies.  What a one-GPU box can run of the multi-device bookkeeping -- every line of it but the
// collective itself, which bmm_multi_selfcheck runs on the device there is.  The product library has no such mode.
int fake_devices() {
    const char* v = dbg_env("BMM_DEBUG_FAKE_DEVICES");
    const int n = v ? atoi(v) : 0;
    return n > 1 ? n : 0;
}

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return set_err(BMM_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                           __FILE__, __LINE__);                                                \
    } while (0)

// device scratch that is released on every return path
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// No C++ exception may cross the C ABI: the entry points that allocate on the host or start threads run
// their bodies through this.
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return set_err(BMM_E_ARG, "out of host memory");
    } catch (const std::exception& e) {
        return set_err(BMM_E_STATE, "unexpected host error: %s", e.what());
    } catch (...) {
        return set_err(BMM_E_STATE, "unexpected host error");
    }
}
// host threads that are always joined, also when starting a later one throws
struct ThreadGroup {
    std::vector<std::thread> th;
    ~ThreadGroup() { join(); }
    void join() { for (std::thread& t : th) if (t.joinable()) t.join(); }
};

// Observations [a, b) of the N x P int32 column-major matrix R hands over, as bit planes: word w of
// observation i at plane[w][i - a0] (feature d at bit d % 32 of word d / 32, bits past P zero -- what
// k_pack_bits writes on the device).  Eight columns at a time into a block of output words that stays in L1:
// every cell of X is read once, in long contiguous runs, eight independent streams in flight per thread (one
// stream alone leaves a core at 6.5 GB/s, eight at 10).  Returns the OR of all cells read: the caller rejects
// the matrix when that has a bit other than bit 0 (data must be 0/1, as k_validate_binary checks).
uint32_t pack_rows_host(const int32_t* X, int64_t N, int P, int64_t a, int64_t b, uint32_t* const* plane, int64_t a0) {
    constexpr int64_t BL = 4096;
    constexpr int NS = 8;
    const int W = (P + 31) / 32;
    uint32_t seen = 0;
    for (int64_t r = a; r < b; r += BL) {
        const int64_t n = b - r < BL ? b - r : BL;
        for (int w = 0; w < W; ++w) {
            uint32_t* __restrict const o = plane[w] + (r - a0);
            const int d0 = 32 * w, nd = P - d0 < 32 ? P - d0 : 32;
            const uint32_t* const col = reinterpret_cast<const uint32_t*>(X) + (int64_t)d0 * N + r;
            int j = 0;
            for (; j + NS <= nd; j += NS) {
                const uint32_t* __restrict c[NS];
                for (int q = 0; q < NS; ++q) c[q] = col + (int64_t)(j + q) * N;
                for (int64_t t = 0; t < n; ++t) {
                    uint32_t acc = 0, s = 0;
                    for (int q = 0; q < NS; ++q) { const uint32_t v = c[q][t]; s |= v; acc |= v << q; }
                    seen |= s;
                    o[t] = j == 0 ? acc : (o[t] | (acc << j));
                }
            }
            for (; j < nd; ++j) {
                const uint32_t* __restrict const c0 = col + (int64_t)j * N;
                for (int64_t t = 0; t < n; ++t) { const uint32_t v = c0[t]; seen |= v; o[t] = j == 0 ? v : (o[t] | (v << j)); }
            }
        }
    }
    return seen;
}

// Pinned staging in pieces of 4 MiB that outlive a call: pinning costs about a millisecond per piece, a run
// needs two on the way in and two on the way out, and an R session calls the samplers again and again.  At
// most eight idle pieces are kept; the pool itself is never destroyed (no HIP call at process exit).
constexpr size_t kStageBytes = (size_t)4 << 20;
struct StagePool {
    std::mutex m;
    std::vector<void*> idle;
    void* get() {
        {
            std::lock_guard<std::mutex> g(m);
            if (!idle.empty()) { void* p = idle.back(); idle.pop_back(); return p; }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, kStageBytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    void put(void* p) noexcept {  // called from destructors: a piece that cannot be kept is freed
        if (!p) return;
        try {
            std::lock_guard<std::mutex> g(m);
            if (idle.size() < 8) { idle.push_back(p); return; }
        } catch (...) {
        }
        (void)hipHostFree(p);
    }
};
StagePool& stage_pool() { static StagePool* const pool = new StagePool(); return *pool; }
struct Stage {  // one piece, back to the pool on every return path
    void* p = stage_pool().get();
    ~Stage() { stage_pool().put(p); }
    Stage() = default;
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// All of a host matrix packed by the crew while the calling thread goes on (a *_run call creates its chain
// and uploads the starting state meanwhile).  The planes land in pinned pieces of the staging pool, one per
// plane, when a plane fits a piece and there are at most four (N <= 2^20, P <= 128: the upload then runs at
// PCIe speed, 0.15 instead of 0.6 ms for the 8 MB of the north-star shape); in ordinary host memory, [w][N],
// otherwise.
struct AsyncPack {
    std::unique_ptr<uint32_t[]> words;
    std::unique_ptr<Stage[]> pinned;
    std::vector<uint32_t*> plane;
    std::atomic<uint32_t> seen{0};
    HostCrew* crew = nullptr;
    void start(HostCrew* cr, const int32_t* X, int64_t N, int P) {
        const int W = (P + 31) / 32;
        crew = cr;
        plane.assign((size_t)W, nullptr);
        if (W <= 4 && (size_t)N * sizeof(uint32_t) <= kStageBytes) {
            pinned.reset(new Stage[(size_t)W]);
            bool ok = true;
            for (int w = 0; w < W; ++w) { plane[(size_t)w] = pinned[(size_t)w].as<uint32_t>(); ok = ok && plane[(size_t)w]; }
            if (!ok) pinned.reset();
        }
        if (!pinned) {
            words.reset(new uint32_t[(size_t)W * (size_t)N]);
            for (int w = 0; w < W; ++w) plane[(size_t)w] = words.get() + (size_t)w * (size_t)N;
        }
        uint32_t* const* const pl = plane.data();
        std::atomic<uint32_t>* const sn = &seen;
        crew->begin(N, 32768, 64, [X, N, P, pl, sn](int64_t lo, int64_t hi) {
            sn->fetch_or(pack_rows_host(X, N, P, lo, hi, pl, 0), std::memory_order_relaxed);
        });
    }
    void join() { if (crew) crew->wait(); }
    void release() { join(); words.reset(); pinned.reset(); plane.clear(); }
    ~AsyncPack() { join(); }
};

// Device memory of a finished call, kept for the next one: a chain's arena, a run's arena and the bit planes
// come from here.  hipMalloc is usually free on this runtime (0.02 ms) but now and then takes 10 ms and more
// when the driver has to map fresh memory (a 220-sweep call at N = 1e6 lasts 37 ms in all), and hipFree costs
// 0.2 ms a piece.  Per device at most six idle blocks and 512 MiB in all are kept; a request takes the smallest
// idle block that fits and is at most twice as large.  bmm_release_pools frees them.
struct DevPool {
    struct Block { void* p; size_t bytes; };
    std::mutex m;
    std::vector<Block> idle[64];
    static constexpr size_t kMaxIdleBytes = (size_t)512 << 20;
    void* get(int device, size_t bytes, size_t* got) {
        if (device >= 0 && device < 64) {
            std::lock_guard<std::mutex> g(m);
            std::vector<Block>& v = idle[device];
            int best = -1;
            for (int i = 0; i < (int)v.size(); ++i)
                if (v[(size_t)i].bytes >= bytes && v[(size_t)i].bytes <= 2 * bytes + 4096 && (best < 0 || v[(size_t)i].bytes < v[(size_t)best].bytes)) best = i;
            if (best >= 0) {
                const Block b = v[(size_t)best];
                v.erase(v.begin() + best);
                *got = b.bytes;
                return b.p;
            }
        }
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;  // the caller reports hipGetLastError
        *got = bytes;
        return p;
    }
    void put(int device, void* p, size_t bytes) noexcept {
        if (!p) return;
        try {
            if (device >= 0 && device < 64) {
                std::lock_guard<std::mutex> g(m);
                std::vector<Block>& v = idle[device];
                if (bytes <= kMaxIdleBytes) {  // the newest block stays, the oldest go: a session repeats its last shape
                    size_t held = bytes;
                    for (const Block& b : v) held += b.bytes;
                    while (!v.empty() && (v.size() >= 6 || held > kMaxIdleBytes)) {
                        held -= v.front().bytes;
                        (void)hipFree(v.front().p);
                        v.erase(v.begin());
                    }
                    v.push_back(Block{p, bytes});
                    return;
                }
            }
        } catch (...) {
        }
        (void)hipFree(p);
    }
};
DevPool& dev_pool() { static DevPool* const pool = new DevPool(); return *pool; }

// pinned host staging that is released on every return path
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create() {
        hipError_t r = hipEventCreateWithFlags(&e[0], hipEventDisableTiming);
        return r == hipSuccess ? hipEventCreateWithFlags(&e[1], hipEventDisableTiming) : r;
    }
};

// ---- progress reports and phase times of the *_run entry points (per calling thread)
struct Progress { bmm_progress_fn fn = nullptr; void* user = nullptr; int every = 0; };
thread_local Progress g_progress;
thread_local double g_phase_ms[BMM_RUN_PHASES] = {0, 0, 0, 0, 0, 0};
struct PhaseClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(int phase) {
        const auto n = std::chrono::steady_clock::now();
        g_phase_ms[phase] += std::chrono::duration<double, std::milli>(n - t).count();
        t = n;
    }
};

// A list of integers known at compile time, and the one lift from run-time values to template arguments: for
// each (list, value) pair the element equal to the value is handed to f as a std::integral_constant, all of
// them in one call.  False, and f not called, when some value is in none of its list's elements.
template <int... V> struct IntList {};
template <class F> bool lift(F&& f) { f(); return true; }
template <class F, int... V, class... Rest>
bool lift(F&& f, IntList<V...>, int v, Rest... rest) {
    return ((v == V && lift([&](auto... c) { f(std::integral_constant<int, V>{}, c...); }, rest...)) || ...);
}

// accumulator counts the resample and predictive kernels are instantiated for
constexpr IntList<4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64> kKT{};  // (52: maxK = 50, BASELINE config 4)
template <int... V>
int pick_kt(IntList<V...>, int cats) { for (int kt : {V...}) if (kt >= cats) return kt; return -1; }
int pick_kt(int cats) { return pick_kt(kKT, cats); }

// workgroup size by accumulator count: the VGPR budget per lane is 512 / (waves per SIMD)
constexpr int kThreadsSmall = 1024;  // KT <= 12: 128 VGPRs
constexpr int kThreadsMid = 768;     // KT 16, 20: 168 VGPRs
constexpr int kThreadsLarge = 512;   // 256 VGPRs
constexpr int kThreadsSplit = 1024;  // two lanes per observation (SPLIT = 2 in kernels.hip.h)
#ifndef BMM_STREAM_MODE
#define BMM_STREAM_MODE 2  // chains that share a device: a hardware queue of its own each (chain_stream_create)
#endif
#ifndef BMM_STAGE_WIDE
#define BMM_STAGE_WIDE 32
#endif
#ifndef BMM_SMALL_SPLIT
#define BMM_SMALL_SPLIT 1  // short launches of 16-32 accumulators run two lanes per observation (plan_kernel)
#endif
#ifndef BMM_SELF_TABLES
#define BMM_SELF_TABLES 1  // small finite-sampler shapes: resample workgroups build their own tables (plan_kernel)
#endif
constexpr int kStageWide = BMM_STAGE_WIDE;  // features in flight per wave where registers allow

// The default workgroup size of the one-lane kernels.  The bit-plane kernel holds no feature loads in flight,
// which frees 20-odd VGPRs: one size up.
constexpr int threads_for(int kt, bool bits) {
    if (bits) return kt <= 20 ? kThreadsSmall : (kt <= 32 ? kThreadsMid : kThreadsLarge);
    return kt <= 12 ? kThreadsSmall : (kt <= 20 ? kThreadsMid : kThreadsLarge);
}

// One instantiation of k_resample, named by what bmm_dbg_kernel_key reports of it.
struct KernelForm {
    int kt = 0;         // accumulators
    int nt = 0;         // threads per workgroup
    int minus = 0;      // own-cluster tables: 0 none (stick-breaking / full), 1 in LDS, 2 in global memory
    bool bits = false;  // X streamed as bit planes (k_pack_bits) instead of the int32 matrix as handed over
    int lanes = 1;      // lanes per observation (SPLIT)
    bool emit = false;  // the weight-emitting twin: what a sweep runs on while its probabilities go to the host
    int gw = kGroupW;   // the shape's group width (bmm_spec.h)
    bool self = false;  // workgroups that build their own table image (SELF)
    bool pk = false;    // k_resample_pk: scores from the packed binary32 image, the definition for the uncertain few
    bool pipe = false;  // ... its second body: the plain trip with unrolled group steps (pk_pipelined, kernels.hip.h)
};
constexpr int tile_of(const KernelForm& f) { return f.nt / f.lanes; }  // observations per tile
constexpr KernelForm resized(KernelForm f, int nt, int lanes = 1) { f.nt = nt; f.lanes = lanes; return f; }
// The emitting twin of a bit-plane chain's kernel: default-sized and one lane per observation whatever the
// chain itself runs (any workgroup size serves any batch), same tables.
constexpr KernelForm emit_twin(const KernelForm& f) {
    return KernelForm{f.kt, threads_for(f.kt, true), f.minus, true, 1, true, f.gw, false};
}

// STG, the one template argument that is not part of the form: features in flight per wave.  16 wherever
// registers are short -- bit planes, more than 20 accumulators, the 256-thread kernels -- and kStageWide
// otherwise, with one exception in either direction at 1024 threads (128 VGPRs): a size that was named
// (BMM_DEBUG_THREADS, the experiment knob of tools/try_threads.sh) gets 16 by that register rule, while the
// default kernel of 4-12 accumulators, which has that size by threads_for, keeps the measured kStageWide.  So
// the int32 kernel of 4-12 accumulators at 1024 threads exists twice, and named_size tells the two apart.
constexpr int stage_width(const KernelForm& f, bool named_size) {
    if (f.bits || f.kt > 20 || f.nt == 256) return 16;
    if (f.nt == kThreadsSmall) return f.nt == threads_for(f.kt, false) && !named_size ? kStageWide : 16;
    return kStageWide;
}

// Which forms are instantiated: the whole kernel set of the library.  (accumulator counts: those of kKT)
constexpr bool instantiated(const KernelForm& f, bool named_size) {
    const bool preferred = f.gw == kGroupW;
    // the packed kernel: the plain bit-plane form (one lane, own-cluster tables in LDS) up to 32 accumulators, at
    // every workgroup size for the preferred width and at the default size for the narrower one
    if (f.pk) return f.bits && f.lanes == 1 && f.minus == 1 && !f.emit && !f.self && f.kt <= 32 &&
                     (preferred || (f.gw == kGroupWAlt && f.nt == threads_for(f.kt, true)));
    // SELF: 256-thread workgroups that build their own table image (finite sampler, small shapes: kernels.hip.h)
    if (f.self) return f.kt <= 12 && f.nt == 256 && f.minus == 1 && f.bits && f.lanes == 1 && !f.emit && preferred;
    // EMIT: the twins of the default-sized bit-plane kernels, every tier and width
    if (f.emit) return f.bits && f.lanes == 1 && f.nt == threads_for(f.kt, true);
    // two lanes per observation, bit planes: more than 32 accumulators at either width, 16 to 32 (for launches too
    // short to give a wave more than a chunk or two) at the preferred one; own-cluster tables from LDS only
    if (f.lanes == 2) return f.bits && f.nt == kThreadsSplit && f.minus != 2 && (f.kt > 32 || (f.kt >= 16 && preferred));
    if (f.lanes != 1) return false;
    // the default-sized kernels: every tier, both layouts, both widths
    if (f.nt == threads_for(f.kt, f.bits) && !named_size) return true;
    // other workgroup sizes for the preferred width only (shapes that fall back to the narrower groups are the
    // ones with big tables), and not with the own-cluster tables in global memory:
    if (!preferred || f.minus == 2) return false;
    // 256 threads: used when a batch is too small to give every CU a workgroup otherwise
    if (f.nt == 256) return true;
    // a chosen size up to 32 accumulators: the stepped-down workgroups of a batch too small to give every CU a
    // default-sized one (bit planes), and BMM_DEBUG_THREADS (the int32 layout with own-cluster tables in LDS only)
    return (f.nt == 1024 || f.nt == 768 || f.nt == 512) && f.kt <= 32 && (f.bits || f.minus == 1);
}

typedef void (*resample_fn)(ChainParams, ResampleArgs);
// The instantiation a form names, nullptr when there is none.  Nothing outside `instantiated` is instantiated.
template <int KT, int NT, int MINUS, bool BITS, int GW, int LANES, bool EMIT, bool SELF, bool NAMED>
resample_fn instance() {
    constexpr KernelForm F{KT, NT, MINUS, BITS, LANES, EMIT, GW, SELF};
    if constexpr (instantiated(F, NAMED)) return k_resample<KT, NT, MINUS, stage_width(F, NAMED), BITS, LANES, EMIT, GW, SELF>;
    else return nullptr;
}
resample_fn lookup(const KernelForm& f, bool named_size = false) {
    resample_fn fn = nullptr;
    if (f.pk) {
        if (!instantiated(f, named_size) || (f.pipe && !pk_pipelined(f.kt, f.nt, f.gw))) return nullptr;
        lift([&](auto kt, auto nt, auto gw) {
            if constexpr (instantiated(KernelForm{kt, nt, 1, true, 1, false, gw, false, true}, false)) {
                // the present body of every form; the second one of the forms that take it (BMM_DEBUG_PK_NOPIPE
                // runs the present body where the second one would run)
                fn = k_resample_pk<kt, nt, gw, false>;
                if constexpr (pk_pipelined(kt, nt, gw)) if (f.pipe) fn = k_resample_pk<kt, nt, gw, true>;
            }
        }, kKT, f.kt, IntList<1024, 768, 512, 256>{}, f.nt, IntList<kGroupW, kGroupWAlt>{}, f.gw);
        return fn;
    }
    lift([&](auto kt, auto nt, auto minus, auto bits, auto gw) {
        // two lanes, EMIT, SELF and a named size come one at a time (lifting them as well would cost the compiler
        // sixteen times the combinations for the same five)
        if (f.lanes == 2) fn = f.emit || f.self ? nullptr : instance<kt, nt, minus, bits != 0, gw, 2, false, false, false>();
        else if (f.lanes != 1 || (f.emit && f.self)) fn = nullptr;
        else if (f.emit) fn = instance<kt, nt, minus, bits != 0, gw, 1, true, false, false>();
        else if (f.self) fn = instance<kt, nt, minus, bits != 0, gw, 1, false, true, false>();
        else if (named_size) fn = instance<kt, nt, minus, bits != 0, gw, 1, false, false, true>();
        else fn = instance<kt, nt, minus, bits != 0, gw, 1, false, false, false>();
    }, kKT, f.kt, IntList<1024, 768, 512, 256>{}, f.nt, IntList<0, 1, 2>{}, f.minus, IntList<0, 1>{}, (int)f.bits,
       IntList<kGroupW, kGroupWAlt>{}, f.gw);
    return fn;
}

// The scorer of stored states (k_score) by accumulator count, group width, own-label tier (0 none: the predictive, and
// the leave-one-out of the explicit samplers; 1 the minus-self tables in LDS, 2 in global memory) and tail (the
// predictive's or the leave-one-out's): one workgroup size, one lane per row.  With an own-label pass the kernel needs
// about 7.5 VGPRs per accumulator (code-object metadata: 118 at 12 accumulators, 256 at 32) and from 40 accumulators on
// would use scratch, so those forms are not instantiated: nullptr, and the chain's rows are scored by k_score_generic
// (loo_setup).  Without one 64 accumulators take 191 VGPRs.
constexpr int kLooMaxOwnKT = 32;
typedef void (*score_fn)(ChainParams, ScoreArgs);
score_fn lookup_score(int kt, int gw, int minus, bool loo) {
    score_fn fn = nullptr;
    lift([&](auto KT, auto GW, auto MINUS) {
        if constexpr (MINUS == 0) fn = loo ? k_score<KT, kScoreThreads, GW, 0, true> : k_score<KT, kScoreThreads, GW, 0, false>;
        else if constexpr (KT <= kLooMaxOwnKT) fn = loo ? k_score<KT, kScoreThreads, GW, MINUS, true> : nullptr;
    }, kKT, kt, IntList<kGroupW, kGroupWAlt>{}, gw, IntList<0, 1, 2>{}, minus);
    return fn;
}

constexpr size_t kLdsMax = 163840;  // gfx950: 160 KiB per workgroup

// The masked scorer of incomplete new rows.  Which form runs is a pure function of the shape:
// the LDS form (k_score_na: kScoreThreads lanes, the whole split image staged) when the shape has a resident kernel and
// the doubled head with the constants and the exp256 table fits in LDS; the global form (k_score_na_generic: 256
// threads, tables from L2, scores in scratch columns) otherwise.  bmm_predict_na_plan reports it, the launches read it.
typedef void (*na_score_fn)(ChainParams, NaScoreArgs);
struct NaForm { bool lds; size_t lds_bytes; int threads; size_t table_bytes; };
NaForm na_form_of(const ChainParams& p, bool generic) {
    const size_t bytes = (size_t)split_layout_of(p).doubles() * sizeof(double);
    const bool lds = !generic && bytes <= kLdsMax;
    return NaForm{lds, lds ? bytes : 0, lds ? kScoreThreads : 256, bytes};
}
na_score_fn lookup_score_na(int kt, int gw) {
    na_score_fn fn = nullptr;
    lift([&](auto KT, auto GW) { fn = k_score_na<KT, kScoreThreads, GW>; }, kKT, kt, IntList<kGroupW, kGroupWAlt>{}, gw);
    return fn;
}
// The one place a kernel is set up for launching with `lds` bytes of dynamic LDS: the attribute that allows
// them, and how many of its workgroups of nt threads the runtime then fits on a CU.
template <class Fn>
hipError_t kernel_fits(Fn fn, int nt, size_t lds, int* blocks_per_cu) {
    *blocks_per_cu = 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, reinterpret_cast<const void*>(fn), nt, lds);
    return e;
}

// What a chain records per sweep for one consumer (the predictive, the leave-one-out summary, the indicator step,
// the allocation sampler's K): while `fold` is set, sweeps j >= from are folded into the consumer's accumulators;
// p: or rows of row_bytes on the device, row j - base receiving sweep j's values.  Installed by a Recording.
struct SweepTrace {
    char* p = nullptr;
    size_t row_bytes = 0;
    int base = 0, from = 0;  // sweep indices
    bool fold = false;
    bool folds(int j) const { return fold && j >= from; }
    template <class T> T* row(int j) const { return p && j >= base ? reinterpret_cast<T*>(p + (size_t)(j - base) * row_bytes) : nullptr; }
};

// The posterior summary's device block, carved by sum_carve: the folds first (what a reset
// zeroes), then the pivot, the outputs of k_sum_finish, an identity permutation, the live sweep's agreement and
// permutation where no recording holds them, and the theta / alpha row of a sweep that no run trace records.
struct SumBufs {
    uint32_t* cnt = nullptr;  // [K][pitch]
    double *theta_sum = nullptr, *theta_sq = nullptr, *alpha_acc = nullptr;
    int32_t* theta_n = nullptr;
    size_t fold_bytes = 0;
    unsigned long long* size_sum = nullptr;
    int32_t *pivot = nullptr, *z_hat = nullptr, *identity = nullptr, *perm_live = nullptr;
    uint32_t* n_max = nullptr;
    int64_t* agree_live = nullptr;
    double *theta_row = nullptr, *alpha_row = nullptr;
};
struct EcrWork;

}  // namespace

struct bmm_chain {
    ChainParams p{};
    int device = 0;  // the HIP device
    HostCrew* crew = nullptr;  // the host threads of the *_run call this chain belongs to (not owned), if any
    int slot = 0;    // the device index the caller named (= device, except under BMM_DEBUG_FAKE_DEVICES)
    hipStream_t stream = nullptr;
    bool dedicated_queue = false;  // the stream has a hardware queue of its own (chains sharing a device)
    int stream_kind = 0;           // what the stream pool takes back: 1 an ordinary non-blocking stream, 2 one with its own queue, 0 neither
    bool shares_device = false;    // another chain runs beside this one on the device (bmm_chain_share_data)
    size_t lds_bytes_base = 0;     // lds_bytes without the SELF kernels' scratch
    int64_t batch = 1;
    double alpha0 = 1.0;
    int grid_max = 0, minus_in_lds = 1;
    bool sharded = false, shard_open = false;  // one chain over several ranks (explicit-parameter samplers)
    bool generic = false;         // shape beyond the resident kernel: tables from global memory
    double* dScratch = nullptr;   // generic path: per-thread score columns
    // allocation probabilities for the host's relabelling: while probs_dst is
    // set, every resample launch also emits its weights (dWts [Kc][N], dWtot [N]) and k_probs_finish
    // normalises them into probs_dst (N x K column-major, device)
    double *dProbs = nullptr, *dWts = nullptr, *dWtot = nullptr;
    double* probs_dst = nullptr;
    int64_t scratch_stride = 0;
    size_t lds_bytes = 0;
    // what the chain's launches run (pick_kernel; on the generic path `form` carries the key of k_resample_generic
    // and fn stays null), and the weight-emitting twin of a bit-plane chain: its form from the start, fn_emit and
    // its grid limit once the first hand-off has set it up (probs_alloc)
    KernelForm form, form_emit{};
    resample_fn fn = nullptr, fn_emit = nullptr;
    int grid_max_emit = 0;

    const int32_t* dX = nullptr;
    int32_t* dX_owned = nullptr;
    uint32_t* dXb = nullptr;      // bit planes of X (k_pack_bits), what the resident kernels stream by default
    // the planes are shared by reference count between the chains of a device that run over the same data
    // (bmm_chain_share_data): the last chain to go frees them, in whatever order chains are destroyed
    struct Planes { uint32_t* d = nullptr; size_t bytes = 0; std::atomic<int> refs{1}; };
    Planes* planes = nullptr;
    bool xb_borrowed = false;     // this chain took its planes from another one
    bool bits = false;
    int num_cus = 0;
    // the chain's fixed state is carved out of one allocation (arena), the buffers of a *_run call out of a
    // second one (run_arena): a malloc / free pair per buffer cost the drop-in call more than a millisecond
    char *arena = nullptr, *run_arena = nullptr;
    size_t arena_bytes = 0, run_arena_bytes = 0;  // as handed out by the device pool
    int32_t* dZ[2] = {nullptr, nullptr};
    int32_t *dNk = nullptr, *dS = nullptr, *dDNk = nullptr, *dDS = nullptr;
    double *dAlpha = nullptr, *dTab = nullptr, *dPi = nullptr, *dTheta = nullptr;
    bool have_data = false, have_init = false, started = false;
    int sweep = 0;  // sweeps completed (= index j of the last one)

    // trace of the *_run entry points
    int burnin = 0, S = 0;
    int32_t* dTrace = nullptr;  // [S][N], 0-based
    double *dThetaTrace = nullptr, *dAlphaTrace = nullptr, *dPiTrace = nullptr;
    char* dOutBlk[2] = {nullptr, nullptr};  // staging of the label trace on its way out (trace_out)
    size_t out_blk_bytes = 0;

    int32_t* dNkTrace = nullptr;  // [n][K] cluster sizes per sweep of the current sweeps_counts call
    int nk_trace_base = 0;        // sweep index of its row 0
    unsigned long long* dDiag = nullptr;
    int* dViable = nullptr;       // stick-breaking / full: the cluster count the concentration's update uses (k_sb_params -> k_sb_theta_tables)
    int* dSelfDone = nullptr;     // SELF kernels: workgroups of the running launch that have read the statistics
    int32_t *dDNkAlt = nullptr, *dDSAlt = nullptr;  // ... and the second set of delta accumulators (self_fold_prev)
    unsigned long long* dPkStat = nullptr;  // -DBMM_DEBUG_HOOKS: k_resample_pk's draws and deferred observations
    int pk_defer_every = 0;       // -DBMM_DEBUG_HOOKS: BMM_DEBUG_PK_DEFER_EVERY as read when the chain was made
    int pk_mid_fail_every = 0;    //   ... and BMM_DEBUG_PK_MID_FAIL_EVERY
    int* dDbgFlag = nullptr;      // -DBMM_DEBUG_HOOKS: raised by a kernel that meets a label out of range
    // posterior predictive of new rows: their bit planes [ceil(P/32)][predM], the predictive
    // table image of the counting samplers (the explicit samplers' own image dTab is the predictive image), the
    // accumulators that live across sweeps, and what a sweep folds and records (pred_rec: rows of predM doubles)
    int64_t predM = 0;
    uint32_t* dXnb = nullptr;
    double *dPredTab = nullptr, *dPredMax = nullptr, *dPredSum = nullptr, *dRespAcc = nullptr;
    bool pred_resp = false;       // the responsibilities are accumulated too
    int pred_folded = 0;          // states folded so far
    score_fn pfn = nullptr;
    int pred_grid_max = 0;
    size_t pred_lds = 0;
    SweepTrace pred_rec;
    // ... of incomplete new rows: the mask planes (laid out as dXnb), the sorted cell list as
    // rows / CSR offsets / columns, the cell pairs that live across sweeps, the split image, and the launch of the
    // shape's form (na_form_of): pn_fn with pn_lds bytes, or k_score_na_generic on score columns (the chain's own on a
    // generic shape, dPnScratch otherwise).  pred_cells = 0: the new rows are complete and take k_score.
    int64_t pred_cells = 0;
    uint32_t* dPnMb = nullptr;
    int64_t *dPnRow = nullptr, *dPnOff = nullptr;
    int32_t* dPnCol = nullptr;
    double *dCellMax = nullptr, *dCellSum = nullptr, *dSplitTab = nullptr, *dPnScratch = nullptr;
    int64_t pn_scratch_stride = 0;
    na_score_fn pn_fn = nullptr;
    int pn_grid_max = 0;
    size_t pn_lds = 0;
    // leave-one-out predictive of the fitted rows: the two table sets of the counting samplers
    // (the explicit samplers score their own image dTab), the accumulators [kLooAcc][N] that live across sweeps, the
    // outputs of k_loo_finish ([kLooOut][N], then the scalars), and what a sweep folds and records (loo_rec: rows of N doubles)
    bool loo_on = false;
    double *dLooTab = nullptr, *dLooAcc = nullptr, *dLooOut = nullptr;
    bool loo_generic = false;    // a resident shape whose rows k_score_generic scores (lookup_score), on scratch columns of its own
    double* dLooScratch = nullptr;
    int64_t loo_scratch_stride = 0;
    int loo_folded = 0;          // states folded so far
    score_fn lfn = nullptr;
    int loo_minus = 0, loo_grid_max = 0;
    size_t loo_lds = 0;
    SweepTrace loo_rec;
    // split-merge moves: sm_moves > 0: that many moves at the start of every sweep from the
    // second; the side bytes, the final scan's log probabilities, the statistic sets of one move ([sm_sets]), the
    // move's cell and the five counters.  Moves are numbered within the sweep they precede (sm_tag, sm_ctr).
    int sm_moves = 0, sm_scans = 0, sm_sets = 0;
    uint8_t *dSmSide = nullptr, *dSmSideLaunch = nullptr;
    double* dSmLq = nullptr;
    int32_t* dSmStat = nullptr;
    SmCell* dSmCell = nullptr;
    long long* dSmCounters = nullptr;
    int sm_tag = -1;
    uint32_t sm_ctr = 0;
    // feature selection: fs_mask: the table builds read the inclusion mask (set once a mask
    // was given or the step armed, and for good: the kernel choice then leaves out the forms that build their own
    // tables); fs_on: a gamma-step behind every sweep end.  One block holds the mask words, the indicator bytes, the
    // step record [3][P] and the two accumulators; fs_rec: the steps that are folded (every one of an armed chain, the
    // kept ones of a run) and the rows of P indicator bytes they are recorded in.
    bool fs_mask = false, fs_on = false;
    double fs_rho = 0.5, fs_logit = 0.0;
    char* dFsBlock = nullptr;
    uint32_t *dFsMask = nullptr, *dFsCount = nullptr;
    uint8_t* dFsGamma = nullptr;
    double *dFsRec = nullptr, *dFsProb = nullptr;
    int fs_folded = 0, fs_last = -1;  // fs_last: the sweep of the last step, -1 none yet
    SweepTrace fs_rec;
    // categorical features: cat_on: the table builds are k_count_tables<TAB_CAT>, reading dCatLev (P
    // bytes: 0 a Bernoulli column, else the L of the column's block), and the kernel choice leaves out the forms that
    // build their own tables; cat_checked: k_cat_check has passed these levels over these data.  One block holds the
    // bytes, the block list and the check's key.
    bool cat_on = false, cat_checked = false;
    std::vector<int32_t> cat_levels;
    std::vector<CatBlock> cat_blocks;
    char* dCatBlock = nullptr;
    uint8_t* dCatLev = nullptr;
    CatBlock* dCatBlocks = nullptr;
    unsigned long long* dCatBad = nullptr;
    // the last k-modes++ initialisation, kept on the host: the k_eff centres [k_eff][W], the
    // picked rows and the final cluster sizes
    int init_keff = 0;
    std::vector<uint32_t> init_centres;
    std::vector<long long> init_rows;
    std::vector<int32_t> init_nk;
    // the allocation sampler: alloc_on: the table builds are k_count_tables<TAB_ALLOC>, reading the open
    // label count dEaK, and (for good) the kernel choice leaves out the forms that build their own tables; alloc_moves
    // > 0: that many eject / absorb moves at the start of every sweep from the second.  One block holds K, log p(K),
    // the moved rows' statistics, the move's cell and the four counters; the side bytes are a block of their own.
    bool alloc_on = false;
    int alloc_moves = 0;
    double alloc_a = 0.0, alloc_e = 1.0;
    char* dEaBlock = nullptr;
    int32_t *dEaK = nullptr, *dEaStat = nullptr;
    double* dEaLogPrior = nullptr;
    EaCell* dEaCell = nullptr;
    long long* dEaCounters = nullptr;
    uint8_t* dEaSide = nullptr;
    int ea_tag = -1;
    uint32_t ea_ctr = 0;
    SweepTrace k_rec;  // a run: one int32 per kept sweep, K after it
    // split-merge moves of the allocation chain: as_moves > 0: that many moves at the start of
    // every sweep from the second, behind its eject / absorb moves.  The side bytes, the log probabilities and the
    // statistic sets are the split-merge buffers above (a DP chain's moves are refused on an armed chain); one block
    // holds the move's cell and the five counters.
    int as_moves = 0, as_scans = 0;
    char* dAsBlock = nullptr;
    AsCell* dAsCell = nullptr;
    long long* dAsCounters = nullptr;
    int as_tag = -1;
    uint32_t as_ctr = 0;
    // log joint trace and keep-best allocation: one block holds the labels' values between the two
    // launches, the row of the last state scored and the keep-best cell; dLjZ the N labels of the best folded state
    // (0-based); lp_rec: the sweeps that are folded and the rows of four doubles they are recorded in
    bool lp_on = false;
    char* dLjBlock = nullptr;
    double *dLjLik = nullptr, *dLjPrior = nullptr, *dLjOut = nullptr;
    LjBest* dLjBest = nullptr;
    int32_t* dLjZ = nullptr;
    int lp_folded = 0;  // states folded so far
    SweepTrace lp_rec;
    // a ladder's exchange point follows this sweep: the recorders that score rung 0's state (the log joint row, the pair
    // check) are enqueued by the ladder behind the exchange, not by the sweep end.  Set whether or not either is armed.
    bool fold_defer = false;
    // pairwise local-dependence check: the chosen features (host and device), their column
    // slices [M][pc_C], one block with the counts of the last state scored, its values and the fold; pc_rec: the
    // sweeps that are folded (every pc_stride-th from its base) and the rows of 2 npairs doubles they are recorded in
    bool pc_on = false;
    int pc_M = 0, pc_stride = 1;
    int64_t pc_C = 0;
    int32_t* dPcFeat = nullptr;
    uint64_t* dPcXt = nullptr;
    char* dPcBlock = nullptr;
    size_t pc_count_bytes = 0, pc_fold_bytes = 0;
    uint32_t *dPcCnt = nullptr, *dPcMarg = nullptr, *dPcNk = nullptr, *dPcN11 = nullptr;
    double *dPcZ = nullptr, *dPcX2 = nullptr, *dPcSumZ = nullptr, *dPcSumZ2 = nullptr, *dPcSumX2 = nullptr;
    long long* dPcSumDf = nullptr;
    int32_t *dPcDf = nullptr, *dPcNz = nullptr;
    int pc_folded = 0;  // states folded so far
    SweepTrace pc_rec;
    // missing data: na_on: the imputation step behind every sweep end.  One block holds the site
    // list (row, word, mask, first cell), the census [2][K P], the rates [K P] of a counting chain and the cells' two
    // folds; na_rec: the steps that are folded (every one of an armed chain, the kept ones of a run).
    bool na_on = false, na_lds = false;
    int64_t na_cells = 0, na_sites = 0, na_folded = 0;
    int na_grid = 0;
    char* dNaBlock = nullptr;
    int64_t *dNaRow = nullptr, *dNaFirst = nullptr;
    int32_t *dNaWord = nullptr, *dNaCnt = nullptr;
    uint32_t *dNaMask = nullptr, *dNaOnes = nullptr;
    double *dNaPhi = nullptr, *dNaSum = nullptr;
    std::vector<int64_t> na_rows;  // the declared cells, as given
    std::vector<int32_t> na_cols;
    SweepTrace na_rec;
    // constrained allocations: cs_on: k_constrain behind every resample launch whose range holds
    // a listed row.  cs_rows: the listed rows, ascending (the host's binary search per launch); one block holds their
    // device copy, the masks and the two counters.
    bool cs_on = false;
    std::vector<int64_t> cs_rows;
    char* dCsBlock = nullptr;
    int64_t* dCsRows = nullptr;
    uint64_t* dCsMasks = nullptr;
    unsigned long long* dCsStats = nullptr;
    // in_run: the chain belongs to a *_run call (run_prepare) -- its kept sweeps record theta, alpha and pi, and what
    // is "not offered inside a run" is refused -- whether or not the run keeps a label trace (dTrace: keep_trace)
    bool in_run = false;
    // posterior summary: sum_on: a fold behind every stride-th sweep sum_rec names; one block
    // of the device pool (sum) and the workspace of one row's ECR pass; sum_rec: the sweeps that are folded and the
    // rows of (int64 agree, K int32 perm) they are recorded in
    bool sum_on = false, sum_have_pivot = false;
    int sum_pivot_kind = 0, sum_stride = 1, sum_folded = 0;
    int64_t sum_pitch = 0;
    char* dSumBlock = nullptr;
    size_t sum_block_bytes = 0;  // as handed out by the device pool
    SumBufs sum;
    EcrWork* sum_ecr = nullptr;
    SweepTrace sum_rec;
    // parallel tempering: temper_on: the table builds are k_count_tables<TAB_TEMPER> at inverse temperature
    // temper_b, and the kernel choice leaves out the forms that build their own tables and the packed one; ladder: the
    // replica ladder a run drives this chain through as its rung 0 (not owned)
    bool temper_on = false;
    double temper_b = 1.0;
    bmm_ladder* ladder = nullptr;
    int prof = 0;             // > 0: HIP events around the resample launches of every prof-th sweep
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    double prof_ms = 0.0;
    int64_t prof_n = 0;
};

namespace {

// device memory for `bytes` more, refused with a message when it is not there
int pred_room(size_t bytes, const char* what) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b)
        return set_err(BMM_E_ARG, "predictive: %s needs %zu bytes of device memory, %zu are free", what, bytes, free_b);
    return BMM_OK;
}
// One recording into a SweepTrace of a chain.  It owns the device rows (none: the sweeps are folded, not recorded),
// installs the window and, when it ends, puts back what was there and waits for the chain's stream before the rows
// may go: on every return path.  Without rows nothing is waited for.
struct Recording {
    bmm_chain* c = nullptr;
    SweepTrace* slot = nullptr;  // where it is installed ...
    SweepTrace before;           // ... and what was there
    hipError_t status = hipSuccess;  // of the wait in end()
    DevBuf rows;
    int alloc(size_t bytes, const char* what) {  // rows that are refused with a message when the room is not there
        const int rc = pred_room(bytes, what);
        if (rc) return rc;
        HIP_TRY(rows.alloc(bytes));
        return BMM_OK;
    }
    void begin(bmm_chain* chain, SweepTrace& s, size_t row_bytes, int base, int from, bool fold) {
        c = chain; slot = &s; before = s;
        s.p = rows.as<char>(); s.row_bytes = row_bytes; s.base = base; s.from = from; s.fold = fold;
    }
    hipError_t end() {
        if (!slot) return status;
        *std::exchange(slot, nullptr) = before;
        return status = rows.p ? hipStreamSynchronize(c->stream) : hipSuccess;
    }
    int end_run(int rc) {  // ... at the end of a run: its status, or that the wait failed
        const hipError_t es = end();
        return rc == BMM_OK && es != hipSuccess ? set_err(BMM_E_HIP, "the run failed: %s", hipGetErrorString(es)) : rc;
    }
    ~Recording() { (void)end(); }
};

// rows x width doubles on the device (row-major) into the caller's column-major ld x width matrix, from row row0 on
int rows_out(const double* dtrace, int rows, int64_t width, double* out, int ld, int row0) {
    std::vector<double> line((size_t)width);
    for (int s = 0; s < rows; ++s) {
        HIP_TRY(hipMemcpy(line.data(), dtrace + (size_t)s * (size_t)width, (size_t)width * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t m = 0; m < width; ++m) out[(size_t)(row0 + s) + (size_t)m * (size_t)ld] = line[(size_t)m];
    }
    return BMM_OK;
}
// the first sweep a run folds (trace row 0 of a run without burn-in is the start, not a sweep)
int run_first_fold(const bmm_chain* c) { return c->burnin > 0 ? c->burnin : 1; }
// ... and the trace of a run, S kept rows recorded from sweep `burnin` on, into the caller's S x width matrix: the rows
// before the first fold (1 without burn-in) stay NaN
int run_rows_out(const bmm_chain* c, const double* dtrace, int64_t width, double* out) {
    const int S = c->S, first = run_first_fold(c) - c->burnin;
    for (int s = 0; s < first && s < S; ++s)
        for (int64_t m = 0; m < width; ++m) out[(size_t)s + (size_t)m * (size_t)S] = std::nan("");
    return S > first ? rows_out(dtrace + (size_t)first * (size_t)width, S - first, width, out, S, first) : BMM_OK;
}

// What is armed for the next whole-run call of the calling thread (bmm_set_partition_summary, bmm_set_partition_search, bmm_set_credible_ball, bmm_set_loo_summary,
// bmm_set_split_merge, bmm_set_feature_select, bmm_set_init, bmm_set_ecr_relabel, bmm_set_logpost, bmm_set_temper, bmm_set_pair_check, bmm_set_missing, bmm_set_constraints, bmm_set_categorical; bmm_alloc_run fills `alloc` for its own run), and what a
// *_run_predict / *_run_relabel / *_run_probs entry point was handed.
struct RunOptions {
    struct { bool on = false; bmm_partition_out o{}; } partition;
    struct { bool on = false, has_opts = false; bmm_partition_search_opts opts{}; bmm_partition_search_out o{}; } psearch;  // bmm_set_partition_search
    struct { bool on = false; double level = 0.0; bmm_credible_ball_out o{}; } cball;  // bmm_set_credible_ball
    struct { bool on = false; bmm_loo_out o{}; } loo;
    struct { int moves = 0, scans = 0; } sm;
    struct { bool on = false; bmm_feature_out o{}; } fs;
    struct { int kind = 0, iters = 0; } init;
    struct { bool on = false; bmm_ecr_out o{}; } ecr;
    struct { bool on = false; bmm_logpost_out o{}; } logpost;
    struct { bool on = false; bmm_temper_out o{}; } temper;
    struct { bool on = false; bmm_pair_check_out o{}; std::vector<int32_t> feat; } pc;
    struct { bool on = false; const int64_t* rows = nullptr; const int32_t* cols = nullptr; int64_t n = 0; bmm_missing_out o{}; } na;
    struct { bool on = false; const double* log_prior_k = nullptr; int K0 = 0, moves = 0; double eject_a = 1.0; int32_t* k_out = nullptr; int64_t* moves_out = nullptr; } alloc;
    struct { int moves = 0, scans = 0; } as;  // bmm_set_alloc_split_merge: taken by bmm_alloc_run alone
    struct { bool on = false; int64_t n = 0; const int64_t* rows = nullptr; const uint64_t* masks = nullptr; } cs;  // bmm_set_constraints
    struct { bool on = false; bmm_summary_opts opts{}; bmm_summary_out o{}; } summary;  // bmm_set_summary
    struct { bool on = false; std::vector<int32_t> levels; } cat;  // bmm_set_categorical (a copy: the caller's vector may go)
    bool keep_trace() const { return !summary.on || summary.opts.keep_trace != 0; }
    const bmm_relabel_hooks* hooks = nullptr;  // *_run_probs
    const bmm_relabel_out* rel = nullptr;      // *_run_relabel
    const int32_t* Xnew = nullptr; int64_t M = 0; const bmm_predict_out* pred = nullptr;  // *_run_predict
    struct { bool on = false; const int64_t* rows = nullptr; const int32_t* cols = nullptr; int64_t n = 0; double* mean = nullptr; } pna;  // bmm_set_newdata_missing
    bool predict() const { return pred && M > 0; }
};
thread_local RunOptions g_armed;
// First statement of every public *_run* entry point, bmm_multi_run included: the armed state moves into the call,
// so whatever the call returns, and wherever it returns from, nothing is armed afterwards.
RunOptions take_run_options() { return std::exchange(g_armed, RunOptions{}); }
// ... and what the bmm_last_* getters read of the thread's last run
thread_local int64_t g_sm_stats[5] = {0, 0, 0, 0, 0};
thread_local int64_t g_as_stats[5] = {0, 0, 0, 0, 0};
thread_local bmm_init_info g_init_info{};

int planes_alloc(bmm_chain* c, size_t words) {
    size_t got = 0;
    uint32_t* d = static_cast<uint32_t*>(dev_pool().get(c->device, words * sizeof(uint32_t), &got));
    if (!d) return set_err(BMM_E_HIP, "allocating the bit planes failed: %s", hipGetErrorString(hipGetLastError()));
    c->planes = new (std::nothrow) bmm_chain::Planes();
    if (!c->planes) { dev_pool().put(c->device, d, got); return set_err(BMM_E_ARG, "out of host memory"); }
    c->planes->d = d;
    c->planes->bytes = got;
    c->dXb = d;
    return BMM_OK;
}

// every cell of X must be 0 or 1: one streaming pass when the matrix is handed over
int validate_binary(bmm_chain* c, const int32_t* dX, int64_t n) {
    DevBuf flagbuf;
    HIP_TRY(flagbuf.alloc(sizeof(int)));
    int* const dflag = flagbuf.as<int>();
    HIP_TRY(hipMemsetAsync(dflag, 0, sizeof(int), c->stream));
    const bool al16 = (reinterpret_cast<uintptr_t>(dX) & 15) == 0;
    const int64_t n16 = al16 ? n / 4 : 0;
    hipLaunchKernelGGL(k_validate_binary, dim3(2048), dim3(256), 0, c->stream,
                       reinterpret_cast<const uint4*>(dX), n16, reinterpret_cast<const uint32_t*>(dX), n, dflag);
    int flag = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(BMM_E_HIP, "validating X failed: %s", hipGetErrorString(e));
    if (flag) return set_err(BMM_E_ARG, "data must be binary: X holds a value other than 0 and 1");
    return BMM_OK;
}

// Default batch -- a pure function of (sampler, N): no device, occupancy or layout enters, so a defaulted batch
// names the same chain everywhere.  Below 2^16 observations: floor(N/8) for the finite sampler, floor(N/16) for the
// DP sampler (above that every "new" draw of a batch shares one label and spurious clusters open on small data).
// From 2^16 observations on: floor(N/4) for both.  The bias of a batch against the sequential scan shrinks
// with N -- the net flow into a cluster during a batch is O(sqrt N), its size O(N) -- and at those sizes it is not
// measurable: the committed batch-1 fixtures (tests/golden/tolerance_*.json; K = 20 at N = 2^16, 1e5, 2^18, 2^19, 1e6, 2e6
// and 1e7, K = 3 at 1e5, seven DP shapes from N = 2^16) are met to 2e-5 in the proportions and 1e-3 in theta-hat at N/4 as at
// N/8, and the DP's shares per generating component and cluster counts at N/4 as at N/16 (tests/test_gpu_tolerance_fixtures.py runs at
// whatever this function returns; profiles/r03/README.md has the numbers, including that a random start ends in the
// generating mode as often at N/4 as at N/8).  What a larger batch buys is launches: a batch costs about 20 us of
// fixed time whatever its size (k_count_tables + the resample launch's own set-up and flush).
// Never rounded: work is handed out per wave in chunks of 64 observations, so a launch that is not a whole number
// of rounds of the chip costs a fraction of a chunk per wave.
constexpr int64_t kLargeN = (int64_t)1 << 16;
int64_t default_batch(int sampler, int64_t N) {
    if (sampler == BMM_SAMPLER_SB || sampler == BMM_SAMPLER_FULL) return N;
    const int64_t div = N >= kLargeN ? 4 : (sampler == BMM_SAMPLER_DP ? 16 : 8);
    const int64_t b = N / div;
    return b < 1 ? 1 : b;
}

TableLayout layout_of(const bmm_chain* c) { return layout_of(c->p, !explicit_params(c->p.mode)); }

// The test variant's switches (-DBMM_DEBUG_HOOKS: environment variables, read through dbg_env, so the product
// library has none of them set).  These steer the shape and the kernel choice and are read when one of these is
// made, once per choice; the others are read where they act: BMM_DEBUG_STREAM (chain_stream_create),
// BMM_DEBUG_FAKE_DEVICES (fake_devices), BMM_DEBUG_BADLABEL, BMM_DEBUG_STRAGGLER, BMM_DEBUG_DRAW_FALLBACK,
// BMM_DEBUG_DRAW_NOEPS and BMM_DEBUG_PK_GENKEY (k_resample_pk draws under the general, per-lane form of the Philox
// key whatever the launch) (launch_resample).
int dbg_env_int(const char* name, int unset) { const char* v = dbg_env(name); return v ? (atoi(v) > 0 ? atoi(v) : 0) : unset; }
struct DebugSwitches {
    bool generic = dbg_env("BMM_DEBUG_GENERIC");        // every shape on the generic path
    bool int32_layout = dbg_env("BMM_X_LAYOUT_INT32");  // chains start on the int32 layout (the *_run calls have no layout argument)
    // n >= 1: the kernel choice sees n compute units -- the grid limits, the short-launch and step-down rules -- so that
    // test-sized batches reach the default-sized kernels and give a wave several chunks (tests/test_gpu_chunks.py)
    int cus = dbg_env_int("BMM_DEBUG_CUS", 0);
    int threads = dbg_env_int("BMM_DEBUG_THREADS", -1); // the one-lane kernel at that many threads where it exists (-1: unset)
    bool split = dbg_env("BMM_DEBUG_SPLIT");            // every launch counts as short (two lanes from 16 accumulators)
    bool nosplit = dbg_env("BMM_DEBUG_NOSPLIT");        // never two lanes per observation
    bool small = dbg_env("BMM_DEBUG_SMALL");            // the 256-thread form whatever the size of the tables
    bool noself = dbg_env("BMM_DEBUG_NOSELF");          // no table-building workgroups
    bool nopk = dbg_env("BMM_DEBUG_NOPK");              // k_resample where k_resample_pk would run (A/B in one library)
    bool pk = dbg_env("BMM_DEBUG_PK");                  // k_resample_pk whatever the length of a launch
    bool nopipe = dbg_env("BMM_DEBUG_PK_NOPIPE");       // k_resample_pk's present body where the second one would run
    // n >= 1: k_resample_pk treats a lane whose observation index is a multiple of n as uncertain, so that certain and
    // settled lanes share a wave (tests/test_gpu_pk_inline.py).  BMM_DEBUG_PK_QUEUE is still accepted and does nothing:
    // the queue it sized is gone
    int pk_defer_every = dbg_env_int("BMM_DEBUG_PK_DEFER_EVERY", 0);
    // n >= 1: k_resample_pk's middle settle tier reports "uncertain" for observation indices that are multiples of n, so
    // that lanes settled by it and by the definition share a wave (tests/test_gpu_pk_mid.py).  BMM_DEBUG_PK_NOMID
    // (launch_resample) skips the middle tier: the definition settles every uncertain lane, as before there was one
    int pk_mid_fail_every = dbg_env_int("BMM_DEBUG_PK_MID_FAIL_EVERY", 0);
};

// What follows from (sampler, N, P, K, batch) alone -- no device state enters.
struct ChainShape {
    ChainParams p{};            // mode, N, P, K and the geometry: W, G, Gm, Kc, KT (priors and seed are the caller's)
    int64_t batch = 1;
    bool generic = false;       // shape beyond the resident kernel
    int minus_in_lds = 1;
    size_t lds_bytes_base = 0;  // resident: what a workgroup keeps in LDS (table image + histogram)
};
ChainParams geometry(int sampler, int P, int K, int kt, int W) {
    ChainParams q{};
    q.mode = sampler; q.P = P; q.K = K; q.KT = kt; q.W = W;
    q.G = (P + W - 1) / W; q.Gm = (P + kGroupWm - 1) / kGroupWm;
    q.Kc = sampler == BMM_SAMPLER_DP ? K + 1 : K;
    return q;
}
// LDS of a resident workgroup: the table image (with the own-cluster tables, or its head only), the histogram
// and the chunk counter
size_t image_bytes(const ChainParams& q, bool own_tables) {
    const TableLayout l = layout_of(q, own_tables && !explicit_params(q.mode));
    return (size_t)(own_tables ? l.doubles() : l.head()) * sizeof(double) + ((size_t)q.K * q.P + q.K + 4) * sizeof(int32_t);
}

// LDS of a k_resample_pk workgroup: the packed image, the binary32 own-cluster image of as many bytes, Nk and E of
// the table image, the histogram with its counters, and kPkQueue words the kernel no longer uses (they were its queue
// of uncertain observations; tests/test_own32_cpu.py restates this sum, so the reservation stays until that test is
// revised: DESIGN.md section 5)
size_t pk_image_bytes(const ChainParams& q) {
    const TableLayout l = layout_of(q, true);
    return (size_t)(2 * pk_tq_doubles(l) + l.tm() - l.nk()) * sizeof(double) + ((size_t)q.K * q.P + q.K + 4 + kPkQueue) * sizeof(int32_t);
}

// The spec's rule for the group width of a shape (bmm_spec.h; the oracle restates it): groups of kGroupW
// features when the whole table image of the shape and the histogram fit in LDS that way, kGroupWAlt
// otherwise.  A pure function of (sampler, K, P).
int group_width_rule(int sampler, int K, int P) {
    const int kt = pick_kt(sampler == BMM_SAMPLER_DP ? K + 1 : K);
    if (kt < 0 || P > kMaxP) return kGroupWAlt;
    return image_bytes(geometry(sampler, P, K, kt, kGroupW), true) <= kLdsMax ? kGroupW : kGroupWAlt;
}

// threads of the generic path (k_resample_generic, k_score_generic): a scratch column of Kc scores each
int64_t generic_threads(int Kc) {
    int64_t threads = (int64_t)256 * 1024;
    const int64_t cap = ((int64_t)256 << 20) / ((int64_t)Kc * 8);  // <= 256 MiB of scratch
    if (threads > cap) threads = cap / 256 * 256;
    return threads < 256 ? 256 : threads;
}

ChainShape chain_shape(int sampler, int64_t N, int P, int K, int64_t batch, const DebugSwitches& d) {
    ChainShape s;
    const int kt = pick_kt(sampler == BMM_SAMPLER_DP ? K + 1 : K);
    ChainParams& p = s.p;
    p = geometry(sampler, P, K, kt, group_width_rule(sampler, K, P));
    p.N = N; p.Ntot = N; p.obs0 = 0;
    s.batch = batch <= 0 ? default_batch(sampler, N) : (batch > N ? N : batch);
    if (explicit_params(sampler)) s.batch = N;
    s.generic = p.KT < 0 || P > kMaxP || d.generic;
    if (!s.generic) {
        s.lds_bytes_base = image_bytes(p, true);
        if (s.lds_bytes_base > kLdsMax && !explicit_params(sampler)) {  // second tier: own-cluster tables stay in L2
            s.minus_in_lds = 0;
            s.lds_bytes_base = image_bytes(p, false);
        }
        if (s.lds_bytes_base > kLdsMax) s.generic = true;  // third tier: nothing resident
    }
    if (s.generic) {
        // any shape: tables gathered from global memory, scores in a scratch column per thread
        p.KT = (p.Kc + 3) / 4 * 4;
        s.minus_in_lds = 0;
        s.lds_bytes_base = 0;
    }
    return s;
}

int32_t* label_row(bmm_chain* c, int j) {
    if (c->dTrace && j >= c->burnin) return c->dTrace + (size_t)(j - c->burnin) * c->p.N;
    return c->dZ[j & 1];
}

// A chain's stream.  The runtime pools at most four hardware queues per priority level and lets later
// streams share them -- with whatever the host framework created before -- and two chains on one queue
// serialise: four chains of the north-star shape on one GPU ran at 10.5 k sweeps/s in all on plain
// streams in a fresh process and at 5.5 k (no overlap at all) at the end of bench.py's sequence of
// workloads; streams on the high-priority level, and GPU_MAX_HW_QUEUES=8, fixed the first case and not
// the second (profiles/r02/README.md).  A stream created with a CU mask -- here the full one -- gets a
// hardware queue of its own from the runtime, whatever came before: 14.9-15.7 k in both cases.  It costs
// about 6 ms more per chain created, and beyond four chains per device the queues start to thrash (8
// chains: 9.9 k against 12.5 k on shared queues).  mode 0: plain stream; 1: high priority; 2: CU mask.
// compute units of a device, asked once per process (hipGetDeviceProperties costs a good part of a
// millisecond, and a drop-in call creates a chain every time)
int device_cus(int device) {
    static std::mutex m;
    static int cus[64];
    if (device < 0 || device >= 64) return 0;
    std::lock_guard<std::mutex> g(m);
    if (cus[device] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); return 0; }
        cus[device] = prop.multiProcessorCount;
    }
    return cus[device];
}

// Streams outlive their chain: creating and destroying a plain one costs about 2 ms each on this runtime
// (tools/hipcost_probe.hip), a fifth of what the rest of a 220-sweep drop-in call at the north-star shape
// spends outside its sweeps; one with a hardware queue of its own (chains sharing a device) costs 6 ms, and a
// process that created and destroyed four of those per call was seen to hang inside the runtime's queue
// creation after some hundred calls (a runtime thread stuck in the driver's queue ioctl, the caller waiting for
// its lock: profiles/r03/README.md).  A destroyed chain's (idle) stream goes back here, up to four of either
// kind per device.
struct StreamPool {
    std::mutex m;
    std::vector<hipStream_t> idle[2][64];  // [0] plain, [1] with a hardware queue of their own
    hipStream_t get(int device, bool dedicated) {
        if (device < 0 || device >= 64) return nullptr;
        std::lock_guard<std::mutex> g(m);
        std::vector<hipStream_t>& v = idle[dedicated ? 1 : 0][device];
        if (v.empty()) return nullptr;
        hipStream_t s = v.back();
        v.pop_back();
        return s;
    }
    bool put(int device, hipStream_t s, bool dedicated) noexcept {
        if (device < 0 || device >= 64) return false;
        try {
            std::lock_guard<std::mutex> g(m);
            std::vector<hipStream_t>& v = idle[dedicated ? 1 : 0][device];
            if (v.size() >= 4) return false;
            v.push_back(s);
            return true;
        } catch (...) {
            return false;
        }
    }
};
StreamPool& stream_pool() { static StreamPool* const pool = new StreamPool(); return *pool; }  // never destroyed: no HIP call at exit

int chain_stream_create(bmm_chain* c, bool dedicated) {
    int mode = dedicated ? BMM_STREAM_MODE : 0;
    if (const char* m = dbg_env("BMM_DEBUG_STREAM")) mode = atoi(m);
    hipError_t e = hipErrorUnknown;
    hipStream_t st = nullptr;
    if (mode == 1) {
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest);
    } else if (mode == 2) {
        st = stream_pool().get(c->device, true);
        if (st) {
            e = hipSuccess;
        } else {
            uint32_t mask[16];
            for (uint32_t& w : mask) w = 0xffffffffu;
            const int cus = device_cus(c->device);
            e = cus > 0 ? hipExtStreamCreateWithCUMask(&st, (uint32_t)((cus + 31) / 32), mask) : hipErrorUnknown;
        }
    }
    int kind = mode == 2 ? 2 : 0;  // 0: not pooled, 1: a plain stream of the pool's kind, 2: one with its own queue
    if (e != hipSuccess) {  // mode 0, or the special stream could not be had
        (void)hipGetLastError();
        st = stream_pool().get(c->device, false);
        if (!st) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        kind = 1;
    }
    c->stream = st;
    c->dedicated_queue = dedicated;
    c->stream_kind = kind;
    return BMM_OK;
}
// an idle stream goes back to the pool of its kind, anything else (and what the pool has no room for) is destroyed
void chain_stream_release(int device, hipStream_t st, int kind) {
    if (!st) return;
    if (kind != 0 && stream_pool().put(device, st, kind == 2)) return;
    (void)hipStreamDestroy(st);
}

// A chain that starts sharing its device with another one moves to a stream with a hardware queue of its
// own (a lone chain keeps a plain stream: the dedicated queue costs about 6 ms to create).  Only before
// the first sweep: nothing but the finished data hand-over has run on the old stream.
int chain_dedicated_queue(bmm_chain* c) {
    if (c->dedicated_queue || c->started) return BMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t old = c->stream;
    const int old_kind = c->stream_kind;
    if (old) HIP_TRY(hipStreamSynchronize(old));
    int rc = chain_stream_create(c, true);
    if (rc) { c->stream = old; c->stream_kind = old_kind; return rc; }
    chain_stream_release(c->device, old, old_kind);
    return BMM_OK;
}

// bump allocation out of one device buffer, 256-byte aligned pieces
struct Carver {
    char* base;
    size_t used = 0;
    template <class T> T* take(size_t n) {
        const size_t off = (used + 255) & ~(size_t)255;
        used = off + n * sizeof(T);
        return base ? reinterpret_cast<T*>(base + off) : nullptr;
    }
};

int chain_alloc(bmm_chain* c) {
    const ChainParams& p = c->p;
    HIP_TRY(hipSetDevice(c->device));
    // (chains that come to share a device are moved to streams with hardware queues of their own:
    // chain_dedicated_queue)
    {
        int rcs = chain_stream_create(c, false);
        if (rcs) return rcs;
    }
    const size_t nz = (size_t)p.N;
    const size_t ns = (size_t)p.K * p.P, nn = (size_t)p.K;
    // (behind the image of a counting sampler: the two binary32 images k_resample_pk reads, Tq and Tm32)
    const size_t ntab = (size_t)layout_of(c).doubles() + (explicit_params(p.mode) ? 0 : 2 * (size_t)pk_tq_doubles(layout_of(c)));
    auto carve = [&](Carver& a) {
        // the statistics, their delta replicas, the table image and the flags first: zeroed in one go
        c->dNk = a.take<int32_t>(nn);
        c->dDNk = a.take<int32_t>(nn * kDeltaReps);
        c->dS = a.take<int32_t>(ns);
        c->dDS = a.take<int32_t>(ns * kDeltaReps);
        c->dTab = a.take<double>(ntab);
#ifdef BMM_DIAG
        c->dDiag = a.take<unsigned long long>(22);
#endif
        c->dSelfDone = a.take<int>(1);
        c->dViable = a.take<int>(1);
        c->dDNkAlt = a.take<int32_t>(nn * kDeltaReps);
        c->dDSAlt = a.take<int32_t>(ns * kDeltaReps);
#ifdef BMM_DEBUG_HOOKS
        c->dDbgFlag = a.take<int>(1);
        c->dPkStat = a.take<unsigned long long>(6);
#endif
        const size_t zeroed = a.used;
        c->dAlpha = a.take<double>(1);
        c->dPi = a.take<double>(nn);
        c->dTheta = a.take<double>(ns);
        c->dZ[0] = a.take<int32_t>(nz);
        c->dZ[1] = a.take<int32_t>(nz);
        return zeroed;
    };
    Carver measure{nullptr};
    carve(measure);
    c->arena = static_cast<char*>(dev_pool().get(c->device, measure.used, &c->arena_bytes));
    if (!c->arena) return set_err(BMM_E_HIP, "allocating the chain's state failed: %s", hipGetErrorString(hipGetLastError()));
    Carver real{c->arena};
    const size_t zeroed = carve(real);
    if (c->generic) HIP_TRY(hipMalloc(&c->dScratch, (size_t)c->scratch_stride * p.Kc * sizeof(double)));
    HIP_TRY(hipMemsetAsync(c->arena, 0, zeroed, c->stream));
    HIP_TRY(hipMemsetAsync(c->dZ[0], 0xff, nz * sizeof(int32_t), c->stream));  // -1 = unassigned
    HIP_TRY(hipMemcpyAsync(c->dAlpha, &c->alpha0, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMM_OK;
}

// test variant only: after a synchronisation, has a kernel met a label outside its range?
int dbg_labels_ok(bmm_chain* c) {
#ifdef BMM_DEBUG_HOOKS
    int flag = 0;
    HIP_TRY(hipMemcpy(&flag, c->dDbgFlag, sizeof(int), hipMemcpyDeviceToHost));
    if (flag) return set_err(BMM_E_STATE, "a resample kernel produced or read a label outside [0, K): kernel bug (debug-hooks build check)");
#else
    (void)c;
#endif
    return BMM_OK;
}

int launch_resample(bmm_chain* c, const int32_t* z_in, int32_t* z_out, int64_t lo, int64_t hi,
                    uint32_t sweep) {
    ResampleArgs a{};
    a.X = c->dX; a.Xb = c->dXb; a.z_in = z_in; a.z_out = z_out; a.tab = c->dTab; a.dNk = c->dDNk; a.dS = c->dDS;
    a.lo = lo; a.hi = hi; a.sweep = sweep; a.minus_in_lds = c->minus_in_lds; a.diag = c->dDiag;
    a.dbg_flag = c->dDbgFlag; a.dbg_inject = (dbg_env("BMM_DEBUG_BADLABEL") ? 1 : 0) | (dbg_env("BMM_DEBUG_STRAGGLER") ? 2 : 0) |
                                             (dbg_env("BMM_DEBUG_DRAW_FALLBACK") ? 4 : 0) | (dbg_env("BMM_DEBUG_DRAW_NOEPS") ? 8 : 0) |
                                             (dbg_env("BMM_DEBUG_PK_GENKEY") ? 16 : 0) | (dbg_env("BMM_DEBUG_PK_NOMID") ? 32 : 0);
    a.Nk = c->dNk; a.S = c->dS; a.alpha_ptr = c->dAlpha; a.self_done = c->dSelfDone;
#ifdef BMM_DEBUG_HOOKS
    a.pk_stat = c->dPkStat;
    a.pk_defer_every = c->pk_defer_every;
    a.pk_mid_fail_every = c->pk_mid_fail_every;
#endif
    const bool emit = c->probs_dst != nullptr;
    const bool use_generic = c->generic || (emit && !c->fn_emit);  // the int32 layout has no emitting twin
    // a kernel that builds its own tables reads the pending deltas and flushes into the other (empty) set, which
    // is the pending one from then on (self_fold_prev, kernels.hip.h)
    const bool self_launch = c->form.self && !emit && !use_generic;
    if (self_launch) { a.dNk_prev = c->dDNk; a.dS_prev = c->dDS; a.dNk = c->dDNkAlt; a.dS = c->dDSAlt; }
    const KernelForm& form = emit ? c->form_emit : c->form;
    const int gmax = emit ? c->grid_max_emit : c->grid_max;
    const int64_t ntiles = use_generic ? 1 : (hi - lo + tile_of(form) - 1) / tile_of(form);
    int grid = (int)(ntiles < gmax ? ntiles : gmax);
    if (use_generic) {
        const int64_t nt256 = (hi - lo + 255) / 256;
        const int64_t maxb = c->scratch_stride / 256;
        grid = (int)(nt256 < maxb ? nt256 : maxb);
    }
    if (emit) { a.wts = c->dWts; a.wtot = c->dWtot; }
    // k_resample_pk addresses an observation by a 32-bit offset from the launch's first (plan_kernel offers it for
    // launches of fewer than 2^31 observations): that first observation is folded into the bases here.  lo and hi stay
    // what they are -- the draw's counter and the test variant's counters are in observation indices.
    if (form.pk && !use_generic) {
        a.Xb += lo;
        if (a.z_in) a.z_in += lo;
        a.z_out += lo;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->prof > 0 && sweep % (uint32_t)c->prof == 0) {
        if (c->ev_used + 2 > c->ev.size()) {
            hipEvent_t a0, a1;
            HIP_TRY(hipEventCreate(&a0));
            HIP_TRY(hipEventCreate(&a1));
            c->ev.push_back(a0); c->ev.push_back(a1);
        }
        e0 = c->ev[c->ev_used]; e1 = c->ev[c->ev_used + 1];
        c->ev_used += 2;
    }
    // a profiled launch carries its own start / stop events (hipExtLaunchKernel): they take the kernel's
    // begin and end timestamps, as rocprofv3's kernel trace does -- a pair of hipEventRecord around the launch
    // would also span the dispatch of the kernel and of the second marker (4-8 us per launch here)
    if (use_generic) {
        if (e0) hipExtLaunchKernelGGL(k_resample_generic, dim3(grid), dim3(256), 0, c->stream, e0, e1, 0, c->p, a,
                                      c->dScratch, c->scratch_stride);
        else hipLaunchKernelGGL(k_resample_generic, dim3(grid), dim3(256), 0, c->stream, c->p, a, c->dScratch,
                                c->scratch_stride);
    } else {
        const resample_fn fn = emit ? c->fn_emit : c->fn;
        const int nt = form.nt;
        const size_t lds = emit ? c->lds_bytes_base : c->lds_bytes;  // the SELF kernels carry scratch behind the image
        if (e0) hipExtLaunchKernelGGL(fn, dim3(grid), dim3(nt), (uint32_t)lds, c->stream, e0, e1, 0, c->p, a);
        else hipLaunchKernelGGL(fn, dim3(grid), dim3(nt), lds, c->stream, c->p, a);
    }
    HIP_TRY(hipGetLastError());
    if (self_launch) { std::swap(c->dDNk, c->dDNkAlt); std::swap(c->dDS, c->dDSAlt); }
    if (emit) {  // before the next k_count_tables rewrites the image's cluster sizes
        const int64_t nb = (hi - lo + 255) / 256;
        hipLaunchKernelGGL(k_probs_finish, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->p,
                           c->dTab, c->dWts, c->dWtot, z_in, lo, hi, c->probs_dst);
        HIP_TRY(hipGetLastError());
    }
    return BMM_OK;
}

// ---- categorical features ----
// what everything that scores a Bernoulli cell by itself answers a chain with levels set
int cat_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s knows the Bernoulli cell only: not offered on a chain with categorical features "
                   "(bmm_chain_set_categorical)", what);
}
// The column map of a levels vector over P columns: feature f of levels[f] = 1 is a Bernoulli column, of L >= 2 a block
// of L neighbouring one-hot columns.  lev (or null): the P bytes k_count_tables<TAB_CAT> reads; blocks (or null): the
// list k_cat_check walks; first_column (or null): F entries.  No device is touched.
int cat_map(const int32_t* levels, int F, int P, std::vector<uint8_t>* lev, std::vector<CatBlock>* blocks, int32_t* first_column) {
    if (!levels || F < 1) return set_err(BMM_E_ARG, "categorical: null or empty levels");
    if (F >= (1 << kCatKeyBits)) return set_err(BMM_E_ARG, "categorical: at most %d features", (1 << kCatKeyBits) - 1);
    int64_t cols = 0;
    for (int f = 0; f < F; ++f) {
        if (levels[f] < 1)
            return set_err(BMM_E_ARG, "categorical: feature %d has %d levels: a feature has at least 1 (1 is a binary feature in one column)", f, levels[f]);
        if (levels[f] > 255) return set_err(BMM_E_ARG, "categorical: feature %d has %d levels: at most 255 are offered", f, levels[f]);
        cols += levels[f];
    }
    if (cols != P) return set_err(BMM_E_ARG, "categorical: the levels take %lld columns, the chain has P = %d", (long long)cols, P);
    if (lev) lev->assign((size_t)P, 0);
    if (blocks) blocks->clear();
    int col = 0;
    for (int f = 0; f < F; ++f) {
        const int L = levels[f];
        if (first_column) first_column[f] = col;
        if (L >= 2) {
            if (lev) std::fill(lev->begin() + col, lev->begin() + col + L, (uint8_t)L);
            if (blocks) blocks->push_back(CatBlock{col, L, f});
        }
        col += L;
    }
    return BMM_OK;
}
// k_cat_check over the resident planes, once per pairing of levels and data: every row has exactly one bit in every block
int cat_check(bmm_chain* c) {
    if (!c->cat_on || !c->have_data || c->cat_checked) return BMM_OK;
    if (!c->bits || !c->dXb) return set_err(BMM_E_UNSUPPORTED, "categorical features read the bit planes: not offered on the int32 layout");
    if (!c->cat_blocks.empty()) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemsetAsync(c->dCatBad, 0xff, sizeof(unsigned long long), c->stream));
        const int64_t nb = (c->p.N + 255) / 256;
        hipLaunchKernelGGL(k_cat_check, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, (const uint32_t*)c->dXb,
                           c->p.N, (const CatBlock*)c->dCatBlocks, (int)c->cat_blocks.size(), c->dCatBad);
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, c->dCatBad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad != ~0ull) {
            const int f = (int)(bad & ((1ull << kCatKeyBits) - 1));
            int col = 0;
            for (int g = 0; g < f; ++g) col += c->cat_levels[(size_t)g];
            return set_err(BMM_E_ARG, "categorical: row %lld does not have exactly one level of feature %d (columns %d..%d): "
                           "a block of one-hot columns holds a single 1 per row", (long long)(bad >> kCatKeyBits), f, col,
                           col + c->cat_levels[(size_t)f] - 1);
        }
    }
    c->cat_checked = true;
    return BMM_OK;
}
// ... behind every hand-over of data to a chain whose levels are set: data that fail are not the chain's data
int cat_data_changed(bmm_chain* c) {
    if (!c->cat_on) return BMM_OK;
    c->cat_checked = false;
    const int rc = cat_check(c);
    if (rc) c->have_data = false;
    return rc;
}

// ---- constrained allocations ----
// what the options that move rows by themselves, or hand the rows' probabilities on, answer an armed chain
int cs_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s is not offered on a chain with constrained rows (bmm_chain_set_constraints): it knows "
                   "nothing of the rows' allowed labels", what);
}
// k_constrain over the listed rows of [lo, hi), stream-ordered behind the launch that wrote z_out there, adding to the
// pending delta set (the one launch_resample left in dDNk / dDS, whichever form it launched).  A range without a listed
// row launches nothing.  project: the rows' labels put inside their sets instead (the starting labels' rule); counted:
// whether something has counted the labels already, so that the deltas must follow.
int launch_constrain(bmm_chain* c, const int32_t* z_in, int32_t* z_out, int64_t lo, int64_t hi, bool project = false,
                     bool counted = true) {
    const auto first = std::lower_bound(c->cs_rows.begin(), c->cs_rows.end(), lo);
    const auto last = std::lower_bound(first, c->cs_rows.end(), hi);
    if (first == last) return BMM_OK;
    const int64_t q0 = first - c->cs_rows.begin();
    ConstrainArgs a{};
    a.rows = c->dCsRows + q0; a.masks = c->dCsMasks + q0; a.n = last - first;
    a.z_in = z_in; a.z_out = z_out; a.X = c->dX; a.Xb = c->dXb;
    if (counted) { a.dNk = c->dDNk; a.dS = c->dDS; }
    a.stats = project ? nullptr : c->dCsStats;
    a.project = project ? 1 : 0;
    const int64_t nb = (a.n + 255) / 256;
    const dim3 grid((unsigned)(nb < 1024 ? nb : 1024));
    if (c->generic || !c->bits) {
        hipLaunchKernelGGL(k_constrain_generic, grid, dim3(256), 0, c->stream, c->p, a);
    } else {
        const size_t hb = counted ? ((size_t)c->p.K * c->p.P + c->p.K) * sizeof(int32_t) : 0;
        hipLaunchKernelGGL(k_constrain, grid, dim3(256), hb, c->stream, c->p, a);
    }
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

// buffers and kernel of the probability hand-off, set up on first use
int probs_alloc(bmm_chain* c, bool with_matrix) {
    const size_t n = (size_t)c->p.N;
    if (c->bits && !c->generic && !c->fn_emit) {
        const resample_fn fn = lookup(c->form_emit);
        int pe = 0;
        const hipError_t e = kernel_fits(fn, c->form_emit.nt, c->lds_bytes_base, &pe);
        if (e != hipSuccess) return set_err(BMM_E_HIP, "kernel set-up failed: %s", hipGetErrorString(e));
        c->fn_emit = fn;
        c->grid_max_emit = (pe < 1 ? 1 : pe) * c->num_cus;
    }
    if (!c->dWts) HIP_TRY(hipMalloc(&c->dWts, n * c->p.Kc * sizeof(double)));
    if (!c->dWtot) HIP_TRY(hipMalloc(&c->dWtot, n * sizeof(double)));
    if (with_matrix && !c->dProbs) HIP_TRY(hipMalloc(&c->dProbs, n * c->p.K * sizeof(double)));
    if (!c->fn_emit && !c->dScratch) {  // int32 layout: the hand-off sweeps run on the generic kernel
        c->scratch_stride = generic_threads(c->p.Kc);
        HIP_TRY(hipMalloc(&c->dScratch, (size_t)c->scratch_stride * c->p.Kc * sizeof(double)));
    }
    return BMM_OK;
}

// replicas 1.. of the delta accumulators folded into replica 0: what the host-side accessors and the
// sharded chain's all-reduce read
int launch_reduce_deltas(bmm_chain* c) {
    const int n = c->p.K * c->p.P + c->p.K;
    hipLaunchKernelGGL(k_reduce_deltas, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->p, c->dDNk, c->dDS);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

int launch_count_tables(bmm_chain* c) {
    auto launch = [c](auto kernel, const uint32_t* mask, int packed, auto... extra) {
        hipLaunchKernelGGL(kernel, dim3(c->p.KT), dim3(kCountTablesThreads), 0, c->stream, c->p, c->dNk, c->dS, c->dDNk, c->dDS,
                           (const double*)c->dAlpha, c->dTab, mask, packed, extra...);
    };
    if (c->alloc_on)  // the allocation sampler: open empty labels keep their prior weight
        launch(k_count_tables<TAB_ALLOC, const int32_t*, double>, nullptr, 0, (const int32_t*)c->dEaK, c->alloc_a);
    else if (c->temper_on)  // a tempered chain: every per-feature term times its inverse temperature
        launch(k_count_tables<TAB_TEMPER, double>, nullptr, 0, c->temper_b);
    else if (c->fs_mask)  // feature selection: excluded features are written as zeros
        launch(k_count_tables<TAB_MASK>, (const uint32_t*)c->dFsMask, 0);
    else if (c->cat_on)  // categorical features: a block's denominator rides on its x = 1 terms
        launch(k_count_tables<TAB_CAT, const uint8_t*>, nullptr, c->form.pk && !c->generic ? 1 : 0, (const uint8_t*)c->dCatLev);
    else
        launch(k_count_tables<TAB_PLAIN>, nullptr, c->form.pk && !c->generic ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

// ---- posterior predictive of new rows ----
// Score the chain's new rows against its current state, stream-ordered behind whatever produced that state:
// logdens / resp receive this state's values (device, may be null); fold adds it to the accumulators.
// The two launches behind both: the table image of a counting chain's state (explicit samplers: the chain's own image,
// group tables of (pi, theta) with log pi in group 0), then the scorer over a.rows rows
int launch_score(bmm_chain* c, ScoreArgs a, bool loo) {
    const ChainParams& p = c->p;
    a.tab = c->dTab;
    if (!explicit_params(p.mode)) {
        double* const tab = loo ? c->dLooTab : c->dPredTab;
        if (loo) hipLaunchKernelGGL(k_state_tables<true>, dim3(p.KT), dim3(512), 0, c->stream, p, c->dNk, c->dS, c->dDNk, c->dDS, c->dAlpha, tab);
        else hipLaunchKernelGGL(k_state_tables<false>, dim3(p.KT), dim3(256), 0, c->stream, p, c->dNk, c->dS, c->dDNk, c->dDS, c->dAlpha, tab);
        HIP_TRY(hipGetLastError());
        a.tab = tab;
    }
    if (c->generic || (loo && c->loo_generic)) {
        double* const scr = c->generic ? c->dScratch : c->dLooScratch;
        const int64_t stride = c->generic ? c->scratch_stride : c->loo_scratch_stride;
        const int64_t nb = (a.rows + 255) / 256, maxb = stride / 256;
        const dim3 grid((unsigned)(nb < maxb ? nb : maxb));
        if (loo) hipLaunchKernelGGL(k_score_generic<true>, grid, dim3(256), 0, c->stream, p, a, scr, stride);
        else hipLaunchKernelGGL(k_score_generic<false>, grid, dim3(256), 0, c->stream, p, a, scr, stride);
    } else {
        const int64_t ntiles = (a.rows + kScoreThreads - 1) / kScoreThreads;
        const int grid_max = loo ? c->loo_grid_max : c->pred_grid_max;
        hipLaunchKernelGGL(loo ? c->lfn : c->pfn, dim3((int)(ntiles < grid_max ? ntiles : grid_max)), dim3(kScoreThreads),
                           loo ? c->loo_lds : c->pred_lds, c->stream, p, a);
    }
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// ... of incomplete new rows: the split image of the current state, then the masked scorer in
// the shape's form; cell (device, may be null) receives this state's P(x_d = 1 | x_O, state) per missing cell
int launch_score_na(bmm_chain* c, double* logdens, double* resp, double* cell, bool fold) {
    const ChainParams& p = c->p;
    hipLaunchKernelGGL(k_split_tables, dim3(p.KT), dim3(256), 0, c->stream, p, c->dNk, c->dS, c->dDNk, c->dDS, c->dAlpha,
                       c->dPi, c->dTheta, c->dSplitTab);
    HIP_TRY(hipGetLastError());
    NaScoreArgs a{};
    a.Xb = c->dXnb; a.Mb = c->dPnMb; a.rows = c->predM; a.tab = c->dSplitTab; a.off = c->dPnOff; a.col = c->dPnCol;
    a.out = logdens; a.resp = resp; a.cell = cell;
    if (fold) {
        a.run_max = c->dPredMax; a.run_sum = c->dPredSum; a.resp_acc = c->pred_resp ? c->dRespAcc : nullptr;
        a.cell_max = c->dCellMax; a.cell_sum = c->dCellSum;
    }
    if (na_form_of(p, c->generic).lds) {
        const int64_t ntiles = (a.rows + kScoreThreads - 1) / kScoreThreads;
        hipLaunchKernelGGL(c->pn_fn, dim3((int)(ntiles < c->pn_grid_max ? ntiles : c->pn_grid_max)), dim3(kScoreThreads),
                           c->pn_lds, c->stream, p, a);
    } else {
        double* const scr = c->generic ? c->dScratch : c->dPnScratch;
        const int64_t stride = c->generic ? c->scratch_stride : c->pn_scratch_stride;
        const int64_t nb = (a.rows + 255) / 256, maxb = stride / 256;
        hipLaunchKernelGGL(k_score_na_generic, dim3((unsigned)(nb < maxb ? nb : maxb)), dim3(256), 0, c->stream, p, a, scr, stride);
    }
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
int enqueue_predict(bmm_chain* c, double* logdens, double* resp, bool fold, double* cell = nullptr) {
    if (c->predM <= 0) return BMM_OK;
    if (c->pred_cells > 0) {
        const int rc = launch_score_na(c, logdens, resp, cell, fold);
        if (rc) return rc;
        if (fold) c->pred_folded++;
        return BMM_OK;
    }
    ScoreArgs a{};
    a.Xb = c->dXnb; a.rows = c->predM; a.out = logdens; a.resp = resp;
    if (fold) { a.run_max = c->dPredMax; a.run_sum = c->dPredSum; a.resp_acc = c->pred_resp ? c->dRespAcc : nullptr; }
    const int rc = launch_score(c, a, false);
    if (rc) return rc;
    if (fold) c->pred_folded++;
    return BMM_OK;
}
// the end of sweep j: its state is folded when a predictive run or bmm_chain_sweeps_predict asked for it
int sweep_end_predict(bmm_chain* c, int j) {
    if (!c->pred_rec.folds(j) || c->predM <= 0) return BMM_OK;
    return enqueue_predict(c, c->pred_rec.row<double>(j), nullptr, true);
}

// ---- leave-one-out predictive of the fitted rows ----
// Score every fitted row against state j with its own contribution removed, stream-ordered behind whatever produced
// that state: ell receives this state's values (device, may be null); fold adds them to the accumulators.
int enqueue_loo(bmm_chain* c, int j, double* ell, bool fold) {
    ScoreArgs a{};
    a.X = c->dX; a.Xb = c->dXb; a.rows = c->p.N; a.z = explicit_params(c->p.mode) ? nullptr : label_row(c, j);
    a.out = ell; a.acc = fold ? c->dLooAcc : nullptr; a.n = c->loo_folded;
    const int rc = launch_score(c, a, true);
    if (rc) return rc;
    if (fold) c->loo_folded++;
    return BMM_OK;
}
// ---- log joint trace and keep-best allocation ----
// Score the chain's state after sweep j from its statistics as they stand, stream-ordered behind whatever produced
// them: the row goes to dLjOut and to `row` (device, may be null); fold also offers the state to the keep-best cell
// and, when it won, copies its labels.
LjArgs lj_args(bmm_chain* c) {
    const ChainParams& p = c->p;
    LjArgs a{};
    a.Nk = c->dNk; a.S = c->dS; a.dNk = c->dDNk; a.dS = c->dDS;
    a.mask = c->fs_mask ? c->dFsMask : nullptr;
    a.alpha_ptr = c->dAlpha;
    a.k_open = c->alloc_on ? c->dEaK : nullptr;
    a.log_prior_k = c->alloc_on ? c->dEaLogPrior : nullptr;
    a.lik = c->dLjLik; a.prior = c->dLjPrior; a.out = c->dLjOut; a.best = c->dLjBest;
    a.rho = c->fs_rho;
    a.kind = c->alloc_on ? LJ_ALLOC : (p.mode == MODE_DP ? LJ_DP : (p.mode == MODE_SB ? LJ_SB : LJ_FINITE));
    return a;
}
int launch_log_joint(bmm_chain* c, const LjArgs& a) {
    const ChainParams& p = c->p;
    hipLaunchKernelGGL(k_log_joint, dim3((unsigned)(p.K + (a.mask ? 1 : 0))), dim3(kLjLanes), 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_log_joint_finish, dim3(1), dim3(64), 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
int enqueue_log_joint(bmm_chain* c, int j, double* row, bool fold) {
    LjArgs a = lj_args(c);
    a.out_row = row; a.sweep = j; a.fold = fold ? 1 : 0;
    const int rc = launch_log_joint(c, a);
    if (rc || !fold) return rc;
    const int64_t nb = (c->p.N + 255) / 256;
    hipLaunchKernelGGL(k_log_joint_keep, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream,
                       (const LjBest*)c->dLjBest, (const int32_t*)label_row(c, j), c->p.N, c->dLjZ);
    HIP_TRY(hipGetLastError());
    c->lp_folded++;
    return BMM_OK;
}
// ---- pairwise local-dependence check ----
// The grid of k_pc_counts and the bytes behind it, a pure function of (N, Kc, M): a tile per kPcTile x kPcTile block of
// the upper triangle, kPcKA labels per workgroup and further label blocks on grid.z, and as many row slices as bring
// the grid to about eight workgroups per compute unit of a 256-unit device, none shorter than two rounds.
struct PcPlan {
    int64_t C, cps, npairs;
    int tiles, slices, kblocks, ka;
    size_t bytes_slices, bytes_counts, bytes_fold;
};
PcPlan pc_plan(int64_t N, int Kc, int M) {
    PcPlan q{};
    q.C = (N + 63) / 64;
    q.npairs = pc_npairs(M);
    const int T = (M + kPcTile - 1) / kPcTile;
    q.tiles = T * (T + 1) / 2;
    q.ka = kPcKA;
    q.kblocks = (Kc + q.ka - 1) / q.ka;
    int64_t most = 2048 / ((int64_t)q.tiles * q.kblocks);
    if (most < 1) most = 1;
    int64_t cps = ((q.C + most - 1) / most + kPcRound - 1) / kPcRound * kPcRound;
    if (cps < 2 * kPcRound) cps = 2 * kPcRound;
    q.cps = cps;
    q.slices = (int)((q.C + cps - 1) / cps);
    q.bytes_slices = (size_t)M * (size_t)q.C * sizeof(uint64_t);
    q.bytes_counts = (size_t)Kc * ((size_t)q.npairs + (size_t)M + 1) * sizeof(uint32_t);
    q.bytes_fold = (size_t)q.npairs * (5 * sizeof(double) + sizeof(long long) + 2 * sizeof(int32_t) + sizeof(uint32_t));
    return q;
}
// Count and score the label row z (device, 0-based, every row seated), stream-ordered behind whatever wrote it: the
// state's values go to dPcZ / dPcX2 / dPcDf and to `row` (device, may be null); fold adds them to the sums.
int enqueue_pair_check(bmm_chain* c, const int32_t* z, double* row, bool fold) {
    const PcPlan q = pc_plan(c->p.N, c->p.K, c->pc_M);
    HIP_TRY(hipMemsetAsync(c->dPcCnt, 0, c->pc_count_bytes, c->stream));
    PcArgs a{};
    a.Xt = c->dPcXt; a.z = z; a.N = c->p.N; a.C = q.C; a.cps = q.cps; a.M = c->pc_M; a.Kc = c->p.K;
    a.cnt = c->dPcCnt; a.marg = c->dPcMarg; a.nk = c->dPcNk;
    const dim3 grid((unsigned)q.tiles, (unsigned)q.slices, (unsigned)q.kblocks);
    hipLaunchKernelGGL((k_pc_counts<kPcKA, kPcR>), grid, dim3(kPcThreads), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    PcStatArgs s{};
    s.cnt = c->dPcCnt; s.marg = c->dPcMarg; s.nk = c->dPcNk; s.M = c->pc_M; s.Kc = c->p.K;
    s.z = c->dPcZ; s.x2 = c->dPcX2; s.df = c->dPcDf; s.out_row = row;
    s.sum_z = c->dPcSumZ; s.sum_z2 = c->dPcSumZ2; s.sum_x2 = c->dPcSumX2; s.sum_df = c->dPcSumDf; s.n_z = c->dPcNz; s.n11 = c->dPcN11;
    s.fold = fold ? 1 : 0;
    hipLaunchKernelGGL(k_pc_stats, dim3((unsigned)((q.npairs + 255) / 256)), dim3(256), 0, c->stream, s);
    HIP_TRY(hipGetLastError());
    if (fold) c->pc_folded++;
    return BMM_OK;
}
// X is cut into the check's column slices once, when it is armed: new data under an armed check would leave slices of
// the old matrix behind, so the data entry points refuse until the check is disarmed
int pc_data_locked(const bmm_chain* c) {
    if (c->na_on)
        return set_err(BMM_E_STATE, "missing cells are declared on the data the chain holds: withdraw them (bmm_chain_set_missing with "
                       "no cells) before new data is set, and declare them again afterwards");
    if (c->pc_on)
        return set_err(BMM_E_STATE, "the pair check is armed on the data the chain holds: disarm it (bmm_chain_set_pair_check with "
                       "no features) before new data is set, and arm it again afterwards");
    return BMM_OK;
}
// whether sweep j is one the check evaluates: folded, and a multiple of the stride from the recording's first row
bool stride_folds(const SweepTrace& rec, int stride, int j) { return rec.folds(j) && (j - rec.base) % stride == 0; }
bool pc_folds(const bmm_chain* c, int j) { return c->pc_on && stride_folds(c->pc_rec, c->pc_stride, j); }
// the posterior summary's share of a sweep end (defined with the ECR pass it enqueues)
int sum_sweep_end(bmm_chain* c, int j);
int sum_start_state(bmm_chain* c, const int32_t* row0);
void sum_release(bmm_chain* c);
// the end of sweep j: what a predictive run, a leave-one-out run, a log joint trace, a pair check or the resident calls
// asked to fold
int sweep_end_folds(bmm_chain* c, int j) {
    int rc = sweep_end_predict(c, j);
    if (rc == BMM_OK && c->loo_rec.folds(j) && c->loo_on) rc = enqueue_loo(c, j, c->loo_rec.row<double>(j), true);
    if (rc == BMM_OK && c->lp_rec.folds(j) && c->lp_on && !c->fold_defer) rc = enqueue_log_joint(c, j, c->lp_rec.row<double>(j), true);
    if (rc == BMM_OK && pc_folds(c, j) && !c->fold_defer) rc = enqueue_pair_check(c, label_row(c, j), c->pc_rec.row<double>(j), true);
    if (rc == BMM_OK && c->sum_on) rc = sum_sweep_end(c, j);
    return rc;
}

// what the predictive, the leave-one-out summary and the split-merge moves answer a chain with a feature mask
// (DESIGN.md section 16): their tables and ratios are those of the model in which every feature clusters
int fs_mask_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s is written for the model in which every feature clusters: not offered on a chain "
                   "with a feature mask (feature selection)", what);
}
int na_refuses(const char* what);  // (... a chain with declared missing cells: DESIGN.md section 23)

// ---- split-merge moves ----
int temper_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s is not offered on a tempered chain (parallel tempering): it is written for the "
                   "likelihood at full power", what);
}
int sm_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_STATE, "split-merge moves are not offered on a sharded chain");
    if (c->na_on) return na_refuses("a split-merge move");
    if (c->cs_on) return cs_refuses("a split-merge move");
    if (c->cat_on) return cat_refuses("the split-merge ratio");
    if (c->temper_on) return temper_refuses("the split-merge ratio");
    if (c->p.mode != MODE_DP)
        return set_err(BMM_E_UNSUPPORTED, "split-merge moves are offered for the DP sampler only (the finite sampler gives an "
                       "emptied label probability 0 for ever: a different model from the one the move's ratio targets)");
    if (c->fs_mask) return fs_mask_refuses("the split-merge ratio");
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "split-merge moves read the bit planes: not offered on the int32 layout");
    if (c->p.P > kSmMaxP) return set_err(BMM_E_UNSUPPORTED, "split-merge moves are offered up to %d features", kSmMaxP);
    if (c->p.N < 2) return set_err(BMM_E_ARG, "a split-merge move needs two rows");
    return BMM_OK;
}
int sm_seated(const bmm_chain* c) {
    if (!c->started || c->sweep < 1) return set_err(BMM_E_STATE, "the chain has rows without a label: run a sweep first");
    return BMM_OK;
}
// the buffers of the moves, for `scans` intermediate scans
int sm_setup(bmm_chain* c, int scans) {
    const size_t n = (size_t)c->p.N;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dSmSide) {
        HIP_TRY(hipMalloc(&c->dSmSide, n));
        HIP_TRY(hipMalloc(&c->dSmSideLaunch, n));
        HIP_TRY(hipMalloc(&c->dSmLq, n * sizeof(double)));
        HIP_TRY(hipMalloc(&c->dSmCell, sizeof(SmCell)));
        HIP_TRY(hipMalloc(&c->dSmCounters, 5 * sizeof(long long)));
        HIP_TRY(hipMemsetAsync(c->dSmCounters, 0, 5 * sizeof(long long), c->stream));
        HIP_TRY(hipMemsetAsync(c->dSmCell, 0, sizeof(SmCell), c->stream));
    }
    if (scans + 2 > c->sm_sets) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // moves enqueued earlier may still use the old sets
        if (c->dSmStat) HIP_TRY(hipFree(c->dSmStat));
        c->dSmStat = nullptr;
        HIP_TRY(hipMalloc(&c->dSmStat, (size_t)(scans + 2) * 2 * (c->p.P + 1) * sizeof(int32_t)));
        c->sm_sets = scans + 2;
    }
    c->sm_scans = scans;
    return BMM_OK;
}
// one move on label row `z`, ahead of sweep `tag`, enqueued on the stream: the DP chain's, or (ALLOC) the allocation
// chain's, which has its own numbering, scans, cell and counters and shares the side bytes and the statistic sets
template <bool ALLOC>
int enqueue_move(bmm_chain* c, int32_t* z, int tag, bool keep_launch) {
    const ChainParams& p = c->p;
    int& last_tag = ALLOC ? c->as_tag : c->sm_tag;
    uint32_t& ctr = ALLOC ? c->as_ctr : c->sm_ctr;
    const int scans = ALLOC ? c->as_scans : c->sm_scans;
    if (last_tag != tag) { last_tag = tag; ctr = 0; }
    SmArgsOf<ALLOC> g{};
    SmArgs& a = g;
    a.Xb = c->dXb; a.z = z; a.Nk = c->dNk; a.S = c->dS; a.alpha_ptr = c->dAlpha;
    a.side = c->dSmSide; a.side_launch = keep_launch ? c->dSmSideLaunch : nullptr; a.lq = c->dSmLq;
    a.stat = c->dSmStat; a.sweep = (uint32_t)tag; a.move = ctr++; a.scans = scans;
    if constexpr (ALLOC) {
        a.cell = &c->dAsCell->m; a.counters = c->dAsCounters;
        g.K = c->dEaK; g.log_prior_k = c->dEaLogPrior; g.as_cell = c->dAsCell; g.a = c->alloc_a;
    } else {
        a.cell = c->dSmCell; a.counters = c->dSmCounters;
    }
    const size_t set_bytes = (size_t)2 * (p.P + 1) * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(c->dSmStat, 0, (size_t)(scans + 2) * set_bytes, c->stream));
    const unsigned grid = (unsigned)((p.N + kSmThreads - 1) / kSmThreads);
    hipLaunchKernelGGL(k_sm_launch<ALLOC>, dim3(grid), dim3(kSmThreads), set_bytes, c->stream, p, g);
    HIP_TRY(hipGetLastError());
    const size_t scan_lds = (size_t)4 * p.P * sizeof(double) + set_bytes;
    for (int t = 1; t <= scans + 1; ++t) {
        hipLaunchKernelGGL(k_sm_scan<ALLOC>, dim3(grid), dim3(kSmThreads), scan_lds, c->stream, p, g, t, t == scans + 1 ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sm_decide<ALLOC>, dim3(1), dim3(1024), 0, c->stream, p, g);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sm_commit<ALLOC>, dim3(grid), dim3(kSmThreads), 0, c->stream, p, g);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// what a step entry point returns of a move just synchronised: the DP move's part of the record (labels 1-based) and
// the two side-byte arrays; `out` is bmm_split_merge_step or bmm_alloc_split_step
template <class Step>
int sm_step_out(bmm_chain* c, const SmCell& h, uint32_t move, Step* out) {
    out->row_i = h.row_i; out->row_j = h.row_j; out->label_a = h.label_a + 1; out->label_b = h.label_b + 1;
    out->kind = h.kind; out->accepted = h.accepted; out->members = h.members;
    for (int q = 0; q < 2; ++q) { out->n_before[q] = h.n_before[q]; out->n_after[q] = h.n_after[q]; }
    out->log_prior = h.log_prior; out->log_lik = h.log_lik; out->log_q = h.log_q; out->log_u = h.log_u; out->log_r = h.log_r;
    out->sweep = (uint32_t)(c->sweep + 1); out->move = move;
    const size_t n = (size_t)c->p.N;
    if (h.kind == SM_SKIPPED) {  // no launch state: every row outside
        if (out->launch_side) std::memset(out->launch_side, 255, n);
        if (out->proposal_side) std::memset(out->proposal_side, 255, n);
        return BMM_OK;
    }
    if (out->launch_side) HIP_TRY(hipMemcpy(out->launch_side, c->dSmSideLaunch, n, hipMemcpyDeviceToHost));
    if (out->proposal_side) HIP_TRY(hipMemcpy(out->proposal_side, c->dSmSide, n, hipMemcpyDeviceToHost));
    return BMM_OK;
}
// the five counters of either kind of move, zeros before the first one
int sm_counters_out(bmm_chain* c, const long long* counters, int64_t out[5]) {
    if (!c || !out) return set_err(BMM_E_ARG, "null argument");
    for (int q = 0; q < 5; ++q) out[q] = 0;
    if (!counters) return BMM_OK;
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    long long h[5];
    HIP_TRY(hipMemcpy(h, counters, sizeof h, hipMemcpyDeviceToHost));
    for (int q = 0; q < 5; ++q) out[q] = h[q];
    return BMM_OK;
}

// ---- the allocation sampler ----
int alloc_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s assumes a fixed number of components: not offered on a chain of the allocation sampler", what);
}
// one eject / absorb move on label row `z`, ahead of sweep `tag`, enqueued on the stream
int enqueue_ea(bmm_chain* c, int32_t* z, int tag) {
    const ChainParams& p = c->p;
    if (c->ea_tag != tag) { c->ea_tag = tag; c->ea_ctr = 0; }
    EaArgs a{};
    a.Xb = c->dXb; a.z = z; a.Nk = c->dNk; a.S = c->dS; a.K = c->dEaK; a.log_prior_k = c->dEaLogPrior;
    a.side = c->dEaSide; a.stat = c->dEaStat; a.cell = c->dEaCell; a.counters = c->dEaCounters;
    a.a = c->alloc_a; a.eject_a = c->alloc_e; a.sweep = (uint32_t)tag; a.move = c->ea_ctr++;
    const size_t set_bytes = (size_t)(p.P + 1) * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(c->dEaStat, 0, set_bytes, c->stream));
    const unsigned grid = (unsigned)((p.N + kEaThreads - 1) / kEaThreads);
    hipLaunchKernelGGL(k_ea_launch, dim3(grid), dim3(kEaThreads), set_bytes, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ea_decide, dim3(1), dim3(1024), 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ea_commit, dim3(grid), dim3(kEaThreads), 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

// ---- feature selection ----
// the gamma-step behind the end of sweep j, stream-ordered: no host wait
int enqueue_fs_gamma(bmm_chain* c, int j) {
    const ChainParams& p = c->p;
    FsArgs a{};
    a.Nk = c->dNk; a.S = c->dS; a.mask = c->dFsMask; a.gamma = c->dFsGamma; a.rec = c->dFsRec;
    a.gamma_row = c->fs_rec.row<uint8_t>(j);
    a.incl_count = c->dFsCount; a.incl_prob = c->dFsProb; a.logit_rho = c->fs_logit; a.sweep = (uint32_t)j;
    a.fold = c->fs_rec.folds(j) ? 1 : 0;
    hipLaunchKernelGGL(k_fs_gamma, dim3((unsigned)((p.P + 31) / 32)), dim3(kFsThreads), 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    if (a.fold) c->fs_folded++;
    c->fs_last = j;
    return BMM_OK;
}

// ---- missing data: the imputation step ----
NaArgs na_args(bmm_chain* c, const int32_t* z, uint32_t sweep, bool fold) {
    NaArgs a{};
    a.row = c->dNaRow; a.word = c->dNaWord; a.mask = c->dNaMask; a.first = c->dNaFirst; a.n_sites = c->na_sites;
    a.Xb = c->dXb; a.z = z; a.S = c->dS; a.cnt = c->dNaCnt; a.Nk = c->dNk; a.dNk = c->dDNk; a.dS = c->dDS;
    a.phi = explicit_params(c->p.mode) ? c->dTheta : c->dNaPhi;
    a.sum_phi = c->dNaSum; a.ones = c->dNaOnes; a.sweep = sweep; a.fold = fold ? 1 : 0;
    return a;
}
// The step behind sweep j, stream-ordered behind everything the sweep enqueued: the census and the auxiliary rates of
// a counting chain (an explicit chain's rates are its theta), then the draw.  The deltas go into the folded S.
int enqueue_na_step(bmm_chain* c, int j) {
    const ChainParams& p = c->p;
    const bool fold = c->na_rec.folds(j);
    const NaArgs a = na_args(c, label_row(c, j), (uint32_t)j, fold);
    const size_t KP = (size_t)p.K * p.P;
    const dim3 grid((unsigned)c->na_grid), wg(kNaThreads);
    if (!explicit_params(p.mode)) {
        HIP_TRY(hipMemsetAsync(c->dNaCnt, 0, 2 * KP * sizeof(int32_t), c->stream));
        if (c->na_lds) hipLaunchKernelGGL(k_na_census<true>, grid, wg, 2 * KP * sizeof(int32_t), c->stream, p, a);
        else hipLaunchKernelGGL(k_na_census<false>, grid, wg, 0, c->stream, p, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_na_phi, dim3((unsigned)((KP + kNaThreads - 1) / kNaThreads)), wg, 0, c->stream, p, a);
        HIP_TRY(hipGetLastError());
    }
    if (c->na_lds) hipLaunchKernelGGL(k_na_draw<true>, grid, wg, KP * (sizeof(double) + sizeof(int32_t)), c->stream, p, a);
    else hipLaunchKernelGGL(k_na_draw<false>, grid, wg, 0, c->stream, p, a);
    HIP_TRY(hipGetLastError());
    if (fold) c->na_folded++;
    return BMM_OK;
}
// what the options that read the data matrix as observed answer a chain with declared missing cells
int na_refuses(const char* what) {
    return set_err(BMM_E_UNSUPPORTED, "%s is not offered on a chain with missing cells (bmm_chain_set_missing): it would read "
                   "the completed matrix as if it were observed", what);
}

// ---- k-modes++ initial allocation ----
// who may be initialised on the device, whatever the moment
int init_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_STATE, "the initialisation is not offered on a sharded chain");
    if (c->na_on) return na_refuses("a data-driven start");
    if (c->cs_on) return cs_refuses("a data-driven start");
    if (c->cat_on) return cat_refuses("a data-driven start (its distance)");
    if (explicit_params(c->p.mode))
        return set_err(BMM_E_UNSUPPORTED, "a data-driven start is offered for the collapsed and DP samplers only: the stick-breaking and "
                       "full samplers start from pi and theta");
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "the initialisation reads the bit planes: not offered on the int32 layout");
    if (c->alloc_on) return alloc_refuses("a device start");
    return BMM_OK;
}
// whether k_init_assign counts its labels in LDS (centres and histogram within kInitLdsBudget: at K = 20 up to P = 1587) or
// leaves the counting to k_count_labels_generic: a pure function of (Kc, P)
bool init_counts_in_lds(int Kc, int P) {
    const size_t W = ((size_t)P + 31) / 32;
    return (size_t)Kc * W * 4 + (size_t)Kc * ((size_t)P + 1) * 4 <= kInitLdsBudget;
}
// One initialisation into `lab` (N labels, 0-based) on the chain's stream: every launch enqueued at once, one wait at
// the end.  The chain itself is not touched.
int init_run(bmm_chain* c, int kind, int Kc, int iters, int32_t* lab, bmm_init_info* info) {
    const ChainParams& p = c->p;
    if (kind != BMM_INIT_KMODES) return set_err(BMM_E_ARG, "unknown kind of initialisation %d", kind);
    if (Kc < 1 || Kc > p.K) return set_err(BMM_E_ARG, "n_centres = %d outside 1..%d", Kc, p.K);
    if (iters < 0) return set_err(BMM_E_ARG, "iters must be >= 0");
    const size_t W = ((size_t)p.P + 31) / 32, N = (size_t)p.N;
    if ((size_t)Kc * W * 4 > (size_t)kInitMaxCentreBytes)
        return set_err(BMM_E_UNSUPPORTED, "%d centres of %zu words need %zu bytes, above the %d the initialisation keeps in LDS", Kc, W,
                       (size_t)Kc * W * 4, kInitMaxCentreBytes);
    if (!c->have_data || !c->dXb) return set_err(BMM_E_STATE, "data matrix not set");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nb = (N + kInitThreads - 1) / kInitThreads;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    // one block: the cell, the rows, the counts and the centres (cleared together), then dist and the block sums
    const size_t o_rows = up(sizeof(InitCell)), o_nk = o_rows + up((size_t)Kc * 8), o_s = o_nk + up((size_t)Kc * 4),
                 o_cen = o_s + up((size_t)Kc * p.P * 4), o_dist = o_cen + up((size_t)Kc * W * 4), o_bs = o_dist + up(N * 4),
                 bytes = o_bs + up(nb * 4);
    DevBuf blk;
    HIP_TRY(blk.alloc(bytes));
    char* const b0 = blk.as<char>();
    HIP_TRY(hipMemsetAsync(b0, 0, o_dist, c->stream));
    InitArgs a{};
    a.Xb = c->dXb; a.lab = lab; a.cell = reinterpret_cast<InitCell*>(b0); a.rows = reinterpret_cast<long long*>(b0 + o_rows);
    a.Nk = reinterpret_cast<int32_t*>(b0 + o_nk); a.S = reinterpret_cast<int32_t*>(b0 + o_s);
    a.centres = reinterpret_cast<uint32_t*>(b0 + o_cen); a.dist = reinterpret_cast<int32_t*>(b0 + o_dist);
    a.blocksum = reinterpret_cast<int32_t*>(b0 + o_bs); a.Kc = Kc;
    struct Timed {  // (EventPair's events carry no time)
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Timed() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e[0]));
    HIP_TRY(hipEventCreate(&ev.e[1]));
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    const dim3 grid((unsigned)nb), wg(kInitThreads);
    for (int m = 0; m < Kc; ++m) {
        if (m > 0) hipLaunchKernelGGL(k_init_pick, dim3(1), dim3(1024), 0, c->stream, p, a, m, (int)nb);
        hipLaunchKernelGGL(k_init_dist, grid, wg, 0, c->stream, p, a, m);
        HIP_TRY(hipGetLastError());
    }
    const bool in_lds = init_counts_in_lds(Kc, p.P);
    const size_t cen_bytes = (size_t)Kc * W * 4, lds = cen_bytes + (in_lds ? (size_t)Kc * (p.P + 1) * 4 : 0);
    // up to kInitLdsBudget (or kInitMaxCentreBytes) of dynamic LDS on top of the kernel's static bytes: past 64 KiB in all
    HIP_TRY(hipFuncSetAttribute(in_lds ? reinterpret_cast<const void*>(k_init_assign<true>) : reinterpret_cast<const void*>(k_init_assign<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int r = 0; r <= iters; ++r) {
        if (r > 0) hipLaunchKernelGGL(k_init_modes, dim3((unsigned)Kc), wg, 0, c->stream, p, a, r);
        if (in_lds) {
            hipLaunchKernelGGL(k_init_assign<true>, grid, wg, lds, c->stream, p, a, r);
        } else {
            // (after `done` the labels no longer change, and the recount of unchanged labels gives the same counts)
            hipLaunchKernelGGL(k_init_assign<false>, grid, wg, lds, c->stream, p, a, r);
            HIP_TRY(hipMemsetAsync(b0 + o_nk, 0, o_cen - o_nk, c->stream));
            hipLaunchKernelGGL(k_count_labels_generic, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, p,
                               (const int32_t*)nullptr, c->dXb, lab, a.Nk, a.S);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    InitCell h{};
    c->init_centres.assign((size_t)Kc * W, 0u);
    c->init_rows.assign((size_t)Kc, 0);
    c->init_nk.assign((size_t)Kc, 0);
    HIP_TRY(hipMemcpyAsync(&h, a.cell, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init_rows.data(), a.rows, (size_t)Kc * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init_nk.data(), a.Nk, (size_t)Kc * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init_centres.data(), a.centres, cen_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    c->init_keff = h.k_eff;
    c->init_centres.resize((size_t)h.k_eff * W);
    c->init_rows.resize((size_t)h.k_eff);
    c->init_nk.resize((size_t)h.k_eff);
    if (info) {
        info->k_eff = h.k_eff;
        info->rounds_run = h.rounds_run;
        info->changed_last = h.rounds_run > 0 ? h.changed[h.rounds_run & 1] : 0;
        info->cost = h.cost[h.rounds_run & 1];
        info->device_ms = (double)ms;
    }
    return BMM_OK;
}
// ... and into the chain: a collapsed chain that has not started gets its initial labels, a seated DP chain between
// sweeps a new allocation and the recount (the tail of bmm_chain_set_labels)
int init_labels(bmm_chain* c, int kind, int n_centres, int iters, bmm_init_info* info) {
    int rc = init_refused(c);
    if (rc) return rc;
    const ChainParams& p = c->p;
    if (p.mode == MODE_COLLAPSED) {
        if (c->started) return set_err(BMM_E_STATE, "chain already started");
        rc = init_run(c, kind, n_centres == 0 ? p.K : n_centres, iters, c->dZ[0], info);
        if (rc) return rc;
        c->have_init = true;
        return BMM_OK;
    }
    rc = sm_seated(c);
    if (rc) return rc;
    if (n_centres == 0) return set_err(BMM_E_ARG, "n_centres must be given for the DP sampler (1..%d)", p.K);
    int32_t* const cur = label_row(c, c->sweep);
    int32_t* const other = c->dZ[(c->sweep + 1) & 1];  // the row the next sweep will overwrite
    rc = init_run(c, kind, n_centres, iters, other, info);
    if (rc) return rc;
    const size_t K = (size_t)p.K, KP = K * p.P;
    const int64_t nb = (p.N + 255) / 256;
    HIP_TRY(hipMemcpyAsync(cur, other, (size_t)p.N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->dNk, 0, K * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->dS, 0, KP * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->dDNk, 0, K * kDeltaReps * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->dDS, 0, KP * kDeltaReps * sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(k_count_labels_generic, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->p, c->dX, c->dXb, cur,
                       c->dNk, c->dS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMM_OK;
}

// The label row that the moves ahead of sweep j work on and the sweep then reads: row j - 1, or a copy of it when the
// trace holds the original (a row of the trace stays as it was recorded, with the theta-hat of its sweep).
int moves_row(bmm_chain* c, int j, int32_t** row) {
    *row = label_row(c, j - 1);
    if (c->dTrace && j - 1 >= c->burnin) {
        int32_t* const copy = c->dZ[(j - 1) & 1];
        HIP_TRY(hipMemcpyAsync(copy, *row, (size_t)c->p.N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        *row = copy;
    }
    return BMM_OK;
}

// one sweep (index j >= 1) enqueued on the stream
// phase 0: whole sweep; 1: z-resample only; 2: parameter draws and tables only (sharded chains)
int enqueue_sweep(bmm_chain* c, int j, int phase = 0) {
    const ChainParams& p = c->p;
    const int32_t* zin = (p.mode != MODE_COLLAPSED && j == 1) ? nullptr : label_row(c, j - 1);
    int32_t* zout = label_row(c, j);
    const bool rec = c->in_run && j >= c->burnin;
    const int s = j - c->burnin;
    double* th_tr = rec ? c->dThetaTrace + (size_t)s * p.K * p.P : nullptr;
    double* al_tr = rec ? c->dAlphaTrace + s : nullptr;
    if (!rec && c->sum_on && c->sum_rec.folds(j)) { th_tr = c->sum.theta_row; al_tr = c->sum.alpha_row; }  // a resident chain's fold
    int32_t* nk_tr = c->dNkTrace ? c->dNkTrace + (size_t)(j - c->nk_trace_base) * p.K : nullptr;
    if (explicit_params(p.mode)) {
        if (phase != 2) {
            int rc = launch_resample(c, zin, zout, 0, p.N, (uint32_t)j);
            if (rc == BMM_OK && c->cs_on) rc = launch_constrain(c, zin, zout, 0, p.N);
            if (rc) return rc;
        }
        if (phase == 1) return launch_reduce_deltas(c);  // sharded chain: the caller all-reduces replica 0 now
        hipLaunchKernelGGL(k_sb_params, dim3(1), dim3(1024), 0, c->stream, p, c->dNk, c->dS, c->dDNk,
                           c->dDS, c->dAlpha, c->dPi, (uint32_t)j, rec ? c->dPiTrace + s : nullptr, c->S,
                           c->dViable, nk_tr);
        HIP_TRY(hipGetLastError());
        // (one workgroup more than clusters: the concentration's update runs beside the theta draws)
        hipLaunchKernelGGL(k_sb_theta_tables, dim3(p.KT + 1), dim3(256), 0, c->stream, p, c->dNk, c->dS,
                           c->dPi, c->dTheta, 1, (uint32_t)j, th_tr, c->dTab, c->dAlpha, al_tr, c->dViable);
        HIP_TRY(hipGetLastError());
        const int rc = sweep_end_folds(c, j);
        // the missing cells, redrawn from the theta this sweep has just drawn: behind everything else of the sweep
        return rc == BMM_OK && c->na_on ? enqueue_na_step(c, j) : rc;
    }
    // the armed moves, ahead of the sweep's first table build: split-merge (a DP chain) or eject / absorb (a finite one)
    const int n_sm = c->sm_moves, n_ea = c->alloc_on ? c->alloc_moves : 0, n_as = c->alloc_on ? c->as_moves : 0;
    if ((n_sm > 0 || n_ea > 0 || n_as > 0) && j >= 2 && phase == 0) {
        int32_t* row = nullptr;
        int rc = moves_row(c, j, &row);
        if (rc) return rc;
        zin = row;
        for (int m = 0; m < n_sm && rc == BMM_OK; ++m) rc = enqueue_move<false>(c, row, j, false);
        for (int m = 0; m < n_ea && rc == BMM_OK; ++m) rc = enqueue_ea(c, row, j);
        for (int m = 0; m < n_as && rc == BMM_OK; ++m) rc = enqueue_move<true>(c, row, j, false);  // (the allocation chain's split-merge moves)
        if (rc) return rc;
    }
    int64_t lo = 0;
    while (lo < p.N) {
        int64_t len = c->batch;
        if (p.mode == MODE_DP && j == 1) {  // seat the first sweep 1,1,2,4,... at a time
            const int64_t dbl = lo < 1 ? 1 : lo;
            if (dbl < len) len = dbl;
        }
        const int64_t hi = lo + len > p.N ? p.N : lo + len;
        // (SELF kernels build their own image from Nk, S and the previous launch's deltas; a sweep that hands its
        // probabilities to the host runs the emitting twin, which reads the image k_count_tables writes)
        int rc = c->form.self && !c->probs_dst ? BMM_OK : launch_count_tables(c);
        if (rc) return rc;
        rc = launch_resample(c, zin, zout, lo, hi, (uint32_t)j);
        if (rc == BMM_OK && c->cs_on) rc = launch_constrain(c, zin, zout, lo, hi);  // before the next table build
        if (rc) return rc;
        lo = hi;
    }
    hipLaunchKernelGGL(k_count_sweep_end, dim3(1), dim3(1024), 0, c->stream, p, c->dNk, c->dS, c->dDNk,
                       c->dDS, c->dAlpha, (uint32_t)j, th_tr, al_tr, nk_tr);
    HIP_TRY(hipGetLastError());
    if (int32_t* const k_row = c->k_rec.row<int32_t>(j))  // the allocation sampler's K after this sweep, device to device
        HIP_TRY(hipMemcpyAsync(k_row, c->dEaK, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (c->fs_on) {  // the gamma-step, from the counts the sweep end has just folded; sweep j + 1 reads its mask
        const int rc = enqueue_fs_gamma(c, j);
        if (rc) return rc;
    }
    const int rc = sweep_end_folds(c, j);
    return rc == BMM_OK && c->na_on ? enqueue_na_step(c, j) : rc;  // the missing cells: behind everything else of the sweep
}

// The resident kernel for a shape, batch and X layout: the forms to try, in order, each with its dynamic LDS.
// The first is always there and is what runs unless a later one is taken; a later one is tried only when the one
// before it was taken and is taken when the runtime fits at least one of its workgroups on a CU (pick_kernel).
// `minus` is the own-cluster tier of KernelForm.  A pure function: no device and no chain enter.
struct KernelPlan {
    int n = 0;
    KernelForm form[3];
    size_t lds[3] = {0, 0, 0};
    bool named_size = false;  // form[0] has its workgroup size from BMM_DEBUG_THREADS (stage_width)
};
KernelPlan plan_kernel(const ChainParams& p, bool bits, int minus, int64_t batch, int num_cus, bool shares_device,
                       size_t lds_bytes_base, const DebugSwitches& d, bool masked = false, bool categorical = false) {
    const bool alt = p.W != kGroupW;  // the narrower groups: default-sized kernels only
    KernelForm f{p.KT, threads_for(p.KT, bits), minus, bits, 1, false, p.W, false};
    KernelPlan plan;
    // The packed kernel takes the place of every form it exists for (not with a feature mask or the allocation
    // sampler's tables: the band of draw_pk rests on k_count_tables' entries, all of them <= 0); its LDS is its own
    // image.  The choice of the form itself -- size, lanes, step-down -- is made as before, from the binary64 image.
    // Only for launches that give a wave at least four chunks.  The rule dates from the kernel's exact pass, a tail of
    // microseconds behind the workgroup's barrier for as little as one queued observation, while the packed scoring
    // saves about 2 us per chunk and wave: same-box, C5 (9.5 chunks per wave) +19 %; the north-star shape and c3 (one
    // chunk per wave) lost 11 % and 6 % with the packed kernel (profiles/r05/README.md).  The pass is gone -- uncertain
    // lanes are settled inside the tile loop -- and the rule stays until a change of its own moves it: it decides
    // which kernel other workloads run (profiles/r08/README.md has ns and c3 with the rule lifted).
    const size_t pk_lds = explicit_params(p.mode) ? 0 : pk_image_bytes(p);
    auto offer = [&](KernelForm g, size_t lds) {
        KernelForm h = g;
        h.pk = true;
        h.pipe = pk_pipelined(h.kt, h.nt, h.gw) && !d.nopipe;
#ifdef BMM_EXP_PK_ALWAYS  // timing experiments only (tools/exp_lib.sh): the rule below lifted, as BMM_DEBUG_PK lifts it
        const bool long_launch = true;
#else
        const bool long_launch = batch >= (int64_t)4 * num_cus * g.nt;
#endif
        if (!masked && !d.nopk && (long_launch || d.pk) && !g.self && !explicit_params(p.mode) && instantiated(h, false) &&
            pk_lds <= kLdsMax && batch < ((int64_t)1 << 31)) { g = h; lds = pk_lds; }
        plan.form[plan.n] = g; plan.lds[plan.n++] = lds;
    };
    // Two lanes per observation: always above 32 accumulators (registers), and from 16 up when a launch is so
    // short that the default form would give a wave at most a chunk or two -- then a launch is all latency
    // (the north-star shape: 15 us per launch of which 4 are arithmetic, VALU busy 27 %), and the two-lane
    // form halves the chain of dependent work per wave (half the categories to score, to exponentiate and
    // to compare per lane) at the same number of workgroups.  Same draw, bit for bit.
    // "Short" = the batch cannot give every CU a one-lane workgroup of 768 threads (196 608 observations on 256
    // CUs): below that the one-lane form steps down to 512 threads and two waves per SIMD.  Same-box, north-star
    // shape by batch: 125 000 two-lane +11 %, 162 500 +11 %, 200 000 -2.5 %, 250 000 -8 % (profiles/r03/ab_smallsplit.log).
    // (not for chains that share their device: several chains' launches fill the chip between them, and then
    // the one-lane form's lower total work wins -- four north-star chains: 14.8 k against 12.1 k sweeps/s)
    const bool short_launch = BMM_SMALL_SPLIT && !shares_device && p.KT >= 16 && !alt && (batch < (int64_t)num_cus * kThreadsMid || d.split);
    if (bits && (p.KT > 32 || short_launch) && minus != 2 && !d.nosplit) {
        const KernelForm g = resized(f, kThreadsSplit, 2);
        if (instantiated(g, false)) f = g;
    }
    if (d.threads >= 0 && !alt) {
        // the experiment knob: honoured up to 20 accumulators, and up to 32 on bit planes below 1024 threads (the
        // other kernels of a chosen size are in the library but nothing runs them)
        const KernelForm g = resized(f, d.threads);
        if (instantiated(g, true) && (p.KT <= 20 || (bits && g.nt != 1024))) { f = g; plan.named_size = true; }
    } else if (bits && f.lanes == 1 && !alt) {
        // a batch that cannot give every CU a workgroup of the default size gets smaller ones -- as long as they
        // still hold the whole batch in one round (250 000 observations: 245 workgroups of 1024 threads, one chunk
        // per wave, beat 256 of 768 where a quarter of the waves takes a second chunk: north-star kernel -6 %)
        for (int nt : {768, 512}) {
            if ((batch + f.nt - 1) / f.nt >= num_cus || nt >= f.nt || (batch + nt - 1) / nt > num_cus) continue;
            if (instantiated(resized(f, nt), false)) f = resized(f, nt);
        }
    }
    offer(f, lds_bytes_base);
    // a batch that cannot give every CU a workgroup runs on 256-thread workgroups instead, when the
    // tables are small enough for several of them per CU (otherwise fewer waves per CU just hurts)
    const int64_t tiles = (batch + f.nt - 1) / f.nt;
    if (!(f.lanes == 1 && !alt && tiles < num_cus && f.nt > 256 && (lds_bytes_base * 4 <= kLdsMax || d.small) && minus != 2 && d.threads < 0))
        return plan;
    f.nt = 256;
    offer(f, lds_bytes_base);
    // ... and such workgroups build the table image themselves when that is at most two logs per thread: the
    // shape is bound by launches then, and this drops k_count_tables from every batch (BASELINE config 2)
    f.self = true;
    const size_t lds = (lds_bytes_base + 7) / 8 * 8 + self_scratch_doubles(p.K, p.KT, p.P) * sizeof(double);  // scratch behind the image
    // (not for a chain with a feature mask: build_tables_self knows no mask, k_count_tables<TAB_MASK> does; nor for
    // categorical features, which keep the packed form: k_count_tables<TAB_CAT> writes its image)
    if (BMM_SELF_TABLES && bits && minus == 1 && !shares_device && self_tables_fit(p.mode, p.K, p.P, 256) && !d.noself &&
        !masked && !categorical && instantiated(f, false) && lds <= kLdsMax)
        offer(f, lds);
    return plan;
}

int tier_of(const bmm_chain* c) { return explicit_params(c->p.mode) ? 0 : (c->minus_in_lds ? 1 : 2); }

// The chain's resident kernel, set up for launching: the last form of the plan that the runtime takes.
int pick_kernel(bmm_chain* c) {
    const KernelPlan plan = plan_kernel(c->p, c->bits, tier_of(c), c->batch, c->num_cus, c->shares_device, c->lds_bytes_base,
                                        DebugSwitches{}, c->fs_mask || c->alloc_on || c->temper_on, c->cat_on);
    hipError_t e = hipSetDevice(c->device);
    for (int i = 0; i < plan.n; ++i) {
        const KernelForm& f = plan.form[i];
        const resample_fn fn = lookup(f, plan.named_size);
        int per_cu = 0;
        if (e == hipSuccess) e = kernel_fits(fn, f.nt, plan.lds[i], &per_cu);
        if (i == 0) {
            if (e != hipSuccess) return set_err(BMM_E_HIP, "kernel set-up failed: %s", hipGetErrorString(e));
            if (per_cu < 1) per_cu = 1;
        } else if (e != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            break;
        }
        c->form = f;
        c->fn = fn;
        c->lds_bytes = plan.lds[i];
        c->grid_max = per_cu * c->num_cus;
    }
    // the weight-emitting twin is set up when a hand-off first asks for it (probs_alloc)
    c->form_emit = c->bits ? emit_twin(c->form) : KernelForm{};
    c->fn_emit = nullptr;
    return BMM_OK;
}

// things that must be in place before the first sweep
int chain_start(bmm_chain* c) {
    const ChainParams& p = c->p;
    if (!c->have_data) return set_err(BMM_E_STATE, "data matrix not set");
    if (c->cat_on && !c->cat_checked) { const int rcc = cat_check(c); if (rcc) return rcc; }
    if (p.mode != MODE_DP && !c->have_init)
        return set_err(BMM_E_STATE, p.mode == MODE_COLLAPSED ? "initial labels not set"
                                                             : "initial pi/theta not set");
    HIP_TRY(hipSetDevice(c->device));
    if (p.mode == MODE_COLLAPSED) {
        // statistics of the initial allocation (collapsed_gibbs.cpp:60-63)
        int32_t* row0 = label_row(c, 0);
        if (c->cs_on) {  // the starting labels, put inside the rows' sets before anything counts them
            const int rc = launch_constrain(c, nullptr, c->dZ[0], 0, p.N, true, false);
            if (rc) return rc;
        }
        if (row0 != c->dZ[0])
            HIP_TRY(hipMemcpyAsync(row0, c->dZ[0], (size_t)p.N * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                   c->stream));
        const size_t hb = ((size_t)p.K * p.P + p.K) * sizeof(int32_t);
        const int64_t nt = (p.N + 255) / 256;
        if (c->generic)
            hipLaunchKernelGGL(k_count_labels_generic, dim3((unsigned)(nt < 2048 ? nt : 2048)), dim3(256), 0,
                               c->stream, p, c->dX, c->dXb, row0, c->dDNk, c->dDS);
        else
            hipLaunchKernelGGL(k_count_labels, dim3((unsigned)(nt < 2048 ? nt : 2048)), dim3(256), hb, c->stream,
                               p, c->dX, c->dXb, row0, c->dDNk, c->dDS);
        HIP_TRY(hipGetLastError());
        if (c->sum_on) {  // (row 0 of a run without burn-in may be the summary's pivot)
            const int rc = sum_start_state(c, row0);
            if (rc) return rc;
        }
    } else if (explicit_params(p.mode)) {
        hipLaunchKernelGGL(k_sb_theta_tables, dim3(p.KT), dim3(256), 0, c->stream, p, c->dNk, c->dS,
                           c->dPi, c->dTheta, 0, 0u, (double*)nullptr, c->dTab, (double*)nullptr, (double*)nullptr,
                           (const int*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    c->started = true;
    return BMM_OK;
}

int check_common(int64_t N, int P, int K, double beta, double gamma) {
    if (N < 1) return set_err(BMM_E_ARG, "N must be >= 1");
    if (P < 1) return set_err(BMM_E_ARG, "P must be >= 1");
    if (K < 1) return set_err(BMM_E_ARG, "K must be >= 1");
    if (!(beta > 0.0) || !(gamma > 0.0)) return set_err(BMM_E_ARG, "beta and gamma must be > 0");
    return BMM_OK;
}

}  // namespace

extern "C" {

const char* bmm_last_error(void) { return g_err; }
int bmm_spec_group_width(void) { return kGroupW; }
int bmm_spec_group_width_own(void) { return kGroupWm; }
// LDS bytes of a k_resample_pk workgroup at (sampler, K, P) with groups of W features; -1 where the shape has no
// resident kernel at all
int64_t bmm_spec_pk_image_bytes(int sampler, int K, int P, int W) {
    if (sampler < 0 || sampler > 3 || K < 1 || P < 1 || P > kMaxP || (W != kGroupW && W != kGroupWAlt)) return -1;
    const int kt = pick_kt(sampler == BMM_SAMPLER_DP ? K + 1 : K);
    if (kt < 0) return -1;
    return (int64_t)pk_image_bytes(geometry(sampler, P, K, kt, W));
}
int bmm_spec_group_width_for(int sampler, int K, int P) {
    if (sampler < 0 || sampler > 3 || K < 1 || P < 1) return -1;
    return group_width_rule(sampler, K, P);
}
int64_t bmm_default_batch(int sampler, int64_t N) { return default_batch(sampler, N); }

int bmm_set_progress(bmm_progress_fn fn, void* user, int every) {
    g_progress.fn = every > 0 ? fn : nullptr;
    g_progress.user = user;
    g_progress.every = fn && every > 0 ? every : 0;
    return BMM_OK;
}
int bmm_last_run_phases(double* ms) {
    if (!ms) return set_err(BMM_E_ARG, "null argument");
    for (int q = 0; q < BMM_RUN_PHASES; ++q) ms[q] = g_phase_ms[q];
    return BMM_OK;
}
int bmm_host_threads(void) { return host_threads(); }

// what the library keeps between calls -- up to eight 4 MiB pieces of pinned staging, and per device up to four
// idle streams of either kind and up to 512 MiB of device blocks -- released now (a long-lived host process that is done
// sampling)
int bmm_release_pools(void) {
    {
        StagePool& sp = stage_pool();
        std::vector<void*> idle;
        { std::lock_guard<std::mutex> g(sp.m); idle.swap(sp.idle); }
        for (void* p : idle) (void)hipHostFree(p);
    }
    StreamPool& st = stream_pool();
    DevPool& dp = dev_pool();
    for (int d = 0; d < 64; ++d) {
        std::vector<hipStream_t> idle, idle_q;
        std::vector<DevPool::Block> blocks;
        { std::lock_guard<std::mutex> g(st.m); idle.swap(st.idle[0][d]); idle_q.swap(st.idle[1][d]); }
        idle.insert(idle.end(), idle_q.begin(), idle_q.end());
        { std::lock_guard<std::mutex> g(dp.m); blocks.swap(dp.idle[d]); }
        if (idle.empty() && blocks.empty()) continue;
        if (hipSetDevice(d) != hipSuccess) { (void)hipGetLastError(); continue; }
        for (hipStream_t s : idle) (void)hipStreamDestroy(s);
        for (const DevPool::Block& b : blocks) (void)hipFree(b.p);
    }
    return BMM_OK;
}

int bmm_device_count(int* n) {
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; return set_err(BMM_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = k;
    return BMM_OK;
}

int bmm_chain_create(bmm_chain** out, int sampler, int64_t N, int P, int K, double alpha, double beta,
                     double gamma, double a, double b, int64_t batch, uint64_t seed, int device) {
    if (!out) return set_err(BMM_E_ARG, "out is null");
    *out = nullptr;
    if (sampler < 0 || sampler > 3) return set_err(BMM_E_ARG, "unknown sampler %d", sampler);
    int rc = check_common(N, P, K, beta, gamma);
    if (rc) return rc;
    if (sampler == BMM_SAMPLER_DP && beta != gamma)  // collapsed_gibbs_dp.cpp:48-50
        return set_err(BMM_E_ARG, "Error: sampler currently not implemented for non-symmetric priors on beta and gamma");
    if (sampler == BMM_SAMPLER_DP && K < 2) return set_err(BMM_E_ARG, "maxK must be >= 2");
    if (alpha < 0.0) return set_err(BMM_E_ARG, "alpha must be >= 0 (0 = sample it)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return set_err(BMM_E_NODEVICE, "no HIP device visible; this path has no CPU fallback");
    const int slot = device;
    if (const int fake = fake_devices()) {
        if (device < 0 || device >= fake) return set_err(BMM_E_ARG, "device %d out of range (have %d)", device, fake);
        device = device % ndev;
    }
    if (device < 0 || device >= ndev) return set_err(BMM_E_ARG, "device %d out of range (have %d)", device, ndev);

    bmm_chain* c = new (std::nothrow) bmm_chain();
    if (!c) return set_err(BMM_E_ARG, "out of host memory");
    const DebugSwitches dbg;
    const ChainShape shape = chain_shape(sampler, N, P, K, batch, dbg);
    ChainParams& p = c->p;
    p = shape.p;
    p.beta = beta; p.gamma = gamma; p.a = a; p.b = b; p.seed = seed;
    p.sample_alpha = alpha == 0.0;  // collapsed_gibbs.cpp:50-54
    c->alpha0 = p.sample_alpha ? 1.0 : alpha;
    c->device = device;
    c->slot = slot;
    c->batch = shape.batch;
    if (p.Kc > kMaxCatsAny) {
        delete c;
        return set_err(BMM_E_UNSUPPORTED, "%d categories exceed the %d this build supports", p.Kc, kMaxCatsAny);
    }
    const int cus = device_cus(device);
    if (cus <= 0) { delete c; return set_err(BMM_E_HIP, "hipGetDeviceProperties failed"); }
    c->bits = !dbg.int32_layout;
    c->pk_defer_every = dbg.pk_defer_every;
    c->pk_mid_fail_every = dbg.pk_mid_fail_every;
    c->generic = shape.generic;
    c->minus_in_lds = shape.minus_in_lds;
    c->lds_bytes_base = c->lds_bytes = shape.lds_bytes_base;
    if (c->generic) {
        c->form = KernelForm{p.KT, 256, tier_of(c), c->bits, 1, false, p.W, false};
        c->scratch_stride = generic_threads(p.Kc);
        c->grid_max = (int)(c->scratch_stride / 256);
    } else {
        c->num_cus = dbg.cus >= 1 ? dbg.cus : cus;
        rc = pick_kernel(c);
        if (rc) { delete c; return rc; }
    }
    rc = chain_alloc(c);
    if (rc) { bmm_chain_destroy(c); return rc; }
    *out = c;
    return BMM_OK;
}

void bmm_chain_destroy(bmm_chain* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
#ifdef BMM_DIAG
    if (c->dDiag) {
        unsigned long long d[22] = {};
        const bool ok = hipMemcpy(d, c->dDiag, sizeof d, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && d[5] && d[0]) {  // (k_resample_pk stamps the launch phases only)
            const double tot = (double)(d[0] + d[1] + d[2] + d[3] + d[4]);
            fprintf(stderr, "[bmm diag] waves=%llu cycles/wave: score %.0f (%.1f%%) pack %.0f (%.1f%%) draw %.0f (%.1f%%) movers %.0f (%.1f%%) prologue %.0f (%.1f%%) movers/wave-launch %.2f\n",
                    d[5], d[0] / (double)d[5], 100 * d[0] / tot, d[1] / (double)d[5], 100 * d[1] / tot, d[2] / (double)d[5],
                    100 * d[2] / tot, d[3] / (double)d[5], 100 * d[3] / tot, d[4] / (double)d[5], 100 * d[4] / tot, d[6] / (double)d[5]);
        }
        if (ok && d[5])
            fprintf(stderr, "[bmm diag launch] ticks per wave and launch: table staging %.0f, tile loop %.0f, waiting for the workgroup %.0f, flush %.0f\n",
                    d[8] / (double)d[5], d[9] / (double)d[5], d[10] / (double)d[5], d[11] / (double)d[5]);
        if (ok && d[7])  // k_resample_pk: wave 0 of each workgroup, slots of its own
            fprintf(stderr, "[bmm diag launch pk] workgroup-launches %llu, ticks from entry to flushed %.0f\n", d[7], d[14] / (double)d[7]);
        if (ok && d[7] && d[17])  // ... and wave 0's trips: between the first and the last lookup of a trip, and the rest of the loop
            fprintf(stderr, "[bmm diag trip pk] trips of wave 0: %llu, ticks per trip: scoring %.0f, outside it %.0f\n", d[17],
                    d[16] / (double)d[17], ((double)d[9] - (double)d[16]) / (double)d[17]);
        if (ok && d[7] && (d[19] || d[21]))  // ... and the lanes wave 0 settled: inside the middle tier, inside the definition
            fprintf(stderr, "[bmm diag settle pk] wave 0 per workgroup-launch: middle tier runs %.4f at %.0f ticks each, definition runs %.4f at %.0f ticks each, "
                    "together %.0f ticks of the tile loop's %.0f (%.2f%%)\n",
                    d[19] / (double)d[7], d[19] ? d[18] / (double)d[19] : 0.0, d[21] / (double)d[7], d[21] ? d[20] / (double)d[21] : 0.0,
                    (double)(d[18] + d[20]) / (double)d[7], d[9] / (double)d[5], 100.0 * (double)(d[18] + d[20]) / (double)d[9]);
#ifdef BMM_DEBUG_HOOKS
        if (ok && d[7] && c->dPkStat) {  // the test variant's counters of every wave, over the chain's life
            unsigned long long v[6] = {};
            if (hipMemcpy(v, c->dPkStat, sizeof v, hipMemcpyDeviceToHost) == hipSuccess && v[0])
                fprintf(stderr, "[bmm diag tiers pk] draws %llu deferred %llu (%.4f%%) middle tier tried %llu settled %llu definition runs %llu\n", v[0],
                        v[1], 100.0 * (double)v[1] / (double)v[0], v[3], v[4], v[5]);
        }
#endif
        if (ok && d[5] && d[12])
            fprintf(stderr, "[bmm diag draw] draws of a wave (64 observations) %llu, of them by the binary64 definition %llu (%.4f%%)\n",
                    d[12], d[13], 100.0 * (double)d[13] / (double)d[12]);
    }
#endif
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->planes && c->planes->refs.fetch_sub(1) == 1) {  // the last chain over these planes
        dev_pool().put(c->device, c->planes->d, c->planes->bytes);
        delete c->planes;
    }
    dev_pool().put(c->device, c->arena, c->arena_bytes);  // the stream is idle (synchronised above)
    dev_pool().put(c->device, c->run_arena, c->run_arena_bytes);
    sum_release(c);
    void* bufs[] = {c->dX_owned, c->dScratch, c->dProbs, c->dWts, c->dWtot, c->dXnb, c->dPredTab, c->dPredMax, c->dPredSum, c->dRespAcc,
                    c->dLooTab, c->dLooAcc, c->dLooOut, c->dLooScratch, c->dSmSide, c->dSmSideLaunch, c->dSmLq, c->dSmStat, c->dSmCell,
                    c->dSmCounters, c->dFsBlock, c->dEaBlock, c->dEaSide, c->dAsBlock, c->dLjBlock, c->dLjZ, c->dPcFeat, c->dPcXt, c->dPcBlock, c->dNaBlock, c->dCsBlock, c->dCatBlock,
                    c->dPnMb, c->dPnRow, c->dPnOff, c->dPnCol, c->dCellMax, c->dCellSum, c->dSplitTab, c->dPnScratch};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    chain_stream_release(c->device, c->stream, c->stream_kind);  // synchronised above
    delete c;
}

// `rows` observations of an int32 matrix (feature d of observation i at X[i + d * ldx]) into the
// chain's bit planes, starting at observation i0
static int pack_rows(bmm_chain* c, const int32_t* dX, int64_t rows, int64_t ldx, int64_t i0) {
    const int64_t nb = (rows + 255) / 256;
    hipLaunchKernelGGL(k_pack_bits, dim3((unsigned)(nb < 16384 ? nb : 16384)), dim3(256), 0, c->stream, dX, rows,
                       ldx, c->p.P, c->dXb + i0, c->p.N);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

int bmm_chain_set_x_layout(bmm_chain* c, int layout) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (layout != BMM_X_BITPLANES && layout != BMM_X_INT32) return set_err(BMM_E_ARG, "unknown X layout %d", layout);
    if (c->have_data || c->started) return set_err(BMM_E_STATE, "the X layout is chosen before the data are set");
    if (c->cat_on && layout == BMM_X_INT32) return set_err(BMM_E_UNSUPPORTED, "categorical features read the bit planes: not offered on the int32 layout");
    c->bits = c->form.bits = layout == BMM_X_BITPLANES;
    if (c->generic) return BMM_OK;  // one kernel for both layouts there
    return pick_kernel(c);
}

int bmm_chain_get_x_layout(const bmm_chain* c, int* layout) {
    if (!c || !layout) return set_err(BMM_E_ARG, "null argument");
    *layout = c->bits ? BMM_X_BITPLANES : BMM_X_INT32;
    return BMM_OK;
}

int bmm_chain_set_data_host(bmm_chain* c, const int32_t* X) {
    if (!c || !X) return set_err(BMM_E_ARG, "null argument");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    if (pc_data_locked(c)) return BMM_E_STATE;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t N = c->p.N;
    const int P = c->p.P;
    if (!c->bits) {  // the matrix itself is what the sweeps stream: one copy, kept
        const size_t bytes = (size_t)N * P * sizeof(int32_t);
        if (!c->dX_owned) HIP_TRY(hipMalloc(&c->dX_owned, bytes));
        HIP_TRY(hipMemcpyAsync(c->dX_owned, X, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->dX = c->dX_owned;
        int rc = validate_binary(c, c->dX, N * P);
        if (rc) return rc;
        c->have_data = true;
        return cat_data_changed(c);
    }
    // Bit planes from a host matrix: the host's own cores validate and pack it, slab by slab, into pinned
    // staging, and only the planes cross PCIe -- 4 * ceil(P/32) bytes per observation instead of 4 * P (8 MB
    // instead of 200 MB at N = 1e6, P = 50; a pageable 200 MB upload alone took 13.5 ms there, a third of
    // a 220-sweep run).  Slab s + 1 is packed while slab s is on its way.  Same planes, bit for bit, as
    // k_pack_bits makes from a matrix already on the device (tests/test_gpu_fullsize.py holds the two
    // hand-overs to the same chain).
    return guarded([&]() -> int {
        const int W = (P + 31) / 32;
        if (!c->dXb) { int rcp = planes_alloc(c, (size_t)W * N); if (rcp) return rcp; }
        int64_t slab = (int64_t)(kStageBytes / ((size_t)W * 4));  // one staging piece of packed words per slab
        slab = slab / 4096 * 4096;
        if (slab < 4096) slab = 4096;
        if (slab > N) slab = N;
        Stage pooled[2];
        PinnedBuf own[2];
        uint32_t* pin[2] = {pooled[0].as<uint32_t>(), pooled[1].as<uint32_t>()};
        if ((size_t)slab * W * 4 > kStageBytes || !pin[0] || !pin[1])  // more than 256 words per observation
            for (int q = 0; q < 2; ++q) { HIP_TRY(own[q].alloc((size_t)slab * W * 4)); pin[q] = own[q].as<uint32_t>(); }
        EventPair done;
        HIP_TRY(done.create());
        HostCrew crew;
        std::vector<uint32_t*> plane((size_t)W);
        int64_t s = 0;
        for (int64_t i0 = 0; i0 < N; i0 += slab, ++s) {
            const int64_t rows = N - i0 < slab ? N - i0 : slab;
            uint32_t* const buf = pin[s & 1];
            if (s >= 2) HIP_TRY(hipEventSynchronize(done.e[s & 1]));  // its previous copy has left the buffer
            std::atomic<uint32_t> seen{0};
            for (int w = 0; w < W; ++w) plane[(size_t)w] = buf + (int64_t)w * slab;
            crew.run(rows, 32768, 64, [&](int64_t lo, int64_t hi) {
                seen.fetch_or(pack_rows_host(X, N, P, i0 + lo, i0 + hi, plane.data(), i0), std::memory_order_relaxed);
            });
            if (seen.load() & ~1u) {
                (void)hipStreamSynchronize(c->stream);
                return set_err(BMM_E_ARG, "data must be binary: X holds a value other than 0 and 1");
            }
            HIP_TRY(hipMemcpy2DAsync(c->dXb + i0, (size_t)N * 4, buf, (size_t)slab * 4, (size_t)rows * 4, (size_t)W,
                                     hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipEventRecord(done.e[s & 1], c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffers go out of scope
        if (c->dX_owned) { (void)hipFree(c->dX_owned); c->dX_owned = nullptr; }
        c->dX = nullptr;
        c->have_data = true;
        return cat_data_changed(c);
    });
}

int bmm_chain_set_data_device(bmm_chain* c, const void* dX) {
    if (!c || !dX) return set_err(BMM_E_ARG, "null argument");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    if (pc_data_locked(c)) return BMM_E_STATE;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dX) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return set_err(BMM_E_ARG, "dX is not a device pointer");
    }
    if (at.device != c->device) return set_err(BMM_E_ARG, "dX lives on device %d, chain on %d", at.device, c->device);
    HIP_TRY(hipSetDevice(c->device));
    // The chain validates and packs on its own non-blocking stream, which nothing orders after the
    // stream that produced dX (a torch kernel, an RCCL broadcast still in flight): wait for the device.
    HIP_TRY(hipDeviceSynchronize());
    const int32_t* x = static_cast<const int32_t*>(dX);
    int rc = validate_binary(c, x, c->p.N * c->p.P);
    if (rc) return rc;
    if (c->bits) {  // packed here and now; the caller's matrix is not read again
        const int W = (c->p.P + 31) / 32;
        if (!c->dXb) { rc = planes_alloc(c, (size_t)W * c->p.N); if (rc) return rc; }
        rc = pack_rows(c, x, c->p.N, c->p.N, 0);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->dX = nullptr;
    } else {
        c->dX = x;  // borrowed for the life of the chain
    }
    c->have_data = true;
    return cat_data_changed(c);
}

// ---- bit planes shared between chains, or filled by the caller (a broadcast) ----------------
int bmm_chain_share_data(bmm_chain* c, bmm_chain* from) {
    if (!c || !from) return set_err(BMM_E_ARG, "null argument");
    if (c->started || c->have_data) return set_err(BMM_E_STATE, "the chain already has its data");
    if (!from->have_data || !from->bits || !from->dXb) return set_err(BMM_E_STATE, "the source chain holds no bit planes");
    if (from->na_on) return set_err(BMM_E_UNSUPPORTED, "the source chain redraws missing cells in its planes (bmm_chain_set_missing): they are its own");
    if (from->slot != c->slot) return set_err(BMM_E_ARG, "chains on different devices cannot share planes");
    if (from->p.N != c->p.N || from->p.P != c->p.P) return set_err(BMM_E_ARG, "the chains differ in N or P");
    if (!c->bits) return set_err(BMM_E_STATE, "the int32 layout streams the caller's matrix: hand it over instead");
    int rcq = chain_dedicated_queue(from);  // two chains on one device: a hardware queue each
    if (rcq == BMM_OK) rcq = chain_dedicated_queue(c);
    if (rcq) return rcq;
    for (bmm_chain* q : {from, c}) {  // and the kernel form that suits a shared device (pick_kernel)
        if (q->shares_device || q->started || q->generic) continue;
        q->shares_device = true;
        rcq = pick_kernel(q);
        if (rcq) return rcq;
    }
    c->planes = from->planes;
    c->planes->refs.fetch_add(1);
    c->dXb = from->dXb;
    c->xb_borrowed = true;
    c->dX = nullptr;
    c->have_data = true;
    return cat_data_changed(c);
}

int bmm_chain_planes(bmm_chain* c, void** dXb, int64_t* n_words) {
    if (!c || !dXb) return set_err(BMM_E_ARG, "null argument");
    if (!c->bits) return set_err(BMM_E_STATE, "the chain streams the int32 layout: it has no bit planes");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (int64_t)((c->p.P + 31) / 32) * c->p.N;
    if (!c->dXb) {
        if (c->started) return set_err(BMM_E_STATE, "chain already started");
        int rcp = planes_alloc(c, (size_t)words);
        if (rcp) return rcp;
    }
    *dXb = c->dXb;
    if (n_words) *n_words = words;
    return BMM_OK;
}

int bmm_chain_planes_filled(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    if (!c->bits || !c->dXb) return set_err(BMM_E_STATE, "no planes to declare filled (bmm_chain_planes first)");
    if (pc_data_locked(c)) return BMM_E_STATE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // whatever filled them ran on a stream of the caller's
    c->dX = nullptr;
    c->have_data = true;
    return cat_data_changed(c);
}

int bmm_chain_set_initial_labels(bmm_chain* c, const int32_t* z1) {
    if (!c || !z1) return set_err(BMM_E_ARG, "null argument");
    if (c->p.mode != MODE_COLLAPSED) return set_err(BMM_E_STATE, "only the finite collapsed sampler takes initial labels");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    // uploaded as R holds them (1-based), checked and shifted on the device: no host pass over N labels
    HIP_TRY(hipSetDevice(c->device));
    const int64_t N = c->p.N;
    DevBuf badbuf;
    HIP_TRY(badbuf.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(badbuf.p, 0xff, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemcpyAsync(c->dZ[1], z1, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const int64_t nb = (N + 255) / 256;
    hipLaunchKernelGGL(k_labels_from_r, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->dZ[1], N,
                       c->p.K, c->dZ[0], badbuf.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, badbuf.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad != ~0ull)
        return set_err(BMM_E_ARG, "initialK[%lld] = %d outside 1..%d", (long long)bad, z1[bad], c->p.K);
    c->have_init = true;
    return BMM_OK;
}

int bmm_chain_set_initial_params(bmm_chain* c, const double* pi, const double* theta) {
    if (!c || !pi || !theta) return set_err(BMM_E_ARG, "null argument");
    if (!explicit_params(c->p.mode)) return set_err(BMM_E_STATE, "only the stick-breaking and full samplers take initial pi/theta");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->dPi, pi, (size_t)c->p.K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->dTheta, theta, (size_t)c->p.K * c->p.P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_init = true;
    return BMM_OK;
}

int bmm_chain_sweeps(bmm_chain* c, int n) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        if (c->sharded && n > 0) return set_err(BMM_E_STATE, "a sharded chain advances by bmm_chain_shard_resample / _finish");
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started) {
            int rc = chain_start(c);
            if (rc) return rc;
        }
        for (int t = 0; t < n; ++t) {
            int rc = enqueue_sweep(c, c->sweep + 1);
            if (rc) return rc;
            c->sweep++;
        }
        return BMM_OK;
    });
}

int bmm_chain_set_shard(bmm_chain* c, int64_t N_total, int64_t first_row) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (c->started) return set_err(BMM_E_STATE, "chain already started");
    if (c->cs_on) return cs_refuses("a shard");
    if (c->cat_on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered on a sharded chain");
    if (!explicit_params(c->p.mode))
        return set_err(BMM_E_UNSUPPORTED, "only the stick-breaking and full samplers shard exactly over observations");
    if (c->sum_on) return set_err(BMM_E_UNSUPPORTED, "a chain with an armed summary does not shard: a shard holds a part of the rows");
    if (first_row < 0 || N_total < first_row + c->p.N) return set_err(BMM_E_ARG, "shard [first_row, first_row + N) lies outside N_total");
    c->p.Ntot = N_total;
    c->p.obs0 = first_row;
    c->sharded = true;
    return BMM_OK;
}

static int shard_resample(bmm_chain* c, bool wait) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (!explicit_params(c->p.mode)) return set_err(BMM_E_UNSUPPORTED, "not a shardable sampler");
    if (c->shard_open) return set_err(BMM_E_STATE, "previous sweep not finished (bmm_chain_shard_finish)");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->started) {
        int rc = chain_start(c);
        if (rc) return rc;
    }
    int rc = enqueue_sweep(c, c->sweep + 1, 1);
    if (rc) return rc;
    c->shard_open = true;
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));  // the deltas are complete: safe to reduce on any stream
    return BMM_OK;
}
int bmm_chain_shard_resample(bmm_chain* c) { return shard_resample(c, true); }
int bmm_chain_shard_resample_async(bmm_chain* c) { return shard_resample(c, false); }

int bmm_chain_stream(bmm_chain* c, void** stream) {
    if (!c || !stream) return set_err(BMM_E_ARG, "null argument");
    *stream = c->stream;
    return BMM_OK;
}

int bmm_chain_shard_deltas(bmm_chain* c, void** dNk, void** dS) {
    if (!c || !dNk || !dS) return set_err(BMM_E_ARG, "null argument");
    *dNk = c->dDNk;
    *dS = c->dDS;
    return BMM_OK;
}

int bmm_chain_shard_finish(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (!c->shard_open) return set_err(BMM_E_STATE, "no sweep open (bmm_chain_shard_resample)");
    HIP_TRY(hipSetDevice(c->device));
    int rc = enqueue_sweep(c, c->sweep + 1, 2);
    if (rc) return rc;
    c->sweep++;
    c->shard_open = false;
    return BMM_OK;
}

int bmm_chain_sweep_probs(bmm_chain* c, double* probs_out) {
    if (!c || !probs_out) return set_err(BMM_E_ARG, "null argument");
    if (c->sharded) return set_err(BMM_E_STATE, "not available on a sharded chain");
    if (c->alloc_on) return alloc_refuses("the probability hand-off of the relabelling");
    if (c->na_on) return na_refuses("the probability hand-off of the relabelling");
    if (c->cs_on) return cs_refuses("the probability hand-off of the relabelling");
    HIP_TRY(hipSetDevice(c->device));
    int rc = probs_alloc(c, true);
    if (rc) return rc;
    c->probs_dst = c->dProbs;
    rc = bmm_chain_sweeps(c, 1);
    c->probs_dst = nullptr;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(probs_out, c->dProbs, (size_t)c->p.N * c->p.K * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMM_OK;
}

int bmm_chain_sweeps_counts(bmm_chain* c, int n, int32_t* nk_out) {
    if (!c || !nk_out) return set_err(BMM_E_ARG, "null argument");
    if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
    if (n == 0) return BMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)n * c->p.K * sizeof(int32_t);
    HIP_TRY(hipMalloc(&c->dNkTrace, bytes));
    c->nk_trace_base = c->sweep + 1;
    int rc = bmm_chain_sweeps(c, n);
    if (rc == BMM_OK) {
        hipError_t e = hipMemcpyAsync(nk_out, c->dNkTrace, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = set_err(BMM_E_HIP, "copying the count trace failed: %s", hipGetErrorString(e));
    } else {
        (void)hipStreamSynchronize(c->stream);
    }
    (void)hipFree(c->dNkTrace);
    c->dNkTrace = nullptr;
    return rc;
}

int bmm_chain_sync(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        c->prof_ms += ms;
        c->prof_n++;
    }
    c->ev_used = 0;
    return dbg_labels_ok(c);
}

int bmm_chain_sweep_index(const bmm_chain* c) { return c ? c->sweep : -1; }

int bmm_chain_get_labels(bmm_chain* c, int32_t* z1) {
    if (!c || !z1) return set_err(BMM_E_ARG, "null argument");
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(z1, label_row(c, c->sweep), (size_t)c->p.N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < c->p.N; ++i) z1[i] = z1[i] < 0 ? BMM_NA_INTEGER : z1[i] + 1;
    return BMM_OK;
}

int bmm_chain_get_counts(bmm_chain* c, int32_t* Nk, int32_t* S) {
    return guarded([&]() -> int {
        if (!c || !Nk || !S) return set_err(BMM_E_ARG, "null argument");
        HIP_TRY(hipSetDevice(c->device));
        int rc = launch_reduce_deltas(c);
        if (rc) return rc;
        rc = bmm_chain_sync(c);
        if (rc) return rc;
        const size_t K = (size_t)c->p.K, KP = K * c->p.P;
        std::vector<int32_t> d(KP > K ? KP : K);
        HIP_TRY(hipMemcpy(Nk, c->dNk, K * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(d.data(), c->dDNk, K * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < K; ++k) Nk[k] += d[k];
        HIP_TRY(hipMemcpy(S, c->dS, KP * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(d.data(), c->dDS, KP * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < KP; ++q) S[q] += d[q];
        return BMM_OK;
    });
}

int bmm_chain_get_alpha(bmm_chain* c, double* alpha) {
    if (!c || !alpha) return set_err(BMM_E_ARG, "null argument");
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(alpha, c->dAlpha, sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}

int bmm_chain_get_params(bmm_chain* c, double* pi, double* theta) {
    if (!c || !pi || !theta) return set_err(BMM_E_ARG, "null argument");
    if (!explicit_params(c->p.mode)) return set_err(BMM_E_STATE, "only the stick-breaking and full samplers carry pi/theta");
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(pi, c->dPi, (size_t)c->p.K * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(theta, c->dTheta, (size_t)c->p.K * c->p.P * sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}

int bmm_chain_profile(bmm_chain* c, int enable) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    c->prof = enable > 0 ? enable : 0;
    c->prof_ms = 0.0;
    c->prof_n = 0;
    return BMM_OK;
}

int bmm_chain_profile_read(bmm_chain* c, double* resample_ms, int64_t* resample_launches) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = bmm_chain_sync(c);
    if (rc) return rc;
    if (resample_ms) *resample_ms = c->prof_ms;
    if (resample_launches) *resample_launches = c->prof_n;
    return BMM_OK;
}

int64_t bmm_chain_batch(const bmm_chain* c) { return c ? c->batch : -1; }

int bmm_chain_kernel_shape(const bmm_chain* c, int* lds_bytes, int* threads, int* grid_max) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (lds_bytes) *lds_bytes = (int)c->lds_bytes;
    if (threads) *threads = c->form.nt;
    if (grid_max) *grid_max = c->grid_max;
    return BMM_OK;
}

int bmm_chain_kernel_form(const bmm_chain* c, int* lanes_per_observation, int* builds_own_tables) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (lanes_per_observation) *lanes_per_observation = c->form.lanes;
    if (builds_own_tables) *builds_own_tables = c->form.self ? 1 : 0;
    return BMM_OK;
}

// ---- posterior predictive of new rows ----
static int pred_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "the predictive density is not offered on a sharded chain");
    if (c->fs_mask) return fs_mask_refuses("the predictive density");
    if (c->alloc_on) return alloc_refuses("the predictive density");
    if (c->cat_on) return cat_refuses("the predictive density");
    return BMM_OK;
}
static int pred_reset(bmm_chain* c) {
    c->pred_folded = 0;
    if (c->predM <= 0) return BMM_OK;
    const int64_t nb = (c->predM + 255) / 256;
    hipLaunchKernelGGL(k_predict_reset, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->predM,
                       c->dPredMax, c->dPredSum);
    HIP_TRY(hipGetLastError());
    if (c->dRespAcc) HIP_TRY(hipMemsetAsync(c->dRespAcc, 0, (size_t)c->predM * c->p.Kc * sizeof(double), c->stream));
    if (c->pred_cells > 0) {  // the cell pairs of incomplete new rows
        const int64_t cb = (c->pred_cells + 255) / 256;
        hipLaunchKernelGGL(k_predict_reset, dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, c->stream, c->pred_cells,
                           c->dCellMax, c->dCellSum);
        HIP_TRY(hipGetLastError());
    }
    return BMM_OK;
}
// the mask of incomplete new rows and everything sized by it (the stream is idle)
static void pred_na_drop(bmm_chain* c) {
    void** bufs[] = {reinterpret_cast<void**>(&c->dPnMb), reinterpret_cast<void**>(&c->dPnRow), reinterpret_cast<void**>(&c->dPnOff),
                     reinterpret_cast<void**>(&c->dPnCol), reinterpret_cast<void**>(&c->dCellMax), reinterpret_cast<void**>(&c->dCellSum),
                     reinterpret_cast<void**>(&c->dPnScratch)};
    for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
    c->pred_cells = 0;
    c->pn_scratch_stride = 0;
}
// n more sweeps folded through `slot` and, with `trace` (n x width, the caller's), recorded; without: enqueued, not waited for
static int sweeps_folded(bmm_chain* c, int n, SweepTrace& slot, int64_t width, double* trace, const char* what) {
    if (n == 0) return BMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    Recording rec;
    int rc = trace ? rec.alloc((size_t)n * (size_t)width * sizeof(double), what) : BMM_OK;
    if (rc) return rc;
    rec.begin(c, slot, (size_t)width * sizeof(double), c->sweep + 1, c->sweep + 1, true);
    rc = bmm_chain_sweeps(c, n);
    const hipError_t e = rec.end();
    if (rc || !trace) return rc;
    if (e != hipSuccess) return set_err(BMM_E_HIP, "the sweeps failed: %s", hipGetErrorString(e));
    return rows_out(rec.rows.as<double>(), n, width, trace, n, 0);
}
// the predictive kernel of the chain's shape, set up on first use
static int pred_setup(bmm_chain* c) {
    if (c->generic || c->pfn) return BMM_OK;
    score_fn f = lookup_score(c->p.KT, c->p.W, 0, false);
    if (!f) return set_err(BMM_E_STATE, "no predictive kernel for %d accumulators", c->p.KT);
    const size_t lds = (size_t)layout_of(c->p, false).head() * sizeof(double);
    if (lds > kLdsMax) return set_err(BMM_E_STATE, "the predictive table image (%zu bytes) does not fit in LDS", lds);
    int per_cu = 0;
    const hipError_t e = kernel_fits(f, kScoreThreads, lds, &per_cu);
    if (e != hipSuccess) return set_err(BMM_E_HIP, "kernel set-up failed: %s", hipGetErrorString(e));
    c->pfn = f;
    c->pred_lds = lds;
    c->pred_grid_max = (per_cu < 1 ? 1 : per_cu) * c->num_cus;
    return BMM_OK;
}

int bmm_chain_predict_responsibilities(bmm_chain* c, int on) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = pred_refused(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pred_resp = on != 0;
    if (c->dRespAcc && !c->pred_resp) { (void)hipFree(c->dRespAcc); c->dRespAcc = nullptr; }
    if (c->pred_resp && !c->dRespAcc && c->predM > 0) {
        const size_t bytes = (size_t)c->predM * c->p.Kc * sizeof(double);
        rc = pred_room(bytes, "the responsibilities (M x Kc doubles)");
        if (rc) { c->pred_resp = false; return rc; }
        HIP_TRY(hipMalloc(&c->dRespAcc, bytes));
    }
    return pred_reset(c);
}

int bmm_chain_set_newdata_host(bmm_chain* c, const int32_t* Xnew, int64_t M) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (M < 0) return set_err(BMM_E_ARG, "M must be >= 0");
        if (M > 0 && !Xnew) return set_err(BMM_E_ARG, "Xnew is null");
        int rc = pred_refused(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // nothing still reads the set that goes
        auto drop = [&]() {
            void** bufs[] = {reinterpret_cast<void**>(&c->dXnb), reinterpret_cast<void**>(&c->dPredMax),
                             reinterpret_cast<void**>(&c->dPredSum), reinterpret_cast<void**>(&c->dRespAcc)};
            for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
            pred_na_drop(c);  // the mask belongs to the set that goes
            c->predM = 0;
            c->pred_folded = 0;
        };
        if (M == 0) { drop(); return BMM_OK; }
        rc = pred_setup(c);
        if (rc) return rc;
        const int P = c->p.P, W = (P + 31) / 32, Kc = c->p.Kc;
        int64_t slab = ((int64_t)64 << 20) / ((int64_t)P * 4);  // rows per staged piece of the int32 matrix
        slab = slab / 4096 * 4096;
        if (slab < 4096) slab = 4096;
        if (slab > M) slab = M;
        const size_t resp_bytes = c->pred_resp ? (size_t)M * Kc * sizeof(double) : 0;
        rc = pred_room((size_t)W * M * 4 + (size_t)2 * M * 8 + resp_bytes + (size_t)slab * P * 4, "the new rows and their accumulators");
        if (rc) return rc;
        DevBuf planes, mx, sm, ra, stage;
        HIP_TRY(planes.alloc((size_t)W * M * sizeof(uint32_t)));
        HIP_TRY(mx.alloc((size_t)M * sizeof(double)));
        HIP_TRY(sm.alloc((size_t)M * sizeof(double)));
        if (resp_bytes) HIP_TRY(ra.alloc(resp_bytes));
        HIP_TRY(stage.alloc((size_t)slab * P * sizeof(int32_t)));
        if (!explicit_params(c->p.mode) && !c->dPredTab)
            HIP_TRY(hipMalloc(&c->dPredTab, (size_t)layout_of(c->p, false).head() * sizeof(double)));
        // validated and packed on the device, a slab of rows at a time (k_validate_binary, k_pack_bits)
        for (int64_t i0 = 0; i0 < M; i0 += slab) {
            const int64_t rows = M - i0 < slab ? M - i0 : slab;
            HIP_TRY(hipMemcpy2DAsync(stage.p, (size_t)rows * 4, Xnew + i0, (size_t)M * 4, (size_t)rows * 4, (size_t)P,
                                     hipMemcpyHostToDevice, c->stream));
            rc = validate_binary(c, stage.as<int32_t>(), rows * P);  // waits
            if (rc == BMM_E_ARG) return set_err(BMM_E_ARG, "newdata must be binary: Xnew holds a value other than 0 and 1");
            if (rc) return rc;
            const int64_t nb = (rows + 255) / 256;
            hipLaunchKernelGGL(k_pack_bits, dim3((unsigned)(nb < 16384 ? nb : 16384)), dim3(256), 0, c->stream,
                               stage.as<int32_t>(), rows, rows, P, planes.as<uint32_t>() + i0, M);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        drop();
        c->dXnb = planes.as<uint32_t>(); planes.p = nullptr;
        c->dPredMax = mx.as<double>(); mx.p = nullptr;
        c->dPredSum = sm.as<double>(); sm.p = nullptr;
        c->dRespAcc = ra.as<double>(); ra.p = nullptr;
        c->predM = M;
        return pred_reset(c);
    });
}

int bmm_chain_predict_state(bmm_chain* c, double* logdens_out, double* resp_out) {
    return guarded([&]() -> int {
        if (!c || !logdens_out) return set_err(BMM_E_ARG, "null argument");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started) { rc = chain_start(c); if (rc) return rc; }
        const size_t M = (size_t)c->predM, Kc = (size_t)c->p.Kc;
        DevBuf ld, rp;
        HIP_TRY(ld.alloc(M * sizeof(double)));
        if (resp_out) {
            rc = pred_room(M * Kc * sizeof(double), "the responsibilities (M x Kc doubles)");
            if (rc) return rc;
            HIP_TRY(rp.alloc(M * Kc * sizeof(double)));
        }
        rc = enqueue_predict(c, ld.as<double>(), resp_out ? rp.as<double>() : nullptr, false);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        hipError_t e = hipMemcpyAsync(logdens_out, ld.p, M * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && resp_out) e = hipMemcpyAsync(resp_out, rp.p, M * Kc * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);  // the scratch goes out of scope
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "copying the predictive failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_chain_sweeps_predict(bmm_chain* c, int n, double* logdens_trace) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        return sweeps_folded(c, n, c->pred_rec, c->predM, logdens_trace, "the log-density trace (n x M doubles)");
    });
}

int bmm_chain_get_predictive(bmm_chain* c, double* lppd, double* resp, int* n_folded) {
    return guarded([&]() -> int {
        if (!c || !lppd) return set_err(BMM_E_ARG, "null argument");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        if (resp && !c->pred_resp) return set_err(BMM_E_STATE, "the responsibilities were not accumulated (bmm_chain_predict_responsibilities)");
        if (n_folded) *n_folded = c->pred_folded;
        if (c->pred_folded < 1) return set_err(BMM_E_STATE, "no state has been folded yet (bmm_chain_sweeps_predict)");
        HIP_TRY(hipSetDevice(c->device));
        const size_t M = (size_t)c->predM, Kc = (size_t)c->p.Kc;
        DevBuf lp, rp;
        HIP_TRY(lp.alloc(M * sizeof(double)));
        if (resp) {
            rc = pred_room(M * Kc * sizeof(double), "the responsibilities (M x Kc doubles)");
            if (rc) return rc;
            HIP_TRY(rp.alloc(M * Kc * sizeof(double)));
        }
        const int64_t nb = ((int64_t)M + 255) / 256;
        hipLaunchKernelGGL(k_predict_finish, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->predM,
                           c->p.Kc, c->pred_folded, c->dPredMax, c->dPredSum, c->dRespAcc, lp.as<double>(),
                           resp ? rp.as<double>() : nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(lppd, lp.p, M * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && resp) e = hipMemcpyAsync(resp, rp.p, M * Kc * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "reading the predictive failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_chain_predict_reset(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    HIP_TRY(hipSetDevice(c->device));
    return pred_reset(c);
}

// ---- ... of incomplete new rows ----
static int na_check_cells(const int64_t* rows, const int32_t* cols, int64_t n, int64_t N, int P);
// the masked scorer of the chain's shape, set up on first use
static int pred_na_setup(bmm_chain* c) {
    const NaForm f = na_form_of(c->p, c->generic);
    if (!f.lds || c->pn_fn) return BMM_OK;
    na_score_fn fn = lookup_score_na(c->p.KT, c->p.W);
    if (!fn) return set_err(BMM_E_STATE, "no masked predictive kernel for %d accumulators", c->p.KT);
    int per_cu = 0;
    const hipError_t e = kernel_fits(fn, kScoreThreads, f.lds_bytes, &per_cu);
    if (e != hipSuccess) return set_err(BMM_E_HIP, "kernel set-up failed: %s", hipGetErrorString(e));
    c->pn_fn = fn;
    c->pn_lds = f.lds_bytes;
    c->pn_grid_max = (per_cu < 1 ? 1 : per_cu) * c->num_cus;
    return BMM_OK;
}

int bmm_chain_set_newdata_missing(bmm_chain* c, const int64_t* rows, const int32_t* cols, int64_t n) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        rc = na_check_cells(rows, cols, n, c->predM, c->p.P);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // nothing still reads the mask that goes
        if (n == 0) { pred_na_drop(c); return pred_reset(c); }
        rc = pred_na_setup(c);
        if (rc) return rc;
        const NaForm f = na_form_of(c->p, c->generic);
        const int64_t M = c->predM;
        const int W = (c->p.P + 31) / 32;
        int64_t stride = 0;
        if (!f.lds && !c->generic) {  // a resident shape in the global form: score columns of its own
            stride = (M + 255) / 256 * 256;
            if (stride > generic_threads(c->p.Kc)) stride = generic_threads(c->p.Kc);
        }
        const size_t plane_bytes = (size_t)W * M * sizeof(uint32_t), cell_bytes = (size_t)n * sizeof(double);
        const size_t scr_bytes = (size_t)stride * c->p.Kc * sizeof(double);
        rc = pred_room(plane_bytes + (size_t)(M + 1 + n) * 8 + (size_t)n * 4 + 2 * cell_bytes + scr_bytes + (c->dSplitTab ? 0 : f.table_bytes),
                       "the mask of the new rows, the cell list and the cell accumulators");
        if (rc) return rc;
        // the mask planes (bit d % 32 of word d / 32, as k_pack_bits lays the data out) and the CSR offsets, on the host
        std::vector<uint32_t> mb((size_t)W * M, 0u);
        std::vector<int64_t> off((size_t)M + 1, 0);
        for (int64_t q = 0; q < n; ++q) {
            mb[(size_t)(cols[q] >> 5) * M + rows[q]] |= 1u << (cols[q] & 31);
            off[(size_t)rows[q] + 1]++;
        }
        for (int64_t m = 0; m < M; ++m) off[(size_t)m + 1] += off[(size_t)m];
        DevBuf dmb, drw, dof, dcl, dmx, dsm, dsc;
        HIP_TRY(dmb.alloc(plane_bytes));
        HIP_TRY(drw.alloc((size_t)n * sizeof(int64_t)));
        HIP_TRY(dof.alloc((size_t)(M + 1) * sizeof(int64_t)));
        HIP_TRY(dcl.alloc((size_t)n * sizeof(int32_t)));
        HIP_TRY(dmx.alloc(cell_bytes));
        HIP_TRY(dsm.alloc(cell_bytes));
        if (scr_bytes) HIP_TRY(dsc.alloc(scr_bytes));
        if (!c->dSplitTab) HIP_TRY(hipMalloc(&c->dSplitTab, f.table_bytes));
        HIP_TRY(hipMemcpy(dmb.p, mb.data(), plane_bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(drw.p, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dof.p, off.data(), (size_t)(M + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dcl.p, cols, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        pred_na_drop(c);
        c->dPnMb = dmb.as<uint32_t>(); dmb.p = nullptr;
        c->dPnRow = drw.as<int64_t>(); drw.p = nullptr;
        c->dPnOff = dof.as<int64_t>(); dof.p = nullptr;
        c->dPnCol = dcl.as<int32_t>(); dcl.p = nullptr;
        c->dCellMax = dmx.as<double>(); dmx.p = nullptr;
        c->dCellSum = dsm.as<double>(); dsm.p = nullptr;
        c->dPnScratch = dsc.as<double>(); dsc.p = nullptr;
        c->pn_scratch_stride = stride;
        c->pred_cells = n;
        return pred_reset(c);
    });
}

int bmm_chain_predict_state_cells(bmm_chain* c, double* logdens_out, double* resp_out, double* cell_out) {
    return guarded([&]() -> int {
        if (!c || !logdens_out) return set_err(BMM_E_ARG, "null argument");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        if (cell_out && c->pred_cells <= 0) return set_err(BMM_E_STATE, "the new rows have no missing cell (bmm_chain_set_newdata_missing)");
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started) { rc = chain_start(c); if (rc) return rc; }
        const size_t M = (size_t)c->predM, Kc = (size_t)c->p.Kc, n = (size_t)c->pred_cells;
        DevBuf ld, rp, cl;
        HIP_TRY(ld.alloc(M * sizeof(double)));
        if (resp_out) {
            rc = pred_room(M * Kc * sizeof(double), "the responsibilities (M x Kc doubles)");
            if (rc) return rc;
            HIP_TRY(rp.alloc(M * Kc * sizeof(double)));
        }
        if (cell_out) HIP_TRY(cl.alloc(n * sizeof(double)));
        rc = enqueue_predict(c, ld.as<double>(), resp_out ? rp.as<double>() : nullptr, false, cell_out ? cl.as<double>() : nullptr);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        hipError_t e = hipMemcpyAsync(logdens_out, ld.p, M * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && resp_out) e = hipMemcpyAsync(resp_out, rp.p, M * Kc * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && cell_out) e = hipMemcpyAsync(cell_out, cl.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);  // the scratch goes out of scope
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "copying the predictive failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_chain_get_predictive_cells(bmm_chain* c, double* cell_mean, int* n_folded) {
    return guarded([&]() -> int {
        if (!c || !cell_mean) return set_err(BMM_E_ARG, "null argument");
        int rc = pred_refused(c);
        if (rc) return rc;
        if (c->predM <= 0) return set_err(BMM_E_STATE, "no new data set (bmm_chain_set_newdata_host)");
        if (c->pred_cells <= 0) return set_err(BMM_E_STATE, "the new rows have no missing cell (bmm_chain_set_newdata_missing)");
        if (n_folded) *n_folded = c->pred_folded;
        if (c->pred_folded < 1) return set_err(BMM_E_STATE, "no state has been folded yet (bmm_chain_sweeps_predict)");
        HIP_TRY(hipSetDevice(c->device));
        const size_t n = (size_t)c->pred_cells;
        DevBuf cm;
        HIP_TRY(cm.alloc(n * sizeof(double)));
        const int64_t nb = ((int64_t)n + 255) / 256;
        hipLaunchKernelGGL(k_predict_cells_finish, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->pred_cells,
                           c->dPnRow, c->dPredMax, c->dPredSum, c->dCellMax, c->dCellSum, cm.as<double>());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cell_mean, cm.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "reading the predictive failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_predict_na_plan(int sampler, int K, int P, bmm_predict_na_plan_out* out) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    if (sampler < 0 || sampler > 3 || K < 1 || P < 1) return set_err(BMM_E_ARG, "bmm_predict_na_plan: sampler in 0 .. 3, K >= 1, P >= 1");
    const DebugSwitches dbg;
    const ChainShape s = chain_shape(sampler, 1, P, K, 1, dbg);
    const NaForm f = na_form_of(s.p, s.generic);
    out->form = f.lds ? BMM_PREDICT_NA_LDS : BMM_PREDICT_NA_GLOBAL;
    out->threads = f.threads;
    out->lds_bytes = (int64_t)f.lds_bytes;
    out->table_bytes = (int64_t)f.table_bytes;
    return BMM_OK;
}

// ... of a run: every kept sweep is folded as it is enqueued (sweep_end_predict)
static int pred_run_check(const RunOptions& o, int P) {
    if (!o.pred) return BMM_OK;
    if (o.M < 0) return set_err(BMM_E_ARG, "M must be >= 0");
    if (o.M > 0 && !o.Xnew) return set_err(BMM_E_ARG, "Xnew is null");
    if (o.M > 0 && !o.pred->lppd) return set_err(BMM_E_ARG, "null buffer: lppd");
    if (o.pna.on && o.M > 0) return na_check_cells(o.pna.rows, o.pna.cols, o.pna.n, o.M, P);  // before a device is touched
    return BMM_OK;
}
static int pred_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.predict()) return BMM_OK;
    c->pred_resp = o.pred->resp != nullptr;
    int rc = bmm_chain_set_newdata_host(c, o.Xnew, o.M);
    if (rc == BMM_OK && o.pna.on && o.pna.n > 0) rc = bmm_chain_set_newdata_missing(c, o.pna.rows, o.pna.cols, o.pna.n);
    if (rc == BMM_OK && o.pred->logdens) rc = rec.alloc((size_t)c->S * (size_t)o.M * sizeof(double), "the log-density trace (S x M doubles)");
    if (rc) return rc;
    rec.begin(c, c->pred_rec, (size_t)o.M * sizeof(double), c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
static int pred_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.predict()) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    if (c->pred_folded < 1) {
        for (int64_t m = 0; m < o.M; ++m) o.pred->lppd[m] = std::nan("");
        if (o.pred->resp) for (int64_t q = 0; q < o.M * c->p.Kc; ++q) o.pred->resp[q] = std::nan("");
    } else {
        rc = bmm_chain_get_predictive(c, o.pred->lppd, o.pred->resp, nullptr);
    }
    if (rc == BMM_OK && o.pna.on && o.pna.n > 0) {
        if (c->pred_folded < 1) for (int64_t q = 0; q < o.pna.n; ++q) o.pna.mean[q] = std::nan("");
        else rc = bmm_chain_get_predictive_cells(c, o.pna.mean, nullptr);
    }
    if (rc == BMM_OK && o.pred->logdens) rc = run_rows_out(c, rec.rows.as<double>(), o.M, o.pred->logdens);
    return rc;
}

// ---- leave-one-out predictive of the fitted rows ----
static int loo_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "the leave-one-out predictive is not offered on a sharded chain");
    if (c->na_on) return na_refuses("the leave-one-out predictive");
    if (c->cs_on) return cs_refuses("the leave-one-out predictive");
    if (c->cat_on) return cat_refuses("the leave-one-out predictive");
    if (c->fs_mask) return fs_mask_refuses("the leave-one-out predictive");
    if (c->alloc_on) return alloc_refuses("the leave-one-out predictive");
    return BMM_OK;
}
static int loo_armed(const bmm_chain* c) {
    if (!c->loo_on) return set_err(BMM_E_STATE, "the leave-one-out summary is not armed (bmm_chain_set_loo)");
    return BMM_OK;
}
static int loo_reset(bmm_chain* c) {
    c->loo_folded = 0;
    const int64_t nb = (c->p.N + 255) / 256;
    hipLaunchKernelGGL(k_loo_reset, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->p.N, c->dLooAcc);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// the kernel of the chain's shape
static int loo_setup(bmm_chain* c) {
    if (c->generic || c->lfn || c->loo_generic) return BMM_OK;
    if (!c->bits)
        return set_err(BMM_E_UNSUPPORTED, "the leave-one-out predictive reads the bit planes: not offered on the int32 layout of a resident shape");
    const int minus = explicit_params(c->p.mode) ? 0 : (c->minus_in_lds ? 1 : 2);
    score_fn f = lookup_score(c->p.KT, c->p.W, minus, true);
    if (!f && minus != 0 && c->p.KT > kLooMaxOwnKT) {  // more accumulators than the own-label form has registers for
        int64_t stride = (c->p.N + 255) / 256 * 256;
        if (stride > generic_threads(c->p.Kc)) stride = generic_threads(c->p.Kc);
        const size_t bytes = (size_t)stride * c->p.Kc * sizeof(double);
        int rc = pred_room(bytes, "the leave-one-out score columns");
        if (rc) return rc;
        HIP_TRY(hipMalloc(&c->dLooScratch, bytes));
        c->loo_scratch_stride = stride;
        c->loo_generic = true;
        return BMM_OK;
    }
    if (!f) return set_err(BMM_E_STATE, "no leave-one-out kernel for %d accumulators", c->p.KT);
    const TableLayout l = layout_of(c->p, minus != 0);
    const size_t lds = (size_t)(minus == 1 ? l.doubles() : l.head()) * sizeof(double);
    if (lds > kLdsMax) return set_err(BMM_E_STATE, "the leave-one-out table image (%zu bytes) does not fit in LDS", lds);
    int per_cu = 0;
    const hipError_t e = kernel_fits(f, kScoreThreads, lds, &per_cu);
    if (e != hipSuccess) return set_err(BMM_E_HIP, "kernel set-up failed: %s", hipGetErrorString(e));
    c->lfn = f;
    c->loo_minus = minus;
    c->loo_lds = lds;
    c->loo_grid_max = (per_cu < 1 ? 1 : per_cu) * c->num_cus;
    return BMM_OK;
}
// a state every row of which is seated: the finite collapsed sampler from its initial labels on, the others after
// their first sweep
static int loo_seated(const bmm_chain* c) {
    if (c->p.mode != MODE_COLLAPSED && c->sweep < 1)
        return set_err(BMM_E_STATE, "no row has a label before the first sweep: there is no leave-one-out predictive of this state");
    return BMM_OK;
}

int bmm_chain_set_loo(bmm_chain* c, int on) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = loo_refused(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // nothing still reads what goes
        if (!on) {
            void** bufs[] = {reinterpret_cast<void**>(&c->dLooTab), reinterpret_cast<void**>(&c->dLooAcc),
                             reinterpret_cast<void**>(&c->dLooOut), reinterpret_cast<void**>(&c->dLooScratch)};
            for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
            c->loo_generic = false;
            c->loo_on = false;
            c->loo_folded = 0;
            return BMM_OK;
        }
        if (c->loo_on) return loo_reset(c);
        if (!c->have_data) return set_err(BMM_E_STATE, "data matrix not set");
        rc = loo_setup(c);
        if (rc) return rc;
        const size_t N = (size_t)c->p.N;
        const bool counting = !explicit_params(c->p.mode);
        const size_t tab_bytes = counting ? (size_t)layout_of(c->p, true).doubles() * sizeof(double) : 0;
        const size_t acc_bytes = N * kLooAcc * sizeof(double), out_bytes = (N * kLooOut + 8) * sizeof(double);
        rc = pred_room(tab_bytes + acc_bytes + out_bytes, "the leave-one-out accumulators (12 doubles per fitted row)");
        if (rc) return rc;
        DevBuf tab, acc, out;
        if (counting) {
            HIP_TRY(tab.alloc(tab_bytes));
            HIP_TRY(hipMemsetAsync(tab.p, 0, tab_bytes, c->stream));  // (the padding groups of the minus-self tables)
        }
        HIP_TRY(acc.alloc(acc_bytes));
        HIP_TRY(out.alloc(out_bytes));
        c->dLooTab = tab.as<double>(); tab.p = nullptr;
        c->dLooAcc = acc.as<double>(); acc.p = nullptr;
        c->dLooOut = out.as<double>(); out.p = nullptr;
        c->loo_on = true;
        return loo_reset(c);
    });
}

int bmm_chain_loo_state(bmm_chain* c, double* ell_out) {
    return guarded([&]() -> int {
        if (!c || !ell_out) return set_err(BMM_E_ARG, "null argument");
        int rc = loo_refused(c);
        if (rc == BMM_OK) rc = loo_armed(c);
        if (rc == BMM_OK) rc = loo_seated(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started) { rc = chain_start(c); if (rc) return rc; }
        const size_t N = (size_t)c->p.N;
        DevBuf el;
        HIP_TRY(el.alloc(N * sizeof(double)));
        rc = enqueue_loo(c, c->sweep, el.as<double>(), false);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        const hipError_t e = hipMemcpyAsync(ell_out, el.p, N * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);  // the scratch goes out of scope
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "copying the leave-one-out predictive failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_chain_sweeps_loo(bmm_chain* c, int n, double* ell_trace) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = loo_refused(c);
        if (rc == BMM_OK) rc = loo_armed(c);
        if (rc) return rc;
        return sweeps_folded(c, n, c->loo_rec, c->p.N, ell_trace, "the leave-one-out trace (n x N doubles)");
    });
}

int bmm_chain_get_loo(bmm_chain* c, const bmm_loo_out* o) {
    return guarded([&]() -> int {
        if (!c || !o) return set_err(BMM_E_ARG, "null argument");
        int rc = loo_refused(c);
        if (rc == BMM_OK) rc = loo_armed(c);
        if (rc) return rc;
        if (o->n_folded) *o->n_folded = c->loo_folded;
        if (c->loo_folded < 1) return set_err(BMM_E_STATE, "no state has been folded yet (bmm_chain_sweeps_loo)");
        HIP_TRY(hipSetDevice(c->device));
        const int64_t N = c->p.N;
        const int64_t nb = (N + 255) / 256;
        double* const scal = c->dLooOut + (size_t)N * kLooOut;
        hipLaunchKernelGGL(k_loo_finish, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, N, c->loo_folded,
                           c->dLooAcc, c->dLooOut);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_loo_reduce, dim3(1), dim3(1024), 0, c->stream, N, c->dLooOut, scal);
            e = hipGetLastError();
        }
        double* const rows[kLooOut] = {o->log_cpo, o->ess, o->lppd, o->mean, o->var};
        for (int q = 0; q < kLooOut && e == hipSuccess; ++q)
            if (rows[q]) e = hipMemcpyAsync(rows[q], c->dLooOut + (size_t)q * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        double sc[5] = {0, 0, 0, 0, 0};
        if (e == hipSuccess) e = hipMemcpyAsync(sc, scal, sizeof sc, hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "reading the leave-one-out summary failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        const bool waic = explicit_params(c->p.mode);  // ell is a log likelihood for the explicit samplers only
        if (o->lpml) *o->lpml = sc[0];
        if (o->min_ess) *o->min_ess = sc[1];
        if (o->p_waic) *o->p_waic = waic ? sc[3] : std::nan("");
        if (o->elpd_waic) *o->elpd_waic = waic ? sc[4] : std::nan("");
        return BMM_OK;
    });
}

int bmm_chain_loo_reset(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = loo_armed(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return loo_reset(c);
}

// ... of a run: armed for it, every kept sweep folded as it is enqueued (sweep_end_folds)
static int loo_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.loo.on) return BMM_OK;
    int rc = bmm_chain_set_loo(c, 1);
    if (rc == BMM_OK && o.loo.o.ell) rc = rec.alloc((size_t)c->S * (size_t)c->p.N * sizeof(double), "the leave-one-out trace (S x N doubles)");
    if (rc) return rc;
    rec.begin(c, c->loo_rec, (size_t)c->p.N * sizeof(double), c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
// the outputs of a run that had the summary armed: S kept rows, the first `burnin ? 0 : 1` of them not folded
static int loo_run_out(bmm_chain* c, const bmm_loo_out& o, const double* dtrace) {
    const int64_t N = c->p.N;
    const double nan = std::nan("");
    int rc = BMM_OK;
    if (c->loo_folded < 1) {
        double* const rows[kLooOut] = {o.log_cpo, o.ess, o.lppd, o.mean, o.var};
        for (double* r : rows) if (r) for (int64_t i = 0; i < N; ++i) r[i] = nan;
        double* const sc[4] = {o.lpml, o.min_ess, o.p_waic, o.elpd_waic};
        for (double* v : sc) if (v) *v = nan;
        if (o.n_folded) *o.n_folded = 0;
    } else {
        rc = bmm_chain_get_loo(c, &o);
    }
    if (rc == BMM_OK && o.ell) rc = run_rows_out(c, dtrace, N, o.ell);
    return rc;
}
static int loo_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.loo.on) return rc;
    rc = rec.end_run(rc);
    return rc == BMM_OK ? loo_run_out(c, o.loo.o, rec.rows.as<double>()) : rc;
}

// ---- log joint trace and keep-best allocation ----
static int lp_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "the log joint is not offered on a sharded chain: a shard holds a part of the counts");
    if (c->cat_on) return cat_refuses("the log joint");
    return BMM_OK;
}
static int lp_armed(const bmm_chain* c) {
    if (!c->lp_on) return set_err(BMM_E_STATE, "the log joint trace is not armed (bmm_chain_set_logpost)");
    return BMM_OK;
}
// a state every row of which is seated, as the leave-one-out summary asks
static int lp_seated(const bmm_chain* c) {
    if (c->p.mode != MODE_COLLAPSED && c->sweep < 1)
        return set_err(BMM_E_STATE, "no row has a label before the first sweep: this state has no log joint");
    return BMM_OK;
}
static int lp_reset(bmm_chain* c) {
    c->lp_folded = 0;
    const LjBest empty{-std::numeric_limits<double>::infinity(), -1, 0};
    HIP_TRY(hipMemcpyAsync(c->dLjBest, &empty, sizeof empty, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // `empty` goes out of scope
    return BMM_OK;
}
// the block behind the scoring launches (any chain may be scored) and, for a chain that keeps its best state, the labels
static int lp_setup(bmm_chain* c, bool keep) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dLjBlock) {
        const size_t K = (size_t)c->p.K;
        auto carve = [&](Carver& v) {
            c->dLjLik = v.take<double>(K + 1);
            c->dLjPrior = v.take<double>(K);
            c->dLjOut = v.take<double>(4);
            c->dLjBest = v.take<LjBest>(1);
        };
        Carver measure{nullptr};
        carve(measure);
        HIP_TRY(hipMalloc(&c->dLjBlock, measure.used));
        Carver real{c->dLjBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dLjBlock, 0, measure.used, c->stream));
        const int rc = lp_reset(c);
        if (rc) return rc;
    }
    if (keep && !c->dLjZ) {
        const int rc = pred_room((size_t)c->p.N * sizeof(int32_t), "the labels of the best state (N int32)");
        if (rc) return rc;
        HIP_TRY(hipMalloc(&c->dLjZ, (size_t)c->p.N * sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(c->dLjZ, 0xff, (size_t)c->p.N * sizeof(int32_t), c->stream));  // -1: no state yet
    }
    return BMM_OK;
}

int bmm_chain_set_logpost(bmm_chain* c, int on) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = lp_refused(c);
        if (rc) return rc;
        if (!on) { c->lp_on = false; return BMM_OK; }  // the best state stays readable
        rc = lp_setup(c, true);
        if (rc) return rc;
        if (c->lp_on) return lp_reset(c);
        c->lp_on = true;
        return lp_reset(c);
    });
}

int bmm_chain_logpost_state(bmm_chain* c, double out[4]) {
    return guarded([&]() -> int {
        if (!c || !out) return set_err(BMM_E_ARG, "null argument");
        int rc = lp_refused(c);
        if (rc == BMM_OK) rc = lp_seated(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started) { rc = chain_start(c); if (rc) return rc; }
        rc = lp_setup(c, false);
        if (rc == BMM_OK) rc = enqueue_log_joint(c, c->sweep, nullptr, false);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        const hipError_t e = hipMemcpyAsync(out, c->dLjOut, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "copying the log joint failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return BMM_OK;
    });
}

int bmm_chain_sweeps_logpost(bmm_chain* c, int n, double* trace) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = lp_refused(c);
        if (rc == BMM_OK) rc = lp_armed(c);
        if (rc) return rc;
        return sweeps_folded(c, n, c->lp_rec, 4, trace, "the log joint trace (n x 4 doubles)");
    });
}

int bmm_chain_get_best(bmm_chain* c, int32_t* z1, double* total, int* sweep) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->dLjZ) return set_err(BMM_E_STATE, "the log joint trace was never armed on this chain (bmm_chain_set_logpost)");
        if (c->lp_folded < 1) return set_err(BMM_E_STATE, "no state has been folded yet (bmm_chain_sweeps_logpost)");
        HIP_TRY(hipSetDevice(c->device));
        LjBest h{};
        hipError_t e = hipMemcpyAsync(&h, c->dLjBest, sizeof h, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && z1) e = hipMemcpyAsync(z1, c->dLjZ, (size_t)c->p.N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "reading the best state failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        if (z1) for (int64_t i = 0; i < c->p.N; ++i) z1[i] = z1[i] < 0 ? BMM_NA_INTEGER : z1[i] + 1;
        if (total) *total = h.sweep < 0 ? std::nan("") : h.total;
        if (sweep) *sweep = h.sweep;
        return BMM_OK;
    });
}

int bmm_chain_logpost_reset(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = lp_armed(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return lp_reset(c);
}

// ... of a run: armed for it, every kept sweep folded as it is enqueued (sweep_end_folds)
static int lp_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.logpost.on) return BMM_OK;
    int rc = bmm_chain_set_logpost(c, 1);
    if (rc == BMM_OK && o.logpost.o.rows) rc = rec.alloc((size_t)c->S * 4 * sizeof(double), "the log joint trace (S x 4 doubles)");
    if (rc) return rc;
    rec.begin(c, c->lp_rec, 4 * sizeof(double), c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
static int lp_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.logpost.on) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    const bmm_logpost_out& out = o.logpost.o;
    if (c->lp_folded < 1) {  // a run of one kept row without burn-in: the starting state alone
        if (out.z_best) for (int64_t i = 0; i < c->p.N; ++i) out.z_best[i] = BMM_NA_INTEGER;
        if (out.best_total) *out.best_total = std::nan("");
        if (out.best_row) *out.best_row = -1;
    } else {
        int sweep = -1;
        rc = bmm_chain_get_best(c, out.z_best, out.best_total, &sweep);
        if (rc) return rc;
        if (out.best_row) *out.best_row = sweep < 0 ? -1 : sweep - c->burnin;
    }
    return out.rows ? run_rows_out(c, rec.rows.as<double>(), 4, out.rows) : BMM_OK;
}

// The log joint of any stack of label rows over the same data, on a transient chain: X packed once, then per state the
// labels uploaded, the statistics recounted (k_count_labels_generic) and the state scored by the launches of a chain.
static int lj_check_labels(const int32_t* z, int S, int64_t N, int K, const int32_t* k_open) {
    for (int s = 0; s < S; ++s) {
        const int top = k_open ? k_open[s] : K;
        if (top < 1 || top > K) return set_err(BMM_E_ARG, "k_open[%d] = %d lies outside 1..%d", s, top, K);
        for (int64_t i = 0; i < N; ++i) {
            const int32_t v = z[(size_t)s + (size_t)i * (size_t)S];
            if (v < 1 || v > top)
                return set_err(BMM_E_ARG, "z[%d, %lld] = %d is not a label in 1..%d (row %d, observation %lld, both 0-based)", s, (long long)i, (int)v, top, s, (long long)i);
        }
    }
    return BMM_OK;
}
int bmm_device_log_joint(int device, const int32_t* X, int64_t N, int P, int sampler, int K, double beta, double gamma,
                         int sample_alpha, double a, double b, const double* log_prior_k, const int32_t* z, int S,
                         const double* alpha, const int32_t* k_open, const uint8_t* mask, double rho, double* out) {
    return guarded([&]() -> int {
        if (!X || !z || !alpha || !out) return set_err(BMM_E_ARG, "null argument");
        if (S < 1) return set_err(BMM_E_ARG, "S must be >= 1");
        if (sampler < 0 || sampler > 3) return set_err(BMM_E_ARG, "unknown sampler %d", sampler);
        if ((log_prior_k != nullptr) != (k_open != nullptr)) return set_err(BMM_E_ARG, "log_prior_k and k_open go together (the allocation sampler)");
        if (log_prior_k && sampler != BMM_SAMPLER_COLLAPSED) return set_err(BMM_E_ARG, "the allocation sampler is the finite collapsed sampler with K unknown");
        if (mask && explicit_params(sampler)) return set_err(BMM_E_UNSUPPORTED, "a feature mask is offered for the collapsed and DP samplers only");
        if (mask && !(rho > 0.0 && rho < 1.0)) return set_err(BMM_E_ARG, "rho must lie strictly inside (0, 1)");
        int rc = check_common(N, P, K, beta, gamma);
        if (rc) return rc;
        for (int s = 0; s < S; ++s)
            if (!(alpha[s] > 0.0) || !(alpha[s] < 1e300)) return set_err(BMM_E_ARG, "alpha[%d] must be > 0 and finite", s);
        rc = lj_check_labels(z, S, N, K, k_open);
        if (rc) return rc;
        bmm_chain* c = nullptr;
        rc = bmm_chain_create(&c, sampler, N, P, K, 1.0, beta, gamma, a, b, 0, 0, device);
        if (rc) return rc;
        struct Guard { bmm_chain* c; ~Guard() { bmm_chain_destroy(c); } } guard{c};
        c->p.sample_alpha = sample_alpha != 0;
        rc = bmm_chain_set_data_host(c, X);
        if (rc == BMM_OK) rc = lp_setup(c, false);
        if (rc) return rc;
        const size_t Kz = (size_t)K, KP = Kz * (size_t)P, W = ((size_t)P + 31) / 32;
        DevBuf dmask, dk, dlp;
        LjArgs args = lj_args(c);
        if (mask) {
            std::vector<uint32_t> words(W, 0u);
            for (int d = 0; d < P; ++d) {
                if (mask[d] > 1) return set_err(BMM_E_ARG, "mask[%d] = %d is neither 0 nor 1", d, (int)mask[d]);
                words[(size_t)d >> 5] |= (uint32_t)mask[d] << (d & 31);
            }
            HIP_TRY(dmask.alloc(W * sizeof(uint32_t)));
            HIP_TRY(hipMemcpy(dmask.p, words.data(), W * sizeof(uint32_t), hipMemcpyHostToDevice));
            args.mask = dmask.as<uint32_t>();
            args.rho = rho;
        }
        if (log_prior_k) {
            HIP_TRY(dk.alloc(sizeof(int32_t)));
            HIP_TRY(dlp.alloc(Kz * sizeof(double)));
            HIP_TRY(hipMemcpy(dlp.p, log_prior_k, Kz * sizeof(double), hipMemcpyHostToDevice));
            args.k_open = dk.as<int32_t>();
            args.log_prior_k = dlp.as<double>();
            args.kind = LJ_ALLOC;
        }
        HIP_TRY(hipMemsetAsync(c->dDNk, 0, Kz * kDeltaReps * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->dDS, 0, KP * kDeltaReps * sizeof(int32_t), c->stream));
        std::vector<int32_t> row((size_t)N);
        const int64_t nb = (N + 255) / 256;
        for (int s = 0; s < S; ++s) {
            for (int64_t i = 0; i < N; ++i) row[(size_t)i] = z[(size_t)s + (size_t)i * (size_t)S] - 1;
            HIP_TRY(hipMemcpyAsync(c->dZ[0], row.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->dAlpha, alpha + s, sizeof(double), hipMemcpyHostToDevice, c->stream));
            if (k_open) HIP_TRY(hipMemcpyAsync(dk.p, k_open + s, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(c->dNk, 0, Kz * sizeof(int32_t), c->stream));
            HIP_TRY(hipMemsetAsync(c->dS, 0, KP * sizeof(int32_t), c->stream));
            hipLaunchKernelGGL(k_count_labels_generic, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, c->stream, c->p, c->dX, c->dXb,
                               (const int32_t*)c->dZ[0], c->dNk, c->dS);
            HIP_TRY(hipGetLastError());
            rc = launch_log_joint(c, args);
            if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
            double h[4];
            const hipError_t e = hipMemcpyAsync(h, c->dLjOut, sizeof h, hipMemcpyDeviceToHost, c->stream);
            const hipError_t e2 = hipStreamSynchronize(c->stream);  // `row` is written again
            if (e != hipSuccess || e2 != hipSuccess) return set_err(BMM_E_HIP, "scoring state %d failed: %s", s, hipGetErrorString(e != hipSuccess ? e : e2));
            for (int q = 0; q < 4; ++q) out[(size_t)s + (size_t)q * (size_t)S] = h[q];
        }
        return BMM_OK;
    });
}

// ---- pairwise local-dependence check ----
static int pc_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "the pair check is not offered on a sharded chain: a shard holds a part of the rows");
    if (c->na_on) return na_refuses("the pair check (its column slices are cut once)");
    if (c->cat_on) return cat_refuses("the pair check");
    if (c->fs_mask)
        return set_err(BMM_E_UNSUPPORTED, "the pair check is written for the model in which every feature clusters: not offered on a "
                       "chain with a feature mask (the pooled model's reference distribution is another one)");
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "the pair check reads the bit planes of X: not offered on a chain on the int32 layout");
    return BMM_OK;
}
static int pc_armed(const bmm_chain* c) {
    if (!c->pc_on) return set_err(BMM_E_STATE, "the pair check is not armed (bmm_chain_set_pair_check)");
    return BMM_OK;
}
static int pc_seated(const bmm_chain* c) {
    if (c->p.mode != MODE_COLLAPSED && c->sweep < 1)
        return set_err(BMM_E_STATE, "no row has a label before the first sweep: this state has unseated rows and no pair check");
    return BMM_OK;
}
// M, the features and the stride, before a device is touched
static int pc_check_args(const int32_t* feat, int M, int stride, int P, int Kc) {
    if (M < 2 || M > kPcMaxM) return set_err(BMM_E_ARG, "the pair check takes 2 to %d features, not %d", kPcMaxM, M);
    if (!feat) return set_err(BMM_E_ARG, "null feature list");
    if (stride < 1) return set_err(BMM_E_ARG, "stride must be >= 1");
    for (int m = 0; m < M; ++m) {
        if (feat[m] < 0 || feat[m] >= P) return set_err(BMM_E_ARG, "feat[%d] = %d is not a feature in 0..%d", m, (int)feat[m], P - 1);
        for (int l = 0; l < m; ++l)
            if (feat[l] == feat[m]) return set_err(BMM_E_ARG, "feat[%d] and feat[%d] are both feature %d: the chosen features must be distinct", l, m, (int)feat[m]);
    }
    if (Kc > kPcKA * 65535)  // label blocks ride on grid.z
        return set_err(BMM_E_ARG, "the pair check is offered up to %d labels, not %d", kPcKA * 65535, Kc);
    const size_t bytes = (size_t)Kc * (size_t)pc_npairs(M) * sizeof(uint32_t);
    if (bytes > (size_t)BMM_PAIR_CHECK_MAX_COUNT_BYTES)
        return set_err(BMM_E_ARG, "the counts of %d labels and %d features take %zu bytes, above the cap of %u: choose fewer features", Kc, M,
                       bytes, (unsigned)BMM_PAIR_CHECK_MAX_COUNT_BYTES);
    return BMM_OK;
}
static void pc_free(bmm_chain* c) {
    void* bufs[] = {c->dPcFeat, c->dPcXt, c->dPcBlock};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    c->dPcFeat = nullptr; c->dPcXt = nullptr; c->dPcBlock = nullptr;
    c->pc_on = false; c->pc_M = 0; c->pc_folded = 0;
}
static int pc_reset(bmm_chain* c) {
    c->pc_folded = 0;
    HIP_TRY(hipMemsetAsync(c->dPcBlock + c->pc_count_bytes, 0, c->pc_fold_bytes, c->stream));
    return BMM_OK;
}

int bmm_chain_set_pair_check(bmm_chain* c, const int32_t* feat, int M, int stride) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        HIP_TRY(hipSetDevice(c->device));
        if (!feat || M == 0) {  // disarm: the memory goes
            HIP_TRY(hipStreamSynchronize(c->stream));
            pc_free(c);
            return BMM_OK;
        }
        int rc = pc_refused(c);
        if (rc == BMM_OK) rc = pc_check_args(feat, M, stride, c->p.P, c->p.K);
        if (rc) return rc;
        if (!c->have_data || !c->dXb) return set_err(BMM_E_STATE, "data matrix not set");
        HIP_TRY(hipStreamSynchronize(c->stream));
        pc_free(c);
        const PcPlan q = pc_plan(c->p.N, c->p.K, M);
        rc = pred_room(q.bytes_slices + q.bytes_counts + 2 * q.bytes_fold, "the pair check (the column slices, M N / 8 bytes, the counts and the fold)");
        if (rc) return rc;
        const size_t np = (size_t)q.npairs, Kz = (size_t)c->p.K;
        auto carve = [&](Carver& v) {
            c->dPcCnt = v.take<uint32_t>(Kz * np);
            c->dPcMarg = v.take<uint32_t>(Kz * (size_t)M);
            c->dPcNk = v.take<uint32_t>(Kz);
            c->pc_count_bytes = v.used;  // what a state's launch zeroes: the three above
            c->dPcSumZ = v.take<double>(np);
            c->dPcSumZ2 = v.take<double>(np);
            c->dPcSumX2 = v.take<double>(np);
            c->dPcSumDf = v.take<long long>(np);
            c->dPcNz = v.take<int32_t>(np);
            c->dPcN11 = v.take<uint32_t>(np);
            c->pc_fold_bytes = v.used - c->pc_count_bytes;  // what a reset zeroes
            c->dPcZ = v.take<double>(np);
            c->dPcX2 = v.take<double>(np);
            c->dPcDf = v.take<int32_t>(np);
        };
        Carver measure{nullptr};
        carve(measure);
        HIP_TRY(hipMalloc(&c->dPcBlock, measure.used));
        Carver real{c->dPcBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dPcBlock, 0, measure.used, c->stream));
        HIP_TRY(hipMalloc(&c->dPcFeat, (size_t)M * sizeof(int32_t)));
        HIP_TRY(hipMalloc(&c->dPcXt, q.bytes_slices));
        HIP_TRY(hipMemcpyAsync(c->dPcFeat, feat, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        const int64_t nb = (q.C + 3) / 4;
        hipLaunchKernelGGL(k_pc_slices, dim3((unsigned)(nb < 1024 ? nb : 1024), (unsigned)M), dim3(256), 0, c->stream,
                           (const uint32_t*)c->dXb, c->p.N, (const int32_t*)c->dPcFeat, q.C, c->dPcXt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));  // `feat` is the caller's
        c->pc_M = M; c->pc_stride = stride; c->pc_C = q.C; c->pc_folded = 0;
        c->pc_on = true;
        return BMM_OK;
    });
}

// the three state vectors, or the counts, of the last state scored: to the host, then the call waits
static int pc_copy_out(bmm_chain* c, void* dst, const void* src, size_t bytes) {
    if (!dst) return BMM_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return BMM_OK;
}
static int pc_score_now(bmm_chain* c) {
    int rc = pc_refused(c);
    if (rc == BMM_OK) rc = pc_armed(c);
    if (rc == BMM_OK) rc = pc_seated(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->started) { rc = chain_start(c); if (rc) return rc; }
    return enqueue_pair_check(c, label_row(c, c->sweep), nullptr, false);
}

int bmm_chain_pair_check_state(bmm_chain* c, double* z_out, double* x2_out, int32_t* df_out) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = pc_score_now(c);
        const size_t np = (size_t)pc_npairs(c->pc_M);
        if (rc == BMM_OK) rc = pc_copy_out(c, z_out, c->dPcZ, np * sizeof(double));
        if (rc == BMM_OK) rc = pc_copy_out(c, x2_out, c->dPcX2, np * sizeof(double));
        if (rc == BMM_OK) rc = pc_copy_out(c, df_out, c->dPcDf, np * sizeof(int32_t));
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rc == BMM_OK && e != hipSuccess) return set_err(BMM_E_HIP, "the pair check failed: %s", hipGetErrorString(e));
        return rc;
    });
}

int bmm_chain_pair_counts(bmm_chain* c, uint32_t* counts, uint32_t* margins, uint32_t* rows) {
    return guarded([&]() -> int {
        if (!c || !counts) return set_err(BMM_E_ARG, "null argument");
        int rc = pc_score_now(c);
        const size_t np = (size_t)pc_npairs(c->pc_M), Kz = (size_t)c->p.K;
        if (rc == BMM_OK) rc = pc_copy_out(c, counts, c->dPcCnt, Kz * np * sizeof(uint32_t));
        if (rc == BMM_OK) rc = pc_copy_out(c, margins, c->dPcMarg, Kz * (size_t)c->pc_M * sizeof(uint32_t));
        if (rc == BMM_OK) rc = pc_copy_out(c, rows, c->dPcNk, Kz * sizeof(uint32_t));
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rc == BMM_OK && e != hipSuccess) return set_err(BMM_E_HIP, "the pair counts failed: %s", hipGetErrorString(e));
        return rc;
    });
}

// n more sweeps, every pc_stride-th evaluated; the rows that are not stay NaN (all bits set)
int bmm_chain_sweeps_pair_check(bmm_chain* c, int n, double* trace) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = pc_refused(c);
        if (rc == BMM_OK) rc = pc_armed(c);
        if (rc || n == 0) return rc;
        HIP_TRY(hipSetDevice(c->device));
        const size_t width = 2 * (size_t)pc_npairs(c->pc_M);
        Recording rec;
        if (trace) {
            rc = rec.alloc((size_t)n * width * sizeof(double), "the pair check trace (n x 2 npairs doubles)");
            if (rc) return rc;
            HIP_TRY(hipMemsetAsync(rec.rows.p, 0xff, (size_t)n * width * sizeof(double), c->stream));
        }
        rec.begin(c, c->pc_rec, width * sizeof(double), c->sweep + 1, c->sweep + 1, true);
        rc = bmm_chain_sweeps(c, n);
        const hipError_t e = rec.end();
        if (rc || !trace) return rc;
        if (e != hipSuccess) return set_err(BMM_E_HIP, "the sweeps failed: %s", hipGetErrorString(e));
        std::vector<double> host((size_t)n * width);
        HIP_TRY(hipMemcpy(host.data(), rec.rows.p, host.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int s = 0; s < n; ++s)
            for (size_t m = 0; m < width; ++m) {
                const double v = host[(size_t)s * width + m];
                trace[(size_t)s + m * (size_t)n] = v != v ? std::nan("") : v;
            }
        return BMM_OK;
    });
}

int bmm_chain_get_pair_check(bmm_chain* c, bmm_pair_check_out* out) {
    return guarded([&]() -> int {
        if (!c || !out) return set_err(BMM_E_ARG, "null argument");
        int rc = pc_armed(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        const size_t np = (size_t)pc_npairs(c->pc_M);
        rc = pc_copy_out(c, out->sum_z, c->dPcSumZ, np * sizeof(double));
        if (rc == BMM_OK) rc = pc_copy_out(c, out->sum_z2, c->dPcSumZ2, np * sizeof(double));
        if (rc == BMM_OK) rc = pc_copy_out(c, out->sum_x2, c->dPcSumX2, np * sizeof(double));
        if (rc == BMM_OK) rc = pc_copy_out(c, out->sum_df, c->dPcSumDf, np * sizeof(long long));
        if (rc == BMM_OK) rc = pc_copy_out(c, out->n_z, c->dPcNz, np * sizeof(int32_t));
        if (rc == BMM_OK) rc = pc_copy_out(c, out->n11, c->dPcN11, np * sizeof(uint32_t));
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rc == BMM_OK && e != hipSuccess) return set_err(BMM_E_HIP, "reading the pair check failed: %s", hipGetErrorString(e));
        if (out->n_folded) *out->n_folded = c->pc_folded;
        return rc;
    });
}

int bmm_chain_pair_check_reset(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = pc_armed(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return pc_reset(c);
}

// ... of a run: refused before a device is touched, armed for it, every stride-th kept sweep folded (sweep_end_folds)
static int pc_run_check(const RunOptions& o, int P, int K) {
    if (!o.pc.on) return BMM_OK;
    return pc_check_args(o.pc.feat.empty() ? nullptr : o.pc.feat.data(), o.pc.o.M, o.pc.o.stride, P, K);
}
static int pc_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.pc.on) return BMM_OK;
    int rc = bmm_chain_set_pair_check(c, o.pc.feat.data(), o.pc.o.M, o.pc.o.stride);
    const size_t width = 2 * (size_t)pc_npairs(o.pc.o.M);
    if (rc == BMM_OK && (o.pc.o.z_rows || o.pc.o.x2_rows)) {
        rc = rec.alloc((size_t)c->S * width * sizeof(double), "the pair check trace (S x 2 npairs doubles)");
        if (rc == BMM_OK) HIP_TRY(hipMemsetAsync(rec.rows.p, 0xff, (size_t)c->S * width * sizeof(double), c->stream));
    }
    if (rc) return rc;
    rec.begin(c, c->pc_rec, width * sizeof(double), c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
static int pc_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.pc.on) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    bmm_pair_check_out out = o.pc.o;
    rc = bmm_chain_get_pair_check(c, &out);
    if (rc || !rec.rows.p) return rc;
    const size_t np = (size_t)pc_npairs(o.pc.o.M), S = (size_t)c->S;
    std::vector<double> host(S * 2 * np);
    HIP_TRY(hipMemcpy(host.data(), rec.rows.p, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; ++s)
        for (size_t m = 0; m < 2 * np; ++m) {
            const double v = host[s * 2 * np + m];
            double* const dst = m < np ? out.z_rows : out.x2_rows;
            if (dst) dst[s + (m < np ? m : m - np) * S] = v != v ? std::nan("") : v;
        }
    return BMM_OK;
}

int bmm_pair_check_plan(int64_t N, int Kc, int M, bmm_pair_check_plan_out* out) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    if (N < 1 || Kc < 1) return set_err(BMM_E_ARG, "N and Kc must be >= 1");
    if (M < 2 || M > kPcMaxM) return set_err(BMM_E_ARG, "the pair check takes 2 to %d features, not %d", kPcMaxM, M);
    const PcPlan q = pc_plan(N, Kc, M);
    out->bytes_slices = (int64_t)q.bytes_slices; out->bytes_counts = (int64_t)q.bytes_counts; out->bytes_fold = (int64_t)q.bytes_fold;
    out->chunks = q.C; out->chunks_per_slice = q.cps; out->chunks_per_round = kPcRound;
    out->tiles = q.tiles; out->row_slices = q.slices; out->label_blocks = q.kblocks; out->ka = q.ka; out->pairs_per_lane = kPcR; out->threads = kPcThreads;
    return BMM_OK;
}

// Any stack of label rows over the same data, on a transient chain: X packed once, the slices cut once, then per state
// the labels uploaded and the state counted and scored by the launches of a chain.
int bmm_device_pair_check(int device, const int32_t* X, int64_t N, int P, int Kc, const int32_t* z, int S,
                          const int32_t* feat, int M, uint32_t* counts, double* rows, const bmm_pair_check_out* out) {
    return guarded([&]() -> int {
        if (!X || !z) return set_err(BMM_E_ARG, "null argument");
        if (S < 1) return set_err(BMM_E_ARG, "S must be >= 1");
        int rc = check_common(N, P, Kc, 0.5, 0.5);
        if (rc == BMM_OK) rc = pc_check_args(feat, M, 1, P, Kc);
        if (rc == BMM_OK) rc = lj_check_labels(z, S, N, Kc, nullptr);
        if (rc) return rc;
        bmm_chain* c = nullptr;
        rc = bmm_chain_create(&c, BMM_SAMPLER_COLLAPSED, N, P, Kc, 1.0, 0.5, 0.5, 1.0, 1.0, 0, 0, device);
        if (rc) return rc;
        struct Guard { bmm_chain* c; ~Guard() { bmm_chain_destroy(c); } } guard{c};
        rc = bmm_chain_set_data_host(c, X);
        if (rc == BMM_OK) rc = bmm_chain_set_pair_check(c, feat, M, 1);
        if (rc) return rc;
        const size_t np = (size_t)pc_npairs(M), Kz = (size_t)Kc;
        std::vector<int32_t> row((size_t)N);
        std::vector<double> vals(2 * np);
        for (int s = 0; s < S; ++s) {
            for (int64_t i = 0; i < N; ++i) row[(size_t)i] = z[(size_t)s + (size_t)i * (size_t)S] - 1;
            HIP_TRY(hipMemcpyAsync(c->dZ[0], row.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            rc = enqueue_pair_check(c, c->dZ[0], nullptr, true);
            if (rc == BMM_OK && counts) rc = pc_copy_out(c, counts + (size_t)s * Kz * np, c->dPcCnt, Kz * np * sizeof(uint32_t));
            if (rc == BMM_OK && rows) rc = pc_copy_out(c, vals.data(), c->dPcZ, np * sizeof(double));
            if (rc == BMM_OK && rows) rc = pc_copy_out(c, vals.data() + np, c->dPcX2, np * sizeof(double));
            const hipError_t e = hipStreamSynchronize(c->stream);  // `row` is written again
            if (rc) return rc;
            if (e != hipSuccess) return set_err(BMM_E_HIP, "scoring state %d failed: %s", s, hipGetErrorString(e));
            if (rows) for (size_t m = 0; m < 2 * np; ++m) rows[(size_t)s + m * (size_t)S] = vals[m];
        }
        if (!out) return BMM_OK;
        bmm_pair_check_out o = *out;
        return bmm_chain_get_pair_check(c, &o);
    });
}

// ---- split-merge moves ----
int bmm_chain_set_split_merge(bmm_chain* c, int moves_per_sweep, int scans) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (moves_per_sweep < 0 || scans < 0 || scans > 4096) return set_err(BMM_E_ARG, "moves_per_sweep and scans must be >= 0 (scans at most 4096)");
        if (moves_per_sweep == 0) { c->sm_moves = 0; return BMM_OK; }
        int rc = sm_refused(c);
        if (rc == BMM_OK) rc = sm_setup(c, scans);
        if (rc) return rc;
        c->sm_moves = moves_per_sweep;
        return BMM_OK;
    });
}

static int sm_ready(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    int rc = sm_refused(c);
    if (rc == BMM_OK) rc = sm_seated(c);
    if (rc == BMM_OK && c->in_run) rc = set_err(BMM_E_STATE, "not offered inside a run");
    if (rc == BMM_OK && !c->dSmStat) rc = sm_setup(c, c->sm_scans);
    return rc;
}

int bmm_chain_split_merge(bmm_chain* c, int n) {
    return guarded([&]() -> int {
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = sm_ready(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        for (int t = 0; t < n; ++t) {
            rc = enqueue_move<false>(c, label_row(c, c->sweep), c->sweep + 1, false);
            if (rc) return rc;
        }
        return BMM_OK;
    });
}

int bmm_chain_split_merge_step(bmm_chain* c, bmm_split_merge_step* out) {
    return guarded([&]() -> int {
        if (!out) return set_err(BMM_E_ARG, "null argument");
        int rc = sm_ready(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        rc = enqueue_move<false>(c, label_row(c, c->sweep), c->sweep + 1, true);
        if (rc) return rc;
        rc = bmm_chain_sync(c);
        if (rc) return rc;
        SmCell h;
        HIP_TRY(hipMemcpy(&h, c->dSmCell, sizeof h, hipMemcpyDeviceToHost));
        return sm_step_out(c, h, c->sm_ctr - 1, out);
    });
}

int bmm_chain_split_merge_stats(bmm_chain* c, int64_t out[5]) {
    return sm_counters_out(c, c ? c->dSmCounters : nullptr, out);
}

// ... of a run: the moves armed for it (bmm_set_split_merge), and their counters for bmm_last_split_merge_stats
static int sm_run_attach(bmm_chain* c, const RunOptions& o) {
    for (int64_t& v : g_sm_stats) v = 0;
    return o.sm.moves > 0 ? bmm_chain_set_split_merge(c, o.sm.moves, o.sm.scans) : BMM_OK;
}
static int sm_run_collect(bmm_chain* c, const RunOptions& o, int rc) {
    return rc == BMM_OK && o.sm.moves > 0 ? bmm_chain_split_merge_stats(c, g_sm_stats) : rc;
}

int bmm_chain_set_labels(bmm_chain* c, const int32_t* z1) {
    return guarded([&]() -> int {
        if (!c || !z1) return set_err(BMM_E_ARG, "null argument");
        if (c->p.mode != MODE_DP) return set_err(BMM_E_UNSUPPORTED, "only a DP chain takes labels between sweeps");
        if (c->cs_on) return cs_refuses("labels set by hand");
        if (c->sharded) return set_err(BMM_E_STATE, "not offered on a sharded chain");
        int rc = sm_seated(c);
        if (rc) return rc;
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        HIP_TRY(hipSetDevice(c->device));
        const int64_t N = c->p.N;
        const size_t K = (size_t)c->p.K, KP = K * c->p.P;
        // uploaded as R holds them (1-based), checked and shifted on the device into the row the next sweep will
        // overwrite; the chain changes only once they have passed
        int32_t* const cur = label_row(c, c->sweep);
        int32_t* const other = c->dZ[(c->sweep + 1) & 1];
        DevBuf tmp, badbuf;
        HIP_TRY(tmp.alloc((size_t)N * sizeof(int32_t)));
        HIP_TRY(badbuf.alloc(sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(badbuf.p, 0xff, sizeof(unsigned long long), c->stream));
        HIP_TRY(hipMemcpyAsync(tmp.p, z1, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        const int64_t nb = (N + 255) / 256;
        const unsigned grid = (unsigned)(nb < 4096 ? nb : 4096);
        hipLaunchKernelGGL(k_labels_from_r, dim3(grid), dim3(256), 0, c->stream, tmp.as<int32_t>(), N, c->p.K, other,
                           badbuf.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, badbuf.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad != ~0ull) return set_err(BMM_E_ARG, "z[%lld] = %d outside 1..%d", (long long)bad, z1[bad], c->p.K);
        HIP_TRY(hipMemcpyAsync(cur, other, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        // the recount: nothing is pending between sweeps (k_count_sweep_end folded the last batch), so the statistics
        // are rebuilt in place
        HIP_TRY(hipMemsetAsync(c->dNk, 0, K * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->dS, 0, KP * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->dDNk, 0, K * kDeltaReps * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->dDS, 0, KP * kDeltaReps * sizeof(int32_t), c->stream));
        hipLaunchKernelGGL(k_count_labels_generic, dim3(grid), dim3(256), 0, c->stream, c->p, c->dX, c->dXb, cur, c->dNk, c->dS);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BMM_OK;
    });
}

// ---- the allocation sampler ----
// who may run it: a whole finite collapsed chain on the bit planes, fixed concentration, rows with labels
static int alloc_refused(const bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (c->na_on) return na_refuses("the allocation sampler");
    if (c->cs_on) return cs_refuses("the allocation sampler");
    if (c->cat_on) return cat_refuses("the allocation sampler");
    if (c->sum_on) return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is not offered on a chain with an armed summary");
    if (c->sharded) return set_err(BMM_E_STATE, "the allocation sampler is not offered on a sharded chain");
    if (c->p.mode != MODE_COLLAPSED)
        return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is the finite collapsed sampler with K unknown: create the chain with that sampler, K = maxK");
    if (c->p.sample_alpha)
        return set_err(BMM_E_UNSUPPORTED, "the allocation sampler keeps the Dirichlet parameter a fixed (the chain's alpha is a): alpha = 0, "
                       "which asks for the concentration's update, is not offered");
    if (c->p.K > kMaxCats) return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is offered up to maxK = %d", kMaxCats);
    if (c->p.P > kEaMaxP) return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is offered up to %d features", kEaMaxP);
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "the eject / absorb moves read the bit planes: not offered on the int32 layout");
    if (c->fs_mask) return fs_mask_refuses("the allocation sampler");
    if (c->temper_on) return temper_refuses("the allocation sampler");
    if (c->predM > 0) return alloc_refuses("the predictive density");
    if (c->loo_on) return alloc_refuses("the leave-one-out predictive");
    if (c->p.K < 2) return set_err(BMM_E_ARG, "maxK must be >= 2");
    if (!c->have_data) return set_err(BMM_E_STATE, "the chain has no rows to seat: set the data first");
    if (!c->have_init) return set_err(BMM_E_STATE, "the chain's rows have no labels: set the initial labels first");
    return BMM_OK;
}
// the chain started and nothing pending: the initial allocation's counts wait in the deltas until a table build folds them
static int alloc_prepare(bmm_chain* c) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->started) {
        const int rc = chain_start(c);
        if (rc) return rc;
    }
    return c->sweep == 0 ? launch_count_tables(c) : BMM_OK;
}
static int alloc_ready(bmm_chain* c) {
    int rc = alloc_refused(c);
    if (rc) return rc;
    if (!c->alloc_on) return set_err(BMM_E_STATE, "the allocation sampler is not armed (bmm_chain_set_alloc)");
    if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
    return alloc_prepare(c);
}
static int alloc_set_k(bmm_chain* c, int K) {
    if (K < 1 || K > c->p.K) return set_err(BMM_E_ARG, "K must lie in 1..maxK = %d", c->p.K);
    int rc = alloc_prepare(c);
    if (rc) return rc;
    std::vector<int32_t> nk((size_t)c->p.K);
    HIP_TRY(hipMemcpyAsync(nk.data(), c->dNk, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = K; k < c->p.K; ++k)
        if (nk[(size_t)k] != 0) return set_err(BMM_E_ARG, "K = %d, but label %d holds %d rows: every label above K must be empty", K, k + 1, nk[(size_t)k]);
    const int32_t k32 = K;
    HIP_TRY(hipMemcpy(c->dEaK, &k32, sizeof k32, hipMemcpyHostToDevice));
    return BMM_OK;
}

int bmm_chain_set_alloc(bmm_chain* c, const double* log_prior_k, int moves_per_sweep, double eject_a) {
    return guarded([&]() -> int {
        int rc = alloc_refused(c);
        if (rc) return rc;
        if (!log_prior_k) return set_err(BMM_E_ARG, "null argument");
        if (moves_per_sweep < 0) return set_err(BMM_E_ARG, "moves_per_sweep must be >= 0");
        if (!(eject_a > 0.0) || !(eject_a < 1e300)) return set_err(BMM_E_ARG, "eject_a must be > 0");
        const int maxK = c->p.K;
        for (int k = 0; k < maxK; ++k)
            if (!(log_prior_k[k] > -1e300 && log_prior_k[k] < 1e300)) return set_err(BMM_E_ARG, "log_prior_k[%d] is not finite: every K in 1..maxK needs positive prior mass", k);
        HIP_TRY(hipSetDevice(c->device));
        const size_t P = (size_t)c->p.P;
        auto carve = [&](Carver& v) {
            c->dEaLogPrior = v.take<double>((size_t)maxK);
            c->dEaCell = v.take<EaCell>(1);
            c->dEaCounters = v.take<long long>(4);
            c->dEaStat = v.take<int32_t>(P + 1);
            c->dEaK = v.take<int32_t>(1);
        };
        const bool first = !c->dEaBlock;
        Carver measure{nullptr};
        carve(measure);
        if (first) {
            HIP_TRY(hipMalloc(&c->dEaBlock, measure.used));
            HIP_TRY(hipMalloc(&c->dEaSide, (size_t)c->p.N));
        }
        Carver real{c->dEaBlock};
        carve(real);
        if (first) {
            HIP_TRY(hipMemsetAsync(c->dEaBlock, 0, measure.used, c->stream));
            const int32_t k32 = maxK;
            HIP_TRY(hipMemcpyAsync(c->dEaK, &k32, sizeof k32, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipMemcpyAsync(c->dEaLogPrior, log_prior_k, (size_t)maxK * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's vector may go
        c->alloc_a = c->alpha0;
        c->alloc_e = eject_a;
        c->alloc_moves = moves_per_sweep;
        if (!c->alloc_on) {
            c->alloc_on = true;
            if (!c->generic) return pick_kernel(c);  // again, without the forms that build their own tables
        }
        return BMM_OK;
    });
}

int bmm_chain_set_k(bmm_chain* c, int K) {
    return guarded([&]() -> int {
        int rc = alloc_ready(c);
        if (rc) return rc;
        return alloc_set_k(c, K);
    });
}

int bmm_chain_get_k(bmm_chain* c, int* K) {
    return guarded([&]() -> int {
        if (!c || !K) return set_err(BMM_E_ARG, "null argument");
        if (!c->alloc_on) return set_err(BMM_E_STATE, "the allocation sampler is not armed (bmm_chain_set_alloc)");
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        int32_t k32 = 0;
        HIP_TRY(hipMemcpy(&k32, c->dEaK, sizeof k32, hipMemcpyDeviceToHost));
        *K = k32;
        return BMM_OK;
    });
}

int bmm_chain_alloc(bmm_chain* c, int n) {
    return guarded([&]() -> int {
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = alloc_ready(c);
        if (rc) return rc;
        for (int t = 0; t < n; ++t) {
            rc = enqueue_ea(c, label_row(c, c->sweep), c->sweep + 1);
            if (rc) return rc;
        }
        return BMM_OK;
    });
}

int bmm_chain_alloc_step(bmm_chain* c, bmm_alloc_step* out) {
    return guarded([&]() -> int {
        if (!out) return set_err(BMM_E_ARG, "null argument");
        int rc = alloc_ready(c);
        if (rc) return rc;
        rc = enqueue_ea(c, label_row(c, c->sweep), c->sweep + 1);
        if (rc) return rc;
        rc = bmm_chain_sync(c);
        if (rc) return rc;
        EaCell h;
        HIP_TRY(hipMemcpy(&h, c->dEaCell, sizeof h, hipMemcpyDeviceToHost));
        out->kind = h.kind; out->accepted = h.accepted; out->j1 = h.j1 + 1; out->j2 = h.j2 + 1;
        out->k_before = h.k_before; out->k_after = h.k_after; out->pe_bits = h.pe_bits; out->members = h.members;
        for (int q = 0; q < 2; ++q) { out->n_before[q] = h.n_before[q]; out->n_after[q] = h.n_after[q]; }
        out->log_prior = h.log_prior; out->log_lik = h.log_lik; out->log_q = h.log_q; out->log_move = h.log_move;
        out->log_u = h.log_u; out->log_r = h.log_r;
        out->sweep = (uint32_t)(c->sweep + 1); out->move = c->ea_ctr - 1;
        if (out->side) HIP_TRY(hipMemcpy(out->side, c->dEaSide, (size_t)c->p.N, hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}

int bmm_chain_alloc_stats(bmm_chain* c, int64_t out[4]) {
    return guarded([&]() -> int {
        if (!c || !out) return set_err(BMM_E_ARG, "null argument");
        for (int q = 0; q < 4; ++q) out[q] = 0;
        if (!c->dEaCounters) return BMM_OK;
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        long long h[4];
        HIP_TRY(hipMemcpy(h, c->dEaCounters, sizeof h, hipMemcpyDeviceToHost));
        for (int q = 0; q < 4; ++q) out[q] = h[q];
        return BMM_OK;
    });
}

// ---- split-merge moves of the allocation chain ----
// who may take them: an armed allocation chain (so whatever bmm_chain_set_alloc refuses stays refused) of two rows or more
static int as_refused(const bmm_chain* c) {
    int rc = alloc_refused(c);
    if (rc) return rc;
    if (!c->alloc_on) return set_err(BMM_E_STATE, "the allocation sampler is not armed (bmm_chain_set_alloc)");
    if (c->p.P > kSmMaxP) return set_err(BMM_E_UNSUPPORTED, "split-merge moves are offered up to %d features", kSmMaxP);
    if (c->p.N < 2) return set_err(BMM_E_ARG, "a split-merge move needs two rows");
    return BMM_OK;
}
// the buffers of the moves, for `scans` intermediate scans
static int as_setup(bmm_chain* c, int scans) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dAsBlock) {
        auto carve = [&](Carver& v) {
            c->dAsCell = v.take<AsCell>(1);
            c->dAsCounters = v.take<long long>(5);
        };
        Carver measure{nullptr};
        carve(measure);
        HIP_TRY(hipMalloc(&c->dAsBlock, measure.used));
        Carver real{c->dAsBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dAsBlock, 0, measure.used, c->stream));
    }
    const int rc = sm_setup(c, scans);  // the side bytes, the log probabilities and the statistic sets
    if (rc) return rc;
    c->as_scans = scans;
    return BMM_OK;
}
static int as_ready(bmm_chain* c) {
    int rc = as_refused(c);
    if (rc) return rc;
    if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
    rc = alloc_prepare(c);
    if (rc == BMM_OK && (!c->dAsBlock || c->sm_sets < c->as_scans + 2)) rc = as_setup(c, c->as_scans);
    return rc;
}

int bmm_chain_set_alloc_split_merge(bmm_chain* c, int moves_per_sweep, int scans) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (moves_per_sweep < 0 || scans < 0 || scans > 4096) return set_err(BMM_E_ARG, "moves_per_sweep and scans must be >= 0 (scans at most 4096)");
        int rc = as_refused(c);
        if (rc == BMM_OK) rc = as_setup(c, scans);
        if (rc) return rc;
        c->as_moves = moves_per_sweep;
        return BMM_OK;
    });
}

int bmm_chain_alloc_split_merge(bmm_chain* c, int n) {
    return guarded([&]() -> int {
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = as_ready(c);
        if (rc) return rc;
        for (int t = 0; t < n; ++t) {
            rc = enqueue_move<true>(c, label_row(c, c->sweep), c->sweep + 1, false);
            if (rc) return rc;
        }
        return BMM_OK;
    });
}

int bmm_chain_alloc_split_merge_step(bmm_chain* c, bmm_alloc_split_step* out) {
    return guarded([&]() -> int {
        if (!out) return set_err(BMM_E_ARG, "null argument");
        int rc = as_ready(c);
        if (rc) return rc;
        rc = enqueue_move<true>(c, label_row(c, c->sweep), c->sweep + 1, true);
        if (rc) return rc;
        rc = bmm_chain_sync(c);
        if (rc) return rc;
        AsCell h;
        HIP_TRY(hipMemcpy(&h, c->dAsCell, sizeof h, hipMemcpyDeviceToHost));
        out->k_before = h.k_before; out->k_after = h.k_after;
        out->moved = h.moved < 0 ? -1 : h.moved + 1; out->pad = 0;
        return sm_step_out(c, h.m, c->as_ctr - 1, out);
    });
}

int bmm_chain_alloc_split_merge_stats(bmm_chain* c, int64_t out[5]) {
    return guarded([&]() -> int { return sm_counters_out(c, c ? c->dAsCounters : nullptr, out); });
}

// ... of a run (bmm_alloc_run): armed, K set (the labels above it empty), K recorded behind every kept sweep
static int alloc_run_check(const RunOptions& o) {
    if (!o.alloc.on && o.as.moves > 0)
        return set_err(BMM_E_UNSUPPORTED, "split-merge moves of the allocation sampler are armed (bmm_set_alloc_split_merge): taken by bmm_alloc_run only");
    if (o.alloc.on && (o.predict() || o.loo.on || o.sm.moves > 0 || o.fs.on || o.init.kind != 0 || o.rel || o.hooks))
        return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is not offered together with relabelling, feature selection, split-merge moves, "
                       "the leave-one-out summary, newdata or a device start: they assume a fixed number of components");
    return BMM_OK;
}
static int alloc_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.alloc.on) return BMM_OK;
    int rc = bmm_chain_set_alloc(c, o.alloc.log_prior_k, o.alloc.moves, o.alloc.eject_a);
    if (rc == BMM_OK) rc = alloc_set_k(c, o.alloc.K0);
    for (int64_t& v : g_as_stats) v = 0;
    if (rc == BMM_OK && o.as.moves > 0) rc = bmm_chain_set_alloc_split_merge(c, o.as.moves, o.as.scans);
    if (rc) return rc;
    HIP_TRY(rec.rows.alloc((size_t)c->S * sizeof(int32_t)));
    const int32_t k0 = o.alloc.K0;
    if (c->burnin == 0) HIP_TRY(hipMemcpy(rec.rows.p, &k0, sizeof k0, hipMemcpyHostToDevice));  // trace row 0: the starting state
    rec.begin(c, c->k_rec, sizeof(int32_t), c->burnin, c->burnin, false);
    return BMM_OK;
}
static int alloc_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.alloc.on) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    const hipError_t ec = hipMemcpy(o.alloc.k_out, rec.rows.p, (size_t)c->S * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (ec != hipSuccess) return set_err(BMM_E_HIP, "copying the K trace failed: %s", hipGetErrorString(ec));
    rc = o.alloc.moves_out ? bmm_chain_alloc_stats(c, o.alloc.moves_out) : BMM_OK;
    return rc == BMM_OK && o.as.moves > 0 ? bmm_chain_alloc_split_merge_stats(c, g_as_stats) : rc;
}

// ---- k-modes++ initial allocation ----
// ... of a run: the start armed for it (bmm_set_init), from the planes that have just arrived
static int init_run_check(const RunOptions& o, int sampler) {
    if (o.init.kind != 0 && sampler != BMM_SAMPLER_COLLAPSED)
        return set_err(BMM_E_UNSUPPORTED, "a device start is armed (bmm_set_init): offered for runs of the finite collapsed sampler only");
    return BMM_OK;
}
static int init_run_attach(bmm_chain* c, const RunOptions& o) {
    return o.init.kind != 0 ? init_labels(c, o.init.kind, 0, o.init.iters, &g_init_info) : BMM_OK;
}

int bmm_chain_init_labels(bmm_chain* c, int kind, int n_centres, int iters, bmm_init_info* info) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        return init_labels(c, kind, n_centres, iters, info);
    });
}

int bmm_chain_get_init_centres(bmm_chain* c, uint32_t* words) {
    if (!c || !words) return set_err(BMM_E_ARG, "null argument");
    if (c->init_keff < 1) return set_err(BMM_E_STATE, "the chain has not been initialised on the device");
    std::memcpy(words, c->init_centres.data(), c->init_centres.size() * sizeof(uint32_t));
    return BMM_OK;
}

int bmm_chain_get_init_rows(bmm_chain* c, int64_t* rows, int32_t* Nk) {
    if (!c || !rows) return set_err(BMM_E_ARG, "null argument");
    if (c->init_keff < 1) return set_err(BMM_E_STATE, "the chain has not been initialised on the device");
    for (int k = 0; k < c->init_keff; ++k) rows[k] = c->init_rows[(size_t)k];
    if (Nk) std::memcpy(Nk, c->init_nk.data(), c->init_nk.size() * sizeof(int32_t));
    return BMM_OK;
}

// ---- feature selection ----
// who may carry a mask: the two counting samplers, whole (not sharded), with rows that have or will get seats
static int fs_refused(const bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (c->na_on) return na_refuses("feature selection");
    if (c->cat_on) return cat_refuses("feature selection");
    if (c->sharded) return set_err(BMM_E_STATE, "feature selection is not offered on a sharded chain");
    if (explicit_params(c->p.mode))
        return set_err(BMM_E_UNSUPPORTED, "feature selection is offered for the collapsed and DP samplers only: the stick-breaking and "
                       "full samplers carry theta, which the collapsed indicator step integrates out");
    // (a DP chain has beta == gamma: bmm_chain_create makes no other; a run armed for one that has not is refused in run_chain)
    if (c->predM > 0) return set_err(BMM_E_UNSUPPORTED, "feature selection is not offered together with newdata: the predictive tables are written for the all-features model");
    if (c->loo_on) return set_err(BMM_E_UNSUPPORTED, "feature selection is not offered together with the leave-one-out summary: its tables are written for the all-features model");
    if (c->sm_moves > 0) return set_err(BMM_E_UNSUPPORTED, "feature selection is not offered together with split-merge moves: their ratio is written for the all-features model");
    if (c->alloc_on) return alloc_refuses("feature selection");
    if (c->temper_on) return temper_refuses("feature selection");
    if (!c->have_data) return set_err(BMM_E_STATE, "the chain has no rows to seat: set the data first");
    if (c->p.mode == MODE_COLLAPSED && !c->have_init) return set_err(BMM_E_STATE, "the chain's rows have no labels: set the initial labels first");
    return BMM_OK;
}
// the block behind a mask, the mask all ones; the kernel choice is made again without the table-building forms
static int fs_setup(bmm_chain* c) {
    if (c->fs_mask) return BMM_OK;
    const size_t P = (size_t)c->p.P, W = (P + 31) / 32;
    HIP_TRY(hipSetDevice(c->device));
    Carver a{nullptr};
    auto carve = [&](Carver& v) {
        c->dFsRec = v.take<double>(3 * P);
        c->dFsProb = v.take<double>(P);
        c->dFsMask = v.take<uint32_t>(W);
        c->dFsCount = v.take<uint32_t>(P);
        c->dFsGamma = v.take<uint8_t>(P);
    };
    carve(a);
    const size_t bytes = a.used;
    if (!c->dFsBlock) HIP_TRY(hipMalloc(&c->dFsBlock, bytes));  // (kept by a call that failed further down: not allocated twice)
    Carver real{c->dFsBlock};
    carve(real);
    std::vector<uint32_t> ones(W, 0xffffffffu);
    if (P % 32) ones[W - 1] = (1u << (P % 32)) - 1u;
    HIP_TRY(hipMemsetAsync(c->dFsBlock, 0, bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->dFsGamma, 1, P, c->stream));
    HIP_TRY(hipMemcpyAsync(c->dFsMask, ones.data(), W * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // `ones` goes out of scope
    c->fs_mask = true;
    c->fs_folded = 0;
    c->fs_last = -1;
    return c->generic ? BMM_OK : pick_kernel(c);
}
static int fs_reset(bmm_chain* c) {
    c->fs_folded = 0;
    HIP_TRY(hipMemsetAsync(c->dFsCount, 0, (size_t)c->p.P * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->dFsProb, 0, (size_t)c->p.P * sizeof(double), c->stream));
    return BMM_OK;
}

int bmm_chain_set_feature_select(bmm_chain* c, int on, double rho) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!on) { c->fs_on = false; return BMM_OK; }  // the mask stays as it is
        if (!(rho > 0.0 && rho < 1.0)) return set_err(BMM_E_ARG, "rho must lie strictly inside (0, 1): it is the prior probability that a feature clusters");
        int rc = fs_refused(c);
        if (rc == BMM_OK) rc = fs_setup(c);
        if (rc == BMM_OK) rc = fs_reset(c);
        if (rc) return rc;
        c->fs_rho = rho;
        c->fs_logit = log_(rho) - log_(1.0 - rho);
        c->fs_rec.fold = true;  // every step from now on
        c->fs_rec.from = 0;
        c->fs_on = true;
        return BMM_OK;
    });
}

int bmm_chain_set_features(bmm_chain* c, const uint8_t* gamma) {
    return guarded([&]() -> int {
        if (!c || !gamma) return set_err(BMM_E_ARG, "null argument");
        int rc = fs_refused(c);
        if (rc) return rc;
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        const int P = c->p.P, W = (P + 31) / 32;
        std::vector<uint32_t> words((size_t)W, 0u);
        std::vector<uint8_t> bytes((size_t)P);
        for (int d = 0; d < P; ++d) {
            if (gamma[d] > 1) return set_err(BMM_E_ARG, "gamma[%d] = %d is neither 0 nor 1", d, (int)gamma[d]);
            bytes[d] = gamma[d];
            words[d >> 5] |= (uint32_t)gamma[d] << (d & 31);
        }
        rc = fs_setup(c);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->dFsMask, words.data(), (size_t)W * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dFsGamma, bytes.data(), (size_t)P, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BMM_OK;
    });
}

int bmm_chain_get_features(bmm_chain* c, uint8_t* gamma) {
    return guarded([&]() -> int {
        if (!c || !gamma) return set_err(BMM_E_ARG, "null argument");
        if (!c->fs_mask) { std::memset(gamma, 1, (size_t)c->p.P); return BMM_OK; }  // every feature clusters
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(gamma, c->dFsGamma, (size_t)c->p.P, hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}

int bmm_chain_feature_step(bmm_chain* c, bmm_feature_step* out) {
    return guarded([&]() -> int {
        if (!c || !out) return set_err(BMM_E_ARG, "null argument");
        if (!c->fs_mask || c->fs_last < 0) return set_err(BMM_E_STATE, "no indicator step has run yet (bmm_chain_set_feature_select, then a sweep)");
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        const size_t P = (size_t)c->p.P;
        if (out->lambda) HIP_TRY(hipMemcpy(out->lambda, c->dFsRec, P * sizeof(double), hipMemcpyDeviceToHost));
        if (out->p) HIP_TRY(hipMemcpy(out->p, c->dFsRec + P, P * sizeof(double), hipMemcpyDeviceToHost));
        if (out->u) HIP_TRY(hipMemcpy(out->u, c->dFsRec + 2 * P, P * sizeof(double), hipMemcpyDeviceToHost));
        if (out->gamma) HIP_TRY(hipMemcpy(out->gamma, c->dFsGamma, P, hipMemcpyDeviceToHost));
        out->sweep = (uint32_t)c->fs_last;
        return BMM_OK;
    });
}

int bmm_chain_sweeps_features(bmm_chain* c, int n, uint8_t* gamma_trace) {
    return guarded([&]() -> int {
        if (!c || !gamma_trace) return set_err(BMM_E_ARG, "null argument");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        if (!c->fs_on) return set_err(BMM_E_STATE, "feature selection is not armed (bmm_chain_set_feature_select)");
        if (n == 0) return BMM_OK;
        HIP_TRY(hipSetDevice(c->device));
        const size_t bytes = (size_t)n * (size_t)c->p.P;
        Recording rec;
        HIP_TRY(rec.rows.alloc(bytes));
        rec.begin(c, c->fs_rec, (size_t)c->p.P, c->sweep + 1, c->fs_rec.from, c->fs_rec.fold);
        int rc = bmm_chain_sweeps(c, n);
        if (rc == BMM_OK) {
            hipError_t e = hipMemcpyAsync(gamma_trace, rec.rows.p, bytes, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = rec.end();
            if (e != hipSuccess) rc = set_err(BMM_E_HIP, "copying the indicator trace failed: %s", hipGetErrorString(e));
        }
        return rc;
    });
}

int bmm_chain_get_feature_summary(bmm_chain* c, double* inclusion, double* inclusion_rb, int* n_folded) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->fs_mask) return set_err(BMM_E_STATE, "feature selection was never armed on this chain (bmm_chain_set_feature_select)");
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        const size_t P = (size_t)c->p.P;
        const double n = (double)c->fs_folded;  // 0: NaN
        if (inclusion) {
            std::vector<uint32_t> cnt(P);
            HIP_TRY(hipMemcpy(cnt.data(), c->dFsCount, P * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t d = 0; d < P; ++d) inclusion[d] = (double)cnt[d] / n;
        }
        if (inclusion_rb) {
            HIP_TRY(hipMemcpy(inclusion_rb, c->dFsProb, P * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t d = 0; d < P; ++d) inclusion_rb[d] = inclusion_rb[d] / n;
        }
        if (n_folded) *n_folded = c->fs_folded;
        return BMM_OK;
    });
}

int bmm_chain_feature_reset(bmm_chain* c) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->fs_mask) return BMM_OK;
        HIP_TRY(hipSetDevice(c->device));
        return fs_reset(c);
    });
}

// ... of a run: armed for it (bmm_set_feature_select), a gamma-step behind every sweep, kept sweeps folded and recorded
static int fs_run_check(const RunOptions& o, int sampler, double beta, double gamma) {
    if (!o.fs.on) return BMM_OK;
    if (explicit_params(sampler))
        return set_err(BMM_E_UNSUPPORTED, "feature selection is offered for the collapsed and DP samplers only: the stick-breaking and "
                       "full samplers carry theta, which the collapsed indicator step integrates out");
    if (sampler == BMM_SAMPLER_DP && beta != gamma)
        return set_err(BMM_E_UNSUPPORTED, "feature selection on the DP sampler needs beta == gamma: its new-cluster term is the model's only then");
    if (o.predict() || o.loo.on || o.sm.moves > 0)
        return set_err(BMM_E_UNSUPPORTED, "feature selection is not offered together with newdata, the leave-one-out summary or split-merge "
                       "moves: their tables and ratios are written for the all-features model");
    const bmm_feature_out& f = o.fs.o;
    if (!(f.rho > 0.0 && f.rho < 1.0)) return set_err(BMM_E_ARG, "rho must lie strictly inside (0, 1): it is the prior probability that a feature clusters");
    if (!f.gamma || !f.inclusion || !f.inclusion_rb || !f.n_selected) return set_err(BMM_E_ARG, "feature selection: null buffer");
    return BMM_OK;
}
static int fs_run_attach(bmm_chain* c, const RunOptions& o, Recording& rec) {
    if (!o.fs.on) return BMM_OK;
    const int rc = bmm_chain_set_feature_select(c, 1, o.fs.o.rho);
    if (rc) return rc;
    const size_t bytes = (size_t)c->S * (size_t)c->p.P;
    HIP_TRY(rec.rows.alloc(bytes));
    HIP_TRY(hipMemsetAsync(rec.rows.p, 1, bytes, c->stream));  // (trace row 0 of a run without burn-in: the initial mask)
    rec.begin(c, c->fs_rec, (size_t)c->p.P, c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
static int fs_run_collect(bmm_chain* c, const RunOptions& o, Recording& rec, int rc) {
    if (!o.fs.on) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    const bmm_feature_out& f = o.fs.o;
    const int S = c->S, P = c->p.P;
    const hipError_t ec = hipMemcpy(f.gamma, rec.rows.p, (size_t)S * (size_t)P, hipMemcpyDeviceToHost);
    if (ec != hipSuccess) return set_err(BMM_E_HIP, "copying the indicator trace failed: %s", hipGetErrorString(ec));
    for (int t = 0; t < S; ++t) {
        int32_t n = 0;
        for (int d = 0; d < P; ++d) n += f.gamma[(size_t)t * P + d];
        f.n_selected[t] = n;
    }
    return bmm_chain_get_feature_summary(c, f.inclusion, f.inclusion_rb, f.n_folded);
}

// ---- missing data: NA cells imputed behind every sweep (include/bmm_mcmc.h "missing data") ----
// the cell list itself: in range and strictly ascending in (row, column).  Nothing of a device is touched.
static int na_check_cells(const int64_t* rows, const int32_t* cols, int64_t n, int64_t N, int P) {
    if (n < 0) return set_err(BMM_E_ARG, "n_cells must be >= 0");
    if (n > 0 && (!rows || !cols)) return set_err(BMM_E_ARG, "null cell list");
    for (int64_t q = 0; q < n; ++q) {
        if (rows[q] < 0 || rows[q] >= N || cols[q] < 0 || cols[q] >= P)
            return set_err(BMM_E_ARG, "missing cell %lld = (%lld, %d) lies outside the %lld x %d matrix", (long long)q, (long long)rows[q],
                           (int)cols[q], (long long)N, P);
        if (q > 0 && (rows[q] < rows[q - 1] || (rows[q] == rows[q - 1] && cols[q] <= cols[q - 1])))
            return set_err(BMM_E_ARG, "the missing cells must be strictly ascending in (row, column): cell %lld is not", (long long)q);
    }
    return BMM_OK;
}
// who may carry missing cells: a whole chain on bit planes of its own, with none of the options that read the matrix
// as observed or cut it once
static int na_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered on a sharded chain");
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "the imputation step rewrites the bit planes: not offered on the int32 layout");
    if (c->cat_on) return cat_refuses("the imputation step");
    if (c->xb_borrowed || c->shares_device || (c->planes && c->planes->refs.load() > 1) || c->ladder)
        return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered on planes that several chains read (bmm_chain_share_data, a "
                       "ladder): every chain would need completed cells of its own");
    if (c->loo_on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with the leave-one-out summary: it would score imputed cells as data");
    if (c->temper_on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered on a tempered chain: the rungs share one matrix");
    if (c->pc_on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with the pair check: its column slices are cut once");
    if (c->fs_mask || c->sm_moves > 0 || c->alloc_on)
        return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with feature selection, split-merge moves or the allocation sampler");
    if (!c->have_data || !c->dXb) return set_err(BMM_E_STATE, "the chain has no data: set the data first");
    if (c->shard_open) return set_err(BMM_E_STATE, "a sweep is open");
    return BMM_OK;
}
static bool na_seated(const bmm_chain* c) { return c->started && (c->p.mode == MODE_COLLAPSED || c->sweep >= 1); }
static void na_disarm(bmm_chain* c) {
    c->na_on = false;
    c->na_cells = c->na_sites = c->na_folded = 0;
    c->na_rows.clear(); c->na_cols.clear();
    c->na_rec = SweepTrace{};
}
static int na_reset(bmm_chain* c) {
    c->na_folded = 0;
    HIP_TRY(hipMemsetAsync(c->dNaSum, 0, (size_t)c->na_cells * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(c->dNaOnes, 0, (size_t)c->na_cells * sizeof(uint32_t), c->stream));
    return BMM_OK;
}

int bmm_chain_set_missing(bmm_chain* c, const int64_t* rows, const int32_t* cols, int64_t n_cells) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = na_check_cells(rows, cols, n_cells, c->p.N, c->p.P);
        if (rc) return rc;
        if (n_cells == 0) {  // withdrawn: the planes keep the cells' last values
            if (c->na_on) HIP_TRY(hipStreamSynchronize(c->stream));
            na_disarm(c);
            return BMM_OK;
        }
        if (c->na_on) return set_err(BMM_E_STATE, "missing cells are already declared: withdraw them first (n_cells = 0)");
        rc = na_refused(c);
        if (rc) return rc;
        if (c->in_run && c->sweep > 0) return set_err(BMM_E_STATE, "not offered inside a run");
        HIP_TRY(hipSetDevice(c->device));
        const ChainParams& p = c->p;
        // the sites: one per (row, plane word) that has a hole
        std::vector<int64_t> srow, sfirst;
        std::vector<int32_t> sword;
        std::vector<uint32_t> smask;
        for (int64_t q = 0; q < n_cells; ++q) {
            const int w = cols[q] >> 5;
            if (srow.empty() || srow.back() != rows[q] || sword.back() != w) {
                srow.push_back(rows[q]); sword.push_back(w); smask.push_back(0u); sfirst.push_back(q);
            }
            smask.back() |= 1u << (cols[q] & 31);
        }
        const size_t ns = srow.size(), nc = (size_t)n_cells, KP = (size_t)p.K * p.P;
        Carver measure{nullptr};
        auto carve = [&](Carver& v) {
            c->dNaRow = v.take<int64_t>(ns);
            c->dNaFirst = v.take<int64_t>(ns);
            c->dNaSum = v.take<double>(nc);
            c->dNaPhi = v.take<double>(KP);
            c->dNaWord = v.take<int32_t>(ns);
            c->dNaMask = v.take<uint32_t>(ns);
            c->dNaCnt = v.take<int32_t>(2 * KP);
            c->dNaOnes = v.take<uint32_t>(nc);
        };
        carve(measure);
        rc = pred_room(measure.used, "the missing cells' site list and folds");
        if (rc) return rc;
        if (c->dNaBlock) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->dNaBlock); c->dNaBlock = nullptr; }
        HIP_TRY(hipMalloc(&c->dNaBlock, measure.used));
        Carver real{c->dNaBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dNaBlock, 0, measure.used, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dNaRow, srow.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dNaFirst, sfirst.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dNaWord, sword.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dNaMask, smask.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        c->na_cells = n_cells; c->na_sites = (int64_t)ns; c->na_folded = 0;
        c->na_lds = na_tables_in_lds(p.K, p.P);
        // a workgroup per kNaThreads sites, up to two per compute unit, grid-stride beyond: every workgroup flushes a
        // table of its own onto the same K P words, and those adds queue per word (north star, step alone: 0.041 ms at two
        // per unit against 0.065 at eight with 1 % of the cells missing, 0.227 against 0.277 with 30 %; one per unit leaves
        // the gathers too few waves: 0.342 at 30 %)
        const int64_t nb = ((int64_t)ns + kNaThreads - 1) / kNaThreads, most = (int64_t)2 * (c->num_cus > 0 ? c->num_cus : 256);
        const int dbg_grid = dbg_env_int("BMM_DEBUG_NA_GRID", 0);  // the test variant: that many workgroups at the most
        c->na_grid = (int)(dbg_grid > 0 && nb > dbg_grid ? dbg_grid : (nb < most ? nb : most));
        if (c->na_lds)  // the draw keeps the rates and the deltas: up to 72 KiB of dynamic LDS
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_na_draw<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(KP * (sizeof(double) + sizeof(int32_t)))));
        // the starting fill; where the rows have seats the counts follow the planes
        const NaArgs a = na_args(c, na_seated(c) ? label_row(c, c->sweep) : nullptr, 0u, false);
        hipLaunchKernelGGL(k_na_fill, dim3((unsigned)c->na_grid), dim3(kNaThreads), 0, c->stream, p, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));  // the host vectors go out of scope
        c->na_rows.assign(rows, rows + n_cells);
        c->na_cols.assign(cols, cols + n_cells);
        c->na_rec = SweepTrace{};
        c->na_rec.fold = true;  // every step from now on
        c->na_rec.from = 0;
        c->na_on = true;
        return BMM_OK;
    });
}

int bmm_chain_impute_step(bmm_chain* c) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->na_on) return set_err(BMM_E_STATE, "no missing cells are declared (bmm_chain_set_missing)");
        HIP_TRY(hipSetDevice(c->device));
        if (!c->started && c->p.mode == MODE_COLLAPSED) {
            const int rc = chain_start(c);
            if (rc) return rc;
        }
        if (!na_seated(c)) return set_err(BMM_E_STATE, "the chain has rows without a label: run a sweep first");
        return enqueue_na_step(c, c->sweep);
    });
}

int bmm_chain_get_missing_state(bmm_chain* c, uint8_t* bits) {
    return guarded([&]() -> int {
        if (!c || !bits) return set_err(BMM_E_ARG, "null argument");
        if (!c->na_on) return set_err(BMM_E_STATE, "no missing cells are declared (bmm_chain_set_missing)");
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        // the sites' words, gathered on the device; a site's cells are consecutive in the list
        const size_t ns = (size_t)c->na_sites;
        DevBuf buf;
        HIP_TRY(buf.alloc(ns * sizeof(uint32_t)));
        const NaArgs a = na_args(c, nullptr, 0u, false);
        hipLaunchKernelGGL(k_na_words, dim3((unsigned)c->na_grid), dim3(kNaThreads), 0, c->stream, c->p, a, buf.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> word(ns);
        HIP_TRY(hipMemcpyAsync(word.data(), buf.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        int64_t last_row = -1, t = -1; int last_w = -1;
        for (int64_t q = 0; q < c->na_cells; ++q) {
            const int64_t i = c->na_rows[(size_t)q];
            const int w = c->na_cols[(size_t)q] >> 5;
            if (i != last_row || w != last_w) { ++t; last_row = i; last_w = w; }
            bits[q] = (uint8_t)((word[(size_t)t] >> (c->na_cols[(size_t)q] & 31)) & 1u);
        }
        return BMM_OK;
    });
}

int bmm_chain_get_missing_summary(bmm_chain* c, double* mean_rb, double* mean_draw, int64_t* n_folded) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->na_on) return set_err(BMM_E_STATE, "no missing cells are declared (bmm_chain_set_missing)");
        int rc = bmm_chain_sync(c);
        if (rc) return rc;
        const size_t nc = (size_t)c->na_cells;
        const double n = (double)c->na_folded;  // 0: NaN
        if (mean_rb) {
            HIP_TRY(hipMemcpy(mean_rb, c->dNaSum, nc * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < nc; ++q) mean_rb[q] = mean_rb[q] / n;
        }
        if (mean_draw) {
            std::vector<uint32_t> cnt(nc);
            HIP_TRY(hipMemcpy(cnt.data(), c->dNaOnes, nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < nc; ++q) mean_draw[q] = (double)cnt[q] / n;
        }
        if (n_folded) *n_folded = c->na_folded;
        return BMM_OK;
    });
}

int bmm_chain_missing_reset(bmm_chain* c) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (!c->na_on) return BMM_OK;
        HIP_TRY(hipSetDevice(c->device));
        return na_reset(c);
    });
}

// ... of a run: armed for it (bmm_set_missing), the step behind every sweep, the kept sweeps folded
static int na_run_check(const RunOptions& o, int64_t N, int P) {
    if (!o.na.on) return BMM_OK;
    int rc = na_check_cells(o.na.rows, o.na.cols, o.na.n, N, P);
    if (rc) return rc;
    if (!o.na.o.mean_rb || !o.na.o.mean_draw || !o.na.o.last || !o.na.o.n_folded) return set_err(BMM_E_ARG, "missing data: null buffer");
    if (dbg_env("BMM_X_LAYOUT_INT32")) return set_err(BMM_E_UNSUPPORTED, "the imputation step rewrites the bit planes: not offered on the int32 layout");
    if (o.loo.on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with the leave-one-out summary: it would score imputed cells as data");
    if (o.temper.on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with parallel tempering: the rungs share one matrix");
    if (o.pc.on) return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with the pair check: its column slices are cut once");
    if (o.fs.on || o.sm.moves > 0 || o.init.kind != 0 || o.alloc.on)
        return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with feature selection, split-merge moves, a device start or "
                       "the allocation sampler");
    if (o.hooks || o.rel)
        return set_err(BMM_E_UNSUPPORTED, "missing cells are not offered together with a probability hand-off (relabel = TRUE): relabel from the "
                       "label trace instead (ECR)");
    return BMM_OK;
}
static int na_run_attach(bmm_chain* c, const RunOptions& o) {
    if (!o.na.on || o.na.n == 0) return BMM_OK;
    const int rc = bmm_chain_set_missing(c, o.na.rows, o.na.cols, o.na.n);
    if (rc) return rc;
    c->na_rec.from = run_first_fold(c);
    return BMM_OK;
}
static int na_run_collect(bmm_chain* c, const RunOptions& o, int rc) {
    if (!o.na.on) return rc;
    if (rc) return rc;
    *o.na.o.n_folded = 0;
    if (o.na.n == 0) return BMM_OK;
    rc = bmm_chain_get_missing_summary(c, o.na.o.mean_rb, o.na.o.mean_draw, o.na.o.n_folded);
    if (rc == BMM_OK) rc = bmm_chain_get_missing_state(c, o.na.o.last);
    return rc;
}

// ---- constrained allocations: known labels and allowed-label sets (include/bmm_mcmc.h "constraints") ----
// the list itself: rows in range and strictly ascending, masks non-zero with no bit at or above K.  No device is touched.
static int cs_check_list(int64_t n, const int64_t* rows, const uint64_t* masks, int64_t N, int K) {
    if (n < 0) return set_err(BMM_E_ARG, "constraints: n must be >= 0");
    if (n > 0 && (!rows || !masks)) return set_err(BMM_E_ARG, "constraints: null list");
    for (int64_t q = 0; q < n; ++q) {
        if (rows[q] < 0 || rows[q] >= N)
            return set_err(BMM_E_ARG, "constraints: row %lld (entry %lld) lies outside the %lld rows", (long long)rows[q], (long long)q, (long long)N);
        if (q > 0 && rows[q] <= rows[q - 1])
            return set_err(BMM_E_ARG, "constraints: the rows must be strictly ascending: entry %lld is not", (long long)q);
        if (masks[q] == 0) return set_err(BMM_E_ARG, "constraints: row %lld has an empty set of allowed labels", (long long)rows[q]);
        if (K < 64 && (masks[q] >> K) != 0)
            return set_err(BMM_E_ARG, "constraints: row %lld allows a label above K = %d", (long long)rows[q], K);
    }
    return BMM_OK;
}
// who may carry constrained rows: a whole chain whose rows only its own sweep moves
static int cs_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered on a sharded chain");
    if (c->alloc_on) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered by the allocation sampler: its moves change which labels exist");
    if (c->sm_moves > 0) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with split-merge moves: they move rows by themselves");
    if (c->temper_on || c->ladder) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered on a tempered chain: an exchange would hand the rows a state that knows nothing of them");
    if (c->loo_on) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with the leave-one-out summary: a held row is not predicted, it is given");
    if (c->shard_open) return set_err(BMM_E_STATE, "a sweep is open");
    return BMM_OK;
}
static bool cs_seated(const bmm_chain* c) { return c->started && (c->p.mode == MODE_COLLAPSED || c->sweep >= 1); }

int bmm_chain_set_constraints(bmm_chain* c, int64_t n, const int64_t* rows, const uint64_t* masks) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        int rc = cs_check_list(n, rows, masks, c->p.N, c->p.K);
        if (rc) return rc;
        if (n == 0) {  // withdrawn: the rows are free from the next sweep on, the counters stay readable
            if (c->cs_on) HIP_TRY(hipStreamSynchronize(c->stream));
            c->cs_on = false;
            c->cs_rows.clear();
            return BMM_OK;
        }
        if (c->cs_on) return set_err(BMM_E_STATE, "constraints are already set: withdraw them first (n = 0)");
        rc = cs_refused(c);
        if (rc) return rc;
        if (c->in_run && c->sweep > 0) return set_err(BMM_E_STATE, "not offered inside a run");
        HIP_TRY(hipSetDevice(c->device));
        Carver measure{nullptr};
        auto carve = [&](Carver& v) {
            c->dCsRows = v.take<int64_t>((size_t)n);
            c->dCsMasks = v.take<uint64_t>((size_t)n);
            c->dCsStats = v.take<unsigned long long>(2);
        };
        carve(measure);
        rc = pred_room(measure.used, "the constrained rows' list");
        if (rc) return rc;
        if (c->dCsBlock) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->dCsBlock); c->dCsBlock = nullptr; }
        HIP_TRY(hipMalloc(&c->dCsBlock, measure.used));
        Carver real{c->dCsBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dCsBlock, 0, measure.used, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dCsRows, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dCsMasks, masks, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        c->cs_rows.assign(rows, rows + n);
        // rows that have labels are put inside their sets now and the counts follow; the finite chain's starting labels
        // are projected when it starts (chain_start), a DP or explicit chain seats its rows in its first sweep
        if (cs_seated(c)) {
            rc = launch_constrain(c, nullptr, label_row(c, c->sweep), 0, c->p.N, true, true);
            if (rc) { c->cs_rows.clear(); return rc; }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's lists may go
        c->cs_on = true;
        return BMM_OK;
    });
}

int bmm_chain_constraint_stats(bmm_chain* c, int64_t* proposed, int64_t* reverted) {
    return guarded([&]() -> int {
        if (!c || !proposed || !reverted) return set_err(BMM_E_ARG, "null argument");
        if (!c->dCsBlock) return set_err(BMM_E_STATE, "no constraints were set (bmm_chain_set_constraints)");
        const int rc = bmm_chain_sync(c);
        if (rc) return rc;
        unsigned long long v[2] = {0, 0};
        HIP_TRY(hipMemcpy(v, c->dCsStats, sizeof v, hipMemcpyDeviceToHost));
        *proposed = (int64_t)v[0]; *reverted = (int64_t)v[1];
        return BMM_OK;
    });
}

// ... of a run: armed for it (bmm_set_constraints), refused before a device is touched
static thread_local int64_t g_cs_stats[2] = {0, 0};
static int cs_run_check(const RunOptions& o, int64_t N, int K) {
    if (!o.cs.on) return BMM_OK;
    const int rc = cs_check_list(o.cs.n, o.cs.rows, o.cs.masks, N, K);
    if (rc) return rc;
    if (o.sm.moves > 0) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with split-merge moves: they move rows by themselves");
    if (o.temper.on) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with parallel tempering: an exchange would hand the rows a state that knows nothing of them");
    if (o.loo.on) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with the leave-one-out summary: a held row is not predicted, it is given");
    if (o.init.kind != 0) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with a device start: it knows nothing of the rows' allowed labels");
    if (o.hooks || o.rel)
        return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered together with a probability hand-off (relabel = TRUE): the "
                       "handed-on rows would be those of draws that were reverted; anchored rows need no relabelling, and ECR reads the labels alone");
    if (o.alloc.on) return set_err(BMM_E_UNSUPPORTED, "constrained rows are not offered by the allocation sampler");
    return BMM_OK;
}
static int cs_run_attach(bmm_chain* c, const RunOptions& o) {
    g_cs_stats[0] = g_cs_stats[1] = 0;
    return o.cs.on ? bmm_chain_set_constraints(c, o.cs.n, o.cs.rows, o.cs.masks) : BMM_OK;
}
static int cs_run_collect(bmm_chain* c, const RunOptions& o, int rc) {
    return rc == BMM_OK && o.cs.on ? bmm_chain_constraint_stats(c, &g_cs_stats[0], &g_cs_stats[1]) : rc;
}

// ---- categorical features (include/bmm_mcmc.h "categorical features") ----
// who may carry levels: a whole counting chain on bit planes whose every armed option reads labels and counts only
static int cat_refused(const bmm_chain* c) {
    if (!c->bits) return set_err(BMM_E_UNSUPPORTED, "categorical features read the bit planes: not offered on the int32 layout");
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered on a sharded chain");
    if (explicit_params(c->p.mode))
        return set_err(BMM_E_UNSUPPORTED, "categorical features are offered for the collapsed and DP samplers only: the stick-breaking "
                       "and full samplers carry a Bernoulli theta per column");
    if (c->alloc_on) return alloc_refuses("a categorical feature");
    if (c->temper_on || c->ladder) return temper_refuses("a categorical feature");
    if (c->fs_mask) return fs_mask_refuses("a categorical feature");
    if (c->sm_moves > 0) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with split-merge moves: their ratio knows the Bernoulli cell only");
    if (c->na_on) return na_refuses("a categorical feature");
    if (c->predM > 0) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with newdata: the predictive tables know the Bernoulli cell only");
    if (c->loo_on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the leave-one-out summary: its tables know the Bernoulli cell only");
    if (c->lp_on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the log joint trace: its cells are Bernoulli cells");
    if (c->pc_on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the pair check: the columns of a block depend on each other by construction");
    if (c->shard_open) return set_err(BMM_E_STATE, "a sweep is open");
    return BMM_OK;
}
static void cat_withdraw(bmm_chain* c) {
    c->cat_on = c->cat_checked = false;
    c->cat_levels.clear();
    c->cat_blocks.clear();
}

int bmm_chain_set_categorical(bmm_chain* c, const int32_t* levels, int F) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (F < 0) return set_err(BMM_E_ARG, "categorical: F must be >= 0");
        if (c->in_run && c->sweep > 0) return set_err(BMM_E_STATE, "not offered inside a run");
        if (F == 0) {  // withdrawn: every column is a Bernoulli column from the next table build on
            if (!c->cat_on) return BMM_OK;
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            cat_withdraw(c);
            return c->generic ? BMM_OK : pick_kernel(c);
        }
        std::vector<uint8_t> lev;
        std::vector<CatBlock> blocks;
        int rc = cat_map(levels, F, c->p.P, &lev, &blocks, nullptr);
        if (rc == BMM_OK) rc = cat_refused(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        const size_t nb = blocks.size() ? blocks.size() : 1;
        Carver measure{nullptr};
        auto carve = [&](Carver& v) {
            c->dCatBad = v.take<unsigned long long>(1);
            c->dCatBlocks = v.take<CatBlock>(nb);
            c->dCatLev = v.take<uint8_t>((size_t)c->p.P);
        };
        carve(measure);
        HIP_TRY(hipStreamSynchronize(c->stream));  // a table build in flight reads the bytes that go
        if (c->dCatBlock) { (void)hipFree(c->dCatBlock); c->dCatBlock = nullptr; }
        const bool was = c->cat_on;
        cat_withdraw(c);
        HIP_TRY(hipMalloc(&c->dCatBlock, measure.used));
        Carver real{c->dCatBlock};
        carve(real);
        HIP_TRY(hipMemsetAsync(c->dCatBlock, 0, measure.used, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dCatLev, lev.data(), lev.size(), hipMemcpyHostToDevice, c->stream));
        if (!blocks.empty())
            HIP_TRY(hipMemcpyAsync(c->dCatBlocks, blocks.data(), blocks.size() * sizeof(CatBlock), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the host vectors go
        c->cat_levels.assign(levels, levels + F);
        c->cat_blocks = blocks;
        c->cat_on = true;
        rc = cat_check(c);  // (a chain without data: checked when they arrive)
        if (rc) {
            cat_withdraw(c);
            if (was && !c->generic) (void)pick_kernel(c);
            return rc;
        }
        return c->generic ? BMM_OK : pick_kernel(c);  // again, without the forms that build their own tables
    });
}

int bmm_chain_get_categorical(const bmm_chain* c, int32_t* levels, int* F) {
    if (!c || !F) return set_err(BMM_E_ARG, "null argument");
    *F = c->cat_on ? (int)c->cat_levels.size() : 0;
    if (levels && c->cat_on) std::memcpy(levels, c->cat_levels.data(), c->cat_levels.size() * sizeof(int32_t));
    return BMM_OK;
}

// The column map and the kernel form of a shape, without a device: first_column (or null) F entries, lev (or null) P
// bytes as k_count_tables<TAB_CAT> reads them.  The form is the last one plan_kernel offers on num_cus compute units.
int bmm_categorical_plan(int sampler, int64_t N, int K, int64_t batch, int num_cus, const int32_t* levels, int F,
                         int32_t* first_column, uint8_t* lev_out, bmm_categorical_plan_out* out) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    if (sampler != BMM_SAMPLER_COLLAPSED && sampler != BMM_SAMPLER_DP)
        return set_err(BMM_E_UNSUPPORTED, "categorical features are offered for the collapsed and DP samplers only");
    if (N < 1 || K < 1 || num_cus < 1 || F < 1 || !levels) return set_err(BMM_E_ARG, "bmm_categorical_plan: N, K, num_cus, F >= 1");
    int64_t P64 = 0;
    for (int f = 0; f < F; ++f) P64 += levels[f] < 1 ? 1 : levels[f];
    if (P64 > (1 << 24)) return set_err(BMM_E_ARG, "categorical: too many columns");
    const int P = (int)P64;
    std::vector<uint8_t> lev;
    std::vector<CatBlock> blocks;
    int rc = cat_map(levels, F, P, &lev, &blocks, first_column);
    if (rc) return rc;
    if (lev_out) std::memcpy(lev_out, lev.data(), lev.size());
    const DebugSwitches dbg;
    const ChainShape s = chain_shape(sampler, N, P, K, batch, dbg);
    *out = bmm_categorical_plan_out{};
    out->n_columns = P;
    out->n_blocks = (int32_t)blocks.size();
    out->generic = s.generic ? 1 : 0;
    out->batch = s.batch;
    if (s.generic) {
        out->threads = 256; out->lanes = 1;
        return BMM_OK;
    }
    const KernelPlan plan = plan_kernel(s.p, true, s.minus_in_lds ? 1 : 2, s.batch, num_cus, false, s.lds_bytes_base, dbg, false, true);
    const KernelForm& f = plan.form[plan.n - 1];
    out->threads = f.nt; out->lanes = f.lanes; out->packed = f.pk ? 1 : 0; out->builds_own_tables = f.self ? 1 : 0;
    return BMM_OK;
}

// ... of a run: armed for it (bmm_set_categorical), refused before a device is touched
static int cat_run_check(const RunOptions& o, int sampler, int P) {
    if (!o.cat.on) return BMM_OK;
    const int rc = cat_map(o.cat.levels.data(), (int)o.cat.levels.size(), P, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (dbg_env("BMM_X_LAYOUT_INT32") != nullptr) return set_err(BMM_E_UNSUPPORTED, "categorical features read the bit planes: not offered on the int32 layout");
    if (explicit_params(sampler))
        return set_err(BMM_E_UNSUPPORTED, "categorical features are offered for the collapsed and DP samplers only: the stick-breaking "
                       "and full samplers carry a Bernoulli theta per column");
    if (o.alloc.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered by the allocation sampler");
    if (o.temper.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with parallel tempering");
    if (o.fs.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with feature selection");
    if (o.sm.moves > 0) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with split-merge moves: their ratio knows the Bernoulli cell only");
    if (o.na.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with missing cells: the imputation step knows the Bernoulli cell only");
    if (o.pred) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with newdata: the predictive tables know the Bernoulli cell only");
    if (o.loo.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the leave-one-out summary: its tables know the Bernoulli cell only");
    if (o.logpost.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the log joint trace: its cells are Bernoulli cells");
    if (o.pc.on) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with the pair check: the columns of a block depend on each other by construction");
    if (o.init.kind != 0) return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with a device start (init_labels): its distance counts a block's columns one by one");
    if (o.hooks || o.rel)
        return set_err(BMM_E_UNSUPPORTED, "categorical features are not offered together with a probability hand-off (relabel = TRUE); ECR reads the labels alone");
    return BMM_OK;
}
static int cat_run_attach(bmm_chain* c, const RunOptions& o) {
    return o.cat.on ? bmm_chain_set_categorical(c, o.cat.levels.data(), (int)o.cat.levels.size()) : BMM_OK;
}

// ---- parallel tempering: a replica ladder (include/bmm_mcmc.h "parallel tempering") ----
// who may be a rung
static int temper_refused(const bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (c->na_on) return na_refuses("parallel tempering");
    if (c->cs_on) return cs_refuses("parallel tempering");
    if (c->cat_on) return cat_refuses("parallel tempering");
    if (c->sum_on) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered on a chain with an armed summary");
    if (explicit_params(c->p.mode))
        return set_err(BMM_E_UNSUPPORTED, "parallel tempering is offered for the collapsed and DP samplers only: the stick-breaking "
                       "and full samplers carry theta, and the power sits on the likelihood with theta integrated out");
    if (c->alloc_on) return alloc_refuses("parallel tempering");
    if (c->fs_mask) return fs_mask_refuses("parallel tempering");
    if (c->sm_moves > 0) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered together with split-merge moves: their ratio would need the tempered likelihood");
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered on a sharded chain");
    return BMM_OK;
}

int bmm_chain_set_temper(bmm_chain* c, int on, double inv_temp) {
    return guarded([&]() -> int {
        int rc = temper_refused(c);
        if (rc) return rc;
        if (on && !(inv_temp > 0.0 && inv_temp <= 1.0)) return set_err(BMM_E_ARG, "inv_temp must lie in (0, 1]");
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        const bool was = c->temper_on;
        c->temper_on = on != 0;
        c->temper_b = on ? inv_temp : 1.0;
        if (was == c->temper_on || c->generic) return BMM_OK;
        return pick_kernel(c);  // again: without, or once more with, the forms a tempered chain leaves out
    });
}

int bmm_chain_get_temper(const bmm_chain* c, int* on, double* inv_temp) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    if (on) *on = c->temper_on ? 1 : 0;
    if (inv_temp) *inv_temp = c->temper_b;
    return BMM_OK;
}

}  // extern "C"

struct bmm_ladder {
    int R = 0, device = 0;
    bmm_chain* ch[kTemperMaxR] = {};
    uint64_t seed = 0;
    uint32_t t = 0;  // exchange points so far
    char* dBlock = nullptr;
    int32_t *dAccept = nullptr, *dWalker = nullptr;
    long long* dCounters = nullptr;
    TemperStep* dRec = nullptr;
    hipEvent_t ready[kTemperMaxR] = {};  // rung r has scored its state
    hipEvent_t done = nullptr;           // the exchange is over
    // a run's recordings (device; owned by the run): [S][R] log_lik rows and [S] walkers at rung 0, row s = sweep - base
    double* lik_rows = nullptr;
    int32_t* walker_rows = nullptr;
    int base = 0, swap_every = 1;
};

namespace {

// One exchange point, enqueued: every rung scores its state on its own stream (the keep-best cell untouched), rung 0's
// stream waits for them, decides and exchanges, the others wait for that.  Nothing blocks the host.
int ladder_exchange(bmm_ladder* l, double* lik_row) {
    const int R = l->R;
    bmm_chain* const c0 = l->ch[0];
    if (R < 2 && !lik_row) return BMM_OK;
    TemperArgs a{};
    for (int r = 0; r < R; ++r) {
        bmm_chain* const c = l->ch[r];
        int rc = lp_setup(c, false);
        if (rc) return rc;
        LjArgs lj = lj_args(c);
        lj.out_row = nullptr; lj.sweep = c->sweep; lj.fold = 0;
        rc = launch_log_joint(c, lj);
        if (rc) return rc;
        if (r > 0) HIP_TRY(hipEventRecord(l->ready[r], c->stream));
        TemperRung& g = a.rung[r];
        g.lj_out = c->dLjOut; g.z = label_row(c, c->sweep); g.Nk = c->dNk; g.S = c->dS; g.dNk = c->dDNk; g.dS = c->dDS;
        g.alpha = c->dAlpha; g.b = c->temper_on ? c->temper_b : 1.0;
    }
    for (int r = 1; r < R; ++r) HIP_TRY(hipStreamWaitEvent(c0->stream, l->ready[r], 0));
    a.R = R; a.t = l->t; a.seed = l->seed; a.accept = l->dAccept; a.walker = l->dWalker; a.counters = l->dCounters;
    a.rec = l->dRec; a.lik_row = lik_row; a.N = c0->p.N; a.K = c0->p.K; a.P = c0->p.P;
    hipLaunchKernelGGL(k_temper_decide, dim3(1), dim3(64), 0, c0->stream, a);
    HIP_TRY(hipGetLastError());
    const int pairs = (R - (int)(l->t & 1u)) / 2;  // r = t mod 2, then every other one, while r + 1 < R
    if (pairs > 0) {
        const int64_t nb = (c0->p.N + 4 * kTemperThreads - 1) / (4 * kTemperThreads);
        hipLaunchKernelGGL(k_temper_exchange, dim3((unsigned)(nb < 256 ? nb : 256), (unsigned)pairs), dim3(kTemperThreads), 0,
                           c0->stream, a);
        HIP_TRY(hipGetLastError());
        // rung 0's kept row of a run: theta-hat and alpha of the state it holds now (nothing is pending behind a
        // sweep end, and the concentration is not drawn again)
        if (c0->in_run && c0->sweep >= c0->burnin && c0->sweep >= 1 && (l->t & 1u) == 0) {
            ChainParams q = c0->p;
            q.sample_alpha = 0;
            const int s = c0->sweep - c0->burnin;
            hipLaunchKernelGGL(k_count_sweep_end, dim3(1), dim3(1024), 0, c0->stream, q, c0->dNk, c0->dS, c0->dDNk, c0->dDS,
                               c0->dAlpha, (uint32_t)c0->sweep, c0->dThetaTrace + (size_t)s * q.K * q.P, c0->dAlphaTrace + s,
                               (int32_t*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(l->done, c0->stream));
        for (int r = 1; r < R; ++r) HIP_TRY(hipStreamWaitEvent(l->ch[r]->stream, l->done, 0));
    }
    l->t++;
    return BMM_OK;
}

int ladder_same_sweep(const bmm_ladder* l) {
    for (int r = 1; r < l->R; ++r)
        if (l->ch[r]->sweep != l->ch[0]->sweep)
            return set_err(BMM_E_STATE, "rung %d is at sweep %d, rung 0 at sweep %d: the rungs of a ladder advance together", r, l->ch[r]->sweep, l->ch[0]->sweep);
    return BMM_OK;
}

// n sweeps of every rung with an exchange point behind every sweep whose index is a multiple of swap_every
int ladder_sweeps(bmm_ladder* l, int n, int swap_every) {
    if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
    if (swap_every < 1) return set_err(BMM_E_ARG, "swap_every must be >= 1");
    int rc = ladder_same_sweep(l);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(l->device));
    bmm_chain* const c0 = l->ch[0];
    for (int r = 0; r < l->R; ++r)
        if (!l->ch[r]->started) { rc = chain_start(l->ch[r]); if (rc) return rc; }
    for (int t = 0; t < n; ++t) {
        const int j = c0->sweep + 1;
        const bool point = j % swap_every == 0;
        c0->fold_defer = point && l->R > 1;
        for (int r = 0; r < l->R && rc == BMM_OK; ++r) {
            rc = enqueue_sweep(l->ch[r], j);
            if (rc == BMM_OK) l->ch[r]->sweep++;
        }
        const bool deferred = std::exchange(c0->fold_defer, false);
        if (rc) return rc;
        const bool kept = l->lik_rows && j >= l->base;
        if (point) {
            rc = ladder_exchange(l, kept ? l->lik_rows + (size_t)(j - l->base) * l->R : nullptr);
            if (rc == BMM_OK && deferred && c0->lp_rec.folds(j) && c0->lp_on) rc = enqueue_log_joint(c0, j, c0->lp_rec.row<double>(j), true);
            if (rc == BMM_OK && deferred && pc_folds(c0, j)) rc = enqueue_pair_check(c0, label_row(c0, j), c0->pc_rec.row<double>(j), true);
            if (rc) return rc;
        }
        if (l->walker_rows && j >= l->base)
            HIP_TRY(hipMemcpyAsync(l->walker_rows + (j - l->base), l->dWalker, sizeof(int32_t), hipMemcpyDeviceToDevice, c0->stream));
    }
    return BMM_OK;
}

int ladder_sync(bmm_ladder* l) {
    HIP_TRY(hipSetDevice(l->device));
    for (int r = 0; r < l->R; ++r) HIP_TRY(hipStreamSynchronize(l->ch[r]->stream));
    return BMM_OK;
}

}  // namespace

extern "C" {

int bmm_ladder_create(bmm_ladder** out, bmm_chain* const* chains, int R, uint64_t seed) {
    return guarded([&]() -> int {
        if (!out || !chains) return set_err(BMM_E_ARG, "null argument");
        *out = nullptr;
        if (R < 1 || R > kTemperMaxR) return set_err(BMM_E_ARG, "a ladder has 1 to %d rungs", kTemperMaxR);
        for (int r = 0; r < R; ++r) {
            const bmm_chain* c = chains[r];
            if (!c) return set_err(BMM_E_ARG, "rung %d: null chain", r);
            for (int q = 0; q < r; ++q)
                if (chains[q] == c) return set_err(BMM_E_ARG, "rung %d: the chain is rung %d already", r, q);
            if (temper_refused(c)) {
                const std::string why = g_err;
                return set_err(BMM_E_UNSUPPORTED, "rung %d: %s", r, why.c_str());
            }
            if (c->in_run && r > 0) return set_err(BMM_E_STATE, "rung %d: the chain is inside a run", r);
            if (c->ladder && r > 0) return set_err(BMM_E_STATE, "rung %d: the chain is rung 0 of a run's ladder", r);
        }
        const bmm_chain* c0 = chains[0];
        if (c0->temper_on && c0->temper_b != 1.0) return set_err(BMM_E_ARG, "rung 0: the first chain runs at inverse temperature 1 (unarmed, or armed with 1.0)");
        double prev = 1.0;
        for (int r = 1; r < R; ++r) {
            const bmm_chain* c = chains[r];
            if (!c->temper_on) return set_err(BMM_E_STATE, "rung %d: the chain is not armed (bmm_chain_set_temper)", r);
            if (!(c->temper_b < prev)) return set_err(BMM_E_ARG, "rung %d: the inverse temperatures must decrease strictly (%.17g after %.17g)", r, c->temper_b, prev);
            prev = c->temper_b;
            if (c->slot != c0->slot || c->device != c0->device) return set_err(BMM_E_UNSUPPORTED, "rung %d: the rungs of a ladder live on one device", r);
            const ChainParams &p = c->p, &p0 = c0->p;
            if (p.mode != p0.mode) return set_err(BMM_E_ARG, "rung %d: another sampler than rung 0's", r);
            if (p.N != p0.N || p.P != p0.P || p.K != p0.K) return set_err(BMM_E_ARG, "rung %d: N, P or K differ from rung 0's", r);
            if (p.beta != p0.beta || p.gamma != p0.gamma || p.a != p0.a || p.b != p0.b || p.sample_alpha != p0.sample_alpha)
                return set_err(BMM_E_ARG, "rung %d: beta, gamma, a, b or the treatment of alpha differ from rung 0's", r);
            if (c->batch != c0->batch) return set_err(BMM_E_ARG, "rung %d: batch %lld, rung 0 has %lld", r, (long long)c->batch, (long long)c0->batch);
            if (c->sweep != c0->sweep) return set_err(BMM_E_STATE, "rung %d: at sweep %d, rung 0 at sweep %d", r, c->sweep, c0->sweep);
            if (!c->have_data || !c0->have_data) return set_err(BMM_E_STATE, "rung %d: no data yet", r);
            if (c->bits != c0->bits || (c->bits ? c->dXb != c0->dXb : c->dX != c0->dX))
                return set_err(BMM_E_STATE, "rung %d: the rungs of a ladder share one copy of the data (bmm_chain_share_data)", r);
        }
        HIP_TRY(hipSetDevice(c0->device));
        std::unique_ptr<bmm_ladder, void (*)(bmm_ladder*)> l(new bmm_ladder(), bmm_ladder_destroy);
        l->R = R; l->device = c0->device; l->seed = seed;
        for (int r = 0; r < R; ++r) l->ch[r] = chains[r];
        auto carve = [&](Carver& v) {
            l->dCounters = v.take<long long>(2 * (size_t)kTemperMaxR);
            l->dRec = v.take<TemperStep>((size_t)kTemperMaxR);
            l->dAccept = v.take<int32_t>((size_t)kTemperMaxR);
            l->dWalker = v.take<int32_t>((size_t)kTemperMaxR);
        };
        Carver measure{nullptr};
        carve(measure);
        HIP_TRY(hipMalloc(&l->dBlock, measure.used));
        Carver real{l->dBlock};
        carve(real);
        HIP_TRY(hipMemset(l->dBlock, 0, measure.used));
        int32_t w[kTemperMaxR];
        for (int r = 0; r < kTemperMaxR; ++r) w[r] = r;
        HIP_TRY(hipMemcpy(l->dWalker, w, sizeof w, hipMemcpyHostToDevice));
        for (int r = 1; r < R; ++r) HIP_TRY(hipEventCreateWithFlags(&l->ready[r], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&l->done, hipEventDisableTiming));
        *out = l.release();
        return BMM_OK;
    });
}

void bmm_ladder_destroy(bmm_ladder* l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    for (int r = 0; r < l->R; ++r)
        if (l->ch[r] && l->ch[r]->stream) (void)hipStreamSynchronize(l->ch[r]->stream);
    for (hipEvent_t e : l->ready) if (e) (void)hipEventDestroy(e);
    if (l->done) (void)hipEventDestroy(l->done);
    if (l->dBlock) (void)hipFree(l->dBlock);
    delete l;
}

int bmm_ladder_sweeps(bmm_ladder* l, int n, int swap_every) {
    return guarded([&]() -> int {
        if (!l) return set_err(BMM_E_ARG, "null ladder");
        return ladder_sweeps(l, n, swap_every);
    });
}

int bmm_ladder_exchange_step(bmm_ladder* l, bmm_exchange_step* out) {
    return guarded([&]() -> int {
        if (!l) return set_err(BMM_E_ARG, "null ladder");
        int rc = ladder_same_sweep(l);
        if (rc == BMM_OK) rc = lp_seated(l->ch[0]);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(l->device));
        for (int r = 0; r < l->R; ++r)
            if (!l->ch[r]->started) { rc = chain_start(l->ch[r]); if (rc) return rc; }
        const uint32_t t = l->t;
        rc = ladder_exchange(l, nullptr);
        const int rs = ladder_sync(l);
        if (rc || rs) return rc ? rc : rs;
        if (out && l->R > 1) {
            TemperStep h[kTemperMaxR];
            HIP_TRY(hipMemcpy(h, l->dRec, (size_t)(l->R - 1) * sizeof(TemperStep), hipMemcpyDeviceToHost));
            for (int r = 0; r + 1 < l->R; ++r) {
                out[r].d = h[r].d; out[r].u = h[r].u; out[r].proposed = h[r].proposed; out[r].accepted = h[r].accepted;
                out[r].point = (int32_t)t; out[r].pad = 0;
            }
        }
        return BMM_OK;
    });
}

int bmm_ladder_stats(bmm_ladder* l, int64_t* proposed, int64_t* accepted, int32_t* walker) {
    return guarded([&]() -> int {
        if (!l) return set_err(BMM_E_ARG, "null ladder");
        int rc = ladder_sync(l);
        if (rc) return rc;
        long long h[2 * kTemperMaxR];
        HIP_TRY(hipMemcpy(h, l->dCounters, sizeof h, hipMemcpyDeviceToHost));
        for (int r = 0; r + 1 < l->R; ++r) {
            if (proposed) proposed[r] = h[r];
            if (accepted) accepted[r] = h[l->R - 1 + r];
        }
        if (walker) HIP_TRY(hipMemcpy(walker, l->dWalker, (size_t)l->R * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------ *_run entry points
namespace {

struct RunIO {
    const int32_t* z0 = nullptr;
    const double *pi0 = nullptr, *theta0 = nullptr;
    double* pi_out = nullptr;
    int32_t* z_out = nullptr;
    double *theta_out = nullptr, *alpha_out = nullptr;
};
// ... of a counting sampler (z0: the finite one's initial labels, null for the DP sampler) and of one that carries pi and theta
RunIO counting_io(const int32_t* z0, int32_t* z_out, double* theta_out, double* alpha_out) {
    return RunIO{z0, nullptr, nullptr, nullptr, z_out, theta_out, alpha_out};
}
RunIO explicit_io(const double* pi0, const double* theta0, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out) {
    return RunIO{nullptr, pi0, theta0, pi_out, z_out, theta_out, alpha_out};
}
// the options of a call with hooks, with relabelling on the device, with the predictive of new rows
RunOptions with_hooks(RunOptions o, const bmm_relabel_hooks* hooks) { o.hooks = hooks; return o; }
RunOptions with_relabel(RunOptions o, const bmm_relabel_out* rel) { o.rel = rel; return o; }
RunOptions with_predict(RunOptions o, const int32_t* Xnew, int64_t M, const bmm_predict_out* pred) {
    o.hooks = pred->hooks; o.rel = pred->relabel; o.Xnew = Xnew; o.M = M; o.pred = pred;
    return o;
}

// Blocks of the outgoing label trace (trace_out): a whole number of observations, at most a staging piece
size_t out_block_rows(int S, size_t el, int64_t N) {
    int64_t B = (int64_t)(kStageBytes / ((size_t)S * el));
    B = B / 32 * 32;
    if (B < 32) B = 32;
    return (size_t)(B > N ? N : B);
}

// buffers of a *_run call: the traces and, for a run that keeps its label trace, that trace and the two device blocks
// of its way out.  A pure function of (sampler, N, P, K, S, keep_trace): run_prepare carves with it and bmm_run_bytes
// measures with it.
struct RunBufs {
    double *theta = nullptr, *alpha = nullptr, *pi = nullptr;
    char* out_blk[2] = {nullptr, nullptr};
    size_t out_blk_bytes = 0;
    int32_t* trace = nullptr;
};
RunBufs run_carve(Carver& a, int sampler, int64_t N, int P, int K, int S, bool keep_trace) {
    RunBufs b;
    b.theta = a.take<double>((size_t)S * K * P);
    b.alpha = a.take<double>((size_t)S);
    b.pi = explicit_params(sampler) ? a.take<double>((size_t)S * K) : nullptr;
    (void)a.take<char>(0);  // (the small traces end on a carving boundary: what the label trace adds is its own bytes)
    if (!keep_trace) return b;
    const size_t el = K <= 254 ? 1 : 4;
    b.out_blk_bytes = out_block_rows(S, el, N) * (size_t)S * el;
    b.out_blk[0] = a.take<char>(b.out_blk_bytes);
    b.out_blk[1] = a.take<char>(b.out_blk_bytes);
    b.trace = a.take<int32_t>((size_t)S * N);
    return b;
}
// ... one allocation (owned by the chain, released with it)
int run_prepare(bmm_chain* c, int nsamples, int burnin, bool keep_trace = true) {
    const int64_t N = c->p.N;
    const int K = c->p.K, P = c->p.P;
    const int S = nsamples - burnin;
    c->burnin = burnin; c->S = S;
    c->in_run = true;
    HIP_TRY(hipSetDevice(c->device));
    Carver measure{nullptr};
    (void)run_carve(measure, c->p.mode, N, P, K, S, keep_trace);
    c->run_arena = static_cast<char*>(dev_pool().get(c->device, measure.used, &c->run_arena_bytes));
    if (!c->run_arena) return set_err(BMM_E_HIP, "allocating the run's buffers failed: %s", hipGetErrorString(hipGetLastError()));
    Carver real{c->run_arena};
    const RunBufs b = run_carve(real, c->p.mode, N, P, K, S, keep_trace);
    c->dThetaTrace = b.theta; c->dAlphaTrace = b.alpha; c->dPiTrace = b.pi;
    c->dOutBlk[0] = b.out_blk[0]; c->dOutBlk[1] = b.out_blk[1]; c->out_blk_bytes = b.out_blk_bytes;
    c->dTrace = b.trace;
    return BMM_OK;
}

// ---- Stephens' relabelling on the device (src/stephens.cpp as it executes) ----
// Workspace of one relabelling: the per-workgroup partial cost matrices, the K x K costs, Q (and log Q for the
// batch), the batch's M x K permutation table.  Everything is stream-ordered: no host round trip.
constexpr size_t kStPartialBudget = (size_t)64 << 20;  // bytes of partial cost matrices at most
constexpr int kStBatchIters = 100;  // stephens.cpp:25; its threshold (10^(-6) = -16, :24) never stops the loop

// workgroups of the cost pass over N rows for `slices` slices: a function of (N, K, slices) only, so that a
// shape always sums in the same order
int st_groups(int64_t N, int K, int slices) {
    int64_t G = (N + 511) / 512;
    const int64_t cap_wg = slices > 1 ? (1024 + slices - 1) / slices : 1024;
    int64_t cap_mem = (int64_t)(kStPartialBudget / ((size_t)slices * K * K * sizeof(double)));
    if (G > cap_wg) G = cap_wg;
    if (G > cap_mem) G = cap_mem;
    return (int)(G < 1 ? 1 : G);
}
// rows of p per workgroup of the cost pass
int64_t st_rows(int64_t N, int G) { return (N + G - 1) / G; }

struct StWork {
    int64_t N = 0;
    int K = 0, M = 0, G1 = 0, GM = 0;
    DevBuf partial, cost, Q, LQ, permb;
    size_t bytes() const {  // what alloc() takes
        const size_t nk = (size_t)N * K * sizeof(double), kk = (size_t)K * K * sizeof(double);
        const size_t g = (size_t)(GM * (M > 0 ? M : 1) > G1 ? GM * (M > 0 ? M : 1) : G1);
        return g * kk + (size_t)(M > 1 ? M : 1) * kk + nk * (M > 0 ? 2 : 1) + (size_t)M * K * sizeof(int32_t);
    }
    void shape(int64_t n, int k, int m) {
        N = n; K = k; M = m;
        G1 = st_groups(N, K, 1);
        GM = m > 0 ? st_groups(N, K, m) : 0;
    }
    int alloc() {
        const size_t nk = (size_t)N * K * sizeof(double), kk = (size_t)K * K * sizeof(double);
        const size_t g = (size_t)(GM * (M > 0 ? M : 1) > G1 ? GM * (M > 0 ? M : 1) : G1);
        HIP_TRY(partial.alloc(g * kk));
        HIP_TRY(cost.alloc((size_t)(M > 1 ? M : 1) * kk));
        HIP_TRY(Q.alloc(nk));
        if (M > 0) {
            HIP_TRY(LQ.alloc(nk));
            HIP_TRY(permb.alloc((size_t)M * K * sizeof(int32_t)));
        }
        return BMM_OK;
    }
};

int st_check_k(int K) {
    if (K < 1 || K > kStephensMaxK)
        return set_err(BMM_E_ARG, "Stephens relabelling on the device supports 1 <= K <= %d categories (K = %d)",
                       kStephensMaxK, K);
    return BMM_OK;
}

// cost matrices of `slices` slices of p (slice_stride apart) against q (or log q) into w.cost
int st_cost(hipStream_t st, StWork& w, const double* p, int64_t slice_stride, int slices, const double* q,
            bool q_is_log, bool batch_form) {
    const int K = w.K, G = slices > 1 ? w.GM : w.G1;
    const int64_t rows = st_rows(w.N, G);
    const int B = st_cost_b(K);
    const dim3 grid((unsigned)G, (unsigned)slices);
    const size_t lds = st_cost_lds(K);
    double* part = w.partial.as<double>();
    switch (B) {
        case 1: hipLaunchKernelGGL(k_st_cost_partial<1>, grid, dim3(256), lds, st, p, w.N, K, slice_stride, q, (int)q_is_log, (int)batch_form, rows, part); break;
        case 2: hipLaunchKernelGGL(k_st_cost_partial<2>, grid, dim3(256), lds, st, p, w.N, K, slice_stride, q, (int)q_is_log, (int)batch_form, rows, part); break;
        case 3: hipLaunchKernelGGL(k_st_cost_partial<3>, grid, dim3(256), lds, st, p, w.N, K, slice_stride, q, (int)q_is_log, (int)batch_form, rows, part); break;
        default: hipLaunchKernelGGL(k_st_cost_partial<4>, grid, dim3(256), lds, st, p, w.N, K, slice_stride, q, (int)q_is_log, (int)batch_form, rows, part); break;
    }
    HIP_TRY(hipGetLastError());
    const int KK = K * K;
    hipLaunchKernelGGL(k_st_cost_reduce, dim3((unsigned)((KK + 63) / 64), (unsigned)slices), dim3(256), 0, st, part, G, KK,
                       w.cost.as<double>());
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

int st_assign(hipStream_t st, const double* cost, int K, int slices, int32_t* perm, int64_t ld) {
    const size_t lds = st_assign_lds(K);
    const int in_lds = st_assign_in_lds(K);
    hipLaunchKernelGGL(k_st_assign, dim3((unsigned)slices), dim3(64), lds, st, cost, K, perm, ld, in_lds);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

unsigned st_grid(int64_t n) { return (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

// my_stephens_batch (stephens.cpp:6-66) over the window p (N x K x M, modified in place: zeros -> 1e-6), enqueued:
// w.Q receives the Q of the last iteration's start, w.LQ its log, w.permb the last iteration's permutations
int st_batch(hipStream_t st, StWork& w, double* p) {
    const int64_t N = w.N, NK = N * w.K;
    const int K = w.K, M = w.M;
    hipLaunchKernelGGL(k_st_replace_zeros, dim3(st_grid(NK * M)), dim3(256), 0, st, p, NK * M);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_st_perm_identity, dim3((unsigned)((M * K + 255) / 256)), dim3(256), 0, st, w.permb.as<int32_t>(), M, K);
    HIP_TRY(hipGetLastError());
    for (int t = 0; t < kStBatchIters; ++t) {
        hipLaunchKernelGGL(k_st_q_batch, dim3(st_grid(NK)), dim3(256), 0, st, p, N, K, M, w.permb.as<int32_t>(),
                           w.Q.as<double>(), w.LQ.as<double>());
        HIP_TRY(hipGetLastError());
        int rc = st_cost(st, w, p, NK, M, w.LQ.as<double>(), true, true);
        if (rc == BMM_OK) rc = st_assign(st, w.cost.as<double>(), K, M, w.permb.as<int32_t>(), M);
        if (rc) return rc;
    }
    return BMM_OK;
}

// my_stephens_online (stephens.cpp:68-94) for sweep j, enqueued: perm -> perm[0], perm[ld], ..; w.Q updated in place
int st_online(hipStream_t st, StWork& w, const double* p, int j, int32_t* perm, int64_t ld) {
    int rc = st_cost(st, w, p, 0, 1, w.Q.as<double>(), false, false);
    if (rc == BMM_OK) rc = st_assign(st, w.cost.as<double>(), w.K, 1, perm, ld);
    if (rc) return rc;
    hipLaunchKernelGGL(k_st_q_online, dim3(st_grid(w.N * w.K)), dim3(256), 0, st, w.Q.as<double>(), p, w.N, w.K, perm, ld,
                       (double)j, (double)(j + 1));
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}

// The sweeps of a relabel = TRUE run with Stephens on the device (collapsed_gibbs.cpp:160-201): the window's
// matrices go into a device ring, the batch runs after sweep burnin - 1, every kept sweep's matrix feeds the online
// step, whose permutation lands in row j - burnin of the S x K device table dPerm.  All of it is enqueued ahead
// of the device as the plain sweeps are.
struct StRun {
    StWork w;
    DevBuf ring, dbuf, perm;  // one matrix buffer: the online step of sweep j is stream-ordered before sweep j + 1
    int W = 0;
};

int st_run_prepare(bmm_chain* c, StRun& r, int W) {
    const int64_t N = c->p.N;
    const int K = c->p.K;
    if (c->burnin < 2 || W < 1)
        return set_err(BMM_E_ARG, "relabel on the device needs the batch step, which the reference runs only with "
                       "burnin >= 2 and burnrelabel >= 1 (burnin = %d, burnrelabel = %d)", c->burnin, W);
    int rc = st_check_k(K);
    if (rc) return rc;
    r.W = W;
    r.w.shape(N, K, W);
    const size_t mat = (size_t)N * K * sizeof(double);
    const size_t need = mat * (size_t)W + mat + r.w.bytes() + (size_t)c->S * K * sizeof(int32_t);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        return set_err(BMM_E_ARG, "relabel on the device: the batch window (%d sweeps of N x K = %lld x %d doubles) and "
                       "its workspace need %zu bytes of device memory, %zu are free", W, (long long)N, K, need, free_b);
    rc = probs_alloc(c, false);
    if (rc) return rc;
    if (r.ring.alloc(mat * (size_t)W) != hipSuccess || r.dbuf.alloc(mat) != hipSuccess || r.perm.alloc((size_t)c->S * K * sizeof(int32_t)) != hipSuccess)
        return set_err(BMM_E_ARG, "relabel on the device: allocating %zu bytes of device memory failed", need);
    rc = r.w.alloc();
    if (rc) return rc;
    // slices of sweeps j < 1 (a window longer than the burn-in) stay zero, as arma::fill::zeros leaves them
    HIP_TRY(hipMemsetAsync(r.ring.p, 0, mat * (size_t)W, c->stream));
    return BMM_OK;
}

// one sweep j of a relabelling run, with its share of Stephens
int st_run_sweep(bmm_chain* c, StRun& r, int j) {
    const int64_t N = c->p.N;
    const int burnin = c->burnin, first_window = burnin - r.W;
    const size_t mat = (size_t)N * c->p.K;
    const bool window = j >= first_window && j < burnin;
    if (window) c->probs_dst = r.ring.as<double>() + (size_t)(j - first_window) * mat;
    else if (j >= burnin) c->probs_dst = r.dbuf.as<double>();
    else c->probs_dst = nullptr;
    int rc = bmm_chain_sweeps(c, 1);
    c->probs_dst = nullptr;
    if (rc) return rc;
    if (j == burnin - 1) return st_batch(c->stream, r.w, r.ring.as<double>());
    if (j >= burnin) return st_online(c->stream, r.w, r.dbuf.as<double>(), j, r.perm.as<int32_t>() + (j - burnin), c->S);
    return BMM_OK;
}

// The sweeps of a run whose allocation probabilities go to the host's relabelling code
// (collapsed_gibbs.cpp:162-172, 187-201): sweeps burnin - burnrelabel .. burnin - 1 fill the batch
// cube (through a device ring when it fits, so that those sweeps need no host round trip), then
// every kept sweep hands its N x K matrix to on_sample -- two device and two pinned host buffers,
// so that sweep j + 1 runs while the host works on sweep j.
int run_sweeps_hooked(bmm_chain* c, int nsamples, const bmm_relabel_hooks* h) {
    const int64_t N = c->p.N;
    const int K = c->p.K, burnin = c->burnin;
    const size_t mat = (size_t)N * K, mat_bytes = mat * sizeof(double);
    // the cube has burnrelabel slices, sweep j in slice j - burnin + burnrelabel (collapsed_gibbs.cpp:163-166);
    // slices of sweeps that do not exist (j < 1: a window longer than the burn-in, which only the
    // stick-breaking wrapper lets through, R/utils.R:97-101) stay zero, as arma::fill::zeros leaves them
    const int W = h->burnrelabel < 0 ? 0 : h->burnrelabel;
    if (W > 0 && !h->probs_batch) return set_err(BMM_E_ARG, "relabel hooks: probs_batch is null");
    const int first_window = burnin - W;  // sweep of slice 0
    for (int q = 0; q < W && q + first_window < 1; ++q) std::memset(h->probs_batch + (size_t)q * mat, 0, mat_bytes);
    int rc = probs_alloc(c, false);
    if (rc) return rc;
    // device ring for the batch window when it takes at most half of the free memory
    DevBuf ring;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const bool use_ring = W > 0 && mat_bytes * (size_t)W <= free_b / 2;
    if (use_ring) {
        HIP_TRY(ring.alloc(mat_bytes * (size_t)W));
        HIP_TRY(hipMemsetAsync(ring.p, 0, mat_bytes * (size_t)W, c->stream));
    }
    DevBuf dbuf[2];
    double* hbuf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Pinned { double** h; hipEvent_t* e; ~Pinned() { for (int q = 0; q < 2; ++q) { if (h[q]) (void)hipHostFree(h[q]); if (e[q]) (void)hipEventDestroy(e[q]); } } } pin{hbuf, ev};
    for (int q = 0; q < 2; ++q) {
        HIP_TRY(dbuf[q].alloc(mat_bytes));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&hbuf[q]), mat_bytes, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
    }
    int pending = -1;  // sweep whose matrix is on its way to hbuf[pending & 1]
    auto deliver = [&](int jj) -> int {
        HIP_TRY(hipEventSynchronize(ev[jj & 1]));
        if (jj < burnin) {  // a window sweep without the ring: straight into the cube
            std::memcpy(h->probs_batch + (size_t)(jj - first_window) * mat, hbuf[jj & 1], mat_bytes);
            return BMM_OK;
        }
        if (h->on_sample && h->on_sample(h->user, jj, hbuf[jj & 1]) != 0)
            return set_err(BMM_E_CALLBACK, "relabel hook on_sample stopped the run at sweep %d", jj);
        return BMM_OK;
    };
    for (int j = 1; j < nsamples; ++j) {
        const bool window = j >= first_window && j < burnin;
        const bool keep = j >= burnin && h->on_sample;
        if (window && use_ring) c->probs_dst = ring.as<double>() + (size_t)(j - first_window) * mat;
        else if (window || keep) c->probs_dst = dbuf[j & 1].as<double>();
        else c->probs_dst = nullptr;
        rc = bmm_chain_sweeps(c, 1);
        const bool staged = c->probs_dst && !(window && use_ring);
        c->probs_dst = nullptr;
        if (rc) return rc;
        // progress of a run that feeds the host's relabelling: as the sweeps are enqueued (the hand-off keeps the
        // host within a sweep of the device from the window on); the cluster count is not fetched here
        if (g_progress.fn && g_progress.every > 0 && (j % g_progress.every == 0 || j == nsamples - 1) &&
            g_progress.fn(g_progress.user, j + 1, nsamples, -1) != 0) {
            (void)hipStreamSynchronize(c->stream);
            return set_err(BMM_E_CALLBACK, "the progress hook stopped the run after sample %d", j + 1);
        }
        if (staged) {
            HIP_TRY(hipMemcpyAsync(hbuf[j & 1], dbuf[j & 1].p, mat_bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipEventRecord(ev[j & 1], c->stream));
        }
        if (pending >= 0) { rc = deliver(pending); pending = -1; if (rc) return rc; }
        if (staged) pending = j;
        if (j == burnin - 1) {  // collapsed_gibbs.cpp:188-190
            if (pending >= 0) { rc = deliver(pending); pending = -1; if (rc) return rc; }
            if (use_ring) {  // slices of sweeps j < 1 arrive as the zeros the ring was filled with
                HIP_TRY(hipMemcpyAsync(h->probs_batch, ring.p, mat_bytes * (size_t)W, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
            }
            if (h->batch_done && h->batch_done(h->user, j, h->probs_batch) != 0)
                return set_err(BMM_E_CALLBACK, "relabel hook batch_done stopped the run");
        }
    }
    if (pending >= 0) { rc = deliver(pending); if (rc) return rc; }
    return BMM_OK;
}

// One-byte labels widened into the caller's int32 trace (0 = unassigned -> NA_integer_), with streaming
// stores: the destination is written once and not read again by this call, so its lines need not be fetched
// first (that read-for-ownership doubles the memory traffic of a plain store loop).
void widen_labels(const uint8_t* src, int32_t* dst, int64_t n) {
    int64_t q = 0;
    for (; q < n && (reinterpret_cast<uintptr_t>(dst + q) & 15); ++q) dst[q] = src[q] ? (int32_t)src[q] : BMM_NA_INTEGER;
    const __m128i zero = _mm_setzero_si128(), na = _mm_set1_epi32(BMM_NA_INTEGER);
    for (; q + 16 <= n; q += 16) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + q));
        const __m128i lo = _mm_unpacklo_epi8(v, zero), hi = _mm_unpackhi_epi8(v, zero);
        __m128i w[4] = {_mm_unpacklo_epi16(lo, zero), _mm_unpackhi_epi16(lo, zero), _mm_unpacklo_epi16(hi, zero), _mm_unpackhi_epi16(hi, zero)};
        for (int k = 0; k < 4; ++k) {
            w[k] = _mm_or_si128(w[k], _mm_and_si128(_mm_cmpeq_epi32(w[k], zero), na));
            _mm_stream_si128(reinterpret_cast<__m128i*>(dst + q + 4 * k), w[k]);
        }
    }
    for (; q < n; ++q) dst[q] = src[q] ? (int32_t)src[q] : BMM_NA_INTEGER;
    _mm_sfence();
}
void copy_labels(const int32_t* src, int32_t* dst, int64_t n) {  // the same for labels that travel as int32
    int64_t q = 0;
    for (; q < n && (reinterpret_cast<uintptr_t>(dst + q) & 15); ++q) dst[q] = src[q];
    for (; q + 4 <= n; q += 4)
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst + q), _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + q)));
    for (; q < n; ++q) dst[q] = src[q];
    _mm_sfence();
}

// The label trace out to the caller's S x N column-major matrix (labels 1-based, NA where unassigned).
// In that layout the S labels of one observation are contiguous, so a block of observations is a contiguous
// run of the caller's buffer: the device transposes the [S][N] trace block by block (k_trace_block), each
// block goes to pinned staging, and the host's cores copy it into place while the next block is on its way --
// every byte of the (pageable) destination is written once, in order, at the speed of the slower of PCIe
// and the host's memory.  Up to 254 labels travel as one byte each and are widened by that host copy (a
// quarter of the PCIe bytes).  Nothing of it can start before the last sweep has finished: each
// observation's run is complete only then.
// perm: the S x K device permutation table of a relabelling run -- the trace then leaves relabelled
int trace_out(bmm_chain* c, int32_t* z_out, PhaseClock* clock, const int32_t* perm = nullptr) {
    const int64_t N = c->p.N;
    const int S = c->S;
    const bool narrow = c->p.K <= 254;
    const size_t el = narrow ? 1 : 4;
    const int64_t B = (int64_t)out_block_rows(S, el, N);
    const size_t blk_bytes = (size_t)B * S * el;  // = c->out_blk_bytes
    // host staging: two pieces of the pool; a trace with so many kept sweeps that 32 observations exceed a
    // piece gets buffers of its own
    Stage pooled[2];
    PinnedBuf own[2];
    void* hblk[2] = {pooled[0].p, pooled[1].p};
    if (blk_bytes > kStageBytes || !hblk[0] || !hblk[1])
        for (int q = 0; q < 2; ++q) { HIP_TRY(own[q].alloc(blk_bytes)); hblk[q] = own[q].p; }
    EventPair ev;
    HIP_TRY(ev.create());
    std::unique_ptr<HostCrew> own_crew;  // a resident chain's trace (no *_run call around it)
    HostCrew* crew = c->crew;
    if (!crew) { own_crew.reset(new HostCrew()); crew = own_crew.get(); }
    // The caller's S x N matrix is usually fresh (R's allocMatrix, numpy.empty): its pages are not there yet, and
    // taking the page faults inside the widening loop makes that loop fault-bound (1.08 GB at C5: 14-21 ms).  The
    // host is idle while the device still runs the sweeps enqueued ahead of this call's blocks, so the crew takes
    // the faults now (MADV_POPULATE_WRITE, Linux 5.14; anything else it answers is ignored: the widening then
    // faults as before).  Every cell of the matrix is overwritten below.
    {
        const uintptr_t page = 4096;
        const uintptr_t lo = (reinterpret_cast<uintptr_t>(z_out) + page - 1) & ~(page - 1);
        const uintptr_t hi = (reinterpret_cast<uintptr_t>(z_out) + (size_t)S * (size_t)N * sizeof(int32_t)) & ~(page - 1);
        if (hi > lo + (64 << 20) / 64) {  // from a megabyte up
            const int64_t pages = (int64_t)((hi - lo) / page);
            crew->begin(pages, 256, 1, [lo, page](int64_t a, int64_t b) {
                (void)madvise(reinterpret_cast<void*>(lo + (uintptr_t)a * page), (size_t)(b - a) * page, MADV_POPULATE_WRITE);
            });
        }
    }
    auto consume = [&](int64_t blk) {
        const int64_t i0 = blk * B, rows = N - i0 < B ? N - i0 : B;
        int32_t* const dst = z_out + (size_t)i0 * S;
        const int64_t n = rows * S;
        if (narrow) {
            const uint8_t* const src = static_cast<const uint8_t*>(hblk[blk & 1]);
            crew->run(n, 1 << 16, 64, [=](int64_t lo, int64_t hi) { widen_labels(src + lo, dst + lo, hi - lo); });
        } else {
            const int32_t* const src = static_cast<const int32_t*>(hblk[blk & 1]);
            crew->run(n, 1 << 16, 64, [=](int64_t lo, int64_t hi) { copy_labels(src + lo, dst + lo, hi - lo); });
        }
    };
    const int64_t nblk = (N + B - 1) / B;
    for (int64_t blk = 0; blk < nblk; ++blk) {
        const int64_t i0 = blk * B, rows = N - i0 < B ? N - i0 : B;
        const dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((S + 31) / 32));
        char* const dblk = c->dOutBlk[blk & 1];
        // block blk - 2 has been consumed (below) before this iteration started: its staging is free
        if (narrow) hipLaunchKernelGGL(k_trace_block<uint8_t>, grid, dim3(256), 0, c->stream, c->dTrace, N, S, i0, rows, reinterpret_cast<uint8_t*>(dblk), perm);
        else hipLaunchKernelGGL(k_trace_block<int32_t>, grid, dim3(256), 0, c->stream, c->dTrace, N, S, i0, rows, reinterpret_cast<int32_t*>(dblk), perm);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hblk[blk & 1], dblk, (size_t)rows * S * el, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(ev.e[blk & 1], c->stream));
        if (blk >= 1) {
            HIP_TRY(hipEventSynchronize(ev.e[(blk - 1) & 1]));
            if (blk == 1 && clock) clock->lap(3);  // the first block has arrived: the sweeps are over
            consume(blk - 1);
        }
    }
    HIP_TRY(hipEventSynchronize(ev.e[(nblk - 1) & 1]));
    if (nblk == 1 && clock) clock->lap(3);
    consume(nblk - 1);
    HIP_TRY(hipStreamSynchronize(c->stream));  // the small traces queued ahead of the blocks
    return BMM_OK;
}

// The sweeps of a run that reports its progress (bmm_set_progress): everything is still enqueued ahead of
// the device, an event after every `every`-th sweep; the calling thread then follows the events and calls
// the hook as each one is reached.  For the DP sampler the cluster sizes at those sweeps ride along (K
// int32 into pinned memory) so that the hook gets the number of clusters in use, as the reference prints
// it (collapsed_gibbs_dp.cpp:99).  step (a relabelling run): enqueues sweep j with its share of the relabelling,
// in place of the plain sweeps.
int run_sweeps_reported(bmm_chain* c, int nsamples, const std::function<int(int)>& step = nullptr) {
    const int every = g_progress.every, K = c->p.K;
    const int total = nsamples - 1, marks = (total + every - 1) / every;
    if (marks < 1) return BMM_OK;
    std::vector<hipEvent_t> evs((size_t)marks, nullptr);
    struct Free { std::vector<hipEvent_t>& v; ~Free() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); } } fr{evs};
    PinnedBuf sizes;
    const bool dp = c->p.mode == MODE_DP;
    if (dp) HIP_TRY(sizes.alloc((size_t)marks * K * sizeof(int32_t)));
    for (int m = 0; m < marks; ++m) {
        const int n = total - m * every < every ? total - m * every : every;
        int rc = BMM_OK;
        if (step) { for (int t = 0; t < n && rc == BMM_OK; ++t) rc = step(c->sweep + 1); }
        else rc = bmm_chain_sweeps(c, n);
        if (rc) return rc;
        if (dp) HIP_TRY(hipMemcpyAsync(sizes.as<int32_t>() + (size_t)m * K, c->dNk, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventCreateWithFlags(&evs[(size_t)m], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(evs[(size_t)m], c->stream));
    }
    for (int m = 0; m < marks; ++m) {
        HIP_TRY(hipEventSynchronize(evs[(size_t)m]));
        const int done = (m + 1) * every < total ? (m + 1) * every : total;  // sweeps finished: j = 1 .. done
        int used = -1;
        if (dp) { used = 0; for (int k = 0; k < K; ++k) used += sizes.as<int32_t>()[(size_t)m * K + k] > 0; }
        if (g_progress.fn(g_progress.user, done + 1, nsamples, used) != 0) {
            (void)hipStreamSynchronize(c->stream);
            return set_err(BMM_E_CALLBACK, "the progress hook stopped the run after sample %d", done + 1);
        }
    }
    return BMM_OK;
}

// the starting state of a run: initial labels or parameters, and trace row 0 when burnin = 0
int run_start_state(bmm_chain* c, const RunIO& io, bool device_init = false) {
    const int sampler = c->p.mode, K = c->p.K, P = c->p.P, S = c->S, burnin = c->burnin;
    const int64_t N = c->p.N;
    HIP_TRY(hipSetDevice(c->device));
    int rc = BMM_OK;
    // (device_init: the labels are computed on the device once the planes are there, bmm_set_init)
    if (sampler == BMM_SAMPLER_COLLAPSED && !device_init) rc = bmm_chain_set_initial_labels(c, io.z0);
    if (explicit_params(sampler)) rc = bmm_chain_set_initial_params(c, io.pi0, io.theta0);
    if (rc) return rc;
    if (burnin == 0) {
        // trace row 0 (DESIGN.md "Quirks"): labels = initial allocation or unassigned (-1 -> NA),
        // theta = NaN (collapsed, never written), 0 (dp, zero-filled) or the initial theta (sb)
        std::vector<double> t0((size_t)K * P, sampler == BMM_SAMPLER_DP ? 0.0 : std::nan(""));
        if (explicit_params(sampler)) std::memcpy(t0.data(), io.theta0, t0.size() * sizeof(double));
        HIP_TRY(hipMemcpy(c->dThetaTrace, t0.data(), t0.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->dAlphaTrace, &c->alpha0, sizeof(double), hipMemcpyHostToDevice));
        if (explicit_params(sampler))
            HIP_TRY(hipMemcpy2D(c->dPiTrace, (size_t)S * sizeof(double), io.pi0, sizeof(double), sizeof(double), K, hipMemcpyHostToDevice));
        if (sampler != BMM_SAMPLER_COLLAPSED && c->dTrace) HIP_TRY(hipMemset(c->dTrace, 0xff, (size_t)N * sizeof(int32_t)));
    }
    return BMM_OK;
}

// the relabelled theta trace: theta_relab(perm(s, k), d, s) = theta(k, d, s) (collapsed_gibbs.cpp:215-217)
void permute_theta(const double* th, const int32_t* perm, int K, int P, int S, double* out) {
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < K; ++k) {
            const int to = perm[s + (size_t)k * S];
            for (int d = 0; d < P; ++d) out[to + (size_t)K * d + (size_t)K * P * s] = th[k + (size_t)K * d + (size_t)K * P * s];
        }
}

// ---- clustering point estimate and posterior similarity (include/bmm_mcmc.h) ----
// Which form of the k_pt_* kernels a shape runs: a pure function of (S, N, Kc, candidates, criterion) -- the
// launches below and bmm_device_partition_plan both read it from here.
constexpr size_t kPtLdsBudget = (size_t)48 << 10;       // bytes of contingency tables per workgroup
constexpr size_t kPtGenericBudget = (size_t)256 << 20;  // bytes of global-memory tables of the generic form
struct PtPlan {
    int el = 1, lds = 1, T = 1, R = 1, blocks = 1, threads = kPtThreads, tri = 0, vi = 0;
    int64_t wgs = 0, pitch = 0;
    size_t lds_bytes = 0, generic_bytes = 0;
};
PtPlan pt_plan(int S, int64_t N, int Kc, int C, int criterion) {
    PtPlan p;
    const size_t tb = (size_t)Kc * Kc * sizeof(uint32_t);
    p.el = Kc <= 256 ? 1 : 4;
    p.lds = Kc <= kPtMaxLdsK ? 1 : 0;
    p.tri = C == S ? 1 : 0;  // stride 1 (or a single row): rc == c
    p.vi = criterion == BMM_PARTITION_VI ? 1 : 0;
    p.pitch = (N + 15) / 16 * 16;
    if (p.lds) {
        p.R = tb <= 1024 ? 4 : 1;
        int64_t T = (int64_t)(kPtLdsBudget / (tb * p.R));
        if (T > 8) T = 8;
        if (T > S) T = S;
        p.T = (int)(T < 1 ? 1 : T);
        p.blocks = (S + p.T - 1) / p.T;
        p.wgs = (int64_t)C * p.blocks;
        p.lds_bytes = (size_t)p.T * p.R * tb;
    } else {
        p.blocks = S;
        int64_t g = (int64_t)(kPtGenericBudget / tb);
        if (g > 1024) g = 1024;
        if (g > (int64_t)C * S) g = (int64_t)C * S;
        p.wgs = g < 1 ? 1 : g;
        p.generic_bytes = (size_t)p.wgs * tb;
    }
    return p;
}
// refused before any device is touched
int pt_check_shape(int S, int64_t N, int Kc, int criterion, int stride) {
    if (S < 1) return set_err(BMM_E_ARG, "partition: S must be >= 1");
    if (N < 1) return set_err(BMM_E_ARG, "partition: N must be >= 1");
    if (S > BMM_PARTITION_MAX_ROWS) return set_err(BMM_E_ARG, "partition: S = %d rows is more than the %d one call takes", S, BMM_PARTITION_MAX_ROWS);
    if (stride < 1) return set_err(BMM_E_ARG, "partition: stride must be >= 1");
    if (Kc < 1 || Kc > BMM_PARTITION_MAX_K) return set_err(BMM_E_ARG, "partition: Kc must be in 1 .. %d (got %d)", BMM_PARTITION_MAX_K, Kc);
    if (criterion != BMM_PARTITION_BINDER && criterion != BMM_PARTITION_VI) return set_err(BMM_E_ARG, "partition: unknown criterion %d", criterion);
    if ((unsigned __int128)S * (unsigned __int128)N * (unsigned __int128)N >= ((unsigned __int128)1 << 63))
        return set_err(BMM_E_ARG, "partition: S * N^2 = %d * %lld^2 does not fit the exact integer totals (must be < 2^63)", S, (long long)N);
    return BMM_OK;
}
// every label of the caller's S x N matrix in lo .. hi (1-based); the first offender is named
int pt_check_labels(const int32_t* z, int S, int64_t N, int lo, int64_t hi, int32_t* max_out, const char* what = "partition") {
    const int64_t total = (int64_t)S * N;
    std::atomic<int64_t> bad{INT64_MAX};
    std::atomic<int32_t> top{0};
    HostCrew crew;
    crew.run(total, 1 << 16, 64, [&](int64_t a, int64_t b) {
        int32_t mx = 0;
        for (int64_t q = a; q < b; ++q) {
            const int32_t v = z[q];
            if (v < lo || v > hi) {
                int64_t cur = bad.load(std::memory_order_relaxed);
                while (q < cur && !bad.compare_exchange_weak(cur, q, std::memory_order_relaxed)) {}
                return;
            }
            if (v > mx) mx = v;
        }
        int32_t cur = top.load(std::memory_order_relaxed);
        while (mx > cur && !top.compare_exchange_weak(cur, mx, std::memory_order_relaxed)) {}
    });
    const int64_t q = bad.load();
    if (q != INT64_MAX)
        return set_err(BMM_E_ARG, "%s: label %d at row %lld, observation %lld (0-based) is outside %d .. %lld: not a partition",
                       what, z[q], (long long)(q % S), (long long)(q / S), lo, (long long)hi);
    if (max_out) *max_out = top.load();
    return BMM_OK;
}

struct PtWork {
    int S = 0, Kc = 0, C = 0, stride = 1;
    int64_t N = 0;
    PtPlan plan;
    DevBuf lab, flag, A, F, Q, G, sum2, loss, best, tabs, dist;
    void shape(int S_, int64_t N_, int Kc_, int criterion, int stride_) {
        S = S_; N = N_; Kc = Kc_; stride = stride_;
        C = (S + stride - 1) / stride;
        plan = pt_plan(S, N, Kc, C, criterion);
    }
    int alloc_labels() {
        HIP_TRY(lab.alloc((size_t)S * plan.pitch * plan.el));
        HIP_TRY(flag.alloc(sizeof(int)));
        HIP_TRY(hipMemset(flag.p, 0, sizeof(int)));
        return BMM_OK;
    }
    int alloc_pairs(bool want_dist) {
        const size_t cs = (size_t)C * S;
        HIP_TRY(A.alloc((size_t)S * sizeof(uint64_t)));
        HIP_TRY(F.alloc((size_t)S * sizeof(double)));
        HIP_TRY(Q.alloc(cs * sizeof(uint64_t)));
        HIP_TRY(G.alloc(cs * sizeof(double)));
        HIP_TRY(sum2.alloc((size_t)C * sizeof(uint64_t)));
        HIP_TRY(loss.alloc((size_t)C * sizeof(double)));
        HIP_TRY(best.alloc(sizeof(int)));
        if (!plan.lds) HIP_TRY(tabs.alloc(plan.generic_bytes));
        if (want_dist) HIP_TRY(dist.alloc(cs * sizeof(double)));
        return BMM_OK;
    }
};

// labels (s, li) at src[s * ss + li * si] - base for observations [i0, i0 + rows) into the label block
int pt_narrow(hipStream_t st, PtWork& w, const int32_t* src, int64_t ss, int64_t si, int base, int64_t i0, int64_t rows) {
    const dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((w.S + 31) / 32));
    if (w.plan.el == 1)
        hipLaunchKernelGGL(k_pt_narrow<uint8_t>, grid, dim3(256), 0, st, src, ss, si, base, w.S, i0, rows, w.Kc, w.lab.as<uint8_t>(), w.plan.pitch, w.flag.as<int>());
    else
        hipLaunchKernelGGL(k_pt_narrow<int32_t>, grid, dim3(256), 0, st, src, ss, si, base, w.S, i0, rows, w.Kc, w.lab.as<int32_t>(), w.plan.pitch, w.flag.as<int>());
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// the caller's S x N column-major matrix (observation i's S labels are contiguous) in blocks of observations
int pt_upload(PtWork& w, const int32_t* z) {
    const int S = w.S;
    int64_t B = (int64_t)(((size_t)32 << 20) / ((size_t)S * sizeof(int32_t))) / 32 * 32;
    if (B < 32) B = 32;
    if (B > w.N) B = w.N;
    DevBuf stage;
    HIP_TRY(stage.alloc((size_t)B * S * sizeof(int32_t)));
    for (int64_t i0 = 0; i0 < w.N; i0 += B) {
        const int64_t rows = w.N - i0 < B ? w.N - i0 : B;
        HIP_TRY(hipMemcpy(stage.p, z + (size_t)i0 * S, (size_t)rows * S * sizeof(int32_t), hipMemcpyHostToDevice));
        const int rc = pt_narrow(nullptr, w, stage.as<int32_t>(), 1, S, 1, i0, rows);
        if (rc) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());  // before the staging block goes
    return BMM_OK;
}
// sizes, pairs, losses, argmin: everything enqueued on st
int pt_compute(hipStream_t st, PtWork& w) {
    const PtPlan& p = w.plan;
    const int S = w.S, C = w.C, Kc = w.Kc;
    const size_t hist = (size_t)4 * Kc * sizeof(uint32_t);
    if (p.el == 1) hipLaunchKernelGGL(k_pt_sizes<uint8_t>, dim3(S), dim3(256), hist, st, w.lab.as<uint8_t>(), p.pitch, w.N, Kc, w.A.as<uint64_t>(), w.F.as<double>());
    else hipLaunchKernelGGL(k_pt_sizes<int32_t>, dim3(S), dim3(256), hist, st, w.lab.as<int32_t>(), p.pitch, w.N, Kc, w.A.as<uint64_t>(), w.F.as<double>());
    HIP_TRY(hipGetLastError());
    uint64_t* const Q = w.Q.as<uint64_t>();
    double* const G = w.G.as<double>();
    if (S > 1) {
        if (p.lds) {
            const dim3 grid((unsigned)p.blocks, (unsigned)C);
            if (p.vi) hipLaunchKernelGGL(k_pt_pairs<true>, grid, dim3(256), p.lds_bytes, st, w.lab.as<uint8_t>(), p.pitch, w.N, S, Kc, w.stride, p.T, p.R, p.tri, Q, G);
            else hipLaunchKernelGGL(k_pt_pairs<false>, grid, dim3(256), p.lds_bytes, st, w.lab.as<uint8_t>(), p.pitch, w.N, S, Kc, w.stride, p.T, p.R, p.tri, Q, G);
        } else {
            const dim3 grid((unsigned)p.wgs);
            uint32_t* const tabs = w.tabs.as<uint32_t>();
            if (p.el == 1) {
                if (p.vi) hipLaunchKernelGGL((k_pt_pairs_generic<uint8_t, true>), grid, dim3(256), 0, st, w.lab.as<uint8_t>(), p.pitch, w.N, S, Kc, w.stride, C, p.tri, tabs, Q, G);
                else hipLaunchKernelGGL((k_pt_pairs_generic<uint8_t, false>), grid, dim3(256), 0, st, w.lab.as<uint8_t>(), p.pitch, w.N, S, Kc, w.stride, C, p.tri, tabs, Q, G);
            } else {
                if (p.vi) hipLaunchKernelGGL((k_pt_pairs_generic<int32_t, true>), grid, dim3(256), 0, st, w.lab.as<int32_t>(), p.pitch, w.N, S, Kc, w.stride, C, p.tri, tabs, Q, G);
                else hipLaunchKernelGGL((k_pt_pairs_generic<int32_t, false>), grid, dim3(256), 0, st, w.lab.as<int32_t>(), p.pitch, w.N, S, Kc, w.stride, C, p.tri, tabs, Q, G);
            }
        }
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pt_loss, dim3(C), dim3(256), 0, st, w.A.as<uint64_t>(), w.F.as<double>(), Q, G, S, C, w.stride, w.N, p.vi, w.sum2.as<uint64_t>(), w.loss.as<double>(), w.dist.as<double>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pt_argmin, dim3(1), dim3(256), 0, st, w.sum2.as<uint64_t>(), w.loss.as<double>(), C, p.vi, w.best.as<int>());
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// after the stream has been waited for: the results out; best_out is the candidate's row, c * stride
int pt_fetch(PtWork& w, double* loss_out, uint64_t* binder2_out, int* best_out, double* dist_out) {
    int flag = 0, best = -1;
    HIP_TRY(hipMemcpy(&flag, w.flag.p, sizeof flag, hipMemcpyDeviceToHost));
    if (flag) return set_err(BMM_E_STATE, "partition: a label outside 0 .. %d reached the device", w.Kc - 1);
    HIP_TRY(hipMemcpy(loss_out, w.loss.p, (size_t)w.C * sizeof(double), hipMemcpyDeviceToHost));
    if (binder2_out) HIP_TRY(hipMemcpy(binder2_out, w.sum2.p, (size_t)w.C * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&best, w.best.p, sizeof best, hipMemcpyDeviceToHost));
    if (best_out) *best_out = best * w.stride;
    if (dist_out) HIP_TRY(hipMemcpy(dist_out, w.dist.p, (size_t)w.C * w.S * sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}
// similarity counts of idx[0 .. M) over the label block's S rows
int pt_psm(hipStream_t st, PtWork& w, const int64_t* idx, int64_t M, uint32_t* cnt_out) {
    const size_t need = (size_t)M * M * sizeof(uint32_t) + (size_t)w.S * M * w.plan.el + (size_t)M * sizeof(int64_t);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        return set_err(BMM_E_ARG, "similarity: %lld x %lld counts and the %d x %lld block of labels need %zu bytes of device memory, %zu are free",
                       (long long)M, (long long)M, w.S, (long long)M, need, free_b);
    DevBuf didx, g, cnt;
    HIP_TRY(didx.alloc((size_t)M * sizeof(int64_t)));
    HIP_TRY(g.alloc((size_t)w.S * M * w.plan.el));
    HIP_TRY(cnt.alloc((size_t)M * M * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(didx.p, idx, (size_t)M * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const dim3 gg((unsigned)((M + 255) / 256), (unsigned)w.S);
    const unsigned nt = (unsigned)((M + 63) / 64);
    if (w.plan.el == 1) {
        hipLaunchKernelGGL(k_pt_gather<uint8_t>, gg, dim3(256), 0, st, w.lab.as<uint8_t>(), w.plan.pitch, didx.as<int64_t>(), M, g.as<uint8_t>());
        hipLaunchKernelGGL(k_pt_psm<uint8_t>, dim3(nt, nt), dim3(256), 0, st, g.as<uint8_t>(), w.S, M, cnt.as<uint32_t>());
    } else {
        hipLaunchKernelGGL(k_pt_gather<int32_t>, gg, dim3(256), 0, st, w.lab.as<int32_t>(), w.plan.pitch, didx.as<int64_t>(), M, g.as<int32_t>());
        hipLaunchKernelGGL(k_pt_psm<int32_t>, dim3(nt, nt), dim3(256), 0, st, g.as<int32_t>(), w.S, M, cnt.as<uint32_t>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cnt_out, cnt.p, (size_t)M * M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BMM_OK;
}
int pt_check_idx(const int64_t* idx, int64_t M, int64_t N) {
    for (int64_t u = 0; u < M; ++u)
        if (idx[u] < 0 || idx[u] >= N) return set_err(BMM_E_ARG, "similarity: idx[%lld] = %lld is outside 0 .. %lld", (long long)u, (long long)idx[u], (long long)(N - 1));
    return BMM_OK;
}

// ---- greedy search for the point estimate (include/bmm_mcmc.h "greedy search") ----
// Which form of the k_ps_* kernels a shape runs: a pure function of (S, N, Kc, Ka, criterion, batch) -- the launches
// below and bmm_partition_search_plan both read it from here.
constexpr size_t kPsLdsBudget = (size_t)48 << 10;                                  // bytes of tables per workgroup
constexpr size_t kPsScoreBytes = (size_t)kPtThreads * kPsChunk * sizeof(int64_t);  // the scores of a workgroup's rows
struct PsPlan {
    int el = 1, KaP = 12, nch = 1, rows = kPtThreads, D = 1, blocks = 1, bound = 0, vi = 0, apply_y = 1, apply_len = 1;
    int64_t wgs = 1, batches = 1, pitch = 0, span = 0;
    size_t lds_bytes = 0, table_bytes = 0;
};
PsPlan ps_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t batch) {
    PsPlan p;
    p.vi = criterion == BMM_PARTITION_VI ? 1 : 0;
    p.nch = (Ka + kPsChunk - 1) / kPsChunk;
    p.KaP = p.nch * kPsChunk + 4;  // runs of 8 slots stay 16-byte aligned, neighbouring labels 4 banks apart
    p.rows = kPtThreads / p.nch;
    p.pitch = (N + 15) / 16 * 16;
    const size_t cell = p.vi ? sizeof(double) : sizeof(uint32_t);
    const size_t tb = (size_t)Kc * p.KaP * cell;
    int64_t D = S;
    if ((int64_t)(kPsLdsBudget / tb) < D) { D = (int64_t)(kPsLdsBudget / tb); p.bound = 1; }
    if (!p.vi && D * N >= ((int64_t)1 << 32)) { D = (((int64_t)1 << 32) - 1) / N; p.bound = 2; }
    p.D = (int)(D < 1 ? 1 : D);
    p.blocks = (S + p.D - 1) / p.D;
    p.lds_bytes = (size_t)p.D * tb > kPsScoreBytes ? (size_t)p.D * tb : kPsScoreBytes;
    if (batch > N) batch = N;
    p.wgs = (batch + p.rows - 1) / p.rows;
    p.batches = (N + batch - 1) / batch;
    p.table_bytes = (size_t)S * Kc * p.KaP * (sizeof(uint32_t) + (p.vi ? 2 * sizeof(double) : 0));
    p.span = 8192;  // rows of a draw per workgroup of k_ps_tables
    p.apply_y = S < 8 ? S : 8;  // k_ps_apply: the draws of a moved row over this many workgroups
    p.apply_len = (S + p.apply_y - 1) / p.apply_y;
    return p;
}
struct PsOpts { int64_t batch = 0, min_batch = 0; int max_passes = 50, Ka = 0; };
// the options resolved against a shape, and everything refused before any device is touched
int ps_check(int S, int64_t N, int Kc, int criterion, const bmm_partition_search_opts* o, bool own_start, PsOpts& r) {
    int rc = pt_check_shape(S, N, Kc, criterion, 1);
    if (rc) return rc;
    if (Kc > BMM_PARTITION_SEARCH_MAX_K)
        return set_err(BMM_E_ARG, "partition search: Kc = %d is above the %d whose tables fit in LDS", Kc, BMM_PARTITION_SEARCH_MAX_K);
    r.batch = o ? o->batch : (N + 7) / 8;
    r.min_batch = o ? o->min_batch : (N + 255) / 256;
    r.max_passes = o ? o->max_passes : 50;
    r.Ka = o ? o->max_clusters : Kc;
    if (r.batch < 1 || r.min_batch < 1) return set_err(BMM_E_ARG, "partition search: batch and min_batch must be >= 1 (got %lld, %lld)", (long long)r.batch, (long long)r.min_batch);
    if (r.max_passes < 1) return set_err(BMM_E_ARG, "partition search: max_passes must be >= 1 (got %d)", r.max_passes);
    if (r.Ka < 1 || r.Ka > BMM_PARTITION_SEARCH_MAX_K)
        return set_err(BMM_E_ARG, "partition search: max_clusters must be in 1 .. %d (got %d)", BMM_PARTITION_SEARCH_MAX_K, r.Ka);
    if (own_start && r.Ka < Kc)
        return set_err(BMM_E_ARG, "partition search: starting from a draw needs max_clusters >= Kc (got %d < %d)", r.Ka, Kc);
    if (r.batch > N) r.batch = N;
    if (r.min_batch > r.batch) r.min_batch = r.batch;
    return BMM_OK;
}
int ps_check_out(const bmm_partition_search_out* o) {
    if (!o || !o->z_hat || !o->binder2 || !o->loss || !o->start_loss || !o->start_binder2 || !o->passes || !o->pass_batch ||
        !o->pass_moved || !o->pass_binder2 || !o->pass_total || !o->converged || !o->n_clusters)
        return set_err(BMM_E_ARG, "partition search: null output buffer");
    return BMM_OK;
}

struct PsWork {
    int S = 0, Kc = 0, Ka = 0;
    int64_t N = 0;
    PsPlan plan;
    DevBuf T, n, phi, phim, sphi, c, best, newc, d2, w, moved, res;
    size_t cells() const { return (size_t)S * Kc * plan.KaP; }
    int alloc(int S_, int64_t N_, int Kc_, int Ka_, int criterion, int64_t batch) {
        S = S_; N = N_; Kc = Kc_; Ka = Ka_;
        plan = ps_plan(S, N, Kc, Ka, criterion, batch);
        HIP_TRY(T.alloc(cells() * sizeof(uint32_t)));
        HIP_TRY(n.alloc((size_t)plan.KaP * sizeof(uint32_t)));
        if (plan.vi) {
            HIP_TRY(phi.alloc(cells() * sizeof(double)));
            HIP_TRY(phim.alloc(cells() * sizeof(double)));
            HIP_TRY(sphi.alloc((size_t)2 * plan.KaP * sizeof(double)));
        }
        HIP_TRY(c.alloc((size_t)N * sizeof(int32_t)));
        HIP_TRY(best.alloc((size_t)N * sizeof(int32_t)));
        HIP_TRY(newc.alloc((size_t)N * sizeof(int32_t)));
        HIP_TRY(d2.alloc((size_t)S * sizeof(uint64_t)));
        HIP_TRY(w.alloc((size_t)S * sizeof(double)));
        HIP_TRY(moved.alloc(sizeof(unsigned long long)));
        HIP_TRY(res.alloc(3 * sizeof(unsigned long long)));
        return BMM_OK;
    }
};
// VI: the phi tables follow the counts
int ps_phi(hipStream_t st, PsWork& w) {
    if (!w.plan.vi) return BMM_OK;
    const int64_t cells = (int64_t)w.cells();
    int64_t g = (cells + kPtThreads - 1) / kPtThreads;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(k_ps_phi, dim3((unsigned)g), dim3(256), 0, st, w.T.as<uint32_t>(), w.n.as<uint32_t>(), cells, w.plan.KaP,
                       w.phi.as<double>(), w.phim.as<double>(), w.sphi.as<double>());
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// tables and sizes of the candidate as it stands in w.c
int ps_rebuild(hipStream_t st, PsWork& w, const uint8_t* lab) {
    const PsPlan& p = w.plan;
    HIP_TRY(hipMemsetAsync(w.T.p, 0, w.cells() * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(w.n.p, 0, (size_t)p.KaP * sizeof(uint32_t), st));
    const dim3 grid((unsigned)((w.N + p.span - 1) / p.span), (unsigned)w.S);
    const size_t lds = ((size_t)w.Kc * p.KaP + p.KaP) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_ps_tables, grid, dim3(256), lds, st, lab, p.pitch, w.N, w.Kc, p.KaP, p.span, w.c.as<int32_t>(), w.T.as<uint32_t>(), w.n.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return ps_phi(st, w);
}
// the totals of the state and the moved count, read back: the one wait of a pass
int ps_total(hipStream_t st, PsWork& w, uint64_t* binder2, double* vi_tot, int64_t* moved) {
    const PsPlan& p = w.plan;
    if (p.vi) hipLaunchKernelGGL(k_ps_total<true>, dim3(w.S), dim3(256), 0, st, w.T.as<uint32_t>(), w.n.as<uint32_t>(), w.Kc, w.Ka, p.KaP, w.d2.as<uint64_t>(), w.w.as<double>());
    else hipLaunchKernelGGL(k_ps_total<false>, dim3(w.S), dim3(256), 0, st, w.T.as<uint32_t>(), w.n.as<uint32_t>(), w.Kc, w.Ka, p.KaP, w.d2.as<uint64_t>(), w.w.as<double>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ps_reduce, dim3(1), dim3(256), 0, st, w.d2.as<uint64_t>(), w.w.as<double>(), w.S, w.moved.as<unsigned long long>(), w.res.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, w.res.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *binder2 = h[0];
    std::memcpy(vi_tot, &h[1], sizeof(double));
    *moved = (int64_t)h[2];
    return BMM_OK;
}
// one pass with batch B: score, apply (and, for VI, the phi tables) per batch, everything enqueued
int ps_pass(hipStream_t st, PsWork& w, const uint8_t* lab, int64_t B) {
    const PsPlan& p = w.plan;
    HIP_TRY(hipMemsetAsync(w.moved.p, 0, sizeof(unsigned long long), st));
    for (int64_t i0 = 0; i0 < w.N; i0 += B) {
        const int64_t i1 = i0 + B < w.N ? i0 + B : w.N;
        const dim3 gs((unsigned)((i1 - i0 + p.rows - 1) / p.rows)), ga((unsigned)((i1 - i0 + kPtThreads - 1) / kPtThreads), (unsigned)p.apply_y);
        if (p.vi) hipLaunchKernelGGL(k_ps_score<true>, gs, dim3(256), p.lds_bytes, st, lab, p.pitch, w.S, w.Kc, w.Ka, p.KaP, p.nch, p.rows, p.D, w.T.as<uint32_t>(), w.phi.as<double>(), w.phim.as<double>(), w.sphi.as<double>(), w.n.as<uint32_t>(), w.c.as<int32_t>(), i0, i1, w.newc.as<int32_t>());
        else hipLaunchKernelGGL(k_ps_score<false>, gs, dim3(256), p.lds_bytes, st, lab, p.pitch, w.S, w.Kc, w.Ka, p.KaP, p.nch, p.rows, p.D, w.T.as<uint32_t>(), nullptr, nullptr, nullptr, w.n.as<uint32_t>(), w.c.as<int32_t>(), i0, i1, w.newc.as<int32_t>());
        hipLaunchKernelGGL(k_ps_apply, ga, dim3(256), 0, st, lab, p.pitch, w.S, w.Kc, p.KaP, p.apply_len, w.T.as<uint32_t>(), w.n.as<uint32_t>(), w.c.as<int32_t>(), w.newc.as<int32_t>(), i0, i1, w.moved.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.c.as<int32_t>() + i0, w.newc.as<int32_t>() + i0, (size_t)(i1 - i0) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        const int rc = ps_phi(st, w);
        if (rc) return rc;
    }
    return BMM_OK;
}
// The search (the header's pseudo-code) from the candidate in w.c (0-based slots), over the label block `lab`
int ps_search(hipStream_t st, PsWork& w, const uint8_t* lab, const PsOpts& o, const bmm_partition_search_out& out) {
    const size_t nb = (size_t)w.N * sizeof(int32_t);
    const bool vi = w.plan.vi != 0;
    const double SN = (double)w.S * (double)w.N;
    auto loss_of = [&](uint64_t b2, double vt) { return vi ? vt / SN : (double)b2 / (2.0 * (double)w.S); };
    int rc = ps_rebuild(st, w, lab);
    if (rc) return rc;
    uint64_t b2 = 0, best_b2 = 0;
    double vt = 0.0, best_vt = 0.0;
    int64_t moved = 0;
    rc = ps_total(st, w, &best_b2, &best_vt, &moved);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(w.best.p, w.c.p, nb, hipMemcpyDeviceToDevice, st));
    *out.start_binder2 = best_b2;
    *out.start_loss = loss_of(best_b2, best_vt);
    int passes = 0, converged = 0;
    int64_t B = o.batch;
    while (passes < o.max_passes) {
        rc = ps_pass(st, w, lab, B);
        if (rc == BMM_OK) rc = ps_total(st, w, &b2, &vt, &moved);
        if (rc) return rc;
        out.pass_batch[passes] = B;
        out.pass_moved[passes] = moved;
        out.pass_binder2[passes] = b2;
        out.pass_total[passes] = vi ? vt : (double)b2;
        ++passes;
        if (moved == 0) { converged = 1; break; }
        if (vi ? vt < best_vt : b2 < best_b2) {
            best_b2 = b2; best_vt = vt;
            HIP_TRY(hipMemcpyAsync(w.best.p, w.c.p, nb, hipMemcpyDeviceToDevice, st));
        } else {
            HIP_TRY(hipMemcpyAsync(w.c.p, w.best.p, nb, hipMemcpyDeviceToDevice, st));
            rc = ps_rebuild(st, w, lab);
            if (rc) return rc;
            if (B == o.min_batch) break;
            B = B / 2 > o.min_batch ? B / 2 : o.min_batch;
        }
    }
    HIP_TRY(hipMemcpyAsync(out.z_hat, w.best.p, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<char> used((size_t)w.Ka, 0);
    for (int64_t i = 0; i < w.N; ++i) { used[(size_t)out.z_hat[i]] = 1; out.z_hat[i] += 1; }
    int nc = 0;
    for (char u : used) nc += u;
    *out.binder2 = best_b2;
    *out.loss = loss_of(best_b2, best_vt);
    *out.passes = passes;
    *out.converged = converged;
    *out.n_clusters = nc;
    return BMM_OK;
}

// ---- credible ball and row-to-cluster similarity (include/bmm_mcmc.h "credible ball") ----
// Which form of the k_cb_* kernels a shape runs: a pure function of (S, N, Kc, Ka, criterion, M, gathered) -- the
// launches below and bmm_credible_ball_plan both read it from here.  The tables are the search's uint32 tables under
// either criterion, so KaP, the threads of a row, the rows of a workgroup and D are those of its Binder form.
struct CbPlan {
    int el = 1, KaP = 12, nch = 1, rows = kPtThreads, D = 1, blocks = 1, bound = 0, vi = 0, gathered = 0;
    int64_t wgs = 1, pitch = 0, span = 0;
    size_t lds_bytes = 0, table_bytes = 0;
};
CbPlan cb_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t M, bool gathered) {
    const PsPlan q = ps_plan(S, N, Kc, Ka, BMM_PARTITION_BINDER, N);
    CbPlan p;
    p.el = q.el; p.KaP = q.KaP; p.nch = q.nch; p.rows = q.rows; p.D = q.D; p.blocks = q.blocks; p.bound = q.bound;
    p.pitch = q.pitch; p.span = q.span;
    p.vi = criterion == BMM_PARTITION_VI ? 1 : 0;
    p.gathered = gathered ? 1 : 0;
    p.wgs = (M + p.rows - 1) / p.rows;
    p.lds_bytes = (size_t)p.D * Kc * p.KaP * sizeof(uint32_t);
    p.table_bytes = (size_t)S * Kc * p.KaP * sizeof(uint32_t);
    return p;
}
// refused before any device is touched
int cb_check(int S, int64_t N, int Kc, int criterion, int Ka, double level) {
    const int rc = pt_check_shape(S, N, Kc, criterion, 1);
    if (rc) return rc;
    if (Kc > BMM_PARTITION_SEARCH_MAX_K)
        return set_err(BMM_E_ARG, "credible ball: Kc = %d is above the %d whose tables fit in LDS", Kc, BMM_PARTITION_SEARCH_MAX_K);
    if (Ka < 1 || Ka > BMM_PARTITION_SEARCH_MAX_K)
        return set_err(BMM_E_ARG, "credible ball: Ka must be in 1 .. %d (got %d)", BMM_PARTITION_SEARCH_MAX_K, Ka);
    if (!(level > 0.0 && level <= 1.0)) return set_err(BMM_E_ARG, "credible ball: level must be in (0, 1] (got %g)", level);
    return BMM_OK;
}
int cb_check_members(const bmm_credible_ball_out& o, int64_t N) {
    if (!o.sim || !o.member_idx) return BMM_OK;
    if (o.member_M < 1) return set_err(BMM_E_ARG, "credible ball: member_M must be >= 1 with member_idx (got %lld)", (long long)o.member_M);
    for (int64_t u = 0; u < o.member_M; ++u)
        if (o.member_idx[u] < 0 || o.member_idx[u] >= N)
            return set_err(BMM_E_ARG, "credible ball: member_idx[%lld] = %lld is outside 0 .. %lld", (long long)u, (long long)o.member_idx[u], (long long)(N - 1));
    return BMM_OK;
}

struct CbWork {
    int S = 0, Kc = 0, Ka = 0;
    int64_t N = 0, M = 0;
    CbPlan plan;
    DevBuf T, n, c, d2, w, k;
    int alloc(int S_, int64_t N_, int Kc_, int Ka_, int criterion, const bmm_credible_ball_out& o) {
        S = S_; N = N_; Kc = Kc_; Ka = Ka_;
        M = o.sim ? (o.member_idx ? o.member_M : N) : 0;
        plan = cb_plan(S, N, Kc, Ka, criterion, M > 0 ? M : N, o.sim && o.member_idx);
        HIP_TRY(T.alloc(plan.table_bytes));
        HIP_TRY(n.alloc((size_t)plan.KaP * sizeof(uint32_t)));
        HIP_TRY(c.alloc((size_t)N * sizeof(int32_t)));
        HIP_TRY(d2.alloc((size_t)S * sizeof(uint64_t)));
        HIP_TRY(w.alloc((size_t)S * sizeof(double)));
        HIP_TRY(k.alloc((size_t)S * sizeof(int32_t)));
        return BMM_OK;
    }
};
// tables, sizes, d2, w and k of the centre in w.c (0-based slots) over the label block: everything enqueued on st
int cb_distances(hipStream_t st, CbWork& w, const uint8_t* lab) {
    const CbPlan& p = w.plan;
    HIP_TRY(hipMemsetAsync(w.T.p, 0, p.table_bytes, st));
    HIP_TRY(hipMemsetAsync(w.n.p, 0, (size_t)p.KaP * sizeof(uint32_t), st));
    const dim3 grid((unsigned)((w.N + p.span - 1) / p.span), (unsigned)w.S);
    const size_t lds = ((size_t)w.Kc * p.KaP + p.KaP) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_ps_tables, grid, dim3(256), lds, st, lab, p.pitch, w.N, w.Kc, p.KaP, p.span, w.c.as<int32_t>(), w.T.as<uint32_t>(), w.n.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (p.vi) hipLaunchKernelGGL(k_ps_total<true>, dim3(w.S), dim3(256), 0, st, w.T.as<uint32_t>(), w.n.as<uint32_t>(), w.Kc, w.Ka, p.KaP, w.d2.as<uint64_t>(), w.w.as<double>());
    else hipLaunchKernelGGL(k_ps_total<false>, dim3(w.S), dim3(256), 0, st, w.T.as<uint32_t>(), w.n.as<uint32_t>(), w.Kc, w.Ka, p.KaP, w.d2.as<uint64_t>(), w.w.as<double>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cb_sizes, dim3(w.S), dim3(256), 0, st, w.T.as<uint32_t>(), w.Kc, w.Ka, p.KaP, w.k.as<int32_t>());
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// sim of the chosen rows from the tables cb_distances left, out to the caller; waits for st
int cb_member(hipStream_t st, CbWork& w, const uint8_t* lab, const bmm_credible_ball_out& o) {
    const CbPlan& p = w.plan;
    const int64_t M = w.M;
    const size_t sim_bytes = (size_t)M * w.Ka * sizeof(uint64_t);
    DevBuf didx, g, sim;
    HIP_TRY(sim.alloc(sim_bytes));
    const uint8_t* rows = lab;
    int64_t pitch = p.pitch;
    if (p.gathered) {  // the labels of the subset once, [S][M]
        HIP_TRY(didx.alloc((size_t)M * sizeof(int64_t)));
        HIP_TRY(g.alloc((size_t)w.S * M));
        HIP_TRY(hipMemcpyAsync(didx.p, o.member_idx, (size_t)M * sizeof(int64_t), hipMemcpyHostToDevice, st));
        const dim3 gg((unsigned)((M + 255) / 256), (unsigned)w.S);
        hipLaunchKernelGGL(k_pt_gather<uint8_t>, gg, dim3(256), 0, st, lab, p.pitch, didx.as<int64_t>(), M, g.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        rows = g.as<uint8_t>();
        pitch = M;
    }
    hipLaunchKernelGGL(k_cb_member, dim3((unsigned)p.wgs), dim3(256), p.lds_bytes, st, rows, pitch, w.S, w.Kc, w.Ka, p.KaP, p.nch, p.rows, p.D,
                       w.T.as<uint32_t>(), M, sim.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o.sim, sim.p, sim_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BMM_OK;
}
// The ball and its three bounds from D_t and k_t as the device produced them (the header's definitions), on the host
struct CbBound { int sweep = -1, ties = 0, k = 0; };
struct CbBall { int m = 0, at = -1, n_in = 0; CbBound hor, up, lo; };  // at: the m-th draw in the order (D_t, t)
template <class V>
CbBall cb_ball(const V* D, const int32_t* k, int S, double level) {
    CbBall r;
    std::vector<int> order((size_t)S);
    for (int t = 0; t < S; ++t) order[(size_t)t] = t;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return D[a] < D[b] || (D[a] == D[b] && a < b); });
    double mm = std::ceil(level * (double)S);
    if (mm < 1.0) mm = 1.0;
    r.m = mm > (double)S ? S : (int)mm;
    r.at = order[(size_t)r.m - 1];
    const V radius = D[r.at];
    int kmin = INT32_MAX, kmax = INT32_MIN;
    for (int t = 0; t < S; ++t)
        if (D[t] <= radius) { ++r.n_in; kmin = k[t] < kmin ? k[t] : kmin; kmax = k[t] > kmax ? k[t] : kmax; }
    // the lowest draw of the ball with the largest D among those with k_t = kk (kk < 0: any k_t)
    auto bound = [&](int kk) {
        CbBound b;
        for (int t = 0; t < S; ++t) {
            if (!(D[t] <= radius) || (kk >= 0 && k[t] != kk)) continue;
            if (b.sweep < 0 || D[t] > D[b.sweep]) { b.sweep = t; b.ties = 1; }
            else if (D[t] == D[b.sweep]) ++b.ties;
        }
        b.k = k[b.sweep];
        return b;
    };
    r.hor = bound(-1);
    r.up = bound(kmin);
    r.lo = bound(kmax);
    return r;
}
// After the stream has been waited for: d2, w, k and the sizes read back, the ball chosen, the outputs filled.
// row(t, dst) copies draw t, 1-based, into dst; `first` is added to every reported draw (the rows a run left out).
template <class RowFn>
int cb_finish(CbWork& w, double level, const bmm_credible_ball_out& o, int first, RowFn row) {
    const int S = w.S;
    std::vector<uint64_t> d2((size_t)S);
    std::vector<double> wv((size_t)S);
    std::vector<int32_t> k((size_t)S);
    std::vector<uint32_t> n((size_t)w.plan.KaP);
    HIP_TRY(hipMemcpy(d2.data(), w.d2.p, (size_t)S * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(wv.data(), w.w.p, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(k.data(), w.k.p, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n.data(), w.n.p, n.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const bool vi = w.plan.vi != 0;
    auto dist_of = [&](int t) { return vi ? wv[(size_t)t] / (double)w.N : (double)d2[(size_t)t] / 2.0; };
    const CbBall b = vi ? cb_ball(wv.data(), k.data(), S, level) : cb_ball(d2.data(), k.data(), S, level);
    for (int t = 0; t < S; ++t) {
        if (o.d2) o.d2[t] = d2[(size_t)t];
        if (o.dist) o.dist[t] = dist_of(t);
        if (o.n_clusters) o.n_clusters[t] = k[(size_t)t];
    }
    if (o.radius) *o.radius = dist_of(b.at);
    if (o.radius2) *o.radius2 = d2[(size_t)b.at];
    if (o.n_in) *o.n_in = b.n_in;
    if (o.sizes) for (int a = 0; a < w.Ka; ++a) o.sizes[a] = (int64_t)n[(size_t)a];
    const bmm_credible_bound* const dst[3] = {&o.horizontal, &o.upper, &o.lower};
    const CbBound* const src[3] = {&b.hor, &b.up, &b.lo};
    for (int q = 0; q < 3; ++q) {
        const bmm_credible_bound& h = *dst[q];
        const CbBound& s = *src[q];
        if (h.sweep) *h.sweep = first + s.sweep;
        if (h.ties) *h.ties = s.ties;
        if (h.n_clusters) *h.n_clusters = s.k;
        if (h.dist) *h.dist = dist_of(s.sweep);
        if (h.d2) *h.d2 = d2[(size_t)s.sweep];
        if (h.z) { const int rc = row(s.sweep, h.z); if (rc) return rc; }
    }
    return BMM_OK;
}

// The summary of a run (bmm_set_partition_summary): what the run checks of it before any device is touched
int pt_run_check(const RunOptions& opts, int S, int64_t N, int K) {
    if (opts.psearch.on) {
        if (!opts.partition.on) return set_err(BMM_E_ARG, "partition search: needs an armed partition summary (bmm_set_partition_summary)");
        PsOpts r;
        int rc = ps_check(S, N, K, opts.partition.o.criterion, opts.psearch.has_opts ? &opts.psearch.opts : nullptr, true, r);
        if (rc == BMM_OK) rc = ps_check_out(&opts.psearch.o);
        if (rc) return rc;
    }
    if (opts.cball.on) {
        if (!opts.partition.on) return set_err(BMM_E_ARG, "credible ball: needs an armed partition summary (bmm_set_partition_summary)");
        const int Ka = opts.psearch.on && opts.psearch.has_opts ? opts.psearch.opts.max_clusters : K;
        int rc = cb_check(S, N, K, opts.partition.o.criterion, Ka, opts.cball.level);
        if (rc == BMM_OK) rc = cb_check_members(opts.cball.o, N);
        if (rc) return rc;
    }
    if (!opts.partition.on) return BMM_OK;
    const bmm_partition_out& o = opts.partition.o;
    if (!o.loss || !o.best || !o.n_used) return set_err(BMM_E_ARG, "partition: null buffer (loss, best, n_used)");
    int rc = pt_check_shape(S, N, K, o.criterion, o.stride);
    if (rc) return rc;
    if (o.psm_M < 0 || (o.psm_M > 0 && (!o.psm_idx || !o.psm_cnt))) return set_err(BMM_E_ARG, "similarity: null buffer or negative count");
    return pt_check_idx(o.psm_idx, o.psm_M, N);
}
// after the last sweep, before the trace leaves: everything on the chain's stream, then one wait
int pt_run_summary(bmm_chain* c, const bmm_partition_out& o, const RunOptions& opts) {
    const int64_t N = c->p.N;
    const int first = (c->burnin == 0 && c->p.mode != MODE_COLLAPSED) ? 1 : 0;  // row 0: the unassigned starting state
    const int Su = c->S - first;
    *o.n_used = Su;
    *o.best = -1;
    if (Su < 1) return BMM_OK;
    PtWork w;
    w.shape(Su, N, c->p.K, o.criterion, o.stride);
    int rc = w.alloc_labels();
    if (rc == BMM_OK) rc = w.alloc_pairs(o.dist != nullptr);
    if (rc == BMM_OK) rc = pt_narrow(c->stream, w, c->dTrace + (size_t)first * N, N, 1, 0, 0, N);
    if (rc == BMM_OK) rc = pt_compute(c->stream, w);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    int best = -1;
    rc = pt_fetch(w, o.loss, o.binder2, &best, o.dist);
    if (rc) return rc;
    *o.best = first + best;
    if (o.z_best) {
        HIP_TRY(hipMemcpy(o.z_best, c->dTrace + (size_t)(first + best) * N, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < N; ++i) o.z_best[i] += 1;
    }
    if (o.psm_M > 0) rc = pt_psm(c->stream, w, o.psm_idx, o.psm_M, o.psm_cnt);
    PsWork sw;
    int Ka = c->p.K;
    if (rc == BMM_OK && opts.psearch.on) {  // the greedy search from the chosen row, over the rows the summary used
        PsOpts r;
        rc = ps_check(Su, N, c->p.K, o.criterion, opts.psearch.has_opts ? &opts.psearch.opts : nullptr, true, r);
        if (rc) return rc;
        rc = sw.alloc(Su, N, c->p.K, r.Ka, o.criterion, r.batch);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(sw.c.p, c->dTrace + (size_t)(first + best) * N, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        rc = ps_search(c->stream, sw, w.lab.as<uint8_t>(), r, opts.psearch.o);
        Ka = r.Ka;
    }
    if (rc == BMM_OK && opts.cball.on) {  // the credible ball around the searched partition, else around the chosen row
        const bmm_credible_ball_out& bo = opts.cball.o;
        CbWork bw;
        rc = bw.alloc(Su, N, c->p.K, Ka, o.criterion, bo);
        if (rc) return rc;
        const int32_t* const centre = opts.psearch.on ? sw.best.as<int32_t>() : c->dTrace + (size_t)(first + best) * N;
        HIP_TRY(hipMemcpyAsync(bw.c.p, centre, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        rc = cb_distances(c->stream, bw, w.lab.as<uint8_t>());
        if (rc == BMM_OK && bw.M > 0) rc = cb_member(c->stream, bw, w.lab.as<uint8_t>(), bo);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        HIP_TRY(hipStreamSynchronize(c->stream));
        rc = cb_finish(bw, opts.cball.level, bo, first, [&](int t, int32_t* dst) -> int {
            HIP_TRY(hipMemcpy(dst, c->dTrace + (size_t)(first + t) * N, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < N; ++i) dst[i] += 1;
            return BMM_OK;
        });
    }
    return rc;
}

// ---- ECR relabelling from the label trace (include/bmm_mcmc.h) ----
// Which form of the k_ecr_* kernels a shape runs: a pure function of (S, N, K) -- the launches below and
// bmm_device_ecr_plan both read it from here.
constexpr size_t kEcrLdsBudget = (size_t)48 << 10;  // bytes of tables, or of vote counters, per workgroup
struct EcrPlan {
    int tab_lds = 1, T = 1, R = 1, row_blocks = 1, slices = 1, votes_lds = 1, votes_wgs = 1;
    int64_t span = 0, pitch = 0;
    size_t tab_lds_bytes = 0, votes_bytes = 0;
};
EcrPlan ecr_plan(int S, int64_t N, int K) {
    EcrPlan p;
    const size_t copy = ((size_t)K * K | 1) * sizeof(uint32_t);
    p.pitch = (N + 15) / 16 * 16;
    p.tab_lds = copy <= kEcrLdsBudget ? 1 : 0;
    p.T = S < kEcrMaxRows ? S : kEcrMaxRows;
    if (p.tab_lds) {
        if ((size_t)p.T * copy > kEcrLdsBudget) p.T = (int)(kEcrLdsBudget / copy);
        while (p.R < kEcrMaxCopies && (size_t)p.T * (2 * p.R) * copy <= kEcrLdsBudget) p.R *= 2;
        p.tab_lds_bytes = (size_t)p.T * p.R * copy;
    }
    p.row_blocks = (S + p.T - 1) / p.T;
    // along N: slices of at least 1024 observations, as many as bring the grid to some 2048 workgroups
    int64_t sl = (N + 1023) / 1024, cap = 2048 / p.row_blocks;
    if (cap < 1) cap = 1;
    if (sl > cap) sl = cap;
    p.span = ((N + sl - 1) / sl + kEcrThreads - 1) / kEcrThreads * kEcrThreads;
    p.slices = (int)((N + p.span - 1) / p.span);
    const size_t words = (size_t)(K + 1) / 2;
    p.votes_lds = words * kEcrThreads * sizeof(uint32_t) <= kEcrLdsBudget ? 1 : 0;
    int64_t wg = (N + kEcrThreads - 1) / kEcrThreads;
    const int64_t wg_cap = p.votes_lds ? 4096 : 1024;
    p.votes_wgs = (int)(wg < wg_cap ? wg : wg_cap);
    p.votes_bytes = words * kEcrThreads * sizeof(uint32_t) * (p.votes_lds ? 1 : (size_t)p.votes_wgs);
    return p;
}
int ecr_check_shape(int S, int64_t N, int K) {
    if (S < 1) return set_err(BMM_E_ARG, "ecr: S must be >= 1");
    if (N < 1) return set_err(BMM_E_ARG, "ecr: N must be >= 1");
    if (N >= ((int64_t)1 << 32)) return set_err(BMM_E_ARG, "ecr: N must be below 2^32 (the tables are uint32)");
    if (S > BMM_PARTITION_MAX_ROWS) return set_err(BMM_E_ARG, "ecr: S = %d rows is more than the %d one call takes", S, BMM_PARTITION_MAX_ROWS);
    if (K < 1 || K > BMM_ECR_MAX_K) return set_err(BMM_E_ARG, "ecr: K must be in 1 .. %d (got %d)", BMM_ECR_MAX_K, K);
    return BMM_OK;
}

struct EcrWork {
    int S = 0, K = 0;
    int64_t N = 0;
    EcrPlan plan;
    DevBuf tables, cost, agree, total, pivot, scratch;
    PinnedBuf htotal;
    int alloc(int S_, int64_t N_, int K_, bool own_pivot) {
        S = S_; N = N_; K = K_;
        plan = ecr_plan(S, N, K);
        const size_t kk = (size_t)K * K;
        HIP_TRY(tables.alloc((size_t)S * kk * sizeof(uint32_t)));
        HIP_TRY(cost.alloc((size_t)S * kk * sizeof(double)));
        HIP_TRY(agree.alloc((size_t)S * sizeof(int64_t)));
        HIP_TRY(total.alloc(sizeof(unsigned long long)));
        HIP_TRY(htotal.alloc(sizeof(unsigned long long)));
        if (own_pivot) HIP_TRY(pivot.alloc((size_t)N * sizeof(int32_t)));
        if (!plan.votes_lds) HIP_TRY(scratch.alloc(plan.votes_bytes));
        return BMM_OK;
    }
};
// The permutations of S rows (row t at lab + t * pitch) against the pivot: given (iterative = false: one pass) or voted
// per iteration.  perm: the rows' part of a device table with leading dimension ld, holding the identity on entry.
// Everything is enqueued on st; the iterative form waits once per iteration for the 8 bytes of total_it.
template <class L>
int ecr_compute(hipStream_t st, EcrWork& w, const L* lab, int64_t pitch, int32_t* pivot, int32_t* perm, int64_t ld,
                bool iterative, int max_iter, int* iterations, int* converged) {
    const EcrPlan& p = w.plan;
    const int S = w.S, K = w.K, KK = K * K;
    uint32_t* const tabs = w.tables.as<uint32_t>();
    long long prev = -1;
    *iterations = 0;
    *converged = iterative ? 0 : 1;
    for (int it = 1; it <= (iterative ? max_iter : 1); ++it) {
        if (iterative) {
            if (p.votes_lds) hipLaunchKernelGGL((k_ecr_votes<L, true>), dim3((unsigned)p.votes_wgs), dim3(kEcrThreads), p.votes_bytes, st, lab, pitch, perm, ld, w.N, S, K, (uint32_t*)nullptr, pivot);
            else hipLaunchKernelGGL((k_ecr_votes<L, false>), dim3((unsigned)p.votes_wgs), dim3(kEcrThreads), 0, st, lab, pitch, perm, ld, w.N, S, K, w.scratch.as<uint32_t>(), pivot);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(tabs, 0, (size_t)S * KK * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(w.total.p, 0, sizeof(unsigned long long), st));
        const dim3 grid((unsigned)p.slices, (unsigned)p.row_blocks);
        if (p.tab_lds) hipLaunchKernelGGL((k_ecr_tables<L, true>), grid, dim3(kEcrThreads), p.tab_lds_bytes, st, lab, pitch, pivot, w.N, S, K, p.T, p.R, p.span, tabs);
        else hipLaunchKernelGGL((k_ecr_tables<L, false>), grid, dim3(kEcrThreads), 0, st, lab, pitch, pivot, w.N, S, K, p.T, p.R, p.span, tabs);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ecr_cost, dim3((unsigned)((KK + kEcrThreads - 1) / kEcrThreads), (unsigned)S), dim3(kEcrThreads), 0, st, tabs, KK, w.cost.as<double>());
        HIP_TRY(hipGetLastError());
        const int rc = st_assign(st, w.cost.as<double>(), K, S, perm, ld);
        if (rc) return rc;
        hipLaunchKernelGGL(k_ecr_agree, dim3((unsigned)S), dim3(64), 0, st, tabs, K, perm, ld, w.agree.as<int64_t>(), w.total.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        *iterations = it;
        if (!iterative) break;
        HIP_TRY(hipMemcpyAsync(w.htotal.p, w.total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // the one round trip of an iteration
        const long long total = (long long)*w.htotal.as<unsigned long long>();
        if (total == prev) { *converged = 1; break; }
        prev = total;
    }
    return BMM_OK;
}
int ecr_perm_identity(hipStream_t st, int32_t* perm, int S, int K) {
    hipLaunchKernelGGL(k_st_perm_identity, dim3((unsigned)((S * K + 255) / 256)), dim3(256), 0, st, perm, S, K);
    HIP_TRY(hipGetLastError());
    return BMM_OK;
}
// N labels, 1-based, every one in 1 .. K
int ecr_check_pivot(const int32_t* pivot, int64_t N, int K) {
    for (int64_t i = 0; i < N; ++i)
        if (pivot[i] < 1 || pivot[i] > K)
            return set_err(BMM_E_ARG, "ecr: pivot label %d at observation %lld (0-based) is outside 1 .. %d", pivot[i], (long long)i, K);
    return BMM_OK;
}
int ecr_upload_pivot(int32_t* dpivot, const int32_t* pivot, int64_t N, hipStream_t st) {
    std::vector<int32_t> h((size_t)N);
    for (int64_t i = 0; i < N; ++i) h[(size_t)i] = pivot[i] - 1;
    HIP_TRY(hipMemcpyAsync(dpivot, h.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // before the host copy goes
    return BMM_OK;
}

// ECR armed for a run (bmm_set_ecr_relabel): what the run checks of it before any device is touched
int ecr_run_check(const RunOptions& opts, int S, int64_t N, int K) {
    if (!opts.ecr.on) return BMM_OK;
    const bmm_ecr_out& o = opts.ecr.o;
    if (opts.alloc.on)
        return set_err(BMM_E_UNSUPPORTED, "ecr: the allocation sampler is not offered together with relabelling: it assumes no fixed number of components");
    if (opts.rel || opts.hooks)
        return set_err(BMM_E_ARG, "ecr: armed together with Stephens' relabelling (a *_run_relabel call or *_run_probs hooks): two relabellings of one run");
    if (!o.permutations || !o.z_original || !o.theta_original || !o.agree || !o.iterations || !o.converged || !o.n_used)
        return set_err(BMM_E_ARG, "ecr: null buffer");
    int rc = ecr_check_shape(S, N, K);
    if (rc) return rc;
    switch (o.pivot_kind) {
        case BMM_ECR_PIVOT_GIVEN:
            if (!o.pivot) return set_err(BMM_E_ARG, "ecr: the pivot is null");
            return ecr_check_pivot(o.pivot, N, K);
        case BMM_ECR_PIVOT_PARTITION:
            if (!opts.partition.on) return set_err(BMM_E_ARG, "ecr: the partition pivot needs an armed partition summary (bmm_set_partition_summary)");
            return BMM_OK;
        case BMM_ECR_PIVOT_ITERATIVE:
            if (o.max_iter < 1) return set_err(BMM_E_ARG, "ecr: max_iter must be >= 1 (got %d)", o.max_iter);
            return BMM_OK;
        default: return set_err(BMM_E_ARG, "ecr: unknown kind of pivot %d", o.pivot_kind);
    }
}
// after the last sweep and the partition summary, before the trace leaves: the S x K table of permutations into perm
int ecr_run(bmm_chain* c, const RunOptions& opts, DevBuf& perm) {
    const bmm_ecr_out& o = opts.ecr.o;
    const int64_t N = c->p.N;
    const int S = c->S, K = c->p.K;
    const int first = (c->burnin == 0 && c->p.mode != MODE_COLLAPSED) ? 1 : 0;  // row 0: the unassigned starting state
    const int Su = S - first;
    *o.n_used = Su;
    *o.iterations = 0;
    *o.converged = 1;
    for (int s = 0; s < S; ++s) o.agree[s] = 0;
    HIP_TRY(perm.alloc((size_t)S * K * sizeof(int32_t)));
    int rc = ecr_perm_identity(c->stream, perm.as<int32_t>(), S, K);
    if (rc) return rc;
    int32_t* pivot = nullptr;  // 0-based, on the device
    if (o.pivot_kind == BMM_ECR_PIVOT_PARTITION) {
        const int best = *opts.partition.o.best;
        if (best >= 0) pivot = c->dTrace + (size_t)best * N;
    }
    if (Su < 1 || (o.pivot_kind == BMM_ECR_PIVOT_PARTITION && !pivot)) {
        if (o.pivot_out) for (int64_t i = 0; i < N; ++i) o.pivot_out[i] = 0;
        return BMM_OK;
    }
    EcrWork w;
    rc = w.alloc(Su, N, K, pivot == nullptr);
    if (rc) return rc;
    if (!pivot) pivot = w.pivot.as<int32_t>();
    if (o.pivot_kind == BMM_ECR_PIVOT_GIVEN) rc = ecr_upload_pivot(pivot, o.pivot, N, c->stream);
    if (rc == BMM_OK)
        rc = ecr_compute<int32_t>(c->stream, w, c->dTrace + (size_t)first * N, N, pivot, perm.as<int32_t>() + first, S,
                                  o.pivot_kind == BMM_ECR_PIVOT_ITERATIVE, o.max_iter, o.iterations, o.converged);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(hipMemcpyAsync(o.agree + first, w.agree.p, (size_t)Su * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (o.pivot_out) HIP_TRY(hipMemcpyAsync(o.pivot_out, pivot, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // before the work buffers go
    if (o.pivot_out) for (int64_t i = 0; i < N; ++i) o.pivot_out[i] += 1;
    return BMM_OK;
}

// ---- posterior summary: online pivot relabelling, memberships folded behind the sweeps (include/bmm_mcmc.h "posterior
// summary") ----
// The launch shapes and the block's bytes: a pure function of (N, P, K) -- the launches below, bmm_summary_plan and
// bmm_run_bytes all read it from here.  k_sum_fold and k_sum_finish stride a grid of at most kSumGridCap workgroups
// (eight of 256 threads per compute unit of a 256-unit device).
constexpr int kSumGridCap = 2048;
constexpr int kSumLaunchesPivot = 8;  // two memsets, k_ecr_tables, k_ecr_cost, k_st_assign, k_ecr_agree, k_sum_fold, k_sum_profiles
constexpr int kSumLaunchesPlain = 2;  // k_sum_fold, k_sum_profiles
void sum_carve(Carver& v, SumBufs& b, int64_t N, int P, int K, int64_t pitch) {
    const size_t Kz = (size_t)K, KP = Kz * (size_t)P;
    b.cnt = v.take<uint32_t>(Kz * (size_t)pitch);
    b.theta_sum = v.take<double>(KP);
    b.theta_sq = v.take<double>(KP);
    b.alpha_acc = v.take<double>(2);
    b.theta_n = v.take<int32_t>(Kz);
    b.fold_bytes = v.used;  // what a reset zeroes: the five above
    b.size_sum = v.take<unsigned long long>(Kz);
    b.pivot = v.take<int32_t>((size_t)N);
    b.z_hat = v.take<int32_t>((size_t)N);
    b.n_max = v.take<uint32_t>((size_t)N);
    b.identity = v.take<int32_t>(Kz);
    b.perm_live = v.take<int32_t>(Kz);
    b.agree_live = v.take<int64_t>(1);
    b.theta_row = v.take<double>(KP);
    b.alpha_row = v.take<double>(1);
}
struct SumPlan {
    int fold_wgs = 1, prof_wgs = 1, finish_wgs = 1;
    int64_t pitch = 0;
    size_t fold_lds = 0, finish_lds = 0, bytes_counts = 0, bytes_block = 0;
};
SumPlan sum_plan(int64_t N, int P, int K) {
    SumPlan q;
    q.pitch = (N + 63) / 64 * 64;
    const int64_t wg = (N + kSumThreads - 1) / kSumThreads;
    q.fold_wgs = q.finish_wgs = (int)(wg < kSumGridCap ? wg : kSumGridCap);
    q.prof_wgs = (int)(((int64_t)K * P + kSumThreads - 1) / kSumThreads);
    q.fold_lds = (size_t)K * sizeof(int32_t);
    q.finish_lds = (size_t)K * sizeof(unsigned long long);
    q.bytes_counts = (size_t)K * (size_t)q.pitch * sizeof(uint32_t);
    Carver measure{nullptr};
    SumBufs b;
    sum_carve(measure, b, N, P, K, q.pitch);
    q.bytes_block = measure.used;
    return q;
}
// the bytes of a recorded sweep: its agreement, then its permutation
size_t sum_row_bytes(int K) { return (sizeof(int64_t) + (size_t)K * sizeof(int32_t) + 7) & ~(size_t)7; }

// stride, N, K and the pivot, before a device is touched
int sum_check_args(int64_t N, int K, const bmm_summary_opts& o) {
    if (o.stride < 1) return set_err(BMM_E_ARG, "summary: stride must be >= 1 (got %d)", o.stride);
    if (N >= ((int64_t)1 << 32)) return set_err(BMM_E_ARG, "summary: N must be below 2^32 (the counts are uint32)");
    if (o.pivot_kind == BMM_SUMMARY_PIVOT_NONE) return BMM_OK;
    if (o.pivot_kind != BMM_SUMMARY_PIVOT_FIRST && o.pivot_kind != BMM_SUMMARY_PIVOT_GIVEN)
        return set_err(BMM_E_ARG, "summary: unknown kind of pivot %d", o.pivot_kind);
    if (K > BMM_ECR_MAX_K)
        return set_err(BMM_E_ARG, "summary: relabelling against a pivot is offered up to K = %d (got %d); without a pivot any K is folded as sampled", BMM_ECR_MAX_K, K);
    if (o.pivot_kind == BMM_SUMMARY_PIVOT_FIRST) return BMM_OK;
    if (!o.pivot) return set_err(BMM_E_ARG, "summary: the pivot is null");
    for (int64_t i = 0; i < N; ++i)
        if (o.pivot[i] < 1 || o.pivot[i] > K)
            return set_err(BMM_E_ARG, "summary: pivot label %d at observation %lld (0-based) is outside 1 .. %d", o.pivot[i], (long long)i, K);
    return BMM_OK;
}
int sum_refused(const bmm_chain* c) {
    if (c->sharded) return set_err(BMM_E_UNSUPPORTED, "the summary is not offered on a sharded chain: a shard holds a part of the rows");
    if (c->alloc_on) return set_err(BMM_E_UNSUPPORTED, "the summary is not offered for the allocation sampler: it assumes no fixed number of components");
    if (c->temper_on || c->ladder) return temper_refuses("the summary");
    return BMM_OK;
}
void sum_release(bmm_chain* c) {
    delete c->sum_ecr;
    c->sum_ecr = nullptr;
    if (c->dSumBlock) dev_pool().put(c->device, c->dSumBlock, c->sum_block_bytes);
    c->dSumBlock = nullptr; c->sum_block_bytes = 0;
    c->sum = SumBufs{};
    c->sum_on = false; c->sum_have_pivot = false; c->sum_folded = 0;
}
int sum_reset(bmm_chain* c) {
    c->sum_folded = 0;
    if (c->sum_pivot_kind == BMM_SUMMARY_PIVOT_FIRST) c->sum_have_pivot = false;
    HIP_TRY(hipMemsetAsync(c->dSumBlock, 0, c->sum.fold_bytes, c->stream));
    return BMM_OK;
}
// the block from the device pool, zeroed; the workspace of one row's ECR pass; a given pivot uploaded.  The stream is idle.
int sum_arm(bmm_chain* c, const bmm_summary_opts& o) {
    int rc = sum_refused(c);
    if (rc == BMM_OK) rc = sum_check_args(c->p.N, c->p.K, o);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    sum_release(c);
    const int64_t N = c->p.N;
    const int K = c->p.K;
    const SumPlan q = sum_plan(N, c->p.P, K);
    c->dSumBlock = static_cast<char*>(dev_pool().get(c->device, q.bytes_block, &c->sum_block_bytes));
    if (!c->dSumBlock) return set_err(BMM_E_HIP, "allocating the summary's buffers (%zu bytes) failed: %s", q.bytes_block, hipGetErrorString(hipGetLastError()));
    Carver real{c->dSumBlock};
    sum_carve(real, c->sum, N, c->p.P, K, q.pitch);
    c->sum_pitch = q.pitch;
    HIP_TRY(hipMemsetAsync(c->dSumBlock, 0, q.bytes_block, c->stream));
    rc = ecr_perm_identity(c->stream, c->sum.identity, 1, K);
    if (rc == BMM_OK) rc = ecr_perm_identity(c->stream, c->sum.perm_live, 1, K);
    if (rc == BMM_OK && o.pivot_kind != BMM_SUMMARY_PIVOT_NONE) {
        c->sum_ecr = new EcrWork();
        rc = c->sum_ecr->alloc(1, N, K, false);
    }
    if (rc == BMM_OK && o.pivot_kind == BMM_SUMMARY_PIVOT_GIVEN) rc = ecr_upload_pivot(c->sum.pivot, o.pivot, N, c->stream);
    if (rc) { (void)hipStreamSynchronize(c->stream); sum_release(c); return rc; }
    c->sum_pivot_kind = o.pivot_kind; c->sum_stride = o.stride;
    c->sum_have_pivot = o.pivot_kind == BMM_SUMMARY_PIVOT_GIVEN;
    c->sum_folded = 0;
    c->sum_on = true;
    return BMM_OK;
}
// the _FIRST pivot: the labels of a kept state, device to device
int sum_take_pivot(bmm_chain* c, const int32_t* z) {
    HIP_TRY(hipMemcpyAsync(c->sum.pivot, z, (size_t)c->p.N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    c->sum_have_pivot = true;
    return BMM_OK;
}
// one row's permutation against the pivot into perm (K entries, the identity on entry): the pass of "ECR" with S = 1
int sum_relabel(bmm_chain* c, const int32_t* z, int32_t* perm) {
    int iterations = 0, converged = 0;
    return ecr_compute<int32_t>(c->stream, *c->sum_ecr, z, c->p.N, c->sum.pivot, perm, 1, false, 1, &iterations, &converged);
}
// the end of sweep j of an armed chain: the _FIRST pivot when j is the first kept sweep, then the fold when the
// stride names j.  Everything is enqueued; nothing waits.
int sum_sweep_end(bmm_chain* c, int j) {
    const SweepTrace& r = c->sum_rec;
    if (!r.fold || j < r.base) return BMM_OK;
    if (c->sum_pivot_kind == BMM_SUMMARY_PIVOT_FIRST && !c->sum_have_pivot) {
        const int rc = sum_take_pivot(c, label_row(c, j));
        if (rc) return rc;
    }
    if (!stride_folds(r, c->sum_stride, j)) return BMM_OK;
    const int64_t N = c->p.N;
    const int K = c->p.K, P = c->p.P;
    const SumPlan q = sum_plan(N, P, K);
    const int32_t* const z = label_row(c, j);
    char* const row = r.row<char>(j);
    int64_t* const agree_out = row ? reinterpret_cast<int64_t*>(row) : c->sum.agree_live;
    const int32_t* perm = c->sum.identity;
    const int64_t* agree_in = nullptr;
    if (c->sum_pivot_kind != BMM_SUMMARY_PIVOT_NONE) {
        int32_t* const perm_row = row ? reinterpret_cast<int32_t*>(row + sizeof(int64_t)) : c->sum.perm_live;
        const int rc = sum_relabel(c, z, perm_row);
        if (rc) return rc;
        perm = perm_row;
        agree_in = c->sum_ecr->agree.as<int64_t>();
    }
    hipLaunchKernelGGL(k_sum_fold, dim3((unsigned)q.fold_wgs), dim3(kSumThreads), q.fold_lds, c->stream, z, perm, N, K, c->sum_pitch, c->sum.cnt);
    HIP_TRY(hipGetLastError());
    const bool rec = c->in_run && j >= c->burnin;  // the sweep's rows of the run's traces, or the rows enqueue_sweep had written for the fold
    const double* const theta = rec ? c->dThetaTrace + (size_t)(j - c->burnin) * K * P : c->sum.theta_row;
    const double* const alpha = rec ? c->dAlphaTrace + (j - c->burnin) : c->sum.alpha_row;
    hipLaunchKernelGGL(k_sum_profiles, dim3((unsigned)q.prof_wgs), dim3(kSumThreads), 0, c->stream, theta, alpha, perm, K, P, c->sum.theta_sum,
                       c->sum.theta_sq, c->sum.theta_n, c->sum.alpha_acc, agree_in, agree_out);
    HIP_TRY(hipGetLastError());
    c->sum_folded++;
    return BMM_OK;
}
// the starting state of a finite collapsed run without burn-in is trace row 0: the _FIRST pivot (chain_start)
int sum_start_state(bmm_chain* c, const int32_t* row0) {
    if (c->sum_pivot_kind != BMM_SUMMARY_PIVOT_FIRST || c->sum_have_pivot || !c->sum_rec.fold || c->sum_rec.base != 0) return BMM_OK;
    return sum_take_pivot(c, row0);
}
// k_sum_finish, then whatever `out` asks for to the host; waits
int sum_get(bmm_chain* c, const bmm_summary_out& out) {
    const int64_t N = c->p.N;
    const int K = c->p.K, P = c->p.P;
    const SumPlan q = sum_plan(N, P, K);
    const size_t Kz = (size_t)K, KP = Kz * (size_t)P, Nz = (size_t)N;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->sum.size_sum, 0, Kz * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_sum_finish, dim3((unsigned)q.finish_wgs), dim3(kSumThreads), q.finish_lds, c->stream, (const uint32_t*)c->sum.cnt, N, K,
                       c->sum_pitch, c->sum.z_hat, c->sum.n_max, c->sum.size_sum);
    HIP_TRY(hipGetLastError());
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIP_TRY(copy(out.z_hat, c->sum.z_hat, Nz * sizeof(int32_t)));
    HIP_TRY(copy(out.n_max, c->sum.n_max, Nz * sizeof(uint32_t)));
    HIP_TRY(copy(out.size_sum, c->sum.size_sum, Kz * sizeof(int64_t)));
    HIP_TRY(copy(out.theta_sum, c->sum.theta_sum, KP * sizeof(double)));
    HIP_TRY(copy(out.theta_sq, c->sum.theta_sq, KP * sizeof(double)));
    HIP_TRY(copy(out.theta_n, c->sum.theta_n, Kz * sizeof(int32_t)));
    HIP_TRY(copy(out.alpha_sum, c->sum.alpha_acc, 2 * sizeof(double)));
    if (out.pivot && c->sum_have_pivot) HIP_TRY(copy(out.pivot, c->sum.pivot, Nz * sizeof(int32_t)));
    if (out.counts)
        HIP_TRY(hipMemcpy2DAsync(out.counts, Nz * sizeof(uint32_t), c->sum.cnt, (size_t)c->sum_pitch * sizeof(uint32_t), Nz * sizeof(uint32_t), Kz,
                                 hipMemcpyDeviceToHost, c->stream));
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(BMM_E_HIP, "reading the summary failed: %s", hipGetErrorString(e));
    if (out.pivot)
        for (int64_t i = 0; i < N; ++i) out.pivot[i] = c->sum_have_pivot ? out.pivot[i] + 1 : 0;
    if (out.n_folded) *out.n_folded = c->sum_folded;
    return BMM_OK;
}
// rows of (agree, perm) for n sweeps: -1 and the identity until a fold writes them
int sum_rows_alloc(bmm_chain* c, Recording& rec, int n) {
    const int K = c->p.K;
    const size_t width = sum_row_bytes(K);
    int rc = rec.alloc((size_t)n * width, "the summary's per-sweep rows (agreement and permutation)");
    if (rc) return rc;
    std::vector<char> host((size_t)n * width, 0);
    for (int s = 0; s < n; ++s) {
        const int64_t none = -1;
        std::memcpy(host.data() + (size_t)s * width, &none, sizeof none);
        int32_t* const perm = reinterpret_cast<int32_t*>(host.data() + (size_t)s * width + sizeof(int64_t));
        for (int k = 0; k < K; ++k) perm[k] = k;
    }
    HIP_TRY(hipMemcpyAsync(rec.rows.p, host.data(), host.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // before the host copy goes
    return BMM_OK;
}
// ... and out again: agree n int64, permutations n x K column-major
int sum_rows_out(bmm_chain* c, const Recording& rec, int n, int64_t* agree, int32_t* permutations) {
    const int K = c->p.K;
    const size_t width = sum_row_bytes(K);
    std::vector<char> host((size_t)n * width);
    HIP_TRY(hipMemcpy(host.data(), rec.rows.p, host.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < n; ++s) {
        if (agree) std::memcpy(agree + s, host.data() + (size_t)s * width, sizeof(int64_t));
        const int32_t* const perm = reinterpret_cast<const int32_t*>(host.data() + (size_t)s * width + sizeof(int64_t));
        if (permutations) for (int k = 0; k < K; ++k) permutations[(size_t)s + (size_t)k * (size_t)n] = perm[k];
    }
    return BMM_OK;
}

// ... of a run: refused before a device is touched, armed for it, every stride-th kept sweep folded (sweep_end_folds)
int sum_run_check(const RunOptions& opts, int64_t N, int K) {
    if (!opts.summary.on) return BMM_OK;
    if (opts.alloc.on)
        return set_err(BMM_E_UNSUPPORTED, "summary: the allocation sampler is not offered together with the summary: it assumes no fixed number of components");
    if (opts.temper.on) return set_err(BMM_E_UNSUPPORTED, "summary: not offered together with parallel tempering");
    if (opts.ecr.on || opts.rel || opts.hooks)
        return set_err(BMM_E_ARG, "summary: armed together with a relabelling of the run (ECR, a *_run_relabel call or *_run_probs hooks): two relabellings of one run");
    if (!opts.keep_trace() && opts.partition.on)
        return set_err(BMM_E_ARG, "summary: keep_trace = 0 together with the partition summary, which reads the label trace");
    return sum_check_args(N, K, opts.summary.opts);
}
int sum_run_attach(bmm_chain* c, const RunOptions& opts, Recording& rec) {
    if (!opts.summary.on) return BMM_OK;
    int rc = sum_arm(c, opts.summary.opts);
    if (rc == BMM_OK) rc = sum_rows_alloc(c, rec, c->S);
    if (rc) return rc;
    rec.begin(c, c->sum_rec, sum_row_bytes(c->p.K), c->burnin, run_first_fold(c), true);
    return BMM_OK;
}
int sum_run_collect(bmm_chain* c, const RunOptions& opts, Recording& rec, int rc) {
    if (!opts.summary.on) return rc;
    rc = rec.end_run(rc);
    if (rc) return rc;
    rc = sum_get(c, opts.summary.o);
    if (rc || !rec.rows.p) return rc;
    return sum_rows_out(c, rec, c->S, opts.summary.o.agree, opts.summary.o.permutations);
}

// the sweeps, then the traces out (data and starting state are in place)
int run_body(bmm_chain* c, int nsamples, const RunIO& io, const RunOptions& opts) {
    const bmm_relabel_out* const rel = opts.rel;
    const int sampler = c->p.mode, K = c->p.K, P = c->p.P, S = c->S;
    HIP_TRY(hipSetDevice(c->device));
    PhaseClock clock;
    StRun st;
    int rc = BMM_OK;
    if (rel) {
        rc = st_run_prepare(c, st, rel->burnrelabel);
        if (rc) return rc;
        auto step = [&](int j) { return st_run_sweep(c, st, j); };
        if (g_progress.fn && g_progress.every > 0) rc = run_sweeps_reported(c, nsamples, step);
        else for (int j = 1; j < nsamples && rc == BMM_OK; ++j) rc = step(j);
    } else if (c->ladder) {  // parallel tempering: the rungs advance together, this chain is rung 0
        bmm_ladder* const l = c->ladder;
        auto step = [&](int) { return ladder_sweeps(l, 1, l->swap_every); };
        rc = g_progress.fn && g_progress.every > 0 ? run_sweeps_reported(c, nsamples, step) : ladder_sweeps(l, nsamples - 1, l->swap_every);
    } else {
        rc = opts.hooks ? run_sweeps_hooked(c, nsamples, opts.hooks)
                   : (g_progress.fn && g_progress.every > 0 ? run_sweeps_reported(c, nsamples) : bmm_chain_sweeps(c, nsamples - 1));
    }
    if (rc) return rc;
    clock.lap(2);
    // theta, alpha, pi: small, queued behind the sweeps
    HIP_TRY(hipMemcpyAsync(io.theta_out, c->dThetaTrace, (size_t)S * K * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(io.alpha_out, c->dAlphaTrace, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (explicit_params(sampler))
        HIP_TRY(hipMemcpyAsync(io.pi_out, c->dPiTrace, (size_t)S * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (opts.partition.on) {  // the clustering summary, from the resident trace (labels as sampled)
        rc = pt_run_summary(c, opts.partition.o, opts);
        if (rc) return rc;
    }
    DevBuf ecr_perm;
    if (opts.ecr.on) {  // ECR: the permutations from the resident trace, then the trace leaves as a relabelling run's does
        rc = ecr_run(c, opts, ecr_perm);
        if (rc) return rc;
    }
    if (rel || opts.ecr.on) {
        const int32_t* const dperm = rel ? st.perm.as<int32_t>() : ecr_perm.as<int32_t>();
        int32_t* const hperm = rel ? rel->permutations : opts.ecr.o.permutations;
        int32_t* const z_original = rel ? rel->z_original : opts.ecr.o.z_original;
        double* const theta_original = rel ? rel->theta_original : opts.ecr.o.theta_original;
        HIP_TRY(hipMemcpyAsync(hperm, dperm, (size_t)S * K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        rc = trace_out(c, z_original, &clock);
        if (rc == BMM_OK) rc = trace_out(c, io.z_out, nullptr, dperm);
        if (rc) return rc;
        std::memcpy(theta_original, io.theta_out, (size_t)S * K * P * sizeof(double));
        permute_theta(theta_original, hperm, K, P, S, io.theta_out);
    } else if (c->dTrace) {
        rc = trace_out(c, io.z_out, &clock);
        if (rc) return rc;
    } else {  // a run without a label trace (bmm_set_summary, keep_trace = 0): the small traces queued above
        HIP_TRY(hipStreamSynchronize(c->stream));
        clock.lap(3);
    }
    clock.lap(4);
    return dbg_labels_ok(c);
}

// planes packed on the host (AsyncPack: one pointer per plane, pinned pieces or ordinary memory) into the chain
int chain_set_planes_host(bmm_chain* c, uint32_t* const* plane) {
    const int W = (c->p.P + 31) / 32;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dXb) { int rcp = planes_alloc(c, (size_t)W * c->p.N); if (rcp) return rcp; }
    for (int w = 0; w < W; ++w)
        HIP_TRY(hipMemcpyAsync(c->dXb + (size_t)w * c->p.N, plane[w], (size_t)c->p.N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->dX = nullptr;
    c->have_data = true;
    return BMM_OK;
}

#ifdef BMM_DEBUG_HOOKS
// Test variant only: the host-side ends of a run on their own, no device involved (tests/test_capi_cpu.py
// holds them to numpy): X packed into planes [w][N] by the crew, and a block of one-byte / int32 labels
// copied into an int32 trace.
extern "C" int bmm_dbg_host_pack(const int32_t* X, int64_t N, int P, uint32_t* out, uint32_t* seen_out) {
    return guarded([&]() -> int {
        const int W = (P + 31) / 32;
        std::vector<uint32_t*> plane((size_t)W);
        for (int w = 0; w < W; ++w) plane[(size_t)w] = out + (size_t)w * (size_t)N;
        std::atomic<uint32_t> seen{0};
        HostCrew crew;
        crew.run(N, 1024, 64, [&](int64_t lo, int64_t hi) {
            seen.fetch_or(pack_rows_host(X, N, P, lo, hi, plane.data(), 0), std::memory_order_relaxed);
        });
        *seen_out = seen.load();
        return BMM_OK;
    });
}
extern "C" int bmm_dbg_host_labels(const void* src, int narrow, int32_t* dst, int64_t n, int jobs) {
    return guarded([&]() -> int {
        HostCrew crew;
        for (int j = 0; j < jobs; ++j) {  // the same crew, job after job, as trace_out uses it
            if (narrow) crew.run(n, 256, 64, [=](int64_t lo, int64_t hi) { widen_labels(static_cast<const uint8_t*>(src) + lo, dst + lo, hi - lo); });
            else crew.run(n, 256, 64, [=](int64_t lo, int64_t hi) { copy_labels(static_cast<const int32_t*>(src) + lo, dst + lo, hi - lo); });
        }
        return BMM_OK;
    });
}
// Test variant only: which k_resample instantiation the chain's launches run -- accumulators, workgroup size, lanes
// per observation, own-cluster tier (0 none, 1 LDS, 2 global memory), X layout (1 bit planes), group width, whether
// it builds its own tables, the weight-emitting twin's workgroup size (0 where there is none and the hand-off runs
// the generic kernel), whether the chain is on the generic kernel altogether, and the emitting twin's grid limit
// (0 until a hand-off has set the twin up) (tests/test_gpu_chunks.py)
static void kernel_key(const KernelForm& f, const KernelForm& twin, bool generic, int grid_max_emit, int* key) {
    const int k[10] = {f.kt, f.nt, f.lanes, f.minus, f.bits ? 1 : 0, f.gw, f.self ? 1 : 0, generic ? 0 : twin.nt, generic ? 1 : 0, grid_max_emit};
    std::memcpy(key, k, sizeof k);
}
// ... whether that kernel is the packed one (k_resample_pk; the key's ten slots describe the form it stands in for),
// and what its launches have counted so far: observations drawn, observations deferred to the binary64 definition
extern "C" int bmm_dbg_kernel_packed(const bmm_chain* c) { return c && !c->generic && c->form.pk ? 1 : 0; }
// ... and whether it runs the second body (tests/test_gpu_pk_pipe.py, tests/test_gpu_pk_plain.py)
extern "C" int bmm_dbg_kernel_pk_pipelined(const bmm_chain* c) { return c && !c->generic && c->form.pk && c->form.pipe ? 1 : 0; }
extern "C" int bmm_dbg_pk_counts(bmm_chain* c, unsigned long long* draws, unsigned long long* deferred) {
    if (!c || !draws || !deferred) return set_err(BMM_E_ARG, "null argument");
    return guarded([&]() -> int {
        unsigned long long v[2] = {0, 0};
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(v, c->dPkStat, sizeof v, hipMemcpyDeviceToHost));
        *draws = v[0]; *deferred = v[1];
        return BMM_OK;
    });
}
// ... and how many of the deferred the packed tier left uncertain by itself without BMM_DEBUG_PK_DEFER_EVERY selecting
// them (tests/test_gpu_pk_inline.py: deferred == selected + this)
extern "C" int bmm_dbg_pk_unselected(bmm_chain* c, unsigned long long* n) {
    if (!c || !n) return set_err(BMM_E_ARG, "null argument");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(n, c->dPkStat + 2, sizeof *n, hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}
// ... and how the deferred were settled: runs of the middle tier (pk_mid_count), of them certain, runs of the
// definition (pk_exact_count) (tests/test_gpu_pk_mid.py: tried == deferred, definition == tried - settled)
extern "C" int bmm_dbg_pk_tier_counts(bmm_chain* c, unsigned long long* mid_tried, unsigned long long* mid_settled,
                                      unsigned long long* exact_runs) {
    if (!c || !mid_tried || !mid_settled || !exact_runs) return set_err(BMM_E_ARG, "null argument");
    return guarded([&]() -> int {
        unsigned long long v[3] = {0, 0, 0};
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(v, c->dPkStat + 3, sizeof v, hipMemcpyDeviceToHost));
        *mid_tried = v[0]; *mid_settled = v[1]; *exact_runs = v[2];
        return BMM_OK;
    });
}
extern "C" int bmm_dbg_kernel_key(const bmm_chain* c, int* key) {
    if (!c || !key) return set_err(BMM_E_ARG, "null argument");
    kernel_key(c->form, c->form_emit, c->generic, c->fn_emit ? c->grid_max_emit : 0, key);
    return BMM_OK;
}
// ... and the same key for a chain that is not created: what chain_shape and plan_kernel make of the arguments, of
// num_cus compute units and of the switches a chain would read, every form the plan offers taken.  No device is
// touched (tests/test_capi_cpu.py holds the measured rules this way; tests/test_gpu_chunks.py holds plan and chain
// to each other).
extern "C" int bmm_dbg_kernel_plan(int sampler, int64_t N, int P, int K, int64_t batch, int num_cus, int shares_device,
                                   int int32_layout, int* key) {
    if (!key || sampler < 0 || sampler > 3 || N < 1 || P < 1 || K < 1 || num_cus < 1) return set_err(BMM_E_ARG, "bad argument");
    const DebugSwitches dbg;
    const ChainShape s = chain_shape(sampler, N, P, K, batch, dbg);
    const bool bits = !int32_layout && !dbg.int32_layout;
    const int minus = explicit_params(sampler) ? 0 : (s.minus_in_lds ? 1 : 2);
    if (s.generic) {
        kernel_key(KernelForm{s.p.KT, 256, minus, bits, 1, false, s.p.W, false}, KernelForm{}, true, 0, key);
        return BMM_OK;
    }
    const KernelPlan plan = plan_kernel(s.p, bits, minus, s.batch, dbg.cus >= 1 ? dbg.cus : num_cus, shares_device != 0,
                                        s.lds_bytes_base, dbg);
    const KernelForm& f = plan.form[plan.n - 1];
    kernel_key(f, bits ? emit_twin(f) : KernelForm{}, false, 0, key);
    return BMM_OK;
}
#endif

// relabelling on the device in a run (*_run_relabel): what is refused before any device is touched
int st_run_check(const RunOptions& opts, int burnin, int K) {
    const bmm_relabel_out* const rel = opts.rel;
    if (!rel) return BMM_OK;
    if (!rel->permutations || !rel->z_original || !rel->theta_original) return set_err(BMM_E_ARG, "null buffer");
    if (burnin < 2 || rel->burnrelabel < 1)
        return set_err(BMM_E_ARG, "relabel on the device needs the batch step, which the reference runs only with "
                       "burnin >= 2 and burnrelabel >= 1 (burnin = %d, burnrelabel = %d)", burnin, rel->burnrelabel);
    return st_check_k(K);
}

int check_run_args(const int32_t* X, int nsamples, int burnin, const RunIO& io, int sampler, bool keep_trace = true) {
    if (!X || (!io.z_out && keep_trace) || !io.theta_out || !io.alpha_out) return set_err(BMM_E_ARG, "null buffer");
    if (sampler == BMM_SAMPLER_COLLAPSED && !io.z0) return set_err(BMM_E_ARG, "initialK is null");
    if (explicit_params(sampler) && (!io.pi0 || !io.theta0 || !io.pi_out)) return set_err(BMM_E_ARG, "null buffer");
    if (nsamples < 1) return set_err(BMM_E_ARG, "nsamples must be >= 1");
    if (burnin < 0 || burnin >= nsamples) return set_err(BMM_E_ARG, "burnin must be in [0, nsamples)");
    return BMM_OK;
}

// ---- a run's replica ladder (bmm_set_temper) ----
// refused before any device is touched
int temper_run_check(const RunOptions& opts, int sampler) {
    if (!opts.temper.on) return BMM_OK;
    const bmm_temper_out& o = opts.temper.o;
    if (sampler != BMM_SAMPLER_COLLAPSED && sampler != BMM_SAMPLER_DP)
        return set_err(BMM_E_UNSUPPORTED, "parallel tempering is offered for the collapsed and DP samplers only");
    if (opts.alloc.on) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered for the allocation sampler");
    if (opts.rel || opts.hooks) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered together with a relabelling run or a probability hand-off");
    if (opts.sm.moves > 0) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered together with split-merge moves: their ratio would need the tempered likelihood");
    if (opts.fs.on) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered together with feature selection");
    if (o.R < 1 || o.R > kTemperMaxR) return set_err(BMM_E_ARG, "temper: a ladder has 1 to %d rungs", kTemperMaxR);
    if (!o.inv_temp) return set_err(BMM_E_ARG, "temper: inv_temp is null");
    if (o.swap_every < 1) return set_err(BMM_E_ARG, "temper: swap_every must be >= 1");
    if (o.inv_temp[0] != 1.0) return set_err(BMM_E_ARG, "temper: inv_temp[0] must be 1");
    for (int r = 1; r < o.R; ++r)
        if (!(o.inv_temp[r] > 0.0 && o.inv_temp[r] < o.inv_temp[r - 1]))
            return set_err(BMM_E_ARG, "temper: inv_temp[%d] must lie in (0, inv_temp[%d])", r, r - 1);
    return BMM_OK;
}
// The helpers and the ladder of a run, released in this order ahead of the run's own chain.
struct TemperRun {
    bmm_chain* c0 = nullptr;
    bmm_ladder* l = nullptr;
    std::vector<bmm_chain*> helpers;
    DevBuf lik, walker;
    ~TemperRun() {
        if (c0) c0->ladder = nullptr;
        bmm_ladder_destroy(l);
        for (bmm_chain* h : helpers) bmm_chain_destroy(h);
    }
};
// chain 0 has its data and its starting state and has not started
int temper_run_attach(bmm_chain* c, const RunOptions& opts, double alpha, int64_t batch, uint64_t seed, TemperRun& tr) {
    if (!opts.temper.on) return BMM_OK;
    const bmm_temper_out& o = opts.temper.o;
    const ChainParams& p = c->p;
    const int R = o.R, S = c->S;
    if (R > 1 && c->sm_moves > 0) return set_err(BMM_E_UNSUPPORTED, "parallel tempering is not offered together with split-merge moves");
    std::vector<bmm_chain*> rungs{c};
    for (int r = 1; r < R; ++r) {
        bmm_chain* h = nullptr;
        int rc = bmm_chain_create(&h, p.mode, p.N, p.P, p.K, alpha, p.beta, p.gamma, p.a, p.b, batch, seed + (uint64_t)r, c->slot);
        if (rc) return rc;
        tr.helpers.push_back(h);
        rungs.push_back(h);
        if (c->bits) {
            rc = bmm_chain_share_data(h, c);
        } else {  // the int32 layout: the run's device matrix, borrowed
            rc = bmm_chain_set_x_layout(h, BMM_X_INT32);
            h->dX = c->dX;
            h->have_data = true;
        }
        if (rc) return rc;
        if (p.mode == MODE_COLLAPSED) {  // the run's initial allocation, as chain 0 holds it (0-based)
            HIP_TRY(hipMemcpyAsync(h->dZ[0], c->dZ[0], (size_t)p.N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            h->have_init = true;
        }
        rc = bmm_chain_set_temper(h, 1, o.inv_temp[r]);
        if (rc) return rc;
    }
    int rc = bmm_ladder_create(&tr.l, rungs.data(), R, seed);
    if (rc) return rc;
    tr.l->swap_every = o.swap_every;
    tr.l->base = c->burnin;
    if (o.loglik) {
        std::vector<double> nan((size_t)S * R, std::nan(""));
        HIP_TRY(tr.lik.alloc(nan.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(tr.lik.p, nan.data(), nan.size() * sizeof(double), hipMemcpyHostToDevice));
        tr.l->lik_rows = tr.lik.as<double>();
    }
    if (o.walker_cold) {
        HIP_TRY(tr.walker.alloc((size_t)S * sizeof(int32_t)));
        HIP_TRY(hipMemset(tr.walker.p, 0, (size_t)S * sizeof(int32_t)));
        tr.l->walker_rows = tr.walker.as<int32_t>();
    }
    tr.c0 = c;
    c->ladder = tr.l;
    return BMM_OK;
}
int temper_run_collect(bmm_chain* c, const RunOptions& opts, TemperRun& tr, int rc) {
    if (!opts.temper.on || !tr.l) return rc;
    const bmm_temper_out& o = opts.temper.o;
    const int R = o.R, S = c->S;
    const int rs = ladder_sync(tr.l);
    if (rc || rs) return rc ? rc : rs;
    rc = bmm_ladder_stats(tr.l, o.proposed, o.accepted, nullptr);
    if (rc) return rc;
    if (o.walker_cold) HIP_TRY(hipMemcpy(o.walker_cold, tr.walker.p, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (o.loglik) {  // [S][R] on the device, S x R column-major for the caller
        std::vector<double> rows((size_t)S * R);
        HIP_TRY(hipMemcpy(rows.data(), tr.lik.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int s = 0; s < S; ++s)
            for (int r = 0; r < R; ++r) o.loglik[(size_t)r * S + s] = rows[(size_t)s * R + r];
    }
    return BMM_OK;
}

int run_chain(int sampler, const int32_t* X, int64_t N, int P, int nsamples, int K, double alpha, double beta,
              double gamma, double a, double b, int burnin, int64_t batch, uint64_t seed, int device,
              const RunIO& io, const RunOptions& opts) {
    return guarded([&]() -> int {
        // refused before any device is touched
        int rc = check_run_args(X, nsamples, burnin, io, sampler, opts.keep_trace());
        if (rc == BMM_OK) rc = cat_run_check(opts, sampler, P);  // (ahead of the options' own checks: it names the pairing)
        if (rc == BMM_OK) rc = pt_run_check(opts, nsamples - burnin, N, K);
        if (rc) return rc;
        g_init_info = bmm_init_info{};
        rc = init_run_check(opts, sampler);
        if (rc == BMM_OK) rc = pred_run_check(opts, P);
        if (rc == BMM_OK) rc = fs_run_check(opts, sampler, beta, gamma);
        if (rc == BMM_OK) rc = alloc_run_check(opts);
        if (rc == BMM_OK) rc = temper_run_check(opts, sampler);
        if (rc == BMM_OK) rc = st_run_check(opts, burnin, K);
        if (rc == BMM_OK) rc = ecr_run_check(opts, nsamples - burnin, N, K);
        if (rc == BMM_OK) rc = pc_run_check(opts, P, K);
        if (rc == BMM_OK) rc = na_run_check(opts, N, P);
        if (rc == BMM_OK) rc = cs_run_check(opts, N, K);
        if (rc == BMM_OK) rc = sum_run_check(opts, N, K);
        if (rc) return rc;
        for (double& v : g_phase_ms) v = 0.0;
        PhaseClock clock;
        // The host's cores start validating and packing X at once (bit planes, the default layout) while this
        // thread creates the chain, allocates the run's buffers and uploads the starting state: the two take
        // about as long at the north-star shape, and only the planes -- 4 * ceil(P/32) bytes per observation
        // instead of 4 * P -- then cross PCIe.
        HostCrew crew;  // the host threads of this call: they pack X now and widen the label trace at the end
        AsyncPack pack;
        const bool host_pack = dbg_env("BMM_X_LAYOUT_INT32") == nullptr;
        if (host_pack) pack.start(&crew, X, N, P);
        bmm_chain* c = nullptr;
        rc = bmm_chain_create(&c, sampler, N, P, K, alpha, beta, gamma, a, b, batch, seed, device);
        if (rc) return rc;
        c->crew = &crew;
        {
            struct Guard { bmm_chain* c; ~Guard() { bmm_chain_destroy(c); } } guard{c};
            TemperRun temper;  // (released ahead of the chain)
            rc = run_prepare(c, nsamples, burnin, opts.keep_trace());
            if (rc == BMM_OK) rc = run_start_state(c, io, opts.init.kind != 0);
            if (rc) return rc;
            clock.lap(1);
            pack.join();
            if (host_pack && c->bits) {
                if (pack.seen.load() & ~1u) return set_err(BMM_E_ARG, "data must be binary: X holds a value other than 0 and 1");
                rc = chain_set_planes_host(c, pack.plane.data());
                pack.release();
            } else {  // the int32 layout (test variant): the resident API's way
                pack.release();
                rc = bmm_chain_set_data_host(c, X);
            }
            if (rc == BMM_OK) rc = init_run_attach(c, opts);
            if (rc == BMM_OK) rc = na_run_attach(c, opts);  // the cells are filled before anything counts them
            if (rc == BMM_OK) rc = cs_run_attach(c, opts);  // the starting labels are projected when the chain starts
            if (rc == BMM_OK) rc = cat_run_attach(c, opts);  // the levels meet the data: k_cat_check
            if (rc) return rc;
            clock.lap(0);
            // what the options record per kept sweep: each ends, and waits for the stream before its rows go, on every way out
            Recording pred_rec, loo_rec, fs_rec, k_rec, lp_rec, pc_rec, sum_rec;
            rc = pred_run_attach(c, opts, pred_rec);
            if (rc == BMM_OK) rc = loo_run_attach(c, opts, loo_rec);
            if (rc == BMM_OK) rc = sm_run_attach(c, opts);
            if (rc == BMM_OK) rc = fs_run_attach(c, opts, fs_rec);
            if (rc == BMM_OK) rc = alloc_run_attach(c, opts, k_rec);
            if (rc == BMM_OK) rc = lp_run_attach(c, opts, lp_rec);
            if (rc == BMM_OK) rc = pc_run_attach(c, opts, pc_rec);
            if (rc == BMM_OK) rc = sum_run_attach(c, opts, sum_rec);
            if (rc == BMM_OK) rc = temper_run_attach(c, opts, alpha, batch, seed, temper);
            if (rc) return rc;
            rc = run_body(c, nsamples, io, opts);
            rc = temper_run_collect(c, opts, temper, rc);
            rc = na_run_collect(c, opts, rc);
            rc = cs_run_collect(c, opts, rc);
            rc = sum_run_collect(c, opts, sum_rec, rc);
            rc = pc_run_collect(c, opts, pc_rec, rc);
            rc = lp_run_collect(c, opts, lp_rec, rc);
            rc = sm_run_collect(c, opts, rc);
            rc = alloc_run_collect(c, opts, k_rec, rc);
            rc = fs_run_collect(c, opts, fs_rec, rc);
            rc = loo_run_collect(c, opts, loo_rec, rc);
            rc = pred_run_collect(c, opts, pred_rec, rc);
            clock.t = std::chrono::steady_clock::now();
        }
        clock.lap(5);  // releasing the chain
        return rc;
    });
}

// ---- RCCL, opened on demand: only a run that spans devices needs it, and a process that has
// torch loaded must end up with one copy of the library (dlopen by soname finds a loaded one)
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
int rccl_open(Rccl& r) {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (r.lib) break;
    }
    if (!r.lib) return set_err(BMM_E_RCCL, "RCCL is needed to broadcast the data across devices and could not be opened: %s", dlerror());
    r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.lib, "ncclCommInitAll"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
    r.Broadcast = reinterpret_cast<decltype(r.Broadcast)>(dlsym(r.lib, "ncclBroadcast"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.lib, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.lib, "ncclGroupEnd"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    if (!r.CommInitAll || !r.CommDestroy || !r.Broadcast || !r.GroupStart || !r.GroupEnd || !r.GetErrorString)
        return set_err(BMM_E_RCCL, "the RCCL library lacks an expected symbol");
    return BMM_OK;
}

// One broadcast of `count` 32-bit words from bufs[0] (on devs[0]) into bufs[r] on devs[r], over a
// communicator built in this process (ncclCommInitAll): the only collective of the chain path.
int rccl_broadcast_words(const std::vector<int>& devs, const std::vector<void*>& bufs, size_t count) {
    const int n = (int)devs.size();
    if (n < 2) return BMM_OK;
    if (fake_devices()) {  // test variant: the "devices" are one device; the broadcast is a copy per receiver
        for (int q = 1; q < n; ++q) HIP_TRY(hipMemcpy(bufs[(size_t)q], bufs[0], count * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_TRY(hipDeviceSynchronize());
        return BMM_OK;
    }
    Rccl r;
    int rc = rccl_open(r);
    if (rc) return rc;
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    ncclResult_t e = r.CommInitAll(comms.data(), n, devs.data());
    if (e != ncclSuccess) return set_err(BMM_E_RCCL, "ncclCommInitAll failed: %s", r.GetErrorString(e));
    std::vector<hipStream_t> st((size_t)n, nullptr);
    hipError_t he = hipSuccess;
    for (int q = 0; q < n && he == hipSuccess; ++q) {
        he = hipSetDevice(devs[(size_t)q]);
        if (he == hipSuccess) he = hipStreamCreateWithFlags(&st[(size_t)q], hipStreamNonBlocking);
    }
    if (he == hipSuccess) {
        e = r.GroupStart();
        // every rank passes its own buffer, in place (the root's holds the data; a send buffer is read
        // on the root only, and a pointer of another device must not be handed to a rank's call)
        for (int q = 0; q < n && e == ncclSuccess; ++q)
            e = r.Broadcast(bufs[(size_t)q], bufs[(size_t)q], count, ncclUint32, 0, comms[(size_t)q], st[(size_t)q]);
        const ncclResult_t e2 = r.GroupEnd();
        if (e == ncclSuccess) e = e2;
        for (int q = 0; q < n && he == hipSuccess; ++q) {
            he = hipSetDevice(devs[(size_t)q]);
            if (he == hipSuccess) he = hipStreamSynchronize(st[(size_t)q]);
        }
    }
    for (int q = 0; q < n; ++q) {
        if (st[(size_t)q]) { (void)hipSetDevice(devs[(size_t)q]); (void)hipStreamDestroy(st[(size_t)q]); }
        if (comms[(size_t)q]) (void)r.CommDestroy(comms[(size_t)q]);
    }
    if (he != hipSuccess) return set_err(BMM_E_HIP, "broadcasting the data failed: %s", hipGetErrorString(he));
    if (e != ncclSuccess) return set_err(BMM_E_RCCL, "ncclBroadcast failed: %s", r.GetErrorString(e));
    return BMM_OK;
}

}  // namespace

extern "C" {

// ---- one chain, one call: the four samplers ------------------------------------------------
int bmm_collapsed_run(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int K, double alpha,
                      double beta, double gamma, double a, double b, int burnin, int64_t batch, uint64_t seed,
                      int device, int32_t* z_out, double* theta_out, double* alpha_out) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_COLLAPSED, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(initialK, z_out, theta_out, alpha_out), opts);
}
int bmm_dp_run(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta, double gamma, double a,
               double b, int burnin, int maxK, int64_t batch, uint64_t seed, int device, int32_t* z_out,
               double* theta_out, double* alpha_out) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_DP, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(nullptr, z_out, theta_out, alpha_out), opts);
}
int bmm_sb_run(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta, int nsamples,
               int maxK, double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed,
               int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_SB, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), opts);
}
int bmm_full_run(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta, int nsamples,
                 int K, double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed,
                 int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_FULL, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), opts);
}

// ---- ... with the hooks that hand every sweep's allocation probabilities to the host ----------
int bmm_collapsed_run_probs(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int K,
                            double alpha, double beta, double gamma, double a, double b, int burnin, int64_t batch,
                            uint64_t seed, int device, int32_t* z_out, double* theta_out, double* alpha_out,
                            const bmm_relabel_hooks* hooks) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_COLLAPSED, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(initialK, z_out, theta_out, alpha_out), with_hooks(opts, hooks));
}
int bmm_dp_run_probs(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta, double gamma,
                     double a, double b, int burnin, int maxK, int64_t batch, uint64_t seed, int device, int32_t* z_out,
                     double* theta_out, double* alpha_out, const bmm_relabel_hooks* hooks) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_DP, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(nullptr, z_out, theta_out, alpha_out), with_hooks(opts, hooks));
}
int bmm_sb_run_probs(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                     int nsamples, int maxK, double alpha, double beta, double gamma, double a, double b, int burnin,
                     uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                     const bmm_relabel_hooks* hooks) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_SB, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), with_hooks(opts, hooks));
}
int bmm_full_run_probs(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                       int nsamples, int K, double alpha, double beta, double gamma, double a, double b, int burnin,
                       uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                       const bmm_relabel_hooks* hooks) {
    const RunOptions opts = take_run_options();
    return run_chain(BMM_SAMPLER_FULL, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), with_hooks(opts, hooks));
}

// ---- ... with the posterior predictive of new rows ---------------------
int bmm_collapsed_run_predict(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int K,
                              double alpha, double beta, double gamma, double a, double b, int burnin, int64_t batch,
                              uint64_t seed, int device, int32_t* z_out, double* theta_out, double* alpha_out,
                              const int32_t* Xnew, int64_t M, const bmm_predict_out* pred) {
    const RunOptions opts = take_run_options();
    if (!pred) return set_err(BMM_E_ARG, "null predictive outputs");
    return run_chain(BMM_SAMPLER_COLLAPSED, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(initialK, z_out, theta_out, alpha_out), with_predict(opts, Xnew, M, pred));
}
int bmm_dp_run_predict(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta, double gamma,
                       double a, double b, int burnin, int maxK, int64_t batch, uint64_t seed, int device,
                       int32_t* z_out, double* theta_out, double* alpha_out, const int32_t* Xnew, int64_t M,
                       const bmm_predict_out* pred) {
    const RunOptions opts = take_run_options();
    if (!pred) return set_err(BMM_E_ARG, "null predictive outputs");
    return run_chain(BMM_SAMPLER_DP, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(nullptr, z_out, theta_out, alpha_out), with_predict(opts, Xnew, M, pred));
}
int bmm_sb_run_predict(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                       int nsamples, int maxK, double alpha, double beta, double gamma, double a, double b, int burnin,
                       uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                       const int32_t* Xnew, int64_t M, const bmm_predict_out* pred) {
    const RunOptions opts = take_run_options();
    if (!pred) return set_err(BMM_E_ARG, "null predictive outputs");
    return run_chain(BMM_SAMPLER_SB, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out),
                     with_predict(opts, Xnew, M, pred));
}
int bmm_full_run_predict(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                         int nsamples, int K, double alpha, double beta, double gamma, double a, double b, int burnin,
                         uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out,
                         double* alpha_out, const int32_t* Xnew, int64_t M, const bmm_predict_out* pred) {
    const RunOptions opts = take_run_options();
    if (!pred) return set_err(BMM_E_ARG, "null predictive outputs");
    return run_chain(BMM_SAMPLER_FULL, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out),
                     with_predict(opts, Xnew, M, pred));
}

// ---- ... with relabel = TRUE, Stephens' relabelling on the device ---------------------------
int bmm_collapsed_run_relabel(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int K,
                              double alpha, double beta, double gamma, double a, double b, int burnin, int64_t batch,
                              uint64_t seed, int device, int32_t* z_out, double* theta_out, double* alpha_out,
                              const bmm_relabel_out* rel) {
    const RunOptions opts = take_run_options();
    if (!rel) return set_err(BMM_E_ARG, "null relabel outputs");
    return run_chain(BMM_SAMPLER_COLLAPSED, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(initialK, z_out, theta_out, alpha_out), with_relabel(opts, rel));
}
int bmm_dp_run_relabel(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta, double gamma,
                       double a, double b, int burnin, int maxK, int64_t batch, uint64_t seed, int device,
                       int32_t* z_out, double* theta_out, double* alpha_out, const bmm_relabel_out* rel) {
    const RunOptions opts = take_run_options();
    if (!rel) return set_err(BMM_E_ARG, "null relabel outputs");
    return run_chain(BMM_SAMPLER_DP, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, batch, seed, device,
                     counting_io(nullptr, z_out, theta_out, alpha_out), with_relabel(opts, rel));
}
int bmm_sb_run_relabel(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                       int nsamples, int maxK, double alpha, double beta, double gamma, double a, double b, int burnin,
                       uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                       const bmm_relabel_out* rel) {
    const RunOptions opts = take_run_options();
    if (!rel) return set_err(BMM_E_ARG, "null relabel outputs");
    return run_chain(BMM_SAMPLER_SB, X, N, P, nsamples, maxK, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), with_relabel(opts, rel));
}
int bmm_full_run_relabel(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                         int nsamples, int K, double alpha, double beta, double gamma, double a, double b, int burnin,
                         uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out,
                         double* alpha_out, const bmm_relabel_out* rel) {
    const RunOptions opts = take_run_options();
    if (!rel) return set_err(BMM_E_ARG, "null relabel outputs");
    return run_chain(BMM_SAMPLER_FULL, X, N, P, nsamples, K, alpha, beta, gamma, a, b, burnin, 0, seed, device,
                     explicit_io(initialPi, initialTheta, pi_out, z_out, theta_out, alpha_out), with_relabel(opts, rel));
}

// The allocation sampler: the finite collapsed run with K in the state.
int bmm_alloc_run(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int maxK, double a,
                  double beta, double gamma, const double* log_prior_k, int K0, int moves_per_sweep, double eject_a,
                  int burnin, int64_t batch, uint64_t seed, int device, int32_t* z_out, double* theta_out,
                  int32_t* k_out, int64_t moves_out[4]) {
    RunOptions opts = take_run_options();
    if (opts.na.on) return set_err(BMM_E_UNSUPPORTED, "missing cells (bmm_set_missing) are not offered by the allocation sampler's run");
    if (opts.cs.on) return set_err(BMM_E_UNSUPPORTED, "constrained rows (bmm_set_constraints) are not offered by the allocation sampler's run");
    if (!log_prior_k || !k_out) return set_err(BMM_E_ARG, "null buffer");
    if (!(a > 0.0)) return set_err(BMM_E_ARG, "a must be > 0");
    if (maxK > kMaxCats) return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is offered up to maxK = %d", kMaxCats);
    if (P > kEaMaxP) return set_err(BMM_E_UNSUPPORTED, "the allocation sampler is offered up to %d features", kEaMaxP);
    if (maxK < 2) return set_err(BMM_E_ARG, "maxK must be >= 2");
    if (K0 < 1 || K0 > maxK) return set_err(BMM_E_ARG, "the initial K must lie in 1..maxK");
    if (nsamples < 1 || burnin < 0 || burnin >= nsamples) return set_err(BMM_E_ARG, "burnin must be in [0, nsamples)");
    std::vector<double> alpha_out((size_t)(nsamples - burnin));
    opts.alloc.on = true; opts.alloc.log_prior_k = log_prior_k; opts.alloc.K0 = K0; opts.alloc.moves = moves_per_sweep;
    opts.alloc.eject_a = eject_a; opts.alloc.k_out = k_out; opts.alloc.moves_out = moves_out;
    return run_chain(BMM_SAMPLER_COLLAPSED, X, N, P, nsamples, maxK, a, beta, gamma, 1.0, 1.0, burnin, batch, seed, device,
                     counting_io(initialK, z_out, theta_out, alpha_out.data()), opts);
}

int bmm_device_stephens_batch(int device, const double* p, int64_t N, int K, int M, double* Q_out, int32_t* perm_out) {
    return guarded([&]() -> int {
        if (!p || !Q_out || !perm_out) return set_err(BMM_E_ARG, "null argument");
        if (N < 1 || M < 1) return set_err(BMM_E_ARG, "N and M must be >= 1");
        int rc = st_check_k(K);
        if (rc) return rc;
        const size_t n = (size_t)N * K * M;
        for (size_t i = 0; i < n; ++i)
            if (!(p[i] >= 0.0) || std::isinf(p[i])) return set_err(BMM_E_ARG, "p must hold finite values >= 0 (element %zu)", i);
        HIP_TRY(hipSetDevice(device));
        StWork w;
        w.shape(N, K, M);
        DevBuf dp;
        HIP_TRY(dp.alloc(n * sizeof(double)));
        rc = w.alloc();
        if (rc) return rc;
        HIP_TRY(hipMemcpy(dp.p, p, n * sizeof(double), hipMemcpyHostToDevice));
        rc = st_batch(nullptr, w, dp.as<double>());
        if (rc) return rc;
        HIP_TRY(hipMemcpy(Q_out, w.Q.p, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(perm_out, w.permb.p, (size_t)M * K * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}

int bmm_device_stephens_online(int device, const double* Q, const double* p, int64_t N, int K, int j, int32_t* perm_out,
                               double* Q_out, double* cost_out) {
    return guarded([&]() -> int {
        if (!Q || !p || !perm_out || !Q_out) return set_err(BMM_E_ARG, "null argument");
        if (N < 1) return set_err(BMM_E_ARG, "N must be >= 1");
        int rc = st_check_k(K);
        if (rc) return rc;
        const size_t nk = (size_t)N * K;
        for (size_t i = 0; i < nk; ++i) {
            if (!(p[i] >= 0.0) || std::isinf(p[i])) return set_err(BMM_E_ARG, "p must hold finite values >= 0 (element %zu)", i);
            if (!(Q[i] > 0.0) || std::isinf(Q[i])) return set_err(BMM_E_ARG, "Q must hold finite values > 0 (element %zu)", i);
        }
        HIP_TRY(hipSetDevice(device));
        StWork w;
        w.shape(N, K, 0);
        DevBuf dp, dperm;
        HIP_TRY(dp.alloc(nk * sizeof(double)));
        HIP_TRY(dperm.alloc((size_t)K * sizeof(int32_t)));
        rc = w.alloc();
        if (rc) return rc;
        HIP_TRY(hipMemcpy(dp.p, p, nk * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(w.Q.p, Q, nk * sizeof(double), hipMemcpyHostToDevice));
        rc = st_online(nullptr, w, dp.as<double>(), j, dperm.as<int32_t>(), 1);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(perm_out, dperm.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(Q_out, w.Q.p, nk * sizeof(double), hipMemcpyDeviceToHost));
        if (cost_out) HIP_TRY(hipMemcpy(cost_out, w.cost.p, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost));
        return BMM_OK;
    });
}

// Which form of every k_st_* kernel a shape runs, from the functions the launches above call (no device is
// touched; tests/test_stephens_cpu.py, and tests/test_gpu_stephens_forms.py proves its reach with it)
int bmm_device_stephens_plan(int64_t N, int K, int M, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    if (N < 1 || M < 0) return set_err(BMM_E_ARG, "N must be >= 1 and M >= 0");
    int rc = st_check_k(K);
    if (rc) return rc;
    StWork w;
    w.shape(N, K, M);
    for (int i = 0; i < 12; ++i) out[i] = 0;
    out[0] = w.G1;
    out[1] = w.GM;
    out[2] = st_rows(N, w.G1);
    out[3] = M > 0 ? st_rows(N, w.GM) : 0;
    out[4] = st_cost_b(K);
    out[5] = st_tile_rows(K);
    out[6] = st_cost_nb(K);
    out[7] = st_cost_ng(K);
    out[8] = st_assign_in_lds(K) ? 1 : 0;
    out[9] = st_assign_cols(K);
    return BMM_OK;
}

// ---- clustering point estimate and posterior similarity: the stand-alone entry points ----
int bmm_set_split_merge(int moves_per_sweep, int scans) {
    if (moves_per_sweep < 0 || scans < 0 || scans > 4096) return set_err(BMM_E_ARG, "moves_per_sweep and scans must be >= 0 (scans at most 4096)");
    g_armed.sm.moves = moves_per_sweep;
    g_armed.sm.scans = scans;
    return BMM_OK;
}
int bmm_set_init(int kind, int iters) {
    if (kind != 0 && kind != BMM_INIT_KMODES) return set_err(BMM_E_ARG, "unknown kind of initialisation %d", kind);
    if (iters < 0) return set_err(BMM_E_ARG, "iters must be >= 0");
    g_armed.init.kind = kind;
    g_armed.init.iters = iters;
    return BMM_OK;
}
int bmm_last_init_info(bmm_init_info* info) {
    if (!info) return set_err(BMM_E_ARG, "null argument");
    *info = g_init_info;
    return BMM_OK;
}
int bmm_set_alloc_split_merge(int moves_per_sweep, int scans) {
    if (moves_per_sweep < 0 || scans < 0 || scans > 4096) return set_err(BMM_E_ARG, "moves_per_sweep and scans must be >= 0 (scans at most 4096)");
    g_armed.as.moves = moves_per_sweep;
    g_armed.as.scans = scans;
    return BMM_OK;
}
int bmm_last_alloc_split_merge_stats(int64_t out[5]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    for (int q = 0; q < 5; ++q) out[q] = g_as_stats[q];
    return BMM_OK;
}
int bmm_last_split_merge_stats(int64_t out[5]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    for (int q = 0; q < 5; ++q) out[q] = g_sm_stats[q];
    return BMM_OK;
}

int bmm_set_feature_select(const bmm_feature_out* out) {
    g_armed.fs.on = out != nullptr;
    if (out) g_armed.fs.o = *out;
    return BMM_OK;
}

int bmm_set_loo_summary(const bmm_loo_out* out) {
    g_armed.loo.on = out != nullptr;
    if (out) g_armed.loo.o = *out;
    return BMM_OK;
}

int bmm_set_logpost(const bmm_logpost_out* out) {
    g_armed.logpost.on = out != nullptr;
    if (out) g_armed.logpost.o = *out;
    return BMM_OK;
}

int bmm_set_temper(const bmm_temper_out* out) {
    g_armed.temper.on = out != nullptr;
    if (out) g_armed.temper.o = *out;
    return BMM_OK;
}

int bmm_set_missing(const int64_t* rows, const int32_t* cols, int64_t n_cells, const bmm_missing_out* out) {
    g_armed.na.on = out != nullptr;
    g_armed.na.rows = rows; g_armed.na.cols = cols; g_armed.na.n = n_cells;
    g_armed.na.o = out ? *out : bmm_missing_out{};
    return BMM_OK;
}
int bmm_set_newdata_missing(const int64_t* rows, const int32_t* cols, int64_t n_cells, double* cell_mean_out) {
    g_armed.pna.on = cell_mean_out != nullptr;
    g_armed.pna.rows = rows; g_armed.pna.cols = cols; g_armed.pna.n = n_cells; g_armed.pna.mean = cell_mean_out;
    return BMM_OK;
}
int bmm_set_constraints(int64_t n, const int64_t* rows, const uint64_t* masks) {
    g_armed.cs.on = n != 0;
    g_armed.cs.n = n; g_armed.cs.rows = rows; g_armed.cs.masks = masks;
    return BMM_OK;
}
int bmm_set_categorical(const int32_t* levels, int F) {
    g_armed.cat.on = false;
    g_armed.cat.levels.clear();
    if (F == 0) return BMM_OK;
    if (F < 0 || !levels) return set_err(BMM_E_ARG, "categorical: null levels or F < 0");
    g_armed.cat.levels.assign(levels, levels + F);
    g_armed.cat.on = true;
    return BMM_OK;
}
int bmm_last_constraint_stats(int64_t* proposed, int64_t* reverted) {
    if (!proposed || !reverted) return set_err(BMM_E_ARG, "null argument");
    *proposed = g_cs_stats[0]; *reverted = g_cs_stats[1];
    return BMM_OK;
}
int bmm_set_pair_check(const bmm_pair_check_out* out) {
    g_armed.pc.on = out != nullptr;
    g_armed.pc.feat.clear();
    if (out) {
        g_armed.pc.o = *out;
        // the features are copied; a list the run will refuse (pc_run_check) is kept only as far as it can be read
        if (out->feat && out->M > 0 && out->M <= kPcMaxM) g_armed.pc.feat.assign(out->feat, out->feat + out->M);
        g_armed.pc.o.feat = nullptr;
    }
    return BMM_OK;
}

int bmm_set_summary(const bmm_summary_opts* opts, const bmm_summary_out* out) {
    g_armed.summary.on = opts != nullptr;
    g_armed.summary.opts = opts ? *opts : bmm_summary_opts{};
    g_armed.summary.o = out ? *out : bmm_summary_out{};
    return BMM_OK;
}

int bmm_set_ecr_relabel(const bmm_ecr_out* out) {
    g_armed.ecr.on = out != nullptr;
    if (out) g_armed.ecr.o = *out;
    return BMM_OK;
}

int bmm_set_partition_summary(const bmm_partition_out* out) {
    g_armed.partition.on = out != nullptr;
    if (out) g_armed.partition.o = *out;
    return BMM_OK;
}

int bmm_set_partition_search(const bmm_partition_search_opts* opts, const bmm_partition_search_out* out) {
    g_armed.psearch.on = out != nullptr;
    g_armed.psearch.has_opts = out != nullptr && opts != nullptr;
    if (out) g_armed.psearch.o = *out;
    if (out && opts) g_armed.psearch.opts = *opts;
    return BMM_OK;
}

int bmm_set_credible_ball(double level, const bmm_credible_ball_out* out) {
    g_armed.cball.on = out != nullptr;
    g_armed.cball.level = level;
    if (out) g_armed.cball.o = *out;
    return BMM_OK;
}

int bmm_device_credible_ball(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion,
                             const int32_t* centre, int Ka, double level, const bmm_credible_ball_out* out) {
    return guarded([&]() -> int {
        if (!z || !centre || !out) return set_err(BMM_E_ARG, "credible ball: null argument");
        int rc = cb_check(S, N, Kc, criterion, Ka, level);
        if (rc == BMM_OK) rc = cb_check_members(*out, N);
        if (rc == BMM_OK) rc = pt_check_labels(z, S, N, 1, Kc, nullptr, "credible ball");
        if (rc) return rc;
        std::vector<int32_t> c0((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            if (centre[i] < 1 || centre[i] > Ka)
                return set_err(BMM_E_ARG, "credible ball: centre label %d at observation %lld (0-based) is outside 1 .. %d", centre[i], (long long)i, Ka);
            c0[(size_t)i] = centre[i] - 1;
        }
        HIP_TRY(hipSetDevice(device));
        PtWork w;
        w.shape(S, N, Kc, criterion, 1);
        rc = w.alloc_labels();
        if (rc == BMM_OK) rc = pt_upload(w, z);
        if (rc) return rc;
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, w.flag.p, sizeof flag, hipMemcpyDeviceToHost));
        if (flag) return set_err(BMM_E_STATE, "credible ball: a label outside 0 .. %d reached the device", Kc - 1);
        CbWork bw;
        rc = bw.alloc(S, N, Kc, Ka, criterion, *out);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(bw.c.p, c0.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
        rc = cb_distances(nullptr, bw, w.lab.as<uint8_t>());
        if (rc == BMM_OK && bw.M > 0) rc = cb_member(nullptr, bw, w.lab.as<uint8_t>(), *out);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipDeviceSynchronize());
        return cb_finish(bw, level, *out, 0, [&](int t, int32_t* dst) -> int {
            for (int64_t i = 0; i < N; ++i) dst[i] = z[(size_t)t + (size_t)i * S];
            return BMM_OK;
        });
    });
}

// Which form of every k_cb_* kernel a shape runs, from the function the launches call (no device is touched)
int bmm_credible_ball_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t M, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    const int rc = cb_check(S, N, Kc, criterion, Ka, 1.0);
    if (rc) return rc;
    if (M < 1) return set_err(BMM_E_ARG, "credible ball: M must be >= 1 (got %lld)", (long long)M);
    const CbPlan p = cb_plan(S, N, Kc, Ka, criterion, M, M != N);
    out[0] = p.el; out[1] = p.KaP; out[2] = p.nch; out[3] = p.rows; out[4] = p.D; out[5] = p.blocks; out[6] = p.bound;
    out[7] = (int64_t)p.lds_bytes; out[8] = p.wgs; out[9] = p.gathered; out[10] = p.vi; out[11] = (int64_t)p.table_bytes;
    return BMM_OK;
}

int bmm_device_partition_search(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion,
                                const int32_t* start, const bmm_partition_search_opts* opts,
                                const bmm_partition_search_out* out) {
    return guarded([&]() -> int {
        if (!z) return set_err(BMM_E_ARG, "null argument");
        PsOpts r;
        int rc = ps_check(S, N, Kc, criterion, opts, start == nullptr, r);
        if (rc == BMM_OK) rc = ps_check_out(out);
        if (rc == BMM_OK) rc = pt_check_labels(z, S, N, 1, Kc, nullptr, "partition search");
        if (rc) return rc;
        if (start)
            for (int64_t i = 0; i < N; ++i)
                if (start[i] < 1 || start[i] > r.Ka)
                    return set_err(BMM_E_ARG, "partition search: start label %d at observation %lld (0-based) is outside 1 .. %d", start[i], (long long)i, r.Ka);
        HIP_TRY(hipSetDevice(device));
        PtWork w;
        w.shape(S, N, Kc, criterion, 1);
        rc = w.alloc_labels();
        if (rc == BMM_OK) rc = pt_upload(w, z);
        if (rc) return rc;
        std::vector<int32_t> c0((size_t)N);
        if (start) {
            for (int64_t i = 0; i < N; ++i) c0[(size_t)i] = start[i] - 1;
        } else {  // the draws' minimiser at stride 1, as bmm_device_partition_distances finds it
            rc = w.alloc_pairs(false);
            if (rc == BMM_OK) rc = pt_compute(nullptr, w);
            if (rc) { (void)hipDeviceSynchronize(); return rc; }
            HIP_TRY(hipDeviceSynchronize());
            std::vector<double> loss((size_t)S);
            int best = -1;
            rc = pt_fetch(w, loss.data(), nullptr, &best, nullptr);
            if (rc) return rc;
            for (int64_t i = 0; i < N; ++i) c0[(size_t)i] = z[(size_t)best + (size_t)i * S] - 1;
        }
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, w.flag.p, sizeof flag, hipMemcpyDeviceToHost));
        if (flag) return set_err(BMM_E_STATE, "partition search: a label outside 0 .. %d reached the device", Kc - 1);
        PsWork sw;
        rc = sw.alloc(S, N, Kc, r.Ka, criterion, r.batch);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(sw.c.p, c0.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
        rc = ps_search(nullptr, sw, w.lab.as<uint8_t>(), r, *out);
        if (rc) (void)hipDeviceSynchronize();
        return rc;
    });
}

// Which form of every k_ps_* kernel a shape runs, from the function the launches call (no device is touched)
int bmm_partition_search_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t batch, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    const bmm_partition_search_opts o{batch, 1, 1, Ka};
    PsOpts r;
    const int rc = ps_check(S, N, Kc, criterion, &o, false, r);
    if (rc) return rc;
    const PsPlan p = ps_plan(S, N, Kc, r.Ka, criterion, r.batch);
    out[0] = p.el; out[1] = p.KaP; out[2] = p.nch; out[3] = p.rows; out[4] = p.D; out[5] = p.blocks; out[6] = p.bound;
    out[7] = (int64_t)p.lds_bytes; out[8] = p.wgs; out[9] = p.batches; out[10] = p.vi; out[11] = (int64_t)p.table_bytes;
    return BMM_OK;
}

int bmm_device_partition_distances(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion, int stride,
                                   double* loss_out, uint64_t* binder2_out, int* best_out, double* dist_out) {
    return guarded([&]() -> int {
        if (!z || !loss_out || !best_out) return set_err(BMM_E_ARG, "null argument");
        int rc = pt_check_shape(S, N, Kc, criterion, stride);
        if (rc == BMM_OK) rc = pt_check_labels(z, S, N, 1, Kc, nullptr);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(device));
        PtWork w;
        w.shape(S, N, Kc, criterion, stride);
        rc = w.alloc_labels();
        if (rc == BMM_OK) rc = w.alloc_pairs(dist_out != nullptr);
        if (rc == BMM_OK) rc = pt_upload(w, z);
        if (rc == BMM_OK) rc = pt_compute(nullptr, w);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipDeviceSynchronize());
        return pt_fetch(w, loss_out, binder2_out, best_out, dist_out);
    });
}

int bmm_device_psm(int device, const int32_t* z, int S, int64_t N, const int64_t* idx, int64_t M, uint32_t* cnt_out) {
    return guarded([&]() -> int {
        if (!z || !idx || !cnt_out) return set_err(BMM_E_ARG, "null argument");
        if (S < 1 || N < 1 || M < 1) return set_err(BMM_E_ARG, "similarity: S, N and M must be >= 1");
        if (S > BMM_PARTITION_MAX_ROWS) return set_err(BMM_E_ARG, "similarity: S = %d rows is more than the %d one call takes", S, BMM_PARTITION_MAX_ROWS);
        int rc = pt_check_idx(idx, M, N);
        int32_t top = 1;
        if (rc == BMM_OK) rc = pt_check_labels(z, S, N, 1, INT32_MAX, &top);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(device));
        PtWork w;
        w.shape(S, N, 1, BMM_PARTITION_BINDER, 1);
        w.Kc = top;  // only the width of a label and the range check depend on it here
        w.plan.el = top <= 256 ? 1 : 4;
        rc = w.alloc_labels();
        if (rc == BMM_OK) rc = pt_upload(w, z);
        if (rc) return rc;
        return pt_psm(nullptr, w, idx, M, cnt_out);
    });
}

// Which form of every k_pt_* kernel a shape runs, from the function the launches call (no device is touched)
int bmm_device_partition_plan(int S, int64_t N, int Kc, int n_candidates, int criterion, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    int rc = pt_check_shape(S, N, Kc, criterion, 1);
    if (rc) return rc;
    bool ok = false;  // C = ceil(S / stride) for some stride
    if (n_candidates >= 1 && n_candidates <= S) {
        const int st = (S + n_candidates - 1) / n_candidates;
        for (int q = st; q >= 1 && q >= st - 1; --q) ok = ok || (S + q - 1) / q == n_candidates;
    }
    if (!ok) return set_err(BMM_E_ARG, "partition: %d candidates is not ceil(%d / stride) for any stride", n_candidates, S);
    const PtPlan p = pt_plan(S, N, Kc, n_candidates, criterion);
    out[0] = p.el; out[1] = p.lds; out[2] = p.T; out[3] = p.R; out[4] = p.blocks; out[5] = p.wgs;
    out[6] = p.threads; out[7] = (int64_t)p.lds_bytes; out[8] = p.tri; out[9] = p.vi; out[10] = (int64_t)p.generic_bytes;
    out[11] = p.pitch;
    return BMM_OK;
}

// ---- ECR relabelling of any stack of label rows: the stand-alone entry points ----
int bmm_device_ecr(int device, const int32_t* z, int S, int64_t N, int K, const int32_t* pivot, int max_iter,
                   int32_t* perm_out, int64_t* agree_out, int32_t* pivot_out, int32_t* z_out, uint32_t* tables_out,
                   int* iterations, int* converged) {
    return guarded([&]() -> int {
        if (!z || !perm_out || !agree_out || !iterations || !converged) return set_err(BMM_E_ARG, "ecr: null argument");
        int rc = ecr_check_shape(S, N, K);
        if (rc) return rc;
        if (!pivot && max_iter < 1) return set_err(BMM_E_ARG, "ecr: max_iter must be >= 1 without a pivot (got %d)", max_iter);
        rc = pt_check_labels(z, S, N, 1, K, nullptr, "ecr");
        if (rc == BMM_OK && pivot) rc = ecr_check_pivot(pivot, N, K);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(device));
        PtWork lw;  // the label block: one byte per label (K <= 128), narrowed as the partition calls narrow it
        lw.shape(S, N, K, BMM_PARTITION_BINDER, 1);
        EcrWork w;
        DevBuf perm;
        rc = lw.alloc_labels();
        if (rc == BMM_OK) rc = w.alloc(S, N, K, true);
        if (rc) return rc;
        HIP_TRY(perm.alloc((size_t)S * K * sizeof(int32_t)));
        rc = pt_upload(lw, z);
        if (rc == BMM_OK) rc = ecr_perm_identity(nullptr, perm.as<int32_t>(), S, K);
        if (rc == BMM_OK && pivot) rc = ecr_upload_pivot(w.pivot.as<int32_t>(), pivot, N, nullptr);
        if (rc == BMM_OK)
            rc = ecr_compute<uint8_t>(nullptr, w, lw.lab.as<uint8_t>(), lw.plan.pitch, w.pivot.as<int32_t>(), perm.as<int32_t>(), S,
                                      pivot == nullptr, max_iter, iterations, converged);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipDeviceSynchronize());
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, lw.flag.p, sizeof flag, hipMemcpyDeviceToHost));
        if (flag) return set_err(BMM_E_STATE, "ecr: a label outside 0 .. %d reached the device", K - 1);
        HIP_TRY(hipMemcpy(perm_out, perm.p, (size_t)S * K * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(agree_out, w.agree.p, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (tables_out) HIP_TRY(hipMemcpy(tables_out, w.tables.p, (size_t)S * K * K * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (pivot_out) {
            HIP_TRY(hipMemcpy(pivot_out, w.pivot.p, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < N; ++i) pivot_out[i] += 1;
        }
        if (z_out) {  // z_out = perm[z - 1] + 1: observation i's S labels are contiguous
            HostCrew crew;
            crew.run(N, 1024, 64, [&](int64_t lo, int64_t hi) {
                for (int64_t i = lo; i < hi; ++i)
                    for (int s = 0; s < S; ++s)
                        z_out[(size_t)i * S + s] = perm_out[(size_t)s + (size_t)(z[(size_t)i * S + s] - 1) * S] + 1;
            });
        }
        return BMM_OK;
    });
}

int bmm_device_ecr_plan(int S, int64_t N, int K, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    int rc = ecr_check_shape(S, N, K);
    if (rc) return rc;
    const EcrPlan p = ecr_plan(S, N, K);
    out[0] = 1; out[1] = p.tab_lds; out[2] = p.T; out[3] = p.R; out[4] = p.row_blocks; out[5] = p.slices;
    out[6] = p.span; out[7] = (int64_t)p.tab_lds_bytes; out[8] = p.votes_lds; out[9] = p.votes_wgs;
    out[10] = (int64_t)p.votes_bytes; out[11] = p.pitch;
    return BMM_OK;
}

// ---- posterior summary: the pure functions and the resident entry points ----
int64_t bmm_run_bytes(int sampler, int64_t N, int P, int K, int S, int keep_trace, int summary) {
    if (sampler < 0 || sampler > 3 || N < 1 || P < 1 || K < 1 || S < 1) return -1;
    Carver measure{nullptr};
    (void)run_carve(measure, sampler, N, P, K, S, keep_trace != 0);
    size_t bytes = measure.used;
    if (summary) bytes += sum_plan(N, P, K).bytes_block + (size_t)S * sum_row_bytes(K);
    return (int64_t)bytes;
}
int bmm_summary_plan(int64_t N, int P, int K, int64_t out[12]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    if (N < 1 || P < 1 || K < 1) return set_err(BMM_E_ARG, "summary: N, P and K must be >= 1");
    if (N >= ((int64_t)1 << 32)) return set_err(BMM_E_ARG, "summary: N must be below 2^32 (the counts are uint32)");
    const SumPlan q = sum_plan(N, P, K);
    out[0] = kSumThreads; out[1] = q.fold_wgs; out[2] = kSumGridCap; out[3] = q.pitch; out[4] = (int64_t)q.fold_lds;
    out[5] = q.prof_wgs; out[6] = q.finish_wgs; out[7] = (int64_t)q.finish_lds; out[8] = (int64_t)q.bytes_counts;
    out[9] = (int64_t)q.bytes_block; out[10] = kSumLaunchesPivot; out[11] = kSumLaunchesPlain;
    return BMM_OK;
}
static int sum_armed(const bmm_chain* c) {
    if (!c->sum_on) return set_err(BMM_E_STATE, "the summary is not armed (bmm_chain_set_summary)");
    return BMM_OK;
}
int bmm_chain_set_summary(bmm_chain* c, const bmm_summary_opts* opts) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        HIP_TRY(hipSetDevice(c->device));
        if (!opts) {  // disarm: the memory goes
            HIP_TRY(hipStreamSynchronize(c->stream));
            sum_release(c);
            return BMM_OK;
        }
        return sum_arm(c, *opts);
    });
}
int bmm_chain_summary_state(bmm_chain* c, int32_t* perm_out, int64_t* agree_out) {
    return guarded([&]() -> int {
        if (!c || !perm_out || !agree_out) return set_err(BMM_E_ARG, "null argument");
        int rc = sum_armed(c);
        if (rc) return rc;
        if (c->p.mode != MODE_COLLAPSED && c->sweep < 1)
            return set_err(BMM_E_STATE, "no row has a label before the first sweep: this state has nothing to relabel");
        const int K = c->p.K;
        HIP_TRY(hipSetDevice(c->device));
        if (c->sum_pivot_kind == BMM_SUMMARY_PIVOT_NONE) {
            for (int k = 0; k < K; ++k) perm_out[k] = k;
            *agree_out = 0;
            return BMM_OK;
        }
        if (!c->sum_have_pivot) return set_err(BMM_E_STATE, "the summary has no pivot yet: it is the state after the first sweep of bmm_chain_sweeps_summary");
        if (!c->started) { rc = chain_start(c); if (rc) return rc; }
        rc = ecr_perm_identity(c->stream, c->sum.perm_live, 1, K);
        if (rc == BMM_OK) rc = sum_relabel(c, label_row(c, c->sweep), c->sum.perm_live);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        HIP_TRY(hipMemcpyAsync(perm_out, c->sum.perm_live, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(agree_out, c->sum_ecr->agree.p, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BMM_OK;
    });
}
// n more sweeps, every sum_stride-th folded from the first on
int bmm_chain_sweeps_summary(bmm_chain* c, int n, int64_t* agree, int32_t* permutations) {
    return guarded([&]() -> int {
        if (!c) return set_err(BMM_E_ARG, "null chain");
        if (n < 0) return set_err(BMM_E_ARG, "n must be >= 0");
        int rc = sum_refused(c);
        if (rc == BMM_OK) rc = sum_armed(c);
        if (rc || n == 0) return rc;
        if (c->in_run) return set_err(BMM_E_STATE, "not offered inside a run");
        HIP_TRY(hipSetDevice(c->device));
        Recording rec;
        if (agree || permutations) {
            rc = sum_rows_alloc(c, rec, n);
            if (rc) return rc;
        }
        rec.begin(c, c->sum_rec, sum_row_bytes(c->p.K), c->sweep + 1, c->sweep + 1, true);
        rc = bmm_chain_sweeps(c, n);
        const hipError_t e = rec.end();
        if (rc || !rec.rows.p) return rc;
        if (e != hipSuccess) return set_err(BMM_E_HIP, "the sweeps failed: %s", hipGetErrorString(e));
        return sum_rows_out(c, rec, n, agree, permutations);
    });
}
int bmm_chain_get_summary(bmm_chain* c, bmm_summary_out* out) {
    return guarded([&]() -> int {
        if (!c || !out) return set_err(BMM_E_ARG, "null argument");
        const int rc = sum_armed(c);
        return rc ? rc : sum_get(c, *out);
    });
}
int bmm_chain_summary_reset(bmm_chain* c) {
    if (!c) return set_err(BMM_E_ARG, "null chain");
    const int rc = sum_armed(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return sum_reset(c);
}

// ---- several independent chains in one call (SURVEY.md section 8 rows b, e) ----------------
// Where bmm_multi_run puts things, as pure bookkeeping (no device is touched; tests/test_capi_cpu.py): the
// distinct devices in first-use order -- the RCCL broadcast list, root first -- and for every chain the chain
// that holds its device's copy of the bit planes (the first chain on that device; a holder names itself).
int bmm_multi_plan(int n_chains, const int* devices, int* n_devices_out, int* devices_out, int* holder_of_chain) {
    if (n_chains < 1 || !n_devices_out || !devices_out || !holder_of_chain) return set_err(BMM_E_ARG, "bad argument");
    int nd = 0;
    for (int c = 0; c < n_chains; ++c) {
        const int d = devices ? devices[c] : 0;
        if (d < 0) return set_err(BMM_E_ARG, "devices[%d] = %d is not a device index", c, d);
        int first = -1;
        for (int e = 0; e < c && first < 0; ++e)
            if ((devices ? devices[e] : 0) == d) first = e;
        holder_of_chain[c] = first < 0 ? c : holder_of_chain[first];
        if (first < 0) devices_out[nd++] = d;
    }
    *n_devices_out = nd;
    return BMM_OK;
}

int bmm_multi_run(int sampler, int n_chains, const int* devices, const int32_t* X, int64_t N, int P,
                  const int32_t* const* initialK, const double* const* initialPi,
                  const double* const* initialTheta, int nsamples, int K, double alpha, double beta,
                  double gamma, double a, double b, int burnin, int64_t batch, uint64_t seed,
                  double* const* pi_out, int32_t* const* z_out, double* const* theta_out,
                  double* const* alpha_out) {
    const RunOptions armed = take_run_options();  // a run of several chains disarms whatever was armed ...
    const bool na_armed = armed.na.on, cs_armed = armed.cs.on, cat_armed = armed.cat.on;
    const RunOptions opts;     // ... and runs every chain without it
    return guarded([&]() -> int {
        // (... but does not run over a matrix whose holes were zeroed as if nothing had been said)
        if (na_armed) return set_err(BMM_E_UNSUPPORTED, "missing cells (bmm_set_missing) are not offered by a run of several chains: they share one matrix");
        if (cs_armed) return set_err(BMM_E_UNSUPPORTED, "constrained rows (bmm_set_constraints) are not offered by a run of several chains");
        if (cat_armed) return set_err(BMM_E_UNSUPPORTED, "categorical features (bmm_set_categorical) are not offered by a run of several chains (bmm_multi_run)");
        if (sampler < 0 || sampler > 3) return set_err(BMM_E_ARG, "unknown sampler %d", sampler);
        if (n_chains < 1) return set_err(BMM_E_ARG, "n_chains must be >= 1");
        if (!z_out || !theta_out || !alpha_out) return set_err(BMM_E_ARG, "null output table");
        if (sampler == BMM_SAMPLER_COLLAPSED && !initialK) return set_err(BMM_E_ARG, "initialK is null");
        if (explicit_params(sampler) && (!initialPi || !initialTheta || !pi_out)) return set_err(BMM_E_ARG, "null buffer table");
        std::vector<RunIO> io((size_t)n_chains);
        for (int c = 0; c < n_chains; ++c) {
            RunIO& q = io[(size_t)c];
            q = explicit_params(sampler) ? explicit_io(initialPi[c], initialTheta[c], pi_out[c], z_out[c], theta_out[c], alpha_out[c])
                                         : counting_io(sampler == BMM_SAMPLER_COLLAPSED ? initialK[c] : nullptr, z_out[c], theta_out[c], alpha_out[c]);
            int rc = check_run_args(X, nsamples, burnin, q, sampler);
            if (rc) return rc;
        }
        // chain c lives on devices[c] (device 0 when the table is null); distinct devices in first-use order
        std::vector<int> dev_of((size_t)n_chains), devs((size_t)n_chains), holder_idx((size_t)n_chains);
        int ndev = 0;
        {
            int rcp = bmm_multi_plan(n_chains, devices, &ndev, devs.data(), holder_idx.data());
            if (rcp) return rcp;
            devs.resize((size_t)ndev);
            for (int c = 0; c < n_chains; ++c) dev_of[(size_t)c] = devices ? devices[c] : 0;
        }
        std::vector<bmm_chain*> chains((size_t)n_chains, nullptr);
        struct Guard {
            std::vector<bmm_chain*>& v;
            ~Guard() { for (bmm_chain* c : v) bmm_chain_destroy(c); }  // shared planes go with their last chain
        } guard{chains};
        int rc = BMM_OK;
        for (int c = 0; c < n_chains && rc == BMM_OK; ++c) {
            rc = bmm_chain_create(&chains[(size_t)c], sampler, N, P, K, alpha, beta, gamma, a, b, batch,
                                  seed + (uint64_t)c, dev_of[(size_t)c]);
            if (rc == BMM_OK) rc = run_prepare(chains[(size_t)c], nsamples, burnin);
        }
        if (rc) return rc;
        // the data: uploaded and packed once, on the first chain's device; the bit planes (not the int32
        // matrix: 160 MB instead of 4 GB at K=20, N=1e7, P=100) broadcast once to the other devices
        std::vector<bmm_chain*> holder(devs.size(), nullptr);  // first chain of each device: owns its planes
        for (size_t q = 0; q < devs.size(); ++q)
            for (int c = 0; c < n_chains && !holder[q]; ++c)
                if (holder_idx[(size_t)c] == c && dev_of[(size_t)c] == devs[q]) holder[q] = chains[(size_t)c];
        rc = bmm_chain_set_data_host(holder[0], X);
        if (rc) return rc;
        if (devs.size() > 1) {
            if (!holder[0]->bits) return set_err(BMM_E_UNSUPPORTED, "a run over several devices broadcasts bit planes");
            std::vector<void*> bufs(devs.size(), nullptr);
            int64_t words = 0;
            for (size_t q = 0; q < devs.size() && rc == BMM_OK; ++q) rc = bmm_chain_planes(holder[q], &bufs[q], &words);
            if (rc == BMM_OK) rc = rccl_broadcast_words(devs, bufs, (size_t)words);
            for (size_t q = 1; q < devs.size() && rc == BMM_OK; ++q) rc = bmm_chain_planes_filled(holder[q]);
            if (rc) return rc;
        }
        for (int c = 0; c < n_chains; ++c) {  // every other chain shares its device's copy
            if (holder_idx[(size_t)c] == c) continue;
            rc = bmm_chain_share_data(chains[(size_t)c], chains[(size_t)holder_idx[(size_t)c]]);
            if (rc) return rc;
        }
        // one host thread per chain; each enqueues on its own stream, so chains on one device overlap
        std::vector<int> status((size_t)n_chains, BMM_OK);
        std::vector<std::string> msg((size_t)n_chains);
        {
            ThreadGroup tg;  // joined also when starting a later thread throws: the workers hold references
            tg.th.reserve((size_t)n_chains);
            for (int c = 0; c < n_chains; ++c)
                tg.th.emplace_back([&, c]() {
                    // no exception may leave a thread: the trace's way out starts helper threads of its own
                    status[(size_t)c] = guarded([&]() -> int {
                        int rcw = run_start_state(chains[(size_t)c], io[(size_t)c]);
                        if (rcw == BMM_OK) rcw = run_body(chains[(size_t)c], nsamples, io[(size_t)c], opts);
                        return rcw;
                    });
                    try {
                        if (status[(size_t)c]) msg[(size_t)c] = bmm_last_error();
                    } catch (...) {  // the message could not be copied: the status stands
                    }
                });
        }
        for (int c = 0; c < n_chains; ++c)
            if (status[(size_t)c]) return set_err(status[(size_t)c], "chain %d: %s", c, msg[(size_t)c].c_str());
        return BMM_OK;
    });
}

// n resident chains advanced by `sweeps` sweeps each, one host thread per chain (launches of chains
// that share a device overlap on their streams).  Returns without waiting for the GPU, as bmm_chain_sweeps.
int bmm_chains_sweeps(bmm_chain* const* chains, int n_chains, int sweeps) {
    return guarded([&]() -> int {
        if (!chains || n_chains < 1) return set_err(BMM_E_ARG, "no chains");
        if (n_chains == 1) return bmm_chain_sweeps(chains[0], sweeps);
        std::vector<int> status((size_t)n_chains, BMM_OK);
        std::vector<std::string> msg((size_t)n_chains);
        {
            ThreadGroup tg;  // joined also when starting a later thread throws
            tg.th.reserve((size_t)n_chains);
            for (int c = 0; c < n_chains; ++c)
                tg.th.emplace_back([&, c]() {
                    status[(size_t)c] = bmm_chain_sweeps(chains[c], sweeps);  // guarded inside
                    try {
                        if (status[(size_t)c]) msg[(size_t)c] = bmm_last_error();
                    } catch (...) {
                    }
                });
        }
        for (int c = 0; c < n_chains; ++c)
            if (status[(size_t)c]) return set_err(status[(size_t)c], "chain %d: %s", c, msg[(size_t)c].c_str());
        return BMM_OK;
    });
}

// The data of resident chains on different devices from the first one's: chains[0] holds the bit planes
// (its data are set); every other chain -- one per further device -- receives them over RCCL, as in
// bmm_multi_run.  What a single-process multi-GPU driver of the resident API (bench.py without
// torch.distributed.run) calls once before the sweeps.
int bmm_chains_broadcast_planes(bmm_chain* const* chains, int n_chains) {
    return guarded([&]() -> int {
        if (!chains || n_chains < 1 || !chains[0]) return set_err(BMM_E_ARG, "no chains");
        if (!chains[0]->have_data || !chains[0]->bits) return set_err(BMM_E_STATE, "the first chain holds no bit planes");
        std::vector<int> devs;
        std::vector<void*> bufs((size_t)n_chains, nullptr);
        int64_t words = 0;
        for (int c = 0; c < n_chains; ++c) {
            bmm_chain* ch = chains[c];
            if (!ch) return set_err(BMM_E_ARG, "null chain");
            for (int d : devs)
                if (d == ch->slot) return set_err(BMM_E_ARG, "one chain per device here; chains on one device share (bmm_chain_share_data)");
            if (ch->p.N != chains[0]->p.N || ch->p.P != chains[0]->p.P) return set_err(BMM_E_ARG, "the chains differ in N or P");
            devs.push_back(ch->slot);
            int rc = bmm_chain_planes(ch, &bufs[(size_t)c], &words);
            if (rc) return rc;
        }
        int rc = rccl_broadcast_words(devs, bufs, (size_t)words);
        for (int c = 1; c < n_chains && rc == BMM_OK; ++c) rc = bmm_chain_planes_filled(chains[c]);
        return rc;
    });
}

// The broadcast of bmm_multi_run on a pattern: fills `words` 32-bit words on devices[0], broadcasts them
// to every listed device through RCCL (also with a single device: the library is opened, a
// communicator built and the collective run) and compares.  What a box without several GPUs can check.
int bmm_multi_selfcheck(int n_devices, const int* devices, int64_t words) {
    return guarded([&]() -> int {
        if (n_devices < 1 || !devices || words < 1) return set_err(BMM_E_ARG, "bad argument");
        std::vector<int> devs(devices, devices + n_devices);
        for (int q = 0; q < n_devices; ++q)
            for (int r2 = 0; r2 < q; ++r2)
                if (devs[(size_t)q] == devs[(size_t)r2]) return set_err(BMM_E_ARG, "devices must be distinct");
        std::vector<uint32_t> pat((size_t)words), got((size_t)words);
        for (int64_t i = 0; i < words; ++i) pat[(size_t)i] = (uint32_t)i * 2654435761u + 12345u;
        std::vector<DevBuf> bufs((size_t)n_devices);
        std::vector<void*> ptrs((size_t)n_devices);
        for (int q = 0; q < n_devices; ++q) {
            HIP_TRY(hipSetDevice(devs[(size_t)q]));
            HIP_TRY(bufs[(size_t)q].alloc((size_t)words * 4));
            ptrs[(size_t)q] = bufs[(size_t)q].p;
            if (q == 0) HIP_TRY(hipMemcpy(ptrs[0], pat.data(), (size_t)words * 4, hipMemcpyHostToDevice));
            else HIP_TRY(hipMemset(ptrs[(size_t)q], 0, (size_t)words * 4));
        }
        if (n_devices == 1) {  // rccl_broadcast_words skips a single device; here the collective itself is the point
            Rccl r;
            int rc = rccl_open(r);
            if (rc) return rc;
            ncclComm_t comm = nullptr;
            ncclResult_t e = r.CommInitAll(&comm, 1, devs.data());
            if (e != ncclSuccess) return set_err(BMM_E_RCCL, "ncclCommInitAll failed: %s", r.GetErrorString(e));
            hipStream_t st = nullptr;
            hipError_t he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (he == hipSuccess) {
                e = r.Broadcast(ptrs[0], ptrs[0], (size_t)words, ncclUint32, 0, comm, st);
                he = hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
            }
            (void)r.CommDestroy(comm);
            if (he != hipSuccess) return set_err(BMM_E_HIP, "self-check stream failed: %s", hipGetErrorString(he));
            if (e != ncclSuccess) return set_err(BMM_E_RCCL, "ncclBroadcast failed: %s", r.GetErrorString(e));
        } else {
            int rc = rccl_broadcast_words(devs, ptrs, (size_t)words);
            if (rc) return rc;
        }
        for (int q = 0; q < n_devices; ++q) {
            HIP_TRY(hipSetDevice(devs[(size_t)q]));
            HIP_TRY(hipMemcpy(got.data(), ptrs[(size_t)q], (size_t)words * 4, hipMemcpyDeviceToHost));
            if (std::memcmp(got.data(), pat.data(), (size_t)words * 4) != 0)
                return set_err(BMM_E_RCCL, "device %d holds different words after the broadcast", devs[(size_t)q]);
        }
        return BMM_OK;
    });
}

int bmm_device_math(int device, int op, const double* in, const double* in2, double* out, int64_t n) {
    if (!in || !out || n < 0 || op < 0 || op > 5) return set_err(BMM_E_ARG, "bad argument");
    if (op == 2 && !in2) return set_err(BMM_E_ARG, "division needs in2");
    HIP_TRY(hipSetDevice(device));
    DevBuf bi, bi2, bo;
    HIP_TRY(bi.alloc(n * sizeof(double)));
    HIP_TRY(bo.alloc(n * sizeof(double)));
    HIP_TRY(hipMemcpy(bi.p, in, n * sizeof(double), hipMemcpyHostToDevice));
    if (in2) {
        HIP_TRY(bi2.alloc(n * sizeof(double)));
        HIP_TRY(hipMemcpy(bi2.p, in2, n * sizeof(double), hipMemcpyHostToDevice));
    }
    if (op == 5)
        hipLaunchKernelGGL(k_test_lgamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, bi.as<double>(), bo.as<double>(), n);
    else
        hipLaunchKernelGGL(k_test_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, bi.as<double>(),
                           bi2.as<double>(), bo.as<double>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, bo.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}

#ifdef BMM_DEBUG_HOOKS
// Test variant only: k_resample_pk's draw (spec = 0) or bmm_spec.h's draw_pk (spec = 1) on n rows of kt scores each and
// their uniforms, on the device (k_test_pk_draw); out[2 i ...] = count and verdict.
int bmm_dbg_pk_draw(int device, int kt, int spec, const float* scores, const double* u, int G, int64_t n, int* out) {
    if (!scores || !u || !out || n < 0) return set_err(BMM_E_ARG, "bad argument");
    if (kt != 4 && kt != 12 && kt != 20 && kt != 32)
        return set_err(BMM_E_ARG, "the draw is instantiated for 4, 12, 20 and 32 accumulators");
    HIP_TRY(hipSetDevice(device));
    DevBuf bs, bu, bo;
    HIP_TRY(bs.alloc((size_t)n * kt * sizeof(float)));
    HIP_TRY(bu.alloc((size_t)n * sizeof(double)));
    HIP_TRY(bo.alloc((size_t)n * 2 * sizeof(int)));
    HIP_TRY(hipMemcpy(bs.p, scores, (size_t)n * kt * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bu.p, u, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n + 255) / 256));
#define BMM_TEST_PK_DRAW(KT)                                                                                              \
    if (spec) hipLaunchKernelGGL((k_test_pk_draw<KT, true>), grid, dim3(256), 0, 0, bs.as<float>(), bu.as<double>(), G, n, bo.as<int>()); \
    else hipLaunchKernelGGL((k_test_pk_draw<KT, false>), grid, dim3(256), 0, 0, bs.as<float>(), bu.as<double>(), G, n, bo.as<int>())
    if (kt == 4) { BMM_TEST_PK_DRAW(4); }
    else if (kt == 12) { BMM_TEST_PK_DRAW(12); }
    else if (kt == 20) { BMM_TEST_PK_DRAW(20); }
    else { BMM_TEST_PK_DRAW(32); }
#undef BMM_TEST_PK_DRAW
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, bo.p, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
    return BMM_OK;
}
#endif

int bmm_device_variates(int device, int kind, double p, double q, uint64_t seed, uint32_t sweep, double* out,
                        int64_t n) {
    if (!out || n < 0 || kind < 0 || kind > 2) return set_err(BMM_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    DevBuf bo;
    HIP_TRY(bo.alloc(n * sizeof(double)));
    hipLaunchKernelGGL(k_test_variates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, p, q, seed, sweep,
                       bo.as<double>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, bo.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}

int bmm_device_variates_ex(int device, int kind, const double* p, const double* q, double a, double b, double N,
                           uint64_t seed, uint32_t sweep, double* out, int64_t n) {
    if (!out || !p || n < 0 || n > (int64_t)1 << 30 || kind < 0 || kind > 4 || (kind != 0 && !q))
        return set_err(BMM_E_ARG, "bad argument");
    if (n == 0) return BMM_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf bp, bq, bo;
    HIP_TRY(bp.alloc(n * sizeof(double)));
    HIP_TRY(bo.alloc(n * sizeof(double)));
    HIP_TRY(hipMemcpy(bp.p, p, n * sizeof(double), hipMemcpyHostToDevice));
    if (q) {
        HIP_TRY(bq.alloc(n * sizeof(double)));
        HIP_TRY(hipMemcpy(bq.p, q, n * sizeof(double), hipMemcpyHostToDevice));
    }
    if (kind <= 2)
        hipLaunchKernelGGL(k_test_variates_ex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, bp.as<double>(),
                           bq.as<double>(), a, b, N, seed, sweep, bo.as<double>(), n);
    else if (kind == 3)
        hipLaunchKernelGGL(k_test_alpha_wave, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, bp.as<double>(),
                           bq.as<double>(), a, b, N, seed, sweep, bo.as<double>(), n);
    else
        hipLaunchKernelGGL(k_test_split_beta, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, 0, bp.as<double>(),
                           bq.as<double>(), seed, sweep, bo.as<double>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, bo.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return BMM_OK;
}

}  // extern "C"

// ---- an ensemble of exact chains (include/bmm_mcmc.h "ensemble of exact chains") ----
namespace {

// What follows from (sampler, N, P, K, chains) alone: the shape of the launches and the bytes, or the refusal.
struct EnsPlan {
    int W = 0, Kc = 0, cpw = 0, groups = 0, launches = 0;
    int64_t slice = 0, state_bytes = 0, row_bytes = 0, label_row_bytes = 0;
};
int ens_plan(int sampler, int64_t N, int P, int K, int chains, EnsPlan& o) {
    if (sampler != BMM_SAMPLER_COLLAPSED && sampler != BMM_SAMPLER_DP)
        return set_err(BMM_E_UNSUPPORTED, "an ensemble runs the collapsed and DP samplers only: the explicit samplers' z-step is exact already");
    if (chains < 1) return set_err(BMM_E_ARG, "chains must be >= 1");
    if (N < 1) return set_err(BMM_E_ARG, "N must be >= 1");
    if (P < 1) return set_err(BMM_E_ARG, "P must be >= 1");
    if (K < 1) return set_err(BMM_E_ARG, "K must be >= 1");
    const bool dp = sampler == BMM_SAMPLER_DP;
    if (dp && K < 2) return set_err(BMM_E_ARG, "maxK must be >= 2");
    o.Kc = dp ? K + 1 : K;
    if (o.Kc > kEnsMaxCats)
        return set_err(BMM_E_UNSUPPORTED, "an ensemble chain scores its categories on the lanes of one wave: %d categories exceed %d", o.Kc, kEnsMaxCats);
    if (P > kEnsMaxP) return set_err(BMM_E_UNSUPPORTED, "an ensemble chain takes at most %d features: P = %d", kEnsMaxP, P);
    if (N >= kEnsMaxN)
        return set_err(BMM_E_UNSUPPORTED, "an ensemble chain takes fewer than %d observations: N = %lld", kEnsMaxN, (long long)N);
    o.slice = ens_slice_bytes(P, K, o.Kc);
    if ((size_t)o.slice > kLdsMax)
        return set_err(BMM_E_UNSUPPORTED, "the terms of one ensemble chain (%lld bytes at K = %d, P = %d) do not fit in the %zu bytes of LDS of a workgroup",
                       (long long)o.slice, K, P, kLdsMax);
    o.W = group_width_rule(sampler, K, P);
    const int fit = (int)(kLdsMax / (size_t)o.slice);
    o.cpw = fit < kEnsWaves ? fit : kEnsWaves;
    o.groups = (chains + o.cpw - 1) / o.cpw;
    o.launches = (int)((N + ens_rows(P) - 1) / ens_rows(P));
    o.state_bytes = (int64_t)chains * (N * 4 + (int64_t)K * 4 + (int64_t)K * P * 4 + 8);
    o.row_bytes = (int64_t)chains * ((int64_t)K * 4 + (int64_t)K * P * 8 + 8);
    o.label_row_bytes = (int64_t)chains * N * 4;
    return BMM_OK;
}
bool ens_options_armed(const RunOptions& o) {
    return o.partition.on || o.psearch.on || o.cball.on || o.loo.on || o.sm.moves > 0 || o.fs.on || o.init.kind != 0 || o.ecr.on ||
           o.logpost.on || o.temper.on || o.pc.on || o.na.on || o.alloc.on || o.as.moves > 0 || o.cs.on || o.summary.on || o.cat.on ||
           o.hooks || o.rel || o.pred || o.pna.on;
}

// The folds of an ensemble: what follows from the plan and (M, loo) alone
struct EnsFoldPlan {
    int64_t acc_bytes = 0, loo_row_bytes = 0, pred_row_bytes = 0;
    int launches = 0;
};
EnsFoldPlan ens_fold_plan(int64_t N, int P, int chains, int64_t M, bool loo) {
    EnsFoldPlan o;
    if (loo) {
        o.acc_bytes += (int64_t)chains * ((kLooAcc + kLooOut) * N + 8) * 8;
        o.loo_row_bytes = (int64_t)chains * N * 8;
        o.launches++;
    }
    if (M > 0) {
        o.acc_bytes += (int64_t)chains * 3 * M * 8 + (int64_t)((P + 31) / 32) * M * 4;
        o.pred_row_bytes = (int64_t)chains * M * 8;
        o.launches++;
    }
    return o;
}
// the struct as handed over: the new rows binary, every table that is asked for in place; no device
int ens_folds_check(const bmm_ensemble_folds& f, int chains, int P) {
    if (f.M < 0) return set_err(BMM_E_ARG, "M must be >= 0");
    auto table = [&](const void* const* t, const char* name) -> int {
        if (!t) return set_err(BMM_E_ARG, "null buffer: %s", name);
        for (int c = 0; c < chains; ++c)
            if (!t[c]) return set_err(BMM_E_ARG, "null buffer: %s (chain %d)", name, c);
        return BMM_OK;
    };
    int rc = BMM_OK;
    if (f.M > 0) {
        if (!f.newdata) return set_err(BMM_E_ARG, "Xnew is null");
        const int64_t cells = f.M * (int64_t)P;
        for (int64_t q = 0; q < cells; ++q)
            if ((uint32_t)f.newdata[q] > 1u) return set_err(BMM_E_ARG, "newdata must be binary: Xnew holds a value other than 0 and 1");
        rc = table(reinterpret_cast<const void* const*>(f.pred_lppd), "pred_lppd");
        if (rc == BMM_OK && f.predictive_trace) rc = table(reinterpret_cast<const void* const*>(f.pred_logdens), "pred_logdens");
        if (rc) return rc;
    }
    if (f.loo) {
        const void* const* t[] = {reinterpret_cast<const void* const*>(f.loo_log_cpo), reinterpret_cast<const void* const*>(f.loo_ess),
                                  reinterpret_cast<const void* const*>(f.loo_lppd), reinterpret_cast<const void* const*>(f.loo_mean),
                                  reinterpret_cast<const void* const*>(f.loo_var)};
        const char* const names[] = {"loo_log_cpo", "loo_ess", "loo_lppd", "loo_mean", "loo_var"};
        for (int q = 0; q < 5 && rc == BMM_OK; ++q) rc = table(t[q], names[q]);
        if (rc == BMM_OK && f.loo_trace) rc = table(reinterpret_cast<const void* const*>(f.loo_ell), "loo_ell");
        if (rc == BMM_OK && (!f.loo_lpml || !f.loo_min_ess)) rc = set_err(BMM_E_ARG, "null buffer: loo_lpml, loo_min_ess");
    }
    return rc;
}
// a device trace [chains][S][width] into each chain's S x width column-major matrix; the rows before the first fold NaN
int ens_trace_out(const double* dtrace, int chains, int64_t width, int S, int first, double* const* out) {
    std::vector<double> hrow((size_t)S * (size_t)width);
    for (int c = 0; c < chains; ++c) {
        HIP_TRY(hipMemcpy(hrow.data(), dtrace + (size_t)c * hrow.size(), hrow.size() * 8, hipMemcpyDeviceToHost));
        for (int s = 0; s < S; ++s)
            for (int64_t m = 0; m < width; ++m)
                out[c][(size_t)s + (size_t)m * (size_t)S] = s < first ? std::nan("") : hrow[(size_t)s * (size_t)width + (size_t)m];
    }
    return BMM_OK;
}
// the outputs of the folds after the run (the stream is idle): as loo_run_out and pred_run_collect fill them
int ens_folds_out(const bmm_ensemble_folds& f, int chains, int64_t N, int64_t M, int S, int burnin, int folded, const double* dlout,
                  const double* dltr, const double* dpout, const double* dptr) {
    const double nan = std::nan("");
    const int first = burnin > 0 ? 0 : 1;
    const size_t n = (size_t)N, m = (size_t)M;
    if (f.n_folded) *f.n_folded = folded;
    if (f.loo) {
        double* const* const rows[kLooOut] = {f.loo_log_cpo, f.loo_ess, f.loo_lppd, f.loo_mean, f.loo_var};
        const size_t lout = n * kLooOut + 8;
        std::vector<double> ho(folded > 0 ? lout : 0);
        for (int c = 0; c < chains; ++c) {
            if (folded > 0) HIP_TRY(hipMemcpy(ho.data(), dlout + (size_t)c * lout, lout * 8, hipMemcpyDeviceToHost));
            for (int q = 0; q < kLooOut; ++q)
                for (size_t i = 0; i < n; ++i) rows[q][c][i] = folded > 0 ? ho[(size_t)q * n + i] : nan;
            f.loo_lpml[c] = folded > 0 ? ho[n * kLooOut] : nan;
            f.loo_min_ess[c] = folded > 0 ? ho[n * kLooOut + 1] : nan;
        }
        if (f.loo_trace) {
            const int rc = ens_trace_out(dltr, chains, N, S, folded > 0 ? first : S, f.loo_ell);
            if (rc) return rc;
        }
    }
    if (M > 0) {
        for (int c = 0; c < chains; ++c) {
            if (folded > 0) HIP_TRY(hipMemcpy(f.pred_lppd[c], dpout + (size_t)c * m, m * 8, hipMemcpyDeviceToHost));
            else for (size_t q = 0; q < m; ++q) f.pred_lppd[c][q] = nan;
        }
        if (f.predictive_trace) {
            const int rc = ens_trace_out(dptr, chains, M, S, folded > 0 ? first : S, f.pred_logdens);
            if (rc) return rc;
        }
    }
    return BMM_OK;
}

}  // namespace

extern "C" {

int bmm_ensemble_plan(int sampler, int64_t N, int P, int K, int chains, int64_t out[8]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    EnsPlan pl;
    const int rc = ens_plan(sampler, N, P, K, chains, pl);
    if (rc) return rc;
    out[0] = pl.W; out[1] = pl.slice; out[2] = pl.cpw; out[3] = pl.groups; out[4] = pl.launches;
    out[5] = pl.state_bytes; out[6] = pl.row_bytes; out[7] = pl.label_row_bytes;
    return BMM_OK;
}

// The run behind both entries; f: the folds asked for, or null (bmm_ensemble_run)
static int ens_run(const RunOptions& opts, int sampler, const int32_t* X, int64_t N, int P, int chains, const int32_t* const* z0,
                   int nsamples, int K, double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed,
                   int device, int32_t* const* z_out, int32_t* const* nk_out, double* const* theta_out, double* const* alpha_out,
                   int32_t* const* z_last, const bmm_ensemble_folds* f) {
    return guarded([&]() -> int {
        // refused before any device is touched
        if (ens_options_armed(opts)) return set_err(BMM_E_UNSUPPORTED, "an ensemble runs plain chains: no run option is offered (the traces feed the stand-alone tools)");
        EnsPlan pl;
        int rc = ens_plan(sampler, N, P, K, chains, pl);
        if (rc) return rc;
        const bool dp = sampler == BMM_SAMPLER_DP;
        if (!(beta > 0.0) || !(gamma > 0.0)) return set_err(BMM_E_ARG, "beta and gamma must be > 0");
        if (dp && beta != gamma)  // collapsed_gibbs_dp.cpp:48-50
            return set_err(BMM_E_ARG, "Error: sampler currently not implemented for non-symmetric priors on beta and gamma");
        if (alpha < 0.0) return set_err(BMM_E_ARG, "alpha must be >= 0 (0 = sample it)");
        if (nsamples < 1) return set_err(BMM_E_ARG, "nsamples must be >= 1");
        if (burnin < 0 || burnin >= nsamples) return set_err(BMM_E_ARG, "burnin must be in [0, nsamples)");
        if (!X || !nk_out || !theta_out || !alpha_out || !z_last || (!dp && !z0)) return set_err(BMM_E_ARG, "null buffer");
        for (int c = 0; c < chains; ++c)
            if (!nk_out[c] || !theta_out[c] || !alpha_out[c] || !z_last[c] || (z_out && !z_out[c]) || (!dp && !z0[c]))
                return set_err(BMM_E_ARG, "null buffer (chain %d)", c);
        if (dbg_env("BMM_X_LAYOUT_INT32") != nullptr)
            return set_err(BMM_E_UNSUPPORTED, "an ensemble reads the bit planes: not offered on the int32 layout");
        const int S = nsamples - burnin;
        const size_t KP = (size_t)K * P, n = (size_t)N;
        // the folds: what is asked for, and its buffers, before a device is touched
        const bool f_loo = f && f->loo != 0, f_pred = f && f->M > 0;
        const int64_t M = f_pred ? f->M : 0;
        if (f) {
            rc = ens_folds_check(*f, chains, P);
            if (rc) return rc;
        }
        // the starting state of every chain, on the host: labels (0-based, -1 unassigned) and their counts
        std::vector<int32_t> hz((size_t)chains * n, -1), hnk((size_t)chains * K, 0), hs((size_t)chains * KP, 0);
        if (!dp) {
            for (int c = 0; c < chains; ++c) {
                int32_t* const nk = hnk.data() + (size_t)c * K;
                int32_t* const s = hs.data() + (size_t)c * KP;
                for (size_t i = 0; i < n; ++i) {
                    const int32_t k = z0[c][i] - 1;
                    if (k < 0 || k >= K) return set_err(BMM_E_ARG, "initialK out of range: chain %d, observation %zu", c, i);
                    hz[(size_t)c * n + i] = k;
                    nk[k]++;
                    for (int d = 0; d < P; ++d) s[(size_t)k * P + d] += X[i + (size_t)d * n] & 1;
                }
            }
        }
        const double alpha0 = alpha == 0.0 ? 1.0 : alpha;
        // the data: validated and packed once, by the chain object every run uses, and shared by all chains
        bmm_chain* h = nullptr;
        rc = bmm_chain_create(&h, sampler, N, P, K, alpha, beta, gamma, a, b, 1, seed, device);
        if (rc) return rc;
        struct Guard { bmm_chain* c; ~Guard() { bmm_chain_destroy(c); } } guard{h};
        if (!h->bits) return set_err(BMM_E_UNSUPPORTED, "an ensemble reads the bit planes: not offered on the int32 layout");
        rc = bmm_chain_set_data_host(h, X);
        if (rc) return rc;
        if (f_pred) {  // the new rows: validated and packed as newdata= packs them (k_validate_binary, k_pack_bits)
            rc = bmm_chain_set_newdata_host(h, f->newdata, M);
            if (rc) return rc;
        }
        const EnsFoldPlan fp = ens_fold_plan(N, P, chains, M, f_loo);
        const bool keep = z_out != nullptr;
        const size_t zt = keep ? (size_t)chains * n * S : 0;
        const size_t need = (size_t)pl.state_bytes + (size_t)pl.row_bytes * S + zt * 4 + (size_t)fp.acc_bytes +
                            (f_loo && f->loo_trace ? (size_t)fp.loo_row_bytes * S : 0) + (f_pred && f->predictive_trace ? (size_t)fp.pred_row_bytes * S : 0);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b)
            return set_err(BMM_E_ARG, "ensemble: the state and the traces of %d chains need %zu bytes of device memory, %zu are free%s", chains,
                           need, free_b, keep ? " (the label trace is optional)" : "");
        DevBuf dz, dnk, ds, dal, dzt, dnkt, dtht, dalt;
        HIP_TRY(dz.alloc(hz.size() * 4));
        HIP_TRY(dnk.alloc(hnk.size() * 4));
        HIP_TRY(ds.alloc(hs.size() * 4));
        HIP_TRY(dal.alloc((size_t)chains * 8));
        if (keep) HIP_TRY(dzt.alloc(zt * 4));
        HIP_TRY(dnkt.alloc((size_t)chains * S * K * 4));
        HIP_TRY(dtht.alloc((size_t)chains * S * KP * 8));
        HIP_TRY(dalt.alloc((size_t)chains * S * 8));
        const std::vector<double> hal((size_t)chains, alpha0);
        hipStream_t st = h->stream;
        HIP_TRY(hipMemcpyAsync(dz.p, hz.data(), hz.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dnk.p, hnk.data(), hnk.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ds.p, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dal.p, hal.data(), hal.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // the host vectors are pageable
        EnsArgs g{};
        g.Xb = h->dXb; g.N = (int)N; g.P = P; g.K = K; g.Kc = pl.Kc; g.W = pl.W;
        g.chains = chains; g.cpw = pl.cpw; g.slice_bytes = (int)pl.slice;
        g.beta = beta; g.gamma = gamma; g.a = a; g.b = b; g.sample_alpha = alpha == 0.0; g.seed = seed;
        g.z = dz.as<int32_t>(); g.Nk = dnk.as<int32_t>(); g.S = ds.as<int32_t>(); g.alpha = dal.as<double>();
        g.rows = S; g.z_tr = keep ? dzt.as<int32_t>() : nullptr; g.nk_tr = dnkt.as<int32_t>();
        g.th_tr = dtht.as<double>(); g.al_tr = dalt.as<double>();
        void (*fn)(EnsArgs) = dp ? k_ens_sweep<true> : k_ens_sweep<false>;
        const size_t lds = (size_t)pl.slice * pl.cpw;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        // the folds: per chain the accumulators ([kLooAcc][N]; [2][M]), the outputs of the finish kernels, the traces
        DevBuf dlacc, dlout, dltr, dpacc, dpout, dptr;
        EnsFoldArgs gl{}, gp{};
        void (*lfn)(EnsFoldArgs) = dp ? k_ens_score<true, true> : k_ens_score<false, true>;
        void (*pfn)(EnsFoldArgs) = dp ? k_ens_score<true, false> : k_ens_score<false, false>;
        const size_t lout = n * kLooOut + 8;  // doubles per chain: k_loo_finish's rows, then k_loo_reduce's scalars
        if (f_loo || f_pred) {
            EnsFoldArgs base{};
            base.N = (int)N; base.P = P; base.K = K; base.Kc = pl.Kc; base.W = pl.W;
            base.chains = chains; base.cpw = pl.cpw; base.slice_bytes = (int)pl.slice;
            base.beta = beta; base.gamma = gamma;
            base.z = dz.as<int32_t>(); base.Nk = dnk.as<int32_t>(); base.S = ds.as<int32_t>(); base.alpha = dal.as<double>();
            base.rows = S;
            gl = base; gp = base;
        }
        if (f_loo) {
            HIP_TRY(dlacc.alloc((size_t)chains * kLooAcc * n * 8));
            HIP_TRY(dlout.alloc((size_t)chains * lout * 8));
            if (f->loo_trace) HIP_TRY(dltr.alloc((size_t)chains * S * n * 8));
            const int64_t nb = (N + 255) / 256;
            for (int c = 0; c < chains; ++c)
                hipLaunchKernelGGL(k_loo_reset, dim3((unsigned)nb), dim3(256), 0, st, N, dlacc.as<double>() + (size_t)c * kLooAcc * n);
            HIP_TRY(hipGetLastError());
            gl.Xb = h->dXb; gl.R = (int)N; gl.acc = dlacc.as<double>(); gl.trace = f->loo_trace ? dltr.as<double>() : nullptr;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(lfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if (f_pred) {
            const size_t m = (size_t)M;
            HIP_TRY(dpacc.alloc((size_t)chains * 2 * m * 8));
            HIP_TRY(dpout.alloc((size_t)chains * m * 8));
            if (f->predictive_trace) HIP_TRY(dptr.alloc((size_t)chains * S * m * 8));
            const int64_t nb = (M + 255) / 256;
            for (int c = 0; c < chains; ++c)
                hipLaunchKernelGGL(k_predict_reset, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, st, M,
                                   dpacc.as<double>() + (size_t)c * 2 * m, dpacc.as<double>() + (size_t)c * 2 * m + m);
            HIP_TRY(hipGetLastError());
            gp.Xb = h->dXnb; gp.R = (int)M; gp.acc = dpacc.as<double>(); gp.trace = f->predictive_trace ? dptr.as<double>() : nullptr;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        int folded = 0;
        for (int j = 1; j < nsamples; ++j) {
            g.sweep = (uint32_t)j;
            g.row = j >= burnin ? j - burnin : -1;
            for (int lo = 0; lo < (int)N; lo += ens_rows(P)) {
                g.lo = lo;
                g.hi = lo + ens_rows(P) < (int)N ? lo + ens_rows(P) : (int)N;
                hipLaunchKernelGGL(fn, dim3((unsigned)pl.groups), dim3((unsigned)pl.cpw * 64), lds, st, g);
            }
            if (g.row >= 0 && (f_loo || f_pred)) {  // a kept sweep: its state is scored behind the launch that ended it
                if (f_loo) {
                    gl.row = g.row; gl.n = folded;
                    hipLaunchKernelGGL(lfn, dim3((unsigned)pl.groups), dim3((unsigned)pl.cpw * 64), lds, st, gl);
                }
                if (f_pred) {
                    gp.row = g.row; gp.n = folded;
                    hipLaunchKernelGGL(pfn, dim3((unsigned)pl.groups), dim3((unsigned)pl.cpw * 64), lds, st, gp);
                }
                ++folded;
            }
            HIP_TRY(hipGetLastError());
        }
        if (folded > 0) {  // the outputs, chain by chain, by the kernels of the single-chain summaries
            const int64_t nbl = (N + 255) / 256, nbp = (M + 255) / 256;
            for (int c = 0; c < chains; ++c) {
                if (f_loo) {
                    double* const out = dlout.as<double>() + (size_t)c * lout;
                    hipLaunchKernelGGL(k_loo_finish, dim3((unsigned)(nbl < 4096 ? nbl : 4096)), dim3(256), 0, st, N, folded,
                                       dlacc.as<double>() + (size_t)c * kLooAcc * n, out);
                    hipLaunchKernelGGL(k_loo_reduce, dim3(1), dim3(1024), 0, st, N, out, out + n * kLooOut);
                }
                if (f_pred) {
                    const double* const ac = dpacc.as<double>() + (size_t)c * 2 * (size_t)M;
                    hipLaunchKernelGGL(k_predict_finish, dim3((unsigned)(nbp < 4096 ? nbp : 4096)), dim3(256), 0, st, M, pl.Kc, folded, ac,
                                       ac + (size_t)M, (const double*)nullptr, dpout.as<double>() + (size_t)c * (size_t)M, (double*)nullptr);
                }
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(st));
        if (f) {
            rc = ens_folds_out(*f, chains, N, M, S, burnin, folded, dlout.as<double>(), dltr.as<double>(), dpout.as<double>(), dptr.as<double>());
            if (rc) return rc;
        }
        // the traces: each chain's block is laid out as its caller's matrix is
        for (int c = 0; c < chains; ++c) {
            if (keep) HIP_TRY(hipMemcpy(z_out[c], dzt.as<int32_t>() + (size_t)c * n * S, n * S * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(nk_out[c], dnkt.as<int32_t>() + (size_t)c * S * K, (size_t)S * K * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(theta_out[c], dtht.as<double>() + (size_t)c * S * KP, (size_t)S * KP * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(alpha_out[c], dalt.as<double>() + (size_t)c * S, (size_t)S * 8, hipMemcpyDeviceToHost));
            if (burnin == 0) {  // row 0 is the start, as in run_counts_chain: z0 or NA, theta NaN or 0, the first alpha
                if (keep) for (size_t i = 0; i < n; ++i) z_out[c][i * S] = dp ? (int32_t)0x80000000 : z0[c][i];
                for (size_t q = 0; q < KP; ++q) theta_out[c][q] = dp ? 0.0 : std::nan("");
                alpha_out[c][0] = alpha0;
                std::memcpy(nk_out[c], hnk.data() + (size_t)c * K, (size_t)K * 4);
            }
        }
        HIP_TRY(hipMemcpy(hz.data(), dz.p, hz.size() * 4, hipMemcpyDeviceToHost));
        for (int c = 0; c < chains; ++c)
            for (size_t i = 0; i < n; ++i) {
                const int32_t v = hz[(size_t)c * n + i];
                z_last[c][i] = v < 0 ? (int32_t)0x80000000 : v + 1;
            }
        return BMM_OK;
    });
}

int bmm_ensemble_run(int sampler, const int32_t* X, int64_t N, int P, int chains, const int32_t* const* z0, int nsamples, int K,
                     double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed, int device,
                     int32_t* const* z_out, int32_t* const* nk_out, double* const* theta_out, double* const* alpha_out,
                     int32_t* const* z_last) {
    const RunOptions opts = take_run_options();
    return ens_run(opts, sampler, X, N, P, chains, z0, nsamples, K, alpha, beta, gamma, a, b, burnin, seed, device, z_out, nk_out,
                   theta_out, alpha_out, z_last, nullptr);
}

int bmm_ensemble_run_ex(int sampler, const int32_t* X, int64_t N, int P, int chains, const int32_t* const* z0, int nsamples, int K,
                        double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed, int device,
                        int32_t* const* z_out, int32_t* const* nk_out, double* const* theta_out, double* const* alpha_out,
                        int32_t* const* z_last, const bmm_ensemble_folds* folds) {
    const RunOptions opts = take_run_options();
    return ens_run(opts, sampler, X, N, P, chains, z0, nsamples, K, alpha, beta, gamma, a, b, burnin, seed, device, z_out, nk_out,
                   theta_out, alpha_out, z_last, folds);
}

int bmm_ensemble_fold_plan(int sampler, int64_t N, int P, int K, int chains, int64_t M, int loo, int64_t out[6]) {
    if (!out) return set_err(BMM_E_ARG, "null argument");
    EnsPlan pl;
    const int rc = ens_plan(sampler, N, P, K, chains, pl);
    if (rc) return rc;
    if (M < 0) return set_err(BMM_E_ARG, "M must be >= 0");
    const EnsFoldPlan fp = ens_fold_plan(N, P, chains, M, loo != 0);
    out[0] = pl.slice; out[1] = pl.cpw; out[2] = fp.acc_bytes; out[3] = fp.loo_row_bytes; out[4] = fp.pred_row_bytes;
    out[5] = fp.launches;
    return BMM_OK;
}

}  // extern "C"
