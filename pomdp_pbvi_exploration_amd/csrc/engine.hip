// Engine object behind include/pbvi_hip.h: device residency of the model tables,
// the alpha-vector set and the belief block, and the kernel sequence of one backup.
//
// Device layouts (T = float | double, S_pad = S rounded up to 32, zero padded):
//   model   : see ModelView in backup_kernels.h
//   alpha   : [V_cap][S_pad]   rows 0..V-1 the set, row V = column-wise max |alpha|
//             (the magnitude row that bounds sum_s b_s |Gamma_v,s| for the tie window)
//   beliefs : [B_pad][S_pad]   B_pad = B rounded up to 256 (zero rows)
//   Gamma   : [N_pad][S_pad]   row (a*O+o)*(V+1)+v, v = V being the magnitude row
//   scores  : [split_k][B_pad][N_pad] f32 partial slabs  (f64 engines: [B][N])
//   results : out_alpha [B][S], action [B], best_v [B][A][O], keep [B]
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "backup_kernels.h"
#include "split_bf16.h"
#include "state_policy_kernels.h"
#include "sweep_kernels.h"
#include "upper_kernels.h"

namespace pbvi {

static thread_local std::string g_err;
static int g_poison = -1;   // -1: read PBVI_POISON from the environment on first use
static bool poison_enabled() {
    if (g_poison < 0) g_poison = getenv("PBVI_POISON") != nullptr ? 1 : 0;
    return g_poison == 1;
}
void set_error(const std::string& msg) { g_err = msg; }

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
            (void)hipGetLastError();                                                         \
            return (_e == hipErrorOutOfMemory || _e == hipErrorMemoryAllocation) ? PBVI_ENOMEM : PBVI_ERUNTIME; \
        }                                                                                    \
    } while (0)

#define FAIL(code, msg)        \
    do {                       \
        set_error(msg);        \
        return (code);         \
    } while (0)

// Host-to-host copy of a result out of the pinned bounce buffer into the caller's (pageable) memory.  One thread moves
// ~12-15 GB/s into cold pages -- for the 24 MB of a belief walk or the 123 MB of an expanded alpha' matrix that, not the
// PCIe transfer (50 GB/s into pinned memory), was the time of the call -- so copies of a few MB and more are split over a
// small pool of worker threads that lives as long as the process (started on first use, parked on a condition variable;
// starting threads per call cost ~0.1 ms each, more than the solve loop's 6-8 MB copies gain).
class CopyPool {
public:
    static CopyPool& get() {
        static CopyPool* pool = new CopyPool();              // leaked on purpose: no destructor order to get wrong at exit
        return *pool;
    }
    void copy(void* dst, const void* src, size_t bytes) {
        constexpr size_t kMinPart = (size_t)2 << 20;
        const unsigned ways = (unsigned)std::min<size_t>(workers_.size() + 1, bytes / kMinPart);
        if (ways <= 1 || getpid() != pid_) {                 // (a forked child has the object but not its threads)
            std::memcpy(dst, src, bytes);
            return;
        }
        const size_t part = ((bytes / ways) + 4095) & ~(size_t)4095;
        unsigned posted = 0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (unsigned w = 1; w < ways; ++w) {
                const size_t o = (size_t)w * part;
                if (o >= bytes) break;
                tasks_.push_back(Task{static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, std::min(part, bytes - o)});
                ++posted;
            }
            pending_ += posted;
        }
        cv_.notify_all();
        std::memcpy(dst, src, std::min(part, bytes));
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
    }

private:
    struct Task {
        char* dst;
        const char* src;
        size_t n;
    };
    CopyPool() {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        unsigned n = getenv("PBVI_COPY_THREADS") ? (unsigned)std::max(1, atoi(getenv("PBVI_COPY_THREADS"))) : 4u;
        n = std::min(n, hw);
        for (unsigned i = 1; i < n; ++i) {
            workers_.emplace_back([this] { run(); });
            workers_.back().detach();
        }
    }
    void run() {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !tasks_.empty(); });
                t = tasks_.back();
                tasks_.pop_back();
            }
            std::memcpy(t.dst, t.src, t.n);
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    const pid_t pid_ = getpid();
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::vector<Task> tasks_;
    size_t pending_ = 0;
    std::vector<std::thread> workers_;
};
static void host_copy(void* dst, const void* src, size_t bytes) { CopyPool::get().copy(dst, src, bytes); }

// What one owner -- an engine, or a call with device buffers of its own -- holds on the device: the bytes (what the cap of
// pbvi_debug_alloc_limit is applied to) and the owning buffers, which enter the list when they are constructed.
struct DevBuf;
struct DevMem {
    int64_t bytes = 0;
    std::vector<DevBuf*> bufs;
    static inline std::atomic<int64_t> live{0};             // the same over the whole process (pbvi_debug_live_bytes)
};

// Memory that somebody else owns: a pointer and the bytes behind it, nothing to allocate, release or count.
struct DevView {
    void* p = nullptr;
    size_t cap = 0;
    template <typename U>
    U* as() const { return reinterpret_cast<U*>(p); }
};

// An owning device buffer, bound for life to the DevMem it is counted in.  Its lifetime class says what an engine's
// after_oom() does with it: MODEL buffers (the model tables and what is derived from them alone) stay, WORKING buffers are
// released.  A SCOPED buffer is a temporary outside the list; like every DevBuf it releases itself when it goes out of scope.
struct DevBuf : DevView {
    enum Life { MODEL, WORKING, SCOPED };
    DevMem& mem;
    const Life life;
    DevBuf(DevMem& m, Life l = WORKING) : mem(m), life(l) {
        if (l != SCOPED) m.bufs.push_back(this);
    }
    DevBuf(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // Deterministic out-of-memory for tests of the MemoryError contract (src/pomdp.py:2399-2401): an engine may hold at
    // most this many bytes of device buffers (pbvi_debug_alloc_limit / PBVI_ALLOC_LIMIT_MB; < 0 = no cap).
    static int64_t& limit_bytes() {
        static int64_t v = getenv("PBVI_ALLOC_LIMIT_MB") ? (int64_t)atoll(getenv("PBVI_ALLOC_LIMIT_MB")) << 20 : -1;
        return v;
    }
    static bool over_limit(int64_t held, size_t want) { return limit_bytes() >= 0 && held + (int64_t)want > limit_bytes(); }
    // Growth headroom (below) is for engines with memory to spare: under a cap only while the engine stays below 3/4 of it,
    // on the device only while four times the request is free -- an early buffer's spare half must not be what a later
    // buffer of the same call lacks.
    static bool headroom_ok(int64_t held, size_t want) {
        if (limit_bytes() >= 0) return held + (int64_t)want <= limit_bytes() / 4 * 3;
        if (want < ((size_t)256 << 20)) return true;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return fr / 4 >= want;
    }
    // grow-only; contents are NOT preserved on growth.  A buffer that grows again doubles (25 % if that fails): in a solve
    // loop the alpha set gains a few rows per backup, and re-allocating a multi-GB buffer (hipFree + hipMalloc,
    // both synchronising, hundreds of ms at 20 GB) on every call would dwarf the backup itself.
    int ensure(size_t bytes) {
        if (bytes <= cap) return PBVI_OK;
        const bool regrow = p != nullptr;
        release();
        if (regrow) {
            for (const size_t want : {bytes * 2, bytes + bytes / 4}) {     // HBM is plentiful; re-allocations are not
                if (!headroom_ok(mem.bytes, want)) continue;
                if (hipMalloc(&p, want) == hipSuccess) {
                    adopt(want);
                    return PBVI_OK;
                }
                (void)hipGetLastError();                 // no room for that much headroom: try less, then the exact size
                p = nullptr;
            }
        }
        if (over_limit(mem.bytes, bytes)) {
            set_error("device allocation of " + std::to_string(bytes) + " bytes refused: the engine holds " + std::to_string(mem.bytes) +
                      " bytes and its cap is " + std::to_string(limit_bytes()) + " (pbvi_debug_alloc_limit)");
            return PBVI_ENOMEM;
        }
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            set_error("hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
            return PBVI_ENOMEM;
        }
        adopt(bytes);
        return PBVI_OK;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            mem.bytes -= (int64_t)cap;
            DevMem::live -= (int64_t)cap;
        }
        p = nullptr;
        cap = 0;
    }
    // this buffer := the allocation of `o`, which is left empty (both are counted in the same DevMem)
    void take(DevBuf& o) {
        release();
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }

   private:
    // the fresh allocation at p is this buffer's
    void adopt(size_t bytes) {
        cap = bytes;
        mem.bytes += (int64_t)bytes;
        DevMem::live += (int64_t)bytes;
        // Debug: fill fresh allocations with 0xFF (NaN floats, -1 ints) so any read of memory the engine did
        // not write shows up in the parity tests instead of hiding behind zero-filled fresh pages.
        if (poison_enabled()) {   // null-stream memset does not order against the engine's non-blocking streams: fence it
            if (hipMemset(p, 0xFF, bytes) != hipSuccess) (void)hipGetLastError();
            (void)hipDeviceSynchronize();
        }
    }
};

// A page-locked host buffer that enters its owner's list when it is constructed (the owner frees the list's buffers in its
// teardown, naming `what` if that fails).
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    const char* const what;
    PinnedBuf(std::vector<PinnedBuf*>& owner, const char* w) : what(w) { owner.push_back(this); }
    PinnedBuf(const PinnedBuf&) = delete;
    // At least `bytes`.  A buffer that is too small is freed and allocated again with `want` >= bytes bytes: the contents are
    // lost, and the caller has made sure that no copy into or out of it is pending.  false: no memory (the buffer is empty).
    bool ensure(size_t bytes, size_t want) {
        if (bytes <= cap) return true;
        (void)release();
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return false;
        }
        cap = want;
        return true;
    }
    hipError_t release() {
        const hipError_t e = p ? hipHostFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    template <typename U>
    U* as() const { return reinterpret_cast<U*>(p); }
};

// The engine's page-locked words, written by copies and by k_publish and read by the host once the stream is idle: flags
// and counts that come back with a call's results (a stack variable would be written by the copy after an early error
// return had released it).  One word per use, so that calls that nest (the rollout's step loop runs backups) cannot meet.
struct PinnedWords {
    int bad_key;              // assemble_keys / assemble_rows_store: keys out of range
    int screen_overflow;      // fp64 engines: the screen's fp32 alpha copy holds an overflowed value (scr_flag_)
    int unused2[2];
    int early[3];             // run_fetch, e_cnt_: provisional keys, rows appended behind them, 1 = the slots overflowed
    int unused7;
    int provisional;          // run_fetch: the provisional row count, read in the middle of the pipeline
    int unused9;
    int survivors;            // rollout: the simulations that go on after the step
    int unused11[5];
    int counters[8];          // copy of counters_ (Counter)
    int deferred[2];          // what the refinement's per-entry pass deferred to the grid-wide passes
    int unused26[6];
};
static_assert(sizeof(PinnedWords) == 128 && offsetof(PinnedWords, screen_overflow) == 4 && offsetof(PinnedWords, early) == 16 &&
                  offsetof(PinnedWords, counters) == 64,
              "PinnedWords: the size, or one of the words k_publish writes, has changed");

// the slots of an engine's device counters (counters_, zeroed at the start of every backup)
enum Counter {
    CNT_QUEUE = 0,            // near-tie queue of the first-max (qcount)
    CNT_ACTION_QUEUE = 1,     // near-tie queue of the action stage (aqcount)
    CNT_VALUE_MAX_QUEUE = 2,  // value_max's near-tie queue
    CNT_UNIQUE = 3,           // distinct (a*, v*) keys (ucount)
    CNT_REFINE_CAND = 4,      // candidates the refinement looked at
    CNT_DEAD = 5,             // dead triples
    CNT_SLOTS = 8,
};

// out[s] = max_v |alpha[v][s]| (out zeroed by the caller).  Row chunks of 128 run as separate blocks and meet in an
// atomic max on the bit pattern (non-negative IEEE values order like unsigned integers): with one block per
// column strip the 5000 dependent loads of a grown alpha set made this latency-bound (0.6 ms at V = 4500).
// true iff ptr is device memory (hipMalloc'ed) rather than ordinary or pinned host memory
static bool is_device_pointer(const void* ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();                         // unregistered host memory
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}
// true iff ptr is page-locked host memory the DMA engines can write directly (hipHostMalloc / pbvi_host_alloc)
static bool is_pinned_host_pointer(const void* ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// How every result reaches the caller's memory, on the engine's main stream (DESIGN.md section 4 has the table).  Device
// memory: one device-to-device copy.  The caller's page-locked memory: the DMA writes it.  Pageable memory: the DMA writes
// the engine's pinned staging buffer (items at 256-byte alignment) and flush() moves them on with host_copy once the
// stream is idle -- a DMA never targets memory the driver has to register first.  Rows in another order than the caller's
// (perm) reach host memory of either kind through the staging buffer in one DMA; flush() puts them in order.
// ONE transaction is open at a time: begin() drops what was queued, add() / add_rows() queue, finish() synchronises the
// stream and completes the staged items.  An add after a failed add does nothing and returns the first error, which
// finish() returns without synchronising: a sequence needs no check per item.  reserve() flushes first (nothing staged
// may be lost when the buffer moves), so raw() hands out pinned memory with nothing staged in it (the belief walk's
// side-stream copies, the prunes' counts, the rollout's trajectories).  What the backup pipeline queues with its last
// read-back (decide) is still queued when backup_run returns: run_fetch completes it with flush(), the stream idle by then.
struct Delivery {
    struct Item {                 // deliver(): `bytes` of device memory `src` to `dst` (NULL: not wanted)
        void* dst;
        const void* src;
        size_t bytes;
    };
    hipStream_t stream = nullptr;
    explicit Delivery(std::vector<PinnedBuf*>& owner) : stage_(owner, "hipHostFree(stage)") {}

    void begin() {
        staged_.clear();
        used_ = 0;
        rc_ = PBVI_OK;
    }
    int add(void* dst, const void* src_dev, size_t bytes) { return add_rows(dst, src_dev, bytes, 1, bytes, nullptr); }
    // n_rows rows of row_bytes, src_ld bytes apart on the device, packed at dst; row i becomes row perm[i] (nullptr: i).
    // direct: the DMA targets a pageable destination too, as it always did for assemble_keys and fetch_exchange -- the two
    // entries where the staged route measured slower than that (profiles/delivery_refactor.md); nothing else asks for it.
    int add_rows(void* dst, const void* src_dev, size_t src_ld, size_t n_rows, size_t row_bytes, const int32_t* perm,
                 bool direct = false) {
        if (rc_ == PBVI_OK && dst != nullptr && n_rows * row_bytes > 0)
            rc_ = queue(static_cast<char*>(dst), static_cast<const char*>(src_dev), src_ld, n_rows, row_bytes, perm, direct);
        return rc_;
    }
    int finish() { return rc_ ? rc_ : flush(); }
    int deliver(std::initializer_list<Item> items) {
        begin();
        for (const Item& it : items) add(it.dst, it.src, it.bytes);
        return finish();
    }
    int flush() {
        HIPCHK(hipStreamSynchronize(stream));
        for (const Staged& it : staged_) {
            const char* from = stage_.as<char>() + it.off;
            if (!it.perm) {
                host_copy(it.dst, from, it.n_rows * it.row_bytes);
                continue;
            }
            for (size_t i = 0; i < it.n_rows; ++i)
                host_copy(it.dst + (size_t)it.perm[i] * it.row_bytes, from + i * it.row_bytes, it.row_bytes);
        }
        staged_.clear();
        used_ = 0;
        return PBVI_OK;
    }
    // the staging buffer holds at least `bytes` and nothing is staged in it
    int reserve(size_t bytes) {
        int rc = flush();
        if (rc) return rc;
        if (!stage_.ensure(bytes, std::max<size_t>(bytes * 2, (size_t)64 << 20))) FAIL(PBVI_ENOMEM, "pinned staging allocation failed");
        return PBVI_OK;
    }
    // ... as raw page-locked memory for the caller's own copies, done before the next transaction
    template <typename U>
    int raw(size_t bytes, U** p) {
        int rc = reserve(bytes);
        if (rc) return rc;
        *p = stage_.as<U>();
        return PBVI_OK;
    }

   private:
    struct Staged {
        char* dst;
        size_t off, n_rows, row_bytes;
        const int32_t* perm;      // the caller's array: alive until the flush
    };
    PinnedBuf stage_;
    std::vector<Staged> staged_;
    size_t used_ = 0;
    int rc_ = PBVI_OK;

    int queue(char* dst, const char* src, size_t src_ld, size_t n_rows, size_t row_bytes, const int32_t* perm, bool direct) {
        const size_t bytes = n_rows * row_bytes;
        const bool device = is_device_pointer(dst);
        if (device && perm) {     // rare (no caller in the package asks for a sorted block in device memory): row by row
            for (size_t i = 0; i < n_rows; ++i)
                HIPCHK(hipMemcpyAsync(dst + (size_t)perm[i] * row_bytes, src + i * src_ld, row_bytes, hipMemcpyDeviceToDevice, stream));
            return PBVI_OK;
        }
        const bool staged = !device && (perm || !(direct || is_pinned_host_pointer(dst)));
        char* to = dst;
        size_t off = 0;
        if (staged) {
            if ((used_ + 255) / 256 * 256 + bytes > stage_.cap) {
                int rc = reserve(bytes);
                if (rc) return rc;
            }
            off = (used_ + 255) / 256 * 256;
            to = stage_.as<char>() + off;
        }
        const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (src_ld == row_bytes)
            HIPCHK(hipMemcpyAsync(to, src, bytes, kind, stream));
        else
            HIPCHK(hipMemcpy2DAsync(to, row_bytes, src, src_ld, row_bytes, n_rows, kind, stream));
        if (staged) {
            staged_.push_back({dst, off, n_rows, row_bytes, perm});
            used_ = off + bytes;
        }
        return PBVI_OK;
    }
};

// keys of the unique rows of the last backup: key[u] = (a*, v*[a*, 0..O-1]) of the u-th distinct (a*, v*) pair
__global__ void k_gather_keys(int U, int A, int O, const int32_t* __restrict__ uniq, const int32_t* __restrict__ action,
                              const int32_t* __restrict__ best_v, int32_t* __restrict__ keys) {
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= U) return;
    const int b = uniq[u], a = action[b];
    keys[(int64_t)u * (1 + O)] = a;
    for (int o = 0; o < O; ++o) keys[(int64_t)u * (1 + O) + 1 + o] = best_v[((int64_t)b * A + a) * O + o];
}

// everything a rank contributes to the exchange, in one int32 buffer:
//   [0] U | [1, 1+B) index | [1+B, 1+2B) action | [1+2B, 1+3B) keep | [1+3B, 1+3B+B*(1+O)) keys of the U distinct rows (rest 0)
// `per` >= B is the common block size of a sharded run (ceil(B_total / ranks)): the message has per-sized sections so
// that every rank sends the same number of integers; entries of beliefs >= B are 0.
__global__ void k_pack_exchange(int B, int per, int U, int A, int O, const int32_t* __restrict__ inv, const int32_t* __restrict__ action,
                                const uint8_t* __restrict__ keep, const int32_t* __restrict__ uniq,
                                const int32_t* __restrict__ best_v, int32_t* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0) out[0] = U;
    if (c >= per) return;
    int32_t* k = out + 1 + 3 * (int64_t)per + (int64_t)c * (1 + O);
    if (c >= B) {
        out[1 + c] = 0;
        out[1 + per + c] = 0;
        out[1 + 2 * per + c] = 0;
        for (int o = 0; o <= O; ++o) k[o] = 0;
        return;
    }
    out[1 + c] = inv[c];
    out[1 + per + c] = action[c];
    out[1 + 2 * per + c] = keep[c];
    if (c < U) {
        const int b = uniq[c], a = action[b];
        k[0] = a;
        for (int o = 0; o < O; ++o) k[1 + o] = best_v[((int64_t)b * A + a) * O + o];
    } else {
        for (int o = 0; o <= O; ++o) k[o] = 0;
    }
}

// the inverse: per-row action / best-alpha arrays in the layout k_assemble reads (only the winning action's entries)
__global__ void k_scatter_keys(int n, int A, int O, int V, const int32_t* __restrict__ keys, int32_t* __restrict__ action,
                               int32_t* __restrict__ best_v, int* __restrict__ bad) {
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= n) return;
    const int a = keys[(int64_t)u * (1 + O)];
    if (a < 0 || a >= A) {
        atomicAdd(bad, 1);
        action[u] = 0;
        return;
    }
    action[u] = a;
    for (int o = 0; o < O; ++o) {
        const int v = keys[(int64_t)u * (1 + O) + 1 + o];
        if (v < 0 || v >= V) atomicAdd(bad, 1);
        best_v[((int64_t)u * A + a) * O + o] = (v < 0 || v >= V) ? 0 : v;
    }
}

template <typename T>
__global__ void k_col_absmax(const T* __restrict__ alpha, int lda, int V, int S_pad, T* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S_pad) return;
    const int v0 = blockIdx.y * 128, v1 = min(V, v0 + 128);
    T m[4] = {T(0), T(0), T(0), T(0)};
    for (int v = v0; v < v1; v += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const T x = (v + j < v1) ? alpha[(int64_t)(v + j) * lda + s] : T(0);
            const T ax = x < T(0) ? -x : x;
            m[j] = ax > m[j] ? ax : m[j];                    // NaN never wins, as before
        }
    }
    const T a = m[0] > m[1] ? m[0] : m[1], b = m[2] > m[3] ? m[2] : m[3];
    const T r = a > b ? a : b;
    if constexpr (sizeof(T) == 4)
        atomicMax(reinterpret_cast<unsigned int*>(out + s), __float_as_uint((float)r));
    else
        atomicMax(reinterpret_cast<unsigned long long*>(out + s), (unsigned long long)__double_as_longlong((double)r));
}

// Dense projection mode: D[ao][s][s'] = sum_{r: rs[s,a,r] = s'} RTO[s,a,o,r]  (one thread per row, no races)
template <typename T>
__global__ void k_densify(ModelView<T> mv, T* __restrict__ D, int64_t rows_pad) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int ao = blockIdx.y;
    if (s >= mv.S) return;
    const int a = ao / mv.O;
    T* row = D + ((int64_t)ao * rows_pad + s) * mv.S_pad;
    for (int r = 0; r < mv.R; ++r)
        row[mv.rs[((int64_t)a * mv.R + r) * mv.S_pad + s]] += mv.rto[((int64_t)ao * mv.R + r) * mv.S_pad + s];
}

// Gamma rows <- gamma * (alpha . D_ao^T) rows: product row v of batch ao goes to Gamma row ao*V+v.
template <typename T>
__global__ void k_scale_rows(const T* __restrict__ prod, int64_t batch_stride, int ld_prod, int V, T gamma,
                             T* __restrict__ gam, int ldg, int width) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int v = blockIdx.y, ao = blockIdx.z;
    if (s >= width) return;
    gam[((int64_t)ao * V + v) * ldg + s] = gamma * prod[(int64_t)ao * batch_stride + (int64_t)v * ld_prod + s];
}

// The A*O magnitude rows (tail of Gamma) from the ELL tables: one row each, not worth a GEMM tile row.
template <typename T>
__global__ void k_project_mag(const T* __restrict__ amax, ModelView<T> mv, T gamma, T* __restrict__ gam_tail, int ldg) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int ao = blockIdx.y;
    if (s >= mv.S_pad) return;
    const int a = ao / mv.O;
    T acc = T(0);
    for (int r = 0; r < mv.R; ++r)
        acc += mv.rto[((int64_t)ao * mv.R + r) * mv.S_pad + s] * amax[mv.rs[((int64_t)a * mv.R + r) * mv.S_pad + s]];
    gam_tail[(int64_t)ao * ldg + s] = gamma * acc;
}

// Indexing of a belief block (pbvi_beliefs_set / pbvi_beliefs_select), all on the device and stream-ordered -- a solve
// backs every new block up exactly once, so this is part of every backup:
//   k_row_flags  one pass over the source rows: flags[b][kt] = row b has mass in K tile kt (32 states), key[b] = its
//                first such tile
//   k_rank_sort  rows ordered by key (stable): the 256-row blocks of the score GEMM get tighter joint supports and more
//                zero tiles to skip (33.8 % -> 29.1 % of the tile steps at |S| = 30000)
//   k_gather_rows_v  the block in that order, 16 bytes per lane, straight from the store rows (no staging copy)
//   tile_or_block  the GEMM's zero map of the block from the row flags (the first rows of k_gather_rows_v's grid)
// The per-belief tile lists and the dead-triple test (backup_kernels.hip) read the same flags.
template <typename T>
__global__ void k_row_flags(const T* __restrict__ src, int ld, const int32_t* __restrict__ ids, int S_pad, int k_tiles,
                            uint8_t* __restrict__ flags, int32_t* __restrict__ key) {
    constexpr int NS = 16 / (int)sizeof(T);              // states per 16-byte chunk
    constexpr int LP = GEMM_BK / NS;                     // lanes per K tile (8 or 16)
    typedef T TN __attribute__((ext_vector_type(NS)));
    __shared__ int red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const T* row = src + (int64_t)(ids ? ids[b] : b) * ld;
    const int chunks = S_pad / NS;                       // rows are padded with zeros to S_pad (a multiple of 32)
    int first = 0x7fffffff;
    for (int c0 = 0; c0 < chunks; c0 += 1024) {          // four 16-byte loads per lane in flight
        TN v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 256 + tid;
            TN z;
#pragma unroll
            for (int e = 0; e < NS; ++e) z[e] = T(0);
            v[j] = c < chunks ? *(const TN*)(row + (int64_t)c * NS) : z;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 256 + tid;
            int f = 0;
#pragma unroll
            for (int e = 0; e < NS; ++e) f |= (v[j][e] != T(0)) ? 1 : 0;
#pragma unroll
            for (int off = 1; off < LP; off <<= 1) f |= __shfl_xor(f, off, 64);
            const int kt = c / LP;
            if (c < chunks && (tid & (LP - 1)) == 0) flags[(int64_t)b * k_tiles + kt] = (uint8_t)f;
            if (f && c < chunks && kt < first) first = kt;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(first, off, 64);
        first = o < first ? o : first;
    }
    if ((tid & 63) == 0) red[tid >> 6] = first;
    __syncthreads();
    if (tid == 0) {
        int m = red[0];
        for (int w = 1; w < 4; ++w) m = red[w] < m ? red[w] : m;
        key[b] = m == 0x7fffffff ? k_tiles : m;          // an empty row sorts behind every other
    }
}

// perm[rank of row i] = i, rank = rows with a smaller (key, index): a stable sort as a rank computation -- no atomics,
// deterministic.  One wave per row (64 lanes share the B comparisons), so 1024 rows keep every CU busy for ~3 us
// (one thread per row was 23 us on four CUs).
__global__ void k_rank_sort(const int32_t* __restrict__ key, int B, int32_t* __restrict__ perm) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int ki = key[i];
    int rank = 0;
    for (int j = lane; j < B; j += 64) {
        const int kj = key[j];
        rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rank += __shfl_xor(rank, off, 64);
    if (lane == 0) perm[rank] = i;
}

// dst row y = src row ids[perm[y]] (either map may be null), 16 bytes per lane; ld is a multiple of 32 elements
__device__ __forceinline__ void tile_or_block(const uint8_t* __restrict__ flags, const int32_t* __restrict__ perm, int B, int k_tiles,
                                              uint8_t* __restrict__ nz, int bx, int tile);
// plane != nullptr (fp32): the rows' split plane too (split_bf16.h), from the same registers
template <typename T>
__global__ void k_gather_rows_v(const T* __restrict__ src, T* __restrict__ dst, int ld, const int32_t* __restrict__ perm,
                                const int32_t* __restrict__ ids, const uint8_t* __restrict__ flags = nullptr, int B = 0,
                                int k_tiles = 0, uint8_t* __restrict__ nz = nullptr, int or_rows = 0,
                                uint32_t* __restrict__ plane = nullptr, int row0 = 0) {
    // The first or_rows rows of the grid build the block's zero map (they need the order only, like the
    // gather): as a kernel of its own in front of the gather it was 14 us on the path to the score GEMM.
    if ((int)blockIdx.y < or_rows) {
        if ((int)blockIdx.x * 64 < k_tiles) tile_or_block(flags, perm, B, k_tiles, nz, blockIdx.x, blockIdx.y);
        return;
    }
    constexpr int NS = 16 / (int)sizeof(T);
    typedef T TN __attribute__((ext_vector_type(NS)));
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c * NS >= ld) return;
    const int row = row0 + (int)blockIdx.y - or_rows;
    int r = row;
    if (perm) r = perm[r];
    if (ids) r = ids[r];
    const TN v = *(const TN*)(src + (int64_t)r * ld + (int64_t)c * NS);
    *(TN*)(dst + (int64_t)row * ld + (int64_t)c * NS) = v;
    if constexpr (NS == 4) {
        if (plane != nullptr) {                           // chunk c = states 4j .. 4j+3 of K tile c / 8, j = c & 7
            uint2 hi, lo;
            split_quad(v[0], v[1], v[2], v[3], hi, lo);
            uint32_t* pw = plane + (int64_t)row * ld + (c >> 3) * GEMM_BK + 2 * (c & 7);
            *(uint2*)pw = hi;
            *(uint2*)(pw + 16) = lo;
        }
    }
}

// The split plane (split_bf16.h) of n floats of rows whose length is a multiple of GEMM_BK, 16 bytes per lane
__global__ void k_split_plane(const float* __restrict__ x, uint32_t* __restrict__ plane, int64_t n) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c * 4 >= n) return;
    const float4 v = *(const float4*)(x + c * 4);
    uint2 hi, lo;
    split_quad(v.x, v.y, v.z, v.w, hi, lo);
    uint32_t* pw = plane + (c >> 3) * GEMM_BK + 2 * (c & 7);
    *(uint2*)pw = hi;
    *(uint2*)(pw + 16) = lo;
}

// nz[tile][kt] = OR of flags[perm[r]][kt] over the rows r of the 256-row tile (rows >= B are padding).  Block =
// 16 row slices x 16 words of 4 K tiles: 16 rows per thread, then an OR over the slices in LDS (one thread per K tile
// looping over 256 rows was a 76 us chain of dependent byte loads in front of the GEMM's tile lists).
__device__ __forceinline__ void tile_or_block(const uint8_t* __restrict__ flags, const int32_t* __restrict__ perm, int B, int k_tiles,
                                              uint8_t* __restrict__ nz, int bx, int tile) {
    __shared__ uint32_t part[16][17];
    const int cw = threadIdx.x & 15, rs = threadIdx.x >> 4;
    const int kt0 = (bx * 16 + cw) * 4;                          // this thread's 4 K tiles
    const int r1 = (tile + 1) * 256 < B ? (tile + 1) * 256 : B;
    uint32_t f = 0;
    if (kt0 < k_tiles) {
        const bool whole = kt0 + 4 <= k_tiles && (k_tiles & 3) == 0;   // aligned 4-byte loads
#pragma unroll 4
        for (int r = tile * 256 + rs; r < r1; r += 16) {
            const uint8_t* p = flags + (int64_t)(perm ? perm[r] : r) * k_tiles + kt0;
            if (whole) {
                f |= *(const uint32_t*)p;
            } else {
                for (int e = 0; e < 4 && kt0 + e < k_tiles; ++e) f |= (uint32_t)p[e] << (8 * e);
            }
        }
    }
    part[rs][cw] = f;
    __syncthreads();
    if (rs == 0 && kt0 < k_tiles) {
        for (int x = 1; x < 16; ++x) f |= part[x][cw];
        for (int e = 0; e < 4 && kt0 + e < k_tiles; ++e) nz[(int64_t)tile * k_tiles + kt0 + e] = ((f >> (8 * e)) & 0xffu) ? 1 : 0;
    }
}

template <typename T>
__global__ void k_gather_rows(const T* __restrict__ src, T* __restrict__ dst, int ld, const int32_t* __restrict__ perm) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ld) return;
    dst[(int64_t)blockIdx.y * ld + s] = src[(int64_t)perm[blockIdx.y] * ld + s];
}

// rows perm[y] of src (leading dimension ld_src) -> rows y of dst (ld_dst), first `cols` columns
template <typename T>
__global__ void k_gather_rows_ld(const T* __restrict__ src, int ld_src, T* __restrict__ dst, int ld_dst, int cols,
                                 const int32_t* __restrict__ perm) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= cols) return;
    dst[(int64_t)blockIdx.y * ld_dst + s] = src[(int64_t)perm[blockIdx.y] * ld_src + s];
}

// hash[r] = sum_i bits(row r, element i) * (2 i + 1)  (mod 2^64): the key the host's alpha-vector container hashes its
// rows by (mdp.py::_AlphaKey -- equality is still decided on the bytes).  Position-weighted: a solve's alpha-vectors are
// largely shifted copies of one another, which a plain sum of bit patterns cannot tell apart.
template <typename T>
__global__ void k_row_hash(const T* __restrict__ rows, int ld, int S, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[4];
    const T* p = rows + (int64_t)blockIdx.x * ld;
    unsigned long long acc = 0;
    for (int s = threadIdx.x; s < S; s += 256) {
        unsigned long long bits;
        if constexpr (sizeof(T) == 4)
            bits = (unsigned long long)__float_as_uint((float)p[s]);
        else
            bits = (unsigned long long)__double_as_longlong((double)p[s]);
        acc += bits * (2ull * (unsigned long long)s + 1ull);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// max_v score[row0 + b][v] for the B extra rows of the belief-side GEMM (the beliefs themselves multiplied by the alpha
// set: b . alpha_v), one wave per row; out[perm ? perm[b] : b]
template <typename T>
__global__ void k_extra_rowmax(SlabView<T> sv, int64_t row0, int B, int V, const int32_t* __restrict__ perm,
                               double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    T m = -std::numeric_limits<T>::infinity();
    for (int v = lane; v < V; v += 64) {
        const T sc = sv.at(row0 + b, v);
        m = sc > m ? sc : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if (lane == 0) out[perm ? perm[b] : b] = (double)m;
}

__global__ void k_unpermute(int B, int AO, const int32_t* __restrict__ perm, const int32_t* __restrict__ action,
                            const int32_t* __restrict__ best_v, int32_t* __restrict__ action_o, int32_t* __restrict__ best_o) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int d = perm[b];
    if (tid == 0) action_o[d] = action[b];
    for (int j = tid; j < AO; j += blockDim.x) best_o[(int64_t)d * AO + j] = best_v[(int64_t)b * AO + j];
}

// ---- early rows (pbvi_backup_run_fetch) ---------------------------------------------------------------------------- //
// The small results of a run_fetch step -- slot, index and action per belief, the call's counters -- stored straight into the
// caller's page-locked arrays and the engine's pinned flag words by one kernel: five D2H copies of 4 KB or less (one of them
// into pageable stack memory) cost the end of every step ~25 us of copy-engine round trips.
__global__ void k_publish(int B, const int32_t* __restrict__ slot, const int32_t* __restrict__ index, const int32_t* __restrict__ action,
                          int32_t* __restrict__ h_slot, int32_t* __restrict__ h_index, int32_t* __restrict__ h_action,
                          const int* __restrict__ counters /* 8 */, const int* __restrict__ e_cnt /* 3 */,
                          const int* __restrict__ scr_flag /* or nullptr */, PinnedWords* __restrict__ words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) {
        h_slot[i] = slot[i];
        h_index[i] = index[i];
        h_action[i] = action[i];
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) words->counters[threadIdx.x] = counters[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x >= 8 && threadIdx.x < 11) words->early[threadIdx.x - 8] = e_cnt[threadIdx.x - 8];
    if (blockIdx.x == 0 && threadIdx.x == 11 && scr_flag != nullptr) words->screen_overflow = scr_flag[0];
}

// One block per distinct key u of the FINAL result: is it among the provisional keys (whose rows are on their way to the
// host already)?  Yes: slot[u] = its provisional position.  No: the row gets the next free slot behind the provisional
// ones and this block copies it there.  cnt[0] = provisional keys, cnt[1] += new rows, cnt[2] = 1 on overflow of the slots.
template <typename T>
__global__ void k_match_rows(int AO, int O, const int* __restrict__ ucount, const int32_t* __restrict__ uniq, const int32_t* __restrict__ action,
                             const int32_t* __restrict__ best, const int32_t* __restrict__ uniq_p, const int32_t* __restrict__ action_p,
                             const int32_t* __restrict__ best_p, int* __restrict__ cnt, int cap_rows, int32_t* __restrict__ slot,
                             const T* __restrict__ rows_dev, T* __restrict__ rows_host, int64_t cols) {
    __shared__ int found_sh, slot_sh;
    const int n = *ucount;
    const int np = cnt[0];
    for (int u = blockIdx.x; u < n; u += gridDim.x) {
        const int b = uniq[u], a = action[b];
        const int32_t* key = best + ((int64_t)b * AO + (int64_t)a * O);
        __syncthreads();
        if (threadIdx.x == 0) found_sh = 0x7fffffff;
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += blockDim.x) {
            const int bp = uniq_p[p];
            bool eq = action_p[bp] == a;
            const int32_t* kp = best_p + ((int64_t)bp * AO + (int64_t)a * O);
            for (int o = 0; eq && o < O; ++o) eq = kp[o] == key[o];
            if (eq) atomicMin(&found_sh, p);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int sl = found_sh;
            if (sl == 0x7fffffff) {
                sl = np + atomicAdd(&cnt[1], 1);
                if (sl >= cap_rows) {
                    cnt[2] = 1;
                    sl = -1;
                }
                slot_sh = sl;
            } else {
                slot_sh = -2;                                // already on the host
            }
            slot[u] = sl;
        }
        __syncthreads();
        const int sl = slot_sh;
        if (sl >= 0) {
            const T* src = rows_dev + (int64_t)u * cols;
            T* dst = rows_host + (int64_t)sl * cols;
            for (int64_t i = threadIdx.x; i < cols; i += blockDim.x) dst[i] = src[i];
        }
    }
}

// Gamma tiled over the alpha set (pbvi_set_gamma_tiling): memory planning, pure host arithmetic (pbvi_gamma_tiling_plan).
// Upper bounds of what the scoring stage allocates for a chunk of Vc alpha rows -- a chunk is scored as the Gamma of a
// Vc-row alpha set, A*O*(Vc+1)+2A rows -- none of which depends on the device: the stream-K continuation tiles are counted
// for 512 blocks (the grid is one block per CU), the fp64 K parts at their 64 MiB ceiling (gemm_f64_split).
struct TilingPlan {
    int64_t chunk_rows = 0, n_chunks = 0, bytes = 0;
};
static int64_t tiling_chunk_bytes(int64_t S_pad, int64_t AO, int64_t A, int64_t B, bool f32, int64_t Vc) {
    const int64_t n = AO * (Vc + 1) + 2 * A, k_tiles = S_pad / GEMM_BK;
    if (f32) {
        const int64_t n_pad = round_up(n, GEMM_BN), m_pad = round_up(B, GEMM_BM), pairs = (m_pad / GEMM_BM) * (n_pad / GEMM_BN);
        return n_pad * S_pad * 4                              // Gamma rows
               + (m_pad * n_pad + (int64_t)512 * 256 * 256) * 4   // first slab + continuation tiles
               + pairs * (k_tiles + 4) * 4 + 4096             // tile lists, counts, stream-K workspace
               + AO * k_tiles;                                // need map
    }
    const int64_t pairs = ((B + 127) / 128) * ((n + 127) / 128 + 4);
    return n * S_pad * 8 + std::max<int64_t>((int64_t)64 << 20, B * n * 8) + pairs * (k_tiles + 35) * 4 + (k_tiles + 2) * 4 +
           AO * k_tiles;
}
static int64_t tiling_matrix_bytes(int64_t AO, int64_t A, int64_t V, int64_t B, bool f32) {
    return B * round_up(AO * (V + 1) + 2 * A, 4) * (f32 ? 4 : 8);
}
// want_rows 0: one chunk when the whole fits, else the fewest equal chunks that fit.  PBVI_OK, PBVI_EINVAL, PBVI_ENOMEM.
static int tiling_plan(int64_t S, int64_t A, int64_t O, int64_t V, int64_t B, bool f32, int64_t budget, int64_t want_rows,
                       TilingPlan* out) {
    if (S <= 0 || A <= 0 || O <= 0 || V <= 0 || B <= 0 || budget < 0 || want_rows < 0 || A * O > 0x7fffffff ||
        S > 0x7fffffff - GEMM_BK)
        return PBVI_EINVAL;
    const int64_t S_pad = round_up(S, GEMM_BK), AO = A * O;
    if ((double)AO * (double)(V + 1) + 2.0 * A > 2147483647.0) return PBVI_EINVAL;
    const int64_t matrix = tiling_matrix_bytes(AO, A, V, B, f32);
    auto bytes_of = [&](int64_t Vc) {
        return Vc >= V ? tiling_chunk_bytes(S_pad, AO, A, B, f32, V) : tiling_chunk_bytes(S_pad, AO, A, B, f32, Vc) + matrix;
    };
    int64_t Vc;
    if (want_rows > 0) {
        Vc = round_up(want_rows, 4);
    } else if (bytes_of(V) <= budget) {
        Vc = round_up(V, 4);
    } else {
        int64_t lo = 4, hi = round_up(V, 4) - 4;             // largest multiple of 4 below V that fits (bytes_of ascends there)
        if (hi < 4 || bytes_of(4) > budget) {
            out->chunk_rows = 4;
            out->n_chunks = (V + 3) / 4;
            out->bytes = bytes_of(4);
            return PBVI_ENOMEM;
        }
        while (lo < hi) {
            const int64_t mid = (lo / 4 + hi / 4 + 1) / 2 * 4;
            if (bytes_of(mid) <= budget) lo = mid;
            else hi = mid - 4;
        }
        const int64_t n = (V + lo - 1) / lo;
        Vc = round_up((V + n - 1) / n, 4);                   // equal chunks: never more rows than `lo`, same count
    }
    out->chunk_rows = Vc;
    out->n_chunks = (V + Vc - 1) / Vc;
    out->bytes = bytes_of(Vc);
    return out->bytes <= budget ? PBVI_OK : PBVI_ENOMEM;
}

// The scoring stage (K1, K2, first-max) runs on an engine or on an fp64 engine's fp32 screen (EngineT::stage_scores).
struct ScoreIO {                      // the pipeline buffers the stage writes / reads: owned by the engine that continues
    int32_t* best_v;
    double* best_score;
    double* err;
    int32_t* queue;                   // near-tie queue (nullptr: no windows, exact arithmetic)
    int* qcount;
    int32_t* hcand;                   // candidates of the queued rows, for the refinement (launch_argmax), or nullptr
    int32_t* hncand;
    const uint8_t* dead;              // exact dead-triple flags, or nullptr
    const double* prd;                // [B][A] b.ER in f64 for the belief-side formulation, or nullptr
    hipEvent_t join;                  // the side-stream work that produced dead / prd
    hipStream_t side;                 // where the GEMM's tile lists may be built, or nullptr
    hipEvent_t* ev;                   // ev[1] after the projection, ev[2] after the GEMM, ev[3] after the argmax
    bool stats;
    double tol_extra;                 // added to the relative tie window (input rounding of a screen)
    bool allow_split;                 // the scores may come from the split bf16 GEMM (not on an fp64 engine's screen)
};
template <typename TS>
struct ScoreStage {
    SlabView<TS> sv;
    GemmPlan plan;
    double tol_rel;
    const int* chain;
    int64_t rd_col0, extra_row0, f64_pairs;
    bool fused;                       // the GEMM generated its Gamma tiles itself (gemm.hip, scheduler 2b)
    int split;                        // 1: bf16 MFMAs on the three-term operand split (gemm.hip, scheduler 2d)
    int chunks;                       // alpha side: chunks Gamma was tiled into (1 = held whole or compact); 0 = belief side
};

// The buffers of one decision: per-belief actions and (a*, v*) keys -> caller order -> distinct keys -> their alpha' rows
// (EngineT::decision_tail).  An engine holds two: the backup's result, and run_fetch's provisional decision.
struct Decision {
    DevBuf act;                       // [B] action per belief, engine order
    DevBuf act_res, best_res;         // [B] actions / [B][A][O] best_v in caller order (a sorted block, or a snapshot)
    DevBuf rep, uniq, inv, slot;      // [B] key dedup: representative, distinct keys' beliefs, belief -> distinct key, hash slots
    DevBuf rows;                      // [distinct][S] the distinct keys' rows
    DevBuf& counts;                   // the count of distinct keys is word `word` of this buffer
    const int word;
    // actions / keys in caller order, where the tail left them (valid while the buffers are: nothing grows them inside a call)
    const int32_t *res_act = nullptr, *res_best = nullptr;
    Decision(DevMem& m, DevBuf& c, int w) : act(m), act_res(m), best_res(m), rep(m), uniq(m), inv(m), slot(m), rows(m), counts(c), word(w) {}
    int* count() const { return counts.as<int>() + word; }
    // for B beliefs with `pairs` keys and rows of row_bytes; caller_order: act_res / best_res will be written
    int ensure(int64_t B, int64_t pairs, size_t row_bytes, bool caller_order) {
        int rc;
        for (DevBuf* b : {&act, &rep, &uniq, &inv, &slot})
            if ((rc = b->ensure((size_t)B * sizeof(int32_t)))) return rc;
        if (caller_order && (rc = act_res.ensure((size_t)B * sizeof(int32_t)))) return rc;
        if (caller_order && (rc = best_res.ensure((size_t)pairs * sizeof(int32_t)))) return rc;
        return rows.ensure((size_t)B * row_bytes);
    }
};

// Where the step loop of the device-resident rollouts takes its action from (EngineT::rollout)
enum RolloutSource {
    ROLLOUT_VALUE_MAX = 0,            // alpha_actions[first argmax_v b.alpha_v]       (pbvi_rollout, lookahead 0)
    ROLLOUT_Q = 1,                    // first argmax_a Q(b, a)                        (pbvi_rollout, lookahead 1)
    ROLLOUT_INFOTAXIS = 2,            // first argmin_a of the expected successor entropy (pbvi_rollout_infotaxis)
    ROLLOUT_SPACE_AWARE = 3,          // first argmin_a of pbvi_space_aware's F, RolloutCall::objective (pbvi_rollout_space_aware)
    ROLLOUT_STATE_POLICY = 4,         // pbvi_state_policy's action under RolloutCall::rule (pbvi_rollout_state_policy)
};
// What the step loop has to know about a source; its stage is EngineT::rollout_stage.  A number that is no source reads as
// value-max until EngineT::rollout refuses it (`known`), which keeps the refusals before that one in their order.
struct RolloutSourceInfo {
    bool known;
    bool needs_alpha;                 // a resident alpha set and alpha_actions [V]
    bool needs_weights;               // pbvi_state_weights_set, and RolloutCall::objective 0 or 1
    bool needs_state_policy;          // pbvi_state_policy_set, and RolloutCall::rule 0, 1 or 2
    // The Bayes step sums the norm in block order, not with atomics: infotaxis (plain or space-aware) meets near-ties between
    // actions on symmetric beliefs, which must not hang on the arrival order of the atomics.  (A rollout against an environment
    // promises the same bits however a run is cut into blocks, and sums in block order whatever its source.)  The state
    // policies too: Thompson sampling reads the belief's bits, which must not depend on that order either.
    bool fixed_order;
    const char* who;                  // the entry point named in the refusals of what only this source needs
};
inline RolloutSourceInfo rollout_source_info(int source) {
    switch (source) {
        case ROLLOUT_VALUE_MAX: return {true, true, false, false, false, "rollout"};
        case ROLLOUT_Q: return {true, true, false, false, false, "rollout"};
        case ROLLOUT_INFOTAXIS: return {true, false, false, false, true, "rollout_infotaxis"};
        case ROLLOUT_SPACE_AWARE: return {true, false, true, false, true, "rollout_space_aware"};
        case ROLLOUT_STATE_POLICY: return {true, false, false, true, true, "rollout_state_policy"};
        default: return {false, true, false, false, false, "rollout"};
    }
}

// One rollout call, as pbvi_rollout / pbvi_rollout_infotaxis / pbvi_rollout_env / pbvi_rollout_space_aware /
// pbvi_rollout_state_policy fill it
struct RolloutCall {
    int source;                                // RolloutSource (anything else is refused)
    const int32_t* alpha_actions = nullptr;    // [V], read by ROLLOUT_VALUE_MAX
    double gamma = 0.0;                        // read by ROLLOUT_Q
    int objective = 0;                         // read by ROLLOUT_SPACE_AWARE: 0 space-aware, 1 expected weight
    int rule = 0;                              // read by ROLLOUT_STATE_POLICY: 0 MLS, 1 voting, 2 Thompson
    const int32_t* start_states;               // [B]
    const uint8_t* end_mask;                   // [S]
    uint64_t first_sim_id, seed;
    int64_t T;
    int32_t *out_states, *out_actions, *out_observations, *out_steps;   // [T+1][B], [T][B], [T][B], [B]; each may be NULL
    // pbvi_rollout_env: the observations come from the environment set with pbvi_env_set_*, and a simulation can be lost
    bool env = false;
    int end_observation = -1;                  // >= 0: the observation on landing in an end state
    const int64_t* shifts = nullptr;           // [B] first frame of each simulation, or NULL (frames only)
    uint8_t* out_lost = nullptr;               // [B] or NULL
};

// The resident belief block and what is derived from it.  `ver` names the rows the block holds: replaced() is the one
// place that moves it (an emptied block is a replaced one), and every derived datum is stamped with the version it
// describes (0: none).  New rows therefore make everything derived stale at once; nobody keeps a list of what to reset.
struct BeliefBlock {
    DevBuf rows;                      // [B_pad][S_pad] the beliefs in engine order; the pad rows are zero
    DevBuf keys, perm;                // [B] sort keys; caller's row of engine row i (sorted blocks)
    DevBuf rowflags;                  // [B][k_tiles] 1 = caller's belief row b has mass in K tile kt
    DevBuf nzA;                       // [B_pad / 256][k_tiles] zero map of the score GEMM's row blocks
    DevBuf plane;                     // fp32: the rows' split plane for the split score GEMM (split_bf16.h)
    DevBuf btl, btc;                  // [B][k_tiles], [B] per-belief non-zero tile lists and their lengths
    int64_t B = 0, B_pad = 0;
    bool sorted = false;              // the rows are reordered (more than one row block of the score GEMM)
    std::vector<int32_t> h_perm;      // the host's copy of perm, fetched on demand (EngineT::host_perm)
    hipEvent_t ev_nzA = nullptr;      // recorded behind the pass that stamped nzA_ver: nzA is complete
    uint64_t ver = 1;
    // rowflags, nzA + ev_nzA, plane, btl / btc, the engine's dead triples (dead_), h_perm
    uint64_t rowflags_ver = 0, nzA_ver = 0, plane_ver = 0, tiles_ver = 0, dead_ver = 0, host_perm_ver = 0;
    explicit BeliefBlock(DevMem& m) : rows(m), keys(m), perm(m), rowflags(m), nzA(m), plane(m), btl(m), btc(m) {}
    void replaced(int64_t b, int64_t b_pad, bool reordered) {
        B = b;
        B_pad = b_pad;
        sorted = reordered;
        ++ver;
    }
    void emptied() { replaced(0, 0, false); }
};

// The working alpha set.  `view` holds V data rows, the magnitude row (column-wise max |alpha|) and zero rows up to the next
// multiple of 256 + 256, inside one of two allocations:
//   buf   -- the set as uploaded (alpha_set / alpha_append: view at row 0), or the PRIMARY set selected from the alpha store,
//            laid out with `off` free rows in FRONT of it: the solve loop's next set is its new rows followed by the previous
//            set (ValueFunction.extend: new-then-old, and first-max ties go to the lower index, so the order is part of the
//            result) -- those rows are gathered into the free rows just before the view, which then starts k rows earlier;
//            nothing else moves, the magnitude row takes the maximum with the new rows.  (Re-gathering 10^4 rows per backup
//            was 0.1 s of a 300-expansion solve, the fp32 copy for the screen of an fp64 engine another 0.09 s.)
//   small -- a selection much smaller than the primary set (compute_change scores the rows an expansion added): gathered
//            here so that the primary set is still there for the next backup.
// `ver` names the rows the view holds; placed() is the one place that moves view, V and ver.  Where the view lies is `place`,
// and whether a selection can still extend the primary layout follows from it: NONE no set; PLAIN uploaded; PRIMARY row `off`
// of buf, `ids` name its rows; BESIDE in `small`, the primary layout waits in buf; the ORPHANs are the same two once the ids
// name nothing any more (the alpha store was reset; also what an fp32 screen holds of its engine's primary layout).
template <typename T>
struct AlphaSet {
    enum Place { NONE, PLAIN, PRIMARY, BESIDE, PRIMARY_ORPHAN, BESIDE_ORPHAN };
    DevBuf buf, small;
    DevView view;
    int64_t V = 0, ld = 0;            // data rows; elements per row (S_pad, set when the engine is initialised)
    uint64_t ver = 1;
    Place place = NONE;
    std::vector<int32_t> ids;         // store ids of the primary set, view order
    int64_t off = 0;                  // first data row of the primary set inside buf
    uint64_t layout_ver = 0;          // counts the fresh layouts of a selected set (an fp64 engine's screen mirrors them)
    explicit AlphaSet(DevMem& m) : buf(m), small(m) {}

    T* rows() const { return view.template as<T>(); }
    T* mag_row() const { return rows() + (size_t)V * ld; }
    size_t row_bytes() const { return (size_t)ld * sizeof(T); }
    static size_t rows_cap(int64_t v) { return (size_t)round_up(v + 1, GEMM_BN); }
    bool on_primary() const { return place == PRIMARY || place == PRIMARY_ORPHAN; }
    bool primary_alive() const { return place == PRIMARY || place == BESIDE; }
    // no rows are kept free in front of the view (true also of a primary layout whose free rows are used up)
    bool starts_allocation() const { return place == PLAIN || (on_primary() && off == 0); }

    // the set is now `v` rows from row `first` of its allocation (BESIDE: of `small`); a primary layout's `off` moves with it
    void placed(Place where, int64_t first, int64_t v) {
        const DevView& own = (where == BESIDE || where == BESIDE_ORPHAN) ? small : buf;
        const size_t skip = (size_t)first * row_bytes();
        place = where;
        if (on_primary()) off = first;
        view.p = static_cast<char*>(own.p) + skip;
        view.cap = own.cap - skip;
        V = v;
        ++ver;
    }
    // the allocations are gone (after_oom)
    void emptied() {
        view = DevView{};
        place = NONE;
        V = off = 0;
        ids.clear();
        ++ver;
    }
    // the ids of the primary layout name store rows that are gone; the view stays
    void primary_given_up() {
        ids.clear();
        if (place == PRIMARY) place = PRIMARY_ORPHAN;
        if (place == BESIDE) place = BESIDE_ORPHAN;
    }

    // What a selection of store rows `id[0, n)` does to the layout (prepend = false: always a fresh, plain one).  `rows` --
    // EXTEND: new rows in front of the primary set (0: the primary set again); FRESH: rows kept free in front.
    struct Selection {
        enum Kind { EXTEND, SMALL, FRESH } kind;
        int64_t rows;
    };
    Selection selection(const int32_t* id, int64_t n, bool prepend) const {
        const int64_t pv = (int64_t)ids.size();
        if (prepend && primary_alive()) {
            if (n >= pv && n - pv <= off && std::equal(ids.begin(), ids.end(), id + (n - pv))) return {Selection::EXTEND, n - pv};
            if (n <= 4096 && 4 * n <= pv) return {Selection::SMALL, 0};      // much smaller than the primary set: beside it
        }
        return {Selection::FRESH, prepend ? std::max<int64_t>(512, n / 2) : 0};
    }
    // the selection's ids enter the primary layout's record
    void selected(const Selection& s, const int32_t* id, int64_t n) {
        if (s.kind != Selection::SMALL) ids.assign(id, id + n);          // (an extension: the new ids in front of the old ones)
        if (s.kind == Selection::FRESH) ++layout_ver;
    }
};

class EngineBase {
   public:
    virtual ~EngineBase() {}
    virtual int alpha_set(const void* alpha, int64_t V) = 0;
    virtual int alpha_append(const void* alpha, int64_t n) = 0;
    virtual int64_t alpha_count() const = 0;
    virtual int beliefs_set(const void* bel, int64_t B) = 0;
    virtual int backup_run(double gamma, int flags, pbvi_stats_t* st) = 0;
    virtual int backup_fetch(void* out_alpha, int32_t* out_action, int32_t* out_best, uint8_t* out_keep) = 0;
    virtual int device_results(void** d_alpha, int32_t** d_action, uint8_t** d_keep) = 0;
    virtual int64_t unique_count() const = 0;
    virtual int fetch_unique(void* out_rows, int32_t* out_index) = 0;
    virtual int fetch_compact(void* out_rows, int32_t* out_index, int32_t* out_action, int32_t* out_best, uint8_t* out_keep) = 0;
    virtual int run_fetch(double gamma, int flags, pbvi_stats_t* st, void* out_rows, int64_t cap_rows, int32_t* out_slot,
                          int32_t* out_index, int32_t* out_action, int32_t* out_best, uint8_t* out_keep, int64_t* n_unique,
                          int64_t* n_slots) = 0;
    virtual int fetch_unique_keys(int32_t* out_keys) = 0;
    virtual int fetch_row_hashes(uint64_t* out) = 0;
    virtual int fetch_exchange(int32_t* out, int64_t per) = 0;
    virtual int assemble_keys(double gamma, int64_t n, const int32_t* keys, void* out_rows) = 0;
    virtual int64_t assemble_keys_store(double gamma, int64_t n, const int32_t* keys, void* out_rows) = 0;
    virtual int prune_dominated(uint8_t* keep) = 0;
    virtual int prune_dominated_masked(const uint8_t* is_new, uint8_t* keep) = 0;
    virtual int value_max(double* out_value, int32_t* out_index) = 0;
    virtual int value_max_store(int64_t n, double* out_value, int32_t* out_index) = 0;
    virtual int64_t store_count(int which) const = 0;
    virtual int set_tie_window(double rel) = 0;
    virtual int set_value_max_exact(int exact) = 0;
    virtual int alpha_layout(int64_t* free_rows, int64_t* layouts) = 0;
    virtual int set_formulation(int f) = 0;
    virtual int set_screen(int mode) = 0;
    virtual int set_score_split(int mode) = 0;
    virtual int set_gamma_tiling(int mode, int64_t chunk_rows) = 0;
    virtual int set_fused(int enable) = 0;
    virtual int64_t device_bytes() const = 0;
    virtual int64_t store_append(int which, const void* rows, int64_t n) = 0;
    virtual int64_t store_append_unique(const int32_t* unique_idx, int64_t n) = 0;
    virtual int store_select(int which, const int32_t* ids, int64_t n) = 0;
    virtual int store_reset(int which) = 0;
    virtual int after_oom() = 0;
    virtual int belief_update(const int32_t* act, const int32_t* obs, void* out) = 0;
    virtual int beliefs_advance(const int32_t* act, const int32_t* obs, const uint8_t* keep, int64_t* out_B) = 0;
    virtual int beliefs_fetch(void* out) = 0;
    virtual int set_rto_f64(const double* rto) = 0;
    virtual int64_t belief_walk(const double* b0, int64_t n, const int32_t* act, const int32_t* obs, const uint8_t* restart,
                                double* out) = 0;
    virtual int64_t beliefs_count() const = 0;
    virtual int walk_keys(int64_t n, uint64_t* out_keys) = 0;
    virtual int backup_value_max(double* out_value) = 0;
    virtual int q_values(double gamma, double* out_q, int32_t* out_action, int32_t* out_best) = 0;
    virtual int64_t debug_slabs(void* out, int64_t cap_bytes) = 0;
    virtual int debug_slabs_fill(int byte) = 0;
    virtual int debug_score_probe(int enable) = 0;
    virtual int debug_refine_counts(int64_t* out) = 0;
    virtual int debug_value_max_route(int64_t* out) = 0;
    virtual int debug_score_probe_fetch(int64_t* dims, double* scalars, double* score, double* mag, double* err,
                                        int32_t* best_v, double* best_score, int32_t* queue, uint8_t* dead, int32_t* perm) = 0;
    virtual int rollout(const RolloutCall& call) = 0;
    virtual int infotaxis(double* out_g, int32_t* out_action, double* out_p_obs, double* out_entropy) = 0;
    virtual int state_weights_set(const double* w) = 0;
    virtual int state_weights_clear() = 0;
    virtual int space_aware(int objective, double* out_f, int32_t* out_action, double* out_terms) = 0;
    virtual int state_policy_set(const int32_t* state_actions) = 0;
    virtual int state_policy_clear() = 0;
    virtual int state_policy(int rule, uint64_t seed, uint64_t first_sim_id, int64_t t, const double* uniforms,
                             int32_t* out_action, int32_t* out_state, double* out_votes) = 0;
    // the HSVI upper bound: the device point store, its sawtooth on the resident block, the bound-greedy action values
    virtual int upper_reset(const double* corner) = 0;
    virtual int upper_append(const double* points, const double* values, const double* gaps, int64_t n) = 0;
    virtual int64_t upper_count() const = 0;
    virtual int upper_bound(int64_t n_visible, int64_t n_hit, double* out_value, int32_t* out_point, int32_t* out_hit) = 0;
    virtual int upper_q(double gamma, int64_t n_visible, int64_t n_hit, double* out_q, int32_t* out_action, double* out_p_obs,
                        double* out_succ_value) = 0;
    // the observation source of rollout_env: recorded frames or another observation law (setting one replaces the other)
    virtual int env_set_frames(const uint8_t* frames, int64_t F, int64_t C, const int32_t* channel_of_action) = 0;
    virtual int env_set_table(const double* obs_prob) = 0;
    virtual int env_clear() = 0;
};

// Order of a score-probe capture among the captures of ALL engines of the process.  One counter, not one per element type:
// an fp64 engine compares its own captures with its fp32 screen's (debug_score_probe_fetch), and a counter kept as a static
// of the class template would be two counters -- the screen's ahead by every capture of every other fp32 engine, so that
// an older capture of the screen was handed out for a newer one of the engine itself.
inline uint64_t next_probe_seq() {
    static std::atomic<uint64_t> seq{0};
    return ++seq;
}

template <typename T>
class EngineT : public EngineBase {
   public:
    static constexpr bool kF32 = sizeof(T) == 4;

    int device_ = 0;
    hipStream_t stream_ = nullptr;
    int S_ = 0, A_ = 0, O_ = 0, R_ = 0, S_pad_ = 0, mode_ = 0;
    // What the engine owns, in front of every member that enters one of these lists when it is constructed: device
    // buffers (with the bytes they hold), page-locked host buffers, events.  The destructor walks all three.
    DevMem mem_;
    std::vector<PinnedBuf*> pinned_;
    std::vector<std::pair<hipEvent_t, const char*>> events_;
    // *e := a new event that the engine destroys in its teardown (nothing to do if *e exists already)
    hipError_t new_event(hipEvent_t* e, unsigned flags, const char* what) {
        if (*e) return hipSuccess;
        const hipError_t err = hipEventCreateWithFlags(e, flags);
        if (err == hipSuccess) events_.push_back({*e, what});
        return err;
    }
    // bytes this engine may still allocate: what its cap leaves, or what the device reports free
    int64_t room() const {
        if (DevBuf::limit_bytes() >= 0) return DevBuf::limit_bytes() - mem_.bytes;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            (void)hipGetLastError();
            return INT64_MAX;
        }
        return (int64_t)fr;
    }
    double tie_rel_user_ = -1.0;

    DevBuf rs_{mem_, DevBuf::MODEL}, rto_{mem_, DevBuf::MODEL}, er_{mem_, DevBuf::MODEL}, sup_{mem_, DevBuf::MODEL};
    AlphaSet<T> al_{mem_};                                   // the working alpha set, its placement and the primary layout's record
    BeliefBlock blk_{mem_};                                  // the resident belief block and what is derived from it
    DevBuf gam_{mem_}, slabs_{mem_}, best_v_{mem_}, best_score_{mem_}, err_{mem_}, dead_{mem_}, queue_{mem_}, hcand_{mem_}, hncand_{mem_}, counters_{mem_, DevBuf::MODEL}, rdot_{mem_}, aqueue_{mem_}, keep_{mem_};
    // the backup's decision: actions, the belief reordering undone (f32, B > 256), K6 key dedup; fin_.rows holds the unique rows
    Decision fin_{mem_, counters_, CNT_UNIQUE};
    DevBuf bv2_{mem_}, bs2_{mem_}, err2_{mem_}, queue2_{mem_}, prune_cnt_{mem_};
    // Gamma tiled over the alpha set (pbvi_set_gamma_tiling): 0 never, 1 when Gamma does not fit, 2 always; rows per chunk
    // (0 = planned); the full-width score matrix the chunks are folded into; the widest stream-K share size of the chunks'
    // GEMMs; events around each chunk's projection / GEMM / fold (statistics)
    int tiling_mode_ = 0;
    int64_t tiling_rows_ = 0;
    DevBuf scores_{mem_}, chain_max_{mem_, DevBuf::MODEL};
    std::vector<hipEvent_t> tile_ev_;
    int tile_ev_chunks_ = 0;
    DevBuf stage_{mem_};   // beliefs_set: the caller's rows, padded, in front of the reordering
    DevBuf out_full_{mem_};   // the per-belief alpha' matrix expanded from fin_.rows (ensure_full)
    DevBuf store_[2]{{mem_}, {mem_}}, ids_{mem_};   // device row stores: [0] alpha-vectors, [1] beliefs
    int64_t store_rows_[2] = {0, 0};
    DevBuf in_ptr_{mem_, DevBuf::MODEL}, in_src_{mem_, DevBuf::MODEL}, bu_act_{mem_}, bu_obs_{mem_}, bu_row_{mem_}, bu_unnorm_{mem_}, bu_mass_{mem_}, bu_out_{mem_}, walk64_{mem_}, rto64_{mem_, DevBuf::MODEL};   // batched belief update
    std::vector<int32_t> h_rs_;                                // host copy of rs [A][R][S_pad] for the lazy CSC build
    DevBuf val_exact_{mem_};   // exact action values
    DevBuf bp_{mem_}, nzP_{mem_}, pmag_{mem_}, prd_{mem_};   // belief-side formulation: projected beliefs, tile map, magnitudes, b.ER
    bool vmax_exact_ = true;                                // f32 engines: re-score value_max's maxima in fp64
    // belief store as a GEMM operand in place (value_max_store): zero maps and tile lists kept per store row, extended
    // as rows are appended
    DevBuf snz_{mem_}, sbtl_{mem_}, sbtc_{mem_};
    int64_t snz_rows_ = 0, sbt_rows_ = 0;
    int64_t walk_rows_ = 0;                                  // rows the last belief_walk left in walk64_
    DevBuf vmax_bk_{mem_};   // max_v b.alpha_v of the last backup's beliefs (belief-side GEMM's extra rows)
    bool have_bk_vmax_ = false;
    hipEvent_t walk_ev_[8] = {};                            // belief_walk: chain -> copy -> host hand-offs, per quarter
    Delivery out_{pinned_};   // every result's way to the caller's memory (owns the pinned staging buffer)
    DevBuf keys_tmp_{mem_}, keys_act_{mem_}, keys_best_{mem_}, keys_rows_{mem_};   // unique-row keys out / rows from keys in (multi-GPU exchange)
    DevBuf acand_{mem_};   // [B][A] action inside the window (k_action_select -> k_refine_action)
    DevBuf q_{mem_}, q_res_{mem_}, q_act_{mem_};   // pbvi_q_values: q [B][A] in engine order / caller order, its argmax [B]
    // pbvi_rollout: trajectories [T+1][n] states | [T][n] actions | [T][n] observations | [n] steps; the live simulations'
    // true states and trajectory rows (caller order, double-buffered across the done-filter), keep flags, the filter's
    // row map (+ 1 int: the survivor count), alpha_actions [V], end mask [S]
    DevBuf ro_traj_{mem_}, ro_state_[2]{{mem_}, {mem_}}, ro_orig_[2]{{mem_}, {mem_}}, ro_keep_{mem_}, ro_dst_{mem_}, ro_aact_{mem_}, ro_end_{mem_};
    int64_t zero_row_ = -1;                                  // first s * A + a whose RTO[s, a, :, :] sums to 0 (-1: none)
    // successor_scores (pbvi_infotaxis, pbvi_space_aware; one call's results are delivered before the next call starts, so the
    // objectives share the buffers): the x-blocks' partials [XB][B][A][O][2 or 3]; the score [B][A] (G or F), its first argmin
    // [B], the summed terms (P(o | b, a) [B][A][O], or (Z, N, D) [B][A][O][3]) and the beliefs' own entropies [B], the last four
    // in the caller's belief order
    DevBuf gs_part_{mem_}, gs_score_{mem_}, gs_act_{mem_}, gs_extra_{mem_}, gs_h_{mem_};
    // pbvi_state_weights_set: w [S] fp64 (a working buffer: after_oom() releases it and no weights are set)
    DevBuf sw_{mem_};
    bool sw_set_ = false;
    // pbvi_state_policy_set: state_actions [S] int32 (a working buffer: after_oom() releases it and no table is set);
    // pbvi_state_policy's results in caller order -- action [B], state [B], votes [B][A] --, Thompson's per-chunk sums
    // (P_c, m_c) [B][ceil(S/256)][2] and the uniforms a caller gave [B]
    DevBuf sp_table_{mem_}, sp_act_{mem_}, sp_state_{mem_}, sp_votes_{mem_}, sp_sums_{mem_}, sp_u_{mem_};
    bool sp_set_ = false;
    DevBuf bu_mpart_{mem_};   // bayes_push(fixed_order): the push blocks' partial masses [B][ceil(S/256)]
    // pbvi_upper_*: the point store of the HSVI upper bound -- CSR rows (ub_ptr_ int64 [P+1], ub_idx_ int32 / ub_val_ fp64 [entries]),
    // per point its entries, value and gap (ub_nnz_ int32, ub_v_ / ub_gap_ fp64 [P]), the corner values ub_c_ fp64 [S].  Working
    // buffers: after_oom() releases them and the store is empty with no corner set.
    DevBuf ub_ptr_{mem_}, ub_idx_{mem_}, ub_val_{mem_}, ub_nnz_{mem_}, ub_v_{mem_}, ub_gap_{mem_}, ub_c_{mem_};
    int64_t ub_count_ = 0, ub_entries_ = 0;
    bool ub_corner_ = false;
    // one sawtooth evaluation's scratch (UpperScratch) and pbvi_upper_bound's results [B], caller order
    DevBuf ub_v0_{mem_}, ub_bnnz_{mem_}, ub_pw_{mem_}, ub_pi_{mem_}, ub_ph_{mem_}, ub_rv_{mem_}, ub_rp_{mem_}, ub_rh_{mem_};
    // pbvi_upper_q: a chunk's un-normalised successors, block masses and successors; every successor's mass and value
    // [B][A][O], engine order; the results Q [B][A], its first argmax [B], p_obs and successor values [B][A][O], caller order
    DevBuf uq_unnorm_{mem_}, uq_mpart_{mem_}, uq_succ_{mem_}, uq_mass_{mem_}, uq_val_{mem_}, uq_q_{mem_}, uq_act_{mem_}, uq_pobs_{mem_}, uq_sval_{mem_};
    // pbvi_env_set_*: the observation source of pbvi_rollout_env.  Frames: env_frames_ uint8 [F][C][S] + env_chan_ int32 [A];
    // table: env_table_ fp64 [S][A][O].  Working buffers: after_oom() releases them and the engine has no environment again.
    enum EnvKind { ENV_NONE = 0, ENV_FRAMES = 1, ENV_TABLE = 2 };
    DevBuf env_frames_{mem_}, env_chan_{mem_}, env_table_{mem_};
    int env_kind_ = ENV_NONE;
    int64_t env_F_ = 0, env_C_ = 0;
    DevBuf env_shift_{mem_}, ro_lost_{mem_};   // pbvi_rollout_env: the call's shifts int64 [n] and lost flags uint8 [n]
    DevBuf rf_q2_{mem_}, rf_q2p_{mem_}, rf_q2d_{mem_};   // k_refine_split: entries / candidates, partial scores, arrival counters
    DevBuf rf_v_{mem_}, rf_slot_{mem_}, rf_sc_{mem_}, rf_entry_{mem_}, rf_n_{mem_}, rf_tiles_{mem_}, rf_ibv_{mem_}, rf_ibi_{mem_}, rf_cnt_{mem_}, rf_W_{mem_}, rf_Cx_{mem_}, rf_nzW_{mem_}, rf_klW_{mem_}, rf_kcW_{mem_};   // refinement work list
    int formulation_ = 0;                                   // 0 auto, 1 project alpha-vectors, 2 project beliefs
    int last_formulation_ = 1;
    int64_t f64_pairs_ = 0;                                 // tile pairs of the last fp64 MFMA GEMM (0: plain kernel)
    int f64_split_ = 1;                                     // its K parts
    // Test-only score probe (pbvi_debug_score_probe): the scoring stage of THIS engine (an fp64 engine's screen has its
    // own) copies what its argmax read and wrote into these buffers before any later stage touches them.
    bool probe_on_ = false;
    uint64_t probe_seq_ = 0;                                // order of the capture among all engines' captures; 0 = none
    DevBuf probe_score_{mem_}, probe_mag_{mem_}, probe_err_{mem_}, probe_bv_{mem_}, probe_bs_{mem_}, probe_queue_{mem_}, probe_dead_{mem_}, probe_words_{mem_};
    struct ProbeInfo {
        int64_t B = 0, G = 0, V = 0, f64_pairs = 0;
        int push = 0, split = 0, chunks = 0, f64_split = 1;
        bool has_chain = false;
        double tol_rel = 0.0, tol_extra = 0.0;
    } probe_info_;
    const int32_t* res_action_ = nullptr;                  // results in caller order
    const int32_t* res_best_ = nullptr;
    int64_t res_unique_ = 0;
    bool full_valid_ = false;
    std::vector<int32_t> h_bu_;                              // bayes_upload's host side: act | obs | row, engine order
    const void* gam_pad_ptr_ = nullptr;                      // Gamma buffer / row count whose pad rows are zero
    int64_t gam_pad_N_ = -1;
    DevBuf scr_flag_{mem_, DevBuf::MODEL};   // fp64 engines: 1 = the screen's fp32 alpha copy holds an overflowed value
    PinnedBuf ids_pin_{pinned_, "hipHostFree(ids)"};         // staging of the ids of a store selection
    PinnedBuf words_{pinned_, "hipHostFree(flag)"};          // one PinnedWords, allocated by init(): see words()
    struct RunFetchDst {                                     // run_fetch: the small per-belief results travel with the pipeline's
        int32_t *slot = nullptr, *index = nullptr, *action = nullptr, *best = nullptr;   // last read-back, not behind a second
        uint8_t* keep = nullptr;                                                         // synchronisation
        bool queued = false;
    };
    // early rows: what run_fetch hands to the pipeline (set before backup_run, taken back after it) and what the pipeline
    // tells run_fetch in return
    struct EarlyRows {
        void* rows = nullptr;                                // page-locked destination of the distinct rows (nullptr: no run_fetch)
        int64_t cap = 0;                                     // rows it has room for
        RunFetchDst dst;
        bool used = false;                                   // this call's provisional rows went (or are going) to `rows`
        bool dma_pending = false;                            // their copy waits for the provisional count
        hipEvent_t ev[2] = {nullptr, nullptr};               // the provisional decision / its rows' copy are complete
    } early_;
    // the provisional decision's buffers (fin_ is the final one's): action values, the slots k_match_rows gives the final
    // keys, the counts {provisional keys, rows appended behind them, 1 = the slots overflowed} (PinnedWords::early)
    DevBuf e_rdot_{mem_}, e_slot_{mem_}, e_cnt_{mem_, DevBuf::MODEL};
    Decision prov_{mem_, e_cnt_, 0};
    hipEvent_t ev_ids_ = nullptr;
    DevBuf nzBw_{mem_, DevBuf::MODEL};   // [A*O][ceil(k_tiles/64)] support tiles of RTO as bit words
    DevBuf nzB_{mem_, DevBuf::MODEL}, klist_{mem_}, kcount_{mem_}, nchunks_{mem_}, need_{mem_}, skws_{mem_};   // zero-tile bookkeeping of the f32 score GEMM
    DevBuf dense_{mem_, DevBuf::MODEL}, nzD_{mem_, DevBuf::MODEL}, nzAlpha_{mem_}, prod_{mem_}, klistD_{mem_}, kcountD_{mem_}, nchunksD_{mem_};   // dense projection mode
    int64_t rows_pad_s_ = 0, dense_pairs_ = 0;
    std::vector<int> h_kcountD_;
    PinnedBuf kc_pin_{pinned_, "hipHostFree(kcount)"};        // landing area of the score GEMM's list lengths (statistics)
    hipStream_t stream2_ = nullptr;                  // belief-only kernels run beside projection + GEMM
    hipStream_t stream3_ = nullptr;                  // the score GEMM's tile lists / stream-K plan: beside both (a few us of
                                                     // work that the GEMM waits for must not queue behind k_dead's 100 us)
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_lists_ = nullptr, ev_xr_[2] = {nullptr, nullptr};
    GemmPlan plan_ = {};
    int64_t slab_bytes_ = 0;                  // what the last score_gemm asked of slabs_ (debug_slabs)
    hipEvent_t ev_[9] = {};
    hipEvent_t ev_pg_[2] = {};                       // around the dense projection's GEMM kernel
    bool have_result_ = false, res_sorted_ = false;
    int64_t res_B_ = 0;
    int screen_mode_ = 1;                                    // fp64 engines: 0 never screen, 1 when the GEMM is large, 2 always
    int split_mode_ = 1;                                     // fp32 backup scores on the split bf16 GEMM: 0 never, 1 when large, 2 always
    bool split_supported_ = false;                           // fp32: the device keeps subnormal bf16 operands (probed at creation)
    int fuse_project_ = 1;                                   // fp32: Gamma tiles generated inside the score GEMM; 0 never, 1 = where it
                                                             // is faster (R = 1), 2 = also for R = 2..7 (measured slower)
    double irr_frac_ = 0.0;                                  // share of (action, K tile) with non-consecutive successors
    DevBuf irr_{mem_, DevBuf::MODEL};   // [A][k_tiles] 1 = a 4-state chunk of the K tile has non-consecutive successors
    DevBuf mat_{mem_}, vlist_{mem_};   // [n-tiles] 1 = projected (straddles groups / tail), 0 = generated
    DevBuf ctile_{mem_};   // [n-tiles] compact tile index of a projected tile (-1: generated)
    std::vector<int32_t> h_ctile_;
    int n_mat_ = 0;                                          // projected tiles = tiles of Gamma that exist in memory when fused
    bool gam_pad_compact_ = false;
    std::vector<uint8_t> h_mat_;
    std::vector<int> h_vlist_;
    int64_t mat_V_ = -1;
    int64_t dead_pairs_ = 0, dead_count_ = 0;
    int* rf_counts_ = nullptr;                               // PinnedWords::deferred of the current backup
    bool last_deferred_nothing_ = false;                     // (the first backup of an engine reads the counts mid-pipeline)
    RefineWork last_work_;                                   // the work list of the most recent refinement pass ...
    bool have_last_work_ = false;                            // ... if there was one (pbvi_debug_refine_counts)
    // what the most recent value_max_device did (pbvi_debug_value_max_route): route, column-tile width, K parts, rows,
    // alpha rows, tile pairs; [6] counts the runs since the engine was created
    int64_t vmax_route_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool owns_streams_ = true;                               // false: a screen running on its fp64 engine's streams
    EngineT<float>* screen_ = nullptr;                       // fp64 engines: the fp32 screen (see ensure_screen)
    std::vector<int32_t> h_reach_ref_;                       // fp64 engines: the tables in the reference's layout, kept
    std::vector<double> h_rto_ref_, h_er_ref_;               //   to build the screen on first use
    // fp64 engines, what the screen's copies reflect: al_.ver, the primary layout mirrored (0: none), its first row; blk_.ver
    struct { uint64_t ver = 0, layout_ver = 0; int64_t off = 0; } screen_alpha_seen_;
    uint64_t screen_bel_seen_ = 0;

    ~EngineT() override {
        (void)hipSetDevice(device_);
        if (screen_) {
            (void)hipStreamSynchronize(stream_);
            delete screen_;
            screen_ = nullptr;
        }
        // every call is checked only to name a failure when PBVI_DEBUG is set; the thread's sticky last-error is cleared at
        // the end either way, so that a later launch check does not report a stale error of this teardown
        static const bool dbg = getenv("PBVI_DEBUG") != nullptr;
        auto chk = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && dbg) fprintf(stderr, "[pbvi] engine teardown: %s: %s\n", what, hipGetErrorString(e));
        };
        for (DevBuf* b : mem_.bufs) b->release();
        for (PinnedBuf* b : pinned_) chk(b->release(), b->what);
        for (const auto& e : events_) chk(hipEventDestroy(e.first), e.second);
        if (owns_streams_) {
            if (stream3_) chk(hipStreamDestroy(stream3_), "hipStreamDestroy(3)");
            if (stream2_) chk(hipStreamDestroy(stream2_), "hipStreamDestroy(2)");
            if (stream_) chk(hipStreamDestroy(stream_), "hipStreamDestroy(1)");
        }
        chk(hipGetLastError(), "sticky error left by an earlier call");
    }

    ModelView<T> view() const {
        ModelView<T> mv;
        mv.S = S_;
        mv.S_pad = S_pad_;
        mv.A = A_;
        mv.O = O_;
        mv.R = R_;
        mv.rs = rs_.as<int32_t>();
        mv.rto = rto_.as<T>();
        mv.er = er_.as<T>();
        mv.sup = sup_.as<uint8_t>();
        return mv;
    }

    int init(int device, int S, int A, int O, int R, const int32_t* reach, const T* rto, const T* er, int mode,
             hipStream_t shared_main = nullptr, hipStream_t shared_side = nullptr, hipStream_t shared_lists = nullptr) {
        device_ = device;
        S_ = S;
        A_ = A;
        O_ = O;
        R_ = R;
        mode_ = mode;
        S_pad_ = (int)round_up(S, GEMM_BK);
        al_.ld = S_pad_;
        if (const char* f = getenv("PBVI_F64_SCREEN")) {      // initial setting (tests run the whole suite with the screen forced)
            const std::string v(f);
            screen_mode_ = (v == "off" || v == "0") ? 0 : (v == "always" || v == "2") ? 2 : 1;
        }
        if (const char* f = getenv("PBVI_SCORE_SPLIT")) {     // initial setting (tests run the whole suite with the split forced)
            const std::string v(f);
            split_mode_ = (v == "off" || v == "0") ? 0 : (v == "always" || v == "2") ? 2 : 1;
        }
        if (const char* f = getenv("PBVI_GAMMA_TILING")) {    // initial setting: off|auto|always[:rows]
            const std::string v(f), m = v.substr(0, v.find(':'));
            tiling_mode_ = (m == "always" || m == "2") ? 2 : (m == "auto" || m == "1") ? 1 : 0;
            tiling_rows_ = v.find(':') == std::string::npos ? 0 : std::max<int64_t>(0, atoll(v.c_str() + v.find(':') + 1));
        }
        if (const char* f = getenv("PBVI_FORMULATION")) {     // initial setting (tests run the whole suite both ways)
            const std::string v(f);
            formulation_ = (v == "alpha" || v == "1") ? 1 : (v == "belief" || v == "2") ? 2 : 0;
        }
        HIPCHK(hipSetDevice(device_));
        if constexpr (kF32) split_supported_ = gemm_split_supported(device_) != 0;
        if (shared_main != nullptr) {   // an fp32 screen lives on its fp64 engine's streams: one pipeline, one order
            stream_ = shared_main;
            stream2_ = shared_side;
            stream3_ = shared_lists;
            owns_streams_ = false;
        } else {
        HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        }
        out_.stream = stream_;
        if (owns_streams_) {   // The side stream gets its own priority class.  Streams of one class share a small pool of hardware
            // queues, assigned round-robin at creation: once a RCCL communicator has created its streams, two
            // normal-priority streams made afterwards can land on one queue and the side work no longer overlaps
            // the projection (measured: ms_project 0.35 -> 0.44 with an idle communicator in the process).
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            static const bool plain_side = getenv("PBVI_SIDE_STREAM_NORMAL") != nullptr;      // debug / A-B only
            if (hi < lo && !plain_side) {
                HIPCHK(hipStreamCreateWithPriority(&stream2_, hipStreamNonBlocking, hi));
                HIPCHK(hipStreamCreateWithPriority(&stream3_, hipStreamNonBlocking, hi));
            } else {
                HIPCHK(hipStreamCreateWithFlags(&stream2_, hipStreamNonBlocking));
                HIPCHK(hipStreamCreateWithFlags(&stream3_, hipStreamNonBlocking));
            }
        }
        if (!words_.ensure(sizeof(PinnedWords), sizeof(PinnedWords))) FAIL(PBVI_ENOMEM, "engine_create: pinned flag words");
        for (auto& e : ev_) HIPCHK(new_event(&e, hipEventDefault, "hipEventDestroy(ev)"));
        for (auto& e : ev_pg_) HIPCHK(new_event(&e, hipEventDefault, "hipEventDestroy(ev_pg)"));
        HIPCHK(new_event(&ev_fork_, hipEventDisableTiming, "hipEventDestroy(fork)"));
        HIPCHK(new_event(&ev_join_, hipEventDisableTiming, "hipEventDestroy(join)"));
        HIPCHK(new_event(&ev_lists_, hipEventDisableTiming, "hipEventDestroy(lists)"));
        for (auto& e : ev_xr_) HIPCHK(new_event(&e, hipEventDisableTiming, "hipEventDestroy(xr)"));

        // re-tile the reference's [S][A][R] / [S][A][O][R] / [S][A] tables to s-contiguous planes
        const size_t n_rs = (size_t)A * R * S_pad_, n_rto = (size_t)A * O * R * S_pad_, n_er = (size_t)A * S_pad_;
        std::vector<int32_t> h_rs;
        std::vector<T> h_rto, h_er;
        try {
            h_rs.assign(n_rs, 0);
            h_rto.assign(n_rto, T(0));
            h_er.assign(n_er, T(0));
        } catch (const std::bad_alloc&) {
            FAIL(PBVI_ENOMEM, "host allocation for table re-tiling failed");
        }
        for (int s = 0; s < S; ++s)
            for (int a = 0; a < A; ++a) {
                h_er[(size_t)a * S_pad_ + s] = er[(size_t)s * A + a];
                if (zero_row_ < 0) {   // a state-action pair nothing can follow: the simulator draw (rollout) refuses the model
                    double tot = 0.0;
                    for (int k = 0; k < O * R; ++k) tot += (double)rto[((size_t)s * A + a) * O * R + k];
                    if (!(tot > 0.0)) zero_row_ = (int64_t)s * A + a;
                }
                for (int r = 0; r < R; ++r) {
                    const int32_t t = reach[((size_t)s * A + a) * R + r];
                    if (t < 0 || t >= S) FAIL(PBVI_EINVAL, "reach_states entry out of range [0,S)");
                    h_rs[((size_t)a * R + r) * S_pad_ + s] = t;
                    for (int o = 0; o < O; ++o)
                        h_rto[(((size_t)a * O + o) * R + r) * S_pad_ + s] = rto[(((size_t)s * A + a) * O + o) * R + r];
                }
            }
        h_rs_ = h_rs;                                        // (the CSC build keeps the caller's successors)
        // Slots of weight zero for every observation -- the reference pads an (s, a) with fewer than R successors by
        // low-index states at probability 0 (src/mdp.py:308-335), and the pad states s >= S are such slots too --
        // contribute exactly 0 whichever state they name.  On the device they name the state that keeps their 4-state
        // chunk's successors consecutive, so that padded models keep the 16-byte alpha loads of the projection and the
        // fused score GEMM (gemm.hip) instead of falling to gathers.
        if (S >= 4)
            for (int a = 0; a < A; ++a)
                for (int r = 0; r < R; ++r) {
                    int32_t* row = h_rs.data() + ((size_t)a * R + r) * S_pad_;
                    for (int c = 0; c < S_pad_ / 4; ++c) {
                        bool wild[4];
                        int j0 = -1, n_wild = 0;
                        for (int j = 0; j < 4; ++j) {
                            const int s = c * 4 + j;
                            bool w = true;
                            for (int o = 0; o < O && w; ++o) w = h_rto[(((size_t)a * O + o) * R + r) * S_pad_ + s] == T(0);
                            wild[j] = w;
                            n_wild += w;
                            if (!w && j0 < 0) j0 = j;
                        }
                        if (n_wild == 0) continue;
                        const int64_t base = j0 >= 0 ? (int64_t)row[c * 4 + j0] - j0 : 0;
                        if (base < 0 || base + 3 >= S) continue;
                        bool ok = true;
                        for (int j = 0; j < 4 && ok; ++j) ok = wild[j] || row[c * 4 + j] == base + j;
                        if (!ok) continue;
                        for (int j = 0; j < 4; ++j)
                            if (wild[j]) row[c * 4 + j] = (int32_t)(base + j);
                    }
                }
        if constexpr (!kF32) {   // reference-layout copies for the fp32 screen (built on the first large backup)
            if (mode == PBVI_SPARSE && (size_t)S * A * O * R <= ((size_t)1 << 28)) {
                try {
                    h_reach_ref_.assign(reach, reach + (size_t)S * A * R);
                    h_rto_ref_.assign(rto, rto + (size_t)S * A * O * R);
                    h_er_ref_.assign(er, er + (size_t)S * A);
                } catch (const std::bad_alloc&) {
                    h_reach_ref_.clear();
                    h_rto_ref_.clear();
                    h_er_ref_.clear();
                }
            }
        }
        int rc;
        if ((rc = rs_.ensure(n_rs * sizeof(int32_t)))) return rc;
        if ((rc = rto_.ensure(n_rto * sizeof(T)))) return rc;
        if ((rc = er_.ensure(n_er * sizeof(T)))) return rc;
        if ((rc = sup_.ensure((size_t)A * O * S_pad_))) return rc;
        HIPCHK(hipMemcpyAsync(rs_.p, h_rs.data(), n_rs * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        HIPCHK(hipMemcpyAsync(rto_.p, h_rto.data(), n_rto * sizeof(T), hipMemcpyHostToDevice, stream_));
        HIPCHK(hipMemcpyAsync(er_.p, h_er.data(), n_er * sizeof(T), hipMemcpyHostToDevice, stream_));
        HIPCHK(launch_support<T>(view(), sup_.as<uint8_t>(), stream_));
        if ((rc = counters_.ensure(CNT_SLOTS * sizeof(int)))) return rc;
        {   // nzB[(a,o)][kt] = 1 iff RTO[:,a,o,:] has support inside K tile kt (32 states)
            const int k_tiles = S_pad_ / GEMM_BK;
            // ... plus one extra row [A*O] for the support of ER (the reward rows in Gamma's tail tile)
            std::vector<uint8_t> h_nz((size_t)(A * O + 1) * k_tiles, 0);
            for (int ao = 0; ao < A * O; ++ao)
                for (int r = 0; r < R; ++r)
                    for (int s = 0; s < S; ++s)
                        if (h_rto[((size_t)ao * R + r) * S_pad_ + s] != T(0)) h_nz[(size_t)ao * k_tiles + s / GEMM_BK] = 1;
            for (int a = 0; a < A; ++a)
                for (int s = 0; s < S; ++s)
                    if (h_er[(size_t)a * S_pad_ + s] != T(0)) h_nz[(size_t)A * O * k_tiles + s / GEMM_BK] = 1;
            if ((rc = nzB_.ensure(h_nz.size()))) return rc;
            HIPCHK(hipMemcpyAsync(nzB_.p, h_nz.data(), h_nz.size(), hipMemcpyHostToDevice, stream_));
            // the same supports as bit words (bit t of word w = K tile 64 w + t), for the dead-triple test
            const int kw = (k_tiles + 63) / 64;
            std::vector<unsigned long long> h_nzw((size_t)A * O * kw, 0ull);
            for (int ao = 0; ao < A * O; ++ao)
                for (int kt = 0; kt < k_tiles; ++kt)
                    if (h_nz[(size_t)ao * k_tiles + kt]) h_nzw[(size_t)ao * kw + kt / 64] |= 1ull << (kt & 63);
            if ((rc = nzBw_.ensure(h_nzw.size() * sizeof(unsigned long long)))) return rc;
            HIPCHK(hipMemcpyAsync(nzBw_.p, h_nzw.data(), h_nzw.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream_));
            std::vector<int32_t> h_irr;
            // For the fused score GEMM (gemm.hip, schedulers 2b / 2c): K tiles that hold a 4-state chunk whose successors
            // (for some r) are not 4 consecutive states.  R = 1: the kernel gathers those itself; R = 2..7: those Gamma tiles
            // are projected and read, so fusing only pays while they are few (grid edges: ~1 in 8 on the olfactory grids;
            // on a model without grid structure every tile is one and the projection kernel stays).
            if (kF32 && R <= 7 && mode == PBVI_SPARSE) {
                h_irr.assign((size_t)A * k_tiles, 0);
                size_t n_irr = 0;
                for (int a = 0; a < A; ++a)
                    for (int r = 0; r < R; ++r)
                        for (int c = 0; c < S_pad_ / 4; ++c) {
                            const int32_t* q = h_rs.data() + ((size_t)a * R + r) * S_pad_ + (size_t)c * 4;
                            int32_t& f = h_irr[(size_t)a * k_tiles + c / 8];
                            if (!f && (q[1] != q[0] + 1 || q[2] != q[0] + 2 || q[3] != q[0] + 3)) {
                                f = 1;
                                ++n_irr;
                            }
                        }
                const double max_irr = getenv("PBVI_FUSE_MAX_IRR") ? atof(getenv("PBVI_FUSE_MAX_IRR")) : 0.30;
                irr_frac_ = (double)n_irr / (double)h_irr.size();
                if (R == 1 || irr_frac_ <= max_irr) {
                    if ((rc = irr_.ensure(h_irr.size() * sizeof(int32_t)))) return rc;
                    HIPCHK(hipMemcpyAsync(irr_.p, h_irr.data(), h_irr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
                }
            }
            HIPCHK(hipStreamSynchronize(stream_));
        }
        if (mode_ == PBVI_DENSE) {   // D[ao] = dense |S| x |S| transition-observation matrices
            rows_pad_s_ = round_up(S, GEMM_BN);
            const size_t n = (size_t)A * O * rows_pad_s_ * S_pad_;
            if ((rc = dense_.ensure(n * sizeof(T)))) return rc;
            HIPCHK(hipMemsetAsync(dense_.p, 0, n * sizeof(T), stream_));
            hipLaunchKernelGGL(k_densify<T>, dim3((S + 255) / 256, A * O), dim3(256), 0, stream_, view(), dense_.as<T>(),
                               rows_pad_s_);
            HIPCHK(hipGetLastError());
            if (kF32) {
                const int k_tiles = S_pad_ / GEMM_BK;
                const size_t per = (size_t)(rows_pad_s_ / GEMM_BN) * k_tiles;
                if ((rc = nzD_.ensure((size_t)A * O * per))) return rc;
                for (int ao = 0; ao < A * O; ++ao)
                    HIPCHK(launch_tile_nonzero_f32((const float*)dense_.p + (size_t)ao * rows_pad_s_ * S_pad_, S_pad_,
                                                   (int)rows_pad_s_, k_tiles, nzD_.as<uint8_t>() + ao * per, stream_));
            }
            HIPCHK(hipStreamSynchronize(stream_));
        }
        HIPCHK(hipStreamSynchronize(stream_));
        return PBVI_OK;
    }

    // ---- alpha set ------------------------------------------------------- //
    // Every writer of the working set ends here, al_ placed() and the rows on their way in stream_.  The magnitude row catches
    // up with the new rows: all of the view's (grown == nullptr: zeroed, then their column maximum) or `n` at `grown` (merged
    // into it).  The caller's arrays have been read when this returns -- a screen's copy is installed in the middle of its
    // fp64 engine's backup, on the streams they share, and does not wait -- and no result of another set can be fetched.
    int alpha_installed(const T* grown = nullptr, int64_t n = 0) {
        if (!grown) {
            HIPCHK(hipMemsetAsync(al_.mag_row(), 0, al_.row_bytes(), stream_));
            grown = al_.rows();
            n = al_.V;
        }
        if (n > 0) {
            hipLaunchKernelGGL(k_col_absmax<T>, dim3((S_pad_ + 255) / 256, (unsigned)((n + 127) / 128)), dim3(256), 0, stream_,
                               grown, S_pad_, (int)n, S_pad_, al_.mag_row());
            HIPCHK(hipGetLastError());
        }
        if (owns_streams_) HIPCHK(hipStreamSynchronize(stream_));
        have_result_ = false;
        return PBVI_OK;
    }

    int alpha_set(const void* alpha, int64_t V) override {
        if (V <= 0 || alpha == nullptr) FAIL(PBVI_EINVAL, "alpha_set: need V > 0 and a non-null array");
        HIPCHK(hipSetDevice(device_));
        int rc = al_.buf.ensure(al_.rows_cap(V) * al_.row_bytes());
        if (rc) return rc;
        al_.placed(al_.PLAIN, 0, V);
        HIPCHK(hipMemsetAsync(al_.view.p, 0, al_.view.cap, stream_));
        HIPCHK(hipMemcpy2DAsync(al_.view.p, al_.row_bytes(), alpha, (size_t)S_ * sizeof(T), (size_t)S_ * sizeof(T), (size_t)V,
                                hipMemcpyHostToDevice, stream_));
        return alpha_installed();
    }

    int alpha_append(const void* alpha, int64_t n) override {
        if (n < 0 || (n > 0 && alpha == nullptr)) FAIL(PBVI_EINVAL, "alpha_append: bad arguments");
        if (n == 0) return PBVI_OK;
        HIPCHK(hipSetDevice(device_));
        const int64_t Vn = al_.V + n;
        const size_t need = al_.rows_cap(Vn) * al_.row_bytes();
        const bool plain = al_.starts_allocation();
        if (need > al_.view.cap || !plain) {   // grow (or move to a plain layout), preserving the resident rows
            // (the rows are copied from the view: it may start inside al_.buf or lie in al_.small)
            int rc = grow_keep(al_.buf, need, (size_t)al_.V * al_.row_bytes(), std::max(need, plain ? al_.buf.cap * 2 : need),
                               al_.view.p, true);
            if (rc) return rc;
        } else {
            // clear the old magnitude row's pad columns / content before it becomes a data row
            HIPCHK(hipMemsetAsync(al_.mag_row(), 0, al_.row_bytes(), stream_));
        }
        al_.placed(al_.PLAIN, 0, Vn);                         // (a primary layout is given up with it)
        HIPCHK(hipMemcpy2DAsync(al_.rows() + (size_t)(Vn - n) * S_pad_, al_.row_bytes(), alpha, (size_t)S_ * sizeof(T),
                                (size_t)S_ * sizeof(T), (size_t)n, hipMemcpyHostToDevice, stream_));
        return alpha_installed();
    }

    int64_t alpha_count() const override { return al_.V; }

    // Belief block from rows on the device -- `src` [.][S_pad], row b of the block = src row (src_ids ? src_ids[b] : b) --
    // reordered, padded to the GEMM's 256-row blocks, with its zero-tile map.  Stream-ordered, no host synchronisation:
    // the host's copy of the order (blk_.h_perm) is fetched when a host-side consumer asks for it (host_perm).
    int beliefs_finish(int64_t B, const T* src, const int32_t* src_ids) {
        const int64_t Bp = round_up(B, GEMM_BM);
        const int k_tiles = S_pad_ / GEMM_BK;
        int rc = blk_.rows.ensure((size_t)Bp * S_pad_ * sizeof(T));
        if (rc) return rc;
        if ((rc = blk_.rowflags.ensure((size_t)B * k_tiles))) return rc;
        if ((rc = blk_.keys.ensure((size_t)B * sizeof(int32_t)))) return rc;
        if ((rc = blk_.perm.ensure((size_t)B * sizeof(int32_t)))) return rc;
        if ((rc = blk_.nzA.ensure((size_t)(Bp / GEMM_BM) * k_tiles))) return rc;
        if (Bp > B) HIPCHK(hipMemsetAsync(blk_.rows.as<T>() + (size_t)B * S_pad_, 0, (size_t)(Bp - B) * S_pad_ * sizeof(T), stream_));
        // the split plane rides along with the gather once score_gemm has allocated it (the first split backup)
        uint32_t* plane = nullptr;
        if (kF32 && split_mode_ != 0 && split_supported_ && blk_.plane.cap >= (size_t)Bp * S_pad_ * sizeof(float)) {
            plane = blk_.plane.as<uint32_t>();
            if (Bp > B) HIPCHK(hipMemsetAsync(plane + (size_t)B * S_pad_, 0, (size_t)(Bp - B) * S_pad_ * sizeof(float), stream_));
        }
        static const bool no_sort = getenv("PBVI_NO_BELIEF_SORT") != nullptr;     // debug / A-B only
        const bool sorted = B > (kF32 ? GEMM_BM : 128) && !no_sort;     // more than one row block of the score GEMM
        hipLaunchKernelGGL(k_row_flags<T>, dim3((unsigned)B), dim3(256), 0, stream_, src, S_pad_, src_ids, S_pad_, k_tiles,
                           blk_.rowflags.as<uint8_t>(), blk_.keys.as<int32_t>());
        HIPCHK(hipGetLastError());
        const int32_t* perm = nullptr;
        if (sorted) {
            hipLaunchKernelGGL(k_rank_sort, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream_, blk_.keys.as<int32_t>(), (int)B,
                               blk_.perm.as<int32_t>());
            HIPCHK(hipGetLastError());
            perm = blk_.perm.as<int32_t>();
        }
        // the zero map (the first rows of the grid) and the rows in that order, one launch
        constexpr int NS = 16 / (int)sizeof(T);
        const int or_rows = (int)(Bp / GEMM_BM);
        // (grid.y is at most 65535: a block near the limit goes in two launches, the zero map with the first)
        for (int64_t r0 = 0, orr = or_rows; r0 < B; orr = 0) {
            const int64_t cnt = std::min<int64_t>(B - r0, 65535 - orr);
            hipLaunchKernelGGL(k_gather_rows_v<T>, dim3((S_pad_ / NS + 255) / 256, (unsigned)(cnt + orr)), dim3(256), 0, stream_, src,
                               blk_.rows.as<T>(), S_pad_, perm, src_ids, blk_.rowflags.as<uint8_t>(), (int)B, k_tiles, blk_.nzA.as<uint8_t>(), (int)orr,
                               plane, (int)r0);
            HIPCHK(hipGetLastError());
            r0 += cnt;
        }
        HIPCHK(new_event(&blk_.ev_nzA, hipEventDisableTiming, "hipEventDestroy(nzA)"));
        HIPCHK(hipEventRecord(blk_.ev_nzA, stream_));
        blk_.replaced(B, Bp, sorted);
        blk_.rowflags_ver = blk_.nzA_ver = blk_.ver;         // what this pass left beside the rows
        blk_.plane_ver = plane != nullptr ? blk_.ver : 0;
        have_result_ = false;
        return PBVI_OK;
    }

    PinnedWords& words() const { return *words_.as<PinnedWords>(); }

    // blk_.h_perm[i] = caller's index of engine row i (sorted blocks), for the host-side consumers of the order
    int host_perm() {
        if (!blk_.sorted || blk_.host_perm_ver == blk_.ver) return PBVI_OK;
        blk_.h_perm.resize((size_t)blk_.B);
        HIPCHK(hipMemcpyAsync(blk_.h_perm.data(), blk_.perm.p, (size_t)blk_.B * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        blk_.host_perm_ver = blk_.ver;
        return PBVI_OK;
    }
    // ... as Delivery::add_rows takes it, after host_perm(): nullptr where the rows lie in the caller's order already
    const int32_t* caller_order() const { return blk_.sorted ? blk_.h_perm.data() : nullptr; }

    int beliefs_set(const void* bel, int64_t B) override {
        if (B <= 0 || bel == nullptr) FAIL(PBVI_EINVAL, "beliefs_set: need B > 0 and a non-null array");
        if (B > 65535) FAIL(PBVI_EUNSUPPORTED, "beliefs_set: at most 65535 beliefs per block");
        HIPCHK(hipSetDevice(device_));
        int rc = stage_.ensure((size_t)B * S_pad_ * sizeof(T));
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(stage_.p, 0, (size_t)B * S_pad_ * sizeof(T), stream_));
        HIPCHK(hipMemcpy2DAsync(stage_.p, (size_t)S_pad_ * sizeof(T), bel, (size_t)S_ * sizeof(T), (size_t)S_ * sizeof(T),
                                (size_t)B, hipMemcpyHostToDevice, stream_));
        if ((rc = beliefs_finish(B, stage_.as<T>(), nullptr))) return rc;
        HIPCHK(hipStreamSynchronize(stream_));               // the caller's array is free again
        return PBVI_OK;
    }

    // ---- batched belief update ---------------------------------------------- //
    int build_inverse_lists() {
        if (in_ptr_.p) return PBVI_OK;
        // CSC of the padded-ELL transition structure per action: for every landing state s' the (s, r) pairs with
        // rs[s,a,r] == s', in ascending s*R+r order (the order np.bincount accumulates in, src/pomdp.py:406).
        std::vector<int32_t> ptr((size_t)A_ * (S_ + 1), 0), src((size_t)A_ * S_ * R_);
        for (int a = 0; a < A_; ++a) {
            int32_t* p = ptr.data() + (size_t)a * (S_ + 1);
            for (int s = 0; s < S_; ++s)
                for (int r = 0; r < R_; ++r) ++p[h_rs_[((size_t)a * R_ + r) * S_pad_ + s] + 1];
            for (int s = 0; s < S_; ++s) p[s + 1] += p[s];
            std::vector<int32_t> fill(p, p + S_);
            int32_t* q = src.data() + (size_t)a * S_ * R_;
            for (int s = 0; s < S_; ++s)
                for (int r = 0; r < R_; ++r) q[fill[h_rs_[((size_t)a * R_ + r) * S_pad_ + s]]++] = s * R_ + r;
        }
        int rc;
        if ((rc = in_ptr_.ensure(ptr.size() * sizeof(int32_t)))) return rc;
        if ((rc = in_src_.ensure(src.size() * sizeof(int32_t)))) return rc;
        HIPCHK(hipMemcpy(in_ptr_.p, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(in_src_.p, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return PBVI_OK;
    }

    // No belief block is resident (every simulation finished, or the engine starts over)
    void block_emptied() {
        blk_.emptied();
        have_result_ = false;
    }

    // The Bayes step's buffers for `rows` beliefs; fixed_order: also the partial masses of a norm summed in block order
    int bayes_ensure(int64_t rows, bool fixed_order) {
        int rc;
        if ((rc = bu_act_.ensure((size_t)rows * sizeof(int32_t)))) return rc;
        if ((rc = bu_obs_.ensure((size_t)rows * sizeof(int32_t)))) return rc;
        if ((rc = bu_row_.ensure((size_t)rows * sizeof(int32_t)))) return rc;
        if ((rc = bu_unnorm_.ensure((size_t)rows * S_ * sizeof(double)))) return rc;
        if ((rc = bu_mass_.ensure((size_t)rows * sizeof(double)))) return rc;
        if (fixed_order && (rc = bu_mpart_.ensure((size_t)rows * ((S_ + 255) / 256) * sizeof(double)))) return rc;
        return PBVI_OK;
    }

    // What belief_update and beliefs_advance refuse, in this order, and what both need before their first launch
    int bayes_begin(const std::string& who, const int32_t* act, const int32_t* obs, bool other_null) {
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, who + ": no belief block resident");
        if (!act || !obs || other_null) FAIL(PBVI_EINVAL, who + ": NULL argument");
        if ((int64_t)S_ * R_ > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, who + ": S*R exceeds int32");
        for (int64_t b = 0; b < blk_.B; ++b)
            if (act[b] < 0 || act[b] >= A_ || obs[b] < 0 || obs[b] >= O_) FAIL(PBVI_EINVAL, who + ": action / observation out of range");
        HIPCHK(hipSetDevice(device_));
        return build_inverse_lists();
    }

    // act / obs / row (row may be NULL) arrive in the caller's belief order and the resident block may be sorted: engine row i
    // holds the caller's row c.  Into bu_act_ / bu_obs_ / bu_row_ in engine order; h_bu_ is read until the stream is synchronised.
    int bayes_upload(const int32_t* act, const int32_t* obs, const int32_t* row) {
        int rc = bayes_ensure(blk_.B, false);
        if (rc || (rc = host_perm())) return rc;
        const size_t n = (size_t)blk_.B;
        h_bu_.resize(3 * n);
        for (size_t i = 0; i < n; ++i) {
            const size_t c = blk_.sorted ? (size_t)blk_.h_perm[i] : i;
            h_bu_[i] = act[c];
            h_bu_[n + i] = obs[c];
            h_bu_[2 * n + i] = row ? row[c] : (int32_t)i;
        }
        DevBuf* to[3] = {&bu_act_, &bu_obs_, &bu_row_};
        for (int k = 0; k < (row ? 3 : 2); ++k)
            HIPCHK(hipMemcpyAsync(to[k]->p, h_bu_.data() + k * n, n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        return PBVI_OK;
    }

    BayesStep<T> bayes_step(bool fixed_order) {
        BayesStep<T> bs{};
        bs.bel = blk_.rows.as<T>();
        bs.ldb = S_pad_;
        bs.B = (int)blk_.B;
        bs.in_ptr = in_ptr_.as<int32_t>();
        bs.in_src = in_src_.as<int32_t>();
        bs.act = bu_act_.as<int32_t>();
        bs.obs = bu_obs_.as<int32_t>();
        bs.unnorm = bu_unnorm_.as<double>();
        bs.mass = bu_mass_.as<double>();
        bs.mass_part = fixed_order ? bu_mpart_.as<double>() : nullptr;
        return bs;
    }

    // First half of the Bayes step on the resident block, from bu_act_ / bu_obs_ in ENGINE row order: the un-normalised rows and
    // their masses, of the rows with out_row[b] >= 0 (nullptr: all).  fixed_order: the norm is summed in block order instead of
    // with atomics on the zeroed masses.
    int bayes_push(const int32_t* out_row, bool fixed_order) {
        if (!fixed_order) HIPCHK(hipMemsetAsync(bu_mass_.p, 0, (size_t)blk_.B * sizeof(double), stream_));
        HIPCHK(launch_belief_push<T>(bayes_step(fixed_order), view(), out_row, stream_));
        return PBVI_OK;
    }

    // Second half: the rows with bu_row_[b] >= 0 normalised into row bu_row_[b] of the nb survivors (caller order), which
    // become the resident block.  The beliefs never leave the device.
    int bayes_norm_finish(int64_t nb, bool sync_before_finish) {
        int rc = stage_.ensure((size_t)nb * S_pad_ * sizeof(T));
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(stage_.p, 0, (size_t)nb * S_pad_ * sizeof(T), stream_));   // pad columns stay zero
        HIPCHK(launch_belief_norm<T>(bayes_step(false), S_, bu_row_.as<int32_t>(), stage_.as<T>(), S_pad_, stream_));
        if (sync_before_finish) HIPCHK(hipStreamSynchronize(stream_));
        return beliefs_finish(nb, stage_.as<T>(), nullptr);
    }

    // out[b] = Bayes update of the resident belief b with (act[b], obs[b]); out: [B][S] T, host or device
    int belief_update(const int32_t* act, const int32_t* obs, void* out) override {
        int rc = bayes_begin("belief_update", act, obs, !out);
        if (rc) return rc;
        if ((rc = bu_out_.ensure((size_t)blk_.B * S_ * sizeof(T)))) return rc;
        if ((rc = bayes_upload(act, obs, nullptr))) return rc;
        // computed in engine order into bu_out_, then gathered back into the caller's order
        if ((rc = bayes_push(nullptr, false))) return rc;
        HIPCHK(launch_belief_norm<T>(bayes_step(false), S_, nullptr, bu_out_.as<T>(), S_, stream_));
        out_.begin();
        out_.add_rows(out, bu_out_.p, (size_t)S_ * sizeof(T), (size_t)blk_.B, (size_t)S_ * sizeof(T), caller_order());
        return out_.finish();
    }

    // Simulator step on the resident block (src/pomdp.py:3305-3311 update, :3326-3329 done-filter): every belief is
    // updated with its own (a, o); rows with keep[b] == 0 are dropped and the survivors become the resident block,
    // in the caller's order.
    int beliefs_advance(const int32_t* act, const int32_t* obs, const uint8_t* keep, int64_t* out_B) override {
        int rc = bayes_begin("beliefs_advance", act, obs, false);
        if (rc) return rc;
        std::vector<int32_t> dst((size_t)blk_.B);           // caller row -> surviving row
        int64_t nb = 0;
        for (int64_t c = 0; c < blk_.B; ++c) dst[(size_t)c] = (!keep || keep[c]) ? (int32_t)nb++ : -1;
        if (out_B) *out_B = nb;
        if (nb == 0) {                                   // every simulation finished
            block_emptied();
            return PBVI_OK;
        }
        if ((rc = bayes_upload(act, obs, dst.data()))) return rc;
        return advance_resident(nb);
    }

    // The Bayes step + done-filter of beliefs_advance from bu_act_ / bu_obs_ / bu_row_ on the device (synchronises before the
    // new block is built: the upload's host side is free again)
    int advance_resident(int64_t nb) {
        int rc = bayes_push(bu_row_.as<int32_t>(), false);
        return rc ? rc : bayes_norm_finish(nb, true);
    }

    // The greedy successor policies' scores of the resident block -- SUCC_ENTROPY: pbvi_infotaxis' G; SUCC_SPACE_AWARE /
    // SUCC_EXPECTED_WEIGHT: pbvi_space_aware's F -- into gs_score_ / gs_act_ (/ gs_extra_ / gs_h_), caller order, left on the
    // device.  Reads the block, the model tables and, for the weighted objectives, the weights only.
    int successor_scores(int objective, bool want_extra, bool want_entropy) {
        const bool weighted = objective != SUCC_ENTROPY;
        const std::string who = weighted ? "space_aware" : "infotaxis";
        if (weighted && !sw_set_) FAIL(PBVI_EINVAL, who + ": no state weights set (call pbvi_state_weights_set)");
        if ((int64_t)S_ * R_ > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, who + ": S*R exceeds int32");
        int rc = build_inverse_lists();
        if (rc) return rc;
        // Exact sizes: a buffer that one objective sized and the other outgrows is allocated anew, not doubled (the headroom
        // of DevBuf::ensure is for buffers that grow call after call), so an engine that runs both holds what the larger needs.
        auto fit = [](DevBuf& buf, size_t bytes) {
            if (bytes > buf.cap) buf.release();
            return buf.ensure(bytes);
        };
        const size_t ba = (size_t)blk_.B * A_, terms = (size_t)succ_terms(objective);
        if ((rc = fit(gs_part_, (size_t)succ_entropy_xblocks(S_) * ba * O_ * terms * sizeof(double)))) return rc;
        if ((rc = fit(gs_score_, ba * sizeof(double)))) return rc;
        if ((rc = fit(gs_act_, (size_t)blk_.B * sizeof(int32_t)))) return rc;
        if (want_extra && (rc = fit(gs_extra_, extra_bytes(objective)))) return rc;
        if (want_entropy && (rc = fit(gs_h_, (size_t)blk_.B * sizeof(double)))) return rc;
        SuccScores<T> ss{};
        ss.bel = blk_.rows.as<T>();
        ss.ldb = S_pad_;
        ss.B = (int)blk_.B;
        ss.perm = blk_.sorted ? blk_.perm.as<int32_t>() : nullptr;
        ss.part = gs_part_.as<double>();
        ss.wgt = weighted ? sw_.as<double>() : nullptr;
        ss.objective = objective;
        ss.score_out = gs_score_.as<double>();
        ss.action_out = gs_act_.as<int32_t>();
        ss.extra_out = want_extra ? gs_extra_.as<double>() : nullptr;
        ss.entropy_out = want_entropy ? gs_h_.as<double>() : nullptr;
        HIPCHK(launch_successor_scores<T>(ss, view(), in_ptr_.as<int32_t>(), in_src_.as<int32_t>(), stream_));
        return PBVI_OK;
    }
    // gs_extra_ of the resident block: Z [B][A][O] for SUCC_ENTROPY, (Z, N, D) [B][A][O][3] for the weighted objectives
    size_t extra_bytes(int objective) const {
        return (size_t)blk_.B * A_ * O_ * (objective == SUCC_ENTROPY ? 1 : 3) * sizeof(double);
    }
    // successor_scores for a caller: the score and whichever of the other arrays are asked for (NULL: not computed)
    int successor_scores_deliver(int objective, double* out_score, int32_t* out_action, double* out_extra, double* out_entropy) {
        HIPCHK(hipSetDevice(device_));
        int rc = successor_scores(objective, out_extra != nullptr, out_entropy != nullptr);
        if (rc) return rc;
        return out_.deliver({{out_score, gs_score_.p, (size_t)blk_.B * A_ * sizeof(double)},
                             {out_action, gs_act_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {out_extra, gs_extra_.p, extra_bytes(objective)},
                             {out_entropy, gs_h_.p, (size_t)blk_.B * sizeof(double)}});
    }

    int infotaxis(double* out_g, int32_t* out_action, double* out_p_obs, double* out_entropy) override {
        if (!out_g) FAIL(PBVI_EINVAL, "infotaxis: NULL out_g");
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "infotaxis: no belief block resident (call pbvi_beliefs_set)");
        return successor_scores_deliver(SUCC_ENTROPY, out_g, out_action, out_p_obs, out_entropy);
    }

    // ---- space-aware infotaxis (pbvi_state_weights_set / _clear, pbvi_space_aware) ---- //
    int state_weights_set(const double* w) override {
        if (!w) FAIL(PBVI_EINVAL, "state_weights_set: NULL weights");
        for (int s = 0; s < S_; ++s)
            if (!std::isfinite(w[s]) || w[s] < 0.0)
                FAIL(PBVI_EINVAL, "state_weights_set: weight " + std::to_string(s) + " is negative or not finite");
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));               // a kernel of an earlier call may still read the old weights
        sw_set_ = false;
        int rc = sw_.ensure((size_t)S_ * sizeof(double));
        if (rc) return rc;
        HIPCHK(hipMemcpy(sw_.p, w, (size_t)S_ * sizeof(double), hipMemcpyHostToDevice));
        sw_set_ = true;
        return PBVI_OK;
    }
    int state_weights_clear() override {
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
        sw_.release();
        sw_set_ = false;
        return PBVI_OK;
    }

    int space_aware(int objective, double* out_f, int32_t* out_action, double* out_terms) override {
        if (!out_f) FAIL(PBVI_EINVAL, "space_aware: NULL out_f");
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "space_aware: no belief block resident (call pbvi_beliefs_set)");
        if (objective != SUCC_SPACE_AWARE && objective != SUCC_EXPECTED_WEIGHT)
            FAIL(PBVI_EINVAL, "space_aware: objective must be 0 (space-aware) or 1 (expected weight)");
        return successor_scores_deliver(objective, out_f, out_action, out_terms, nullptr);
    }

    // ---- state policies (pbvi_state_policy_set / _clear, pbvi_state_policy) ---- //
    int state_policy_set(const int32_t* state_actions) override {
        if (!state_actions) FAIL(PBVI_EINVAL, "state_policy_set: NULL state_actions");
        if (A_ > STATE_POLICY_MAX_A) FAIL(PBVI_EUNSUPPORTED, "state_policy_set: more than 256 actions");
        for (int s = 0; s < S_; ++s)
            if (state_actions[s] < 0 || state_actions[s] >= A_)
                FAIL(PBVI_EINVAL, "state_policy_set: state_actions[" + std::to_string(s) + "] is outside [0, A)");
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));               // a kernel of an earlier call may still read the old table
        sp_set_ = false;
        int rc = sp_table_.ensure((size_t)S_ * sizeof(int32_t));
        if (rc) return rc;
        HIPCHK(hipMemcpy(sp_table_.p, state_actions, (size_t)S_ * sizeof(int32_t), hipMemcpyHostToDevice));
        sp_set_ = true;
        return PBVI_OK;
    }
    int state_policy_clear() override {
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
        sp_table_.release();
        sp_set_ = false;
        return PBVI_OK;
    }

    // The state policy `rule` of the resident block into sp_act_ / sp_state_ (/ sp_votes_), caller order, left on the device.
    // Thompson's uniform: d_uniforms [B] (device, caller order), or hashed from (seed, first_sim_id + orig[c], t) -- orig
    // (device, caller row -> simulation row) nullptr: the caller row itself.  Reads the block and the table only.
    int state_policy_stage(int rule, const double* d_uniforms, uint64_t seed, uint64_t first_sim_id, const int32_t* orig, int64_t t) {
        int rc;
        if ((rc = sp_act_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if ((rc = sp_state_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if (rule == STATE_POLICY_VOTING && (rc = sp_votes_.ensure((size_t)blk_.B * A_ * sizeof(double)))) return rc;
        if (rule == STATE_POLICY_THOMPSON && (rc = sp_sums_.ensure((size_t)blk_.B * state_policy_chunks(S_) * 2 * sizeof(double)))) return rc;
        StatePolicy<T> sp{};
        sp.bel = blk_.rows.as<T>();
        sp.ldb = S_pad_;
        sp.B = (int)blk_.B;
        sp.S = S_;
        sp.A = A_;
        sp.perm = blk_.sorted ? blk_.perm.as<int32_t>() : nullptr;
        sp.table = sp_table_.as<int32_t>();
        sp.rule = rule;
        sp.uniforms = d_uniforms;
        sp.seed = seed;
        sp.first_id = first_sim_id;
        sp.orig = orig;
        sp.t = t;
        sp.chunk_sums = rule == STATE_POLICY_THOMPSON ? sp_sums_.as<double>() : nullptr;
        sp.action_out = sp_act_.as<int32_t>();
        sp.state_out = sp_state_.as<int32_t>();
        sp.votes_out = rule == STATE_POLICY_VOTING ? sp_votes_.as<double>() : nullptr;
        HIPCHK(launch_state_policy<T>(sp, stream_));
        return PBVI_OK;
    }

    int state_policy(int rule, uint64_t seed, uint64_t first_sim_id, int64_t t, const double* uniforms, int32_t* out_action,
                     int32_t* out_state, double* out_votes) override {
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "state_policy: no belief block resident (call pbvi_beliefs_set)");
        if (!sp_set_) FAIL(PBVI_EINVAL, "state_policy: no state policy set (call pbvi_state_policy_set)");
        if (rule != STATE_POLICY_MLS && rule != STATE_POLICY_VOTING && rule != STATE_POLICY_THOMPSON)
            FAIL(PBVI_EINVAL, "state_policy: rule must be 0 (most likely state), 1 (voting) or 2 (Thompson)");
        if (!out_action) FAIL(PBVI_EINVAL, "state_policy: NULL out_action");
        if (uniforms && rule != STATE_POLICY_THOMPSON) FAIL(PBVI_EINVAL, "state_policy: uniforms belong to rule 2 (Thompson)");
        for (int64_t b = 0; uniforms && b < blk_.B; ++b)
            if (!(uniforms[b] >= 0.0 && uniforms[b] <= 1.0))
                FAIL(PBVI_EINVAL, "state_policy: uniforms[" + std::to_string(b) + "] is outside [0, 1]");
        if (t < 0 || t >= (1ll << 31)) FAIL(PBVI_EINVAL, "state_policy: t must be in [0, 2^31)");
        HIPCHK(hipSetDevice(device_));
        int rc;
        if (uniforms) {
            if ((rc = sp_u_.ensure((size_t)blk_.B * sizeof(double)))) return rc;
            HIPCHK(hipMemcpyAsync(sp_u_.p, uniforms, (size_t)blk_.B * sizeof(double), hipMemcpyHostToDevice, stream_));
        }
        if ((rc = state_policy_stage(rule, uniforms ? sp_u_.as<double>() : nullptr, seed, first_sim_id, nullptr, t))) return rc;
        const bool votes = rule == STATE_POLICY_VOTING;       // (out_votes is rule 1's: the other rules leave it alone)
        return out_.deliver({{out_action, sp_act_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {out_state, sp_state_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {votes ? out_votes : nullptr, sp_votes_.p, (size_t)blk_.B * A_ * sizeof(double)}});
    }

    // ---- HSVI upper bound (pbvi_upper_reset / _append / _count / _bound / _q) ---- //
    int upper_reset(const double* corner) override {
        if (!corner) FAIL(PBVI_EINVAL, "upper_reset: NULL corner values");
        for (int s = 0; s < S_; ++s)
            if (!std::isfinite(corner[s])) FAIL(PBVI_EINVAL, "upper_reset: corner value " + std::to_string(s) + " is not finite");
        HIPCHK(hipSetDevice(device_));
        ub_count_ = ub_entries_ = 0;
        ub_corner_ = false;
        int rc = ub_c_.ensure((size_t)S_ * sizeof(double));
        if (rc) return rc;
        HIPCHK(hipMemcpy(ub_c_.p, corner, (size_t)S_ * sizeof(double), hipMemcpyHostToDevice));
        ub_corner_ = true;
        return PBVI_OK;
    }

    int64_t upper_count() const override { return ub_count_; }

    // n points behind the store's: their non-zeros in ascending state order, found on the host (a point is a belief: every
    // entry finite and >= 0, at least one > 0)
    int upper_append(const double* points, const double* values, const double* gaps, int64_t n) override {
        if (!ub_corner_) FAIL(PBVI_EINVAL, "upper_append: no corner values set (call pbvi_upper_reset)");
        if (n < 0 || (n > 0 && (!points || !values || !gaps))) FAIL(PBVI_EINVAL, "upper_append: NULL argument");
        if (n == 0) return PBVI_OK;
        if (ub_count_ + n > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "upper_append: more than 2^31 - 1 points");
        std::vector<int64_t> ptr((size_t)n + 1);
        std::vector<int32_t> idx, nnz((size_t)n);
        std::vector<double> val;
        ptr[0] = ub_entries_;
        for (int64_t i = 0; i < n; ++i) {
            const double* row = points + (size_t)i * S_;
            int32_t cnt = 0;
            for (int s = 0; s < S_; ++s) {
                const double x = row[s];
                if (!(x >= 0.0) || !std::isfinite(x))
                    FAIL(PBVI_EINVAL, "upper_append: point " + std::to_string(i) + " has a negative or non-finite entry at state " +
                                          std::to_string(s));
                if (x > 0.0) {
                    idx.push_back(s);
                    val.push_back(x);
                    ++cnt;
                }
            }
            if (cnt == 0) FAIL(PBVI_EINVAL, "upper_append: point " + std::to_string(i) + " is all zeros");
            if (std::isnan(values[i]) || std::isnan(gaps[i])) FAIL(PBVI_EINVAL, "upper_append: NaN value or gap");
            nnz[(size_t)i] = cnt;
            ptr[(size_t)i + 1] = ptr[(size_t)i] + cnt;
        }
        HIPCHK(hipSetDevice(device_));
        const size_t P = (size_t)ub_count_, E = (size_t)ub_entries_, ne = idx.size(), un = (size_t)n;
        int rc;
        if ((rc = grow_keep(ub_ptr_, (P + un + 1) * sizeof(int64_t), P ? (P + 1) * sizeof(int64_t) : 0))) return rc;
        if ((rc = grow_keep(ub_idx_, (E + ne) * sizeof(int32_t), E * sizeof(int32_t)))) return rc;
        if ((rc = grow_keep(ub_val_, (E + ne) * sizeof(double), E * sizeof(double)))) return rc;
        if ((rc = grow_keep(ub_nnz_, (P + un) * sizeof(int32_t), P * sizeof(int32_t)))) return rc;
        if ((rc = grow_keep(ub_v_, (P + un) * sizeof(double), P * sizeof(double)))) return rc;
        if ((rc = grow_keep(ub_gap_, (P + un) * sizeof(double), P * sizeof(double)))) return rc;
        HIPCHK(hipStreamSynchronize(stream_));               // (no earlier kernel still reads the store)
        HIPCHK(hipMemcpy(ub_ptr_.as<int64_t>() + P, ptr.data(), (un + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ub_idx_.as<int32_t>() + E, idx.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ub_val_.as<double>() + E, val.data(), ne * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ub_nnz_.as<int32_t>() + P, nnz.data(), un * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ub_v_.as<double>() + P, values, un * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ub_gap_.as<double>() + P, gaps, un * sizeof(double), hipMemcpyHostToDevice));
        ub_count_ += n;
        ub_entries_ += (int64_t)ne;
        return PBVI_OK;
    }

    UpperStore upper_store() const {
        return UpperStore{ub_ptr_.as<int64_t>(), ub_idx_.as<int32_t>(), ub_val_.as<double>(), ub_nnz_.as<int32_t>(),
                          ub_v_.as<double>(), ub_gap_.as<double>(), ub_c_.as<double>()};
    }

    // What pbvi_upper_bound and pbvi_upper_q refuse, in this order
    int upper_begin(const std::string& who, int64_t n_visible, int64_t n_hit, bool null_output) {
        if (null_output) FAIL(PBVI_EINVAL, who + ": NULL required output");
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, who + ": no belief block resident (call pbvi_beliefs_set)");
        if (!ub_corner_) FAIL(PBVI_EINVAL, who + ": no corner values set (call pbvi_upper_reset)");
        if (n_visible < 0 || n_visible > n_hit) FAIL(PBVI_EINVAL, who + ": need 0 <= n_visible <= n_hit");
        if (n_hit > ub_count_) FAIL(PBVI_EINVAL, who + ": n_hit exceeds the points in the store");
        HIPCHK(hipSetDevice(device_));
        return PBVI_OK;
    }

    // The scratch of a sawtooth evaluation of `rows` rows against n_hit points
    int upper_scratch(int64_t rows, int64_t n_hit, UpperScratch* ws) {
        const size_t cells = (size_t)rows * (size_t)std::max(1, upper_chunks(n_hit));
        int rc;
        if ((rc = ub_v0_.ensure((size_t)rows * sizeof(double)))) return rc;
        if ((rc = ub_bnnz_.ensure((size_t)rows * sizeof(int32_t)))) return rc;
        if ((rc = ub_pw_.ensure(cells * sizeof(double)))) return rc;
        if ((rc = ub_pi_.ensure(cells * sizeof(int32_t)))) return rc;
        if ((rc = ub_ph_.ensure(cells * sizeof(int32_t)))) return rc;
        *ws = UpperScratch{ub_v0_.as<double>(), ub_bnnz_.as<int32_t>(), ub_pw_.as<double>(), ub_pi_.as<int32_t>(), ub_ph_.as<int32_t>()};
        return PBVI_OK;
    }

    // The sawtooth of the resident block (pbvi_upper_bound).  Reads the block and the point store only.
    int upper_bound(int64_t n_visible, int64_t n_hit, double* out_value, int32_t* out_point, int32_t* out_hit) override {
        int rc = upper_begin("upper_bound", n_visible, n_hit, !out_value);
        if (rc) return rc;
        UpperScratch ws{};
        if ((rc = upper_scratch(blk_.B, n_hit, &ws))) return rc;
        if ((rc = ub_rv_.ensure((size_t)blk_.B * sizeof(double)))) return rc;
        if ((rc = ub_rp_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if ((rc = ub_rh_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        HIPCHK(launch_upper_sawtooth<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, S_, blk_.sorted ? blk_.perm.as<int32_t>() : nullptr, upper_store(),
                                        n_visible, n_hit, ws, ub_rv_.as<double>(), ub_rp_.as<int32_t>(), ub_rh_.as<int32_t>(),
                                        stream_));
        return out_.deliver({{out_value, ub_rv_.p, (size_t)blk_.B * sizeof(double)},
                             {out_point, ub_rp_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {out_hit, ub_rh_.p, (size_t)blk_.B * sizeof(int32_t)}});
    }

    // The bound-greedy action values of the resident block (pbvi_upper_q): the normalised successors of every (belief, action,
    // observation) are materialised as many beliefs at a time as half the memory still at hand holds (at least one), valued by
    // the sawtooth kernels, and folded into Q per belief.  Reads the block, the model tables and the point store only.
    int upper_q(double gamma, int64_t n_visible, int64_t n_hit, double* out_q, int32_t* out_action, double* out_p_obs,
                double* out_succ_value) override {
        int rc = upper_begin("upper_q", n_visible, n_hit, !out_q);
        if (rc) return rc;
        const int64_t AO = (int64_t)A_ * O_;
        if ((int64_t)S_ * R_ > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "upper_q: S*R exceeds int32");
        if (AO > 65535) FAIL(PBVI_EUNSUPPORTED, "upper_q: A*O exceeds 65535");
        if ((rc = build_inverse_lists())) return rc;
        const size_t all = (size_t)blk_.B * (size_t)AO;
        if ((rc = uq_mass_.ensure(all * sizeof(double)))) return rc;
        if ((rc = uq_val_.ensure(all * sizeof(double)))) return rc;
        if ((rc = uq_q_.ensure((size_t)blk_.B * A_ * sizeof(double)))) return rc;
        if ((rc = uq_act_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if (out_p_obs && (rc = uq_pobs_.ensure(all * sizeof(double)))) return rc;
        if (out_succ_value && (rc = uq_sval_.ensure(all * sizeof(double)))) return rc;
        // bytes one belief's successors take: un-normalised and normalised rows, block masses, the sawtooth's scratch
        const int64_t nblk = (S_ + 255) / 256, chunks = std::max(1, upper_chunks(n_hit));
        const int64_t per_belief = AO * ((int64_t)S_ * (int64_t)(sizeof(double) + sizeof(T)) + nblk * 8 + 12 + chunks * 16);
        const int64_t held = (int64_t)(uq_unnorm_.cap + uq_succ_.cap + uq_mpart_.cap + ub_v0_.cap + ub_bnnz_.cap + ub_pw_.cap +
                                       ub_pi_.cap + ub_ph_.cap);
        const int64_t nb = std::max<int64_t>(1, std::min({blk_.B, (int64_t)65535 / AO, (room() / 2 + held) / per_belief}));
        const size_t rows = (size_t)nb * (size_t)AO;
        if ((rc = uq_unnorm_.ensure(rows * S_ * sizeof(double)))) return rc;
        if ((rc = uq_succ_.ensure(rows * S_ * sizeof(T)))) return rc;
        if ((rc = uq_mpart_.ensure(rows * (size_t)nblk * sizeof(double)))) return rc;
        UpperScratch ws{};
        if ((rc = upper_scratch((int64_t)rows, n_hit, &ws))) return rc;
        BayesStep<T> bs = bayes_step(true);                 // the Bayes step of every (a, o), norm in block order, over uq_*
        bs.act = bs.obs = nullptr;
        bs.unnorm = uq_unnorm_.as<double>();
        bs.mass_part = uq_mpart_.as<double>();
        for (int64_t b0 = 0; b0 < blk_.B; b0 += nb) {
            const int cnt = (int)std::min(nb, blk_.B - b0);
            bs.every_ao_from = (int)b0;
            bs.B = (int)(cnt * AO);
            bs.mass = uq_mass_.as<double>() + b0 * AO;
            HIPCHK(launch_belief_push<T>(bs, view(), nullptr, stream_));
            HIPCHK(launch_belief_norm<T>(bs, S_, nullptr, uq_succ_.as<T>(), S_, stream_));
            HIPCHK(launch_upper_sawtooth<T>(uq_succ_.as<T>(), S_, (int)(cnt * AO), S_, nullptr, upper_store(), n_visible, n_hit, ws,
                                            uq_val_.as<double>() + b0 * AO, nullptr, nullptr, stream_));
        }
        HIPCHK(launch_upper_q_finish<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, view(), blk_.sorted ? blk_.perm.as<int32_t>() : nullptr, gamma,
                                        uq_mass_.as<double>(), uq_val_.as<double>(), uq_q_.as<double>(), uq_act_.as<int32_t>(),
                                        out_p_obs ? uq_pobs_.as<double>() : nullptr, out_succ_value ? uq_sval_.as<double>() : nullptr,
                                        stream_));
        return out_.deliver({{out_q, uq_q_.p, (size_t)blk_.B * A_ * sizeof(double)},
                             {out_action, uq_act_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {out_p_obs, uq_pobs_.p, all * sizeof(double)},
                             {out_succ_value, uq_sval_.p, all * sizeof(double)}});
    }

    // ---- environments (pbvi_env_set_frames / pbvi_env_set_table / pbvi_env_clear) ---- //
    int env_clear() override {
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
        env_frames_.release();
        env_chan_.release();
        env_table_.release();
        env_kind_ = ENV_NONE;
        env_F_ = env_C_ = 0;
        return PBVI_OK;
    }
    int env_set_frames(const uint8_t* frames, int64_t F, int64_t C, const int32_t* channel) override {
        if (!frames || !channel) FAIL(PBVI_EINVAL, "env_set_frames: NULL argument");
        if (F < 1 || C < 1) FAIL(PBVI_EINVAL, "env_set_frames: F and C must be at least 1");
        if (O_ > 255) FAIL(PBVI_EUNSUPPORTED, "env_set_frames: frames hold one byte per observation, so O must be at most 255");
        if (C > 0x7fffffff || F > INT64_MAX / C / S_) FAIL(PBVI_EUNSUPPORTED, "env_set_frames: F * C * S exceeds int64");
        for (int a = 0; a < A_; ++a)
            if (channel[a] < 0 || channel[a] >= C)
                FAIL(PBVI_EINVAL, "env_set_frames: channel_of_action[" + std::to_string(a) + "] is outside [0, C)");
        const size_t bytes = (size_t)F * (size_t)C * (size_t)S_;
        for (size_t k = 0; k < bytes; ++k)
            if (frames[k] >= O_)
                FAIL(PBVI_EINVAL, "env_set_frames: frame entry " + std::to_string(k) + " is " + std::to_string((int)frames[k]) +
                                      ", not an observation in [0, O)");
        int rc = env_clear();                                // (exact sizes: a released buffer does not grow with headroom)
        if (rc) return rc;
        if ((rc = env_frames_.ensure(bytes)) || (rc = env_chan_.ensure((size_t)A_ * sizeof(int32_t)))) {
            env_frames_.release();                            // (the error text is the failed allocation's)
            env_chan_.release();
            return rc;
        }
        HIPCHK(hipMemcpy(env_frames_.p, frames, bytes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(env_chan_.p, channel, (size_t)A_ * sizeof(int32_t), hipMemcpyHostToDevice));
        env_kind_ = ENV_FRAMES;
        env_F_ = F;
        env_C_ = C;
        return PBVI_OK;
    }
    int env_set_table(const double* obs_prob) override {
        if (!obs_prob) FAIL(PBVI_EINVAL, "env_set_table: NULL argument");
        const size_t rows = (size_t)S_ * A_;
        for (size_t k = 0; k < rows; ++k) {
            double tot = 0.0;
            for (int o = 0; o < O_; ++o) {
                const double p = obs_prob[k * O_ + o];
                if (!(p >= 0.0) || !std::isfinite(p))
                    FAIL(PBVI_EINVAL, "env_set_table: obs_prob[s', a, o] is negative or not finite at s' = " + std::to_string(k / A_) +
                                          ", a = " + std::to_string(k % A_) + ", o = " + std::to_string(o));
                tot += p;
            }
            if (!(tot > 0.0) || !std::isfinite(tot))
                FAIL(PBVI_EINVAL, "env_set_table: obs_prob[s', a, :] sums to 0 (or overflows) at s' = " + std::to_string(k / A_) +
                                      ", a = " + std::to_string(k % A_));
        }
        int rc = env_clear();
        if (rc) return rc;
        if ((rc = env_table_.ensure(rows * O_ * sizeof(double)))) return rc;
        HIPCHK(hipMemcpy(env_table_.p, obs_prob, rows * O_ * sizeof(double), hipMemcpyHostToDevice));
        env_kind_ = ENV_TABLE;
        return PBVI_OK;
    }

    // The stage of a rollout call's action source on the resident block; *index = what it leaves on the device for the draw:
    // for ROLLOUT_VALUE_MAX an alpha row per belief in ENGINE row order (the draw maps it through RolloutStep::alpha_actions),
    // for every other source an action per belief in CALLER row order.  t: the step; orig: the live simulations' rows in the
    // call (device, caller order) -- what a source that draws (Thompson) forms its simulation ids from.
    int rollout_stage(const RolloutCall& call, int64_t t, const int32_t* orig, const int32_t** index) {
        int rc;
        switch (call.source) {
            case ROLLOUT_STATE_POLICY:
                rc = state_policy_stage(call.rule, nullptr, call.seed, call.first_sim_id, orig, t);
                *index = sp_act_.as<int32_t>();
                return rc;
            case ROLLOUT_VALUE_MAX:
                rc = value_max_device(resident());
                *index = bv2_.as<int32_t>();
                return rc;
            case ROLLOUT_Q:
                rc = run_q(call.gamma, false);
                *index = q_act_.as<int32_t>();
                return rc;
            default:                                          // the two that score the successors
                rc = successor_scores(call.source == ROLLOUT_INFOTAXIS ? (int)SUCC_ENTROPY : call.objective, false, false);
                *index = gs_act_.as<int32_t>();
                return rc;
        }
    }

    // T lock-step simulation steps of the resident block on the device (pbvi_rollout, pbvi_rollout_infotaxis, pbvi_rollout_env,
    // pbvi_rollout_space_aware).  Per step: the action source's stage with its index left on the device (value-max or Q-values
    // against the resident alpha set, or successor_scores' G or F: rollout_stage); the simulator
    // draw (the model's own joint draw, or the successor from the model and the observation from the environment); the first half of the Bayes step for the rows not done; with
    // an environment the lost rule on their masses; the done-filter; the norm of the rows that go on.  Finished and lost rows
    // are dropped after EVERY step ("Device-resident rollouts"): the one host read per step is the survivor count,
    // which sizes the next step's launches.
    int rollout(const RolloutCall& call) override {
        const int source = call.source;
        const RolloutSourceInfo info = rollout_source_info(source);
        const bool env = call.env, uses_alpha = info.needs_alpha;
        const int64_t n_steps = call.T;
        if (env && env_kind_ == ENV_NONE) FAIL(PBVI_EINVAL, "rollout_env: no environment set (call pbvi_env_set_frames or pbvi_env_set_table)");
        if (env && call.end_observation >= O_) FAIL(PBVI_EINVAL, "rollout_env: end_observation is not below O");
        if (env && call.shifts && env_kind_ != ENV_FRAMES) FAIL(PBVI_EINVAL, "rollout_env: shifts are for a frame environment, and a table is set");
        if (uses_alpha && al_.V <= 0) FAIL(PBVI_EINVAL, "rollout: no alpha set resident (call pbvi_alpha_set)");
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "rollout: no belief block resident (call pbvi_beliefs_set)");
        if ((uses_alpha && !call.alpha_actions) || !call.start_states || !call.end_mask) FAIL(PBVI_EINVAL, "rollout: NULL argument");
        if (!info.known) FAIL(PBVI_EINVAL, "rollout: lookahead must be 0 or 1");
        if (info.needs_weights && call.objective != SUCC_SPACE_AWARE && call.objective != SUCC_EXPECTED_WEIGHT)
            FAIL(PBVI_EINVAL, std::string(info.who) + ": objective must be 0 (space-aware) or 1 (expected weight)");
        if (info.needs_weights && !sw_set_) FAIL(PBVI_EINVAL, std::string(info.who) + ": no state weights set (call pbvi_state_weights_set)");
        if (info.needs_state_policy && call.rule != STATE_POLICY_MLS && call.rule != STATE_POLICY_VOTING && call.rule != STATE_POLICY_THOMPSON)
            FAIL(PBVI_EINVAL, std::string(info.who) + ": rule must be 0 (most likely state), 1 (voting) or 2 (Thompson)");
        if (info.needs_state_policy && !sp_set_) FAIL(PBVI_EINVAL, std::string(info.who) + ": no state policy set (call pbvi_state_policy_set)");
        if (n_steps < 1) FAIL(PBVI_EINVAL, "rollout: T must be at least 1");
        if (source == ROLLOUT_Q && mode_ != PBVI_SPARSE)
            FAIL(PBVI_EUNSUPPORTED, "rollout: lookahead = 1 is not available on a PBVI_DENSE engine (create it with PBVI_SPARSE)");
        const int64_t n0 = blk_.B;
        if (n_steps >= 0x7fffffff || (n_steps + 1) * n0 > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "rollout: T * B exceeds the int32 trajectory slot index");
        if ((int64_t)S_ * R_ > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "rollout: S*R exceeds int32");
        for (int64_t b = 0; b < n0; ++b)
            if (call.start_states[b] < 0 || call.start_states[b] >= S_) FAIL(PBVI_EINVAL, "rollout: start state out of range [0,S)");
        for (int64_t v = 0; uses_alpha && v < al_.V; ++v)
            if (call.alpha_actions[v] < 0 || call.alpha_actions[v] >= A_) FAIL(PBVI_EINVAL, "rollout: alpha_actions entry out of range [0,A)");
        if (zero_row_ >= 0)
            FAIL(PBVI_EINVAL, "rollout: RTO[s,a,:,:] sums to 0 for s = " + std::to_string(zero_row_ / A_) + ", a = " +
                                  std::to_string(zero_row_ % A_) + ": nothing can follow that state-action pair");
        const bool frames = env && env_kind_ == ENV_FRAMES;
        if (frames) {                                         // the reference would index past its data: refused before any launch
            int64_t top = 0;
            for (int64_t b = 0; call.shifts && b < n0; ++b) {
                if (call.shifts[b] < 0) FAIL(PBVI_EINVAL, "rollout_env: negative shift");
                top = std::max(top, call.shifts[b]);
            }
            if (top > env_F_ || n_steps > env_F_ - top)
                FAIL(PBVI_EINVAL, "rollout_env: max(shift) + T = " + std::to_string(top) + " + " + std::to_string(n_steps) +
                                      " exceeds the " + std::to_string(env_F_) + " frames of the environment");
        }
        HIPCHK(hipSetDevice(device_));
        const bool fixed_order = env || info.fixed_order;      // (RolloutSourceInfo says why)
        int rc;
        if (env) {
            if ((rc = ro_lost_.ensure((size_t)n0))) return rc;
            HIPCHK(hipMemsetAsync(ro_lost_.p, 0, (size_t)n0, stream_));
        }
        if (frames) {
            if ((rc = env_shift_.ensure((size_t)n0 * sizeof(int64_t)))) return rc;
            if (call.shifts) HIPCHK(hipMemcpyAsync(env_shift_.p, call.shifts, (size_t)n0 * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
            else HIPCHK(hipMemsetAsync(env_shift_.p, 0, (size_t)n0 * sizeof(int64_t), stream_));
        }
        const size_t n_st = (size_t)(n_steps + 1) * n0, n_ao = (size_t)n_steps * n0, n_traj = n_st + 2 * n_ao + (size_t)n0;
        if ((rc = ro_traj_.ensure(n_traj * sizeof(int32_t)))) return rc;
        for (int k = 0; k < 2; ++k) {
            if ((rc = ro_state_[k].ensure((size_t)n0 * sizeof(int32_t)))) return rc;
            if ((rc = ro_orig_[k].ensure((size_t)n0 * sizeof(int32_t)))) return rc;
        }
        if ((rc = ro_keep_.ensure((size_t)n0))) return rc;
        if ((rc = ro_dst_.ensure((size_t)(n0 + 1) * sizeof(int32_t)))) return rc;
        if (uses_alpha && (rc = ro_aact_.ensure((size_t)al_.V * sizeof(int32_t)))) return rc;
        if ((rc = ro_end_.ensure((size_t)S_))) return rc;
        if ((rc = bayes_ensure(n0, fixed_order))) return rc;
        if ((rc = build_inverse_lists())) return rc;
        int32_t* tr_states = ro_traj_.as<int32_t>();
        int32_t* tr_actions = tr_states + n_st;
        int32_t* tr_obs = tr_actions + n_ao;
        int32_t* tr_steps = tr_obs + n_ao;
        {   // slots never reached stay -1; row 0 of the states = the start states; a simulation that never finishes took T steps
            std::vector<int32_t> iota((size_t)n0), full((size_t)n0, (int32_t)n_steps);
            for (int64_t b = 0; b < n0; ++b) iota[(size_t)b] = (int32_t)b;
            HIPCHK(hipMemsetAsync(ro_traj_.p, 0xFF, (n_traj - (size_t)n0) * sizeof(int32_t), stream_));
            HIPCHK(hipMemcpyAsync(tr_states, call.start_states, (size_t)n0 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(tr_steps, full.data(), (size_t)n0 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(ro_state_[0].p, call.start_states, (size_t)n0 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(ro_orig_[0].p, iota.data(), (size_t)n0 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            if (uses_alpha) HIPCHK(hipMemcpyAsync(ro_aact_.p, call.alpha_actions, (size_t)al_.V * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(ro_end_.p, call.end_mask, (size_t)S_, hipMemcpyHostToDevice, stream_));
            HIPCHK(hipStreamSynchronize(stream_));            // the caller's arrays and the two vectors are free again
        }
        RolloutEnv renv{};
        renv.end_observation = call.end_observation;
        if (frames) {
            renv.frames = env_frames_.as<uint8_t>();
            renv.C = (int)env_C_;
            renv.channel = env_chan_.as<int32_t>();
            renv.shift = env_shift_.as<int64_t>();
        } else if (env) {
            renv.table = env_table_.as<double>();
        }
        // True states: live in ro_state_[0]; the draw leaves the next states in [1], row for row, and the filter moves the
        // survivors' back up into [0].  Trajectory rows: the filter moves them from one ro_orig_ buffer to the other.
        RolloutStep rs{};
        rs.n0 = (int)n0;
        rs.V = (int)al_.V;
        rs.seed = call.seed;
        rs.first_id = call.first_sim_id;
        rs.alpha_actions = source == ROLLOUT_VALUE_MAX ? ro_aact_.as<int32_t>() : nullptr;
        rs.state = ro_state_[0].as<int32_t>();
        rs.end_mask = ro_end_.as<uint8_t>();
        rs.act_e = bu_act_.as<int32_t>();
        rs.obs_e = bu_obs_.as<int32_t>();
        rs.row_e = bu_row_.as<int32_t>();
        rs.next_state = ro_state_[1].as<int32_t>();
        rs.keep = ro_keep_.as<uint8_t>();
        rs.tr_states = tr_states;
        rs.tr_actions = tr_actions;
        rs.tr_obs = tr_obs;
        rs.steps = tr_steps;
        int* d_count = ro_dst_.as<int>() + n0;
        int oc = 0;
        for (int64_t t = 0; t < n_steps; ++t) {
            if ((rc = rollout_stage(call, t, ro_orig_[oc].as<int32_t>(), &rs.index))) return rc;
            rs.n = (int)blk_.B;
            rs.t = (int)t;
            rs.perm = blk_.sorted ? blk_.perm.as<int32_t>() : nullptr;
            rs.orig = ro_orig_[oc].as<int32_t>();
            // draw (bu_row_: provisional, -1 = done), push of the rows not done, then the lost rule on their masses
            HIPCHK(launch_rollout_draw<T>(rs, view(), env ? &renv : nullptr, stream_));
            if ((rc = bayes_push(rs.row_e, fixed_order))) return rc;
            if (env) HIPCHK(launch_rollout_lost(rs, bu_mass_.as<double>(), ro_lost_.as<uint8_t>(), stream_));
            HIPCHK(launch_rollout_compact(rs, ro_dst_.as<int32_t>(), ro_state_[0].as<int32_t>(), ro_orig_[oc ^ 1].as<int32_t>(),
                                          d_count, stream_));
            oc ^= 1;
            int* h_count = &words().survivors;
            HIPCHK(hipMemcpyAsync(h_count, d_count, sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIPCHK(hipStreamSynchronize(stream_));
            const int64_t nb = *h_count;
            if (nb < 0 || nb > rs.n) FAIL(PBVI_ERUNTIME, "rollout: survivor count out of range");
            if (nb == 0) {                                    // every simulation finished
                block_emptied();
                break;
            }
            // the norm of the rows that go on (bu_row_: now the filter's rows)
            if ((rc = bayes_norm_finish(nb, false))) return rc;
        }
        if (env && call.out_lost) HIPCHK(hipMemcpyAsync(call.out_lost, ro_lost_.p, (size_t)n0, hipMemcpyDeviceToHost, stream_));
        const int32_t* src[4] = {tr_states, tr_actions, tr_obs, tr_steps};
        int32_t* dsts[4] = {call.out_states, call.out_actions, call.out_observations, call.out_steps};
        const size_t len[4] = {n_st, n_ao, n_ao, (size_t)n0};
        // one transfer of the whole trajectory buffer into the pinned staging area, then host copies of the parts asked for
        if (dsts[0] || dsts[1] || dsts[2] || dsts[3]) {
            char* h_traj = nullptr;
            if ((rc = out_.raw(n_traj * sizeof(int32_t), &h_traj))) return rc;
            HIPCHK(hipMemcpyAsync(h_traj, ro_traj_.p, n_traj * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            HIPCHK(hipStreamSynchronize(stream_));
            for (int k = 0; k < 4; ++k)
                if (dsts[k]) host_copy(dsts[k], h_traj + (size_t)(src[k] - tr_states) * sizeof(int32_t), len[k] * sizeof(int32_t));
        } else {
            HIPCHK(hipStreamSynchronize(stream_));
        }
        return PBVI_OK;
    }

    // The raw slab buffer as the last score_gemm's kernel left it (pbvi_debug_slabs); out == nullptr: the size only
    int64_t debug_slabs(void* out, int64_t cap_bytes) override {
        if (slab_bytes_ <= 0 || slabs_.p == nullptr || (int64_t)slabs_.cap < slab_bytes_)
            FAIL(PBVI_EINVAL, "debug_slabs: no score GEMM has run");
        if (!out) return slab_bytes_;
        if (cap_bytes < slab_bytes_) FAIL(PBVI_EINVAL, "debug_slabs: the output array is smaller than the slab buffer");
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipMemcpyAsync(out, slabs_.p, (size_t)slab_bytes_, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        return slab_bytes_;
    }
    // Every byte of that buffer set to `byte` (pbvi_debug_slabs_fill): what a later GEMM does not write stays so
    int debug_slabs_fill(int byte) override {
        if (slab_bytes_ <= 0 || slabs_.p == nullptr || (int64_t)slabs_.cap < slab_bytes_)
            FAIL(PBVI_EINVAL, "debug_slabs_fill: no score GEMM has run");
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipMemsetAsync(slabs_.p, byte & 0xff, (size_t)slab_bytes_, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        return PBVI_OK;
    }

    // The bookkeeping of the most recent refinement pass (pbvi_debug_refine_counts): the three words of RefineWork::cnt as
    // that pass left them (uncapped) and the capacities it ran with.  A copy on request; nothing is kept per call but the
    // RefineWork itself.
    int debug_refine_counts(int64_t* out) override {
        if (!out) FAIL(PBVI_EINVAL, "debug_refine_counts: out is NULL");
        if (!have_last_work_) FAIL(PBVI_EINVAL, "debug_refine_counts: no refinement has run");
        const RefineWork& w = last_work_;
        int cnt[3] = {0, 0, 0};
        if (w.cnt != nullptr) {                              // (nullptr: PBVI_REFINE_INBLOCK, no work list at all)
            if (rf_cnt_.p == nullptr || w.cnt != rf_cnt_.as<int>())
                FAIL(PBVI_EINVAL, "debug_refine_counts: the work list of that pass has been released");
            HIPCHK(hipSetDevice(device_));
            HIPCHK(hipStreamSynchronize(stream_));
            HIPCHK(hipMemcpy(cnt, w.cnt, sizeof(cnt), hipMemcpyDeviceToHost));
        }
        out[0] = cnt[0];
        out[1] = cnt[1];
        out[2] = cnt[2];
        out[3] = w.item_cap;
        out[4] = w.slot_cap;
        out[5] = w.w_slot_cap;
        out[6] = w.q2_cap;
        out[7] = w.defer_min;
        return PBVI_OK;
    }

    // The route of the most recent value_max_device (pbvi_debug_value_max_route): host words only, nothing on the device.
    int debug_value_max_route(int64_t* out) override {
        if (!out) FAIL(PBVI_EINVAL, "debug_value_max_route: out is NULL");
        if (vmax_route_[6] == 0) FAIL(PBVI_EINVAL, "debug_value_max_route: no value-max has run");
        for (int i = 0; i < 8; ++i) out[i] = vmax_route_[i];
        return PBVI_OK;
    }

    // ---- test-only score probe (pbvi_debug_score_probe / _fetch) ---- //
    void probe_release() {
        for (DevBuf* b : {&probe_score_, &probe_mag_, &probe_err_, &probe_bv_, &probe_bs_, &probe_queue_, &probe_dead_, &probe_words_})
            b->release();
        probe_seq_ = 0;
    }
    int debug_score_probe(int enable) override {
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
        probe_on_ = enable != 0;
        probe_seq_ = 0;                                      // a capture counts from the moment the probe was enabled
        if (!probe_on_) probe_release();
        if (screen_) {
            screen_->probe_on_ = probe_on_;
            screen_->probe_seq_ = 0;
            if (!probe_on_) screen_->probe_release();
        }
        return PBVI_OK;
    }
    // End of the scoring stage, behind launch_argmax and in front of every later stage, on the pipeline's stream: what the
    // argmax read (scores and magnitudes through its SlabView) and what it wrote (windows, first maxima, queue).
    int probe_capture(const SlabView<T>& sv, const ScoreIO& io, const ScoreStage<T>& out) {
        int rc;
        const int64_t G = (int64_t)A_ * O_, pairs = blk_.B * G, n = pairs * al_.V;
        probe_seq_ = 0;                                      // (a stage that fails below leaves nothing to fetch)
        if (n > ((int64_t)1 << 24))
            FAIL(PBVI_EINVAL, "score probe: B * A * O * V = " + std::to_string(n) + " exceeds 2^24 (the probe is for tests)");
        if ((rc = probe_score_.ensure((size_t)n * sizeof(double)))) return rc;
        if ((rc = probe_mag_.ensure((size_t)pairs * sizeof(double)))) return rc;
        if ((rc = probe_err_.ensure((size_t)pairs * sizeof(double)))) return rc;
        if ((rc = probe_bs_.ensure((size_t)pairs * sizeof(double)))) return rc;
        if ((rc = probe_bv_.ensure((size_t)pairs * sizeof(int32_t)))) return rc;
        if ((rc = probe_queue_.ensure((size_t)pairs * sizeof(int32_t)))) return rc;
        if ((rc = probe_dead_.ensure((size_t)pairs))) return rc;
        if ((rc = probe_words_.ensure(2 * sizeof(int)))) return rc;
        HIPCHK(launch_score_probe<T>(sv, (int)al_.V, (int)G, (int)blk_.B, probe_score_.as<double>(), probe_mag_.as<double>(), stream_));
        HIPCHK(hipMemcpyAsync(probe_err_.p, io.err, (size_t)pairs * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        HIPCHK(hipMemcpyAsync(probe_bs_.p, io.best_score, (size_t)pairs * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        HIPCHK(hipMemcpyAsync(probe_bv_.p, io.best_v, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
        if (io.queue != nullptr) {
            HIPCHK(hipMemcpyAsync(probe_queue_.p, io.queue, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
            HIPCHK(hipMemcpyAsync(probe_words_.p, io.qcount, sizeof(int), hipMemcpyDeviceToDevice, stream_));
        } else {
            HIPCHK(hipMemsetAsync(probe_words_.p, 0, sizeof(int), stream_));
        }
        if (io.dead != nullptr) HIPCHK(hipMemcpyAsync(probe_dead_.p, io.dead, (size_t)pairs, hipMemcpyDeviceToDevice, stream_));
        else HIPCHK(hipMemsetAsync(probe_dead_.p, 0, (size_t)pairs, stream_));
        if (out.chain != nullptr)
            HIPCHK(hipMemcpyAsync(probe_words_.as<int>() + 1, out.chain, sizeof(int), hipMemcpyDeviceToDevice, stream_));
        probe_info_.B = blk_.B;
        probe_info_.G = G;
        probe_info_.V = al_.V;
        probe_info_.f64_pairs = out.f64_pairs;
        probe_info_.f64_split = f64_split_;
        probe_info_.push = sv.push;
        probe_info_.split = out.split;
        probe_info_.chunks = out.chunks;
        probe_info_.has_chain = out.chain != nullptr;
        probe_info_.tol_rel = out.tol_rel;
        probe_info_.tol_extra = io.tol_extra;
        probe_seq_ = next_probe_seq();
        return PBVI_OK;
    }
    // The capture of THIS engine to host arrays (any of them may be nullptr); perm is the caller's (debug_score_probe_fetch)
    int probe_copy_out(int64_t* dims, double* scalars, double* score, double* mag, double* err, int32_t* best_v,
                       double* best_score, int32_t* queue, uint8_t* dead) {
        const ProbeInfo& pi = probe_info_;
        const int64_t pairs = pi.B * pi.G;
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
        int w[2] = {0, -1};
        HIPCHK(hipMemcpy(w, probe_words_.p, (pi.has_chain ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost));
        if (w[0] < 0 || w[0] > pairs) FAIL(PBVI_ERUNTIME, "score probe: queue count out of range");
        if (dims) {
            const int64_t d[8] = {pi.B, pi.G, pi.V, w[0], pi.push, pi.f64_pairs, pi.f64_split, pi.chunks};
            std::copy(d, d + 8, dims);
        }
        if (scalars) {
            scalars[0] = (double)pi.split;
            scalars[1] = pi.has_chain ? (double)w[1] : -1.0;
            scalars[2] = pi.tol_rel;
            scalars[3] = pi.tol_extra;
        }
        if (score) HIPCHK(hipMemcpy(score, probe_score_.p, (size_t)pairs * pi.V * sizeof(double), hipMemcpyDeviceToHost));
        if (mag) HIPCHK(hipMemcpy(mag, probe_mag_.p, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (err) HIPCHK(hipMemcpy(err, probe_err_.p, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (best_score) HIPCHK(hipMemcpy(best_score, probe_bs_.p, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (best_v) HIPCHK(hipMemcpy(best_v, probe_bv_.p, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (queue && w[0] > 0) HIPCHK(hipMemcpy(queue, probe_queue_.p, (size_t)w[0] * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (dead) HIPCHK(hipMemcpy(dead, probe_dead_.p, (size_t)pairs, hipMemcpyDeviceToHost));
        return PBVI_OK;
    }
    int debug_score_probe_fetch(int64_t* dims, double* scalars, double* score, double* mag, double* err, int32_t* best_v,
                                double* best_score, int32_t* queue, uint8_t* dead, int32_t* perm) override {
        // an fp64 engine: the stage that ran last -- its screen's, or its own (screen off, or the screen overflowed)
        const bool on_screen = screen_ != nullptr && screen_->probe_seq_ > probe_seq_;
        const uint64_t seq = on_screen ? screen_->probe_seq_ : probe_seq_;
        const int64_t Bc = on_screen ? screen_->probe_info_.B : probe_info_.B;
        if (seq == 0 || (on_screen ? screen_->probe_score_.p : probe_score_.p) == nullptr)
            FAIL(PBVI_EINVAL, "score probe: nothing captured since the probe was enabled");
        int rc = on_screen ? screen_->probe_copy_out(dims, scalars, score, mag, err, best_v, best_score, queue, dead)
                           : probe_copy_out(dims, scalars, score, mag, err, best_v, best_score, queue, dead);
        if (rc) return rc;
        if (perm) {                                          // caller's row of engine row i (the order is this engine's)
            if (Bc != blk_.B) FAIL(PBVI_EINVAL, "score probe: the belief block changed since the capture");
            if ((rc = host_perm())) return rc;
            for (int64_t i = 0; i < blk_.B; ++i) perm[i] = blk_.sorted ? blk_.h_perm[(size_t)i] : (int32_t)i;
        }
        return PBVI_OK;
    }

    // resident belief block back to the host (or a device buffer), caller order: [B][S] T
    int beliefs_fetch(void* out) override {
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "beliefs_fetch: no belief block resident");
        if (!out) FAIL(PBVI_EINVAL, "beliefs_fetch: NULL argument");
        HIPCHK(hipSetDevice(device_));
        int rc = host_perm();
        if (rc) return rc;
        out_.begin();
        out_.add_rows(out, blk_.rows.p, (size_t)S_pad_ * sizeof(T), (size_t)blk_.B, (size_t)S_ * sizeof(T), caller_order());
        return out_.finish();
    }

    int64_t beliefs_count() const override { return blk_.B; }

    // ---- device row stores ------------------------------------------------ //
    int64_t store_append(int which, const void* rows, int64_t n) override {
        if (which < 0 || which > 1 || n < 0 || (n > 0 && rows == nullptr)) FAIL(PBVI_EINVAL, "store_append: bad arguments");
        if (hipSetDevice(device_) != hipSuccess) FAIL(PBVI_ERUNTIME, "hipSetDevice failed");
        T* dst = nullptr;
        int rc = store_reserve(which, n, &dst);
        if (rc) return rc;
        if (n > 0) {
            if (hipMemsetAsync(dst, 0, (size_t)n * S_pad_ * sizeof(T), stream_) != hipSuccess ||
                hipMemcpy2DAsync(dst, (size_t)S_pad_ * sizeof(T), rows, (size_t)S_ * sizeof(T), (size_t)S_ * sizeof(T),
                                 (size_t)n, hipMemcpyHostToDevice, stream_) != hipSuccess ||
                hipStreamSynchronize(stream_) != hipSuccess)
                FAIL(PBVI_ERUNTIME, "store_append: upload failed");
        }
        return store_commit(which, n);
    }

    // distinct alpha' rows of the last backup -> alpha store, device to device (ids are consecutive from the return)
    int64_t store_append_unique(const int32_t* unique_idx, int64_t n) override {
        int rc = need_result("backup_store_unique");
        if (rc) return rc;
        if (n <= 0 || n > 65535 || unique_idx == nullptr) FAIL(PBVI_EINVAL, "backup_store_unique: bad arguments (1 <= n <= 65535)");
        for (int64_t i = 0; i < n; ++i)
            if (unique_idx[i] < 0 || unique_idx[i] >= res_unique_) FAIL(PBVI_EINVAL, "backup_store_unique: row index out of range");
        T* dst = nullptr;
        if ((rc = store_reserve(0, n, &dst))) return rc;
        if ((rc = ids_.ensure((size_t)n * sizeof(int32_t)))) return rc;
        HIPCHK(hipMemcpyAsync(ids_.p, unique_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        if (S_pad_ > S_) HIPCHK(hipMemsetAsync(dst, 0, (size_t)n * S_pad_ * sizeof(T), stream_));   // pad columns stay zero
        hipLaunchKernelGGL(k_gather_rows_ld<T>, dim3((S_ + 255) / 256, (unsigned)n), dim3(256), 0, stream_, fin_.rows.as<T>(), S_,
                           dst, S_pad_, S_, ids_.as<int32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream_));            // unique_idx is the caller's host memory
        return store_commit(0, n);
    }

    // make room for n more rows in a store, keeping what is there; returns the destination of the new rows
    int store_reserve(int which, int64_t n, T** dst) {
        DevBuf& st = store_[which];
        const int64_t have = store_rows_[which];
        const size_t need = (size_t)(have + n) * S_pad_ * sizeof(T);
        int rc = grow_keep(st, need, (size_t)have * S_pad_ * sizeof(T));
        if (rc) return rc;
        *dst = st.as<T>() + (size_t)have * S_pad_;
        return PBVI_OK;
    }
    // the n rows written behind a store's rows are its rows now; returns the id of the first of them
    int64_t store_commit(int which, int64_t n) {
        const int64_t first = store_rows_[which];
        store_rows_[which] = first + n;
        return first;
    }

    // fp64 copy of RTO (reference layout [S][A][O][R]) for the belief walk of an f32 engine: the host mirror keeps
    // fp64 belief values, and they should not depend on the engine's arithmetic type
    int set_rto_f64(const double* rto) override {
        if (!rto) FAIL(PBVI_EINVAL, "set_rto_f64: NULL table");
        HIPCHK(hipSetDevice(device_));
        std::vector<double> h((size_t)A_ * O_ * R_ * S_pad_, 0.0);
        for (int s = 0; s < S_; ++s)
            for (int a = 0; a < A_; ++a)
                for (int o = 0; o < O_; ++o)
                    for (int r = 0; r < R_; ++r)
                        h[(((size_t)a * O_ + o) * R_ + r) * S_pad_ + s] = rto[(((size_t)s * A_ + a) * O_ + o) * R_ + r];
        int rc = rto64_.ensure(h.size() * sizeof(double));
        if (rc) return rc;
        HIPCHK(hipMemcpy(rto64_.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        return PBVI_OK;
    }

    // FSVI-style walk: n chained Bayes updates on the device (fp64), every new belief appended to the belief store
    // and copied to `out` [n][S] fp64.  Returns the store id of the first new belief.
    int64_t belief_walk(const double* b0, int64_t n, const int32_t* act, const int32_t* obs, const uint8_t* restart,
                        double* out) override {
        if (!b0 || n <= 0 || !act || !obs || !out) FAIL(PBVI_EINVAL, "belief_walk: bad arguments");
        if ((int64_t)S_ * R_ > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "belief_walk: S*R exceeds int32");
        for (int64_t i = 0; i < n; ++i)
            if (act[i] < 0 || act[i] >= A_ || obs[i] < 0 || obs[i] >= O_) FAIL(PBVI_EINVAL, "belief_walk: action / observation out of range");
        HIPCHK(hipSetDevice(device_));
        int rc = build_inverse_lists();
        if (rc) return rc;
        const int blocks = (S_pad_ + 255) / 256;
        if ((rc = walk64_.ensure((size_t)(n + 1) * S_ * sizeof(double)))) return rc;      // row 0 = b0
        if ((rc = bu_unnorm_.ensure((size_t)2 * S_ * sizeof(double)))) return rc;          // ping-pong: raw row of step i
        if ((rc = bu_mass_.ensure((size_t)2 * blocks * sizeof(double)))) return rc;      // and its block partials
        T* dst = nullptr;
        if ((rc = store_reserve(1, n, &dst))) return rc;
        double* rows = walk64_.as<double>();
        HIPCHK(hipMemcpyAsync(rows, b0, (size_t)S_ * sizeof(double), hipMemcpyHostToDevice, stream_));
        const ModelView<T> mv = view();
        // The fp64 rows go back to the host while the chain is still running: in quarters, each copied by the side
        // stream into the pinned buffer as soon as its last step is done, and moved on to the caller's memory by this
        // thread while the device works on the next quarter (the 24 MB of a 99-step walk at S = 30000 took 1.4 ms
        // after a 1.2 ms chain; now most of it hides behind the chain).
        const bool to_host = !is_device_pointer(out);
        constexpr int kChunks = 4;
        int64_t chunk_end[kChunks];
        int n_chunks = 0;
        char* h_rows = nullptr;                                                  // the staging buffer as raw pinned memory
        if (to_host && n >= 2 * kChunks) {
            out_.begin();                                                        // (nothing of an earlier call is staged)
            if ((rc = out_.raw((size_t)n * S_ * sizeof(double), &h_rows))) return rc;
            for (auto& e : walk_ev_) HIPCHK(new_event(&e, hipEventDisableTiming, "hipEventDestroy(walk)"));
            n_chunks = kChunks;
            for (int c = 0; c < kChunks; ++c) chunk_end[c] = n * (c + 1) / kChunks;
        }
        // step i: one kernel pushes belief i (b0 at the start and after a restart, else the previous step's raw row
        // normalised on the fly) and writes belief i (rows64 row i, store row i - 1); the last belief is finished by a
        // normalisation of its own.  A quarter of the rows is complete once the kernel after its last step is queued.
        static const bool two_kernels = getenv("PBVI_WALK_TWO_KERNELS") != nullptr;      // debug / A-B only: the unfused chain
        auto queue_copy = [&](int c) -> int {
            const int64_t r0 = c ? chunk_end[c - 1] : 0, r1 = chunk_end[c];
            HIPCHK(hipEventRecord(walk_ev_[2 * c], stream_));
            HIPCHK(hipStreamWaitEvent(stream2_, walk_ev_[2 * c], 0));
            HIPCHK(hipMemcpyAsync(h_rows + (size_t)r0 * S_ * sizeof(double), rows + (size_t)(r0 + 1) * S_,
                                  (size_t)(r1 - r0) * S_ * sizeof(double), hipMemcpyDeviceToHost, stream2_));
            HIPCHK(hipEventRecord(walk_ev_[2 * c + 1], stream2_));
            return PBVI_OK;
        };
        int c_next = 0;
        double* un[2] = {bu_unnorm_.as<double>(), bu_unnorm_.as<double>() + S_};
        double* pa[2] = {bu_mass_.as<double>(), bu_mass_.as<double>() + blocks};
        for (int64_t i = 0; i < n; ++i) {
            if (two_kernels) {
                const double* base = (restart && restart[i]) ? rows : rows + (size_t)i * S_;       // row i = b_i (row 0 = b0)
                HIPCHK(launch_walk_step<T>(base, mv, rto64_.as<double>(), in_ptr_.as<int32_t>(), in_src_.as<int32_t>(), act[i], obs[i],
                                           un[0], pa[0], rows + (size_t)(i + 1) * S_, dst + (size_t)i * S_pad_, stream_));
                if (c_next < n_chunks && i + 1 == chunk_end[c_next]) {
                    if ((rc = queue_copy(c_next))) return rc;
                    ++c_next;
                }
                continue;
            }
            const bool from_b0 = i == 0 || (restart && restart[i]);
            const double* prev_un = i > 0 ? un[(i - 1) & 1] : nullptr;
            HIPCHK(launch_walk_fused<T>(from_b0 ? rows : nullptr, prev_un, i > 0 ? pa[(i - 1) & 1] : nullptr,
                                        i > 0 ? rows + (size_t)i * S_ : nullptr, i > 0 ? dst + (size_t)(i - 1) * S_pad_ : nullptr, mv,
                                        rto64_.as<double>(), in_ptr_.as<int32_t>(), in_src_.as<int32_t>(), act[i], obs[i], un[i & 1],
                                        pa[i & 1], stream_));
            if (c_next < n_chunks && i == chunk_end[c_next]) {         // beliefs 1 .. i are written
                if ((rc = queue_copy(c_next))) return rc;
                ++c_next;
            }
        }
        if (!two_kernels) {
            HIPCHK(launch_walk_finish<T>(un[(n - 1) & 1], pa[(n - 1) & 1], mv, rows + (size_t)n * S_, dst + (size_t)(n - 1) * S_pad_, stream_));
            while (c_next < n_chunks) {
                if ((rc = queue_copy(c_next))) return rc;
                ++c_next;
            }
        }
        if (n_chunks > 0) {
            for (int c = 0; c < n_chunks; ++c) {
                const int64_t r0 = c ? chunk_end[c - 1] : 0;
                HIPCHK(hipEventSynchronize(walk_ev_[2 * c + 1]));
                host_copy((char*)out + (size_t)r0 * S_ * sizeof(double), h_rows + (size_t)r0 * S_ * sizeof(double),
                            (size_t)(chunk_end[c] - r0) * S_ * sizeof(double));
            }
            HIPCHK(hipStreamSynchronize(stream_));
        } else if ((rc = out_.deliver({{out, rows + S_, (size_t)n * S_ * sizeof(double)}}))) {
            return rc;
        }
        walk_rows_ = n;
        return store_commit(1, n);
    }

    // max_v b.alpha_v of the last backup's beliefs against its alpha set, caller order (belief-side formulation only)
    int backup_value_max(double* out_value) override {
        if (!have_result_ || !have_bk_vmax_)
            FAIL(PBVI_EUNSUPPORTED, "backup_fetch_value_max: the last backup did not run in the belief-side formulation");
        if (!out_value) FAIL(PBVI_EINVAL, "backup_fetch_value_max: NULL destination");
        HIPCHK(hipSetDevice(device_));
        return out_.deliver({{out_value, vmax_bk_.p, (size_t)res_B_ * sizeof(double)}});
    }

    // position-weighted bit-pattern hashes (k_row_hash) of the fp64 rows of the last walk (rows 1..n of walk64_), for the
    // host's dedup keys
    int walk_keys(int64_t n, uint64_t* out_keys) override {
        if (n <= 0 || n != walk_rows_ || !out_keys) FAIL(PBVI_EINVAL, "belief_walk_keys: n must be the length of the last walk");
        HIPCHK(hipSetDevice(device_));
        int rc = keys_tmp_.ensure((size_t)n * sizeof(uint64_t));
        if (rc) return rc;
        hipLaunchKernelGGL(k_row_hash<double>, dim3((unsigned)n), dim3(256), 0, stream_, walk64_.as<double>() + S_, S_, S_,
                           keys_tmp_.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        return out_.deliver({{out_keys, keys_tmp_.p, (size_t)n * sizeof(uint64_t)}});
    }

    // After a call returned PBVI_ENOMEM: back to the state of a fresh engine (model tables kept, every working set, row
    // store and scratch buffer released), so that the caller -- PBVI_Solver.solve turns the error into "return the
    // partial result" like src/pomdp.py:2399-2401 -- can go on using the engine with whatever it uploads next.
    int after_oom() override {
        HIPCHK(hipSetDevice(device_));
        (void)hipStreamSynchronize(stream_);
        if (stream2_) (void)hipStreamSynchronize(stream2_);
        if (stream3_) (void)hipStreamSynchronize(stream3_);
        for (DevBuf* b : mem_.bufs)
            if (b->life == DevBuf::WORKING) b->release();
        al_.emptied();                                       // (its view pointed into a working buffer)
        env_kind_ = ENV_NONE;                                // (its buffers were working buffers)
        env_F_ = env_C_ = 0;
        ub_count_ = ub_entries_ = 0;                         // (so were the point store's)
        ub_corner_ = false;
        sw_set_ = false;                                     // (the weights were a working buffer)
        sp_set_ = false;                                     // (so was the state policy's table)
        block_emptied();
        store_rows_[0] = store_rows_[1] = 0;
        snz_rows_ = sbt_rows_ = 0;
        walk_rows_ = 0;
        have_bk_vmax_ = false;
        mat_V_ = -1;
        gam_pad_ptr_ = nullptr;
        last_deferred_nothing_ = false;
        have_last_work_ = false;                             // (its lists were working buffers)
        probe_seq_ = 0;                                      // (the capture's buffers were working buffers)
        if (screen_) {
            screen_alpha_seen_ = {};
            screen_bel_seen_ = 0;
            return screen_->after_oom();
        }
        return PBVI_OK;
    }

    int store_reset(int which) override {
        if (which < 0 || which > 1) FAIL(PBVI_EINVAL, "store_reset: bad store");
        store_rows_[which] = 0;
        if (which == 1) snz_rows_ = sbt_rows_ = 0;
        if (which == 0) al_.primary_given_up();
        return PBVI_OK;
    }

    int store_select(int which, const int32_t* ids, int64_t n) override {
        if (which < 0 || which > 1 || n <= 0 || ids == nullptr) FAIL(PBVI_EINVAL, "store_select: bad arguments");
        if (n > 65535 && which == 1) FAIL(PBVI_EUNSUPPORTED, "at most 65535 beliefs per block");
        for (int64_t i = 0; i < n; ++i)
            if (ids[i] < 0 || ids[i] >= store_rows_[which]) FAIL(PBVI_EINVAL, "store_select: id out of range");
        HIPCHK(hipSetDevice(device_));
        const int rc = ids_.ensure((size_t)n * sizeof(int32_t));
        if (rc) return rc;
        return which == 0 ? select_alpha(ids, n) : select_beliefs(ids, n);
    }

    // Resident block := stored beliefs, gathered straight from the store rows in sorted order (no staging copy).  The ids travel
    // through a pinned buffer of the engine's own, so nothing here waits for the device: the backup is enqueued behind it.
    int select_beliefs(const int32_t* ids, int64_t n) {
        const size_t bytes = (size_t)n * sizeof(int32_t);
        if (ids_pin_.cap < bytes) {
            HIPCHK(hipStreamSynchronize(stream_));
            if (!ids_pin_.ensure(bytes, std::max<size_t>(bytes, 65536))) FAIL(PBVI_ENOMEM, "store_select: pinned staging for the ids");
        } else if (ev_ids_) {
            HIPCHK(hipEventSynchronize(ev_ids_));        // the previous selection's copy has left the buffer
        }
        std::memcpy(ids_pin_.p, ids, bytes);
        HIPCHK(hipMemcpyAsync(ids_.p, ids_pin_.p, bytes, hipMemcpyHostToDevice, stream_));
        HIPCHK(new_event(&ev_ids_, hipEventDisableTiming, "hipEventDestroy(ids)"));
        HIPCHK(hipEventRecord(ev_ids_, stream_));
        return beliefs_finish(n, store_[1].as<T>(), ids_.as<int32_t>());
    }

    // Working alpha set := stored rows in the caller's order, laid out as AlphaSet::selection says.  EXTEND: the new rows go
    // into the free rows in front of the primary set; the magnitude row stays where it is, row n of the new view.  SMALL: into
    // al_.small.  FRESH: free rows in front, the data, the magnitude row, and 256 + padding zero rows behind (the view's
    // 256-row padding reaches further back as the view starts earlier).
    int select_alpha(const int32_t* ids, int64_t n) {
        static const bool no_prepend = getenv("PBVI_NO_ALPHA_PREPEND") != nullptr;      // debug / A-B only
        HIPCHK(hipMemcpyAsync(ids_.p, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        const auto sel = al_.selection(ids, n, !no_prepend);
        if (sel.kind == sel.EXTEND) {
            al_.placed(al_.PRIMARY, al_.off - sel.rows, n);
        } else {
            const bool small = sel.kind == sel.SMALL;
            const size_t rows = (size_t)sel.rows + al_.rows_cap(n) + (small || no_prepend ? 0 : GEMM_BN);
            const int rc = (small ? al_.small : al_.buf).ensure(rows * al_.row_bytes());
            if (rc) return rc;
            al_.placed(small ? al_.BESIDE : no_prepend ? al_.PLAIN : al_.PRIMARY, sel.rows, n);
            HIPCHK(hipMemsetAsync(al_.mag_row(), 0, (rows - (size_t)sel.rows - (size_t)n) * al_.row_bytes(), stream_));
        }
        const int64_t fresh = sel.kind == sel.EXTEND ? sel.rows : n;       // rows to gather: they lead the view
        for (int64_t r0 = 0; r0 < fresh; r0 += 65535) {
            const unsigned c = (unsigned)std::min<int64_t>(65535, fresh - r0);
            hipLaunchKernelGGL(k_gather_rows<T>, dim3((S_pad_ + 255) / 256, c), dim3(256), 0, stream_, store_[0].as<T>(),
                               al_.rows() + (size_t)r0 * S_pad_, S_pad_, ids_.as<int32_t>() + r0);
            HIPCHK(hipGetLastError());
        }
        al_.selected(sel, ids, n);
        return sel.kind == sel.EXTEND ? alpha_installed(al_.rows(), fresh) : alpha_installed();
    }

    // device pointer to the stream-K share size (K-tile steps of the longest f32 chain) or nullptr
    const int* chain_steps() const {
        if (!kF32 || !plan_.streamk) return nullptr;
        return streamk_workspace(plan_, skws_.as<int>()).plan;
    }
    double tie_window(int k_chunk) const {
        if (!kF32) return 0.0;
        if (tie_rel_user_ > 0.0) return tie_rel_user_;
        if (plan_.streamk) return -1.0;            // computed on the device from the stream-K share size
        const double u = 5.9604644775390625e-08;   // 2^-24
        return 8.0 * u * std::sqrt((double)std::max(k_chunk, 1)) + 8.0 * u;
    }

    // score GEMM: C = beliefs[B_pad][S_pad] . Y[rows_y][S_pad]^T -> slabs_.  Y's zero structure:
    // G row groups of v_group rows with support nzB (nullptr = dense Y).
    // scores of X rows (default: the resident belief block) against the rows of Y
    int score_gemm(const T* Y, int64_t rows_y, const uint8_t* nzB, int G, int v_group, SlabView<T>* sv,
                   const T* X = nullptr, int64_t x_rows = 0, const uint8_t* nzX = nullptr, hipStream_t list_stream = nullptr,
                   const FusedB* fused = nullptr, int* split = nullptr /* in: wanted, out: done (scheduler 2d) */,
                   int f64_route = -1 /* fp64 scoring: -1 by this GEMM's shape, 0 the plain kernel, n the MFMA tiles in n K parts */);

    int project_dense(double gamma);   // K1-dense: Gamma = gamma * alpha . D_ao^T as A*O (batched) GEMMs
    // What the pipeline ends with: the backup's decision, or (pbvi_q_values, the rollout's lookahead) the exact Q values
    // behind the refinement -- with the keys in caller order too where the caller asked for them
    enum Mode { MODE_BACKUP, MODE_Q, MODE_Q_BEST };
    int run_backup(double gamma, int flags, pbvi_stats_t* st, Mode mode);
    int backup_run(double gamma, int flags, pbvi_stats_t* st) override { return run_backup(gamma, flags, st, MODE_BACKUP); }
    // The Q mode: it overwrites the stage buffers of an earlier backup, whose result is no longer fetchable afterwards
    int run_q(double gamma, bool want_best) {
        const int rc = run_backup(gamma, 0, nullptr, want_best ? MODE_Q_BEST : MODE_Q);
        have_result_ = have_bk_vmax_ = false;
        return rc;
    }

    // ---- the scoring stage (K1, K2, first-max), runnable on this engine or on an fp64 engine's fp32 screen ---- //
    bool choose_push(int64_t N) const;
    int stage_scores(double gamma, bool use_push, const ScoreIO& io, ScoreStage<T>* out);
    int stage_scores_tiled(double gamma, const ScoreIO& io, int want_split, int64_t Vc, int64_t n_chunks, ScoreStage<T>* out);
    int ensure_exact(DevBuf& b, size_t bytes);

    // ---- one backup, stage by stage; TS is the scorer's precision ---- //
    // What the stages share: each field is set by the stage named and read by the later ones.
    template <typename TS>
    struct Call {
        static constexpr bool windows = sizeof(TS) == 4;              // fp32 scores: tie windows + fp64 re-decision
        static constexpr bool screened = sizeof(TS) != sizeof(T);
        EngineT<TS>& scorer;              // this engine, or its fp32 screen
        double gamma;
        int flags;
        int64_t pairs;                    // B * A * O
        bool use_push, stats;             // belief-side formulation; the caller wants pbvi_stats_t
        bool q_only, q_best;              // MODE_Q / MODE_Q_BEST: finish_q_values ends the call; it writes the keys too
        bool no_side = false;             // side_stream_work: PBVI_NO_SIDE_STREAM
        hipStream_t lists = nullptr;      // side_stream_work: where the GEMM's tile lists may be built, or nullptr
        bool early_wanted = false;        // side_stream_work: run_fetch's provisional decision applies to this call
        ScoreIO io;                       // score
        ScoreStage<TS> sc;
        const int* h_kcount = nullptr;    // score: the page-locked landing area of the GEMM's list lengths, and how many
        size_t n_kcount = 0;
        bool xr_pending = false;          // extra_row_maxima: ev_xr_[1] is still to be waited for
        RefineWork work;                  // refine
        bool speculate = false;           // refine: the deferred counts are read at the end of the call
        int h_cnt[CNT_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};      // all counters in the one read-back that precedes the final sync
    };

    // One backup: `scorer` (this engine, or its fp32 screen) produces scores and first maxima; this engine, which owns
    // the operands in their original precision, decides near-ties, actions and assembles the rows.  The stages follow in the
    // order in which run_pipeline calls them.
    template <typename TS>
    int run_pipeline(EngineT<TS>& scorer, double gamma, int flags, pbvi_stats_t* st, Mode mode) {
        int rc;
        const int64_t N = (int64_t)A_ * O_ * (al_.V + 1) + 2 * A_;   // per (a, o): alpha rows + magnitude row
        const int64_t pairs = blk_.B * A_ * O_;
        if (N > 0x7fffffff || pairs > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "backup_run: A*O*(V+1) or B*A*O exceeds int32");
        Call<TS> c{scorer, gamma, flags, pairs, scorer.choose_push(N), st != nullptr, mode != MODE_BACKUP, mode == MODE_Q_BEST};
        last_formulation_ = c.use_push ? 2 : 1;
        if ((rc = prepare_backup(c))) return rc;
        if ((rc = side_stream_work(c))) return rc;
        if ((rc = score(c))) return rc;
        if ((rc = extra_row_maxima(c))) return rc;
        if ((rc = provisional_decision(c))) return rc;
        if ((rc = refine(c))) return rc;
        if ((rc = hand_over_early_rows(c))) return rc;
        if (c.q_only) return finish_q_values(c);
        if ((rc = decide(c))) return rc;
        if ((rc = speculative_repeat(c))) return rc;
        // 11. what the fetches and the next call need to know about this result
        if (c.windows && dead_count_ < 0) dead_count_ = c.h_cnt[CNT_DEAD];
        full_valid_ = false;
        res_sorted_ = blk_.sorted;
        have_result_ = true;
        have_bk_vmax_ = c.use_push && !c.screened;
        res_B_ = blk_.B;
        res_unique_ = c.h_cnt[CNT_UNIQUE];
        if (st) fill_stats(c, st);
        return PBVI_OK;
    }

    // 1. The buffers of the stages up to the refinement; counters cleared.
    template <typename TS>
    int prepare_backup(Call<TS>& c) {
        int rc;
        if ((rc = best_v_.ensure((size_t)c.pairs * sizeof(int32_t)))) return rc;
        if ((rc = best_score_.ensure((size_t)c.pairs * sizeof(double)))) return rc;
        if ((rc = err_.ensure((size_t)c.pairs * sizeof(double)))) return rc;
        if ((rc = queue_.ensure((size_t)c.pairs * sizeof(int32_t)))) return rc;
        if ((rc = hcand_.ensure((size_t)c.pairs * QCAND * sizeof(int32_t)))) return rc;
        if ((rc = hncand_.ensure((size_t)c.pairs * sizeof(int32_t)))) return rc;
        if ((rc = dead_.ensure((size_t)c.pairs))) return rc;
        if ((rc = rdot_.ensure((size_t)blk_.B * A_ * 2 * sizeof(double)))) return rc;
        if ((rc = aqueue_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if ((rc = acand_.ensure((size_t)blk_.B * A_))) return rc;
        // (the decision's buffers too in front of the scoring stage, which plans Gamma tiling with what is free)
        if (!c.q_only && (rc = fin_.ensure(blk_.B, c.pairs, (size_t)S_ * sizeof(T), blk_.sorted))) return rc;
        if ((rc = keep_.ensure((size_t)blk_.B))) return rc;
        if (c.windows && (rc = out_.reserve(256))) return rc;      // the pinned bounce buffer of the fetches that follow, allocated while the stream is idle
        HIPCHK(hipMemsetAsync(counters_.p, 0, CNT_SLOTS * sizeof(int), stream_));
        HIPCHK(hipEventRecord(ev_[0], stream_));
        return PBVI_OK;
    }

    // 2. Belief-only work (dead triples, b.ER: ~0.1 ms each) on the side stream, beside the projection.
    // (Beside the persistent stream-K GEMM they starve: k_rdot took 3.1 ms there instead of 0.1.)
    template <typename TS>
    int side_stream_work(Call<TS>& c) {
        int rc;
        static const bool no_side = getenv("PBVI_NO_SIDE_STREAM") != nullptr;      // debug / A-B only
        c.no_side = no_side;
        hipStream_t side = no_side ? stream_ : stream2_;
        const int k_tiles = S_pad_ / GEMM_BK;
        HIPCHK(hipEventRecord(ev_fork_, stream_));
        HIPCHK(hipStreamWaitEvent(side, ev_fork_, 0));
        static const bool lists_on_side = getenv("PBVI_LISTS_ON_SIDE") != nullptr;      // debug / A-B only: lists behind k_dead
        c.lists = no_side ? nullptr : (lists_on_side ? side : stream3_);
        // (the tile lists need the block's zero map only: where the block was indexed just now they do not wait for its gather)
        if (c.lists != nullptr && c.lists != side)
            HIPCHK(hipStreamWaitEvent(c.lists, (!c.screened && blk_.ev_nzA != nullptr && blk_.nzA_ver == blk_.ver) ? blk_.ev_nzA : ev_fork_, 0));
        if (c.windows) {   // exact, from the supports of the ORIGINAL operands (an fp32 copy may have flushed tiny values to zero)
            if ((rc = blk_.btl.ensure((size_t)blk_.B * k_tiles * sizeof(int32_t)))) return rc;
            if ((rc = blk_.btc.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
            if ((rc = val_exact_.ensure((size_t)blk_.B * A_ * (1 + O_) * ACTION_SPLIT * sizeof(double)))) return rc;
            // Dead triples and the per-belief tile lists are a function of the belief block and the model alone: computed on
            // the first backup of a block, kept for the following ones (a solve backs a block up once; update_passes > 1,
            // the belief-dominance loops of the notebooks and the benchmark back the same block up again and again).  Like
            // the block's sort order and zero-tile map they index the INPUT; nothing of a backup's result is kept.
            static const bool no_cache = getenv("PBVI_NO_DEAD_CACHE") != nullptr;       // debug / A-B only
            if (blk_.dead_ver != blk_.ver || blk_.tiles_ver != blk_.ver || dead_pairs_ != c.pairs || no_cache) {
                const bool have_flags = blk_.rowflags_ver == blk_.ver && blk_.rowflags.p != nullptr;   // left by the block's indexing pass
                HIPCHK(launch_dead<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, view(), nzBw_.as<unsigned long long>(), k_tiles, dead_.as<uint8_t>(),
                                      blk_.btl.as<int32_t>(), blk_.btc.as<int32_t>(), counters_.as<int>() + CNT_DEAD, side,
                                      have_flags ? blk_.rowflags.as<uint8_t>() : nullptr,
                                      have_flags && blk_.sorted ? blk_.perm.as<int32_t>() : nullptr));
                blk_.tiles_ver = blk_.dead_ver = blk_.ver;
                dead_pairs_ = c.pairs;
                dead_count_ = -1;                                // read back with this call's counters
            }
        }
        if (c.use_push) {   // b . ER[:,a] in f64 (the alpha-side gets it from Gamma's reward rows)
            if ((rc = prd_.ensure((size_t)blk_.B * A_ * sizeof(double)))) return rc;
            HIPCHK(launch_rdot<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, view(), c.windows ? blk_.btl.as<int32_t>() : nullptr,
                                  c.windows ? blk_.btc.as<int32_t>() : nullptr, prd_.as<double>(), side));
        }
        // (run_fetch's provisional pipeline: its counters are cleared here, beside the projection, not in front of its kernels)
        c.early_wanted = c.windows && !c.q_only && early_.rows != nullptr && !(c.flags & PBVI_BELIEF_DOMINANCE) && early_.cap >= blk_.B && !no_side;
        if (c.early_wanted) {
            if ((rc = e_cnt_.ensure(4 * sizeof(int)))) return rc;
            HIPCHK(hipMemsetAsync(e_cnt_.p, 0, 4 * sizeof(int), side));
        }
        HIPCHK(hipEventRecord(ev_join_, side));
        return PBVI_OK;
    }

    // 3. K1, K2 and the first maxima, on the scorer (stage_scores).
    template <typename TS>
    int score(Call<TS>& c) {
        int rc;
        ScoreIO& io = c.io;
        io.best_v = best_v_.as<int32_t>();
        io.best_score = best_score_.as<double>();
        io.err = err_.as<double>();
        io.queue = c.windows ? queue_.as<int32_t>() : nullptr;
        io.qcount = counters_.as<int>() + CNT_QUEUE;
        io.hcand = c.windows ? hcand_.as<int32_t>() : nullptr;
        io.hncand = c.windows ? hncand_.as<int32_t>() : nullptr;
        io.dead = c.windows ? dead_.as<uint8_t>() : nullptr;
        io.prd = c.use_push ? prd_.as<double>() : nullptr;
        io.join = ev_join_;
        io.side = c.lists;
        io.ev = ev_;
        io.stats = c.stats;
        // a screen multiplies operands rounded to fp32 (alpha, belief, RTO: 2^-24 relative each) and gamma in fp32
        io.tol_extra = c.screened ? 4.0 * 5.9604644775390625e-08 : 0.0;
        io.allow_split = !c.screened;
        if (c.windows && !c.use_push && c.scorer.tiling_mode_ != 0) {   // Gamma tiling plans with what is free: the refinement's work
            RefineWork reserve;                                       // lists (the largest buffers of the later stages) come first
            if ((rc = refine_work(c.pairs, al_.V, &reserve))) return rc;
        }
        if ((rc = c.scorer.stage_scores(c.gamma, c.use_push, io, &c.sc))) return rc;
        // List lengths of this GEMM, for the statistics (K5 rebuilds the lists for its own GEMM later): into PAGE-LOCKED memory.
        // (The copy used to land in a std::vector: a device-to-pageable copy is staged by the runtime and holds the host until
        // the GEMM and the argmax in front of it have finished, so nothing behind the argmax was enqueued before then.)
        if (c.stats && (c.windows || c.sc.f64_pairs > 0)) {
            c.n_kcount = c.windows ? (size_t)c.sc.plan.tiles_m * c.sc.plan.tiles_n : (size_t)c.sc.f64_pairs;
            // (no copy into it is pending: every call ends synchronised)
            if (!kc_pin_.ensure(c.n_kcount * sizeof(int), std::max<size_t>(c.n_kcount * 2, 4096) * sizeof(int)))
                FAIL(PBVI_ENOMEM, "pinned buffer for the list lengths");
            c.h_kcount = kc_pin_.as<int>();                                 // (the copy itself is enqueued behind the refinement: hand_over_early_rows)
        }
        return PBVI_OK;
    }

    // 4. Belief side: max_v b.alpha_v of these beliefs from the GEMM's extra rows (exact engines only).
    template <typename TS>
    int extra_row_maxima(Call<TS>& c) {
        if (!c.use_push || c.screened) return PBVI_OK;
        // beside the refinement, on the side stream: a wave per belief row over V scores is 0.1 ms that nothing in this
        // call waits for (the slabs stay as they are until the next GEMM; K5 is not run with this formulation's extras
        // pending -- it joins first, below)
        int rc;
        if ((rc = vmax_bk_.ensure((size_t)blk_.B * sizeof(double)))) return rc;
        hipStream_t xs = c.no_side ? stream_ : stream2_;
        if (xs != stream_) {
            HIPCHK(hipEventRecord(ev_xr_[0], stream_));
            HIPCHK(hipStreamWaitEvent(xs, ev_xr_[0], 0));
        }
        hipLaunchKernelGGL(k_extra_rowmax<TS>, dim3((unsigned)((blk_.B + 3) / 4)), dim3(256), 0, xs, c.sc.sv, c.sc.extra_row0, (int)blk_.B,
                           (int)al_.V, blk_.sorted ? blk_.perm.as<int32_t>() : nullptr, vmax_bk_.as<double>());
        HIPCHK(hipGetLastError());
        if (xs != stream_) {
            HIPCHK(hipEventRecord(ev_xr_[1], xs));
            c.xr_pending = true;
        }
        return PBVI_OK;
    }

    // caller order -> key dedup -> the distinct keys' rows, for the actions in d.act and the keys in best_v_ as they are now.
    // snapshot: best_v_ of an unsorted block is copied, not aliased (the provisional decision: the refinement rewrites it in
    // place).  d.res_act / d.res_best are the actions and keys in caller order.
    int decision_tail(Decision& d, double gamma, bool snapshot) {
        const int AO = A_ * O_;
        d.res_act = d.act.as<int32_t>();
        d.res_best = best_v_.as<int32_t>();
        // results to the caller's belief order, then K6: dedup by (a*, v*) key
        if (blk_.sorted) {
            hipLaunchKernelGGL(k_unpermute, dim3((unsigned)blk_.B), dim3(64), 0, stream_, (int)blk_.B, AO, blk_.perm.as<int32_t>(), d.act.as<int32_t>(),
                               best_v_.as<int32_t>(), d.act_res.as<int32_t>(), d.best_res.as<int32_t>());
            HIPCHK(hipGetLastError());
            d.res_act = d.act_res.as<int32_t>();
            d.res_best = d.best_res.as<int32_t>();
        } else if (snapshot) {                                   // (one row block: the keys as they are now)
            HIPCHK(hipMemcpyAsync(d.best_res.p, best_v_.p, (size_t)blk_.B * AO * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
            d.res_best = d.best_res.as<int32_t>();
        }
        HIPCHK(launch_dedup((int)blk_.B, A_, O_, d.res_act, d.res_best, d.rep.as<int32_t>(), d.uniq.as<int32_t>(), d.inv.as<int32_t>(),
                            d.slot.as<int32_t>(), d.count(), stream_));
        // K3: alpha' rows of the unique keys only
        HIPCHK(launch_assemble<T>(al_.rows(), S_pad_, view(), gamma, d.res_act, d.res_best, d.uniq.as<int32_t>(), d.count(), (int)blk_.B,
                                  d.rows.as<T>(), S_, stream_));
        return PBVI_OK;
    }

    // 5. Early rows (pbvi_backup_run_fetch): the first maxima and the action values they give decide MOST beliefs' keys for
    // good -- the refinement re-decides near-ties only -- so the distinct rows of that provisional decision are assembled
    // and written to the caller's page-locked buffer on the side stream NOW, under the refinement, the action stage and
    // the dedup (the 8 MB of rows used to cross PCIe after all of them: 0.17 ms of a 3 ms backup).  Afterwards the final
    // keys are matched against the provisional ones (k_match_rows): rows already on the host keep their slot, the few
    // that the refinement changed are appended.  Snapshots, because the refinement rewrites best_v / best_score in place.
    template <typename TS>
    int provisional_decision(Call<TS>& c) {
        early_.used = false;
        if (!c.early_wanted) return PBVI_OK;
        int rc;
        if ((rc = prov_.ensure(blk_.B, c.pairs, (size_t)S_ * sizeof(T), true))) return rc;
        if ((rc = e_rdot_.ensure((size_t)blk_.B * A_ * 2 * sizeof(double)))) return rc;
        if ((rc = e_slot_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        for (hipEvent_t& ev : early_.ev) HIPCHK(new_event(&ev, hipEventDisableTiming, "hipEventDestroy(early)"));
        // The provisional decision itself is 40 us of small kernels: they run HERE, on the main stream in front of the
        // refinement (which rewrites best_v / best_score in place), and only the copy -- 8 MB over PCIe, ~150 us, few blocks
        // -- goes to the side stream.  (Snapshots of the three arrays + the whole provisional pipeline beside the
        // refinement cost it 0.13 ms: a net loss.)
        HIPCHK(launch_action<TS>((int)blk_.B, c.scorer.view(), c.sc.sv, c.sc.rd_col0, c.sc.tol_rel, c.sc.chain, best_score_.as<double>(), err_.as<double>(),
                                 e_rdot_.as<double>(), e_rdot_.as<double>() + (size_t)blk_.B * A_, prov_.act.as<int32_t>(), nullptr, nullptr, stream_,
                                 c.io.tol_extra, nullptr, c.sc.split));
        if ((rc = decision_tail(prov_, c.gamma, true))) return rc;
        HIPCHK(hipEventRecord(early_.ev[0], stream_));
        hipStream_t es = stream2_;
        HIPCHK(hipStreamWaitEvent(es, early_.ev[0], 0));
        // The copy is a plain hipMemcpyAsync on the side stream, sized by the host: it waits (hand_over_early_rows, once the
        // refinement is enqueued) for this 4-byte count.  A copy KERNEL storing to the page-locked buffer needs no host and reaches the
        // link's rate (54.7 GB/s, profiles/microbench/pcie_store.hip) -- but beside it k_refine took 0.24 ms instead of 0.14
        // whatever its grid (8 .. 1024 blocks): the runtime's copy disturbs the refinement far less (0.15 ms).
        early_.dma_pending = true;
        HIPCHK(hipMemcpyAsync(&words().provisional, e_cnt_.p, sizeof(int), hipMemcpyDeviceToHost, es));
        HIPCHK(hipEventRecord(early_.ev[0], es));
        early_.used = true;
        return PBVI_OK;
    }

    // the grid-wide passes over what the per-entry pass deferred (rf_counts_, read by the host)
    int refine_deferred(double gamma, const RefineWork& work) {
        HIPCHK(launch_refine_deferred<T>(true, (int)al_.V, A_ * O_, blk_.rows.as<T>(), S_pad_, al_.rows(), S_pad_, view(), gamma,
                                         best_v_.as<int32_t>(), best_score_.as<double>(), err_.as<double>(), work,
                                         rf_counts_[0], rf_counts_[1], stream_));
        return PBVI_OK;
    }

    // 6. fp64 re-decision of near-ties.  The per-entry pass hands entries with many tied candidates on to grid-wide
    // passes whose launch needs the host to know how many there are -- a read-back in the middle of the pipeline
    // (~30 us of idle device).  A value function either has such ties (absorbing goals, unexplored regions: every backup
    // of a solve loop) or it has not (the synthetic sets): after a backup that deferred nothing the next one SPECULATES
    // that it will not either -- the later stages are enqueued at once, the counts are read at the end, and if there was
    // deferred work after all it runs then and the later stages are repeated (speculative_repeat).
    template <typename TS>
    int refine(Call<TS>& c) {
        if (!c.windows) return PBVI_OK;
        int rc;
        RefineWork& work = c.work;
        if ((rc = refine_work(c.pairs, al_.V, &work))) return rc;   // (reserved by `score` already in a tiled call)
        if constexpr (kF32 && !Call<TS>::screened) {
            // Gamma is in HBM as the GEMM read it (projection kernel, not the fused GEMM): the per-entry pass first
            // separates candidates by fp64 sums over those fp32 rows (backup_kernels.h, RefineWork::gam)
            static const bool no_l1 = getenv("PBVI_NO_L1_SCREEN") != nullptr;      // debug / A-B only
            // (not in a tiled call: a chunk's rows are gone by now)
            if (!no_l1 && !c.use_push && !c.sc.fused && c.sc.chunks <= 1 && mode_ == PBVI_SPARSE) {
                work.gam = (const float*)gam_.p;
                work.ldg = S_pad_;
                work.l1_rel = (double)(R_ + 4) * 5.9604644775390625e-08;
            }
        }
        // the candidates k_argmax left for the rows it queued (backup_kernels.h, RefineWork::hcand)
        static const bool no_handover = getenv("PBVI_NO_CAND_HANDOVER") != nullptr;      // debug / A-B only: k_refine scans
        if (!no_handover) {
            work.hcand = c.io.hcand;
            work.hncand = c.io.hncand;
        }
        // the counts land in two of the engine's pinned flag words -- not in the staging buffer: run_fetch stages results
        // through that one before the counts are read, and a Delivery::add may reset or reallocate it
        rf_counts_ = words().deferred;
        rf_counts_[0] = rf_counts_[1] = 0;
        last_work_ = work;                                       // (pbvi_debug_refine_counts)
        have_last_work_ = true;
        static const bool no_spec = getenv("PBVI_NO_SPECULATION") != nullptr;      // debug / A-B only
        // (not with the belief-dominance test: its own value-max refinement re-uses the work-list buffers, so the
        // deferred entries of this one have to be finished first)
        // (nor for pbvi_q_values, whose one stage behind the refinement needs the final best_v)
        c.speculate = !no_spec && !c.q_only && last_deferred_nothing_ && work.items_v != nullptr && !(c.flags & PBVI_BELIEF_DOMINANCE);
        HIPCHK((launch_refine_scan<T, TS>(true, c.sc.sv, (int)al_.V, A_ * O_, (int)c.pairs, queue_.as<int32_t>(), c.io.qcount, blk_.rows.as<T>(), S_pad_,
                                          al_.rows(), S_pad_, view(), c.gamma, blk_.btl.as<int32_t>(), blk_.btc.as<int32_t>(),
                                          nzB_.as<uint8_t>(), best_v_.as<int32_t>(), best_score_.as<double>(), err_.as<double>(),
                                          counters_.as<int>() + CNT_REFINE_CAND, work, rf_counts_, stream_)));
        if (!c.speculate && work.items_v != nullptr) {
            HIPCHK(hipStreamSynchronize(stream_));
            last_deferred_nothing_ = rf_counts_[0] == 0 && rf_counts_[1] == 0;
            if ((rc = refine_deferred(c.gamma, work))) return rc;
        }
        return PBVI_OK;
    }

    // 7. The refinement is enqueued: now the host can wait for the provisional count and send the early rows on their way.
    // Then the list lengths' copy, and the end of the refinement's time.
    template <typename TS>
    int hand_over_early_rows(Call<TS>& c) {
        if (early_.used && early_.dma_pending) {
            HIPCHK(hipEventSynchronize(early_.ev[0]));
            const int np = words().provisional;
            if (np > 0)
                HIPCHK(hipMemcpyAsync(early_.rows, prov_.rows.p, (size_t)np * S_ * sizeof(T), hipMemcpyDeviceToHost, stream2_));
            HIPCHK(hipEventRecord(early_.ev[1], stream2_));
            early_.dma_pending = false;
        }
        if (c.h_kcount != nullptr)   // statistics: not in front of the provisional decision and the refinement (K5 re-uses kcount_ later)
            HIPCHK(hipMemcpyAsync(kc_pin_.p, c.scorer.kcount_.p, c.n_kcount * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipEventRecord(ev_[4], stream_));
        return PBVI_OK;
    }

    // the tile lists of the resident block (blk_.btl / blk_.btc) exist: from the beliefs alone, where k_dead did not leave them
    int ensure_belief_tiles() {
        if (blk_.tiles_ver == blk_.ver) return PBVI_OK;
        int rc;
        const int k_tiles = S_pad_ / GEMM_BK;
        if ((rc = blk_.btl.ensure((size_t)blk_.B * k_tiles * sizeof(int32_t)))) return rc;
        if ((rc = blk_.btc.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        HIPCHK(launch_belief_tiles<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, S_, k_tiles, blk_.btl.as<int32_t>(), blk_.btc.as<int32_t>(), stream_));
        blk_.tiles_ver = blk_.ver;
        return PBVI_OK;
    }

    // The end of every call: the counters (and the overflow flag of a screen) into the page-locked words, one
    // synchronisation, the counters into the call's array.  published: k_publish has stored the words itself, no copy;
    // timed: ev_[7] ends the stage times (pbvi_q_values keeps none).
    int end_call(bool screened, bool published, bool timed, int* h_cnt) {
        PinnedWords* w = &words();
        if (!published) {
            // (into the page-locked words: a copy into the stack array is staged by the runtime)
            HIPCHK(hipMemcpyAsync(w->counters, counters_.p, sizeof(w->counters), hipMemcpyDeviceToHost, stream_));
            // did an alpha value leave the fp32 range when the screen's copy was made?
            if (screened && scr_flag_.p) HIPCHK(hipMemcpyAsync(&w->screen_overflow, scr_flag_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
        }
        if (timed) HIPCHK(hipEventRecord(ev_[7], stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        std::memcpy(h_cnt, w->counters, sizeof(w->counters));
        return PBVI_OK;
    }

    // 8. pbvi_q_values: best_v is final; exact Q of every (belief, action) from it, and nothing else
    template <typename TS>
    int finish_q_values(Call<TS>& c) {
        int rc;
        if (c.xr_pending) HIPCHK(hipStreamWaitEvent(stream_, ev_xr_[1], 0));       // (the side stream still reads this call's slabs)
        if ((rc = ensure_belief_tiles())) return rc;   // pure fp64 scoring: k_dead did not run; the same lists from the beliefs alone
        if ((rc = q_.ensure((size_t)blk_.B * A_ * sizeof(double)))) return rc;
        if ((rc = q_res_.ensure((size_t)blk_.B * A_ * sizeof(double)))) return rc;
        if ((rc = q_act_.ensure((size_t)blk_.B * sizeof(int32_t)))) return rc;
        if (c.q_best && (rc = fin_.best_res.ensure((size_t)c.pairs * sizeof(int32_t)))) return rc;
        HIPCHK(launch_q_exact<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, al_.rows(), S_pad_, (int)al_.V, view(), c.gamma, blk_.btl.as<int32_t>(),
                                 blk_.btc.as<int32_t>(), best_v_.as<int32_t>(), c.windows ? dead_.as<uint8_t>() : nullptr,
                                 blk_.sorted ? blk_.perm.as<int32_t>() : nullptr, q_.as<double>(), q_res_.as<double>(), q_act_.as<int32_t>(),
                                 c.q_best ? fin_.best_res.as<int32_t>() : nullptr, stream_));
        if ((rc = end_call(c.screened, false, false, c.h_cnt))) return rc;
        if (c.windows && dead_count_ < 0) dead_count_ = c.h_cnt[CNT_DEAD];    // k_dead counted this block's dead triples in this call
        return PBVI_OK;
    }

    // 9. The stages behind the refinement: K4 actions, the decision tail (K6, K3), run_fetch's key matching, K5 belief
    // dominance, the small results published or staged, the end of the call.  Run again by speculative_repeat.
    template <typename TS>
    int decide(Call<TS>& c) {
        int rc;
        const int AO = A_ * O_;
        const ScoreStage<TS>& sc = c.sc;
        int* aqcount = counters_.as<int>() + CNT_ACTION_QUEUE;
        bool publish = false;
        // K4: action
        double* rdot_err = rdot_.as<double>() + (size_t)blk_.B * A_;
        HIPCHK(launch_action<TS>((int)blk_.B, c.scorer.view(), sc.sv, sc.rd_col0, sc.tol_rel, sc.chain, best_score_.as<double>(),
                                 err_.as<double>(), rdot_.as<double>(), rdot_err, fin_.act.as<int32_t>(),
                                 c.windows ? aqueue_.as<int32_t>() : nullptr, aqcount, stream_, c.io.tol_extra,
                                 c.windows ? acand_.as<uint8_t>() : nullptr, sc.split));
        if (c.windows)
            HIPCHK(launch_refine_action<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, al_.rows(), S_pad_, view(), c.gamma,
                                           blk_.btl.as<int32_t>(), blk_.btc.as<int32_t>(), aqueue_.as<int32_t>(), aqcount, rdot_.as<double>(), rdot_err, best_v_.as<int32_t>(),
                                           best_score_.as<double>(), err_.as<double>(), val_exact_.as<double>(),
                                           fin_.act.as<int32_t>(), stream_, acand_.as<uint8_t>()));
        HIPCHK(hipEventRecord(ev_[5], stream_));
        if ((rc = decision_tail(fin_, c.gamma, false))) return rc;
        res_action_ = fin_.res_act;
        res_best_ = fin_.res_best;
        if (early_.used) {   // final keys against the provisional ones whose rows are on their way (or there) already
            HIPCHK(hipStreamWaitEvent(stream_, early_.ev[1], 0));          // (the provisional count and rows are complete)
            HIPCHK(hipMemsetAsync(e_cnt_.as<int>() + 1, 0, 2 * sizeof(int), stream_));
            hipLaunchKernelGGL(k_match_rows<T>, dim3((unsigned)std::min<int64_t>(blk_.B, 2048)), dim3(256), 0, stream_, AO, O_, fin_.count(),
                               fin_.uniq.as<int32_t>(), res_action_, res_best_, prov_.uniq.as<int32_t>(), prov_.res_act, prov_.res_best,
                               e_cnt_.as<int>(), (int)early_.cap, e_slot_.as<int32_t>(), fin_.rows.as<T>(), (T*)early_.rows, (int64_t)S_);
            HIPCHK(hipGetLastError());
            const RunFetchDst& d = early_.dst;
            publish = d.slot != nullptr && !(c.flags & PBVI_BELIEF_DOMINANCE) && d.best == nullptr && d.keep == nullptr &&
                      is_pinned_host_pointer(d.slot) && is_pinned_host_pointer(d.index) && is_pinned_host_pointer(d.action);
            if (!publish) HIPCHK(hipMemcpyAsync(words().early, e_cnt_.p, sizeof(words().early), hipMemcpyDeviceToHost, stream_));
        }
        HIPCHK(hipEventRecord(ev_[6], stream_));
        if (c.xr_pending) {                            // the extra rows' maxima read the slabs K5's GEMM is about to overwrite
            HIPCHK(hipStreamWaitEvent(stream_, ev_xr_[1], 0));
            c.xr_pending = false;
        }
        // K5: belief dominance (keep is written in caller order)
        if (c.flags & PBVI_BELIEF_DOMINANCE) {
            if ((rc = value_max_device(resident(), true))) return rc;
            HIPCHK(launch_keep<T>(blk_.rows.as<T>(), S_pad_, fin_.rows.as<T>(), S_, (int)blk_.B, S_, bs2_.as<double>(), fin_.inv.as<int32_t>(),
                                  blk_.sorted ? blk_.perm.as<int32_t>() : nullptr, keep_.as<uint8_t>(), stream_));
        } else {
            HIPCHK(hipMemsetAsync(keep_.p, 1, (size_t)blk_.B, stream_));
        }
        RunFetchDst& dst = early_.dst;
        dst.queued = false;
        if (publish) {                                       // run_fetch into page-locked arrays: one kernel stores everything small
            hipLaunchKernelGGL(k_publish, dim3((unsigned)((blk_.B + 255) / 256)), dim3(256), 0, stream_, (int)blk_.B, e_slot_.as<int32_t>(),
                               fin_.inv.as<int32_t>(), res_action_, (int32_t*)dst.slot, (int32_t*)dst.index, (int32_t*)dst.action,
                               counters_.as<int>(), e_cnt_.as<int>(), (c.screened && scr_flag_.p) ? scr_flag_.as<int>() : nullptr, &words());
            HIPCHK(hipGetLastError());
            dst.queued = true;
        } else if (early_.used && dst.slot != nullptr) {     // run_fetch: slots, index, actions (best, keep) with this read-back
            out_.begin();
            out_.add(dst.slot, e_slot_.p, (size_t)blk_.B * sizeof(int32_t));
            if ((rc = out_add_small((size_t)blk_.B, dst.index, dst.action, dst.best, dst.keep))) return rc;
            dst.queued = true;
        }
        return end_call(c.screened, publish, true, c.h_cnt);
    }

    // 10. A speculating call reads the refinement's counts now: there was deferred work after all -- do it, then the later
    // stages again.
    template <typename TS>
    int speculative_repeat(Call<TS>& c) {
        if (!c.speculate) return PBVI_OK;
        last_deferred_nothing_ = rf_counts_[0] == 0 && rf_counts_[1] == 0;
        if (last_deferred_nothing_) return PBVI_OK;
        int rc;
        if ((rc = refine_deferred(c.gamma, c.work))) return rc;
        HIPCHK(hipMemsetAsync(counters_.as<int>() + CNT_ACTION_QUEUE, 0, sizeof(int), stream_));
        HIPCHK(hipMemsetAsync(counters_.as<int>() + CNT_UNIQUE, 0, sizeof(int), stream_));   // (value_max resets its own queue)
        return decide(c);
    }

    // 12. pbvi_stats_t of the call: stage times from ev_[0..7], counters, the GEMM's tile counts.
    template <typename TS>
    void fill_stats(const Call<TS>& c, pbvi_stats_t* st) const {
        const int AO = A_ * O_;
        const int64_t N = (int64_t)AO * (al_.V + 1) + 2 * A_;
        const ScoreStage<TS>& sc = c.sc;
        const GemmPlan& plan = sc.plan;
        std::memset(st, 0, sizeof(*st));
        auto el = [&](int i, int j) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev_[i], ev_[j]);
            return (double)t;
        };
        st->ms_project = el(0, 1);
        st->ms_score = el(1, 2);
        st->ms_argmax = el(2, 3);
        st->ms_refine = el(3, 4);
        st->ms_action = el(4, 5);
        st->ms_assemble = el(5, 6);
        st->ms_dominance = el(6, 7);
        st->ms_total = el(0, 7);
        st->n_pairs = c.pairs;
        const int* h = c.h_cnt;
        st->n_refine_candidates = h[4];
        st->n_refined = h[0];
        st->n_refined_actions = h[1];
        st->n_unique = h[CNT_UNIQUE];
        st->formulation = last_formulation_;
        st->n_dead = c.windows ? dead_count_ : 0;              // counted by k_dead (when the block was first backed up)
        if (mode_ == PBVI_DENSE) {
            if (kF32) {
                float t = 0.f;
                (void)hipEventElapsedTime(&t, ev_pg_[0], ev_pg_[1]);
                st->ms_project_gemm = (double)t;
            }
            st->project_flops = 2LL * AO * al_.V * (int64_t)S_ * S_;
            st->project_flops_executed = st->project_flops;
            if (kF32) {
                int64_t kt_sum = 0;
                for (int64_t i = 0; i < dense_pairs_ && i < (int64_t)h_kcountD_.size(); ++i) kt_sum += h_kcountD_[(size_t)i];
                st->project_flops_executed = kt_sum * 2LL * GEMM_BM * GEMM_BN * GEMM_BK;
            }
        }
        st->score_flops = 2 * blk_.B * (int64_t)S_ * AO * al_.V;
        int64_t kt_sum = 0;                                  // the GEMM's list lengths (none where it kept no lists)
        for (size_t i = 0; i < c.n_kcount; ++i) kt_sum += c.h_kcount[i];
        if (c.windows) {
            st->score_flops_executed = kt_sum * 2LL * GEMM_BM * GEMM_BN * GEMM_BK;
            st->score_tiles_dense = (int64_t)plan.tiles_m * plan.tiles_n * plan.k_tiles;
            st->score_tiles_run = kt_sum;
            st->split_k = plan.max_chunks;
        } else if (sc.f64_pairs > 0) {   // fp64 MFMA path: 128 x 128 tiles, lists in 32-column steps
            st->score_flops_executed = kt_sum * 2LL * 128 * gemm_f64_bn((int)std::min<int64_t>(c.use_push ? al_.V : N, 0x7fffffff)) * 32;
            st->score_tiles_dense = sc.f64_pairs * (S_pad_ / GEMM_BK);
            st->score_tiles_run = kt_sum;
            st->split_k = 1;
        } else {
            st->score_flops_executed = st->score_flops;
            st->split_k = 1;
        }
        st->screened = c.screened ? 1 : 0;
        st->fused_projection = sc.fused ? 1 : 0;
        st->score_split = sc.split;
        st->gamma_chunks = sc.chunks;
        if (sc.chunks > 1) {                                 // sums over the chunks; the folds count with the argmax
            double fold = 0.0;
            c.scorer.tile_times(ev_[0], &st->ms_project, &st->ms_score, &fold);
            st->ms_argmax = fold + el(2, 3);
        }
    }

    int ensure_screen();
    int sync_screen();

    // per-belief alpha' matrix [B][S] (the reference seam) expanded from the unique rows on first use
    int ensure_full() {
        if (full_valid_) return PBVI_OK;
        int rc = out_full_.ensure((size_t)res_B_ * S_ * sizeof(T));
        if (rc) return rc;
        HIPCHK(launch_expand_rows<T>(fin_.rows.as<T>(), fin_.inv.as<int32_t>(), out_full_.as<T>(), (int)res_B_, S_, stream_));
        full_valid_ = true;
        return PBVI_OK;
    }

    // What every fetch of a backup's results begins with: fails unless one is resident -- with "<who>: no backup result
    // resident", or with `text` where an entry words it differently -- and makes the engine's device current.
    int need_result(const std::string& who, const std::string& text = "") {
        if (!have_result_) FAIL(PBVI_EINVAL, text.empty() ? who + ": no backup result resident" : text);
        HIPCHK(hipSetDevice(device_));
        return PBVI_OK;
    }

    int backup_fetch(void* out_alpha, int32_t* out_action, int32_t* out_best, uint8_t* out_keep) override {
        int rc = need_result("", "backup_fetch: no backup result resident (call pbvi_backup_run first)");
        if (rc) return rc;
        if (out_alpha && (rc = ensure_full())) return rc;
        out_.begin();
        out_.add(out_alpha, out_full_.p, (size_t)res_B_ * S_ * sizeof(T));
        out_add_small((size_t)res_B_, nullptr, out_action, out_best, out_keep);
        return out_.finish();
    }

    // the small per-belief results of the decision, each to where the caller wants it (NULL: not wanted): index into the
    // distinct rows, actions, best_alpha_ind, keep mask.  Into the open transaction; returns its first error.
    int out_add_small(size_t B, int32_t* index, int32_t* action, int32_t* best, uint8_t* keep) {
        out_.add(index, fin_.inv.p, B * sizeof(int32_t));
        out_.add(action, res_action_, B * sizeof(int32_t));
        out_.add(best, res_best_, B * A_ * O_ * sizeof(int32_t));
        return out_.add(keep, keep_.p, B);
    }

    int64_t unique_count() const override { return have_result_ ? res_unique_ : -1; }

    int fetch_unique(void* out_rows, int32_t* out_index) override {
        int rc = need_result("backup_fetch_unique");
        if (rc) return rc;
        return out_.deliver({{out_rows, fin_.rows.p, (size_t)res_unique_ * S_ * sizeof(T)},
                             {out_index, fin_.inv.p, (size_t)res_B_ * sizeof(int32_t)}});
    }

    // everything a caller of backup() needs, in one staged transfer and one synchronisation: the U distinct rows, the
    // per-belief index into them, actions, best_alpha_ind and the keep mask (any destination may be NULL)
    // pbvi_backup_run + pbvi_backup_fetch_compact in one call; the rows go to page-locked `out_rows` in SLOT order
    // (out_slot[u] = row of distinct key u) and most of them leave while the refinement is still running (run_pipeline).
    int run_fetch(double gamma, int flags, pbvi_stats_t* st, void* out_rows, int64_t cap_rows, int32_t* out_slot, int32_t* out_index,
                  int32_t* out_action, int32_t* out_best, uint8_t* out_keep, int64_t* n_unique, int64_t* n_slots) override {
        if (!out_rows || !out_slot || !out_index || !out_action) FAIL(PBVI_EINVAL, "backup_run_fetch: NULL destination");
        if (cap_rows < blk_.B) FAIL(PBVI_EINVAL, "backup_run_fetch: out_rows must have room for one row per belief");
        if (!is_pinned_host_pointer(out_rows)) FAIL(PBVI_EINVAL, "backup_run_fetch: out_rows must be page-locked host memory (pbvi_host_alloc)");
        early_.rows = out_rows;
        early_.cap = cap_rows;
        early_.dst = RunFetchDst{out_slot, out_index, out_action, out_best, out_keep, false};
        int rc = backup_run(gamma, flags, st);
        const bool queued = early_.dst.queued;
        early_.rows = nullptr;                               // (whether or not the backup failed; `used` stays for what follows)
        early_.dst = RunFetchDst{};
        if (rc) return rc;
        int64_t used = res_unique_;
        const bool early_ok = early_.used && !words().early[2];
        if (early_ok) used = (int64_t)words().early[0] + words().early[1];
        // the small arrays came with the pipeline's last read-back (host-side copies of staged items; the stream is idle)
        if (queued && (rc = out_.flush())) return rc;
        if (!queued || !early_ok) {   // the early path did not apply: everything now; the slots overflowed: rows in the plain order
            out_.begin();
            out_.add(out_rows, fin_.rows.p, (size_t)res_unique_ * S_ * sizeof(T));
            if (!queued) out_add_small((size_t)res_B_, out_index, out_action, out_best, out_keep);
            if ((rc = out_.finish())) return rc;
        }
        if (!early_ok)
            for (int64_t u = 0; u < res_unique_; ++u) out_slot[u] = (int32_t)u;
        if (n_unique) *n_unique = res_unique_;
        if (n_slots) *n_slots = used;
        early_.used = false;
        return PBVI_OK;
    }

    int fetch_compact(void* out_rows, int32_t* out_index, int32_t* out_action, int32_t* out_best, uint8_t* out_keep) override {
        int rc = need_result("backup_fetch_compact");
        if (rc) return rc;
        out_.begin();
        out_.add(out_rows, fin_.rows.p, (size_t)res_unique_ * S_ * sizeof(T));
        out_add_small((size_t)res_B_, out_index, out_action, out_best, out_keep);
        return out_.finish();
    }

    // position-weighted bit-pattern hashes of the U distinct rows of the last backup (see k_row_hash)
    int fetch_row_hashes(uint64_t* out) override {
        int rc = need_result("backup_fetch_row_hashes");
        if (rc) return rc;
        if (!out) FAIL(PBVI_EINVAL, "backup_fetch_row_hashes: NULL destination");
        if (res_unique_ <= 0) return PBVI_OK;
        if ((rc = keys_tmp_.ensure((size_t)res_unique_ * sizeof(uint64_t)))) return rc;
        hipLaunchKernelGGL(k_row_hash<T>, dim3((unsigned)res_unique_), dim3(256), 0, stream_, fin_.rows.as<T>(), S_, S_,
                           keys_tmp_.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        return out_.deliver({{out, keys_tmp_.p, (size_t)res_unique_ * sizeof(uint64_t)}});
    }

    // (a*, v*[a*,:]) of every unique row of the last backup: [U][1+O] int32, host or device destination
    int fetch_unique_keys(int32_t* out_keys) override {
        int rc = need_result("backup_fetch_unique_keys");
        if (rc) return rc;
        if (!out_keys) FAIL(PBVI_EINVAL, "backup_fetch_unique_keys: NULL destination");
        if (res_unique_ <= 0) return PBVI_OK;
        if ((rc = keys_tmp_.ensure((size_t)res_unique_ * (1 + O_) * sizeof(int32_t)))) return rc;
        hipLaunchKernelGGL(k_gather_keys, dim3((unsigned)((res_unique_ + 63) / 64)), dim3(64), 0, stream_, (int)res_unique_, A_, O_,
                           fin_.uniq.as<int32_t>(), res_action_, res_best_, keys_tmp_.as<int32_t>());
        HIPCHK(hipGetLastError());
        return out_.deliver({{out_keys, keys_tmp_.p, (size_t)res_unique_ * (1 + O_) * sizeof(int32_t)}});
    }

    // one buffer with everything this rank contributes to the multi-GPU exchange (layout: k_pack_exchange): the kernel
    // writes a device destination itself, a host destination is delivered from keys_tmp_
    int fetch_exchange(int32_t* out, int64_t per) override {
        int rc = need_result("backup_fetch_exchange");
        if (rc) return rc;
        if (!out) FAIL(PBVI_EINVAL, "backup_fetch_exchange: NULL destination");
        if (per < res_B_ || per > 0x7fffffff) FAIL(PBVI_EINVAL, "backup_fetch_exchange: per must be >= the number of beliefs of the last backup");
        const size_t n = 1 + 3 * (size_t)per + (size_t)per * (1 + O_);
        const bool direct = is_device_pointer(out);
        if (!direct && (rc = keys_tmp_.ensure(n * sizeof(int32_t)))) return rc;
        int32_t* dst = direct ? out : keys_tmp_.as<int32_t>();
        hipLaunchKernelGGL(k_pack_exchange, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, stream_, (int)res_B_, (int)per,
                           (int)res_unique_, A_, O_, fin_.inv.as<int32_t>(), res_action_, keep_.as<uint8_t>(), fin_.uniq.as<int32_t>(),
                           res_best_, dst);
        HIPCHK(hipGetLastError());
        out_.begin();               // a host destination of either kind by DMA, as it always was (direct: see Delivery::add_rows)
        if (!direct) out_.add_rows(out, dst, n * sizeof(int32_t), 1, n * sizeof(int32_t), nullptr, true);
        return out_.finish();
    }

    // The head the two assemble entries share: their buffers -- with room for the n rows behind the alpha store's (to_store)
    // or in keys_rows_, *rows / *ld say where -- and the keys (host or device memory) uploaded and scattered into per-row
    // decisions: keys_act_ / keys_best_, what launch_assemble reads; the word behind the n actions counts the keys out of range.
    int keys_to_decisions(int64_t n, const int32_t* keys, bool to_store, T** rows, int* ld) {
        HIPCHK(hipSetDevice(device_));
        int rc;
        if ((rc = keys_tmp_.ensure((size_t)n * (1 + O_) * sizeof(int32_t)))) return rc;
        if ((rc = keys_act_.ensure((size_t)(n + 1) * sizeof(int32_t)))) return rc;      // [n] actions + 1 error counter
        if ((rc = keys_best_.ensure((size_t)n * A_ * O_ * sizeof(int32_t)))) return rc;
        if ((rc = to_store ? store_reserve(0, n, rows) : keys_rows_.ensure((size_t)n * S_ * sizeof(T)))) return rc;
        if (!to_store) *rows = keys_rows_.as<T>();
        *ld = to_store ? S_pad_ : S_;
        int* bad = keys_act_.as<int>() + n;
        HIPCHK(hipMemcpyAsync(keys_tmp_.p, keys, (size_t)n * (1 + O_) * sizeof(int32_t), hipMemcpyDefault, stream_));
        HIPCHK(hipMemsetAsync(bad, 0, sizeof(int), stream_));
        hipLaunchKernelGGL(k_scatter_keys, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream_, (int)n, A_, O_, (int)al_.V,
                           keys_tmp_.as<int32_t>(), keys_act_.as<int32_t>(), keys_best_.as<int32_t>(), bad);
        HIPCHK(hipGetLastError());
        return PBVI_OK;
    }
    // ... and their tail: the n assembled rows (ld elements apart) to out_rows (NULL: not wanted), the count of bad keys with
    // them (direct: see Delivery::add_rows), and the verdict on it
    int deliver_assembled(const char* who, int64_t n, const T* rows, int64_t ld, void* out_rows, bool direct) {
        out_.begin();
        out_.add(&words().bad_key, keys_act_.as<int>() + n, sizeof(int));
        out_.add_rows(out_rows, rows, (size_t)ld * sizeof(T), (size_t)n, (size_t)S_ * sizeof(T), nullptr, direct);
        int rc = out_.finish();
        if (rc) return rc;
        if (words().bad_key) FAIL(PBVI_EINVAL, std::string(who) + ": action or alpha index out of range");
        return PBVI_OK;
    }

    // alpha' rows from keys against the RESIDENT alpha set (K3 of src/pomdp.py:1497-1506 for given winners): what a
    // rank needs to rebuild the rows other ranks found, since the alpha set and the model are replicated.
    int assemble_keys(double gamma, int64_t n, const int32_t* keys, void* out_rows) override {
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "assemble_keys: no alpha set resident");
        if (n <= 0 || n > 65535 || !keys || !out_rows) FAIL(PBVI_EINVAL, "assemble_keys: bad arguments (1 <= n <= 65535)");
        T* rows = nullptr;
        int ld = 0;
        int rc = keys_to_decisions(n, keys, false, &rows, &ld);
        if (rc) return rc;
        HIPCHK(launch_assemble<T>(al_.rows(), S_pad_, view(), gamma, keys_act_.as<int32_t>(), keys_best_.as<int32_t>(), nullptr,
                                  nullptr, (int)n, rows, ld, stream_));
        return deliver_assembled("assemble_keys", n, rows, ld, out_rows, true);
    }

    // Same, and the rows also join the alpha store (ids consecutive from the return value): the sharded backup's
    // "every replica appends the same rows" step, device to device.  out_rows may be NULL.
    int64_t assemble_keys_store(double gamma, int64_t n, const int32_t* keys, void* out_rows) override {
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "assemble_rows_store: no alpha set resident");
        if (n <= 0 || n > 65535 || !keys) FAIL(PBVI_EINVAL, "assemble_rows_store: bad arguments (1 <= n <= 65535)");
        T* dst = nullptr;
        int ld = 0;
        int rc = keys_to_decisions(n, keys, true, &dst, &ld);
        if (rc) return rc;
        if (S_pad_ > S_) HIPCHK(hipMemsetAsync(dst, 0, (size_t)n * S_pad_ * sizeof(T), stream_));   // pad columns stay zero
        HIPCHK(launch_assemble<T>(al_.rows(), S_pad_, view(), gamma, keys_act_.as<int32_t>(), keys_best_.as<int32_t>(), nullptr,
                                  nullptr, (int)n, dst, ld, stream_));
        if ((rc = deliver_assembled("assemble_rows_store", n, dst, ld, out_rows, false))) return rc;
        return store_commit(0, n);
    }

    int device_results(void** d_alpha, int32_t** d_action, uint8_t** d_keep) override {
        int rc = need_result("", "no backup result resident");
        if (rc) return rc;
        if (d_alpha) {
            if ((rc = ensure_full())) return rc;
            HIPCHK(hipStreamSynchronize(stream_));
            *d_alpha = out_full_.p;
        }
        if (d_action) *d_action = const_cast<int32_t*>(res_action_);
        if (d_keep) *d_keep = keep_.as<uint8_t>();
        return PBVI_OK;
    }

    int prune_dominated(uint8_t* keep) override {
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "prune_dominated: no alpha set resident");
        if (!keep) FAIL(PBVI_EINVAL, "prune_dominated: keep is NULL");
        if (al_.V > 4 * 65535) FAIL(PBVI_EUNSUPPORTED, "prune_dominated: at most 262140 alpha-vectors");   // grid.y = ceil(V / 4)
        HIPCHK(hipSetDevice(device_));
        int rc = prune_cnt_.ensure((size_t)al_.V * sizeof(int));
        if (rc) return rc;
        int* h_cnt = nullptr;
        if ((rc = out_.raw((size_t)al_.V * sizeof(int), &h_cnt))) return rc;
        HIPCHK(hipMemsetAsync(prune_cnt_.p, 0, (size_t)al_.V * sizeof(int), stream_));
        HIPCHK(launch_dominated<T>(al_.rows(), S_pad_, (int)al_.V, S_, prune_cnt_.as<int>(), stream_));
        return keep_from_counts(prune_cnt_.as<int>(), h_cnt, keep);
    }
    // Both prunes end here: the V domination counts into pinned memory, and a row is kept iff it was dominated once (by itself)
    int keep_from_counts(const int* d_cnt, int* h_cnt, uint8_t* keep) {
        HIPCHK(hipMemcpyAsync(h_cnt, d_cnt, (size_t)al_.V * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        for (int64_t i = 0; i < al_.V; ++i) keep[i] = (h_cnt[i] == 1) ? 1 : 0;
        return PBVI_OK;
    }

    // The same mask from the pairs that hold at least one new row (k_dominated_rect): exact whenever the rows with
    // is_new == 0 are free of mutual domination, which is NOT checked.  The row list (old rows, then new rows) and the
    // start counts (1 for an old row, which never meets itself; 0 for a new one, which does, once) are built here and
    // travel through the pinned staging buffer in one copy; the counts come back into the same buffer.
    int prune_dominated_masked(const uint8_t* is_new, uint8_t* keep) override {
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "prune_dominated_masked: no alpha set resident");
        if (!is_new) FAIL(PBVI_EINVAL, "prune_dominated_masked: is_new is NULL");
        if (!keep) FAIL(PBVI_EINVAL, "prune_dominated_masked: keep is NULL");
        if (al_.V > 4 * 65535) FAIL(PBVI_EUNSUPPORTED, "prune_dominated_masked: at most 262140 alpha-vectors");   // as prune_dominated
        const int V = (int)al_.V;
        int n_new = 0;
        for (int i = 0; i < V; ++i) n_new += is_new[i] ? 1 : 0;
        if (n_new == 0) {                                    // no pair to test: nothing is launched
            std::memset(keep, 1, (size_t)V);
            return PBVI_OK;
        }
        HIPCHK(hipSetDevice(device_));
        int rc = prune_cnt_.ensure((size_t)2 * V * sizeof(int));
        if (rc) return rc;
        int* h_cnt = nullptr;
        if ((rc = out_.raw((size_t)3 * V * sizeof(int), &h_cnt))) return rc;
        int32_t* h_rows = h_cnt + V;
        int* h_out = h_rows + V;
        const int n_old = V - n_new;
        for (int i = 0, o = 0, f = n_old; i < V; ++i) {
            h_cnt[i] = is_new[i] ? 0 : 1;
            h_rows[is_new[i] ? f++ : o++] = i;
        }
        int* d_cnt = prune_cnt_.as<int>();
        HIPCHK(hipMemcpyAsync(d_cnt, h_cnt, (size_t)2 * V * sizeof(int), hipMemcpyHostToDevice, stream_));
        int piece = 65535;
        if (const char* c = getenv("PBVI_PRUNE_PIECE")) piece = (int)std::min<int64_t>(65535, std::max<int64_t>(1, atoll(c)));   // tests
        HIPCHK(launch_dominated_masked<T>(al_.rows(), S_pad_, S_, d_cnt + V, n_old, n_new, d_cnt, piece, stream_));
        return keep_from_counts(d_cnt, h_out, keep);
    }

    // What value_max_device scores: B rows (the GEMM reads zero rows up to the next multiple of its row block behind
    // them) with their zero map, and the rows' tile lists for the fp64 re-scoring -- nullptr: the resident block's, built
    // where they are missing (ensure_belief_tiles)
    struct Operand {
        const T* rows;
        int64_t B;
        const uint8_t* nzA;
        const int32_t *btl, *btc;
    };
    Operand resident() const { return {blk_.rows.as<T>(), blk_.B, blk_.nzA.as<uint8_t>(), nullptr, nullptr}; }
    // exact (f64-refined) max_v b.alpha_v of the operand's rows into bs2_/bv2_.  need_exact: the caller compares the maxima
    // strictly (K5's keep mask), so an f32 engine re-scores them in fp64 whatever pbvi_set_value_max_exact says
    int value_max_device(const Operand& x, bool need_exact = false);
    void note_vmax_route(int route, int bn, int k_parts, int64_t rows, int64_t pairs) {
        vmax_route_[0] = route;
        vmax_route_[1] = bn;
        vmax_route_[2] = k_parts;
        vmax_route_[3] = rows;
        vmax_route_[4] = al_.V;
        vmax_route_[5] = pairs;
        vmax_route_[6] += 1;
    }

    int value_max(double* out_value, int32_t* out_index) override {
        if (al_.V <= 0 || blk_.B <= 0) FAIL(PBVI_EINVAL, "value_max: need a resident alpha set and belief block");
        HIPCHK(hipSetDevice(device_));
        int rc = value_max_device(resident());
        if (rc) return rc;
        if ((rc = host_perm())) return rc;  // device results are in sorted belief order
        out_.begin();
        out_.add_rows(out_value, bs2_.p, sizeof(double), (size_t)blk_.B, sizeof(double), caller_order());
        out_.add_rows(out_index, bv2_.p, sizeof(int32_t), (size_t)blk_.B, sizeof(int32_t), caller_order());
        return out_.finish();
    }

    // One-step lookahead values of the resident block against the working alpha set: the backup's pipeline up to best_v
    // (run_q), launch_q_exact behind it, results copied out in the caller's belief order.  best_v_ and
    // the other stage buffers are overwritten, so an earlier backup's results are no longer fetchable afterwards.
    int q_values(double gamma, double* out_q, int32_t* out_action, int32_t* out_best) override {
        if (!out_q) FAIL(PBVI_EINVAL, "q_values: NULL out_q");
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "q_values: no alpha set resident (call pbvi_alpha_set)");
        if (blk_.B <= 0) FAIL(PBVI_EINVAL, "q_values: no belief block resident (call pbvi_beliefs_set)");
        if (mode_ != PBVI_SPARSE) FAIL(PBVI_EUNSUPPORTED, "q_values: not available on a PBVI_DENSE engine (create it with PBVI_SPARSE)");
        int rc = run_q(gamma, out_best != nullptr);
        if (rc) return rc;
        return out_.deliver({{out_q, q_res_.p, (size_t)blk_.B * A_ * sizeof(double)},
                             {out_action, q_act_.p, (size_t)blk_.B * sizeof(int32_t)},
                             {out_best, fin_.best_res.p, (size_t)blk_.B * A_ * O_ * sizeof(int32_t)}});
    }

    int64_t store_count(int which) const override { return (which == 0 || which == 1) ? store_rows_[which] : -1; }

    // Grow a buffer to `need` bytes, at least doubling it, keeping its first `used` bytes.  The new allocation is a scoped
    // owner until the kept bytes have arrived: a failure on the way releases it and leaves the buffer and the engine's
    // byte count as they were.  For alpha_append: `alloc` != 0 moves to a new allocation of exactly that size even where the
    // buffer is large enough, the kept bytes come from `src` (default: the start of the buffer), `zero` clears the new
    // allocation first.
    int grow_keep(DevBuf& b, size_t need, size_t used, size_t alloc = 0, const void* src = nullptr, bool zero = false) {
        if (alloc == 0 && need <= b.cap) return PBVI_OK;
        DevBuf nb(mem_, DevBuf::SCOPED);
        int rc = nb.ensure(alloc ? alloc : std::max(need, b.cap * 2));
        if (rc) return rc;
        if (zero) HIPCHK(hipMemsetAsync(nb.p, 0, nb.cap, stream_));
        if (used > 0) HIPCHK(hipMemcpyAsync(nb.p, src ? src : b.p, used, hipMemcpyDeviceToDevice, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        b.take(nb);
        return PBVI_OK;
    }

    // max_v b.alpha_v (exact, like value_max) for rows [0, n) of the BELIEF STORE against the working alpha set, with the
    // store itself as the GEMM operand: no gather, no sort, and the zero maps / tile lists of rows seen before are reused.
    // compute_change (src/pomdp.py:2141-2169) scores the whole accumulated belief set after every backup; that set only
    // grows, and its rows already sit in the store in arrival order (a walk's successive beliefs overlap heavily, so
    // 256-row blocks of the store have tight joint support without sorting).
    int value_max_store(int64_t n, double* out_value, int32_t* out_index) override {
        if (al_.V <= 0) FAIL(PBVI_EINVAL, "value_max_store: no alpha set resident");
        if (n <= 0 || n > store_rows_[1] || (!out_value && !out_index)) FAIL(PBVI_EINVAL, "value_max_store: bad arguments");
        HIPCHK(hipSetDevice(device_));
        int rc;
        const int k_tiles = S_pad_ / GEMM_BK;
        const int64_t have = store_rows_[1], have_pad = round_up(have, GEMM_BM);
        // rows [have, have_pad) are read by the last row block: make them exist and be zero
        if ((size_t)have_pad * S_pad_ * sizeof(T) > store_[1].cap) {
            T* unused = nullptr;
            if ((rc = store_reserve(1, have_pad - have, &unused))) return rc;
        }
        T* base = store_[1].as<T>();
        if (have_pad > have)
            HIPCHK(hipMemsetAsync(base + (size_t)have * S_pad_, 0, (size_t)(have_pad - have) * S_pad_ * sizeof(T), stream_));
        // zero maps: complete blocks computed earlier stay; the block that was partial then and everything after is (re)done
        if ((rc = grow_keep(snz_, (size_t)(have_pad / GEMM_BM) * k_tiles, (size_t)(snz_rows_ / GEMM_BM) * k_tiles))) return rc;
        {
            const int64_t r0 = snz_rows_ / GEMM_BM * GEMM_BM;
            if (have_pad > r0) {
                uint8_t* nz = snz_.as<uint8_t>() + (size_t)(r0 / GEMM_BM) * k_tiles;
                if constexpr (kF32)
                    HIPCHK(launch_tile_nonzero_f32((const float*)(base + (size_t)r0 * S_pad_), S_pad_, (int)(have_pad - r0), k_tiles, nz, stream_));
                else
                    HIPCHK(launch_tile_nonzero_f64((const double*)(base + (size_t)r0 * S_pad_), S_pad_, (int)(have_pad - r0), k_tiles, nz, stream_));
            }
            snz_rows_ = have;
        }
        const bool lists = kF32 && !vmax_skinny();   // per-row tile lists for the f64 refinement
        if (lists) {
            if ((rc = grow_keep(sbtl_, (size_t)have * k_tiles * sizeof(int32_t), (size_t)sbt_rows_ * k_tiles * sizeof(int32_t)))) return rc;
            if ((rc = grow_keep(sbtc_, (size_t)have * sizeof(int32_t), (size_t)sbt_rows_ * sizeof(int32_t)))) return rc;
            for (int64_t r0 = sbt_rows_; r0 < have; r0 += 32768) {
                const int cnt = (int)std::min<int64_t>(32768, have - r0);
                HIPCHK(launch_belief_tiles<T>(base + (size_t)r0 * S_pad_, S_pad_, cnt, S_, k_tiles,
                                              sbtl_.as<int32_t>() + (size_t)r0 * k_tiles, sbtc_.as<int32_t>() + r0, stream_));
            }
            sbt_rows_ = have;
        }
        // value_max_device on windows of the store: each window is the operand, the resident block is not touched
        const int64_t window = 32768;
        rc = PBVI_OK;
        for (int64_t r0 = 0; r0 < n && rc == PBVI_OK; r0 += window) {
            const int64_t cnt = std::min<int64_t>(window, n - r0);
            rc = value_max_device({base + (size_t)r0 * S_pad_, cnt, snz_.as<uint8_t>() + (size_t)(r0 / GEMM_BM) * k_tiles,
                                   lists ? sbtl_.as<int32_t>() + (size_t)r0 * k_tiles : nullptr,
                                   lists ? sbtc_.as<int32_t>() + r0 : nullptr});
            if (rc == PBVI_OK)
                rc = out_.deliver({{out_value ? out_value + r0 : nullptr, bs2_.p, (size_t)cnt * sizeof(double)},
                                   {out_index ? out_index + r0 : nullptr, bv2_.p, (size_t)cnt * sizeof(int32_t)}});
        }
        if (rc != PBVI_OK) (void)hipStreamSynchronize(stream_);
        return rc;
    }

    // Work list of the f64 refinement (see RefineWork): room for every candidate of up to 16M (entry, alpha) pairs
    // and the tile lists of up to 65536 entries; what does not fit is scored by the entry's own block.
    int refine_work(int64_t max_entries, int64_t V, RefineWork* w) {
        static const bool off = getenv("PBVI_REFINE_INBLOCK") != nullptr;     // debug / A-B only
        *w = RefineWork{};
        if (off) return PBVI_OK;
        const int k_tiles = S_pad_ / GEMM_BK;
        // capacities move in powers of two: the alpha set grows by a few rows per backup in a solve loop and a
        // reallocation (hipFree + hipMalloc, both synchronising) per call would cost more than the refinement
        auto pow2 = [](int64_t x, int64_t lo, int64_t hi) {
            int64_t p = lo;
            while (p < x && p < hi) p <<= 1;
            return p;
        };
        int64_t items = pow2(max_entries * V, (int64_t)1 << 16, (int64_t)1 << 24);
        int64_t slots = pow2(max_entries, 1024, 65536);
        if (const char* c = getenv("PBVI_REFINE_ITEM_CAP")) items = std::max<int64_t>(1, atoll(c));   // tests: force the
        if (const char* c = getenv("PBVI_REFINE_SLOT_CAP")) slots = std::max<int64_t>(1, atoll(c));   // overflow paths
        if (items <= 0 || slots <= 0) return PBVI_OK;
        int rc;
        if ((rc = rf_v_.ensure((size_t)items * sizeof(int32_t)))) return rc;
        if ((rc = rf_slot_.ensure((size_t)items * sizeof(int32_t)))) return rc;
        if ((rc = rf_sc_.ensure((size_t)items * sizeof(double)))) return rc;
        if ((rc = rf_entry_.ensure((size_t)slots * sizeof(int32_t)))) return rc;
        if ((rc = rf_n_.ensure((size_t)slots * sizeof(int32_t)))) return rc;
        if ((rc = rf_tiles_.ensure((size_t)slots * k_tiles * sizeof(int32_t)))) return rc;
        const size_t zero_bytes = 16 + (size_t)slots * (sizeof(unsigned long long) + sizeof(int32_t));
        if ((rc = rf_cnt_.ensure(zero_bytes))) return rc;      // [cnt: 16 B][emax][eidx]
        if ((rc = rf_ibv_.ensure((size_t)slots * sizeof(double)))) return rc;
        if ((rc = rf_ibi_.ensure((size_t)slots * sizeof(int32_t)))) return rc;
        w->items_v = rf_v_.as<int32_t>();
        w->items_slot = rf_slot_.as<int32_t>();
        w->scores = rf_sc_.as<double>();
        w->slot_entry = rf_entry_.as<int32_t>();
        w->slot_n = rf_n_.as<int32_t>();
        w->tiles = rf_tiles_.as<int32_t>();
        w->emax = reinterpret_cast<unsigned long long*>(rf_cnt_.as<char>() + 16);
        w->eidx = reinterpret_cast<int32_t*>(rf_cnt_.as<char>() + 16 + (size_t)slots * sizeof(unsigned long long));
        w->zero_bytes = zero_bytes;
        w->ib_val = rf_ibv_.as<double>();
        w->ib_idx = rf_ibi_.as<int32_t>();
        w->cnt = rf_cnt_.as<int>();
        {   // hand-over to k_refine_split (entries the level-1 screen leaves undecided; ~1 % of the queue)
            int64_t q2 = std::min<int64_t>(max_entries, 16384);
            if (const char* c = getenv("PBVI_REFINE_Q2_CAP")) q2 = std::max<int64_t>(1, std::min<int64_t>(q2, atoll(c)));   // tests: force the hand-over's overflow path
            const size_t need = (size_t)q2 * (2 + 8) * sizeof(int32_t);
            if ((rc = rf_q2_.ensure(need))) return rc;
            if ((rc = rf_q2p_.ensure((size_t)q2 * 16 * 8 * sizeof(double)))) return rc;
            if (rf_q2d_.cap < (size_t)q2 * sizeof(int)) {
                if ((rc = rf_q2d_.ensure((size_t)q2 * sizeof(int)))) return rc;
                HIPCHK(hipMemsetAsync(rf_q2d_.p, 0, rf_q2d_.cap, stream_));      // arrival counters: zero between launches
            }
            w->q2_entry = rf_q2_.as<int32_t>();
            w->q2_n = rf_q2_.as<int32_t>() + q2;
            w->q2_cand = rf_q2_.as<int32_t>() + 2 * q2;
            w->q2_part = rf_q2p_.as<double>();
            w->q2_done = rf_q2d_.as<int>();
            w->q2_cap = (int)q2;
        }
        w->item_cap = (int)items;
        w->slot_cap = (int)slots;
        // GEMM path of the tie-heavy entries: fp64 weight rows for as many slots as ~2 GiB holds
        int64_t w_slots = std::min<int64_t>(std::min<int64_t>(slots, 65535),                       // grid.y of the weights kernel
                                            ((int64_t)2 << 30) / ((int64_t)S_pad_ * sizeof(double)));
        if (const char* c = getenv("PBVI_REFINE_DEFER_MIN")) w->defer_min = atoi(c);                 // A/B: -1 = every candidate to the grid-wide pass
        if (const char* c = getenv("PBVI_REFINE_W_SLOTS")) w_slots = std::min<int64_t>(slots, std::max<int64_t>(0, atoll(c)));   // tests
        if (w_slots > 0) {
            if ((rc = build_inverse_lists())) return rc;
            const int kt32 = S_pad_ / GEMM_BK;
            if ((rc = rf_W_.ensure((size_t)w_slots * S_pad_ * sizeof(double)))) return rc;
            if ((rc = rf_Cx_.ensure((size_t)w_slots * V * sizeof(double)))) return rc;
            if ((rc = rf_nzW_.ensure((size_t)((w_slots + 255) / 256) * kt32))) return rc;
            if ((rc = rf_klW_.ensure(gemm_f64_klist_ints((int)w_slots, (int)V, kt32) * sizeof(int)))) return rc;
            if ((rc = rf_kcW_.ensure(gemm_f64_kcount_ints((int)w_slots, (int)V, kt32) * sizeof(int)))) return rc;
            w->W = rf_W_.as<double>();
            w->Cx = rf_Cx_.as<double>();
            w->nzW = rf_nzW_.as<uint8_t>();
            w->klistW = rf_klW_.as<int>();
            w->kcountW = rf_kcW_.as<int>();
            w->in_ptr = in_ptr_.as<int32_t>();
            w->in_src = in_src_.as<int32_t>();
        }
        w->w_slot_cap = (int)w_slots;
        return PBVI_OK;
    }

    // fp32 engines: value-max GEMMs against at most 64 alpha rows take the skinny fp64-accumulating tile (value_max_device)
    bool vmax_skinny() const {
        static const bool off = getenv("PBVI_NO_SKINNY") != nullptr;      // debug / A-B only
        return kF32 && !off && al_.V > 0 && al_.V <= 64 && mode_ == PBVI_SPARSE;
    }
    // automatic score split: from this many dense 256x256x32 tile-steps of the padded score GEMM (C4: 274k)
    static constexpr int64_t kSplitMinSteps = 16384;
    bool split_pays(int64_t n_rows_alloc, int k_tiles) const {
        const int64_t dense_steps = (blk_.B_pad / GEMM_BM) * (n_rows_alloc / GEMM_BN) * (int64_t)k_tiles;
        return dense_steps >= kSplitMinSteps;
    }
    // fp32: bring the resident block's split plane up to date (allocated on first use, rebuilt from blk_.rows when a path that
    // changes blk_.rows did not write it).  false: it does not fit (the caller keeps the fp32 GEMM).  The split kernel addresses
    // 256 rows of the plane with 32-bit byte offsets, hence the bound on S_pad.
    bool split_plane() {
        const size_t bytes = (size_t)blk_.B_pad * S_pad_ * sizeof(float);
        if (bytes == 0 || S_pad_ > (1 << 22)) return false;
        if (blk_.plane.cap < bytes) {
            if (!DevBuf::headroom_ok(mem_.bytes, bytes) || blk_.plane.ensure(bytes) != PBVI_OK) return false;
            blk_.plane_ver = 0;
        }
        if (blk_.plane_ver != blk_.ver) {
            const int64_t n = (int64_t)blk_.B_pad * S_pad_;
            hipLaunchKernelGGL(k_split_plane, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream_, blk_.rows.as<float>(),
                               blk_.plane.as<uint32_t>(), n);
            if (hipGetLastError() != hipSuccess) return false;
            blk_.plane_ver = blk_.ver;
        }
        return true;
    }
    // fp64 engines: MFMA GEMM unless the problem is a handful of tiles (the plain kernel is as good there)
    static bool f64_uses_mfma(int64_t m_rows, int64_t n_rows) {
        static const bool simple = getenv("PBVI_F64_SIMPLE") != nullptr;      // debug / A-B only
        return !simple && m_rows * n_rows >= 64 * 64;
    }

    int set_fused(int enable) override {
        fuse_project_ = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
        if (screen_) screen_->fuse_project_ = fuse_project_;
        return PBVI_OK;
    }
    int set_screen(int mode) override {
        if (mode < 0 || mode > 2) FAIL(PBVI_EINVAL, "set_f64_screen: 0 = never, 1 = automatic, 2 = always");
        screen_mode_ = mode;
        return PBVI_OK;
    }
    int set_score_split(int mode) override {
        if (mode < 0 || mode > 2) FAIL(PBVI_EINVAL, "set_score_split: 0 = never, 1 = automatic, 2 = always");
        split_mode_ = mode;
        return PBVI_OK;
    }
    int set_formulation(int f) override {
        if (f < 0 || f > 2) FAIL(PBVI_EINVAL, "set_formulation: 0 = auto, 1 = project alpha-vectors, 2 = project beliefs");
        formulation_ = f;
        return PBVI_OK;
    }
    // f32 engines: value_max / value_max_store return the fp32 GEMM's maxima as they are (relative error of the order
    // of 1e-7, bounded by the tie window) instead of re-scoring every belief's candidates in fp64.  For callers that
    // only compare values against a tolerance (compute_change); argmax users keep the default.  K5 of a backup is not
    // covered: it passes need_exact to value_max_device.
    int set_value_max_exact(int exact) override {
        vmax_exact_ = exact != 0;
        return PBVI_OK;
    }
    int alpha_layout(int64_t* free_rows, int64_t* layouts) override {
        if (free_rows) *free_rows = al_.on_primary() ? al_.off : 0;
        if (layouts) *layouts = (int64_t)al_.layout_ver;
        return al_.on_primary() ? 1 : 0;
    }

    int set_tie_window(double rel) override {
        tie_rel_user_ = rel;
        return PBVI_OK;
    }
    int set_gamma_tiling(int mode, int64_t chunk_rows) override {
        if (mode < 0 || mode > 2 || chunk_rows < 0)
            FAIL(PBVI_EINVAL, "set_gamma_tiling: mode 0 = never, 1 = automatic, 2 = always; chunk_rows >= 0");
        tiling_mode_ = mode;
        tiling_rows_ = chunk_rows;
        if (screen_) {
            screen_->tiling_mode_ = mode;
            screen_->tiling_rows_ = chunk_rows;
        }
        return PBVI_OK;
    }
    // statistics of a tiled call: kernel times summed over the chunks (events recorded by stage_scores_tiled)
    void tile_times(hipEvent_t first, double* ms_project, double* ms_gemm, double* ms_fold) const {
        *ms_project = *ms_gemm = *ms_fold = 0.0;
        hipEvent_t prev = first;
        for (int c = 0; c < tile_ev_chunks_; ++c) {
            float t[3] = {0.f, 0.f, 0.f};
            (void)hipEventElapsedTime(&t[0], prev, tile_ev_[(size_t)3 * c]);
            (void)hipEventElapsedTime(&t[1], tile_ev_[(size_t)3 * c], tile_ev_[(size_t)3 * c + 1]);
            (void)hipEventElapsedTime(&t[2], tile_ev_[(size_t)3 * c + 1], tile_ev_[(size_t)3 * c + 2]);
            *ms_project += t[0];
            *ms_gemm += t[1];
            *ms_fold += t[2];
            prev = tile_ev_[(size_t)3 * c + 2];
        }
    }
    int64_t device_bytes() const override { return mem_.bytes + (screen_ ? screen_->mem_.bytes : 0); }
};

template <typename T>
int EngineT<T>::score_gemm(const T* Y, int64_t rows_y, const uint8_t* nzB, int G, int v_group, SlabView<T>* sv,
                           const T* X, int64_t x_rows, const uint8_t* nzX, hipStream_t list_stream, const FusedB* fused,
                           int* split, int f64_route) {
    int rc;
    const int64_t m_rows = X ? x_rows : blk_.B;
    const int64_t m_pad = X ? round_up(x_rows, GEMM_BM) : blk_.B_pad;
    const bool own_block = X == nullptr;
    if (!X) {
        X = blk_.rows.as<T>();
        nzX = blk_.nzA.as<uint8_t>();
    }
    if constexpr (kF32) {
        const int64_t n_pad = round_up(rows_y, GEMM_BN);
        if (m_pad > 0x7fffffff || n_pad > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "score_gemm: operand rows exceed int32");
        plan_ = make_gemm_plan((int)m_pad, (int)n_pad, S_pad_);
        const size_t pairs = (size_t)plan_.tiles_m * plan_.tiles_n;
        if ((rc = slabs_.ensure((size_t)plan_.c_floats * sizeof(float)))) return rc;
        slab_bytes_ = (int64_t)plan_.c_floats * (int64_t)sizeof(float);
        if ((rc = klist_.ensure(pairs * plan_.k_tiles * sizeof(int)))) return rc;
        if ((rc = kcount_.ensure(pairs * sizeof(int)))) return rc;
        if ((rc = nchunks_.ensure(pairs * sizeof(int)))) return rc;
        if ((rc = skws_.ensure(streamk_workspace_ints(plan_) * sizeof(int)))) return rc;
        int sp = split != nullptr && *split && plan_.streamk && (fused == nullptr || fused->R == 1) ? 1 : 0;
        if (sp && (!own_block || !split_plane())) sp = 0;      // no plane: the fp32 GEMM (same outputs)
        if (split != nullptr) *split = sp;
        ScoreGemmArgs g;
        g.A = sp ? blk_.plane.as<float>() : (const float*)X;
        g.B = (const float*)Y;
        g.lda = g.ldb = S_pad_;
        g.C = slabs_.as<float>();
        g.plan = plan_;
        g.nzA = nzX;
        g.nzB = nzB;
        g.G = G;
        g.v_group = v_group;
        g.n_rows = (int)rows_y;
        g.klist = klist_.as<int>();
        g.kcount = kcount_.as<int>();
        g.nchunks = nchunks_.as<int>();
        g.stream = stream_;
        g.streamk_ws = skws_.as<int>();
        g.list_stream = list_stream;
        g.list_event = ev_lists_;
        g.fused = fused;
        g.split = sp;
        HIPCHK(launch_score_gemm_f32(g));
        sv->slabs = slabs_.as<T>();
        sv->slab_stride = plan_.slab_stride;
        sv->ldc = plan_.ldc;
        sv->nchunks = nchunks_.as<int>();
        sv->tiles_m = plan_.tiles_m;
        sv->fixed = 0;
        sv->first_block = plan_.streamk ? streamk_workspace(plan_, skws_.as<int>()).first_block : nullptr;
    } else {
        const int kt32s = S_pad_ / GEMM_BK;
        const bool mfma = f64_route < 0 ? f64_uses_mfma(m_rows, rows_y) : f64_route > 0;
        const int split = !mfma ? 1 : f64_route > 0 ? f64_route : gemm_f64_split((int)m_rows, (int)rows_y, kt32s);
        if ((rc = slabs_.ensure((size_t)split * m_rows * rows_y * sizeof(T)))) return rc;
        slab_bytes_ = (int64_t)split * m_rows * rows_y * (int64_t)sizeof(T);
        f64_pairs_ = 0;
        f64_split_ = split;
        if (!mfma) {
            HIPCHK(launch_gemm_nt_simple<T>(X, S_pad_, Y, S_pad_, slabs_.as<T>(), (int)rows_y, (int)m_rows, (int)rows_y,
                                            S_, stream_));
        } else {
            const int kt32 = S_pad_ / GEMM_BK;
            if ((rc = klist_.ensure(gemm_f64_klist_ints((int)m_rows, (int)rows_y, kt32) * sizeof(int)))) return rc;
            if ((rc = kcount_.ensure(gemm_f64_kcount_ints((int)m_rows, (int)rows_y, kt32) * sizeof(int)))) return rc;
            HIPCHK(launch_gemm_nt_f64((const double*)X, S_pad_, (int)m_rows, (const double*)Y, S_pad_, (int)rows_y,
                                      slabs_.as<double>(), (int)rows_y, S_pad_, nzX, nzB, G, v_group, klist_.as<int>(),
                                      kcount_.as<int>(), stream_, split, m_rows * rows_y));
            f64_pairs_ = (int64_t)gemm_f64_pairs((int)m_rows, (int)rows_y);
        }
        sv->slabs = slabs_.as<T>();
        sv->slab_stride = 0;                  // the K parts were folded into the first slab by the launcher
        sv->ldc = (int)rows_y;
        sv->nchunks = nullptr;
        sv->tiles_m = 0;
        sv->fixed = 1;
    }
    return PBVI_OK;
}

template <typename T>
int EngineT<T>::project_dense(double gamma) {
    int rc;
    const int AO = A_ * O_;
    const int64_t Vt = al_.V, Vt_pad = round_up(Vt, GEMM_BM);   // the magnitude row is projected separately below
    int64_t ld_prod, batch_stride;
    if constexpr (kF32) {
        const int64_t n_pad = rows_pad_s_;
        GemmPlan pl = make_gemm_plan((int)Vt_pad, (int)n_pad, S_pad_, /*single_chunk=*/true);
        const size_t pairs = (size_t)pl.tiles_m * pl.tiles_n;
        ld_prod = n_pad;
        batch_stride = Vt_pad * n_pad;
        if ((rc = prod_.ensure((size_t)AO * batch_stride * sizeof(float)))) return rc;
        if ((rc = nzAlpha_.ensure((size_t)pl.tiles_m * pl.k_tiles))) return rc;
        if ((rc = klistD_.ensure((size_t)AO * pairs * pl.k_tiles * sizeof(int)))) return rc;
        if ((rc = kcountD_.ensure((size_t)AO * pairs * sizeof(int)))) return rc;
        if ((rc = nchunksD_.ensure((size_t)AO * pairs * sizeof(int)))) return rc;
        dense_pairs_ = (int64_t)AO * pairs;
        HIPCHK(hipMemsetAsync(prod_.p, 0, (size_t)AO * batch_stride * sizeof(float), stream_));   // pairs with empty lists
        HIPCHK(launch_tile_nonzero_f32((const float*)al_.view.p, S_pad_, (int)Vt_pad, pl.k_tiles, nzAlpha_.as<uint8_t>(), stream_));
        BatchedGemmArgs g;
        g.A = (const float*)al_.view.p;
        g.B = (const float*)dense_.p;
        g.lda = g.ldb = S_pad_;
        g.C = prod_.as<float>();
        g.plan = pl;
        g.nzA = nzAlpha_.as<uint8_t>();
        g.nzB = nzD_.as<uint8_t>();       // per n-tile flags
        g.n_rows = S_;
        g.klist = klistD_.as<int>();
        g.kcount = kcountD_.as<int>();
        g.nchunks = nchunksD_.as<int>();
        g.stream = stream_;
        g.batch = AO;
        g.batch_stride_b = rows_pad_s_ * (int64_t)S_pad_;
        g.batch_stride_c = batch_stride;
        g.ev_before = ev_pg_[0];
        g.ev_after = ev_pg_[1];
        HIPCHK(launch_batched_gemm_f32(g));
    } else {
        ld_prod = S_;
        batch_stride = Vt * S_;
        if ((rc = prod_.ensure((size_t)AO * batch_stride * sizeof(T)))) return rc;
        for (int ao = 0; ao < AO; ++ao)
            HIPCHK(launch_gemm_nt_simple<T>(al_.rows(), S_pad_, dense_.as<T>() + (size_t)ao * rows_pad_s_ * S_pad_, S_pad_,
                                            prod_.as<T>() + (size_t)ao * batch_stride, (int)ld_prod, (int)Vt, S_, S_, stream_));
    }
    dim3 grid((S_ + 255) / 256, (unsigned)Vt, AO);
    hipLaunchKernelGGL(k_scale_rows<T>, grid, dim3(256), 0, stream_, prod_.as<T>(), batch_stride, (int)ld_prod, (int)al_.V,
                       (T)gamma, gam_.as<T>(), S_pad_, S_);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_project_mag<T>, dim3((S_pad_ + 255) / 256, AO), dim3(256), 0, stream_,
                       al_.mag_row(), view(), (T)gamma, gam_.as<T>() + (size_t)AO * al_.V * S_pad_, S_pad_);
    HIPCHK(hipGetLastError());
    return PBVI_OK;
}

template <typename T>
int EngineT<T>::value_max_device(const Operand& x, bool need_exact) {
    int rc;
    const int64_t B = x.B;
    const int64_t Vt = al_.V + 1;   // + magnitude row
    if ((rc = bv2_.ensure((size_t)B * sizeof(int32_t)))) return rc;
    if ((rc = bs2_.ensure((size_t)B * sizeof(double)))) return rc;
    if ((rc = err2_.ensure((size_t)B * sizeof(double)))) return rc;
    if ((rc = queue2_.ensure((size_t)B * sizeof(int32_t)))) return rc;
    int* qc = counters_.as<int>() + CNT_VALUE_MAX_QUEUE;
    HIPCHK(hipMemsetAsync(qc, 0, sizeof(int), stream_));
    if constexpr (kF32) {
        if (vmax_skinny()) {
            // A few dozen alpha rows (compute_change: every known belief against the rows an expansion added): on the
            // 256 x 256 tile of the fp32 engine nine tenths of the MFMA work would be padding and the launch MFMA-bound on
            // it.  The fp64 tile engine's 32- / 64-column variant with both operands widened on the way into LDS streams
            // the belief block once instead -- and its scores are exact products summed in fp64, so there is no tie window
            // and nothing to re-score.
            const int kt32 = S_pad_ / GEMM_BK;
            const int split = gemm_f64_split((int)B, (int)al_.V, kt32);
            const int64_t slab = B * al_.V;
            if ((rc = slabs_.ensure((size_t)split * slab * sizeof(double)))) return rc;
            if ((rc = klist_.ensure(gemm_f64_klist_ints((int)B, (int)al_.V, kt32) * sizeof(int)))) return rc;
            if ((rc = kcount_.ensure(gemm_f64_kcount_ints((int)B, (int)al_.V, kt32) * sizeof(int)))) return rc;
            HIPCHK(launch_gemm_nt_f64_ff32((const float*)x.rows, S_pad_, (int)B, (const float*)al_.view.p, S_pad_, (int)al_.V,
                                           slabs_.as<double>(), (int)al_.V, S_pad_, x.nzA, klist_.as<int>(),
                                           kcount_.as<int>(), stream_, split, slab));
            const SlabView<double> svd = SlabView<double>::single(slabs_.as<double>(), (int)al_.V);   // K parts folded into the first slab by the launcher
            HIPCHK(launch_argmax<double>(svd, (int)al_.V, 1, (int)B, nullptr, 0.0, 0.0, nullptr, 0, bv2_.as<int32_t>(),
                                         bs2_.as<double>(), err2_.as<double>(), nullptr, qc, stream_));
            note_vmax_route(1, gemm_f64_bn((int)al_.V), split, B, (int64_t)gemm_f64_pairs((int)B, (int)al_.V));
            return PBVI_OK;
        }
    }
    SlabView<T> sv;
    if ((rc = score_gemm(al_.rows(), Vt, nullptr, 1, (int)al_.V, &sv, x.rows, B, x.nzA))) return rc;
    const int k_chunk = kF32 ? plan_.chunk_len * GEMM_BK : S_pad_;
    // every belief is re-scored exactly in f32 engines (flag_all): the comparison that
    // follows (new value > old best value) is strict and must not see GEMM rounding.  pbvi_set_value_max_exact(0)
    // lifts that for pbvi_value_max / pbvi_value_max_store only: K5 (need_exact) keeps it
    const bool rescore = kF32 && (vmax_exact_ || need_exact);
    HIPCHK(launch_argmax<T>(sv, (int)al_.V, 1, (int)B, nullptr, tie_window(k_chunk), 0.0, chain_steps(), 1, bv2_.as<int32_t>(),
                            bs2_.as<double>(), err2_.as<double>(), rescore ? queue2_.as<int32_t>() : nullptr, qc, stream_));
    if (rescore) {
        if (x.btl == nullptr && (rc = ensure_belief_tiles())) return rc;   // (the backup's k_dead builds them too)
        const int32_t *btl = x.btl ? x.btl : blk_.btl.as<int32_t>(), *btc = x.btl ? x.btc : blk_.btc.as<int32_t>();
        RefineWork work;
        if ((rc = refine_work(B, al_.V, &work))) return rc;
        last_work_ = work;                                       // (pbvi_debug_refine_counts)
        have_last_work_ = true;
        HIPCHK(launch_refine<T>(false, sv, (int)al_.V, 1, (int)B, queue2_.as<int32_t>(), qc, x.rows, S_pad_,
                                al_.rows(), S_pad_, view(), 0.0, btl, btc, nullptr,
                                bv2_.as<int32_t>(), bs2_.as<double>(), err2_.as<double>(), nullptr, work, stream_));
    }
    if constexpr (kF32)
        note_vmax_route(rescore ? 2 : 3, GEMM_BN, 0, B, (int64_t)plan_.tiles_m * plan_.tiles_n);
    else
        note_vmax_route(f64_pairs_ > 0 ? 4 : 5, f64_pairs_ > 0 ? gemm_f64_bn((int)Vt) : 0, f64_split_, B, f64_pairs_);
    return PBVI_OK;
}

// fp64 -> fp32 copy of operand rows for the screen (round to nearest even, like NumPy's astype)
// *overflow (may be null) is set when a finite value leaves the fp32 range: the screen's scores would be inf / NaN
__global__ void k_narrow(const double* __restrict__ src, float* __restrict__ dst, int64_t n, int* __restrict__ overflow) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    int bad = 0;
    if (i + 3 < n) {
        const double2 a = *(const double2*)(src + i), b = *(const double2*)(src + i + 2);
        const float4 f = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
        *(float4*)(dst + i) = f;
        bad = (isinf(f.x) && !isinf(a.x)) || (isinf(f.y) && !isinf(a.y)) || (isinf(f.z) && !isinf(b.x)) || (isinf(f.w) && !isinf(b.y));
    } else {
        for (int64_t j = i; j < n; ++j) {
            const float f = (float)src[j];
            dst[j] = f;
            bad |= isinf(f) && !isinf(src[j]);
        }
    }
    if (bad && overflow != nullptr) atomicOr(overflow, 1);
}

template <typename T>
bool EngineT<T>::choose_push(int64_t N) const {
    // Which operand is projected through the model (same scores, re-associated):
    //   alpha-side (the reference's order): Gamma = A*O*(V+1)+2A rows, GEMM  [B] x [Gamma rows]
    //   belief-side: bp = B*A*O rows,                                  GEMM  [B*A*O] x [V]
    // The belief side wins when B << V (the solve loop: ~100 new beliefs against thousands of alpha-vectors):
    // fewer rows to project and far less tile padding.  Sparse mode only.
    const int AO = A_ * O_;
    if (mode_ == PBVI_DENSE || (int64_t)blk_.B * AO > 0x7fffffff || !(kF32 || f64_uses_mfma(blk_.B * AO, al_.V))) return false;
    const int64_t bm = kF32 ? GEMM_BM : 128;                       // GEMM tile edge and sustained rate per dtype
    const double rate = kF32 ? 130e12 : 45e12;
    // projection cost per row, measured at C4: the alpha side writes only the Gamma tiles the GEMM will read
    // (0.34 ms for 18450 rows), the belief side writes every row in full and re-reads the inverse lists per
    // belief (2.1 ms for 18432 rows)
    auto cost = [&](int64_t m_rows, int64_t n_rows, int64_t proj_rows, double proj_rate) {
        const double tiles = (double)((m_rows + bm - 1) / bm) * (double)((n_rows + bm - 1) / bm);
        return tiles * S_pad_ * (2.0 * bm * bm / rate) + (double)proj_rows * S_pad_ * sizeof(T) / proj_rate;
    };
    const double c_pull = cost(blk_.B, N, N, 6e12), c_push = cost(blk_.B * AO, al_.V, blk_.B * AO, 1e12);
    if (formulation_ != 0) return formulation_ == 2;
    // Memory before speed: Gamma[A,O,V,S] is what the reference's CuPy path dies allocating (Sea_Robin_Real.ipynb:913,
    // 21.95 GB at |V| = 1386).  Where this engine would have to hold all of it (no fused generation: R > 1, fp64 scoring)
    // and it does not fit beside what the engine already holds while the projected beliefs do, the belief side is taken
    // whatever the cost model says -- its footprint grows with B, which the caller can cut (PBVI_Solver.backup halves the
    // belief block on MemoryError), not with V.
    const bool gamma_compact = kF32 && R_ == 1 && fuse_project_ >= 1 && irr_.p != nullptr;
    const int64_t row = (int64_t)S_pad_ * (int64_t)sizeof(T);
    const int64_t n_pull = kF32 ? round_up(N, GEMM_BN) : N, m_push = round_up((int64_t)blk_.B * AO + blk_.B, GEMM_BM);
    const int64_t gam_new = gamma_compact ? 0 : std::max<int64_t>(0, n_pull * row - (int64_t)gam_.cap);
    // (with Gamma tiling on, the alpha side fits whatever |V| is: the cost model alone decides)
    if (gam_new > ((int64_t)1 << 28) && tiling_mode_ == 0) {
        // the score slabs count too
        auto slabs = [&](int64_t m, int64_t n) {
            if constexpr (kF32) return make_gemm_plan((int)round_up(m, GEMM_BM), (int)round_up(n, GEMM_BN), S_pad_).c_floats * 4;
            else return (int64_t)gemm_f64_split((int)m, (int)n, S_pad_ / GEMM_BK) * m * n * 8;
        };
        const int64_t pull = gam_new + std::max<int64_t>(0, slabs(blk_.B, N) - (int64_t)slabs_.cap);
        const int64_t push = std::max<int64_t>(0, m_push * row - (int64_t)bp_.cap) +
                             std::max<int64_t>(0, slabs((int64_t)blk_.B * AO + blk_.B, al_.V) - (int64_t)slabs_.cap);
        if (push < pull && pull > room()) return true;
    }
    return c_push < 0.8 * c_pull;
}

// K1 + K2 + first-max: projection, score GEMM and the argmax over alpha-vectors with near-tie detection, of THIS
// engine's resident alpha set and belief block (its element type T), into the pipeline buffers `io` names.  Run on
// the engine itself, or -- by an fp64 engine -- on its fp32 screen.
template <typename T>
int EngineT<T>::stage_scores(double gamma, bool use_push, const ScoreIO& io, ScoreStage<T>* out) {
    int rc;
    const int AO = A_ * O_;
    const int64_t Vt = al_.V + 1;                 // alpha rows + magnitude row
    const int64_t N = (int64_t)AO * Vt + 2 * A_;   // Gamma rows: alpha groups, A*O magnitude rows, A reward + A |reward| rows
    const int64_t pairs = blk_.B * AO;
    const ModelView<T> mv = view();
    const int k_tiles = S_pad_ / GEMM_BK;
    const int64_t n_rows_alloc = kF32 ? round_up(N, GEMM_BN) : N;
    // One reachable state per (s, a) -- every large model of the reference -- on an fp32 engine: the score GEMM generates
    // the Gamma tiles that lie inside one (a, o) group itself (gemm.hip, scheduler 2b); only the tiles that straddle two
    // groups and the tail tile are projected ("mat" tiles).  Then only THOSE tiles exist in memory: tile tn of Gamma
    // lives at compact tile ctile[tn] (C4: one tile, 30 MB, instead of 2.24 GB; the reference's CuPy path died
    // allocating Gamma[A,O,V,S], Sea_Robin_Real.ipynb:913).
    // The split bf16 GEMM (gemm.hip, scheduler 2d) for the alpha-side scores of an fp32 engine, unless the caller set its
    // own tie window (defined against the fp32 GEMM) or the device flushes subnormal bf16 operands.  Automatic: by shape
    // only (split_pays), so the fused and the projected route decide alike.  With R > 1 the split takes the projected
    // route: the R > 1 fused kernel (scheduler 2c, never chosen by default) has no split variant.
    int want_split = 0;
    if constexpr (kF32)
        want_split = io.allow_split && !use_push && tie_rel_user_ <= 0.0 && split_supported_ &&
                     (split_mode_ == 2 || (split_mode_ == 1 && split_pays(n_rows_alloc, k_tiles)));
    bool will_fuse = false;
    if constexpr (kF32) {
        static const bool no_fuse = getenv("PBVI_NO_FUSED_PROJECT") != nullptr;     // debug / A-B only
        will_fuse = !use_push && mode_ == PBVI_SPARSE && !no_fuse && irr_.p != nullptr &&
                    (R_ == 1 ? fuse_project_ >= 1 : (R_ <= 7 && fuse_project_ >= 2 && !want_split));
    }
    static const bool no_compact = getenv("PBVI_NO_COMPACT_GAMMA") != nullptr;      // debug / A-B only
    const bool compact = will_fuse && R_ == 1 && !no_compact;
    if (will_fuse) {
        const int tiles_n = (int)(n_rows_alloc / GEMM_BN);
        if (mat_V_ != al_.V || (int)h_mat_.size() != tiles_n) {
            h_mat_.assign((size_t)tiles_n, 0);
            h_ctile_.assign((size_t)tiles_n, -1);
            n_mat_ = 0;
            for (int tn = 0; tn < tiles_n; ++tn) {
                const int64_t r0 = (int64_t)tn * 256, r1 = r0 + 255;
                h_mat_[(size_t)tn] = (r1 >= (int64_t)AO * al_.V || r0 / al_.V != r1 / al_.V) ? 1 : 0;
                if (h_mat_[(size_t)tn]) h_ctile_[(size_t)tn] = n_mat_++;
            }
            // the 4-row blocks of alpha rows the projection still has to visit: those with a row in a
            // projected tile for some group, and the block that holds the magnitude row
            h_vlist_.clear();
            for (int64_t vb = 0; vb * 4 < Vt; ++vb) {
                bool hit = vb * 4 + 4 > al_.V;
                for (int ao = 0; ao < AO && !hit; ++ao)
                    for (int64_t v = vb * 4; v < vb * 4 + 4 && v < al_.V && !hit; ++v) hit = h_mat_[(size_t)((ao * al_.V + v) >> 8)] != 0;
                if (hit) h_vlist_.push_back((int)vb);
            }
            if ((rc = mat_.ensure((size_t)tiles_n))) return rc;
            if ((rc = ctile_.ensure((size_t)tiles_n * sizeof(int32_t)))) return rc;
            if ((rc = vlist_.ensure(h_vlist_.size() * sizeof(int)))) return rc;
            HIPCHK(hipMemcpyAsync(mat_.p, h_mat_.data(), (size_t)tiles_n, hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(ctile_.p, h_ctile_.data(), (size_t)tiles_n * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            HIPCHK(hipMemcpyAsync(vlist_.p, h_vlist_.data(), h_vlist_.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
            mat_V_ = al_.V;
            gam_pad_ptr_ = nullptr;                          // the pad rows sit elsewhere now
        }
    }
    out->chunks = use_push ? 0 : 1;
    if (!use_push && tiling_mode_ != 0 && !will_fuse && mode_ == PBVI_SPARSE) {
        // Gamma tiled over the alpha set?  What this stage may use: the engine's room plus the buffers it would re-allocate,
        // less what the later stages of the call still ask for (early rows, the belief-dominance GEMM's slabs, small
        // buffers; the refinement's work lists were reserved by run_pipeline already).
        const int64_t held = (int64_t)(gam_.cap + slabs_.cap + scores_.cap + klist_.cap);
        const int64_t free_now = room();
        const int64_t avail = free_now > INT64_MAX - held ? INT64_MAX : free_now + held;
        const int64_t reserve = avail / 16 + 2 * blk_.B * (int64_t)S_pad_ * (int64_t)sizeof(T) +
                                (blk_.B_pad * round_up(Vt, GEMM_BN) + (int64_t)512 * 256 * 256) * (int64_t)sizeof(T);
        const int64_t budget = std::max<int64_t>(0, avail - reserve);
        TilingPlan tp;
        bool plan = tiling_mode_ == 2;
        if (tiling_mode_ == 1) plan = tiling_chunk_bytes(S_pad_, AO, A_, blk_.B, kF32, al_.V) > budget;
        if (plan) {
            rc = tiling_plan(S_, A_, O_, al_.V, blk_.B, kF32, budget, tiling_rows_, &tp);
            if (rc == PBVI_EINVAL) FAIL(PBVI_EINVAL, "gamma tiling: shape out of range");
            if (rc == PBVI_ENOMEM && tiling_rows_ == 0)
                FAIL(PBVI_ENOMEM, "gamma tiling: a 4-row chunk and the score matrix need " + std::to_string(tp.bytes) +
                                      " bytes, the engine may still allocate " + std::to_string(budget));
            // (a chunk size the caller named is tried as it is: the planner's figures are upper bounds)
            if (tp.n_chunks > 1) return stage_scores_tiled(gamma, io, want_split, tp.chunk_rows, tp.n_chunks, out);
        }
    }
    if (!use_push) {
        const int64_t rows_held = compact ? (int64_t)n_mat_ * GEMM_BN : n_rows_alloc;
        if ((rc = gam_.ensure((size_t)rows_held * S_pad_ * sizeof(T)))) return rc;
        // zero the Gamma pad rows the GEMM tiles read -- once per (buffer, row count, layout): nothing writes rows >= N,
        // and the fill of up to 255 rows (27 MB, 39 us at |S| = 30000) sat in front of every backup's score GEMM.
        // (Defensive: the pad rows become score columns >= N, which neither k_argmax nor k_fold_chunk reads; a build
        // without the row count in the key answered every sequence of tests/test_engine_sequences.py alike.  The key keeps
        // the rows finite and zero for a reader that may come.)
        if (n_rows_alloc > N && (gam_pad_ptr_ != gam_.p || gam_pad_N_ != N || gam_pad_compact_ != compact || mode_ == PBVI_DENSE)) {
            // (the pad rows are the end of the last tile, which is always a projected one: contiguous in either layout)
            const int64_t first = compact ? (int64_t)(n_mat_ - 1) * GEMM_BN + (N - (n_rows_alloc - GEMM_BN)) : N;
            HIPCHK(hipMemsetAsync(gam_.as<T>() + (size_t)first * S_pad_, 0, (size_t)(n_rows_alloc - N) * S_pad_ * sizeof(T), stream_));
            gam_pad_ptr_ = gam_.p;
            gam_pad_N_ = N;
            gam_pad_compact_ = compact;
        }
    }
    const int32_t* ctile = compact ? ctile_.as<int32_t>() : nullptr;
    SlabView<T> sv;
    out->extra_row0 = -1;
    out->fused = false;
    out->split = 0;
    if (use_push) {
        // K1 (belief side): every belief through every (a, o); K2: [B*A*O] x [V]
        if ((rc = build_inverse_lists())) return rc;
        // B extra rows behind the projected ones: the beliefs themselves, so the same GEMM also yields b . alpha_v --
        // compute_change's max_v b.alpha_v of these beliefs against this alpha set (pbvi_backup_fetch_value_max)
        // rides in the M padding (1800 + 100 rows of 2048 in a solve loop).
        const int64_t M = (int64_t)AO * blk_.B, Mx = M + blk_.B, M_pad = round_up(Mx, GEMM_BM);
        if ((rc = bp_.ensure((size_t)M_pad * S_pad_ * sizeof(T)))) return rc;
        if ((rc = pmag_.ensure((size_t)pairs * sizeof(double)))) return rc;
        if ((rc = nzP_.ensure((size_t)(M_pad / GEMM_BM) * k_tiles))) return rc;
        HIPCHK(hipMemsetAsync(pmag_.p, 0, (size_t)pairs * sizeof(double), stream_));
        HIPCHK(hipMemcpyAsync(bp_.as<T>() + (size_t)M * S_pad_, blk_.rows.p, (size_t)blk_.B * S_pad_ * sizeof(T), hipMemcpyDeviceToDevice, stream_));
        if (M_pad > Mx)
            HIPCHK(hipMemsetAsync(bp_.as<T>() + (size_t)Mx * S_pad_, 0, (size_t)(M_pad - Mx) * S_pad_ * sizeof(T), stream_));
        // the GEMM's zero-tile map of bp: the projection marks the tiles of its own rows while it writes them; only the row
        // tiles that also hold the belief rows / the pad are scanned afterwards (a pass over all of bp was 0.18 ms at the
        // Sea-Robin shape)
        HIPCHK(hipMemsetAsync(nzP_.p, 0, (size_t)(M_pad / GEMM_BM) * k_tiles, stream_));
        HIPCHK(launch_push_project<T>(blk_.rows.as<T>(), S_pad_, (int)blk_.B, mv, in_ptr_.as<int32_t>(), in_src_.as<int32_t>(), gamma,
                                      al_.mag_row(), bp_.as<T>(), S_pad_, pmag_.as<double>(), stream_,
                                      nzP_.as<uint8_t>()));
        {
            const int64_t t0 = M / GEMM_BM;                  // first row tile with a row that is not a projected one
            const T* from = bp_.as<T>() + (size_t)t0 * GEMM_BM * S_pad_;
            uint8_t* to = nzP_.as<uint8_t>() + (size_t)t0 * k_tiles;
            if constexpr (kF32)
                HIPCHK(launch_tile_nonzero_f32((const float*)from, S_pad_, (int)(M_pad - t0 * GEMM_BM), k_tiles, to, stream_));
            else
                HIPCHK(launch_tile_nonzero_f64((const double*)from, S_pad_, (int)(M_pad - t0 * GEMM_BM), k_tiles, to, stream_));
        }
        HIPCHK(hipEventRecord(io.ev[1], stream_));
        if ((rc = score_gemm(al_.rows(), al_.V, nullptr, 1, (int)al_.V, &sv, bp_.as<T>(), Mx, nzP_.as<uint8_t>()))) return rc;
        out->extra_row0 = M;
        sv.push = 1;
        sv.push_B = (int)blk_.B;
        sv.push_A = A_;
        sv.push_O = O_;
        sv.aux_mag = pmag_.as<double>();
        sv.aux_rd = io.prd;
    } else {
        // K1: Gamma projection of the V alpha rows and the magnitude row (only tiles the GEMM will read)
        const uint8_t* need = nullptr;
        FusedB fb{};
        const FusedB* fused = nullptr;
        // f64 engines: the 128-row tiles of their MFMA GEMM nest inside these 256-row ones, so the set is a superset;
        // the plain kernel (tiny problems) reads every Gamma element and needs them all written.
        // (a fused engine projects one or two tiles' worth of rows -- the tiles that straddle groups, the tail: all of their K
        // tiles are written, and the 12 us of k_need_tiles leave the front of every backup)
        if ((kF32 || f64_uses_mfma(blk_.B, N)) && !(will_fuse && R_ == 1)) {
            if ((rc = need_.ensure((size_t)AO * k_tiles))) return rc;
            HIPCHK(launch_need_tiles(blk_.nzA.as<uint8_t>(), (int)(blk_.B_pad / GEMM_BM), nzB_.as<uint8_t>(), AO, (int)al_.V, k_tiles,
                                     need_.as<uint8_t>(), stream_));
            need = need_.as<uint8_t>();
        }
        if (mode_ == PBVI_DENSE) {
            if (Vt > 65535) FAIL(PBVI_EUNSUPPORTED, "dense mode: at most 65534 alpha-vectors");
            // pad columns s >= S of the Gamma rows stay zero: clear them once per run (cheap) -- k_scale_rows writes s < S
            HIPCHK(hipMemsetAsync(gam_.p, 0, (size_t)N * S_pad_ * sizeof(T), stream_));
            if ((rc = project_dense(gamma))) return rc;
            if (kF32 && io.stats) {
                h_kcountD_.resize(kcountD_.cap / sizeof(int));
                HIPCHK(hipMemcpyAsync(h_kcountD_.data(), kcountD_.p, kcountD_.cap, hipMemcpyDeviceToHost, stream_));
            }
        } else {
            if constexpr (kF32) {
                if (will_fuse) {
                    fb.alpha = (const float*)al_.view.p;
                    fb.lda = S_pad_;
                    fb.rs = rs_.as<int32_t>();
                    fb.rto = (const float*)rto_.p;
                    fb.S_pad = S_pad_;
                    fb.O = O_;
                    fb.V = (int)al_.V;
                    fb.R = R_;
                    fb.gamma = (float)gamma;
                    fb.mat = mat_.as<uint8_t>();
                    fb.irr = irr_.as<int32_t>();
                    fb.ctile = ctile;
                    fused = &fb;
                }
            }
            HIPCHK(launch_project<T>(al_.rows(), S_pad_, (int)Vt, mv, (T)gamma, gam_.as<T>(), S_pad_, need, k_tiles, stream_,
                                     fused ? mat_.as<uint8_t>() : nullptr, fused && R_ == 1 ? vlist_.as<int>() : nullptr,
                                     fused && R_ == 1 ? (int)h_vlist_.size() : 0,
                                     fused && R_ > 1 ? irr_.as<int32_t>() : nullptr, ctile));
        }
        HIPCHK(launch_tail_rows<T>(mv, gam_.as<T>(), (int64_t)AO * Vt, S_pad_, stream_, ctile));
        HIPCHK(hipEventRecord(io.ev[1], stream_));
        // K2: scores
        // (its tile lists and stream-K plan are built on the side stream, beside the projection)
        int split = want_split;
        if ((rc = score_gemm(gam_.as<T>(), N, nzB_.as<uint8_t>(), AO, (int)al_.V, &sv, nullptr, 0, nullptr, io.side, fused, &split)))
            return rc;
        out->split = split;
        out->fused = fused != nullptr;
    }
    HIPCHK(hipEventRecord(io.ev[2], stream_));
    HIPCHK(hipStreamWaitEvent(stream_, io.join, 0));       // dead flags + rdot ready
    out->plan = plan_;    // value_max_device (K5) re-plans; keep this GEMM's for the stats
    const int k_chunk = kF32 ? plan_.chunk_len * GEMM_BK : S_pad_;
    out->tol_rel = tie_window(k_chunk);
    out->chain = chain_steps();
    out->rd_col0 = (int64_t)AO * Vt;
    out->f64_pairs = f64_pairs_;
    HIPCHK(launch_argmax<T>(sv, (int)al_.V, AO, (int)blk_.B, io.dead, out->tol_rel, 0.0, out->chain, 0, io.best_v, io.best_score,
                            io.err, io.queue, io.qcount, stream_, io.tol_extra, out->split, io.hcand, io.hncand));
    if (probe_on_ && (rc = probe_capture(sv, io, *out))) return rc;      // tests only (pbvi_debug_score_probe)
    HIPCHK(hipEventRecord(io.ev[3], stream_));
    out->sv = sv;
    return PBVI_OK;
}

// A buffer planned to the byte: DevBuf::ensure gives a buffer that GROWS up to twice the request while there is headroom,
// which the tiling plan did not count.  Released first, it is allocated at exactly `bytes`.
template <typename T>
int EngineT<T>::ensure_exact(DevBuf& b, size_t bytes) {
    if (bytes > b.cap && b.p != nullptr) {
        HIPCHK(hipStreamSynchronize(stream_));
        b.release();
    }
    return b.ensure(bytes);
}

// The alpha-side scoring stage with Gamma tiled over the alpha set (pbvi_set_gamma_tiling): n_chunks chunks of Vc alpha
// rows (the last one ragged).  A chunk of Gamma is exactly the Gamma of a smaller alpha set -- rows [v0, v0 + vc) of
// the view followed by one more row that k_project takes for the magnitude row: the NEXT chunk's first row, whose scores
// nobody reads, or, behind the last chunk, the true max_v |alpha| row over the whole set -- so projection, need map and
// GEMM run as they are on one chunk-sized Gamma buffer, and k_fold_chunk sums each chunk's partial slabs into the
// full-width score matrix.  First-max, tie windows, refinement and the action stage then see ONE matrix: ties across
// chunk seams go to the lowest global index by construction.
template <typename T>
int EngineT<T>::stage_scores_tiled(double gamma, const ScoreIO& io, int want_split, int64_t Vc, int64_t n_chunks,
                                   ScoreStage<T>* out) {
    int rc;
    const int AO = A_ * O_;
    const int64_t Vt = al_.V + 1, N = (int64_t)AO * Vt + 2 * A_;
    const ModelView<T> mv = view();
    const int k_tiles = S_pad_ / GEMM_BK;
    const int64_t ldd = round_up(N, 4);
    if (ldd > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "gamma tiling: score matrix wider than int32");
    // the fold target first (the chunk size was planned beside it), then the buffers of the largest chunk
    if ((rc = ensure_exact(scores_, (size_t)blk_.B * ldd * sizeof(T)))) return rc;
    const int64_t n_big = (int64_t)AO * (Vc + 1) + 2 * A_, rows_big = kF32 ? round_up(n_big, GEMM_BN) : n_big;
    if ((rc = ensure_exact(gam_, (size_t)rows_big * S_pad_ * sizeof(T)))) return rc;
    if constexpr (kF32) {
        if ((rc = ensure_exact(slabs_, (size_t)make_gemm_plan((int)blk_.B_pad, (int)rows_big, S_pad_).c_floats * sizeof(float)))) return rc;
    } else {
        const int sp = f64_uses_mfma(blk_.B, n_big) ? gemm_f64_split((int)blk_.B, (int)n_big, k_tiles) : 1;
        if ((rc = ensure_exact(slabs_, (size_t)sp * blk_.B * n_big * sizeof(T)))) return rc;
    }
    // fp64 scoring has no tie window: copies of an alpha row get equal bits because every column is summed in one order,
    // and the first of them wins.  Left to its own shape, a ragged last chunk may be small enough for the plain kernel, or
    // for another K split, than the chunks before it; a copy behind that seam then differs in its last bits and can win.
    // So the route of the largest chunk is the route of every chunk of the call.
    const bool f64_mfma = !kF32 && f64_uses_mfma(blk_.B, n_big);
    const int f64_route = kF32 ? -1 : f64_mfma ? gemm_f64_split((int)blk_.B, (int)n_big, k_tiles) : 0;
    if ((rc = need_.ensure((size_t)AO * k_tiles))) return rc;
    if ((rc = chain_max_.ensure(sizeof(int)))) return rc;
    HIPCHK(hipMemsetAsync(chain_max_.p, 0, sizeof(int), stream_));
    tile_ev_chunks_ = 0;
    if (io.stats) {
        if ((int64_t)tile_ev_.size() < 3 * n_chunks) tile_ev_.resize((size_t)(3 * n_chunks), nullptr);
        for (auto& e : tile_ev_) HIPCHK(new_event(&e, hipEventDefault, "hipEventDestroy(tile)"));
        tile_ev_chunks_ = (int)n_chunks;
    }
    double tol = 0.0;
    bool on_device = false;                                  // some chunk's window comes from its stream-K share size
    out->split = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t v0 = c * Vc, vc = std::min<int64_t>(Vc, al_.V - v0);
        const bool last = c == n_chunks - 1;
        const int64_t n_c = (int64_t)AO * (vc + 1) + 2 * A_, rows_c = kF32 ? round_up(n_c, GEMM_BN) : n_c;
        // pad rows of this chunk's shape: the (buffer, row count, layout) key covers the ragged last chunk
        if (rows_c > n_c && (gam_pad_ptr_ != gam_.p || gam_pad_N_ != n_c || gam_pad_compact_)) {
            HIPCHK(hipMemsetAsync(gam_.as<T>() + (size_t)n_c * S_pad_, 0, (size_t)(rows_c - n_c) * S_pad_ * sizeof(T), stream_));
            gam_pad_ptr_ = gam_.p;
            gam_pad_N_ = n_c;
            gam_pad_compact_ = false;
        }
        const uint8_t* need = nullptr;
        if (kF32 || f64_mfma) {
            HIPCHK(launch_need_tiles(blk_.nzA.as<uint8_t>(), (int)(blk_.B_pad / GEMM_BM), nzB_.as<uint8_t>(), AO, (int)vc, k_tiles,
                                     need_.as<uint8_t>(), stream_));
            need = need_.as<uint8_t>();
        }
        HIPCHK(launch_project<T>(al_.rows() + (size_t)v0 * S_pad_, S_pad_, (int)(vc + 1), mv, (T)gamma, gam_.as<T>(), S_pad_,
                                 need, k_tiles, stream_));
        HIPCHK(launch_tail_rows<T>(mv, gam_.as<T>(), (int64_t)AO * (vc + 1), S_pad_, stream_, nullptr));
        if (c == 0) HIPCHK(hipEventRecord(io.ev[1], stream_));
        if (io.stats) HIPCHK(hipEventRecord(tile_ev_[(size_t)3 * c], stream_));
        // (tile lists and stream-K plan on the main stream: the list buffers are the previous chunk's GEMM's)
        SlabView<T> sv;
        int split = want_split;
        if ((rc = score_gemm(gam_.as<T>(), n_c, nzB_.as<uint8_t>(), AO, (int)vc, &sv, nullptr, 0, nullptr, nullptr, nullptr, &split,
                             f64_route)))
            return rc;
        if (io.stats) HIPCHK(hipEventRecord(tile_ev_[(size_t)3 * c + 1], stream_));
        if (c > 0 && split != out->split) FAIL(PBVI_ERUNTIME, "gamma tiling: the chunks' GEMMs disagree about the operand split");
        out->split = split;
        const double t = tie_window(kF32 ? plan_.chunk_len * GEMM_BK : S_pad_);
        if (t < 0.0) on_device = true;
        else tol = std::max(tol, t);
        HIPCHK(launch_fold_chunk<T>(sv, (int)blk_.B, AO, (int)vc, (int)al_.V, (int)v0, last ? AO + 2 * A_ : 0, scores_.as<T>(), ldd,
                                    chain_steps(), chain_max_.as<int>(), stream_));
        if (io.stats) HIPCHK(hipEventRecord(tile_ev_[(size_t)3 * c + 2], stream_));
    }
    HIPCHK(hipEventRecord(io.ev[2], stream_));
    HIPCHK(hipStreamWaitEvent(stream_, io.join, 0));       // dead flags + rdot ready
    const SlabView<T> full = SlabView<T>::single(scores_.as<T>(), (int)ldd);
    out->plan = plan_;                                     // (the last chunk's: statistics)
    out->tol_rel = on_device ? -1.0 : tol;                 // the widest window over the chunks
    out->chain = on_device ? chain_max_.as<int>() : nullptr;
    out->rd_col0 = (int64_t)AO * Vt;
    out->extra_row0 = -1;
    out->f64_pairs = f64_pairs_;
    out->fused = false;
    out->chunks = (int)n_chunks;
    HIPCHK(launch_argmax<T>(full, (int)al_.V, AO, (int)blk_.B, io.dead, out->tol_rel, 0.0, out->chain, 0, io.best_v, io.best_score,
                            io.err, io.queue, io.qcount, stream_, io.tol_extra, out->split, io.hcand, io.hncand));
    if (probe_on_ && (rc = probe_capture(full, io, *out))) return rc;    // tests only (pbvi_debug_score_probe)
    HIPCHK(hipEventRecord(io.ev[3], stream_));
    out->sv = full;
    return PBVI_OK;
}

// fp64 engines: an fp32 twin of the model on the same device and streams, used as a SCREEN.  The fp64 MFMA GEMM runs at
// its instruction's ceiling (47.6 TFLOP/s measured) -- a third of the fp32 stream-K GEMM -- and decides
// nothing the fp32 one cannot decide except near-ties.  So the scores are computed in fp32 on rounded copies of the
// operands, with the tie window widened by the input roundings, and every (belief, action, observation) whose winner
// is not clear is re-scored from the fp64 originals (the refinement fp32 engines already have, instantiated for
// double).  Indices and values are those of the pure fp64 path up to its own summation-order noise.
template <typename T>
int EngineT<T>::ensure_screen() {
    if constexpr (kF32) {
        return PBVI_OK;
    } else {
        if (screen_) return PBVI_OK;
        if (h_rto_ref_.empty()) FAIL(PBVI_ERUNTIME, "screen: host tables were not kept");
        std::vector<float> rto32(h_rto_ref_.begin(), h_rto_ref_.end()), er32(h_er_ref_.begin(), h_er_ref_.end());
        auto* e = new (std::nothrow) EngineT<float>();
        if (!e) FAIL(PBVI_ENOMEM, "screen: host allocation failed");
        const int rc = e->init(device_, S_, A_, O_, R_, h_reach_ref_.data(), rto32.data(), er32.data(), PBVI_SPARSE, stream_, stream2_, stream3_);
        if (rc != PBVI_OK) {
            delete e;
            return rc;
        }
        e->formulation_ = formulation_;
        e->fuse_project_ = fuse_project_;
        e->probe_on_ = probe_on_;
        screen_ = e;
        return PBVI_OK;
    }
}

template <typename T>
int EngineT<T>::sync_screen() {
    if constexpr (kF32) {
        return PBVI_OK;
    } else {
        EngineT<float>* sc = screen_;
        int rc;
        if (screen_alpha_seen_.ver != al_.ver) {
            if (!scr_flag_.p) {
                if ((rc = scr_flag_.ensure(sizeof(int)))) return rc;
                HIPCHK(hipMemsetAsync(scr_flag_.p, 0, sizeof(int), stream_));
            }
            auto narrow = [&](int64_t rows) -> int {             // the view's first `rows` rows -> the screen's view
                const int64_t n = rows * S_pad_;
                if (n <= 0) return PBVI_OK;
                hipLaunchKernelGGL(k_narrow, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, stream_, al_.rows(), sc->al_.rows(), n,
                                   scr_flag_.as<int>());
                HIPCHK(hipGetLastError());
                return PBVI_OK;
            };
            // The screen's copy mirrors this engine's layout row for row (same free rows in front of a primary set), so a
            // set that grew at the front costs the fp32 copy its new rows only.  (The screen never selects by itself.)
            const bool prim = al_.on_primary();
            const int64_t off = prim ? al_.off : 0, V = al_.V;
            const auto where = prim ? sc->al_.PRIMARY_ORPHAN : sc->al_.PLAIN;
            const size_t rows_total = prim ? al_.buf.cap / al_.row_bytes() : al_.rows_cap(V);
            if (prim && screen_alpha_seen_.layout_ver == al_.layout_ver && screen_alpha_seen_.off >= off &&
                sc->al_.buf.cap >= rows_total * sc->al_.row_bytes()) {
                const int64_t k = screen_alpha_seen_.off - off;
                sc->al_.placed(where, off, V);
                if ((rc = narrow(k))) return rc;
                if ((rc = sc->alpha_installed(sc->al_.rows(), k))) return rc;
            } else {
                if ((rc = sc->al_.buf.ensure(rows_total * sc->al_.row_bytes()))) return rc;
                sc->al_.placed(where, off, V);
                HIPCHK(hipMemsetAsync(scr_flag_.p, 0, sizeof(int), stream_));        // a fresh copy: no row has overflowed yet
                if ((rc = narrow(V))) return rc;
                HIPCHK(hipMemsetAsync(sc->al_.mag_row(), 0, (rows_total - (size_t)off - (size_t)V) * sc->al_.row_bytes(), stream_));
                if ((rc = sc->alpha_installed())) return rc;
            }
            screen_alpha_seen_ = {al_.ver, prim ? al_.layout_ver : 0, off};      // layout 0: no primary layout is mirrored
        }
        if (screen_bel_seen_ != blk_.ver) {
            const int k_tiles = S_pad_ / GEMM_BK;
            if ((rc = sc->blk_.rows.ensure((size_t)blk_.B_pad * S_pad_ * sizeof(float)))) return rc;
            if ((rc = sc->blk_.nzA.ensure((size_t)(blk_.B_pad / GEMM_BM) * k_tiles))) return rc;
            const int64_t n = (int64_t)blk_.B_pad * S_pad_;      // same row order as this engine's block (pad rows are zero)
            hipLaunchKernelGGL(k_narrow, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, stream_, blk_.rows.as<double>(),
                               sc->blk_.rows.template as<float>(), n, (int*)nullptr);
            HIPCHK(hipGetLastError());
            HIPCHK(launch_tile_nonzero_f32(sc->blk_.rows.template as<float>(), S_pad_, (int)blk_.B_pad, k_tiles, sc->blk_.nzA.template as<uint8_t>(), stream_));
            sc->blk_.replaced(blk_.B, blk_.B_pad, false);
            sc->have_result_ = false;
            screen_bel_seen_ = blk_.ver;
        }
        sc->formulation_ = formulation_;
        sc->tie_rel_user_ = tie_rel_user_;
        sc->tiling_mode_ = tiling_mode_;
        sc->tiling_rows_ = tiling_rows_;
        return PBVI_OK;
    }
}

template <typename T>
int EngineT<T>::run_backup(double gamma, int flags, pbvi_stats_t* st, Mode mode) {
    if (al_.V <= 0) FAIL(PBVI_EINVAL, "backup_run: no alpha set resident (call pbvi_alpha_set)");
    if (blk_.B <= 0) FAIL(PBVI_EINVAL, "backup_run: no belief block resident (call pbvi_beliefs_set)");
    HIPCHK(hipSetDevice(device_));
    if constexpr (!kF32) {
        const int64_t N = (int64_t)A_ * O_ * (al_.V + 1) + 2 * A_;
        // worth it once the score GEMM is more than a few tiles (tiger, the 4x3 grid, S = 600 models stay pure fp64)
        const double gemm_flops = 2.0 * (double)round_up(blk_.B, 128) * (double)N * (double)S_pad_;   // ~0.4 ms of fp64 MFMA
        const bool want = screen_mode_ == 2 || (screen_mode_ == 1 && f64_uses_mfma(blk_.B, N) && gemm_flops >= 2e10);
        if (want && mode_ == PBVI_SPARSE && !h_rto_ref_.empty()) {
            int rc = ensure_screen();
            if (rc) return rc;
            if ((rc = sync_screen())) return rc;
            words().screen_overflow = 0;
            if ((rc = run_pipeline<float>(*screen_, gamma, flags, st, mode))) return rc;
            // |alpha| beyond FLT_MAX became inf in the screen's copy (NaN scores follow): the fp64 pipeline decides alone
            if (words().screen_overflow) return run_pipeline<T>(*this, gamma, flags, st, mode);
            return PBVI_OK;
        }
    }
    return run_pipeline<T>(*this, gamma, flags, st, mode);
}

// --------------------------------------------------------------------------- //
// The handle-free sweep entries (include/pbvi_hip.h; kernels in sweep_kernels.hip): MDP value iteration, the Fast Informed
// Bound and finite-state controller evaluation.  Each takes the model tables, sweeps on device buffers of its own and
// leaves nothing behind.
//
// The model tables as the sweep kernels read them: from the caller's [S][A][..] order to rs [A][R][S], rto [A][O][R][S],
// er [A][S], so that with s across the lanes every table load is coalesced (the MDP's transition probabilities are an rto
// with O = 1).  Host work only.  False (and nothing to use) when a reachable state lies outside [0, S).
// --------------------------------------------------------------------------- //
struct SweepTables {
    std::vector<int32_t> rs;
    std::vector<double> rto, er;
};
static bool retile_sweep_tables(int S, int A, int O, int R, const int32_t* rs, const double* rto, const double* er,
                                SweepTables& t) {
    t.rs.resize((size_t)S * A * R);
    t.rto.resize((size_t)S * A * R * O);
    t.er.resize((size_t)S * A);
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a) {
            t.er[(size_t)a * S + s] = er[(size_t)s * A + a];
            for (int r = 0; r < R; ++r) {
                const size_t src = ((size_t)s * A + a) * R + r;
                if (rs[src] < 0 || rs[src] >= S) return false;
                t.rs[((size_t)a * R + r) * S + s] = rs[src];
            }
            for (int o = 0; o < O; ++o)
                for (int r = 0; r < R; ++r)
                    t.rto[(((size_t)a * O + o) * R + r) * S + s] = rto[(((size_t)s * A + a) * O + o) * R + r];
        }
    return true;
}

// --------------------------------------------------------------------------- //
// One run of sweeps: the stream, the device memory and the per-sweep changes of one call of a sweep entry.  The entry
// declares its DevBufs on `mem` behind the run (so they are released before the stream is destroyed), then: open, sweep,
// fetch the result, report.  The host memory an upload reads must outlive the run.
// --------------------------------------------------------------------------- //
struct SweepRun {
    struct Alloc {                                           // src: host memory to upload, or nullptr (allocated only)
        DevBuf& buf;
        size_t bytes;
        const void* src;
    };
    struct Guard {                                           // (in front of the buffers: they are released first)
        hipStream_t st = nullptr;
        ~Guard() {
            if (st) (void)hipStreamDestroy(st);
        }
    } guard;
    DevMem mem;
    DevBuf d_changes{mem};                                   // [max(horizon, 1)]: changes[it] = largest change of sweep it
    std::vector<double> changes;                             // its host mirror
    int done = 0;                                            // sweeps that ran

    // Every allocation is made before the first copy is enqueued: an out-of-memory return leaves no copy in flight.
    int open(int device, int horizon, std::initializer_list<Alloc> bufs) {
        HIPCHK(hipSetDevice(device));
        const size_t ch_bytes = (size_t)std::max(horizon, 1) * sizeof(double);
        int rc;
        for (const Alloc& a : bufs)
            if ((rc = a.buf.ensure(a.bytes))) return rc;
        if ((rc = d_changes.ensure(ch_bytes))) return rc;
        HIPCHK(hipStreamCreateWithFlags(&guard.st, hipStreamNonBlocking));
        for (const Alloc& a : bufs)
            if (a.src) HIPCHK(hipMemcpyAsync(a.buf.p, a.src, a.bytes, hipMemcpyHostToDevice, guard.st));
        HIPCHK(hipMemsetAsync(d_changes.p, 0, ch_bytes, guard.st));
        changes.assign((size_t)std::max(horizon, 1), 0.0);
        return PBVI_OK;
    }
    // Up to `horizon` sweeps, `launch(it, stream)` enqueues sweep it.  Sweeps go out in batches of 64 with one read-back of
    // their changes per batch; the first change below `limit` ends the run (the sweeps enqueued behind it left at once).
    template <typename Launch>
    int sweep(int horizon, double limit, Launch&& launch) {
        bool converged = false;
        const int batch = 64;
        for (int it0 = 0; it0 < horizon && !converged; it0 += batch) {
            const int it1 = std::min(horizon, it0 + batch);
            for (int it = it0; it < it1; ++it) HIPCHK(launch(it, guard.st));
            HIPCHK(hipMemcpyAsync(changes.data() + it0, d_changes.as<double>() + it0, (size_t)(it1 - it0) * sizeof(double),
                                  hipMemcpyDeviceToHost, guard.st));
            HIPCHK(hipStreamSynchronize(guard.st));
            for (int it = it0; it < it1; ++it) {
                done = it + 1;
                if (changes[(size_t)it] < limit) {
                    converged = true;
                    break;
                }
            }
        }
        return PBVI_OK;
    }
    int fetch(void* dst, const DevBuf& src, size_t bytes) {
        HIPCHK(hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, guard.st));
        HIPCHK(hipStreamSynchronize(guard.st));
        return PBVI_OK;
    }
    void report(double* out_changes, int32_t* out_iterations) const {
        if (out_changes)
            for (int it = 0; it < done; ++it) out_changes[it] = changes[(size_t)it];
        if (out_iterations) *out_iterations = done;
    }
};

// MDP value iteration (VI_Solver.solve, src/mdp.py:1485-1510).  The rows are zeroed before the first sweep: that is
// what horizon = 0 returns.
static int mdp_value_iteration(int device, int S, int A, int R, const int32_t* rs, const double* prob, const double* er,
                               const double* v0, double gamma, double limit, int horizon, double* out_rows,
                               double* out_changes, int32_t* out_iterations) {
    if (S <= 0 || A <= 0 || R <= 0 || horizon < 0 || !rs || !prob || !er || !v0 || !out_rows)
        FAIL(PBVI_EINVAL, "mdp_value_iteration: bad arguments");
    if ((int64_t)S * A * R > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "mdp_value_iteration: S*A*R exceeds int32");
    const size_t n = (size_t)S * A * R, n_rows = (size_t)S * A;
    SweepTables h;
    if (!retile_sweep_tables(S, A, 1, R, rs, prob, er, h)) FAIL(PBVI_EINVAL, "mdp_value_iteration: reachable state out of range");
    SweepRun run;
    DevBuf d_rs{run.mem}, d_p{run.mem}, d_er{run.mem}, d_v[2]{{run.mem}, {run.mem}}, d_rows{run.mem};
    int rc;
    if ((rc = run.open(device, horizon, {{d_rs, n * sizeof(int32_t), h.rs.data()},
                                         {d_p, n * sizeof(double), h.rto.data()},
                                         {d_er, n_rows * sizeof(double), h.er.data()},
                                         {d_v[0], (size_t)S * sizeof(double), v0},
                                         {d_v[1], (size_t)S * sizeof(double), nullptr},
                                         {d_rows, n_rows * sizeof(double), nullptr}})))
        return rc;
    HIPCHK(hipMemsetAsync(d_rows.p, 0, n_rows * sizeof(double), run.guard.st));
    ViSweep vs{};
    vs.S = S, vs.A = A, vs.O = 1, vs.R = R;
    vs.rs = d_rs.as<int32_t>(), vs.rto = d_p.as<double>(), vs.er = d_er.as<double>();
    vs.gamma = gamma, vs.limit = limit, vs.changes = run.d_changes.as<double>(), vs.rows = d_rows.as<double>();
    if ((rc = run.sweep(horizon, limit, [&](int it, hipStream_t st) {
            vs.it = it, vs.v_in = d_v[it & 1].as<double>(), vs.v_out = d_v[(it + 1) & 1].as<double>();
            return launch_vi_sweep(vs, st);
        })))
        return rc;
    if ((rc = run.fetch(out_rows, d_rows, n_rows * sizeof(double)))) return rc;
    run.report(out_changes, out_iterations);
    return PBVI_OK;
}

// Fast Informed Bound (Hauskrecht 2000).  The two Q buffers are state-major [S][A] on the device (k_fib_sweep), action-major
// [A][S] at the caller.
static int fib_value_iteration(int device, int S, int A, int O, int R, const int32_t* rs, const double* rto, const double* er,
                               const double* q0, double gamma, double limit, int horizon, double* out_rows,
                               double* out_changes, int32_t* out_iterations) {
    if (S <= 0 || A <= 0 || O <= 0 || R <= 0 || horizon < 0 || !rs || !rto || !er || !q0 || !out_rows)
        FAIL(PBVI_EINVAL, "fib_value_iteration: bad arguments");
    if ((int64_t)S * A * O * R > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "fib_value_iteration: S*A*O*R exceeds int32");
    const size_t n_rs = (size_t)S * A * R, n_rto = n_rs * O, n_q = (size_t)S * A;
    SweepTables h;
    if (!retile_sweep_tables(S, A, O, R, rs, rto, er, h)) FAIL(PBVI_EINVAL, "fib_value_iteration: reachable state out of range");
    if (horizon == 0) {                                      // nothing to sweep: q0 comes back as it is
        memcpy(out_rows, q0, n_q * sizeof(double));
        if (out_iterations) *out_iterations = 0;
        return PBVI_OK;
    }
    std::vector<double> h_q(n_q);
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a) h_q[(size_t)s * A + a] = q0[(size_t)a * S + s];
    SweepRun run;
    DevBuf d_rs{run.mem}, d_rto{run.mem}, d_er{run.mem}, d_q[2]{{run.mem}, {run.mem}};
    int rc;
    if ((rc = run.open(device, horizon, {{d_rs, n_rs * sizeof(int32_t), h.rs.data()},
                                         {d_rto, n_rto * sizeof(double), h.rto.data()},
                                         {d_er, n_q * sizeof(double), h.er.data()},
                                         {d_q[0], n_q * sizeof(double), h_q.data()},
                                         {d_q[1], n_q * sizeof(double), nullptr}})))
        return rc;
    FibSweep fs{};
    fs.S = S, fs.A = A, fs.O = O, fs.R = R;
    fs.rs = d_rs.as<int32_t>(), fs.rto = d_rto.as<double>(), fs.er = d_er.as<double>();
    fs.gamma = gamma, fs.limit = limit, fs.changes = run.d_changes.as<double>();
    if ((rc = run.sweep(horizon, limit, [&](int it, hipStream_t st) {
            fs.it = it, fs.q_in = d_q[it & 1].as<double>(), fs.q_out = d_q[(it + 1) & 1].as<double>();
            return launch_fib_sweep(fs, st);
        })))
        return rc;
    // sweep done-1 was the last to write: its Q is in buffer done & 1 (the sweeps enqueued after it left at once)
    if ((rc = run.fetch(h_q.data(), d_q[run.done & 1], n_q * sizeof(double)))) return rc;
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a) out_rows[(size_t)a * S + s] = h_q[(size_t)s * A + a];
    run.report(out_changes, out_iterations);
    return PBVI_OK;
}

// --------------------------------------------------------------------------- //
// Finite-state controller evaluation: Jacobi sweeps of
//   V'[n][s] = ER[s,a_n] + gamma * sum_o sum_r RTO[s,a_n,o,r] * V[succ[n][o]][rs[s,a_n,r]]
// The nodes run on the device in the order of their actions (stable; rows and successors are renumbered on the way in
// and the rows put back on the way out), so that nodes which share an action, and with it every table element, are
// neighbours a register tile can cover.  A sweep does not depend on the numbering of the nodes: the result is the same,
// bit for bit.
// --------------------------------------------------------------------------- //
static int controller_value_iteration(int device, int S, int A, int O, int R, const int32_t* rs, const double* rto,
                                      const double* er, int N, const int32_t* node_action, const int32_t* node_succ,
                                      const double* v0, double gamma, double limit, int horizon, double* out_rows,
                                      double* out_changes, int32_t* out_iterations) {
    if (S <= 0 || A <= 0 || O <= 0 || R <= 0 || N <= 0 || horizon < 0 || !rs || !rto || !er || !node_action || !node_succ ||
        !v0 || !out_rows)
        FAIL(PBVI_EINVAL, "controller_value_iteration: bad arguments");
    if ((int64_t)S * A * O * R > 0x7fffffff) FAIL(PBVI_EUNSUPPORTED, "controller_value_iteration: S*A*O*R exceeds int32");
    const int s_blocks = (S + 255) / 256;
    if ((int64_t)N * s_blocks > 0x7fffffff)
        FAIL(PBVI_EUNSUPPORTED, "controller_value_iteration: N*ceil(S/256) exceeds int32");
    std::vector<int> per_action((size_t)A + 1, 0);           // nodes per action, then the first position of each action
    for (int n = 0; n < N; ++n) {
        if (node_action[n] < 0 || node_action[n] >= A) FAIL(PBVI_EINVAL, "controller_value_iteration: node action out of range");
        ++per_action[(size_t)node_action[n] + 1];
        for (int o = 0; o < O; ++o)
            if (node_succ[(size_t)n * O + o] < 0 || node_succ[(size_t)n * O + o] >= N)
                FAIL(PBVI_EINVAL, "controller_value_iteration: successor node out of range");
    }
    SweepTables h;
    if (!retile_sweep_tables(S, A, O, R, rs, rto, er, h))
        FAIL(PBVI_EINVAL, "controller_value_iteration: reachable state out of range");
    const size_t n_rs = (size_t)S * A * R, n_rto = n_rs * O, n_er = (size_t)S * A, n_v = (size_t)N * S;
    if (horizon == 0) {                                      // nothing to sweep: v0 comes back as it is
        memcpy(out_rows, v0, n_v * sizeof(double));
        if (out_iterations) *out_iterations = 0;
        return PBVI_OK;
    }
    // the nodes in the order of their actions; a tile never crosses from one action to the next
    const int most = *std::max_element(per_action.begin() + 1, per_action.end());
    const int node_tile = most >= 2 ? CONTROLLER_NODE_TILE : 1;
    std::vector<int32_t> tile_first;
    for (int a = 0; a < A; ++a) {
        if (node_tile > 1)
            for (int k = 0; k < per_action[(size_t)a + 1]; k += node_tile) tile_first.push_back(per_action[(size_t)a] + k);
        per_action[(size_t)a + 1] += per_action[(size_t)a];
    }
    tile_first.push_back(N);
    const int tiles = node_tile > 1 ? (int)tile_first.size() - 1 : N;
    std::vector<int32_t> order((size_t)N), pos((size_t)N), h_action((size_t)N), h_succ((size_t)N * O);
    for (int n = 0; n < N; ++n) {
        pos[(size_t)n] = per_action[(size_t)node_action[n]]++;
        order[(size_t)pos[(size_t)n]] = n;
    }
    std::vector<double> h_v(n_v);
    for (int p = 0; p < N; ++p) {
        const size_t n = (size_t)order[(size_t)p];
        h_action[(size_t)p] = node_action[n];
        for (int o = 0; o < O; ++o) h_succ[(size_t)p * O + o] = pos[(size_t)node_succ[n * O + o]];
        memcpy(h_v.data() + (size_t)p * S, v0 + n * S, (size_t)S * sizeof(double));
    }
    SweepRun run;
    DevBuf d_rs{run.mem}, d_rto{run.mem}, d_er{run.mem}, d_action{run.mem}, d_succ{run.mem}, d_tiles{run.mem},
        d_v[2]{{run.mem}, {run.mem}};
    int rc;
    if ((rc = run.open(device, horizon, {{d_rs, n_rs * sizeof(int32_t), h.rs.data()},
                                         {d_rto, n_rto * sizeof(double), h.rto.data()},
                                         {d_er, n_er * sizeof(double), h.er.data()},
                                         {d_action, (size_t)N * sizeof(int32_t), h_action.data()},
                                         {d_succ, (size_t)N * O * sizeof(int32_t), h_succ.data()},
                                         {d_tiles, tile_first.size() * sizeof(int32_t), tile_first.data()},
                                         {d_v[0], n_v * sizeof(double), h_v.data()},
                                         {d_v[1], n_v * sizeof(double), nullptr}})))
        return rc;
    ControllerSweep cs{};
    cs.S = S, cs.A = A, cs.O = O, cs.R = R, cs.N = N;
    cs.rs = d_rs.as<int32_t>(), cs.rto = d_rto.as<double>(), cs.er = d_er.as<double>();
    cs.node_action = d_action.as<int32_t>(), cs.node_succ = d_succ.as<int32_t>();
    cs.node_tile = node_tile, cs.tiles = tiles, cs.tile_first = d_tiles.as<int32_t>();   // (tiles * s_blocks <= N * s_blocks)
    cs.gamma = gamma, cs.limit = limit, cs.changes = run.d_changes.as<double>();
    if ((rc = run.sweep(horizon, limit, [&](int it, hipStream_t st) {
            cs.it = it, cs.v_in = d_v[it & 1].as<double>(), cs.v_out = d_v[(it + 1) & 1].as<double>();
            return launch_controller_sweep(cs, st);
        })))
        return rc;
    // sweep done-1 was the last to write: its V is in buffer done & 1 (the sweeps enqueued after it left at once)
    if ((rc = run.fetch(h_v.data(), d_v[run.done & 1], n_v * sizeof(double)))) return rc;
    for (int p = 0; p < N; ++p)
        memcpy(out_rows + (size_t)order[(size_t)p] * S, h_v.data() + (size_t)p * S, (size_t)S * sizeof(double));
    run.report(out_changes, out_iterations);
    return PBVI_OK;
}

}  // namespace pbvi

// --------------------------------------------------------------------------- //
// C-ABI
// --------------------------------------------------------------------------- //
struct pbvi_engine {
    pbvi::EngineBase* impl;
};

extern "C" {

int pbvi_version(void) { return 100; }

int pbvi_debug_poison(int enable) {
    const int prev = pbvi::poison_enabled() ? 1 : 0;
    pbvi::g_poison = enable ? 1 : 0;
    return prev;
}
int64_t pbvi_debug_alloc_limit(int64_t mb) {
    const int64_t prev = pbvi::DevBuf::limit_bytes();
    pbvi::DevBuf::limit_bytes() = mb < 0 ? -1 : mb << 20;
    return prev < 0 ? -1 : prev >> 20;
}
int64_t pbvi_debug_live_bytes(void) { return pbvi::DevMem::live.load(); }


int pbvi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* pbvi_last_error(void) { return pbvi::g_err.c_str(); }

int pbvi_engine_create(pbvi_engine_t** out, int device, int32_t S, int32_t A, int32_t O, int32_t R,
                       const int32_t* reach_states, const void* rto, const void* exp_reward, int dtype, int mode) {
    using namespace pbvi;
    if (!out) FAIL(PBVI_EINVAL, "engine_create: out is NULL");
    *out = nullptr;
    if (S <= 0 || A <= 0 || O <= 0 || R <= 0) FAIL(PBVI_EINVAL, "engine_create: S, A, O, R must be positive");
    if (!reach_states || !rto || !exp_reward) FAIL(PBVI_EINVAL, "engine_create: NULL table");
    if (dtype != PBVI_F32 && dtype != PBVI_F64) FAIL(PBVI_EINVAL, "engine_create: dtype must be PBVI_F32 or PBVI_F64");
    if (mode != PBVI_SPARSE && mode != PBVI_DENSE) FAIL(PBVI_EINVAL, "engine_create: unknown mode");
    // Limits of the backup kernels, refused here rather than by a launcher in the middle of a backup: the action kernel
    // keeps one value per action in a 256-thread block, and (action, observation) pairs / (action, term) pairs index
    // grid.y and grid.z (at most 65535).  A * (1 + O) <= 65535 implies A * O <= 65535.
    if (A > 256) FAIL(PBVI_EUNSUPPORTED, "engine_create: at most 256 actions (A <= 256)");
    if ((int64_t)A * (1 + (int64_t)O) > 65535)
        FAIL(PBVI_EUNSUPPORTED, "engine_create: at most 65535 action-observation terms (A * (1 + O) <= 65535)");
    int ndev = pbvi_device_count();
    if (ndev <= 0) FAIL(PBVI_ERUNTIME, "engine_create: no HIP device visible");
    if (device < 0 || device >= ndev) FAIL(PBVI_EINVAL, "engine_create: device index out of range");
    EngineBase* impl = nullptr;
    int rc;
    if (dtype == PBVI_F32) {
        auto* e = new (std::nothrow) EngineT<float>();
        if (!e) FAIL(PBVI_ENOMEM, "engine_create: host allocation failed");
        rc = e->init(device, S, A, O, R, reach_states, (const float*)rto, (const float*)exp_reward, mode);
        impl = e;
    } else {
        auto* e = new (std::nothrow) EngineT<double>();
        if (!e) FAIL(PBVI_ENOMEM, "engine_create: host allocation failed");
        rc = e->init(device, S, A, O, R, reach_states, (const double*)rto, (const double*)exp_reward, mode);
        impl = e;
    }
    if (rc != PBVI_OK) {
        delete impl;
        return rc;
    }
    pbvi_engine* h = new (std::nothrow) pbvi_engine{impl};
    if (!h) {
        delete impl;
        FAIL(PBVI_ENOMEM, "engine_create: host allocation failed");
    }
    *out = h;
    return PBVI_OK;
}

void pbvi_engine_destroy(pbvi_engine_t* e) {
    if (!e) return;
    delete e->impl;
    delete e;
}

#define NEED(e)                                            \
    do {                                                   \
        if (!(e) || !(e)->impl) {                          \
            pbvi::set_error("NULL engine handle");         \
            return PBVI_EINVAL;                            \
        }                                                  \
    } while (0)

int pbvi_alpha_set(pbvi_engine_t* e, const void* alpha, int64_t V) {
    NEED(e);
    return e->impl->alpha_set(alpha, V);
}
int pbvi_alpha_append(pbvi_engine_t* e, const void* alpha, int64_t V_add) {
    NEED(e);
    return e->impl->alpha_append(alpha, V_add);
}
int64_t pbvi_alpha_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->alpha_count() : -1; }
int pbvi_beliefs_set(pbvi_engine_t* e, const void* beliefs, int64_t B) {
    NEED(e);
    return e->impl->beliefs_set(beliefs, B);
}
int pbvi_backup_run(pbvi_engine_t* e, double gamma, int flags, pbvi_stats_t* stats) {
    NEED(e);
    return e->impl->backup_run(gamma, flags, stats);
}
int pbvi_backup_fetch(pbvi_engine_t* e, void* out_alpha, int32_t* out_action, int32_t* out_best_alpha, uint8_t* out_keep) {
    NEED(e);
    return e->impl->backup_fetch(out_alpha, out_action, out_best_alpha, out_keep);
}
int64_t pbvi_backup_store_unique(pbvi_engine_t* e, const int32_t* unique_idx, int64_t n) {
    NEED(e);
    return e->impl->store_append_unique(unique_idx, n);
}

int pbvi_backup_fetch_row_hashes(pbvi_engine_t* e, uint64_t* out_hashes) {
    NEED(e);
    return e->impl->fetch_row_hashes(out_hashes);
}
int pbvi_backup_fetch_unique_keys(pbvi_engine_t* e, int32_t* out_keys) {
    NEED(e);
    return e->impl->fetch_unique_keys(out_keys);
}
int pbvi_backup_fetch_exchange(pbvi_engine_t* e, int32_t* out) {
    NEED(e);
    return e->impl->fetch_exchange(out, e->impl->beliefs_count());
}
int pbvi_backup_fetch_exchange_padded(pbvi_engine_t* e, int64_t per, int32_t* out) {
    NEED(e);
    return e->impl->fetch_exchange(out, per);
}
int64_t pbvi_assemble_rows_store(pbvi_engine_t* e, double gamma, int64_t n, const int32_t* keys, void* out_rows) {
    NEED(e);
    return e->impl->assemble_keys_store(gamma, n, keys, out_rows);
}
// Host side of the key exchange (no engine, no device): the ranks' messages -> globally distinct keys in order of first
// occurrence + per-belief positions.  A few hundred keys and <= 65535 beliefs per rank: one pass with a small
// open-addressing table (the NumPy version -- np.unique over key rows, five fancy-index passes -- took 0.36 ms for eight
// messages of 1024 beliefs; this is a few microseconds).
int64_t pbvi_exchange_merge(const int32_t* all_meta, int32_t world, int64_t stride, int64_t per, int32_t key_width,
                            int64_t n_total, int32_t* out_keys, int32_t* out_index, int32_t* out_action, uint8_t* out_keep) {
    if (!all_meta || world <= 0 || per <= 0 || key_width <= 0 || n_total < 0 || !out_keys || !out_index ||
        !out_action || !out_keep) {
        pbvi::set_error("exchange_merge: bad arguments");
        return PBVI_EINVAL;
    }
    const int64_t n_meta = 1 + 3 * per + per * (int64_t)key_width;
    // (positions and counts are int32 words of the message: one message must stay addressable by them)
    if (per > 0x7fffffff / ((int64_t)key_width + 3) || stride < n_meta || n_total > (int64_t)world * per ||
        (int64_t)world * per > 0x7fffffff) {
        pbvi::set_error("exchange_merge: message stride / belief count do not fit the block size");
        return PBVI_EINVAL;
    }
    int64_t total = 0;
    for (int r = 0; r < world; ++r) {
        const int64_t c = all_meta[(int64_t)r * stride];
        if (c < 0 || c > per) {
            pbvi::set_error("exchange_merge: corrupt message (unique-row count out of range)");
            return PBVI_EINVAL;
        }
        total += c;
    }
    size_t cap = 16;
    while (cap < (size_t)total * 2 + 1) cap <<= 1;
    std::vector<int32_t> table, pos;
    try {
        table.assign(cap, -1);                               // slot -> position in out_keys
        pos.assign((size_t)std::max<int64_t>(total, 1), 0);  // (rank, u) -> position, ranks concatenated
    } catch (const std::bad_alloc&) {
        pbvi::set_error("exchange_merge: host allocation failed");
        return PBVI_ENOMEM;
    }
    int64_t n_keys = 0, base = 0;
    for (int r = 0; r < world; ++r) {
        const int32_t* msg = all_meta + (int64_t)r * stride;
        const int32_t* keys = msg + 1 + 3 * per;
        const int64_t c = msg[0];
        for (int64_t u = 0; u < c; ++u) {
            const int32_t* k = keys + u * key_width;
            uint64_t h = 1469598103934665603ull;
            for (int j = 0; j < key_width; ++j) h = (h ^ (uint32_t)k[j]) * 1099511628211ull;
            size_t slot = (size_t)(h ^ (h >> 29)) & (cap - 1);
            for (;;) {
                const int32_t at = table[slot];
                if (at < 0) {                                // first occurrence: the key gets the next position
                    std::memcpy(out_keys + n_keys * key_width, k, (size_t)key_width * sizeof(int32_t));
                    table[slot] = (int32_t)n_keys;
                    pos[(size_t)(base + u)] = (int32_t)n_keys++;
                    break;
                }
                if (std::memcmp(out_keys + (int64_t)at * key_width, k, (size_t)key_width * sizeof(int32_t)) == 0) {
                    pos[(size_t)(base + u)] = at;            // the same row found by another rank (or twice by this one)
                    break;
                }
                slot = (slot + 1) & (cap - 1);
            }
        }
        // this rank's beliefs, global belief order: rank r holds [r * per, min((r + 1) * per, n_total))
        const int64_t lo = std::min<int64_t>((int64_t)r * per, n_total), hi = std::min<int64_t>(lo + per, n_total);
        for (int64_t j = 0; j < hi - lo; ++j) {
            const int32_t u = msg[1 + j];
            if (u < 0 || u >= c) {
                pbvi::set_error("exchange_merge: corrupt message (row index out of range)");
                return PBVI_EINVAL;
            }
            out_index[lo + j] = pos[(size_t)(base + u)];
            out_action[lo + j] = msg[1 + per + j];
            out_keep[lo + j] = msg[1 + 2 * per + j] ? 1 : 0;
        }
        base += c;
    }
    return n_keys;
}
int pbvi_assemble_rows(pbvi_engine_t* e, double gamma, int64_t n, const int32_t* keys, void* out_rows) {
    NEED(e);
    return e->impl->assemble_keys(gamma, n, keys, out_rows);
}
int pbvi_engine_after_oom(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->after_oom();
}
int pbvi_backup_device_results(pbvi_engine_t* e, void** d_alpha, int32_t** d_action, uint8_t** d_keep) {
    NEED(e);
    return e->impl->device_results(d_alpha, d_action, d_keep);
}
int64_t pbvi_backup_unique_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->unique_count() : -1; }
int pbvi_backup_fetch_unique(pbvi_engine_t* e, void* out_rows, int32_t* out_index) {
    NEED(e);
    return e->impl->fetch_unique(out_rows, out_index);
}
int pbvi_backup_run_fetch(pbvi_engine_t* e, double gamma, int flags, pbvi_stats_t* stats, void* out_rows, int64_t cap_rows,
                          int32_t* out_slot, int32_t* out_index, int32_t* out_action, int32_t* out_best_alpha, uint8_t* out_keep,
                          int64_t* n_unique, int64_t* n_slots) {
    NEED(e);
    return e->impl->run_fetch(gamma, flags, stats, out_rows, cap_rows, out_slot, out_index, out_action, out_best_alpha, out_keep,
                              n_unique, n_slots);
}
int pbvi_backup_fetch_compact(pbvi_engine_t* e, void* out_rows, int32_t* out_index, int32_t* out_action,
                              int32_t* out_best_alpha, uint8_t* out_keep) {
    NEED(e);
    return e->impl->fetch_compact(out_rows, out_index, out_action, out_best_alpha, out_keep);
}
void* pbvi_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) return nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        pbvi::set_error("pbvi_host_alloc: hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
        return nullptr;
    }
    return p;
}
void pbvi_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}
int pbvi_debug_gemm_dense(int enable) { return pbvi::set_gemm_force_dense(enable); }
int pbvi_debug_split_schedule(int schedule) { return pbvi::set_gemm_split_schedule(schedule); }
int pbvi_debug_split_stagger(int on) { return pbvi::set_gemm_split_stagger(on); }
int64_t pbvi_debug_slabs(pbvi_engine_t* e, void* out, int64_t cap_bytes) {
    NEED(e);
    return e->impl->debug_slabs(out, cap_bytes);
}
int pbvi_debug_slabs_fill(pbvi_engine_t* e, int byte) {
    NEED(e);
    return e->impl->debug_slabs_fill(byte);
}
int pbvi_debug_score_probe(pbvi_engine_t* e, int enable) {
    NEED(e);
    return e->impl->debug_score_probe(enable);
}
int pbvi_debug_refine_counts(pbvi_engine_t* e, int64_t out[8]) {
    NEED(e);
    return e->impl->debug_refine_counts(out);
}
int pbvi_debug_value_max_route(pbvi_engine_t* e, int64_t out[8]) {
    NEED(e);
    return e->impl->debug_value_max_route(out);
}
int pbvi_debug_score_probe_fetch(pbvi_engine_t* e, int64_t* dims, double* scalars, double* score, double* mag, double* err,
                                 int32_t* best_v, double* best_score, int32_t* queue, uint8_t* dead, int32_t* perm) {
    NEED(e);
    return e->impl->debug_score_probe_fetch(dims, scalars, score, mag, err, best_v, best_score, queue, dead, perm);
}
int pbvi_backup(pbvi_engine_t* e, const void* beliefs, int64_t B, double gamma, int flags, void* out_alpha,
                int32_t* out_action, int32_t* out_best_alpha, uint8_t* out_keep, pbvi_stats_t* stats) {
    NEED(e);
    int rc = e->impl->beliefs_set(beliefs, B);
    if (rc) return rc;
    rc = e->impl->backup_run(gamma, flags, stats);
    if (rc) return rc;
    return e->impl->backup_fetch(out_alpha, out_action, out_best_alpha, out_keep);
}
int pbvi_q_values(pbvi_engine_t* e, double gamma, double* out_q, int32_t* out_action, int32_t* out_best_v) {
    NEED(e);
    return e->impl->q_values(gamma, out_q, out_action, out_best_v);
}
int pbvi_prune_dominated(pbvi_engine_t* e, uint8_t* keep) {
    NEED(e);
    return e->impl->prune_dominated(keep);
}
int pbvi_prune_dominated_masked(pbvi_engine_t* e, const uint8_t* is_new, uint8_t* keep) {
    NEED(e);
    return e->impl->prune_dominated_masked(is_new, keep);
}
int pbvi_value_max(pbvi_engine_t* e, double* out_value, int32_t* out_index) {
    NEED(e);
    return e->impl->value_max(out_value, out_index);
}
int64_t pbvi_alpha_store_append(pbvi_engine_t* e, const void* rows, int64_t n) {
    NEED(e);
    return e->impl->store_append(0, rows, n);
}
int pbvi_value_max_store(pbvi_engine_t* e, int64_t n, double* out_value, int32_t* out_index) {
    NEED(e);
    return e->impl->value_max_store(n, out_value, out_index);
}
int64_t pbvi_belief_store_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->store_count(1) : -1; }
int64_t pbvi_alpha_store_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->store_count(0) : -1; }
int pbvi_alpha_select(pbvi_engine_t* e, const int32_t* ids, int64_t V) {
    NEED(e);
    return e->impl->store_select(0, ids, V);
}
int pbvi_alpha_store_reset(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->store_reset(0);
}
int64_t pbvi_belief_store_append(pbvi_engine_t* e, const void* rows, int64_t n) {
    NEED(e);
    return e->impl->store_append(1, rows, n);
}
int pbvi_beliefs_select(pbvi_engine_t* e, const int32_t* ids, int64_t B) {
    NEED(e);
    return e->impl->store_select(1, ids, B);
}
int pbvi_belief_store_reset(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->store_reset(1);
}
int pbvi_beliefs_advance(pbvi_engine_t* e, const int32_t* actions, const int32_t* observations, const uint8_t* keep,
                         int64_t* out_B) {
    NEED(e);
    return e->impl->beliefs_advance(actions, observations, keep, out_B);
}

int pbvi_backup_fetch_value_max(pbvi_engine_t* e, double* out_value) {
    NEED(e);
    return e->impl->backup_value_max(out_value);
}
int pbvi_belief_walk_keys(pbvi_engine_t* e, int64_t n, uint64_t* out_keys) {
    NEED(e);
    return e->impl->walk_keys(n, out_keys);
}
int64_t pbvi_belief_walk(pbvi_engine_t* e, const double* b0, int64_t n, const int32_t* actions, const int32_t* observations,
                         const uint8_t* restart, double* out_beliefs) {
    NEED(e);
    return e->impl->belief_walk(b0, n, actions, observations, restart, out_beliefs);
}

int pbvi_engine_set_rto_f64(pbvi_engine_t* e, const double* rto) {
    NEED(e);
    return e->impl->set_rto_f64(rto);
}

// What every rollout entry point takes: the simulations, the stream, the length and the trajectory arrays
static pbvi::RolloutCall rollout_call(const int32_t* start_states, const uint8_t* end_mask, uint64_t first_sim_id, uint64_t seed,
                                      int64_t T, int32_t* out_states, int32_t* out_actions, int32_t* out_observations,
                                      int32_t* out_steps) {
    pbvi::RolloutCall c{};
    c.start_states = start_states;
    c.end_mask = end_mask;
    c.first_sim_id = first_sim_id;
    c.seed = seed;
    c.T = T;
    c.out_states = out_states;
    c.out_actions = out_actions;
    c.out_observations = out_observations;
    c.out_steps = out_steps;
    return c;
}

int pbvi_rollout(pbvi_engine_t* e, const int32_t* alpha_actions, int lookahead, double gamma, const int32_t* start_states,
                 const uint8_t* end_mask, uint64_t first_sim_id, uint64_t seed, int64_t T, int32_t* out_states,
                 int32_t* out_actions, int32_t* out_observations, int32_t* out_steps) {
    NEED(e);
    // (any other lookahead is refused by the step loop as a source it does not know)
    pbvi::RolloutCall c = rollout_call(start_states, end_mask, first_sim_id, seed, T, out_states, out_actions, out_observations, out_steps);
    c.source = lookahead == 0 ? pbvi::ROLLOUT_VALUE_MAX : lookahead == 1 ? pbvi::ROLLOUT_Q : -1;
    c.alpha_actions = alpha_actions;
    c.gamma = gamma;
    return e->impl->rollout(c);
}
int pbvi_infotaxis(pbvi_engine_t* e, double* out_g, int32_t* out_action, double* out_p_obs, double* out_entropy) {
    NEED(e);
    return e->impl->infotaxis(out_g, out_action, out_p_obs, out_entropy);
}
int pbvi_upper_reset(pbvi_engine_t* e, const double* corner) {
    NEED(e);
    return e->impl->upper_reset(corner);
}
int pbvi_upper_append(pbvi_engine_t* e, const double* points, const double* values, const double* gaps, int64_t n) {
    NEED(e);
    return e->impl->upper_append(points, values, gaps, n);
}
int64_t pbvi_upper_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->upper_count() : -1; }
int pbvi_upper_bound(pbvi_engine_t* e, int64_t n_visible, int64_t n_hit, double* out_value, int32_t* out_point, int32_t* out_hit) {
    NEED(e);
    return e->impl->upper_bound(n_visible, n_hit, out_value, out_point, out_hit);
}
int pbvi_upper_q(pbvi_engine_t* e, double gamma, int64_t n_visible, int64_t n_hit, double* out_q, int32_t* out_action,
                 double* out_p_obs, double* out_succ_value) {
    NEED(e);
    return e->impl->upper_q(gamma, n_visible, n_hit, out_q, out_action, out_p_obs, out_succ_value);
}
int pbvi_rollout_infotaxis(pbvi_engine_t* e, const int32_t* start_states, const uint8_t* end_mask, uint64_t first_sim_id,
                           uint64_t seed, int64_t T, int32_t* out_states, int32_t* out_actions, int32_t* out_observations,
                           int32_t* out_steps) {
    NEED(e);
    pbvi::RolloutCall c = rollout_call(start_states, end_mask, first_sim_id, seed, T, out_states, out_actions, out_observations, out_steps);
    c.source = pbvi::ROLLOUT_INFOTAXIS;
    return e->impl->rollout(c);
}
int pbvi_env_set_frames(pbvi_engine_t* e, const uint8_t* frames, int64_t F, int64_t C, const int32_t* channel_of_action) {
    NEED(e);
    return e->impl->env_set_frames(frames, F, C, channel_of_action);
}
int pbvi_env_set_table(pbvi_engine_t* e, const double* obs_prob) {
    NEED(e);
    return e->impl->env_set_table(obs_prob);
}
int pbvi_env_clear(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->env_clear();
}
int pbvi_rollout_env(pbvi_engine_t* e, int policy, const int32_t* alpha_actions, double gamma, const int32_t* start_states,
                     const uint8_t* end_mask, int end_observation, const int64_t* shifts, uint64_t first_sim_id, uint64_t seed,
                     int64_t T, int32_t* out_states, int32_t* out_actions, int32_t* out_observations, int32_t* out_steps,
                     uint8_t* out_lost) {
    using namespace pbvi;
    NEED(e);
    // (the step loop knows two more sources, pbvi_rollout_space_aware's and pbvi_rollout_state_policy's: this entry point's
    // numbers are refused here)
    if (policy != pbvi::ROLLOUT_VALUE_MAX && policy != pbvi::ROLLOUT_Q && policy != pbvi::ROLLOUT_INFOTAXIS)
        FAIL(PBVI_EINVAL, "rollout_env: policy must be 0 (value-max), 1 (Q) or 2 (infotaxis)");
    pbvi::RolloutCall c = rollout_call(start_states, end_mask, first_sim_id, seed, T, out_states, out_actions, out_observations, out_steps);
    c.source = policy;
    c.alpha_actions = alpha_actions;
    c.gamma = gamma;
    c.env = true;
    c.end_observation = end_observation;
    c.shifts = shifts;
    c.out_lost = out_lost;
    return e->impl->rollout(c);
}
int pbvi_state_weights_set(pbvi_engine_t* e, const double* weights) {
    NEED(e);
    return e->impl->state_weights_set(weights);
}
int pbvi_state_weights_clear(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->state_weights_clear();
}
int pbvi_space_aware(pbvi_engine_t* e, int objective, double* out_f, int32_t* out_action, double* out_terms) {
    NEED(e);
    return e->impl->space_aware(objective, out_f, out_action, out_terms);
}
int pbvi_rollout_space_aware(pbvi_engine_t* e, int objective, int use_env, const int32_t* start_states, const uint8_t* end_mask,
                             int end_observation, const int64_t* shifts, uint64_t first_sim_id, uint64_t seed, int64_t T,
                             int32_t* out_states, int32_t* out_actions, int32_t* out_observations, int32_t* out_steps,
                             uint8_t* out_lost) {
    using namespace pbvi;
    NEED(e);
    if (use_env != 0 && use_env != 1) FAIL(PBVI_EINVAL, "rollout_space_aware: use_env must be 0 (the model's world) or 1 (the environment)");
    if (!use_env && (end_observation != -1 || shifts != nullptr))
        FAIL(PBVI_EINVAL, "rollout_space_aware: end_observation and shifts belong to an environment (use_env = 0 takes -1 and NULL)");
    pbvi::RolloutCall c = rollout_call(start_states, end_mask, first_sim_id, seed, T, out_states, out_actions, out_observations, out_steps);
    c.source = pbvi::ROLLOUT_SPACE_AWARE;
    c.objective = objective;
    c.env = use_env != 0;
    c.end_observation = end_observation;
    c.shifts = shifts;
    c.out_lost = use_env ? out_lost : nullptr;
    const int64_t n0 = e->impl->beliefs_count();
    const int rc = e->impl->rollout(c);
    if (rc == PBVI_OK && !use_env && out_lost && n0 > 0) memset(out_lost, 0, (size_t)n0);   // nothing is lost in the model's world
    return rc;
}
int pbvi_state_policy_set(pbvi_engine_t* e, const int32_t* state_actions) {
    NEED(e);
    return e->impl->state_policy_set(state_actions);
}
int pbvi_state_policy_clear(pbvi_engine_t* e) {
    NEED(e);
    return e->impl->state_policy_clear();
}
int pbvi_state_policy(pbvi_engine_t* e, int rule, uint64_t seed, uint64_t first_sim_id, int64_t t, const double* uniforms,
                      int32_t* out_action, int32_t* out_state, double* out_votes) {
    NEED(e);
    return e->impl->state_policy(rule, seed, first_sim_id, t, uniforms, out_action, out_state, out_votes);
}
int pbvi_rollout_state_policy(pbvi_engine_t* e, int rule, int use_env, const int32_t* start_states, const uint8_t* end_mask,
                              int end_observation, const int64_t* shifts, uint64_t first_sim_id, uint64_t seed, int64_t T,
                              int32_t* out_states, int32_t* out_actions, int32_t* out_observations, int32_t* out_steps,
                              uint8_t* out_lost) {
    using namespace pbvi;
    NEED(e);
    if (use_env != 0 && use_env != 1) FAIL(PBVI_EINVAL, "rollout_state_policy: use_env must be 0 (the model's world) or 1 (the environment)");
    if (!use_env && (end_observation != -1 || shifts != nullptr))
        FAIL(PBVI_EINVAL, "rollout_state_policy: end_observation and shifts belong to an environment (use_env = 0 takes -1 and NULL)");
    pbvi::RolloutCall c = rollout_call(start_states, end_mask, first_sim_id, seed, T, out_states, out_actions, out_observations, out_steps);
    c.source = pbvi::ROLLOUT_STATE_POLICY;
    c.rule = rule;
    c.env = use_env != 0;
    c.end_observation = end_observation;
    c.shifts = shifts;
    c.out_lost = use_env ? out_lost : nullptr;
    const int64_t n0 = e->impl->beliefs_count();
    const int rc = e->impl->rollout(c);
    if (rc == PBVI_OK && !use_env && out_lost && n0 > 0) memset(out_lost, 0, (size_t)n0);   // nothing is lost in the model's world
    return rc;
}
int pbvi_beliefs_fetch(pbvi_engine_t* e, void* out_beliefs) {
    NEED(e);
    return e->impl->beliefs_fetch(out_beliefs);
}

int64_t pbvi_beliefs_count(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->beliefs_count() : -1; }

int pbvi_mdp_value_iteration(int device, int32_t S, int32_t A, int32_t R, const int32_t* reach_states,
                             const double* reach_prob, const double* exp_reward, const double* v0, double gamma,
                             double max_change_limit, int32_t horizon, double* out_rows, double* out_changes,
                             int32_t* out_iterations) {
    return pbvi::mdp_value_iteration(device, S, A, R, reach_states, reach_prob, exp_reward, v0, gamma, max_change_limit,
                                     horizon, out_rows, out_changes, out_iterations);
}

int pbvi_fib_value_iteration(int device, int32_t S, int32_t A, int32_t O, int32_t R, const int32_t* reach_states,
                             const double* rto, const double* exp_reward, const double* q0, double gamma,
                             double max_change_limit, int32_t horizon, double* out_rows, double* out_changes,
                             int32_t* out_iterations) {
    return pbvi::fib_value_iteration(device, S, A, O, R, reach_states, rto, exp_reward, q0, gamma, max_change_limit,
                                     horizon, out_rows, out_changes, out_iterations);
}

int pbvi_controller_value_iteration(int device, int32_t S, int32_t A, int32_t O, int32_t R, const int32_t* reach_states,
                                    const double* rto, const double* exp_reward, int32_t N, const int32_t* node_action,
                                    const int32_t* node_succ, const double* v0, double gamma, double max_change_limit,
                                    int32_t horizon, double* out_rows, double* out_changes, int32_t* out_iterations) {
    return pbvi::controller_value_iteration(device, S, A, O, R, reach_states, rto, exp_reward, N, node_action, node_succ, v0,
                                            gamma, max_change_limit, horizon, out_rows, out_changes, out_iterations);
}

int pbvi_belief_update(pbvi_engine_t* e, const int32_t* actions, const int32_t* observations, void* out_beliefs) {
    NEED(e);
    return e->impl->belief_update(actions, observations, out_beliefs);
}
int pbvi_set_formulation(pbvi_engine_t* e, int formulation) {
    NEED(e);
    return e->impl->set_formulation(formulation);
}
int pbvi_set_fused_projection(pbvi_engine_t* e, int enable) {
    NEED(e);
    return e->impl->set_fused(enable);
}
int pbvi_set_f64_screen(pbvi_engine_t* e, int mode) {
    NEED(e);
    return e->impl->set_screen(mode);
}
int pbvi_set_score_split(pbvi_engine_t* e, int mode) {
    NEED(e);
    return e->impl->set_score_split(mode);
}
int pbvi_set_value_max_exact(pbvi_engine_t* e, int exact) {
    NEED(e);
    return e->impl->set_value_max_exact(exact);
}
int pbvi_alpha_layout(pbvi_engine_t* e, int64_t* free_rows, int64_t* layouts) {
    NEED(e);
    return e->impl->alpha_layout(free_rows, layouts);
}
int pbvi_set_gamma_tiling(pbvi_engine_t* e, int mode, int64_t chunk_rows) {
    NEED(e);
    return e->impl->set_gamma_tiling(mode, chunk_rows);
}
int pbvi_gamma_tiling_plan(int32_t S, int32_t A, int32_t O, int64_t V, int64_t B, int dtype, int64_t budget_bytes,
                           int64_t* chunk_rows, int64_t* n_chunks, int64_t* bytes_needed) {
    using namespace pbvi;
    if (!chunk_rows || !n_chunks || !bytes_needed || (dtype != 0 && dtype != 1))
        FAIL(PBVI_EINVAL, "gamma_tiling_plan: null output or dtype not 0 (fp32) / 1 (fp64)");
    pbvi::TilingPlan tp;
    const int rc = pbvi::tiling_plan(S, A, O, V, B, dtype == 0, budget_bytes, *chunk_rows, &tp);
    if (rc == PBVI_EINVAL) FAIL(PBVI_EINVAL, "gamma_tiling_plan: S, A, O, V, B must be positive, budget and chunk_rows >= 0, A*O*(V+1)+2A within int32");
    *chunk_rows = tp.chunk_rows;
    *n_chunks = tp.n_chunks;
    *bytes_needed = tp.bytes;
    if (rc == PBVI_ENOMEM)
        FAIL(PBVI_ENOMEM, "gamma_tiling_plan: chunks of " + std::to_string(tp.chunk_rows) + " alpha rows need " +
                              std::to_string(tp.bytes) + " bytes, the budget is " + std::to_string(budget_bytes));
    return PBVI_OK;
}
int pbvi_set_tie_window(pbvi_engine_t* e, double rel) {
    NEED(e);
    return e->impl->set_tie_window(rel);
}
int64_t pbvi_device_bytes(const pbvi_engine_t* e) { return (e && e->impl) ? e->impl->device_bytes() : -1; }

}  // extern "C"
