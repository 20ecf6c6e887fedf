namespace {

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            std::fprintf(stderr, "mapad_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MAPAD_ERR_DEVICE;                                                                        \
        }                                                                                                   \
    } while (0)

// Device memory that frees itself with its owner (on the thread that destroys the owner: its device must be current).  Move-only; a moved-from buffer is empty.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~DevBuf() { release(); }
    void swap(DevBuf& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    // room for n elements (n + n / 8 + 64, or exactly n); what was there is not kept.  A failed allocation leaves the buffer empty and no error for the next hipGetLastError
    int ensure(size_t n, bool exact = false) {
        if (n <= cap) return MAPAD_OK;
        release();
        const size_t want = exact ? n : n + n / 8 + 64;
        if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return MAPAD_ERR_NOMEM; }
        cap = want;
        return MAPAD_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// One event, created when first asked for and destroyed with its owner.  Move-only.
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete; DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept { std::swap(e, o.e); }
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { reset(); std::swap(e, o.e); } return *this; }
    ~DevEvent() { reset(); }
    int ensure(unsigned flags = 0) { if (!e) HIP_TRY(hipEventCreateWithFlags(&e, flags)); return MAPAD_OK; }
    void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// Page-locked host memory for everything that crosses PCIe (results out, staged inputs in): DMA at link speed instead of the driver's
// staged copies of pageable memory.  Pinning is slow (the pages are locked one by one), so blocks are recycled: power-of-two sizes, a few
// kept per size, process-wide (results may outlive the context they came from).
class PinnedPool {
public:
    static PinnedPool& instance() { static PinnedPool p; return p; }
    void* take(size_t bytes, size_t& got) {
        size_t cap = 1 << 16;
        while (cap < bytes) cap <<= 1;
        got = cap;
        {
            std::lock_guard<std::mutex> g(mu_);
            auto& fl = free_[cap];
            if (!fl.empty()) { void* p = fl.back(); fl.pop_back(); return p; }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess) return nullptr;
        return p;
    }
    void give(void* p, size_t cap) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            auto& fl = free_[cap];
            if (fl.size() < 6) { fl.push_back(p); return; }
        }
        (void)hipHostFree(p);
    }
private:
    std::mutex mu_;
    std::map<size_t, std::vector<void*>> free_;
};
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0, cap_bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    bool resize(size_t count) {
        if (count * sizeof(T) > cap_bytes) {
            PinnedPool::instance().give(p, cap_bytes);
            p = (T*)PinnedPool::instance().take(std::max<size_t>(count * sizeof(T), 1), cap_bytes);
            if (!p) { cap_bytes = 0; n = 0; return false; }
        }
        n = count;
        return true;
    }
    T* data() { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T& operator[](size_t i) { return p[i]; }
    ~PinnedBuf() { PinnedPool::instance().give(p, cap_bytes); }
};

// Host memory the GPU and the host both see while a kernel runs (the host tail's hand-over ring and its control word): page-locked AND coherent — fine-grained,
// not cached in the GPU's L2 —, which plain hipHostMalloc memory is not unless HIP_HOST_COHERENT=1.  Not pooled: one per batch slot, grown when needed.
struct CoherentBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    CoherentBuf() = default;
    CoherentBuf(const CoherentBuf&) = delete;
    CoherentBuf& operator=(const CoherentBuf&) = delete;
    bool ensure(size_t bytes) {
        if (bytes <= cap) return true;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = 1 << 16;
        while (want < bytes) want <<= 1;
        void* q = nullptr;
        if (hipHostMalloc(&q, want, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return false;
        p = (uint8_t*)q; cap = want;
        return true;
    }
    ~CoherentBuf() { if (p) (void)hipHostFree(p); }
};

// Page-locked blocks are recycled: pinning and unpinning cost milliseconds per block, and hipHostFree waits for the device — in a chunk loop
// that allocates its read buffers per chunk (mapad-amd map) this stalled the whole pipeline once per chunk.  Blocks come in power-of-two sizes;
// up to 8 GB of freed blocks are kept for reuse.
struct HostBlockCache {
    std::mutex mu;
    std::multimap<size_t, void*> free_blocks;
    std::unordered_map<void*, size_t> size_of;
    size_t cached = 0;
    static size_t bucket(size_t bytes) { size_t b = 65536; while (b < bytes) b <<= 1; return b; }
    void* alloc(size_t bytes) {
        const size_t want = bucket(bytes);
        {
            std::lock_guard<std::mutex> l(mu);
            auto it = free_blocks.find(want);
            if (it != free_blocks.end()) { void* p = it->second; free_blocks.erase(it); cached -= want; return p; }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> l(mu);
        size_of[p] = want;
        return p;
    }
    void release(void* p) {
        size_t sz = 0;
        {
            std::lock_guard<std::mutex> l(mu);
            auto it = size_of.find(p);
            if (it == size_of.end()) return;  // not ours
            sz = it->second;
            if (cached + sz <= (8ull << 30)) { free_blocks.emplace(sz, p); cached += sz; return; }
            size_of.erase(it);
        }
        (void)hipHostFree(p);
    }
};
HostBlockCache& host_blocks() { static HostBlockCache* c = new HostBlockCache(); return *c; }  // never destroyed: the runtime may be gone at exit

}  // namespace
