// Who owns device memory in libpffft_hip.so: one owner type per allocation (DevBuf / PinnedBuf), the per-stream scratch pool of a setup
// (StreamScratch) and the one recipe every twiddle table is built by.  Nothing here pools, caches or reuses freed memory.
// No object of these types may have static storage duration: nothing may call hipFree during static destruction (the process-lifetime
// caches - split_sub_table in dma_tu.hip, the counter ring of pfdsp_mix.h - keep raw pointers that are never freed).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "cxmath.h"
#include "fft_stock.h"

namespace pf {

int fail(hipError_t e, const char* what);   // plan_tu.hip (pf_host.h: PF_CHECK)
bool stream_capturing(hipStream_t st);

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }   // (takes a pointer of any device, whatever the current one is)
    static constexpr const char* what = "hipMalloc";
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
    static constexpr const char* what = "hipHostMalloc";
};

// move-only owner of ONE allocation: freed when the owner goes, never by hand
template <class Mem>
class OwnedBuf {
public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~OwnedBuf() { reset(); }
    void* get() const { return p_; }
    template <typename T> T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    // at least `bytes` bytes (contents are NOT kept when it has to grow; the free waits for the device: kernels still using the old
    // allocation finish first).  On failure the buffer is left empty and the error is reported like PF_CHECK reports it
    int grow(size_t bytes) {
        if (bytes_ >= bytes) return 0;
        reset();
        const hipError_t e = Mem::alloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return fail(e, Mem::what); }
        bytes_ = bytes;
        return 0;
    }
    void reset() {
        if (p_) (void)Mem::free(p_);
        p_ = nullptr; bytes_ = 0;
    }
private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};
using DevBuf = OwnedBuf<DeviceMem>;
using PinnedBuf = OwnedBuf<PinnedMem>;

// Per-stream scratch of a setup: kernels of one stream serialise, two streams running the same setup concurrently must not share work
// buffers.  `mu` is held by a caller from acquire() until EVERY launch that uses the entry is enqueued: it guards host-side enqueue only,
// and a second thread growing the same stream's buffer can then never free memory whose kernels are not yet in the stream.
// More than MAX_STREAMS streams: ONE entry goes - the stream that used the pool longest ago - not the whole map (a caller cycling through
// nine streams would otherwise free and re-allocate every stream's buffers on every call).  An entry a HIP graph has recorded (`captured`)
// is never the victim, and a buffer it outgrows is retired (kept until the pool goes) instead of freed: a replay dereferences the
// pointers it froze at capture time.
class StreamScratch {
public:
    struct Entry { DevBuf buf[2]; unsigned long long last_use = 0; bool captured = false; };
    static constexpr size_t MAX_STREAMS = 8;
    std::mutex mu;

    // the entry of `st`, created on first use (under mu)
    Entry& acquire(hipStream_t st) {
        if (tab_.size() >= MAX_STREAMS && !tab_.count(st)) {
            auto victim = tab_.end();
            for (auto it = tab_.begin(); it != tab_.end(); ++it)
                if (!it->second.captured && (victim == tab_.end() || it->second.last_use < victim->second.last_use)) victim = it;
            if (victim != tab_.end()) tab_.erase(victim);
        }
        Entry& e = tab_[st];
        e.last_use = ++clock_;
        if (stream_capturing(st)) e.captured = true;
        return e;
    }
    // buffer i of an entry grown to `bytes` (under mu; while the stream is capturing the allocation fails: warm the setup up with the
    // largest batch first)
    int grow(Entry& e, int i, size_t bytes) {
        if (e.captured && e.buf[i] && e.buf[i].bytes() < bytes) retired_.push_back(std::move(e.buf[i]));
        return e.buf[i].grow(bytes);
    }
    void clear() { tab_.clear(); retired_.clear(); }

private:
    std::map<hipStream_t, Entry> tab_;
    unsigned long long clock_ = 0;
    std::vector<DevBuf> retired_;
};

// W_denom^j: every table entry of the library - the angle in extended precision, rounded once
template <typename T>
static cx<T> unit_root(long long j, long long denom) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)j / (long double)denom;
    cx<T> w;
    w.x = (T)cosl(a); w.y = (T)sinl(a);
    return w;
}
// scale * W_denom^j (conj_: its conjugate): the product formed in extended precision, rounded once (the folded tables of fft_dct.h)
template <typename T>
static cx<T> scaled_unit_root(long long j, long long denom, long double scale, bool conj_) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)j / (long double)denom;
    cx<T> w;
    w.x = (T)(scale * cosl(a)); w.y = (T)(scale * (conj_ ? -sinl(a) : sinl(a)));
    return w;
}
template <typename T>
static std::vector<cx<T>> unit_roots(size_t count, long long denom) {
    std::vector<cx<T>> tw(count);
    for (size_t j = 0; j < count; ++j) tw[j] = unit_root<T>((long long)j, denom);
    return tw;
}
template <typename E>
static int upload_table(DevBuf& d, const std::vector<E>& h) {
    const size_t bytes = sizeof(E) * h.size();
    int rc = d.grow(bytes);
    if (rc) return rc;
    const hipError_t e = hipMemcpy(d.get(), h.data(), bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail(e, "hipMemcpy of a twiddle table");
}
// W_denom^j, j < count
template <typename T>
static int upload_roots(DevBuf& d, size_t count, long long denom) { return upload_table(d, unit_roots<T>(count, denom)); }
// the compact per-stage table of a Stockham plan (twmode 2): stage st holds its Ns base twiddles W_{Ns R}^jm from tw_off on
template <typename T>
static int upload_stock_table(DevBuf& d, const StockPlan& sp) {
    std::vector<cx<T>> tc(sp.ctab + 1);
    for (int st = 1; st < sp.ns; ++st) {
        const StockStage& g = sp.st[st];
        for (int jm = 0; jm < g.Ns; ++jm) tc[g.tw_off + jm] = unit_root<T>(jm, (long long)g.Ns * g.R);
    }
    return upload_table(d, tc);
}

}  // namespace pf
