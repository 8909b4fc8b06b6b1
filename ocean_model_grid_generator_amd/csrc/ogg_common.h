// Host-side plumbing shared by the translation units of libogg_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ogg_hip.h"

namespace ogg {

int set_error(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// OGG_SYM_DEFAULT / OGG_SYM_MIRROR / OGG_SYM_NONE of a caller -> mirror the caps' columns or not (include/ogg_hip.h)
bool cap_symmetry(int requested);

// Scratch from the stream-ordered allocator (no host synchronisation), returned to it on EVERY exit path of the call.
class AsyncScratch {
   public:
    explicit AsyncScratch(hipStream_t s) : s_(s) {}
    AsyncScratch(const AsyncScratch&) = delete;
    AsyncScratch& operator=(const AsyncScratch&) = delete;
    ~AsyncScratch() {
        if (p_) (void)hipFreeAsync(p_, s_);
    }
    int alloc(void** out, size_t bytes) {
        hipError_t e = hipMallocAsync(&p_, bytes ? bytes : 1, s_);
        if (e != hipSuccess) {
            p_ = nullptr;
            return set_error(e == hipErrorOutOfMemory ? OGG_ENOMEM : OGG_EHIP, "hipMallocAsync(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        }
        *out = p_;
        return OGG_OK;
    }

   private:
    void* p_ = nullptr;
    hipStream_t s_;
};

}  // namespace ogg

#define OGG_HIP_CHECK(expr)                                                                              \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess)                                                                           \
            return ogg::set_error(OGG_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define OGG_LAUNCH_CHECK() OGG_HIP_CHECK(hipGetLastError())

#define OGG_REQUIRE(cond, code, ...)                      \
    do {                                                  \
        if (!(cond)) return ogg::set_error(code, __VA_ARGS__); \
    } while (0)

namespace ogg {

// hipMalloc'd buffers of a host-pointer entry, freed on EVERY exit path of the call (the synchronous sibling of AsyncScratch).
class Buffers {
   public:
    Buffers() = default;
    Buffers(const Buffers&) = delete;
    Buffers& operator=(const Buffers&) = delete;
    ~Buffers() {
        for (void* q : p_) (void)hipFree(q);
    }
    // a buffer of n elements of T (a workspace of n bytes is n chars)
    template <typename T>
    int alloc(T** out, size_t n) {
        const size_t bytes = n * sizeof(T);
        hipError_t e = hipMalloc(out, bytes ? bytes : 8);
        if (e != hipSuccess)
            return set_error(e == hipErrorOutOfMemory ? OGG_ENOMEM : OGG_EHIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        p_.push_back(*out);
        return OGG_OK;
    }
    // n elements from host memory into a buffer (send), or back (get); put: a new buffer holding a copy of n elements of host memory
    template <typename T>
    static int send(T* dev, const T* host, size_t n) {
        OGG_HIP_CHECK(hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice));
        return OGG_OK;
    }
    template <typename T>
    static int get(T* host, const T* dev, size_t n) {
        OGG_HIP_CHECK(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
        return OGG_OK;
    }
    template <typename T>
    int put(T** out, const T* host, size_t n) {
        if (int e = alloc(out, n)) return e;
        return send(*out, host, n);
    }

   private:
    std::vector<void*> p_;
};

// the sections of a workspace, one after the other from ``off`` on 256-byte boundaries (the exchange grid's: 64): take(bytes) gives
// the next section's offset, and after the last take off is the size of the whole
struct Sections {
    long off, align = 256;
    long take(long bytes) {
        const long o = off;
        off += (bytes + align - 1) / align * align;
        return o;
    }
};

// the one refusal of a workspace that is missing or too small for the call ``who``
inline int check_workspace(const char* who, const void* ws, long wsb, long need) {
    OGG_REQUIRE(ws && wsb >= need, OGG_EARG, "%s: workspace of %ld bytes, %ld needed", who, wsb, need);
    return OGG_OK;
}

// a typed pointer into a workspace
template <typename P>
P* at(void* ws, long off) { return reinterpret_cast<P*>(static_cast<char*>(ws) + off); }
template <typename P>
const P* at(const void* ws, long off) { return reinterpret_cast<const P*>(static_cast<const char*>(ws) + off); }

// workgroups of NT threads for n items of a grid-stride loop: at least one, at most cap
template <int NT>
unsigned grid_for(long n, long cap) { return (unsigned)std::min<long>(std::max<long>((n + NT - 1) / NT, 1), cap); }

// an environment knob: def when unset, else the whole string must be an integer in lo .. hi (a pure host read, done when a call is
// set up, before any device work)
inline int knob(const char* name, int def, int lo, int hi, int* out) {
    *out = def;
    if (const char* e = getenv(name)) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        OGG_REQUIRE(end != e && *end == '\0' && v >= lo && v <= hi, OGG_EARG, "%s=%s: an integer %d .. %d", name, e, lo, hi);
        *out = (int)v;
    }
    return OGG_OK;
}

}  // namespace ogg
