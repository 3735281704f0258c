// buffers.hpp -- HIP status handling and the owners of device memory, pinned host memory and events behind both handles.
// A handle holds these as members: what it owns goes when it is deleted.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <type_traits>

#include "../../include/lbaudiodetective.h"

namespace lbad {

OSStatus hip_status(hipError_t e, const char* what, int line);
#define LBAD_HIP(expr)                                                   \
    do {                                                                 \
        OSStatus st__ = ::lbad::hip_status((expr), #expr, __LINE__);     \
        if (st__ != noErr) return st__;                                  \
    } while (0)

// bytes the buffers below hold right now: [0] device, [1] pinned (LBAudioDetectiveDebugLiveBytes)
inline std::atomic<uint64_t> g_live_bytes[2];

// A block of device (Pinned == false) or pinned host memory: a pointer and a capacity in elements of T (bytes for void).
// Move-only.  An empty buffer calls no HIP function, not in reserve(0) and not in its destructor.
template <typename T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    // room for n elements, exactly: nothing happens when there is; otherwise the old block goes first, and a failed
    // allocation leaves the buffer empty.  flags: hipHostMalloc's (pinned only)
    OSStatus reserve(size_t n, unsigned flags = hipHostMallocDefault) {
        if (cap_ >= n) return noErr;
        reset();
        void* p = nullptr;
        LBAD_HIP(Pinned ? hipHostMalloc(&p, n * kElem, flags) : hipMalloc(&p, n * kElem));
        p_ = static_cast<T*>(p);
        cap_ = n;
        g_live_bytes[Pinned] += n * kElem;
        return noErr;
    }
    // the same with a quarter more than asked for (the detective's io, converter and file blocks, which grow call by call)
    OSStatus reserve_slack(size_t n) { return cap_ >= n ? noErr : reserve(n + n / 4); }
    void reset() {
        if (!p_) return;
        (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        g_live_bytes[Pinned] -= cap_ * kElem;
        p_ = nullptr;
        cap_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }

private:
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

// A device block and the pinned block it is filled from, always sized together: after a failed reserve neither half is
// there and the capacity is 0.
template <typename T>
struct StagingPair {
    DeviceBuffer<T> dev;
    PinnedBuffer<T> host;
    size_t capacity() const { return host.capacity(); }
    OSStatus reserve(size_t n) {
        if (capacity() >= n) return noErr;
        dev.reset();
        host.reset();
        OSStatus st = dev.reserve(n);
        if (st == noErr) st = host.reserve(n);
        if (st != noErr) dev.reset();
        return st;
    }
};

// An event that orders the reuse of a scratch block: made on first use, recorded behind the last kernel that touches the block.
// The destructor destroys the event and NEVER waits for it: what a Dispose has to await it awaits by name, before any memory
// goes -- an event may sit behind work that never finishes (the sharded query's collective, api_rccl.cpp).
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    OSStatus create() {
        if (!ev) LBAD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return noErr;
    }
    OSStatus wait() const {
        if (ev) LBAD_HIP(hipEventSynchronize(ev));
        return noErr;
    }
    OSStatus wait_or_create() { return ev ? wait() : create(); }
    OSStatus record(hipStream_t stream) {
        LBAD_HIP(hipEventRecord(ev, stream));
        return noErr;
    }
    operator hipEvent_t() const { return ev; }
};

}  // namespace lbad
