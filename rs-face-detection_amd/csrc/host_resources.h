// host_resources.h -- what the host layer (detector.hip and the *_host.h layers next to it) owns, by type: device buffer, page-locked block, event,
// stream, and the ring of page-locked slots that per-call descriptors travel through.  Host only.  A holder frees in its
// destructor and cannot be copied; creating what is already held is a no-op, so a "first call" may simply ask again.
#pragma once
#include "rfd_common.h"

namespace rfd {

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

struct DevBuf : NoCopy {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    int reserve(size_t bytes) // grows by freeing, then allocating: the contents are never carried over
    {
        if (bytes <= cap) return RFD_OK;
        if (p) RFD_HIP(hipFree(p));
        p = nullptr; cap = 0;
        RFD_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return RFD_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

template <class T> struct Pinned : NoCopy { // page-locked host memory, `count` elements of T
    T *p = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    int alloc(size_t count)
    {
        if (!p) RFD_HIP(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
        return RFD_OK;
    }
    operator T *() const { return p; }
};

struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags = hipEventDisableTiming) // hipEventDefault: one that hipEventElapsedTime accepts
    {
        if (!e) RFD_HIP(hipEventCreateWithFlags(&e, flags));
        return RFD_OK;
    }
    operator hipEvent_t() const { return e; }
};

struct Stream : NoCopy { // non-blocking: not ordered with the NULL stream
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    int create()
    {
        if (!s) RFD_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return RFD_OK;
    }
    operator hipStream_t() const { return s; }
};

// kSlots page-locked slots, each with the event of the last copy out of it.  A call takes the next slot, waits until that copy
// has run (kSlots calls ago: in practice never), fills the slot, enqueues its copies and records; so enqueueing never waits
// for the previous call, and the slot may still be read by a pending copy when the call returns.
template <int kSlots> struct PinnedRing {
    Pinned<char> slot[kSlots];
    Event done[kSlots];
    int next = 0, cur = 0;
    int ensure(size_t bytes_per_slot, unsigned event_flags = hipEventDisableTiming)
    {
        for (int i = 0; i < kSlots; ++i) {
            RFD_TRY(slot[i].alloc(bytes_per_slot));
            RFD_TRY(done[i].create(event_flags));
        }
        return RFD_OK;
    }
    template <class T> int acquire(T **p)
    {
        cur = next;
        next = (next + 1) % kSlots;
        RFD_HIP(hipEventSynchronize(done[cur])); // the copy that last used this slot has run
        *p = (T *)slot[cur].p;
        return RFD_OK;
    }
    int record(hipStream_t stream) // behind the copies out of the slot acquire() handed out last
    {
        RFD_HIP(hipEventRecord(done[cur], stream));
        return RFD_OK;
    }
};

} // namespace rfd
