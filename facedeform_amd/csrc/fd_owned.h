// fd_owned.h -- owners of what the host layer holds on the device: buffers, page-locked blocks, events, streams, graph
// executables.  Each is a plain value member of the handle that owns the resource (fd_ctx, fd_batch, fd_shot_dev, fd_morph)
// and releases it when the handle is deleted, members in reverse order of declaration: a stream is declared before whatever is
// enqueued on it.  None can be copied, so one that would be deduced into a variadic launch (hipLaunchKernelGGL) does not
// compile: pass its member there, and wherever the address of the pointer is taken.  Otherwise an owner converts to its raw
// pointer or handle.  Every function returns the runtime's own result and drains nothing; the error texts and codes stay with
// the callers.  A handle that is borrowed from another owner stays a raw hipEvent_t / hipStream_t / pointer, and says so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fd {

template <typename T> struct OwnedElem { static constexpr size_t bytes = sizeof(T); };
template <> struct OwnedElem<void> { static constexpr size_t bytes = 1; };      // the void * scratches count bytes

// A device buffer of `cap` elements (bytes for DevBuf<void>).  It only ever grows: cap is 0 while p is being replaced, so a
// failed allocation leaves no capacity behind for a later, smaller request to trust (hipFree drains the device: nothing reads
// the old block when the new one is handed out).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    operator T *() const { return p; }

    void reset()
    {
        cap = 0;
        if (p) { (void)hipFree(p); p = nullptr; }
    }
    // a new block of max(count, 1) elements, whatever is held; for buffers whose capacity is kept elsewhere, one for several
    hipError_t alloc(size_t count)
    {
        reset();
        if (count == 0) count = 1;
        const hipError_t e = hipMalloc((void **)&p, count * OwnedElem<T>::bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = count;
        return hipSuccess;
    }
    hipError_t grow(size_t count) { return count <= cap ? hipSuccess : alloc(count); }
};

// `count` page-locked elements
template <typename T>
struct Pinned {
    T *p = nullptr;

    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned() { reset(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }

    void reset()
    {
        if (p) { (void)hipHostFree(p); p = nullptr; }
    }
    hipError_t alloc(size_t count, unsigned flags)
    {
        reset();
        const hipError_t e = hipHostMalloc((void **)&p, (count ? count : 1) * OwnedElem<T>::bytes, flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    // a block that leaves through the C ABI (fd_host_alloc) and comes back through it (fd_host_free)
    T *release() { T *q = p; p = nullptr; return q; }
    void adopt(T *q) { reset(); p = q; }
};

struct Event {
    hipEvent_t ev = nullptr;

    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    operator hipEvent_t() const { return ev; }

    // for the events a handle creates up front: the runtime's result, nothing drained
    hipError_t create(unsigned flags)
    {
        const hipError_t e = hipEventCreateWithFlags(&ev, flags);
        if (e != hipSuccess) ev = nullptr;
        return e;
    }
    // created on first use, and only then; a failure is drained and leaves it null
    bool make(unsigned flags = hipEventDisableTiming)
    {
        if (ev) return true;
        if (create(flags) != hipSuccess) { (void)hipGetLastError(); return false; }
        return true;
    }
};

struct Stream {
    hipStream_t s = nullptr;

    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }

    hipError_t create(unsigned flags = hipStreamNonBlocking)
    {
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e != hipSuccess) s = nullptr;
        return e;
    }
};

struct GraphExec {
    hipGraphExec_t exec = nullptr;

    GraphExec() = default;
    GraphExec(const GraphExec &) = delete;
    GraphExec &operator=(const GraphExec &) = delete;
    ~GraphExec() { reset(); }
    operator hipGraphExec_t() const { return exec; }

    void reset()
    {
        if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    }
};

}  // namespace fd
