// A fake of the handful of HIP runtime calls facedeform_amd/csrc/fd_owned.h uses, for tests/tools/owned_check.cpp: malloc behind
// every resource, a log of the calls in order, a table of what is live and how often each was released, and a switch that makes
// the n-th allocation or creation from now fail.  One translation unit only.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0;
typedef struct FakeEvent *hipEvent_t;
typedef struct FakeStream *hipStream_t;
typedef struct FakeGraphExec *hipGraphExec_t;

namespace fake {
inline std::vector<std::string> log;               // the runtime calls, in order
inline std::map<void *, int> released;             // every resource handed out -> times released
inline std::map<void *, size_t> bytes;             // the size asked for
inline int fail_in = 0;                            // > 0: the fail_in-th allocation / creation from now fails
inline hipError_t last_error = hipSuccess;

inline hipError_t make(const char *call, void **out, size_t n)
{
    log.push_back(call);
    if (fail_in > 0 && --fail_in == 0) {
        *out = (void *)(size_t)0xdead;             // what a careless owner would keep
        return last_error = hipErrorOutOfMemory;
    }
    *out = malloc(n ? n : 1);
    released[*out] = 0;
    bytes[*out] = n;
    return hipSuccess;
}
inline hipError_t drop(const char *call, void *p)
{
    log.push_back(call);
    if (!released.count(p) || released[p] != 0) { released[p] += 1; return last_error = 1; }     // unknown, or released twice
    released[p] = 1;
    free(p);
    return hipSuccess;
}
inline size_t live()
{
    size_t n = 0;
    for (const auto &r : released) n += r.second == 0;
    return n;
}
inline bool all_released_once()
{
    for (const auto &r : released)
        if (r.second != 1) return false;
    return true;
}
inline hipGraphExec_t graph_exec()                 // the header creates none: fd_capi.hip's ensure_graph instantiates into the owner
{
    void *p;
    (void)make("hipGraphInstantiate", &p, 1);
    return (hipGraphExec_t)p;
}
}  // namespace fake

inline hipError_t hipMalloc(void **p, size_t n) { return fake::make("hipMalloc", p, n); }
inline hipError_t hipFree(void *p) { return fake::drop("hipFree", p); }
inline hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return fake::make("hipHostMalloc", p, n); }
inline hipError_t hipHostFree(void *p) { return fake::drop("hipHostFree", p); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return fake::make("hipEventCreateWithFlags", (void **)e, 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake::drop("hipEventDestroy", e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return fake::make("hipStreamCreateWithFlags", (void **)s, 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake::drop("hipStreamDestroy", s); }
inline hipError_t hipGraphExecDestroy(hipGraphExec_t g) { return fake::drop("hipGraphExecDestroy", g); }
inline hipError_t hipGetLastError()
{
    fake::log.push_back("hipGetLastError");
    const hipError_t e = fake::last_error;
    fake::last_error = hipSuccess;
    return e;
}
