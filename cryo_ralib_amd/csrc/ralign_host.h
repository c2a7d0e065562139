// Host-side plumbing shared by the library's translation units: the last-error string, the HIP error macros, the check in front of
// every dynamic-LDS raise and the owner of stream-ordered scratch.  Host code only -- no kernels -- and nothing here is exported:
// everything between the visibility pragmas stays out of the dynamic symbol table.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/ralign.h"

// the MFMA operand type of the kernel headers (ralign_kernels.h declares the same), for the files that do not include that one
namespace ralign { typedef float f32x4 __attribute__((ext_vector_type(4))); }

#pragma GCC visibility push(hidden)

// the thread's last-error string (ra_last_error); its one definition lives in ralign_engine.hip
void set_error(const std::string &msg);

// the message as the last error; returns RA_ERR_ARG
inline int arg_error(const char *msg) { set_error(msg); return RA_ERR_ARG; }

// "<what>: <HIP's text>" as the last error; returns RA_ERR_HIP
inline int hip_error(const char *what, hipError_t he)
{
    set_error(std::string(what) + ": " + hipGetErrorString(he));
    return RA_ERR_HIP;
}

// return from the calling function with "<call> failed: <HIP's text> (<file>:<line>)" unless the call succeeds
#define RA_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t err__ = (call);                                                            \
        if (err__ != hipSuccess) {                                                            \
            char buf__[512];                                                                  \
            snprintf(buf__, sizeof(buf__), "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), \
                     __FILE__, __LINE__);                                                     \
            set_error(buf__);                                                                 \
            return RA_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

// a kernel launch in a chain of steps that stops at the first failure: skipped unless `he` is still hipSuccess
#define RA_LAUNCH(he, ...) do { if ((he) == hipSuccess) { hipLaunchKernelGGL(__VA_ARGS__); (he) = hipGetLastError(); } } while (0)

// Every site that raises a kernel's dynamic LDS goes through here.  The host rules that size the dynamic part know nothing of the
// __shared__ arrays a kernel declares: the static size is read from the loaded code object and the sum compared with what a
// workgroup of this device can have, BEFORE anything is launched -- a kernel that gains a static array then fails here, by name,
// instead of in a launch.  This is the form of the engine-less entry points (no engine: nullptr); the engine's own overload adds
// the row of its ledger from *stat and *limit (ra_lds_report).
int raise_dynamic_lds(std::nullptr_t, const void *fn, const char *name, size_t dyn, int *stat = nullptr, int *limit = nullptr);
#define RA_LDS(e, kernel, dyn) raise_dynamic_lds(e, (const void *)(kernel), #kernel, dyn)

// what the reference-compatible surface needs of an engine without seeing its struct (ralign_engine.hip): the mode of the next
// search, and the device workspace ra_create plans for a config in bytes ((size_t)-1: bad geometry)
void ra_engine_switch_mode(ra_engine *e, int mode);
size_t ra_planned_workspace_bytes(const ra_config *rc);

// Scratch of one entry point on its stream: get() allocates stream-ordered, the destructor frees on the same stream, so every
// exit path releases everything.  The first failure stays as status(); later get()s return nullptr without calling HIP.
class StreamScratch {
public:
    explicit StreamScratch(hipStream_t stream) : stream_(stream) {}
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
    ~StreamScratch() { for (size_t i = ptrs_.size(); i-- > 0;) (void)hipFreeAsync(ptrs_[i], stream_); }
    template <class T> T *get(size_t count)
    {
        void *p = nullptr;
        if (status_ != hipSuccess || (status_ = hipMallocAsync(&p, count * sizeof(T), stream_)) != hipSuccess) return nullptr;
        ptrs_.push_back(p);
        return (T *)p;
    }
    hipError_t status() const { return status_; }

private:
    hipStream_t stream_;
    hipError_t status_ = hipSuccess;
    std::vector<void *> ptrs_;
};

#pragma GCC visibility pop
