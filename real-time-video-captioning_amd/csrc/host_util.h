// Host-side helpers shared by the C-ABI translation units (gitcap.hip, student.hip, tinyvit.hip): the part of a handle the
// three have in common and the plumbing that goes with it (error text, device selection, tracked allocations, weight upload).
#pragma once
#include <hip/hip_runtime.h>

#include "host_logic.h"      // pad_to, host_f2bf, e4m3 encodings, tensor table (HIP-free: also built under ASan for the CPU)

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

// What gitcap, gitcap_student and gitcap_tinyvit derive from.
struct HandleCore {
    int device = 0;
    mutable std::string err;        // *_last_error(handle)
    std::vector<void*> allocs;      // device buffers of dev_alloc, freed by free_allocs
    int64_t ws_bytes = 0;           // their bytes
};

// *_last_error(NULL): the message of the last failed create or null-handle call of handle type H (one string per type)
template <class H>
std::string& create_err() {
    static std::string s;
    return s;
}

// Records the message on the handle, or (h == nullptr: spell the type, fail<gitcap>(nullptr, ...)) as H's create error.
template <class H>
int fail(const H* h, int code, const std::string& msg) {
    (h ? h->err : create_err<H>()) = msg;
    return code;
}

#define HIP_OK(h, expr)                                                                               \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(h, GITCAP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// status of a gitcap_dbg_* hook from its launcher's: a launcher refuses arguments with hipErrorInvalidValue
inline int dbg_rc(hipError_t e) { return e == hipSuccess ? 0 : (e == hipErrorInvalidValue ? GITCAP_ERR_ARG : GITCAP_ERR_HIP); }

// Makes a handle's device current for the duration of an entry point and restores the caller's.
struct DeviceGuard {
    int prev = -1; bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define GUARD(h) DeviceGuard guard_((h)->device); if (!guard_.ok) return fail(h, GITCAP_ERR_HIP, "cannot select the handle's device")

// A zero-filled device buffer of `count` T that lives as long as the handle.
template <class H, typename T>
int dev_alloc(H* h, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, GITCAP_ERR_NOMEM, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
    e = hipMemset(q, 0, bytes);
    if (e != hipSuccess) return fail(h, GITCAP_ERR_HIP, std::string("hipMemset workspace: ") + hipGetErrorString(e));
    h->allocs.push_back(q);
    h->ws_bytes += (int64_t)bytes;
    *p = (T*)q;
    return 0;
}

inline void free_allocs(HandleCore& c) {
    for (void* p : c.allocs) (void)hipFree(p);
    c.allocs.clear();
}

// A GEMM weight's upload: fp32 [rows][cols] -> t.p = bf16 [rows padded to a multiple of row_pad][pitch], zero padded
// (pitch >= cols), t.bytes = its size.  On failure the tensor holds nothing (t.p null, not loaded, t.bytes untouched).
template <class H>
int upload_bf16_panel(H* h, DevTensor& t, const float* data, int64_t rows, int64_t cols, int row_pad, int64_t pitch) {
    std::vector<uint16_t> hb((size_t)pad_to((int)rows, row_pad) * pitch, 0);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t k = 0; k < cols; ++k) hb[(size_t)(r * pitch + k)] = host_f2bf(data[r * cols + k]);
    HIP_OK(h, hipMalloc(&t.p, hb.size() * 2));
    const hipError_t e = hipMemcpy(t.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(t.p); t.p = nullptr; t.loaded = false;
        return fail(h, GITCAP_ERR_HIP, std::string("hipMemcpy(t.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice): ") + hipGetErrorString(e));
    }
    t.bytes = (int64_t)hb.size() * 2;
    return 0;
}

// The attachment of *_attach_token_logprobs (LpAttach, host_logic.h) is taken, and with that consumed, by every greedy-family
// entry point before its argument checks.  `who` leads the message ("greedy", "student_greedy", ...).
template <class H>
int lp_check(H* h, const char* who, const LpAttach& lp, int max_len) {
    if (lp.p && lp.ld < max_len) return fail(h, GITCAP_ERR_ARG, std::string(who) + ": the attached token log-probability buffer has ld < max_len");
    return 0;
}

// The attachment of *_attach_top_logprobs (TopkAttach, host_logic.h): the setter's argument check (0 = fine; a clearing call never
// gets here), and the taking call's check of the row pitch against the positions it writes.
inline const char* tk_attach_bad(int k, const int64_t* ids, const float* lp, int ld) {
    if (k < 1 || k > 32) return "k outside [1, 32]";
    if (ld < 1 || ((uintptr_t)ids & 7) != 0 || ((uintptr_t)lp & 3) != 0) return "ld < 1 or a misaligned pointer";
    return nullptr;
}
template <class H>
int tk_check(H* h, const char* who, const TopkAttach& tk, int positions) {
    if (tk.k && tk.ld < positions) return fail(h, GITCAP_ERR_ARG, std::string(who) + ": the attached top-k buffers have ld < the positions the call writes");
    return 0;
}

// The draft of the *_greedy_draft entry points of both handles: ids [B][ld], columns 1..n the draft's tokens; accepted_out nullable.
struct Draft { const int64_t* ids; int ld, n; int32_t* accepted_out; };

// Ordering of a window ring's pushes and reads, whichever streams they are issued on: a push waits for the last read and the
// last push (they share the staging rows) and records the ring event; a read waits for the ring event and records the read event.
struct RingOrder {
    hipEvent_t ev_ring = nullptr, ev_read = nullptr;
    bool ring_rec = false, read_rec = false;
    hipError_t ensure() {       // lazy create
        const hipError_t e = ev_ring ? hipSuccess : hipEventCreateWithFlags(&ev_ring, hipEventDisableTiming);
        return e != hipSuccess || ev_read ? e : hipEventCreateWithFlags(&ev_read, hipEventDisableTiming);
    }
    hipError_t before_push(hipStream_t s) {
        const hipError_t e = read_rec ? hipStreamWaitEvent(s, ev_read, 0) : hipSuccess;
        return e == hipSuccess && ring_rec ? hipStreamWaitEvent(s, ev_ring, 0) : e;
    }
    hipError_t after_push(hipStream_t s) { const hipError_t e = hipEventRecord(ev_ring, s); ring_rec |= e == hipSuccess; return e; }
    hipError_t before_read(hipStream_t s) { return hipStreamWaitEvent(s, ev_ring, 0); }     // a full ring has been pushed to
    hipError_t after_read(hipStream_t s) { const hipError_t e = hipEventRecord(ev_read, s); read_rec |= e == hipSuccess; return e; }
    void destroy() {
        if (ev_ring) (void)hipEventDestroy(ev_ring);
        if (ev_read) (void)hipEventDestroy(ev_read);
        ev_ring = ev_read = nullptr;
    }
};

// A table the host plans for a launch, on its way to the device: one page-locked int32 buffer and the event "the previous transfer
// has read it".  Every use is wait(), fill p, copy() once or more, mark(); the device buffer is the user's.
struct HostStage {
    int32_t* p = nullptr;
    hipEvent_t ev = nullptr;
    hipError_t ensure(size_t words) {       // lazy create
        const hipError_t e = p ? hipSuccess : hipHostMalloc((void**)&p, words * sizeof(int32_t), hipHostMallocDefault);
        return e != hipSuccess || ev ? e : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    }
    hipError_t wait() { return ev ? hipEventSynchronize(ev) : hipSuccess; }        // (an event never recorded is complete)
    // words o .. o + n - 1 -> dev
    hipError_t copy(int32_t* dev, size_t o, size_t n, hipStream_t s) { return hipMemcpyAsync(dev, p + o, n * sizeof(int32_t), hipMemcpyHostToDevice, s); }
    hipError_t mark(hipStream_t s) { return hipEventRecord(ev, s); }
    void destroy() { if (p) (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); p = nullptr; ev = nullptr; }
};
