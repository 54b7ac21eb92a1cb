// What a handle owns, one move-only owner of pointer size per kind of resource (host code; rcw_api.hip alone includes it): the destructor gives
// it back, reset() does so early, get() lends the raw pointer.  The allocating members carry the runtime call's name: RCW_HIP's message quotes it.
#pragma once
#include <hip/hip_runtime.h>

class RcwBuf {   // hipMalloc / hipFree
    void* p_ = nullptr;
public:
    RcwBuf() = default;  RcwBuf(RcwBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    RcwBuf& operator=(RcwBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~RcwBuf() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    hipError_t hipMalloc(size_t bytes) { reset(); const hipError_t e = ::hipMalloc(&p_, bytes); if (e != hipSuccess) p_ = nullptr; return e; }
    template <typename T = void> T* get() const { return static_cast<T*>(p_); }
};

class RcwPinned {   // hipHostMalloc / hipHostFree
    void* p_ = nullptr;
public:
    RcwPinned() = default;  RcwPinned(RcwPinned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    RcwPinned& operator=(RcwPinned&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~RcwPinned() { reset(); }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
    hipError_t hipHostMalloc(size_t bytes) { reset(); const hipError_t e = ::hipHostMalloc(&p_, bytes, hipHostMallocDefault); if (e != hipSuccess) p_ = nullptr; return e; }
    template <typename T = void> T* get() const { return static_cast<T*>(p_); }
};

class RcwStream {   // hipStreamCreateWithFlags(hipStreamNonBlocking) / hipStreamDestroy
    hipStream_t s_ = nullptr;
public:
    RcwStream() = default;  RcwStream(RcwStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    ~RcwStream() { reset(); }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    hipError_t hipStreamCreate() { reset(); const hipError_t e = ::hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); if (e != hipSuccess) s_ = nullptr; return e; }
    hipStream_t get() const { return s_; }
};

class RcwEvent {   // hipEventCreateWithFlags / hipEventDestroy
    hipEvent_t e_ = nullptr;
public:
    RcwEvent() = default;  RcwEvent(RcwEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    RcwEvent& operator=(RcwEvent&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~RcwEvent() { reset(); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipError_t hipEventCreate(unsigned flags = hipEventDefault) { reset(); const hipError_t e = ::hipEventCreateWithFlags(&e_, flags); if (e != hipSuccess) e_ = nullptr; return e; }
    hipEvent_t get() const { return e_; }
};
