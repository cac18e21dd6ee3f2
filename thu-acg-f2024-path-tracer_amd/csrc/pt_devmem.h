// Device memory of the host runtime (host-only): the two ways the library holds a hipMalloc allocation.
//   DevMem  : one allocation for the length of a call, freed when it goes out of scope.
//   GrowBuf : a buffer cached on a scene or communicator and re-used by later calls; it only ever grows.
// Both report a failure through hip_ok under the caller's label ("hipMalloc(path pool)", ...) and hold bytes, never words.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace pt {

bool hip_ok(hipError_t e, const char* what);   // pt_scene_upload.cpp

class DevMem {
    void* p_ = nullptr;

public:
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    ~DevMem() { release(); }
    // A request of 0 bytes succeeds and allocates a few: an empty input or output still has a pointer to hand to a launcher.
    bool alloc(size_t bytes, const char* what) {
        release();
        if (hip_ok(hipMalloc(&p_, bytes ? bytes : 8), what)) return true;
        p_ = nullptr;
        return false;
    }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    template <class T>
    T* as() const { return (T*)p_; }
    explicit operator bool() const { return p_ != nullptr; }
};

class GrowBuf {
    void* p_ = nullptr;
    size_t cap_ = 0;
    bool pinned_host_;   // hipHostMalloc / hipHostFree in place of hipMalloc / hipFree

public:
    explicit GrowBuf(bool pinned_host = false) : pinned_host_(pinned_host) {}
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { release(); }
    // At least `bytes` of capacity: nothing to do when it is there, else the old buffer is freed and forgotten BEFORE the new one is
    // asked for (the two need not fit side by side), and the new capacity counts only once the allocation has succeeded.
    bool reserve(size_t bytes, const char* what) {
        if (bytes <= cap_) return true;
        release();
        if (!hip_ok(pinned_host_ ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes), what)) {
            p_ = nullptr;
            return false;
        }
        cap_ = bytes;
        return true;
    }
    void release() {
        if (p_) (void)(pinned_host_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    template <class T>
    T* as() const { return (T*)p_; }
    explicit operator bool() const { return p_ != nullptr; }
};

}  // namespace pt
