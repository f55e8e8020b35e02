// host_common.h -- host-side plumbing shared by the handles and operator entry points of libl3hip.so: the error return of an
// operator, the "is this device there?" check, the bfloat16 read-back widening, and the one owner of hipMalloc'ed memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

namespace l3 {

void set_op_error(const std::string& msg);       // engine.hip: l3_last_error(NULL) of an entry point without an engine

// ... and its return code
inline int fail(int code, const std::string& msg) {
    set_op_error(msg);
    return code;
}

// the device exists and is now the calling thread's current device
inline bool device_ok(int device) {
    int n = 0;
    return device >= 0 && hipGetDeviceCount(&n) == hipSuccess && device < n && hipSetDevice(device) == hipSuccess;
}

inline std::string no_gpu_message(const char* fn, int device) {
    return std::string(fn) + ": HIP device " + std::to_string(device) + " not available (libl3hip needs an AMD GPU)";
}

// TensorFlow 'SAME' padding: output length and the padding in front, for n inputs, window k, stride s
inline void tf_same(int n, int k, int s, int* out, int* before) {
    *out = (n + s - 1) / s;
    int total = (*out - 1) * s + k - n;
    if (total < 0) total = 0;
    *before = total / 2;
}

// bfloat16 storage read back as the float of the same value
inline void widen_bf16(float* dst, const uint16_t* src, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t u = (uint32_t)src[i] << 16;
        memcpy(dst + i, &u, 4);
    }
}

// Owner of device buffers: whatever alloc / put / grow handed out and release has not taken back is freed by clear() or the
// destructor.  It selects no device and never synchronises: its owner makes the device current and waits for whatever may still
// use a buffer before that buffer goes (hipFree itself waits for the device).
class DeviceBufs {
public:
    DeviceBufs() = default;
    DeviceBufs(const DeviceBufs&) = delete;
    DeviceBufs& operator=(const DeviceBufs&) = delete;
    ~DeviceBufs() { clear(); }

    // nullptr on failure; a zero count still gives a small buffer, so no caller meets a null pointer
    template <class T>
    T* alloc(size_t count) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes_of<T>(count)) != hipSuccess) return failed<T>();
        owned_.push_back(p);
        return static_cast<T*>(p);
    }
    // alloc + asynchronous copy of `count` elements on s: `host` must stay valid until s has consumed it
    template <class T>
    T* put(const T* host, size_t count, hipStream_t s) {
        T* d = alloc<T>(count);
        if (d && count > 0 && hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess) {
            release(d);
            return failed<T>();
        }
        return d;
    }
    void release(void* p) {
        if (!p) return;
        for (size_t i = 0; i < owned_.size(); ++i)
            if (owned_[i] == p) {
                owned_[i] = owned_.back();
                owned_.pop_back();
                (void)hipFree(p);
                return;
            }
    }
    // *p holds at least `count` elements afterwards, or is null (and *cap 0) if the allocation failed.  Reallocates only when
    // count > *cap (or nothing was allocated yet); returns whether *p is a new, empty buffer: whatever the caller had cached in
    // the old one is gone.
    template <class T>
    bool grow(T** p, size_t* cap, size_t count) {
        if (*p != nullptr && count <= *cap) return false;
        release(*p);
        *cap = 0;
        *p = alloc<T>(count);
        if (*p) *cap = count;
        return *p != nullptr;
    }
    void clear() {
        for (void* p : owned_) (void)hipFree(p);
        owned_.clear();
    }
    bool ok() const { return ok_; }          // no alloc / put / grow has failed so far: one check after a run of them
    template <class T>
    static size_t bytes_of(size_t count) { return (count ? count : 4) * sizeof(T); }

private:
    template <class T>
    T* failed() {
        ok_ = false;
        return nullptr;
    }
    std::vector<void*> owned_;
    bool ok_ = true;
};

}  // namespace l3
