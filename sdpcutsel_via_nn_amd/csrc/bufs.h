// The two owners of the library's device and pinned host memory.  Move-only; the destructor frees.  Nothing here knows the
// handle: whoever grows a buffer under launches in flight waits first (common.h: grow).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

// a device array of `size()` elements of T
template <class T> class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }
    // frees what it holds, then allocates `count` elements; on failure it ends empty
    hipError_t reset(size_t count)
    {
        release();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = (T *)q; n_ = count;
        return hipSuccess;
    }
    void release()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
};

// pinned host memory of `size()` bytes: mapped (the device reads and writes it through dev()) or default (the source or
// target of hipMemcpyAsync; dev() is NULL)
class HostBuf {
    void *p_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;
    bool mapped_;

public:
    explicit HostBuf(bool mapped) : mapped_(mapped) {}
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept : p_(o.p_), dev_(o.dev_), n_(o.n_), mapped_(o.mapped_) { o.p_ = o.dev_ = nullptr; o.n_ = 0; }
    HostBuf &operator=(HostBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; dev_ = o.dev_; n_ = o.n_; mapped_ = o.mapped_;
            o.p_ = o.dev_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~HostBuf() { release(); }

    void *get() const { return p_; }
    void *dev() const { return dev_; }
    size_t size() const { return n_; }
    hipError_t reset(size_t bytes)
    {
        release();
        void *q = nullptr;
        hipError_t e = hipHostMalloc(&q, bytes, mapped_ ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (mapped_ && (e = hipHostGetDevicePointer(&dev_, q, 0)) != hipSuccess) {
            (void)hipHostFree(q);
            dev_ = nullptr;
            return e;
        }
        p_ = q; n_ = bytes;
        return hipSuccess;
    }
    void release()
    {
        if (p_) (void)hipHostFree(p_);
        p_ = dev_ = nullptr; n_ = 0;
    }
};
