// device_buf.h — RAII device buffer and the HIP error check shared by the C-ABI and the builder; how a set of buffers grows
// under kernels that may still read it (Reserve) and how a call's small host tables reach the device (StagedTable).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <stdexcept>
#include <string>

namespace cph {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            if (e_ == hipErrorOutOfMemory) throw std::bad_alloc();                        \
            throw ::cph::HipError(std::string("HIP error: ") + hipGetErrorString(e_) + " at " + #expr); \
        }                                                                                 \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    void alloc(size_t count) {
        if (count <= n && p) return;
        release();
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)));
        n = count;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// Grows buffers of an owner whose last kernels are followed by `ev` (meaningful once `used`): r(buf, count) -> buf.p, long
// enough.  A buffer that holds an allocation is replaced only after idle(), one host wait per Reserve; a first allocation,
// which nothing can be reading, needs none.
struct Reserve {
    hipEvent_t ev;
    bool used;
    bool waited = false;
    void idle() {
        if (used && !waited) HIP_CHECK(hipEventSynchronize(ev));
        waited = true;
    }
    template <class T>
    T* operator()(DevBuf<T>& b, size_t count) {
        if (count <= b.n && b.p) return b.p;
        if (b.p) idle();
        b.alloc(count);
        return b.p;
    }
};

// table_take(need, bytes) -> the 16-byte-aligned offset of the next piece of a table; `need`, its size so far, runs along.
inline size_t table_take(size_t& need, size_t bytes) {
    const size_t o = need;
    need = (need + bytes + 15) & ~(size_t)15;
    return o;
}

// A table that is written on the host and read by kernels.  begin(need, r) -> the pinned buffer to write `need` bytes into: it
// waits until the copy of the previous table has read that buffer (the one host wait of the steady state, never for a
// kernel); buffers that are too short are replaced at need * 2, after r.idle().  send(bytes, st) enqueues the one copy and
// the event behind it -> the device address.  The owner's device is current whenever a member runs.
struct StagedTable {
    uint8_t* pin = nullptr;
    size_t pin_bytes = 0;
    DevBuf<uint8_t> dev;
    hipEvent_t ev = nullptr;
    bool sent = false;                    // a copy has been enqueued (ev is meaningful)
    ~StagedTable() {
        if (pin) (void)hipHostFree(pin);
        if (ev) (void)hipEventDestroy(ev);
    }
    uint8_t* begin(size_t need, Reserve& r) {
        if (sent) HIP_CHECK(hipEventSynchronize(ev));
        if (pin_bytes < need || dev.n < need) {
            r.idle();
            if (pin_bytes < need) {
                if (pin) HIP_CHECK(hipHostFree(pin));
                pin = nullptr;
                pin_bytes = 0;
                HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&pin), need * 2, hipHostMallocDefault));
                pin_bytes = need * 2;
            }
            dev.alloc(need * 2);
        }
        if (!ev) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return pin;
    }
    const uint8_t* send(size_t bytes, hipStream_t st) {
        HIP_CHECK(hipMemcpyAsync(dev.p, pin, bytes, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(ev, st));
        sent = true;
        return dev.p;
    }
};

}  // namespace cph
