// Who frees device memory and events (no HIP here: render.hip supplies the backend, and
// tests/test_device_buf.py a counting fake).  Two move-only owners and the one rule for buffers that
// share a capacity.  Nothing here pools, caches or reuses: who frees, never when or how much.
//
// Backend B, static functions returning 0 or the backend's error code:
//   int malloc(void**, size_t), int free(void*), int get_device(int*), int set_device(int),
//   using event_t (a handle, null when empty), int event_create(event_t*), int event_destroy(event_t)
#pragma once
#include <cstddef>
#include <initializer_list>
#include <utility>

namespace nd {

// Makes `device` current for a scope and restores the caller's current device after it, if it differed.
template <class B>
struct OnDevice {
    int prev = 0;
    bool switched = false;
    explicit OnDevice(int device) { switched = B::get_device(&prev) == 0 && prev != device && B::set_device(device) == 0; }
    OnDevice(const OnDevice&) = delete;
    ~OnDevice() { if (switched) B::set_device(prev); }
};

// One device allocation that only grows.  A buffer here can reach 119 GB, so the old block and the new
// one are never live together: growing forgets the capacity, frees, then allocates, and a failed
// allocation leaves the buffer empty (null, 0 bytes) -- never a stale capacity over a null pointer --
// so that the next reserve allocates again.
template <class B>
class DevBuf {
    void* ptr_ = nullptr;
    size_t bytes_ = 0;
    int device_ = 0;

  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_), device_(o.device_) { o.ptr_ = nullptr, o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr_ = std::exchange(o.ptr_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
            device_ = o.device_;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    // At least `bytes` on `device`; no backend call where the buffer already holds them.  Returns the
    // backend's error.
    int reserve(int device, size_t bytes) {
        if (bytes <= bytes_) return 0;
        release();
        OnDevice<B> on(device);
        const int err = B::malloc(&ptr_, bytes);
        if (err) ptr_ = nullptr;
        else bytes_ = bytes, device_ = device;
        return err;
    }
    // Frees with the buffer's device current; the buffer is empty afterwards.
    void release() {
        if (!ptr_) return;
        bytes_ = 0;
        OnDevice<B> on(device_);
        B::free(std::exchange(ptr_, nullptr));
    }
    template <typename T>
    T* as() const { return static_cast<T*>(ptr_); }
    size_t bytes() const { return bytes_; }
    int device() const { return device_; }
    explicit operator bool() const { return ptr_ != nullptr; }
};

// Buffers whose sizes follow one count (slots, samples, buckets, queue entries) share that count as
// their capacity.  A group that grows frees all of its buffers before it allocates any of them, and the
// capacity stays 0 until all of them are allocated.  one(buf, bytes, what) reserves one buffer and
// returns 0 or the caller's error, which ends the call.
template <class B>
struct GroupItem {
    DevBuf<B>* buf;
    size_t bytes;
    const char* what;
};
template <class B, class ReserveOne>
int reserve_group(size_t& cap, size_t count, std::initializer_list<GroupItem<B>> items, ReserveOne&& one) {
    if (count <= cap) return 0;
    cap = 0;
    for (const GroupItem<B>& it : items) it.buf->release();
    for (const GroupItem<B>& it : items)
        if (const int rc = one(*it.buf, it.bytes, it.what)) return rc;
    cap = count;
    return 0;
}

// An event, created on first use on the device current then and destroyed with that device current.
template <class B>
class DevEvent {
    typename B::event_t ev_{};
    int device_ = 0;

  public:
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() {
        if (!ev_) return;
        OnDevice<B> on(device_);
        B::event_destroy(ev_);
    }
    // The event into *out, created if this is its first use.  Returns the backend's error.
    int get(typename B::event_t* out) {
        if (!ev_) {
            if (const int err = B::get_device(&device_)) return err;
            if (const int err = B::event_create(&ev_)) {
                ev_ = typename B::event_t{};
                return err;
            }
        }
        *out = ev_;
        return 0;
    }
    // The event as last used (null before its first use).
    typename B::event_t handle() const { return ev_; }
};

}  // namespace nd
