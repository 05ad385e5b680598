// stream_scratch.h -- the one mechanism behind every launch sequence's per-(device, stream) scratch: a grow-only device
// buffer, a side stream with its fork / join events, and the registry that keeps one entry of them (plus a launch mutex) per
// stream.  Host code only: nothing here is seen by a kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <utility>

namespace cw {

// Key of the per-(device, stream) scratch the launch sequences keep (the NULL stream exists once per device).  Every
// entry also holds a launch mutex: a sequence of launches that shares scratch -- memset counters, scan, parse, redo; the
// chained slices of one hash -- is queued under it, so that two host threads using the same stream cannot interleave
// their sequences (stream order then keeps each sequence atomic).
static inline uint64_t ws_key(hipStream_t s)
{
    int d = 0;
    (void)hipGetDevice(&d);
    return ((uint64_t)reinterpret_cast<uintptr_t>(s) << 4) | (uint64_t)(d & 15);
}

// Owning device buffer that only grows.  No destructor: whoever owns it calls release() (a registry entry through
// StreamScratch, which never runs at process exit, when the HIP runtime may be gone already).
class DeviceBuf {
    void *p_ = nullptr;
    size_t bytes_ = 0;

public:
    // no-op when large enough (first or a larger call only); else frees and allocates max(bytes, floor_bytes).  On failure
    // the buffer is empty and the HIP error is returned as it came: whether that fails the call is the caller's decision.
    hipError_t reserve(size_t bytes, size_t floor_bytes = 0)
    {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess) return e;
        const size_t want = bytes < floor_bytes ? floor_bytes : bytes;
        if ((e = hipMalloc(&p_, want)) != hipSuccess) { p_ = nullptr; return e; }
        bytes_ = want;
        return hipSuccess;
    }
    hipError_t release()
    {
        const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        p_ = nullptr; bytes_ = 0;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }
};

// A stream beside the caller's, with the two events that order it: created on first use, destroyed by release().
struct SideStream {
    enum Priority { normal, greatest, least };
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool borrowed = false; // the stream is `lender`'s; the events are always this object's own

    // no-op once open; non-blocking stream of the given priority, or `lender`'s stream if that is given
    hipError_t open(Priority prio, hipStream_t lender = nullptr)
    {
        hipError_t e = hipSuccess;
        if (!stream && lender) { stream = lender; borrowed = true; }
        if (!stream && prio == normal) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (!stream && prio != normal) {
            int least_p = 0, greatest_p = 0;
            if ((e = hipDeviceGetStreamPriorityRange(&least_p, &greatest_p)) == hipSuccess)
                e = hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio == greatest ? greatest_p : least_p);
        }
        if (e == hipSuccess && !fork) e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
        if (e == hipSuccess && !join) e = hipEventCreateWithFlags(&join, hipEventDisableTiming);
        return e;
    }
    void release()
    {
        if (stream && !borrowed) (void)hipStreamDestroy(stream);
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        stream = nullptr; fork = join = nullptr; borrowed = false;
    }

    // One fork of the caller's stream onto the side stream.  The constructor records `fork` on the caller's stream and makes
    // the side stream wait for it (`err`: what that returned; nothing is forked then).  join() records `join` on the side
    // stream and makes the caller's stream wait.  A function that leaves early, with an error, without having joined is
    // joined by the destructor: work already queued on the side stream reads the caller's buffers, and the caller's stream
    // has to stay ordered behind it.  (What that join returns is dropped: the function is returning an error already.)
    class Fork {
        SideStream &s_;
        hipStream_t caller_;
        bool pending_;

    public:
        hipError_t err;
        Fork(SideStream &s, hipStream_t caller) : s_(s), caller_(caller)
        {
            err = hipEventRecord(s.fork, caller);
            if (err == hipSuccess) err = hipStreamWaitEvent(s.stream, s.fork, 0);
            pending_ = err == hipSuccess;
        }
        Fork(const Fork &) = delete;
        Fork &operator=(const Fork &) = delete;
        hipError_t join()
        {
            pending_ = false;
            const hipError_t e = hipEventRecord(s_.join, s_.stream);
            return e == hipSuccess ? hipStreamWaitEvent(caller_, s_.join, 0) : e;
        }
        ~Fork() { if (pending_) (void)join(); }
    };
};

// Every StreamScratch of the process, whatever its entries hold: what release_stream_workspaces / release_all_workspaces walk.
class ScratchRegistry {
public:
    static ScratchRegistry *&head() { static ScratchRegistry *h = nullptr; return h; } // (no order among translation units needed)
    ScratchRegistry *const next;
    virtual void release(hipStream_t stream) = 0;
    virtual void release_all() = 0;

protected:
    ScratchRegistry() : next(head()) { head() = this; } // registries are namespace-scope objects: built one at a time, at load
    ~ScratchRegistry() = default;
};

using LaunchLock = std::lock_guard<std::mutex>;

// The dynamic-LDS limits of a launch function's kernels (`done`: that function's own flag): each set is made once per process; a
// failure is the call's, and the next call tries again.  Once a set is made, a call only reads the flag.
inline hipError_t set_lds_limits_once(std::atomic<bool> &done, std::initializer_list<std::pair<const void *, uint32_t>> limits)
{
    if (done.load(std::memory_order_acquire)) return hipSuccess;
    static std::mutex lock;
    std::lock_guard<std::mutex> g(lock);
    for (auto it = limits.begin(); !done.load(std::memory_order_relaxed) && it != limits.end(); ++it) {
        const hipError_t e = hipFuncSetAttribute(it->first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)it->second);
        if (e != hipSuccess) return e;
    }
    done.store(true, std::memory_order_release);
    return hipSuccess;
}

// One T per (device, stream), each with the launch mutex of ws_key()'s comment.  There is one mutex per (registry, stream)
// and not one per stream, because launch functions nest on a stream: chunk_hash_launch calls the hash's launch function
// under its entry's mutex, lz4_launch the fused call's hook.  T has a `release()` that gives back everything it owns.
template <class T> class StreamScratch final : public ScratchRegistry {
public:
    struct Entry : T { std::mutex launch; };
    // find or insert; the reference stays valid while other threads insert (std::unordered_map never moves its nodes)
    Entry &at(hipStream_t stream)
    {
        std::lock_guard<std::mutex> g(lock_);
        return map_[ws_key(stream)];
    }
    Entry *find(hipStream_t stream)
    {
        std::lock_guard<std::mutex> g(lock_);
        auto it = map_.find(ws_key(stream));
        return it == map_.end() ? nullptr : &it->second;
    }
    // The entry goes together with its mutex: only to be called when no launch on that stream is in flight on another
    // thread, that is, by the stream's owner on its way to destroying the stream.
    void release(hipStream_t stream) override
    {
        std::lock_guard<std::mutex> g(lock_);
        auto it = map_.find(ws_key(stream));
        if (it == map_.end()) return;
        (void)it->second.release();
        map_.erase(it);
    }
    void release_all() override
    {
        std::lock_guard<std::mutex> g(lock_);
        for (auto &kv : map_) (void)kv.second.release();
        map_.clear();
    }

private:
    std::mutex lock_;
    std::unordered_map<uint64_t, Entry> map_;
};

} // namespace cw
