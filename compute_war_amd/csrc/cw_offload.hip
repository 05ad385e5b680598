// cw_offload.hip -- the HashOffload batch object (HashOffload.h:13-64: Reset / Enqueue / Start / Complete over one stream and two device
// buffers of its own) and the single consumer thread that drains the queue of submitted objects (hashing_offload_entry_point, :160-183).

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

#include "cw_host.h"

using namespace cw::host;

struct cw_offload {
    int hash_alg;
    int n_blocks;           // offloadCount
    size_t block_bytes;
    char *data = nullptr;   // host
    char *results = nullptr;
    void (*on_complete)(void *) = nullptr;
    void *arg = nullptr;
    std::atomic<int> state{CW_OFFLOAD_INIT};
    int error = CW_OK;      // why the object is in CW_OFFLOAD_FAILED
    char error_msg[256] = "";
    int device = -1;        // the device the object was created on
    hipStream_t stream = nullptr;
    DevBuf d_src, d_dig;
};

namespace {
int offload_fail(cw_offload *h, int rc) // record the failure on the object, so that waiters and Complete() see it
{
    h->error = rc;
    strncpy(h->error_msg, cw_last_error(), sizeof h->error_msg - 1);
    h->state.store(CW_OFFLOAD_FAILED);
    return rc;
}
} // namespace

extern "C" {

cw_offload_t *cw_offload_create(int hash_alg, int n_blocks, size_t block_bytes)
{
    if (ensure_init() != CW_OK) return nullptr;
    if (n_blocks <= 0 || cw_digest_bytes(hash_alg) == 0 || check_block(block_bytes) != CW_OK) {
        fail(CW_ERR_BAD_ARG, "cw_offload_create: bad arguments");
        return nullptr;
    }
    cw_offload *h = new cw_offload;
    h->hash_alg = hash_alg; h->n_blocks = n_blocks; h->block_bytes = block_bytes;
    h->device = current_device();
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        h->d_src.reserve((size_t)n_blocks * block_bytes + 16) != CW_OK || h->d_dig.reserve((size_t)n_blocks * cw_digest_bytes(hash_alg)) != CW_OK) {
        cw_offload_destroy(h);
        fail(CW_ERR_HIP, "cw_offload_create: device resources");
        return nullptr;
    }
    return h;
}

void cw_offload_destroy(cw_offload_t *h)
{
    if (!h) return;
    h->d_src.release(); h->d_dig.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int cw_offload_reset(cw_offload_t *h, char *data, char *results, void (*on_complete)(void *), void *arg)
{
    if (!h) return fail(CW_ERR_BAD_ARG, "NULL offload");
    h->data = data; h->results = results; h->on_complete = on_complete; h->arg = arg;
    h->error = CW_OK; h->error_msg[0] = 0;
    h->state.store(CW_OFFLOAD_INIT);
    return CW_OK;
}

int cw_offload_enqueue(cw_offload_t *h)
{
    if (!h) return fail(CW_ERR_BAD_ARG, "NULL offload");
    int want = CW_OFFLOAD_INIT;
    if (!h->state.compare_exchange_strong(want, CW_OFFLOAD_QUEUED)) return fail(CW_ERR_STATE, "Enqueue: state %d != hInit", want);
    return CW_OK;
}

int cw_offload_start(cw_offload_t *h)
{
    if (!h) return fail(CW_ERR_BAD_ARG, "NULL offload");
    if (h->state.load() != CW_OFFLOAD_QUEUED) return fail(CW_ERR_STATE, "Start: state %d != hQueued", h->state.load());
    // everything that can fail is checked or attempted BEFORE the object counts as offloaded; a failure leaves it in
    // CW_OFFLOAD_FAILED with the reason on the object (cw_offload_error), never in hOffloaded with nothing in flight
    if (!h->data || !h->results) return offload_fail(h, fail(CW_ERR_BAD_ARG, "Start: Reset() gave no data/results"));
    const size_t bytes = (size_t)h->n_blocks * h->block_bytes, db = cw_digest_bytes(h->hash_alg);
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(h->d_src.p, h->data, bytes, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return offload_fail(h, fail(CW_ERR_HIP, "Start: %s", hipGetErrorString(e)));
    int rc = dev_hash(h->hash_alg, (const uint8_t *)h->d_src.p, h->block_bytes, h->block_bytes, (size_t)h->n_blocks, (uint8_t *)h->d_dig.p, h->stream);
    if (rc != CW_OK) { (void)hipStreamSynchronize(h->stream); return offload_fail(h, rc); }
    e = hipMemcpyAsync(h->results, h->d_dig.p, (size_t)h->n_blocks * db, hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(h->stream); return offload_fail(h, fail(CW_ERR_HIP, "Start: %s", hipGetErrorString(e))); }
    h->state.store(CW_OFFLOAD_OFFLOADED);
    return CW_OK;
}

int cw_offload_complete(cw_offload_t *h)
{
    if (!h) return fail(CW_ERR_BAD_ARG, "NULL offload");
    if (h->state.load() == CW_OFFLOAD_FAILED) return fail(h->error, "Complete: the offload failed: %s", h->error_msg);
    if (h->state.load() != CW_OFFLOAD_OFFLOADED) return fail(CW_ERR_STATE, "Complete: state %d != hOffloaded", h->state.load());
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return offload_fail(h, fail(CW_ERR_HIP, "Complete: %s", hipGetErrorString(e)));
    h->state.store(CW_OFFLOAD_COMPLETE);
    if (h->on_complete) h->on_complete(h->arg);
    return CW_OK;
}

int cw_offload_completed(const cw_offload_t *h) { return h && h->state.load() == CW_OFFLOAD_COMPLETE; }
int cw_offload_state(const cw_offload_t *h) { return h ? h->state.load() : CW_ERR_BAD_ARG; }
int cw_offload_error(const cw_offload_t *h) { return h ? h->error : CW_ERR_BAD_ARG; }

int cw_offload_do(cw_offload_t *h)
{
    int rc = cw_offload_start(h);
    return rc == CW_OK ? cw_offload_complete(h) : rc;
}

// ---- the offload thread (:160-183) ---------------------------------------------------------------------------
namespace {
std::mutex q_lock;               // hashLock
std::condition_variable q_cv;    // hashCV
std::deque<cw_offload *> q_work; // hashQueue
bool q_finished = false;         // allWorkFinished
std::thread q_thread;
bool q_running = false;

void offload_entry_point()
{
    std::unique_lock<std::mutex> lk(q_lock);
    for (;;) {
        if (q_work.empty()) {
            if (q_finished) break; // drain before exiting
            q_cv.wait(lk);
            continue;
        }
        cw_offload *h = q_work.front();
        q_work.pop_front();
        lk.unlock();
        if (cw_offload_do(h) != CW_OK) {
            // the reason is on the object (CW_OFFLOAD_FAILED, cw_offload_error); whoever waits for the callback is
            // still woken, and finds Completed() false
            fprintf(stderr, "libcwhc: offload failed: %s\n", cw_last_error());
            if (h->state.load() != CW_OFFLOAD_FAILED) offload_fail(h, CW_ERR_STATE);
            if (h->on_complete) h->on_complete(h->arg);
        }
        lk.lock();
    }
}
} // namespace

int cw_offload_thread_start(void)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    std::lock_guard<std::mutex> g(q_lock);
    if (q_running) return CW_OK;
    q_finished = false;
    q_thread = std::thread(offload_entry_point);
    q_running = true;
    return CW_OK;
}

int cw_offload_submit(cw_offload_t *h)
{
    int rc = cw_offload_enqueue(h);
    if (rc != CW_OK) return rc;
    {
        std::lock_guard<std::mutex> g(q_lock);
        if (!q_running) return fail(CW_ERR_STATE, "offload thread not started");
        q_work.push_back(h);
    }
    q_cv.notify_one();
    return CW_OK;
}

void cw_offload_thread_stop(void)
{
    {
        std::lock_guard<std::mutex> g(q_lock);
        if (!q_running) return;
        q_finished = true;
    }
    q_cv.notify_all();
    q_thread.join();
    std::lock_guard<std::mutex> g(q_lock);
    q_running = false;
}

} // extern "C"
