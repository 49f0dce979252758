// mcd_cache.hip -- the stream writer of include/mcd_cache.h (host code only; no kernel): blocks of activation rows leave the
// device while the encoder runs and are appended to their cache files by a worker thread, so that the end of a dissection
// only finalises the files.
//   launch thread (push):  event on the launch stream -> the copy stream waits for it -> D2H copy into a pinned slot ->
//                          done-event of the slot (and of the file, for reserve) -> job posted
//   worker thread:         waits for the slot's done-event (blocking-sync event: it sleeps, it does not spin), appends the
//                          rows through mcd_cache_io_t, gives the slot back
// The worker runs no Python and takes no lock the launch thread holds while it queues GPU work, except the ring's mutex for the
// moment of a slot hand-over.  The ring of pinned slots is allocated once per process (pinning memory costs milliseconds per
// slot) and is lent to one writer at a time.
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mcd_common.h"
#include "../../include/mcd_cache.h"

namespace {

struct Slot {
    void* host = nullptr;
    hipEvent_t done = nullptr;
};

// the process-wide ring: kept between writers, rebuilt only when one asks for more or larger slots
struct Ring {
    std::mutex mu;
    std::vector<Slot> slots;
    size_t slot_bytes = 0;
    int device = -1;
    bool lent = false;
};
Ring g_ring;

struct Job {
    int slot, file;
    int64_t row0, n;
};

struct Writer {
    int device = 0;
    hipStream_t copy = nullptr;
    hipEvent_t ready = nullptr;               // recorded on the launch stream by every push
    std::vector<void*> files;
    std::vector<int64_t> widths;
    std::vector<hipEvent_t> file_done;        // the device block of the file's last push has been read
    std::vector<char> file_pushed;
    mcd_cache_io_t io{};
    int n_slots = 0;
    size_t slot_bytes = 0;

    std::mutex mu;
    std::condition_variable cv_job, cv_free;
    std::deque<Job> jobs;
    std::vector<int> free_slots;
    bool stop = false;
    int err = MCD_OK;                         // the first error, with its text
    std::string err_text;
    std::thread worker;

    void fail(int code, const std::string& text) {   // mu held
        if (err == MCD_OK) {
            err = code;
            err_text = text;
        }
    }
};

void ring_release_storage(Ring& r) {   // r.mu held
    for (Slot& s : r.slots) {
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.host) (void)hipHostFree(s.host);
    }
    r.slots.clear();
    r.slot_bytes = 0;
}

// lends the ring to a writer: at least n_slots slots of at least slot_bytes on `device`
int ring_borrow(int device, int n_slots, size_t slot_bytes) {
    std::lock_guard<std::mutex> g(g_ring.mu);
    MCD_REQUIRE(!g_ring.lent, MCD_E_UNSUPPORTED, "mcd_cache_stream_open: another stream writer of this process is still open");
    if (g_ring.device != device || g_ring.slot_bytes < slot_bytes || (int)g_ring.slots.size() < n_slots) {
        ring_release_storage(g_ring);
        g_ring.device = device;
        for (int i = 0; i < n_slots; ++i) {
            Slot s;
            hipError_t e = hipHostMalloc(&s.host, slot_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventBlockingSync);
            if (e != hipSuccess) {
                if (s.host) (void)hipHostFree(s.host);
                ring_release_storage(g_ring);
                return mcd_fail(MCD_E_LAUNCH, "mcd_cache_stream_open: pinned slot %d of %zu bytes: %s", i, slot_bytes, hipGetErrorString(e));
            }
            g_ring.slots.push_back(s);
        }
        g_ring.slot_bytes = slot_bytes;
    }
    g_ring.lent = true;
    return MCD_OK;
}

void ring_return() {
    std::lock_guard<std::mutex> g(g_ring.mu);
    g_ring.lent = false;
}

void worker_main(Writer* w) {
    (void)hipSetDevice(w->device);
    for (;;) {
        Job j;
        {
            std::unique_lock<std::mutex> lk(w->mu);
            w->cv_job.wait(lk, [&] { return w->stop || !w->jobs.empty(); });
            if (w->jobs.empty()) return;           // stop, and everything posted has been written
            j = w->jobs.front();
            w->jobs.pop_front();
        }
        const Slot& s = g_ring.slots[(size_t)j.slot];   // the vector does not change while the ring is lent
        const hipError_t e = hipEventSynchronize(s.done);
        bool ok;
        {
            std::lock_guard<std::mutex> g(w->mu);
            if (e != hipSuccess) w->fail(MCD_E_LAUNCH, std::string("mcd_cache_stream: device -> host copy: ") + hipGetErrorString(e));
            ok = w->err == MCD_OK;                 // after the first error the rest of the queue is only drained
        }
        if (ok && w->io.append(w->files[(size_t)j.file], (const float*)s.host, j.row0, j.n) != 0) {
            const char* t = w->io.last_error ? w->io.last_error() : nullptr;
            std::lock_guard<std::mutex> g(w->mu);
            w->fail(MCD_E_UNSUPPORTED, std::string("mcd_cache_stream: append: ") + (t ? t : "failed"));
        }
        {
            std::lock_guard<std::mutex> g(w->mu);
            w->free_slots.push_back(j.slot);
        }
        w->cv_free.notify_one();
    }
}

void writer_destroy(Writer* w) {   // the worker has ended (or never started)
    for (hipEvent_t e : w->file_done)
        if (e) (void)hipEventDestroy(e);
    if (w->ready) (void)hipEventDestroy(w->ready);
    if (w->copy) (void)hipStreamDestroy(w->copy);
    delete w;
}

int writer_end(void* handle, bool commit, const char* who) {
    Writer* w = (Writer*)handle;
    MCD_REQUIRE(w, MCD_E_ARG, "%s: NULL handle", who);
    {
        std::lock_guard<std::mutex> g(w->mu);
        w->stop = true;
    }
    w->cv_job.notify_one();
    if (w->worker.joinable()) w->worker.join();      // drains the queue first: every job's copy has completed when it returns
    ring_return();
    for (void* f : w->files) {
        if (commit && w->err == MCD_OK) {
            if (w->io.close(f) != 0) {
                const char* t = w->io.last_error ? w->io.last_error() : nullptr;
                w->fail(MCD_E_UNSUPPORTED, std::string("mcd_cache_stream_close: ") + (t ? t : "finalisation failed"));
            }
        } else {
            w->io.abort(f);
        }
    }
    const int err = w->err;
    const std::string text = w->err_text;
    writer_destroy(w);
    return err == MCD_OK ? MCD_OK : mcd_fail(err, "%s", text.c_str());
}

}  // namespace

extern "C" int mcd_cache_stream_open(int n_files, void* const* files, const int64_t* widths, const mcd_cache_io_t* io, int n_slots,
                                     size_t slot_bytes, void** handle) {
    MCD_REQUIRE(handle, MCD_E_ARG, "mcd_cache_stream_open: NULL handle pointer");
    *handle = nullptr;
    const bool io_ok = io && io->append && io->close && io->abort;
    bool args_ok = io_ok && n_files >= 1 && files && widths && n_slots >= 1 && n_slots <= 1024 && slot_bytes >= 4;
    for (int i = 0; args_ok && i < n_files; ++i) args_ok = files[i] != nullptr && widths[i] > 0;
    if (!args_ok) {
        if (io_ok && files)      // the files are the writer's from the call on: an error removes them
            for (int i = 0; i < n_files; ++i)
                if (files[i]) io->abort(files[i]);
        return mcd_fail(MCD_E_ARG, "mcd_cache_stream_open: bad argument");
    }
    Writer* w = new Writer;
    w->files.assign(files, files + n_files);
    w->widths.assign(widths, widths + n_files);
    w->io = *io;
    w->file_done.assign((size_t)n_files, nullptr);
    w->file_pushed.assign((size_t)n_files, 0);
    w->n_slots = n_slots;
    w->slot_bytes = slot_bytes;
    hipError_t e = hipGetDevice(&w->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&w->copy, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ready, hipEventDisableTiming);
    for (int i = 0; e == hipSuccess && i < n_files; ++i) e = hipEventCreateWithFlags(&w->file_done[(size_t)i], hipEventDisableTiming);
    int rc = e == hipSuccess ? MCD_OK : mcd_fail(MCD_E_LAUNCH, "mcd_cache_stream_open: %s", hipGetErrorString(e));
    if (rc == MCD_OK) rc = ring_borrow(w->device, n_slots, slot_bytes);
    if (rc != MCD_OK) {
        for (void* f : w->files) w->io.abort(f);
        writer_destroy(w);
        return rc;
    }
    for (int i = 0; i < n_slots; ++i) w->free_slots.push_back(i);
    w->worker = std::thread(worker_main, w);
    *handle = w;
    return MCD_OK;
}

extern "C" int mcd_cache_stream_reserve(void* handle, int file, mcd_stream_t stream) {
    Writer* w = (Writer*)handle;
    MCD_REQUIRE(w && file >= 0 && file < (int)w->files.size(), MCD_E_ARG, "mcd_cache_stream_reserve: bad handle or file %d", file);
    if (!w->file_pushed[(size_t)file]) return MCD_OK;
    const hipError_t e = hipStreamWaitEvent((hipStream_t)stream, w->file_done[(size_t)file], 0);
    MCD_REQUIRE(e == hipSuccess, MCD_E_LAUNCH, "mcd_cache_stream_reserve: %s", hipGetErrorString(e));
    return MCD_OK;
}

extern "C" int mcd_cache_stream_push(void* handle, int file, const float* device_block, int64_t row0, int64_t n,
                                     mcd_stream_t stream) {
    Writer* w = (Writer*)handle;
    MCD_REQUIRE(w && file >= 0 && file < (int)w->files.size(), MCD_E_ARG, "mcd_cache_stream_push: bad handle or file %d", file);
    MCD_REQUIRE(row0 >= 0 && n >= 0, MCD_E_ARG, "mcd_cache_stream_push: bad rows");
    if (n == 0) return MCD_OK;
    MCD_REQUIRE(device_block, MCD_E_ARG, "mcd_cache_stream_push: NULL block");
    const int64_t width = w->widths[(size_t)file];
    MCD_REQUIRE((uint64_t)n <= w->slot_bytes / 4 / (uint64_t)width, MCD_E_ARG,
                "mcd_cache_stream_push: %lld rows of %lld floats do not fit a slot of %zu bytes", (long long)n, (long long)width, w->slot_bytes);
    const size_t bytes = (size_t)n * (size_t)width * 4;
    int slot;
    {
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv_free.wait(lk, [&] { return !w->free_slots.empty(); });   // back-pressure: the worker gives every slot back
        slot = w->free_slots.back();
        w->free_slots.pop_back();
    }
    const Slot& s = g_ring.slots[(size_t)slot];
    hipError_t e = hipEventRecord(w->ready, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(w->copy, w->ready, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(s.host, device_block, bytes, hipMemcpyDeviceToHost, w->copy);
    if (e == hipSuccess) e = hipEventRecord(s.done, w->copy);
    if (e == hipSuccess) e = hipEventRecord(w->file_done[(size_t)file], w->copy);
    if (e != hipSuccess) {
        // whatever part was queued may still write the slot: it goes back only once the copy stream is idle
        (void)hipStreamSynchronize(w->copy);
        std::lock_guard<std::mutex> g(w->mu);
        w->free_slots.push_back(slot);
        w->fail(MCD_E_LAUNCH, std::string("mcd_cache_stream_push: ") + hipGetErrorString(e));
        return mcd_fail(MCD_E_LAUNCH, "mcd_cache_stream_push: %s", hipGetErrorString(e));
    }
    w->file_pushed[(size_t)file] = 1;
    {
        std::lock_guard<std::mutex> g(w->mu);
        w->jobs.push_back(Job{slot, file, row0, n});
    }
    w->cv_job.notify_one();
    return MCD_OK;
}

extern "C" int mcd_cache_stream_close(void* handle) { return writer_end(handle, true, "mcd_cache_stream_close"); }

extern "C" int mcd_cache_stream_abort(void* handle) { return writer_end(handle, false, "mcd_cache_stream_abort"); }
