/*
 * tests/native/fake_device.cpp -- TEST INFRASTRUCTURE: a CPU fake of the HIP device, for linking hvqm4_amd/csrc/hvq_runtime.cpp
 * unchanged into a host program (tests/native/fake_driver.cpp, tests/test_fake_device.py).  It implements exactly the HIP calls the
 * runtime uses (fakehip/hip/hip_runtime.h).
 *
 * MEMORY.  Every device or pinned allocation is a malloc of its own (a sanitizer build guards each one) and is entered in a registry
 * with its kind and size; fake_span() aborts unless a range lies inside one live allocation.  Fresh memory is filled with 0xCD: HIP
 * promises nothing about the content of hipMalloc / hipHostMalloc memory, and a reader of bytes nobody wrote then shows.
 *
 * SCHEDULER.  A stream is a FIFO of operations: copy, memset, kernel, event record, event wait.  FAKEHIP_SCHEDULE chooses when they run:
 *   eager   every operation runs inside the call that queues it: a GPU that is always ahead of the host.
 *   late    nothing runs inside the call; an operation runs only when the host observes it or an observed operation depends on it: a
 *           GPU that is always as far behind as HIP allows.  A dependency that holds only because the GPU is usually fast fails here.
 * The rules of `late`, each with the HIP rule it rests on:
 *   - hipStreamSynchronize(s) drains s.  [Blocks until all work queued on s has completed.]
 *   - hipEventSynchronize(e) drains the stream e was last recorded on, up to that record.  [Waits for the work captured by the most
 *     recent hipEventRecord; an event never recorded is complete.]
 *   - hipEventQuery(e) answers hipErrorNotReady ONCE per record, then behaves as hipEventSynchronize.  [Query may say "not ready" for
 *     any work that has not finished; a polling loop must get there eventually.]
 *   - a queued hipStreamWaitEvent first drains the recording stream up to the record the event held WHEN THE WAIT WAS QUEUED; a wait on
 *     an event never recorded is a no-op.  [hipStreamWaitEvent captures the event's state at the call; later records do not move it.]
 *   - operations of one stream run in queue order.  [Stream order.]  Different streams have no order but the events'.  All the runtime's
 *     streams are hipStreamNonBlocking, so the null stream orders nothing against them either.
 *   - hipFree and hipHostFree drain everything, then free.  [hipFree synchronises the device; hipHostFree is given the same: the driver
 *     unpins under a device-wide wait.]
 *   - a blocking hipMemcpy runs at once and drains nothing.  [It is ordered with the null stream only, see above.]
 *   - hipMemcpyAsync from PINNED host memory, and hvq_launch_upload's kernel, read the source when they RUN.  [The DMA engine / the
 *     kernel reads pinned memory in place; the host must keep it unchanged until the operation has completed.]
 *   - hipMemcpyAsync from PAGEABLE host memory snapshots the source at the call.  [The runtime stages pageable sources before it
 *     returns; the source is the caller's again on return.]
 *   - hipMemcpyAsync to PAGEABLE host memory drains its stream through the copy before it returns.  [Pageable device-to-host copies are
 *     synchronous with respect to the host.]
 *   - hipStreamDestroy returns at once; what the stream holds still runs (at the next full drain).  [Destroy releases the stream once
 *     its work has completed, without waiting.]
 *   - process exit drains everything.
 * A test that fails only because this file is stricter than HIP is a bug in this file.
 *
 * One mutex guards all of it: hvq_submit_many_device_async calls HIP from a worker thread.
 */
#include "fake_device.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

struct fakehipStream;

struct fakehipEvent {
    uint64_t recorded = 0;             /* ticket of the newest hipEventRecord (0: never recorded) */
    uint64_t completed = 0;            /* newest ticket whose record has run */
    uint64_t queried = 0;              /* ticket hipEventQuery has answered "not ready" for */
    fakehipStream *stream = nullptr;   /* stream of the newest record */
    bool destroyed = false;
};

struct Op {
    const char *name;
    std::function<void()> body;        /* copy, memset, kernel */
    fakehipEvent *ev = nullptr;        /* record / wait */
    uint64_t ticket = 0;
    fakehipStream *wait_on = nullptr;  /* wait: the stream the awaited record was queued on */
    bool is_wait = false;
};

struct fakehipStream {
    std::deque<Op> q;
    bool draining = false, destroyed = false;
};

namespace {

struct Alloc { size_t size; FakeKind kind; };

struct State {
    std::recursive_mutex mu;
    bool late = false;
    std::map<uintptr_t, Alloc> allocs;
    std::vector<std::unique_ptr<fakehipStream>> streams;
    std::vector<std::unique_ptr<fakehipEvent>> events;
    uint64_t next_ticket = 1;
    fakehipStream null_stream;
    uint64_t ops_queued = 0, ops_deferred = 0;
    State()
    {
        const char *e = getenv("FAKEHIP_SCHEDULE");
        if (e && !strcmp(e, "late")) late = true;
        else if (e && strcmp(e, "eager")) { fprintf(stderr, "fakehip: FAKEHIP_SCHEDULE must be eager or late\n"); abort(); }
    }
    ~State();
};

State &S() { static State s; return s; }
typedef std::lock_guard<std::recursive_mutex> Lock;

void run_op(Op &op);

/* run the operations of s from the front, up to and including the record of `ticket` on `ev` (ev == nullptr: all of them) */
void drain(fakehipStream *s, fakehipEvent *ev, uint64_t ticket)
{
    if (ev && ev->completed >= ticket) return;
    if (s->draining) fake_die("fakehip: stream %p waits for itself (an event wait on work queued behind it): a deadlock on a GPU", (void *)s);
    s->draining = true;
    while (!s->q.empty()) {
        Op op = std::move(s->q.front());
        s->q.pop_front();
        run_op(op);
        if (ev && ev->completed >= ticket) break;
    }
    s->draining = false;
    if (ev && ev->completed < ticket) fake_die("fakehip: record %llu of event %p is not on the stream it was queued on", (unsigned long long)ticket, (void *)ev);
}

void run_op(Op &op)
{
    if (op.is_wait) { drain(op.wait_on, op.ev, op.ticket); return; }
    if (op.ev) { if (op.ev->completed < op.ticket) op.ev->completed = op.ticket; return; }
    op.body();
}

void drain_all()
{
    State &st = S();
    /* a stream's drain may run other streams' operations (event waits); repeat until nothing is left anywhere */
    for (bool any = true; any;) {
        any = false;
        if (!st.null_stream.q.empty()) { any = true; drain(&st.null_stream, nullptr, 0); }
        for (size_t i = 0; i < st.streams.size(); ++i)
            if (!st.streams[i]->q.empty()) { any = true; drain(st.streams[i].get(), nullptr, 0); }
    }
}

State::~State()
{
    Lock lk(mu);
    drain_all();                                   /* process exit drains everything */
    for (auto &kv : allocs) free((void *)kv.first);
    allocs.clear();
}

fakehipStream *stream_of(hipStream_t s) { return s ? s : &S().null_stream; }

hipError_t enqueue(hipStream_t hs, Op op)
{
    State &st = S();
    fakehipStream *s = stream_of(hs);
    if (s->destroyed) fake_die("fakehip: %s queued on a destroyed stream", op.name);
    ++st.ops_queued;
    if (!st.late && !s->draining) {
        /* eager: the queue is empty, the operation runs here */
        run_op(op);
        return hipSuccess;
    }
    ++st.ops_deferred;
    s->q.push_back(std::move(op));
    return hipSuccess;
}

const Alloc *find(const void *ptr, uintptr_t *base)
{
    State &st = S();
    const uintptr_t a = (uintptr_t)ptr;
    auto it = st.allocs.upper_bound(a);
    if (it == st.allocs.begin()) return nullptr;
    --it;
    if (a >= it->first + it->second.size && !(it->second.size == 0 && a == it->first)) return nullptr;
    if (base) *base = it->first;
    return &it->second;
}

hipError_t alloc(void **p, size_t bytes, FakeKind kind)
{
    if (!p) return hipErrorInvalidValue;
    void *m = malloc(bytes ? bytes : 1);
    if (!m) return hipErrorOutOfMemory;
    memset(m, 0xCD, bytes ? bytes : 1);
    Lock lk(S().mu);
    S().allocs[(uintptr_t)m] = Alloc{ bytes, kind };
    *p = m;
    return hipSuccess;
}

hipError_t release(void *p, FakeKind kind, const char *what)
{
    if (!p) return hipSuccess;
    State &st = S();
    Lock lk(st.mu);
    drain_all();
    auto it = st.allocs.find((uintptr_t)p);
    if (it == st.allocs.end() || it->second.kind != kind) fake_die("fakehip: %s(%p): not the start of a live %s allocation", what, p, kind == FAKE_DEVICE ? "device" : "pinned");
    st.allocs.erase(it);
    free(p);
    return hipSuccess;
}

}  // namespace

void fake_die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    fflush(stderr);
    abort();
}

const void *fake_span(const void *ptr, size_t len, const char *what)
{
    Lock lk(S().mu);
    uintptr_t base = 0;
    const Alloc *a = find(ptr, &base);
    if (!a) fake_die("fake_span: %s: %p (+%zu) lies in no live device or pinned allocation", what, ptr, len);
    const uintptr_t off = (uintptr_t)ptr - base;
    if (len > a->size - off)
        fake_die("fake_span: %s: [%p, +%zu) leaves its %s allocation [%p, +%zu) by %zu bytes", what, ptr, len, a->kind == FAKE_DEVICE ? "device" : "pinned",
                 (void *)base, a->size, len - (a->size - off));
    return ptr;
}

FakeKind fake_kind(const void *ptr)
{
    Lock lk(S().mu);
    const Alloc *a = find(ptr, nullptr);
    return a ? a->kind : FAKE_NONE;
}

hipError_t fake_enqueue(hipStream_t s, const char *name, std::function<void()> body)
{
    Lock lk(S().mu);
    Op op{};
    op.name = name; op.body = std::move(body);
    return enqueue(s, std::move(op));
}

void fake_drain_all(void) { Lock lk(S().mu); drain_all(); }
bool fake_schedule_late(void) { return S().late; }

extern "C" {

const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNotReady: return "device not ready";
    }
    return "unknown error";
}

hipError_t hipGetDeviceCount(int *n) { if (!n) return hipErrorInvalidValue; *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { if (least) *least = 0; if (greatest) *greatest = -1; return hipSuccess; }

hipError_t hipMalloc(void **p, size_t bytes) { return alloc(p, bytes, FAKE_DEVICE); }
hipError_t hipFree(void *p) { return release(p, FAKE_DEVICE, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return alloc(p, bytes, FAKE_PINNED); }
hipError_t hipHostFree(void *p) { return release(p, FAKE_PINNED, "hipHostFree"); }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
    if (!s) return hipErrorInvalidValue;
    /* the rules above (no order against the null stream) hold for non-blocking streams only */
    if (!(flags & hipStreamNonBlocking)) fake_die("fakehip: a blocking stream: the fake models hipStreamNonBlocking streams only");
    Lock lk(S().mu);
    S().streams.emplace_back(new fakehipStream());
    *s = S().streams.back().get();
    return hipSuccess;
}

hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int) { return hipStreamCreateWithFlags(s, flags); }

hipError_t hipStreamDestroy(hipStream_t s)
{
    if (!s) return hipErrorInvalidValue;
    Lock lk(S().mu);
    /* what it holds still runs (drain_all); nothing new may be queued */
    s->destroyed = true;
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s)
{
    Lock lk(S().mu);
    drain(stream_of(s), nullptr, 0);
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    if (e->destroyed) fake_die("fakehip: hipStreamWaitEvent on a destroyed event");
    if (!e->recorded || e->completed >= e->recorded) return hipSuccess;      /* never recorded, or complete already: no-op */
    Op op{};
    op.name = "wait"; op.is_wait = true; op.ev = e; op.ticket = e->recorded; op.wait_on = e->stream;
    return enqueue(s, std::move(op));
}

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    S().events.emplace_back(new fakehipEvent());
    *e = S().events.back().get();
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }

hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    /* queued records and waits keep working (HIP releases the event once they have completed); the host may not use it again */
    e->destroyed = true;
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    if (e->destroyed) fake_die("fakehip: hipEventRecord on a destroyed event");
    Op op{};
    op.name = "record"; op.ev = e; op.ticket = S().next_ticket++;
    e->recorded = op.ticket; e->stream = stream_of(s);
    return enqueue(s, std::move(op));
}

hipError_t hipEventSynchronize(hipEvent_t e)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    if (e->destroyed) fake_die("fakehip: hipEventSynchronize on a destroyed event");
    if (e->recorded) drain(e->stream, e, e->recorded);
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t e)
{
    if (!e) return hipErrorInvalidValue;
    Lock lk(S().mu);
    if (e->destroyed) fake_die("fakehip: hipEventQuery on a destroyed event");
    if (!e->recorded || e->completed >= e->recorded) return hipSuccess;
    if (e->queried != e->recorded) { e->queried = e->recorded; return hipErrorNotReady; }
    drain(e->stream, e, e->recorded);
    return hipSuccess;
}

hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    if (!ms || !a || !b) return hipErrorInvalidValue;
    Lock lk(S().mu);
    /* HIP: hipErrorNotReady while either record has not completed */
    if (!a->recorded || !b->recorded || a->completed < a->recorded || b->completed < b->recorded) return hipErrorNotReady;
    *ms = 0.f;
    return hipSuccess;
}

static void check_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const char *what)
{
    if (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice) {
        fake_span(dst, bytes, what);
        if (fake_kind(dst) != FAKE_DEVICE) fake_die("fakehip: %s: destination %p is not device memory", what, dst);
    }
    if (kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice) {
        fake_span(src, bytes, what);
        if (fake_kind(src) != FAKE_DEVICE) fake_die("fakehip: %s: source %p is not device memory", what, src);
    }
    if (kind == hipMemcpyHostToDevice && fake_kind(src) != FAKE_NONE) fake_span(src, bytes, what);
    if (kind == hipMemcpyDeviceToHost && fake_kind(dst) != FAKE_NONE) fake_span(dst, bytes, what);
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (!bytes) return hipSuccess;
    Lock lk(S().mu);
    check_copy(dst, src, bytes, kind, "hipMemcpy");
    memmove(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    if (!bytes) return hipSuccess;
    Lock lk(S().mu);
    check_copy(dst, src, bytes, kind, "hipMemcpyAsync");
    if (kind == hipMemcpyHostToDevice && fake_kind(src) == FAKE_NONE) {
        /* pageable source: staged before the call returns */
        std::shared_ptr<std::vector<uint8_t>> snap(new std::vector<uint8_t>((const uint8_t *)src, (const uint8_t *)src + bytes));
        return fake_enqueue(s, "copy (pageable source)", [=]() { fake_span(dst, bytes, "hipMemcpyAsync when it runs"); memcpy(dst, snap->data(), bytes); });
    }
    const hipError_t e = fake_enqueue(s, "copy", [=]() {
        check_copy(dst, src, bytes, kind, "hipMemcpyAsync when it runs");       /* both ends are still allocated */
        memmove(dst, src, bytes);
    });
    /* pageable destination: synchronous with respect to the host */
    if (kind == hipMemcpyDeviceToHost && fake_kind(dst) == FAKE_NONE) drain(stream_of(s), nullptr, 0);
    return e;
}

hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s)
{
    if (!bytes) return hipSuccess;
    Lock lk(S().mu);
    fake_span(dst, bytes, "hipMemsetAsync");
    return fake_enqueue(s, "memset", [=]() { fake_span(dst, bytes, "hipMemsetAsync when it runs"); memset(dst, value, bytes); });
}

}  // extern "C"
