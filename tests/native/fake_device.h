/*
 * tests/native/fake_device.h -- TEST INFRASTRUCTURE: what the fake kernels (fake_kernels.cpp) and the driver (fake_driver.cpp) need from
 * the CPU fake device (fake_device.cpp) beyond the HIP calls of fakehip/hip/hip_runtime.h.
 */
#ifndef FAKE_DEVICE_H
#define FAKE_DEVICE_H

#include <hip/hip_runtime.h>

#include <functional>
#include <vector>

enum FakeKind { FAKE_NONE = 0, FAKE_DEVICE = 1, FAKE_PINNED = 2 };

/* aborts with a message unless [ptr, ptr + len) lies inside ONE live device or pinned allocation; returns ptr */
const void *fake_span(const void *ptr, size_t len, const char *what);
/* kind of the live allocation that holds ptr, FAKE_NONE for pageable host memory */
FakeKind fake_kind(const void *ptr);
/* queue a kernel body on a stream: runs at once (eager) or when the host observes it (late) */
hipError_t fake_enqueue(hipStream_t s, const char *name, std::function<void()> body);
/* abort with a message: a fake kernel found something the GPU would silently get wrong */
[[noreturn]] void fake_die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
/* everything queued anywhere runs now (what process exit does) */
void fake_drain_all(void);
bool fake_schedule_late(void);

/* fake_kernels.cpp: one line per picture of every export launch (hvq_launch_rgb / _tensor / _resample), written when the launch RUNS */
struct FakeExportRecord { int call, job; uint64_t hash; };      /* FNV-1a-64 of the source Y | U | V planes as read at that moment */
const std::vector<FakeExportRecord> &fake_export_log(void);

#endif
