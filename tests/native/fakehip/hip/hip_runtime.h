/*
 * tests/native/fakehip/hip/hip_runtime.h -- TEST INFRASTRUCTURE: the part of the HIP API that hvqm4_amd/csrc/hvq_runtime.cpp uses,
 * declared for the CPU fake device (tests/native/fake_device.cpp).  Put this directory in front of the include path and the
 * runtime compiles, unchanged, with a host compiler.
 */
#ifndef FAKEHIP_HIP_RUNTIME_H
#define FAKEHIP_HIP_RUNTIME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
    hipErrorNotReady = 600
} hipError_t;

typedef struct fakehipStream *hipStream_t;
typedef struct fakehipEvent *hipEvent_t;

typedef enum hipMemcpyKind {
    hipMemcpyHostToHost = 0,
    hipMemcpyHostToDevice = 1,
    hipMemcpyDeviceToHost = 2,
    hipMemcpyDeviceToDevice = 3,
    hipMemcpyDefault = 4
} hipMemcpyKind;

#define hipStreamNonBlocking    0x01u
#define hipEventDisableTiming   0x02u
#define hipHostMallocDefault    0x0u

const char *hipGetErrorString(hipError_t e);
hipError_t hipGetDeviceCount(int *n);
hipError_t hipSetDevice(int device);
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest);

hipError_t hipMalloc(void **p, size_t bytes);
hipError_t hipFree(void *p);
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags);
hipError_t hipHostFree(void *p);

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags);
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);

hipError_t hipEventCreate(hipEvent_t *e);
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventQuery(hipEvent_t e);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b);

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif
