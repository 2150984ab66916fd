/*
 * hvq_metrics.hip -- picture metrics for CDNA4 / gfx950 (MI355X): per plane sum_a, sum_b, sum |a - b| and sum (a - b)^2 of a resident
 * picture `a` against a reference `b` (another resident picture, the caller's device memory, or zeros), as exact 64-bit integers
 * (hvq_picture_metrics, include/hvqm4_amd.h).  One launch serves any number of pairs of any sizes and samplings: grid row = pair.
 *
 * A unit of its own (its own Makefile rule and flags): the code of the kernels in hvq_kernels.hip does not change with it.
 *
 * Shape.  A workgroup of HVQ_MT_LANES lanes takes HVQ_MT_CHUNK consecutive 16-byte units of ONE plane (the job record says which
 * workgroup starts which plane), so it carries four accumulators.  A lane issues its HVQ_MT_UNITS loads of a and of b -- each wave
 * instruction one contiguous 1 KiB run -- before it touches the first, then per dword: v_sad_u8 for |a - b| and, against 0, for the
 * two sums; even and odd bytes spread into packed 16-bit halves, v_pk_sub_i16, v_dot2 for the squares.  The lane's partial sums go
 * 64 bits wide, across the wave by shuffles, across the four waves through LDS, and out as ONE 64-bit no-return atomic add per
 * value and workgroup, device scope, into the record (zeroed by the memset queued in front of the launch).  Integer addition: the
 * result does not depend on the order of arrival.  Nothing is read twice: the kernel should run at the rate HBM delivers 2 x
 * pic_bytes per pair.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_atomic, never flat (hvq_kernels.hip) */
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

static_assert(HVQ_MT_LANES == 256u && HVQ_MT_LANES % 64u == 0, "four waves: the LDS stage below");

/* Accumulator widths.  A lane sees HVQ_MT_UNITS * 16 = 64 samples of each picture, whatever the picture's size (the largest the
 * library opens, 8192 x 8192, only has more workgroups): its sums are at most 64 * 255 = 16 320 and its squares at most
 * 64 * 255^2 = 4 161 600 < 2^31 -- 32 bits, signed for v_dot2, hold them.  Everything that leaves the lane's own loop is 64 bits. */
static_assert((u64)HVQ_MT_UNITS * 16u * 255u * 255u < ((u64)1 << 31), "a lane's sum of squares must fit the signed 32-bit accumulator of v_dot2");

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool HAS_B>
__device__ __forceinline__ void lane_sums(const GLB u32x4 *__restrict__ a, const GLB u32x4 *__restrict__ b, u32 first, u32 n,
                                          u32 &sum_a, u32 &sum_b, u32 &sad, int &sse)
{
    u32x4 va[HVQ_MT_UNITS], vb[HVQ_MT_UNITS];
#pragma unroll
    for (u32 k = 0; k < HVQ_MT_UNITS; ++k) {
        const u32 i = first + k * HVQ_MT_LANES;
        const u32x4 z = { 0u, 0u, 0u, 0u };
        /* a unit past the plane's end contributes zeros; the load itself is predicated: nothing outside the plane is read */
        va[k] = i < n ? __builtin_nontemporal_load(a + i) : z;
        vb[k] = HAS_B && i < n ? __builtin_nontemporal_load(b + i) : z;
    }
#pragma unroll
    for (u32 k = 0; k < HVQ_MT_UNITS; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 x = va[k][c], y = vb[k][c];
            sum_a = __builtin_amdgcn_sad_u8(x, 0u, sum_a);
            if (HAS_B) {
                sum_b = __builtin_amdgcn_sad_u8(y, 0u, sum_b);
                sad = __builtin_amdgcn_sad_u8(x, y, sad);
            }
            const s16x2 de = __builtin_bit_cast(s16x2, x & 0x00FF00FFu) - __builtin_bit_cast(s16x2, y & 0x00FF00FFu);
            const s16x2 dq = __builtin_bit_cast(s16x2, (x >> 8) & 0x00FF00FFu) - __builtin_bit_cast(s16x2, (y >> 8) & 0x00FF00FFu);
            sse = __builtin_amdgcn_sdot2(de, de, sse, false);
            sse = __builtin_amdgcn_sdot2(dq, dq, sse, false);
        }
}

__global__ __launch_bounds__(HVQ_MT_LANES)
void hvq_metrics_kernel(const HvqMetricsJob *__restrict__ jobs)
{
    const HvqMetricsJob &J = jobs[blockIdx.y];
    const u32 wg = blockIdx.x;
    if (wg >= J.wg_first[3]) return;                                   /* past this picture: leave (uniform) */
    const u32 p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);       /* the workgroup's plane */
    const u32 n = J.units[p];
    const u32 first = (wg - J.wg_first[p]) * HVQ_MT_CHUNK + threadIdx.x;
    const GLB u32x4 *a = (const GLB u32x4 *)(uintptr_t)(J.a + J.plane_off[p]);
    u32 sum_a = 0, sum_b = 0, sad = 0;
    int sse = 0;
    if (J.b) lane_sums<true>(a, (const GLB u32x4 *)(uintptr_t)(J.b + J.plane_off[p]), first, n, sum_a, sum_b, sad, sse);
    else { lane_sums<false>(a, nullptr, first, n, sum_a, sum_b, sad, sse); sad = sum_a; }      /* |a - 0| = a */

    __shared__ u64 part[HVQ_MT_LANES / 64u][4];
    const u64 w0 = wave_sum(sum_a), w1 = wave_sum(sum_b), w2 = wave_sum(sad), w3 = wave_sum((u64)(u32)sse);
    if ((threadIdx.x & 63u) == 0) {
        u64 *row = part[threadIdx.x >> 6];
        row[0] = w0; row[1] = w1; row[2] = w2; row[3] = w3;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        u64 t = 0;
#pragma unroll
        for (u32 w = 0; w < HVQ_MT_LANES / 64u; ++w) t += part[w][threadIdx.x];
        GLB u64 *out = (GLB u64 *)(uintptr_t)J.out + p * 4u + threadIdx.x;
        (void)__hip_atomic_fetch_add(out, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* jobs_dev: HvqMetricsJob[njobs] in device memory; max_wgs = max over jobs of wg_first[3].  The records the jobs point to are zero
 * when the launch runs (the caller queues the memset in front of it on the same stream). */
extern "C" hipError_t hvq_launch_metrics(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0 || !max_wgs) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_metrics_kernel, dim3(max_wgs, (uint32_t)njobs), dim3(HVQ_MT_LANES), 0, stream, (const HvqMetricsJob *)jobs_dev);
    return hipGetLastError();
}
