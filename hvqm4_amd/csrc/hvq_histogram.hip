/*
 * hvq_histogram.hip -- 256-bin histograms of pictures for CDNA4 / gfx950 (MI355X): per plane the count of every sample value of a
 * picture `a` (HVQ_HIST_VALUES) or of every |a - b| against a reference `b` (HVQ_HIST_ABSDIFF), as exact 32-bit integers
 * (hvq_picture_histograms, include/hvqm4_amd.h).  One launch serves any number of pictures of any sizes and samplings: grid row = picture.
 *
 * A unit of its own (its own Makefile rule and flags): the code of the other kernels does not change with it.
 *
 * Shape.  The memory side is hvq_metrics.hip's: a workgroup of HVQ_HG_LANES lanes works on ONE plane; per chunk a lane issues its
 * HVQ_HG_UNITS 16-byte nontemporal loads of a (and of b) -- each wave instruction one contiguous 1 KiB run -- before it touches the
 * first; units past the plane's end are predicated off and counted nowhere.  Counting is what sets this kernel apart: every wave owns
 * private 256-bin histograms in LDS (four copies picked by lane bits, 16.5 KiB per workgroup) and adds into them with no-return
 * workgroup-scope atomics (ds_add_u32), one per sample -- except where sixteen equal samples make one add of 16, and a wave that
 * holds nothing else one add for all its lanes: many lanes of a wave adding into ONE word is the slow case of the LDS (a flat picture
 * took 6 x the time of a natural one without this, and takes less than half of it with).  A workgroup takes ONE chunk of
 * HVQ_HG_CHUNK units, then lane v sums the copies of bin v and issues one no-return device-scope global_atomic_add for it if it is
 * not zero, into the record (zeroed by the memset queued in front of the launch).  Integer addition: the result does not depend on the order of arrival.  What was measured to get here --
 * same-address conflicts, chunks per workgroup, ABSDIFF against VALUES -- is DESIGN.md 4.5.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"

typedef uint32_t u32;
#define GLB __attribute__((address_space(1)))           /* global_load / global_atomic, never flat (hvq_kernels.hip) */
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

/* a wave's histogram is kept HVQ_HG_COPIES times, lane l adding into copy l % HVQ_HG_COPIES: neighbouring lanes hold neighbouring
 * samples, which are often equal or close, and land in different words and -- the copies being 8 dwords more than 256 apart -- banks */
#define HVQ_HG_COPIES 4u
#define HVQ_HG_STRIDE (HVQ_HG_BINS + 8u)
static_assert((HVQ_HG_COPIES & (HVQ_HG_COPIES - 1u)) == 0 && HVQ_HG_COPIES <= 64u, "a lane's copy is picked by its low lane bits");

static_assert(HVQ_HG_LANES == 256u, "lane v flushes bin v: as many lanes as bins");
#define HVQ_HG_WAVES (HVQ_HG_LANES / 64u)

__device__ __forceinline__ void lds_add(u32 *h, u32 bin, u32 v)
{
    (void)__hip_atomic_fetch_add(h + bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* the four samples of a dword */
__device__ __forceinline__ void count_dword(u32 *h, u32 x)
{
    lds_add(h, x & 255u, 1u);
    lds_add(h, (x >> 8) & 255u, 1u);
    lds_add(h, (x >> 16) & 255u, 1u);
    lds_add(h, x >> 24, 1u);
}

/* per byte |x - y|: even and odd bytes spread into packed 16-bit halves (hvq_metrics.hip), v_pk_sub_i16 both ways, v_pk_max_i16 */
__device__ __forceinline__ u32 absdiff_bytes(u32 x, u32 y)
{
    const s16x2 xe = __builtin_bit_cast(s16x2, x & 0x00FF00FFu), ye = __builtin_bit_cast(s16x2, y & 0x00FF00FFu);
    const s16x2 xo = __builtin_bit_cast(s16x2, (x >> 8) & 0x00FF00FFu), yo = __builtin_bit_cast(s16x2, (y >> 8) & 0x00FF00FFu);
    const s16x2 de = __builtin_elementwise_max(xe - ye, ye - xe), dq = __builtin_elementwise_max(xo - yo, yo - xo);
    return __builtin_bit_cast(u32, de) | (__builtin_bit_cast(u32, dq) << 8);
}

template <bool HAS_B>
__device__ __forceinline__ void count_chunk(u32 *h, u32 *hw, const GLB u32x4 *__restrict__ a, const GLB u32x4 *__restrict__ b, u32 first, u32 n)
{
    u32x4 va[HVQ_HG_UNITS], vb[HVQ_HG_UNITS];
#pragma unroll
    for (u32 k = 0; k < HVQ_HG_UNITS; ++k) {
        const u32 i = first + k * HVQ_HG_LANES;
        const u32x4 z = { 0u, 0u, 0u, 0u };
        /* the load of a unit past the plane's end is predicated: nothing outside the plane is read */
        va[k] = i < n ? __builtin_nontemporal_load(a + i) : z;
        vb[k] = HAS_B && i < n ? __builtin_nontemporal_load(b + i) : z;
    }
#pragma unroll
    for (u32 k = 0; k < HVQ_HG_UNITS; ++k) {
        if (first + k * HVQ_HG_LANES >= n) continue;                   /* ... and nothing of it is counted */
        u32x4 d = va[k];
        if (HAS_B) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d[c] = absdiff_bytes(va[k][c], vb[k][c]);
        }
        /* sixteen equal samples (flat areas, black frames, identical pictures): one add of 16 ... */
        const bool flat = d[0] == d[1] && d[0] == d[2] && d[0] == d[3] && d[0] == ((d[0] >> 8) | (d[0] << 24));
        /* ... and when every lane of the wave that is inside the plane holds the same sixteen, its first lane adds for all: the lanes
         * inside the plane are a prefix of the wave, so that lane is among them */
        const u32 lead = __builtin_amdgcn_readfirstlane(d[0]);
        const u32 inside = (u32)__popcll(__ballot(1));                 /* counted here, where all those lanes are still active */
        if (__all(flat && d[0] == lead)) {
            if ((threadIdx.x & 63u) == 0) lds_add(hw, lead & 255u, 16u * inside);
            continue;
        }
        if (flat) { lds_add(h, d[0] & 255u, 16u); continue; }
#pragma unroll
        for (int c = 0; c < 4; ++c) count_dword(h, d[c]);
    }
}

__global__ __launch_bounds__(HVQ_HG_LANES)
void hvq_histogram_kernel(const HvqHistogramJob *__restrict__ jobs)
{
    const HvqHistogramJob &J = jobs[blockIdx.y];
    const u32 wg = blockIdx.x;
    if (wg >= J.wg_first[3]) return;                                   /* past this picture: leave (uniform) */
    const u32 p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);       /* the workgroup's plane */
    const u32 n = J.units[p];
    const u32 first = (wg - J.wg_first[p]) * HVQ_HG_CHUNK + threadIdx.x;

    __shared__ u32 hist[HVQ_HG_WAVES * HVQ_HG_COPIES][HVQ_HG_STRIDE];
#pragma unroll
    for (u32 w = 0; w < HVQ_HG_WAVES * HVQ_HG_COPIES; ++w) hist[w][threadIdx.x] = 0u;
    __syncthreads();

    u32 *hw = hist[(threadIdx.x >> 6) * HVQ_HG_COPIES];                                            /* the wave's first copy */
    u32 *h = hist[(threadIdx.x >> 6) * HVQ_HG_COPIES + (threadIdx.x & (HVQ_HG_COPIES - 1u))];      /* the lane's copy */
    const GLB u32x4 *a = (const GLB u32x4 *)(uintptr_t)(J.a + J.plane_off[p]);
    const GLB u32x4 *b = (const GLB u32x4 *)(uintptr_t)(J.b + J.plane_off[p]);
    if (J.b) count_chunk<true>(h, hw, a, b, first, n);
    else count_chunk<false>(h, hw, a, nullptr, first, n);
    __syncthreads();

    u32 t = 0;
#pragma unroll
    for (u32 w = 0; w < HVQ_HG_WAVES * HVQ_HG_COPIES; ++w) t += hist[w][threadIdx.x];
    if (t) {
        GLB u32 *out = (GLB u32 *)(uintptr_t)J.out + p * HVQ_HG_BINS + threadIdx.x;
        (void)__hip_atomic_fetch_add(out, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* jobs_dev: HvqHistogramJob[njobs] in device memory; max_wgs = max over jobs of wg_first[3].  The records the jobs point to are zero
 * when the launch runs (the caller queues the memset in front of it on the same stream). */
extern "C" hipError_t hvq_launch_histograms(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0 || !max_wgs) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_histogram_kernel, dim3(max_wgs, (uint32_t)njobs), dim3(HVQ_HG_LANES), 0, stream, (const HvqHistogramJob *)jobs_dev);
    return hipGetLastError();
}
