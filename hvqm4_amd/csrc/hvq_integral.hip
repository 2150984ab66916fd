/*
 * hvq_integral.hip -- summed-area tables for CDNA4 / gfx950 (MI355X): one plane of resident pictures becomes its inclusive table of
 * sums (uint32, modulo 2^32) and, where asked, of squares (uint64) (hvq_integral_pictures); the tables and the plane become a picture in
 * slot layout again, the local mean, the local deviation or a threshold relative to them over a window of any size at four reads a
 * table (hvq_window_pictures); and rectangles in device memory become their counts, sums and sums of squares (hvq_rect_sums).
 * include/hvqm4_amd.h specifies the values; hvq_integral.h holds the code of the lanes, shared with the tests' fake device, and says why
 * the wrapped corners are exact and what bounds every loop.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * hvq_integral_pictures is two launches behind one job table, grid row = picture in both.  The tables are the only working memory.
 *   1  row     a wave owns ONE row and walks it in chunks of 256 samples: a lane a dword of the plane, the four byte sums in the lane,
 *              the inclusive prefix of the lanes' totals by six shuffles, and a carry from chunk to chunk (the last lane's prefix,
 *              broadcast).  A wave reads 256 and writes 1024 (and 2048) consecutive bytes a chunk.  Four waves, four rows, a workgroup;
 *              they share nothing: no barrier, no LDS.
 *   2  column  a lane owns four adjacent columns and adds the rows' prefixes downwards in place, sixteen bytes a row, a wave 1 KiB a row.
 * No private memory, no atomics; no workgroup waits for another, and none reads what another writes.
 *
 * hvq_window_kernel: grid row = picture, a workgroup a tile of 64 x 16 samples of Y, a lane four adjacent samples and one dword stored;
 * the workgroups behind the Y tiles fill U | V with 128.  hvq_rect_kernel: a lane a rectangle, eight loads.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_integral.h"

typedef uint32_t u32;
typedef uint64_t u64;

template <bool SQUARES>
__device__ static inline __attribute__((always_inline)) void row_body(const HvqIntegralJob &J, u32 y, u32 lane)
{
    u32 carry = 0u;
    u64 qcarry = 0u;
    for (u32 c = 0; c < J.chunks; ++c) {
        const u32 v = hvq_ig_row_load(J, y, c, lane);
        const u32 t = hvq_ig_sum4(v), tq = hvq_ig_sq4(v);
        u32 s = t;
        u64 q = tq;
#pragma unroll
        for (u32 d = 1u; d < HVQ_IG_WAVE; d <<= 1) {
            s = hvq_ig_scan_step(s, __shfl_up(s, d), lane, d);
            if (SQUARES) q = hvq_ig_scan_step64(q, (u64)__shfl_up((unsigned long long)q, d), lane, d);
        }
        hvq_ig_row_store(J, y, c, lane, v, carry + s - t, qcarry + q - tq);
        carry += __shfl(s, (int)HVQ_IG_WAVE - 1);
        if (SQUARES) qcarry += (u64)__shfl((unsigned long long)q, (int)HVQ_IG_WAVE - 1);
    }
}

__global__ __launch_bounds__(HVQ_IG_RLANES)
void hvq_integral_row_kernel(const HvqIntegralJob *__restrict__ jobs)
{
    const HvqIntegralJob &J = jobs[blockIdx.y];
    const u32 y = blockIdx.x * HVQ_IG_WAVES + threadIdx.x / HVQ_IG_WAVE, lane = threadIdx.x & (HVQ_IG_WAVE - 1u);
    if (y >= J.ny) return;                                            /* uniform over the wave: every lane of a wave has the same row */
    if (J.squares) row_body<true>(J, y, lane);                        /* uniform */
    else row_body<false>(J, y, lane);
}

__global__ __launch_bounds__(HVQ_IG_CLANES)
void hvq_integral_column_kernel(const HvqIntegralJob *__restrict__ jobs)
{
    const HvqIntegralJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.colgroups) return;                            /* uniform */
    hvq_ig_column(J, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(HVQ_WN_LANES)
void hvq_window_kernel(const HvqWindowJob *__restrict__ jobs)
{
    const HvqWindowJob &J = jobs[blockIdx.y];
    const u32 t = blockIdx.x, lane = threadIdx.x;
    if (t >= J.tiles) return;                                         /* uniform */
    u32 *out = (u32 *)(uintptr_t)J.dst;
    if (t < J.ytiles) {                                               /* uniform */
        u32 x, y;
        hvq_wn_place(J, t, lane, &x, &y);
        if (x < J.nx && y < J.ny) out[((u64)y * J.nx + x) >> 2] = hvq_wn_dword(J, x, y);
        return;
    }
    u32 *chroma = out + (((u64)J.nx * J.ny) >> 2);
#pragma unroll
    for (u32 u = 0; u < HVQ_WN_PER; ++u) {
        const u32 d = hvq_wn_chroma(t - J.ytiles, lane, u);
        if (d < J.cdwords) chroma[d] = 0x80808080u;
    }
}

__global__ __launch_bounds__(HVQ_RC_LANES)
void hvq_rect_kernel(const HvqRectHead *__restrict__ head)
{
    const HvqRectHead &H = *head;
    const u32 r = blockIdx.x * HVQ_RC_LANES + threadIdx.x;
    if (r < H.nrects) hvq_rc_rect(H, (const HvqRectTables *)(head + 1), r);
}

/* jobs_dev: HvqIntegralJob[npics] in device memory, npics <= 65535; the maxima are over the pictures: of rowgroups and of colgroups */
extern "C" hipError_t hvq_launch_integral(const void *jobs_dev, int npics, uint32_t max_rowgroups, uint32_t max_colgroups, hipStream_t stream)
{
    if (npics <= 0 || !max_rowgroups || !max_colgroups) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqIntegralJob *jobs = (const HvqIntegralJob *)jobs_dev;
    hipLaunchKernelGGL(hvq_integral_row_kernel, dim3(max_rowgroups, (uint32_t)npics), dim3(HVQ_IG_RLANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_integral_column_kernel, dim3(max_colgroups, (uint32_t)npics), dim3(HVQ_IG_CLANES), 0, stream, jobs);
    return hipGetLastError();
}

/* jobs_dev: HvqWindowJob[npics] in device memory, npics <= 65535 */
extern "C" hipError_t hvq_launch_window(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_window_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_WN_LANES), 0, stream, (const HvqWindowJob *)jobs_dev);
    return hipGetLastError();
}

/* head_dev: an HvqRectHead and HvqRectTables[npics] behind it, in device memory */
extern "C" hipError_t hvq_launch_rects(const void *head_dev, int npics, uint32_t nrects, hipStream_t stream)
{
    if (npics <= 0 || !nrects) return hipSuccess;
    hipLaunchKernelGGL(hvq_rect_kernel, dim3((nrects + HVQ_RC_LANES - 1u) / HVQ_RC_LANES), dim3(HVQ_RC_LANES), 0, stream, (const HvqRectHead *)head_dev);
    return hipGetLastError();
}
