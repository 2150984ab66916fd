/*
 * hvq_distance.hip -- exact distance transforms for CDNA4 / gfx950 (MI355X): the foreground of one plane of resident pictures becomes a
 * map of its distances to the background (hvq_distance_pictures: squared Euclidean, city block or chessboard, integers, nothing
 * rounded), and a map becomes a mask picture in slot layout again (hvq_distance_mask).  include/hvqm4_amd.h specifies the values;
 * hvq_distance.h holds the code of the lanes, shared with the tests' fake device, and says why the transform is separable and what
 * bounds every loop.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * hvq_distance_pictures is two launches behind one job table, grid row = picture in both.  The map is the only working memory.
 *   1  column  a lane owns four adjacent columns and walks them down and up; a wave reads 256 and writes 1024 consecutive bytes a row.
 *              The map then holds g, the vertical distance to the column's nearest background sample.
 *   2  row     a workgroup owns as many whole rows as hold 8192 samples, stages their g into 16 KiB of LDS as uint16, and behind ONE
 *              barrier overwrites them in place: a lane a sample, consecutive lanes consecutive samples, searching outwards in LDS.
 * No private memory, no atomics; no workgroup waits for another, and none reads what another writes.
 *
 * hvq_distance_mask_kernel has the map kernel's shape (hvq_map.hip): a tile is HVQ_MP_TILE consecutive dwords of a plane; a Y dword
 * reads sixteen bytes of distances, U and V are filled with 128.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_map.h"
#include "hvq_distance.h"

typedef uint32_t u32;

__global__ __launch_bounds__(HVQ_DT_CLANES)
void hvq_distance_column_kernel(const HvqDistanceJob *__restrict__ jobs)
{
    const HvqDistanceJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.colgroups) return;                            /* uniform */
    hvq_dt_column(J, blockIdx.x, threadIdx.x);
}

template <u32 METRIC>
__device__ static inline __attribute__((always_inline)) void row_body(const HvqDistanceJob &J, u32 group, u32 lane, uint16_t *G)
{
    const u32 rounds = (hvq_dt_row_samples(J, group) + HVQ_DT_LANES * 4u - 1u) / (HVQ_DT_LANES * 4u);
    for (u32 r = 0; r < rounds; ++r) hvq_dt_row_stage(J, group, r, lane, G);
    __syncthreads();                                                  /* from here on the rows of the map are overwritten */
    for (u32 r = 0; r < rounds; ++r) hvq_dt_row_store<METRIC>(J, group, r, lane, G);
}

__global__ __launch_bounds__(HVQ_DT_LANES)
void hvq_distance_row_kernel(const HvqDistanceJob *__restrict__ jobs)
{
    const HvqDistanceJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.rowgroups) return;                            /* uniform */
    __shared__ __attribute__((aligned(16))) uint16_t G[HVQ_DT_SPAN];
    if (J.metric == HVQ_DT_EUCLID2) row_body<HVQ_DT_EUCLID2>(J, blockIdx.x, threadIdx.x, G);        /* uniform */
    else if (J.metric == HVQ_DT_CITY) row_body<HVQ_DT_CITY>(J, blockIdx.x, threadIdx.x, G);
    else row_body<HVQ_DT_CHESS>(J, blockIdx.x, threadIdx.x, G);
}

__global__ __launch_bounds__(HVQ_MP_LANES)
void hvq_distance_mask_kernel(const HvqDistMaskJob *__restrict__ jobs)
{
    const HvqDistMaskJob *P = jobs + 3u * blockIdx.y;                 /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqDistMaskJob &J = *P;
    const u32 lane = threadIdx.x, n = J.dwords;
    u32 *out = (u32 *)(uintptr_t)J.dst;
#pragma unroll
    for (u32 u = 0; u < HVQ_MP_PER; ++u) {
        const u32 d = hvq_mp_dword(t, lane, u);
        if (d < n) out[d] = J.body == HVQ_DM_FILL ? 0x80808080u : hvq_dm_dword(J, d);
    }
}

/* jobs_dev: HvqDistanceJob[npics] in device memory, npics <= 65535; the maxima are over the pictures: of colgroups and of rowgroups */
extern "C" hipError_t hvq_launch_distance(const void *jobs_dev, int npics, uint32_t max_colgroups, uint32_t max_rowgroups, hipStream_t stream)
{
    if (npics <= 0 || !max_colgroups || !max_rowgroups) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqDistanceJob *jobs = (const HvqDistanceJob *)jobs_dev;
    hipLaunchKernelGGL(hvq_distance_column_kernel, dim3(max_colgroups, (uint32_t)npics), dim3(HVQ_DT_CLANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_distance_row_kernel, dim3(max_rowgroups, (uint32_t)npics), dim3(HVQ_DT_LANES), 0, stream, jobs);
    return hipGetLastError();
}

/* jobs_dev: HvqDistMaskJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535 */
extern "C" hipError_t hvq_launch_distance_mask(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_distance_mask_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_MP_LANES), 0, stream, (const HvqDistMaskJob *)jobs_dev);
    return hipGetLastError();
}
