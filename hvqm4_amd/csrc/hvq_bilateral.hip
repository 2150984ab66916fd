/*
 * hvq_bilateral.hip -- bilateral filters for CDNA4 / gfx950 (MI355X): resident pictures through a weighted mean whose weights depend on
 * the samples themselves (spatial[|j|][|i|] * range[|guide difference|]), plane by plane, into uint8 pictures of the same geometry in
 * slot layout (hvq_bilateral_pictures, include/hvqm4_amd.h: the values, exact integers with one rounding).  One launch serves any number
 * of pictures of any sizes, samplings, parameter sets and guides: grid row = picture (three HvqBilateralJob, one per plane), grid column
 * = one tile of one of its planes, Y's first; workgroups past the picture's tiles leave.  The call's parameter sets lie behind the jobs.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * Two bodies, chosen per plane on the host (hvq_bl_job); the values do not depend on the choice.  The arithmetic is hvq_bilateral.h's,
 * shared with the tests' fake device; this file stages, puts the barrier behind the staging and stores.
 *   Stage.    A tile is HVQ_BL_TW x HVQ_BL_TH targets.  Its 16 + 2 ry source rows, row indices clamped into the plane, go into LDS as 20
 *             aligned dwords each (the tile's 64 bytes and 8 of halo on either side; a dword outside the row becomes the row's edge
 *             sample), a lane up to three dwords, all loads issued before the first is stored; the guide's tile the same way when the
 *             picture has a guide; the plane's 256 range bytes by the first wave, a dword a lane.  Nothing clamps after this.
 *   Taps.     A double loop over the window.  The spatial factor of a tap is workgroup-uniform: a row of the table is one scalar qword
 *             load, a factor of 0 skips the tap by a uniform branch.  Per tap a lane reads the neighbour dword of its four targets (two
 *             aligned dwords and v_alignbyte_b32; the guide's likewise), takes four |differences|, four range bytes from LDS, and adds
 *             w and w * a by 24-bit multiply-adds.  Then one exact 32-bit division a sample.
 *   Copy.     A plane of radius 0 in both axes: a tile is HVQ_BL_CTW x HVQ_BL_CTH samples, a lane moves a dword in each of four rows.
 * LDS: two tiles of 30 x 20 dwords and 64 dwords of range table, 4.9 KiB.  No atomics, no private memory, no scratch buffer; every
 * target byte is written once, by one store; nothing else is written.  No workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_bilateral.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

static_assert(HVQ_BL_LANES == 256u && HVQ_BL_TW == 64u && HVQ_BL_TH == 16u, "the lane map: 16 dwords x 16 rows of targets");

__device__ __forceinline__ void stage(u64 plane, u32 nx, u32 ny, u32 c0, u32 r0, u32 ry, u32 *raw)
{
    const u32 lane = threadIdx.x, rows = HVQ_BL_TH + 2u * ry;
    u32 v[3];
#pragma unroll
    for (u32 u = 0; u < 3u; ++u) {
        const u32 idx = lane + HVQ_BL_LANES * u, rr = idx / HVQ_BL_ROW_DWORDS, k = idx - rr * HVQ_BL_ROW_DWORDS;
        v[u] = 0;
        if (rr < rows) v[u] = hvq_bl_stage_value(((const GLB u32 *)(uintptr_t)plane)[(u64)hvq_bl_stage_row(r0, rr, ry, ny) * (nx >> 2) + hvq_bl_stage_dword(c0, k, nx)], c0, k, nx);
    }
#pragma unroll
    for (u32 u = 0; u < 3u; ++u) {
        const u32 idx = lane + HVQ_BL_LANES * u;
        if (idx < rows * HVQ_BL_ROW_DWORDS) raw[idx] = v[u];
    }
}

__device__ __forceinline__ void general_body(const HvqBilateralJob &J, const uint8_t *set, u32 c0, u32 r0, u32 *A, u32 *G, u32 *range)
{
    const u32 lane = threadIdx.x;
    const bool guided = J.guide != 0;                                  /* uniform */
    stage(J.src, J.nx, J.ny, c0, r0, J.ry, A);
    if (guided) stage(J.guide, J.nx, J.ny, c0, r0, J.ry, G);
    if (lane < 64u) range[lane] = ((const GLB u32 *)(uintptr_t)(set + HVQ_BL_RANGE_AT))[lane];
    __syncthreads();
    const u32 v = guided ? hvq_bl_lane(lane, J.rx, J.ry, 1, set + HVQ_BL_SPATIAL_AT, A, G, (const uint8_t *)range)
                         : hvq_bl_lane(lane, J.rx, J.ry, 0, set + HVQ_BL_SPATIAL_AT, A, A, (const uint8_t *)range);
    const u32 row = r0 + (lane >> 4), colx = c0 + (lane & 15u) * 4u;
    if (row < J.ny && colx < J.nx) *(GLB u32 *)(uintptr_t)(J.dst + (u64)row * J.nx + colx) = v;
}

__device__ __forceinline__ void copy_body(const HvqBilateralJob &J, u32 c0, u32 r0)
{
    const u32 lane = threadIdx.x;
    const u32 nx = J.nx, ny = J.ny;
    const u32 col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);    /* rows rb, rb + 4, rb + 8, rb + 12 */
    if (col >= nx) return;                                            /* nx is a multiple of 4: a dword lies inside the row or outside */
    const GLB u32 *in = (const GLB u32 *)(uintptr_t)(J.src + col);
    GLB u32 *out = (GLB u32 *)(uintptr_t)(J.dst + col);
    u32 v[4];
#pragma unroll
    for (u32 s = 0; s < 4u; ++s) v[s] = rb + 4u * s < ny ? in[(u64)(rb + 4u * s) * (nx >> 2)] : 0u;
#pragma unroll
    for (u32 s = 0; s < 4u; ++s)
        if (rb + 4u * s < ny) out[(u64)(rb + 4u * s) * (nx >> 2)] = v[s];
}

__global__ __launch_bounds__(HVQ_BL_LANES)
void hvq_bilateral_kernel(const HvqBilateralJob *__restrict__ jobs, const uint8_t *__restrict__ sets)
{
    const HvqBilateralJob *P = jobs + 3u * blockIdx.y;                 /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqBilateralJob &J = *P;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    __shared__ u32 A[HVQ_BL_BUF], G[HVQ_BL_BUF], range[64];
    if (J.body == HVQ_BL_COPY) copy_body(J, tx * HVQ_BL_CTW, ty * HVQ_BL_CTH);
    else general_body(J, sets + (size_t)J.ps * HVQ_BL_PLANE_BYTES, tx * HVQ_BL_TW, ty * HVQ_BL_TH, A, G, range);
}

/* jobs_dev: HvqBilateralJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, and behind them the call's
 * parameter sets (HVQ_BL_PLANE_BYTES a plane), npics <= 65535; max_tiles = max over the pictures of the tiles of their three planes
 * together */
extern "C" hipError_t hvq_launch_bilateral(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqBilateralJob *jobs = (const HvqBilateralJob *)jobs_dev;
    hipLaunchKernelGGL(hvq_bilateral_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_BL_LANES), 0, stream, jobs, (const uint8_t *)(jobs + 3 * (size_t)npics));
    return hipGetLastError();
}
