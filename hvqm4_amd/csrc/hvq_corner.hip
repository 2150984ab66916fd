/*
 * hvq_corner.hip -- corner detection for CDNA4 / gfx950 (MI355X): one plane of resident pictures becomes a mask picture in slot layout,
 * a row index and an ordered list of corners, with the response map where it is asked for (hvq_corner_pictures).  include/hvqm4_amd.h
 * specifies the values; hvq_corner.h holds the code of the lanes, shared with the tests' fake device, and says what lies where in LDS.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * Four launches behind one job table, grid row = picture in each.  No memory besides the outputs.
 *   1  tile     a workgroup takes a 64 x 16 tile: it stages the bytes with a halo of nms + r + 1, clamped when staged, as aligned
 *               dwords; computes both gradients once per staged position; forms gx gx, gx gy, gy gy as sums that slide along the rows
 *               and then down the columns (2 products enter and leave per position, whatever r is); computes the 64-bit response over
 *               the tile and its nms halo into LDS; suppresses from LDS; a lane stores one dword of the mask and, where asked, 32 bytes
 *               of responses.  The workgroups behind the tiles fill the two planes of the mask that are not analysed.
 *   2  count    a wave a row: ballots over the bytes of the mask, the population counts add up to the row's corners.
 *   3  scan     ONE workgroup a picture turns the counts into the row index (rows[y] = the corners above row y) and writes the head
 *               of the list.
 *   4  list     a wave a row: the same ballots place the row's corners behind rows[y] in x order; the response of a corner is
 *               computed again from the plane, by the function that launch 1 used.
 * No private memory; no workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_corner.h"

typedef uint32_t u32;
typedef uint64_t u64;

__global__ __launch_bounds__(HVQ_CR_LANES)
void hvq_corner_tile_kernel(const HvqCornerJob *__restrict__ jobs)
{
    const HvqCornerJob &J = jobs[blockIdx.y];
    const u32 lane = threadIdx.x, tiles = J.tx * J.ty;
    u32 t = blockIdx.x;
    if (t >= tiles) {                                                 /* past the tiles: a fill tile of one of the other planes, or none (uniform) */
        t -= tiles;
        u32 f = 0u;
        if (t >= J.fill_tiles[0]) { t -= J.fill_tiles[0]; f = 1u; }
        if (t >= J.fill_tiles[f]) return;
        hvq_cr_fill(J, f, t, lane);
        return;
    }
    __shared__ __attribute__((aligned(16))) u32 L[HVQ_CR_LDS];
    hvq_cr_stage(J, t, lane, L);
    __syncthreads();
    hvq_cr_gradients(J, lane, L);
    __syncthreads();
    hvq_cr_hsums(J, lane, L);
    __syncthreads();                                                  /* G is dead: the responses go over it */
    hvq_cr_responses(J, t, lane, L);
    __syncthreads();
    hvq_cr_suppress(J, t, lane, L);
}

/* the corners of 64 dwords of a row, lane l holding dword l: bit l of b[s] says that byte s of that dword is 255 */
__device__ static inline u32 corner_ballots(u32 v, u64 b[4])
{
    u32 n = 0u;
#pragma unroll
    for (u32 s = 0; s < 4u; ++s) {
        b[s] = __ballot((v >> (8u * s)) & 1u);
        n += (u32)__popcll(b[s]);
    }
    return n;
}

__global__ __launch_bounds__(HVQ_CR_LANES)
void hvq_corner_count_kernel(const HvqCornerJob *__restrict__ jobs)
{
    const HvqCornerJob &J = jobs[blockIdx.y];
    const u32 lane = threadIdx.x & 63u, y = blockIdx.x * (HVQ_CR_LANES / 64u) + (threadIdx.x >> 6);
    if (y >= J.ny) return;                                            /* wave-uniform */
    u32 count = 0u;
    for (u32 d0 = 0; d0 < (J.nx >> 2); d0 += 64u) {
        u64 b[4];
        count += corner_ballots(hvq_cr_mask_dword(J, y, d0 + lane), b);
    }
    if (!lane) hvq_cr_count_store(J, y, count);
}

__global__ __launch_bounds__(HVQ_CR_LANES)
void hvq_corner_scan_kernel(const HvqCornerJob *__restrict__ jobs)
{
    const HvqCornerJob &J = jobs[blockIdx.x];
    const u32 lane = threadIdx.x;
    __shared__ u32 S[2][HVQ_CR_LANES];
    const u32 mine = hvq_cr_scan_sum(J, lane);
    S[0][lane] = mine;
    __syncthreads();
    for (u32 k = 0; k < 8u; ++k) {                                    /* inclusive scan by doubling: the result stands in S[0] */
        const u32 f = k & 1u, s = 1u << k;
        S[f ^ 1u][lane] = S[f][lane] + (lane >= s ? S[f][lane - s] : 0u);
        __syncthreads();
    }
    hvq_cr_scan_store(J, lane, S[0][lane] - mine);
    if (lane == HVQ_CR_LANES - 1u) hvq_cr_head(J, S[0][lane]);
}

__global__ __launch_bounds__(HVQ_CR_LANES)
void hvq_corner_list_kernel(const HvqCornerJob *__restrict__ jobs)
{
    const HvqCornerJob &J = jobs[blockIdx.y];
    const u32 lane = threadIdx.x & 63u, y = blockIdx.x * (HVQ_CR_LANES / 64u) + (threadIdx.x >> 6);
    if (y >= J.ny) return;                                            /* wave-uniform */
    const u32 *rows = (const u32 *)(uintptr_t)J.rows;
    u32 base = rows[y];
    if (rows[y + 1u] == base || base >= J.cap) return;                /* no corner in this row, or no room left for one: wave-uniform */
    const u64 below = (1ull << lane) - 1ull;
    for (u32 d0 = 0; d0 < (J.nx >> 2); d0 += 64u) {
        u64 b[4];
        const u32 v = hvq_cr_mask_dword(J, y, d0 + lane), n = corner_ballots(v, b);
        if (v) {
            u32 j = base + (u32)(__popcll(b[0] & below) + __popcll(b[1] & below) + __popcll(b[2] & below) + __popcll(b[3] & below));
#pragma unroll
            for (u32 s = 0; s < 4u; ++s)
                if ((v >> (8u * s)) & 1u) hvq_cr_emit(J, 4u * (d0 + lane) + s, y, ++j);
        }
        base += n;
    }
}

/* jobs_dev: HvqCornerJob[npics] in device memory, npics <= 65535; max_tiles is the most of hvq_cr_tiles, max_rows the most of ny */
extern "C" hipError_t hvq_launch_corner(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_rows, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles || !max_rows) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqCornerJob *jobs = (const HvqCornerJob *)jobs_dev;
    const u32 n = (u32)npics, row_wgs = (max_rows + HVQ_CR_LANES / 64u - 1u) / (HVQ_CR_LANES / 64u);
    hipLaunchKernelGGL(hvq_corner_tile_kernel, dim3(max_tiles, n), dim3(HVQ_CR_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_corner_count_kernel, dim3(row_wgs, n), dim3(HVQ_CR_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_corner_scan_kernel, dim3(n), dim3(HVQ_CR_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_corner_list_kernel, dim3(row_wgs, n), dim3(HVQ_CR_LANES), 0, stream, jobs);
    return hipGetLastError();
}
