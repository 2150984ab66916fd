/*
 * hvq_rank.hip -- rank filters for CDNA4 / gfx950 (MI355X): resident pictures through erosion, dilation, the range and the 3 x 3 or 5 x 5
 * median, plane by plane, into uint8 pictures of the same geometry in slot layout (hvq_rank_pictures, include/hvqm4_amd.h: the values;
 * they select samples and never round).  One launch serves any number of pictures of any sizes, samplings and operations: grid row =
 * picture (three HvqRankJob, one per plane), grid column = one tile of one of its planes, Y's first; workgroups past the picture's tiles
 * leave.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * Four bodies, chosen per plane on the host (hvq_rk_job); the values do not depend on the choice.  The phases of the three that compute
 * are hvq_rank.h's, shared with the tests' fake device; this file stages, puts the barriers between the phases and stores.
 *   Stage.    A tile is HVQ_RK_TW x HVQ_RK_TH targets.  Its 16 + 2 r source rows, row indices clamped into the plane, go into LDS as 24
 *             aligned dwords each (the tile's 64 bytes and 16 of halo on either side; a dword outside the row becomes the row's edge
 *             sample), a lane up to five dwords, all loads issued before the first is stored.  Nothing clamps after this.
 *   Min/max.  Windows by doubling, ceil(log2 (2 r + 1)) steps an axis instead of 2 r + 1 taps: horizontal over the staged rows, then
 *             vertical over the tile's 16 dwords a row; four samples a dword through v_pk_min_u16 / v_pk_max_u16 on the even and the
 *             odd bytes.  A step reads one LDS array and writes another, a barrier between two; the last leaves the lane's dword in a
 *             register.  RANGE runs min and max side by side through the same steps and subtracts.
 *   Median.   The columns under one another are sorted once (3 or 9 exchanges a dword of four columns) into one LDS array a level; a
 *             lane then reads the 3 or 5 neighbouring columns of its four targets from every level (three aligned dwords and
 *             v_alignbyte_b32) and selects: 12 min / max for 3 x 3, the pruned network of hvq_rank.h (134 min / max) for 5 x 5, in
 *             registers, the dwords unpacked into even and odd bytes once.
 *   Copy.     A plane that is copied (radius 0 under MIN, MAX, MEDIAN): a tile is HVQ_RK_CTW x HVQ_RK_CTH samples, a lane moves a dword in
 *             each of four rows.
 * LDS: five arrays of 46 x 24 dwords, 21.6 KiB.  No private memory, no scratch buffer; every target byte is written once, by one store;
 * nothing else is written.  No workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_rank.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

static_assert(HVQ_RK_LANES == 256u && HVQ_RK_TW == 64u && HVQ_RK_TH == 16u, "the lane maps: 16 dwords x 16 rows of targets");

__device__ __forceinline__ void stage(const HvqRankJob &J, u32 c0, u32 r0, u32 r, u32 *raw)
{
    const u32 lane = threadIdx.x, nx = J.nx, ny = J.ny, rows = HVQ_RK_TH + 2u * r;
    u32 v[5];
#pragma unroll
    for (u32 u = 0; u < 5u; ++u) {
        const u32 idx = lane + HVQ_RK_LANES * u, rr = idx / HVQ_RK_ROW_DWORDS, k = idx - rr * HVQ_RK_ROW_DWORDS;
        v[u] = 0;
        if (rr < rows) v[u] = hvq_rk_stage_value(((const GLB u32 *)(uintptr_t)J.src)[(u64)hvq_rk_stage_row(r0, rr, r, ny) * (nx >> 2) + hvq_rk_stage_dword(c0, k, nx)], c0, k, nx);
    }
#pragma unroll
    for (u32 u = 0; u < 5u; ++u) {
        const u32 idx = lane + HVQ_RK_LANES * u;
        if (idx < rows * HVQ_RK_ROW_DWORDS) raw[idx] = v[u];
    }
    __syncthreads();
}

__device__ __forceinline__ void store(const HvqRankJob &J, u32 c0, u32 r0, u32 v)
{
    const u32 lane = threadIdx.x, row = r0 + (lane >> 4), colx = c0 + (lane & 15u) * 4u;
    if (row < J.ny && colx < J.nx) *(GLB u32 *)(uintptr_t)(J.dst + (u64)row * J.nx + colx) = v;
}

/* the arrays: min steps alternate between P0 and P1, max steps between Q0 and Q1; the first step of either reads the staged rows */
#define ADVANCE() { smin = dmin; dmin = dmin == P0 ? P1 : P0; smax = dmax; dmax = dmax == Q0 ? Q1 : Q0; }

__device__ __forceinline__ void minmax_body(const HvqRankJob &J, u32 c0, u32 r0, u32 *buf)
{
    const u32 lane = threadIdx.x, rx = J.rx, ry = J.ry, op = J.op, rows = HVQ_RK_TH + 2u * ry;
    const int do_min = op != HVQ_RK_OP_MAX, do_max = op != HVQ_RK_OP_MIN;      /* uniform */
    u32 *const P0 = buf + HVQ_RK_BUF, *const P1 = buf + 2u * HVQ_RK_BUF, *const Q0 = buf + 3u * HVQ_RK_BUF, *const Q1 = buf + 4u * HVQ_RK_BUF;
    stage(J, c0, r0, ry, buf);
    const u32 *smin = buf, *smax = buf;
    u32 *dmin = P0, *dmax = Q0;
    u32 c;
    const u32 wx = 2u * rx + 1u, wy = 2u * ry + 1u;
    HVQ_RK_STEPS(wx, c) {
        hvq_rk_h_step(lane, rows, c, do_min, do_max, smin, dmin, smax, dmax);
        __syncthreads();
        ADVANCE()
    }
    hvq_rk_h_last(lane, rows, rx, wx - c, do_min, do_max, smin, dmin, smax, dmax);
    __syncthreads();
    ADVANCE()
    HVQ_RK_STEPS(wy, c) {
        hvq_rk_v_step(lane, rows, c, do_min, do_max, smin, dmin, smax, dmax);
        __syncthreads();
        ADVANCE()
    }
    store(J, c0, r0, hvq_rk_v_last(lane, wy - c, op, smin, smax));
}

__device__ __forceinline__ void median_body(const HvqRankJob &J, u32 c0, u32 r0, u32 *buf)
{
    const u32 lane = threadIdx.x;
    u32 *const S = buf + HVQ_RK_BUF;
    if (J.body == HVQ_RK_MED3) {                                       /* uniform */
        stage(J, c0, r0, 1u, buf);
        hvq_rk_med_sort3(lane, buf, S);
        __syncthreads();
        store(J, c0, r0, hvq_rk_med_select3(lane, S));
    } else {
        stage(J, c0, r0, 2u, buf);
        hvq_rk_med_sort5(lane, buf, S);
        __syncthreads();
        store(J, c0, r0, hvq_rk_med_select5(lane, S));
    }
}

__device__ __forceinline__ void copy_body(const HvqRankJob &J, u32 c0, u32 r0)
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

__global__ __launch_bounds__(HVQ_RK_LANES)
void hvq_rank_kernel(const HvqRankJob *__restrict__ jobs)
{
    const HvqRankJob *P = jobs + 3u * blockIdx.y;                      /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqRankJob &J = *P;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    __shared__ u32 buf[5u * HVQ_RK_BUF];
    if (J.body == HVQ_RK_COPY) copy_body(J, tx * HVQ_RK_CTW, ty * HVQ_RK_CTH);
    else if (J.body == HVQ_RK_MINMAX) minmax_body(J, tx * HVQ_RK_TW, ty * HVQ_RK_TH, buf);
    else median_body(J, tx * HVQ_RK_TW, ty * HVQ_RK_TH, buf);
}

/* jobs_dev: HvqRankJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535; max_tiles = max over the
 * pictures of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_rank(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_rank_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_RK_LANES), 0, stream, (const HvqRankJob *)jobs_dev);
    return hipGetLastError();
}
