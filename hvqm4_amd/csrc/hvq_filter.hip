/*
 * hvq_filter.hip -- separable integer filters for CDNA4 / gfx950 (MI355X): resident pictures filtered plane by plane into uint8 pictures
 * of the same geometry in slot layout (hvq_filter_pictures, include/hvqm4_amd.h: the values, exact integers with one rounding).  One
 * launch serves any number of pictures of any sizes, samplings and filters: grid row = picture (three HvqFilterJob, one per plane), grid
 * column = one tile of one of its planes, Y's first; workgroups past the picture's tiles leave.  The table of the planes' filters
 * (HvqFilterPlaneDev) lies behind the job table in the same upload.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * Two bodies, chosen per plane on the host (hvq_fl_job); the values do not depend on the choice.
 *   Filter.  A tile is HVQ_FL_TW x HVQ_FL_TH targets.  (1) Its 16 + 2 rmax source rows, row indices clamped into the plane, are staged
 *            into LDS as 24 aligned dwords each (the tile's 64 bytes and 16 of halo on either side; a dword outside the row is replaced
 *            by one inside and never looked at), a lane up to five dwords, all loads issued before the first is stored.  (2) Per
 *            term, lane (column c, wave g) makes the horizontal sums of column c for the staged rows g, g + 4, ... from the bytes in
 *            LDS, column indices clamped into the plane: tap by tap, the tap in a scalar register, six or twelve rows' sums in named
 *            registers, their reads in flight together; 32 bits, into an LDS array of the term's own.  (3) The lane walks the 4 + 2 ry
 *            rows under its four target rows 4 g .. 4 g + 3 once, four a step, and adds each, weighted, to the targets it has a share
 *            in.  Then combine, shift, bias, clamp; the tile's bytes meet in LDS and every lane stores one dword.  LDS: 4.3 KiB + 2 x
 *            11.5 KiB + 1 KiB.
 *   Copy.    A plane whose filter is the identity ("luma only" leaves two of three planes as they are): a tile is HVQ_FL_CTW x
 *            HVQ_FL_CTH samples, a lane moves a dword in each of four rows, a wave 256 adjacent bytes of a row at a time.
 * The taps are uniform over the workgroup: lane l loads tap l & 31 of each array once, beside the staging loads, and a loop reads tap i
 * from that register into a scalar one (v_readlane); no tap array in private memory, no memory access per tap.  Zero taps are skipped
 * in the horizontal pass.  Every target byte is written once, by one store; nothing else is written.  No workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_filter.h"

typedef uint32_t u32;
typedef int32_t i32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

static_assert(HVQ_FL_LANES == 256u && HVQ_FL_TW == 64u && HVQ_FL_TH == 16u && HVQ_FL_MAX_ROWS <= 48u, "the lane maps below: 64 columns x 4 waves, 4 target rows and 12 staged rows a lane");

/* one term: the horizontal sums of the staged rows into hs, then the vertical pass into the lane's four cells.  U: the staged rows a
 * wave makes the sums of, 6 (up to 24 staged rows: rmax <= 4) or 12.  vwx / vwy: lane l holds tap l & 31 of the term; a tap reaches the
 * scalar unit by v_readlane with a uniform index, without a trip to memory inside the loops.  The LDS reads of a step do not depend on a
 * condition, so that they are all in flight together: a row past the staged ones is replaced by the last one, and its sum is not stored
 * (horizontal) or meets a weight of 0 (vertical). */
template <u32 U>
__device__ __forceinline__ void term_pass(const HvqFilterTermDev *__restrict__ T, i32 vwx, i32 vwy, u32 c0, u32 nx, u32 rows, u32 rmax, u32 g, u32 cl,
                                          const uint8_t *rawb, i32 *hs, i32 (&cell)[4])
{
    const u32 rx = (u32)T->rx, ry = (u32)T->ry;
    i32 acc[U];
    u32 rowb[U];                                                      /* uniform: the byte offsets of the wave's staged rows */
#pragma unroll
    for (u32 u = 0; u < U; ++u) { acc[u] = 0; rowb[u] = min(g + 4u * u, rows - 1u) * (HVQ_FL_ROW_DWORDS * 4u); }
    for (u32 i = 0; i <= 2u * rx; ++i) {
        const i32 w = __builtin_amdgcn_readlane(vwx, (int)i);
        if (!w) continue;
        const uint8_t *b = rawb + hvq_fl_tap_byte(c0, c0 + cl, i, rx, nx);
#pragma unroll
        for (u32 u = 0; u < U; ++u) acc[u] += w * (i32)b[rowb[u]];
    }
#pragma unroll
    for (u32 u = 0; u < U; ++u)
        if (g + 4u * u < rows) hs[(g + 4u * u) * 64u + cl] = acc[u];   /* uniform within the wave */
    __syncthreads();
    /* target row 4 g + j, tap k meets staged row 4 g + j + k + (rmax - ry): the rows 4 g + (rmax - ry) + m, m = j + k < 4 + 2 ry, four a step */
    const i32 *col = hs + (4u * g + rmax - ry) * 64u + cl;
    const u32 last = 3u + 2u * ry;
    for (u32 m0 = 0; m0 <= last; m0 += 4u) {
        i32 h[4];
#pragma unroll
        for (u32 q = 0; q < 4u; ++q) h[q] = col[min(m0 + q, last) * 64u];
#pragma unroll
        for (u32 q = 0; q < 4u; ++q)
#pragma unroll
            for (u32 j = 0; j < 4u; ++j) {
                const u32 k = m0 + q - j;                             /* uniform; beyond 2 ry (or wrapped below 0): no share */
                const i32 w = __builtin_amdgcn_readlane(vwy, (int)(k & 31u));
                cell[j] += (k <= 2u * ry ? w : 0) * h[q];
            }
    }
}

__device__ __forceinline__ void filter_body(const HvqFilterJob &J, const HvqFilterPlaneDev *__restrict__ F, u32 c0, u32 r0, u32 *raw, i32 *hs0, i32 *hs1, u32 *outw)
{
    const u32 lane = threadIdx.x, cl = lane & 63u;
    const u32 g = __builtin_amdgcn_readfirstlane(lane >> 6);          /* the wave: what depends on it alone stays in scalar registers */
    const u32 nx = J.nx, ny = J.ny;
    const u32 rmax = (u32)F->rmax, rows = HVQ_FL_TH + 2u * rmax;
    const bool two = F->terms == 2;                                   /* uniform */
    /* the taps, one a lane, requested before the rows: term[1] of a filter of one term is zeros in the table */
    const i32 vwx0 = F->term[0].wx[cl & 31u], vwy0 = F->term[0].wy[cl & 31u], vwx1 = F->term[1].wx[cl & 31u], vwy1 = F->term[1].wy[cl & 31u];
    /* (1) stage: dword idx of the tile's rows, idx = staged row * 24 + k */
    {
        u32 v[5];
#pragma unroll
        for (u32 u = 0; u < 5u; ++u) {
            const u32 idx = lane + HVQ_FL_LANES * u, rr = idx / HVQ_FL_ROW_DWORDS, k = idx - rr * HVQ_FL_ROW_DWORDS;
            v[u] = 0;
            if (rr < rows) v[u] = ((const GLB u32 *)(uintptr_t)J.src)[(u64)hvq_fl_stage_row(r0, rr, rmax, ny) * (nx >> 2) + hvq_fl_stage_dword(c0, k, nx)];
        }
#pragma unroll
        for (u32 u = 0; u < 5u; ++u) {
            const u32 idx = lane + HVQ_FL_LANES * u;
            if (idx < rows * HVQ_FL_ROW_DWORDS) raw[idx] = v[u];
        }
    }
    __syncthreads();
    i32 t0[4] = { 0, 0, 0, 0 }, t1[4] = { 0, 0, 0, 0 };
    if (rows <= 24u) {                                                /* uniform */
        term_pass<6>(&F->term[0], vwx0, vwy0, c0, nx, rows, rmax, g, cl, (const uint8_t *)raw, hs0, t0);
        if (two) term_pass<6>(&F->term[1], vwx1, vwy1, c0, nx, rows, rmax, g, cl, (const uint8_t *)raw, hs1, t1);   /* its own array: no barrier in between */
    } else {
        term_pass<12>(&F->term[0], vwx0, vwy0, c0, nx, rows, rmax, g, cl, (const uint8_t *)raw, hs0, t0);
        if (two) term_pass<12>(&F->term[1], vwx1, vwy1, c0, nx, rows, rmax, g, cl, (const uint8_t *)raw, hs1, t1);
    }
    const i32 combine = F->combine, half = F->half, shift = F->shift, bias = F->bias;
    uint8_t *outb = (uint8_t *)outw;
#pragma unroll
    for (u32 j = 0; j < 4u; ++j) outb[(g * 4u + j) * 64u + cl] = (uint8_t)hvq_fl_finish(t0[j], t1[j], combine, half, shift, bias);
    __syncthreads();
    const u32 row = r0 + (lane >> 4), colx = c0 + (lane & 15u) * 4u;
    if (row < ny && colx < nx) *(GLB u32 *)(uintptr_t)(J.dst + (u64)row * nx + colx) = outw[lane];
}

__device__ __forceinline__ void copy_body(const HvqFilterJob &J, u32 c0, u32 r0)
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

__global__ __launch_bounds__(HVQ_FL_LANES)
void hvq_filter_kernel(const HvqFilterJob *__restrict__ jobs, const HvqFilterPlaneDev *__restrict__ filters)
{
    const HvqFilterJob *P = jobs + 3u * blockIdx.y;                    /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqFilterJob &J = *P;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    __shared__ u32 raw[HVQ_FL_MAX_ROWS * HVQ_FL_ROW_DWORDS];
    __shared__ i32 hs0[HVQ_FL_MAX_ROWS * 64u];
    __shared__ i32 hs1[HVQ_FL_MAX_ROWS * 64u];
    __shared__ u32 outw[HVQ_FL_LANES];
    if (J.body == HVQ_FL_COPY) copy_body(J, tx * HVQ_FL_CTW, ty * HVQ_FL_CTH);
    else filter_body(J, filters + J.pf, tx * HVQ_FL_TW, ty * HVQ_FL_TH, raw, hs0, hs1, outw);
}

/* jobs_dev: HvqFilterJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535, and behind them the
 * HvqFilterPlaneDev the jobs name; max_tiles = max over the pictures of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_filter(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqFilterJob *jobs = (const HvqFilterJob *)jobs_dev;
    hipLaunchKernelGGL(hvq_filter_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_FL_LANES), 0, stream, jobs, (const HvqFilterPlaneDev *)(jobs + 3u * (size_t)npics));
    return hipGetLastError();
}
