/*
 * hvq_scale.hip -- the area filter for CDNA4 / gfx950 (MI355X): resident pictures resampled plane by plane into uint8 pictures of another
 * geometry in slot layout (hvq_scale_pictures, include/hvqm4_amd.h: the values, exact integers with one rounding).  One launch serves any
 * number of pictures of any sizes, ratios and samplings: grid row = picture (three HvqScaleJob, one per plane), grid column = one tile
 * of one of its planes, Y's first; workgroups past the picture's tiles leave.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * Two bodies, chosen per plane on the host (hvq_sc_body); the values do not depend on the choice.
 *   Tiled.   A tile is HVQ_SC_TW x HVQ_SC_TH targets.  Its source rows go through LDS, `chunk` rows at a time: (1) the four waves copy the
 *            rows' dwords, a wave eight rows, lanes side by side, the eight loads issued before the first is stored -- aligned dwords
 *            around the crop's bytes, which lie inside the picture (HvqScaleJob); (2) lane (column c,
 *            wave g) makes the horizontal sums of column c for the rows g, g + 4, ... of the chunk from the bytes in LDS -- once per
 *            source row and target column, 32 bits (at most 255 nx < 2^21) -- into a second LDS array; (3) the lane adds them, weighted,
 *            into the cells of its four target rows 4 g .. 4 g + 3 (32 bits when 255 nx ny < 2^32, otherwise 64: HVQ_SC_WIDE).  The row
 *            ranges of a wave are uniform: no divergence in the vertical pass.  At the end a cell is divided (hvq_sc_div: exact), the
 *            tile's bytes meet in LDS and every lane stores one dword.  LDS: 16 KiB + 8 KiB + 1 KiB.
 *   Direct.  A tile is HVQ_SC_DTW x HVQ_SC_DTH targets: a lane computes four adjacent samples in each of four rows from global memory and
 *            stores four dwords, a wave 256 adjacent bytes of a row at a time: at most 2 x 2 taps a sample when the host chooses it
 *            (identity, enlargement); any ratio when it is forced (tests).  Identity from a dword-aligned source copies dwords.
 * Every target byte is written once, by one store; nothing else is written.  No workgroup waits for another; the cells are named
 * registers (fully unrolled): no private memory.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_scale.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

static_assert(HVQ_SC_LANES == 256u && HVQ_SC_TW == 64u && HVQ_SC_TH == 16u, "the lane maps below: 64 columns x 4 waves, 4 rows a lane");

template <typename CELL>
__device__ __forceinline__ void tiled_body(const HvqScaleJob &J, u32 c0, u32 r0, u32 *raw, u32 *hs, u32 *outw)
{
    const u32 lane = threadIdx.x, cl = lane & 63u;
    const u32 g = __builtin_amdgcn_readfirstlane(lane >> 6);          /* the wave: what depends on it alone stays in scalar registers */
    const u32 nx = J.nx, ny = J.ny, mx = J.mx, my = J.my, rd = J.row_dwords, chunk = J.chunk;
    const u32 qx = J.mul_x, sx = J.shift_x, qy = J.mul_y, sy = J.shift_y;
    const u32 c = c0 + cl;
    /* the tile's source columns [X0, X1) and rows [Y0, Y1) */
    const u32 c_end = min(c0 + HVQ_SC_TW, mx), r_end = min(r0 + HVQ_SC_TH, my);
    const u32 X0 = hvq_sc_first(nx, mx, c0, qx, sx), X1 = hvq_sc_end(nx, mx, c_end - 1u, qx, sx);
    const u32 Y0 = hvq_sc_first(ny, my, r0, qy, sy), Y1 = hvq_sc_end(ny, my, r_end - 1u, qy, sy);
    const u64 row0 = J.src + X0;
    const u32 mis = (u32)row0 & 3u;                                   /* pitch is a multiple of 4: the same for every row */
    const u32 ndw = (mis + (X1 - X0) + 3u) >> 2;                      /* <= row_dwords (hvq_sc_job) */
    /* this lane's column: its taps [xs, xe), empty past the plane */
    const u32 xs = c < mx ? hvq_sc_first(nx, mx, c, qx, sx) : 0u, xe = c < mx ? hvq_sc_end(nx, mx, c, qx, sx) : 0u;
    const u32 xlo = nx * c, xhi = nx * (c + 1u);
    CELL cell[4] = { 0, 0, 0, 0 };
    for (u32 cy = Y0; cy < Y1; cy += chunk) {
        const u32 rows = min(chunk, Y1 - cy);
        __syncthreads();                                              /* the previous chunk's sums are added */
        for (u32 k = cl; k < ndw; k += 64u) {                          /* one round unless a row has more than 64 dwords */
            const GLB u32 *p = (const GLB u32 *)(uintptr_t)(row0 - mis + (u64)cy * J.pitch) + k;
            u32 v[8];
#pragma unroll
            for (u32 u = 0; u < 8u; ++u) v[u] = g + 4u * u < rows ? p[(u64)(g + 4u * u) * (J.pitch >> 2)] : 0u;
#pragma unroll
            for (u32 u = 0; u < 8u; ++u)
                if (g + 4u * u < rows) raw[(g + 4u * u) * rd + k] = v[u];
        }
        __syncthreads();
        const uint8_t *rawb = (const uint8_t *)raw;
        for (u32 rr = g; rr < rows; rr += 4u) {
            const uint8_t *b = rawb + (rr * rd * 4u + mis);           /* source column X0 of the row */
            u32 s = 0, at = mx * xs;
            for (u32 x = xs; x < xe; ++x, at += mx) s += (min(at + mx, xhi) - max(at, xlo)) * b[x - X0];
            hs[rr * 64u + cl] = s;
        }
        __syncthreads();
#pragma unroll
        for (u32 j = 0; j < 4u; ++j) {
            const u32 r = r0 + g * 4u + j;
            if (r < my) {                                             /* uniform within the wave */
                const u32 ys = max(hvq_sc_first(ny, my, r, qy, sy), cy), ye = min(hvq_sc_end(ny, my, r, qy, sy), cy + rows);
                const u32 ylo = ny * r, yhi = ny * (r + 1u);
                u32 at = my * ys;
                for (u32 y = ys; y < ye; ++y, at += my) cell[j] += (CELL)(min(at + my, yhi) - max(at, ylo)) * hs[(y - cy) * 64u + cl];
            }
        }
    }
    const u64 half = ((u64)nx * ny) >> 1;
    uint8_t *outb = (uint8_t *)outw;
#pragma unroll
    for (u32 j = 0; j < 4u; ++j) outb[(g * 4u + j) * 64u + cl] = (uint8_t)hvq_sc_div((u64)cell[j] + half, J.magic);
    __syncthreads();
    const u32 row = r0 + (lane >> 4), col = c0 + (lane & 15u) * 4u;
    if (row < my && col < mx) *(GLB u32 *)(uintptr_t)(J.dst + (u64)row * mx + col) = outw[lane];
}

template <typename CELL>
__device__ __forceinline__ void direct_body(const HvqScaleJob &J, u32 c0, u32 r0)
{
    const u32 lane = threadIdx.x;
    const u32 nx = J.nx, ny = J.ny, mx = J.mx, my = J.my;
    const u32 qx = J.mul_x, sx = J.shift_x, qy = J.mul_y, sy = J.shift_y;
    const u32 col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);    /* rows rb, rb + 4, rb + 8, rb + 12 */
    if (col >= mx) return;                                            /* mx is a multiple of 4: a dword lies inside the row or outside */
    GLB u32 *out = (GLB u32 *)(uintptr_t)(J.dst + col);
    if (nx == mx && ny == my && !(J.src & 3u)) {                       /* identity from an aligned source: the dwords as they stand (uniform) */
        const GLB u32 *in = (const GLB u32 *)(uintptr_t)(J.src + col);
        u32 v[4];
#pragma unroll
        for (u32 s = 0; s < 4u; ++s) v[s] = rb + 4u * s < my ? in[(u64)(rb + 4u * s) * (J.pitch >> 2)] : 0u;
#pragma unroll
        for (u32 s = 0; s < 4u; ++s)
            if (rb + 4u * s < my) out[(u64)(rb + 4u * s) * (mx >> 2)] = v[s];
        return;
    }
    const u64 half = ((u64)nx * ny) >> 1;
#pragma unroll
    for (u32 s = 0; s < 4u; ++s) {
        const u32 r = rb + 4u * s;
        if (r >= my) break;
        const u32 ys = hvq_sc_first(ny, my, r, qy, sy), ye = hvq_sc_end(ny, my, r, qy, sy), ylo = ny * r, yhi = ny * (r + 1u);
        u32 word = 0;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
            const u32 c = col + i;
            const u32 xs = hvq_sc_first(nx, mx, c, qx, sx), xe = hvq_sc_end(nx, mx, c, qx, sx), xlo = nx * c, xhi = nx * (c + 1u);
            CELL cell = 0;
            u32 aty = my * ys;
            for (u32 y = ys; y < ye; ++y, aty += my) {
                const GLB uint8_t *p = (const GLB uint8_t *)(uintptr_t)(J.src + (u64)y * J.pitch);
                u32 t = 0, at = mx * xs;
                for (u32 x = xs; x < xe; ++x, at += mx) t += (min(at + mx, xhi) - max(at, xlo)) * p[x];
                cell += (CELL)(min(aty + my, yhi) - max(aty, ylo)) * t;
            }
            word |= hvq_sc_div((u64)cell + half, J.magic) << (8u * i);
        }
        out[(u64)r * (mx >> 2)] = word;
    }
}

__global__ __launch_bounds__(HVQ_SC_LANES)
void hvq_scale_kernel(const HvqScaleJob *__restrict__ jobs)
{
    const HvqScaleJob *P = jobs + 3u * blockIdx.y;                     /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqScaleJob &J = *P;
    const u32 body = J.body;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    __shared__ u32 raw[HVQ_SC_RAW_DWORDS];
    __shared__ u32 hs[HVQ_SC_MAX_CHUNK * 64u];
    __shared__ u32 outw[HVQ_SC_LANES];
    if (body & HVQ_SC_TILED) {
        if (body & HVQ_SC_WIDE) tiled_body<u64>(J, tx * HVQ_SC_TW, ty * HVQ_SC_TH, raw, hs, outw);
        else tiled_body<u32>(J, tx * HVQ_SC_TW, ty * HVQ_SC_TH, raw, hs, outw);
    } else {
        if (body & HVQ_SC_WIDE) direct_body<u64>(J, tx * HVQ_SC_DTW, ty * HVQ_SC_DTH);
        else direct_body<u32>(J, tx * HVQ_SC_DTW, ty * HVQ_SC_DTH);
    }
}

/* jobs_dev: HvqScaleJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535; max_tiles = max over the
 * pictures of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_scale(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_scale_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_SC_LANES), 0, stream, (const HvqScaleJob *)jobs_dev);
    return hipGetLastError();
}
