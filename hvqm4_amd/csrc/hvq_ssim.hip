/*
 * hvq_ssim.hip -- windowed SSIM for CDNA4 / gfx950 (MI355X): per plane the exact sum of the fixed-point window values and the number of
 * windows of a resident picture `a` against a reference `b` (another resident picture or the caller's device memory), and on request
 * the map of window values (hvq_picture_ssim, include/hvqm4_amd.h: the specification).  One launch serves any number of pairs of any
 * sizes and samplings: grid row = pair.
 *
 * A unit of its own (its own Makefile rule, the plain flags of hvq_metrics.o): the code of the other kernels does not change with it.
 *
 * Shape.  A workgroup of HVQ_SS_LANES lanes takes one tile of at most HVQ_SS_TR x HVQ_SS_TC windows of ONE plane (the job record says
 * which workgroup starts which plane): (HVQ_SS_TR + 1) x (HVQ_SS_TC + 1) = 16 x 64 blocks of 4 x 4 samples, the last block row and
 * column shared with the neighbouring tiles (the halo: 8 % more block work, most of it L2 hits).  Lanes run linearly over the tile's
 * blocks, whatever its width: a lane loads the 4 + 4 dwords of a block (one dword per block row and picture: a plane's rows are only
 * 4-byte aligned in general), forms s1 | s2 (packed), ss and s12 with v_sad_u8 and v_dot4_u32_u8 and puts them into LDS, 12 bytes per
 * block.  After ONE barrier lanes run linearly over the tile's windows: the four neighbouring blocks are added, A, B, C, D formed in
 * 32-bit integers, q in float32 (one rounding per operation, the correctly rounded division), f = rint(q * 2^24).  q goes to the map
 * when the pair has one.  f and the number of windows evaluated are lane partials, summed across the wave by shuffles, across the four
 * waves through LDS, and leave as ONE 64-bit no-return atomic add per value and workgroup, device scope, into the record (zeroed by
 * the memset queued in front of the launch).  Integer addition: the record does not depend on the order of arrival.  Loads are issued
 * only for blocks inside the plane: nothing outside a plane is read.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"

#pragma clang fp contract(off)

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_store / global_atomic, never flat (hvq_kernels.hip) */

#define SS_BR (HVQ_SS_TR + 1u)                          /* block rows of a tile */
#define SS_BC (HVQ_SS_TC + 1u)                          /* block columns of a tile */
#define SS_BLOCKS (SS_BR * SS_BC)
#define SS_PER_LANE ((SS_BLOCKS + HVQ_SS_LANES - 1u) / HVQ_SS_LANES)      /* blocks, and at most windows, of a lane */

static_assert(HVQ_SS_LANES == 256u && HVQ_SS_LANES % 64u == 0, "four waves: the LDS stage below");
static_assert(SS_BLOCKS * 12u <= 16384u, "the tile's block integers fit 16 KiB of LDS");
/* the linear index -> (row, column) split below multiplies by floor(65536 / width) + 1: exact while index * width < 65536 */
static_assert((SS_BLOCKS - 1u) * SS_BC < 65536u, "the reciprocal split of a block or window index must be exact");

/* Widths (include/hvqm4_amd.h).  A block has 16 samples of each picture, a window 64:
 *   block s1, s2 <= 16 * 255 = 4080 and window s1, s2 <= 16320: 16 bits each, so s1 | s2 << 16 adds without a carry between the halves;
 *   window ss <= 2 * 64 * 255^2 = 8 323 200, s12 <= 4 161 600; 64 ss, s1 s2, s1^2 + s2^2 and everything built from them stay below 2^30. */
static_assert(64u * 255u <= 0xFFFFu, "a window's s1 and s2 must fit the 16-bit halves they are packed into");
static_assert((u64)64 * 2u * 64u * 255u * 255u < ((u64)1 << 30), "64 ss must fit a signed 32-bit integer with room for the constants");
static_assert((u64)2 * (64u * 255u) * (64u * 255u) + 416u < ((u64)1 << 30), "A = 2 s1 s2 + 416 and C = s1^2 + s2^2 + 416 must fit 32 bits");
static_assert((u64)2 * 64u * 64u * 255u * 255u + 235963u < ((u64)1 << 30), "|B| = |2 covar + 235963| and D = vars + 235963 must fit 32 bits");
/* |q| <= 1 up to its roundings: f <= 2^24 + 2, and a lane adds at most SS_PER_LANE of them in 32 bits */
static_assert((u64)SS_PER_LANE * ((1u << 24) + 2u) < ((u64)1 << 31), "a lane's sum of f must fit a signed 32-bit integer");

__device__ __forceinline__ i64 wave_sum(i64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(HVQ_SS_LANES)
void hvq_ssim_kernel(const HvqSsimJob *__restrict__ jobs)
{
    const HvqSsimJob &J = jobs[blockIdx.y];
    const u32 wg = blockIdx.x;
    if (wg >= J.wg_first[3]) return;                                   /* past this pair: leave (uniform) */
    const u32 p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);       /* the workgroup's plane */
    const u32 tile = wg - J.wg_first[p];
    const u32 ty = tile / J.tiles_x[p], tx = tile - ty * J.tiles_x[p];
    const u32 bw = J.bw[p], bh = J.bh[p];
    const u32 r0 = ty * HVQ_SS_TR, c0 = tx * HVQ_SS_TC;                /* the tile's first block = its first window */
    const u32 tbw = min(SS_BC, bw - c0), tbh = min(SS_BR, bh - r0);    /* blocks of the tile: all inside the plane */
    const u32 twc = tbw - 1u, twr = tbh - 1u;                          /* windows of the tile: at least 1 x 1 */
    const u32 nblk = tbw * tbh, nwin = twc * twr;
    const u32 t = threadIdx.x;

    __shared__ u32 l_sp[SS_BLOCKS], l_ss[SS_BLOCKS], l_s12[SS_BLOCKS];
    __shared__ i64 part[HVQ_SS_LANES / 64u][2];

    /* ---- blocks: lane t takes blocks t, t + 256, ... of the tile in row-major order; all loads first */
    {
        const u32 pitch = bw * 4u;                                     /* bytes of a plane's row */
        const u32 base = J.plane_off[p] + r0 * 4u * pitch + c0 * 4u;
        const GLB uint8_t *pa = (const GLB uint8_t *)(uintptr_t)J.a + base;
        const GLB uint8_t *pb = (const GLB uint8_t *)(uintptr_t)J.b + base;
        const u32 recip = 65536u / tbw + 1u;
        u32 va[SS_PER_LANE][4], vb[SS_PER_LANE][4];
#pragma unroll
        for (u32 k = 0; k < SS_PER_LANE; ++k) {
            const u32 i = t + k * HVQ_SS_LANES;
            const u32 r = (i * recip) >> 16, c = i - r * tbw;
            const u32 off = r * 4u * pitch + c * 4u;
#pragma unroll
            for (u32 y = 0; y < 4; ++y) {
                /* a block past the tile's end contributes nothing; the load itself is predicated: nothing outside the plane is read */
                va[k][y] = i < nblk ? *(const GLB u32 *)(pa + off + y * pitch) : 0u;
                vb[k][y] = i < nblk ? *(const GLB u32 *)(pb + off + y * pitch) : 0u;
            }
        }
#pragma unroll
        for (u32 k = 0; k < SS_PER_LANE; ++k) {
            const u32 i = t + k * HVQ_SS_LANES;
            u32 s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
            for (u32 y = 0; y < 4; ++y) {
                const u32 x = va[k][y], z = vb[k][y];
                s1 = __builtin_amdgcn_sad_u8(x, 0u, s1);
                s2 = __builtin_amdgcn_sad_u8(z, 0u, s2);
                ss = __builtin_amdgcn_udot4(x, x, ss, false);
                ss = __builtin_amdgcn_udot4(z, z, ss, false);
                s12 = __builtin_amdgcn_udot4(x, z, s12, false);
            }
            if (i < nblk) { l_sp[i] = s1 | (s2 << 16); l_ss[i] = ss; l_s12[i] = s12; }
        }
    }
    __syncthreads();

    /* ---- windows: lane t takes windows t, t + 256, ... of the tile in row-major order */
    int sum_f = 0;
    u32 count = 0;
    {
        const u32 cols = bw - 1u;                                      /* window columns of the plane: the map's row length */
        GLB float *map = J.map ? (GLB float *)(uintptr_t)J.map + J.map_off[p] + (size_t)r0 * cols + c0 : nullptr;
        const u32 recip = 65536u / twc + 1u;
#pragma unroll
        for (u32 k = 0; k < SS_PER_LANE; ++k) {
            const u32 j = t + k * HVQ_SS_LANES;
            if (j < nwin) {
                const u32 r = (j * recip) >> 16, c = j - r * twc;
                const u32 i = r * tbw + c;
                const u32 sp = l_sp[i] + l_sp[i + 1u] + l_sp[i + tbw] + l_sp[i + tbw + 1u];
                const int ss = (int)(l_ss[i] + l_ss[i + 1u] + l_ss[i + tbw] + l_ss[i + tbw + 1u]);
                const int s12 = (int)(l_s12[i] + l_s12[i + 1u] + l_s12[i + tbw] + l_s12[i + tbw + 1u]);
                const int s1 = (int)(sp & 0xFFFFu), s2 = (int)(sp >> 16);
                const int sq = s1 * s1 + s2 * s2, cr = s1 * s2;
                const int vars = 64 * ss - sq, covar = 64 * s12 - cr;
                const int A = 2 * cr + 416, B = 2 * covar + 235963, C = sq + 416, D = vars + 235963;
                const float num = (float)A * (float)B, den = (float)C * (float)D;
                const float q = num / den;
                if (map) map[(size_t)r * cols + c] = q;
                sum_f += __float2int_rn(q * 16777216.0f);
                count += 1u;
            }
        }
    }

    const i64 w0 = wave_sum((i64)sum_f), w1 = wave_sum((i64)count);
    if ((t & 63u) == 0) { part[t >> 6][0] = w0; part[t >> 6][1] = w1; }
    __syncthreads();
    if (t < 2u) {
        i64 v = 0;
#pragma unroll
        for (u32 w = 0; w < HVQ_SS_LANES / 64u; ++w) v += part[w][t];
        GLB u64 *out = (GLB u64 *)(uintptr_t)J.out + p * 2u + t;
        (void)__hip_atomic_fetch_add(out, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* jobs_dev: HvqSsimJob[njobs] in device memory; max_wgs = max over jobs of wg_first[3].  The records the jobs point to are zero when
 * the launch runs (the caller queues the memset in front of it on the same stream). */
extern "C" hipError_t hvq_launch_ssim(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0 || !max_wgs) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_ssim_kernel, dim3(max_wgs, (uint32_t)njobs), dim3(HVQ_SS_LANES), 0, stream, (const HvqSsimJob *)jobs_dev);
    return hipGetLastError();
}
