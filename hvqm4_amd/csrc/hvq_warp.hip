/*
 * hvq_warp.hip -- affine warps for CDNA4 / gfx950 (MI355X): resident pictures moved plane by plane through a per-picture affine map
 * from target to source, bilinear taps in exact integers with one rounding, into uint8 pictures of a target geometry in slot layout
 * (hvq_warp_pictures, include/hvqm4_amd.h: the values).  One launch serves any number of pictures of any sizes, samplings and maps:
 * grid row = picture (three HvqWarpJob, one per plane), grid column = one tile of one of its planes, Y's first; workgroups past the
 * picture's tiles leave.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * A tile is HVQ_WP_TW x HVQ_WP_TH targets; lane (column c, wave g) computes the targets (c, 4 g .. 4 g + 3).  NU and NV of the tile's
 * first target are 64-bit and uniform (scalar registers); a lane adds its 32-bit delta, shifts and saturates (hvq_wp_u8), and works
 * in 32 bits from there.  Two bodies, chosen per plane on the host (hvq_wp_choose); the values do not depend on the choice.
 *   Direct.  The lane loads its four taps as bytes from global memory, the indices clamped into the plane: always inside it.
 *   Tiled.   The workgroup computes the source bounding box of its tile from the tile's four corners (hvq_wp_box), clamped into the
 *            plane, and stages it into LDS as aligned dwords, `pitch` (odd) dwords a row, four loads a lane in flight at a time; the
 *            taps are LDS byte reads.  Under a quarter turn a wave's 64 targets lie in 64 source rows: 64 cache lines a direct load,
 *            but 16 x 64 staged bytes that every row of the tile shares.
 * Under HVQ_WARP_CONSTANT a tap whose index the clamp moved is replaced by the fill.  The tile's bytes meet in LDS and every lane
 * stores one dword.  Every target byte is written once, by one store; nothing else is written.  No workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_warp.h"

typedef uint32_t u32;
typedef int32_t i32;
typedef uint64_t u64;
typedef int64_t i64;
#define GLB __attribute__((address_space(1)))

static_assert(HVQ_WP_LANES == 256u && HVQ_WP_TW == 64u && HVQ_WP_TH == 16u, "the lane maps below: 64 columns x 4 waves, 4 target rows a lane");

template <bool TILED>
__device__ __forceinline__ void warp_body(const HvqWarpJob &J, u32 c0, u32 r0, u32 *raw, u32 *outw)
{
    const u32 lane = threadIdx.x, cl = lane & 63u;
    const u32 g = __builtin_amdgcn_readfirstlane(lane >> 6);          /* the wave: what depends on it alone stays in scalar registers */
    const u32 nx = J.nx, ny = J.ny, su = J.su, sv = J.sv;
    const bool constant = J.border != 0u;                             /* uniform */
    const u32 fill = J.fill;
    HvqWarpBox B = { 0, 0, 0, 0 };
    const u32 pitch = J.pitch;
    if (TILED) {
        B = hvq_wp_box(&J, c0, r0);                                   /* uniform */
        const u32 bw = (u32)(B.x1 >> 2) - (u32)(B.x0 >> 2) + 1u, bh = (u32)(B.y1 - B.y0) + 1u, mul = J.pitch_mul;
        const u32 total = bh * pitch;                                 /* <= J.rows * pitch <= HVQ_WP_LDS_DWORDS */
        const GLB u32 *in = (const GLB u32 *)(uintptr_t)J.src + (u64)(u32)B.y0 * (nx >> 2) + (u32)(B.x0 >> 2);
        for (u32 base = 0; base < total; base += 4u * HVQ_WP_LANES) {
            u32 v[4];
#pragma unroll
            for (u32 u = 0; u < 4u; ++u) {
                const u32 idx = base + lane + HVQ_WP_LANES * u, rr = hvq_wp_stage_row(idx, mul), k = idx - rr * pitch;
                v[u] = 0;
                if (idx < total && k < bw) v[u] = in[(u64)rr * (nx >> 2) + k];
            }
#pragma unroll
            for (u32 u = 0; u < 4u; ++u) {
                const u32 idx = base + lane + HVQ_WP_LANES * u;
                if (idx < total && idx < HVQ_WP_LDS_DWORDS) raw[idx] = v[u];
            }
        }
        __syncthreads();
    }
    /* the lane's column: NU, NV of (c0 + cl, r0 + 4 g) as the tile's origin plus a 32-bit delta; the next row is bu, bv further */
    const i64 ou = J.cu + (i64)J.au * c0 + (i64)J.bu * r0, ov = J.cv + (i64)J.av * c0 + (i64)J.bv * r0;
    i32 du = J.au * (i32)cl + J.bu * (i32)(4u * g), dv = J.av * (i32)cl + J.bv * (i32)(4u * g);
    const uint8_t *rawb = (const uint8_t *)raw;
    const GLB uint8_t *srcb = (const GLB uint8_t *)(uintptr_t)J.src;
    uint8_t *outb = (uint8_t *)outw;
#pragma unroll
    for (u32 j = 0; j < 4u; ++j, du += J.bu, dv += J.bv) {
        const i32 u8 = hvq_wp_u8(ou + du, su, nx), v8 = hvq_wp_u8(ov + dv, sv, ny);
        const i32 ix = u8 >> 8, iy = v8 >> 8;
        const u32 fx = (u32)u8 & 255u, fy = (u32)v8 & 255u;
        const i32 x0 = hvq_wp_clamp(ix, nx), x1 = hvq_wp_clamp(ix + 1, nx), y0 = hvq_wp_clamp(iy, ny), y1 = hvq_wp_clamp(iy + 1, ny);
        u32 t00, t01, t10, t11;
        if (TILED) {
            const u32 a0 = hvq_wp_lds_byte(&B, pitch, x0, y0), a1 = hvq_wp_lds_byte(&B, pitch, x0, y1), dx = (u32)(x1 - x0);
            t00 = rawb[a0]; t01 = rawb[a0 + dx]; t10 = rawb[a1]; t11 = rawb[a1 + dx];
        } else {
            const GLB uint8_t *p0 = srcb + (u64)(u32)y0 * nx, *p1 = srcb + (u64)(u32)y1 * nx;
            t00 = p0[x0]; t01 = p0[x1]; t10 = p1[x0]; t11 = p1[x1];
        }
        if (constant) {
            const bool ox0 = x0 != ix, ox1 = x1 != ix + 1, oy0 = y0 != iy, oy1 = y1 != iy + 1;
            t00 = ox0 || oy0 ? fill : t00; t01 = ox1 || oy0 ? fill : t01;
            t10 = ox0 || oy1 ? fill : t10; t11 = ox1 || oy1 ? fill : t11;
        }
        outb[(g * 4u + j) * 64u + cl] = (uint8_t)hvq_wp_finish(fx, fy, t00, t01, t10, t11);
    }
    __syncthreads();
    const u32 row = r0 + (lane >> 4), colx = c0 + (lane & 15u) * 4u;
    if (row < J.my && colx < J.mx) *(GLB u32 *)(uintptr_t)(J.dst + (u64)row * J.mx + colx) = outw[lane];
}

__global__ __launch_bounds__(HVQ_WP_LANES)
void hvq_warp_kernel(const HvqWarpJob *__restrict__ jobs)
{
    const HvqWarpJob *P = jobs + 3u * blockIdx.y;                     /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqWarpJob &J = *P;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    __shared__ u32 raw[HVQ_WP_LDS_DWORDS];
    __shared__ u32 outw[HVQ_WP_LANES];
    if (J.body == HVQ_WP_TILED) warp_body<true>(J, tx * HVQ_WP_TW, ty * HVQ_WP_TH, raw, outw);
    else warp_body<false>(J, tx * HVQ_WP_TW, ty * HVQ_WP_TH, raw, outw);
}

/* jobs_dev: HvqWarpJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535; max_tiles = max over
 * the pictures of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_warp(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_warp_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_WP_LANES), 0, stream, (const HvqWarpJob *)jobs_dev);
    return hipGetLastError();
}
