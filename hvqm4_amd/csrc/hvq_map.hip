/*
 * hvq_map.hip -- point operations for CDNA4 / gfx950 (MI355X): resident pictures through lookup tables, out = table[in], plane by plane,
 * into uint8 pictures of the same geometry in slot layout (hvq_map_pictures), and the tables themselves from histogram records where
 * they lie (hvq_histogram_tables).  include/hvqm4_amd.h specifies the values of both; nothing is rounded in the first, the second is
 * exact integer arithmetic.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * hvq_map_kernel.  One launch serves any number of pictures of any sizes and samplings: grid row = picture (three HvqMapJob, one per
 * plane), grid column = one tile of one of its planes, Y's first; workgroups past the picture's tiles leave.  A tile is HVQ_MP_TILE
 * consecutive dwords of the plane (a point operation does not look at rows), a lane takes HVQ_MP_PER of them, HVQ_MP_LANES apart; all
 * loads are issued before the first lookup.  Lookup body: lane l stages byte l of the plane's table into LDS, one barrier, then four LDS
 * byte reads a dword (hvq_mp_lookup4 of hvq_map.h, shared with the tests' fake device).  Copy body (a plane whose bit of `planes` is
 * clear): the same tile without table and barrier.  LDS: 256 bytes (HVQ_MP_WIDE: 1 KiB).  A lane reads only the dwords that it later
 * writes, so dst may be src.  No private memory, no scratch buffer; every target byte is written once, by one store.  No workgroup waits
 * for another.
 *
 * hvq_tables_kernel.  Grid row = record, grid column = plane; lane v holds bin v.  The phases are hvq_map.h's (hvq_tb_*): an inclusive
 * scan of the counts and of v h[v] in eight steps, the values single lanes know, Otsu's arg-max tree over 192-bit comparisons, and the
 * entry of every lane, stored as a byte.  LDS: one HvqTbLds, 13 KiB.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_map.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

__global__ __launch_bounds__(HVQ_MP_LANES)
void hvq_map_kernel(const HvqMapJob *__restrict__ jobs)
{
    const HvqMapJob *P = jobs + 3u * blockIdx.y;                      /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqMapJob &J = *P;
    const u32 lane = threadIdx.x, n = J.dwords;
    const GLB u32 *in = (const GLB u32 *)(uintptr_t)J.src;
    GLB u32 *out = (GLB u32 *)(uintptr_t)J.dst;
    __shared__ HvqMpEntry T[256];
    u32 v[HVQ_MP_PER];
#pragma unroll
    for (u32 u = 0; u < HVQ_MP_PER; ++u) {
        const u32 d = hvq_mp_dword(t, lane, u);
        v[u] = d < n ? in[d] : 0u;
    }
    if (J.body == HVQ_MP_LOOKUP) {                                    /* uniform */
        T[lane] = ((const GLB uint8_t *)(uintptr_t)J.table)[lane];
        __syncthreads();
#pragma unroll
        for (u32 u = 0; u < HVQ_MP_PER; ++u) v[u] = hvq_mp_lookup4(T, v[u]);
    }
#pragma unroll
    for (u32 u = 0; u < HVQ_MP_PER; ++u) {
        const u32 d = hvq_mp_dword(t, lane, u);
        if (d < n) out[d] = v[u];
    }
}

__global__ __launch_bounds__(HVQ_TB_LANES)
void hvq_tables_kernel(const HvqTableJob *__restrict__ jobs)
{
    const HvqTableJob &J = jobs[blockIdx.y];
    const u32 lane = threadIdx.x, p = blockIdx.x;
    const u32 kind = J.rule[p ? 1 : 0].kind, a = J.rule[p ? 1 : 0].a, b = J.rule[p ? 1 : 0].b;     /* uniform */
    GLB uint8_t *out = (GLB uint8_t *)(uintptr_t)(J.out + 256u * p);
    __shared__ HvqTbLds L;
    if (kind >= HVQ_TB_EQUALIZE) {
        hvq_tb_load(&L, lane, ((const GLB u32 *)(uintptr_t)J.hist)[256u * p + lane]);
        __syncthreads();
        for (u32 k = 0; k < 8u; ++k) {
            hvq_tb_scan(&L, lane, k);
            __syncthreads();
        }
        hvq_tb_select(&L, lane, kind, a, b);
        __syncthreads();
        if (kind == HVQ_TB_OTSU)
            for (u32 s = 128u; s; s >>= 1) {
                hvq_tb_reduce(&L, lane, s);
                __syncthreads();
            }
    }
    out[lane] = hvq_tb_value(&L, lane, kind, a);
}

/* jobs_dev: HvqMapJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535; max_tiles = max over the
 * pictures of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_map(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_map_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_MP_LANES), 0, stream, (const HvqMapJob *)jobs_dev);
    return hipGetLastError();
}

/* jobs_dev: HvqTableJob[nrecords] in device memory, nrecords <= 65535 */
extern "C" hipError_t hvq_launch_tables(const void *jobs_dev, int nrecords, hipStream_t stream)
{
    if (nrecords <= 0) return hipSuccess;
    if (nrecords > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_tables_kernel, dim3(3u, (uint32_t)nrecords), dim3(HVQ_TB_LANES), 0, stream, (const HvqTableJob *)jobs_dev);
    return hipGetLastError();
}
