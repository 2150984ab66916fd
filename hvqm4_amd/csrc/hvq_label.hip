/*
 * hvq_label.hip -- connected components for CDNA4 / gfx950 (MI355X): the foreground of one plane of resident pictures becomes a label map
 * and a table of records (hvq_label_pictures), and labels and records become a mask picture in slot layout again
 * (hvq_select_components).  include/hvqm4_amd.h specifies the values; hvq_label.h holds the code of the lanes, shared with the tests'
 * fake device, and says why every loop is bounded.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * hvq_label_pictures is seven launches behind one job table, grid row = picture in each.  The label map is the parent array (entry =
 * parent's raster index + 1, 0 background); there is no scratch memory besides the outputs.
 *   0  begin    a lane a picture zeroes row 0 of the records, where later lanes store their status.
 *   1  tile     a workgroup labels a 64 x 16 tile in 4 KiB of LDS: a lane loads a dword of the plane, its four entries start as the run
 *               inside the dword, join left and up (and the diagonals under 8-connectivity where the sample above is background) by LDS
 *               atomic-min unions -- not where left and above-left are foreground too: that union adds nothing --, and go out as the
 *               root's raster index + 1, sixteen bytes a lane.
 *   2  seam     a lane a sample on a tile's upper row or left column: unions across the seam on the global map, every access an
 *               agent-scope atomic.  A retry follows another lane's progress; no lane waits for another.
 *   3  flatten  the tile roots that a seam union linked (entries whose parent lies in another tile) walk to their root and point at
 *               it; a plane of one tile has no seams and skips 2 and 3.
 *   4  number   ONE workgroup a picture walks the map in raster order, 4096 entries a round: roots (entry == own index + 1) are counted
 *               per lane, scanned over the workgroup in LDS, and get their numbers, marked with bit 31; the records 1 .. stored are
 *               initialised, row 0 gets K, stored and F.  Ascending roots are ascending first samples.
 *   5  resolve  every entry walks to a marked entry and becomes that number, still marked (another lane's walk may pass through it);
 *               the records gather by 64-bit integer atomics, after the lanes of a wave that share a number have added up.
 *   6  finish   the mark leaves.
 * No private memory; no workgroup waits for another.
 *
 * hvq_select_kernel has the map kernel's shape (hvq_map.hip): a tile is HVQ_MP_TILE consecutive dwords of a plane; a Y dword reads
 * sixteen bytes of labels and the records of their numbers, U and V are filled with 128.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_map.h"
#include "hvq_label.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define HVQ_LB_SHARED 4u                                              /* numbers a wave adds up before its lanes flush alone */

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_begin_kernel(const HvqLabelJob *__restrict__ jobs, u32 n)
{
    const u32 i = blockIdx.x * HVQ_LB_LANES + threadIdx.x;
    if (i < n) hvq_lb_head_begin(jobs[i]);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_tile_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.y];
    const u32 tile = blockIdx.x, lane = threadIdx.x;
    if (tile >= J.tx * J.ty) return;                                  /* uniform */
    __shared__ u32 P[HVQ_LB_TILE];
    hvq_lb_tile_load(J, tile, lane, P);
    __syncthreads();
    u32 ok = hvq_lb_tile_merge(J, lane, P);
    __syncthreads();
    ok &= hvq_lb_tile_store(J, tile, lane, P);
    if (!ok) hvq_lb_head_status(J);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_seam_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.y];
    if (blockIdx.x * HVQ_LB_LANES >= J.seams) return;                 /* uniform */
    if (!hvq_lb_seam(J, blockIdx.x * HVQ_LB_LANES + threadIdx.x)) hvq_lb_head_status(J);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_flatten_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.chunks) return;                               /* uniform */
    if (!hvq_lb_flatten(J, blockIdx.x, threadIdx.x)) hvq_lb_head_status(J);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_number_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.x];
    const u32 lane = threadIdx.x, N = hvq_lb_samples(J), rounds = (N + HVQ_LB_SPAN - 1u) / HVQ_LB_SPAN;
    __shared__ u32 S[2][HVQ_LB_LANES];
    __shared__ u32 F;
    if (!lane) F = 0u;
    u32 base = 0u, fg = 0u;
    for (u32 r = 0; r < rounds; ++r) {
        const u32 mask = hvq_lb_number_count(J, r, lane, &fg), mine = (u32)__popc(mask);
        S[0][lane] = mine;
        __syncthreads();
        for (u32 k = 0; k < 8u; ++k) {                                /* inclusive scan by doubling: the result stands in S[0] */
            const u32 f = k & 1u, s = 1u << k;
            S[f ^ 1u][lane] = S[f][lane] + (lane >= s ? S[f][lane - s] : 0u);
            __syncthreads();
        }
        const u32 incl = S[0][lane], total = S[0][HVQ_LB_LANES - 1u];
        hvq_lb_number_store(J, r, lane, mask, base + incl - mine);
        base += total;
        __syncthreads();                                              /* S is written again */
    }
    atomicAdd(&F, fg);
    __syncthreads();
    if (!lane) hvq_lb_head_counts(J, base, F);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_resolve_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.chunks) return;                               /* uniform */
    const u64 K = ((const u64 *)(uintptr_t)J.comps)[0];
    const u32 stored = K < J.cap ? (u32)K : J.cap;
    HvqLbRec R;
    if (!hvq_lb_resolve(J, blockIdx.x, threadIdx.x, stored, &R)) hvq_lb_head_status(J);
    /* the lanes of a wave that hold a run mostly share a few numbers (a blob's interior, its neighbours): the lanes of one number add up
     * and one of them flushes, for up to HVQ_LB_SHARED numbers a wave; what is left after that flushes lane by lane */
    u64 have = __ballot(R.k != 0u);
    for (u32 round = 0; have && round < HVQ_LB_SHARED; ++round) {     /* wave-uniform */
        const u32 k0 = (u32)__shfl((int)R.k, (int)__ffsll((long long)have) - 1);
        const bool mine = R.k == k0;
        HvqLbRec A;
        hvq_lb_rec_none(&A);
        if (mine) A = R;
        for (int m = 1; m < 64; m <<= 1) {
            const u32 x0 = (u32)__shfl_xor((int)A.x0, m), y0 = (u32)__shfl_xor((int)A.y0, m);
            const u32 x1 = (u32)__shfl_xor((int)A.x1, m), y1 = (u32)__shfl_xor((int)A.y1, m);
            A.x0 = x0 < A.x0 ? x0 : A.x0; A.y0 = y0 < A.y0 ? y0 : A.y0;
            A.x1 = x1 > A.x1 ? x1 : A.x1; A.y1 = y1 > A.y1 ? y1 : A.y1;
            A.area += (u64)__shfl_xor((unsigned long long)A.area, m);
            A.sx += (u64)__shfl_xor((unsigned long long)A.sx, m);
            A.sy += (u64)__shfl_xor((unsigned long long)A.sy, m);
        }
        A.k = k0;
        if ((threadIdx.x & 63u) == (u32)__ffsll((long long)have) - 1u) hvq_lb_rec_flush(J, stored, &A);
        if (mine) R.k = 0u;
        have = __ballot(R.k != 0u);
    }
    hvq_lb_rec_flush(J, stored, &R);
}

__global__ __launch_bounds__(HVQ_LB_LANES)
void hvq_label_finish_kernel(const HvqLabelJob *__restrict__ jobs)
{
    const HvqLabelJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.chunks) return;                               /* uniform */
    hvq_lb_finish(J, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(HVQ_MP_LANES)
void hvq_select_kernel(const HvqSelectJob *__restrict__ jobs)
{
    const HvqSelectJob *P = jobs + 3u * blockIdx.y;                   /* the picture's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqSelectJob &J = *P;
    const u32 lane = threadIdx.x, n = J.dwords;
    u32 *out = (u32 *)(uintptr_t)J.dst;
    u32 stored = 0u;
    if (J.body == HVQ_SL_SELECT) {                                    /* uniform */
        const u64 s = ((const u64 *)(uintptr_t)J.comps)[1];
        stored = s < J.cap ? (u32)s : J.cap;
    }
#pragma unroll
    for (u32 u = 0; u < HVQ_MP_PER; ++u) {
        const u32 d = hvq_mp_dword(t, lane, u);
        if (d < n) out[d] = J.body == HVQ_SL_SELECT ? hvq_sl_dword(J, stored, d) : 0x80808080u;
    }
}

/* jobs_dev: HvqLabelJob[npics] in device memory, npics <= 65535; the maxima are over the pictures: of tx ty, of seams and of chunks */
extern "C" hipError_t hvq_launch_label(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_seams, uint32_t max_chunks,
                                       hipStream_t stream)
{
    if (npics <= 0 || !max_tiles || !max_chunks) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    const HvqLabelJob *jobs = (const HvqLabelJob *)jobs_dev;
    const u32 n = (u32)npics, seam_wgs = (max_seams + HVQ_LB_LANES - 1u) / HVQ_LB_LANES;
    hipLaunchKernelGGL(hvq_label_begin_kernel, dim3((n + HVQ_LB_LANES - 1u) / HVQ_LB_LANES), dim3(HVQ_LB_LANES), 0, stream, jobs, n);
    hipLaunchKernelGGL(hvq_label_tile_kernel, dim3(max_tiles, n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    if (seam_wgs) hipLaunchKernelGGL(hvq_label_seam_kernel, dim3(seam_wgs, n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    if (seam_wgs) hipLaunchKernelGGL(hvq_label_flatten_kernel, dim3(max_chunks, n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_label_number_kernel, dim3(n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_label_resolve_kernel, dim3(max_chunks, n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    hipLaunchKernelGGL(hvq_label_finish_kernel, dim3(max_chunks, n), dim3(HVQ_LB_LANES), 0, stream, jobs);
    return hipGetLastError();
}

/* jobs_dev: HvqSelectJob[3 * npics] in device memory, Y, U, V of a picture one behind the other, npics <= 65535 */
extern "C" hipError_t hvq_launch_select(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_select_kernel, dim3(max_tiles, (uint32_t)npics), dim3(HVQ_MP_LANES), 0, stream, (const HvqSelectJob *)jobs_dev);
    return hipGetLastError();
}
