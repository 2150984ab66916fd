/*
 * hvq_compose.hip -- composition for CDNA4 / gfx950 (MI355X): uint8 pictures in slot layout built from ordered lists of layers, each a
 * rectangle of a resident picture with a signed integer weight per plane that replaces (PUT) or joins (ADD) what lies below it, one
 * rounding at the end (hvq_compose_pictures, include/hvqm4_amd.h: the values).  One launch serves any number of targets of any sizes,
 * samplings and layer lists: grid row = target (three HvqComposeJob, one per plane), grid column = one tile of one of its planes, Y's
 * first; workgroups past the target's tiles leave.
 *
 * A unit of its own (its own Makefile rule, the plain flags): the code of the other kernels does not change with it.
 *
 * A tile is HVQ_CP_TW x HVQ_CP_TH targets; lane l owns the dword of columns 4 (l & 15) .. + 3 of row l >> 4 and keeps its four
 * accumulators in registers.  The workgroup walks the records of its plane of the target's layers in order; index and record are
 * uniform (scalar loads), and a layer whose rectangle misses the tile costs that load and one uniform branch.  Two bodies, chosen per
 * layer plane on the host (hvq_cp_body); the values do not depend on the choice.
 *   Aligned.  A target dword is covered whole or not at all; a covered lane loads the one aligned source dword that lands on it.
 *   General.  A cover mask per byte; a lane with a covered byte builds its four source bytes from the two aligned dwords that hold
 *             them, each loaded only where it lies inside the source plane (a dword that lies outside holds no covered byte).
 * PUT is a select on the accumulator, not a branch.  Every target byte is written once, by one dword store; nothing else is written.
 * No LDS, no scratch, no workgroup waits for another.
 *
 * HVQ_CP_ABLATE (measurements only, wrong values; tools/compose_bench.py): 1 no source loads (a covered lane takes its
 * source index for the bytes), 2 no unpacking, multiplying, rounding and packing (a lane stores the last source dword it loaded).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_compose.h"

typedef uint32_t u32;
typedef int32_t i32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))

#ifndef HVQ_CP_ABLATE
#define HVQ_CP_ABLATE 0
#endif

static_assert(HVQ_CP_LANES == 256u && HVQ_CP_TW == 64u && HVQ_CP_TH == 16u, "the lane map below: 16 dwords a row, 16 rows");

__global__ __launch_bounds__(HVQ_CP_LANES)
void hvq_compose_kernel(const HvqComposeJob *__restrict__ jobs, const HvqComposeRec *__restrict__ recs)
{
    const HvqComposeJob *P = jobs + 3u * blockIdx.y;                  /* the target's planes */
    u32 t = blockIdx.x;
    if (t >= P->tiles) {                                              /* past Y: a tile of U, of V, or none (uniform) */
        t -= P->tiles; ++P;
        if (t >= P->tiles) {
            t -= P->tiles; ++P;
            if (t >= P->tiles) return;
        }
    }
    const HvqComposeJob &J = *P;
    const u32 ty = t / J.tiles_x, tx = t - ty * J.tiles_x;
    const u32 c0 = tx * HVQ_CP_TW, r0 = ty * HVQ_CP_TH;
    const u32 lane = threadIdx.x;
    const i32 x = (i32)(c0 + (lane & 15u) * 4u), y = (i32)(r0 + (lane >> 4));
    i32 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const HvqComposeRec *R = recs + 3u * (u64)J.first + J.plane;
    for (u32 k = 0; k < J.count; ++k, R += 3) {
        const HvqComposeRec &r = *R;                                  /* uniform: scalar registers */
        if (hvq_cp_misses(&r, c0, r0)) continue;                      /* uniform */
        const GLB u32 *in = (const GLB u32 *)(uintptr_t)r.src;
        const u32 put = r.mode == HVQ_CP_PUT;
        const i32 w = r.weight;
        const u32 m = hvq_cp_cover(&r, x, y);
        const i32 a = hvq_cp_src_byte(&r, x, y);
        u32 s = 0;
        if (r.body == HVQ_CP_ALIGNED) {                               /* uniform; m is 0 or 15, a a multiple of 4 */
#if HVQ_CP_ABLATE == 1
            if (m) s = (u32)a + (u32)(uintptr_t)in;
#else
            if (m) s = in[a >> 2];
#endif
        } else if (m) {
            const i32 q = a >> 2, n = hvq_cp_src_dwords(&r);
            u32 lo = 0, hi = 0;
#if HVQ_CP_ABLATE == 1
            lo = (u32)q + (u32)(uintptr_t)in; hi = lo + (u32)n;
#else
            if (q >= 0 && q < n) lo = in[q];
            if ((a & 3) && q + 1 >= 0 && q + 1 < n) hi = in[q + 1];
#endif
            s = hvq_cp_funnel(lo, hi, (u32)a);
        }
#if HVQ_CP_ABLATE == 2
        a0 = m ? (i32)s : a0;
        (void)put; (void)w;
        continue;
#endif
        a0 = hvq_cp_step(a0, m & 1u, put, w, s & 255u);
        a1 = hvq_cp_step(a1, m & 2u, put, w, (s >> 8) & 255u);
        a2 = hvq_cp_step(a2, m & 4u, put, w, (s >> 16) & 255u);
        a3 = hvq_cp_step(a3, m & 8u, put, w, s >> 24);
    }
    if ((u32)y < J.my && (u32)x < J.mx) {
#if HVQ_CP_ABLATE == 2
        *(GLB u32 *)(uintptr_t)(J.dst + (u64)(u32)y * J.mx + (u32)x) = (u32)a0 + (u32)(a1 | a2 | a3);
        return;
#endif
        const u32 out = hvq_cp_finish(a0, J.half, J.shift, J.bias) | hvq_cp_finish(a1, J.half, J.shift, J.bias) << 8 |
                        hvq_cp_finish(a2, J.half, J.shift, J.bias) << 16 | hvq_cp_finish(a3, J.half, J.shift, J.bias) << 24;
        *(GLB u32 *)(uintptr_t)(J.dst + (u64)(u32)y * J.mx + (u32)x) = out;
    }
}

/* tab_dev: HvqComposeJob[3 * ntargets], Y, U, V of a target one behind the other, and behind them HvqComposeRec[3 * nlayers], in device
 * memory; ntargets <= 65535; max_tiles = max over the targets of the tiles of their three planes together */
extern "C" hipError_t hvq_launch_compose(const void *tab_dev, int ntargets, uint32_t max_tiles, hipStream_t stream)
{
    if (ntargets <= 0 || !max_tiles) return hipSuccess;
    if (ntargets > 65535) return hipErrorInvalidValue;
    const HvqComposeJob *jobs = (const HvqComposeJob *)tab_dev;
    const HvqComposeRec *recs = (const HvqComposeRec *)(jobs + 3u * (size_t)ntargets);
    hipLaunchKernelGGL(hvq_compose_kernel, dim3(max_tiles, (uint32_t)ntargets), dim3(HVQ_CP_LANES), 0, stream, jobs, recs);
    return hipGetLastError();
}
