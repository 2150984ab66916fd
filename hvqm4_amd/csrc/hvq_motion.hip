/*
 * hvq_motion.hip -- block-matching motion fields between pictures for CDNA4 / gfx950 (MI355X): per B x B block of the luma plane of a
 * picture `a` the displacement (dy, dx), |dy|, |dx| <= R, at which the luma plane of a reference `b` has the smallest sum of absolute
 * differences, by full search, with the tie rule of include/hvqm4_amd.h (hvq_picture_motion: the specification).  One launch serves any
 * number of pictures of any sizes: grid row = picture, grid column = a tile of HVQ_MV_TILE x HVQ_MV_TILE samples of `a`.
 *
 * A unit of its own (its own Makefile rule and flags): the code of the other kernels does not change with it.
 *
 * Shape.  A workgroup of HVQ_MV_LANES lanes stages its tile of `a` and the window of `b` the tile can reach -- the tile widened by R on
 * every side, bytes outside the picture predicated off and held as zeros -- into LDS, then each of its four waves searches whole blocks
 * of the tile on its own: no reduction crosses waves, and no wave waits for global memory once per block.  The window lies in LDS so that
 * the byte at x - R of the tile's first column starts a dword: a candidate column x0 + dx with dx = -R + 4 g then starts a dword for
 * every block and every g, and one v_qsad_pk_u16_u8 on two neighbouring dwords of a row of `b` and one dword of `a` adds that dword's
 * four byte differences to the costs of the four candidates dx = -R + 4 g + (0, 1, 2, 3) at once, in four packed 16-bit sums (the
 * largest cost, 65280, fits).  The shift by R % 4 is paid once, by v_alignbyte_b32 when the window is staged, not per candidate.  A lane
 * owns one task (dy, g) per round; a wave's lanes cover the (2 R + 1) x ceil((2 R + 1) / 4) tasks of a block 64 at a time, in at most
 * HVQ_MV_ROUNDS rounds (R = 15: 248 tasks, 4 rounds, 97 % of the lanes at work).  What a lane's task of a round is -- its offset inside
 * a block's window, dy, dx and the low bits of its four keys -- is the same for every block and is worked out once per workgroup
 * (struct Task), so a round costs no division and four short key updates.  The rows of `a` are the same for every lane of the wave:
 * the block is read once from LDS, one dword a lane, and v_readlane_b32 hands every dword to a scalar register, the scalar operand of
 * its v_qsad in every round.  The row pitch of the window is 32 - ceil((2 R + 1) / 4) dwords: lane t of a round then reads bank
 * (constant - t) mod 32 (ds_read_b32 counts conflicts within 32 lanes over 32 banks).  A candidate whose block leaves the picture is
 * predicated off (its key is all ones), not clamped.  The winner is the unsigned minimum of the packed keys
 * cost << 15 | L1 << 10 | (dy + R) << 5 | (dx + R), reduced across the wave; cost_zero comes from the lane that owns (0, 0); lane 0
 * writes the record with one 16-byte vector store.  Nothing is zeroed in front of the launch, nothing is atomic.  What was measured to
 * get here is DESIGN.md 4.5.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_store, never flat (hvq_kernels.hip) */
typedef int i32x4 __attribute__((ext_vector_type(4)));

/* dwords of the window at radius R: (HVQ_MV_TILE + 2 R) rows of pitch 32 - ng(R) */
constexpr u32 mv_groups(u32 R) { return (2u * R + 1u + 3u) / 4u; }
constexpr u32 mv_window(u32 R) { return (HVQ_MV_TILE + 2u * R) * (32u - mv_groups(R)); }
constexpr u32 mv_window_max()
{
    u32 m = 0;
    for (u32 R = 0; R <= HVQ_MV_MAX_RADIUS; ++R) m = mv_window(R) > m ? mv_window(R) : m;
    return m;
}
#define HVQ_MV_WINDOW 2256u
static_assert(mv_window_max() == HVQ_MV_WINDOW, "the LDS window holds the tile's reach at every radius");
/* a row of the window is HVQ_MV_TILE / 4 + ng dwords wide; the pitch must hold it: 16 + ng <= 32 - ng */
static_assert(HVQ_MV_TILE / 4u + 2u * mv_groups(HVQ_MV_MAX_RADIUS) <= 32u, "the pitch holds a row at the largest radius");
static_assert(HVQ_MV_LANES == 256u, "four waves of 64 lanes");

/* rounds of 64 tasks a block takes at most: (2 R + 1) * ceil((2 R + 1) / 4) <= 31 * 8 = 248 */
#define HVQ_MV_ROUNDS 4u
static_assert((2u * HVQ_MV_MAX_RADIUS + 1u) * mv_groups(HVQ_MV_MAX_RADIUS) <= 64u * HVQ_MV_ROUNDS, "a wave covers a block's tasks in HVQ_MV_ROUNDS rounds");
#define HVQ_MV_APITCH (HVQ_MV_TILE / 4u)                /* dwords of a row of the tile of a in LDS */

/* what a lane's task of round r is, the same for every block: worked out once per workgroup, not once per block and round */
struct Task {
    u32 off;            /* dyi * pitch + g: the task's first dword inside a block's window */
    int dy, dx0;        /* dy, and dx of the first of the four candidates */
    u32 klo[4];         /* L1 << 10 | dy + R << 5 | dx + R of candidate k; all ones: no such candidate (dx > R, or no task) */
};

template <u32 B>
__device__ __forceinline__ void search_tile(const HvqMotionJob &J, const u32 *win, const u32 *atile, u32 R, u32 ty, u32 tx)
{
    constexpr u32 BD = B / 4u;                          /* dwords of a block's row */
    constexpr u32 NBT = HVQ_MV_TILE / B;                /* blocks of a tile's side */
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 ng = (2u * R + 4u) / 4u, pitch = 32u - ng;
    const u32 ntasks = (2u * R + 1u) * ng;
    const u32 tz = R * ng + R / 4u;                     /* the task that holds (0, 0): dy + R = R, dx = -R + 4 (R / 4) + R % 4 */
    const int iR = (int)R;
    const u32 ymax = J.h - B, xmax = J.w - B;           /* the largest corner of a block inside the picture */

    Task T[HVQ_MV_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < HVQ_MV_ROUNDS; ++r) {
        const bool live = r * 64u + lane < ntasks;
        const u32 t = live ? r * 64u + lane : 0u;       /* an idle lane reads what lane 0 reads; its keys are all ones */
        const u32 dyi = t / ng, g = t - dyi * ng;
        T[r].off = dyi * pitch + g;
        T[r].dy = (int)dyi - iR;
        T[r].dx0 = (int)(4u * g) - iR;
#pragma unroll
        for (u32 k = 0; k < 4u; ++k) {
            const int dy = T[r].dy, dx = T[r].dx0 + (int)k;
            T[r].klo[k] = live && dx <= iR ? (u32)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx)) << 10 | dyi << 5 | (u32)(dx + iR) : ~0u;
        }
    }

    for (u32 bi = wave; bi < NBT * NBT; bi += HVQ_MV_LANES / 64u) {
        const u32 br = bi / NBT, bc = bi % NBT;
        const u32 r = ty * NBT + br, c = tx * NBT + bc;
        if (r >= J.rows || c >= J.cols) continue;       /* a tile at the right or bottom edge has fewer blocks (uniform in the wave) */
        const int y0 = (int)(r * B), x0 = (int)(c * B);
        /* the block of a, dword (i, j) in lane i * BD + j, then every dword in a scalar register */
        const u32 av = atile[(br * B + (lane / BD) % B) * HVQ_MV_APITCH + bc * BD + lane % BD];
        u32 as[B * BD];
#pragma unroll
        for (u32 q = 0; q < B * BD; ++q) as[q] = (u32)__builtin_amdgcn_readlane((int)av, (int)q);
        const u32 *blk = win + br * B * pitch + bc * BD;
        u32 best = ~0u, cz = 0;
#pragma unroll
        for (u32 rd = 0; rd < HVQ_MV_ROUNDS; ++rd) {
            if (rd * 64u >= ntasks) break;              /* uniform */
            const u32 *p = blk + T[rd].off;
            u64 acc = 0;
#pragma unroll
            for (u32 i = 0; i < B; ++i) {
                u32 s[BD + 1u];
#pragma unroll
                for (u32 j = 0; j <= BD; ++j) s[j] = p[i * pitch + j];
#pragma unroll
                for (u32 j = 0; j < BD; ++j) acc = __builtin_amdgcn_qsad_pk_u16_u8(((u64)s[j + 1u] << 32) | s[j], as[i * BD + j], acc);
            }
            /* a candidate whose block leaves the picture is predicated off: as unsigned, a negative corner is above every maximum */
            const bool yok = (u32)(y0 + T[rd].dy) <= ymax;
#pragma unroll
            for (u32 k = 0; k < 4u; ++k) {
                const u32 cost = (u32)(acc >> (16u * k)) & 0xFFFFu;
                const bool ok = yok && (u32)(x0 + T[rd].dx0 + (int)k) <= xmax;
                best = min(best, ok ? cost << 15 | T[rd].klo[k] : ~0u);
            }
            if (rd == tz >> 6) cz = (u32)(acc >> (16u * (R & 3u))) & 0xFFFFu;         /* kept by every lane, read from the owner below */
        }
#pragma unroll
        for (int m = 32; m; m >>= 1) best = min(best, (u32)__shfl_xor((int)best, m));
        cz = (u32)__shfl((int)cz, (int)(tz & 63u));
        if (lane == 0) {
            const i32x4 rec = { (int)((best >> 5) & 31u) - iR, (int)(best & 31u) - iR, (int)(best >> 15), (int)cz };
            *((GLB i32x4 *)(uintptr_t)J.out + (size_t)r * J.cols + c) = rec;
        }
    }
}

__global__ __launch_bounds__(HVQ_MV_LANES)
void hvq_motion_kernel(const HvqMotionJob *__restrict__ jobs, u32 block, u32 R)
{
    const HvqMotionJob &J = jobs[blockIdx.y];
    if (blockIdx.x >= J.tiles) return;                                 /* past this picture: leave (uniform) */
    const u32 ty = blockIdx.x / J.tiles_x, tx = blockIdx.x - ty * J.tiles_x;

    __shared__ u32 win[HVQ_MV_WINDOW];
    __shared__ u32 atile[HVQ_MV_TILE * HVQ_MV_APITCH];
    const u32 ng = (2u * R + 4u) / 4u, pitch = 32u - ng, width = HVQ_MV_TILE / 4u + ng, nrows = HVQ_MV_TILE + 2u * R;
    const u32 sh = (0u - R) & 3u;                                      /* (x of the window's first byte) mod 4: a tile starts at a multiple of 64 */
    const int w = (int)J.w, h = (int)J.h;
    const GLB u32 *a = (const GLB u32 *)(uintptr_t)J.a;
    const GLB u32 *b = (const GLB u32 *)(uintptr_t)J.b;
    /* the tile of a: one coalesced pass, so that no wave waits for global memory once per block */
#pragma unroll
    for (u32 idx = threadIdx.x; idx < HVQ_MV_TILE * HVQ_MV_APITCH; idx += HVQ_MV_LANES) {
        const u32 y = ty * HVQ_MV_TILE + idx / HVQ_MV_APITCH, x = tx * HVQ_MV_TILE + 4u * (idx % HVQ_MV_APITCH);
        atile[idx] = y < J.h && x < J.w ? a[(y * J.w + x) / 4u] : 0u;
    }
    for (u32 idx = threadIdx.x; idx < nrows * width; idx += HVQ_MV_LANES) {
        const u32 row = idx / width, col = idx - row * width;
        const int y = (int)(ty * HVQ_MV_TILE + row) - (int)R;
        const int xlo = (int)(tx * HVQ_MV_TILE + 4u * col) - (int)R - (int)sh;      /* a multiple of 4: the dword that holds the first byte */
        /* a dword of b lies inside its row or outside it (w is a multiple of 4): nothing outside plane Y is read */
        u32 lo = 0, hi = 0;
        if (y >= 0 && y < h) {
            if (xlo >= 0 && xlo < w) lo = b[((u32)y * J.w + (u32)xlo) / 4u];
            if (sh && xlo + 4 >= 0 && xlo + 4 < w) hi = b[((u32)y * J.w + (u32)(xlo + 4)) / 4u];
        }
        win[row * pitch + col] = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    __syncthreads();

    if (block == 16u) search_tile<16u>(J, win, atile, R, ty, tx);
    else search_tile<8u>(J, win, atile, R, ty, tx);
}

/* jobs_dev: HvqMotionJob[njobs] in device memory; max_tiles = max over jobs of `tiles`; block 8 or 16, radius 0 .. HVQ_MV_MAX_RADIUS */
extern "C" hipError_t hvq_launch_motion(const void *jobs_dev, int njobs, uint32_t max_tiles, int block, int radius, hipStream_t stream)
{
    if (njobs <= 0 || !max_tiles) return hipSuccess;
    if (njobs > 65535 || (block != 8 && block != 16) || radius < 0 || radius > (int)HVQ_MV_MAX_RADIUS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_motion_kernel, dim3(max_tiles, (uint32_t)njobs), dim3(HVQ_MV_LANES), 0, stream, (const HvqMotionJob *)jobs_dev,
                       (u32)block, (u32)radius);
    return hipGetLastError();
}
