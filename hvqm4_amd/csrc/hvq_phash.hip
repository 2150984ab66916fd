/*
 * hvq_phash.hip -- perceptual hashes of resident pictures and nearest-hash search for CDNA4 / gfx950 (MI355X): hvq_picture_hashes and
 * hvq_hash_nearest of include/hvqm4_amd.h (the specification; the shared arithmetic: hvq_phash.h).
 *
 * A unit of its own (its own Makefile rule and flags): the code of the other kernels does not change with it.
 *
 * hvq_phash_cells_kernel, grid row = picture.  The 32 x 32 grid and the 32-row x 9-column grid share their 32 row cells, and everything
 * else (S8, D, the sums) follows from them: one pass over the luma plane with 32 row weights and 32 + 9 column weights.  A workgroup takes
 * cells_pw consecutive row cells (HvqHashJob) and up to HVQ_PH_LANES column units of 16 (or 8) samples; the lanes of one row cell stand
 * lanes_x side by side and rows_pp rows deep (640 x 480: a row cell is 15 rows of 40 units; four row cells a workgroup, 64 lanes each).
 * The sample rows that only partly lie in a cell (its first and last, when h is no multiple of 32) are read for the neighbouring cell
 * too: from L2, the plane comes from memory once.
 *   rows     A lane walks down its unit: four 16-byte loads (nontemporal, address space 1) are issued before the first is used, and
 *            acc[j] += wy(r, y) * sample j, sixteen 32-bit registers (at most 255 * sum_y wy = 255 h < 2^21).
 *   columns  Then, once per lane and grid, the lane's samples are weighted into column cells: consecutive samples of one cell are summed
 *            in a register (a lane's 16 samples touch two or three cells of a 640-wide plane) and leave the lane as ONE 64-bit LDS add per
 *            cell touched -- not one per sample: a row cell of 640 x 480 is 40 lanes x about 5 adds against 9 600 samples.
 *   out      The lanes add the workgroup's cells (41 per row cell) into the picture's cells in library memory (zeroed in front of the launch), 64-bit
 *            no-return atomics at agent scope.  Cells are 64 bits wide from the workgroup on: 255 w h exceeds 2^32 from 16.8 M samples.
 * Integer addition: the cells do not depend on the order of arrival.  No workgroup waits for another.
 *
 * hvq_phash_finish_kernel, one workgroup per picture: the 1024 means in sixteenths (64-bit divisions, four a lane), the DCT pass over c
 * (256 lanes, 32 bits), the pass over r (64 lanes, 64 bits), a 64-element rank for the two middle values, the three ballots, one lane
 * stores the record.
 *
 * hvq_hash_nearest_kernel: a lane owns a query, a workgroup HVQ_HN_LANES of them.  The database passes through LDS in tiles of HVQ_HN_TILE
 * hashes (every lane of a wave reads the same word: a broadcast); a pair costs two v_xor, two v_bcnt_u32_b32 (the second adds onto the
 * first), and the running minimum of d << 24 | j (one v_lshl_or, one v_min_u32: the smallest (d, j) is the smallest key), the count and
 * the first index within the threshold, all in registers.  "Earlier than me" (self_offset) bounds the tiles a workgroup walks; only the
 * tiles that straddle some lane's bound compare j with it.  The record leaves as one 16-byte store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_phash.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_atomic, never flat (hvq_kernels.hip) */
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

static_assert(HVQ_PH_LANES == 256u && HVQ_PH_COLS == 41u && HVQ_PH_ROWS == 32u, "the lane roles of both hash kernels");
/* a lane's row sums: 255 * (sum over y of wy(r, y) = h); a lane's run of one cell: 16 samples * 32 * that */
static_assert(255ull * HVQ_PH_MAX_SIDE < (1ull << 21) && 16ull * 32ull * 255ull * HVQ_PH_MAX_SIDE < (1ull << 32), "32-bit registers hold a lane's sums");
static_assert(32ull * HVQ_PH_MAX_SIDE * HVQ_PH_MAX_SIDE < (1ull << 32), "sample offsets and scaled positions fit 32 bits");
/* the DCT: |pass over c| <= 32 * 4096 * 4080 < 2^31 */
static_assert(32ll * 4096ll * 4080ll < (1ll << 31), "the first DCT pass fits 32 bits");

__device__ const HvqPhDct PH_DCT = hvq_ph_dct();

template <int NC> struct PhVec;
template <> struct PhVec<16> { typedef u32x4 type; };
template <> struct PhVec<8> { typedef u32x2 type; };

/* the lane's NC row sums into the workgroup's cells of grid G (its columns start at `first` of the 41) */
template <int NC, u32 G>
__device__ __forceinline__ void ph_columns(const u32 (&acc)[NC], u32 x0, u32 w, u32 first, u64 *cells)
{
    u32 p = G * x0;                                     /* position in units of 1 / G sample; a cell is w of them wide */
    u32 c = p / w, bound = w * (c + 1u);
    u32 run = 0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        u32 rem = G;
        while (rem) {                                   /* at most ceil(G / w) + 1 rounds: a sample wider than a cell (w < G) feeds several */
            const u32 take = min(rem, bound - p);
            run += take * acc[j];
            p += take; rem -= take;
            if (p == bound) {
                (void)__hip_atomic_fetch_add(&cells[first + c], (u64)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                run = 0; ++c; bound += w;
            }
        }
    }
    if (run) (void)__hip_atomic_fetch_add(&cells[first + c], (u64)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NC>
__device__ __forceinline__ void ph_body(const HvqHashJob &J, u32 r0, u32 xc, u64 *wg_cells)
{
    typedef typename PhVec<NC>::type V;
    const u32 lane = threadIdx.x;
    const u32 sub = lane >> J.sub_shift, within = lane - (sub << J.sub_shift);   /* the lane's row cell of the workgroup's, its place among that cell's lanes */
    const u32 ry = within / J.lanes_x, ux = within - ry * J.lanes_x;
    const u32 u = xc * HVQ_PH_LANES + ux;                               /* the lane's unit of the row */
    const bool on = ry < J.rows_pp && u < J.units;
    const u32 w = J.w, h = J.h, r = r0 + sub;
    u64 *cells = wg_cells + sub * HVQ_PH_COLS;
    const u32 ylo = hvq_ph_first(32u, h, r), yhi = hvq_ph_end(32u, h, r);   /* the rows with a share in row cell r */
    const u32 most = (h + 31u) / 32u + 1u;                              /* no row cell has more rows: uniform over the workgroup */
    const GLB uint8_t *a = (const GLB uint8_t *)(uintptr_t)J.a + (size_t)u * NC;
    u32 acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0;
    for (u32 i0 = 0; i0 < most; i0 += 4u * J.rows_pp) {
        V v[4];
        u32 wy[4];
#pragma unroll
        for (u32 k = 0; k < 4u; ++k) {
            const u32 y = ylo + i0 + ry + k * J.rows_pp;
            const bool ok = on && y < yhi;
            V z;
#pragma unroll
            for (int d = 0; d < NC / 4; ++d) z[d] = 0u;
            /* the load itself is predicated: nothing outside the plane is read (y < yhi <= h, u < units) */
            v[k] = ok ? __builtin_nontemporal_load((const GLB V *)(a + y * w)) : z;
            wy[k] = ok ? hvq_ph_weight(32u, h, r, y) : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < 4u; ++k)
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] += wy[k] * ((v[k][j >> 2] >> (8 * (j & 3))) & 255u);
    }
    if (on) {
        ph_columns<NC, 32u>(acc, u * NC, w, 0u, cells);
        ph_columns<NC, 9u>(acc, u * NC, w, 32u, cells);
    }
}

__global__ __launch_bounds__(HVQ_PH_LANES)
void hvq_phash_cells_kernel(const HvqHashJob *__restrict__ jobs)
{
    const HvqHashJob &J = jobs[blockIdx.y];
    const u32 wg = blockIdx.x;
    if (wg >= J.wgs) return;                                            /* past this picture: leave (uniform) */
    const u32 lane = threadIdx.x;
    __shared__ u64 cells[HVQ_PH_MAX_CPW * HVQ_PH_COLS];
    const u32 ncells = J.cells_pw * HVQ_PH_COLS;
    for (u32 i = lane; i < ncells; i += HVQ_PH_LANES) cells[i] = 0;
    __syncthreads();
    const u32 groups = HVQ_PH_ROWS / J.cells_pw;                        /* workgroups that share a chunk of columns */
    const u32 xc = wg / groups, r0 = (wg - xc * groups) * J.cells_pw;
    if (J.w & 8u) ph_body<8>(J, r0, xc, cells);                         /* rows of an odd number of 8-byte units: 8-byte loads */
    else ph_body<16>(J, r0, xc, cells);
    __syncthreads();
    for (u32 i = lane; i < ncells; i += HVQ_PH_LANES) {                 /* the cells of consecutive row cells lie one behind the other */
        const u64 v = cells[i];
        GLB u64 *acc = (GLB u64 *)(uintptr_t)J.acc + r0 * HVQ_PH_COLS + i;
        if (v) (void)__hip_atomic_fetch_add(acc, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(HVQ_PH_LANES)
void hvq_phash_finish_kernel(const HvqHashJob *__restrict__ jobs)
{
    const HvqHashJob &J = jobs[blockIdx.x];
    const u32 t = threadIdx.x;
    __shared__ u64 S[HVQ_PH_CELLS];
    __shared__ int32_t M[1024];
    __shared__ int32_t G[256];
    __shared__ i64 F[64];
    __shared__ i64 mid[2];
    const GLB u64 *acc = (const GLB u64 *)(uintptr_t)J.acc;
    for (u32 i = t; i < HVQ_PH_CELLS; i += HVQ_PH_LANES) S[i] = acc[i];
    __syncthreads();
    const u64 wh = (u64)J.w * J.h;
#pragma unroll
    for (u32 k = 0; k < 4u; ++k) {
        const u32 i = t + k * HVQ_PH_LANES;                             /* cell (i / 32, i % 32) of S32 */
        M[i] = hvq_ph_mean16(S[(i >> 5) * HVQ_PH_COLS + (i & 31u)], wh);
    }
    __syncthreads();
    {
        const u32 r = t >> 3, l = t & 7u;                               /* the pass over c: 32 x 8 values, one a lane */
        int32_t s = 0;
#pragma unroll
        for (u32 c = 0; c < 32u; ++c) s += PH_DCT.c[l][c] * M[r * 32u + c];
        G[t] = s;
    }
    __syncthreads();
    const u32 k8 = (t >> 3) & 7u, l8 = t & 7u;                          /* element (k8, l8) of the 8 x 8 arrays: lanes 0 .. 63 */
    i64 f = 0;
    if (t < 64u) {
#pragma unroll
        for (u32 r = 0; r < 32u; ++r) f += (i64)PH_DCT.c[k8][r] * G[r * 8u + l8];
        F[t] = f;
    }
    __syncthreads();
    if (t < 64u) {
        u32 rank = 0;                                                   /* ties ranked by index: the ranks are a permutation */
        for (u32 j = 0; j < 64u; ++j) { const i64 g = F[j]; rank += (g < f || (g == f && j < t)) ? 1u : 0u; }
        if (rank == 31u) mid[0] = f;
        if (rank == 32u) mid[1] = f;
    }
    __syncthreads();
    if (t < 64u) {                                                      /* wave 0, every lane of it */
        u64 block = 0, d0 = 0, d1 = 0;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
            const u32 row = (4u * k8 + i) * HVQ_PH_COLS;
#pragma unroll
            for (u32 j = 0; j < 4u; ++j) block += S[row + 4u * l8 + j];
            d0 += S[row + 32u + l8];
            d1 += S[row + 33u + l8];
        }
        const u64 total = wave_sum(block);                              /* the sum of all S32 = 16 T */
        /* lane e holds element e = 8 r + c, which is bit 63 - e of the hash */
        const u64 ah = __brevll(__ballot(64u * block > total));
        const u64 dh = __brevll(__ballot(d1 > d0));
        const u64 ph = __brevll(__ballot(2 * f > mid[0] + mid[1]));
        if (t == 0) {
            GLB u64 *out = (GLB u64 *)(uintptr_t)J.out;
            out[0] = ah; out[1] = dh; out[2] = ph; out[3] = total / 1024u;
        }
    }
}

/* jobs_dev: HvqHashJob[njobs] in device memory; max_wgs = max over jobs of wgs.  The cells the jobs point to are zero when the first launch
 * runs (the caller queues the memset in front of it on the same stream); the second launch writes every record. */
extern "C" hipError_t hvq_launch_hashes(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (njobs > 65535 || !max_wgs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_phash_cells_kernel, dim3(max_wgs, (uint32_t)njobs), dim3(HVQ_PH_LANES), 0, stream, (const HvqHashJob *)jobs_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hvq_phash_finish_kernel, dim3((uint32_t)njobs), dim3(HVQ_PH_LANES), 0, stream, (const HvqHashJob *)jobs_dev);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------------------------------ nearest hashes */
#define HN_EMPTY_KEY ((65u << 24) | 0xFFFFFFu)          /* above every key of a candidate: d <= 64 */

/* `n` hashes of the staged tile, the first of them candidate j0.  CHECK: some lane's bound lies inside the tile */
template <bool CHECK>
__device__ __forceinline__ void hn_tile(const u64 *tile, u32 n, u32 j0, u64 q, u32 lim, u32 thr, u32 &key, u32 &cnt, u32 &first)
{
#pragma unroll 8
    for (u32 k = 0; k < n; ++k) {
        const u64 x = q ^ tile[k];
        u32 d = (u32)__builtin_popcount((u32)x) + (u32)__builtin_popcount((u32)(x >> 32));
        const u32 j = j0 + k;
        if (CHECK) d = j < lim ? d : 65u;               /* no candidate of this lane: never the minimum's distance below 65, never within */
        key = min(key, (d << 24) | j);
        const bool in = d <= thr;
        cnt += in ? 1u : 0u;
        first = min(first, in ? j : 0xFFFFFFFFu);
    }
}

__global__ __launch_bounds__(HVQ_HN_LANES)
void hvq_hash_nearest_kernel(const u64 *__restrict__ q_, u32 nq, u32 q_stride, const u64 *__restrict__ db_, u32 ndb, u32 db_stride,
                             i64 self_offset, u32 thr, int32_t *__restrict__ out_)
{
    const GLB u64 *q = (const GLB u64 *)(uintptr_t)q_;
    const GLB u64 *db = (const GLB u64 *)(uintptr_t)db_;
    __shared__ u64 tile[HVQ_HN_TILE];
    const u32 lane = threadIdx.x;
    const u32 i0 = blockIdx.x * HVQ_HN_LANES, i = i0 + lane;
    const u32 i1 = min(nq, i0 + HVQ_HN_LANES) - 1u;                     /* the workgroup's last query */
    const bool on = i < nq;
    const u64 qi = on ? q[(size_t)i * q_stride] : 0ull;
    /* candidates j < lim; self_offset < 0: all (the host passes -1 for every offset that admits all) */
    const u32 lim = self_offset < 0 ? ndb : (u32)min((i64)ndb, self_offset + (i64)i);
    const u32 lim_lo = self_offset < 0 ? ndb : (u32)min((i64)ndb, self_offset + (i64)i0);    /* uniform: the smallest and the largest bound */
    const u32 lim_hi = self_offset < 0 ? ndb : (u32)min((i64)ndb, self_offset + (i64)i1);
    u32 key = HN_EMPTY_KEY, cnt = 0, first = 0xFFFFFFFFu;
    for (u32 t0 = 0; t0 < lim_hi; t0 += HVQ_HN_TILE) {
        const u32 n = min(HVQ_HN_TILE, lim_hi - t0);
        __syncthreads();                                                /* the tile before this one has been read */
#pragma unroll
        for (u32 k = 0; k < HVQ_HN_TILE / HVQ_HN_LANES; ++k) {
            const u32 s = k * HVQ_HN_LANES + lane;
            if (s < n) tile[s] = db[(size_t)(t0 + s) * db_stride];      /* t0 + s < lim_hi <= ndb */
        }
        __syncthreads();
        if (t0 + n <= lim_lo) hn_tile<false>(tile, n, t0, qi, lim, thr, key, cnt, first);
        else hn_tile<true>(tile, n, t0, qi, lim, thr, key, cnt, first);
    }
    if (on) {
        const u32 d = key >> 24;
        i32x4 rec;
        rec[0] = d > 64u ? -1 : (int32_t)(key & 0xFFFFFFu);
        rec[1] = d > 64u ? 65 : (int32_t)d;
        rec[2] = (int32_t)cnt;
        rec[3] = (int32_t)first;                                        /* 0xFFFFFFFF: -1 */
        ((GLB i32x4 *)(uintptr_t)out_)[i] = rec;
    }
}

extern "C" hipError_t hvq_launch_hash_nearest(const uint64_t *q, uint32_t nq, uint32_t q_stride, const uint64_t *db, uint32_t ndb, uint32_t db_stride,
                                              int64_t self_offset, uint32_t threshold, int32_t *out, hipStream_t stream)
{
    if (!nq) return hipSuccess;
    if (nq > HVQ_HN_MAX || ndb > HVQ_HN_MAX || threshold > 64u || !q_stride || !db_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hvq_hash_nearest_kernel, dim3((nq + HVQ_HN_LANES - 1u) / HVQ_HN_LANES), dim3(HVQ_HN_LANES), 0, stream,
                       q, nq, q_stride, db, ndb, db_stride, (i64)self_offset, threshold, out);
    return hipGetLastError();
}
