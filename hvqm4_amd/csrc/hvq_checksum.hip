/*
 * hvq_checksum.hip -- checksums of resident pictures for CDNA4 / gfx950 (MI355X): zlib's CRC-32 and Adler-32 of every plane and of the
 * picture Y | U | V, computed where the picture lies (hvq_picture_checksums, include/hvqm4_amd.h; the arithmetic: hvq_checksum.h).  Two
 * launches, the second queued behind the first: grid row = picture in both.
 *
 * A unit of its own (its own Makefile rule and flags): the code of the other kernels does not change with it.
 *
 * Shape of hvq_checksum_kernel.  A workgroup of HVQ_CK_LANES lanes takes HVQ_CK_CHUNK consecutive 16-byte units of ONE plane, counted from
 * the plane's end, so that exactly c * 16 KiB lie behind workgroup c's chunk and only the chunk at the plane's START can be short: its
 * missing units are leading zeros, which a CRC register of 0 does not see and which add nothing to Adler's sums.  A lane issues its
 * HVQ_CK_UNITS loads -- each wave instruction one contiguous 1 KiB run, nontemporal, address space 1 -- before it touches the first.
 *   CRC.   Everything is the raw register R (start 0, no final xor), linear over GF(2): the chunk's R is the xor over its dwords d of
 *          d * x^(32 + 8 * bytes behind the dword) mod P.  The byte step (HVQ_CK_STEP) turns a lane's 16 dwords into the lane's R at the
 *          end of its last unit; one product with the lane's own constant x^(8 * 16 (255 - lane)) moves it to the chunk's end; an xor
 *          butterfly across the wave and LDS across the four waves give the chunk's R; one lane multiplies by x^(8 * 16384 c), a product
 *          of compile-time constants picked by the bits of c, and issues ONE no-return 32-bit atomic xor.
 *   Adler. Per unit s = sum d (v_sad_u8) and t = sum (16 - b) d_b (v_dot4_u32_u8); the lane adds 16 (units behind it in the chunk) s + t
 *          in 32 bits (bound asserted below); the workgroup's totals are 64-bit, the chunk's own offset 16384 c S is added once per
 *          workgroup, and two no-return 64-bit atomic adds leave it.  Nothing is reduced mod 65521 here.
 * All atomics are agent scope into the picture's accumulator, which the caller zeroes in front of the launch.  xor and integer addition:
 * the result does not depend on the order of arrival.
 *
 * hvq_checksum_finish_kernel, one lane per picture, turns the accumulators into the eight values: the CRC's initial-register and final-xor
 * terms, the two mod 65521, and the picture's values from the planes' by the combine identities.
 *
 * HVQ_CK_STEP picks the byte step; 1 is built, 0 and 2 lost to it by measurement and stay for comparison:
 *   0  shift/xor: a unit's dwords xored into the register, 32 single-bit steps each; units joined Horner-style by x^(8 * 4096)
 *   1  slice-by-4 tables in LDS (4 KiB, built by the workgroup), four dependent lookups per dword; units joined as in 0
 *   2  xor matrix: every dword times its own compile-time constant x^(32 + 8 * bytes behind it in the lane's run), 32 conditional xors of
 *      literals, no dependency between dwords and no Horner step
 * HVQ_CK_ABLATE (measurements only, wrong values): 1 no byte step, 2 no per-lane and per-workgroup products, 3 no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_checksum.h"

#ifndef HVQ_CK_STEP
#define HVQ_CK_STEP 1
#endif
#ifndef HVQ_CK_ABLATE
#define HVQ_CK_ABLATE 0
#endif

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_atomic, never flat (hvq_kernels.hip) */
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

static_assert(HVQ_CK_LANES == 256u && HVQ_CK_LANES % 64u == 0, "four waves: the LDS stage, the 256 table entries and the 256 lane constants");
static_assert(HVQ_CK_UNITS == 4u, "the xor matrix names 16 dwords");
constexpr u32 CK_STRIDE_BYTES = HVQ_CK_LANES * 16u;     /* between two units of a lane */
constexpr u32 CK_CHUNK_BYTES = HVQ_CK_CHUNK * 16u;
/* chunk indices: a plane has at most HVQ_CK_MAX_UNITS / HVQ_CK_CHUNK chunks */
constexpr int CK_CHUNK_BITS = 12;
static_assert(HVQ_CK_MAX_UNITS / HVQ_CK_CHUNK <= (1u << CK_CHUNK_BITS), "the bits of a chunk index mul_chunks walks");
/* Accumulator widths.  A unit has s <= 16 * 255 = 4080 and t <= 255 * (16 + ... + 1) = 34 680; the lane weighs s with 16 * (units behind
 * it in the chunk) <= 16 * 1023.  Four units: 32 bits hold the lane's sums.  Everything that leaves the lane's own loop is 64 bits. */
static_assert((u64)HVQ_CK_UNITS * (16ull * (HVQ_CK_CHUNK - 1u) * 4080ull + 34680ull) < (1ull << 32), "a lane's weighted sum must fit 32 bits");

/* a * K for a constant K: the 32 columns K * x^i are literals */
struct CkCols { u32 c[32]; };
constexpr CkCols ck_cols(u32 k)
{
    CkCols t{};
    for (int i = 31; i >= 0; --i) { t.c[i] = k; k = (k >> 1) ^ (HVQ_CRC_POLY & (0u - (k & 1u))); }
    return t;
}
template <u32 K>
__device__ __forceinline__ u32 mulc(u32 a)
{
    constexpr CkCols C = ck_cols(K);
    u32 p = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) p ^= C.c[i] & (0u - ((a >> i) & 1u));
    return p;
}

/* x^(8 * 16 * (255 - lane)): from the end of a lane's last unit to the end of the chunk */
struct CkLaneK { u32 k[HVQ_CK_LANES]; };
constexpr CkLaneK ck_lane_k()
{
    CkLaneK t{};
    u32 v = HVQ_CRC_ONE;
    for (int l = (int)HVQ_CK_LANES - 1; l >= 0; --l) { t.k[l] = v; v = hvq_gf_mul(v, hvq_gf_xpow8(16)); }
    return t;
}
__device__ const CkLaneK CK_LANE_K = ck_lane_k();

/* r * x^(8 * 16384 * c): one constant per set bit of c (uniform over the workgroup) */
template <int J>
__device__ __forceinline__ u32 mul_chunks(u32 r, u32 c)
{
    if constexpr (J < CK_CHUNK_BITS) {
        constexpr u32 K = hvq_gf_xpow8((u64)CK_CHUNK_BYTES << J);
        if ((c >> J) & 1u) r = mulc<K>(r);
        return mul_chunks<J + 1>(r, c);
    } else {
        return r;
    }
}

#if HVQ_CK_STEP == 2
/* dword j of unit k has 4 (3 - j) bytes behind it in the unit and (3 - k) strides behind the unit */
template <int KJ>
__device__ __forceinline__ u32 matrix_terms(const u32x4 (&v)[HVQ_CK_UNITS])
{
    if constexpr (KJ < 16) {
        constexpr int k = KJ / 4, j = KJ % 4;
        constexpr u32 K = hvq_gf_xpow8(4u + 4u * (3u - j) + (u64)CK_STRIDE_BYTES * (3u - k));
        return mulc<K>(v[k][j]) ^ matrix_terms<KJ + 1>(v);
    } else {
        return 0u;
    }
}
#endif

__device__ __forceinline__ u32 wave_xor(u32 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

#ifdef HVQ_CK_WAVES                                      /* measurements: a floor under the occupancy, that is a cap on the registers */
__attribute__((amdgpu_waves_per_eu(HVQ_CK_WAVES, 8)))
#endif
__global__ __launch_bounds__(HVQ_CK_LANES)
void hvq_checksum_kernel(const HvqChecksumJob *__restrict__ jobs)
{
    const HvqChecksumJob &J = jobs[blockIdx.y];
    const u32 wg = blockIdx.x;
    if (wg >= J.wg_first[3]) return;                                   /* past this picture: leave (uniform) */
    const u32 p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);       /* the workgroup's plane */
    const u32 n = J.units[p];
    const u32 c = wg - J.wg_first[p];                                  /* whole chunks behind this one */
    const u32 lane = threadIdx.x;
    /* the lane's first unit; negative: in front of the plane (only in the chunk at the plane's start) */
    const int first = (int)n - (int)((c + 1u) * HVQ_CK_CHUNK) + (int)lane;
    const GLB u32x4 *a = (const GLB u32x4 *)(uintptr_t)(J.a + J.plane_off[p]);

#if HVQ_CK_STEP == 1
    /* T[m][b]: the register after byte b and m zero bytes.  Lane b builds entry b of all four: T[m + 1][b] = T[m][b] stepped by a byte */
    __shared__ u32 T[4][256];
    {
        u32 t = lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) t = (t >> 1) ^ (HVQ_CRC_POLY & (0u - (t & 1u)));
        T[0][lane] = t;
        __syncthreads();
#pragma unroll
        for (int m = 1; m < 4; ++m) { t = (t >> 8) ^ T[0][t & 255u]; T[m][lane] = t; }
        __syncthreads();
    }
#endif

    u32x4 v[HVQ_CK_UNITS];
#pragma unroll
    for (u32 k = 0; k < HVQ_CK_UNITS; ++k) {
        const int i = first + (int)(k * HVQ_CK_LANES);
        const u32x4 z = { 0u, 0u, 0u, 0u };
        /* a unit in front of the plane contributes zeros; the load itself is predicated: nothing outside the plane is read */
        v[k] = i >= 0 ? __builtin_nontemporal_load(a + i) : z;
    }

    /* Adler: s_all = sum d, w = sum over the lane's units of 16 (units behind it in the chunk) s + t */
    u32 s_all = 0, w = 0;
#pragma unroll
    for (u32 k = 0; k < HVQ_CK_UNITS; ++k) {
        u32 s = 0, t = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 top = 16u - 4u * j;                              /* weight of the dword's first byte */
            s = __builtin_amdgcn_sad_u8(v[k][j], 0u, s);
            t = __builtin_amdgcn_udot4(v[k][j], top | ((top - 1u) << 8) | ((top - 2u) << 16) | ((top - 3u) << 24), t, false);
        }
        w += 16u * (HVQ_CK_CHUNK - 1u - k * HVQ_CK_LANES - lane) * s + t;
        s_all += s;
    }

    /* CRC: the lane's R at the end of its last unit */
    u32 r = 0;
#if HVQ_CK_ABLATE == 1
#pragma unroll
    for (u32 k = 0; k < HVQ_CK_UNITS; ++k) r ^= v[k][0] ^ v[k][1] ^ v[k][2] ^ v[k][3];
#elif HVQ_CK_STEP == 2
    r = matrix_terms<0>(v);
#else
#pragma unroll
    for (u32 k = 0; k < HVQ_CK_UNITS; ++k) {
        u32 u = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            u ^= v[k][j];
#if HVQ_CK_STEP == 0
#pragma unroll
            for (int b = 0; b < 32; ++b) u = (u >> 1) ^ (HVQ_CRC_POLY & (0u - (u & 1u)));
#else
            u = T[3][u & 255u] ^ T[2][(u >> 8) & 255u] ^ T[1][(u >> 16) & 255u] ^ T[0][u >> 24];
#endif
        }
        r = (k ? mulc<hvq_gf_xpow8(CK_STRIDE_BYTES)>(r) : 0u) ^ u;
    }
#endif
#if HVQ_CK_ABLATE != 2
    r = hvq_gf_mul(r, CK_LANE_K.k[lane]);                              /* ... moved to the end of the chunk */
#endif

    __shared__ u64 part[HVQ_CK_LANES / 64u][3];
    const u64 w0 = wave_xor(r), w1 = wave_sum(s_all), w2 = wave_sum(w);
    if ((lane & 63u) == 0) {
        u64 *row = part[lane >> 6];
        row[0] = w0; row[1] = w1; row[2] = w2;
    }
    __syncthreads();
    if (lane < 3u) {
        u64 t = 0, s = 0;
#pragma unroll
        for (u32 k = 0; k < HVQ_CK_LANES / 64u; ++k) {
            if (lane == 0) t ^= part[k][0]; else t += part[k][lane];
            s += part[k][1];
        }
        GLB u64 *acc = (GLB u64 *)(uintptr_t)J.acc + p * 4u;
#if HVQ_CK_ABLATE != 3
        if (lane == 0) {
#if HVQ_CK_ABLATE != 2
            t = mul_chunks<0>((u32)t, c);                              /* ... and to the end of the plane */
#endif
            (void)__hip_atomic_fetch_xor((GLB u32 *)acc, (u32)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 2) t += (u64)CK_CHUNK_BYTES * c * s;           /* the bytes behind the chunk weigh every byte of it */
            (void)__hip_atomic_fetch_add(acc + lane, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#else
        if (t + s == 0x123456789ull) acc[lane] = t;                    /* keeps the reduction alive */
#endif
    }
}

__global__ __launch_bounds__(64)
void hvq_checksum_finish_kernel(const HvqChecksumJob *__restrict__ jobs, int njobs)
{
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= njobs) return;
    const HvqChecksumJob &J = jobs[i];
    const GLB u64 *acc = (const GLB u64 *)(uintptr_t)J.acc;
    GLB u64 *out = (GLB u64 *)(uintptr_t)J.out;
    u32 crc[3], adler[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        crc[p] = (u32)acc[p * 4] ^ hvq_gf_mul(0xFFFFFFFFu, J.xlen[p]) ^ 0xFFFFFFFFu;
        adler[p] = hvq_adler32_of_sums(acc[p * 4 + 1], acc[p * 4 + 2], 16ull * J.units[p]);
    }
    const u32 crc_pic = hvq_crc32_combine_x(hvq_crc32_combine_x(crc[0], crc[1], J.xlen[1]), crc[2], J.xlen[2]);
    const u32 adler_pic = hvq_adler32_combine_u(hvq_adler32_combine_u(adler[0], adler[1], 16ull * J.units[1]), adler[2], 16ull * J.units[2]);
    out[0] = crc[0]; out[1] = crc[1]; out[2] = crc[2]; out[3] = crc_pic;
    out[4] = adler[0]; out[5] = adler[1]; out[6] = adler[2]; out[7] = adler_pic;
}

/* jobs_dev: HvqChecksumJob[njobs] in device memory; max_wgs = max over jobs of wg_first[3].  The accumulators the jobs point to are zero
 * when the first launch runs (the caller queues the memset in front of it on the same stream); the second launch writes every record. */
extern "C" hipError_t hvq_launch_checksums(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;
    if (max_wgs) {
        hipLaunchKernelGGL(hvq_checksum_kernel, dim3(max_wgs, (uint32_t)njobs), dim3(HVQ_CK_LANES), 0, stream, (const HvqChecksumJob *)jobs_dev);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hvq_checksum_finish_kernel, dim3(((uint32_t)njobs + 63u) / 64u), dim3(64), 0, stream, (const HvqChecksumJob *)jobs_dev, njobs);
    return hipGetLastError();
}
