/*
 * hvq_jpeg.hip -- baseline JPEG (JFIF) files of pictures for CDNA4 / gfx950 (MI355X): forward DCT, quantisation, Huffman coding, bit
 * packing and byte stuffing into a variable-length output, byte for byte the file of include/hvqm4_amd.h (hvq_encode_jpeg: the
 * specification).  One call serves any number of pictures of any sizes and samplings.
 *
 * A unit of its own (its own Makefile rule and flags): the code of the other kernels does not change with it.
 *
 * No workgroup waits for another inside a launch: no flags, no spinning, no look-back.  The restart interval of the specification (one
 * MCU row) makes every MCU row an independent, byte-aligned piece of the file, and where a piece lies is settled BETWEEN launches:
 *   1. measure   grid (largest mh of the call, n), workgroups past a picture's last interval leave.  A workgroup codes its interval
 *                exactly as the emit launch will and writes only the interval's stuffed byte length, one dword of the context's scratch.
 *   2. lay out   grid n, one wave a picture: the prefix sum of the interval lengths (and of the two bytes of an RST marker behind all
 *                but the last) replaces the lengths by offsets into the file; lengths[i] is written; when the file fits its capacity
 *                the header (built on the host, shipped behind the job table) is copied in front and EOI written at the end, and the
 *                picture's first scratch dword says so.
 *   3. emit      the same coding as 1, now storing each interval's bytes and its RST marker at its offset -- nothing when the file
 *                does not fit.  Recomputing the transform costs arithmetic; keeping coded intervals between the launches would cost a
 *                worst-case scratch of 6.5 bytes a sample.
 *
 * Coding an interval.  A workgroup of HVQ_JP_LANES lanes takes HVQ_JP_LANES / (hs vs + 2) whole MCUs a chunk, one lane an 8 x 8 block
 * (the blocks of an MCU in coding order are neighbouring lanes); a wide picture takes several chunks, the bit position, the partial last
 * byte and the three DC predictors carried from one to the next.  Per chunk:
 *   a. a lane loads its block as 16 dwords (a dword beyond the plane's last column repeats that column's sample, a row beyond the last
 *      row repeats it: pitches are multiples of 4, blocks start on multiples of 8, a dword is inside or outside as a whole), transforms it
 *      in registers (even/odd halves of the table: the same integers as the full sums) and stores the quantised coefficients in zigzag
 *      order as 16-bit values into LDS, [k][lane]: the scans below index LDS, not a register file -- no private memory -- and keeps a
 *      64-bit mask of the coefficients that are not zero: the scans visit only those (runs are differences of bit positions);
 *   b. it counts the bits of its block; a prefix sum over the lanes gives every block its bit position;
 *   c. it ORs its codes into the chunk's bit buffer in LDS with ds_or_b32 (a code of up to 26 bits touches two dwords; which lane comes
 *      first does not matter); the buffer holds the stream big-endian inside dwords: stream byte i is byte i ^ 3 of it;
 *   d. the whole bytes of the chunk are divided evenly among the lanes, a second prefix sum over each lane's count of 0xFF bytes gives
 *      its first output byte, and (emit) it stores its bytes, a zero behind every 0xFF, with byte stores: two workgroups may own bytes of
 *      one output dword, and the output is never read.
 * Static LDS: 16 KB of coefficients, 26 KB of bit buffer (128 blocks of 64 x 26 bits: the bound of the header text), 3 KB of tables.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvq_desc.h"
#include "hvq_jpeg.h"

typedef uint32_t u32;
typedef uint64_t u64;
#define GLB __attribute__((address_space(1)))           /* global_load / global_store, never flat (hvq_kernels.hip) */

#define JP_L HVQ_JP_LANES
#define JP_BITBUF (JP_L * 64u * HVQ_JPEG_CODE_BITS / 32u + 2u)        /* dwords: the chunk's bits, the carried bits, one dword of slack for put() */
static_assert(JP_L == 128u, "two waves: block_scan");

/* zigzag position of a natural index */
struct Izz { uint8_t v[64]; };
constexpr Izz make_izz() { Izz z = {}; for (int k = 0; k < 64; ++k) z.v[HVQ_JPEG_ZZ[k]] = (uint8_t)k; return z; }
static constexpr Izz IZZ = make_izz();

struct Shared {
    int16_t coef[64u * JP_L];
    u32 bits[JP_BITBUF];
    u32 ac[2][256];
    u32 dc[2][16];
    u32 q[2][64];
    int dcv[JP_L];
    int carry[4];
    u32 wsum[2];
};
static_assert(sizeof(Shared) <= 65536u, "static LDS of a workgroup");

__device__ __forceinline__ u32 wave_scan(u32 v)
{
    const u32 lane = threadIdx.x & 63u;
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        const u32 o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

/* exclusive prefix sum over the workgroup's 128 lanes and the total; two barriers: what was written before it is visible behind it */
__device__ __forceinline__ u32 block_scan(u32 v, u32 *wsum, u32 *total)
{
    const u32 inc = wave_scan(v);
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    const u32 w0 = wsum[0], w1 = wsum[1];
    __syncthreads();
    *total = w0 + w1;
    return (threadIdx.x >> 6 ? w0 : 0u) + inc - v;
}

/* `len` bits of `code` at bit `pos` of the big-endian stream in dwords */
__device__ __forceinline__ void put(u32 *bits, u32 pos, u32 code, u32 len)
{
    const u64 v = (u64)code << (64u - (pos & 31u) - len);
    atomicOr(&bits[pos >> 5], (u32)(v >> 32));
    if ((u32)v) atomicOr(&bits[(pos >> 5) + 1u], (u32)v);
}

/* one pass over a block's coefficients in LDS: counts its bits, and with PUT writes them at `pos` */
template <bool PUT>
__device__ __forceinline__ u32 code_block(Shared &S, u32 t, u32 tab, int diff, u64 nz, u32 pos)
{
    const u32 p0 = pos;
    {
        const u32 sz = 32u - (u32)__clz(diff < 0 ? -diff : diff);              /* __clz(0) = 32: size 0 */
        const u32 c = S.dc[tab][sz];
        if (PUT) {
            put(S.bits, pos, c >> 8, c & 255u);
            if (sz) put(S.bits, pos + (c & 255u), (u32)(diff < 0 ? diff + (1 << sz) - 1 : diff), sz);
        }
        pos += (c & 255u) + sz;
    }
    u64 m = nz & ~1ull;                                                    /* the AC coefficients that are not zero: the scan visits only those */
    u32 prev = 0;
    while (m) {
        const u32 k = (u32)__builtin_ctzll(m);
        m &= m - 1ull;
        u32 run = k - prev - 1u;
        prev = k;
        const int v = S.coef[k * JP_L + t];
        while (run >= 16u) {
            const u32 z = S.ac[tab][0xF0];
            if (PUT) put(S.bits, pos, z >> 8, z & 255u);
            pos += z & 255u;
            run -= 16u;
        }
        const u32 sz = 32u - (u32)__clz(v < 0 ? -v : v);
        const u32 c = S.ac[tab][run << 4 | sz];
        /* the code and the value bits as one field of at most 26 bits */
        if (PUT) put(S.bits, pos, (c >> 8) << sz | (u32)(v < 0 ? v + (1 << sz) - 1 : v), (c & 255u) + sz);
        pos += (c & 255u) + sz;
    }
    if (!(nz >> 63)) {                                                     /* coefficient 63 is zero: EOB */
        const u32 e = S.ac[tab][0];
        if (PUT) put(S.bits, pos, e >> 8, e & 255u);
        pos += e & 255u;
    }
    return pos - p0;
}

/* the lane's block: load with edge replication, DCT, quantise, coefficients into LDS in zigzag order */
__device__ __forceinline__ u64 transform_block(Shared &S, u32 t, const uint8_t GLB *plane, u32 pw, u32 ph, u32 x0, u32 y0, u32 tab)
{
    int r[8][8];
    u64 nz = 0;                                                            /* bit k: coefficient k of the zigzag order is not zero */
    const bool in0 = x0 + 4u <= pw, in1 = x0 + 8u <= pw;
#pragma unroll
    for (u32 y = 0; y < 8u; ++y) {
        const u32 yy = y0 + y < ph ? y0 + y : ph - 1u;
        const uint8_t GLB *row = plane + (size_t)yy * pw;
        const u32 edge = (u32)row[pw - 1u] * 0x01010101u;
        const u32 d0 = in0 ? *(const u32 GLB *)(row + x0) : edge;
        const u32 d1 = in1 ? *(const u32 GLB *)(row + x0 + 4u) : edge;
        int x[8];
#pragma unroll
        for (u32 n = 0; n < 4u; ++n) { x[n] = (int)(d0 >> (8u * n) & 255u) - 128; x[4u + n] = (int)(d1 >> (8u * n) & 255u) - 128; }
        int s[4], d[4];
#pragma unroll
        for (u32 n = 0; n < 4u; ++n) { s[n] = x[n] + x[7u - n]; d[n] = x[n] - x[7u - n]; }
#pragma unroll
        for (u32 k = 0; k < 8u; ++k) {
            int a = 1024;
#pragma unroll
            for (u32 n = 0; n < 4u; ++n) a += HVQ_JPEG_C[k][n] * (k & 1u ? d[n] : s[n]);
            r[y][k] = a >> 11;
        }
    }
#pragma unroll
    for (u32 l = 0; l < 8u; ++l) {
        int s[4], d[4];
#pragma unroll
        for (u32 y = 0; y < 4u; ++y) { s[y] = r[y][l] + r[7u - y][l]; d[y] = r[y][l] - r[7u - y][l]; }
#pragma unroll
        for (u32 k = 0; k < 8u; ++k) {
            int a = 16384;
#pragma unroll
            for (u32 y = 0; y < 4u; ++y) a += HVQ_JPEG_C[k][y] * (k & 1u ? d[y] : s[y]);
            const int v = hvq_jpeg_quantise(a >> 15, S.q[tab][k * 8u + l]);
            S.coef[(u32)IZZ.v[k * 8u + l] * JP_L + t] = (int16_t)v;
            if (v) nz |= 1ull << IZZ.v[k * 8u + l];
            if (k == 0 && l == 0) S.dcv[t] = v;
        }
    }
    return nz;
}

template <bool EMIT>
__global__ __launch_bounds__(JP_L) void hvq_jpeg_code_kernel(const HvqJpegJob *__restrict__ jobs, const HvqJpegQuant *__restrict__ quant, u32 *__restrict__ scr)
{
    __shared__ Shared S;
    const HvqJpegJob &J = jobs[blockIdx.y];
    const u32 j = blockIdx.x, t = threadIdx.x;
    if (j >= J.mh) return;                                                /* workgroups past the picture's last interval leave */
    u32 off = 0;
    if (EMIT) {
        if (!scr[J.scr_first]) return;                                    /* the file does not fit: nothing of it is written */
        off = scr[J.scr_first + 1u + j];
    }
    for (u32 i = t; i < 512u; i += JP_L) (&S.ac[0][0])[i] = (&HVQ_JPEG_CODES.ac[0][0])[i];
    if (t < 32u) (&S.dc[0][0])[t] = (&HVQ_JPEG_CODES.dc[0][0])[t];
    (&S.q[0][0])[t] = (&quant->q[0][0])[t];
    if (t < 4u) S.carry[t] = 0;
    const u32 w = J.w, h = J.h, hs = J.hs, vs = J.vs, mw = J.mw;
    const u32 hv = hs * vs, bpm = hv + 2u, mpc = JP_L / bpm, nch = (mw + mpc - 1u) / mpc;
    const u32 cw = w / hs, ch = h / vs;
    const u32 mi = t / bpm, b = t - mi * bpm;
    const u32 comp = b < hv ? 0u : b - hv + 1u, tab = comp ? 1u : 0u;
    /* the lane whose block precedes this one in its component: the MCU's previous Y block, or the same block of the MCU before */
    const u32 pred = comp == 0u && b > 0u ? t - 1u : comp == 0u ? t - bpm + hv - 1u : t - bpm;
    const uint8_t GLB *src = (const uint8_t GLB *)J.src;
    const uint8_t GLB *plane = comp == 0u ? src : comp == 1u ? src + (size_t)w * h : src + (size_t)w * h + (size_t)cw * ch;
    const u32 pw = comp ? cw : w, ph = comp ? ch : h;
    uint8_t GLB *out = (uint8_t GLB *)J.out;
    u32 cb = 0, cval = 0, outpos = 0;                                     /* bits carried into the chunk (< 8), their value, stuffed bytes so far */
    __syncthreads();
    for (u32 c = 0; c < nch; ++c) {
        const u32 mx = c * mpc + mi;
        const bool active = mi < mpc && mx < mw;
        u64 nz = 0;
        if (active) {
            const u32 bx = comp ? mx : mx * hs + b % hs, by = comp ? j : j * vs + b / hs;
            nz = transform_block(S, t, plane, pw, ph, bx * 8u, by * 8u, tab);
        }
        __syncthreads();
        int diff = 0;
        u32 nbits = 0;
        if (active) {
            diff = S.dcv[t] - (mi || (comp == 0u && b > 0u) ? S.dcv[pred] : S.carry[comp]);       /* the chunk's first MCU: only its later Y blocks have a predecessor in it */
            nbits = code_block<false>(S, t, tab, diff, nz, 0u);
        }
        u32 total;
        const u32 start = cb + block_scan(nbits, S.wsum, &total);
        /* the predictors the next chunk starts from: the chunk's last MCU (read above, in front of the scan's barriers) */
        const u32 last_mx = (c + 1u) * mpc < mw ? (c + 1u) * mpc - 1u : mw - 1u;
        if (active && mx == last_mx && (comp || b == hv - 1u)) S.carry[comp] = S.dcv[t];
        const bool last = c + 1u == nch;
        const u32 totbits = cb + total, padded = last ? (totbits + 7u) & ~7u : totbits;
        const u32 ndw = (padded + 31u) / 32u + 1u;
        for (u32 i = t; i < ndw; i += JP_L) S.bits[i] = i == 0u && cb ? cval << (32u - cb) : 0u;
        __syncthreads();
        if (active) code_block<true>(S, t, tab, diff, nz, start);
        if (t == 0u && padded != totbits) put(S.bits, totbits, (1u << (padded - totbits)) - 1u, padded - totbits);     /* 1-bits up to the byte */
        __syncthreads();
        const u32 nb = padded >> 3;
        const uint8_t *bytes = (const uint8_t *)S.bits;
        cb = padded & 7u;
        cval = cb ? (u32)bytes[nb ^ 3u] >> (8u - cb) : 0u;
        /* stuffing: the lane's share of the chunk's whole bytes */
        const u32 per = (nb + JP_L - 1u) / JP_L;
        const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
        u32 ff = 0;
        for (u32 i = lo; i < hi; ++i) ff += bytes[i ^ 3u] == 0xFFu;
        u32 allff;
        const u32 before = block_scan(ff, S.wsum, &allff);
        if (EMIT) {
            uint8_t GLB *o = out + off + outpos + lo + before;
            for (u32 i = lo; i < hi; ++i) {
                const uint8_t v = bytes[i ^ 3u];
                *o++ = v;
                if (v == 0xFFu) *o++ = 0;
            }
        }
        outpos += nb + allff;
        __syncthreads();                                                  /* the next chunk's lanes overwrite what this one's still read */
    }
    if (t == 0u) {
        if (!EMIT) scr[J.scr_first + 1u + j] = outpos;
        else if (j + 1u < J.mh) { out[off + outpos] = 0xFF; out[off + outpos + 1u] = (uint8_t)(0xD0u + (j & 7u)); }
    }
}

/* one wave a picture: interval lengths -> offsets, the file's length, and when it fits the header and EOI */
__global__ __launch_bounds__(64) void hvq_jpeg_layout_kernel(const HvqJpegJob *__restrict__ jobs, u32 *__restrict__ scr)
{
    const HvqJpegJob &J = jobs[blockIdx.x];
    const u32 lane = threadIdx.x, mh = J.mh;
    u32 *iv = scr + J.scr_first + 1u;
    u32 running = HVQ_JPEG_HEADER_BYTES;
    for (u32 j0 = 0; j0 < mh; j0 += 64u) {
        const u32 j = j0 + lane;
        const u32 v = j < mh ? iv[j] + (j + 1u < mh ? 2u : 0u) : 0u;
        const u32 inc = wave_scan(v);
        if (j < mh) iv[j] = running + inc - v;
        running += __shfl(inc, 63);
    }
    const u64 total = (u64)running + 2u;
    const bool fits = total <= J.cap;
    if (lane == 0u) { *(u64 GLB *)J.len = total; scr[J.scr_first] = fits; }
    if (!fits) return;
    uint8_t GLB *out = (uint8_t GLB *)J.out;
    const uint8_t GLB *hdr = (const uint8_t GLB *)jobs + J.hdr_off;
    for (u32 i = lane; i < HVQ_JPEG_HEADER_BYTES; i += 64u) out[i] = hdr[i];
    if (lane < 2u) out[total - 2u + lane] = lane ? 0xD9 : 0xFF;
}

/* the three launches of a call, on one stream: njobs pictures, the largest mh among them, the quantisers quant_off bytes into the
 * table, the context's scratch */
extern "C" hipError_t hvq_launch_jpeg(const void *jobs_dev, int njobs, uint32_t max_mh, uint32_t quant_off, void *scratch, hipStream_t stream)
{
    if (njobs <= 0 || !max_mh) return hipSuccess;
    const HvqJpegJob *jobs = (const HvqJpegJob *)jobs_dev;
    const HvqJpegQuant *quant = (const HvqJpegQuant *)((const uint8_t *)jobs_dev + quant_off);
    const dim3 grid(max_mh, (unsigned)njobs);
    hipLaunchKernelGGL(hvq_jpeg_code_kernel<false>, grid, dim3(JP_L), 0, stream, jobs, quant, (u32 *)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hvq_jpeg_layout_kernel, dim3((unsigned)njobs), dim3(64), 0, stream, jobs, (u32 *)scratch);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hvq_jpeg_code_kernel<true>, grid, dim3(JP_L), 0, stream, jobs, quant, (u32 *)scratch);
    return hipGetLastError();
}
