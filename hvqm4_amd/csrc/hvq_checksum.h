/*
 * hvq_checksum.h -- the arithmetic hvq_picture_checksums rests on (include/hvqm4_amd.h), shared by the kernel (hvq_checksum.hip), the
 * runtime (hvq_runtime.cpp: the job records' constants, hvq_crc32_combine, hvq_adler32_combine) and the CPU fake device's body of the
 * launch.  C++ only; every function is constexpr, so the kernel's constants are computed by the compiler.
 *
 * CRC-32 as zlib computes it: reflected polynomial P = 0xEDB88320, a register whose bit 31 is x^0 and bit 0 is x^31.  One step of the
 * register, r = (r >> 1) ^ (P & -(r & 1)), multiplies it by x mod P.  R(M) is the register after the bytes M, started from 0, no final
 * xor: it is linear over GF(2) in M, leading zero bytes leave it 0, and
 *       R(A | B) = R(A) * x^(8 |B|)  ^  R(B)                      (* = hvq_gf_mul, the product mod P)
 *       crc32(M) = R(M)  ^  0xFFFFFFFF * x^(8 |M|)  ^  0xFFFFFFFF
 *       crc32(A | B) = crc32(A) * x^(8 |B|)  ^  crc32(B)
 * A little-endian dword d xored into a register of 0 and stepped 32 times is d * x^32.
 */
#ifndef HVQ_CHECKSUM_H
#define HVQ_CHECKSUM_H

#include <stdint.h>

#define HVQ_CRC_POLY   0xEDB88320u
#define HVQ_CRC_ONE    0x80000000u         /* x^0 */
#define HVQ_ADLER_BASE 65521u

/* a * b mod P.  With `b` a constant the compiler knows, the 32 values b * x^i fold into literals: 32 conditional xors are left. */
constexpr uint32_t hvq_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (HVQ_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

/* x^(8 * bytes) mod P, square and multiply */
constexpr uint32_t hvq_gf_xpow8(uint64_t bytes)
{
    uint32_t r = HVQ_CRC_ONE, sq = 0x00800000u;                /* sq = x^8 */
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) r = hvq_gf_mul(r, sq);
        sq = hvq_gf_mul(sq, sq);
    }
    return r;
}

/* the register after `len` more bytes, one bit at a time: what every faster byte step must equal */
constexpr uint32_t hvq_crc_raw(uint32_t r, const uint8_t *p, uint64_t len)
{
    for (uint64_t i = 0; i < len; ++i) {
        r ^= p[i];
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (HVQ_CRC_POLY & (0u - (r & 1u)));
    }
    return r;
}

/* zlib's crc32_combine: the CRC-32 of A | B from those of A and of B, |B| = len_b */
constexpr uint32_t hvq_crc32_combine_x(uint32_t crc_a, uint32_t crc_b, uint32_t xpow_len_b) { return hvq_gf_mul(crc_a, xpow_len_b) ^ crc_b; }

/* zlib's adler32_combine: the Adler-32 of A | B from those of A and of B, |B| = len_b */
constexpr uint32_t hvq_adler32_combine_u(uint32_t a, uint32_t b, uint64_t len_b)
{
    const uint64_t rem = len_b % HVQ_ADLER_BASE, a_lo = a & 0xFFFFu, a_hi = a >> 16, b_lo = b & 0xFFFFu, b_hi = b >> 16;
    const uint64_t lo = (a_lo + b_lo + HVQ_ADLER_BASE - 1u) % HVQ_ADLER_BASE;                      /* both count the seed 1 */
    const uint64_t hi = (rem * a_lo + a_hi + b_hi + HVQ_ADLER_BASE - rem) % HVQ_ADLER_BASE;        /* b's rows start from a_lo, not from 1 */
    return (uint32_t)(lo | (hi << 16));
}

/* Adler-32 of a plane of `len` bytes from its two exact sums: sum d_i and sum (len - i) d_i, i from 0 */
constexpr uint32_t hvq_adler32_of_sums(uint64_t sum, uint64_t wsum, uint64_t len)
{
    const uint64_t lo = (1u + sum % HVQ_ADLER_BASE) % HVQ_ADLER_BASE;
    const uint64_t hi = (len % HVQ_ADLER_BASE + wsum % HVQ_ADLER_BASE) % HVQ_ADLER_BASE;
    return (uint32_t)(lo | (hi << 16));
}

#endif
