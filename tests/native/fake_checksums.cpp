/*
 * tests/native/fake_checksums.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_checksums (hvqm4_amd/csrc/hvq_checksum.hip) for the CPU
 * fake device.  Linked into the checksum driver only (tests/test_checksums_cpu.py); the other drivers link without it, and the runtime's
 * weak reference then makes hvq_picture_checksums refuse.
 *
 * The launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_checksum_kernel does
 * (pictures x workgroups, the record's plane mapping, chunks counted from the plane's end), reaches every byte through fake_span at that
 * moment, steps the CRC register one bit at a time, XORS and ADDS into the accumulator as the kernel's atomics do -- an accumulator that
 * was not zeroed in front of the launch shows in the values -- and then finishes every record as hvq_checksum_finish_kernel does.
 */
#include "fake_device.h"

#include <cstdint>
#include <cstdlib>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_checksum.h"

extern "C" hipError_t hvq_launch_checksums(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;                              /* hvq_launch_checksums: one grid row per picture */
    return fake_enqueue(stream, "checksums", [=]() {
        const HvqChecksumJob *jobs = (const HvqChecksumJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqChecksumJob), "checksums: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqChecksumJob &J = jobs[k];
            if (J.a & 15u) fake_die("checksums: job %d: the picture is not 16-byte aligned (the kernel loads 16-byte units)", k);
            if ((J.out | J.acc) & 7u) fake_die("checksums: job %d: the record or the accumulator is not 8-byte aligned (64-bit atomics and stores)", k);
            if (J.wg_first[0] != 0 || J.wg_first[3] > max_wgs) fake_die("checksums: job %d needs %u workgroups, the grid has %u per picture", k, J.wg_first[3], max_wgs);
            uint64_t *acc = (uint64_t *)fake_span((const void *)(uintptr_t)J.acc, 96, "checksums: an accumulator");
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= J.wg_first[3]) break;                                  /* hvq_checksum_kernel: workgroups past the picture leave */
                const uint32_t p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);
                if (J.plane_off[p] & 15u) fake_die("checksums: job %d: plane %u does not start on a 16-byte boundary", k, p);
                if (J.units[p] > HVQ_CK_MAX_UNITS) fake_die("checksums: job %d: plane %u has %u units", k, p, J.units[p]);
                const uint64_t c = wg - J.wg_first[p];                           /* whole chunks behind this one */
                if (c * HVQ_CK_CHUNK >= J.units[p]) fake_die("checksums: job %d: workgroup %u of plane %u lies in front of the plane's %u units", k, wg, p, J.units[p]);
                const uint64_t last = J.units[p] - c * HVQ_CK_CHUNK, first = last > HVQ_CK_CHUNK ? last - HVQ_CK_CHUNK : 0;
                const size_t off = (size_t)J.plane_off[p] + (size_t)first * 16u, len = (size_t)(last - first) * 16u;
                const uint8_t *a = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.a + off), len, "checksums: a workgroup's units of the picture");
                const uint64_t behind = c * HVQ_CK_CHUNK * 16u;                  /* bytes of the plane behind this chunk */
                uint64_t s = 0, w = 0;
                for (size_t i = 0; i < len; ++i) { s += a[i]; w += (uint64_t)a[i] * (behind + (len - i)); }
                const uint32_t r = hvq_gf_mul(hvq_crc_raw(0u, a, len), hvq_gf_xpow8(behind));
                acc[p * 4u + 0] ^= r; acc[p * 4u + 1] += s; acc[p * 4u + 2] += w;
            }
            /* every unit of every plane belongs to exactly one workgroup */
            for (uint32_t p = 0; p < 3; ++p)
                if ((uint64_t)(J.wg_first[p + 1] - J.wg_first[p]) * HVQ_CK_CHUNK < J.units[p] ||
                    (J.units[p] && (uint64_t)(J.wg_first[p + 1] - J.wg_first[p] - 1u) * HVQ_CK_CHUNK >= J.units[p]))
                    fake_die("checksums: job %d: plane %u of %u units has %u workgroups", k, p, J.units[p], J.wg_first[p + 1] - J.wg_first[p]);
        }
        /* hvq_checksum_finish_kernel, behind every workgroup of the first launch */
        for (int k = 0; k < njobs; ++k) {
            const HvqChecksumJob &J = jobs[k];
            const uint64_t *acc = (const uint64_t *)fake_span((const void *)(uintptr_t)J.acc, 96, "checksums: an accumulator");
            uint64_t *out = (uint64_t *)fake_span((const void *)(uintptr_t)J.out, 64, "checksums: an output record");
            uint32_t crc[3], adler[3];
            for (int p = 0; p < 3; ++p) {
                if (acc[p * 4] >> 32) fake_die("checksums: job %d: plane %d: the high half of the CRC accumulator is not zero", k, p);
                crc[p] = (uint32_t)acc[p * 4] ^ hvq_gf_mul(0xFFFFFFFFu, J.xlen[p]) ^ 0xFFFFFFFFu;
                adler[p] = hvq_adler32_of_sums(acc[p * 4 + 1], acc[p * 4 + 2], 16ull * J.units[p]);
            }
            out[0] = crc[0]; out[1] = crc[1]; out[2] = crc[2];
            out[3] = hvq_crc32_combine_x(hvq_crc32_combine_x(crc[0], crc[1], J.xlen[1]), crc[2], J.xlen[2]);
            out[4] = adler[0]; out[5] = adler[1]; out[6] = adler[2];
            out[7] = hvq_adler32_combine_u(hvq_adler32_combine_u(adler[0], adler[1], 16ull * J.units[1]), adler[2], 16ull * J.units[2]);
        }
    });
}
