/*
 * tests/native/fake_histograms.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_histograms (hvqm4_amd/csrc/hvq_histogram.hip) for the
 * CPU fake device.  Linked into the histogram driver only (tests/test_histograms_cpu.py); the other drivers link without it, and the
 * runtime's weak reference then makes hvq_picture_histograms refuse.
 *
 * The launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_histogram_kernel does
 * (pictures x workgroups, the record's plane mapping, HVQ_HG_CHUNK units a workgroup), reaches every byte through fake_span at that
 * moment, counts a workgroup's share in 256 bins of its own and ADDS the non-zero ones into the record as the kernel's atomics do -- a
 * record that was not zeroed in front of the launch shows in the values.
 */
#include "fake_device.h"

#include <cstdint>
#include <cstdlib>

#include "../../hvqm4_amd/csrc/hvq_desc.h"

extern "C" hipError_t hvq_launch_histograms(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;                              /* hvq_launch_histograms: one grid row per picture */
    return fake_enqueue(stream, "histograms", [=]() {
        const HvqHistogramJob *jobs = (const HvqHistogramJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqHistogramJob), "histograms: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqHistogramJob &J = jobs[k];
            if ((J.a | J.b) & 15u) fake_die("histograms: job %d: a picture is not 16-byte aligned (the kernel loads 16-byte units)", k);
            if (J.out & 3u) fake_die("histograms: job %d: the record is not 4-byte aligned (32-bit atomics)", k);
            if (J.wg_first[0] != 0 || J.wg_first[3] > max_wgs) fake_die("histograms: job %d needs %u workgroups, the grid has %u per picture", k, J.wg_first[3], max_wgs);
            uint32_t *out = (uint32_t *)fake_span((const void *)(uintptr_t)J.out, 3u * HVQ_HG_BINS * sizeof(uint32_t), "histograms: an output record");
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= J.wg_first[3]) break;                                  /* hvq_histogram_kernel: workgroups past the picture leave */
                const uint32_t p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);
                if (J.plane_off[p] & 15u) fake_die("histograms: job %d: plane %u does not start on a 16-byte boundary", k, p);
                if (J.units[p] > HVQ_HG_MAX_UNITS) fake_die("histograms: job %d: plane %u has %u units", k, p, J.units[p]);
                const uint64_t first = (uint64_t)(wg - J.wg_first[p]) * HVQ_HG_CHUNK;
                if (first >= J.units[p]) fake_die("histograms: job %d: workgroup %u of plane %u starts behind the plane's %u units", k, wg, p, J.units[p]);
                const uint64_t last = first + HVQ_HG_CHUNK < J.units[p] ? first + HVQ_HG_CHUNK : J.units[p];
                const size_t off = (size_t)J.plane_off[p] + (size_t)first * 16u, len = (size_t)(last - first) * 16u;
                const uint8_t *a = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.a + off), len, "histograms: a workgroup's units of the picture");
                const uint8_t *b = J.b ? (const uint8_t *)fake_span((const void *)(uintptr_t)(J.b + off), len, "histograms: a workgroup's units of the reference") : nullptr;
                uint32_t bins[HVQ_HG_BINS] = { 0 };
                for (size_t i = 0; i < len; ++i) bins[b ? (uint32_t)abs((int)a[i] - (int)b[i]) : a[i]]++;
                for (uint32_t v = 0; v < HVQ_HG_BINS; ++v)
                    if (bins[v]) out[p * HVQ_HG_BINS + v] += bins[v];
            }
            /* every unit of every plane belongs to exactly one workgroup */
            for (uint32_t p = 0; p < 3; ++p)
                if ((uint64_t)(J.wg_first[p + 1] - J.wg_first[p]) * HVQ_HG_CHUNK < J.units[p] ||
                    (J.units[p] && (uint64_t)(J.wg_first[p + 1] - J.wg_first[p] - 1u) * HVQ_HG_CHUNK >= J.units[p]))
                    fake_die("histograms: job %d: plane %u of %u units has %u workgroups", k, p, J.units[p], J.wg_first[p + 1] - J.wg_first[p]);
        }
    });
}
