/*
 * tests/native/fake_metrics.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_metrics (hvqm4_amd/csrc/hvq_metrics.hip) for the CPU
 * fake device.  Linked into the metrics driver only (tests/test_metrics_cpu.py); the driver of tests/test_fake_device.py links without it,
 * and the runtime's weak reference then makes hvq_picture_metrics refuse.
 *
 * The launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_metrics_kernel does
 * (pairs x workgroups, the record's plane mapping), reaches every byte through fake_span at that moment, computes the four sums scalar
 * and ADDS them into the record as the kernel's atomics do: a record that was not zeroed in front of the launch shows in the values.
 */
#include "fake_device.h"

#include <cstdint>
#include <cstdlib>

#include "../../hvqm4_amd/csrc/hvq_desc.h"

extern "C" hipError_t hvq_launch_metrics(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0 || !max_wgs) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;                              /* hvq_launch_metrics: one grid row per pair */
    return fake_enqueue(stream, "metrics", [=]() {
        const HvqMetricsJob *jobs = (const HvqMetricsJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqMetricsJob), "metrics: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqMetricsJob &J = jobs[k];
            if ((J.a | J.b) & 15u) fake_die("metrics: job %d: a picture is not 16-byte aligned (the kernel loads 16-byte units)", k);
            if (J.out & 7u) fake_die("metrics: job %d: the record is not 8-byte aligned (64-bit atomics)", k);
            if (J.wg_first[0] != 0 || J.wg_first[3] > max_wgs) fake_die("metrics: job %d needs %u workgroups, the grid has %u per pair", k, J.wg_first[3], max_wgs);
            uint64_t *rec = (uint64_t *)fake_span((const void *)(uintptr_t)J.out, 96, "metrics: an output record");
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= J.wg_first[3]) break;                                  /* hvq_metrics_kernel: workgroups past the picture leave */
                const uint32_t p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);
                if (J.plane_off[p] & 15u) fake_die("metrics: job %d: plane %u does not start on a 16-byte boundary", k, p);
                const uint32_t first = (wg - J.wg_first[p]) * HVQ_MT_CHUNK;
                if (first >= J.units[p]) fake_die("metrics: job %d: workgroup %u of plane %u starts behind the plane's %u units", k, wg, p, J.units[p]);
                const uint32_t last = first + HVQ_MT_CHUNK < J.units[p] ? first + HVQ_MT_CHUNK : J.units[p];
                const size_t off = (size_t)J.plane_off[p] + (size_t)first * 16u, len = (size_t)(last - first) * 16u;
                const uint8_t *a = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.a + off), len, "metrics: a workgroup's units of picture a");
                const uint8_t *b = J.b ? (const uint8_t *)fake_span((const void *)(uintptr_t)(J.b + off), len, "metrics: a workgroup's units of the reference") : nullptr;
                uint64_t sa = 0, sb = 0, sad = 0, sse = 0;
                for (size_t i = 0; i < len; ++i) {
                    const int x = a[i], y = b ? b[i] : 0, d = x - y;
                    sa += (uint64_t)x; sb += (uint64_t)y; sad += (uint64_t)abs(d); sse += (uint64_t)(d * d);
                }
                rec[p * 4u + 0] += sa; rec[p * 4u + 1] += sb; rec[p * 4u + 2] += sad; rec[p * 4u + 3] += sse;
            }
            /* every unit of every plane belongs to exactly one workgroup */
            for (uint32_t p = 0; p < 3; ++p)
                if ((uint64_t)(J.wg_first[p + 1] - J.wg_first[p]) * HVQ_MT_CHUNK < J.units[p] ||
                    (J.units[p] && (uint64_t)(J.wg_first[p + 1] - J.wg_first[p] - 1u) * HVQ_MT_CHUNK >= J.units[p]))
                    fake_die("metrics: job %d: plane %u of %u units has %u workgroups", k, p, J.units[p], J.wg_first[p + 1] - J.wg_first[p]);
        }
    });
}
