/*
 * tests/native/fake_ssim.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_ssim (hvqm4_amd/csrc/hvq_ssim.hip) for the CPU fake device.
 * Linked into the SSIM driver only (tests/test_ssim_cpu.py); the drivers of tests/test_fake_device.py and tests/test_metrics_cpu.py link
 * without it, and the runtime's weak reference then makes hvq_picture_ssim refuse.
 *
 * The launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_ssim_kernel does (pairs x
 * workgroups, the record's plane and tile mapping), reaches every byte through fake_span at that moment -- sample rows of the tile's
 * blocks, the tile's rows of the map -- computes the window values scalar (include/hvqm4_amd.h) and ADDS sum_f and the number of windows
 * into the record as the kernel's atomics do: a record that was not zeroed in front of the launch shows in the values, and so does a
 * tiling that drops or repeats a window.
 */
#include "fake_device.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"

extern "C" hipError_t hvq_launch_ssim(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0 || !max_wgs) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;                              /* hvq_launch_ssim: one grid row per pair */
    return fake_enqueue(stream, "ssim", [=]() {
        const HvqSsimJob *jobs = (const HvqSsimJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqSsimJob), "ssim: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqSsimJob &J = jobs[k];
            if ((J.a | J.b) & 3u) fake_die("ssim: job %d: a picture is not 4-byte aligned (the kernel loads dwords)", k);
            if (!J.a || !J.b) fake_die("ssim: job %d: a picture is missing", k);
            if (J.out & 7u) fake_die("ssim: job %d: the record is not 8-byte aligned (64-bit atomics)", k);
            if (J.map & 3u) fake_die("ssim: job %d: the map is not 4-byte aligned", k);
            if (J.wg_first[0] != 0 || J.wg_first[3] > max_wgs) fake_die("ssim: job %d needs %u workgroups, the grid has %u per pair", k, J.wg_first[3], max_wgs);
            int64_t *rec = (int64_t *)fake_span((const void *)(uintptr_t)J.out, 48, "ssim: an output record");
            for (uint32_t p = 0; p < 3; ++p) {
                const uint32_t rows = J.bh[p] ? J.bh[p] - 1u : 0u, cols = J.bw[p] ? J.bw[p] - 1u : 0u;
                const uint32_t wgs = J.wg_first[p + 1] - J.wg_first[p];
                const uint32_t want = rows && cols ? ((rows + HVQ_SS_TR - 1u) / HVQ_SS_TR) * ((cols + HVQ_SS_TC - 1u) / HVQ_SS_TC) : 0u;
                if (wgs != want) fake_die("ssim: job %d: plane %u of %u x %u windows has %u workgroups, not %u", k, p, rows, cols, wgs, want);
                if (wgs && J.tiles_x[p] != (cols + HVQ_SS_TC - 1u) / HVQ_SS_TC) fake_die("ssim: job %d: plane %u has %u tiles per row", k, p, J.tiles_x[p]);
                if (J.plane_off[p] & 3u) fake_die("ssim: job %d: plane %u does not start on a 4-byte boundary", k, p);
            }
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= J.wg_first[3]) break;                                  /* hvq_ssim_kernel: workgroups past the pair leave */
                const uint32_t p = (wg >= J.wg_first[1]) + (wg >= J.wg_first[2]);
                const uint32_t tile = wg - J.wg_first[p], ty = tile / J.tiles_x[p], tx = tile % J.tiles_x[p];
                const uint32_t bw = J.bw[p], bh = J.bh[p], r0 = ty * HVQ_SS_TR, c0 = tx * HVQ_SS_TC;
                if (r0 + 1u >= bh || c0 + 1u >= bw) fake_die("ssim: job %d: workgroup %u of plane %u starts a tile without a window", k, wg, p);
                const uint32_t tbw = bw - c0 < HVQ_SS_TC + 1u ? bw - c0 : HVQ_SS_TC + 1u, tbh = bh - r0 < HVQ_SS_TR + 1u ? bh - r0 : HVQ_SS_TR + 1u;
                const size_t pitch = (size_t)bw * 4u;
                std::vector<int64_t> s1((size_t)tbw * tbh), s2(s1.size()), ss(s1.size()), s12(s1.size());
                for (uint32_t y = 0; y < tbh * 4u; ++y) {
                    const size_t off = (size_t)J.plane_off[p] + ((size_t)r0 * 4u + y) * pitch + (size_t)c0 * 4u;
                    const uint8_t *a = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.a + off), (size_t)tbw * 4u, "ssim: a sample row of a tile of picture a");
                    const uint8_t *b = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.b + off), (size_t)tbw * 4u, "ssim: a sample row of a tile of the reference");
                    for (uint32_t x = 0; x < tbw * 4u; ++x) {
                        const size_t i = (size_t)(y / 4u) * tbw + x / 4u;
                        const int64_t u = a[x], v = b[x];
                        s1[i] += u; s2[i] += v; ss[i] += u * u + v * v; s12[i] += u * v;
                    }
                }
                const uint32_t cols = bw - 1u;
                int64_t sum_f = 0, count = 0;
                for (uint32_t r = 0; r + 1u < tbh; ++r) {
                    float *row = J.map ? (float *)fake_span((const void *)(uintptr_t)(J.map + ((size_t)J.map_off[p] + (size_t)(r0 + r) * cols + c0) * 4u),
                                                            (size_t)(tbw - 1u) * 4u, "ssim: a tile's row of the map") : nullptr;
                    for (uint32_t c = 0; c + 1u < tbw; ++c) {
                        const size_t i = (size_t)r * tbw + c;
                        auto win = [&](const std::vector<int64_t> &v) { return v[i] + v[i + 1] + v[i + tbw] + v[i + tbw + 1]; };
                        const int64_t w1 = win(s1), w2 = win(s2), wss = win(ss), w12 = win(s12);
                        const int64_t vars = 64 * wss - w1 * w1 - w2 * w2, covar = 64 * w12 - w1 * w2;
                        const int64_t A = 2 * w1 * w2 + 416, B = 2 * covar + 235963, C = w1 * w1 + w2 * w2 + 416, D = vars + 235963;
                        if (llabs(A) >= (1ll << 30) || llabs(B) >= (1ll << 30) || llabs(C) >= (1ll << 30) || llabs(D) >= (1ll << 30))
                            fake_die("ssim: job %d: a window integer leaves 32 bits", k);
                        const float num = (float)(int32_t)A * (float)(int32_t)B, den = (float)(int32_t)C * (float)(int32_t)D;
                        const float q = num / den;
                        if (row) row[c] = q;
                        sum_f += (int64_t)nearbyintf(q * 16777216.0f);           /* the default rounding mode: half to even */
                        ++count;
                    }
                }
                rec[p * 2u + 0] += sum_f; rec[p * 2u + 1] += count;
            }
        }
    });
}
