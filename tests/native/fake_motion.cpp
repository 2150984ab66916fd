/*
 * tests/native/fake_motion.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_motion (hvqm4_amd/csrc/hvq_motion.hip) for the CPU fake
 * device.  Linked into the motion driver only (tests/test_motion_cpu.py); the other drivers link without it, and the runtime's weak
 * reference then makes hvq_picture_motion refuse.
 *
 * The launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_motion_kernel does
 * (pictures x tiles of HVQ_MV_TILE x HVQ_MV_TILE samples, the blocks of a tile), reaches every byte through fake_span at that moment --
 * the luma planes and the field, nothing else -- and searches every block with scalar loops: every candidate of the square whose block
 * lies inside the picture, the smallest packed key of hvq_desc.h.  It checks that every record is written exactly once.
 */
#include "fake_device.h"

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"

extern "C" hipError_t hvq_launch_motion(const void *jobs_dev, int njobs, uint32_t max_tiles, int block, int radius, hipStream_t stream)
{
    if (njobs <= 0 || !max_tiles) return hipSuccess;
    if (njobs > 65535 || (block != 8 && block != 16) || radius < 0 || radius > (int)HVQ_MV_MAX_RADIUS) return hipErrorInvalidValue;
    return fake_enqueue(stream, "motion", [=]() {
        const HvqMotionJob *jobs = (const HvqMotionJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqMotionJob), "motion: the job records");
        const int B = block, R = radius;
        for (int k = 0; k < njobs; ++k) {
            const HvqMotionJob &J = jobs[k];
            if ((J.a | J.b | J.out) & 15u) fake_die("motion: job %d: a plane or the field is not 16-byte aligned", k);
            if (!J.a || !J.b || !J.out) fake_die("motion: job %d: a null address", k);
            if (!J.w || !J.h || J.w % (uint32_t)B || J.h % (uint32_t)B || J.w >= HVQ_MV_MAX_SIDE || J.h >= HVQ_MV_MAX_SIDE)
                fake_die("motion: job %d: %u x %u is not made of blocks of %d", k, J.w, J.h, B);
            if (J.rows != J.h / (uint32_t)B || J.cols != J.w / (uint32_t)B) fake_die("motion: job %d: %u x %u blocks for %u x %u samples", k, J.rows, J.cols, J.w, J.h);
            if (J.tiles_x != (J.w + HVQ_MV_TILE - 1u) / HVQ_MV_TILE || J.tiles != J.tiles_x * ((J.h + HVQ_MV_TILE - 1u) / HVQ_MV_TILE) || J.tiles > max_tiles)
                fake_die("motion: job %d: %u tiles, %u a row, the grid has %u per picture", k, J.tiles, J.tiles_x, max_tiles);
            const int W = (int)J.w, H = (int)J.h;
            const uint8_t *a = (const uint8_t *)fake_span((const void *)(uintptr_t)J.a, (size_t)W * H, "motion: the luma plane of the picture");
            const uint8_t *b = (const uint8_t *)fake_span((const void *)(uintptr_t)J.b, (size_t)W * H, "motion: the luma plane of the reference");
            int32_t *out = (int32_t *)fake_span((const void *)(uintptr_t)J.out, (size_t)J.rows * J.cols * 16u, "motion: the field");
            std::vector<uint8_t> written((size_t)J.rows * J.cols, 0);
            const uint32_t nbt = HVQ_MV_TILE / (uint32_t)B;
            for (uint32_t t = 0; t < max_tiles; ++t) {
                if (t >= J.tiles) break;                                         /* hvq_motion_kernel: workgroups past the picture leave */
                const uint32_t ty = t / J.tiles_x, tx = t % J.tiles_x;
                for (uint32_t bi = 0; bi < nbt * nbt; ++bi) {
                    const uint32_t r = ty * nbt + bi / nbt, c = tx * nbt + bi % nbt;
                    if (r >= J.rows || c >= J.cols) continue;
                    const int y0 = (int)r * B, x0 = (int)c * B;
                    uint32_t best = ~0u, cz = ~0u;
                    for (int dy = -R; dy <= R; ++dy) {
                        if (y0 + dy < 0 || y0 + dy + B > H) continue;
                        for (int dx = -R; dx <= R; ++dx) {
                            if (x0 + dx < 0 || x0 + dx + B > W) continue;
                            uint32_t cost = 0;
                            for (int i = 0; i < B; ++i)
                                for (int j = 0; j < B; ++j)
                                    cost += (uint32_t)abs((int)a[(size_t)(y0 + i) * W + x0 + j] - (int)b[(size_t)(y0 + dy + i) * W + x0 + dx + j]);
                            const uint32_t key = cost << 15 | (uint32_t)(abs(dy) + abs(dx)) << 10 | (uint32_t)(dy + R) << 5 | (uint32_t)(dx + R);
                            if (key < best) best = key;
                            if (!dy && !dx) cz = cost;
                        }
                    }
                    if (written[(size_t)r * J.cols + c]++) fake_die("motion: job %d: block (%u, %u) is written twice", k, r, c);
                    int32_t *rec = out + ((size_t)r * J.cols + c) * 4u;
                    rec[0] = (int32_t)((best >> 5) & 31u) - R; rec[1] = (int32_t)(best & 31u) - R; rec[2] = (int32_t)(best >> 15); rec[3] = (int32_t)cz;
                }
            }
            for (size_t i = 0; i < written.size(); ++i)
                if (!written[i]) fake_die("motion: job %d: block %zu of %u x %u is not written", k, i, J.rows, J.cols);
        }
    });
}
