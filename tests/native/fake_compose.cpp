/*
 * tests/native/fake_compose.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_compose (hvqm4_amd/csrc/hvq_compose.hip) for the CPU
 * fake device.  Linked into the compose driver only (tests/test_compose_cpu.py); the other drivers link without it, and the runtime's
 * weak reference then makes hvq_compose_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_compose_kernel does --
 * targets x planes x tiles, and within a tile lane by lane: the layers in order, the uniform skip of a layer that misses the tile, the
 * cover mask, the aligned body's one dword or the general body's two, the select of PUT, the finish, one dword store -- with the
 * kernel's own arithmetic of hvq_compose.h, and reaches every byte of the pictures through fake_span at that moment.  It dies on a load
 * outside the source plane, on a record that does not describe a layer (rectangles that leave their planes, a body that the rule of
 * hvq_cp_body does not allow: aligned where the numbers are not), on a cover mask of the aligned body that is neither empty nor whole,
 * and on a target byte that is stored other than once: a map of the plane counts the stores.  fake_compose_counts reports how many
 * layer planes ran through each body, for the test that compares them with the host rule.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_compose.h"

static uint64_t g_counts[2];                                                         /* layer planes met by a job: aligned, general */
extern "C" void fake_compose_counts(uint64_t out[2], int reset)
{
    out[0] = g_counts[0]; out[1] = g_counts[1];
    if (reset) g_counts[0] = g_counts[1] = 0;
}

namespace {

uint32_t load_dword(const HvqComposeRec &r, int32_t q, int k, int l)
{
    if (q < 0 || q >= hvq_cp_src_dwords(&r)) fake_die("compose: job %d, layer %d: dword %d lies outside the source plane of %d dwords", k, l, q, hvq_cp_src_dwords(&r));
    uint32_t v;
    memcpy(&v, fake_span((const void *)(uintptr_t)(r.src + (uint64_t)q * 4u), 4, "compose: a dword of a source plane"), 4);
    return v;
}

void check_rec(const HvqComposeJob &J, const HvqComposeRec &r, int k, int l)
{
    if (!r.pitch || !r.ny || r.pitch > 8192u || r.ny > 8192u || (r.pitch & 3u) || (r.src & 3u)) fake_die("compose: job %d, layer %d: a source plane of %u x %u at %#llx", k, l, r.pitch, r.ny, (unsigned long long)r.src);
    if (r.w < 1 || r.h < 1 || r.sx < 0 || r.sy < 0 || r.dx < 0 || r.dy < 0) fake_die("compose: job %d, layer %d: the rectangle %d, %d, %d x %d -> %d, %d", k, l, r.sx, r.sy, r.w, r.h, r.dx, r.dy);
    if ((uint32_t)(r.sx + r.w) > r.pitch || (uint32_t)(r.sy + r.h) > r.ny) fake_die("compose: job %d, layer %d: the rectangle leaves its %u x %u source plane", k, l, r.pitch, r.ny);
    if ((uint32_t)(r.dx + r.w) > J.mx || (uint32_t)(r.dy + r.h) > J.my) fake_die("compose: job %d, layer %d: the rectangle leaves the %u x %u target plane", k, l, J.mx, J.my);
    if (r.mode != HVQ_CP_PUT && r.mode != HVQ_CP_ADD) fake_die("compose: job %d, layer %d: mode %u", k, l, r.mode);
    if (r.body != HVQ_CP_ALIGNED && r.body != HVQ_CP_GENERAL) fake_die("compose: job %d, layer %d: body %u", k, l, r.body);
    if (r.body == HVQ_CP_ALIGNED && hvq_cp_body(r.sx, r.dx, r.w, 0) != HVQ_CP_ALIGNED) fake_die("compose: job %d, layer %d: the aligned body for %d -> %d, %d wide", k, l, r.sx, r.dx, r.w);
    if (r.weight > HVQ_CP_MAX_GAIN || r.weight < -HVQ_CP_MAX_GAIN) fake_die("compose: job %d, layer %d: weight %d", k, l, r.weight);
}

}

extern "C" hipError_t hvq_launch_compose(const void *tab_dev, int ntargets, uint32_t max_tiles, hipStream_t stream)
{
    if (ntargets <= 0 || !max_tiles) return hipSuccess;
    if (ntargets > 65535) return hipErrorInvalidValue;                               /* hvq_launch_compose: one grid row per target */
    return fake_enqueue(stream, "compose", [=]() {
        const int njobs = 3 * ntargets;
        const HvqComposeJob *jobs = (const HvqComposeJob *)fake_span(tab_dev, (size_t)njobs * sizeof(HvqComposeJob), "compose: the job records");
        uint32_t nrecs = 0;
        for (int k = 0; k < njobs; ++k) if (jobs[k].count) nrecs = std::max(nrecs, 3u * (jobs[k].first + jobs[k].count));
        const HvqComposeRec *recs = nullptr;
        if (nrecs) recs = (const HvqComposeRec *)((const uint8_t *)fake_span(tab_dev, (size_t)njobs * sizeof(HvqComposeJob) + (size_t)nrecs * sizeof(HvqComposeRec), "compose: the layer records") +
                                                  (size_t)njobs * sizeof(HvqComposeJob));
        for (int k = 0; k < njobs; ++k) {
            const HvqComposeJob &J = jobs[k];
            if (!J.mx || !J.my || J.mx > 8192u || J.my > 8192u || (J.mx & 3u) || (J.dst & 3u)) fake_die("compose: job %d: %u x %u at %#llx", k, J.mx, J.my, (unsigned long long)J.dst);
            if (J.plane != (uint32_t)(k % 3) || J.count > 256u) fake_die("compose: job %d: plane %u, %u layers", k, J.plane, J.count);
            if (J.shift < 0 || J.shift > 22 || J.half != (J.shift ? 1 << (J.shift - 1) : 0) || J.bias < -255 || J.bias > 255) fake_die("compose: job %d: shift %d, half %d, bias %d", k, J.shift, J.half, J.bias);
            if (J.tiles_x != (J.mx + HVQ_CP_TW - 1u) / HVQ_CP_TW || J.tiles != J.tiles_x * ((J.my + HVQ_CP_TH - 1u) / HVQ_CP_TH)) fake_die("compose: job %d: the tiles do not describe %u x %u", k, J.mx, J.my);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("compose: target %d needs %u tiles, the grid has %u per target", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            if (k % 3 && (J.first != jobs[k - 1].first || J.count != jobs[k - 1].count || J.shift != jobs[k - 1].shift)) fake_die("compose: job %d: the planes of a target differ", k);
            int64_t gain = 0;
            for (uint32_t l = 0; l < J.count; ++l) {
                const HvqComposeRec &r = recs[3u * (J.first + l) + J.plane];
                check_rec(J, r, k, (int)l);
                gain += r.weight < 0 ? -(int64_t)r.weight : r.weight;
                ++g_counts[r.body == HVQ_CP_GENERAL];
            }
            if (gain > HVQ_CP_MAX_GAIN) fake_die("compose: job %d: a gain of %lld", k, (long long)gain);
            std::vector<uint8_t> stored((size_t)J.mx * J.my, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * HVQ_CP_TW, r0 = ty * HVQ_CP_TH;
                for (uint32_t lane = 0; lane < HVQ_CP_LANES; ++lane) {
                    const int32_t x = (int32_t)(c0 + (lane & 15u) * 4u), y = (int32_t)(r0 + (lane >> 4));
                    int32_t acc[4] = { 0, 0, 0, 0 };
                    for (uint32_t l = 0; l < J.count; ++l) {
                        const HvqComposeRec &r = recs[3u * (J.first + l) + J.plane];
                        if (hvq_cp_misses(&r, c0, r0)) continue;
                        const uint32_t m = hvq_cp_cover(&r, x, y);
                        const int32_t a = hvq_cp_src_byte(&r, x, y);
                        uint32_t s = 0;
                        if (r.body == HVQ_CP_ALIGNED) {
                            if (m != 0u && m != 15u) fake_die("compose: job %d, layer %u: the aligned body meets the cover mask %u", k, l, m);
                            if (m && (a & 3)) fake_die("compose: job %d, layer %u: the aligned body meets source byte %d", k, l, a);
                            if (m) s = load_dword(r, a >> 2, k, (int)l);
                        } else if (m) {
                            const int32_t q = a >> 2, n = hvq_cp_src_dwords(&r);
                            uint32_t lo = 0, hi = 0;
                            if (q >= 0 && q < n) lo = load_dword(r, q, k, (int)l);
                            if ((a & 3) && q + 1 >= 0 && q + 1 < n) hi = load_dword(r, q + 1, k, (int)l);
                            s = hvq_cp_funnel(lo, hi, (uint32_t)a);
                            for (int32_t i = 0; i < 4; ++i)                          /* a covered byte comes from a dword that was loaded */
                                if ((m >> i & 1u) && (((a + i) >> 2) < 0 || ((a + i) >> 2) >= n)) fake_die("compose: job %d, layer %u: covered byte %d lies outside the source plane", k, l, a + i);
                        }
                        for (uint32_t i = 0; i < 4u; ++i) acc[i] = hvq_cp_step(acc[i], m >> i & 1u, r.mode == HVQ_CP_PUT, r.weight, s >> (8u * i) & 255u);
                    }
                    if ((uint32_t)y < J.my && (uint32_t)x < J.mx) {
                        uint32_t out = 0;
                        for (uint32_t i = 0; i < 4u; ++i) out |= hvq_cp_finish(acc[i], J.half, J.shift, J.bias) << (8u * i);
                        memcpy((void *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)(uint32_t)y * J.mx + (uint32_t)x), 4, "compose: a dword of the target plane"), &out, 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)y * J.mx + (uint32_t)x + i];
                    }
                }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("compose: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
