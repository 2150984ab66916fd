/*
 * tests/native/fake_groups_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives the runtime (hvqm4_amd/csrc/hvq_runtime.cpp,
 * linked unchanged against the CPU fake device) through one flush of a batch large enough to be split into launch groups
 * (hvq_context_set_group_bytes).  It writes every picture it reads back and judges nothing: tests/test_launch_groups_fake.py compares
 * with the oracle and with the same batch in one group, and reads the order of the launches off the runtime's own
 * HVQM4_AMD_FLUSH_TIMING lines on stderr.
 *
 *   fake_groups_driver groups <outdir> <golden dir> <budget in bytes>
 *
 * The batch: 32 streams of 64 x 48 in 4:2:0, submitted in turns -- 31 of the GOP IPBBPBB (HVQM4 1.5 and 1.3 alternating) and, as stream 11,
 * one whose P pictures carry future-referencing macroblocks (pselfref64x48_15): its raster-order walk runs behind the launch of its own
 * group, level and queue.  Once host-parsed, once parsed on the device.
 *
 * results.txt, one fact per line:
 *   P <clip> <ordinal> <offset into pictures.bin> <bytes> <stream> <label>     a picture read back
 *   N <clip> <ordinal> <stream> <label>                                        a picture that is no longer resident (stream 11: four slots)
 *   G <label> <launch groups> <launches> <launch queues>                        of the flushed batch
 */
#define DRIVER_NAME "fake_groups_driver"
#include "fake_driver_common.h"

static FILE *g_bin;
static size_t g_bin_off = 0;

static void scenario_groups(unsigned long long budget)
{
    for (int dev = 0; dev < 2; ++dev) {
        const char *label = dev ? "groups/device" : "groups/host";
        HvqContext *ctx = nullptr;
        CHECK(hvq_context_create(0, &ctx));
        CHECK(hvq_context_set_group_bytes(ctx, budget));
        std::vector<std::pair<int, const Clip *>> sc;
        for (int s = 0; s < 32; ++s) {
            const Clip &c = clip(s == 11 ? "pselfref64x48_15" : (s & 1) ? "gop64x48_13" : "gop64x48_15");
            /* the self-reference clip in a ring of four slots: what its P pictures read as previous content is handed to a later picture soon
             * after, so a walk that ran a second time, behind another group's launch, would find it gone */
            const int sid = s == 11 ? hvq_stream_open(ctx, c.info.width, c.info.height, c.info.h_samp, c.info.v_samp, c.info.is_1_5, 4) : open_stream(ctx, c);
            CHECK(sid);
            sc.push_back({ sid, &c });
        }
        std::vector<int> sids, types;
        std::vector<const uint8_t *> pics;
        std::vector<size_t> lens;
        for (size_t k = 0;; ++k) {                         /* picture k of every stream, then k + 1 */
            bool any = false;
            for (auto &s : sc)
                if (k < s.second->pics.size()) {
                    const Pic &p = s.second->pics[k];
                    sids.push_back(s.first); types.push_back(p.type); pics.push_back(p.p); lens.push_back(p.len);
                    any = true;
                }
            if (!any) break;
        }
        const int n = (int)sids.size();
        if (dev) CHECK(hvq_submit_many_device(ctx, n, sids.data(), types.data(), pics.data(), lens.data(), nullptr));
        else CHECK(hvq_submit_many(ctx, n, sids.data(), types.data(), pics.data(), lens.data(), 3, nullptr));
        CHECK(hvq_flush(ctx));
        HvqStats st;
        CHECK(hvq_get_stats(ctx, &st));
        const int groups = hvq_context_launch_groups(ctx);
        CHECK(groups);
        fprintf(g_res, "G %s %d %u %u\n", label, groups, st.launches, st.launch_queues);
        for (auto &s : sc) {
            const uint32_t pb = hvq_stream_pic_bytes(ctx, s.first);
            for (int k = 0; k < (int)s.second->pics.size(); ++k) {
                std::vector<uint8_t> buf(pb);
                const int rc = hvq_read_picture(ctx, s.first, k, buf.data(), buf.size());
                if (rc == HVQ_E_STATE) { fprintf(g_res, "N %s %d %d %s\n", s.second->name.c_str(), k, s.first, label); continue; }   /* its slot was reused */
                CHECK(rc);
                fwrite(buf.data(), 1, pb, g_bin);
                fprintf(g_res, "P %s %d %zu %u %d %s\n", s.second->name.c_str(), k, g_bin_off, pb, s.first, label);
                g_bin_off += pb;
            }
        }
        hvq_context_destroy(ctx);
    }
}

int main(int argc, char **argv)
{
    if (argc < 5 || strcmp(argv[1], "groups")) { fprintf(stderr, "usage: " DRIVER_NAME " groups <outdir> <golden dir> <budget in bytes>\n"); return 2; }
    g_out = argv[2]; g_golden = argv[3];
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    g_bin = fopen((g_out + "/pictures.bin").c_str(), "wb");
    if (!g_res || !g_bin) { fprintf(stderr, DRIVER_NAME ": cannot write into %s\n", g_out.c_str()); return 2; }
    scenario_groups(strtoull(argv[4], nullptr, 10));
    fake_drain_all();
    fclose(g_res); fclose(g_bin);
    return 0;
}
