/*
 * tests/native/fake_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives the runtime (hvqm4_amd/csrc/hvq_runtime.cpp,
 * linked unchanged against the CPU fake device) through include/hvqm4_amd.h, scenario by scenario.  It writes every picture it reads back
 * and the export log into an output directory and judges nothing: tests/test_fake_device.py compares with the oracle.
 *
 *   fake_driver <scenario> <outdir> <golden dir> [corrupted picture file]
 *
 * results.txt, one fact per line:
 *   P <clip> <ordinal> <offset into pictures.bin> <bytes> <FNV-1a-64 of those bytes> <label>     a picture read back
 *   N <clip> <ordinal> <label>                                                                  a picture that reads as not resident
 *   E <clip> <ordinal> <FNV-1a-64 of the source planes when the export ran> <label>             one picture of one export launch
 *   R <label> <return code>                                                                     a return code the test wants to see
 *   X <export pictures asked for> <export pictures logged>
 * The caller-side resources of the exports (a stream, destination memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_driver"
#include "fake_driver_common.h"

static FILE *g_bin;
static size_t g_bin_off = 0;
struct Asked { std::string clip; int ordinal; std::string label; };
static std::vector<std::vector<Asked>> g_exports;              /* per export call, in call order */

static uint64_t fnv1a(const uint8_t *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

static void submit_host(HvqContext *ctx, int sid, const Clip &c)
{
    for (const Pic &p : c.pics) CHECK(hvq_stream_submit(ctx, sid, p.type, p.p, p.len));
}

/* the pictures of several (stream, clip) pairs as the arrays of the hvq_submit_many_* calls; by_turns: picture k of every stream, then k + 1 */
struct Many { std::vector<int> sids, types; std::vector<const uint8_t *> pics; std::vector<size_t> lens; };
static Many many_of(const std::vector<std::pair<int, const Clip *>> &sc, bool by_turns)
{
    Many m;
    auto add = [&](int sid, const Pic &p) { m.sids.push_back(sid); m.types.push_back(p.type); m.pics.push_back(p.p); m.lens.push_back(p.len); };
    if (!by_turns) { for (auto &s : sc) for (const Pic &p : s.second->pics) add(s.first, p); return m; }
    for (size_t k = 0;; ++k) {
        bool any = false;
        for (auto &s : sc) if (k < s.second->pics.size()) { add(s.first, s.second->pics[k]); any = true; }
        if (!any) break;
    }
    return m;
}

enum Form { FORM_COPY, FORM_ASYNC, FORM_ARENA };
static void submit_device(HvqContext *ctx, const Many &m, Form form)
{
    const int n = (int)m.sids.size();
    if (form == FORM_COPY) CHECK(hvq_submit_many_device(ctx, n, m.sids.data(), m.types.data(), m.pics.data(), m.lens.data(), nullptr));
    else if (form == FORM_ASYNC) CHECK(hvq_submit_many_device_async(ctx, n, m.sids.data(), m.types.data(), m.pics.data(), m.lens.data(), nullptr));
    else {
        std::vector<size_t> offs((size_t)n);
        size_t total = 0;
        for (int i = 0; i < n; ++i) { offs[(size_t)i] = total; total += hvq_arena_stride(m.lens[(size_t)i]); }
        void *base = nullptr;
        CHECK(hvq_arena_reserve(ctx, total, &base));
        for (int i = 0; i < n; ++i) memcpy((uint8_t *)base + offs[(size_t)i], m.pics[(size_t)i], m.lens[(size_t)i]);
        CHECK(hvq_submit_many_arena(ctx, n, m.sids.data(), m.types.data(), offs.data(), m.lens.data(), nullptr));
    }
}

/* read pictures [first, first + count) of a stream back; `clip_first` = the clip picture that ordinal `first` is */
static void read_back(HvqContext *ctx, int sid, const Clip &c, const char *label, int first = 0, int count = -1, int clip_first = 0, bool allow_gone = false)
{
    const uint32_t pb = hvq_stream_pic_bytes(ctx, sid);
    std::vector<uint8_t> buf(pb);
    if (count < 0) count = (int)c.pics.size();
    for (int k = 0; k < count; ++k) {
        const int rc = hvq_read_picture(ctx, sid, first + k, buf.data(), buf.size());
        if (rc == HVQ_E_STATE && allow_gone) { fprintf(g_res, "N %s %d %s\n", c.name.c_str(), clip_first + k, label); continue; }
        CHECK(rc);
        fwrite(buf.data(), 1, pb, g_bin);
        fprintf(g_res, "P %s %d %zu %u %016llx %s\n", c.name.c_str(), clip_first + k, g_bin_off, pb, (unsigned long long)fnv1a(buf.data(), pb), label);
        g_bin_off += pb;
    }
}

/* the same through hvq_read_pictures (read stream, gather kernel from four pictures on) */
static void read_back_bulk(HvqContext *ctx, int sid, const Clip &c, const char *label)
{
    const uint32_t pb = hvq_stream_pic_bytes(ctx, sid);
    const int n = (int)c.pics.size();
    uint8_t *pin = (uint8_t *)hvq_pinned_alloc((size_t)n * pb);
    if (!pin) exit(3);
    std::vector<int> sids((size_t)n, sid), ords((size_t)n);
    std::vector<void *> dst((size_t)n);
    for (int k = 0; k < n; ++k) { ords[(size_t)k] = k; dst[(size_t)k] = pin + (size_t)k * pb; }
    CHECK(hvq_read_pictures(ctx, n, sids.data(), ords.data(), dst.data()));
    for (int k = 0; k < n; ++k) {
        fwrite(pin + (size_t)k * pb, 1, pb, g_bin);
        fprintf(g_res, "P %s %d %zu %u %016llx %s\n", c.name.c_str(), k, g_bin_off, pb, (unsigned long long)fnv1a(pin + (size_t)k * pb, pb), label);
        g_bin_off += pb;
    }
    hvq_pinned_free(pin);
}

/* one export call over pictures [0, n) of several streams, 16 x 12 float32 each, on the caller's stream; kind: 0 tensors, 1 triangle filter, 2 RGB24 */
struct Exported { std::vector<void *> mem; };
static void export_pictures(HvqContext *ctx, const std::vector<std::pair<int, const Clip *>> &sc, hipStream_t caller, int kind, const char *label, Exported *keep)
{
    std::vector<int> sids, ords;
    std::vector<Asked> asked;
    for (auto &s : sc)
        for (int k = 0; k < (int)s.second->pics.size(); ++k) { sids.push_back(s.first); ords.push_back(k); asked.push_back(Asked{ s.second->name, k, label }); }
    const int n = (int)sids.size();
    const float mul[3] = { 1.f, 1.f, 1.f }, add[3] = { 0.f, 0.f, 0.f };
    if (kind == 2) {
        std::vector<HvqExportDst> dst((size_t)n);
        size_t i = 0;
        for (auto &s : sc)
            for (size_t k = 0; k < s.second->pics.size(); ++k, ++i) {
                void *d = nullptr;
                if (hipMalloc(&d, (size_t)s.second->info.width * s.second->info.height * 3u) != hipSuccess) exit(3);
                keep->mem.push_back(d);
                dst[i] = HvqExportDst{ d, 0, 0 };
            }
        CHECK(hvq_export_pictures(ctx, n, sids.data(), ords.data(), HVQ_FMT_RGB24, dst.data(), caller));
    } else {
        std::vector<HvqTensorDst> dst((size_t)n);
        for (int i = 0; i < n; ++i) {
            void *d = nullptr;
            if (hipMalloc(&d, 3u * 12u * 16u * 4u) != hipSuccess) exit(3);
            keep->mem.push_back(d);
            dst[(size_t)i] = HvqTensorDst{ d, 0, 0, 16, 12, 0, 0, 0, 0 };
        }
        if (kind == 0) CHECK(hvq_export_tensors(ctx, n, sids.data(), ords.data(), HVQ_T_F32, mul, add, dst.data(), caller));
        else CHECK(hvq_export_resampled(ctx, n, sids.data(), ords.data(), HVQ_T_F32, HVQ_FILTER_TRIANGLE, mul, add, dst.data(), caller));
    }
    g_exports.push_back(asked);
}

static void free_exported(Exported *e) { for (void *p : e->mem) (void)hipFree(p); e->mem.clear(); }

static const char *ALL[] = { "i16", "ip8", "ipb32", "gop64x48_15", "gop64x48_13", "portrait48x64", "portrait152x280", "nest_exact280x152", "wide296x160",
    "weird128x96", "weird64x64", "realistic128x96", "flat128x96", "ragged24x40", "twogops64x48", "natural128x96", "bigshift64x48", "yuv444_64x48",
    "yuv444_13_portrait48x64", "yuv444_296x160", "yuv422_64x48", "yuv422_13_portrait48x64", "yuv422_296x160", "weird160x128", "longescape64x48",
    "pselfref64x48_15", "pselfref64x48_13", "pselfref444_48x64", "pselfref422_64x48", "bigscalars64x64", "literals96x96", "crossplane420_64x48",
    "crossplane422_13_64x48", "crossplane444_48x64" };
static const char *SEVEN[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "yuv444_64x48", "ip8" };

/* every golden clip alone, once through each parse path */
static void scenario_clips(int part, int parts)
{
    int i = 0;
    for (const char *nm : ALL) {
        if (i++ % parts != part) continue;
        const Clip &c = clip(nm);
        for (int dev = 0; dev < 2; ++dev) {
            HvqContext *ctx = nullptr;
            CHECK(hvq_context_create(0, &ctx));
            const int sid = open_stream(ctx, c);
            if (dev) submit_device(ctx, many_of({ { sid, &c } }, false), FORM_COPY);
            else submit_host(ctx, sid, c);
            CHECK(hvq_flush(ctx));
            if (dev) read_back_bulk(ctx, sid, c, "clips/device");
            else read_back(ctx, sid, c, "clips/host");
            hvq_context_destroy(ctx);
        }
    }
}

/* the open, decode, export and close history of the GPU float export's `goldens` case */
static void goldens_history(HvqContext *ctx, hipStream_t caller)
{
    for (const char *nm : ALL) {
        const Clip &c = clip(nm);
        const int sid = open_stream(ctx, c);
        submit_host(ctx, sid, c);
        CHECK(hvq_flush(ctx));
        for (int dt = 0; dt < 3; ++dt) {
            Exported ex;
            export_pictures(ctx, { { sid, &c } }, caller, 0, "seven/history", &ex);
            if (hipStreamSynchronize(caller) != hipSuccess) exit(3);
            free_exported(&ex);
        }
        CHECK(hvq_stream_close(ctx, sid));
    }
}

/* seven tiny streams opened, submitted and flushed one after the other with nothing in between, one export over all, then the read-back */
static void scenario_seven(bool history)
{
    HvqContext *ctx = nullptr;
    CHECK(hvq_context_create(0, &ctx));
    hipStream_t caller = caller_stream();
    if (history) goldens_history(ctx, caller);
    std::vector<std::pair<int, const Clip *>> sc;
    for (const char *nm : SEVEN) {
        const Clip &c = clip(nm);
        const int sid = open_stream(ctx, c);
        submit_host(ctx, sid, c);
        CHECK(hvq_flush(ctx));
        sc.push_back({ sid, &c });
    }
    Exported ex;
    export_pictures(ctx, sc, caller, 0, history ? "seven/history" : "seven", &ex);
    for (auto &s : sc) read_back(ctx, s.first, *s.second, history ? "seven/history" : "seven");
    if (hipStreamSynchronize(caller) != hipSuccess) exit(3);
    free_exported(&ex);
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
    hvq_context_destroy(ctx);
    (void)hipStreamDestroy(caller);
}

/* five streams of different geometry submitted in turns, one flush: the launch shape comes from the fullest tile of another stream */
static void scenario_interleaved()
{
    static const char *names[] = { "wide296x160", "ip8", "literals96x96", "yuv444_13_portrait48x64", "pselfref422_64x48" };
    for (int dev = 0; dev < 2; ++dev) {
        HvqContext *ctx = nullptr;
        CHECK(hvq_context_create(0, &ctx));
        std::vector<std::pair<int, const Clip *>> sc;
        for (const char *nm : names) sc.push_back({ open_stream(ctx, clip(nm)), &clip(nm) });
        const Many m = many_of(sc, true);
        if (dev) submit_device(ctx, m, FORM_COPY);
        else CHECK(hvq_submit_many(ctx, (int)m.sids.size(), m.sids.data(), m.types.data(), m.pics.data(), m.lens.data(), 3, nullptr));
        CHECK(hvq_flush(ctx));
        for (auto &s : sc) read_back(ctx, s.first, *s.second, dev ? "interleaved/device" : "interleaved/host");
        hvq_context_destroy(ctx);
    }
}

static void scenario_lifecycle()
{
    HvqContext *ctx = nullptr;
    CHECK(hvq_context_create(0, &ctx));
    hipStream_t caller = caller_stream();
    const Clip &a = clip("gop64x48_15"), &b = clip("yuv422_64x48"), &d = clip("ragged24x40"), &e = clip("yuv444_64x48");
    Exported ex;
    /* 1. a stream closed between two flushes of the others, another geometry opened in its place */
    const int sa = open_stream(ctx, a), sb = open_stream(ctx, b), sd = open_stream(ctx, d);
    submit_host(ctx, sa, a); submit_host(ctx, sd, d);
    CHECK(hvq_flush(ctx));
    /* 2. closed with an export of its pictures still queued on the caller's stream */
    export_pictures(ctx, { { sd, &d }, { sa, &a } }, caller, 2, "lifecycle/close", &ex);
    read_back(ctx, sd, d, "lifecycle/close");
    CHECK(hvq_stream_close(ctx, sd));
    const int se = open_stream(ctx, e);
    submit_host(ctx, sb, b); submit_host(ctx, se, e);
    CHECK(hvq_flush(ctx));
    read_back(ctx, sb, b, "lifecycle/second");
    read_back(ctx, se, e, "lifecycle/second");
    /* 3. a flush into slots that a queued export still has to read: the clip once more into its stream, which reuses slots of the first pass */
    export_pictures(ctx, { { sa, &a } }, caller, 1, "lifecycle/reuse", &ex);
    submit_host(ctx, sa, a);
    CHECK(hvq_flush(ctx));
    read_back(ctx, sa, a, "lifecycle/reuse", (int)a.pics.size(), (int)a.pics.size(), 0);
    /* 4. the context destroyed with work queued: another flush, an export behind it, nothing waited for */
    submit_host(ctx, sb, b);
    CHECK(hvq_flush(ctx));
    export_pictures(ctx, { { se, &e } }, caller, 0, "lifecycle/destroy", &ex);
    hvq_context_destroy(ctx);
    if (hipStreamSynchronize(caller) != hipSuccess) exit(3);
    free_exported(&ex);
    (void)hipStreamDestroy(caller);
}

/* batches of two GPU-parsed streams through hvq_flush_begin, the submit of the next batch, hvq_flush_next: both arenas and both sets of parse
 * buffers are reused; each of the three submit forms is used */
static void scenario_streaming()
{
    static const char *pairs[6][2] = { { "gop64x48_15", "yuv422_64x48" }, { "ragged24x40", "weird64x64" }, { "yuv444_64x48", "ipb32" },
                                       { "portrait48x64", "gop64x48_13" }, { "literals96x96", "ip8" }, { "bigshift64x48", "yuv422_13_portrait48x64" } };
    static const Form forms[6] = { FORM_COPY, FORM_ASYNC, FORM_ARENA, FORM_ASYNC, FORM_ARENA, FORM_COPY };
    HvqContext *ctx = nullptr;
    CHECK(hvq_context_create(0, &ctx));
    std::vector<std::pair<int, const Clip *>> batch[6];
    Many keep[6];                                             /* the deferred copy reads these until the next flush */
    for (int k = 0; k < 6; ++k) {
        for (int j = 0; j < 2; ++j) batch[k].push_back({ open_stream(ctx, clip(pairs[k][j])), &clip(pairs[k][j]) });
        keep[k] = many_of(batch[k], true);
    }
    submit_device(ctx, keep[0], forms[0]);
    CHECK(hvq_flush_begin(ctx));
    for (int k = 1; k < 6; ++k) {
        submit_device(ctx, keep[k], forms[k]);
        CHECK(hvq_flush_next(ctx));                           /* ends batch k - 1, begins batch k */
        for (auto &s : batch[k - 1]) read_back_bulk(ctx, s.first, *s.second, "streaming");
    }
    CHECK(hvq_flush_end(ctx));
    for (auto &s : batch[5]) read_back_bulk(ctx, s.first, *s.second, "streaming");
    hvq_context_destroy(ctx);
}

/* one stream of a three-stream batch carries a corrupted P picture: the flush reports it, the other streams are decoded, the dropped
 * pictures read as not resident */
static void scenario_dropped(const char *corrupt_path)
{
    std::vector<uint8_t> bad;
    {
        FILE *f = corrupt_path ? fopen(corrupt_path, "rb") : nullptr;
        if (!f) { fprintf(stderr, "fake_driver: dropped needs the corrupted picture\n"); exit(2); }
        uint8_t tmp[4096];
        for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) bad.insert(bad.end(), tmp, tmp + n);
        fclose(f);
    }
    HvqContext *ctx = nullptr;
    CHECK(hvq_context_create(0, &ctx));
    const Clip &a = clip("gop64x48_15"), &b = clip("ipb32"), &d = clip("yuv444_64x48");
    const int sa = open_stream(ctx, a), sb = open_stream(ctx, b), sd = open_stream(ctx, d);
    Many m = many_of({ { sa, &a }, { sb, &b }, { sd, &d } }, true);
    for (size_t i = 0, seen = 0; i < m.sids.size(); ++i)
        if (m.sids[i] == sb && seen++ == 1) { m.pics[i] = bad.data(); m.lens[i] = bad.size(); }       /* the P picture of ipb32 */
    submit_device(ctx, m, FORM_COPY);
    fprintf(g_res, "R dropped/flush %d\n", hvq_flush(ctx));
    read_back(ctx, sa, a, "dropped");
    read_back(ctx, sd, d, "dropped");
    read_back(ctx, sb, b, "dropped", 0, -1, 0, true);
    hvq_context_destroy(ctx);
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_driver <scenario> <outdir> <golden dir> [corrupted picture]\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    g_bin = fopen((g_out + "/pictures.bin").c_str(), "wb");
    if (!g_res || !g_bin) { fprintf(stderr, "fake_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "clips0") scenario_clips(0, 2);
    else if (sc == "clips1") scenario_clips(1, 2);
    else if (sc == "seven") scenario_seven(false);
    else if (sc == "seven_history") scenario_seven(true);
    else if (sc == "interleaved") scenario_interleaved();
    else if (sc == "lifecycle") scenario_lifecycle();
    else if (sc == "streaming") scenario_streaming();
    else if (sc == "dropped") scenario_dropped(argc > 4 ? argv[4] : nullptr);
    else { fprintf(stderr, "fake_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    /* the export log against what was asked for: launch c of the log is export call c of this program */
    size_t asked = 0;
    for (auto &v : g_exports) asked += v.size();
    for (const FakeExportRecord &r : fake_export_log()) {
        if (r.call < 0 || (size_t)r.call >= g_exports.size() || r.job < 0 || (size_t)r.job >= g_exports[(size_t)r.call].size()) { fprintf(g_res, "E ? -1 0 unknown\n"); continue; }
        const Asked &a = g_exports[(size_t)r.call][(size_t)r.job];
        fprintf(g_res, "E %s %d %016llx %s\n", a.clip.c_str(), a.ordinal, (unsigned long long)r.hash, a.label.c_str());
    }
    fprintf(g_res, "X %zu %zu\n", asked, fake_export_log().size());
    fclose(g_res); fclose(g_bin);
    return 0;
}
