/*
 * tests/native/fake_scale_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_scale_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_scale.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_scale_cpu.py compares with hvqm4_amd.scale.of_picture
 * on the oracle's pictures.
 *
 *   fake_scale_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   P <label> <source> <form> <k> <source geometry: w h hs vs> <target geometry: w h hs vs> <crop: x y w h> <crc32 of the bytes read back> <guard>
 *       source: a clip's name, or `synth`; form: pic (the resident picture k), inv (the caller's memory: picture k with every byte inverted),
 *       scaled (the caller's memory: picture k scaled to the "source geometry" by an earlier call, never read back in between), synth
 *       (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), flat (every byte k), tie (2 x 2 blocks { 0, 0, 0, k }); guard: 1 when the
 *       256 bytes behind the output still hold the sentinel
 *   R <label> <return code>                           a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the output buffers after refused calls
 * Caller-side resources (a stream, outputs, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_scale_driver"
#include "fake_slot_driver.h"

struct Crop { int x, y, w, h; };

/* one picture of a call and what the test is told about it: Picture::g is the source geometry */
struct ScaleItem : Picture { Geom to; Crop crop; };

static ScaleItem resident(int sid, const Clip &c, int k, Geom to, Crop crop = Crop{ 0, 0, 0, 0 }) { return ScaleItem{ resident_picture(sid, c, k), to, crop }; }

static ScaleItem in_memory(HvqContext *ctx, int sid, const Clip &c, int k, size_t offset, std::vector<void *> *keep, Geom to, Crop crop = Crop{ 0, 0, 0, 0 })
{
    return ScaleItem{ inverted_picture(ctx, sid, c, k, offset, keep), to, crop };
}

/* the kit's rules, and tie: 2 x 2 blocks { 0, 0, 0, k } (4:4:4) */
static ScaleItem made(int sid, Geom from, const char *form, int k, std::vector<void *> *keep, Geom to, Crop crop = Crop{ 0, 0, 0, 0 })
{
    if (std::string(form) != "tie") return ScaleItem{ made_picture(sid, from, form, k, keep), to, crop };
    std::vector<uint8_t> host(bytes_of(from));
    for (size_t i = 0; i < host.size(); ++i) { const size_t x = i % (size_t)from.w, y = i / (size_t)from.w; host[i] = (uint8_t)((x & 1u) && (y & 1u) ? k : 0); }
    return ScaleItem{ { sid, -1, uploaded(host, 0, keep), "synth", form, k, from }, to, crop };
}

struct Call { std::vector<uint8_t *> out; std::vector<ScaleItem> items; std::string label; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes longer than the picture */
static Call call_scale(HvqContext *ctx, const std::vector<ScaleItem> &items, bool null_src, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    std::vector<HvqScaleDst> dst;
    Call c{ {}, items, label };
    for (const ScaleItem &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src);
        const int64_t nb = hvq_scale_bytes(p.to.w, p.to.h, p.to.hs, p.to.vs);
        CHECK(nb);
        c.out.push_back(guarded_room((size_t)nb, 0));
        dst.push_back(HvqScaleDst{ c.out.back(), p.to.w, p.to.h, p.to.hs, p.to.vs, p.crop.x, p.crop.y, p.crop.w, p.crop.h });
    }
    CHECK(hvq_scale_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), dst.data(), caller));
    return c;
}

/* after the caller's stream has been waited for */
static void write_call(Call *c, bool release = true)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const ScaleItem &p = c->items[i];
        const size_t nb = (size_t)hvq_scale_bytes(p.to.w, p.to.h, p.to.hs, p.to.vs);
        const ReadBack r = read_room(c->out[i], nb, 0);
        fprintf(g_res, "P %s %s %s %d %d %d %d %d %d %d %d %d %d %d %d %d %u %d\n", c->label.c_str(), p.source.c_str(), p.form.c_str(), p.kk, p.g.w, p.g.h, p.g.hs,
                p.g.vs, p.to.w, p.to.h, p.to.hs, p.to.vs, p.crop.x, p.crop.y, p.crop.w, p.crop.h, r.crc, r.guard);
        if (release) HIP(hipFree(c->out[i]));
    }
    if (release) c->out.clear();
}

/* the shapes of tests/test_gpu_scale.py on resident pictures: identity in every sampling, ratios 2 and 4, ratios that are no integers with
 * tile seams inside the picture, enlargement, sampling conversion at the same and at half size, crops */
static std::vector<ScaleItem> shapes(HvqContext *ctx, std::map<std::string, int> *sids)
{
    auto sid = [&](const char *nm) {
        auto it = sids->find(nm);
        if (it != sids->end()) return it->second;
        return (*sids)[nm] = decode(ctx, clip(nm));
    };
    auto last = [&](const char *nm) { return (int)clip(nm).pics.size() - 1; };
    std::vector<ScaleItem> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64" }) v.push_back(resident(sid(nm), clip(nm), last(nm), geom_of(clip(nm))));
    for (int k = 0; k < 2; ++k) {
        v.push_back(resident(sid("natural128x96"), clip("natural128x96"), k, Geom{ 64, 48, 2, 2 }));
        v.push_back(resident(sid("natural128x96"), clip("natural128x96"), k, Geom{ 32, 24, 2, 2 }));
    }
    v.push_back(resident(sid("ragged24x40"), clip("ragged24x40"), last("ragged24x40"), Geom{ 16, 16, 2, 2 }));
    v.push_back(resident(sid("ragged24x40"), clip("ragged24x40"), last("ragged24x40"), Geom{ 8, 8, 2, 2 }));
    v.push_back(resident(sid("wide296x160"), clip("wide296x160"), last("wide296x160"), Geom{ 104, 56, 2, 2 }));
    v.push_back(resident(sid("nest_exact280x152"), clip("nest_exact280x152"), last("nest_exact280x152"), Geom{ 96, 56, 2, 2 }));
    v.push_back(resident(sid("portrait152x280"), clip("portrait152x280"), last("portrait152x280"), Geom{ 56, 104, 2, 2 }));
    v.push_back(resident(sid("i16"), clip("i16"), 0, Geom{ 40, 24, 2, 2 }));
    v.push_back(resident(sid("gop64x48_15"), clip("gop64x48_15"), 3, Geom{ 64, 104, 2, 2 }));
    for (int d = 1; d <= 2; ++d) {
        v.push_back(resident(sid("yuv444_64x48"), clip("yuv444_64x48"), last("yuv444_64x48"), Geom{ 64 / d, 48 / d, 2, 2 }));
        v.push_back(resident(sid("gop64x48_15"), clip("gop64x48_15"), last("gop64x48_15"), Geom{ 64 / d, 48 / d, 1, 1 }));
        v.push_back(resident(sid("yuv422_64x48"), clip("yuv422_64x48"), last("yuv422_64x48"), Geom{ 64 / d, 48 / d, 2, 2 }));
    }
    v.push_back(resident(sid("natural128x96"), clip("natural128x96"), 2, Geom{ 48, 40, 2, 2 }, Crop{ 40, 24, 88, 72 }));
    v.push_back(resident(sid("yuv444_64x48"), clip("yuv444_64x48"), 1, Geom{ 24, 16, 1, 1 }, Crop{ 3, 5, 41, 33 }));
    v.push_back(resident(sid("yuv444_64x48"), clip("yuv444_64x48"), 1, Geom{ 64, 48, 2, 2 }, Crop{ 23, 15, 41, 33 }));
    v.push_back(resident(sid("natural128x96"), clip("natural128x96"), 1, Geom{ 8, 8, 2, 2 }, Crop{ 120, 88, 8, 8 }));
    v.push_back(resident(sid("natural128x96"), clip("natural128x96"), 1, Geom{ 16, 24, 2, 2 }, Crop{ 62, 2, 8, 8 }));
    return v;
}

static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::map<std::string, int> sids;
    const std::vector<ScaleItem> v = shapes(ctx, &sids);
    Call a = call_scale(ctx, v, true, caller, "goldens/all");
    Call b = call_scale(ctx, { v[7] }, false, caller, "goldens/one");
    fprintf(g_res, "R goldens/n0 %d\n", hvq_scale_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; the tie pictures; the
 * 32x limit in both directions; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sb = decode(ctx, b);
    const int st = hvq_stream_open(ctx, 16, 16, 1, 1, 1, 3), sl = hvq_stream_open(ctx, 256, 256, 2, 2, 1, 3);
    CHECK(st); CHECK(sl);
    std::vector<void *> keep;
    std::vector<ScaleItem> items;
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        items.push_back(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep, Geom{ 40, 24, 2, 2 }));
        items.push_back(resident(sa, a, k, Geom{ 40, 24, 2, 2 }));
    }
    items.push_back(in_memory(ctx, sb, b, 1, 16, &keep, Geom{ 16, 16, 1, 1 }, Crop{ 2, 4, 20, 30 }));
    items.push_back(made(st, Geom{ 16, 16, 1, 1 }, "tie", 2, &keep, Geom{ 8, 8, 1, 1 }));
    items.push_back(made(st, Geom{ 16, 16, 1, 1 }, "tie", 1, &keep, Geom{ 8, 8, 1, 1 }));
    items.push_back(made(sl, Geom{ 256, 256, 2, 2 }, "synth", 7, &keep, Geom{ 8, 8, 2, 2 }));
    items.push_back(made(sl, Geom{ 256, 256, 2, 2 }, "synth", 9, &keep, Geom{ 8, 8, 1, 1 }));
    items.push_back(made(sl, Geom{ 256, 256, 2, 2 }, "flat", 201, &keep, Geom{ 72, 40, 2, 1 }));
    Call c = call_scale(ctx, items, false, caller, "memory");
    Call d = call_scale(ctx, items, false, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    for (void *p : keep) HIP(hipFree(p));
}

/* 8192 x 2064 -> 256 x 72: cells beyond 32 bits */
static void scenario_cells64(HvqContext *&ctx, hipStream_t caller)
{
    const Geom big{ 8192, 2064, 2, 2 };
    const int sid = hvq_stream_open(ctx, big.w, big.h, big.hs, big.vs, 1, 3);
    CHECK(sid);
    std::vector<void *> keep;
    Call c = call_scale(ctx, { made(sid, big, "synth", 64, &keep, Geom{ 256, 72, 2, 2 }), made(sid, big, "flat", 255, &keep, Geom{ 256, 72, 2, 2 }) }, false, caller, "cells64");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    for (void *p : keep) HIP(hipFree(p));
}

/* one launch, many shapes: 300 pictures of eight clips, the targets, samplings and crops mixed; the same call twice */
static void scenario_many(HvqContext *&ctx, hipStream_t caller)
{
    const char *names[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96" };
    std::vector<std::pair<int, const Clip *>> sc;
    for (const char *nm : names) sc.push_back({ decode(ctx, clip(nm)), &clip(nm) });
    std::vector<ScaleItem> items;
    auto r8 = [](int v) { return std::max(8, (v + 8) / 16 * 8); };
    for (int i = 0; i < 300; ++i) {
        const auto &s = sc[(size_t)i % sc.size()];
        const Geom g = geom_of(*s.second);
        const int k = i % (int)s.second->pics.size(), v = (i / (int)sc.size() + i) % 5;
        if (v == 0) items.push_back(resident(s.first, *s.second, k, Geom{ r8(g.w), r8(g.h), g.hs, g.vs }));
        else if (v == 1) items.push_back(resident(s.first, *s.second, k, Geom{ g.w + 8, std::max(8, g.h - 8), g.hs, g.vs }));
        else if (v == 2) items.push_back(resident(s.first, *s.second, k, Geom{ g.w, g.h, g.hs == 2 && g.vs == 2 ? 1 : 2, g.hs == 2 && g.vs == 2 ? 1 : 2 }));
        else if (v == 3) items.push_back(resident(s.first, *s.second, k, Geom{ 24, 16, 2, 1 }));
        else {
            const int cw = std::max(8, g.w / 4 * 2), ch = std::max(8, g.h / 4 * 2);
            items.push_back(resident(s.first, *s.second, k, Geom{ 24, 16, 2, 1 }, Crop{ g.w - cw, g.h - ch, cw, ch }));
        }
    }
    Call a = call_scale(ctx, items, false, caller, "many");
    Call b = call_scale(ctx, items, false, caller, "many/again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* the forced direct body and the chosen one on the same pictures */
static void scenario_body(HvqContext *&ctx, hipStream_t caller)
{
    std::map<std::string, int> sids;
    std::vector<ScaleItem> v = shapes(ctx, &sids);
    std::vector<void *> keep;
    const int sl = hvq_stream_open(ctx, 256, 256, 2, 2, 1, 3);
    CHECK(sl);
    v.push_back(made(sl, Geom{ 256, 256, 2, 2 }, "synth", 5, &keep, Geom{ 8, 8, 2, 2 }));
    Call a = call_scale(ctx, v, false, caller, "body/chosen");
    fprintf(g_res, "R body/force %d\n", hvq_scale_force_direct(ctx, 1));
    Call b = call_scale(ctx, v, false, caller, "body/direct");
    fprintf(g_res, "R body/unforce %d\n", hvq_scale_force_direct(ctx, 0));
    Call c = call_scale(ctx, v, false, caller, "body/chosen_again");
    fprintf(g_res, "R body/tiled %d\n", hvq_scale_body(296, 160, 104, 56));
    fprintf(g_res, "R body/identity %d\n", hvq_scale_body(64, 48, 64, 48));
    fprintf(g_res, "R body/enlarge %d\n", hvq_scale_body(16, 16, 40, 24));
    fprintf(g_res, "R body/beyond %d\n", hvq_scale_body(264, 256, 8, 8));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
    write_call(&c);
    for (void *p : keep) HIP(hipFree(p));
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the outputs are those of the pictures as they were.  Then the scaled pictures straight into a second call as its sources, nothing
 * waited for in between (what a consumer of src= does), and a context destroyed with a call still queued */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const Geom half{ 40, 24, 2, 2 };
    std::vector<ScaleItem> items;
    for (int k = 0; k < n; ++k) items.push_back(resident(sa, a, k, half));
    Call c = call_scale(ctx, items, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        HvqScaleDst d{ c.out[0], half.w, half.h, half.hs, half.vs, 0, 0, 0, 0 };
        fprintf(g_res, "R reuse/evicted %d\n", hvq_scale_pictures(ctx, 1, &sa, &items[0].k, nullptr, &d, caller));
    }
    /* the first call's outputs as the sources of a second one: a stream of their geometry carries them */
    const int carrier = hvq_stream_open(ctx, half.w, half.h, half.hs, half.vs, 1, 3);
    CHECK(carrier);
    std::vector<ScaleItem> chain;
    for (int k = 0; k < n; ++k) chain.push_back(ScaleItem{ { carrier, -1, c.out[(size_t)k], a.name, "scaled", k, half }, Geom{ 16, 16, 1, 1 }, Crop{ 0, 0, 0, 0 } });
    Call g = call_scale(ctx, chain, false, caller, "reuse/chain");
    std::vector<ScaleItem> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        ScaleItem p = resident(sa, a, 2 * n + k, half);
        late_call.push_back(p);
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_scale(ctx, late_call, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(resident(se, e, k, Geom{ 32, 24, 2, 2 }));
    Call f = call_scale(ctx, other, false, caller, "reuse/destroy");
    hvq_context_destroy(ctx);
    ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&g);
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &d = a;
    const int sa = decode(ctx, a);
    /* a ring of 3 slots: the clip's first pictures are gone when its last ones are decoded */
    const int sd = hvq_stream_open(ctx, d.info.width, d.info.height, d.info.h_samp, d.info.v_samp, d.info.is_1_5, 3);
    CHECK(sd);
    for (const Pic &p : d.pics) CHECK(hvq_stream_submit(ctx, sd, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    const int last = (int)d.pics.size() - 1;
    const int big = hvq_stream_open(ctx, 520, 8, 2, 2, 1, 3);
    CHECK(big);
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    const Geom ok{ 32, 24, 2, 2 };
    const size_t nb = (size_t)hvq_scale_bytes(ok.w, ok.h, ok.hs, ok.vs), bytes = 2u * nb + 16u;
    void *out = nullptr, *mem = nullptr;
    HIP(hipMalloc(&out, bytes));
    HIP(hipMalloc(&mem, 520u * 8u * 3u / 2u + hvq_stream_pic_bytes(ctx, sa) + 32u));
    std::vector<uint8_t> sent(bytes, SENTINEL);
    HIP(hipMemcpy(out, sent.data(), sent.size(), hipMemcpyHostToDevice));
    uint8_t *o = (uint8_t *)out;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, Geom g1, Crop c1, uint8_t *p1) {
        HvqScaleDst dst[2] = { { o, ok.w, ok.h, ok.hs, ok.vs, 0, 0, 0, 0 }, { p1, g1.w, g1.h, g1.hs, g1.vs, c1.x, c1.y, c1.w, c1.h } };
        fprintf(g_res, "R refused/%s %d\n", label, hvq_scale_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), dst, caller));
    };
    const Crop whole{ 0, 0, 0, 0 };
    uint8_t *o1 = o + nb;
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, ok, whole, o1);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, ok, whole, o1);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, ok, whole, o1);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, ok, whole, o1);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, ok, whole, o1);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, ok, whole, o1);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, ok, whole, o1);
    refuse("null_ptr", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, whole, nullptr);
    refuse("misaligned_ptr", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, whole, o1 + 8);
    refuse("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, ok, whole, o1);
    refuse("beyond_32", ctx, 2, { sa, big }, { 0, -1 }, { nullptr, mem }, Geom{ 16, 8, 2, 2 }, whole, o1);
    refuse("crop_empty", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 8, 8, 16, -8 }, o1);
    refuse("crop_w0_with_offset", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 2, 0, 0, 0 }, o1);
    refuse("crop_leaves_right", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 40, 0, 32, 16 }, o1);
    refuse("crop_leaves_bottom", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 0, 40, 32, 16 }, o1);
    refuse("crop_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ -2, 0, 32, 16 }, o1);
    refuse("crop_odd_x", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 1, 0, 32, 16 }, o1);
    refuse("crop_odd_h", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 0, 0, 32, 15 }, o1);
    refuse("crop_narrow", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 0, 0, 6, 16 }, o1);
    refuse("crop_low", ctx, 2, { sa, sa }, { 0, 1 }, {}, ok, Crop{ 0, 0, 16, 6 }, o1);
    refuse("geometry_width", ctx, 2, { sa, sa }, { 0, 1 }, {}, Geom{ 36, 24, 2, 2 }, whole, o1);
    refuse("geometry_sampling", ctx, 2, { sa, sa }, { 0, 1 }, {}, Geom{ 32, 24, 1, 2 }, whole, o1);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, ok, whole, o1);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, ok, whole, o1);
    fprintf(g_res, "R refused/n0 %d\n", hvq_scale_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
    fprintf(g_res, "R refused/bytes_geometry %d\n", (int)hvq_scale_bytes(36, 24, 2, 2));
    fprintf(g_res, "R refused/force_null %d\n", hvq_scale_force_direct(nullptr, 1));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_scale(ctx, { resident(sa, a, 1, ok), resident(sd, d, last, ok) }, false, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_scale_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_scale_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "goldens") run_scenario(scenario_goldens);
    else if (sc == "memory") run_scenario(scenario_memory);
    else if (sc == "cells64") run_scenario(scenario_cells64);
    else if (sc == "many") run_scenario(scenario_many);
    else if (sc == "body") run_scenario(scenario_body);
    else if (sc == "reuse") run_scenario(scenario_reuse);
    else if (sc == "refused") run_scenario(scenario_refused);
    else { fprintf(stderr, "fake_scale_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
