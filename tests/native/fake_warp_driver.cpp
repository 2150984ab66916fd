/*
 * tests/native/fake_warp_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_warp_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_warp.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_warp_cpu.py compares with
 * hvqm4_amd.warp.of_picture on the oracle's pictures.
 *
 *   fake_warp_driver <scenario> <outdir> <golden dir>
 *
 * <outdir>/warps.txt, written by the test, names the warps: one a line, `<name> m00 m01 m10 m11 t0 t1 border fill0 fill1 fill2 tw th ths
 * tvs` -- the members of HvqWarp in their order and the target geometry the warp is meant for: tw 0 the source's size, tw -1 the source's
 * with width and height exchanged, ths 0 the source's sampling.  The driver never builds a warp of its own, except the malformed ones of
 * `refused`, which it derives from the first of the file.
 *
 * results.txt, one fact per line:
 *   P <label> <source> <form> <k> <source geometry: w h hs vs> <warp name> <target geometry: w h hs vs> <crc32 of the bytes read back> <guard>
 *       source: a clip's name, or `synth`; form: pic (the resident picture k), inv (the caller's memory: picture k with every byte inverted),
 *       warped:<name> (the caller's memory: picture k through warp <name> by an earlier call, never read back in between), synth
 *       (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), flat (every byte k), check (a 0 / 255 checkerboard, 255 where x + y + k is
 *       odd, in every plane); guard: 1 when the 256 bytes before and the 256 bytes behind the output still hold the sentinel
 *   R <label> <return code>                           a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the output buffers after refused calls
 * Caller-side resources (a stream, outputs, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_warp_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

static std::vector<std::string> g_names;             /* the warps of warps.txt in their order */
static std::vector<HvqWarp> g_warps;
static std::vector<Geom> g_targets;                  /* and the target geometries they are meant for */

static void load_warps()
{
    std::ifstream f(g_out + "/warps.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name;
        if (!(in >> name)) continue;
        HvqWarp w;
        memset(&w, 0, sizeof w);
        int fill[3];
        Geom t;
        in >> w.m00 >> w.m01 >> w.m10 >> w.m11 >> w.t0 >> w.t1 >> w.border >> fill[0] >> fill[1] >> fill[2] >> t.w >> t.h >> t.hs >> t.vs;
        if (!in) { fprintf(stderr, "fake_warp_driver: warps.txt: the line of %s is short\n", name.c_str()); exit(2); }
        for (int p = 0; p < 3; ++p) w.fill[p] = (uint8_t)fill[p];
        g_names.push_back(name);
        g_warps.push_back(w);
        g_targets.push_back(t);
    }
    if (g_warps.empty()) { fprintf(stderr, "fake_warp_driver: no warps in %s/warps.txt\n", g_out.c_str()); exit(2); }
}

static Geom target_of(Geom g, int warp)
{
    const Geom t = g_targets[(size_t)warp];
    Geom o = g;
    if (t.w == -1) { o.w = g.h; o.h = g.w; }
    else if (t.w > 0) { o.w = t.w; o.h = t.h; }
    if (t.hs > 0) { o.hs = t.hs; o.vs = t.vs; }
    return o;
}

/* Item::entry: the warp of warps.txt */
struct Call { std::vector<uint8_t *> room; std::vector<Item> items; std::string label; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes before and behind the picture */
static Call call_warp(HvqContext *ctx, const std::vector<Item> &items, bool null_src, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    std::vector<HvqWarp> warps;
    std::vector<HvqWarpDst> dst;
    Call c{ {}, items, label };
    for (const Item &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); warps.push_back(g_warps[(size_t)p.entry]);
        const Geom t = target_of(p.g, p.entry);
        c.room.push_back(guarded_room(bytes_of(t)));
        dst.push_back(HvqWarpDst{ c.room.back() + GUARD, t.w, t.h, t.hs, t.vs });
    }
    CHECK(hvq_warp_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), warps.data(), dst.data(), caller));
    return c;
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        const Geom t = target_of(p.g, p.entry);
        const ReadBack r = read_room(c->room[i], bytes_of(t));
        fprintf(g_res, "P %s %s %s %d %d %d %d %d %s %d %d %d %d %u %d\n", c->label.c_str(), p.source.c_str(), p.form.c_str(), p.kk, p.g.w, p.g.h, p.g.hs, p.g.vs,
                g_names[(size_t)p.entry].c_str(), t.w, t.h, t.hs, t.vs, r.crc, r.guard);
        HIP(hipFree(c->room[i]));
    }
    c->room.clear();
}

/* every warp of the file on the last picture of clips of the three samplings, of a ragged one and of two with tile seams inside */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64", "ragged24x40", "wide296x160", "i16" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int f = 0; f < (int)g_warps.size(); ++f) v.push_back(resident(sid, c, (int)c.pics.size() - 1, f));
    }
    Call a = call_warp(ctx, v, true, caller, "goldens/all");
    Call b = call_warp(ctx, { v[1] }, false, caller, "goldens/one");
    fprintf(g_res, "R goldens/n0 %d\n", hvq_warp_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; made pictures of the
 * smallest geometry in the three samplings, of 72 x 24 and of 136 x 40, random, flat and the 0 / 255 checkerboard, through every warp;
 * the longest and the highest plane; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    std::vector<void *> keep;
    std::vector<Item> items;
    const int nf = (int)g_warps.size();
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        items.push_back(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep, k % nf));
        items.push_back(resident(sa, a, k, (k + 1) % nf));
    }
    const Geom shapes[] = { { 8, 8, 2, 2 }, { 8, 8, 2, 1 }, { 8, 8, 1, 1 }, { 72, 24, 2, 2 }, { 24, 72, 2, 1 }, { 136, 40, 2, 2 }, { 104, 56, 1, 1 }, { 8192, 8, 2, 2 }, { 8, 8192, 2, 2 } };
    for (const Geom &g : shapes) {
        const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
        CHECK(sid);
        const bool big = g.w > 1000 || g.h > 1000;
        for (int f = 0; f < nf; ++f) {
            if (big && f % 5) continue;
            items.push_back(made(sid, g, "synth", f + g.w, &keep, f));
            if (!big) items.push_back(made(sid, g, "check", f & 1, &keep, f));
        }
        items.push_back(made(sid, g, "flat", 201, &keep, g.w % nf));
    }
    Call c = call_warp(ctx, items, false, caller, "memory");
    Call d = call_warp(ctx, items, false, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    for (void *p : keep) HIP(hipFree(p));
}

/* one launch, many shapes: 300 pictures of eight clips, the warps of the file in turn; the same call twice */
static void scenario_many(HvqContext *&ctx, hipStream_t caller)
{
    const char *names[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96" };
    std::vector<std::pair<int, const Clip *>> sc;
    for (const char *nm : names) sc.push_back({ decode(ctx, clip(nm)), &clip(nm) });
    std::vector<Item> items;
    for (int i = 0; i < 300; ++i) {
        const auto &s = sc[(size_t)i % sc.size()];
        items.push_back(resident(s.first, *s.second, i % (int)s.second->pics.size(), (i / (int)sc.size() + i) % (int)g_warps.size()));
    }
    Call a = call_warp(ctx, items, false, caller, "many");
    Call b = call_warp(ctx, items, false, caller, "many/again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* every warp under the chosen body, under the forced direct body and under the tiled body wherever LDS holds the box */
static void scenario_body(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane444_48x64", "wide296x160", "ragged24x40", "yuv422_296x160" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int f = 0; f < (int)g_warps.size(); ++f) v.push_back(resident(sid, c, (int)c.pics.size() - 1, f));
    }
    Call a = call_warp(ctx, v, false, caller, "body/chosen");
    fprintf(g_res, "R body/force %d\n", hvq_warp_force_direct(ctx, 1));
    Call b = call_warp(ctx, v, false, caller, "body/direct");
    fprintf(g_res, "R body/force_tiled %d\n", hvq_warp_force_direct(ctx, 2));
    Call d = call_warp(ctx, v, false, caller, "body/tiled");
    fprintf(g_res, "R body/unforce %d\n", hvq_warp_force_direct(ctx, 0));
    Call c = call_warp(ctx, v, false, caller, "body/chosen_again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
    write_call(&d);
    write_call(&c);
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the outputs are those of the pictures as they were.  Then the warped pictures straight into a second call as its sources, nothing
 * waited for in between (what a consumer of src= does), and a context destroyed with a call still queued.  The warps keep the geometry. */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const int f0 = 1 % (int)g_warps.size(), f1 = 2 % (int)g_warps.size();
    std::vector<Item> items;
    for (int k = 0; k < n; ++k) items.push_back(resident(sa, a, k, f0));
    Call c = call_warp(ctx, items, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        HvqWarpDst d{ c.room[0] + GUARD, a.info.width, a.info.height, a.info.h_samp, a.info.v_samp };
        fprintf(g_res, "R reuse/evicted %d\n", hvq_warp_pictures(ctx, 1, &sa, &items[0].k, nullptr, &g_warps[(size_t)f0], &d, caller));
    }
    std::vector<Item> chain;
    for (int k = 0; k < n; ++k) chain.push_back(Item{ { sa, -1, c.room[(size_t)k] + GUARD, a.name, "warped:" + g_names[(size_t)f0], k, geom_of(a) }, f1 });
    Call g = call_warp(ctx, chain, false, caller, "reuse/chain");
    std::vector<Item> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Item p = resident(sa, a, 2 * n + k, f0);
        late_call.push_back(p);
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_warp(ctx, late_call, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(resident(se, e, k, f1));
    Call f = call_warp(ctx, other, false, caller, "reuse/destroy");
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
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    const Geom ga = geom_of(a);
    const size_t nb = bytes_of(ga), bytes = 2u * nb + 16u;
    void *out = nullptr, *mem = nullptr;
    HIP(hipMalloc(&out, bytes));
    HIP(hipMalloc(&mem, nb + 32u));
    std::vector<uint8_t> sent(bytes, SENTINEL);
    HIP(hipMemcpy(out, sent.data(), sent.size(), hipMemcpyHostToDevice));
    uint8_t *o = (uint8_t *)out, *o1 = o + nb;
    const HvqWarp good = g_warps[0];
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const HvqWarp *w1, uint8_t *p1,
                      Geom g1, bool null_warps = false, bool null_dst = false) {
        HvqWarp w[2] = { good, w1 ? *w1 : good };
        HvqWarpDst dst[2] = { { o, ga.w, ga.h, ga.hs, ga.vs }, { p1, g1.w, g1.h, g1.hs, g1.vs } };
        fprintf(g_res, "R refused/%s %d\n", label, hvq_warp_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), null_warps ? nullptr : w, null_dst ? nullptr : dst, caller));
    };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, ga);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, nullptr, o1, ga);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, nullptr, o1, ga);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, nullptr, o1, ga);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, nullptr, o1, ga);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, nullptr, o1, ga);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, nullptr, o1, ga);
    refuse("null_ptr", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, nullptr, ga);
    refuse("misaligned_ptr", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1 + 8, ga);
    refuse("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, nullptr, o1, ga);
    refuse("null_warps", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, ga, true);
    refuse("null_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, ga, false, true);
    refuse("geometry_width", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, Geom{ 12, 8, 2, 2 });
    refuse("geometry_sampling", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, Geom{ 16, 8, 1, 2 });
    refuse("geometry_zero", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, o1, Geom{ 0, 0, 2, 2 });
    /* the malformed warps: each as the warp of the second picture */
    auto bad = [&](const char *label, void (*spoil)(HvqWarp *)) {
        HvqWarp w = good;
        spoil(&w);
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_warp_check(&w));
        refuse(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, &w, o1, ga);
    };
    bad("m00_above", [](HvqWarp *w) { w->m00 = HVQ_WARP_MAX_SCALE + 1; });
    bad("m01_below", [](HvqWarp *w) { w->m01 = -HVQ_WARP_MAX_SCALE - 1; });
    bad("m10_above", [](HvqWarp *w) { w->m10 = 2147483647; });
    bad("m11_below", [](HvqWarp *w) { w->m11 = -2147483647 - 1; });
    bad("border_2", [](HvqWarp *w) { w->border = 2; });
    bad("border_negative", [](HvqWarp *w) { w->border = -1; });
    bad("pad", [](HvqWarp *w) { w->pad = 1; });
    fprintf(g_res, "R refused/check_null %d\n", hvq_warp_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_warp_check(&good));
    {
        HvqWarp lim = good;                                     /* at the limits: accepted */
        lim.m00 = HVQ_WARP_MAX_SCALE; lim.m11 = -HVQ_WARP_MAX_SCALE; lim.t0 = 2147483647; lim.t1 = -2147483647 - 1; lim.m01 = lim.m10 = 0;
        fprintf(g_res, "R refused/check_limits %d\n", hvq_warp_check(&lim));
    }
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, nullptr, o1, ga);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, nullptr, o1, ga);
    fprintf(g_res, "R refused/n0 %d\n", hvq_warp_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, caller));
    fprintf(g_res, "R refused/force_null %d\n", hvq_warp_force_direct(nullptr, 1));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    {
        Call c = call_warp(ctx, { resident(sa, a, 1, (int)g_warps.size() - 1), resident(sd, d, last, 0) }, false, caller, "refused/then_ok");
        HIP(hipStreamSynchronize(caller));
        write_call(&c);
    }
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_warp_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_warps();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_warp_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "goldens") run_scenario(scenario_goldens);
    else if (sc == "memory") run_scenario(scenario_memory);
    else if (sc == "many") run_scenario(scenario_many);
    else if (sc == "body") run_scenario(scenario_body);
    else if (sc == "reuse") run_scenario(scenario_reuse);
    else if (sc == "refused") run_scenario(scenario_refused);
    else { fprintf(stderr, "fake_warp_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
