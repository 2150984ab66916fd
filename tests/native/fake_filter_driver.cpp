/*
 * tests/native/fake_filter_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_filter_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_filter.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_filters_cpu.py compares with
 * hvqm4_amd.filters.of_picture on the oracle's pictures.
 *
 *   fake_filter_driver <scenario> <outdir> <golden dir>
 *
 * <outdir>/filters.txt, written by the test, names the filters: one a line, `<name>` and then, for luma and for chroma, `terms combine
 * shift bias` and for each of the two terms `rx ry wx[0..30] wy[0..30]` -- the members of HvqFilter in their order.  The driver never
 * builds a filter of its own, except the malformed ones of `refused`, which it derives from the first of the file.
 *
 * results.txt, one fact per line:
 *   P <label> <source> <form> <k> <geometry: w h hs vs> <filter name> <crc32 of the bytes read back> <guard>
 *       source: a clip's name, or `synth`; form: pic (the resident picture k), inv (the caller's memory: picture k with every byte inverted),
 *       filtered:<name> (the caller's memory: picture k through filter <name> by an earlier call, never read back in between), synth
 *       (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), flat (every byte k), check (a 0 / 255 checkerboard, 255 where x + y + k is
 *       odd, in every plane); guard: 1 when the 256 bytes before and the 256 bytes behind the output still hold the sentinel
 *   R <label> <return code>                           a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the output buffers after refused calls
 * Caller-side resources (a stream, outputs, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_filter_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

static std::vector<std::string> g_names;             /* the filters of filters.txt in their order */
static std::vector<HvqFilter> g_filters;

static void load_filters()
{
    std::ifstream f(g_out + "/filters.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name;
        if (!(in >> name)) continue;
        HvqFilter flt;
        memset(&flt, 0, sizeof flt);
        for (HvqPlaneFilter *p : { &flt.luma, &flt.chroma }) {
            in >> p->terms >> p->combine >> p->shift >> p->bias;
            for (HvqFilterTerm &t : p->term) {
                in >> t.rx >> t.ry;
                for (int16_t &w : t.wx) { int v; in >> v; w = (int16_t)v; }
                for (int16_t &w : t.wy) { int v; in >> v; w = (int16_t)v; }
            }
        }
        if (!in) { fprintf(stderr, "fake_filter_driver: filters.txt: the line of %s is short\n", name.c_str()); exit(2); }
        g_names.push_back(name);
        g_filters.push_back(flt);
    }
    if (g_filters.empty()) { fprintf(stderr, "fake_filter_driver: no filters in %s/filters.txt\n", g_out.c_str()); exit(2); }
}

/* Item::entry: the filter of filters.txt */
struct Call { std::vector<uint8_t *> room; std::vector<Item> items; std::string label; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes before and behind the picture.
 * use_which: the whole table of filters.txt and `which`; otherwise every item names the same filter, passed alone without `which` */
static Call call_filter(HvqContext *ctx, const std::vector<Item> &items, bool null_src, bool use_which, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<void *> dst;
    Call c{ {}, items, label };
    for (const Item &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); which.push_back(p.entry);
        c.room.push_back(guarded_room(bytes_of(p.g)));
        dst.push_back(c.room.back() + GUARD);
    }
    if (use_which) CHECK(hvq_filter_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), g_filters.data(), (int)g_filters.size(), which.data(), dst.data(), caller));
    else CHECK(hvq_filter_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), &g_filters[(size_t)items[0].entry], 1, nullptr, dst.data(), caller));
    return c;
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        const ReadBack r = read_room(c->room[i], bytes_of(p.g));
        fprintf(g_res, "P %s %s %s %d %d %d %d %d %s %u %d\n", c->label.c_str(), p.source.c_str(), p.form.c_str(), p.kk, p.g.w, p.g.h, p.g.hs, p.g.vs,
                g_names[(size_t)p.entry].c_str(), r.crc, r.guard);
        HIP(hipFree(c->room[i]));
    }
    c->room.clear();
}

/* every filter of the file on the last picture of clips of the three samplings, of a ragged one and of two with tile seams inside */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64", "ragged24x40", "wide296x160", "i16" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int f = 0; f < (int)g_filters.size(); ++f) v.push_back(resident(sid, c, (int)c.pics.size() - 1, f));
    }
    Call a = call_filter(ctx, v, true, true, caller, "goldens/all");
    Call b = call_filter(ctx, { v[1] }, false, false, caller, "goldens/one");
    fprintf(g_res, "R goldens/n0 %d\n", hvq_filter_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; made pictures of the
 * smallest geometry in the three samplings, of 72 x 24 and of 136 x 40, random, flat and the 0 / 255 checkerboard, through every filter;
 * on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    std::vector<void *> keep;
    std::vector<Item> items;
    const int nf = (int)g_filters.size();
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        items.push_back(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep, k % nf));
        items.push_back(resident(sa, a, k, (k + 1) % nf));
    }
    const Geom shapes[] = { { 8, 8, 2, 2 }, { 8, 8, 2, 1 }, { 8, 8, 1, 1 }, { 72, 24, 2, 2 }, { 72, 24, 1, 1 }, { 136, 40, 2, 2 }, { 136, 40, 2, 1 } };
    for (const Geom &g : shapes) {
        const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
        CHECK(sid);
        for (int f = 0; f < nf; ++f) {
            items.push_back(made(sid, g, "synth", f + g.w, &keep, f));
            items.push_back(made(sid, g, "check", f & 1, &keep, f));
        }
        items.push_back(made(sid, g, "flat", 201, &keep, g.w % nf));
    }
    Call c = call_filter(ctx, items, false, true, caller, "memory");
    Call d = call_filter(ctx, items, false, true, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    for (void *p : keep) HIP(hipFree(p));
}

/* one launch, many shapes: 300 pictures of eight clips, the filters of the file in turn; the same call twice */
static void scenario_many(HvqContext *&ctx, hipStream_t caller)
{
    const char *names[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96" };
    std::vector<std::pair<int, const Clip *>> sc;
    for (const char *nm : names) sc.push_back({ decode(ctx, clip(nm)), &clip(nm) });
    std::vector<Item> items;
    for (int i = 0; i < 300; ++i) {
        const auto &s = sc[(size_t)i % sc.size()];
        items.push_back(resident(s.first, *s.second, i % (int)s.second->pics.size(), (i / (int)sc.size() + i) % (int)g_filters.size()));
    }
    Call a = call_filter(ctx, items, false, true, caller, "many");
    Call b = call_filter(ctx, items, false, true, caller, "many/again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* identity planes through the copy body (chosen) and through the filter body (forced) */
static void scenario_body(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane444_48x64", "wide296x160", "ragged24x40" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int f = 0; f < (int)g_filters.size(); ++f) v.push_back(resident(sid, c, (int)c.pics.size() - 1, f));
    }
    Call a = call_filter(ctx, v, false, true, caller, "body/chosen");
    fprintf(g_res, "R body/force %d\n", hvq_filter_force_filter(ctx, 1));
    Call b = call_filter(ctx, v, false, true, caller, "body/filter");
    fprintf(g_res, "R body/unforce %d\n", hvq_filter_force_filter(ctx, 0));
    Call c = call_filter(ctx, v, false, true, caller, "body/chosen_again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
    write_call(&c);
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the outputs are those of the pictures as they were.  Then the filtered pictures straight into a second call as its sources, nothing
 * waited for in between (what a consumer of src= does), and a context destroyed with a call still queued */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const int f0 = 1 % (int)g_filters.size(), f1 = 2 % (int)g_filters.size();
    std::vector<Item> items;
    for (int k = 0; k < n; ++k) items.push_back(resident(sa, a, k, f0));
    Call c = call_filter(ctx, items, false, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        void *d = c.room[0] + GUARD;
        fprintf(g_res, "R reuse/evicted %d\n", hvq_filter_pictures(ctx, 1, &sa, &items[0].k, nullptr, &g_filters[(size_t)f0], 1, nullptr, &d, caller));
    }
    std::vector<Item> chain;
    for (int k = 0; k < n; ++k) chain.push_back(Item{ { sa, -1, c.room[(size_t)k] + GUARD, a.name, "filtered:" + g_names[(size_t)f0], k, geom_of(a) }, f1 });
    Call g = call_filter(ctx, chain, false, false, caller, "reuse/chain");
    std::vector<Item> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Item p = resident(sa, a, 2 * n + k, f0);
        late_call.push_back(p);
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_filter(ctx, late_call, false, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(resident(se, e, k, f1));
    Call f = call_filter(ctx, other, false, false, caller, "reuse/destroy");
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

    const size_t nb = bytes_of(geom_of(a)), bytes = 2u * nb + 16u;
    void *out = nullptr, *mem = nullptr;
    HIP(hipMalloc(&out, bytes));
    HIP(hipMalloc(&mem, nb + 32u));
    std::vector<uint8_t> sent(bytes, SENTINEL);
    HIP(hipMemcpy(out, sent.data(), sent.size(), hipMemcpyHostToDevice));
    uint8_t *o = (uint8_t *)out, *o1 = o + nb;
    const HvqFilter good = g_filters[0];
    const int two[2] = { 0, 0 };
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const HvqFilter *f, int nf,
                      const int *which, uint8_t *p1) {
        void *dst[2] = { o, p1 };
        fprintf(g_res, "R refused/%s %d\n", label, hvq_filter_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), f, nf, which, dst, caller));
    };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, o1);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, &good, 1, nullptr, o1);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, &good, 1, nullptr, o1);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, &good, 1, nullptr, o1);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, &good, 1, nullptr, o1);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, &good, 1, nullptr, o1);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, &good, 1, nullptr, o1);
    refuse("null_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, nullptr);
    refuse("misaligned_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, o1 + 8);
    refuse("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, o1);
    refuse("null_filters", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, 1, nullptr, o1);
    refuse("nfilters_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 0, nullptr, o1);
    {
        std::vector<HvqFilter> many(65, good);
        refuse("nfilters_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, many.data(), 65, two, o1);
    }
    const int w_hi[2] = { 0, 1 }, w_lo[2] = { 0, -1 };
    refuse("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_hi, o1);
    refuse("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_lo, o1);
    /* the malformed filters: each in the chroma plane of the second filter of a table whose first is well formed and the only one used */
    auto bad = [&](const char *label, void (*spoil)(HvqPlaneFilter *)) {
        HvqFilter tab[2] = { good, good };
        spoil(&tab[1].chroma);
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_filter_check(&tab[1]));
        refuse(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, tab, 2, two, o1);
    };
    bad("terms_0", [](HvqPlaneFilter *p) { p->terms = 0; });
    bad("terms_3", [](HvqPlaneFilter *p) { p->terms = 3; });
    bad("radius_16", [](HvqPlaneFilter *p) { p->term[0].rx = 16; });
    bad("radius_negative", [](HvqPlaneFilter *p) { p->term[0].ry = -1; });
    bad("tap_beyond", [](HvqPlaneFilter *p) { p->term[0].wx[2 * p->term[0].rx + 1] = 1; });
    bad("tap_beyond_y", [](HvqPlaneFilter *p) { p->term[0].wy[30] = -1; });   /* the first filter of the file has a radius below 15 */
    bad("combine_3", [](HvqPlaneFilter *p) { p->combine = 3; });
    bad("combine_negative", [](HvqPlaneFilter *p) { p->combine = -1; });
    bad("shift_23", [](HvqPlaneFilter *p) { p->shift = 23; });
    bad("shift_negative", [](HvqPlaneFilter *p) { p->shift = -1; });
    bad("bias_256", [](HvqPlaneFilter *p) { p->bias = 256; });
    bad("bias_minus_256", [](HvqPlaneFilter *p) { p->bias = -256; });
    bad("gain_0", [](HvqPlaneFilter *p) { for (HvqFilterTerm &t : p->term) memset(t.wx, 0, sizeof t.wx); });
    bad("gain_above", [](HvqPlaneFilter *p) { p->terms = 1; p->term[0].rx = p->term[0].ry = 0; p->term[0].wx[0] = 2049; p->term[0].wy[0] = 2048; p->shift = 22; });
    fprintf(g_res, "R refused/check_null %d\n", hvq_filter_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_filter_check(&good));
    {
        HvqFilter unused = good;                                /* a term that is not in use is not looked at */
        if (unused.luma.terms == 1) { unused.luma.term[1].rx = 99; unused.luma.term[1].wx[30] = 7; }
        fprintf(g_res, "R refused/check_unused_term %d\n", hvq_filter_check(&unused));
    }
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, &good, 1, nullptr, o1);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, &good, 1, nullptr, o1);
    fprintf(g_res, "R refused/n0 %d\n", hvq_filter_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    fprintf(g_res, "R refused/force_null %d\n", hvq_filter_force_filter(nullptr, 1));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works, with a table of 64 filters */
    CHECK(hvq_flush(ctx));
    {
        std::vector<HvqFilter> keep_all = g_filters;
        std::vector<std::string> keep_names = g_names;
        while (g_filters.size() < 64) { g_filters.push_back(keep_all[g_filters.size() % keep_all.size()]); g_names.push_back(keep_names[g_names.size() % keep_names.size()]); }
        Call c = call_filter(ctx, { resident(sa, a, 1, 63), resident(sd, d, last, 0) }, false, true, caller, "refused/then_ok");
        HIP(hipStreamSynchronize(caller));
        write_call(&c);
    }
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_filter_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_filters();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_filter_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "goldens") run_scenario(scenario_goldens);
    else if (sc == "memory") run_scenario(scenario_memory);
    else if (sc == "many") run_scenario(scenario_many);
    else if (sc == "body") run_scenario(scenario_body);
    else if (sc == "reuse") run_scenario(scenario_reuse);
    else if (sc == "refused") run_scenario(scenario_refused);
    else { fprintf(stderr, "fake_filter_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
