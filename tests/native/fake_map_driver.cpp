/*
 * tests/native/fake_map_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_map_pictures and hvq_histogram_tables of
 * the runtime (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device, tests/native/fake_map.cpp and
 * tests/native/fake_histograms.cpp) through include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_map_cpu.py
 * compares with hvqm4_amd.maps on the oracle's pictures.
 *
 *   fake_map_driver <scenario> <outdir> <golden dir>
 *
 * The test writes into <outdir>: tables.bin (records of 768 bytes: the tables `t<i>` below), rules.txt (one rule a line: `<name>` and
 * then, for luma and for chroma, `kind a b pad` -- the members of HvqTableRule in their order) and records.bin (histogram records, uint32
 * [3][256] each, for the scenario `tables`).  The driver builds no table and no rule of its own, except the malformed rules of `refused`,
 * which it derives from the first of the file.
 *
 * results.txt, one fact per line:
 *   P <label> <source> <form> <k> <geometry: w h hs vs> <table> <planes> <crc32 of the bytes read back> <guard>
 *       source: a clip's name, or `synth`; form: pic (the resident picture k), inv (the caller's memory: picture k with every byte
 *       inverted), synth (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), inplace (synth, and the output IS the source);
 *       table: t<i> (record i of tables.bin), o<i> (record i of tables_out.bin, below), r:<name> (the table the GPU made of the
 *       picture's own histogram through rule <name>); guard: 1 when the 256 bytes before and behind the output still hold the sentinel
 *   R <label> <return code>                           a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the output buffers after refused calls
 * <label>.bin (tables_out.bin, chain.bin): table records read back, 768 bytes each.
 * Caller-side resources (a stream, outputs, picture memory, tables) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_map_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

static std::vector<std::string> g_names;             /* the rules of rules.txt in their order */
static std::vector<HvqTableRule> g_rules;
static std::vector<uint8_t> g_tables;                /* tables.bin */
static uint8_t *g_tables_dev;                        /* ... in device memory */
static int g_ntables;

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void load_inputs()
{
    std::ifstream f(g_out + "/rules.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name;
        if (!(in >> name)) continue;
        HvqTableRule r;
        memset(&r, 0, sizeof r);
        for (HvqTablePlane *p : { &r.luma, &r.chroma }) in >> p->kind >> p->a >> p->b >> p->pad;
        if (!in) { fprintf(stderr, DRIVER_NAME ": rules.txt: the line of %s is short\n", name.c_str()); exit(2); }
        g_names.push_back(name);
        g_rules.push_back(r);
    }
    g_tables = slurp(g_out + "/tables.bin");
    if (g_rules.empty() || g_tables.empty() || g_tables.size() % HVQ_MAP_TABLE_BYTES) { fprintf(stderr, DRIVER_NAME ": no rules or tables in %s\n", g_out.c_str()); exit(2); }
    g_ntables = (int)(g_tables.size() / HVQ_MAP_TABLE_BYTES);
    HIP(hipMalloc((void **)&g_tables_dev, g_tables.size()));
    HIP(hipMemcpy(g_tables_dev, g_tables.data(), g_tables.size(), hipMemcpyHostToDevice));
}

/* Item::entry: the record of the call's tables */

/* the caller's memory filled by the rule synth, between guards; inplace: the call writes where it reads */
static Item made_guarded(int sid, Geom g, bool inplace, int k, int table)
{
    uint8_t *room = guarded_room(bytes_of(g));
    const std::vector<uint8_t> host = filled(g, "synth", k);
    HIP(hipMemcpy(room + GUARD, host.data(), host.size(), hipMemcpyHostToDevice));
    return Item{ { sid, -1, room + GUARD, "synth", inplace ? "inplace" : "synth", k, g }, table };
}
static uint8_t *room_of(const Item &made) { return (uint8_t *)made.src - GUARD; }

struct Call { std::vector<uint8_t *> room; std::vector<Item> items; std::string label, prefix; int planes; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes before and behind the picture (an
 * in-place item: its source's).  tables / ntables / use_which: the three forms of the header */
static Call call_map(HvqContext *ctx, const std::vector<Item> &items, const uint8_t *tables, int ntables, bool use_which, int planes, hipStream_t caller,
                     const char *label, const char *prefix = "t")
{
    const int n = (int)items.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<void *> dst;
    Call c{ {}, items, label, prefix, planes };
    for (const Item &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); which.push_back(p.entry);
        c.room.push_back(p.form == "inplace" ? room_of(p) : guarded_room(bytes_of(p.g)));
        dst.push_back(c.room.back() + GUARD);
    }
    CHECK(hvq_map_pictures(ctx, n, sids.data(), ords.data(), src.data(), tables, ntables, use_which ? which.data() : nullptr, planes, dst.data(), caller));
    return c;
}

/* after the caller's stream has been waited for; `rule`: the items' tables are r:<rule name> */
static void write_call(Call *c, bool free_rooms = true)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        const ReadBack r = read_room(c->room[i], bytes_of(p.g));
        const std::string table = c->prefix == "r:" ? "r:" + g_names[(size_t)p.entry] : c->prefix + std::to_string(p.entry);
        fprintf(g_res, "P %s %s %s %d %d %d %d %d %s %d %u %d\n", c->label.c_str(), p.source.c_str(), p.form.c_str(), p.kk, p.g.w, p.g.h, p.g.hs, p.g.vs,
                table.c_str(), c->planes, r.crc, r.guard);
        if (free_rooms) HIP(hipFree(c->room[i]));
    }
    if (free_rooms) c->room.clear();
}

static void write_bin(const char *label, const uint8_t *dev, size_t bytes)
{
    std::vector<uint8_t> host(bytes);
    HIP(hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost));
    FILE *f = fopen((g_out + "/" + label + ".bin").c_str(), "wb");
    if (!f || fwrite(host.data(), 1, bytes, f) != bytes) { fprintf(stderr, DRIVER_NAME ": cannot write %s.bin\n", label); exit(2); }
    fclose(f);
}

/* every table of the file on the last picture of clips of the three samplings, of a ragged one and of two with tile seams inside */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    for (const char *nm : { "crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64", "ragged24x40", "wide296x160", "i16" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int t = 0; t < g_ntables; ++t) v.push_back(resident(sid, c, (int)c.pics.size() - 1, t));
    }
    Call a = call_map(ctx, v, g_tables_dev, g_ntables, true, 7, caller, "goldens/all");
    Call b = call_map(ctx, { resident(v[1].sid, clip("crossplane420_64x48"), v[1].k, 0) }, g_tables_dev + HVQ_MAP_TABLE_BYTES, 1, false, 7, caller, "goldens/one");
    b.items[0].entry = 1;                                            /* a table of one: record 1 of the file */
    fprintf(g_res, "R goldens/n0 %d\n", hvq_map_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; made pictures of the
 * smallest geometry in the three samplings, of 72 x 24, of 136 x 40, of planes just past a tile (136 x 64; the 108 x 76 chroma of 216 x
 * 152: a tile and four dwords) and of rows of 8192, into memory of their
 * own and in place; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    std::vector<void *> keep;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<Item> items;
        for (int k = 0; k < (int)a.pics.size(); ++k) {
            items.push_back(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep, k % g_ntables));
            items.push_back(resident(sa, a, k, (k + 1) % g_ntables));
        }
        const Geom shapes[] = { { 8, 8, 2, 2 }, { 8, 8, 2, 1 }, { 8, 8, 1, 1 }, { 72, 24, 2, 2 }, { 72, 24, 1, 1 }, { 136, 40, 2, 2 }, { 136, 40, 2, 1 }, { 136, 64, 2, 2 }, { 216, 152, 2, 2 }, { 8192, 8, 2, 2 } };
        for (const Geom &g : shapes) {
            const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
            CHECK(sid);
            for (int t = 0; t < 4; ++t) {
                items.push_back(made_guarded(sid, g, false, t + g.w, (t + g.h) % g_ntables));
                items.push_back(made_guarded(sid, g, true, t + g.w + 7, (t + g.h + 1) % g_ntables));
            }
        }
        Call c = call_map(ctx, items, g_tables_dev, g_ntables, true, 7, pass ? nullptr : caller, pass ? "memory/nullstream" : "memory");
        HIP(hipStreamSynchronize(pass ? nullptr : caller));
        write_call(&c, false);
        for (size_t i = 0; i < c.items.size(); ++i) {
            if (c.items[i].form == "synth") HIP(hipFree(room_of(c.items[i])));       /* the source of a made picture that was not in place */
            HIP(hipFree(c.room[i]));
        }
    }
    for (void *p : keep) HIP(hipFree(p));
}

/* one launch, many shapes: 300 pictures of eight clips, the tables of the file in turn; the same call twice */
static void scenario_many(HvqContext *&ctx, hipStream_t caller)
{
    const char *names[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96" };
    std::vector<std::pair<int, const Clip *>> sc;
    for (const char *nm : names) sc.push_back({ decode(ctx, clip(nm)), &clip(nm) });
    std::vector<Item> items;
    for (int i = 0; i < 300; ++i) {
        const auto &s = sc[(size_t)i % sc.size()];
        items.push_back(resident(s.first, *s.second, i % (int)s.second->pics.size(), (i / (int)sc.size() + i) % g_ntables));
    }
    Call a = call_map(ctx, items, g_tables_dev, g_ntables, true, 7, caller, "many");
    Call b = call_map(ctx, items, g_tables_dev, g_ntables, true, 7, caller, "many/again");
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
}

/* each mask 1 .. 7 on pictures of the three samplings */
static void scenario_planes(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<Item> v;
    int t = 0;
    for (const char *nm : { "crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64", "wide296x160" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        v.push_back(resident(sid, c, 0, t++ % g_ntables));
        v.push_back(resident(sid, c, (int)c.pics.size() - 1, t++ % g_ntables));
    }
    std::vector<Call> calls;
    for (int planes = 1; planes <= 7; ++planes) calls.push_back(call_map(ctx, v, g_tables_dev, g_ntables, true, planes, caller, ("planes/" + std::to_string(planes)).c_str()));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
}

/* records.bin through every rule of the file (record i of the call: record i / nrules of the file through rule i % nrules), read back into
 * tables_out.bin; then, nothing waited for in between, one 8 x 8 picture per table through it: n tables for n pictures without `which` */
static void scenario_tables(HvqContext *&ctx, hipStream_t caller)
{
    const std::vector<uint8_t> rec = slurp(g_out + "/records.bin");
    const size_t rb = 3u * HVQ_HIST_BINS * sizeof(uint32_t);
    if (rec.empty() || rec.size() % rb) { fprintf(stderr, DRIVER_NAME ": no records in %s/records.bin\n", g_out.c_str()); exit(2); }
    const int nrec = (int)(rec.size() / rb), nr = (int)g_rules.size(), n = nrec * nr;
    std::vector<uint8_t> host((size_t)n * rb);
    std::vector<int> which;
    for (int i = 0; i < n; ++i) { memcpy(&host[(size_t)i * rb], &rec[(size_t)(i / nr) * rb], rb); which.push_back(i % nr); }
    uint32_t *hist = nullptr;
    uint8_t *room = nullptr;
    const size_t tb = (size_t)n * HVQ_MAP_TABLE_BYTES;
    HIP(hipMalloc((void **)&hist, host.size()));
    HIP(hipMemcpy(hist, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP(hipMalloc((void **)&room, tb + 2u * GUARD));
    std::vector<uint8_t> fill(tb + 2u * GUARD, SENTINEL);
    HIP(hipMemcpy(room, fill.data(), fill.size(), hipMemcpyHostToDevice));
    CHECK(hvq_histogram_tables(ctx, n, hist, g_rules.data(), nr, which.data(), room + GUARD, caller));
    const Geom g = { 8, 8, 2, 2 };
    const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
    CHECK(sid);
    std::vector<Item> items;
    for (int i = 0; i < n; ++i) items.push_back(made_guarded(sid, g, false, i, i));
    Call c = call_map(ctx, items, room + GUARD, n, false, 7, caller, "tables/map", "o");
    fprintf(g_res, "R tables/n0 %d\n", hvq_histogram_tables(ctx, 0, nullptr, nullptr, 0, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    HIP(hipMemcpy(fill.data(), room, fill.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (size_t i = 0; i < GUARD; ++i) same += (fill[i] == SENTINEL) + (fill[GUARD + tb + i] == SENTINEL);
    fprintf(g_res, "S tables/guards %zu %zu\n", same, 2u * GUARD);
    write_bin("tables_out", room + GUARD, tb);
    write_call(&c);
    for (const Item &p : items) HIP(hipFree(room_of(p)));
    HIP(hipFree(hist));
    HIP(hipFree(room));
}

/* histograms -> tables -> map on one stream, nothing waited for in between; then flushes that hand the slots of the pictures to later
 * ones before anything has run (late schedule): the outputs are those of the pictures as they were.  HVQ_E_STATE for a picture whose
 * slot is gone and for one that is queued; the chain again on the later pictures; a context destroyed with a chain still queued */
static void scenario_chain(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size(), ne = (int)e.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const int nr = (int)g_rules.size();
    std::vector<void *> keep;
    auto chain = [&](int sid, const Clip &c, int first, int count, const char *label, bool dump) {
        std::vector<int> sids((size_t)count, sid), ords, which;
        std::vector<Item> items;
        for (int k = 0; k < count; ++k) {
            ords.push_back(first + k); which.push_back(k % nr);
            Item p = resident(sid, c, first + k, k % nr);
            p.kk = k;                                                /* reported as the clip's pictures: a later pass decodes the same clip */
            items.push_back(p);
        }
        uint32_t *hist = nullptr;
        uint8_t *tabs = nullptr;
        HIP(hipMalloc((void **)&hist, (size_t)count * 3u * HVQ_HIST_BINS * sizeof(uint32_t)));
        HIP(hipMalloc((void **)&tabs, (size_t)count * HVQ_MAP_TABLE_BYTES));
        keep.push_back(hist); keep.push_back(tabs);
        CHECK(hvq_picture_histograms(ctx, count, sids.data(), ords.data(), nullptr, HVQ_HIST_VALUES, nullptr, hist, caller));
        CHECK(hvq_histogram_tables(ctx, count, hist, g_rules.data(), nr, which.data(), tabs, caller));
        Call call = call_map(ctx, items, tabs, count, false, 7, caller, label, "r:");
        if (dump) { HIP(hipStreamSynchronize(caller)); write_bin("chain", tabs, (size_t)count * HVQ_MAP_TABLE_BYTES); }
        return call;
    };
    Call c = chain(sa, a, 0, n, "chain", false);
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        void *d = c.room[0] + GUARD;
        const int zero = 0;
        fprintf(g_res, "R chain/evicted %d\n", hvq_map_pictures(ctx, 1, &sa, &zero, nullptr, g_tables_dev, 1, nullptr, 7, &d, caller));
        CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));
        const int queued = 3 * n;
        fprintf(g_res, "R chain/queued %d\n", hvq_map_pictures(ctx, 1, &sa, &queued, nullptr, g_tables_dev, 1, nullptr, 7, &d, caller));
        CHECK(hvq_flush(ctx));
    }
    Call d = chain(sa, a, 2 * n, n, "chain/late", true);
    Call f = chain(se, e, 0, ne, "chain/destroy", false);
    hvq_context_destroy(ctx);
    ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&f);
    for (void *p : keep) HIP(hipFree(p));
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

    const size_t nb = bytes_of(geom_of(a)), rb = 3u * HVQ_HIST_BINS * sizeof(uint32_t), bytes = 2u * nb + 16u + 2u * HVQ_MAP_TABLE_BYTES;
    void *out = nullptr, *mem = nullptr;
    HIP(hipMalloc(&out, bytes));
    HIP(hipMalloc(&mem, std::max(nb, 2u * rb) + 32u));
    std::vector<uint8_t> sent(bytes, SENTINEL);
    HIP(hipMemcpy(out, sent.data(), sent.size(), hipMemcpyHostToDevice));
    uint8_t *o = (uint8_t *)out, *o1 = o + nb, *ot = o + 2u * nb + 16u;
    const uint8_t *T = g_tables_dev;
    const int two[2] = { 0, 0 };
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const uint8_t *tables, int nt,
                      const int *which, int planes, uint8_t *p1) {
        void *dst[2] = { o, p1 };
        fprintf(g_res, "R refused/%s %d\n", label, hvq_map_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), tables, nt, which, planes, dst, caller));
    };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 7, o1);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, T, 1, nullptr, 7, o1);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, T, 1, nullptr, 7, o1);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, T, 1, nullptr, 7, o1);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, T, 1, nullptr, 7, o1);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, T, 1, nullptr, 7, o1);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, T, 1, nullptr, 7, o1);
    refuse("null_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 7, nullptr);
    refuse("misaligned_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 7, o1 + 8);
    refuse("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 7, o1);
    refuse("null_tables", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, 1, nullptr, 7, o1);
    refuse("misaligned_tables", ctx, 2, { sa, sa }, { 0, 1 }, {}, T + 8, 1, nullptr, 7, o1);
    refuse("ntables_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 0, nullptr, 7, o1);
    refuse("ntables_65536", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 65536, two, 7, o1);
    refuse("ntables_3_without_which", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 3, nullptr, 7, o1);
    const int w_hi[2] = { 0, 1 }, w_lo[2] = { 0, -1 };
    refuse("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, w_hi, 7, o1);
    refuse("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, w_lo, 7, o1);
    refuse("planes_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 0, o1);
    refuse("planes_8", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, 8, o1);
    refuse("planes_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, T, 1, nullptr, -1, o1);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, T, 1, nullptr, 7, o1);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, T, 1, nullptr, 7, o1);
    fprintf(g_res, "R refused/n0 %d\n", hvq_map_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, caller));
    /* hvq_histogram_tables: two records in `mem`, the tables behind the pictures' outputs */
    const HvqTableRule good = g_rules[0];
    const uint32_t *H = (const uint32_t *)mem;
    auto refuse_t = [&](const char *label, HvqContext *cx, int n, const uint32_t *hist, const HvqTableRule *rules, int nrules, const int *which, uint8_t *tables) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_histogram_tables(cx, n, hist, rules, nrules, which, tables, caller));
    };
    refuse_t("t_null_context", nullptr, 2, H, &good, 1, nullptr, ot);
    refuse_t("t_null_hist", ctx, 2, nullptr, &good, 1, nullptr, ot);
    refuse_t("t_misaligned_hist", ctx, 2, H + 1, &good, 1, nullptr, ot);
    refuse_t("t_null_tables", ctx, 2, H, &good, 1, nullptr, nullptr);
    refuse_t("t_misaligned_tables", ctx, 2, H, &good, 1, nullptr, ot + 8);
    refuse_t("t_null_rules", ctx, 2, H, nullptr, 1, nullptr, ot);
    refuse_t("t_nrules_0", ctx, 2, H, &good, 0, nullptr, ot);
    {
        std::vector<HvqTableRule> many(65, good);
        refuse_t("t_nrules_65", ctx, 2, H, many.data(), 65, two, ot);
    }
    refuse_t("t_which_high", ctx, 2, H, &good, 1, w_hi, ot);
    refuse_t("t_which_negative", ctx, 2, H, &good, 1, w_lo, ot);
    refuse_t("t_too_many", ctx, 65536, H, &good, 1, nullptr, ot);
    refuse_t("t_negative_n", ctx, -1, H, &good, 1, nullptr, ot);
    /* the malformed rules: each in the chroma plane of the second entry of a table whose first is well formed and the only one used */
    auto bad = [&](const char *label, void (*spoil)(HvqTablePlane *)) {
        HvqTableRule tab[2] = { good, good };
        memset(&tab[1].chroma, 0, sizeof tab[1].chroma);
        spoil(&tab[1].chroma);
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_table_check(&tab[1]));
        refuse_t(label, ctx, 2, H, tab, 2, two, ot);
    };
    bad("kind_5", [](HvqTablePlane *p) { p->kind = 5; });
    bad("kind_negative", [](HvqTablePlane *p) { p->kind = -1; });
    bad("flat_256", [](HvqTablePlane *p) { p->kind = HVQ_TBL_FLAT; p->a = 256; });
    bad("flat_negative", [](HvqTablePlane *p) { p->kind = HVQ_TBL_FLAT; p->a = -1; });
    bad("flat_b", [](HvqTablePlane *p) { p->kind = HVQ_TBL_FLAT; p->b = 1; });
    bad("stretch_500", [](HvqTablePlane *p) { p->kind = HVQ_TBL_STRETCH; p->a = 500; });
    bad("stretch_b_500", [](HvqTablePlane *p) { p->kind = HVQ_TBL_STRETCH; p->b = 500; });
    bad("stretch_negative", [](HvqTablePlane *p) { p->kind = HVQ_TBL_STRETCH; p->b = -1; });
    bad("equalize_a", [](HvqTablePlane *p) { p->kind = HVQ_TBL_EQUALIZE; p->a = 1; });
    bad("otsu_b", [](HvqTablePlane *p) { p->kind = HVQ_TBL_OTSU; p->b = 1; });
    bad("identity_a", [](HvqTablePlane *p) { p->kind = HVQ_TBL_IDENTITY; p->a = 1; });
    bad("pad", [](HvqTablePlane *p) { p->pad = 1; });
    fprintf(g_res, "R refused/check_null %d\n", hvq_table_check(nullptr));
    for (size_t i = 0; i < g_rules.size(); ++i) fprintf(g_res, "R refused/check_good_%s %d\n", g_names[i].c_str(), hvq_table_check(&g_rules[i]));
    fprintf(g_res, "R refused/t_n0 %d\n", hvq_histogram_tables(ctx, 0, nullptr, nullptr, 0, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works, with the last table of the file */
    CHECK(hvq_flush(ctx));
    {
        Call c = call_map(ctx, { resident(sa, a, 1, g_ntables - 1), resident(sd, d, last, 0) }, g_tables_dev, g_ntables, true, 7, caller, "refused/then_ok");
        HIP(hipStreamSynchronize(caller));
        write_call(&c);
    }
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_map_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_inputs();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_map_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "goldens") run_scenario(scenario_goldens);
    else if (sc == "memory") run_scenario(scenario_memory);
    else if (sc == "many") run_scenario(scenario_many);
    else if (sc == "planes") run_scenario(scenario_planes);
    else if (sc == "tables") run_scenario(scenario_tables);
    else if (sc == "chain") run_scenario(scenario_chain);
    else if (sc == "refused") run_scenario(scenario_refused);
    else { fprintf(stderr, "fake_map_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    HIP(hipFree(g_tables_dev));
    fclose(g_res);
    return 0;
}
