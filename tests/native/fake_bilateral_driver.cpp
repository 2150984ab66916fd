/*
 * tests/native/fake_bilateral_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_bilateral_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_bilateral.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_bilateral_cpu.py compares with
 * hvqm4_amd.bilateral.of_picture on the oracle's pictures.
 *
 *   fake_bilateral_driver <scenario> <outdir> <golden dir>
 *
 * <outdir>/sets.txt, written by the test, names the table's entries: one a line, `<name>` and then, for luma and for chroma, `rx ry
 * <spatial: 128 hex digits> <range: 512 hex digits>` -- the members of HvqBilateralPlane in their order, pad 0.  The driver never builds
 * an entry of its own, except the malformed ones of `refused`, which it derives from the first of the file.
 *
 * results.txt, one fact per line:
 *   P <label> <source> <form> <k> <geometry: w h hs vs> <set name> <guide> <crc32 of the bytes read back> <guard>
 *       source, form, k: as fake_rank_driver's (pic, inv, synth, flat, check; smoothed:<name> -- the caller's memory: picture k through
 *       entry <name> by an earlier call, never read back in between); guide: self (no guide), copy (the caller's memory: a copy of the
 *       source), res<j> (the resident picture j of the source's stream), flat<v> (the caller's memory: every byte v), inv (the caller's
 *       memory: the source with every byte inverted); guard: 1 when the 256 bytes before and behind the output still hold the sentinel
 *   R <label> <return code>                           a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the output buffers after refused calls
 *   E <label> <the library's words for the refusal>
 * Caller-side resources (a stream, outputs, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_bilateral_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

static std::vector<std::string> g_names;             /* the entries of sets.txt in their order */
static std::vector<HvqBilateral> g_sets;

static void unhex(const std::string &hex, uint8_t *out, size_t n, const std::string &name)
{
    if (hex.size() != 2 * n) { fprintf(stderr, DRIVER_NAME ": sets.txt: a table of %s has %zu hex digits, not %zu\n", name.c_str(), hex.size(), 2 * n); exit(2); }
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
}

static void load_sets()
{
    std::ifstream f(g_out + "/sets.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name;
        if (!(in >> name)) continue;
        HvqBilateral b;
        memset(&b, 0, sizeof b);
        for (HvqBilateralPlane *p : { &b.luma, &b.chroma }) {
            std::string sp, rg;
            in >> p->rx >> p->ry >> sp >> rg;
            if (!in) { fprintf(stderr, DRIVER_NAME ": sets.txt: the line of %s is short\n", name.c_str()); exit(2); }
            unhex(sp, &p->spatial[0][0], 64, name);
            unhex(rg, p->range, 256, name);
        }
        g_names.push_back(name);
        g_sets.push_back(b);
    }
    if (g_sets.empty()) { fprintf(stderr, DRIVER_NAME ": no entries in %s/sets.txt\n", g_out.c_str()); exit(2); }
}

/* an item of a call with its guide: what the library gets, and what the P line says of it */
struct Guided { Item item; HvqMetricsRef guide; std::string gform; };

static const HvqMetricsRef SELF = { -1, 0, nullptr };
static Guided self_guided(const Item &p) { return Guided{ p, SELF, "self" }; }

struct Call { std::vector<uint8_t *> room; std::vector<Guided> items; std::string label; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes before and behind the picture.
 * use_which: the whole table of sets.txt and `which`; otherwise every item names the same entry, passed alone without `which`.
 * null_guide: guide == NULL (every item guides itself) */
static Call call_bil(HvqContext *ctx, const std::vector<Guided> &items, bool null_src, bool null_guide, bool use_which, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<HvqMetricsRef> guide;
    std::vector<void *> dst;
    Call c{ {}, items, label };
    for (const Guided &q : items) {
        const Item &p = q.item;
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); which.push_back(p.entry); guide.push_back(q.guide);
        c.room.push_back(guarded_room(bytes_of(p.g)));
        dst.push_back(c.room.back() + GUARD);
    }
    if (use_which) CHECK(hvq_bilateral_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), null_guide ? nullptr : guide.data(), g_sets.data(), (int)g_sets.size(), which.data(), dst.data(), caller));
    else CHECK(hvq_bilateral_pictures(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), null_guide ? nullptr : guide.data(), &g_sets[(size_t)items[0].item.entry], 1, nullptr, dst.data(), caller));
    return c;
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i].item;
        const ReadBack r = read_room(c->room[i], bytes_of(p.g));
        fprintf(g_res, "P %s %s %s %d %d %d %d %d %s %s %u %d\n", c->label.c_str(), p.source.c_str(), p.form.c_str(), p.kk, p.g.w, p.g.h, p.g.hs, p.g.vs,
                g_names[(size_t)p.entry].c_str(), c->items[i].gform.c_str(), r.crc, r.guard);
        HIP(hipFree(c->room[i]));
    }
    c->room.clear();
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; made pictures of the
 * smallest geometry in the three samplings, of 72 x 24 and of 136 x 40, random, flat and the 0 / 255 checkerboard, through every entry;
 * on the caller's stream and on the null stream; no guides, once with guide == NULL and once with an array of {-1, 0, NULL} */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    std::vector<void *> keep;
    std::vector<Guided> items;
    const int nf = (int)g_sets.size();
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        items.push_back(self_guided(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep, k % nf)));
        items.push_back(self_guided(resident(sa, a, k, (k + 1) % nf)));
    }
    const Geom shapes[] = { { 8, 8, 2, 2 }, { 8, 8, 2, 1 }, { 8, 8, 1, 1 }, { 72, 24, 2, 2 }, { 72, 24, 1, 1 }, { 136, 40, 2, 2 }, { 136, 40, 2, 1 } };
    for (const Geom &g : shapes) {
        const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
        CHECK(sid);
        for (int f = 0; f < nf; ++f) {
            items.push_back(self_guided(made(sid, g, "synth", f + g.w, &keep, f)));
            items.push_back(self_guided(made(sid, g, "check", f & 1, &keep, f)));
        }
        items.push_back(self_guided(made(sid, g, "flat", 201, &keep, g.w % nf)));
    }
    Call c = call_bil(ctx, items, false, true, true, caller, "memory");
    Call d = call_bil(ctx, items, false, false, true, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    for (void *p : keep) HIP(hipFree(p));
}

/* every form of a guide, mixed with unguided pictures in one call, through every entry: clips of two samplings, one with tile seams
 * inside its planes; the planes of radius 0 through both bodies */
static void scenario_guides(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<Guided> items;
    const int nf = (int)g_sets.size();
    for (const char *nm : { "yuv422_64x48", "wide296x160", "crossplane444_48x64" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c), n = (int)c.pics.size();
        const Geom g = geom_of(c);
        for (int f = 0; f < nf; ++f) {
            const int k = f % n, j = (f + 1) % n;
            const Item p = resident(sid, c, k, f);
            switch (f % 5) {
            case 0: items.push_back(self_guided(p)); break;
            case 1: items.push_back(Guided{ p, { -1, 0, uploaded(read_back(ctx, sid, k), f & 2 ? 16 : 0, &keep) }, "copy" }); break;
            case 2: items.push_back(Guided{ p, { sid, j, nullptr }, "res" + std::to_string(j) }); break;
            case 3: items.push_back(Guided{ p, { -1, 0, uploaded(filled(g, "flat", 90 + f), 0, &keep) }, "flat" + std::to_string(90 + f) }); break;
            default: items.push_back(Guided{ p, { -1, 0, uploaded(inverted(ctx, sid, k), 0, &keep) }, "inv" }); break;
            }
        }
        /* the caller's memory guided by a resident picture */
        items.push_back(Guided{ in_memory(ctx, sid, c, 0, 0, &keep, 1 % nf), { sid, n - 1, nullptr }, "res" + std::to_string(n - 1) });
    }
    Call a = call_bil(ctx, items, false, false, true, caller, "guides");
    fprintf(g_res, "R guides/force %d\n", hvq_bilateral_force_general(ctx, 1));
    Call b = call_bil(ctx, items, false, false, true, caller, "guides/general");
    fprintf(g_res, "R guides/unforce %d\n", hvq_bilateral_force_general(ctx, 0));
    HIP(hipStreamSynchronize(caller));
    write_call(&a);
    write_call(&b);
    for (void *p : keep) HIP(hipFree(p));
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures (and of its resident guides) to later ones,
 * nothing waited for in between: the outputs are those of the pictures as they were.  Then the smoothed pictures straight into a second
 * call as its sources, nothing waited for in between (what a consumer of src= does), and a context destroyed with a call still queued */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const int f0 = 1 % (int)g_sets.size(), f1 = 2 % (int)g_sets.size();
    std::vector<Guided> items;
    for (int k = 0; k < n; ++k) {
        const int j = (k + 1) % n;
        items.push_back(k & 1 ? Guided{ resident(sa, a, k, f0), { sa, j, nullptr }, "res" + std::to_string(j) } : self_guided(resident(sa, a, k, f0)));
    }
    Call c = call_bil(ctx, items, false, false, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        void *d = c.room[0] + GUARD;
        fprintf(g_res, "R reuse/evicted %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &items[0].item.k, nullptr, nullptr, &g_sets[(size_t)f0], 1, nullptr, &d, caller));
        const HvqMetricsRef gone = { sa, 0, nullptr };
        const int late = 2 * n;
        fprintf(g_res, "R reuse/evicted_guide %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &late, nullptr, &gone, &g_sets[(size_t)f0], 1, nullptr, &d, caller));
    }
    std::vector<Guided> chain;
    for (int k = 0; k < n; ++k) {
        /* the form names the first call's entry: even pictures were smoothed unguided; the test follows only those */
        if (k & 1) continue;
        chain.push_back(self_guided(Item{ { sa, -1, c.room[(size_t)k] + GUARD, a.name, "smoothed:" + g_names[(size_t)f0], k, geom_of(a) }, f1 }));
    }
    Call g = call_bil(ctx, chain, false, true, false, caller, "reuse/chain");
    std::vector<Guided> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Item p = resident(sa, a, 2 * n + k, f0);
        late_call.push_back(self_guided(p));
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(self_guided(p));
    }
    Call d = call_bil(ctx, late_call, false, true, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(self_guided(resident(se, e, k, f1)));
    Call f = call_bil(ctx, other, false, true, false, caller, "reuse/destroy");
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
    const Clip &a = clip("gop64x48_15"), &d = a, &other = clip("yuv444_64x48");
    const int sa = decode(ctx, a), so = decode(ctx, other);
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
    const HvqBilateral good = g_sets[0];
    const int two[2] = { 0, 0 };
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, std::vector<HvqMetricsRef> guide,
                      const HvqBilateral *f, int nf, const int *which, uint8_t *p1) {
        void *dst[2] = { o, p1 };
        const int rc = hvq_bilateral_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), guide.empty() ? nullptr : guide.data(), f, nf, which, dst, caller);
        fprintf(g_res, "R refused/%s %d\n", label, rc);
        fprintf(g_res, "E %s %s\n", label, rc < 0 ? hvq_last_error_string() : "");
    };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, nullptr, o1);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, {}, &good, 1, nullptr, o1);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, {}, &good, 1, nullptr, o1);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, {}, &good, 1, nullptr, o1);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, {}, &good, 1, nullptr, o1);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, {}, &good, 1, nullptr, o1);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, {}, &good, 1, nullptr, o1);
    refuse("null_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, nullptr, nullptr);
    refuse("misaligned_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, nullptr, o1 + 8);
    refuse("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, nullptr, o1);
    refuse("null_sets", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, nullptr, 1, nullptr, o1);
    refuse("nsets_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 0, nullptr, o1);
    {
        std::vector<HvqBilateral> many(65, good);
        refuse("nsets_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, many.data(), 65, two, o1);
    }
    const int w_hi[2] = { 0, 1 }, w_lo[2] = { 0, -1 };
    refuse("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, w_hi, o1);
    refuse("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, &good, 1, w_lo, o1);
    /* the guides */
    refuse("guide_other_geometry", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { so, 0, nullptr } }, &good, 1, nullptr, o1);
    refuse("guide_stream_and_pointer", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { sa, 0, mem } }, &good, 1, nullptr, o1);
    refuse("guide_misaligned", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { -1, 0, (uint8_t *)mem + 8 } }, &good, 1, nullptr, o1);
    refuse("guide_stream_minus_2", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { -2, 0, nullptr } }, &good, 1, nullptr, o1);
    refuse("guide_bad_stream", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { 99, 0, nullptr } }, &good, 1, nullptr, o1);
    refuse("guide_bad_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { sa, 1000, nullptr } }, &good, 1, nullptr, o1);
    refuse("guide_evicted", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { sd, 0, nullptr } }, &good, 1, nullptr, o1);
    refuse("guide_queued", ctx, 2, { sa, sa }, { 0, 1 }, {}, { SELF, { sa, queued, nullptr } }, &good, 1, nullptr, o1);
    /* the malformed entries: each in the chroma plane of the second entry of a table whose first is well formed and the only one used */
    auto bad = [&](const char *label, void (*spoil)(HvqBilateralPlane *)) {
        HvqBilateral tab[2] = { good, good };
        spoil(&tab[1].chroma);
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_bilateral_check(&tab[1]));
        refuse(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, {}, tab, 2, two, o1);
    };
    bad("radius_8", [](HvqBilateralPlane *p) { p->rx = 8; });
    bad("radius_8_y", [](HvqBilateralPlane *p) { p->ry = 8; });
    bad("radius_negative", [](HvqBilateralPlane *p) { p->ry = -1; });
    bad("spatial_0", [](HvqBilateralPlane *p) { p->spatial[0][0] = 0; });
    bad("range_0", [](HvqBilateralPlane *p) { p->range[0] = 0; });
    bad("pad", [](HvqBilateralPlane *p) { p->pad[0] = 1; });
    bad("pad_1", [](HvqBilateralPlane *p) { p->pad[1] = -1; });
    fprintf(g_res, "R refused/check_null %d\n", hvq_bilateral_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_bilateral_check(&good));
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, {}, &good, 1, nullptr, o1);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, {}, &good, 1, nullptr, o1);
    fprintf(g_res, "R refused/n0 %d\n", hvq_bilateral_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    fprintf(g_res, "R refused/force_null %d\n", hvq_bilateral_force_general(nullptr, 1));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works, with a table of 64 entries and a guide */
    CHECK(hvq_flush(ctx));
    {
        std::vector<HvqBilateral> keep_all = g_sets;
        std::vector<std::string> keep_names = g_names;
        while (g_sets.size() < 64) { g_sets.push_back(keep_all[g_sets.size() % keep_all.size()]); g_names.push_back(keep_names[g_names.size() % keep_names.size()]); }
        Call c = call_bil(ctx, { Guided{ resident(sa, a, 1, 63), { sa, 2, nullptr }, "res2" }, self_guided(resident(sd, d, last, 0)) }, false, false, true, caller, "refused/then_ok");
        HIP(hipStreamSynchronize(caller));
        write_call(&c);
    }
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

/* for a driver linked WITHOUT fake_bilateral.cpp: the call checks its arguments first (HVQ_E_ARG) and a well-formed one is then refused
 * with HVQ_E_NOGPU; nothing is written */
static void scenario_nogpu(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15");
    const int sa = decode(ctx, a);
    const size_t nb = bytes_of(geom_of(a));
    uint8_t *room = guarded_room(nb);
    void *dst = room + GUARD;
    const int zero = 0, high = 1;
    const HvqMetricsRef wrong = { sa, 0, room };
    HvqBilateral bad = g_sets[0];
    bad.chroma.range[0] = 0;
    fprintf(g_res, "R nogpu/bad_which %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &zero, nullptr, nullptr, &g_sets[0], 1, &high, &dst, caller));
    fprintf(g_res, "R nogpu/bad_set %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &zero, nullptr, nullptr, &bad, 1, nullptr, &dst, caller));
    fprintf(g_res, "R nogpu/bad_guide %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &zero, nullptr, &wrong, &g_sets[0], 1, nullptr, &dst, caller));
    fprintf(g_res, "R nogpu/well_formed %d\n", hvq_bilateral_pictures(ctx, 1, &sa, &zero, nullptr, nullptr, &g_sets[0], 1, nullptr, &dst, caller));
    fprintf(g_res, "E well_formed %s\n", hvq_last_error_string());
    fprintf(g_res, "R nogpu/n0 %d\n", hvq_bilateral_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(nb + 2 * GUARD);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S nogpu %zu %zu\n", same, back.size());
    HIP(hipFree(room));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: " DRIVER_NAME " <scenario> <outdir> <golden dir>\n"); return 2; }
    g_out = argv[2];
    load_sets();
    return driver_main(argc, argv, { { "memory", scenario_memory }, { "guides", scenario_guides }, { "reuse", scenario_reuse }, { "refused", scenario_refused }, { "nogpu", scenario_nogpu } });
}
