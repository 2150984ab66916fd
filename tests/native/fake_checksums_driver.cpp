/*
 * tests/native/fake_checksums_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_checksums of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_checksums.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_checksums_cpu.py compares with tests/checksums_ref.py
 * on the oracle's pictures.
 *
 *   fake_checksums_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   C <label> <clip> <ordinal> <form> <8 numbers>     one record read back: crc32 Y, U, V, picture, adler32 Y, U, V, picture
 *       form: pic (the resident picture), inv (the caller's memory: the picture with every byte inverted, 255 - x)
 *   R <label> <return code>                           a return code the test wants to see
 *   E <label> <text>                                  the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>     an output buffer after refused calls
 * Caller-side resources (a stream, output records, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_checksums_driver"
#include "fake_record_driver.h"

/* one picture of a call and what the test is told about it */
struct Item { int sid, k; const void *src; std::string clip, form; int kk; };

static Item resident(int sid, const Clip &c, int k) { return Item{ sid, k, nullptr, c.name, "pic", k }; }

/* the caller's memory: picture k of stream sid read back, every byte inverted, in device memory at `offset` bytes into an allocation */
static Item in_memory(HvqContext *ctx, int sid, const Clip &c, int k, size_t offset, std::vector<void *> *keep)
{
    return Item{ sid, -1, uploaded(inverted(ctx, sid, k), offset, keep), c.name, "inv", k };
}

struct Call { uint64_t *out; std::vector<Item> items; std::string label; };

/* queue one call on `caller`; out is filled with 0xFF bytes first (the call must replace every one of them) */
static Call call_checksums(HvqContext *ctx, const std::vector<Item> &items, bool null_src, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    for (const Item &p : items) { sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); }
    void *out = record_room((size_t)n * 64u);
    CHECK(hvq_picture_checksums(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), (uint64_t *)out, caller));
    return Call{ (uint64_t *)out, items, label };
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const std::vector<uint64_t> host = take_records(&c->out, c->items.size() * 8u);
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        fprintf(g_res, "C %s %s %d %s", c->label.c_str(), p.clip.c_str(), p.kk, p.form.c_str());
        for (int v = 0; v < 8; ++v) fprintf(g_res, " %llu", (unsigned long long)host[i * 8u + (size_t)v]);
        fprintf(g_res, "\n");
    }
}

static const char *SIX[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8" };

/* six clips of three samplings in one context: per clip one call over its pictures (src = NULL), then one call over all clips with the
 * pictures interleaved, a call of one picture, and n == 0 */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    for (const char *nm : SIX) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Item> items;
        for (int k = 0; k < (int)c.pics.size(); ++k) items.push_back(resident(sid, c, k));
        calls.push_back(call_checksums(ctx, items, true, caller, "goldens/clip"));
    }
    std::vector<Item> mixed;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) mixed.push_back(resident(s.first, *s.second, (round * 3 + 1) % (int)s.second->pics.size()));
    calls.push_back(call_checksums(ctx, mixed, false, caller, "goldens/mixed"));
    calls.push_back(call_checksums(ctx, { resident(sc[1].first, *sc[1].second, 1) }, false, caller, "goldens/one"));
    fprintf(g_res, "R goldens/n0 %d\n", hvq_picture_checksums(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; on the caller's stream
 * and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sb = decode(ctx, b);
    std::vector<void *> keep;
    std::vector<Item> items;
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        items.push_back(in_memory(ctx, sa, a, k, k & 1 ? 16 : 0, &keep));
        items.push_back(resident(sa, a, k));
    }
    items.push_back(in_memory(ctx, sb, b, 1, 16, &keep));
    items.push_back(resident(sb, b, 1));
    Call c = call_checksums(ctx, items, false, caller, "memory");
    Call d = call_checksums(ctx, items, false, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    for (void *p : keep) HIP(hipFree(p));
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the records are those of the pictures as they were */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    std::vector<Item> items;
    for (int k = 0; k < n; ++k) items.push_back(resident(sa, a, k));
    Call c = call_checksums(ctx, items, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_checksums(ctx, 1, &sa, &items[0].k, nullptr, c.out, caller));
    /* the newest pictures, with a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    std::vector<Item> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Item p = resident(sa, a, 2 * n + k);
        late_call.push_back(p);
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_checksums(ctx, late_call, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(resident(se, e, k));
    Call f = call_checksums(ctx, other, false, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

/* two calls back to back on one stream, nothing waited for in between: they share the context's accumulators.  A small call, then a
 * larger one (the accumulators grow with the first still queued), then the small one again */
static void scenario_backtoback(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("wide296x160"), &b = clip("gop64x48_15");
    const int sa = decode(ctx, a), sb = decode(ctx, b);
    std::vector<Item> small, large;
    for (int k = 0; k < 2; ++k) small.push_back(resident(sa, a, k));
    for (int rep = 0; rep < 6; ++rep) {
        for (int k = 0; k < (int)b.pics.size(); ++k) large.push_back(resident(sb, b, k));
        for (int k = 0; k < (int)a.pics.size(); ++k) large.push_back(resident(sa, a, k));
    }
    Call c = call_checksums(ctx, small, false, caller, "backtoback/small");
    Call d = call_checksums(ctx, large, false, caller, "backtoback/large");
    Call e = call_checksums(ctx, small, false, caller, "backtoback/again");
    Call f = call_checksums(ctx, large, false, caller, "backtoback/large2");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    write_call(&f);
}

/* every refusal of the specification, into one sentinel-filled buffer that must come back untouched */
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

    Sentinels sent;
    void *out = sent.room(2u * 64u + 8u), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    uint64_t *o = (uint64_t *)out;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, uint64_t *dst) {
        write_code("refused", label, hvq_picture_checksums(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), dst, caller));
    };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, o);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, o);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, o);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, o);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, o);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, o);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, o);
    refuse("null_out", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr);
    refuse("misaligned_out", ctx, 2, { sa, sa }, { 0, 1 }, {}, (uint64_t *)((uint8_t *)out + 4));
    refuse("too_many", ctx, 65536, { sa }, { 0 }, {}, o);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, o);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, o);
    write_code("refused", "n0", hvq_picture_checksums(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_checksums(ctx, { resident(sa, a, 1), resident(sd, d, last) }, false, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "reuse", scenario_reuse },
                                     { "backtoback", scenario_backtoback }, { "refused", scenario_refused } });
}
