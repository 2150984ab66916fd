/*
 * tests/native/fake_histograms_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_histograms of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_histograms.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_histograms_cpu.py compares with tests/histograms_ref.py
 * on the oracle's pictures.
 *
 *   fake_histograms_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   H <label> <clip> <a form> <a ordinal> <b form> <b ordinal> <768 numbers>     one record read back: the bins of Y, U, V
 *       a form: pic (the resident picture), inv (the caller's memory: the picture with every byte inverted, 255 - x)
 *       b form: none (HVQ_HIST_VALUES), pic (a resident reference), inv (a reference in the caller's memory, inverted)
 *   R <label> <return code>                           a return code the test wants to see
 *   E <label> <text>                                  the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>     an output buffer after refused calls
 * Caller-side resources (a stream, output records, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_histograms_driver"
#include "fake_record_driver.h"

static const size_t REC = 3u * HVQ_HIST_BINS;           /* dwords of a record */

/* one side of a pair: a resident picture (mem == NULL) or the caller's memory, and what the test is told about it */
struct Side { int sid, k; const void *mem; const char *form; int kk; };
struct Item { std::string clip; Side a, b; };          /* b.form "none": HVQ_HIST_VALUES */

static Side resident(int sid, int k) { return Side{ sid, k, nullptr, "pic", k }; }
static Side none() { return Side{ -1, 0, nullptr, "none", 0 }; }

/* the caller's memory: picture k of stream sid read back, every byte inverted, in device memory at `offset` bytes into an allocation */
static Side in_memory(HvqContext *ctx, int sid, int k, size_t offset, std::vector<void *> *keep)
{
    return Side{ sid, -1, uploaded(inverted(ctx, sid, k), offset, keep), "inv", k };
}

struct Call { uint32_t *out; std::vector<Item> items; std::string label; };

/* queue one call on `caller`; out is filled with 0xFF bytes first (the call must replace every one of them).  The mode is that of the
 * first item: a call is all values or all differences */
static Call call_histograms(HvqContext *ctx, const std::vector<Item> &items, bool null_src, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    const bool values = !strcmp(items[0].b.form, "none");
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    std::vector<HvqMetricsRef> ref;
    for (const Item &p : items) {
        sids.push_back(p.a.sid); ords.push_back(p.a.k); src.push_back(p.a.mem);
        ref.push_back(p.b.mem ? HvqMetricsRef{ -1, 0, p.b.mem } : HvqMetricsRef{ p.b.sid, p.b.k, nullptr });
    }
    void *out = record_room((size_t)n * REC * 4u);
    CHECK(hvq_picture_histograms(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), values ? HVQ_HIST_VALUES : HVQ_HIST_ABSDIFF,
                                 values ? nullptr : ref.data(), (uint32_t *)out, caller));
    return Call{ (uint32_t *)out, items, label };
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const std::vector<uint32_t> host = take_records(&c->out, c->items.size() * REC);
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        fprintf(g_res, "H %s %s %s %d %s %d", c->label.c_str(), p.clip.c_str(), p.a.form, p.a.kk, p.b.form, p.b.kk);
        for (size_t v = 0; v < REC; ++v) fprintf(g_res, " %u", host[i * REC + v]);
        fprintf(g_res, "\n");
    }
}

static const char *SIX[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8" };

/* six clips of three samplings in one context: per clip its pictures' values (src = NULL), every picture against its predecessor and
 * against itself; then one call over all clips with the pictures interleaved, a call of one picture, and n == 0 */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    for (const char *nm : SIX) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Item> values, prev, self;
        for (int k = 0; k < (int)c.pics.size(); ++k) {
            values.push_back(Item{ c.name, resident(sid, k), none() });
            if (k) prev.push_back(Item{ c.name, resident(sid, k), resident(sid, k - 1) });
            self.push_back(Item{ c.name, resident(sid, k), resident(sid, k) });
        }
        calls.push_back(call_histograms(ctx, values, true, caller, "goldens/values"));
        if (!prev.empty()) calls.push_back(call_histograms(ctx, prev, true, caller, "goldens/prev"));
        calls.push_back(call_histograms(ctx, self, false, caller, "goldens/self"));
    }
    std::vector<Item> mixed;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) mixed.push_back(Item{ s.second->name, resident(s.first, (round * 3 + 1) % (int)s.second->pics.size()), none() });
    calls.push_back(call_histograms(ctx, mixed, false, caller, "goldens/mixed"));
    calls.push_back(call_histograms(ctx, { Item{ sc[1].second->name, resident(sc[1].first, 1), resident(sc[1].first, 0) } }, false, caller, "goldens/one"));
    fprintf(g_res, "R goldens/n0 %d\n", hvq_picture_histograms(ctx, 0, nullptr, nullptr, nullptr, HVQ_HIST_VALUES, nullptr, nullptr, caller));
    fprintf(g_res, "R goldens/n0_absdiff %d\n", hvq_picture_histograms(ctx, 0, nullptr, nullptr, nullptr, HVQ_HIST_ABSDIFF, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* the caller's memory as a and as b, at the start of an allocation and 16 bytes into one, mixed with resident pictures and with a
 * reference of another stream of the same geometry; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sb = decode(ctx, b), sa2 = decode(ctx, a);
    const int na = (int)a.pics.size();
    std::vector<void *> keep;
    std::vector<Item> values, diffs;
    for (int k = 0; k < na; ++k) {
        values.push_back(Item{ a.name, in_memory(ctx, sa, k, k & 1 ? 16 : 0, &keep), none() });
        values.push_back(Item{ a.name, resident(sa, k), none() });
        diffs.push_back(Item{ a.name, in_memory(ctx, sa, k, k & 1 ? 0 : 16, &keep), resident(sa2, (k + 1) % na) });     /* memory against another stream */
        diffs.push_back(Item{ a.name, resident(sa, k), in_memory(ctx, sa, (k + 1) % na, 16, &keep) });                  /* resident against memory */
        diffs.push_back(Item{ a.name, in_memory(ctx, sa, k, 0, &keep), in_memory(ctx, sa, (k + 2) % na, 0, &keep) });   /* memory against memory */
    }
    values.push_back(Item{ b.name, in_memory(ctx, sb, 1, 16, &keep), none() });
    diffs.push_back(Item{ b.name, resident(sb, 0), in_memory(ctx, sb, 1, 16, &keep) });
    Call c = call_histograms(ctx, values, false, caller, "memory/values");
    Call d = call_histograms(ctx, diffs, false, caller, "memory/diffs");
    Call e = call_histograms(ctx, diffs, false, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    for (void *p : keep) HIP(hipFree(p));
}

/* calls queued on the caller's stream, then flushes that hand the slots of their pictures to later ones, nothing waited for in between:
 * the records are those of the pictures as they were */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    std::vector<Item> values, diffs;
    for (int k = 0; k < n; ++k) {
        values.push_back(Item{ a.name, resident(sa, k), none() });
        diffs.push_back(Item{ a.name, resident(sa, k), resident(sa, (k + 1) % n) });
    }
    Call c = call_histograms(ctx, values, false, caller, "reuse/values");
    Call c2 = call_histograms(ctx, diffs, false, caller, "reuse/diffs");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    const int zero = 0, newest = 3 * n - 1;
    const HvqMetricsRef gone = { sa, 0, nullptr };
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_histograms(ctx, 1, &sa, &zero, nullptr, HVQ_HIST_VALUES, nullptr, c.out, caller));
    fprintf(g_res, "R reuse/evicted_ref %d\n", hvq_picture_histograms(ctx, 1, &sa, &newest, nullptr, HVQ_HIST_ABSDIFF, &gone, c.out, caller));
    /* the newest pictures, with a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    std::vector<Item> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        late_call.push_back(Item{ a.name, resident(sa, 2 * n + k), resident(sa, 2 * n + (k + 1) % n) });
        late.push_back(Item{ a.name, resident(sa, k), resident(sa, (k + 1) % n) });     /* reported as the clip's pictures: the third pass decodes the same clip */
    }
    Call d = call_histograms(ctx, late_call, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(Item{ e.name, resident(se, k), none() });
    Call f = call_histograms(ctx, other, false, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&c2);
    write_call(&d);
    write_call(&f);
}

/* every refusal of the specification, into one sentinel-filled buffer that must come back untouched */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &d = a, &g = clip("yuv422_64x48");
    const int sa = decode(ctx, a), sg = decode(ctx, g);
    /* a ring of 3 slots: the clip's first pictures are gone when its last ones are decoded */
    const int sd = hvq_stream_open(ctx, d.info.width, d.info.height, d.info.h_samp, d.info.v_samp, d.info.is_1_5, 3);
    CHECK(sd);
    for (const Pic &p : d.pics) CHECK(hvq_stream_submit(ctx, sd, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    const int last = (int)d.pics.size() - 1;
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    Sentinels sent;
    void *out = sent.room(2u * REC * 4u + 8u), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    uint32_t *o = (uint32_t *)out;
    const int V = HVQ_HIST_VALUES, D = HVQ_HIST_ABSDIFF;
    typedef std::vector<HvqMetricsRef> Refs;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, int mode,
                      Refs ref, uint32_t *dst) {
        write_code("refused", label, hvq_picture_histograms(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), mode,
                                                                           ref.empty() ? nullptr : ref.data(), dst, caller));
    };
    const Refs ok = { { sa, 1, nullptr }, { sa, 0, nullptr } };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, V, {}, o);
    refuse("null_context_absdiff", nullptr, 2, { sa, sa }, { 0, 1 }, {}, D, ok, o);
    refuse("bad_mode", ctx, 2, { sa, sa }, { 0, 1 }, {}, 2, {}, o);
    refuse("negative_mode", ctx, 2, { sa, sa }, { 0, 1 }, {}, -1, ok, o);
    refuse("values_with_ref", ctx, 2, { sa, sa }, { 0, 1 }, {}, V, ok, o);
    refuse("absdiff_without_ref", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, {}, o);
    refuse("absdiff_against_zeros", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { -1, 0, nullptr } }, o);
    refuse("absdiff_against_zeros_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { -1, 7, nullptr } }, o);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, V, {}, o);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, V, {}, o);
    refuse("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, V, {}, o);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, V, {}, o);
    refuse("src_with_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, V, {}, o);
    refuse("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, V, {}, o);
    refuse("ref_bad_stream", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { 99, 0, nullptr } }, o);
    refuse("ref_below_minus_one", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { -2, 0, mem } }, o);
    refuse("ref_bad_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { sa, 1000, nullptr } }, o);
    refuse("ref_pointer_with_stream", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { sa, 0, mem } }, o);
    refuse("ref_misaligned", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { -1, 0, (uint8_t *)mem + 8 } }, o);
    refuse("ref_other_geometry", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { sg, 0, nullptr } }, o);
    refuse("null_out", ctx, 2, { sa, sa }, { 0, 1 }, {}, V, {}, nullptr);
    refuse("misaligned_out", ctx, 2, { sa, sa }, { 0, 1 }, {}, V, {}, (uint32_t *)((uint8_t *)out + 2));
    refuse("too_many", ctx, 65536, { sa }, { 0 }, {}, V, {}, o);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, V, {}, o);
    refuse("evicted_ref", ctx, 2, { sd, sd }, { last, last }, {}, D, { { sd, last, nullptr }, { sd, 0, nullptr } }, o);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, V, {}, o);
    refuse("queued_ref", ctx, 2, { sa, sa }, { 0, 1 }, {}, D, { { sa, 1, nullptr }, { sa, queued, nullptr } }, o);
    write_code("refused", "n0", hvq_picture_histograms(ctx, 0, nullptr, nullptr, nullptr, V, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* the well-formed calls right after them work */
    CHECK(hvq_flush(ctx));
    Call c = call_histograms(ctx, { Item{ a.name, resident(sa, 1), none() }, Item{ d.name, resident(sd, last), none() } }, false, caller, "refused/then_ok");
    Call e = call_histograms(ctx, { Item{ a.name, resident(sa, 1), resident(sd, last) } }, false, caller, "refused/then_ok_absdiff");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&e);
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "reuse", scenario_reuse },
                                     { "refused", scenario_refused } });
}
