/*
 * tests/native/fake_jpeg_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_encode_jpeg of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_jpeg.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_jpeg_cpu.py compares with tests/jpeg_ref.py on the
 * oracle's pictures.
 *
 *   fake_jpeg_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   J <label> <clip> <ordinal> <form> <quality> <cap> <length> <file in hex, or - when length > cap> <tail bytes that still hold the sentinel> <tail bytes>
 *       one file read back.  form: pic (a resident picture), mem (the caller's memory: a copy of that picture of the clip); the tail is
 *       what lies between the file's end and cap (everything within cap when the file did not fit)
 *   R <label> <return code>                           a return code the test wants to see
 *   E <label> <text>                                  the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>     the destinations and lengths after refused calls
 *   G <label> <guard bytes that still hold the sentinel> <guard bytes>     the 64 bytes on either side of every destination of the label's calls
 * Caller-side resources (a stream, destinations, lengths, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_jpeg_driver"
#include "fake_record_driver.h"
#include "../../hvqm4_amd/csrc/hvq_jpeg.h"

static const size_t GUARD = 64;
static const uint8_t SENT = 0xEE;

/* a picture of a call: resident (mem == NULL) or a copy of picture kk of the clip in the caller's memory; cap < 0: hvq_jpeg_bound */
struct Item { const Clip *clip; int sid, k, kk; const void *mem; long long cap; };

static Item resident(const Clip &c, int sid, int k, long long cap = -1) { return Item{ &c, sid, k, k, nullptr, cap }; }

static Item in_memory(HvqContext *ctx, const Clip &c, int sid, int k, size_t offset, std::vector<void *> *keep, long long cap = -1)
{
    return Item{ &c, sid, -1, k, uploaded(read_back(ctx, sid, k), offset, keep), cap };
}

struct Call { std::vector<void *> alloc; std::vector<uint64_t> cap; void *lengths; std::vector<Item> items; std::string label; int quality; };

/* queue one call on `caller`; every destination lies between two guards in an allocation of its own, all of it filled with the sentinel;
 * the lengths lie between guards too */
static Call call_jpeg(HvqContext *ctx, const std::vector<Item> &items, int quality, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    Call c{ {}, {}, nullptr, items, label, quality };
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    std::vector<void *> out;
    for (const Item &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.mem);
        const uint64_t cap = p.cap >= 0 ? (uint64_t)p.cap : hvq_jpeg_bound(p.clip->info.width, p.clip->info.height, p.clip->info.h_samp, p.clip->info.v_samp);
        void *d = nullptr;
        HIP(hipMalloc(&d, cap + 2u * GUARD));
        std::vector<uint8_t> ee(cap + 2u * GUARD, SENT);
        HIP(hipMemcpy(d, ee.data(), ee.size(), hipMemcpyHostToDevice));
        c.alloc.push_back(d); c.cap.push_back(cap);
        out.push_back((uint8_t *)d + GUARD);
    }
    HIP(hipMalloc(&c.lengths, (size_t)n * 8u + 2u * GUARD));
    std::vector<uint8_t> ee((size_t)n * 8u + 2u * GUARD, SENT);
    HIP(hipMemcpy(c.lengths, ee.data(), ee.size(), hipMemcpyHostToDevice));
    CHECK(hvq_encode_jpeg(ctx, n, sids.data(), ords.data(), src.data(), quality, out.data(), c.cap.data(), (uint64_t *)((uint8_t *)c.lengths + GUARD), caller));
    return c;
}

static size_t g_guard_same, g_guard_total;

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const size_t n = c->items.size();
    std::vector<uint8_t> lh(n * 8u + 2u * GUARD);
    HIP(hipMemcpy(lh.data(), c->lengths, lh.size(), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < GUARD; ++g) g_guard_same += (lh[g] == SENT) + (lh[GUARD + n * 8u + g] == SENT);
    g_guard_total += 2u * GUARD;
    for (size_t i = 0; i < n; ++i) {
        const Item &p = c->items[i];
        const uint64_t cap = c->cap[i];
        uint64_t len;
        memcpy(&len, lh.data() + GUARD + i * 8u, 8);
        std::vector<uint8_t> host(cap + 2u * GUARD);
        HIP(hipMemcpy(host.data(), c->alloc[i], host.size(), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < GUARD; ++g) g_guard_same += (host[g] == SENT) + (host[GUARD + cap + g] == SENT);
        g_guard_total += 2u * GUARD;
        fprintf(g_res, "J %s %s %d %s %d %llu %llu ", c->label.c_str(), p.clip->name.c_str(), p.kk, p.mem ? "mem" : "pic", c->quality, (unsigned long long)cap, (unsigned long long)len);
        const uint64_t from = len <= cap ? len : 0;
        if (len <= cap) for (uint64_t b = 0; b < len; ++b) fprintf(g_res, "%02x", host[GUARD + b]);
        else fprintf(g_res, "-");
        size_t same = 0;
        for (uint64_t b = from; b < cap; ++b) same += host[GUARD + b] == SENT;
        fprintf(g_res, " %zu %llu\n", same, (unsigned long long)(cap - from));
        HIP(hipFree(c->alloc[i]));
    }
    HIP(hipFree(c->lengths));
    c->alloc.clear();
}

static void write_guards(const char *label) { fprintf(g_res, "G %s %zu %zu\n", label, g_guard_same, g_guard_total); }

static const char *SIX[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8" };

/* six clips of three samplings in one context: per clip every picture at quality 90; one call over all clips interleaved at quality 50;
 * qualities 1 and 100 on the first two pictures of every clip; n == 0 */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    for (const char *nm : SIX) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Item> all;
        for (int k = 0; k < (int)c.pics.size(); ++k) all.push_back(resident(c, sid, k));
        calls.push_back(call_jpeg(ctx, all, 90, caller, "goldens/q90"));
    }
    std::vector<Item> mixed, two;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) {
            const int n = (int)s.second->pics.size();
            mixed.push_back(resident(*s.second, s.first, (round * 2 + 1) % n));
            two.push_back(resident(*s.second, s.first, round % n));
        }
    calls.push_back(call_jpeg(ctx, mixed, 50, caller, "goldens/mixed"));
    calls.push_back(call_jpeg(ctx, two, 1, caller, "goldens/q1"));
    calls.push_back(call_jpeg(ctx, two, 100, caller, "goldens/q100"));
    fprintf(g_res, "R goldens/n0 %d\n", hvq_encode_jpeg(ctx, 0, nullptr, nullptr, nullptr, 90, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    write_guards("goldens");
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* the caller's memory as the picture, at the start of an allocation and 16 bytes into one, mixed with resident pictures, two streams of
 * different sizes and samplings in one call; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sb = decode(ctx, b);
    const int na = (int)a.pics.size();
    std::vector<void *> keep;
    std::vector<Item> items;
    for (int k = 0; k < na; ++k) {
        items.push_back(in_memory(ctx, a, sa, (k + 1) % na, k & 1 ? 16 : 0, &keep));
        items.push_back(resident(a, sa, k));
    }
    items.push_back(in_memory(ctx, b, sb, 1, 16, &keep));
    items.push_back(resident(b, sb, 2));
    Call c = call_jpeg(ctx, items, 90, caller, "memory/q90");
    Call d = call_jpeg(ctx, items, 100, caller, "memory/q100");
    Call e = call_jpeg(ctx, items, 35, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    write_guards("memory");
    for (void *p : keep) HIP(hipFree(p));
}

/* capacities: the arguments behind the golden directory give, for pictures 0 .. 3 of gop64x48_15 at quality 90, the exact lengths (the test's reference knows them): picture
 * 1 gets one byte less than it needs, its neighbours exactly what they need; then the smallest capacity the call takes, 631; then the
 * call again with what the first reported */
static void scenario_overflow(HvqContext *&ctx, hipStream_t caller)
{
    if (g_extra.size() != 4) { fprintf(stderr, "fake_jpeg_driver: overflow takes the four exact lengths\n"); exit(2); }
    std::vector<long long> lengths;
    for (const std::string &a : g_extra) lengths.push_back(atoll(a.c_str()));
    const Clip &a = clip("gop64x48_15");
    const int sa = decode(ctx, a);
    std::vector<Item> items, tiny, again;
    for (int k = 0; k < 4; ++k) {
        items.push_back(resident(a, sa, k, lengths[(size_t)k] - (k == 1)));
        tiny.push_back(resident(a, sa, k, 631));
        again.push_back(resident(a, sa, k, lengths[(size_t)k]));
    }
    Call c = call_jpeg(ctx, items, 90, caller, "overflow/short");
    Call d = call_jpeg(ctx, tiny, 90, caller, "overflow/tiny");
    Call e = call_jpeg(ctx, again, 90, caller, "overflow/again");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    write_guards("overflow");
}

/* every refusal of the specification, into two sentinel-filled destinations and lengths that must come back untouched */
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

    const uint64_t room = hvq_jpeg_bound(a.info.width, a.info.height, a.info.h_samp, a.info.v_samp);
    const size_t stride = ((size_t)room + 15u) & ~(size_t)15u;
    Sentinels sent;
    void *out = sent.room(2u * stride + 32u), *mem = nullptr;                          /* two destinations, then the lengths */
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    uint8_t *o0 = (uint8_t *)out, *o1 = o0 + stride;
    uint64_t *len = (uint64_t *)(o0 + 2u * stride);
    typedef std::vector<void *> Outs;
    typedef std::vector<const void *> Srcs;
    typedef std::vector<uint64_t> Caps;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, Srcs src, int quality, Outs dst, Caps cap, uint64_t *lengths, int null_what = 0) {
        write_code("refused", label, hvq_encode_jpeg(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), quality,
                                                                    null_what == 1 ? nullptr : dst.data(), null_what == 2 ? nullptr : cap.data(), lengths, caller));
    };
    const Outs oo = { o0, o1 };
    const Caps cc = { room, room };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, cc, len);
    refuse("quality_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, 0, oo, cc, len);
    refuse("quality_101", ctx, 2, { sa, sa }, { 0, 1 }, {}, 101, oo, cc, len);
    refuse("quality_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, -5, oo, cc, len);
    refuse("null_out", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, cc, len, 1);
    refuse("null_cap", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, cc, len, 2);
    refuse("null_lengths", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, cc, nullptr);
    refuse("misaligned_lengths", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, cc, (uint64_t *)((uint8_t *)len + 4));
    refuse("null_destination", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, { o0, nullptr }, cc, len);
    refuse("misaligned_destination", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, { o0, o1 + 8 }, cc, len);
    refuse("cap_630", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, { room, 630 }, len);
    refuse("cap_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, 90, oo, { room, 0 }, len);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, 90, oo, cc, len);
    refuse("negative_stream", ctx, 2, { sa, -1 }, { 0, 0 }, {}, 90, oo, cc, len);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, 90, oo, cc, len);
    refuse("negative_ordinal", ctx, 2, { sa, sa }, { 0, -1 }, {}, 90, oo, cc, len);
    refuse("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, 90, oo, cc, len);
    refuse("src_misaligned", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, 90, oo, cc, len);
    refuse("src_bad_stream", ctx, 2, { sa, 99 }, { 0, -1 }, { nullptr, mem }, 90, oo, cc, len);
    refuse("too_many", ctx, 65536, { sa }, { 0 }, {}, 90, oo, cc, len);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, {}, 90, oo, cc, len);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, {}, 90, oo, cc, len);
    write_code("refused", "n0", hvq_encode_jpeg(ctx, 0, nullptr, nullptr, nullptr, 90, nullptr, nullptr, nullptr, caller));
    write_code("refused", "n0_bad_quality", hvq_encode_jpeg(ctx, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* hvq_jpeg_header and hvq_jpeg_bound */
    uint8_t hdr[700];
    size_t hl = 0;
    write_code("header", "ok", hvq_jpeg_header(64, 48, 2, 2, 90, hdr, sizeof hdr, &hl));
    fprintf(g_res, "R header/len %d\n", (int)hl);
    write_code("header", "no_len", hvq_jpeg_header(64, 48, 2, 2, 90, hdr, 629, nullptr));
    write_code("header", "short", hvq_jpeg_header(64, 48, 2, 2, 90, hdr, 628, &hl));
    write_code("header", "null", hvq_jpeg_header(64, 48, 2, 2, 90, nullptr, 700, &hl));
    write_code("header", "quality", hvq_jpeg_header(64, 48, 2, 2, 0, hdr, sizeof hdr, &hl));
    write_code("header", "geometry", hvq_jpeg_header(60, 48, 2, 2, 90, hdr, sizeof hdr, &hl));
    fprintf(g_res, "R bound/64x48 %d\n", (int)hvq_jpeg_bound(64, 48, 2, 2));
    fprintf(g_res, "R bound/geometry %d\n", (int)hvq_jpeg_bound(64, 48, 1, 2));
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_jpeg(ctx, { resident(a, sa, 1), resident(d, sd, last) }, 90, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_guards("refused");
    HIP(hipFree(mem));
}

/* the division helper the kernels and the fake body share (hvq_jpeg.h) against `/`, exhaustively: every numerator up to HVQ_JPEG_DIV_MAX
 * (1151 = the largest |F| a transform of 8-bit samples can give, 1024, plus the largest Q >> 1, 127, is below it) with every Q in
 * 1 .. 255, and hvq_jpeg_quantise on every F in [-1151, 1151] against the header text's formula */
static void scenario_helpers()
{
    long bad_div = 0, bad_q = 0, tried = 0;
    for (uint32_t q = 1; q <= 255; ++q) {
        const uint32_t m = hvq_jpeg_recip(q);
        for (uint32_t n = 0; n <= HVQ_JPEG_DIV_MAX; ++n, ++tried) bad_div += hvq_jpeg_div(n, m) != n / q;
        for (int f = -1151; f <= 1151; ++f) {
            const int a = f < 0 ? -f : f, want = (f < 0 ? -1 : 1) * (int)(((uint32_t)a + (q >> 1)) / q);
            bad_q += hvq_jpeg_quantise(f, hvq_jpeg_qpack(q)) != want;
        }
    }
    fprintf(g_res, "R helpers/tried %ld\nR helpers/div_mismatches %ld\nR helpers/quantise_mismatches %ld\n", tried, bad_div, bad_q);
    fprintf(g_res, "R helpers/div_max %u\n", HVQ_JPEG_DIV_MAX);
    for (int q : { 1, 49, 50, 100 })
        for (int t = 0; t < 2; ++t) {
            fprintf(g_res, "Q %d %d", q, t);
            for (int k = 0; k < 64; ++k) fprintf(g_res, " %u", hvq_jpeg_q(HVQ_JPEG_QBASE[t][k], q));
            fprintf(g_res, "\n");
        }
    fprintf(g_res, "G helpers 1 1\n");
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "overflow", scenario_overflow },
                                     { "refused", scenario_refused }, { "helpers", nullptr, scenario_helpers } }, " [lengths]");
}
