/*
 * tests/native/fake_ssim_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_ssim of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_ssim.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_ssim_cpu.py compares with tests/ssim_ref.py on the
 * oracle's pictures.
 *
 *   fake_ssim_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   W <label> <clip a> <ordinal a> <form> <clip b> <ordinal b> <6 numbers>     one record read back: [Y, U, V][sum_f, windows]
 *       form: pic (a resident reference), inv (the caller's memory: picture b with every byte inverted, 255 - x)
 *   Q <label> <clip a> <ordinal a> <form> <clip b> <ordinal b> <guard words intact> <guard words> <n> <n hex words>
 *       the pair's map read back, the bits of its floats, and the sentinel words behind it
 *   R <label> <return code>                                                    a return code the test wants to see
 *   E <label> <text>                                                           the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>                     an output buffer after refused calls
 * Caller-side resources (a stream, output records, maps, reference memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_ssim_driver"
#include "fake_record_driver.h"

static const uint32_t GUARD = 0xA5A5A5A5u;
static const size_t GUARD_WORDS = 16;

/* one pair of a call and what the test is told about it */
struct Pair { int sid, k; HvqMetricsRef ref; std::string clip_a, form, clip_b; int kb; int windows; bool map; };

static int windows_of(const Clip &c)
{
    const int n = hvq_ssim_windows(c.info.width, c.info.height, c.info.h_samp, c.info.v_samp, nullptr);
    CHECK(n);
    return n;
}

static Pair against_picture(int sid, const Clip &a, int k, int sid_b, const Clip &b, int kb, bool map)
{
    return Pair{ sid, k, HvqMetricsRef{ sid_b, kb, nullptr }, a.name, "pic", b.name, kb, windows_of(a), map };
}

/* the caller's memory: picture kb of stream sid_b read back, every byte inverted, in device memory at `offset` bytes into an allocation */
static Pair against_memory(HvqContext *ctx, int sid, const Clip &a, int k, int sid_b, const Clip &b, int kb, size_t offset, bool map, std::vector<void *> *keep)
{
    return Pair{ sid, k, HvqMetricsRef{ -1, 0, uploaded(inverted(ctx, sid_b, kb), offset, keep) }, a.name, "inv", b.name, kb, windows_of(a), map };
}

struct Call { int64_t *out; std::vector<float *> maps; std::vector<Pair> pairs; std::string label; };

/* queue one call on `caller`; out and the maps are filled with 0xFF bytes first (the call must replace every one of them), behind each
 * map lie GUARD_WORDS sentinel words (the call must leave them) */
static Call call_ssim(HvqContext *ctx, const std::vector<Pair> &pairs, hipStream_t caller, const char *label)
{
    const int n = (int)pairs.size();
    std::vector<int> sids, ords;
    std::vector<HvqMetricsRef> refs;
    std::vector<float *> maps;
    bool any = false;
    for (const Pair &p : pairs) {
        sids.push_back(p.sid); ords.push_back(p.k); refs.push_back(p.ref);
        float *m = nullptr;
        if (p.map) {
            any = true;
            std::vector<uint32_t> fill((size_t)p.windows + GUARD_WORDS, 0xFFFFFFFFu);
            for (size_t g = 0; g < GUARD_WORDS; ++g) fill[(size_t)p.windows + g] = GUARD;
            HIP(hipMalloc((void **)&m, fill.size() * 4u));
            HIP(hipMemcpy(m, fill.data(), fill.size() * 4u, hipMemcpyHostToDevice));
        }
        maps.push_back(m);
    }
    void *out = record_room((size_t)n * 48u);
    CHECK(hvq_picture_ssim(ctx, n, sids.data(), ords.data(), refs.data(), (int64_t *)out, any ? maps.data() : nullptr, caller));
    return Call{ (int64_t *)out, maps, pairs, label };
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const std::vector<int64_t> host = take_records(&c->out, c->pairs.size() * 6u);
    for (size_t i = 0; i < c->pairs.size(); ++i) {
        const Pair &p = c->pairs[i];
        fprintf(g_res, "W %s %s %d %s %s %d", c->label.c_str(), p.clip_a.c_str(), p.k, p.form.c_str(), p.clip_b.c_str(), p.kb);
        for (int v = 0; v < 6; ++v) fprintf(g_res, " %lld", (long long)host[i * 6u + (size_t)v]);
        fprintf(g_res, "\n");
        if (!c->maps[i]) continue;
        std::vector<uint32_t> m((size_t)p.windows + GUARD_WORDS);
        HIP(hipMemcpy(m.data(), c->maps[i], m.size() * 4u, hipMemcpyDeviceToHost));
        size_t intact = 0;
        for (size_t g = 0; g < GUARD_WORDS; ++g) intact += m[(size_t)p.windows + g] == GUARD;
        fprintf(g_res, "Q %s %s %d %s %s %d %zu %zu %d", c->label.c_str(), p.clip_a.c_str(), p.k, p.form.c_str(), p.clip_b.c_str(), p.kb, intact, GUARD_WORDS, p.windows);
        for (int v = 0; v < p.windows; ++v) fprintf(g_res, " %x", m[(size_t)v]);
        fprintf(g_res, "\n");
        HIP(hipFree(c->maps[i]));
    }
}

static const char *SEVEN[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16" };

/* seven clips of three samplings in one context: per clip one call of (k, k - 1), (k, k) and (k, inverted k) for every picture with a map
 * for every pair, the same call without maps, then one call over all clips with the forms interleaved and a map for every other pair,
 * and a call of one pair */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    std::vector<void *> keep;
    for (const char *nm : SEVEN) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Pair> pairs;
        for (int k = 0; k < (int)c.pics.size(); ++k) {
            if (k) pairs.push_back(against_picture(sid, c, k, sid, c, k - 1, true));
            pairs.push_back(against_picture(sid, c, k, sid, c, k, true));
            pairs.push_back(against_memory(ctx, sid, c, k, sid, c, k, k & 1 ? 16 : 0, true, &keep));
        }
        calls.push_back(call_ssim(ctx, pairs, caller, "goldens/maps"));
        for (Pair &p : pairs) p.map = false;
        calls.push_back(call_ssim(ctx, pairs, caller, "goldens/nomaps"));
    }
    std::vector<Pair> mixed;
    int i = 0;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) {
            const int n = (int)s.second->pics.size(), k = (round * 3 + 1) % n;
            const bool map = i & 1;
            mixed.push_back(i % 3 == 0 ? against_picture(s.first, *s.second, k, s.first, *s.second, k ? k - 1 : n - 1, map)
                          : i % 3 == 1 ? against_memory(ctx, s.first, *s.second, k, s.first, *s.second, k, 16, map, &keep)
                                       : against_picture(s.first, *s.second, k, s.first, *s.second, k, map));
            ++i;
        }
    calls.push_back(call_ssim(ctx, mixed, caller, "goldens/mixed"));
    calls.push_back(call_ssim(ctx, { against_picture(sc[1].first, *sc[1].second, 1, sc[1].first, *sc[1].second, 0, true) }, caller, "goldens/one"));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    for (void *p : keep) HIP(hipFree(p));
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the records are those of the pictures as they were; then a call destroyed with the context while still queued */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    std::vector<Pair> pairs;
    for (int k = 0; k < n; ++k) pairs.push_back(against_picture(sa, a, k, sa, a, (k + 1) % n, (k & 1) == 0));
    Call c = call_ssim(ctx, pairs, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 4 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    const HvqMetricsRef self{ sa, 0, nullptr };
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_ssim(ctx, 1, &sa, &pairs[0].k, &self, c.out, nullptr, caller));
    /* the newest pictures, with a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    std::vector<Pair> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Pair p = against_picture(sa, a, 2 * n + k, sa, a, 2 * n + (k ? k - 1 : 0), true);
        late_call.push_back(p);
        p.k = k; p.kb = k ? k - 1 : 0;                          /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_ssim(ctx, late_call, caller, "reuse/late");
    d.pairs = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(against_picture(se, e, k, se, e, k ? k - 1 : 0, true));
    Call f = call_ssim(ctx, other, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

/* every refusal of the specification, into sentinel-filled buffers that must come back untouched */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &b = clip("yuv422_64x48"), &d = a;
    const int sa = decode(ctx, a), sb = decode(ctx, b);
    /* a ring of 3 slots: the clip's first pictures are gone when its last ones are decoded */
    const int sd = hvq_stream_open(ctx, d.info.width, d.info.height, d.info.h_samp, d.info.v_samp, d.info.is_1_5, 3);
    CHECK(sd);
    for (const Pic &p : d.pics) CHECK(hvq_stream_submit(ctx, sd, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    const int last = (int)d.pics.size() - 1;
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    const size_t bytes = 8u + 2u * 48u + 8u, mbytes = ((size_t)windows_of(a) + 2u) * 4u;         /* sentinels on both sides of out; a map with room */
    Sentinels sent;
    void *outbuf = sent.room(bytes), *map0 = sent.room(mbytes), *map1 = sent.room(mbytes), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    int64_t *o = (int64_t *)((uint8_t *)outbuf + 8);
    float *good_maps[2] = { (float *)map0, (float *)map1 };
    auto refuse = [&](const char *label, int n, std::vector<int> sids, std::vector<int> ords, std::vector<HvqMetricsRef> refs, int64_t *dst, float *const *maps) {
        write_code("refused", label, hvq_picture_ssim(ctx, n, sids.data(), ords.data(), refs.empty() ? nullptr : refs.data(), dst, maps, caller));
    };
    const HvqMetricsRef S0{ sa, 0, nullptr }, S1{ sa, 1, nullptr };
    refuse("geometry", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ sb, 1, nullptr } }, o, good_maps);
    refuse("ptr_with_stream", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ sa, 0, mem } }, o, good_maps);
    refuse("misaligned_ptr", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ -1, 0, (uint8_t *)mem + 8 } }, o, good_maps);
    refuse("bad_stream", 2, { sa, 99 }, { 0, 0 }, { S1, S0 }, o, good_maps);
    refuse("bad_ordinal", 2, { sa, sa }, { 0, 1000 }, { S1, S0 }, o, good_maps);
    refuse("bad_ref_stream", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ 99, 0, nullptr } }, o, good_maps);
    refuse("bad_ref_ordinal", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ sa, -1, nullptr } }, o, good_maps);
    refuse("ref_stream_below_minus_one", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ -2, 0, nullptr } }, o, good_maps);
    refuse("null_ref", 2, { sa, sa }, { 0, 1 }, {}, o, good_maps);
    refuse("zeros_ref", 2, { sa, sa }, { 0, 1 }, { S1, HvqMetricsRef{ -1, 0, nullptr } }, o, good_maps);
    refuse("null_out", 2, { sa, sa }, { 0, 1 }, { S1, S0 }, nullptr, good_maps);
    refuse("misaligned_out", 2, { sa, sa }, { 0, 1 }, { S1, S0 }, (int64_t *)((uint8_t *)o + 4), good_maps);
    float *bad_maps[2] = { (float *)map0, (float *)((uint8_t *)map1 + 2) };
    refuse("misaligned_map", 2, { sa, sa }, { 0, 1 }, { S1, S0 }, o, bad_maps);
    refuse("too_many", 65536, { sa }, { 0 }, { S1 }, o, nullptr);
    refuse("evicted", 2, { sd, sd }, { last, 0 }, { HvqMetricsRef{ sd, last, nullptr }, HvqMetricsRef{ sd, last, nullptr } }, o, good_maps);
    refuse("evicted_ref", 2, { sd, sd }, { last, last }, { HvqMetricsRef{ sd, last, nullptr }, HvqMetricsRef{ sd, 0, nullptr } }, o, good_maps);
    refuse("queued", 2, { sa, sa }, { 0, queued }, { S1, S0 }, o, good_maps);
    write_code("refused", "null_context", hvq_picture_ssim(nullptr, 1, &sa, &last, &S0, o, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_ssim(ctx, { against_picture(sa, a, 1, sa, a, 0, true), against_picture(sd, d, last, sd, d, last, false) }, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "reuse", scenario_reuse }, { "refused", scenario_refused } });
}
