/*
 * tests/native/fake_metrics_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_metrics of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_metrics.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_metrics_cpu.py compares with tests/metrics_ref.py
 * on the oracle's pictures.
 *
 *   fake_metrics_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   M <label> <clip a> <ordinal a> <form> <clip b> <ordinal b> <12 numbers>    one record read back: [Y, U, V][sum_a, sum_b, sad, sse]
 *       form: pic (a resident reference), zeros ("-" 0 for b), inv (the caller's memory: picture b with every byte inverted, 255 - x)
 *   R <label> <return code>                                                    a return code the test wants to see
 *   E <label> <text>                                                           the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>                     an output buffer after refused calls
 * Caller-side resources (a stream, output records, reference memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_metrics_driver"
#include "fake_record_driver.h"

/* one pair of a call and what the test is told about it */
struct Pair { int sid, k; HvqMetricsRef ref; std::string clip_a, form, clip_b; int kb; };

static Pair against_picture(int sid, const Clip &a, int k, int sid_b, const Clip &b, int kb) { return Pair{ sid, k, HvqMetricsRef{ sid_b, kb, nullptr }, a.name, "pic", b.name, kb }; }
static Pair against_zeros(int sid, const Clip &a, int k) { return Pair{ sid, k, HvqMetricsRef{ -1, 0, nullptr }, a.name, "zeros", "-", 0 }; }

/* the caller's memory: picture kb of stream sid_b read back, every byte inverted, in device memory at `offset` bytes into an allocation */
static Pair against_memory(HvqContext *ctx, int sid, const Clip &a, int k, int sid_b, const Clip &b, int kb, size_t offset, std::vector<void *> *keep)
{
    return Pair{ sid, k, HvqMetricsRef{ -1, 0, uploaded(inverted(ctx, sid_b, kb), offset, keep) }, a.name, "inv", b.name, kb };
}

struct Call { uint64_t *out; std::vector<Pair> pairs; std::string label; };

/* queue one call on `caller`; out is filled with 0xFF bytes first (the call must replace every one of them) */
static Call call_metrics(HvqContext *ctx, const std::vector<Pair> &pairs, bool null_ref, hipStream_t caller, const char *label)
{
    const int n = (int)pairs.size();
    std::vector<int> sids, ords;
    std::vector<HvqMetricsRef> refs;
    for (const Pair &p : pairs) { sids.push_back(p.sid); ords.push_back(p.k); refs.push_back(p.ref); }
    void *out = record_room((size_t)n * 96u);
    CHECK(hvq_picture_metrics(ctx, n, sids.data(), ords.data(), null_ref ? nullptr : refs.data(), (uint64_t *)out, caller));
    return Call{ (uint64_t *)out, pairs, label };
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const std::vector<uint64_t> host = take_records(&c->out, c->pairs.size() * 12u);
    for (size_t i = 0; i < c->pairs.size(); ++i) {
        const Pair &p = c->pairs[i];
        fprintf(g_res, "M %s %s %d %s %s %d", c->label.c_str(), p.clip_a.c_str(), p.k, p.form.c_str(), p.clip_b.c_str(), p.kb);
        for (int v = 0; v < 12; ++v) fprintf(g_res, " %llu", (unsigned long long)host[i * 12u + (size_t)v]);
        fprintf(g_res, "\n");
    }
}

static const char *SIX[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8" };

/* six clips of three samplings in one context: per clip a call of (k, k - 1), (k, k) and zeros for every picture, one call with ref = NULL,
 * then one call over all clips with the forms interleaved, and a call of one pair */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    for (const char *nm : SIX) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Pair> pairs, zeros;
        for (int k = 0; k < (int)c.pics.size(); ++k) {
            if (k) pairs.push_back(against_picture(sid, c, k, sid, c, k - 1));
            pairs.push_back(against_picture(sid, c, k, sid, c, k));
            pairs.push_back(against_zeros(sid, c, k));
            zeros.push_back(against_zeros(sid, c, k));
        }
        calls.push_back(call_metrics(ctx, pairs, false, caller, "goldens/clip"));
        calls.push_back(call_metrics(ctx, zeros, true, caller, "goldens/nullref"));
    }
    std::vector<Pair> mixed;
    for (int round = 0, i = 0; round < 2; ++round)
        for (auto &s : sc) {
            const int n = (int)s.second->pics.size(), k = (round * 3 + 1) % n;
            const int form = i++ % 3;
            mixed.push_back(form == 0 ? against_picture(s.first, *s.second, k, s.first, *s.second, k ? k - 1 : n - 1) : form == 1 ? against_zeros(s.first, *s.second, k)
                                      : against_picture(s.first, *s.second, k, s.first, *s.second, k));
        }
    calls.push_back(call_metrics(ctx, mixed, false, caller, "goldens/mixed"));
    calls.push_back(call_metrics(ctx, { against_picture(sc[1].first, *sc[1].second, 1, sc[1].first, *sc[1].second, 0) }, false, caller, "goldens/one"));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* references in the caller's memory, at the start of an allocation and 16 bytes into one; the same clip in two streams: across them */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sa2 = decode(ctx, a), sb = decode(ctx, b);
    std::vector<void *> keep;
    std::vector<Pair> pairs;
    for (int k = 0; k < (int)a.pics.size(); ++k) {
        pairs.push_back(against_memory(ctx, sa, a, k, sa, a, k ? k - 1 : k, k & 1 ? 16 : 0, &keep));
        pairs.push_back(against_picture(sa, a, k, sa2, a, k));
    }
    pairs.push_back(against_memory(ctx, sb, b, 1, sb, b, 0, 16, &keep));
    pairs.push_back(against_zeros(sb, b, 1));
    Call c = call_metrics(ctx, pairs, false, caller, "memory");
    Call d = call_metrics(ctx, pairs, false, nullptr, "memory/nullstream");
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
    std::vector<Pair> pairs;
    for (int k = 0; k < n; ++k) {
        pairs.push_back(against_picture(sa, a, k, sa, a, (k + 1) % n));
        pairs.push_back(against_zeros(sa, a, k));
    }
    Call c = call_metrics(ctx, pairs, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 4 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_metrics(ctx, 1, &sa, &pairs[0].k, nullptr, c.out, caller));
    /* the newest pictures, with a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    std::vector<Pair> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Pair p = against_picture(sa, a, 2 * n + k, sa, a, 2 * n + (k ? k - 1 : 0));
        late_call.push_back(p);
        p.k = k; p.kb = k ? k - 1 : 0;                          /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_metrics(ctx, late_call, false, caller, "reuse/late");
    d.pairs = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(against_zeros(se, e, k));
    Call f = call_metrics(ctx, other, false, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

/* every refusal of the specification, into one sentinel-filled buffer that must come back untouched */
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

    Sentinels sent;
    void *out = sent.room(2u * 96u + 8u), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    uint64_t *o = (uint64_t *)out;
    auto refuse = [&](const char *label, int n, std::vector<int> sids, std::vector<int> ords, std::vector<HvqMetricsRef> refs, uint64_t *dst) {
        write_code("refused", label, hvq_picture_metrics(ctx, n, sids.data(), ords.data(), refs.empty() ? nullptr : refs.data(), dst, caller));
    };
    const HvqMetricsRef Z{ -1, 0, nullptr };
    refuse("geometry", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ sb, 1, nullptr } }, o);
    refuse("ptr_with_stream", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ sa, 0, mem } }, o);
    refuse("misaligned_ptr", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ -1, 0, (uint8_t *)mem + 8 } }, o);
    refuse("bad_stream", 2, { sa, 99 }, { 0, 0 }, {}, o);
    refuse("bad_ordinal", 2, { sa, sa }, { 0, 1000 }, {}, o);
    refuse("bad_ref_stream", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ 99, 0, nullptr } }, o);
    refuse("bad_ref_ordinal", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ sa, -1, nullptr } }, o);
    refuse("ref_stream_below_minus_one", 2, { sa, sa }, { 0, 1 }, { Z, HvqMetricsRef{ -2, 0, nullptr } }, o);
    refuse("null_out", 2, { sa, sa }, { 0, 1 }, {}, nullptr);
    refuse("misaligned_out", 2, { sa, sa }, { 0, 1 }, {}, (uint64_t *)((uint8_t *)out + 4));
    refuse("too_many", 65536, { sa }, { 0 }, {}, o);
    refuse("evicted", 2, { sd, sd }, { last, 0 }, {}, o);
    refuse("evicted_ref", 2, { sd, sd }, { last, last }, { Z, HvqMetricsRef{ sd, 0, nullptr } }, o);
    refuse("queued", 2, { sa, sa }, { 0, queued }, {}, o);
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_metrics(ctx, { against_picture(sa, a, 1, sa, a, 0), against_zeros(sd, d, last) }, false, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "reuse", scenario_reuse },
                                     { "refused", scenario_refused } });
}
