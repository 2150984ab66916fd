/*
 * tests/native/fake_motion_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_motion of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_motion.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_motion_cpu.py compares with tests/motion_ref.py on the
 * oracle's pictures.
 *
 *   fake_motion_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   F <label> <clip> <a ordinal> <b form> <b ordinal> <block> <radius> <rows> <cols> <rows * cols * 4 numbers>     one field read back
 *       b form: pic (a resident reference), mem (the caller's memory: a copy of that picture of the clip)
 *   R <label> <return code>                           a return code the test wants to see
 *   E <label> <text>                                  the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>     the fields after refused calls
 *   G <label> <guard bytes that still hold the sentinel> <guard bytes>     the 64 bytes on either side of every field of the label's calls
 * Caller-side resources (a stream, fields, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_motion_driver"
#include "fake_record_driver.h"

static const size_t GUARD = 64;

/* the reference of a pair: a resident picture (mem == NULL) or the caller's memory, and what the test is told about it */
struct Ref { int sid, k; const void *mem; const char *form; int kk; };
struct Item { const Clip *clip; int sid, k, kk; Ref b; };      /* kk: the ordinal the test is told (the clip's picture) */

static Ref resident(int sid, int k) { return Ref{ sid, k, nullptr, "pic", k }; }

/* the caller's memory: picture k of stream sid read back into device memory at `offset` bytes into an allocation */
static Ref in_memory(HvqContext *ctx, int sid, int k, size_t offset, std::vector<void *> *keep)
{
    return Ref{ -1, 0, uploaded(read_back(ctx, sid, k), offset, keep), "mem", k };
}

struct Call { std::vector<void *> alloc; std::vector<size_t> bytes; std::vector<Item> items; std::string label; int block, radius; };

static size_t field_bytes(const Clip &c, int block) { return (size_t)(c.info.width / block) * (size_t)(c.info.height / block) * 16u; }

/* queue one call on `caller`; every field lies between two guards in an allocation of its own, all of it filled with 0xEE bytes first
 * (the call must replace every byte of the field and none of the guards) */
static Call call_motion(HvqContext *ctx, const std::vector<Item> &items, int block, int radius, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    Call c{ {}, {}, items, label, block, radius };
    std::vector<int> sids, ords;
    std::vector<HvqMetricsRef> ref;
    std::vector<int32_t *> out;
    for (const Item &p : items) {
        sids.push_back(p.sid); ords.push_back(p.k);
        ref.push_back(p.b.mem ? HvqMetricsRef{ -1, 0, p.b.mem } : HvqMetricsRef{ p.b.sid, p.b.k, nullptr });
        const size_t fb = field_bytes(*p.clip, block);
        void *d = nullptr;
        HIP(hipMalloc(&d, fb + 2u * GUARD));
        std::vector<uint8_t> ee(fb + 2u * GUARD, 0xEE);
        HIP(hipMemcpy(d, ee.data(), ee.size(), hipMemcpyHostToDevice));
        c.alloc.push_back(d); c.bytes.push_back(fb);
        out.push_back((int32_t *)((uint8_t *)d + GUARD));
    }
    CHECK(hvq_picture_motion(ctx, n, sids.data(), ords.data(), ref.data(), block, radius, out.data(), caller));
    return c;
}

static size_t g_guard_same, g_guard_total;

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        std::vector<uint8_t> host(c->bytes[i] + 2u * GUARD);
        HIP(hipMemcpy(host.data(), c->alloc[i], host.size(), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < GUARD; ++g) g_guard_same += (host[g] == 0xEE) + (host[GUARD + c->bytes[i] + g] == 0xEE);
        g_guard_total += 2u * GUARD;
        const int32_t *f = (const int32_t *)(host.data() + GUARD);
        fprintf(g_res, "F %s %s %d %s %d %d %d %d %d", c->label.c_str(), p.clip->name.c_str(), p.kk, p.b.form, p.b.kk, c->block, c->radius,
                p.clip->info.height / c->block, p.clip->info.width / c->block);
        for (size_t v = 0; v < c->bytes[i] / 4u; ++v) fprintf(g_res, " %d", f[v]);
        fprintf(g_res, "\n");
        HIP(hipFree(c->alloc[i]));
    }
    c->alloc.clear();
}

static void write_guards(const char *label)
{
    fprintf(g_res, "G %s %zu %zu\n", label, g_guard_same, g_guard_total);
}

static const char *SIX[] = { "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8" };

/* six clips of three samplings in one context: per clip every picture against its predecessor at B = 8 with R = 15 and R = 3, and at
 * B = 16 with R = 15 where blocks of 16 tile the clip; one call over all clips interleaved; a call of one picture against itself; n == 0 */
static void scenario_goldens(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<std::pair<int, const Clip *>> sc;
    std::vector<Call> calls;
    for (const char *nm : SIX) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        sc.push_back({ sid, &c });
        std::vector<Item> prev;
        for (int k = 1; k < (int)c.pics.size(); ++k) prev.push_back(Item{ &c, sid, k, k, resident(sid, k - 1) });
        calls.push_back(call_motion(ctx, prev, 8, 15, caller, "goldens/b8r15"));
        calls.push_back(call_motion(ctx, prev, 8, 3, caller, "goldens/b8r3"));
        if (c.info.width % 16 == 0 && c.info.height % 16 == 0) calls.push_back(call_motion(ctx, prev, 16, 15, caller, "goldens/b16r15"));
    }
    std::vector<Item> mixed;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) {
            const int n = (int)s.second->pics.size(), k = (round * 2 + 1) % n;
            mixed.push_back(Item{ s.second, s.first, k, k, resident(s.first, (k + n - 1) % n) });
        }
    calls.push_back(call_motion(ctx, mixed, 8, 15, caller, "goldens/mixed"));
    calls.push_back(call_motion(ctx, { Item{ sc[1].second, sc[1].first, 1, 1, resident(sc[1].first, 1) } }, 8, 7, caller, "goldens/self"));
    fprintf(g_res, "R goldens/n0 %d\n", hvq_picture_motion(ctx, 0, nullptr, nullptr, nullptr, 8, 15, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    for (Call &c : calls) write_call(&c);
    write_guards("goldens");
    for (auto &s : sc) CHECK(hvq_stream_close(ctx, s.first));
}

/* the caller's memory as b, at the start of an allocation and 16 bytes into one, mixed with resident references and with a reference of
 * another stream of the same geometry, two streams of different sizes in one call; on the caller's stream and on the null stream */
static void scenario_memory(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48"), &b = clip("ragged24x40");
    const int sa = decode(ctx, a), sb = decode(ctx, b), sa2 = decode(ctx, a);
    const int na = (int)a.pics.size();
    std::vector<void *> keep;
    std::vector<Item> items;
    for (int k = 0; k < na; ++k) {
        items.push_back(Item{ &a, sa, k, k, in_memory(ctx, sa, (k + 1) % na, k & 1 ? 16 : 0, &keep) });
        items.push_back(Item{ &a, sa, k, k, resident(sa2, (k + 2) % na) });                 /* a reference of another stream */
    }
    items.push_back(Item{ &b, sb, 0, 0, in_memory(ctx, sb, 1, 16, &keep) });
    items.push_back(Item{ &b, sb, 2, 2, resident(sb, 1) });
    Call c = call_motion(ctx, items, 8, 15, caller, "memory/b8r15");
    Call d = call_motion(ctx, items, 8, 0, caller, "memory/b8r0");
    Call e = call_motion(ctx, items, 8, 5, nullptr, "memory/nullstream");
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    write_guards("memory");
    for (void *p : keep) HIP(hipFree(p));
}

/* calls queued on the caller's stream, then flushes that hand the slots of their pictures to later ones, nothing waited for in between:
 * the later writer of a slot waits, the fields are those of the pictures as they were.  Then a picture of the batch in flight, as a and
 * as b: the call ends that batch itself */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    std::vector<Item> first;
    for (int k = 0; k < n; ++k) first.push_back(Item{ &a, sa, k, k, resident(sa, (k + 1) % n) });
    Call c = call_motion(ctx, first, 8, 15, caller, "reuse/first");
    Call c2 = call_motion(ctx, first, 16, 4, caller, "reuse/first16");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    const int zero = 0, newest = 3 * n - 1;
    const HvqMetricsRef gone = { sa, 0, nullptr }, here = { sa, newest, nullptr };
    int32_t *field = (int32_t *)((uint8_t *)c.alloc[0] + GUARD);
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_motion(ctx, 1, &sa, &zero, &here, 8, 15, &field, caller));
    fprintf(g_res, "R reuse/evicted_ref %d\n", hvq_picture_motion(ctx, 1, &sa, &newest, &gone, 8, 15, &field, caller));
    /* a fourth pass begun and not ended: its pictures belong to the batch in flight */
    for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
    CHECK(hvq_flush_begin(ctx));
    std::vector<Item> flight_a, flight_b, other;
    /* reported as the clip's pictures: every pass decodes the same clip.  The ring of n + 3 slots holds the newest n + 3 pictures */
    flight_a.push_back(Item{ &a, sa, 3 * n + 2, 2, Ref{ sa, 3 * n - 1, nullptr, "pic", n - 1 } });
    Call d = call_motion(ctx, flight_a, 8, 15, caller, "reuse/inflight_a");
    for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
    CHECK(hvq_flush_begin(ctx));
    flight_b.push_back(Item{ &a, sa, 4 * n - 1, n - 1, Ref{ sa, 4 * n + 4, nullptr, "pic", 4 } });
    Call d2 = call_motion(ctx, flight_b, 8, 15, caller, "reuse/inflight_b");
    /* a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    for (int k = 1; k < (int)e.pics.size(); ++k) other.push_back(Item{ &e, se, k, k, resident(se, k - 1) });
    Call f = call_motion(ctx, other, 16, 15, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&c2);
    write_call(&d);
    write_call(&d2);
    write_call(&f);
    write_guards("reuse");
}

/* every refusal of the specification, into two sentinel-filled fields that must come back untouched */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &d = a, &g = clip("yuv422_64x48"), &q = clip("ragged24x40");
    const int sa = decode(ctx, a), sg = decode(ctx, g), sq = decode(ctx, q);
    /* a ring of 3 slots: the clip's first pictures are gone when its last ones are decoded */
    const int sd = hvq_stream_open(ctx, d.info.width, d.info.height, d.info.h_samp, d.info.v_samp, d.info.is_1_5, 3);
    CHECK(sd);
    for (const Pic &p : d.pics) CHECK(hvq_stream_submit(ctx, sd, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    const int last = (int)d.pics.size() - 1;
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    const size_t fb = field_bytes(a, 8);                                                /* the largest field a call below could write */
    Sentinels sent;
    void *out = sent.room(2u * fb + 16u), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    int32_t *o0 = (int32_t *)out, *o1 = (int32_t *)((uint8_t *)out + fb);
    typedef std::vector<HvqMetricsRef> Refs;
    typedef std::vector<int32_t *> Outs;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, Refs ref, int block, int radius, Outs dst, bool null_out = false) {
        write_code("refused", label, hvq_picture_motion(cx, n, sids.data(), ords.data(), ref.empty() ? nullptr : ref.data(), block, radius,
                                                                       null_out ? nullptr : dst.data(), caller));
    };
    const Refs ok = { { sa, 1, nullptr }, { sa, 0, nullptr } };
    const Outs oo = { o0, o1 };
    refuse("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, ok, 8, 15, oo);
    refuse("block_4", ctx, 2, { sa, sa }, { 0, 1 }, ok, 4, 15, oo);
    refuse("block_0", ctx, 2, { sa, sa }, { 0, 1 }, ok, 0, 15, oo);
    refuse("block_32", ctx, 2, { sa, sa }, { 0, 1 }, ok, 32, 15, oo);
    refuse("block_12", ctx, 2, { sa, sa }, { 0, 1 }, ok, 12, 15, oo);
    refuse("radius_16", ctx, 2, { sa, sa }, { 0, 1 }, ok, 8, 16, oo);
    refuse("radius_negative", ctx, 2, { sa, sa }, { 0, 1 }, ok, 8, -1, oo);
    refuse("block_16_does_not_tile", ctx, 2, { sa, sq }, { 0, 1 }, { { sa, 1, nullptr }, { sq, 0, nullptr } }, 16, 8, oo);
    refuse("without_ref", ctx, 2, { sa, sa }, { 0, 1 }, {}, 8, 15, oo);
    refuse("against_zeros", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { -1, 0, nullptr } }, 8, 15, oo);
    refuse("against_zeros_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { -1, 7, nullptr } }, 8, 15, oo);
    refuse("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, ok, 8, 15, oo);
    refuse("negative_stream", ctx, 2, { sa, -1 }, { 0, 0 }, ok, 8, 15, oo);
    refuse("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, ok, 8, 15, oo);
    refuse("negative_ordinal", ctx, 2, { sa, sa }, { 0, -1 }, ok, 8, 15, oo);
    refuse("ref_bad_stream", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { 99, 0, nullptr } }, 8, 15, oo);
    refuse("ref_below_minus_one", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { -2, 0, mem } }, 8, 15, oo);
    refuse("ref_bad_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { sa, 1000, nullptr } }, 8, 15, oo);
    refuse("ref_pointer_with_stream", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { sa, 0, mem } }, 8, 15, oo);
    refuse("ref_misaligned", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { -1, 0, (uint8_t *)mem + 8 } }, 8, 15, oo);
    refuse("ref_other_sampling", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { sg, 0, nullptr } }, 8, 15, oo);
    refuse("ref_other_size", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { sq, 0, nullptr } }, 8, 15, oo);
    refuse("null_out", ctx, 2, { sa, sa }, { 0, 1 }, ok, 8, 15, oo, true);
    refuse("null_field", ctx, 2, { sa, sa }, { 0, 1 }, ok, 8, 15, { o0, nullptr });
    refuse("misaligned_field", ctx, 2, { sa, sa }, { 0, 1 }, ok, 8, 15, { o0, (int32_t *)((uint8_t *)o1 + 8) });
    refuse("too_many", ctx, 65536, { sa }, { 0 }, ok, 8, 15, oo);
    refuse("evicted", ctx, 2, { sd, sd }, { last, 0 }, { { sd, last, nullptr }, { sd, last, nullptr } }, 8, 15, oo);
    refuse("evicted_ref", ctx, 2, { sd, sd }, { last, last }, { { sd, last, nullptr }, { sd, 0, nullptr } }, 8, 15, oo);
    refuse("queued", ctx, 2, { sa, sa }, { 0, queued }, ok, 8, 15, oo);
    refuse("queued_ref", ctx, 2, { sa, sa }, { 0, 1 }, { { sa, 1, nullptr }, { sa, queued, nullptr } }, 8, 15, oo);
    write_code("refused", "n0", hvq_picture_motion(ctx, 0, nullptr, nullptr, nullptr, 8, 15, nullptr, caller));
    write_code("refused", "n0_bad_block", hvq_picture_motion(ctx, 0, nullptr, nullptr, nullptr, 7, 15, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* hvq_motion_blocks */
    int32_t dims[2] = { -7, -7 };
    write_code("blocks", "64x48_8", hvq_motion_blocks(64, 48, 2, 2, 8, dims));
    fprintf(g_res, "R blocks/64x48_8_rows %d\nR blocks/64x48_8_cols %d\n", dims[0], dims[1]);
    write_code("blocks", "64x48_16", hvq_motion_blocks(64, 48, 2, 2, 16, nullptr));
    write_code("blocks", "24x40_16", hvq_motion_blocks(24, 40, 2, 2, 16, dims));
    write_code("blocks", "64x48_12", hvq_motion_blocks(64, 48, 2, 2, 12, dims));
    write_code("blocks", "geometry", hvq_motion_blocks(60, 48, 2, 2, 8, dims));
    /* the well-formed calls right after them work */
    CHECK(hvq_flush(ctx));
    Call c = call_motion(ctx, { Item{ &a, sa, 1, 1, resident(sd, last) }, Item{ &d, sd, last, last, resident(sa, 0) } }, 8, 15, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_guards("refused");
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "reuse", scenario_reuse },
                                     { "refused", scenario_refused } });
}
