/*
 * tests/native/fake_phash_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_picture_hashes of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_phash.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_phash_cpu.py compares with tests/phash_ref.py
 * on the oracle's pictures.
 *
 *   fake_phash_driver <scenario> <outdir> <golden dir>
 *
 * results.txt, one fact per line:
 *   H <label> <clip> <ordinal> <form> <4 numbers>     one record read back: ahash, dhash, phash, sum_y
 *       form: pic (the resident picture), inv (the caller's memory: the picture with every byte inverted, 255 - x)
 *   R <label> <return code>                           a return code the test wants to see
 *   E <label> <text>                                  the library's words for the R line before it, to the end of the line (`refused` only)
 *   S <label> <bytes that still hold the sentinel> <bytes>     an output buffer after refused calls
 *   Q <label> <i> <hash> / D <label> <j> <hash>       the queries and the database of a hvq_hash_nearest call, as the call saw them
 *   A <label> <self_offset> <threshold>               its other arguments
 *   N <label> <i> <4 numbers>                         one record read back: nearest, distance, within, first_within
 * Caller-side resources (a stream, output records, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_phash_driver"
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
static Call call_hashes(HvqContext *ctx, const std::vector<Item> &items, bool null_src, hipStream_t caller, const char *label)
{
    const int n = (int)items.size();
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    for (const Item &p : items) { sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); }
    void *out = record_room((size_t)n * 32u);
    CHECK(hvq_picture_hashes(ctx, n, sids.data(), ords.data(), null_src ? nullptr : src.data(), (uint64_t *)out, caller));
    return Call{ (uint64_t *)out, items, label };
}

/* after the caller's stream has been waited for */
static void write_call(Call *c)
{
    const std::vector<uint64_t> host = take_records(&c->out, c->items.size() * 4u);
    for (size_t i = 0; i < c->items.size(); ++i) {
        const Item &p = c->items[i];
        fprintf(g_res, "H %s %s %d %s", c->label.c_str(), p.clip.c_str(), p.kk, p.form.c_str());
        for (int v = 0; v < 4; ++v) fprintf(g_res, " %llu", (unsigned long long)host[i * 4u + (size_t)v]);
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
        calls.push_back(call_hashes(ctx, items, true, caller, "goldens/clip"));
    }
    std::vector<Item> mixed;
    for (int round = 0; round < 2; ++round)
        for (auto &s : sc) mixed.push_back(resident(s.first, *s.second, (round * 3 + 1) % (int)s.second->pics.size()));
    calls.push_back(call_hashes(ctx, mixed, false, caller, "goldens/mixed"));
    calls.push_back(call_hashes(ctx, { resident(sc[1].first, *sc[1].second, 1) }, false, caller, "goldens/one"));
    fprintf(g_res, "R goldens/n0 %d\n", hvq_picture_hashes(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
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
    Call c = call_hashes(ctx, items, false, caller, "memory");
    Call d = call_hashes(ctx, items, false, nullptr, "memory/nullstream");
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
    Call c = call_hashes(ctx, items, false, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    fprintf(g_res, "R reuse/evicted %d\n", hvq_picture_hashes(ctx, 1, &sa, &items[0].k, nullptr, c.out, caller));
    /* the newest pictures, with a call of another stream's pictures behind them in the chain; destroyed with that one still queued */
    std::vector<Item> late_call, late, other;
    for (int k = 0; k < n; ++k) {
        Item p = resident(sa, a, 2 * n + k);
        late_call.push_back(p);
        p.kk = k;                                               /* reported as the clip's pictures: the third pass decodes the same clip */
        late.push_back(p);
    }
    Call d = call_hashes(ctx, late_call, false, caller, "reuse/late");
    d.items = late;
    for (int k = 0; k < (int)e.pics.size(); ++k) other.push_back(resident(se, e, k));
    Call f = call_hashes(ctx, other, false, caller, "reuse/destroy");
    hvq_context_destroy(ctx); ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

/* two calls back to back on one stream, nothing waited for in between: they share the context's cells.  A small call, then a
 * larger one (the cells grow with the first still queued), then the small one again */
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
    Call c = call_hashes(ctx, small, false, caller, "backtoback/small");
    Call d = call_hashes(ctx, large, false, caller, "backtoback/large");
    Call e = call_hashes(ctx, small, false, caller, "backtoback/again");
    Call f = call_hashes(ctx, large, false, caller, "backtoback/large2");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    write_call(&d);
    write_call(&e);
    write_call(&f);
}

/* one hvq_hash_nearest call on `caller`: the hashes lie `q_stride` / `db_stride` words apart in device memory, db == nullptr: in place */
struct Near { int32_t *out; int nq; std::string label; };
static Near call_nearest(HvqContext *ctx, const std::vector<uint64_t> &q, int q_stride, const std::vector<uint64_t> *db, int db_stride, int64_t off,
                         int thr, hipStream_t caller, const char *label, std::vector<void *> *keep)
{
    auto upload = [&](const std::vector<uint64_t> &h, int stride) {
        std::vector<uint64_t> host(h.size() * (size_t)stride + 1u, 0x1111111111111111ull);        /* never empty; the words between are noise */
        for (size_t i = 0; i < h.size(); ++i) host[i * (size_t)stride] = h[i];
        void *d = nullptr;
        HIP(hipMalloc(&d, host.size() * 8u));
        keep->push_back(d);
        HIP(hipMemcpy(d, host.data(), host.size() * 8u, hipMemcpyHostToDevice));
        return (const uint64_t *)d;
    };
    const uint64_t *dq = upload(q, q_stride);
    const uint64_t *dd = db ? upload(*db, db_stride) : dq;
    const std::vector<uint64_t> &dbv = db ? *db : q;
    for (size_t i = 0; i < q.size(); ++i) fprintf(g_res, "Q %s %zu %llu\n", label, i, (unsigned long long)q[i]);
    for (size_t j = 0; j < dbv.size(); ++j) fprintf(g_res, "D %s %zu %llu\n", label, j, (unsigned long long)dbv[j]);
    fprintf(g_res, "A %s %lld %d\n", label, (long long)off, thr);
    void *out = nullptr;
    HIP(hipMalloc(&out, q.size() * 16u + 16u));
    std::vector<uint8_t> ff(q.size() * 16u + 16u, 0xFF);
    HIP(hipMemcpy(out, ff.data(), ff.size(), hipMemcpyHostToDevice));
    CHECK(hvq_hash_nearest(ctx, dq, (int)q.size(), q_stride, dbv.empty() ? nullptr : dd, (int)dbv.size(), db ? db_stride : q_stride, off, thr, (int32_t *)out, caller));
    return Near{ (int32_t *)out, (int)q.size(), label };
}

static void write_near(Near *c)
{
    std::vector<int32_t> host((size_t)c->nq * 4u + 4u);
    HIP(hipMemcpy(host.data(), c->out, host.size() * 4u, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->nq; ++i)
        fprintf(g_res, "N %s %d %d %d %d %d\n", c->label.c_str(), i, host[(size_t)i * 4u], host[(size_t)i * 4u + 1u], host[(size_t)i * 4u + 2u], host[(size_t)i * 4u + 3u]);
    size_t same = 0;
    for (int v = 0; v < 4; ++v) same += host[(size_t)c->nq * 4u + (size_t)v] == -1;
    fprintf(g_res, "S %s %zu 4\n", c->label.c_str(), same);                /* the 16 bytes behind the records still hold 0xFF */
    HIP(hipFree(c->out));
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

/* hvq_hash_nearest: hand-made sets with exact duplicates and equal distances, self_offset in place and on a block, thresholds 0 and 64,
 * more than one workgroup of queries and more than one tile of database, strides, an empty database; and the records of a clip's
 * pictures straight from hvq_picture_hashes, column by column, nothing waited for in between */
static void scenario_nearest(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<Near> calls;
    std::vector<uint64_t> base;
    for (int i = 0; i < 40; ++i) base.push_back(rnd());
    std::vector<uint64_t> db;
    for (int j = 0; j < 300; ++j) {                              /* few bits away from few bases: many equal distances, some exact duplicates */
        uint64_t h = base[(size_t)(rnd() % base.size())];
        const int flips = (int)(rnd() % 4u);
        for (int f = 0; f < flips; ++f) h ^= 1ull << (rnd() % 64u);
        db.push_back(h);
    }
    std::vector<uint64_t> q(db.begin() + 10, db.begin() + 70);
    for (int i = 0; i < 20; ++i) q.push_back(rnd());
    calls.push_back(call_nearest(ctx, q, 1, &db, 1, -1, 10, caller, "nearest/all", &keep));
    calls.push_back(call_nearest(ctx, q, 3, &db, 4, -1, 0, caller, "nearest/strides_thr0", &keep));
    calls.push_back(call_nearest(ctx, q, 1, &db, 1, -1, 64, caller, "nearest/thr64", &keep));
    calls.push_back(call_nearest(ctx, db, 1, nullptr, 1, 0, 6, caller, "nearest/inplace", &keep));
    calls.push_back(call_nearest(ctx, q, 1, &db, 1, 10, 6, caller, "nearest/block", &keep));       /* q = db[10 .. 70) + strangers, offset 10 */
    calls.push_back(call_nearest(ctx, q, 1, &db, 1, 1000, 6, caller, "nearest/offset_beyond", &keep));
    std::vector<uint64_t> none, one(1, db[5]);
    calls.push_back(call_nearest(ctx, q, 1, &none, 1, -1, 10, caller, "nearest/ndb0", &keep));
    calls.push_back(call_nearest(ctx, one, 1, &one, 1, -1, 10, caller, "nearest/one", &keep));
    /* 600 queries (three workgroups) against 2100 hashes (more than two tiles), in place too */
    std::vector<uint64_t> big;
    for (int j = 0; j < 2100; ++j) big.push_back(base[(size_t)(rnd() % base.size())] ^ (1ull << (rnd() % 64u)) ^ ((rnd() & 1u) ? 1ull << (rnd() % 64u) : 0ull));
    std::vector<uint64_t> bq(big.begin() + 900, big.begin() + 1500);
    calls.push_back(call_nearest(ctx, bq, 1, &big, 1, -1, 2, caller, "nearest/big", &keep));
    calls.push_back(call_nearest(ctx, bq, 1, &big, 2, 900, 2, caller, "nearest/big_block", &keep));
    calls.push_back(call_nearest(ctx, big, 1, nullptr, 1, 0, 1, caller, "nearest/big_inplace", &keep));
    fprintf(g_res, "R nearest/nq0 %d\n", hvq_hash_nearest(ctx, nullptr, 0, 1, nullptr, 0, 1, -1, 10, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    for (Near &c : calls) write_near(&c);

    /* the records of a clip's pictures, then de-duplication of each column in place, on one stream, nothing waited for */
    const Clip &a = clip("gop64x48_15");
    const int sa = decode(ctx, a), n = (int)a.pics.size();
    std::vector<Item> items;
    for (int k = 0; k < n; ++k) items.push_back(resident(sa, a, k));
    Call h = call_hashes(ctx, items, false, caller, "nearest/records");
    void *out = nullptr;
    HIP(hipMalloc(&out, (size_t)n * 16u * 3u));
    for (int col = 0; col < 3; ++col)
        CHECK(hvq_hash_nearest(ctx, h.out + col, n, 4, h.out + col, n, 4, 0, 12, (int32_t *)out + (size_t)col * (size_t)n * 4u, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<int32_t> host((size_t)n * 12u);
    HIP(hipMemcpy(host.data(), out, host.size() * 4u, hipMemcpyDeviceToHost));
    for (int col = 0; col < 3; ++col)
        for (int i = 0; i < n; ++i) {
            const int32_t *r = &host[((size_t)col * (size_t)n + (size_t)i) * 4u];
            fprintf(g_res, "N nearest/column%d %d %d %d %d %d\n", col, i, r[0], r[1], r[2], r[3]);
        }
    write_call(&h);
    HIP(hipFree(out));
    for (void *p : keep) HIP(hipFree(p));
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
    void *out = sent.room(2u * 32u + 8u), *mem = nullptr;
    HIP(hipMalloc(&mem, hvq_stream_pic_bytes(ctx, sa) + 32u));
    uint64_t *o = (uint64_t *)out;
    auto refuse = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, uint64_t *dst) {
        write_code("refused", label, hvq_picture_hashes(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), dst, caller));
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
    write_code("refused", "n0", hvq_picture_hashes(ctx, 0, nullptr, nullptr, nullptr, nullptr, caller));
    /* hvq_hash_nearest: q and db are the picture memory (its contents do not matter), out is the sentinel buffer (16-byte aligned) */
    const uint64_t *hq = (const uint64_t *)mem;
    int32_t *ho = (int32_t *)out;
    auto near = [&](const char *label, HvqContext *cx, const uint64_t *q, int nq, int qs, const uint64_t *db, int ndb, int ds, int thr, int32_t *dst) {
        write_code("refused", ("near_" + std::string(label)).c_str(), hvq_hash_nearest(cx, q, nq, qs, db, ndb, ds, -1, thr, dst, caller));
    };
    near("null_context", nullptr, hq, 4, 1, hq, 4, 1, 10, ho);
    near("null_q", ctx, nullptr, 4, 1, hq, 4, 1, 10, ho);
    near("misaligned_q", ctx, (const uint64_t *)((const uint8_t *)mem + 4), 4, 1, hq, 4, 1, 10, ho);
    near("null_db", ctx, hq, 4, 1, nullptr, 4, 1, 10, ho);
    near("misaligned_db", ctx, hq, 4, 1, (const uint64_t *)((const uint8_t *)mem + 4), 4, 1, 10, ho);
    near("null_out", ctx, hq, 4, 1, hq, 4, 1, 10, nullptr);
    near("misaligned_out", ctx, hq, 4, 1, hq, 4, 1, 10, (int32_t *)((uint8_t *)out + 8));
    near("q_stride0", ctx, hq, 4, 0, hq, 4, 1, 10, ho);
    near("db_stride_negative", ctx, hq, 4, 1, hq, 4, -1, 10, ho);
    near("threshold65", ctx, hq, 4, 1, hq, 4, 1, 65, ho);
    near("threshold_negative", ctx, hq, 4, 1, hq, 4, 1, -1, ho);
    near("nq_negative", ctx, hq, -1, 1, hq, 4, 1, 10, ho);
    near("nq_too_many", ctx, hq, (1 << 24) + 1, 1, hq, 4, 1, 10, ho);
    near("ndb_too_many", ctx, hq, 4, 1, hq, (1 << 24) + 1, 1, 10, ho);
    HIP(hipStreamSynchronize(caller));
    sent.write("refused");
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    Call c = call_hashes(ctx, { resident(sa, a, 1), resident(sd, d, last) }, false, caller, "refused/then_ok");
    HIP(hipStreamSynchronize(caller));
    write_call(&c);
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    return driver_main(argc, argv, { { "goldens", scenario_goldens }, { "memory", scenario_memory }, { "reuse", scenario_reuse },
                                     { "backtoback", scenario_backtoback }, { "refused", scenario_refused },
                                     { "nearest", scenario_nearest } });
}
