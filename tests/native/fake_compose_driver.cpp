/*
 * tests/native/fake_compose_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_compose_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_compose.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_compose_cpu.py compares with
 * hvqm4_amd.compose.of_pictures on the oracle's pictures.
 *
 *   fake_compose_driver <scenario> <outdir> <golden dir>
 *
 * Scenario `script` runs <outdir>/script.txt, written by the test, one command a line:
 *   CLIP <name>                         decode the clip into a stream of its own; streams are numbered in the order of CLIP and SHAPE
 *   SHAPE <w> <h> <hs> <vs>             open a stream of that geometry, nothing decoded: it carries the caller's memory
 *   PIC <stream> <k>                    a picture of the calls: the resident picture k; pictures are numbered in their order
 *   MEM <stream> <form> <k> <offset>    ... the caller's memory, `offset` bytes into an allocation.  form: inv (picture k of the stream's
 *                                       clip, every byte inverted), synth (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), flat
 *                                       (every byte k), check (a 0 / 255 checkerboard, 255 where x + y + k is odd, in every plane)
 *   OUT <stream> <call> <target>        ... the caller's memory: target <target> of the earlier call number <call>, never read back in between
 *   T <w> <h> <hs> <vs> <shift> <b0> <b1> <b2> <first> <count>      a target of the next call
 *   L <picture> <mode> <sx> <sy> <w> <h> <dx> <dy> <w0> <w1> <w2>   a layer of the next call
 *   FORCE <on>                          hvq_compose_force_general; R force <setting before>
 *   CALL <label> <null>                 the call of the T and L lines since the last one, on the caller's stream or (null 1) the null stream
 *   COUNT <label>                       wait for both streams; B <label> <layer planes through the aligned body> <through the general body> since the last COUNT
 * and at the end, for every call, P <label> <target> <w> <h> <hs> <vs> <crc32 of the bytes read back> <guard>; guard: 1 when the 256
 * bytes before and the 256 bytes behind the output still hold the sentinel.  The scenarios `reuse` and `refused` are programs of their own
 * below; they add  R <label> <return code>  and  S <label> <bytes that still hold the sentinel> <bytes>.
 * Caller-side resources (a stream, outputs, picture memory) come from the fake's HIP calls, as a caller's would from HIP.
 */
#define DRIVER_NAME "fake_compose_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

extern "C" void fake_compose_counts(uint64_t out[2], int reset);

struct Source { int sid, k; const void *src; };
struct Call { std::string label; std::vector<uint8_t *> room; std::vector<Geom> geoms; };

/* queue one call on `caller`; every output is its own allocation filled with the sentinel, GUARD bytes before and behind the picture;
 * dst[t].ptr is set here */
static Call call_compose(HvqContext *ctx, const std::vector<Source> &pics, const std::vector<int> &which, std::vector<HvqComposeLayer> layers, std::vector<HvqComposeDst> dst,
                         hipStream_t caller, const std::string &label)
{
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    for (int p : which) { sids.push_back(pics[(size_t)p].sid); ords.push_back(pics[(size_t)p].k); src.push_back(pics[(size_t)p].src); }
    Call c{ label, {}, {} };
    for (HvqComposeDst &d : dst) {
        const Geom t{ d.width, d.height, d.h_samp, d.v_samp };
        c.room.push_back(guarded_room(bytes_of(t)));
        c.geoms.push_back(t);
        d.ptr = c.room.back() + GUARD;
    }
    CHECK(hvq_compose_pictures(ctx, (int)layers.size(), sids.data(), ords.data(), src.data(), layers.data(), (int)dst.size(), dst.data(), caller));
    return c;
}

/* after the stream of the call has been waited for */
static void write_call(Call *c)
{
    for (size_t i = 0; i < c->room.size(); ++i) {
        const Geom t = c->geoms[i];
        const ReadBack r = read_room(c->room[i], bytes_of(t));
        fprintf(g_res, "P %s %zu %d %d %d %d %u %d\n", c->label.c_str(), i, t.w, t.h, t.hs, t.vs, r.crc, r.guard);
        HIP(hipFree(c->room[i]));
    }
    c->room.clear();
}

static void scenario_script(HvqContext *&ctx, hipStream_t caller)
{
    struct Str { int sid; Geom g; const Clip *c; };
    std::vector<Str> streams;
    std::vector<Source> pics;
    std::vector<void *> keep;
    std::vector<Call> calls;
    std::vector<HvqComposeLayer> layers;
    std::vector<HvqComposeDst> dst;
    std::vector<int> which;
    std::ifstream f(g_out + "/script.txt");
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "CLIP") {
            std::string nm; in >> nm;
            const Clip &c = clip(nm);
            streams.push_back(Str{ decode(ctx, c), geom_of(c), &c });
        } else if (cmd == "SHAPE") {
            Geom g; in >> g.w >> g.h >> g.hs >> g.vs;
            const int sid = hvq_stream_open(ctx, g.w, g.h, g.hs, g.vs, 1, 3);
            CHECK(sid);
            streams.push_back(Str{ sid, g, nullptr });
        } else if (cmd == "PIC") {
            int s, k; in >> s >> k;
            pics.push_back(Source{ streams[(size_t)s].sid, k, nullptr });
        } else if (cmd == "MEM") {
            int s, k; std::string form; size_t off; in >> s >> form >> k >> off;
            const Str &st = streams[(size_t)s];
            pics.push_back(Source{ st.sid, -1, uploaded(form == "inv" ? inverted(ctx, st.sid, k) : filled(st.g, form, k), off, &keep) });
        } else if (cmd == "OUT") {
            int s, c, t; in >> s >> c >> t;
            pics.push_back(Source{ streams[(size_t)s].sid, -1, calls[(size_t)c].room[(size_t)t] + GUARD });
        } else if (cmd == "T") {
            HvqComposeDst d; memset(&d, 0, sizeof d);
            in >> d.width >> d.height >> d.h_samp >> d.v_samp >> d.shift >> d.bias[0] >> d.bias[1] >> d.bias[2] >> d.first >> d.count;
            dst.push_back(d);
        } else if (cmd == "L") {
            HvqComposeLayer l; int p;
            in >> p >> l.mode >> l.sx >> l.sy >> l.w >> l.h >> l.dx >> l.dy >> l.weight[0] >> l.weight[1] >> l.weight[2];
            layers.push_back(l); which.push_back(p);
        } else if (cmd == "FORCE") {
            int on; in >> on;
            fprintf(g_res, "R force %d\n", hvq_compose_force_general(ctx, on));
        } else if (cmd == "CALL") {
            std::string label; int null; in >> label >> null;
            calls.push_back(call_compose(ctx, pics, which, layers, dst, null ? nullptr : caller, label));
            layers.clear(); dst.clear(); which.clear();
        } else if (cmd == "COUNT") {
            std::string label; in >> label;
            HIP(hipStreamSynchronize(caller));
            HIP(hipStreamSynchronize(nullptr));
            uint64_t n[2];
            fake_compose_counts(n, 1);
            fprintf(g_res, "B %s %llu %llu\n", label.c_str(), (unsigned long long)n[0], (unsigned long long)n[1]);
        } else { fprintf(stderr, DRIVER_NAME ": script.txt: %s\n", cmd.c_str()); exit(2); }
        if (!in) { fprintf(stderr, DRIVER_NAME ": script.txt: the line `%s` is short\n", line.c_str()); exit(2); }
    }
    HIP(hipStreamSynchronize(caller));
    HIP(hipStreamSynchronize(nullptr));
    for (Call &c : calls) write_call(&c);
    for (void *p : keep) HIP(hipFree(p));
}

static HvqComposeLayer layer(int mode, int wt, int dx = 0, int dy = 0) { return HvqComposeLayer{ mode, 0, 0, 0, 0, dx, dy, { wt, wt, wt } }; }
static HvqComposeDst target(Geom g, int first, int count, int shift, int bias) { return HvqComposeDst{ nullptr, g.w, g.h, g.hs, g.vs, first, count, shift, { bias, bias, bias } }; }

/* `mean`: target k = (picture k + picture (k + 1) mod n + 1) >> 1 of the pictures `from` .. `from` + n - 1 of stream sid */
static Call call_mean(HvqContext *ctx, int sid, Geom g, int n, int from, hipStream_t caller, const char *label)
{
    std::vector<Source> pics;
    std::vector<int> which;
    std::vector<HvqComposeLayer> layers;
    std::vector<HvqComposeDst> dst;
    for (int k = 0; k < n; ++k) pics.push_back(Source{ sid, from + k, nullptr });
    for (int k = 0; k < n; ++k) {
        which.push_back(k); which.push_back((k + 1) % n);
        layers.push_back(layer(HVQ_CMP_ADD, 1)); layers.push_back(layer(HVQ_CMP_ADD, 1));
        dst.push_back(target(g, 2 * k, 2, 1, 0));
    }
    return call_compose(ctx, pics, which, layers, dst, caller, label);
}

/* a call queued on the caller's stream, then flushes that hand the slots of its pictures to later ones, nothing waited for in between:
 * the outputs are those of the pictures as they were.  Then the composed pictures straight into a second call as its sources (`diff`:
 * target k = out k - out (k + 1) mod n + 128), and a context destroyed with a call still queued. */
static void scenario_reuse(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int n = (int)a.pics.size();
    const int sa = decode(ctx, a), se = decode(ctx, e);
    const Geom ga = geom_of(a);
    Call c = call_mean(ctx, sa, ga, n, 0, caller, "reuse");
    for (int pass = 0; pass < 2; ++pass) {                      /* 2 n later pictures into a ring of n + 3 slots: every slot of the first pass is rewritten */
        for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sa, p.type, p.p, p.len));
        CHECK(hvq_flush(ctx));
    }
    {
        const int zero = 0;
        HvqComposeLayer l = layer(HVQ_CMP_PUT, 1);
        HvqComposeDst d = target(ga, 0, 1, 0, 0);
        d.ptr = c.room[0] + GUARD;
        fprintf(g_res, "R reuse/evicted %d\n", hvq_compose_pictures(ctx, 1, &sa, &zero, nullptr, &l, 1, &d, caller));
    }
    std::vector<Source> outs;
    std::vector<int> which;
    std::vector<HvqComposeLayer> layers;
    std::vector<HvqComposeDst> dst;
    for (int k = 0; k < n; ++k) outs.push_back(Source{ sa, -1, c.room[(size_t)k] + GUARD });
    for (int k = 0; k < n; ++k) {
        which.push_back(k); which.push_back((k + 1) % n);
        layers.push_back(layer(HVQ_CMP_ADD, 1)); layers.push_back(layer(HVQ_CMP_ADD, -1));
        dst.push_back(target(ga, 2 * k, 2, 0, 128));
    }
    Call g = call_compose(ctx, outs, which, layers, dst, caller, "reuse/chain");
    Call d = call_mean(ctx, sa, ga, n, 2 * n, caller, "reuse/late");
    Call f = call_mean(ctx, se, geom_of(e), (int)e.pics.size(), 0, caller, "reuse/destroy");
    hvq_context_destroy(ctx);
    ctx = nullptr;
    HIP(hipStreamSynchronize(caller));
    write_call(&g);
    write_call(&c);
    write_call(&d);
    write_call(&f);
}

struct Args {
    HvqContext *ctx;
    int nlayers, ntargets;
    std::vector<int> sids, ords;
    std::vector<const void *> src;
    std::vector<HvqComposeLayer> layers;
    std::vector<HvqComposeDst> dst;
    bool null_sids = false, null_ords = false, null_src = true, null_layers = false, null_dst = false;
};

static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("gop64x48_15"), &e = clip("yuv444_64x48");
    const int sa = decode(ctx, a), se = decode(ctx, e);
    /* a ring of 3 slots: the clip's first pictures are gone when its last ones are decoded */
    const int sd = hvq_stream_open(ctx, a.info.width, a.info.height, a.info.h_samp, a.info.v_samp, a.info.is_1_5, 3);
    CHECK(sd);
    for (const Pic &p : a.pics) CHECK(hvq_stream_submit(ctx, sd, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    CHECK(hvq_stream_submit(ctx, sa, a.pics[0].type, a.pics[0].p, a.pics[0].len));      /* queued, not flushed: ordinal n of sa */
    const int queued = (int)a.pics.size();

    const Geom ga = geom_of(a);
    const size_t nb = bytes_of(ga), bytes = 2u * nb + 16u;
    void *out = nullptr, *mem = nullptr;
    HIP(hipMalloc(&out, bytes));
    HIP(hipMalloc(&mem, nb + 32u));
    std::vector<uint8_t> sent(bytes, SENTINEL);
    HIP(hipMemcpy(out, sent.data(), sent.size(), hipMemcpyHostToDevice));
    uint8_t *o = (uint8_t *)out;
    /* the good call: two targets of the clip's geometry, three layers; target 0 takes layers 0 and 1, target 1 layers 1 and 2; layer 1 a
     * 16 x 16 rectangle from (8, 8) to (32, 16) */
    auto good = [&]() {
        Args g;
        g.ctx = ctx; g.nlayers = 3; g.ntargets = 2;
        g.sids = { sa, sa, sa }; g.ords = { 0, 1, 2 }; g.src = { nullptr, nullptr, nullptr };
        g.layers = { layer(HVQ_CMP_PUT, 2), HvqComposeLayer{ HVQ_CMP_ADD, 8, 8, 16, 16, 32, 16, { 1, 1, 1 } }, layer(HVQ_CMP_ADD, -3) };
        g.dst = { target(ga, 0, 2, 1, 0), target(ga, 1, 2, 2, 128) };
        g.dst[0].ptr = o; g.dst[1].ptr = o + nb;
        return g;
    };
    auto run = [&](const char *label, const Args &g) {
        fprintf(g_res, "R refused/%s %d\n", label,
                hvq_compose_pictures(g.ctx, g.nlayers, g.null_sids ? nullptr : g.sids.data(), g.null_ords ? nullptr : g.ords.data(), g.null_src ? nullptr : g.src.data(),
                                     g.null_layers ? nullptr : g.layers.data(), g.ntargets, g.null_dst ? nullptr : g.dst.data(), caller));
    };
#define REFUSE(label, change) do { Args g = good(); change; run(label, g); } while (0)
    REFUSE("null_context", g.ctx = nullptr);
    REFUSE("null_streams", g.null_sids = true);
    REFUSE("null_ordinals", g.null_ords = true);
    REFUSE("null_layers", g.null_layers = true);
    REFUSE("null_dst", g.null_dst = true);
    REFUSE("negative_layers", g.nlayers = -1);
    REFUSE("negative_targets", g.ntargets = -1);
    REFUSE("too_many_targets", g.ntargets = 65536);
    REFUSE("too_many_layers", g.nlayers = HVQ_CMP_MAX_TOTAL + 1);
    REFUSE("bad_stream", g.sids[2] = 99);
    REFUSE("bad_ordinal", g.ords[2] = 1000);
    REFUSE("misaligned_src", (g.null_src = false, g.ords[2] = -1, g.src[2] = (uint8_t *)mem + 8));
    REFUSE("src_with_ordinal", (g.null_src = false, g.src[2] = mem));
    REFUSE("src_with_bad_stream", (g.null_src = false, g.ords[2] = -1, g.sids[2] = 99, g.src[2] = mem));
    REFUSE("minus_one_without_src", g.ords[2] = -1);
    REFUSE("null_ptr", g.dst[1].ptr = nullptr);
    REFUSE("misaligned_ptr", g.dst[1].ptr = o + nb + 8);
    REFUSE("sampling_differs", g.sids[2] = se);                                       /* a 4:4:4 layer in a 4:2:0 target */
    REFUSE("sampling_differs_target", (g.dst[1].h_samp = 1, g.dst[1].v_samp = 1));
    REFUSE("source_leaves_x", g.layers[1].sx = 56);
    REFUSE("source_leaves_y", g.layers[1].sy = 40);
    REFUSE("source_too_wide", (g.layers[1].sx = 0, g.layers[1].w = 72));
    REFUSE("target_leaves_x", g.layers[1].dx = 56);
    REFUSE("target_leaves_y", g.layers[1].dy = 40);
    REFUSE("whole_leaves_target", g.layers[0].dx = 2);
    REFUSE("whole_in_smaller_target", (g.dst[0].width = 32, g.dst[0].height = 32));
    REFUSE("odd_sx", g.layers[1].sx = 9);
    REFUSE("odd_w", g.layers[1].w = 15);
    REFUSE("odd_dx", g.layers[1].dx = 33);
    REFUSE("odd_sy", g.layers[1].sy = 9);
    REFUSE("odd_h", g.layers[1].h = 15);
    REFUSE("odd_dy", g.layers[1].dy = 17);
    REFUSE("empty_h", g.layers[1].h = 0);
    REFUSE("whole_with_sx", (g.layers[1].w = 0, g.layers[1].h = 0, g.layers[1].sy = 0));
    REFUSE("negative_sx", g.layers[1].sx = -2);
    REFUSE("negative_dy", g.layers[1].dy = -2);
    REFUSE("negative_w", g.layers[1].w = -16);
    REFUSE("mode_2", g.layers[2].mode = 2);
    REFUSE("mode_negative", g.layers[0].mode = -1);
    REFUSE("gain_above", (g.layers[1].weight[1] = HVQ_CMP_MAX_GAIN - 2, g.layers[2].weight[1] = -3));
    REFUSE("shift_above", g.dst[1].shift = HVQ_CMP_MAX_SHIFT + 1);
    REFUSE("shift_negative", g.dst[0].shift = -1);
    REFUSE("bias_above", g.dst[1].bias[2] = 256);
    REFUSE("bias_below", g.dst[0].bias[0] = -256);
    REFUSE("first_negative", g.dst[1].first = -1);
    REFUSE("count_negative", g.dst[1].count = -1);
    REFUSE("range_beyond", g.dst[1].first = 2);
    REFUSE("first_beyond", (g.dst[1].first = 4, g.dst[1].count = 0));
    REFUSE("unused_layer_checked", (g.dst[1].first = 0, g.dst[1].count = 1, g.layers[2].sx = 2));   /* layer 2 belongs to no target: still checked */
    REFUSE("geometry_width", g.dst[1].width = 12);
    REFUSE("geometry_sampling", (g.dst[1].h_samp = 1, g.dst[1].v_samp = 2));
    REFUSE("geometry_zero", (g.dst[1].width = 0, g.dst[1].height = 0));
    REFUSE("evicted", (g.sids = { sd, sd, sd }, g.ords = { queued - 1, queued - 2, 0 }));
    REFUSE("queued", g.ords[2] = queued);
    {                                                                                 /* more layers than a target takes */
        Args g = good();
        g.nlayers = HVQ_CMP_MAX_LAYERS + 1;
        g.sids.assign((size_t)g.nlayers, sa); g.ords.assign((size_t)g.nlayers, 0); g.layers.assign((size_t)g.nlayers, layer(HVQ_CMP_ADD, 1));
        g.dst[0].count = g.dst[1].count = 1;
        g.dst[1].first = 0; g.dst[1].count = g.nlayers;
        run("too_many_in_target", g);
    }
    REFUSE("n0", (g.ntargets = 0, g.nlayers = 0));                     /* ntargets == 0: HVQ_OK, nothing looked at */
    {
        HvqComposeLayer l = layer(HVQ_CMP_PUT, 1);
        fprintf(g_res, "R refused/check_good %d\n", hvq_compose_check(&l));
        fprintf(g_res, "R refused/check_null %d\n", hvq_compose_check(nullptr));
        l.mode = 5;
        fprintf(g_res, "R refused/check_mode %d\n", hvq_compose_check(&l));
        l = layer(HVQ_CMP_ADD, -HVQ_CMP_MAX_GAIN);
        l.w = 2; l.h = 2;
        fprintf(g_res, "R refused/check_rect %d\n", hvq_compose_check(&l));
    }
    fprintf(g_res, "R refused/force_null %d\n", hvq_compose_force_general(nullptr, 1));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sent.size());
    HIP(hipMemcpy(back.data(), out, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works */
    CHECK(hvq_flush(ctx));
    {
        Call c = call_mean(ctx, sa, ga, 2, 0, caller, "refused/then_ok");
        HIP(hipStreamSynchronize(caller));
        write_call(&c);
    }
    HIP(hipFree(out));
    HIP(hipFree(mem));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_compose_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_compose_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "script") run_scenario(scenario_script);
    else if (sc == "reuse") run_scenario(scenario_reuse);
    else if (sc == "refused") run_scenario(scenario_refused);
    else { fprintf(stderr, "fake_compose_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
