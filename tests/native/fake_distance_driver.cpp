/*
 * tests/native/fake_distance_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_distance_pictures and
 * hvq_distance_mask of the runtime (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and
 * tests/native/fake_distance.cpp) through include/hvqm4_amd.h.  It writes what it read back and judges nothing:
 * tests/test_distance_cpu.py compares with hvqm4_amd.distance.
 *
 *   fake_distance_driver <scenario> <outdir> <golden dir>
 *
 * The test writes into <outdir>: calls.txt and pictures.bin.  calls.txt, one fact per line:
 *   M <mode> <lo> <hi> <invert>                                     a mask entry; they are numbered from 0
 *   P <w> <h> <hs> <vs> <plane> <lo> <hi> <metric> <border> <mask, or -1>   a picture: its bytes are the next ones of pictures.bin
 * The driver builds no picture, rule or mask of its own, except the malformed ones of `refused`.
 *
 * Scenarios.  cases: the pictures of calls.txt in the caller's memory (src), ONE hvq_distance_pictures (equal rules share an entry), then
 * ONE hvq_distance_mask over the pictures that name a mask, then ONE hvq_distance_pictures whose src are that call's outputs (the 255s of
 * Y, EUCLID2, no border), all on the same stream with no wait in between.  resident: the pictures of three clips where they lie, and the
 * same pictures inverted in the caller's memory, in one call; mask and chain behind it.  refused: every refusal of the header's lists.
 * nogpu: what a program linked without fake_distance.cpp gets.
 *
 * Outputs: dist.bin (the maps one behind the other, uint32), mask.bin (the pictures of the mask call), chain.bin (the maps of the last
 * call).  results.txt:
 *   G <label> <index> <guard>       1 when the 256 bytes before and behind that output still hold the sentinel
 *   P <clip> <form> <k>             resident: the picture behind output <index> (form pic or inv), in order
 *   R <label> <return code>         a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the outputs after refused calls
 */
#define DRIVER_NAME "fake_distance_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

struct Want { Geom g; HvqDistanceRule rule; int mask; std::vector<uint8_t> bytes; };
static std::vector<Want> g_pics;
static std::vector<HvqDistanceMask> g_masks;

static void load_inputs()
{
    std::ifstream f(g_out + "/calls.txt");
    std::ifstream bin(g_out + "/pictures.bin", std::ios::binary);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "M") {
            HvqDistanceMask m;
            memset(&m, 0, sizeof m);
            in >> m.mode >> m.lo >> m.hi >> m.invert;
            g_masks.push_back(m);
        } else if (what == "P") {
            Want w;
            memset(&w.rule, 0, sizeof w.rule);
            in >> w.g.w >> w.g.h >> w.g.hs >> w.g.vs >> w.rule.plane >> w.rule.lo >> w.rule.hi >> w.rule.metric >> w.rule.border >> w.mask;
            w.bytes.resize(bytes_of(w.g));
            bin.read((char *)w.bytes.data(), (std::streamsize)w.bytes.size());
            if (!bin) { fprintf(stderr, DRIVER_NAME ": pictures.bin is short\n"); exit(2); }
            g_pics.push_back(w);
        }
        if (!in) { fprintf(stderr, DRIVER_NAME ": calls.txt: a short line: %s\n", line.c_str()); exit(2); }
    }
}

static size_t plane_samples(Geom g, int plane)
{
    return plane ? (size_t)(g.w >> (g.hs == 2)) * (size_t)(g.h >> (g.vs == 2)) : (size_t)g.w * g.h;
}

static FILE *out_file(const char *name)
{
    FILE *f = fopen((g_out + "/" + name).c_str(), "wb");
    if (!f) { fprintf(stderr, DRIVER_NAME ": cannot write %s\n", name); exit(2); }
    return f;
}

/* a room read back: its bytes into `f`, a G line about its guards */
static void write_room(FILE *f, const char *label, size_t index, uint8_t *room, size_t nb)
{
    std::vector<uint8_t> host(nb + 2 * GUARD);
    HIP(hipMemcpy(host.data(), room, host.size(), hipMemcpyDeviceToHost));
    int guard = 1;
    for (size_t g = 0; g < GUARD; ++g) guard &= host[g] == SENTINEL && host[GUARD + nb + g] == SENTINEL;
    if (fwrite(host.data() + GUARD, 1, nb, f) != nb) exit(2);
    fprintf(g_res, "G %s %zu %d\n", label, index, guard);
    HIP(hipFree(room));
}

struct One { int sid, k; const void *src; Geom g; HvqDistanceRule rule; int mask; };

/* ONE distance call, ONE mask call behind it, ONE distance call on its outputs, then the wait and the files */
static void distance_mask_distance(HvqContext *ctx, const std::vector<One> &v, hipStream_t caller)
{
    const int n = (int)v.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<HvqDistanceRule> rules;
    std::vector<uint8_t *> droom;
    std::vector<uint32_t *> dist;
    for (const One &p : v) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src);
        size_t r = 0;
        while (r < rules.size() && memcmp(&rules[r], &p.rule, sizeof p.rule)) ++r;
        if (r == rules.size()) rules.push_back(p.rule);
        which.push_back((int)r);
        droom.push_back(guarded_room(4u * plane_samples(p.g, p.rule.plane)));
        dist.push_back((uint32_t *)(droom.back() + GUARD));
    }
    CHECK(hvq_distance_pictures(ctx, n, sids.data(), ords.data(), src.data(), rules.data(), (int)rules.size(), which.data(), dist.data(), caller));
    std::vector<int> msid, mwhich, mords;
    std::vector<const uint32_t *> mdist;
    std::vector<uint8_t *> mroom, croom;
    std::vector<void *> dst;
    std::vector<const void *> csrc;
    std::vector<uint32_t *> cdist;
    std::vector<size_t> mnb, cnb;
    for (int i = 0; i < n; ++i) {
        if (v[(size_t)i].mask < 0) continue;
        msid.push_back(sids[(size_t)i]); mwhich.push_back(v[(size_t)i].mask); mdist.push_back(dist[(size_t)i]); mords.push_back(-1);
        mnb.push_back(bytes_of(v[(size_t)i].g));
        mroom.push_back(guarded_room(mnb.back()));
        dst.push_back(mroom.back() + GUARD);
        csrc.push_back(mroom.back() + GUARD);
        cnb.push_back(4u * plane_samples(v[(size_t)i].g, 0));
        croom.push_back(guarded_room(cnb.back()));
        cdist.push_back((uint32_t *)(croom.back() + GUARD));
    }
    if (!msid.empty()) {
        const HvqDistanceRule again = { 0, 255, 255, HVQ_DST_EUCLID2, 0, { 0, 0, 0 } };
        CHECK(hvq_distance_mask(ctx, (int)msid.size(), msid.data(), mdist.data(), g_masks.data(), (int)g_masks.size(), mwhich.data(), dst.data(), caller));
        CHECK(hvq_distance_pictures(ctx, (int)msid.size(), msid.data(), mords.data(), csrc.data(), &again, 1, nullptr, cdist.data(), caller));
    }
    HIP(hipStreamSynchronize(caller));
    FILE *fd = out_file("dist.bin"), *fm = out_file("mask.bin"), *fc = out_file("chain.bin");
    for (int i = 0; i < n; ++i) write_room(fd, "dist", (size_t)i, droom[(size_t)i], 4u * plane_samples(v[(size_t)i].g, v[(size_t)i].rule.plane));
    for (size_t i = 0; i < mroom.size(); ++i) write_room(fm, "mask", i, mroom[i], mnb[i]);
    for (size_t i = 0; i < croom.size(); ++i) write_room(fc, "chain", i, croom[i], cnb[i]);
    fclose(fd); fclose(fm); fclose(fc);
}

static void scenario_cases(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    std::map<std::string, int> streams;
    for (const Want &w : g_pics) {
        const std::string key = std::to_string(w.g.w) + "x" + std::to_string(w.g.h) + ":" + std::to_string(w.g.hs) + std::to_string(w.g.vs);
        if (!streams.count(key)) { streams[key] = hvq_stream_open(ctx, w.g.w, w.g.h, w.g.hs, w.g.vs, 1, 3); CHECK(streams[key]); }
        v.push_back(One{ streams[key], -1, uploaded(w.bytes, v.size() & 1 ? 16 : 0, &keep), w.g, w.rule, w.mask });
    }
    distance_mask_distance(ctx, v, caller);
    fprintf(g_res, "R cases/n0 %d\n", hvq_distance_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    fprintf(g_res, "R cases/mask_n0 %d\n", hvq_distance_mask(ctx, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    for (void *p : keep) HIP(hipFree(p));
}

/* the rule and the mask come from the first P line of calls.txt */
static void scenario_resident(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    for (const char *nm : { "crossplane420_64x48", "yuv422_296x160", "crossplane444_48x64" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int k = 0; k < (int)c.pics.size() && k < 3; ++k) {
            const Picture a = resident_picture(sid, c, k), b = inverted_picture(ctx, sid, c, k, k & 1 ? 16 : 0, &keep);
            HvqDistanceRule r = g_pics[0].rule;
            r.plane = k % 3;
            r.metric = k % 3;
            v.push_back(One{ a.sid, a.k, a.src, a.g, r, r.plane == 0 ? g_pics[0].mask : -1 });
            v.push_back(One{ b.sid, b.k, b.src, b.g, r, r.plane == 0 ? g_pics[0].mask : -1 });
            fprintf(g_res, "P %s pic %d\nP %s inv %d\n", nm, k, nm, k);
        }
    }
    distance_mask_distance(ctx, v, caller);
    for (void *p : keep) HIP(hipFree(p));
}

/* one picture, every call refused: the outputs keep their sentinel */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t lb = 4u * plane_samples(g, 0), pb = bytes_of(g);
    uint8_t *room = guarded_room(2 * (lb + pb), 0);
    uint32_t *L[2] = { (uint32_t *)room, (uint32_t *)(room + lb) };
    void *D[2] = { room + 2 * lb, room + 2 * lb + pb };
    void *mem = nullptr;
    HIP(hipMalloc(&mem, pb + 32));
    const HvqDistanceRule good = { 0, 255, 255, 0, 0, { 0, 0, 0 } };
    const HvqDistanceMask mgood = { 0, 1, 9, 0, { 0, 0, 0, 0 } };
    const int two[2] = { 0, 0 }, w_hi[2] = { 0, 1 }, w_lo[2] = { -1, 0 };
    auto dis = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const HvqDistanceRule *rules, int nrules,
                   const int *which, uint32_t *const *dist) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_distance_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), rules, nrules, which, dist, caller));
    };
    uint32_t *Lnull[2] = { L[0], nullptr }, *Lmis[2] = { L[0], L[1] + 1 };
    dis("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L);
    dis("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, &good, 1, nullptr, L);
    dis("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, &good, 1, nullptr, L);
    dis("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, &good, 1, nullptr, L);
    dis("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, &good, 1, nullptr, L);
    dis("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, &good, 1, nullptr, L);
    dis("null_rules", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, 1, nullptr, L);
    dis("nrules_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 0, nullptr, L);
    {
        std::vector<HvqDistanceRule> many(65, good);
        dis("nrules_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, many.data(), 65, two, L);
    }
    dis("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_hi, L);
    dis("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_lo, L);
    dis("null_dist", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, nullptr);
    dis("null_map", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Lnull);
    dis("misaligned_map", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Lmis);
    dis("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L);
    dis("negative_n", ctx, -1, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L);
    auto bad = [&](const char *label, HvqDistanceRule r) {                      /* in the second entry of a table whose first is the only one used */
        const HvqDistanceRule tab[2] = { good, r };
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_distance_check(&tab[1]));
        dis(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, tab, 2, two, L);
    };
    bad("plane_3", { 3, 0, 0, 0, 0, { 0, 0, 0 } }); bad("plane_negative", { -1, 0, 0, 0, 0, { 0, 0, 0 } }); bad("lo_above_hi", { 0, 9, 8, 0, 0, { 0, 0, 0 } });
    bad("lo_negative", { 0, -1, 8, 0, 0, { 0, 0, 0 } }); bad("hi_256", { 0, 0, 256, 0, 0, { 0, 0, 0 } }); bad("metric_3", { 0, 0, 0, 3, 0, { 0, 0, 0 } });
    bad("metric_negative", { 0, 0, 0, -1, 0, { 0, 0, 0 } }); bad("border_2", { 0, 0, 0, 0, 2, { 0, 0, 0 } }); bad("border_negative", { 0, 0, 0, 0, -1, { 0, 0, 0 } });
    bad("pad_0", { 0, 0, 0, 0, 0, { 1, 0, 0 } }); bad("pad_2", { 0, 0, 0, 0, 0, { 0, 0, 1 } });
    fprintf(g_res, "R refused/check_null %d\n", hvq_distance_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_distance_check(&good));
    auto msk = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, const uint32_t *const *dist, const HvqDistanceMask *s, int nsel, const int *which,
                   void *const *dst) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_distance_mask(cx, n, sids.data(), dist, s, nsel, which, dst, caller));
    };
    void *Dnull[2] = { D[0], nullptr }, *Dmis[2] = { (uint8_t *)D[0] + 8, D[1] };
    msk("m_null_context", nullptr, 2, { sa, sa }, L, &mgood, 1, nullptr, D);
    msk("m_bad_stream", ctx, 2, { sa, 99 }, L, &mgood, 1, nullptr, D);
    msk("m_null_dist", ctx, 2, { sa, sa }, nullptr, &mgood, 1, nullptr, D);
    msk("m_null_map", ctx, 2, { sa, sa }, Lnull, &mgood, 1, nullptr, D);
    msk("m_misaligned_map", ctx, 2, { sa, sa }, Lmis, &mgood, 1, nullptr, D);
    msk("m_null_sel", ctx, 2, { sa, sa }, L, nullptr, 1, nullptr, D);
    msk("m_nsel_0", ctx, 2, { sa, sa }, L, &mgood, 0, nullptr, D);
    {
        std::vector<HvqDistanceMask> many(65, mgood);
        msk("m_nsel_65", ctx, 2, { sa, sa }, L, many.data(), 65, two, D);
    }
    msk("m_which_high", ctx, 2, { sa, sa }, L, &mgood, 1, w_hi, D);
    msk("m_which_negative", ctx, 2, { sa, sa }, L, &mgood, 1, w_lo, D);
    msk("m_null_dst", ctx, 2, { sa, sa }, L, &mgood, 1, nullptr, nullptr);
    msk("m_null_destination", ctx, 2, { sa, sa }, L, &mgood, 1, nullptr, Dnull);
    msk("m_misaligned_destination", ctx, 2, { sa, sa }, L, &mgood, 1, nullptr, Dmis);
    msk("m_too_many", ctx, 65536, { sa, sa }, L, &mgood, 1, nullptr, D);
    msk("m_negative_n", ctx, -1, { sa, sa }, L, &mgood, 1, nullptr, D);
    auto mbad = [&](const char *label, HvqDistanceMask s) {
        const HvqDistanceMask tab[2] = { mgood, s };
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_distance_mask_check(&tab[1]));
        msk(label, ctx, 2, { sa, sa }, L, tab, 2, two, D);
    };
    mbad("m_lo_above_hi", { 0, 5, 4, 0, { 0, 0, 0, 0 } }); mbad("m_mode_2", { 2, 0, 0, 0, { 0, 0, 0, 0 } }); mbad("m_invert_2", { 0, 0, 9, 2, { 0, 0, 0, 0 } });
    mbad("m_pad_0", { 0, 0, 9, 0, { 1, 0, 0, 0 } }); mbad("m_pad_3", { 0, 0, 9, 0, { 0, 0, 0, 1 } }); mbad("m_root_lo", { 1, 1, 1, 0, { 0, 0, 0, 0 } });
    mbad("m_root_hi", { 1, 0, 9, 0, { 0, 0, 0, 0 } }); mbad("m_root_invert", { 1, 0, 0, 1, { 0, 0, 0, 0 } });
    fprintf(g_res, "R refused/check_m_null %d\n", hvq_distance_mask_check(nullptr));
    fprintf(g_res, "R refused/check_m_good %d\n", hvq_distance_mask_check(&mgood));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(2 * (lb + pb));
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed calls right after them work */
    fprintf(g_res, "R refused/then_ok %d\n", hvq_distance_pictures(ctx, 2, std::vector<int>{ sa, sa }.data(), std::vector<int>{ 0, 1 }.data(), nullptr, &good, 1, nullptr, L, caller));
    fprintf(g_res, "R refused/then_mask_ok %d\n", hvq_distance_mask(ctx, 2, std::vector<int>{ sa, sa }.data(), L, &mgood, 1, nullptr, D, caller));
    HIP(hipStreamSynchronize(caller));
    HIP(hipFree(room));
    HIP(hipFree(mem));
}

/* a program linked without fake_distance.cpp: both calls check their arguments first and then say that the kernels are missing */
static void scenario_nogpu(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t lb = 4u * plane_samples(g, 0), pb = bytes_of(g);
    uint8_t *room = guarded_room(lb + pb, 0);
    uint32_t *L[1] = { (uint32_t *)room };
    void *D[1] = { room + lb };
    const HvqDistanceRule good = { 0, 255, 255, 0, 0, { 0, 0, 0 } }, bad = { 0, 255, 255, 5, 0, { 0, 0, 0 } };
    const HvqDistanceMask mgood = { 0, 1, 9, 0, { 0, 0, 0, 0 } }, mbad = { 0, 9, 1, 0, { 0, 0, 0, 0 } };
    const int sid[1] = { sa }, ord[1] = { 0 };
    fprintf(g_res, "R nogpu/distance_bad_rule %d\n", hvq_distance_pictures(ctx, 1, sid, ord, nullptr, &bad, 1, nullptr, L, caller));
    fprintf(g_res, "R nogpu/distance %d\n", hvq_distance_pictures(ctx, 1, sid, ord, nullptr, &good, 1, nullptr, L, caller));
    fprintf(g_res, "R nogpu/mask_bad_range %d\n", hvq_distance_mask(ctx, 1, sid, L, &mbad, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/mask %d\n", hvq_distance_mask(ctx, 1, sid, L, &mgood, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/n0 %d\n", hvq_distance_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(lb + pb);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S nogpu %zu %zu\n", same, back.size());
    HIP(hipFree(room));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_distance_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_inputs();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_distance_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "cases") run_scenario(scenario_cases);
    else if (sc == "resident") run_scenario(scenario_resident);
    else if (sc == "refused") run_scenario(scenario_refused);
    else if (sc == "nogpu") run_scenario(scenario_nogpu);
    else { fprintf(stderr, "fake_distance_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
