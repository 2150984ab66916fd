/* CPU, AddressSanitizer + UBSan: the host entropy parse (hvq_parse.c) and the GPU parse core run on the CPU
 * (gparse_emul.c, chains and flat path) fed mutated P/B pictures: 1..24 random byte overwrites behind the section table,
 * bit flips, truncations.  Every picture is parsed by the host parser with 1 and with 4 threads, whose verdicts (return
 * code and refusal flags) must agree; any read outside an allocation or any undefined behaviour aborts the process.
 * usage: parse_fuzz_asan <w> <h> <h_samp> <v_samp> <is15> <rounds> <seed> <file with records: u32 frame_type, u32 len, len bytes ...>
 * Built together with hvq_parse.c and gparse_emul.c by tests/test_malformed_pb.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../hvqm4_amd/csrc/hvq_parse.h"
#include "../../hvqm4_amd/csrc/hvq_gparse_core.h"

int gparse_emul2(const uint8_t *pic, uint32_t len, int frame_type, int w, int h, int hs, int vs, int is15,
                 uint8_t *blob, uint32_t cap, uint8_t *nest_out, HvqParseResult *res, int mode);

#define REFUSE (HVQ_F_CLAMPED | HVQ_F_CAPPED | HVQ_F_MALFORMED)

static uint32_t rnd(uint32_t *s) { *s ^= *s << 13; *s ^= *s >> 17; *s ^= *s << 5; return *s; }

typedef struct { int ft; uint32_t len; uint8_t *data; } Rec;

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), hs = atoi(argv[3]), vs = atoi(argv[4]), is15 = atoi(argv[5]);
    const long rounds = atol(argv[6]);
    uint32_t seed = (uint32_t)atol(argv[7]) * 2654435761u + 1u;
    FILE *f = fopen(argv[8], "rb");
    if (!f) return 2;
    Rec recs[64];
    int nrec = 0;
    uint32_t hd[2];
    while (nrec < 64 && fread(hd, 4, 2, f) == 2) {
        recs[nrec].ft = (int)hd[0]; recs[nrec].len = hd[1];
        recs[nrec].data = malloc(hd[1]);
        if (fread(recs[nrec].data, 1, hd[1], f) != hd[1]) return 4;
        if (hd[0] != 0x10 && hd[1] > 0x60) ++nrec;             /* P/B pictures only */
        else free(recs[nrec].data);
    }
    fclose(f);
    if (!nrec) return 5;
    HvqParser *p1 = hvq_parser_create(w, h, hs, vs, is15), *p4 = hvq_parser_create(w, h, hs, vs, is15);
    if (!p1 || !p4 || hvq_parser_set_threads(p4, 4) != 4) return 3;
    const size_t cap = hvq_parser_blob_bound(p1);
    uint8_t *b1 = malloc(cap), *b4 = malloc(cap), *be = malloc(cap), *nest = malloc(2048);
    long refused = 0, emulated = 0;
    for (long r = 0; r < rounds; ++r) {
        const Rec *src = &recs[r % nrec];
        uint32_t len = src->len;
        const uint32_t mode = rnd(&seed) % 8;
        if (mode == 7) len = 0x50 + rnd(&seed) % (src->len - 0x50);          /* truncated */
        uint8_t *pic = malloc(len);                                          /* exactly sized: ASan guards the next byte */
        memcpy(pic, src->data, len);
        if (mode < 5) {                                                      /* 1..24 byte overwrites behind 0x50 */
            const uint32_t n = 1 + rnd(&seed) % 24;
            for (uint32_t k = 0; k < n; ++k) pic[0x50 + rnd(&seed) % (len - 0x50)] = (uint8_t)rnd(&seed);
        } else if (mode < 7) {                                               /* bit flips behind the header */
            const uint32_t n = 1 + rnd(&seed) % 12;
            for (uint32_t k = 0; k < n; ++k) { const uint32_t v = rnd(&seed); pic[8 + v % (len - 8)] ^= (uint8_t)(1u << (v >> 29)); }
        }
        size_t l1 = 0, l4 = 0;
        const int rc1 = hvq_parse_picture(p1, src->ft, pic, len, b1, cap, &l1);
        const uint32_t f1 = rc1 ? 0u : (((const HvqPicHeader *)b1)->flags | hvq_parser_last_flags(p1)) & REFUSE;
        const int rc4 = hvq_parse_picture(p4, src->ft, pic, len, b4, cap, &l4);
        const uint32_t f4 = rc4 ? 0u : (((const HvqPicHeader *)b4)->flags | hvq_parser_last_flags(p4)) & REFUSE;
        if (rc1 != rc4 || f1 != f4) {
            fprintf(stderr, "round %ld: 1 thread rc %d flags %#x, 4 threads rc %d flags %#x\n", r, rc1, f1, rc4, f4);
            return 6;
        }
        if (rc1 == 0 && !f1 && (l1 != l4 || memcmp(b1, b4, l1))) { fprintf(stderr, "round %ld: blobs differ by thread count\n", r); return 7; }
        refused += rc1 || f1;
        if (r % 16 == 0) {                                                   /* the device parse core: slower, every 16th picture */
            HvqParseResult res;
            for (int m = 0; m < 2; ++m) {
                if (gparse_emul2(pic, len, src->ft, w, h, hs, vs, is15, be, (uint32_t)cap, nest, &res, m) < 0) return 8;
                ++emulated;
            }
        }
        free(pic);
    }
    printf("fuzz ok: %ld pictures, %ld refused, %ld device-core runs\n", rounds, refused, emulated);
    hvq_parser_destroy(p1); hvq_parser_destroy(p4);
    free(b1); free(b4); free(be); free(nest);
    for (int k = 0; k < nrec; ++k) free(recs[k].data);
    return 0;
}
