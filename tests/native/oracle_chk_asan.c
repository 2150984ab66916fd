/* CPU, AddressSanitizer + UBSan: the checked oracle (oracle/hvq_oracle_chk.c) on a mutated corpus.  Proves its guard list complete:
 * the picture and each of the three picture buffers are heap allocations of EXACTLY their size, so that any access a guard misses
 * lands in a red zone and ends the run.  Prints one line per mutant: "<index> <class mask> <bits past the end> <cross-plane reads>".
 * usage: oracle_chk_asan <w> <h> <h_samp> <v_samp> <is15> <file>
 * The file holds records { u32 frame_type, u32 len, u32 is_mutant, len bytes } in decode order, the mutants of a picture in front of
 * the stream's own picture: a mutant is decoded against the references of that picture and changes nothing, the stream's own picture
 * must be defined and moves the player's rotation (h4m:2087-2137).  Built by tests/test_mutants_vs_oracle.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/hvq_oracle.h"

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    HvqOracle *o = hvqc_create(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    FILE *f = fopen(argv[6], "rb");
    if (!o || !f) return 2;
    const uint32_t ps = hvqc_picsize(o);
    uint8_t *buf[3];                                    /* past, present, future */
    for (int i = 0; i < 3; ++i) buf[i] = calloc(1, ps);
    uint32_t hd[3];
    long index = 0;
    int rotated = 0;
    while (fread(hd, 4, 3, f) == 3) {
        const int ft = (int)hd[0];
        uint8_t *pic = malloc(hd[1] ? hd[1] : 1);       /* exactly sized */
        if (fread(pic, 1, hd[1], f) != hd[1]) return 4;
        if (ft != 0x30 && !rotated) { uint8_t *t = buf[0]; buf[0] = buf[2]; buf[2] = t; }
        rotated = 1;
        HvqoReport rep;
        if (hd[2]) {
            uint8_t *work = malloc(ps);
            memcpy(work, buf[1], ps);
            hvqo_check_picture(o, ft, pic, hd[1], work, buf[0], buf[2], &rep);
            printf("%ld %u %u %u\n", index++, rep.cls, rep.past_bits, rep.cross);
            free(work);
        } else {
            if (hvqo_check_picture(o, ft, pic, hd[1], buf[1], buf[0], buf[2], &rep)) { fprintf(stderr, "the stream's own picture is class %#x\n", rep.cls); return 5; }
            if (ft != 0x30) { uint8_t *t = buf[1]; buf[1] = buf[2]; buf[2] = t; }
            rotated = 0;
        }
        free(pic);
    }
    fclose(f);
    for (int i = 0; i < 3; ++i) free(buf[i]);
    hvqc_destroy(o);
    printf("oracle ok: %ld mutants\n", index);
    return 0;
}
