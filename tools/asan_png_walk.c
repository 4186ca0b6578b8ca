/* DEVELOPMENT / TEST TOOLING: the host side of the PNG calls on damaged files under AddressSanitizer and UBSan, as a stand-alone
 * CPU program (tools/asan_png_walk.sh builds and runs it; no GPU, no Python in the process).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called.  The corpus file (written by tests/png_damage.py --host-corpus) holds the files whose
 * status is decided on the host -- truncated and re-cut containers, IHDR rewrites up to 2^31, broken zlib headers, the APNG
 * container sweep -- each with the statuses tests/png_spec_ref.py and tests/apng_ref.py expect.  Every file is a heap copy of
 * exactly its size, so a read past its end is ASan's to see.  Three calls are driven over the corpus:
 *   debig_png_info_get;  debig_png_decode_batch, one file per call and in batches of 64;  debig_apng_info_get.
 * Record layout, little-endian: u32 kind (0: a PNG case, 1: APNG walk only), u32 decode status, u32 info status, u32 APNG walk
 * status, u64 out_cap, u32 length, the file. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"

#define CHECK(c, i) do { if (!(c)) { fprintf(stderr, "%s:%d: record %u: %s\n", __FILE__, __LINE__, (unsigned)(i), #c); exit(1); } } while (0)
#define BATCH 64u

typedef struct rec {
    uint32_t kind, st, ist, ast, len;
    uint64_t cap;
    uint8_t *data;
} rec;

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    rec *recs = NULL;
    uint32_t n = 0, cap_recs = 0;
    uint8_t head[28];
    while (fread(head, 1, sizeof head, f) == sizeof head) {
        if (n == cap_recs) {
            cap_recs = cap_recs ? 2 * cap_recs : 1024;
            recs = (rec *)realloc(recs, cap_recs * sizeof(rec));
            if (!recs) return 2;
        }
        rec *r = &recs[n];
        r->kind = rd32(head); r->st = rd32(head + 4); r->ist = rd32(head + 8); r->ast = rd32(head + 12);
        r->cap = (uint64_t)rd32(head + 16) | ((uint64_t)rd32(head + 20) << 32);
        r->len = rd32(head + 24);
        r->data = (uint8_t *)malloc(r->len ? r->len : 1); /* exactly the file: no slack behind it */
        if (!r->data || fread(r->data, 1, r->len, f) != r->len) { fprintf(stderr, "record %u is cut short\n", n); return 2; }
        n++;
    }
    fclose(f);
    if (n < 1000) { fprintf(stderr, "only %u records\n", n); return 2; }

    uint32_t n_png = 0, n_apng = 0;
    uint8_t *out = (uint8_t *)malloc(64); /* never written: every status here is decided before the device */
    memset(out, 0xA5, 64);
    /* ---- one file per call */
    for (uint32_t i = 0; i < n; i++) {
        const rec *r = &recs[i];
        debig_apng_info ai;
        debig_apng_frame fr[4];
        CHECK(debig_apng_info_get(r->data, r->len, &ai, fr, 4) == r->ast, i);
        CHECK(debig_apng_info_get(r->data, r->len, &ai, NULL, 0) == r->ast, i);
        n_apng++;
        if (r->kind != 0) continue;
        debig_png_info inf;
        CHECK(debig_png_info_get(r->data, r->len, &inf) == r->ist, i);
        CHECK(debig_png_info_get(r->data, r->len, NULL) == r->ist, i);
        const uint8_t *in = r->data;
        const uint64_t size = r->len;
        uint8_t *o = out;
        uint32_t st = 0xABCDu;
        CHECK(debig_png_decode_batch(&in, &size, &o, &r->cap, &st, &inf, 1, 0) == 0, i);
        CHECK(st == r->st, i);
        st = 0xABCDu;
        CHECK(debig_png_decode_batch(&in, &size, &o, &r->cap, &st, NULL, 1, DEBIG_PNG_FORCE_GENERAL) == 0, i);
        CHECK(st == r->st, i);
        n_png++;
    }
    /* ---- batches of 64 (the last one shorter) */
    const uint8_t *ins[BATCH];
    uint64_t sizes[BATCH], caps[BATCH];
    uint8_t *outs[BATCH];
    uint32_t status[BATCH], idx[BATCH], m = 0;
    debig_png_info infos[BATCH];
    for (uint32_t i = 0; i <= n; i++) {
        if (i < n && recs[i].kind == 0) {
            ins[m] = recs[i].data; sizes[m] = recs[i].len; caps[m] = recs[i].cap; outs[m] = out; status[m] = 0xABCDu; idx[m] = i;
            m++;
        }
        if (m == BATCH || (i == n && m)) {
            CHECK(debig_png_decode_batch(ins, sizes, outs, caps, status, infos, m, 0) == 0, idx[0]);
            for (uint32_t k = 0; k < m; k++) CHECK(status[k] == recs[idx[k]].st, idx[k]);
            m = 0;
        }
    }
    for (uint32_t k = 0; k < 64; k++) CHECK(out[k] == 0xA5, k);
    CHECK(debig_png_decode_batch(NULL, NULL, NULL, NULL, NULL, NULL, 0, 0) == 0, 0);
    for (uint32_t i = 0; i < n; i++) free(recs[i].data);
    free(recs);
    free(out);
    printf("asan_png_walk: ok (%u PNG cases, %u APNG walks)\n", n_png, n_apng);
    return 0;
}
