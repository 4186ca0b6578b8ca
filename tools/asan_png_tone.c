/* DEVELOPMENT / TEST TOOLING: the host side of debig_png_decode_batch_tensor_tone under AddressSanitizer and UBSan, as a
 * stand-alone CPU program (tools/asan_png_tone.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- debig_png_tone_table, the argument checks and the statuses
 * decided when IHDR has been read (E_BOX > E_WARP > E_COLOR > E_TONE > what comes later in the file) -- is decided on the host,
 * before any device is looked for.  The files are a signature and an IHDR chunk with nothing behind them. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"

#define SENTINEL 0xABCDu
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

/* signature + IHDR (the chunk CRCs are checked on the device: never reached) -> its length (33) */
static size_t stub_png(uint8_t *f, uint32_t w, uint32_t h, uint8_t depth, uint8_t ct)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    memcpy(f, sig, 8);
    const uint8_t ihdr[25] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                              (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, depth, ct, 0, 0, 0, 0, 0, 0, 0};
    memcpy(f + 8, ihdr, 25);
    return 33;
}

#define N 5
static uint8_t *files[N];
static uint64_t sizes[N];
static uint32_t status[N];
static debig_png_warp warps[N];
static debig_png_color colors[N];
static debig_png_tone tones[N];
static void *const OUT = (void *)(uintptr_t)0x10000; /* never dereferenced */

static int call(const debig_png_tensor_desc *d, const debig_png_warp *ws, const debig_png_color *cs, const debig_png_tone *ts,
                const uint8_t *tables, uint32_t n_tables, const debig_png_alpha_desc *ad, const debig_png_filter_desc *fd,
                const debig_png_warp_desc *wd, const debig_png_box *bx)
{
    for (uint32_t i = 0; i < N; i++) status[i] = SENTINEL;
    return debig_png_decode_batch_tensor_tone((const uint8_t *const *)files, sizes, OUT, bx, ws, cs, ts, tables, n_tables, status, NULL, N,
                                              0, d, ad, fd, wd);
}

static void untouched(int rc)
{
    CHECK(rc == DEBIG_PNG_BAD_ARG);
    for (uint32_t i = 0; i < N; i++) CHECK(status[i] == SENTINEL);
}

int main(void)
{
    /* heap copies of exactly the files' sizes: a read past their end is ASan's to see */
    uint8_t tmp[64];
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, wident[6] = {1, 0, 0, 0, 1, 0};
    for (uint32_t i = 0; i < N; i++) {
        sizes[i] = stub_png(tmp, 9, 7, 8, i & 2 ? 6 : 2);
        files[i] = (uint8_t *)malloc(sizes[i]);
        memcpy(files[i], tmp, sizes[i]);
        memcpy(warps[i].m, wident, sizeof wident);
        memcpy(colors[i].m, ident, sizeof ident);
    }

    /* ---- the table helper: heap buffers of exactly 256 entries */
    uint32_t *hist = (uint32_t *)calloc(256, sizeof(uint32_t));
    uint8_t *lut = (uint8_t *)malloc(256);
    CHECK(hist && lut);
    for (uint32_t op = DEBIG_PNG_TONE_AUTOCONTRAST; op <= DEBIG_PNG_TONE_EQUALIZE; op++) {
        CHECK(debig_png_tone_table(op, 0, hist, lut) == 1); /* empty: the identity */
        for (uint32_t i = 0; i < 256; i++) CHECK(lut[i] == i);
        hist[200] = 0xFFFFFFFFu; /* one bin: the identity */
        CHECK(debig_png_tone_table(op, 0, hist, lut) == 1);
        for (uint32_t i = 0; i < 256; i++) CHECK(lut[i] == i);
        hist[200] = 0;
        CHECK(debig_png_tone_table(op, 1, hist, lut) == 0);
        CHECK(debig_png_tone_table(op, 0, NULL, lut) == 0);
    }
    hist[0] = hist[25] = 1;
    CHECK(debig_png_tone_table(DEBIG_PNG_TONE_AUTOCONTRAST, 0, hist, lut) == 1);
    CHECK(lut[0] == 0 && lut[25] == 255 && lut[24] == 244 && lut[255] == 255); /* (Pillow's double rule gives 254 at 25) */
    for (uint32_t i = 0; i < 256; i++) hist[i] = 0xFFFFFFFFu; /* the sums need 64 bits */
    CHECK(debig_png_tone_table(DEBIG_PNG_TONE_EQUALIZE, 0, hist, lut) == 1);
    CHECK(lut[0] == 0 && lut[128] == 128 && lut[255] == 255);
    for (uint32_t i = 0; i < 256; i++) hist[i] = i < 128 ? 0 : 4; /* 20 x 20-like: step 1 ... entries above 255 are clamped */
    CHECK(debig_png_tone_table(DEBIG_PNG_TONE_EQUALIZE, 0, hist, lut) == 1);
    CHECK(lut[127] == 0 && lut[255] == 255 && lut[200] == 255);
    for (uint32_t bits = 0; bits <= 9; bits++) {
        const int ok = debig_png_tone_table(DEBIG_PNG_TONE_POSTERIZE, bits, NULL, lut);
        CHECK(ok == (bits >= 1 && bits <= 8));
        if (ok) CHECK(lut[255] == (uint8_t)(0xFF00u >> bits) && lut[0] == 0);
    }
    for (uint32_t thr = 0; thr <= 258; thr++) {
        const int ok = debig_png_tone_table(DEBIG_PNG_TONE_SOLARIZE, thr, NULL, lut);
        CHECK(ok == (thr <= 256));
        if (ok) CHECK(lut[255] == (thr <= 255 ? 0 : 255) && lut[0] == (thr == 0 ? 255 : 0));
    }
    CHECK(debig_png_tone_table(DEBIG_PNG_TONE_NONE, 0, hist, lut) == 0 && debig_png_tone_table(DEBIG_PNG_TONE_TABLE, 0, hist, lut) == 0);
    CHECK(debig_png_tone_table(6, 0, hist, lut) == 0 && debig_png_tone_table(0xFFFFFFFFu, 0, hist, lut) == 0);
    free(hist);
    free(lut);

    /* ---- the argument checks: status stays unwritten */
    debig_png_tensor_desc d;
    memset(&d, 0, sizeof d);
    d.out_w = 8;
    d.out_h = 6;
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    for (int j = 0; j < 4; j++) d.scale[j] = 1.0f;
    debig_png_warp_desc wd;
    memset(&wd, 0, sizeof wd);
    debig_png_alpha_desc ad;
    memset(&ad, 0, sizeof ad);
    debig_png_filter_desc fd = {DEBIG_PNG_FILTER_BICUBIC, 0};
    uint8_t *tables = (uint8_t *)calloc(2, 256); /* exactly n_tables x 256 bytes */
    CHECK(tables);
    untouched(call(&d, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL));   /* tones NULL */
    untouched(call(&d, NULL, NULL, tones, NULL, 1, NULL, NULL, NULL, NULL));  /* tables NULL with n_tables > 0 */
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_16;
    untouched(call(&d, NULL, NULL, tones, NULL, 0, NULL, NULL, NULL, NULL));  /* 16 bits */
    d.out_format = DEBIG_PNG_FMT_RGBA | DEBIG_PNG_FMT_8;
    ad.mode = DEBIG_PNG_ALPHA_PREMULTIPLIED;
    untouched(call(&d, NULL, NULL, tones, NULL, 0, &ad, NULL, NULL, NULL));   /* PREMULTIPLIED */
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    ad.mode = DEBIG_PNG_ALPHA_OVER;
    untouched(call(&d, NULL, colors, tones, NULL, 0, &ad, NULL, NULL, NULL)); /* alpha with a matrix */
    untouched(call(&d, NULL, colors, tones, NULL, 0, NULL, &fd, NULL, NULL)); /* BICUBIC with a matrix */
    untouched(call(&d, warps, NULL, tones, NULL, 0, NULL, NULL, NULL, NULL)); /* warps without their descriptor */
    untouched(call(&d, NULL, NULL, tones, NULL, 0, NULL, NULL, &wd, NULL));   /* the descriptor without warps */
    untouched(call(&d, warps, NULL, tones, NULL, 0, NULL, &fd, &wd, NULL));   /* a filter descriptor under a warp */
    untouched(call(&d, warps, NULL, tones, NULL, 0, &ad, NULL, &wd, NULL));
    untouched(call(NULL, NULL, NULL, tones, NULL, 0, NULL, NULL, NULL, NULL));
    d.out_format = DEBIG_PNG_FMT_NATIVE;
    CHECK(call(&d, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL) == DEBIG_PNG_BAD_FORMAT && status[0] == SENTINEL);
    CHECK(debig_png_decode_batch_tensor_tone(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL) == 0);

    /* ---- the order of the statuses decided at IHDR: E_BOX > E_WARP > E_COLOR > E_TONE > what the file holds later (here: nothing) */
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    warps[0].m[2] = NAN;
    warps[1].m[0] = 32769.0;
    colors[0].m[5] = colors[1].m[6] = colors[2].m[7] = NAN;
    const debig_png_tone bad[N] = {{DEBIG_PNG_TONE_POSTERIZE, 9}, {7, 0}, {DEBIG_PNG_TONE_EQUALIZE, 1}, {DEBIG_PNG_TONE_TABLE, 2},
                                   {DEBIG_PNG_TONE_TABLE, 1}};
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    CHECK(call(&d, warps, colors, bad, tables, 2, NULL, NULL, &wd, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_COLOR && status[3] == DEBIG_PNG_E_TONE);
    CHECK(status[4] != DEBIG_PNG_OK && status[4] != DEBIG_PNG_E_TONE && status[4] != SENTINEL); /* the file ends behind IHDR */
    const uint32_t later = status[4];
    CHECK(call(&d, NULL, colors, bad, tables, 2, NULL, NULL, NULL, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_COLOR && status[2] == DEBIG_PNG_E_COLOR && status[3] == DEBIG_PNG_E_TONE &&
          status[4] == later);
    d.resize_flags = DEBIG_PNG_RESIZE_ANTIALIAS;
    d.out_format = DEBIG_PNG_FMT_GRAY | DEBIG_PNG_FMT_8;
    CHECK(call(&d, NULL, NULL, bad, tables, 2, &ad, &fd, NULL, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_TONE && status[2] == DEBIG_PNG_E_TONE && status[3] == DEBIG_PNG_E_TONE &&
          status[4] == later);
    CHECK(call(&d, NULL, NULL, bad, tables, 1, &ad, &fd, NULL, boxes) == 0); /* one table only: index 1 is out of range too */
    CHECK(status[4] == DEBIG_PNG_E_TONE);
    free(tables);
    for (uint32_t i = 0; i < N; i++) free(files[i]);
    puts("asan_png_tone: ok");
    return 0;
}
