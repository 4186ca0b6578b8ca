/* DEVELOPMENT / TEST TOOLING: the host side of debig_png_decode_batch_tensor_color and debig_png_decode_batch_tensor_warp_color
 * under AddressSanitizer and UBSan, as a stand-alone CPU program (tools/asan_png_color.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- the quantiser, the argument checks and the statuses decided
 * when IHDR has been read (E_BOX > E_WARP > E_COLOR > what comes later in the file) -- is decided on the host, before any device
 * is looked for.  The files are a signature and an IHDR chunk with nothing behind them. */
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

#define N 4
static uint8_t *files[N];
static uint64_t sizes[N];
static uint32_t status[N];
static debig_png_warp warps[N];
static debig_png_color colors[N];
static void *const OUT = (void *)(uintptr_t)0x10000; /* never dereferenced */

static int color_call(const debig_png_tensor_desc *d, const debig_png_filter_desc *fd, const debig_png_color *cs, const debig_png_box *bx)
{
    for (uint32_t i = 0; i < N; i++) status[i] = SENTINEL;
    return debig_png_decode_batch_tensor_color((const uint8_t *const *)files, sizes, OUT, bx, cs, status, NULL, N, 0, d, fd);
}

static int warp_call(const debig_png_tensor_desc *d, const debig_png_warp_desc *wd, const debig_png_warp *ws, const debig_png_color *cs,
                     const debig_png_box *bx)
{
    for (uint32_t i = 0; i < N; i++) status[i] = SENTINEL;
    return debig_png_decode_batch_tensor_warp_color((const uint8_t *const *)files, sizes, OUT, bx, ws, cs, status, NULL, N, 0, d, wd);
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
        sizes[i] = stub_png(tmp, 9, 7, i & 1 ? 16 : 8, i & 2 ? 6 : 2);
        files[i] = (uint8_t *)malloc(sizes[i]);
        memcpy(files[i], tmp, sizes[i]);
        memcpy(warps[i].m, wident, sizeof wident);
        memcpy(colors[i].m, ident, sizeof ident);
    }

    /* ---- the quantiser: the identity, the limits on both sides, halves away from zero, what it refuses */
    int32_t k[9];
    int64_t o[3];
    for (uint32_t bits = 8; bits <= 16; bits += 8) {
        const int64_t vmax = (int64_t)(((1u << bits) - 1u) << (30u - bits));
        CHECK(debig_png_color_quantise(ident, bits, k, o) == 1);
        for (uint32_t j = 0; j < 9; j++) CHECK(k[j] == (j % 4 == 0 ? 65536 : 0));
        CHECK(o[0] == 0 && o[1] == 0 && o[2] == 0);
        for (int sign = -1; sign <= 1; sign += 2) {
            double M[12];
            for (uint32_t j = 0; j < 12; j++) M[j] = sign * 16.0;
            CHECK(debig_png_color_quantise(M, bits, k, o) == 1);
            for (uint32_t j = 0; j < 9; j++) CHECK(k[j] == sign * (1 << 20));
            for (uint32_t c = 0; c < 3; c++) CHECK(o[c] == sign * 16 * vmax);
            for (uint32_t j = 0; j < 12; j++) {
                const double bad[4] = {sign * 16.0001, nextafter(sign * 16.0, sign * INFINITY), sign * INFINITY, NAN};
                for (uint32_t b = 0; b < 4; b++) {
                    memcpy(M, ident, sizeof M);
                    M[j] = bad[b];
                    CHECK(debig_png_color_quantise(M, bits, k, o) == 0);
                }
            }
        }
        const double halves[12] = {0.5 / 65536, -0.5 / 65536, 1.5 / 65536, 1.0, -1.5 / 65536, 0.49999 / 65536, -0.49999 / 65536, -1.0, 0, 0, 0, 0.5};
        CHECK(debig_png_color_quantise(halves, bits, k, o) == 1);
        CHECK(k[0] == 1 && k[1] == -1 && k[2] == 2 && k[3] == -2 && k[4] == 0 && k[5] == 0);
        CHECK(o[0] == vmax && o[1] == -vmax && o[2] == (vmax + 1) / 2);
    }
    CHECK(debig_png_color_quantise(ident, 12, k, o) == 0);

    /* ---- the argument checks: status stays unwritten */
    debig_png_tensor_desc d;
    memset(&d, 0, sizeof d);
    d.out_w = 8;
    d.out_h = 6;
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    for (int j = 0; j < 4; j++) d.scale[j] = 1.0f;
    debig_png_filter_desc fd = {DEBIG_PNG_FILTER_BICUBIC, 0};
    untouched(color_call(&d, &fd, colors, NULL));
    fd.filter = 3;
    untouched(color_call(&d, &fd, colors, NULL));
    fd.filter = DEBIG_PNG_FILTER_NEAREST;
    fd.reserved = 1;
    untouched(color_call(&d, &fd, colors, NULL));
    untouched(color_call(&d, NULL, NULL, NULL));
    untouched(color_call(NULL, NULL, colors, NULL));
    debig_png_warp_desc wd;
    memset(&wd, 0, sizeof wd);
    untouched(warp_call(&d, &wd, warps, NULL, NULL));
    untouched(warp_call(&d, &wd, NULL, colors, NULL));
    untouched(warp_call(&d, NULL, warps, colors, NULL));
    wd.alpha_mode = DEBIG_PNG_ALPHA_OVER;
    untouched(warp_call(&d, &wd, warps, colors, NULL));
    wd.alpha_mode = DEBIG_PNG_ALPHA_STRAIGHT;
    wd.filter = DEBIG_PNG_FILTER_BICUBIC;
    untouched(warp_call(&d, &wd, warps, colors, NULL));
    wd.filter = DEBIG_PNG_FILTER_BILINEAR;
    const uint32_t grey[2] = {DEBIG_PNG_FMT_GRAY | DEBIG_PNG_FMT_8, DEBIG_PNG_FMT_GRAY_ALPHA | DEBIG_PNG_FMT_16};
    for (int g = 0; g < 2; g++) {
        d.out_format = grey[g];
        untouched(color_call(&d, NULL, colors, NULL));
        untouched(warp_call(&d, &wd, warps, colors, NULL));
    }
    d.out_format = DEBIG_PNG_FMT_NATIVE;
    CHECK(color_call(&d, NULL, colors, NULL) == DEBIG_PNG_BAD_FORMAT && status[0] == SENTINEL);
    CHECK(warp_call(&d, &wd, warps, colors, NULL) == DEBIG_PNG_BAD_FORMAT && status[0] == SENTINEL);
    CHECK(debig_png_decode_batch_tensor_color(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);
    CHECK(debig_png_decode_batch_tensor_warp_color(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);

    /* ---- the order of the statuses decided at IHDR: E_BOX > E_WARP > E_COLOR > what the file holds later (here: nothing) */
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (uint32_t i = 0; i < 3; i++) colors[i].m[5 + i] = i == 1 ? 16.5 : NAN;
    warps[0].m[2] = NAN;
    warps[1].m[0] = 32769.0;
    const uint32_t fmts[2] = {DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8, DEBIG_PNG_FMT_RGBA | DEBIG_PNG_FMT_16};
    for (int f = 0; f < 2; f++) {
        d.out_format = fmts[f];
        CHECK(warp_call(&d, &wd, warps, colors, boxes) == 0);
        CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_COLOR);
        CHECK(status[3] != DEBIG_PNG_OK && status[3] != DEBIG_PNG_E_COLOR && status[3] != SENTINEL); /* the file ends behind IHDR */
        const uint32_t later = status[3];
        d.resize_flags = DEBIG_PNG_RESIZE_ANTIALIAS;
        CHECK(color_call(&d, f ? &fd : NULL, colors, boxes) == 0);
        d.resize_flags = 0;
        CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_COLOR && status[2] == DEBIG_PNG_E_COLOR && status[3] == later);
        fd.reserved = 0;
    }
    for (uint32_t i = 0; i < N; i++) free(files[i]);
    puts("asan_png_color: ok");
    return 0;
}
